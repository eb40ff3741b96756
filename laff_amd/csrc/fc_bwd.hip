// fc_bwd.hip -- backward of the FC projection A = act(X W^T + bias) for gfx950, fp32: laff_fc_backward.
//
//   dZ = dA (.) act'(A)      tanh: 1 - A^2    sigmoid: A (1 - A)    relu: A > 0    none: 1       (A is the SAVED forward output)
//   dW = dZ^T X   [D, Dk]    contraction over the N rows
//   db = sum_n dZ [D]
//   dX = dZ W     [N, Dk]    contraction over the D columns
//
// One kernel template, two products.  Both run on v_mfma_f32_32x32x2_f32 (bit-for-bit an fp32 fmaf chain in k order), a block of four
// wavefronts (2 x 2) owns a TM x TN output tile, each wavefront WM x WN accumulators of 32 x 32, and the operands pass through LDS in
// steps of KT = 32 of the contraction index.  dZ is never stored: it is formed from dA and A on their way to LDS, so it is always
// the MFMA's A operand (its index is the output row) and the plain matrix (X or W) the B operand (its index is the output column, which
// sits on the lane: a wavefront stores 128 consecutive bytes per accumulator register).
//
// The MFMA wants lane l to hold A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]:
//   dW: both operands have the contraction index n as their ROW index in memory.  Their tiles are copied as they are, [KT][TM] and
//       [KT][TN]; a fragment read takes 32 consecutive floats of row k -- the "transposed" operand costs nothing but the read pattern.
//   dX: W has the contraction index j as its row index, read like the above.  dZ has it as its COLUMN index: its tile is kept
//       [TM][KT + 1], and the fragment read walks down a column; the odd pitch spreads the 32 rows over 32 banks.
//
// A product's sum is cut into chunks when its output tiles alone would not fill the chip: the sum over N of dW and db, the sum over D
// of dX.  fc_bwd_plan derives the tile edge and the cut from (N, Dk, D) only.  A chunk's tile goes to the workspace and fc_bwd_reduce adds
// the chunks in chunk order; with one chunk -- for dW and db always at N <= 128, the training batch -- the tile goes straight to the
// output and there is no workspace.  db is summed by the blocks of the first column tile, thread t owning column t of the staged dZ
// tile, in row order.  No atomics anywhere: two calls give the same bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>

#include "fc_bwd_common.h"
#include "fc_bwd_tile.h"
#include "kernels.h"

namespace laff {

namespace {

using namespace fcbwd;

// the tile body is fc_bwd_tile.h's; a block's tile and where it goes are decided here
template <int WM, int WN, bool DX, bool FAST>
__global__ __launch_bounds__(THREADS) void fc_bwd_kernel(FcBwdArgs a) {
    constexpr int TM = 64 * WM, TN = 64 * WN;
    const bool mm = DX || a.dW != nullptr;                  // db alone: one column of blocks, no product
    const int M = DX ? a.N : a.D, NC = a.Dk;                // the output is [M, NC]
    const int tiles_n = mm ? (NC + TN - 1) / TN : 1, tiles_m = (M + TM - 1) / TM;
    int bid = blockIdx.x;
    const int tn = bid % tiles_n;
    bid /= tiles_n;
    const int tm = bid % tiles_m, chunk = bid / tiles_m;
    const bool cut = (DX ? a.chunks_dx : a.chunks) > 1;
    float* out = cut ? a.part + (size_t)chunk * M * NC : DX ? a.dX : a.dW;
    const int ldo = cut ? NC : DX ? a.lddx : a.lddw;
    float* db_out = DX || a.db == nullptr ? nullptr : a.chunks > 1 ? a.part_db + (size_t)chunk * a.D : a.db;
    fc_bwd_tile<WM, WN, DX, FAST>(a, tm, tn, chunk, out, ldo, db_out);
}

// out[r, c] = part[0][r, c] + part[1][r, c] + ... in chunk order
__global__ __launch_bounds__(THREADS) void fc_bwd_reduce(const float* part, size_t chunk_stride, int chunks, int rows, int cols, float* out,
                                                          int ldo) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (size_t)rows * cols) return;
    float s = part[i];
    for (int c = 1; c < chunks; ++c) s += part[c * chunk_stride + i];
    out[(i / cols) * ldo + i % cols] = s;
}

// the tiles and the cut of one product, [rows, cols] summed over K (plan_tiles, fc_bwd_tile.h)
void plan_product(int rows, int cols, int K, int* edge, int* chunks, int* len) {
    plan_tiles(tiles_of(rows, cols, 128), tiles_of(rows, cols, 64), K, edge, chunks, len);
}

// whole tiles, whole steps and 16-byte aligned rows: what the FAST instantiations take for granted
bool fc_bwd_fast(const FcBwdArgs& a, bool dx, int edge) {
    const unsigned vec = dx ? 1u | 4u : 1u | (a.dW ? 2u : 0u);
    return (a.vec & vec) == vec && (dx ? a.N : a.D) % edge == 0 && (dx || a.dW ? a.Dk % edge == 0 : true) && (dx ? a.D : a.N) % KT == 0;
}

template <bool DX>
hipError_t launch_product(const FcBwdArgs& a, int edge, long long blocks, hipStream_t st) {
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(THREADS);
    const bool fast = fc_bwd_fast(a, DX, edge);
    if (edge == 128 && fast) hipLaunchKernelGGL((fc_bwd_kernel<2, 2, DX, true>), grid, block, 0, st, a);
    else if (edge == 128) hipLaunchKernelGGL((fc_bwd_kernel<2, 2, DX, false>), grid, block, 0, st, a);
    else if (fast) hipLaunchKernelGGL((fc_bwd_kernel<1, 1, DX, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((fc_bwd_kernel<1, 1, DX, false>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_reduce(const float* part, int chunks, int rows, int cols, float* out, int ldo, hipStream_t st) {
    const size_t n = (size_t)rows * cols;
    hipLaunchKernelGGL(fc_bwd_reduce, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, part, n, chunks, rows, cols, out, ldo);
    return hipGetLastError();
}

}  // namespace

void fc_bwd_plan(int N, int Dk, int D, FcBwdPlan* p) {
    plan_product(D, Dk, N, &p->tile_dw, &p->chunks, &p->chunk_rows);
    plan_product(N, Dk, D, &p->tile_dx, &p->chunks_dx, &p->chunk_len_dx);
    p->ws_db = p->chunks > 1 ? (size_t)p->chunks * D * sizeof(float) : 0;
    p->ws_dw = p->chunks > 1 ? (size_t)p->chunks * D * Dk * sizeof(float) + p->ws_db : 0;
    p->ws_dx = p->chunks_dx > 1 ? (size_t)p->chunks_dx * N * Dk * sizeof(float) : 0;
}

hipError_t launch_fc_backward(const FcBwdArgs& a0, hipStream_t st) {
    FcBwdArgs a = a0;
    FcBwdPlan p;
    fc_bwd_plan(a.N, a.Dk, a.D, &p);
    a.chunks = p.chunks;
    a.chunk_rows = p.chunk_rows;
    a.chunks_dx = p.chunks_dx;
    a.chunk_len_dx = p.chunk_len_dx;
    // the partial tiles of dW, then those of db; dX's use the same workspace afterwards (the launches are ordered on the stream)
    if (a.chunks > 1 && a.part) a.part_db = a.part + (a.dW ? (size_t)a.chunks * a.D * a.Dk : 0);
    if (a.dW || a.db) {
        const long long blocks = (a.dW ? tiles_of(a.D, a.Dk, p.tile_dw) : (a.D + p.tile_dw - 1) / p.tile_dw) * a.chunks;
        if (hipError_t e = launch_product<false>(a, p.tile_dw, blocks, st)) return e;
        if (a.chunks > 1) {
            if (a.dW)
                if (hipError_t e = launch_reduce(a.part, a.chunks, a.D, a.Dk, a.dW, a.lddw, st)) return e;
            if (a.db)
                if (hipError_t e = launch_reduce(a.part_db, a.chunks, 1, a.D, a.db, a.D, st)) return e;
        }
    }
    if (a.dX) {
        if (hipError_t e = launch_product<true>(a, p.tile_dx, tiles_of(a.N, a.Dk, p.tile_dx) * a.chunks_dx, st)) return e;
        if (a.chunks_dx > 1) return launch_reduce(a.part, a.chunks_dx, a.N, a.Dk, a.dX, a.lddx, st);
    }
    return hipSuccess;
}

}  // namespace laff
