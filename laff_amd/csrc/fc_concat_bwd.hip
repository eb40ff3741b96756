// fc_concat_bwd.hip -- backward of the concat layer A = act(sum_s X_s W[:, c_s : c_s + Dk_s]^T + bias) for gfx950, fp32: the dense
// segments of laff_fc_concat_backward, the counterpart of fc_concat.hip's one-launch forward.
//
//   dZ = dA (.) act'(A)                      (A is the SAVED forward output; dact of fc_bwd_common.h)
//   dW[:, c_s : c_s + Dk_s] = dZ^T X_s       every dense segment in ONE launch, the window of the one [D, lddw] gradient written in place
//   db = sum_n dZ                            by the blocks of the first segment's first column tile, in row order
//   dX_s = dZ W[:, c_s : c_s + Dk_s]         every segment that wants one in ONE launch, W read in place at the window
//
// The tile body is fc_bwd.hip's (fc_bwd_tile.h): the same fp32 MFMA chain, the same staging, so an element has the bits that
// laff_fc_backward on the window gives it with the same cut.  What is new is who owns which tile: the launch arguments carry a
// prefix table of the segments' tile counts, a block finds its (segment, tile) there -- a tile belongs to one segment and ends at
// the window's edge -- and binds that segment's X, window and output into the body's arguments.  One tile edge and one instantiation
// per launch: FAST only when every segment is made of whole tiles with 16-byte aligned rows, else the general one for all.
//
// The cut of a sum (over N for dW and db, over D for dX) comes from the launch's tiles over ALL segments, so from (N, D, the
// widths) alone: one chunk at N <= 128 for dW and db.  With more, a chunk's tiles go to the workspace -- the segments' columns side by
// side in one partial row -- and ONE reduce launch adds the chunks in chunk order into every window.  No atomics: two calls, same bits.
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

// one launch: the body's arguments with the per-segment fields left open, and the segments
struct ConcatBwdLaunch {
    FcBwdArgs base;                           // X, dX, Dk, ldx, lddx, vec: bound per block; W, dW: the whole matrices
    int n;                                    // segments of this launch
    int tile_start[CONCAT_MAX_SEG + 1];       // prefix sums of the segments' tiles (one chunk's)
    int part_col[CONCAT_MAX_SEG + 1];         // prefix sums of their widths: a segment's first column in a partial row
    const float* X[CONCAT_MAX_SEG];
    float* dX[CONCAT_MAX_SEG];
    int ldx[CONCAT_MAX_SEG], lddx[CONCAT_MAX_SEG], dk[CONCAT_MAX_SEG], col[CONCAT_MAX_SEG];
    unsigned vec[CONCAT_MAX_SEG];
};

template <int WM, int WN, bool DX, bool FAST>
__global__ __launch_bounds__(THREADS) void fc_concat_bwd_kernel(ConcatBwdLaunch g) {
    constexpr int TN = 64 * WN;
    const int total = g.tile_start[g.n], chunk = (int)blockIdx.x / total;
    int t = (int)blockIdx.x % total, s = 0;
    while (s + 1 < g.n && t >= g.tile_start[s + 1]) ++s;                    // block-uniform: scalar loads from the arguments
    t -= g.tile_start[s];
    FcBwdArgs a = g.base;
    const int col = g.col[s];
    a.Dk = g.dk[s];
    a.vec = g.vec[s];
    if constexpr (DX) {
        a.W = g.base.W + col;
        a.dX = g.dX[s];
        a.lddx = g.lddx[s];
    } else {
        a.X = g.X[s];
        a.ldx = g.ldx[s];
        a.dW = g.base.dW ? g.base.dW + col : nullptr;
    }
    const bool mm = DX || a.dW != nullptr;                                  // db alone: one column of blocks of the first segment
    const int M = DX ? a.N : a.D, tiles_n = mm ? (a.Dk + TN - 1) / TN : 1;
    const int tn = t % tiles_n, tm = t / tiles_n;
    const bool cut = (DX ? a.chunks_dx : a.chunks) > 1;
    const int pcols = g.part_col[g.n];
    float* out = cut ? a.part + (size_t)chunk * M * pcols + g.part_col[s] : DX ? a.dX : a.dW;
    const int ldo = cut ? pcols : DX ? a.lddx : a.lddw;
    float* db_out = DX || a.db == nullptr || s != 0 ? nullptr : a.chunks > 1 ? a.part_db + (size_t)chunk * a.D : a.db;
    fc_bwd_tile<WM, WN, DX, FAST>(a, tm, tn, chunk, out, ldo, db_out);
}

// out_s[r, c] = part[0][r, col_s + c] + part[1][r, col_s + c] + ... in chunk order, for every segment s of a partial row
struct ConcatBwdReduce {
    const float* part;
    int chunks, rows, n;
    int part_col[CONCAT_MAX_SEG + 1];
    float* out[CONCAT_MAX_SEG];
    int ldo[CONCAT_MAX_SEG];
};
__global__ __launch_bounds__(THREADS) void fc_concat_bwd_reduce(ConcatBwdReduce r) {
    const int pcols = r.part_col[r.n];
    const size_t stride = (size_t)r.rows * pcols, i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= stride) return;
    float sum = r.part[i];
    for (int c = 1; c < r.chunks; ++c) sum += r.part[c * stride + i];
    const int row = (int)(i / pcols), pc = (int)(i % pcols);
    int s = 0;
    while (s + 1 < r.n && pc >= r.part_col[s + 1]) ++s;
    r.out[s][(size_t)row * r.ldo[s] + (pc - r.part_col[s])] = sum;
}

template <bool DX>
hipError_t launch_product(const ConcatBwdLaunch& g, int edge, bool fast, int chunks, hipStream_t st) {
    const long long blocks = (long long)g.tile_start[g.n] * chunks;
    if (blocks == 0) return hipSuccess;
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(THREADS);
    if (edge == 128 && fast) hipLaunchKernelGGL((fc_concat_bwd_kernel<2, 2, DX, true>), grid, block, 0, st, g);
    else if (edge == 128) hipLaunchKernelGGL((fc_concat_bwd_kernel<2, 2, DX, false>), grid, block, 0, st, g);
    else if (fast) hipLaunchKernelGGL((fc_concat_bwd_kernel<1, 1, DX, true>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((fc_concat_bwd_kernel<1, 1, DX, false>), grid, block, 0, st, g);
    return hipGetLastError();
}

hipError_t launch_reduce(const ConcatBwdReduce& r, hipStream_t st) {
    const size_t n = (size_t)r.rows * r.part_col[r.n];
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fc_concat_bwd_reduce, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, r);
    return hipGetLastError();
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void fc_concat_bwd_plan(int N, int D, const int* dk, int n, int dx_cols, FcBwdPlan* p) {
    long long w128 = 0, w64 = 0, x128 = 0, x64 = 0, cols = 0;
    for (int s = 0; s < n; ++s) {
        w128 += tiles_of(D, dk[s], 128), w64 += tiles_of(D, dk[s], 64);
        x128 += tiles_of(N, dk[s], 128), x64 += tiles_of(N, dk[s], 64);
        cols += dk[s];
    }
    plan_tiles(w128, w64, N, &p->tile_dw, &p->chunks, &p->chunk_rows);
    plan_tiles(x128, x64, D, &p->tile_dx, &p->chunks_dx, &p->chunk_len_dx);
    p->ws_db = p->chunks > 1 ? (size_t)p->chunks * D * sizeof(float) : 0;
    p->ws_dw = p->chunks > 1 ? (size_t)p->chunks * D * cols * sizeof(float) + p->ws_db : 0;
    p->ws_dx = p->chunks_dx > 1 ? (size_t)p->chunks_dx * N * dx_cols * sizeof(float) : 0;
}

hipError_t launch_fc_concat_backward(const FcConcatBwdArgs& q, hipStream_t st) {
    if (q.nseg < 1 || q.N < 1) return hipSuccess;
    int dk[CONCAT_MAX_SEG], dx_cols = 0;
    for (int s = 0; s < q.nseg; ++s) {
        dk[s] = q.seg[s].dk;
        if (q.seg[s].dX) dx_cols += dk[s];
    }
    FcBwdPlan p;
    fc_concat_bwd_plan(q.N, q.D, dk, q.nseg, dx_cols, &p);

    ConcatBwdLaunch g{};
    FcBwdArgs& b = g.base;
    b.W = q.W; b.A = q.A; b.dA = q.dA; b.dW = q.dW; b.db = q.db;
    b.N = q.N; b.D = q.D; b.ldw = q.ldw; b.lda = q.lda; b.ldda = q.ldda; b.lddw = q.lddw; b.act = q.act;
    b.chunks = p.chunks; b.chunk_rows = p.chunk_rows; b.chunks_dx = p.chunks_dx; b.chunk_len_dx = p.chunk_len_dx;
    b.part = q.part;
    const unsigned vec_z = aligned16(q.A) && aligned16(q.dA) && q.lda % 4 == 0 && q.ldda % 4 == 0 ? 1u : 0u;

    if (q.dW || q.db) {
        // db alone: the first segment's column of blocks and nothing else
        const int edge = p.tile_dw, n = q.dW ? q.nseg : 1;
        bool fast = vec_z && q.D % edge == 0 && q.N % KT == 0;
        g.n = n;
        for (int s = 0; s < n; ++s) {
            const FcConcatBwdSeg& f = q.seg[s];
            g.X[s] = f.X; g.ldx[s] = f.ldx; g.dk[s] = f.dk; g.col[s] = f.col;
            g.vec[s] = vec_z | (f.X && aligned16(f.X) && f.ldx % 4 == 0 ? 2u : 0u);
            if (q.dW) fast = fast && (g.vec[s] & 2u) && f.dk % edge == 0;
            g.tile_start[s + 1] = g.tile_start[s] + (int)(q.dW ? tiles_of(q.D, f.dk, edge) : (q.D + edge - 1) / edge);
            g.part_col[s + 1] = g.part_col[s] + f.dk;
        }
        if (p.chunks > 1) b.part_db = q.part + (q.dW ? (size_t)p.chunks * q.D * g.part_col[n] : 0);
        if (hipError_t e = launch_product<false>(g, edge, fast, p.chunks, st)) return e;
        if (p.chunks > 1) {
            if (q.dW) {
                ConcatBwdReduce r{};
                r.part = q.part; r.chunks = p.chunks; r.rows = q.D; r.n = n;
                for (int s = 0; s < n; ++s) {
                    r.part_col[s + 1] = g.part_col[s + 1];
                    r.out[s] = q.dW + g.col[s];
                    r.ldo[s] = q.lddw;
                }
                if (hipError_t e = launch_reduce(r, st)) return e;
            }
            if (q.db) {
                ConcatBwdReduce r{};
                r.part = b.part_db; r.chunks = p.chunks; r.rows = 1; r.n = 1;
                r.part_col[1] = q.D; r.out[0] = q.db; r.ldo[0] = q.D;
                if (hipError_t e = launch_reduce(r, st)) return e;
            }
        }
    }
    if (dx_cols) {
        const int edge = p.tile_dx;
        bool fast = vec_z && q.N % edge == 0 && q.D % KT == 0;
        int n = 0;
        ConcatBwdReduce r{};
        for (int s = 0; s < q.nseg; ++s) {
            const FcConcatBwdSeg& f = q.seg[s];
            if (!f.dX) continue;
            g.dX[n] = f.dX; g.lddx[n] = f.lddx; g.dk[n] = f.dk; g.col[n] = f.col;
            g.vec[n] = vec_z | (aligned16(q.W + f.col) && q.ldw % 4 == 0 ? 4u : 0u);
            fast = fast && (g.vec[n] & 4u) && f.dk % edge == 0;
            g.tile_start[n + 1] = g.tile_start[n] + (int)tiles_of(q.N, f.dk, edge);
            g.part_col[n + 1] = g.part_col[n] + f.dk;
            r.part_col[n + 1] = g.part_col[n + 1]; r.out[n] = f.dX; r.ldo[n] = f.lddx;
            ++n;
        }
        g.n = n;
        if (hipError_t e = launch_product<true>(g, edge, fast, p.chunks_dx, st)) return e;
        if (p.chunks_dx > 1) {
            r.part = q.part; r.chunks = p.chunks_dx; r.rows = q.N; r.n = n;
            return launch_reduce(r, st);
        }
    }
    return hipSuccess;
}

}  // namespace laff
