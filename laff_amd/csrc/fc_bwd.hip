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
#include "kernels.h"

namespace laff {

namespace {

constexpr int KT = 32, THREADS = 256, SPLIT_LEN = 128, FILL_64 = 512, FILL_128 = 256;

typedef float bw_f32x4 __attribute__((ext_vector_type(4)));
typedef float bw_f32x16 __attribute__((ext_vector_type(16)));

// the G groups of a thread at once: one switch per step, not one per element
template <int ACT, int G>
__device__ __forceinline__ void dact_groups(const bw_f32x4 (&a)[G], const bw_f32x4 (&g)[G], bw_f32x4 (&z)[G]) {
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) z[i][e] = dact<ACT>(a[i][e], g[i][e]);
}

// columns [c, c + 4) of a row of `width` floats, zeros past its end; one 16-byte load when the row allows it
__device__ __forceinline__ bw_f32x4 load4(const float* row, int c, int width, bool vec) {
    bw_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && c + 3 < width) {
        v = *reinterpret_cast<const bw_f32x4*>(row + c);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < width) v[e] = row[c + e];
    }
    return v;
}

template <int WM, int WN, bool DX, bool FAST>
__global__ __launch_bounds__(THREADS) void fc_bwd_kernel(FcBwdArgs a) {
    constexpr int TM = 64 * WM, TN = 64 * WN;
    constexpr int GA = TM / 32, GB = TN / 32;               // 16-byte groups per thread and step of either operand
    constexpr int PA = KT + 1;                              // dX: pitch of the [TM][KT] tile of dZ
    __shared__ __attribute__((aligned(16))) float sA[DX ? TM * PA : KT * TM];
    __shared__ __attribute__((aligned(16))) float sB[KT * TN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const bool mm = DX || a.dW != nullptr;                  // db alone: one column of blocks, no product
    const int M = DX ? a.N : a.D, NC = a.Dk;                // the output is [M, NC]
    const int tiles_n = mm ? (NC + TN - 1) / TN : 1, tiles_m = (M + TM - 1) / TM;
    int bid = blockIdx.x;
    const int tn = bid % tiles_n;
    bid /= tiles_n;
    const int tm = bid % tiles_m, chunk = bid / tiles_m;
    const int m0 = tm * TM, c0 = tn * TN;
    const int klen = DX ? a.chunk_len_dx : a.chunk_rows;
    const int kbeg = chunk * klen, kend = min(DX ? a.D : a.N, kbeg + klen);
    const float* B = DX ? a.W : a.X;
    const int ldb = DX ? a.ldw : a.ldx;
    const bool vec_z = a.vec & 1, vec_b = a.vec & (DX ? 4 : 2);
    const bool do_db = !DX && a.db != nullptr && tn == 0;

    // One step's operands go from global memory to registers (fetch) and from there to LDS (stage); fetch for step k + 1 is issued before
    // the MFMAs of step k and nothing looks at its registers until stage, so the loads fly under the MFMAs.  dZ = dA (.) act'(A) is
    // therefore formed in stage, not in fetch.  FAST is the instantiation for shapes made of whole tiles and whole steps with 16-byte
    // aligned rows (fc_bwd_fast): plain 16-byte loads and no branch.  The choice is the kernel's, not a branch inside it: where two
    // paths meet, hipcc copies the loaded registers into common ones and waits for the loads to do so -- before the MFMAs.
    bw_f32x4 ra[GA], rg[GA], rb[GB];
    auto fetch = [&](int k0) {
        if constexpr (FAST) {
#pragma unroll
            for (int i = 0; i < GA; ++i) {
                const int g = tid + i * THREADS;
                // dZ's tile: dW walks [k = row n][m = column j], dX walks [m = row n][k = column j]
                const int r = DX ? m0 + g / (KT / 4) : k0 + g / (TM / 4);
                const int c = DX ? k0 + 4 * (g % (KT / 4)) : m0 + 4 * (g % (TM / 4));
                ra[i] = *reinterpret_cast<const bw_f32x4*>(a.A + (size_t)r * a.lda + c);
                rg[i] = *reinterpret_cast<const bw_f32x4*>(a.dA + (size_t)r * a.ldda + c);
            }
            if (mm) {
#pragma unroll
                for (int i = 0; i < GB; ++i) {
                    const int g = tid + i * THREADS;
                    rb[i] = *reinterpret_cast<const bw_f32x4*>(B + (size_t)(k0 + g / (TN / 4)) * ldb + c0 + 4 * (g % (TN / 4)));
                }
            }
        } else {
            const bw_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < GA; ++i) {
                const int g = tid + i * THREADS;
                const int r = DX ? m0 + g / (KT / 4) : k0 + g / (TM / 4);
                const int c = DX ? k0 + 4 * (g % (KT / 4)) : m0 + 4 * (g % (TM / 4));
                const int cend = DX ? kend : a.D;           // dX: a chunk ends inside the row
                const bool in = r < (DX ? a.N : kend) && c < cend;
                ra[i] = in ? load4(a.A + (size_t)r * a.lda, c, cend, vec_z) : zero;
                rg[i] = in ? load4(a.dA + (size_t)r * a.ldda, c, cend, vec_z) : zero;   // past the end: zeros, and dact(0, 0) = 0
            }
            if (mm) {
#pragma unroll
                for (int i = 0; i < GB; ++i) {
                    const int g = tid + i * THREADS;
                    const int r = k0 + g / (TN / 4), c = c0 + 4 * (g % (TN / 4));
                    rb[i] = r < kend && c < NC ? load4(B + (size_t)r * ldb, c, NC, vec_b) : zero;
                }
            }
        }
    };
    auto stage = [&]() {
        bw_f32x4 z[GA];
        switch (a.act) {
            case LAFF_ACT_TANH: dact_groups<LAFF_ACT_TANH>(ra, rg, z); break;
            case LAFF_ACT_SIGMOID: dact_groups<LAFF_ACT_SIGMOID>(ra, rg, z); break;
            case LAFF_ACT_RELU: dact_groups<LAFF_ACT_RELU>(ra, rg, z); break;
            default: dact_groups<LAFF_ACT_NONE>(ra, rg, z); break;
        }
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const int g = tid + i * THREADS;
            if constexpr (DX) {
                float* p = sA + (g / (KT / 4)) * PA + 4 * (g % (KT / 4));
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = z[i][e];
            } else {
                *reinterpret_cast<bw_f32x4*>(sA + (g / (TM / 4)) * TM + 4 * (g % (TM / 4))) = z[i];
            }
        }
        if (mm) {
#pragma unroll
            for (int i = 0; i < GB; ++i) {
                const int g = tid + i * THREADS;
                *reinterpret_cast<bw_f32x4*>(sB + (g / (TN / 4)) * TN + 4 * (g % (TN / 4))) = rb[i];
            }
        }
    };

    bw_f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float dbacc = 0.f;

    if (kbeg < kend) fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        stage();
        __syncthreads();
        if (k0 + KT < kend) fetch(k0 + KT);                 // the next step's loads fly under this step's MFMAs
        if (mm) {
            // the fragments of sub-step kk + 1 are read while the MFMAs of kk run
            float fa[2][WM], fb[2][WN];
            auto frags = [&](int kk) {
                const int k = 2 * kk + hh;
#pragma unroll
                for (int i = 0; i < WM; ++i) {
                    const int m = (wm * WM + i) * 32 + l31;
                    fa[kk & 1][i] = DX ? sA[m * PA + k] : sA[k * TM + m];
                }
#pragma unroll
                for (int j = 0; j < WN; ++j) fb[kk & 1][j] = sB[k * TN + (wn * WN + j) * 32 + l31];
            };
            frags(0);
#pragma unroll
            for (int kk = 0; kk < KT / 2; ++kk) {
                if (kk + 1 < KT / 2) frags(kk + 1);
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk & 1][i], fb[kk & 1][j], acc[i][j], 0, 0, 0);
            }
        }
        if constexpr (!DX) {
            if (do_db && tid < TM) {
#pragma unroll 8
                for (int k = 0; k < KT; ++k) dbacc += sA[k * TM + tid];            // rows past kend hold zeros
            }
        }
        __syncthreads();
    }

    const bool cut = (DX ? a.chunks_dx : a.chunks) > 1;
    float* out = cut ? a.part + (size_t)chunk * M * NC : DX ? a.dX : a.dW;
    const int ldo = cut ? NC : DX ? a.lddx : a.lddw;
    if (mm) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const int col = c0 + (wn * WN + j) * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + (wm * WM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;     // the MFMA's C/D map
                    if (row < M && col < NC) out[(size_t)row * ldo + col] = acc[i][j][r];
                }
            }
    }
    if constexpr (!DX) {
        if (do_db && tid < TM && m0 + tid < a.D) (a.chunks > 1 ? a.part_db + (size_t)chunk * a.D : a.db)[m0 + tid] = dbacc;
    }
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

long long tiles_of(int rows, int cols, int edge) { return (long long)((rows + edge - 1) / edge) * ((cols + edge - 1) / edge); }

// The tiles and the cut of one product, [rows, cols] summed over K.  128 x 128 tiles where they fill the chip -- at least FILL_128
// blocks, on their own or with the sum cut into pieces of SPLIT_LEN or more -- and 64 x 64 tiles otherwise, cut until there are FILL_64
// blocks.  A chunk's length is a multiple of KT.
void plan_product(int rows, int cols, int K, int* edge, int* chunks, int* len) {
    const long long pieces = std::max(1, (K + SPLIT_LEN - 1) / SPLIT_LEN);
    const long long t128 = std::max(1LL, tiles_of(rows, cols, 128)), t64 = std::max(1LL, tiles_of(rows, cols, 64));     // rows == 0: N == 0
    const long long c128 = std::min(pieces, (FILL_128 + t128 - 1) / t128), c64 = std::min(pieces, (FILL_64 + t64 - 1) / t64);
    const bool big = t128 * c128 >= FILL_128;
    const long long c = big ? c128 : c64;
    *edge = big ? 128 : 64;
    *len = K > 0 ? (int)(((K + c - 1) / c + KT - 1) / KT * KT) : KT;
    *chunks = K > 0 ? (K + *len - 1) / *len : 1;
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
