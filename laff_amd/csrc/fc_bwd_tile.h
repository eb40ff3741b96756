// fc_bwd_tile.h -- the tile body and the cut of the dense backward products, shared by fc_bwd.hip (one X: laff_fc_backward) and
// fc_concat_bwd.hip (the column windows of a concat layer in one launch: laff_fc_concat_backward).  DESIGN.md 4.20, 4.30.
//
// A block of four wavefronts (2 x 2) owns a TM x TN output tile of  dW = dZ^T X  (DX = false) or  dX = dZ W  (DX = true), each wavefront
// WM x WN accumulators of 32 x 32 on v_mfma_f32_32x32x2_f32 (bit-for-bit an fp32 fmaf chain in k order); the operands pass through
// LDS in steps of KT = 32 of the contraction index and dZ = dA (.) act'(A) is formed on the way.  The including kernel says which
// tile the block owns and where it goes; everything else is read from FcBwdArgs.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fc_bwd_common.h"
#include "kernels.h"

namespace laff {
namespace fcbwd {

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

// Tile (tm, tn) of chunk `chunk` of one product.  out / ldo: where the tile's [M, NC] matrix starts and its pitch (the output itself,
// or this chunk's partial matrix); db_out: where this chunk's db [D] goes, or null -- the blocks of the first column tile sum it.
template <int WM, int WN, bool DX, bool FAST>
__device__ __forceinline__ void fc_bwd_tile(const FcBwdArgs& a, int tm, int tn, int chunk, float* out, int ldo, float* db_out) {
    constexpr int TM = 64 * WM, TN = 64 * WN;
    constexpr int GA = TM / 32, GB = TN / 32;               // 16-byte groups per thread and step of either operand
    constexpr int PA = KT + 1;                              // dX: pitch of the [TM][KT] tile of dZ
    __shared__ __attribute__((aligned(16))) float sA[DX ? TM * PA : KT * TM];
    __shared__ __attribute__((aligned(16))) float sB[KT * TN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const bool mm = DX || a.dW != nullptr;                  // db alone: one column of blocks, no product
    const int M = DX ? a.N : a.D, NC = a.Dk;                // the output is [M, NC]
    const int m0 = tm * TM, c0 = tn * TN;
    const int klen = DX ? a.chunk_len_dx : a.chunk_rows;
    const int kbeg = chunk * klen, kend = min(DX ? a.D : a.N, kbeg + klen);
    const float* B = DX ? a.W : a.X;
    const int ldb = DX ? a.ldw : a.ldx;
    const bool vec_z = a.vec & 1, vec_b = a.vec & (DX ? 4 : 2);
    const bool do_db = !DX && db_out != nullptr && tn == 0;

    // One step's operands go from global memory to registers (fetch) and from there to LDS (stage); fetch for step k + 1 is issued before
    // the MFMAs of step k and nothing looks at its registers until stage, so the loads fly under the MFMAs.  dZ = dA (.) act'(A) is
    // therefore formed in stage, not in fetch.  FAST is the instantiation for shapes made of whole tiles and whole steps with 16-byte
    // aligned rows: plain 16-byte loads and no branch.  The choice is the kernel's, not a branch inside it: where two
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
        if (do_db && tid < TM && m0 + tid < a.D) db_out[m0 + tid] = dbacc;
    }
}

inline long long tiles_of(int rows, int cols, int edge) { return (long long)((rows + edge - 1) / edge) * ((cols + edge - 1) / edge); }

// The tile edge and the cut of a product whose outputs make t128 tiles of 128 x 128 or t64 of 64 x 64, summed over K.  128 x 128
// tiles where they fill the chip -- at least FILL_128 blocks, on their own or with the sum cut into pieces of SPLIT_LEN or more --
// and 64 x 64 tiles otherwise, cut until there are FILL_64 blocks.  A chunk's length is a multiple of KT.
inline void plan_tiles(long long t128, long long t64, int K, int* edge, int* chunks, int* len) {
    const long long pieces = std::max(1, (K + SPLIT_LEN - 1) / SPLIT_LEN);
    t128 = std::max(1LL, t128), t64 = std::max(1LL, t64);                   // no rows: N == 0
    const long long c128 = std::min(pieces, (FILL_128 + t128 - 1) / t128), c64 = std::min(pieces, (FILL_64 + t64 - 1) / t64);
    const bool big = t128 * c128 >= FILL_128;
    const long long c = big ? c128 : c64;
    *edge = big ? 128 : 64;
    *len = K > 0 ? (int)(((K + c - 1) / c + KT - 1) / KT * KT) : KT;
    *chunks = K > 0 ? (K + *len - 1) / *len : 1;
}

}  // namespace fcbwd
}  // namespace laff
