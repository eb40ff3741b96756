// sim_hist.hip -- the 'hist' measure (generalised Jaccard / histogram intersection; loss.py:43-65, evaluation.py:19-41):
//
//   S[t, v] = (1 / H) sum_h J(T[t, h, :], V[v, h, :]),   J(x, y) = sum_k min(x_k, y_k) / (sum_k max(x_k, y_k) + eps)
//
// min-sum is not a matrix product, so this is an SGEMM-shaped fp32 VALU kernel with min / max + add in place of the FMA.  A
// workgroup of 256 threads owns 128 text rows x 64 video rows; K runs through the LDS in steps of 16 (two buffers, one barrier per
// step, the next step's global loads in flight during the arithmetic); a thread keeps an 8 x 4 block of pairs, an intersection and
// a union sum each, in registers and issues four VALU instructions per element pair: v_min_f32, v_max_f32 and two adds.
//
// Both sums are accumulated, as the reference does.  The shortcut sum max = sum x + sum y - sum min halves the arithmetic and is as
// accurate on non-negative inputs, but on signed inputs (the towers' tanh embeddings) it hands the error of the larger sum to the
// smaller one: measured on such embeddings (H = 2, d = 32) it missed 4 e_ref + 2^-23 by a factor of 1.9 where this form sits at 0.4.
//
// A pair's sums are added in order within a chunk of 128 elements, and the chunks in order into a second accumulator, so the
// rounding error grows like sqrt(128) + sqrt(d / 128) ulps and not like sqrt(d).  Heads are walked one after the other; a head's
// last step is zero-filled past d (min(0, 0) = max(0, 0) = 0: exact), as are the rows past Nt / Nv.  No atomics: every sum has one
// fixed order, the result is bitwise reproducible and does not depend on the load path (16-byte loads when base and pitch allow it,
// 4-byte loads otherwise).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace laff {

namespace {

constexpr int SH_BM = 128;          // text rows of a workgroup's tile
constexpr int SH_BN = 64;           // video rows
constexpr int SH_BK = 16;           // elements of K per LDS step
constexpr int SH_THREADS = 256;     // 16 x 16 threads, 8 x 4 pairs each
constexpr int SH_CHUNK_STEPS = 8;   // steps (128 elements) summed in order before they go to the second accumulator

// N (4 or 8) consecutive elements k .. k+N-1 of a head of one row, zero past the head's end d and for a row past the matrix (`in`
// false; `row` is then another row of the matrix, so that every address formed is a valid one)
template <int N>
__device__ __forceinline__ void sh_load(const float* __restrict__ row, bool in, int k, int d, bool vec, float (&r)[N]) {
    if (vec && k + N <= d) {
#pragma unroll
        for (int i = 0; i < N; i += 4) {
            const float4 q = *reinterpret_cast<const float4*>(row + k + i);
            r[i] = q.x; r[i + 1] = q.y; r[i + 2] = q.z; r[i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) r[i] = row[min(k + i, d - 1)];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = (in && k + i < d) ? r[i] : 0.0f;
}

template <bool MULTI>
__global__ __launch_bounds__(SH_THREADS, 2) void sim_hist_kernel(const SimHistArgs a) {
    __shared__ __attribute__((aligned(16))) float As[2][SH_BK][SH_BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][SH_BK][SH_BN];

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long t0 = (long)(blockIdx.x / a.tilesV) * SH_BM, v0 = (long)(blockIdx.x % a.tilesV) * SH_BN;
    // loader role: text row ar, elements ak .. ak+7 of every step; video row br, elements bk .. bk+3
    const int ar = tid & (SH_BM - 1), ak = (tid >> 7) * 8, br = tid & (SH_BN - 1), bk = (tid >> 6) * 4;
    const bool tin = t0 + ar < a.Nt, vin = v0 + br < a.Nv;
    const float* tp = a.T + (tin ? t0 + ar : 0L) * a.ldt;
    const float* vp = a.V + (vin ? v0 + br : 0L) * a.ldv;
    const bool vecT = a.vec & 1, vecV = a.vec & 2;
    const int d = a.d, sph = (d + SH_BK - 1) / SH_BK, total = a.H * sph;

    float lo[8][4], hi[8][4], lo2[8][4], hi2[8][4], accS[MULTI ? 8 : 1][4];      // sum min / sum max: chunk, head; sum of J
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo[i][j] = hi[i][j] = lo2[i][j] = hi2[i][j] = 0.0f;
            if constexpr (MULTI) accS[i][j] = 0.0f;
        }
    float ra[8], rb[4];
    sh_load<8>(tp, tin, ak, d, vecT, ra);
    sh_load<4>(vp, vin, bk, d, vecV, rb);

    int h = 0, ks = 0;                                     // head, step within the head
    for (int s = 0; s < total; ++s) {
        const int buf = s & 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) As[buf][ak + i][ar] = ra[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[buf][bk + i][br] = rb[i];
        __syncthreads();                                   // this buffer was last read two steps ago, before the previous barrier
        const bool last = ks == sph - 1;
        const int h1 = last ? h + 1 : h, ks1 = last ? 0 : ks + 1;
        if (s + 1 < total) {
            const long off = (long)h1 * d;
            sh_load<8>(tp + off, tin, ks1 * SH_BK + ak, d, vecT, ra);
            sh_load<4>(vp + off, vin, ks1 * SH_BK + bk, d, vecV, rb);
        }
#pragma unroll 2
        for (int kk = 0; kk < SH_BK; ++kk) {
            const float4 a0 = *reinterpret_cast<const float4*>(&As[buf][kk][ty * 4]);
            const float4 a1 = *reinterpret_cast<const float4*>(&As[buf][kk][64 + ty * 4]);
            const float4 b0 = *reinterpret_cast<const float4*>(&Bs[buf][kk][tx * 4]);
            const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float y[4] = {b0.x, b0.y, b0.z, b0.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lo[i][j] += fminf(x[i], y[j]);
                    hi[i][j] += fmaxf(x[i], y[j]);
                }
        }
        if (last || (ks & (SH_CHUNK_STEPS - 1)) == SH_CHUNK_STEPS - 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lo2[i][j] += lo[i][j];
                    hi2[i][j] += hi[i][j];
                    lo[i][j] = hi[i][j] = 0.0f;
                }
        }
        if (last) {                                        // the head is complete
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float jac = lo2[i][j] / (hi2[i][j] + a.eps);                  // IEEE: 0 / 0 = NaN when eps == 0
                    lo2[i][j] = hi2[i][j] = 0.0f;
                    if constexpr (MULTI) {
                        accS[i][j] += jac;
                    } else {
                        const long row = t0 + ty * 4 + (i & 3) + (i >> 2) * 64, col = v0 + tx * 4 + j;
                        if (row < a.Nt && col < a.Nv) a.S[row * a.lds + col] = jac;
                    }
                }
        }
        h = h1;
        ks = ks1;
    }
    if constexpr (MULTI) {
        const float heads = (float)a.H;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long row = t0 + ty * 4 + (i & 3) + (i >> 2) * 64, col = v0 + tx * 4 + j;
                if (row < a.Nt && col < a.Nv) a.S[row * a.lds + col] = accS[i][j] / heads;
            }
    }
}

}  // namespace

bool sim_hist_tiles(int Nt, int Nv, unsigned* tilesV, unsigned* tiles) {
    const long tv = ((long)Nv + SH_BN - 1) / SH_BN, n = (((long)Nt + SH_BM - 1) / SH_BM) * tv;
    if (n > 0x7fffffffL) return false;
    *tilesV = (unsigned)tv;
    *tiles = (unsigned)n;
    return true;
}

hipError_t launch_sim_hist(const SimHistArgs& a, unsigned tiles, hipStream_t st) {
    if (a.H > 1) hipLaunchKernelGGL(sim_hist_kernel<true>, dim3(tiles), dim3(SH_THREADS), 0, st, a);
    else hipLaunchKernelGGL(sim_hist_kernel<false>, dim3(tiles), dim3(SH_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace laff
