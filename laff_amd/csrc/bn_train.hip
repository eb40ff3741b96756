// bn_train.hip -- the stage between a projection's activation and its output in training mode, for gfx950, fp32: dropout by a
// counter-based mask, then BatchNorm1d on batch statistics; forward and backward.
//
//   m[n,c] = keep(seed, n, c) / (1 - p)        U = A (.) m        (m = 1 when p == 0)
//   forward:   mean = sum_n U / N    var = sum_n (U - mean)^2 / N    invstd = 1 / sqrt(var + eps)    Y = gamma (U - mean) invstd + beta
//              running_mean = (1 - momentum) running_mean + momentum mean      running_var likewise with var N / (N - 1)
//   backward:  xhat = (U - mean) invstd    dbeta = sum_n dY    dgamma = sum_n dY (.) xhat
//              dU = gamma invstd (dY - dbeta / N - xhat dgamma / N)             dA = dU (.) m
//   without a BatchNorm stage (gamma == null):  Y = U,  dA = dY (.) m.
//
// The mask is Philox4x32-10 with key (seed lo, seed hi) and counter (c >> 2, n, 0, 0); element (n, c) takes word c & 3 and is kept iff
// word >= thresh = floor(p 2^32).  A lane holds four aligned consecutive columns of a row: one generator call per 16 bytes.  The mask is
// recomputed by the backward and never stored.
//
// A block of 256 threads owns 32 columns (8 lanes x 16 bytes) and a chunk of BN_TRAIN_ROWS = 256 rows, 32 interleaved row groups of 8
// rows each: the strip of U stays in registers between the statistics and the normalising pass, A is read once.  A column sum is each
// thread's 8 rows in row order, then the 32 group sums in group order (sum_rows_fixed_order_of).  The variance is the corrected
// two-pass form: mean0 = sum / n in fp32, then d = U - mean0, S1 = sum d, S2 = sum d^2, and in float64 on the eight lanes of group 0
// mean = mean0 + S1 / n, M2 = S2 - S1^2 / n -- S1 is rounding residue, nothing cancels.  N > 256 is cut into row chunks (grid.y):
// launch PART leaves each chunk's (mean, M2) -- backward: (sum dY, sum dY xhat) -- in the workspace as float64, launch APPLY merges
// them in chunk order (Chan's update) in every block of a column strip and normalises.  No atomics: two calls give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bn_train_common.h"

namespace laff {

namespace {

using namespace bn_strip;

// Philox4x32-10, counter (c0, c1, 0, 0)
__device__ __forceinline__ uint4 philox4x32_10(unsigned c0, unsigned c1, unsigned k0, unsigned k1) {
    unsigned c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// t (.) m for the mask bits `keep` (bit e: column c + e is kept)
__device__ __forceinline__ float4 masked(float4 t, unsigned keep, float scale) {
    return make_float4(keep & 1 ? t.x * scale : 0.f, keep & 2 ? t.y * scale : 0.f, keep & 4 ? t.z * scale : 0.f, keep & 8 ? t.w * scale : 0.f);
}

// The thread's rows of the chunk: slot i is row grp + 32 i (valid below nr).  u = A (.) m, zeros in slots without a row; keep holds
// the four mask bits of slot i at bit 4 i (all ones without dropout).  The loads are issued first, the generator runs under them.
template <bool FAST>
__device__ __forceinline__ void load_strip(const BnTrainArgs& a, int r0, int nr, int c, float4 (&u)[SLOTS], unsigned& keep) {
    const int grp = threadIdx.x / DW_LANES;
    const bool has = c < a.D;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int r = grp + i * DW_GROUPS;
        u[i] = has && r < nr ? load4<FAST>(a.A + (size_t)(r0 + r) * a.lda, c, a.D) : zero4();
    }
    keep = 0xffffffffu;
    if (a.drop) {
        const unsigned long long s = *a.seed;
        keep = 0;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const uint4 w = philox4x32_10((unsigned)c >> 2, (unsigned)(r0 + grp + i * DW_GROUPS), (unsigned)s, (unsigned)(s >> 32));
            const unsigned k = (w.x >= a.thresh ? 1u : 0u) | (w.y >= a.thresh ? 2u : 0u) | (w.z >= a.thresh ? 4u : 0u) | (w.w >= a.thresh ? 8u : 0u);
            u[i] = masked(u[i], k, a.scale);
            keep |= k << (4 * i);
        }
    }
}

template <bool FAST, int MODE>
__global__ __launch_bounds__(THREADS) void bn_train_fwd(BnTrainArgs a) {
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    __shared__ float4 bc[4][DW_LANES];
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    const int c = blockIdx.x * COLS + 4 * ln;
    const int r0 = blockIdx.y * BN_TRAIN_ROWS, nr = min(BN_TRAIN_ROWS, a.N - r0);
    float4 u[SLOTS];
    unsigned keep;
    load_strip<FAST>(a, r0, nr, c, u, keep);

    if (a.gamma) {
        double mean[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0};          // of all N rows, in group 0
        if constexpr (MODE != APPLY) {
            strip_mean_m2(u, nr, sh, bc[0], mean, m2);                                  // slots without a row hold zeros
            if (MODE == PART && grp == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < a.D) {
                        a.part[(size_t)(2 * blockIdx.y) * a.D + c + e] = mean[e];
                        a.part[(size_t)(2 * blockIdx.y + 1) * a.D + c + e] = m2[e];
                    }
            }
            if constexpr (MODE == PART) return;
        } else if (grp == 0) {
            // the chunks' (mean, M2) merged in chunk order
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < a.D) merge_mean_m2(a.part, a.D, a.N, c + e, mean[e], m2[e]);
        }
        if (grp == 0) {
            // the mean goes to the rows as fp32 head and tail: at mean 30 and deviation 0.01 the head's rounding alone is 1e-4 of y
            f4a mu{}, lo{}, w{}, b{};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e >= a.D) continue;
                const double invstd = 1.0 / sqrt(m2[e] / a.N + a.eps);
                mu.v[e] = (float)mean[e];
                lo.v[e] = (float)(mean[e] - (double)mu.v[e]);
                w.v[e] = a.gamma[c + e] * (float)invstd;
                b.v[e] = a.beta[c + e];
                if (blockIdx.y == 0) {
                    a.save_mean[c + e] = mu.v[e];
                    a.save_invstd[c + e] = (float)invstd;
                    update_running(a.running_mean + c + e, a.running_var + c + e, a.momentum, mean[e], m2[e], a.N);
                }
            }
            bc[0][ln] = vec(mu);
            bc[1][ln] = vec(w);
            bc[2][ln] = vec(b);
            bc[3][ln] = vec(lo);
        }
        __syncthreads();
        const float4 mu = bc[0][ln], w = bc[1][ln], b = bc[2][ln], lo = bc[3][ln];
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const float4 d = sub4(sub4(u[i], mu), lo);
            u[i] = make_float4(fmaf(d.x, w.x, b.x), fmaf(d.y, w.y, b.y), fmaf(d.z, w.z, b.z), fmaf(d.w, w.w, b.w));
        }
    }
    if (c < a.D) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int r = grp + i * DW_GROUPS;
            if (r < nr) store4<FAST>(a.out + (size_t)(r0 + r) * a.ldo, c, a.D, u[i]);
        }
    }
}

template <bool FAST, int MODE>
__global__ __launch_bounds__(THREADS) void bn_train_bwd(BnTrainArgs a) {
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    __shared__ float4 bc[2][DW_LANES];
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    const int c = blockIdx.x * COLS + 4 * ln;
    const int r0 = blockIdx.y * BN_TRAIN_ROWS;
    const int nr = MODE == APPLY && !a.out ? 0 : min(BN_TRAIN_ROWS, a.N - r0);       // dgamma / dbeta alone: no row is read again
    float4 u[SLOTS], g[SLOTS];
    unsigned keep;
    load_strip<FAST>(a, r0, a.gamma ? nr : 0, c, u, keep);                            // without statistics only the mask is needed, not A
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int r = grp + i * DW_GROUPS;
        g[i] = c < a.D && r < nr ? load4<FAST>(a.dY + (size_t)(r0 + r) * a.lddy, c, a.D) : zero4();
    }

    if (a.gamma) {
        const float4 mu = cols4(a.save_mean, c, a.D), is = cols4(a.save_invstd, c, a.D);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) u[i] = grp + i * DW_GROUPS < nr ? mul4(sub4(u[i], mu), is) : zero4();      // xhat
        double tot[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};               // dbeta, dgamma over all N rows, in group 0
        if constexpr (MODE != APPLY) {
            float4 own1, own2;
            strip_dot(g, u, own1, own2);
            const float4 s1 = sum_groups(own1, sh);
            __syncthreads();
            const float4 s2 = sum_groups(own2, sh);
            if (grp == 0) {
                const f4a t1 = arr(s1), t2 = arr(s2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tot[0][e] = t1.v[e];
                    tot[1][e] = t2.v[e];
                    if (MODE == PART && c + e < a.D) {
                        a.part[(size_t)(2 * blockIdx.y) * a.D + c + e] = tot[0][e];
                        a.part[(size_t)(2 * blockIdx.y + 1) * a.D + c + e] = tot[1][e];
                    }
                }
            }
            if constexpr (MODE == PART) return;
        } else if (grp == 0) {
            const int chunks = (a.N + BN_TRAIN_ROWS - 1) / BN_TRAIN_ROWS;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e >= a.D) continue;
                for (int k = 0; k < chunks; ++k) {
                    tot[0][e] += a.part[(size_t)(2 * k) * a.D + c + e];
                    tot[1][e] += a.part[(size_t)(2 * k + 1) * a.D + c + e];
                }
            }
        }
        if (grp == 0) {
            f4a k1{}, k2{};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e >= a.D) continue;
                if (blockIdx.y == 0) {
                    if (a.dbeta) a.dbeta[c + e] = (float)tot[0][e];
                    if (a.dgamma) a.dgamma[c + e] = (float)tot[1][e];
                }
                k1.v[e] = (float)(tot[0][e] / a.N);
                k2.v[e] = (float)(tot[1][e] / a.N);
            }
            bc[0][ln] = vec(k1);
            bc[1][ln] = vec(k2);
        }
        if (!a.out) return;
        __syncthreads();
        const float4 k1 = bc[0][ln], k2 = bc[1][ln], w = mul4(cols4(a.gamma, c, a.D), is);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) g[i] = bn_du(g[i], u[i], w, k1, k2);
    }
    if (a.out && c < a.D) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int r = grp + i * DW_GROUPS;
            if (r < nr) store4<FAST>(a.out + (size_t)(r0 + r) * a.ldo, c, a.D, a.drop ? masked(g[i], keep >> (4 * i), a.scale) : g[i]);
        }
    }
}

template <bool FWD, int MODE>
hipError_t launch(const BnTrainArgs& a, int row_blocks, hipStream_t st) {
    const dim3 grid((unsigned)((a.D + COLS - 1) / COLS), (unsigned)row_blocks), block(THREADS);
    if constexpr (FWD) {
        if (a.fast) hipLaunchKernelGGL((bn_train_fwd<true, MODE>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((bn_train_fwd<false, MODE>), grid, block, 0, st, a);
    } else {
        if (a.fast) hipLaunchKernelGGL((bn_train_bwd<true, MODE>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((bn_train_bwd<false, MODE>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

template <bool FWD>
hipError_t launch_direction(const BnTrainArgs& a, hipStream_t st) {
    const int row_blocks = (a.N + BN_TRAIN_ROWS - 1) / BN_TRAIN_ROWS;
    if (!a.gamma || row_blocks == 1) return launch<FWD, WHOLE>(a, row_blocks, st);          // without statistics every chunk is on its own
    if (hipError_t e = launch<FWD, PART>(a, row_blocks, st)) return e;
    return launch<FWD, APPLY>(a, FWD || a.out ? row_blocks : 1, st);
}

}  // namespace

void bn_train_plan(int N, int D, bool has_bn, BnTrainPlan* p) {
    p->chunks = has_bn ? std::max(1, (N + BN_TRAIN_ROWS - 1) / BN_TRAIN_ROWS) : 1;
    p->launches = p->chunks > 1 ? 2 : 1;
    p->ws = p->chunks > 1 ? (size_t)p->chunks * 2 * D * sizeof(double) : 0;
}

hipError_t launch_bn_train_forward(const BnTrainArgs& a, hipStream_t st) { return launch_direction<true>(a, st); }
hipError_t launch_bn_train_backward(const BnTrainArgs& a, hipStream_t st) { return launch_direction<false>(a, st); }

}  // namespace laff
