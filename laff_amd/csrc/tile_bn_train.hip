// tile_bn_train.hip -- training-mode BatchNorm1d(H C) over a feature tiled H times, X.repeat(1, H), for gfx950, fp32: the no-transform
// feature of the LAFF towers (TransformNet(fc=False, batch_norm=True)), forward and backward.  The tiled input is
// never formed: the H copies of column c share their batch statistics, which are formed once per input column.
//
//   forward:   mean[c], var[c], invstd[c] of X[:, c]       Y[n, hC+c] = gamma[hC+c] (X[n,c] - mean[c]) invstd[c] + beta[hC+c]
//              running_mean[hC+c], running_var[hC+c] as bn_train.hip updates them
//   backward:  xhat = (X - mean) invstd    dbeta[hC+c] = sum_n dY[n,hC+c]    dgamma[hC+c] = sum_n dY[n,hC+c] xhat[n,c]
//              dU_h = gamma_h invstd (dY_h - dbeta_h / N - xhat dgamma_h / N)      dX[n,c] = sum_h dU_h[n,c], h ascending
//
// The strip, the sums and their order are those of bn_train.hip (bn_train_common.h): Y, the running statistics, dgamma and dbeta have
// the bits of laff_dropout_bn_train(_backward) with p = 0 on the materialised X.repeat(1, H).  grid = (column strips of C, row chunks,
// heads).  Forward: a block owns one head of a strip and forms the strip's statistics itself (X is H times smaller than Y and stays in
// L2), so one launch has the blocks of the materialised route.  Backward: with dX one block walks the heads of its strip in ascending
// order, the strip of xhat and the dX accumulator in registers, the next head's dY in flight under the current head's sums; without
// dX (a pre-extracted feature) the heads are spread over grid.z like the forward's.  N > 256: launch PART leaves the chunks' float64
// partials in the workspace, launch APPLY merges them in chunk order.  No atomics: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bn_train_common.h"

namespace laff {

namespace {

using namespace bn_strip;

// the thread's rows of columns [col0 + c, col0 + c + 4) of a matrix whose logical rows are C wide from col0 on; zeros without a row
template <bool FAST>
__device__ __forceinline__ void load_rows(const float* base, int ld, int r0, int nr, int c, int C, float4 (&t)[SLOTS]) {
    const int grp = threadIdx.x / DW_LANES;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int r = grp + i * DW_GROUPS;
        t[i] = c < C && r < nr ? load4<FAST>(base + (size_t)(r0 + r) * ld, c, C) : zero4();
    }
}
template <bool FAST>
__device__ __forceinline__ void store_rows(float* base, int ld, int r0, int nr, int c, int C, const float4 (&t)[SLOTS]) {
    const int grp = threadIdx.x / DW_LANES;
    if (c >= C) return;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int r = grp + i * DW_GROUPS;
        if (r < nr) store4<FAST>(base + (size_t)(r0 + r) * ld, c, C, t[i]);
    }
}

template <bool FAST, int MODE>
__global__ __launch_bounds__(THREADS) void tile_bn_fwd(TileBnTrainArgs a) {
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    __shared__ float4 bc[4][DW_LANES];
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    const int c = blockIdx.x * COLS + 4 * ln, h = blockIdx.z;
    const size_t hc = (size_t)h * a.C;
    const int r0 = blockIdx.y * BN_TRAIN_ROWS, nr = min(BN_TRAIN_ROWS, a.N - r0);
    float4 u[SLOTS];
    load_rows<FAST>(a.X, a.ldx, r0, nr, c, a.C, u);

    double mean[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0};              // of all N rows, in group 0
    if constexpr (MODE != APPLY) {
        strip_mean_m2(u, nr, sh, bc[0], mean, m2);
        if constexpr (MODE == PART) {                                                 // one head's blocks: the statistics have no head
            if (grp == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < a.C) {
                        a.part[(size_t)(2 * blockIdx.y) * a.C + c + e] = mean[e];
                        a.part[(size_t)(2 * blockIdx.y + 1) * a.C + c + e] = m2[e];
                    }
            }
            return;
        }
    } else if (grp == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < a.C) merge_mean_m2(a.part, a.C, a.N, c + e, mean[e], m2[e]);
    }
    if (grp == 0) {
        f4a mu{}, lo{}, w{}, b{};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c + e >= a.C) continue;
            const double invstd = 1.0 / sqrt(m2[e] / a.N + a.eps);
            mu.v[e] = (float)mean[e];
            lo.v[e] = (float)(mean[e] - (double)mu.v[e]);
            w.v[e] = a.gamma[hc + c + e] * (float)invstd;
            b.v[e] = a.beta[hc + c + e];
            if (blockIdx.y == 0) {
                if (h == 0) {
                    a.save_mean[c + e] = mu.v[e];
                    a.save_invstd[c + e] = (float)invstd;
                }
                update_running(a.running_mean + hc + c + e, a.running_var + hc + c + e, a.momentum, mean[e], m2[e], a.N);
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
    store_rows<FAST>(a.Y + hc, a.ldy, r0, nr, c, a.C, u);
}

// heads [blockIdx.z hpb, + hpb) of the strip; launch PART and every launch without dX have hpb == 1
template <bool FAST, int MODE>
__global__ __launch_bounds__(THREADS) void tile_bn_bwd(TileBnTrainArgs a, int hpb) {
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    __shared__ float4 bc[2][DW_LANES];
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    const int c = blockIdx.x * COLS + 4 * ln;
    const int h0 = blockIdx.z * hpb, h1 = min(a.H, h0 + hpb);
    const int HC = a.H * a.C;
    const int r0 = blockIdx.y * BN_TRAIN_ROWS;
    const int nr = MODE == APPLY && !a.dX ? 0 : min(BN_TRAIN_ROWS, a.N - r0);         // dgamma / dbeta alone: no row is read again
    float4 u[SLOTS], g[SLOTS], dx[SLOTS];
    load_rows<FAST>(a.X, a.ldx, r0, nr, c, a.C, u);
    load_rows<FAST>(a.dY + (size_t)h0 * a.C, a.lddy, r0, nr, c, a.C, g);
    const float4 mu = cols4(a.save_mean, c, a.C), is = cols4(a.save_invstd, c, a.C);
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        u[i] = grp + i * DW_GROUPS < nr ? mul4(sub4(u[i], mu), is) : zero4();          // xhat
        dx[i] = zero4();
    }

    for (int h = h0; h < h1; ++h) {
        const size_t hc = (size_t)h * a.C;
        float4 gn[SLOTS];                                                              // the next head's dY; zeros behind the last
        load_rows<FAST>(a.dY + hc + a.C, a.lddy, r0, h + 1 < h1 ? nr : 0, c, a.C, gn);
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
                    if (MODE == PART && c + e < a.C) {
                        a.part[(size_t)(2 * blockIdx.y) * HC + hc + c + e] = tot[0][e];
                        a.part[(size_t)(2 * blockIdx.y + 1) * HC + hc + c + e] = tot[1][e];
                    }
                }
            }
            if constexpr (MODE == PART) return;
        } else if (grp == 0) {
            const int chunks = (a.N + BN_TRAIN_ROWS - 1) / BN_TRAIN_ROWS;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e >= a.C) continue;
                for (int k = 0; k < chunks; ++k) {
                    tot[0][e] += a.part[(size_t)(2 * k) * HC + hc + c + e];
                    tot[1][e] += a.part[(size_t)(2 * k + 1) * HC + hc + c + e];
                }
            }
        }
        if (grp == 0) {
            f4a k1{}, k2{};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e >= a.C) continue;
                if (blockIdx.y == 0) {
                    if (a.dbeta) a.dbeta[hc + c + e] = (float)tot[0][e];
                    if (a.dgamma) a.dgamma[hc + c + e] = (float)tot[1][e];
                }
                k1.v[e] = (float)(tot[0][e] / a.N);
                k2.v[e] = (float)(tot[1][e] / a.N);
            }
            bc[0][ln] = vec(k1);
            bc[1][ln] = vec(k2);
        }
        if (!a.dX) return;                                                             // hpb == 1: the block's one head is done
        __syncthreads();
        const float4 k1 = bc[0][ln], k2 = bc[1][ln], w = mul4(cols4(a.gamma + hc, c, a.C), is);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            dx[i] = add4(dx[i], bn_du(g[i], u[i], w, k1, k2));
            g[i] = gn[i];
        }
        __syncthreads();                                                               // bc and sh are free for the next head
    }
    if (a.dX) store_rows<FAST>(a.dX, a.lddx, r0, nr, c, a.C, dx);
}

template <bool FWD, int MODE>
hipError_t launch(const TileBnTrainArgs& a, int row_blocks, int head_blocks, int hpb, hipStream_t st) {
    const dim3 grid((unsigned)((a.C + COLS - 1) / COLS), (unsigned)row_blocks, (unsigned)head_blocks), block(THREADS);
    if constexpr (FWD) {
        if (a.fast) hipLaunchKernelGGL((tile_bn_fwd<true, MODE>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((tile_bn_fwd<false, MODE>), grid, block, 0, st, a);
    } else {
        if (a.fast) hipLaunchKernelGGL((tile_bn_bwd<true, MODE>), grid, block, 0, st, a, hpb);
        else hipLaunchKernelGGL((tile_bn_bwd<false, MODE>), grid, block, 0, st, a, hpb);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tile_bn_train_forward(const TileBnTrainArgs& a, hipStream_t st) {
    const int row_blocks = (a.N + BN_TRAIN_ROWS - 1) / BN_TRAIN_ROWS;
    if (row_blocks == 1) return launch<true, WHOLE>(a, 1, a.H, 1, st);
    if (hipError_t e = launch<true, PART>(a, row_blocks, 1, 1, st)) return e;
    return launch<true, APPLY>(a, row_blocks, a.H, 1, st);
}

hipError_t launch_tile_bn_train_backward(const TileBnTrainArgs& a, hipStream_t st) {
    const int row_blocks = (a.N + BN_TRAIN_ROWS - 1) / BN_TRAIN_ROWS;
    const int head_blocks = a.dX ? 1 : a.H, hpb = a.dX ? a.H : 1;                      // dX sums the heads in one block, in order
    if (row_blocks == 1) return launch<false, WHOLE>(a, 1, head_blocks, hpb, st);
    if (hipError_t e = launch<false, PART>(a, row_blocks, a.H, 1, st)) return e;
    return launch<false, APPLY>(a, a.dX ? row_blocks : 1, head_blocks, hpb, st);
}

}  // namespace laff
