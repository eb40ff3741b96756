// bn_train_common.h -- what the training-mode BatchNorm kernels share (bn_train.hip, tile_bn_train.hip): the strip a block of 256
// threads keeps in registers (32 columns x a chunk of BN_TRAIN_ROWS rows, 32 interleaved row groups of 8 rows each), its accesses, and
// the per-column arithmetic behind the column sums in its one fixed order.  tile_bn_train.hip promises the bits of bn_train.hip on the
// materialised input: the promise holds because both run the functions of this file.
#pragma once
#include <hip/hip_runtime.h>

#include "attn_common.h"
#include "kernels.h"

namespace laff {
namespace bn_strip {

constexpr int THREADS = DW_GROUPS * DW_LANES, COLS = 4 * DW_LANES, SLOTS = BN_TRAIN_ROWS / DW_GROUPS;
enum { WHOLE = 0, PART = 1, APPLY = 2 };         // the one launch of an uncut shape; the two of a cut one

struct f4a { float v[4]; };
__device__ __forceinline__ f4a arr(float4 t) { return f4a{{t.x, t.y, t.z, t.w}}; }
__device__ __forceinline__ float4 vec(const f4a& t) { return make_float4(t.v[0], t.v[1], t.v[2], t.v[3]); }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// columns [c, c + 4) of a row of D floats; FAST: one 16-byte access, else element by element and nothing past the row's end
template <bool FAST>
__device__ __forceinline__ float4 load4(const float* row, int c, int D) {
    if constexpr (FAST) {
        return *reinterpret_cast<const float4*>(row + c);
    } else {
        f4a v{};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < D) v.v[e] = row[c + e];
        return vec(v);
    }
}
template <bool FAST>
__device__ __forceinline__ void store4(float* row, int c, int D, float4 t) {
    if constexpr (FAST) {
        *reinterpret_cast<float4*>(row + c) = t;
    } else {
        const f4a v = arr(t);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < D) row[c + e] = v.v[e];
    }
}
// the lane's four entries of a per-column vector, zeros past D (4-byte accesses: a [D] vector promises no more)
__device__ __forceinline__ float4 cols4(const float* v, int c, int D) { return load4<false>(v, c, D); }

// the column sums of the block's chunk from each thread's own sum: the 32 group sums in group order, in the threads of group 0
__device__ __forceinline__ float4 sum_groups(float4 own, float4 (&sh)[DW_GROUPS][DW_LANES]) {
    return sum_rows_fixed_order_of([=](int) { return own; }, DW_GROUPS, sh);
}

// (mean, M2) of the nr rows of the strip u (slot i is row grp + 32 i; slots without a row hold zeros), the corrected two-pass form:
// mean0 = sum / nr in fp32, then d = u - mean0, S1 = sum d, S2 = sum d^2, and in float64 mean = mean0 + S1 / nr, M2 = S2 - S1^2 / nr.
// Valid in the threads of group 0.  bc0 is a broadcast row of the block; every thread of the block calls this.
__device__ __forceinline__ void strip_mean_m2(const float4 (&u)[SLOTS], int nr, float4 (&sh)[DW_GROUPS][DW_LANES], float4 (&bc0)[DW_LANES],
                                              double (&mean)[4], double (&m2)[4]) {
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    float4 own = zero4();
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) own = add4(own, u[i]);
    const float4 s = sum_groups(own, sh);
    if (grp == 0) bc0[ln] = scl4(s, 1.0f / (float)nr);
    __syncthreads();
    const float4 mean0 = bc0[ln];
    float4 own1 = zero4(), own2 = zero4();
#pragma unroll
    for (int i = 0; i < SLOTS; ++i)
        if (grp + i * DW_GROUPS < nr) {
            const float4 d = sub4(u[i], mean0);
            own1 = add4(own1, d);
            own2 = add4(own2, mul4(d, d));
        }
    const float4 s1 = sum_groups(own1, sh);
    __syncthreads();
    const float4 s2 = sum_groups(own2, sh);
    if (grp == 0) {
        const f4a m0 = arr(mean0), t1 = arr(s1), t2 = arr(s2);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mean[e] = (double)m0.v[e] + (double)t1.v[e] / nr;
            m2[e] = fmax(0.0, (double)t2.v[e] - (double)t1.v[e] * (double)t1.v[e] / nr);
        }
    }
}

// the chunks' (mean, M2) of column col, part[chunk][2][D], merged in chunk order (Chan's update) onto mean = m2 = 0
__device__ __forceinline__ void merge_mean_m2(const double* part, int D, int N, int col, double& mean, double& m2) {
    const int chunks = (N + BN_TRAIN_ROWS - 1) / BN_TRAIN_ROWS;
    double n = 0.0;
    for (int k = 0; k < chunks; ++k) {
        const double nk = (double)min(BN_TRAIN_ROWS, N - k * BN_TRAIN_ROWS), tot = n + nk;
        const double mk = part[(size_t)(2 * k) * D + col], delta = mk - mean;
        mean += delta * (nk / tot);
        m2 += part[(size_t)(2 * k + 1) * D + col] + delta * delta * (n * nk / tot);
        n = tot;
    }
}

// one channel's running statistics after a batch of N rows with (mean, M2)
__device__ __forceinline__ void update_running(float* running_mean, float* running_var, double momentum, double mean, double m2, int N) {
    *running_mean = (float)((1.0 - momentum) * *running_mean + momentum * mean);
    *running_var = (float)((1.0 - momentum) * *running_var + momentum * (m2 / (N - 1)));
}

// the thread's (sum dY, sum dY xhat) over its slots of a chunk: g and xhat hold zeros in slots without a row
__device__ __forceinline__ void strip_dot(const float4 (&g)[SLOTS], const float4 (&xhat)[SLOTS], float4& own1, float4& own2) {
    own1 = zero4();
    own2 = zero4();
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        own1 = add4(own1, g[i]);
        own2 = add4(own2, mul4(g[i], xhat[i]));
    }
}

// dU = w (dY - k1 - xhat k2) with w = gamma invstd, k1 = dbeta / N, k2 = dgamma / N
__device__ __forceinline__ float4 bn_du(float4 g, float4 xhat, float4 w, float4 k1, float4 k2) {
    return mul4(w, sub4(sub4(g, k1), mul4(xhat, k2)));
}

}  // namespace bn_strip
}  // namespace laff
