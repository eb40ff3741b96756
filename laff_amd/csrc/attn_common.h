// attn_common.h -- what the attention kernels share: fuse.hip (forward), fuse_bwd.hip and frame_bwd.hip (backward).  The backward
// kernels recompute the forward, so a helper that both directions call is the ONE definition of that step: the softmax below is the
// forward's and the backward's, and the fixed-order row sum is what makes two backward calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace laff {

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 scl4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 fma4(float4 a, float s, float4 c) {
    return make_float4(fmaf(a.x, s, c.x), fmaf(a.y, s, c.y), fmaf(a.z, s, c.z), fmaf(a.w, s, c.w));
}
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// a wave-uniform value as the scalar it is (the wave index: derived from threadIdx it looks divergent to the compiler)
__device__ __forceinline__ int pinned(int v) { return __builtin_amdgcn_readfirstlane(v); }

// 16 bytes past the cache: a plane or a gradient row that is read or written exactly once.  (fuse_bwd.hip applies the builtins to its
// scalar-base pointers itself, on f4 / v4: through these wrappers its <L, 2> kernels came out with other instructions.)
typedef float nt_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 f4(nt_f32x4 v) { return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ nt_f32x4 v4(float4 v) { return nt_f32x4{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ float4 load_nt(const nt_f32x4* p) { return f4(__builtin_nontemporal_load(p)); }
__device__ __forceinline__ void store_nt(nt_f32x4* p, float4 v) { __builtin_nontemporal_store(v4(v), p); }

// softmax over L logits held identically by every lane
template <int L>
__device__ __forceinline__ void softmax_L(float (&lg)[L]) {
    float m = lg[0];
#pragma unroll
    for (int l = 1; l < L; ++l) m = fmaxf(m, lg[l]);
    float s = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        lg[l] = expf(lg[l] - m);
        s += lg[l];
    }
    const float inv = 1.0f / s;
#pragma unroll
    for (int l = 0; l < L; ++l) lg[l] *= inv;
}

// dz_l = a_l (da_l - sum_k a_k da_k), in place of da
template <int L>
__device__ __forceinline__ void softmax_bwd_L(const float (&a)[L], float (&da)[L]) {
    float abar = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) abar = fmaf(a[l], da[l], abar);
#pragma unroll
    for (int l = 0; l < L; ++l) da[l] = a[l] * (da[l] - abar);
}

// The partial dw rows of one column added in a fixed order, by a 256-thread block that takes 32 columns (8 lanes x 16 bytes: one
// 128-byte line per partial row): the rows are cut into 32 interleaved groups, one per 8 lanes; each group adds its rows in row order
// and threads 0..7 add the 32 group sums in group order.  (One thread per column walking all rows was a chain of rows / 8 round trips
// on two to sixteen workgroups.)  `rows` points at the lane's four columns of the first row; a lane without columns passes rows = 0.
// The whole block calls this (it holds a barrier); the sum is returned in the threads of group 0.
// sum_rows_fixed_order_of is the same sum over rows that are formed on the way: row(r) gives the lane's four columns of row r.
constexpr int DW_GROUPS = 32, DW_LANES = 8;
template <class Row>
__device__ __forceinline__ float4 sum_rows_fixed_order_of(Row row, int nrows, float4 (&sh)[DW_GROUPS][DW_LANES]) {
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    float4 acc = zero4();
#pragma unroll 8
    for (int r = grp; r < nrows; r += DW_GROUPS) acc = add4(acc, row(r));
    sh[grp][ln] = acc;
    __syncthreads();
    float4 t = sh[0][ln];
    if (grp == 0) {
#pragma unroll
        for (int k = 1; k < DW_GROUPS; ++k) t = add4(t, sh[k][ln]);
    }
    return t;
}
__device__ __forceinline__ float4 sum_rows_fixed_order(const float* rows, int nrows, long pitch, float4 (&sh)[DW_GROUPS][DW_LANES]) {
    return sum_rows_fixed_order_of([=](int r) { return *(const float4*)(rows + (long)r * pitch); }, nrows, sh);
}

}  // namespace laff
