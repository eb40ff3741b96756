// expert_train.hip -- the expert stage of the LAFF towers in training mode (laff_expert_stage_train, laff_expert_stage_train_backward;
// model/model.py:1848-1873, :1653-1694 of the reference): the expert embedding added to each of the L projected planes of a tower and
// `l2norm(local_embs, dim=2)` after it, written as the stacked [N, L, D] tensor that the fusion reads in place.  One launch forwards,
// one launch backwards plus the small merge of the expert table's partial column sums.  fp32 throughout, 16-byte accesses, no atomics.
//
//   v = x_l[n, :] + expert[l, :]          r = 1 / (sqrt(sum v^2) + 1e-13 + 1e-14)          Y[n, l, :] = v r   (or v without l2norm)
//   s = |v|    dv = r g - v (r^2 / s) (v . g)   (second term 0 where s == 0; dv = g without l2norm)    dx_l = dv    d_expert[l] = sum_n dv
//
// Traffic (HBM): forward reads x once and writes Y once; backward reads x and dY once and writes dx once -- the second walk of a chunk
// of EXPERT_ROWS rows (the write pass after the row sums) finds its lines in L2.  The expert table is L D floats and stays cached.
#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ void st4(float* p, float4 v) { *(float4*)p = v; }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float dot4f(float4 a, float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float row_rnorm(float ss) { return 1.0f / (sqrtf(ss) + 1e-13f + 1e-14f); }

// one wavefront per (row, plane): the sum of squares first, then the scaled row
__global__ __launch_bounds__(256) void expert_stage_forward_kernel(ExpertStageArgs a) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (item >= (long)a.N * a.L) return;
    const long n = item / a.L;
    const int l = (int)(item - n * a.L);
    const float* x = a.x[l] + n * a.ldx[l];
    const float* e = a.expert ? a.expert + (long)l * a.lde : nullptr;
    float* y = a.Y + n * a.ldn + (long)l * a.ldl;
    float r = 1.0f;
    if (a.l2norm) {
        float ss = 0.f;
        for (int col = lane * 4; col < a.D; col += 256) {
            float4 v = ld4(x + col);
            if (e) v = add4(v, ld4(e + col));
            ss += dot4f(v, v);
        }
        ss = wave_allsum(ss);
        r = row_rnorm(ss);
        if (lane == 0) a.rnorm[(long)l * a.N + n] = r;
    }
    for (int col = lane * 4; col < a.D; col += 256) {
        float4 v = ld4(x + col);
        if (e) v = add4(v, ld4(e + col));
        if (a.l2norm) v = make_float4(v.x * r, v.y * r, v.z * r, v.w * r);
        st4(y + col, v);
    }
}

// one block per (chunk of EXPERT_ROWS rows, plane).  Pass A: a wavefront per row forms s^2 = sum v^2 and v . g and leaves the row's two
// factors in LDS.  Pass B: every thread owns columns t*4 + 1024 k, walks the chunk's rows in ascending order, writes dx and keeps the
// column sum of dv in registers: the block's partial of d_expert, stored to part[chunk][l][D].
__global__ __launch_bounds__(256) void expert_stage_backward_kernel(ExpertStageArgs a) {
    __shared__ float sh_r[EXPERT_ROWS], sh_c[EXPERT_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.x, l = blockIdx.y;
    const long n0 = (long)chunk * EXPERT_ROWS;
    const int rows = (int)((a.N - n0) < EXPERT_ROWS ? (a.N - n0) : EXPERT_ROWS);
    const float* e = a.expert ? a.expert + (long)l * a.lde : nullptr;
    if (a.l2norm) {
        for (int i = wave; i < rows; i += 4) {                            // wave-uniform
            const long n = n0 + i;
            const float* x = a.x[l] + n * a.ldx[l];
            const float* g = a.dY + n * a.ldn + (long)l * a.ldl;
            float ss = 0.f, vg = 0.f;
            for (int col = lane * 4; col < a.D; col += 256) {
                float4 v = ld4(x + col);
                if (e) v = add4(v, ld4(e + col));
                ss += dot4f(v, v);
                vg += dot4f(v, ld4(g + col));
            }
            ss = wave_allsum(ss);
            vg = wave_allsum(vg);
            if (lane == 0) {
                const float r = a.rnorm[(long)l * a.N + n], s = sqrtf(ss);
                sh_r[i] = r;
                sh_c[i] = s > 0.f ? r * (r * (vg / s)) : 0.f;          // (r r / s overflows for a tiny row; |vg / s| <= |g|)
            }
        }
        __syncthreads();
    }
    for (int col = threadIdx.x * 4; col < a.D; col += 1024) {
        const float4 ev = e ? ld4(e + col) : make_float4(0, 0, 0, 0);
        float4 acc = make_float4(0, 0, 0, 0);
        for (int i = 0; i < rows; ++i) {
            const long n = n0 + i;
            float4 dv = ld4(a.dY + n * a.ldn + (long)l * a.ldl + col);
            if (a.l2norm) {
                const float4 v = add4(ld4(a.x[l] + n * a.ldx[l] + col), ev);
                const float r = sh_r[i], c = sh_c[i];
                dv = make_float4(r * dv.x - v.x * c, r * dv.y - v.y * c, r * dv.z - v.z * c, r * dv.w - v.w * c);
            }
            st4(a.dx[l] + n * a.lddx[l] + col, dv);
            acc = add4(acc, dv);
        }
        if (a.part) st4(a.part + ((long)chunk * a.L + l) * a.D + col, acc);
    }
}

// d_expert[l, col] = the chunks' partials added in chunk order (zero chunks: zeros)
__global__ __launch_bounds__(256) void expert_stage_merge_kernel(const float* __restrict__ part, float* __restrict__ d_expert, int chunks,
                                                                 long LD) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= LD) return;
    float4 acc = make_float4(0, 0, 0, 0);
    for (int c = 0; c < chunks; ++c) acc = add4(acc, ld4(part + (long)c * LD + i));
    st4(d_expert + i, acc);
}

}  // namespace

void expert_stage_plan(int N, int L, int D, int* chunks, size_t* ws) {
    *chunks = (N + EXPERT_ROWS - 1) / EXPERT_ROWS;
    *ws = (size_t)*chunks * L * D * sizeof(float);
}

hipError_t launch_expert_stage_forward(const ExpertStageArgs& a, hipStream_t st) {
    const long items = (long)a.N * a.L;
    if (!items) return hipSuccess;
    hipLaunchKernelGGL(expert_stage_forward_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_expert_stage_backward(const ExpertStageArgs& a, hipStream_t st) {
    int chunks;
    size_t ws;
    expert_stage_plan(a.N, a.L, a.D, &chunks, &ws);
    if (chunks) {
        hipLaunchKernelGGL(expert_stage_backward_kernel, dim3((unsigned)chunks, (unsigned)a.L), dim3(256), 0, st, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (a.d_expert) {
        const long LD = (long)a.L * a.D;
        hipLaunchKernelGGL(expert_stage_merge_kernel, dim3((unsigned)((LD / 4 + 255) / 256)), dim3(256), 0, st, a.part, a.d_expert, chunks, LD);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace laff
