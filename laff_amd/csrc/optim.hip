// optim.hip -- the optimizer step for gfx950, fp32: the global L2 norm of a list of gradients (laff_grad_sqnorm), the clip that follows it
// (laff_grad_scale) and Adam / RMSprop with that clip folded in (laff_optim_step).  DESIGN.md 4.21.
//
// A tensor list is cut into chunks of OPTIM_CHUNK elements, each inside one tensor; a launch takes up to OPTIM_TABLE tensors, whose
// pointers, element counts and first chunks travel BY VALUE in the launch arguments (48 bytes an entry, 3.5 KiB of the 4 KiB there are):
// no device-side table, no copy, no allocation, nothing to synchronise -- a call is capturable.  The grid is min(chunks, OPTIM_GRID_CAP)
// blocks that stride over the chunks; a block walks the table forward as its chunk index grows (chunks ascend, so the walk is O(count) for
// the whole block), all of it wave-uniform scalar work.
//
// The norm is two-stage without atomics or a finishing block: every block of optim_sqnorm leaves ONE float64 partial at its own index
// (g * g of two fp32 values is exact in float64), and every block of a consumer (optim_scale, optim_update) sums ALL partials again, in
// index order: the block's first wavefront runs the chain ((part[0] + part[1]) + part[2]) + ... over partials it loads 64 at a time, one
// a lane, and hands the sum to the other three through LDS.  Every block of every launch forms the same bits of
//   total = sqrt(sum),  c = min(1, max_norm / (total + 1e-6))   (float64, c rounded to fp32 once; a NaN total gives a NaN c, as torch's clamp)
// and two calls give the same bits.  At most OPTIM_GRID_CAP partials per launch.
//
// Each kernel is built twice and the host picks per launch (the choice is between kernels, not a branch inside one: DESIGN.md 4.20):
// FAST when every base pointer of the launch is 16-byte aligned -- 16-byte loads and stores, a chunk being 4 of them a thread, and a
// scalar tail of fewer than 4 elements in a tensor's last chunk -- else single floats throughout.  Nothing stronger than 4-byte
// alignment is assumed of a tensor; a chunk starts OPTIM_CHUNK elements further, so it keeps its tensor's alignment.
//
// The update is fp32, one rounding per operation in torch's own order (foreach Adam / RMSprop, not capturable); contraction into FMAs is
// switched off for this file, sqrt and / are the correctly rounded ones (no fast-math).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_reduce.h"

#pragma clang fp contract(off)

namespace laff {

namespace {

constexpr int THREADS = 256;
constexpr int VECS = OPTIM_CHUNK / (4 * THREADS);       // 16-byte accesses per thread and full chunk
static_assert(OPTIM_CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of 16-byte accesses per thread");
static_assert(sizeof(OptimTable) + 128 + 256 <= 4096, "the table, the scalars beside it and the implicit arguments must fit 4 KiB");

// the block's sum of one double per thread, the same bits in every thread: butterfly inside a wave, then the waves in order
__device__ __forceinline__ double block_allsum(double v, double* sh) {
    v = wave_allsum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// lane l's value of v, in every lane (l is a constant after unrolling: two v_readlane_b32)
__device__ __forceinline__ double lane_value(double v, int l) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
    u = ((unsigned long long)hi << 32) | lo;
    __builtin_memcpy(&v, &u, 8);
    return v;
}

// Sum of the np partials in index order, ((part[0] + part[1]) + part[2]) + ..., the same bits in every thread.  The block's first
// wavefront (a wave-uniform branch) loads 64 partials at a time, one a lane, the next 64 already in flight, and adds them lane by lane;
// lanes past the end hold +0.0, which leaves a sum of squares as it is, NaN included.  The other wavefronts wait for the result in LDS.
__device__ __forceinline__ double partial_sum(const double* __restrict__ part, int np, double* sh) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        double s = 0.0;
        double x = lane < np ? part[lane] : 0.0;
        for (int base = 0; base < np; base += 64) {
            const int ahead = base + 64 + lane;
            const double nx = ahead < np ? part[ahead] : 0.0;
#pragma unroll
            for (int l = 0; l < 64; ++l) s += lane_value(x, l);
            x = nx;
        }
        if (lane == 0) sh[0] = s;
    }
    __syncthreads();
    return sh[0];
}

// torch.clamp(max_norm / (total + 1e-6), max=1.0): NaN stays NaN
__device__ __forceinline__ float clip_coef(double total, double max_norm) {
    const double r = max_norm / (total + 1e-6);
    return (float)(r > 1.0 ? 1.0 : r);
}

// the entry of chunk `ch`, found by walking on from the entry of the block's previous chunk
__device__ __forceinline__ const OptimEntry& entry_of(const OptimTable& tb, int& ti, long long ch) {
    while (ti + 1 < tb.count && tb.t[ti + 1].first <= ch) ++ti;
    return tb.t[ti];
}

template <bool FAST>
__global__ __launch_bounds__(THREADS) void optim_sqnorm(const OptimTable tb, double* __restrict__ part) {
    __shared__ double sh[4];
    double acc = 0.0;
    int ti = 0;
    for (long long ch = blockIdx.x; ch < tb.chunks; ch += gridDim.x) {
        const OptimEntry& e = entry_of(tb, ti, ch);
        const long long e0 = (ch - e.first) * OPTIM_CHUNK;
        const long long left = e.n - e0;
        const int len = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
        const float* __restrict__ g = e.g + e0;
        if constexpr (FAST) {
            const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
            if (len == OPTIM_CHUNK) {
                float4 x[VECS];
#pragma unroll
                for (int k = 0; k < VECS; ++k) x[k] = g4[threadIdx.x + k * THREADS];
#pragma unroll
                for (int k = 0; k < VECS; ++k)
                    acc += (double)x[k].x * x[k].x + (double)x[k].y * x[k].y + (double)x[k].z * x[k].z + (double)x[k].w * x[k].w;
            } else {
                const int nv = len >> 2;
                for (int v = threadIdx.x; v < nv; v += THREADS) {
                    const float4 x = g4[v];
                    acc += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
                }
                const int i = (nv << 2) + threadIdx.x;
                if (i < len) acc += (double)g[i] * g[i];
            }
        } else {
            for (int i = threadIdx.x; i < len; i += THREADS) acc += (double)g[i] * g[i];
        }
    }
    acc = block_allsum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

template <bool FAST>
__global__ __launch_bounds__(THREADS) void optim_scale(const OptimTable tb, const double* __restrict__ part, int np, double max_norm,
                                                       float* __restrict__ total_out) {
    __shared__ double sh[4];
    const double total = sqrt(partial_sum(part, np, sh));
    const float c = clip_coef(total, max_norm);
    if (total_out && blockIdx.x == 0 && threadIdx.x == 0) *total_out = (float)total;
    if (c == 1.0f) return;                               // 1 * g is g to the bit: nothing to store
    int ti = 0;
    for (long long ch = blockIdx.x; ch < tb.chunks; ch += gridDim.x) {
        const OptimEntry& e = entry_of(tb, ti, ch);
        const long long e0 = (ch - e.first) * OPTIM_CHUNK;
        const long long left = e.n - e0;
        const int len = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
        float* __restrict__ g = e.p + e0;                // the scaled tensor sits in the entry's writable slot
        if constexpr (FAST) {
            float4* __restrict__ g4 = reinterpret_cast<float4*>(g);
            if (len == OPTIM_CHUNK) {
                float4 x[VECS];
#pragma unroll
                for (int k = 0; k < VECS; ++k) x[k] = g4[threadIdx.x + k * THREADS];
#pragma unroll
                for (int k = 0; k < VECS; ++k) {
                    x[k].x = c * x[k].x; x[k].y = c * x[k].y; x[k].z = c * x[k].z; x[k].w = c * x[k].w;
                    g4[threadIdx.x + k * THREADS] = x[k];
                }
            } else {
                const int nv = len >> 2;
                for (int v = threadIdx.x; v < nv; v += THREADS) {
                    float4 x = g4[v];
                    x.x = c * x.x; x.y = c * x.y; x.z = c * x.z; x.w = c * x.w;
                    g4[v] = x;
                }
                const int i = (nv << 2) + threadIdx.x;
                if (i < len) g[i] = c * g[i];
            }
        } else {
            for (int i = threadIdx.x; i < len; i += THREADS) g[i] = c * g[i];
        }
    }
}

// one element of the step; s2 is Adam's second moment only
template <int KIND>
__device__ __forceinline__ void update_one(float& p, float g, float& s1, float& s2, const OptimScalars& h, float c, float step_size,
                                           float bc2_sqrt) {
    float gh = c * g;
    if (h.wd != 0.0f) gh = gh + h.wd * p;
    if constexpr (KIND == LAFF_OPT_ADAM) {
        const float m = s1 + (gh - s1) * h.omb1;
        const float v = h.b2 * s2 + (h.omb2 * gh) * gh;
        s1 = m;
        s2 = v;
        p = p - step_size * (m / (sqrtf(v) / bc2_sqrt + h.eps));
    } else {
        const float s = h.b2 * s1 + (h.omb2 * gh) * gh;
        s1 = s;
        p = p - h.lr * (gh / (sqrtf(s) + h.eps));
    }
}

template <int KIND>
__device__ __forceinline__ void update_vec(float4* __restrict__ p4, const float4* __restrict__ g4, float4* __restrict__ a4,
                                           float4* __restrict__ b4, int v, const OptimScalars& h, float c, float step_size, float bc2_sqrt) {
    float4 p = p4[v];
    const float4 g = g4[v];
    float4 a = a4[v];
    float4 b = KIND == LAFF_OPT_ADAM ? b4[v] : float4{0.f, 0.f, 0.f, 0.f};
    update_one<KIND>(p.x, g.x, a.x, b.x, h, c, step_size, bc2_sqrt);
    update_one<KIND>(p.y, g.y, a.y, b.y, h, c, step_size, bc2_sqrt);
    update_one<KIND>(p.z, g.z, a.z, b.z, h, c, step_size, bc2_sqrt);
    update_one<KIND>(p.w, g.w, a.w, b.w, h, c, step_size, bc2_sqrt);
    p4[v] = p;
    a4[v] = a;
    if constexpr (KIND == LAFF_OPT_ADAM) b4[v] = b;
}

template <int KIND, bool FAST>
__global__ __launch_bounds__(THREADS) void optim_update(const OptimTable tb, const OptimScalars h, const double* __restrict__ part, int np,
                                                        double max_norm, float* __restrict__ total_out) {
    __shared__ double sh[4];
    float c = 1.0f;
    if (max_norm > 0.0) {                                // uniform: a launch argument
        const double total = sqrt(partial_sum(part, np, sh));
        c = clip_coef(total, max_norm);
        if (total_out && blockIdx.x == 0 && threadIdx.x == 0) *total_out = (float)total;
    }
    const float step_size = h.lr / h.bc1, bc2_sqrt = sqrtf(h.bc2);
    int ti = 0;
    for (long long ch = blockIdx.x; ch < tb.chunks; ch += gridDim.x) {
        const OptimEntry& e = entry_of(tb, ti, ch);
        const long long e0 = (ch - e.first) * OPTIM_CHUNK;
        const long long left = e.n - e0;
        const int len = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
        float* __restrict__ p = e.p + e0;
        const float* __restrict__ g = e.g + e0;
        float* __restrict__ s1 = e.s1 + e0;
        float* __restrict__ s2 = KIND == LAFF_OPT_ADAM ? e.s2 + e0 : nullptr;
        const int nv = FAST ? len >> 2 : 0;
        if constexpr (FAST) {
            float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
            const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
            float4* __restrict__ a4 = reinterpret_cast<float4*>(s1);
            float4* __restrict__ b4 = reinterpret_cast<float4*>(s2);
            if (len == OPTIM_CHUNK) {
#pragma unroll
                for (int k = 0; k < VECS; ++k) update_vec<KIND>(p4, g4, a4, b4, threadIdx.x + k * THREADS, h, c, step_size, bc2_sqrt);
            } else {
                for (int v = threadIdx.x; v < nv; v += THREADS) update_vec<KIND>(p4, g4, a4, b4, v, h, c, step_size, bc2_sqrt);
            }
        }
        // FAST: the tail of fewer than 4 elements (none in a full chunk); else the whole chunk
        for (int i = (nv << 2) + threadIdx.x; i < len; i += THREADS) {
            float pv = p[i], a = s1[i], b = 0.0f;
            if constexpr (KIND == LAFF_OPT_ADAM) b = s2[i];
            update_one<KIND>(pv, g[i], a, b, h, c, step_size, bc2_sqrt);
            p[i] = pv;
            s1[i] = a;
            if constexpr (KIND == LAFF_OPT_ADAM) s2[i] = b;
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

long long chunks_of(long long n) { return (n + OPTIM_CHUNK - 1) / OPTIM_CHUNK; }

// Cuts the non-empty tensors of a list into launches of up to OPTIM_TABLE and hands each to `launch(table, fast, grid)`.
template <typename Launch>
hipError_t for_each_launch(const laff_optim_tensor* t, int count, OptimLaunches* done, Launch launch) {
    OptimTable tb{};
    bool fast = true;
    auto flush = [&]() -> hipError_t {
        if (tb.count == 0) return hipSuccess;
        const unsigned grid = (unsigned)(tb.chunks < OPTIM_GRID_CAP ? tb.chunks : OPTIM_GRID_CAP);
        launch(tb, fast, grid);
        ++(fast ? done->fast : done->generic);
        tb.count = 0;
        tb.chunks = 0;
        fast = true;
        return hipGetLastError();
    };
    for (int i = 0; i < count; ++i) {
        if (t[i].n == 0) continue;
        OptimEntry& e = tb.t[tb.count++];
        e.p = t[i].p; e.g = t[i].g; e.s1 = t[i].s1; e.s2 = t[i].s2; e.n = t[i].n; e.first = tb.chunks;
        tb.chunks += chunks_of(t[i].n);
        fast = fast && aligned16(e.p) && aligned16(e.g) && aligned16(e.s1) && aligned16(e.s2);
        if (tb.count == OPTIM_TABLE)
            if (hipError_t err = flush(); err != hipSuccess) return err;
    }
    return flush();
}

}  // namespace

void optim_plan(int count, const long long* n, OptimPlan* p) {
    long long chunks = 0;
    int in_table = 0;
    *p = OptimPlan{};
    auto flush = [&]() {
        if (!in_table) return;
        ++p->launches;
        p->partials += (int)(chunks < OPTIM_GRID_CAP ? chunks : OPTIM_GRID_CAP);
        chunks = 0;
        in_table = 0;
    };
    for (int i = 0; i < count; ++i) {
        if (n[i] == 0) continue;
        chunks += chunks_of(n[i]);
        if (++in_table == OPTIM_TABLE) flush();
    }
    flush();
}

hipError_t launch_optim_sqnorm(const laff_optim_tensor* t, int count, double* part, OptimLaunches* done, hipStream_t st) {
    double* seg = part;                                  // every launch writes its own segment of the partials
    return for_each_launch(t, count, done, [&](const OptimTable& tb, bool fast, unsigned grid) {
        if (fast) hipLaunchKernelGGL(optim_sqnorm<true>, dim3(grid), dim3(THREADS), 0, st, tb, seg);
        else hipLaunchKernelGGL(optim_sqnorm<false>, dim3(grid), dim3(THREADS), 0, st, tb, seg);
        seg += grid;
    });
}

hipError_t launch_optim_scale(const laff_optim_tensor* t, int count, double max_norm, const double* part, int np, float* total_out,
                              OptimLaunches* done, hipStream_t st) {
    float* out = total_out;                              // the first launch stores the norm
    hipError_t e = for_each_launch(t, count, done, [&](const OptimTable& tb, bool fast, unsigned grid) {
        if (fast) hipLaunchKernelGGL(optim_scale<true>, dim3(grid), dim3(THREADS), 0, st, tb, part, np, max_norm, out);
        else hipLaunchKernelGGL(optim_scale<false>, dim3(grid), dim3(THREADS), 0, st, tb, part, np, max_norm, out);
        out = nullptr;
    });
    if (e == hipSuccess && out) {                        // nothing to scale: one block over an empty table stores the norm
        hipLaunchKernelGGL(optim_scale<true>, dim3(1), dim3(THREADS), 0, st, OptimTable{}, part, np, max_norm, out);
        ++done->fast;
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_optim_update(const laff_optim_tensor* t, int count, int kind, const OptimScalars& h, double max_norm, const double* part,
                               int np, float* total_out, OptimLaunches* done, hipStream_t st) {
    float* out = total_out;
    return for_each_launch(t, count, done, [&](const OptimTable& tb, bool fast, unsigned grid) {
        const dim3 g(grid), b(THREADS);
        if (kind == LAFF_OPT_ADAM && fast)
            hipLaunchKernelGGL((optim_update<LAFF_OPT_ADAM, true>), g, b, 0, st, tb, h, part, np, max_norm, out);
        else if (kind == LAFF_OPT_ADAM)
            hipLaunchKernelGGL((optim_update<LAFF_OPT_ADAM, false>), g, b, 0, st, tb, h, part, np, max_norm, out);
        else if (fast)
            hipLaunchKernelGGL((optim_update<LAFF_OPT_RMSPROP, true>), g, b, 0, st, tb, h, part, np, max_norm, out);
        else
            hipLaunchKernelGGL((optim_update<LAFF_OPT_RMSPROP, false>), g, b, 0, st, tb, h, part, np, max_norm, out);
        out = nullptr;
    });
}

}  // namespace laff
