// rerank.hip -- k-reciprocal re-ranking (model/ReRank.py: re_ranking, re_ranking_tkb_simple) for P independent problems per launch.
//
// A problem is one candidate set: the similarity blocks qq [Q,Q], qg [Q,G], gg [G,G] by pointer and pitch; N = Q + G items.  The
// concatenated N x N matrix is never formed: orig[j, i] = 2 - 2 x[j, i] is read from its block where it is needed, and
// D[i, j] = orig[j, i] / max_k orig[k, i] (column i of orig over its maximum, IEEE division) is recomputed from it.
//
//   rerank_rank     4 items per block, one wavefront each: column i of orig into an LDS slab (the 4 columns of a row are adjacent in
//                   memory, so the strided column read fetches each line once per block), its maximum, D[i, :], then k1+1 rounds of
//                   a wave-wide arg-min (ties: lower index) -> rank [N, k1+1], colmax [N]
//   rerank_expand   one wavefront per item: R(i, k1) by ballot over the k1+1 neighbours' lists, every R(c, kh) of its members with the
//                   2/3 overlap test, members marked in an N-byte LDS map whose in-order scan is the sorted, deduplicated expansion
//                   set; V[i, e] = exp(-D[i, e]) / sum  -> sparse rows idx1 / val1 [N, L1], cnt1 [N]
//   rerank_qe       one wavefront per item (k2 != 1): the rows rank[i][0..k2) of V added in that order into an N-float LDS row, / k2,
//                   scanned in order -> sparse rows idx2 / val2 [N, L2], cnt2 [N]
//   rerank_jaccard  per (query row, 64 gallery items): the query's sparse row scattered into an N-float LDS row; per gallery item
//                   m = sum min(V[i,k], V[j,k]) over the item's entries, 1 - m / (2 - m), blended with D[i, j]
//
// All arithmetic is fp32 with IEEE division and expf; sums run lane-strided + butterfly (wave_reduce.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

namespace {

constexpr int RR_WAVES = 4;               // items per block in the wave-per-item kernels
constexpr int RR_THREADS = 64 * RR_WAVES;
constexpr int RR_JAC_ITEMS = 64;          // gallery items per block of the Jaccard pass

// a lane's LDS stores made visible to the other lanes of its wavefront (the LDS is in order per wave; this pins the compiler)
__device__ __forceinline__ void rr_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned rr_lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// orig[j, i] = 2 - 2 x[j, i] of the block matrix [[qq, qg], [qg^T, gg]] (2 x is exact: one rounding, contracted or not)
__device__ __forceinline__ float rr_orig(const RerankProblem& p, int j, int i) {
    const int Q = p.Q;
    float x;
    if (i < Q) x = j < Q ? p.qq[(long)j * p.ldqq + i] : p.qg[(long)i * p.ldqg + (j - Q)];
    else x = j < Q ? p.qg[(long)j * p.ldqg + (i - Q)] : p.gg[(long)(j - Q) * p.ldgg + (i - Q)];
    return 2.0f - 2.0f * x;
}

// fp32 -> unsigned key of the same order
__device__ __forceinline__ unsigned rr_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(RR_THREADS) void rerank_rank_kernel(const RerankArgs a) {
    extern __shared__ float rr_slab[];                      // [RR_WAVES][N]
    const RerankProblem& p = a.p[blockIdx.y];
    const int N = p.Q + p.G, i0 = blockIdx.x * RR_WAVES;
    if (i0 >= N) return;
    for (int t = threadIdx.x; t < RR_WAVES * N; t += RR_THREADS) {
        const int c = t & (RR_WAVES - 1), j = t / RR_WAVES;
        if (i0 + c < N) rr_slab[c * N + j] = rr_orig(p, j, i0 + c);
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = i0 + w;
    if (i >= N) return;                                     // no block-wide barrier below
    float* col = rr_slab + w * N;
    float m = -INFINITY;
    for (int j = lane; j < N; j += 64) m = fmaxf(m, col[j]);
    m = wave_allmax(m);
    for (int j = lane; j < N; j += 64) col[j] = col[j] / m; // a lane only ever touches the elements j = lane (mod 64)
    const int K1 = a.k1 + 1;
    for (int r = 0; r < K1; ++r) {
        unsigned long long best = ~0ull;
        for (int j = lane; j < N; j += 64) {
            const unsigned long long k = ((unsigned long long)rr_key(col[j]) << 32) | (unsigned)j;
            best = k < best ? k : best;
        }
        best = wave_allmin(best);
        const int jb = (int)(unsigned)best;
        if ((jb & 63) == lane) col[jb] = INFINITY;          // taken (its owner is the only lane that reads it again)
        if (lane == 0) p.rank[(long)i * K1 + r] = jb;
    }
    if (lane == 0) p.colmax[i] = m;
}

// is `who` among the first n entries of item j's neighbour list?
__device__ __forceinline__ bool rr_lists(const int* rank, int K1, int j, int n, int who) {
    bool f = false;
    for (int t = 0; t < n; ++t) f |= rank[(long)j * K1 + t] == who;
    return f;
}

__global__ __launch_bounds__(RR_THREADS) void rerank_expand_kernel(const RerankArgs a) {
    __shared__ unsigned rr_mark[RR_WAVES][RERANK_MAX_N / 4];      // one byte per item
    __shared__ int rr_ri[RR_WAVES][64];
    __shared__ int rr_e[RR_WAVES][RERANK_MAX_CAP];
    const RerankProblem& p = a.p[blockIdx.y];
    const int N = p.Q + p.G, w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * RR_WAVES + w;
    if (i >= N) return;                                     // wave-uniform; the kernel has no block-wide barrier
    const int K1 = a.k1 + 1, KH = a.kh + 1;
    unsigned char* mark = reinterpret_cast<unsigned char*>(rr_mark[w]);
    for (int t = lane; t < (N + 3) / 4; t += 64) rr_mark[w][t] = 0u;
    // R(i, k1): the neighbours whose own list holds i
    int j = 0;
    bool in = false;
    if (lane < K1) {
        j = p.rank[(long)i * K1 + lane];
        in = rr_lists(p.rank, K1, j, K1, i);
    }
    const unsigned long long mi = __builtin_amdgcn_ballot_w64(in);
    const int nri = __popcll(mi);
    rr_wave_fence();                                        // the map is zero before it is marked
    if (in) {
        rr_ri[w][rr_lanes_below(mi)] = j;
        mark[j] = 1;
    }
    rr_wave_fence();
    // R(c, kh) of every member c, taken when more than 2/3 of it lies in R(i, k1)
    for (int ci = 0; ci < nri; ++ci) {
        const int c = rr_ri[w][ci];
        int jc = 0;
        bool inc = false, both = false;
        if (lane < KH) {
            jc = p.rank[(long)c * K1 + lane];
            inc = rr_lists(p.rank, K1, jc, KH, c);
            if (inc)
                for (int s = 0; s < nri; ++s) both |= rr_ri[w][s] == jc;
        }
        const int nc = __popcll(__builtin_amdgcn_ballot_w64(inc)), nb = __popcll(__builtin_amdgcn_ballot_w64(both));
        if (3 * nb > 2 * nc && inc) mark[jc] = 1;           // nb > 2/3 nc in integers (equal to the float test for all sizes here)
    }
    rr_wave_fence();
    // the marked items in index order = the sorted, deduplicated expansion set
    int cnt = 0;
    for (int base = 0; base < N; base += 64) {
        const int e = base + lane;
        const bool f = e < N && mark[e];
        const unsigned long long mf = __builtin_amdgcn_ballot_w64(f);
        if (f) rr_e[w][cnt + rr_lanes_below(mf)] = e;
        cnt += __popcll(mf);
    }
    rr_wave_fence();
    const float cm = p.colmax[i];
    float s = 0.0f;
    for (int t = lane; t < cnt; t += 64) s += expf(-(rr_orig(p, rr_e[w][t], i) / cm));
    s = wave_allsum(s);
    int* idx = p.idx1 + (long)i * p.L1;
    float* val = p.val1 + (long)i * p.L1;
    for (int t = lane; t < cnt; t += 64) {
        const int e = rr_e[w][t];
        idx[t] = e;
        val[t] = expf(-(rr_orig(p, e, i) / cm)) / s;
    }
    if (lane == 0) p.cnt1[i] = cnt;
}

__global__ __launch_bounds__(RR_THREADS) void rerank_qe_kernel(const RerankArgs a) {
    extern __shared__ float rr_slab[];                      // [RR_WAVES][N]
    const RerankProblem& p = a.p[blockIdx.y];
    const int N = p.Q + p.G, w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * RR_WAVES + w;
    if (i >= N) return;                                     // wave-uniform; no block-wide barrier
    float* acc = rr_slab + w * N;
    for (int t = lane; t < N; t += 64) acc[t] = 0.0f;
    const int K1 = a.k1 + 1;
    for (int r = 0; r < a.k2; ++r) {                        // rows in the order of the neighbour list, as the mean adds them
        rr_wave_fence();
        const int src = p.rank[(long)i * K1 + r], n = p.cnt1[src];
        const int* idx = p.idx1 + (long)src * p.L1;
        const float* val = p.val1 + (long)src * p.L1;
        for (int t = lane; t < n; t += 64) acc[idx[t]] += val[t];      // a row's indices are distinct
    }
    rr_wave_fence();
    const float k2 = (float)a.k2;
    int* oi = p.idx2 + (long)i * p.L2;
    float* ov = p.val2 + (long)i * p.L2;
    int cnt = 0;
    for (int base = 0; base < N; base += 64) {
        const int e = base + lane;
        const float v = e < N ? acc[e] : 0.0f;
        const bool f = v != 0.0f;
        const unsigned long long mf = __builtin_amdgcn_ballot_w64(f);
        if (f) {
            const int pos = cnt + rr_lanes_below(mf);
            oi[pos] = e;
            ov[pos] = v / k2;
        }
        cnt += __popcll(mf);
    }
    if (lane == 0) p.cnt2[i] = cnt;
}

__global__ __launch_bounds__(RR_THREADS) void rerank_jaccard_kernel(const RerankArgs a) {
    extern __shared__ float rr_slab[];                      // [N]: the query's row of V, dense
    const RerankProblem& p = a.p[blockIdx.z];
    const int Q = p.Q, N = Q + p.G, i = blockIdx.y, g0 = blockIdx.x * RR_JAC_ITEMS;
    if (i >= Q || g0 >= p.G) return;                        // block-uniform
    for (int t = threadIdx.x; t < N; t += RR_THREADS) rr_slab[t] = 0.0f;
    __syncthreads();
    {
        const int n = p.cnt2[i];
        const int* idx = p.idx2 + (long)i * p.L2;
        const float* val = p.val2 + (long)i * p.L2;
        for (int t = threadIdx.x; t < n; t += RR_THREADS) rr_slab[idx[t]] = val[t];
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float cm = p.colmax[i], wj = 1.0f - a.lambda, wd = a.lambda;
    for (int g = g0 + w; g < min(g0 + RR_JAC_ITEMS, p.G); g += RR_WAVES) {
        const int j = Q + g, n = p.cnt2[j];
        const int* idx = p.idx2 + (long)j * p.L2;
        const float* val = p.val2 + (long)j * p.L2;
        float m = 0.0f;
        for (int t = lane; t < n; t += 64) m += fminf(rr_slab[idx[t]], val[t]);
        m = wave_allsum(m);
        if (lane == 0) {
            const float jac = 1.0f - m / (2.0f - m);
            p.out[(long)i * p.ldo + g] = jac * wj + (rr_orig(p, j, i) / cm) * wd;
        }
    }
}

// ---- re_ranking_tkb_simple: count[v] = 1 + #{u : v among the k1 best of gg[u]}; out[q, c] = log(count[c] + 1) on q's topK columns
__global__ void rerank_tkb_init_kernel(int* count, int G, float* out, int Q, long ldo) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < G) count[t] = 1;
    if (t < (long)Q * G) out[(t / G) * ldo + t % G] = 0.0f;
}

__global__ void rerank_tkb_hist_kernel(const int* nn, long n, int G, int* count) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int v = nn[t];
    if (v >= 0 && v < G) atomicAdd(count + v, 1);
}

__global__ void rerank_tkb_scatter_kernel(const int* cand, int Q, int K, int G, const int* count, float* out, long ldo) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)Q * K) return;
    const int c = cand[t];
    if (c >= 0 && c < G) out[(t / K) * ldo + c] = logf((float)(count[c] + 1));
}

}  // namespace

size_t rerank_lds_bytes(int maxN) { return (size_t)RR_WAVES * maxN * sizeof(float); }

hipError_t launch_rerank(const RerankArgs& a, int maxQ, int maxG, int maxN, hipStream_t st) {
    const dim3 items((maxN + RR_WAVES - 1) / RR_WAVES, a.count);
    const size_t slab = rerank_lds_bytes(maxN);
    hipLaunchKernelGGL(rerank_rank_kernel, items, dim3(RR_THREADS), slab, st, a);
    hipLaunchKernelGGL(rerank_expand_kernel, items, dim3(RR_THREADS), 0, st, a);
    if (a.k2 != 1) hipLaunchKernelGGL(rerank_qe_kernel, items, dim3(RR_THREADS), slab, st, a);
    hipLaunchKernelGGL(rerank_jaccard_kernel, dim3((maxG + RR_JAC_ITEMS - 1) / RR_JAC_ITEMS, maxQ, a.count), dim3(RR_THREADS),
                       (size_t)maxN * sizeof(float), st, a);
    return hipGetLastError();
}

hipError_t launch_rerank_tkb(const int* nn, int G, int k1, const int* cand, int Q, int K, int* count, float* out, long ldo,
                             hipStream_t st) {
    const long cells = std::max((long)Q * G, (long)G), n = (long)G * k1, qk = (long)Q * K;
    hipLaunchKernelGGL(rerank_tkb_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, count, G, out, Q, ldo);
    hipLaunchKernelGGL(rerank_tkb_hist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, nn, n, G, count);
    if (qk) hipLaunchKernelGGL(rerank_tkb_scatter_kernel, dim3((unsigned)((qk + 255) / 256)), dim3(256), 0, st, cand, Q, K, G, count, out, ldo);
    return hipGetLastError();
}

}  // namespace laff
