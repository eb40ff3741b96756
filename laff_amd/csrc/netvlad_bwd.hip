// netvlad_bwd.hip -- training the NetVLAD caption encoder (laff_netvlad_encode_train, laff_netvlad_backward): the
// gradients of fc1.weight and centeroids, both [K, D].  The word2vec table gets none (the reference feeds it rows without a graph).
//
// With the forward's names (netvlad.hip) and w_k = u_k / max(|u_k|, eps), v = flatten(w), o = v / max(|v|, eps), g = dL/do of a caption:
//   dv   = (g - o (o.g)) / |v|                    or g / eps where |v| was clamped
//   du_k = (dv_k - w_k (w_k.dv_k)) / |u_k|        or dv_k / eps where |u_k| was clamped          w_k = o_k max(|v|, eps)
//   d_centroids[k] = - sum_i s_ik du_ik           da_mk = xh_m.du_k - c_k.du_k                   dz_mk = a_mk (da_mk - sum_j a_mj da_mj)
//   d_fc1[k]       = sum_r dz_rk xh_r
// The saving forward is netvlad.hip's two launches with the assignments and 1 / max(|x|, eps) written into the reserve, and a pooling
// kernel that also stores the clamped norms and which of them were clamped: the backward never rebuilds u from the tokens.  (The
// pooling kernel is a copy: a body shared through a header changed the register allocation of the inference kernel.)
//
// The backward, three launches:
//   netvlad_bwd_caption_kernel   one workgroup (4 waves) per caption: o.g, then wave w forms du_k for k = w, w + 4, ... (a lane owns the
//                                columns d4 = lane, lane + 64, ...; the two dot products per cluster are wavefront reductions) into the
//                                workspace DU [N, K, D] and e_k = c_k.du_k; then the caption's xh rows go through LDS in chunks of
//                                VLAD_MC as in the forward, du_k comes back from DU (it need not fit on chip at any K, D), da, the
//                                softmax backward, dz -> workspace [R, K].  s_k -> workspace [N, K].
//   netvlad_bwd_partial_kernel   the sums over token rows (d_fc1) and over captions (d_centroids) of one chunk of rows / captions and
//                                one band of 256 columns: wave w owns the cluster quads w, w + 4, ..., a lane one column float4.
//   netvlad_bwd_reduce_kernel    the chunks' partial sums in ascending order; writes every element of the wanted outputs once.
// Chunk boundaries depend on (N, R) alone and every sum runs r / i ascending inside a chunk, chunks ascending: no atomics, the same
// bits from every run.
#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

typedef float vlad_f4 __attribute__((ext_vector_type(4)));

constexpr int VLAD_THREADS = 256;
constexpr int VLAD_MC = 8;                  // token rows per LDS chunk
constexpr float VLAD_EPS = 1e-12f;          // F.normalize's eps

__device__ __forceinline__ float dot4(vlad_f4 a, vlad_f4 b, float s) {
    s = fmaf(a.x, b.x, s);
    s = fmaf(a.y, b.y, s);
    s = fmaf(a.z, b.z, s);
    return fmaf(a.w, b.w, s);
}

// rows mb .. mb + mc of the batch as xh = x / max(|x|, eps) into xs [mc, D]; a row whose id is outside the table is NaN
__device__ __forceinline__ void vlad_stage_rows(const NetvladArgs& a, float* xs, int mb, int mc, int tid) {
    const int D = a.D, D4 = D >> 2;
    for (int idx = tid; idx < mc * D4; idx += VLAD_THREADS) {
        const int m = idx / D4, d4 = idx - m * D4;
        const int id = a.ids[mb + m];
        vlad_f4 x = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        if ((unsigned)id < (unsigned)a.V) x = reinterpret_cast<const vlad_f4*>(a.table + (long)id * D)[d4] * a.rnorm[mb + m];
        *reinterpret_cast<vlad_f4*>(xs + m * D + 4 * d4) = x;
    }
}
// ... and their assignment rows into as [mc, 64], zeros past K
__device__ __forceinline__ void vlad_stage_assign(const NetvladArgs& a, float* as, int mb, int mc, int tid) {
    const int K = a.K;
    for (int idx = tid; idx < mc * 64; idx += VLAD_THREADS) {
        const int m = idx >> 6, k = idx & 63;
        as[idx] = k < K ? a.assign[(long)(mb + m) * K + k] : 0.0f;
    }
}
// s_k = sum_m a_mk, m ascending; a caption of Z zero rows: Z / K (the softmax of a zero row is 1/K for every cluster)
__device__ __forceinline__ float vlad_cluster_mass(const NetvladArgs& a, int i, int b, int e, int k) {
    float s = 0.0f;
    for (int m = b; m < e; ++m) s += a.assign[(long)m * a.K + k];
    if (e == b) s = (float)a.zero_rows[i] * (1.0f / (float)a.K);
    return s;
}

// u of one (cluster quad, column float4) item over the chunk staged in LDS, on top of `u`
__device__ __forceinline__ void vlad_accumulate(vlad_f4 (&u)[4], const float* xs, const float* as, int mc, int D, int kq, int d4) {
    for (int m = 0; m < mc; ++m) {
        const vlad_f4 x = *reinterpret_cast<const vlad_f4*>(xs + m * D + 4 * d4);
        const vlad_f4 w = *reinterpret_cast<const vlad_f4*>(as + m * 64 + 4 * kq);
        u[0] += w.x * x;
        u[1] += w.y * x;
        u[2] += w.z * x;
        u[3] += w.w * x;
    }
}

// netvlad.hip's netvlad_vlad_kernel, operation for operation (the same bits in out), which also stores den [i, k] = max(|u_k|, eps),
// den [i, K] = max(|v|, eps) and clamped [i, .] = 1 where the norm was not above eps
__global__ __launch_bounds__(VLAD_THREADS) void netvlad_vlad_train_kernel(NetvladArgs a, float* save_den, int* save_clamped) {
    __shared__ __attribute__((aligned(16))) float xs[VLAD_MC * NETVLAD_MAX_D];
    __shared__ __attribute__((aligned(16))) float as[VLAD_MC * 64];
    __shared__ float s_sum[64], s_nrm2[64], s_scale[64];
    const int i = blockIdx.x;
    const int K = a.K, D = a.D, D4 = D >> 2, KQ = (K + 3) >> 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = a.row_off[i], e = a.row_off[i + 1], M = e - b;
    float* orow = a.out + (long)i * a.ldo;
    const int nch = M > 0 ? (M + VLAD_MC - 1) / VLAD_MC : 1;
    const int nd = (D4 + 63) >> 6;              // column float4s per lane, the same for every lane of the wave (wave_allsum)

    if (tid < K) s_sum[tid] = vlad_cluster_mass(a, i, b, e, tid);

    int mb = b, mc = 0;
    for (int ch = 0; ch < nch; ++ch) {
        mb = b + ch * VLAD_MC;
        mc = min(VLAD_MC, e - mb);
        if (ch) __syncthreads();                // the previous chunk is no longer read
        vlad_stage_rows(a, xs, mb, mc, tid);
        vlad_stage_assign(a, as, mb, mc, tid);
        __syncthreads();
        if (ch == nch - 1) break;               // the last chunk stays in LDS for both passes below
        for (int kq = wave; kq < KQ; kq += 4)
            for (int j = 0; j < nd; ++j) {
                const int d4 = lane + 64 * j;
                if (d4 >= D4) continue;
                vlad_f4 u[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = 4 * kq + c;
                    u[c] = ch && k < K ? *reinterpret_cast<const vlad_f4*>(orow + (long)k * D + 4 * d4) : vlad_f4{0.0f, 0.0f, 0.0f, 0.0f};
                }
                vlad_accumulate(u, xs, as, mc, D, kq, d4);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (4 * kq + c < K) *reinterpret_cast<vlad_f4*>(orow + (long)(4 * kq + c) * D + 4 * d4) = u[c];
            }
    }

    // the final u of an item: the partial sum of the earlier chunks, the last chunk, minus s_k c_k
    const bool carried = nch > 1;
    auto final_u = [&](vlad_f4 (&u)[4], int kq, int d4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 4 * kq + c;
            u[c] = carried && k < K ? *reinterpret_cast<const vlad_f4*>(orow + (long)k * D + 4 * d4) : vlad_f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        vlad_accumulate(u, xs, as, mc, D, kq, d4);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 4 * kq + c;
            if (k < K) u[c] -= s_sum[k] * reinterpret_cast<const vlad_f4*>(a.centroids + (long)k * D)[d4];
        }
    };

    for (int kq = wave; kq < KQ; kq += 4) {
        float sq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < nd; ++j) {
            const int d4 = lane + 64 * j;
            if (d4 >= D4) continue;
            vlad_f4 u[4];
            final_u(u, kq, d4);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sq[c] = fmaf(u[c].x, u[c].x, sq[c]);
                sq[c] = fmaf(u[c].y, u[c].y, sq[c]);
                sq[c] = fmaf(u[c].z, u[c].z, sq[c]);
                sq[c] = fmaf(u[c].w, u[c].w, sq[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float t = wave_allsum(sq[c]);
            if (lane == 0 && 4 * kq + c < K) s_nrm2[4 * kq + c] = t;
        }
    }
    __syncthreads();
    if (tid == 0) {
        // intra-normalisation scales, then the norm of the intra-normalised row: sum_k (|u_k| / max(|u_k|, eps))^2
        float* sd = save_den + (long)i * (K + 1);
        int* sc = save_clamped + (long)i * (K + 1);
        float g2 = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float n = sqrtf(s_nrm2[k]), den = fmaxf(n, VLAD_EPS);
            const float r = n / den;
            g2 = fmaf(r, r, g2);
            s_scale[k] = 1.0f / den;
            sd[k] = den;
            sc[k] = !(n > VLAD_EPS);
        }
        const float gn = sqrtf(g2), gden = fmaxf(gn, VLAD_EPS);
        const float ginv = 1.0f / gden;
        sd[K] = gden;
        sc[K] = !(gn > VLAD_EPS);
        for (int k = 0; k < K; ++k) s_scale[k] *= ginv;
    }
    __syncthreads();
    for (int kq = wave; kq < KQ; kq += 4)
        for (int j = 0; j < nd; ++j) {
            const int d4 = lane + 64 * j;
            if (d4 >= D4) continue;
            vlad_f4 u[4];
            final_u(u, kq, d4);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int k = 4 * kq + c;
                if (k < K) *reinterpret_cast<vlad_f4*>(orow + (long)k * D + 4 * d4) = u[c] * s_scale[k];
            }
        }
}

__global__ __launch_bounds__(VLAD_THREADS) void netvlad_bwd_caption_kernel(NetvladBwdArgs p) {
    __shared__ __attribute__((aligned(16))) float xs[VLAD_MC * NETVLAD_MAX_D];
    __shared__ float as[VLAD_MC * 64], s_da[VLAD_MC * 64];
    __shared__ float s_e[64], s_t[VLAD_MC], s_red[4];
    const NetvladArgs& a = p.f;
    const int i = blockIdx.x;
    const int K = a.K, D = a.D, D4 = D >> 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = a.row_off[i], e = a.row_off[i + 1], M = e - b;
    const vlad_f4* o4 = reinterpret_cast<const vlad_f4*>(a.out + (long)i * a.ldo);
    const vlad_f4* g4 = reinterpret_cast<const vlad_f4*>(p.g + (long)i * p.ldg);
    const vlad_f4* c4 = reinterpret_cast<const vlad_f4*>(a.centroids);
    const float* den = p.den + (long)i * (K + 1);
    const int* clamped = p.clamped + (long)i * (K + 1);
    vlad_f4* du4 = reinterpret_cast<vlad_f4*>(p.du + (long)i * K * D);
    const vlad_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

    if (tid < K) p.mass[(long)i * K + tid] = vlad_cluster_mass(a, i, b, e, tid);

    // o.g: a thread's float4s in ascending order, the butterfly, the four waves in order
    float og = 0.0f;
    for (int idx = tid; idx < K * D4; idx += VLAD_THREADS) og = dot4(o4[idx], g4[idx], og);
    og = wave_allsum(og);
    if (lane == 0) s_red[wave] = og;
    __syncthreads();
    og = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    const float den_v = den[K], rv = 1.0f / den_v;
    const bool clamped_v = clamped[K] != 0;

    // du_k and e_k = c_k.du_k, a cluster per wave at a time
    for (int k = wave; k < K; k += 4) {
        const bool clamped_u = clamped[k] != 0;
        const float ru = 1.0f / den[k];
        vlad_f4 dv[4], w[4];
        float t = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d4 = lane + 64 * j;
            dv[j] = w[j] = zero;
            if (d4 < D4) {
                const vlad_f4 o = o4[k * D4 + d4], g = g4[k * D4 + d4];
                dv[j] = (clamped_v ? g : g - o * og) * rv;
                w[j] = o * den_v;
                t = dot4(w[j], dv[j], t);
            }
        }
        t = wave_allsum(t);
        float ek = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d4 = lane + 64 * j;
            if (d4 < D4) {
                const vlad_f4 du = (clamped_u ? dv[j] : dv[j] - w[j] * t) * ru;
                du4[k * D4 + d4] = du;
                ek = dot4(c4[k * D4 + d4], du, ek);
            }
        }
        ek = wave_allsum(ek);
        if (lane == 0) s_e[k] = ek;
    }

    if (!p.d_fc1) return;                       // dz feeds d_fc1 alone
    // the caption's rows, VLAD_MC at a time: da_mk = xh_m.du_k - e_k, the softmax backward, dz
    const int nch = (M + VLAD_MC - 1) / VLAD_MC;
    for (int ch = 0; ch < nch; ++ch) {
        const int mb = b + ch * VLAD_MC, mc = min(VLAD_MC, e - mb);
        __syncthreads();                        // du and e_k are written / the previous chunk is no longer read
        vlad_stage_rows(a, xs, mb, mc, tid);
        vlad_stage_assign(a, as, mb, mc, tid);
        __syncthreads();
        for (int k = wave; k < K; k += 4) {
            vlad_f4 du[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d4 = lane + 64 * j;
                du[j] = d4 < D4 ? du4[k * D4 + d4] : zero;
            }
            const float ek = s_e[k];
            for (int m = 0; m < mc; ++m) {
                float t = 0.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int d4 = lane + 64 * j;
                    if (d4 < D4) t = dot4(*reinterpret_cast<const vlad_f4*>(xs + m * D + 4 * d4), du[j], t);
                }
                t = wave_allsum(t);
                if (lane == 0) s_da[m * 64 + k] = t - ek;
            }
        }
        __syncthreads();
        if (tid < mc) {
            float t = 0.0f;
            for (int k = 0; k < K; ++k) t = fmaf(as[tid * 64 + k], s_da[tid * 64 + k], t);
            s_t[tid] = t;
        }
        __syncthreads();
        for (int idx = tid; idx < mc * K; idx += VLAD_THREADS) {
            const int m = idx / K, k = idx - m * K;
            p.dz[(long)(mb + m) * K + k] = as[m * 64 + k] * (s_da[m * 64 + k] - s_t[m]);
        }
    }
}

// blockIdx.x: a band of 64 column float4s; blockIdx.y: the row chunks of d_fc1 (when wanted), then the caption chunks of d_centroids
__global__ __launch_bounds__(VLAD_THREADS) void netvlad_bwd_partial_kernel(NetvladBwdArgs p) {
    const NetvladArgs& a = p.f;
    const int K = a.K, D4 = a.D >> 2, KQ = (K + 3) >> 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int d4 = blockIdx.x * 64 + lane;
    if (d4 >= D4) return;
    const int nfc = p.d_fc1 ? p.chunks_r : 0;
    const bool cent = (int)blockIdx.y >= nfc;
    const int chunk = cent ? (int)blockIdx.y - nfc : (int)blockIdx.y;
    vlad_f4 acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[q][c] = vlad_f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (!cent) {
        const int r0 = chunk * p.rows_per_chunk, r1 = min(a.R, r0 + p.rows_per_chunk);
        for (int r = r0; r < r1; ++r) {
            const int id = a.ids[r];
            vlad_f4 x = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
            if ((unsigned)id < (unsigned)a.V) x = reinterpret_cast<const vlad_f4*>(a.table)[(long)id * D4 + d4] * a.rnorm[r];
            const float* z = p.dz + (long)r * K;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kq = wave + 4 * q;
                if (kq >= KQ) continue;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = 4 * kq + c;
                    if (k < K) acc[q][c] += z[k] * x;
                }
            }
        }
    } else {
        const int i0 = chunk * p.caps_per_chunk, i1 = min(a.N, i0 + p.caps_per_chunk);
        for (int i = i0; i < i1; ++i) {
            const float* s = p.mass + (long)i * K;
            const vlad_f4* du = reinterpret_cast<const vlad_f4*>(p.du) + (long)i * K * D4 + d4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kq = wave + 4 * q;
                if (kq >= KQ) continue;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = 4 * kq + c;
                    if (k < K) acc[q][c] -= s[k] * du[(long)k * D4];
                }
            }
        }
    }
    vlad_f4* out = reinterpret_cast<vlad_f4*>(cent ? p.part_cent : p.part_fc1) + (long)chunk * K * D4 + d4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int kq = wave + 4 * q;
        if (kq >= KQ) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 4 * kq + c;
            if (k < K) out[(long)k * D4] = acc[q][c];
        }
    }
}

// blockIdx.y = 0: d_fc1, 1: d_centroids; one float4 of [K, D] per thread, the chunks in ascending order (none: zeros)
__global__ __launch_bounds__(VLAD_THREADS) void netvlad_bwd_reduce_kernel(NetvladBwdArgs p) {
    const long n4 = (long)p.f.K * (p.f.D >> 2);
    const long idx = (long)blockIdx.x * VLAD_THREADS + threadIdx.x;
    float* dst = blockIdx.y ? p.d_cent : p.d_fc1;
    if (idx >= n4 || !dst) return;
    const vlad_f4* part = reinterpret_cast<const vlad_f4*>(blockIdx.y ? p.part_cent : p.part_fc1) + idx;
    const int nch = blockIdx.y ? p.chunks_n : p.chunks_r;
    vlad_f4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ch = 0; ch < nch; ++ch) s += part[(long)ch * n4];
    reinterpret_cast<vlad_f4*>(dst)[idx] = s;
}

hipError_t launch_netvlad_encode_train(const NetvladArgs& a, float* den, int* clamped, hipStream_t st) {
    if (a.R > 0)
        if (hipError_t e = launch_netvlad_assign(a, st); e != hipSuccess) return e;
    netvlad_vlad_train_kernel<<<a.N, VLAD_THREADS, 0, st>>>(a, den, clamped);
    return hipGetLastError();
}

hipError_t launch_netvlad_backward(const NetvladBwdArgs& p, hipStream_t st) {
    const NetvladArgs& a = p.f;
    const int D4 = a.D >> 2;
    if (a.N > 0) {
        netvlad_bwd_caption_kernel<<<a.N, VLAD_THREADS, 0, st>>>(p);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        const unsigned chunks = (unsigned)((p.d_fc1 ? p.chunks_r : 0) + (p.d_cent ? p.chunks_n : 0));
        if (chunks) {
            netvlad_bwd_partial_kernel<<<dim3((unsigned)((D4 + 63) / 64), chunks), VLAD_THREADS, 0, st>>>(p);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    netvlad_bwd_reduce_kernel<<<dim3((unsigned)(((long)a.K * D4 + VLAD_THREADS - 1) / VLAD_THREADS), 2), VLAD_THREADS, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace laff
