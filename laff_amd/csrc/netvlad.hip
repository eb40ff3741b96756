// netvlad.hip -- the NetVLAD caption encoder of the text tower, the inference forward (training: netvlad_bwd.hip)
// (reference model/model.py:529-549 NetVLADTxtEncoder over model/Attention.py:862-918 NetVLAD.forward).
//
// Per caption, over its M word2vec rows x_m (the distinct known words; or Z zero rows when no word is known):
//   xh_m = x_m / max(|x_m|, 1e-12)                 a_m = softmax_k(xh_m . fc1[k])          s_k = sum_m a_mk
//   u_k  = sum_m a_mk xh_m - s_k c_k               out = flatten_k(u_k / max(|u_k|, 1e-12)), then / max(|out|, 1e-12)
//
// Two launches:
//   netvlad_assign_kernel  one lane per token row: |x|, the K logits and the softmax -> workspace A [R, K] and 1/max(|x|, eps) [R].
//                          fc1 is read at wave-uniform addresses (scalar loads), so a wave streams it once for 64 tokens.
//   netvlad_vlad_kernel    one workgroup (4 waves) per caption.  The caption's tokens go through LDS in chunks of VLAD_MC rows
//                          (xh rows and their a rows).  Wave w owns the cluster quads kq = w, w + 4, ...; a lane owns the columns
//                          d4 = lane, lane + 64, ... (float4), so u of one (quad, d4) item is 16 registers and a quad's squared norms
//                          finish in a wavefront reduction (wave_reduce.h).  Chunks before the last accumulate through the caption's
//                          own output row (the lane reads back what it wrote).  The last chunk is applied twice: once for the
//                          cluster norms, once more to write the scaled row (same operations, same bits), so each row is written
//                          once with 16-byte stores and u never has to fit on chip whatever K, D and M are.
// Every sum runs in an order fixed by the caption alone (m ascending, d inside a lane ascending, the butterfly across lanes), so a
// caption's row is bitwise independent of the rest of its batch and of its position in it.
#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

typedef float vlad_f4 __attribute__((ext_vector_type(4)));

constexpr int VLAD_THREADS = 256;
constexpr int VLAD_MC = 8;                  // token rows per LDS chunk
constexpr float VLAD_EPS = 1e-12f;          // F.normalize's eps

template <int KT>
__global__ __launch_bounds__(256) void netvlad_assign_kernel(NetvladArgs a) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.R) return;
    const int K = a.K, D4 = a.D >> 2;
    const int id = a.ids[r];
    float* A = a.assign + r * K;
    if ((unsigned)id >= (unsigned)a.V) {        // an id outside the table poisons its caption instead of reading past it
        a.rnorm[r] = __builtin_nanf("");
        for (int k = 0; k < K; ++k) A[k] = __builtin_nanf("");
        return;
    }
    const vlad_f4* x = reinterpret_cast<const vlad_f4*>(a.table + (long)id * a.D);
    float ss = 0.0f;
    for (int d4 = 0; d4 < D4; ++d4) {
        const vlad_f4 v = x[d4];
        ss = fmaf(v.x, v.x, ss);
        ss = fmaf(v.y, v.y, ss);
        ss = fmaf(v.z, v.z, ss);
        ss = fmaf(v.w, v.w, ss);
    }
    const float inv = 1.0f / fmaxf(sqrtf(ss), VLAD_EPS);
    float acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0.0f;
    const vlad_f4* W = reinterpret_cast<const vlad_f4*>(a.fc1);
    constexpr int KB = KT < 32 ? KT : 32;       // clusters per sweep of the row: 64 would take more SGPRs than there are
#pragma unroll
    for (int h = 0; h < KT / KB; ++h)
        for (int d4 = 0; d4 < D4; ++d4) {
            const vlad_f4 v = x[d4] * inv;
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) {
                const int k = h * KB + kk;
                const vlad_f4 w = W[(long)(k < K ? k : 0) * D4 + d4];      // k >= K: a spare accumulator, never read
                acc[k] = fmaf(v.x, w.x, acc[k]);
                acc[k] = fmaf(v.y, w.y, acc[k]);
                acc[k] = fmaf(v.z, w.z, acc[k]);
                acc[k] = fmaf(v.w, w.w, acc[k]);
            }
        }
    float mx = acc[0];
#pragma unroll
    for (int k = 1; k < KT; ++k)
        if (k < K) mx = fmaxf(mx, acc[k]);
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        acc[k] = expf(acc[k] - mx);
        if (k < K) sum += acc[k];
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K) A[k] = acc[k] / sum;
    a.rnorm[r] = inv;
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

__global__ __launch_bounds__(VLAD_THREADS) void netvlad_vlad_kernel(NetvladArgs a) {
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

    if (tid < K) {
        float s = 0.0f;
        for (int m = b; m < e; ++m) s += a.assign[(long)m * K + tid];
        if (M == 0) s = (float)a.zero_rows[i] * (1.0f / (float)K);     // softmax of a zero row: 1/K for every cluster
        s_sum[tid] = s;
    }

    int mb = b, mc = 0;
    for (int ch = 0; ch < nch; ++ch) {
        mb = b + ch * VLAD_MC;
        mc = min(VLAD_MC, e - mb);
        if (ch) __syncthreads();                // the previous chunk is no longer read
        for (int idx = tid; idx < mc * D4; idx += VLAD_THREADS) {
            const int m = idx / D4, d4 = idx - m * D4;
            const int id = a.ids[mb + m];
            vlad_f4 x = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
            if ((unsigned)id < (unsigned)a.V) x = reinterpret_cast<const vlad_f4*>(a.table + (long)id * D)[d4] * a.rnorm[mb + m];
            *reinterpret_cast<vlad_f4*>(xs + m * D + 4 * d4) = x;
        }
        for (int idx = tid; idx < mc * 64; idx += VLAD_THREADS) {
            const int m = idx >> 6, k = idx & 63;
            as[idx] = k < K ? a.assign[(long)(mb + m) * K + k] : 0.0f;
        }
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
        float g2 = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float n = sqrtf(s_nrm2[k]), den = fmaxf(n, VLAD_EPS);
            const float r = n / den;
            g2 = fmaf(r, r, g2);
            s_scale[k] = 1.0f / den;
        }
        const float ginv = 1.0f / fmaxf(sqrtf(g2), VLAD_EPS);
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

// the soft assignments and 1 / max(|x|, eps) of the R > 0 token rows; the saving forward (netvlad_bwd.hip) starts with it as well
hipError_t launch_netvlad_assign(const NetvladArgs& a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.R + 255) / 256);
    if (a.K <= 8) netvlad_assign_kernel<8><<<blocks, 256, 0, st>>>(a);
    else if (a.K <= 16) netvlad_assign_kernel<16><<<blocks, 256, 0, st>>>(a);
    else if (a.K <= 32) netvlad_assign_kernel<32><<<blocks, 256, 0, st>>>(a);
    else netvlad_assign_kernel<64><<<blocks, 256, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_netvlad_encode(const NetvladArgs& a, hipStream_t st) {
    if (a.R > 0)
        if (hipError_t e = launch_netvlad_assign(a, st); e != hipSuccess) return e;
    netvlad_vlad_kernel<<<a.N, VLAD_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace laff
