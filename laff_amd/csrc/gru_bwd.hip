// gru_bwd.hip -- backpropagation through time for the GRU caption encoder (laff_gru_backward).
//
// The saving forward step (gru.hip, SAVE) left, per direction and per active (step t, row), at the packed position
// pos(t, row) = off[t] + row (off = prefix sum of batch_sizes; M = sum of batch_sizes rows in all) of the reserve:
//   r, z, n, q = W_hn h_prev + b_hn, h_prev                 five planes of [M, H]
// One launch per time step walks the recurrence backwards (t descending for the forward direction, ascending for the reverse one, both
// in the same launch, grid.z).  Step t:
//   dh_rec[row, u] = sum_{k < 3H} dGH_nb[row, k] W_hh[k, u]   on v_mfma_f32_16x16x4_f32, over the rows that the consuming step (t + 1
//                                                             forward, t - 1 reverse) had as well -- a prefix; 0 for the others
//   dh   = (dh_rec + carry[row]) + pool                       pool: dout / len at every step (mean), dout at the row's last step (last)
//   da_n = dh (1 - z) (1 - n^2)    da_z = dh (h_prev - n) z (1 - z)    da_r = da_n q r (1 - r)
//   dGI[pos] = (da_r, da_z, da_n)  dGH[pos] = (da_r, da_z, da_n r)     carry[row] = dh z
// dGI and dGH are row-major [M, 3H], so that the weight gradients are plain GEMMs afterwards (laff_fc_backward's launch path):
// dW_hh = dGH^T H_prev, dW_ih = dGI^T X, dX = dGI W_ih.  The launch boundary orders the steps; no workgroup talks to another and there
// are no float atomics: carry[row, u] is read and written by the one thread that owns the element.
//
// A workgroup (4 waves) owns 16*RT rows x 16*UT hidden units.  The K = 3H sum is split over the 4 waves by 16-wide chunks (wave w: chunks
// [w*nk/4, (w+1)*nk/4), nk = 3H/16) and the partials are added in LDS as (p0 + p2) + (p1 + p3), as gru.hip does: the split and every
// MFMA's k order depend on H only, so every output is the same bits whichever tile a step picks.
//
// Operands: dGH_nb is read where it lies (lane l: 16 bytes of row l&15 at column 16*kc + 4*(l>>4)); W_hh comes in the transposed pack
//   WpT[ut][kc][lane][j] = W_hh[16*kc + 4*(lane>>4) + j][16*ut + (lane&15)]                                  (laff_gru_pack_whh_t)
// MFMA j of chunk kc takes component j of both: lane group G = lane>>4 supplies k = 16*kc + 4*G + j.
#include <algorithm>

#include "kernels.h"

namespace laff {

typedef float grub_f4 __attribute__((ext_vector_type(4)));

constexpr int GRUB_THREADS = 256;

__global__ __launch_bounds__(256) void gru_pack_whh_t_kernel(const float* __restrict__ W, int H, float* __restrict__ Wp) {
    const int nk = 3 * (H >> 4);
    const long total = 3L * H * H;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const int j = (int)(o & 3), lane = (int)((o >> 2) & 63);
        const long q = o >> 8;
        const int kc = (int)(q % nk), ut = (int)(q / nk);
        Wp[o] = W[(long)(16 * kc + 4 * (lane >> 4) + j) * H + 16 * ut + (lane & 15)];
    }
}

template <int RT, int UT>
__global__ __launch_bounds__(GRUB_THREADS) void gru_bwd_step_kernel(GruBwdStepArgs s) {
    const GruBwdDirArgs D = blockIdx.z ? s.d1 : s.d0;
    const int row0 = blockIdx.y * 16 * RT;
    if (row0 >= D.B) return;
    const int H = s.H, H3 = 3 * H, nk = H3 >> 4;
    const int u0 = blockIdx.x * 16 * UT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NA = RT * UT;                     // accumulators per wave: (row tile, unit tile)
    __shared__ grub_f4 red[2][NA][64];

    grub_f4 acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = grub_f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (row0 < D.Bnb) {                             // uniform over the workgroup; a tile past the prefix keeps dh_rec = 0
        const float* A = D.dgh_nb + (long)(row0 + (lane & 15)) * H3 + 4 * (lane >> 4);
        const grub_f4* W = reinterpret_cast<const grub_f4*>(D.WpT) + (long)(u0 >> 4) * nk * 64 + lane;
        bool live[RT];                              // rows past the prefix are not read: they belong to another step or lie past M
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) live[rt] = row0 + 16 * rt + (lane & 15) < D.Bnb;
        const int kb = wave * nk / 4, ke = (wave + 1) * nk / 4;
        for (int kc = kb; kc < ke; ++kc) {
            grub_f4 a[RT], b[UT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                a[rt] = grub_f4{0.0f, 0.0f, 0.0f, 0.0f};
                if (live[rt]) a[rt] = *reinterpret_cast<const grub_f4*>(A + (long)rt * 16 * H3 + 16 * kc);
            }
#pragma unroll
            for (int ut = 0; ut < UT; ++ut) b[ut] = W[((long)ut * nk + kc) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ut = 0; ut < UT; ++ut)
                        acc[rt * UT + ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][j], b[ut][j], acc[rt * UT + ut], 0, 0, 0);
        }
    }
    // fixed-order reduction of the 4 K-slices: (p0 + p2) + (p1 + p3); the total ends in red[0]
    if (wave >= 2)
#pragma unroll
        for (int a = 0; a < NA; ++a) red[wave - 2][a][lane] = acc[a];
    __syncthreads();
    if (wave < 2)
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[a] += red[wave][a][lane];
    __syncthreads();
    if (wave == 1)
#pragma unroll
        for (int a = 0; a < NA; ++a) red[0][a][lane] = acc[a];
    __syncthreads();
    if (wave == 0)
#pragma unroll
        for (int a = 0; a < NA; ++a) red[0][a][lane] = acc[a] + red[0][a][lane];
    __syncthreads();

    // gate epilogue: consecutive threads take consecutive hidden units of one row
    const float* red0 = reinterpret_cast<const float*>(&red[0][0][0]);
    const long plane = (long)s.M * H;
    for (int e = threadIdx.x; e < 256 * RT * UT; e += GRUB_THREADS) {
        const int uu = e % (16 * UT), i = e / (16 * UT);
        const int row = row0 + i;
        if (row >= D.B) break;                      // e grows with i: every later element of this thread is past B too
        const int u = u0 + uu;
        const int cl = (uu & 15) + 16 * ((i & 15) >> 2), reg = i & 3;    // C/D map of 16x16x4: col = lane&15, row = 4*(lane>>4)+reg
        const int a0 = (i >> 4) * UT + (uu >> 4);
        const float* rs = D.res + ((long)D.off + row) * H + u;
        const float r = rs[0], z = rs[plane], n = rs[2 * plane], q = rs[3 * plane], hp = rs[4 * plane];
        float* cp = D.carry + (long)row * H + u;
        const int len = s.lens[row];
        const int orow = s.perm[row];
        float pool = 0.0f;
        if ((unsigned)orow < (unsigned)s.N) {
            const float* g = s.dout + (long)orow * s.lddo;
            if (s.pooling == LAFF_GRU_MEAN) pool = g[D.col0 + u] / (float)len;
            else if (s.pooling == LAFF_GRU_LAST) pool = D.t == len - 1 ? g[u] : 0.0f;
            else pool = g[u] / (float)len + (D.t == len - 1 ? g[H + u] : 0.0f);
        }
        const float dh = (red0[(a0 * 64 + cl) * 4 + reg] + *cp) + pool;
        const float da_n = dh * (1.0f - z) * (1.0f - n * n);
        const float da_z = dh * (hp - n) * z * (1.0f - z);
        const float da_r = da_n * q * r * (1.0f - r);
        float* gi = D.dgi + (long)row * H3 + u;
        float* gh = D.dgh + (long)row * H3 + u;
        gi[0] = da_r;
        gi[H] = da_z;
        gi[2 * H] = da_n;
        gh[0] = da_r;
        gh[H] = da_z;
        gh[2 * H] = da_n * r;
        *cp = dh * z;
    }
}

__global__ __launch_bounds__(256) void gru_gather_rows_kernel(const float* __restrict__ table, int V, int D, const int* __restrict__ ids,
                                                              int M, float* __restrict__ X) {
    const long total = (long)M * D;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const int m = (int)(o / D), c = (int)(o % D);
        const int id = ids[m];
        X[o] = (unsigned)id < (unsigned)V ? table[(long)id * D + c] : __builtin_nanf("");
    }
}

// one workgroup per distinct token: its positions in ascending order, forward direction's row before the reverse one's
__global__ __launch_bounds__(256) void gru_embed_grad_kernel(const float* __restrict__ dX0, const float* __restrict__ dX1, int M, int D,
                                                             const int* __restrict__ seg_off, const int* __restrict__ seg_tok,
                                                             const int* __restrict__ seg_pos, int V, float* __restrict__ d_we) {
    const int seg = blockIdx.x;
    const int tok = seg_tok[seg];
    if ((unsigned)tok >= (unsigned)V) return;
    const int pb = max(seg_off[seg], 0), pe = min(seg_off[seg + 1], M);      // seg_pos has M entries
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float sum = 0.0f;
        for (int p = pb; p < pe; ++p) {
            const int pos = seg_pos[p];
            if ((unsigned)pos >= (unsigned)M) continue;
            float v = dX0[(long)pos * D + c];
            if (dX1) v += dX1[(long)pos * D + c];
            sum += v;
        }
        d_we[(long)tok * D + c] = sum;
    }
}

hipError_t launch_gru_pack_whh_t(const float* W, int H, float* Wp, hipStream_t st) {
    const long total = 3L * H * H;
    const int blocks = (int)std::min<long>((total + 255) / 256, 8192);
    gru_pack_whh_t_kernel<<<blocks, 256, 0, st>>>(W, H, Wp);
    return hipGetLastError();
}

hipError_t launch_gru_bwd_step(const GruBwdStepArgs& s, int ndirs, hipStream_t st) {
    const int B = std::max(s.d0.B, ndirs > 1 ? s.d1.B : 0);
    if (gru_step_big(B, s.H, ndirs)) {
        dim3 grid(s.H / 32, (B + 63) / 64, ndirs);
        gru_bwd_step_kernel<4, 2><<<grid, GRUB_THREADS, 0, st>>>(s);
    } else {
        dim3 grid(s.H / 16, (B + 15) / 16, ndirs);
        gru_bwd_step_kernel<1, 1><<<grid, GRUB_THREADS, 0, st>>>(s);
    }
    return hipGetLastError();
}

hipError_t launch_gru_gather_rows(const float* table, int V, int D, const int* ids, int M, float* X, hipStream_t st) {
    const long total = (long)M * D;
    if (total == 0) return hipSuccess;
    const int blocks = (int)std::min<long>((total + 255) / 256, 8192);
    gru_gather_rows_kernel<<<blocks, 256, 0, st>>>(table, V, D, ids, M, X);
    return hipGetLastError();
}

hipError_t launch_gru_embed_grad(const float* dX0, const float* dX1, int M, int D, const int* seg_off, const int* seg_tok,
                                 const int* seg_pos, int U, int V, float* d_we, hipStream_t st) {
    if (U == 0) return hipSuccess;
    gru_embed_grad_kernel<<<U, 256, 0, st>>>(dX0, dX1, M, D, seg_off, seg_tok, seg_pos, V, d_we);
    return hipGetLastError();
}

}  // namespace laff
