// selfattn_fuse.hip -- the multi-head self-attention fusion block (Multi_head_MyApply_selfAttention of the reference) for gfx950, forward
// and backward: laff_selfattn_fuse, laff_selfattn_fuse_backward.  fp32.  DESIGN.md section 4.31.
//
// Per group (row n, head h), over the head's d columns of the L planes x_l:
//   tokens   u_0 = max_l x_l | mean_l x_l  [PRE: a prepended token]     u_{PRE + l} = x_l           T = L + PRE
//   t_i = u_i / (rho_i + e'),  rho_i = |u_i|,  e' = 1e-13 + 1e-14  [l2norm_each_head]   else t_i = u_i
//   z_ij = s t_i . t_j  (symmetric: T (T + 1) / 2 dot products)          A = softmax_j z
//   r_i = sum_j A_ij t_j + t_i        xh_i = (r_i - mean r_i) / sqrt(var r_i + 1e-5)  (biased var)       o_i = gamma (.) xh_i + beta
//   E = mean_i o_i | max_i o_i | o_token        or every o_i is stored (the Attention_1 output type, PRE = 0)
// Backward, the forward recomputed from the planes (nothing else is saved), do_i from dE by the pooling (or read from dO):
//   dgamma += do_i (.) xh_i     dbeta += do_i     dxh = do_i (.) gamma
//   dr_i = rstd_i (dxh - mean dxh - xh_i mean(dxh (.) xh_i))
//   dA_ij = dr_i . t_j          dS_ij = A_ij (dA_ij - sum_k A_ik dA_ik)
//   dt_j = dr_j + sum_i A_ij dr_i + s sum_i (dS_ij + dS_ji) t_i
//   du_j = dt_j / (rho_j + e') - t_j (t_j . dt_j) / rho_j  [l2norm_each_head]
//   dx_l = du_{PRE + l} + [mean token] du_0 / L + [max token] du_0 where plane l holds the maximum
// Maxima (the prepended max token, the max pooling): the LOWEST index wins a tie -- a `>` comparison in ascending index.
//
// Mapping: one wavefront per group, lane i owns columns {256 j + 4 i .. + 3} of the head, j < NCH (d <= 512); the tokens stay in
// registers.  A block of four wavefronts walks groups_per_block consecutive groups g = n H + h.  dgamma / dbeta: every wavefront keeps
// its share in registers, the block adds the four shares through LDS in wave order and writes ONE partial row [2 d] to the workspace, a
// second launch adds the partial rows in row order (sum_rows_fixed_order).  No atomics: two calls give the same bits.
// The picking types (a token index) compute one row of A only, and one dr_i.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_common.h"
#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

namespace {

__device__ __forceinline__ float bsum(float v) { return wave_allsum(v); }
__device__ __forceinline__ float4 sel4(int4 idx, int i, float4 v) {
    return make_float4(idx.x == i ? v.x : 0.f, idx.y == i ? v.y : 0.f, idx.z == i ? v.z : 0.f, idx.w == i ? v.w : 0.f);
}
// running maximum with the index of its first occurrence
__device__ __forceinline__ void max4(float4& m, int4& idx, float4 v, int i) {
    if (v.x > m.x) m.x = v.x, idx.x = i;
    if (v.y > m.y) m.y = v.y, idx.y = i;
    if (v.z > m.z) m.z = v.z, idx.z = i;
    if (v.w > m.w) m.w = v.w, idx.w = i;
}

template <int NCH>
struct Lane {
    bool own[NCH];
    int col[NCH];            // the lane's first column of chunk j in the head; a lane without columns reads column 0 and clears the value
    __device__ __forceinline__ Lane(int d) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            own[j] = j * 256 + lane * 4 < d;
            col[j] = own[j] ? j * 256 + lane * 4 : 0;
        }
    }
    __device__ __forceinline__ float4 load(const float* row, int j) const {
        const float4 v = load_nt((const nt_f32x4*)(row + col[j]));
        return own[j] ? v : zero4();
    }
    __device__ __forceinline__ float4 load_cached(const float* row, int j) const {
        const float4 v = *(const float4*)(row + col[j]);
        return own[j] ? v : zero4();
    }
};

// is token i's output wanted at all (wave-uniform)
__device__ __forceinline__ bool active(const SelfAttnArgs& a, int i) { return a.pool != LAFF_SA_POOL_TOKEN || i == a.token; }

// the tokens of a group: every plane's load first, then the prepended token, then the optional normalisation
template <int L, int PRE, int NCH>
__device__ __forceinline__ void tokens_of(const SelfAttnArgs& a, const Lane<NCH>& ln, long n, int hoff, float4 (&t)[L + PRE][NCH],
                                          int4 (&arg)[NCH], float (&rho)[L + PRE], float (&inv_rho)[L + PRE]) {
    constexpr int T = L + PRE;
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int j = 0; j < NCH; ++j) t[PRE + l][j] = ln.load(a.x[l] + n * a.ldx[l] + hoff, j);
    if constexpr (PRE) {
        if (a.prepend == LAFF_SA_PREPEND_MAX) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                t[0][j] = t[1][j];
                arg[j] = make_int4(0, 0, 0, 0);
#pragma unroll
                for (int l = 1; l < L; ++l) max4(t[0][j], arg[j], t[1 + l][j], l);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                float4 s = t[1][j];
#pragma unroll
                for (int l = 1; l < L; ++l) s = add4(s, t[1 + l][j]);
                t[0][j] = scl4(s, 1.0f / L);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < T; ++i) rho[i] = 1.f, inv_rho[i] = 1.f;
    if (a.l2n) {
#pragma unroll
        for (int i = 0; i < T; ++i) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) ss += dot4(t[i][j], t[i][j]);
            rho[i] = sqrtf(bsum(ss));
            inv_rho[i] = 1.0f / (rho[i] + 1e-13f + 1e-14f);
#pragma unroll
            for (int j = 0; j < NCH; ++j) t[i][j] = scl4(t[i][j], inv_rho[i]);
        }
    }
}

// A[i][:] = softmax_j(s t_i . t_j) for the active rows i; the other rows hold zeros
template <int T, int NCH>
__device__ __forceinline__ void weights_of(const SelfAttnArgs& a, const float4 (&t)[T][NCH], float (&A)[T][T]) {
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int k = i; k < T; ++k) {
            float z = 0.f;
            if (active(a, i) || active(a, k)) {
                float p = 0.f;
#pragma unroll
                for (int j = 0; j < NCH; ++j) p += dot4(t[i][j], t[k][j]);
                z = bsum(p) * a.scale;
            }
            A[i][k] = z;
            A[k][i] = z;
        }
#pragma unroll
    for (int i = 0; i < T; ++i) {
        if (active(a, i)) {
            softmax_L<T>(A[i]);
        } else {
#pragma unroll
            for (int k = 0; k < T; ++k) A[i][k] = 0.f;
        }
    }
}

// xh_i and rstd_i of token i: the residual row normalised over the head's d columns (zeros in the columns the lane does not own)
template <int T, int NCH>
__device__ __forceinline__ float normalised_of(int i, const Lane<NCH>& ln, float inv_d, const float4 (&t)[T][NCH], const float (&A)[T][T],
                                               float4 (&xh)[NCH]) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        float4 r = t[i][j];
#pragma unroll
        for (int k = 0; k < T; ++k) r = fma4(t[k][j], A[i][k], r);
        xh[j] = r;
        s += (r.x + r.y) + (r.z + r.w);
    }
    const float mu = bsum(s) * inv_d;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        xh[j] = ln.own[j] ? make_float4(xh[j].x - mu, xh[j].y - mu, xh[j].z - mu, xh[j].w - mu) : zero4();
        q += dot4(xh[j], xh[j]);
    }
    const float rstd = 1.0f / sqrtf(bsum(q) * inv_d + 1e-5f);
#pragma unroll
    for (int j = 0; j < NCH; ++j) xh[j] = scl4(xh[j], rstd);
    return rstd;
}

__device__ __forceinline__ float4 affine4(float4 g, float4 xh, float4 b) {
    return make_float4(fmaf(g.x, xh.x, b.x), fmaf(g.y, xh.y, b.y), fmaf(g.z, xh.z, b.z), fmaf(g.w, xh.w, b.w));
}

}  // namespace

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <int L, int PRE, int NCH>
__global__ __launch_bounds__(256) void selfattn_fwd_kernel(SelfAttnArgs a) {
    constexpr int T = L + PRE;
    const int wave = pinned((int)(threadIdx.x >> 6));
    const int d = a.d;
    const Lane<NCH> ln(d);
    float4 gam[NCH], bet[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) gam[j] = ln.load_cached(a.gamma, j), bet[j] = ln.load_cached(a.beta, j);
    const long total = (long)a.N * a.H;
    const long begin = (long)blockIdx.x * a.groups_per_block, end = min(begin + a.groups_per_block, total);
    const float inv_d = 1.0f / d;
#pragma unroll 1
    for (long g = begin + wave; g < end; g += 4) {                    // wave-uniform: all 64 lanes reach every reduction
        const long n = g / a.H;
        const int hoff = (int)(g - n * a.H) * d;
        float4 t[T][NCH];
        int4 arg[NCH];
        float rho[T], inv_rho[T], A[T][T];
        tokens_of<L, PRE, NCH>(a, ln, n, hoff, t, arg, rho, inv_rho);
        weights_of<T, NCH>(a, t, A);
        float4 acc[NCH];
        int4 eidx[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) acc[j] = zero4(), eidx[j] = make_int4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (!active(a, i)) continue;
            float4 o[NCH];
            normalised_of<T, NCH>(i, ln, inv_d, t, A, o);
#pragma unroll
            for (int j = 0; j < NCH; ++j) o[j] = affine4(gam[j], o[j], bet[j]);
            if (a.pool == LAFF_SA_POOL_ALL) {
                float* row = a.O + n * a.ldon + (long)i * a.ldol + hoff;
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    if (ln.own[j]) store_nt((nt_f32x4*)(row + ln.col[j]), o[j]);
            } else if (a.pool == LAFF_SA_POOL_MAX && i > 0) {
#pragma unroll
                for (int j = 0; j < NCH; ++j) max4(acc[j], eidx[j], o[j], i);
            } else {
#pragma unroll
                for (int j = 0; j < NCH; ++j) acc[j] = add4(acc[j], o[j]);        // mean: the sum; max: o_0; token: the one o_i
            }
        }
        if (a.pool != LAFF_SA_POOL_ALL) {
            float* row = a.E + n * a.lde + hoff;
            const float k = a.pool == LAFF_SA_POOL_MEAN ? 1.0f / T : 1.0f;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                if (ln.own[j]) store_nt((nt_f32x4*)(row + ln.col[j]), scl4(acc[j], k));
        }
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
template <int L, int PRE, int NCH>
__global__ __launch_bounds__(256) void selfattn_bwd_kernel(SelfAttnArgs a) {
    constexpr int T = L + PRE;
    __shared__ __attribute__((aligned(16))) float sh[4][2][256 * NCH];
    const int lane = threadIdx.x & 63, wave = pinned((int)(threadIdx.x >> 6));
    const int d = a.d;
    const Lane<NCH> ln(d);
    float4 gam[NCH], bet[NCH], dgp[NCH], dbp[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        gam[j] = ln.load_cached(a.gamma, j), bet[j] = ln.load_cached(a.beta, j);
        dgp[j] = zero4(), dbp[j] = zero4();
    }
    const long total = (long)a.N * a.H;
    const long begin = (long)blockIdx.x * a.groups_per_block, end = min(begin + a.groups_per_block, total);
    const float inv_d = 1.0f / d;
#pragma unroll 1
    for (long g = begin + wave; g < end; g += 4) {
        const long n = g / a.H;
        const int hoff = (int)(g - n * a.H) * d;
        float4 t[T][NCH], dE[NCH];
        int4 arg[NCH], eidx[NCH];
        float rho[T], inv_rho[T], A[T][T];
        if (a.pool != LAFF_SA_POOL_ALL) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) dE[j] = ln.load(a.dE + n * a.lde + hoff, j);
        }
        tokens_of<L, PRE, NCH>(a, ln, n, hoff, t, arg, rho, inv_rho);
        weights_of<T, NCH>(a, t, A);
        if (a.pool == LAFF_SA_POOL_MAX) {                             // which token holds each column's maximum
            float4 m[NCH];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                float4 o[NCH];
                normalised_of<T, NCH>(i, ln, inv_d, t, A, o);
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    o[j] = affine4(gam[j], o[j], bet[j]);
                    if (i == 0) m[j] = o[j], eidx[j] = make_int4(0, 0, 0, 0);
                    else max4(m[j], eidx[j], o[j], i);
                }
            }
        }
        float4 dr[T][NCH];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (!active(a, i)) {
#pragma unroll
                for (int j = 0; j < NCH; ++j) dr[i][j] = zero4();
                continue;
            }
            float4 xh[NCH], dxh[NCH];
            const float rstd = normalised_of<T, NCH>(i, ln, inv_d, t, A, xh);
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                float4 go;
                if (a.pool == LAFF_SA_POOL_ALL) go = ln.load(a.dO + n * a.ldon + (long)i * a.ldol + hoff, j);
                else if (a.pool == LAFF_SA_POOL_MAX) go = sel4(eidx[j], i, dE[j]);
                else if (a.pool == LAFF_SA_POOL_MEAN) go = scl4(dE[j], 1.0f / T);
                else go = dE[j];
                dgp[j] = add4(dgp[j], mul4(go, xh[j]));
                dbp[j] = add4(dbp[j], go);
                dxh[j] = mul4(go, gam[j]);
                s1 += (dxh[j].x + dxh[j].y) + (dxh[j].z + dxh[j].w);
                s2 += dot4(dxh[j], xh[j]);
            }
            const float m1 = bsum(s1) * inv_d, m2 = bsum(s2) * inv_d;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                dr[i][j] = ln.own[j] ? make_float4(rstd * (dxh[j].x - m1 - xh[j].x * m2), rstd * (dxh[j].y - m1 - xh[j].y * m2),
                                                   rstd * (dxh[j].z - m1 - xh[j].z * m2), rstd * (dxh[j].w - m1 - xh[j].w * m2))
                                     : zero4();
        }
        float dS[T][T];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (active(a, i)) {
#pragma unroll
                for (int k = 0; k < T; ++k) {
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) p += dot4(dr[i][j], t[k][j]);
                    dS[i][k] = bsum(p);
                }
                softmax_bwd_L<T>(A[i], dS[i]);
            } else {
#pragma unroll
                for (int k = 0; k < T; ++k) dS[i][k] = 0.f;
            }
        }
        float4 du0[NCH];
#pragma unroll
        for (int k = 0; k < T; ++k) {
            float4 dt[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                dt[j] = dr[k][j];
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    dt[j] = fma4(dr[i][j], A[i][k], dt[j]);
                    dt[j] = fma4(t[i][j], a.scale * (dS[i][k] + dS[k][i]), dt[j]);
                }
            }
            if (a.l2n) {
                float p = 0.f;
#pragma unroll
                for (int j = 0; j < NCH; ++j) p += dot4(t[k][j], dt[j]);
                const float q = bsum(p) / rho[k];
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    dt[j] = make_float4(fmaf(-t[k][j].x, q, dt[j].x * inv_rho[k]), fmaf(-t[k][j].y, q, dt[j].y * inv_rho[k]),
                                        fmaf(-t[k][j].z, q, dt[j].z * inv_rho[k]), fmaf(-t[k][j].w, q, dt[j].w * inv_rho[k]));
            }
            if (PRE && k == 0) {
#pragma unroll
                for (int j = 0; j < NCH; ++j) du0[j] = dt[j];
                continue;
            }
            const int l = k - PRE;
            if constexpr (PRE) {
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    dt[j] = a.prepend == LAFF_SA_PREPEND_MAX ? add4(dt[j], sel4(arg[j], l, du0[j])) : fma4(du0[j], 1.0f / L, dt[j]);
            }
            float* row = a.dx[l] + n * a.lddx[l] + hoff;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                if (ln.own[j]) store_nt((nt_f32x4*)(row + ln.col[j]), dt[j]);
        }
    }
    if (a.part) {                                                     // kernel-uniform
        // the four shares of the block, added in wave order: one partial row [dgamma | dbeta] per block
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            *(float4*)&sh[wave][0][j * 256 + lane * 4] = dgp[j];
            *(float4*)&sh[wave][1][j * 256 + lane * 4] = dbp[j];
        }
        __syncthreads();
        const int c = (int)threadIdx.x * 4;
        if (c < d) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float4 s = add4(add4(add4(*(const float4*)&sh[0][k][c], *(const float4*)&sh[1][k][c]), *(const float4*)&sh[2][k][c]),
                                      *(const float4*)&sh[3][k][c]);
                *(float4*)(a.part + ((long)blockIdx.x * 2 + k) * d + c) = s;
            }
        }
    }
}

// dgamma | dbeta = the partial rows [2 d] added in a fixed order (a block takes 32 columns); rows = 0 writes zeros
__global__ __launch_bounds__(256) void selfattn_bwd_param_kernel(const float* __restrict__ part, int rows, int d, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta) {
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    const int col = ((int)blockIdx.x * DW_LANES + ln) * 4;            // in [dgamma | dbeta]; a float4 never straddles the two (d % 4 == 0)
    const bool valid = col < 2 * d;
    const float4 t = sum_rows_fixed_order(part + (valid ? col : 0), valid ? rows : 0, 2L * d, sh);
    if (grp == 0 && valid) {
        float* out = col < d ? dgamma : dbeta;
        if (out) *(float4*)(out + (col < d ? col : col - d)) = t;
    }
}

void selfattn_plan(int N, int H, int* groups_per_block, int* chunks) {
    const long total = (long)N * H;
    const long want = (total + 3) / 4, cap = 4096;                    // about 4096 blocks at most, whatever the device
    long P = want < cap ? want : cap;
    if (P < 1) P = 1;
    long R = (total + P - 1) / P;
    R = (R + 3) & ~3L;
    if (R < 4) R = 4;
    P = (total + R - 1) / R;
    *groups_per_block = (int)R;
    *chunks = (int)P;
}

template <int L, int PRE>
static hipError_t launch_selfattn_LP(const SelfAttnArgs& a, bool backward, hipStream_t st) {
    const dim3 grid((unsigned)a.chunks), block(256);
    if (a.d <= 256) {
        if (backward) hipLaunchKernelGGL((selfattn_bwd_kernel<L, PRE, 1>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((selfattn_fwd_kernel<L, PRE, 1>), grid, block, 0, st, a);
    } else {
        if (backward) hipLaunchKernelGGL((selfattn_bwd_kernel<L, PRE, 2>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((selfattn_fwd_kernel<L, PRE, 2>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

template <int L>
static hipError_t launch_selfattn_L(const SelfAttnArgs& a, bool backward, hipStream_t st) {
    return a.prepend != LAFF_SA_PREPEND_NONE ? launch_selfattn_LP<L, 1>(a, backward, st) : launch_selfattn_LP<L, 0>(a, backward, st);
}

static hipError_t launch_selfattn(const SelfAttnArgs& a, bool backward, hipStream_t st) {
    switch (a.L) {
        case 1: return launch_selfattn_L<1>(a, backward, st);
        case 2: return launch_selfattn_L<2>(a, backward, st);
        case 3: return launch_selfattn_L<3>(a, backward, st);
        case 4: return launch_selfattn_L<4>(a, backward, st);
        case 5: return launch_selfattn_L<5>(a, backward, st);
        case 6: return launch_selfattn_L<6>(a, backward, st);
        case 7: return launch_selfattn_L<7>(a, backward, st);
        case 8: return launch_selfattn_L<8>(a, backward, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_selfattn_fuse(SelfAttnArgs& a, hipStream_t st) {
    selfattn_plan(a.N, a.H, &a.groups_per_block, &a.chunks);
    return launch_selfattn(a, false, st);
}

hipError_t launch_selfattn_fuse_backward(SelfAttnArgs& a, float* dgamma, float* dbeta, hipStream_t st) {
    const bool params = dgamma || dbeta;
    if (a.N > 0) {
        selfattn_plan(a.N, a.H, &a.groups_per_block, &a.chunks);
        if (!params) a.part = nullptr;
        const hipError_t e = launch_selfattn(a, true, st);
        if (e != hipSuccess) return e;
    }
    if (!params) return hipSuccess;
    const int groups = (2 * a.d / 4 + DW_LANES - 1) / DW_LANES;
    hipLaunchKernelGGL(selfattn_bwd_param_kernel, dim3((unsigned)groups), dim3(256), 0, st, a.part, a.N > 0 ? a.chunks : 0, a.d, dgamma,
                       dbeta);
    return hipGetLastError();
}

}  // namespace laff
