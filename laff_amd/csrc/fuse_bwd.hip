// fuse_bwd.hip -- backward of the LAFF attention fusion (fuse.hip, fuse_reg_kernel / fuse_stream_kernel) for gfx950: laff_fuse_backward.
//
// The forward is recomputed from the planes; nothing but the inputs is saved.  Per (row n, head h), in the notation of DESIGN.md 4.19
// (rho_l = |raw_l|, e' = 1e-13 + 1e-14, e = 1e-14):
//   x_l = raw_l / (rho_l + e')  [L2NORM_EACH_HEAD]      s = sum_l x_l         ws = w (.) s / L  [MUL]  else w
//   a = softmax_l(x_l . ws + b)                         g = sum_l a_l x_l + [WITH_AVE] gw s
//   r = |g|                                             E = g / (r + e)
//   dg   = dE / (r + e) - E (E . dE) / r
//   da_l = dg . x_l                                     dz_l = a_l (da_l - sum_k a_k da_k)
//   q    = sum_l dz_l x_l                               dw_h += q (.) s / L  [MUL]  else q
//   dx_l = (a_l + [WITH_AVE] gw) dg + dz_l ws + [MUL] (w (.) q) / L
//   draw_l = dx_l / (rho_l + e') - x_l (x_l . dx_l) / rho_l   [L2NORM_EACH_HEAD]
//   JUST_AVERAGE: dx_l = dE / L.   db = sum dz_l = 0 identically: zeros are written, nothing is reduced.
//
// Mapping: one wavefront per (n, h) as in the forward, lane i owns columns {256 j + 4 i .. +3} of the head.  The grid is head-major:
// block -> (head, chunk of rows_per_block rows); each of the block's four wavefronts walks rows chunk * R + wave, + 4, ... and keeps its
// share of dw_h in registers, the block adds the four shares through LDS in wave order and writes ONE partial row to the workspace; a
// second launch adds the partial rows of a head in row order.  No atomics anywhere: two calls give the same bits.
// Without split heads (every head reads columns [0, d) and dx_l is the sum over the heads) a block walks ALL heads of its rows, one
// after the other, and the wavefront that wrote dx_l for head 0 adds the later heads to its own elements -- the sum over heads stays
// inside one wavefront, in head order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_common.h"
#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

namespace {

__device__ __forceinline__ float bsum(float v) { return wave_allsum(v); }
// A wave-uniform row base + the lane's unsigned byte offset: the scalar-base + 32-bit lane offset form of the global instructions, no
// 64-bit address arithmetic per lane.  row_base() holds the base in scalar registers and hides it from the optimiser: left to itself
// hipcc re-associates (base + n * ld) + lane offset into (base + lane offset) + n * ld and keeps one 64-bit per-lane pointer per load
// and store alive across the row loop (36 VGPRs in <4, 2>).
#define LAFF_GLOBAL __attribute__((address_space(1)))
typedef LAFF_GLOBAL char* gptr;
__device__ __forceinline__ gptr row_base(const float* p) {
    gptr g = (gptr)p;
    asm("" : "+s"(g));
    return g;
}
__device__ __forceinline__ LAFF_GLOBAL nt_f32x4* at(gptr base, unsigned byte_off) { return (LAFF_GLOBAL nt_f32x4*)(base + byte_off); }
__device__ __forceinline__ float4 ld(gptr base, unsigned byte_off) { return f4(*at(base, byte_off)); }
__device__ __forceinline__ void st(gptr base, unsigned byte_off, float4 v) { *at(base, byte_off) = v4(v); }
__device__ __forceinline__ float4 ld_nt(gptr base, unsigned byte_off) { return f4(__builtin_nontemporal_load(at(base, byte_off))); }
__device__ __forceinline__ void st_nt(gptr base, unsigned byte_off, float4 v) { __builtin_nontemporal_store(v4(v), at(base, byte_off)); }
}  // namespace

// ---- register-resident variant: d <= 256 * NCH -------------------------------------------------------------------------------
template <int L, int NCH>
__global__ __launch_bounds__(256) void fuse_bwd_reg_kernel(FuseBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float sh_dw[4][256 * NCH];
    const int lane = threadIdx.x & 63, wave = pinned((int)(threadIdx.x >> 6));
    const int d = a.d;
    const bool nosplit = a.head_stride == 0;
    const int chunk = nosplit ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)a.H);
    const int h_begin = nosplit ? 0 : (int)(blockIdx.x % (unsigned)a.H), h_end = nosplit ? a.H : h_begin + 1;
    const long row_begin = (long)chunk * a.rows_per_block, row_end = min(row_begin + a.rows_per_block, (long)a.N);
    const bool javg = a.flags & LAFF_ATT_JUST_AVERAGE, mul = a.flags & LAFF_ATT_MUL, l2n = a.flags & LAFF_ATT_L2NORM_EACH_HEAD;
    bool own[NCH];
    unsigned boff[NCH];                // byte offset of the lane's columns in a head; columns beyond d: a valid address (column 0),
                                       // the value is cleared after the load
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        own[j] = j * 256 + lane * 4 < d;
        boff[j] = own[j] ? (unsigned)(j * 256 + lane * 4) * 4u : 0u;
    }
    for (int h = h_begin; h < h_end; ++h) {                       // block-uniform
        const int hoff = h * a.head_stride;
        const bool accumulate = nosplit && h > 0;                 // dx_l already holds the earlier heads, written by this very lane
        float4 wv[NCH], dwp[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            wv[j] = (own[j] && a.w) ? ld(row_base(a.w + (long)h * d), boff[j]) : zero4();
            dwp[j] = zero4();
        }
        const float bias = javg ? 0.f : a.b[h];
        const float ave = (!javg && (a.flags & LAFF_ATT_WITH_AVE)) ? a.gw[h] : 0.f;
#pragma unroll 1
        for (long n = row_begin + wave; n < row_end; n += 4) {        // wave-uniform: all 64 lanes reach every reduction
            float4 x[L][NCH], dE[NCH];
            // every load of the row first: (L + 1) * NCH requests in flight together
#pragma unroll
            for (int l = 0; l < L; ++l)
#pragma unroll
                for (int j = 0; j < NCH; ++j) x[l][j] = ld_nt(row_base(a.x[l] + n * a.ldx[l] + hoff), boff[j]);
#pragma unroll
            for (int j = 0; j < NCH; ++j) dE[j] = ld_nt(row_base(a.dE + n * a.lde + (long)h * d), boff[j]);
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                if (!own[j]) {
                    dE[j] = zero4();
#pragma unroll
                    for (int l = 0; l < L; ++l) x[l][j] = zero4();
                }
            float rho[L], inv_rho[L];
            if (l2n) {
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    float ss = 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) ss += dot4(x[l][j], x[l][j]);
                    rho[l] = sqrtf(bsum(ss));
                    inv_rho[l] = 1.0f / (rho[l] + 1e-13f + 1e-14f);
#pragma unroll
                    for (int j = 0; j < NCH; ++j) x[l][j] = scl4(x[l][j], inv_rho[l]);
                }
            }
            float al[L], dz[L];
            float4 dg[NCH], ws[NCH], wq[NCH];
            if (javg) {
#pragma unroll
                for (int l = 0; l < L; ++l) al[l] = 0.f, dz[l] = 0.f;
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    dg[j] = scl4(dE[j], 1.0f / L);
                    ws[j] = zero4();
                    wq[j] = zero4();
                }
            } else {
                float4 sum[NCH], g[NCH];
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    sum[j] = x[0][j];
#pragma unroll
                    for (int l = 1; l < L; ++l) sum[j] = add4(sum[j], x[l][j]);
                }
                // the forward's logits, in its own order of operations: (x_l (.) s / L) . w
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) {
                        const float4 c = mul ? mul4(x[l][j], scl4(sum[j], 1.0f / L)) : x[l][j];
                        p += dot4(c, wv[j]);
                    }
                    al[l] = bsum(p) + bias;
                }
                softmax_L<L>(al);
                float ss = 0.f, gd = 0.f;
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    g[j] = scl4(x[0][j], al[0]);
#pragma unroll
                    for (int l = 1; l < L; ++l) g[j] = fma4(x[l][j], al[l], g[j]);
                    g[j] = fma4(sum[j], ave, g[j]);
                    ss += dot4(g[j], g[j]);
                    gd += dot4(g[j], dE[j]);
                }
                const float r = sqrtf(bsum(ss));
                const float inv = 1.0f / (r + 1e-14f);
                // dg = dE / (r + e) - E (E . dE) / r  with  E = g inv,  E . dE = (g . dE) inv
                const float k = bsum(gd) * inv * inv / r;
#pragma unroll
                for (int j = 0; j < NCH; ++j) dg[j] = make_float4(fmaf(-g[j].x, k, dE[j].x * inv), fmaf(-g[j].y, k, dE[j].y * inv),
                                                                  fmaf(-g[j].z, k, dE[j].z * inv), fmaf(-g[j].w, k, dE[j].w * inv));
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) p += dot4(dg[j], x[l][j]);
                    dz[l] = bsum(p);
                }
                softmax_bwd_L<L>(al, dz);
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    float4 q = scl4(x[0][j], dz[0]);
#pragma unroll
                    for (int l = 1; l < L; ++l) q = fma4(x[l][j], dz[l], q);
                    const float4 sl = scl4(sum[j], 1.0f / L);
                    ws[j] = mul ? mul4(wv[j], sl) : wv[j];
                    wq[j] = mul ? scl4(mul4(wv[j], q), 1.0f / L) : zero4();
                    dwp[j] = add4(dwp[j], mul ? mul4(q, sl) : q);
                }
            }
            // dx_l, one plane at a time
#pragma unroll
            for (int l = 0; l < L; ++l) {
                float4 dx[NCH];
                const float c = al[l] + ave;
#pragma unroll
                for (int j = 0; j < NCH; ++j) dx[j] = javg ? dg[j] : fma4(dg[j], c, fma4(ws[j], dz[l], wq[j]));
                if (l2n) {
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) p += dot4(x[l][j], dx[j]);
                    const float t = bsum(p) / rho[l];
#pragma unroll
                    for (int j = 0; j < NCH; ++j)
                        dx[j] = make_float4(fmaf(-x[l][j].x, t, dx[j].x * inv_rho[l]), fmaf(-x[l][j].y, t, dx[j].y * inv_rho[l]),
                                            fmaf(-x[l][j].z, t, dx[j].z * inv_rho[l]), fmaf(-x[l][j].w, t, dx[j].w * inv_rho[l]));
                }
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    if (own[j]) {
                        const gptr row = row_base(a.dx[l] + n * a.lddx[l] + hoff);
                        if (accumulate) st(row, boff[j], add4(ld(row, boff[j]), dx[j]));
                        else st_nt(row, boff[j], dx[j]);
                    }
            }
        }
        if (a.dw_part) {                                          // kernel-uniform
            // the four shares of the block, added in wave order: one partial row per (head, chunk)
#pragma unroll
            for (int j = 0; j < NCH; ++j) *(float4*)&sh_dw[wave][j * 256 + lane * 4] = dwp[j];
            __syncthreads();
            const int c = (int)threadIdx.x * 4;
            if (c < d) {
                const float4 t = add4(add4(add4(*(const float4*)&sh_dw[0][c], *(const float4*)&sh_dw[1][c]), *(const float4*)&sh_dw[2][c]),
                                      *(const float4*)&sh_dw[3][c]);
                *(float4*)(a.dw_part + ((long)h * a.part_rows + chunk) * d + c) = t;
            }
            __syncthreads();
        }
    }
}

// ---- streaming variant: any d % 4 == 0 (the planes are re-read from L2 in passes; used for d > 512) ------------------------------
// Each wavefront keeps its share of dw_h in its OWN partial row of the workspace (4 rows per (head, chunk)), which it writes at its first
// row and adds to, element by element with the lane that wrote it, at the later ones.
template <int L>
__global__ __launch_bounds__(256) void fuse_bwd_stream_kernel(FuseBwdArgs a) {
    const int lane = threadIdx.x & 63, wave = pinned((int)(threadIdx.x >> 6));
    const int d = a.d;
    const bool nosplit = a.head_stride == 0;
    const int chunk = nosplit ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)a.H);
    const int h_begin = nosplit ? 0 : (int)(blockIdx.x % (unsigned)a.H), h_end = nosplit ? a.H : h_begin + 1;
    const long row_begin = (long)chunk * a.rows_per_block, row_end = min(row_begin + a.rows_per_block, (long)a.N);
    const bool javg = a.flags & LAFF_ATT_JUST_AVERAGE, mul = a.flags & LAFF_ATT_MUL, l2n = a.flags & LAFF_ATT_L2NORM_EACH_HEAD;
    for (int h = h_begin; h < h_end; ++h) {
        const int hoff = h * a.head_stride;
        const bool accumulate = nosplit && h > 0;
        const float* wrow = a.w ? a.w + (long)h * d : nullptr;
        float* dwrow = a.dw_part ? a.dw_part + (((long)h * a.part_rows) + (long)chunk * 4 + wave) * d : nullptr;
        const float bias = javg ? 0.f : a.b[h];
        const float ave = (!javg && (a.flags & LAFF_ATT_WITH_AVE)) ? a.gw[h] : 0.f;
        bool first = true;
#pragma unroll 1
        for (long n = row_begin + wave; n < row_end; n += 4) {
            const float* xr[L];
            float* dxr[L];
#pragma unroll
            for (int l = 0; l < L; ++l) {
                xr[l] = a.x[l] + n * a.ldx[l] + hoff;
                dxr[l] = a.dx[l] + n * a.lddx[l] + hoff;
            }
            const float* dEr = a.dE + n * a.lde + (long)h * d;
            float rho[L], inv_rho[L];
#pragma unroll
            for (int l = 0; l < L; ++l) rho[l] = 1.0f, inv_rho[l] = 1.0f;
            if (l2n) {
                float ss[L];
#pragma unroll
                for (int l = 0; l < L; ++l) ss[l] = 0.f;
                for (int col = lane * 4; col < d; col += 256)
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        const float4 v = *(const float4*)(xr[l] + col);
                        ss[l] += dot4(v, v);
                    }
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    rho[l] = sqrtf(bsum(ss[l]));
                    inv_rho[l] = 1.0f / (rho[l] + 1e-13f + 1e-14f);
                }
            }
            float al[L], dz[L];
            float inv = 0.f, k = 0.f;
#pragma unroll
            for (int l = 0; l < L; ++l) al[l] = 0.f, dz[l] = 0.f;
            if (!javg) {
                float p[L];
#pragma unroll
                for (int l = 0; l < L; ++l) p[l] = 0.f;
                for (int col = lane * 4; col < d; col += 256) {
                    const float4 wv = *(const float4*)(wrow + col);
                    float4 xv[L], s = zero4();
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        xv[l] = scl4(*(const float4*)(xr[l] + col), inv_rho[l]);
                        s = add4(s, xv[l]);
                    }
                    s = scl4(s, 1.0f / L);
#pragma unroll
                    for (int l = 0; l < L; ++l) p[l] += dot4(mul ? mul4(xv[l], s) : xv[l], wv);
                }
#pragma unroll
                for (int l = 0; l < L; ++l) al[l] = bsum(p[l]) + bias;
                softmax_L<L>(al);
                float ss = 0.f, gd = 0.f;
                for (int col = lane * 4; col < d; col += 256) {
                    float4 g = zero4();
#pragma unroll
                    for (int l = 0; l < L; ++l) g = fma4(scl4(*(const float4*)(xr[l] + col), inv_rho[l]), al[l] + ave, g);
                    ss += dot4(g, g);
                    gd += dot4(g, *(const float4*)(dEr + col));
                }
                const float r = sqrtf(bsum(ss));
                inv = 1.0f / (r + 1e-14f);
                k = bsum(gd) * inv * inv / r;
                float q[L];
#pragma unroll
                for (int l = 0; l < L; ++l) q[l] = 0.f;
                for (int col = lane * 4; col < d; col += 256) {
                    float4 xv[L], g = zero4();
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        xv[l] = scl4(*(const float4*)(xr[l] + col), inv_rho[l]);
                        g = fma4(xv[l], al[l] + ave, g);
                    }
                    const float4 e = *(const float4*)(dEr + col);
                    const float4 dg = make_float4(fmaf(-g.x, k, e.x * inv), fmaf(-g.y, k, e.y * inv), fmaf(-g.z, k, e.z * inv),
                                                  fmaf(-g.w, k, e.w * inv));
#pragma unroll
                    for (int l = 0; l < L; ++l) q[l] += dot4(dg, xv[l]);
                }
#pragma unroll
                for (int l = 0; l < L; ++l) dz[l] = bsum(q[l]);
                softmax_bwd_L<L>(al, dz);
            }
            // dx_l of one column chunk from the row's scalars (and this wavefront's share of dw_h when `with_dw`)
            auto columns = [&](int col, float4 (&xv)[L], float4 (&dx)[L], bool with_dw) {
                const float4 e = *(const float4*)(dEr + col);
                float4 s = zero4();
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    xv[l] = scl4(*(const float4*)(xr[l] + col), inv_rho[l]);
                    s = add4(s, xv[l]);
                }
                if (javg) {
#pragma unroll
                    for (int l = 0; l < L; ++l) dx[l] = scl4(e, 1.0f / L);
                    return;
                }
                const float4 wv = *(const float4*)(wrow + col);
                float4 g = zero4(), q = zero4();
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    g = fma4(xv[l], al[l] + ave, g);
                    q = fma4(xv[l], dz[l], q);
                }
                const float4 dg = make_float4(fmaf(-g.x, k, e.x * inv), fmaf(-g.y, k, e.y * inv), fmaf(-g.z, k, e.z * inv),
                                              fmaf(-g.w, k, e.w * inv));
                const float4 sl = scl4(s, 1.0f / L);
                const float4 ws = mul ? mul4(wv, sl) : wv;
                const float4 wq = mul ? scl4(mul4(wv, q), 1.0f / L) : zero4();
#pragma unroll
                for (int l = 0; l < L; ++l) dx[l] = fma4(dg, al[l] + ave, fma4(ws, dz[l], wq));
                if (with_dw && dwrow) {
                    const float4 t = mul ? mul4(q, sl) : q;
                    float4* p = (float4*)(dwrow + col);
                    *p = first ? t : add4(*p, t);
                }
            };
            auto store = [&](int l, int col, float4 v) {
                float4* p = (float4*)(dxr[l] + col);
                *p = accumulate ? add4(*p, v) : v;
            };
            float t[L];
#pragma unroll
            for (int l = 0; l < L; ++l) t[l] = 0.f;
            for (int col = lane * 4; col < d; col += 256) {
                float4 xv[L], dx[L];
                columns(col, xv, dx, true);
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    if (l2n) t[l] += dot4(xv[l], dx[l]);
                    else store(l, col, dx[l]);
                }
            }
            if (l2n) {
#pragma unroll
                for (int l = 0; l < L; ++l) t[l] = bsum(t[l]) / rho[l];
                for (int col = lane * 4; col < d; col += 256) {
                    float4 xv[L], dx[L];
                    columns(col, xv, dx, false);
#pragma unroll
                    for (int l = 0; l < L; ++l)
                        store(l, col, make_float4(fmaf(-xv[l].x, t[l], dx[l].x * inv_rho[l]), fmaf(-xv[l].y, t[l], dx[l].y * inv_rho[l]),
                                                  fmaf(-xv[l].z, t[l], dx[l].z * inv_rho[l]), fmaf(-xv[l].w, t[l], dx[l].w * inv_rho[l])));
                }
            }
            first = false;
        }
        if (first && dwrow)                                       // a wavefront without rows (or JUST_AVERAGE: no dw_part at all)
            for (int col = lane * 4; col < d; col += 256) *(float4*)(dwrow + col) = zero4();
    }
}

// dw[h, c] = the partial rows of head h added in a fixed order (sum_rows_fixed_order: a block takes 32 columns); db = 0.
__global__ __launch_bounds__(256) void fuse_bwd_dw_kernel(const float* __restrict__ part, int rows, int H, int d, float* __restrict__ dw,
                                                          float* __restrict__ db) {
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (db && i < H) db[i] = 0.f;
    if (!dw) return;                                              // kernel-uniform
    const int ln = threadIdx.x & (DW_LANES - 1), grp = threadIdx.x / DW_LANES;
    const int col = ((int)blockIdx.x * DW_LANES + ln) * 4;        // in the stacked [H d] row; a float4 never straddles heads (d % 4 == 0)
    const bool valid = col < H * d;
    const int h = valid ? col / d : 0, c = col - h * d;
    const float4 t = sum_rows_fixed_order(part + (long)h * rows * d + c, valid ? rows : 0, d, sh);
    if (grp == 0 && valid) *(float4*)(dw + col) = t;
}

void fuse_bwd_plan(int N, int H, int d, unsigned flags, int* rows_per_block, int* chunks, int* part_rows) {
    const int Hg = (flags & LAFF_ATT_NO_SPLIT_HEAD) ? 1 : H;
    const long want = (N + 3L) / 4, cap = 4096 / Hg > 1 ? 4096 / Hg : 1;      // about 4096 blocks at most, whatever the device
    long P = want < cap ? want : cap;
    if (P < 1) P = 1;
    long R = (N + P - 1) / P;
    R = (R + 3) & ~3L;
    if (R < 4) R = 4;
    P = (N + R - 1) / R;
    *rows_per_block = (int)R;
    *chunks = (int)P;
    *part_rows = (flags & LAFF_ATT_JUST_AVERAGE) ? 0 : (int)(d <= 512 ? P : 4 * P);
}

template <int L>
static hipError_t launch_fuse_bwd_L(const FuseBwdArgs& a, unsigned grid, hipStream_t st) {
    if (a.d <= 256)
        hipLaunchKernelGGL((fuse_bwd_reg_kernel<L, 1>), dim3(grid), dim3(256), 0, st, a);
    else if (a.d <= 512)
        hipLaunchKernelGGL((fuse_bwd_reg_kernel<L, 2>), dim3(grid), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((fuse_bwd_stream_kernel<L>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fuse_backward(FuseBwdArgs& a, float* dw, float* db, hipStream_t st) {
    int chunks = 0;
    fuse_bwd_plan(a.N, a.H, a.d, a.flags, &a.rows_per_block, &chunks, &a.part_rows);
    if (!dw || (a.flags & LAFF_ATT_JUST_AVERAGE)) a.dw_part = nullptr;
    const unsigned grid = (unsigned)chunks * (unsigned)(a.head_stride ? a.H : 1);
    hipError_t e = hipErrorInvalidValue;
    switch (a.L) {
        case 1: e = launch_fuse_bwd_L<1>(a, grid, st); break;
        case 2: e = launch_fuse_bwd_L<2>(a, grid, st); break;
        case 3: e = launch_fuse_bwd_L<3>(a, grid, st); break;
        case 4: e = launch_fuse_bwd_L<4>(a, grid, st); break;
        case 5: e = launch_fuse_bwd_L<5>(a, grid, st); break;
        case 6: e = launch_fuse_bwd_L<6>(a, grid, st); break;
        case 7: e = launch_fuse_bwd_L<7>(a, grid, st); break;
        case 8: e = launch_fuse_bwd_L<8>(a, grid, st); break;
    }
    if (e != hipSuccess || (!dw && !db)) return e;
    const int groups = (a.H * a.d / 4 + DW_LANES - 1) / DW_LANES;              // (x 256 threads: more than H of them, for db)
    hipLaunchKernelGGL(fuse_bwd_dw_kernel, dim3((unsigned)groups), dim3(256), 0, st, a.dw_part, a.dw_part ? a.part_rows : 0, a.H, a.d,
                       dw, db);
    return hipGetLastError();
}

}  // namespace laff
