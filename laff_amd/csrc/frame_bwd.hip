// frame_bwd.hip -- backward of the per-video frame attention (fuse.hip, frame_fuse_kernel) for gfx950: laff_frame_fuse_backward.
//
// The forward is recomputed from the frames; nothing but the inputs is saved.  Per video, in the notation of DESIGN.md 4.22 (frames
// x_f, f < Fmax; frames at or past len are zeros whatever the buffer holds and are never read; e = 1e-14):
//   s = sum_f x_f        ws = w (.) s / Fmax  [MUL]  else w        z_f = x_f . ws + b      (a padded frame: z_f = b)
//   a = softmax over all Fmax logits     t = sum_f a_f x_f     g = t + [WITH_AVE] gw s     r = |g|     V = g / (r + e)
//   dg   = dV / (r + e) - g (g . dV) / ((r + e)^2 r)
//   da_f = dg . x_f          c = dg . t          dz_f = a_f (da_f - c)          q = sum_{f < len} dz_f x_f
//   dx_f = (a_f + [WITH_AVE] gw) dg + dz_f ws + [MUL] (w (.) q) / Fmax   for f < len;     dx_f = 0 for f >= len
//   dw  += q (.) s / Fmax  [MUL]  else q                                  db = 0: zeros are written, nothing is reduced
//
// Mapping, as the forward: one 256-thread workgroup per (feature, video), wave v walks frames v, v + 4, ..., lane i owns columns
// {256 j + 4 i .. +3}, j < NCH.  Every wave ends pass 1 with the whole of ws, t, s and dg in its own registers (the four partial
// softmaxes are merged through LDS, each wave reads all four), so pass 2 needs no block-wide step per frame.
//   pass 0  [MUL only] s, for ws                                   (the forward's own pre-pass)
//   pass 1  online softmax per wave: M, S, t (and s without MUL); the Fmax - len padded logits enter S analytically
//   pass 2  per frame a_f, da_f, dz_f; q accumulates; dx_f WITHOUT the (w (.) q) / Fmax term is stored
//   pass 3  [MUL only] q is complete: the lane that wrote an element of dx_f adds (w (.) q) / Fmax to it (its own store, read back
//           from L2 -- no ordering between lanes is involved)
// The frames of passes 1 to 3 come from L2 (100 KB a video at (50, 512)).  A wave requests FB frames before it uses the first.
// dw: the block writes ONE partial row to the workspace, frame_bwd_dw_kernel adds the B rows of a feature in a fixed order.  No
// atomics anywhere: two calls give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "attn_common.h"
#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

namespace {

// a . b added to p as four explicit fused multiply-adds: the rounding does not depend on where the call is inlined, so da_f and c
// (the same product when a video has one frame of weight 1) come out with the same bits
__device__ __forceinline__ float dotf(float4 a, float4 b, float p) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, p)))); }
template <int NCH>
__device__ __forceinline__ float wdot(const float4 (&a)[NCH], const float4 (&b)[NCH]) {
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) p = dotf(a[j], b[j], p);
    return wave_allsum(p);
}

}  // namespace

template <int NCH>
__global__ __launch_bounds__(256) void frame_bwd_kernel(FrameBwdGroup grp) {
    __shared__ __attribute__((aligned(16))) float sh_acc[4][NCH * 256];
    __shared__ __attribute__((aligned(16))) float sh_sum[4][NCH * 256];
    __shared__ float sh_m[4], sh_s[4];
    constexpr int FB = 8 / NCH;                                   // frames a wave requests together: 32 VGPRs of loads in flight
    const int lane = threadIdx.x & 63, wave = pinned((int)(threadIdx.x >> 6));
    const int B = grp.B, d = grp.d, Fmax = grp.Fmax;
    const int feat = (int)blockIdx.x / B, bidx = (int)blockIdx.x - feat * B;
    const FrameBwdArgs& a = grp.f[feat];
    const int len = grp.lens ? min(max(grp.lens[bidx], 0), Fmax) : Fmax;
    const float* base = a.frames + (long)bidx * Fmax * d;
    float* dbase = a.dframes + (long)bidx * Fmax * d;
    float* part = grp.dw_part ? grp.dw_part + ((long)feat * B + bidx) * d : nullptr;
    const bool mul = grp.flags & LAFF_ATT_MUL;
    const float bias = a.b[0];
    const float ave = (grp.flags & LAFF_ATT_WITH_AVE) ? a.gw[0] : 0.f;
    const float inv_F = 1.0f / Fmax;

    // the padded rows of dframes: zeros ([len d, Fmax d) is one contiguous run; the frames there are never read)
    for (long i = (long)len * d + (long)threadIdx.x * 4; i < (long)Fmax * d; i += 1024) *(float4*)(dbase + i) = zero4();
    if (len == 0) {                                               // block-uniform: V = 0 there, no gradient, nothing for dw
        if (part && (int)threadIdx.x * 4 < d) *(float4*)(part + threadIdx.x * 4) = zero4();
        return;
    }

    bool own[NCH];
    int coff[NCH];                     // the lane's columns; beyond d: a valid address (column 0), the value is cleared after the load
    float4 ws[NCH], xs[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        own[j] = j * 256 + lane * 4 < d;
        coff[j] = own[j] ? j * 256 + lane * 4 : 0;
        ws[j] = own[j] ? *(const float4*)(a.w + coff[j]) : zero4();
        xs[j] = zero4();
    }
    // the frames f0, f0 + 4, ... of one trip, all requested before the first is used
    auto load_batch = [&](const float* rows, int f0, float4 (&xb)[FB][NCH]) {
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            const int f = min(f0 + 4 * i, len - 1);               // (beyond the clip: a valid address, never folded in)
#pragma unroll
            for (int j = 0; j < NCH; ++j) xb[i][j] = *(const float4*)(rows + (long)f * d + coff[j]);
        }
    };

    if (mul) {
        // pass 0: s over the len real frames, ws = w (.) s / Fmax (the mean counts the padded zeros, as the reference does)
        for (int f0 = wave; f0 < len; f0 += 4 * FB) {
            float4 xb[FB][NCH];
            load_batch(base, f0, xb);
#pragma unroll
            for (int i = 0; i < FB; ++i) {
                if (f0 + 4 * i >= len) break;
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    if (own[j]) xs[j] = add4(xs[j], xb[i][j]);
            }
        }
#pragma unroll
        for (int j = 0; j < NCH; ++j) *(float4*)&sh_sum[wave][j * 256 + lane * 4] = xs[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c = j * 256 + lane * 4;
            xs[j] = add4(add4(*(float4*)&sh_sum[0][c], *(float4*)&sh_sum[1][c]), add4(*(float4*)&sh_sum[2][c], *(float4*)&sh_sum[3][c]));
            ws[j] = mul4(ws[j], scl4(xs[j], inv_F));
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NCH; ++j) *(float4*)&sh_sum[wave][j * 256 + lane * 4] = xs[j];      // s, kept for dw: the wave's own copy
    }

    // pass 1: the wave's online softmax over its frames
    float m = -INFINITY, sden = 0.f;
    float4 acc[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) acc[j] = zero4();
    for (int f0 = wave; f0 < len; f0 += 4 * FB) {
        float4 xb[FB][NCH];
        load_batch(base, f0, xb);
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            if (f0 + 4 * i >= len) break;                           // wave-uniform
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                if (!own[j]) xb[i][j] = zero4();
            const float lg = wdot<NCH>(xb[i], ws) + bias;
            const float mn = fmaxf(m, lg);
            const float rs = expf(m - mn), e = expf(lg - mn);
            sden = sden * rs + e;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                acc[j] = fma4(xb[i][j], e, scl4(acc[j], rs));
                if (!mul) xs[j] = add4(xs[j], xb[i][j]);
            }
            m = mn;
        }
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        *(float4*)&sh_acc[wave][j * 256 + lane * 4] = acc[j];
        if (!mul) *(float4*)&sh_sum[wave][j * 256 + lane * 4] = xs[j];
    }
    if (lane == 0) {
        sh_m[wave] = m;
        sh_s[wave] = sden;
    }
    __syncthreads();
    // the four partial softmaxes + the (Fmax - len) padded frames whose logit is exactly `bias`; every wave forms the whole of g
    float M = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
    const int npad = Fmax - len;
    if (npad > 0) M = fmaxf(M, bias);
    float S = npad > 0 ? npad * expf(bias - M) : 0.f;
    float sc[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        sc[v] = (sh_m[v] == -INFINITY) ? 0.f : expf(sh_m[v] - M);
        S += sh_s[v] * sc[v];
    }
    const float invS = 1.0f / S;
    float4 dg[NCH];
    float c;
    {
        float4 t[NCH], g[NCH], dv[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int col = j * 256 + lane * 4;
            float4 u = zero4();
#pragma unroll
            for (int v = 0; v < 4; ++v) u = fma4(*(float4*)&sh_acc[v][col], sc[v], u);
            t[j] = scl4(u, invS);
            if (!mul) xs[j] = add4(add4(add4(*(float4*)&sh_sum[0][col], *(float4*)&sh_sum[1][col]), *(float4*)&sh_sum[2][col]),
                                   *(float4*)&sh_sum[3][col]);
            g[j] = fma4(xs[j], ave, t[j]);
            dv[j] = own[j] ? *(const float4*)(a.dV + (long)bidx * grp.lddv + coff[j]) : zero4();
        }
        const float r = sqrtf(wdot<NCH>(g, g));
        const float gd = wdot<NCH>(g, dv);
        // dg = dV / (r + e) - g (g . dV) / ((r + e)^2 r); a video whose g is zero (all its frames are) has V = 0 and gets no gradient
        const float inv = r > 0.f ? 1.0f / (r + 1e-14f) : 0.f;
        const float k = r > 0.f ? gd * inv * inv / r : 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            dg[j] = make_float4(fmaf(-g[j].x, k, dv[j].x * inv), fmaf(-g[j].y, k, dv[j].y * inv), fmaf(-g[j].z, k, dv[j].z * inv),
                                fmaf(-g[j].w, k, dv[j].w * inv));
        c = wdot<NCH>(t, dg);
    }
    __syncthreads();                                              // sh_acc is written again after pass 2

    // pass 2: a_f, da_f, dz_f per frame; q; dx_f without the (w (.) q) / Fmax term
    const bool one = Fmax == 1;                                   // a softmax over one logit is constant: dz = 0, exactly
    float4 q[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) q[j] = zero4();
    for (int f0 = wave; f0 < len; f0 += 4 * FB) {
        float4 xb[FB][NCH];
        load_batch(base, f0, xb);
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            if (f0 + 4 * i >= len) break;                           // wave-uniform
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                if (!own[j]) xb[i][j] = zero4();
            const float lg = wdot<NCH>(xb[i], ws) + bias;
            const float da = wdot<NCH>(xb[i], dg);
            const float af = expf(lg - M) * invS;
            const float dz = one ? 0.f : af * (da - c);
            float* row = dbase + (long)(f0 + 4 * i) * d;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                q[j] = fma4(xb[i][j], dz, q[j]);
                if (own[j]) *(float4*)(row + coff[j]) = fma4(dg[j], af + ave, scl4(ws[j], dz));
            }
        }
    }
    if (!part && !mul) return;                                    // kernel-uniform: nobody reads q
#pragma unroll
    for (int j = 0; j < NCH; ++j) *(float4*)&sh_acc[wave][j * 256 + lane * 4] = q[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int col = j * 256 + lane * 4;
        q[j] = add4(add4(add4(*(float4*)&sh_acc[0][col], *(float4*)&sh_acc[1][col]), *(float4*)&sh_acc[2][col]), *(float4*)&sh_acc[3][col]);
    }
    if (part && wave == 0) {
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            if (own[j])
                *(float4*)(part + coff[j]) = mul ? mul4(q[j], scl4(*(float4*)&sh_sum[0][j * 256 + lane * 4], inv_F)) : q[j];
    }
    if (!mul) return;

    // pass 3: the rows this lane stored in pass 2 get (w (.) q) / Fmax
#pragma unroll
    for (int j = 0; j < NCH; ++j) q[j] = own[j] ? scl4(mul4(*(const float4*)(a.w + coff[j]), q[j]), inv_F) : zero4();
    for (int f0 = wave; f0 < len; f0 += 4 * FB) {
        float4 xb[FB][NCH];
        load_batch(dbase, f0, xb);
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            if (f0 + 4 * i >= len) break;                           // wave-uniform
            float* row = dbase + (long)(f0 + 4 * i) * d;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                if (own[j]) *(float4*)(row + coff[j]) = add4(xb[i][j], q[j]);
        }
    }
}

// dw of feature blockIdx.y = its B partial rows added in a fixed order (sum_rows_fixed_order: a block takes 32 columns); db = 0.
__global__ __launch_bounds__(256) void frame_bwd_dw_kernel(FrameBwdGroup grp) {
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    const FrameBwdArgs& a = grp.f[blockIdx.y];
    if (a.db && blockIdx.x == 0 && threadIdx.x == 0) a.db[0] = 0.f;
    if (!a.dw || !grp.dw_part) return;                            // kernel-uniform
    const int ln = threadIdx.x & (DW_LANES - 1), g = threadIdx.x / DW_LANES;
    const int col = ((int)blockIdx.x * DW_LANES + ln) * 4;
    const bool valid = col < grp.d;
    const float4 t = sum_rows_fixed_order(grp.dw_part + (long)blockIdx.y * grp.B * grp.d + col, valid ? grp.B : 0, grp.d, sh);
    if (g == 0 && valid) *(float4*)(a.dw + col) = t;
}

int frame_bwd_variant(int d) { return d <= 256 ? 1 : d <= 512 ? 2 : 4; }

hipError_t launch_frame_fuse_backward(const FrameBwdGroup& g, bool tail, hipStream_t st) {
    const dim3 grid((unsigned)((long)g.B * g.count));
    switch (frame_bwd_variant(g.d)) {
        case 1: hipLaunchKernelGGL((frame_bwd_kernel<1>), grid, dim3(256), 0, st, g); break;
        case 2: hipLaunchKernelGGL((frame_bwd_kernel<2>), grid, dim3(256), 0, st, g); break;
        default: hipLaunchKernelGGL((frame_bwd_kernel<4>), grid, dim3(256), 0, st, g); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !tail) return e;
    hipLaunchKernelGGL(frame_bwd_dw_kernel, dim3((unsigned)((g.d / 4 + DW_LANES - 1) / DW_LANES), (unsigned)g.count), dim3(256), 0, st, g);
    return hipGetLastError();
}

}  // namespace laff
