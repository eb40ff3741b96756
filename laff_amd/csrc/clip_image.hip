// clip_image.hip -- the CLIP image encoder (clip.model.CLIP.encode_image: VisualTransformer, reference model/clip/model.py:153-243,
// 342-343), inference only.  Per frame f (g = res / patch, L = g^2 + 1 tokens, rows f L + t):
//
//   x = [class_embedding ; conv1(frame) as g^2 patch rows] + positional_embedding;  x = ln_pre(x)
//   layers x { x += out_proj(attn(ln_1(x)));  x += c_proj(QuickGELU(c_fc(ln_2(x)))) }   (pre-LN, full MHA, head dim 64)
//   feature = ln_post(x[class row]) . proj
//
// The residual stream x stays fp32 [F L, W]; the matrix operands are the encoder's precision T (_Float16 or float).  The transformer
// core is the text encoder's (clip.hip): clip_gemm_kernel with its three epilogues, clip_ln_kernel (CLIP_LN_PATCH: class / patch row +
// positional row -> ln_pre -> x (fp32), and ln_1 of layer 0 -> operand, in one pass; CLIP_LN_ROW at stride L: the class rows), the
// weight packs and the block's launch sequence (launch_clip_block_qkv / _post).  The kernels of this file:
//   vit_patch_kernel      pixels -> patch operand rows [F g^2, Kp] T in conv1.weight's (c, ky, kx) order, zero past 3 p^2
//   vit_attn_f16_kernel   softmax(q k^T / 8) v per (frame, head) on v_mfma_f32_16x16x32_f16, fp32 softmax (fp16 mode)
//   vit_attn_f32_kernel   the same in fp32 on the vector ALU (fp32 mode)
//   vit_mean_kernel       the per-video mean of the frame features, ascending frame order
//
// The last block: only the class rows are pooled, so its queries, out_proj, ln_2 and MLP run on the F class rows alone (the GEMMs
// write the residual rows f L through ldc = L W); its K and V come from every row (in_proj rows W .. 3W).  Exact.
//
// Batch invariance: every reduction's split and order depends on the model's dimensions only (the GEMM's full-K chain per output,
// the LayerNorm's one-wave butterfly, attention inside one frame, the mean in ascending frame order), so a frame's feature is bitwise
// the same in any batch and any chunking of it.
#include <algorithm>

#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

constexpr int VIT_THREADS = 256;
// the fp16 attention's key tiles of 16 (an even count: 32-key PV slices) by the token count: L <= 64 (ViT-B/32), 128, 224 (ViT-B/16),
// 288 (ViT-L/14); the largest one covers VIT_MAX_TOKENS
constexpr int VIT_NKT[4] = {4, 8, 14, 18};
static_assert(VIT_NKT[3] * 16 >= VIT_MAX_TOKENS, "the largest key-tile class must cover VIT_MAX_TOKENS");

struct VitAttnArgs {
    const float* q;        // query row i of frame f at q + (f nq + i) ldq + 64 h
    const float* kv;       // [F L, 3W] fp32: K at column W + 64 h, V at 2W + 64 h
    void* out;             // [F nq, W] operand
    int W, L, nq, ldq;
};

template <typename T>
__global__ __launch_bounds__(256) void vit_patch_kernel(const float* __restrict__ pix, int F, int res, int P, int g, int Kp,
                                                        T* __restrict__ out) {
    const int K = 3 * P * P, gg = g * g, PP = P * P;
    const long total = (long)F * gg * Kp;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const long row = o / Kp;
        const int k = (int)(o - row * Kp);
        float v = 0.0f;
        if (k < K) {
            const long f = row / gg;
            const int p = (int)(row - f * gg), py = p / g, px = p - py * g;
            const int c = k / PP, r = k - c * PP, ky = r / P, kx = r - ky * P;
            v = pix[((f * 3 + c) * res + py * P + ky) * (long)res + px * P + kx];
        }
        out[o] = (T)v;
    }
}

// fp16 attention.  One workgroup per (frame, head); K (fp16, [Lp][64], 16-byte chunk c of key j at chunk c ^ (j & 7)) and V^T (fp16,
// [64][vld]) of the frame's L keys in LDS, zero for the padded keys L .. Lp - 1 (Lp = 16 NKT, the smallest class that holds L: every
// loop over the tiles is unrolled at compile time and stays in registers).  Wave w takes the 16-query
// blocks w, w + 4, ...:
//   S^T = K Q^T / 8 as 16 x 16 tiles (A = 16 keys, B = 16 queries, 2 MFMAs over the head dim): lane holds query lane & 15 and keys
//         16 kt + 4 (lane >> 4) + r, r = 0..3, of every tile kt, in registers;
//   softmax per query in fp32: the lane's own max / sum over its tiles, then the xor-16 / xor-32 partners (the lanes of its query);
//   O = P V per 32-key slice: the A operand is the lane's own probabilities of tiles 2j, 2j + 1 (k slots 0..3 and 4..7: keys
//       32 j + 4 (lane >> 4) + r and 32 j + 16 + 4 (lane >> 4) + r), the B operand V^T at the same keys for column lane & 15.
// The probabilities are normalised (fp32) before the fp16 cast; O accumulates in fp32 over the slices in ascending order.
template <int NKT>
__global__ __launch_bounds__(VIT_THREADS) void vit_attn_f16_kernel(VitAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char vit_smem[];
    constexpr int Lp = NKT * 16, vld = Lp + 8;
    const int f = blockIdx.x, h = blockIdx.y, W = a.W, L = a.L, nq = a.nq;
    clip_h8* ks = reinterpret_cast<clip_h8*>(vit_smem);                         // [Lp * 8] chunks
    _Float16* vt = reinterpret_cast<_Float16*>(vit_smem + (size_t)Lp * 128);  // [64][vld]
    clip_f4* kbias = reinterpret_cast<clip_f4*>(vit_smem + (size_t)Lp * 128 + 64 * vld * 2);   // [Lp / 4]: 0, or -inf past L
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ql = lane & 15, grp = lane >> 4;
    const float* kv = a.kv + (long)f * L * 3 * W + h * 64;
    for (int e = threadIdx.x; e < Lp * 8; e += VIT_THREADS) {
        const int j = e >> 3, c = e & 7;
        clip_h8 kk, vv;
        if (j < L) {
            const float* p = kv + (long)j * 3 * W + 8 * c;
            const clip_f4 k0 = *reinterpret_cast<const clip_f4*>(p + W), k1 = *reinterpret_cast<const clip_f4*>(p + W + 4);
            const clip_f4 v0 = *reinterpret_cast<const clip_f4*>(p + 2 * W), v1 = *reinterpret_cast<const clip_f4*>(p + 2 * W + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                kk[i] = (_Float16)k0[i];
                kk[i + 4] = (_Float16)k1[i];
                vv[i] = (_Float16)v0[i];
                vv[i + 4] = (_Float16)v1[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) kk[i] = vv[i] = (_Float16)0.0f;
        }
        ks[j * 8 + (c ^ (j & 7))] = kk;
        if (c == 0 && (j & 3) == 0)
            kbias[j >> 2] = clip_f4{j < L ? 0.0f : -__builtin_inff(), j + 1 < L ? 0.0f : -__builtin_inff(),
                                   j + 2 < L ? 0.0f : -__builtin_inff(), j + 3 < L ? 0.0f : -__builtin_inff()};
#pragma unroll
        for (int i = 0; i < 8; ++i) vt[(8 * c + i) * vld + j] = vv[i];
    }
    __syncthreads();

    const int nqb = (nq + 15) >> 4;
    for (int qb = wave; qb < nqb; qb += VIT_THREADS / 64) {
        asm volatile("" ::: "memory");                        // K / V fragments are read per query block, not hoisted into registers
        // B operand: query min(16 qb + ql, nq - 1) (the rows past nq are computed and not stored), scaled by 1/8 (exact)
        const int qi = min(qb * 16 + ql, nq - 1);
        const float* qp = a.q + ((long)f * nq + qi) * a.ldq + h * 64 + 8 * grp;
        clip_h8 qf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const clip_f4 q0 = *reinterpret_cast<const clip_f4*>(qp + 32 * s), q1 = *reinterpret_cast<const clip_f4*>(qp + 32 * s + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                qf[s][i] = (_Float16)(q0[i] * 0.125f);
                qf[s][i + 4] = (_Float16)(q1[i] * 0.125f);
            }
        }
        clip_f4 sc[NKT];
        float m = -__builtin_inff();
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            sc[kt] = clip_f4{0.0f, 0.0f, 0.0f, 0.0f};
            const int j = kt * 16 + ql;
#pragma unroll
            for (int s = 0; s < 2; ++s)
                sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ks[j * 8 + ((4 * s + grp) ^ (j & 7))], qf[s], sc[kt], 0, 0, 0);
            sc[kt] += kbias[kt * 4 + grp];                      // keys 16 kt + 4 grp + r (a table: no per-key compares to keep live)
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, sc[kt][r]);
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float sum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[kt][r] = expf(sc[kt][r] - m);              // exp(-inf) = 0 for the padded keys
                sum += sc[kt][r];
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        clip_f4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = clip_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < NKT / 2; ++j) {
            clip_h8 p;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r] = (_Float16)(sc[2 * j][r] * inv);
                p[r + 4] = (_Float16)(sc[2 * j + 1][r] * inv);
            }
            const int k0 = 32 * j + 4 * grp;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const _Float16* vr = vt + (dt * 16 + ql) * vld + k0;
                const clip_h4 lo = *reinterpret_cast<const clip_h4*>(vr), hi = *reinterpret_cast<const clip_h4*>(vr + 16);
                const clip_h8 b = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(p, b, o[dt], 0, 0, 0);
            }
        }
        // C/D map: column (head dim) 16 dt + ql, row (query) 4 grp + r
        _Float16* out = reinterpret_cast<_Float16*>(a.out);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = qb * 16 + 4 * grp + r;
            if (i < nq)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) out[((long)f * nq + i) * W + h * 64 + dt * 16 + ql] = (_Float16)o[dt][r];
        }
    }
}

// fp32 attention.  One workgroup per (frame, head); K ([L][65], padded: lane j reads row j) and V ([L][64]) of the frame in LDS; wave w
// takes queries w, w + 4, ...  Lane j scores keys j + 64 c (c < 5); fp32 softmax (one butterfly each for the max and the sum); the
// output column d = lane sums p_j v_j in ascending j.
__global__ __launch_bounds__(VIT_THREADS) void vit_attn_f32_kernel(VitAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char vit_smem[];
    constexpr int NC = (VIT_MAX_TOKENS + 63) / 64;
    const int f = blockIdx.x, h = blockIdx.y, W = a.W, L = a.L, nq = a.nq;
    float* ks = reinterpret_cast<float*>(vit_smem);       // [L][65]
    float* vs = ks + L * 65;                               // [L][64]
    float* ps = vs + L * 64;                               // [4][64 NC]
    float* qs = ps + 4 * 64 * NC;                          // [4][64]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* kv = a.kv + (long)f * L * 3 * W + h * 64;
    for (int e = threadIdx.x; e < L * 64; e += VIT_THREADS) {
        const int j = e >> 6, d = e & 63;
        ks[j * 65 + d] = kv[(long)j * 3 * W + W + d];
        vs[j * 64 + d] = kv[(long)j * 3 * W + 2 * W + d];
    }
    __syncthreads();
    float* pw = ps + wave * 64 * NC;
    float* qw = qs + wave * 64;
    for (int i = wave; i < nq; i += VIT_THREADS / 64) {
        qw[lane] = a.q[((long)f * nq + i) * a.ldq + h * 64 + lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float s[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = 0.0f;
#pragma unroll 8
        for (int d = 0; d < 64; ++d) {
            const float qd = qw[d];
#pragma unroll
            for (int c = 0; c < NC; ++c) s[c] = fmaf(qd, ks[min(lane + 64 * c, L - 1) * 65 + d], s[c]);
        }
        float m = -__builtin_inff();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            s[c] = lane + 64 * c < L ? s[c] * 0.125f : -__builtin_inff();
            m = fmaxf(m, s[c]);
        }
        m = wave_allmax(m);
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float e = lane + 64 * c < L ? expf(s[c] - m) : 0.0f;
            pw[lane + 64 * c] = e;
            sum += e;
        }
        sum = wave_allsum(sum);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float o = 0.0f;
        for (int j = 0; j < L; ++j) o = fmaf(pw[j], vs[j * 64 + lane], o);
        reinterpret_cast<float*>(a.out)[((long)f * nq + i) * W + h * 64 + lane] = o / sum;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // every lane has read pw / qw before the next query overwrites them
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// out_mean[v][e] = (sum of out[f][e] over frame_off[v] <= f < frame_off[v + 1], ascending f) / frame count
__global__ __launch_bounds__(256) void vit_mean_kernel(const float* __restrict__ out, int ldo, const int* __restrict__ frame_off, int V,
                                                       int E, float* __restrict__ mean, int ldm) {
    const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (long)V * E) return;
    const int v = (int)(o / E), e = (int)(o - (long)v * E);
    const int f0 = frame_off[v], f1 = frame_off[v + 1];
    float s = 0.0f;
    for (int f = f0; f < f1; ++f) s += out[(long)f * ldo + e];
    mean[(long)v * ldm + e] = s / (float)(f1 - f0);
}

namespace {

unsigned long long vit_attn_attr[5];

size_t vit_attn_f16_smem(int nkt) { return (size_t)nkt * 16 * 128 + (size_t)64 * (nkt * 16 + 8) * 2 + (size_t)nkt * 16 * 4; }
size_t vit_attn_f32_smem(int L) { return ((size_t)L * 129 + 4 * 64 * ((VIT_MAX_TOKENS + 63) / 64) + 4 * 64) * sizeof(float); }

template <int C>
hipError_t vit_attn_f16(const VitAttnArgs& a, int F, int heads, hipStream_t st) {
    const int smem = (int)vit_attn_f16_smem(VIT_NKT[C]);
    CLIP_TRY(smem_attr_once(vit_attn_attr[1 + C], vit_attn_f16_kernel<VIT_NKT[C]>, smem));
    vit_attn_f16_kernel<VIT_NKT[C]><<<dim3(F, heads), VIT_THREADS, smem, st>>>(a);
    return hipGetLastError();
}

hipError_t vit_attn(const VitAttnArgs& a, int F, int heads, int fp16, hipStream_t st) {
    if (fp16) {
        if (a.L <= VIT_NKT[0] * 16) return vit_attn_f16<0>(a, F, heads, st);
        if (a.L <= VIT_NKT[1] * 16) return vit_attn_f16<1>(a, F, heads, st);
        if (a.L <= VIT_NKT[2] * 16) return vit_attn_f16<2>(a, F, heads, st);
        return vit_attn_f16<3>(a, F, heads, st);
    }
    // the attribute once, at the largest size any call takes
    CLIP_TRY(smem_attr_once(vit_attn_attr[0], vit_attn_f32_kernel, (int)vit_attn_f32_smem(VIT_MAX_TOKENS)));
    vit_attn_f32_kernel<<<dim3(F, heads), VIT_THREADS, vit_attn_f32_smem(a.L), st>>>(a);
    return hipGetLastError();
}

template <typename T>
hipError_t vit_encode_t(const ClipImageArgs& e, hipStream_t st) {
    constexpr int fp16 = sizeof(T) == 2;
    const laff_clip_visual& m = *e.model;
    const int W = m.width, F = e.F, P = m.patch_size, res = m.input_resolution, g = res / P, gg = g * g, L = gg + 1, R = F * L;
    char* big = reinterpret_cast<char*>(e.big);
    float* pout = reinterpret_cast<float*>(big + e.patch_out);
    {
        const long total = (long)F * gg * e.Kp;
        const int blocks = (int)std::min<long>((total + 255) / 256, 16384);
        vit_patch_kernel<T><<<blocks, 256, 0, st>>>(e.pixels, F, res, P, g, e.Kp, reinterpret_cast<T*>(big));
        CLIP_TRY(hipGetLastError());
    }
    CLIP_TRY(launch_clip_gemm(big, m.conv1_weight, nullptr, pout, F * gg, W, e.Kp, W, CLIP_EPI_F32, fp16, st));
    ClipLnArgs ln{};                                       // every row; layer 0's ln_1 runs with ln_pre (CLIP_LN_PATCH)
    ln.X = e.X;
    ln.out = e.A;
    ln.W = W;
    ln.rows = R;
    ln.stride = 1;
    ln.round_f32 = 1;
    ln.pos_emb = m.positional_embedding;
    ln.patch = pout;
    ln.cls = m.class_embedding;
    ln.pre_gamma = m.ln_pre_weight;
    ln.pre_beta = m.ln_pre_bias;
    ln.L = L;
    ClipLnArgs cls = ln;                                   // the class rows x[f L] -> a_cls
    cls.out = e.a_cls;
    cls.rows = F;
    cls.stride = L;
    const size_t sz = sizeof(T);
    for (int l = 0; l < m.layers; ++l) {
        const laff_clip_block& b = m.blocks[l];
        const int mode = l == 0 ? CLIP_LN_PATCH : CLIP_LN_ROW;
        if (l + 1 < m.layers) {
            CLIP_TRY(launch_clip_block_qkv(b, mode, ln, e.big, fp16, st));
            CLIP_TRY(vit_attn(VitAttnArgs{reinterpret_cast<const float*>(e.big), reinterpret_cast<const float*>(e.big), e.A, W, L, L,
                                          3 * W},
                              F, m.heads, fp16, st));
            CLIP_TRY(launch_clip_block_post(b, ln, e.big, fp16, st));
        } else {
            // K and V of every row (in_proj rows W .. 3W into QKV columns W .. 3W); the rest on the class rows x[f L] alone
            ln.gamma = cls.gamma = b.ln_1_weight;
            ln.beta = cls.beta = b.ln_1_bias;
            CLIP_TRY(launch_clip_ln(mode, ln, fp16, st));
            const char* kvw = reinterpret_cast<const char*>(b.in_proj_weight) + (size_t)W * W * sz;
            CLIP_TRY(launch_clip_gemm(e.A, kvw, b.in_proj_bias + W, reinterpret_cast<float*>(e.big) + W, R, 2 * W, W, 3 * W, CLIP_EPI_F32,
                                      fp16, st));
            CLIP_TRY(launch_clip_ln(CLIP_LN_ROW, cls, fp16, st));
            CLIP_TRY(launch_clip_gemm(e.a_cls, b.in_proj_weight, b.in_proj_bias, e.q_cls, F, W, W, W, CLIP_EPI_F32, fp16, st));
            CLIP_TRY(vit_attn(VitAttnArgs{e.q_cls, reinterpret_cast<const float*>(e.big), e.a_cls, W, L, 1, W}, F, m.heads, fp16, st));
            CLIP_TRY(launch_clip_block_post(b, cls, e.big, fp16, st));
        }
    }
    cls.gamma = m.ln_post_weight;
    cls.beta = m.ln_post_bias;
    CLIP_TRY(launch_clip_ln(CLIP_LN_ROW, cls, fp16, st));
    CLIP_TRY(launch_clip_gemm(e.a_cls, m.proj, nullptr, e.out, F, m.embed_dim, W, e.ldo, CLIP_EPI_F32, fp16, st));
    if (e.V > 0) {
        const long n = (long)e.V * m.embed_dim;
        vit_mean_kernel<<<(int)((n + 255) / 256), 256, 0, st>>>(e.out, e.ldo, e.frame_off, e.V, m.embed_dim, e.out_mean, e.ldm);
        CLIP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_clip_image_encode(const ClipImageArgs& e, int fp16, hipStream_t st) {
    return fp16 ? vit_encode_t<_Float16>(e, st) : vit_encode_t<float>(e, st);
}

}  // namespace laff
