// clip.hip -- the CLIP text encoder (clip.model.CLIP.encode_text, reference model/clip/model.py:153-206, 245-358), inference only.
//
//   x = token_embedding[id] + positional_embedding[pos]
//   L x { x += out_proj(attn(ln_1(x)));  x += c_proj(QuickGELU(c_fc(ln_2(x)))) }     (pre-LN, causal MHA, head dim 64)
//   feature = ln_final(x[eot row]) . text_projection
//
// Ragged rows.  Caption i is given by its ids up to and including p_i = argmax(ids_i) (the row the reference pools): with a causal
// mask no later position can reach row p_i, so the rows after it are never computed.  The captions' rows are concatenated; row_off
// [N+1] gives where each starts, and the pooled row of caption i is row_off[i+1] - 1.
//
// The residual stream x stays fp32 [R, W].  The matrix operands are the encoder's precision T (_Float16 or float).  The kernels and the
// block's launch sequence (launch_clip_block_qkv / _post) are shared with the image encoder (clip_image.hip):
//   clip_ln_kernel     LayerNorm (fp32 statistics) of a row -> operand T; rows at a stride, the token embedding gather for layer 0,
//                      the pooled rows, or the image's patch embedding + ln_pre
//   clip_gemm_kernel   out[r][c] = sum_k A[r][k] * B[c][k] (B = a packed nn.Linear weight [out, in]) with three epilogues:
//                      + bias -> fp32 (in_proj, text_projection), + bias, QuickGELU -> T (c_fc), + bias added in place to x
//                      (out_proj, c_proj: every element has one owner, no atomics)
//   clip_attn_kernel   softmax(q k^T / 8 + causal) v per (caption, head), fp32, from the fp32 QKV rows -> operand T
//   clip_pack_kernel   an fp32 weight -> operand T: transposed (text_projection, proj), or zero-padded columns (conv1)
//
// Batch invariance: every reduction's split and order depends on the model's dimensions only.  A GEMM output is one full-K MFMA chain
// in ascending K-steps from zero in one wave, the LayerNorm sums are one wave's butterfly over a fixed lane map, and attention reads
// only its own caption.  So a caption's feature is bitwise the same in any batch and any chunking of it.
//
// The GEMM tile and the LayerNorm helper are in clip_core.h (shared with bert.hip).
#include <algorithm>

#include "clip_core.h"

namespace laff {

constexpr int CLIP_CTX = 77;

template <typename T, int EPI>
__global__ __launch_bounds__(CLIP_THREADS) void clip_gemm_kernel(ClipGemmArgs g) {
    clip_gemm_tile<T, EPI>(g);
}

// One wave per row: x (fp32, width W <= 1024: W / 64 values per lane, element lane + 64 k) -> LayerNorm -> operand T.
//   CLIP_LN_ROW    x = X[row * stride]          (stride 1: every row; stride L: the image's class rows)
//   CLIP_LN_EMBED  x = token_embedding[ids[row]] + positional_embedding[row - row_off[caption]], also written to X[row]
//   CLIP_LN_POOL   x = X[row_off[row + 1] - 1]        (row = caption)
//   CLIP_LN_PATCH  x = ln_pre((t == 0 ? class_embedding : patch[f g^2 + t - 1]) + pos[t]), also written to X[row]  (row = f L + t)
// F32: the affine result is rounded to fp32 before the conversion to T (the image tower); otherwise fmaf rounds straight to T (the
// text tower: one rounding, v_fma_mixlo_f16 for fp16).  The two differ in the last fp16 bit now and then; each tower keeps its own.
template <typename T, int MODE, bool F32>
__global__ __launch_bounds__(CLIP_THREADS) void clip_ln_kernel(ClipLnArgs a) {
    const int row = blockIdx.x * (CLIP_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;                             // whole waves: the butterflies below see all 64 lanes
    const int W = a.W, nv = W >> 6;
    float x[16];
    if constexpr (MODE == CLIP_LN_EMBED) {
        int lo = 0, hi = a.N;                              // the caption: the last c with row_off[c] <= row
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.row_off[mid] <= row) lo = mid;
            else hi = mid;
        }
        const int pos = row - a.row_off[lo], id = a.ids[row];
        const bool ok = (unsigned)id < (unsigned)a.V && (unsigned)pos < (unsigned)a.ctx;
        const float* te = a.tok_emb + (long)(ok ? id : 0) * W;
        const float* pe = a.pos_emb + (long)(ok ? pos : 0) * W;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < nv) {
                const int e = lane + 64 * k;
                x[k] = ok ? te[e] + pe[e] : __builtin_nanf("");   // an id outside the table poisons its row instead of reading past it
                a.X[(long)row * W + e] = x[k];
            }
    } else if constexpr (MODE == CLIP_LN_PATCH) {
        const int L = a.L, f = row / L, t = row - f * L;
        const float* src = t == 0 ? a.cls : a.patch + ((long)f * (L - 1) + t - 1) * W;
        const float* pe = a.pos_emb + (long)t * W;
        float e[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < nv) e[k] = src[lane + 64 * k] + pe[lane + 64 * k];
        clip_layernorm(e, nv, W, lane, a.pre_gamma, a.pre_beta, 1e-5f,
                       [&](int k, float v) { a.X[(long)row * W + lane + 64 * k] = x[k] = v; });
    } else {
        const long src = MODE == CLIP_LN_POOL ? a.row_off[row + 1] - 1 : (long)row * a.stride;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < nv) x[k] = a.X[src * W + lane + 64 * k];
    }
    T* out = reinterpret_cast<T*>(a.out) + (long)row * W;
    clip_layernorm(x, nv, W, lane, a.gamma, a.beta, 1e-5f, [&](int k, float v) {
        if constexpr (F32) asm("" : "+v"(v));              // v stays an fp32 value: the conversion cannot fuse with the fmaf
        out[lane + 64 * k] = (T)v;
    });
}

// One workgroup per (caption, head): q, k, v of the caption's L <= 77 rows in LDS; wave w takes query rows w, w + 4, ...
// Lane j scores key j and j + 64; the softmax is fp32 (max-subtracted exp, one butterfly each for the max and the sum); the output
// column d = lane sums p_j v_j in ascending j.
template <typename T>
__global__ __launch_bounds__(CLIP_THREADS) void clip_attn_kernel(ClipAttnArgs a) {
    __shared__ float qs[CLIP_CTX][64];
    __shared__ float ks[CLIP_CTX][65];                     // padded: lane j reads row j
    __shared__ float vs[CLIP_CTX][64];
    __shared__ float ps[CLIP_THREADS / 64][2 * 64];
    const int cap = blockIdx.x, h = blockIdx.y;
    const int r0 = a.row_off[cap], L = min(a.row_off[cap + 1] - r0, CLIP_CTX);
    const int W = a.W, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < L * 64; e += CLIP_THREADS) {
        const int i = e >> 6, d = e & 63;
        const float* p = a.qkv + (long)(r0 + i) * 3 * W + h * 64 + d;
        qs[i][d] = p[0];
        ks[i][d] = p[W];
        vs[i][d] = p[2 * W];
    }
    __syncthreads();
    const int j1 = min(lane + 64, CLIP_CTX - 1);
    for (int i = wave; i < L; i += CLIP_THREADS / 64) {
        float d0 = 0.0f, d1 = 0.0f;
        const int j0 = min(lane, L - 1);
#pragma unroll 8
        for (int d = 0; d < 64; ++d) {
            d0 = fmaf(qs[i][d], ks[j0][d], d0);
            d1 = fmaf(qs[i][d], ks[j1][d], d1);
        }
        const float ninf = -__builtin_inff();
        const float s0 = lane <= i ? d0 * 0.125f : ninf, s1 = lane + 64 <= i ? d1 * 0.125f : ninf;
        const float m = wave_allmax(fmaxf(s0, s1));
        const float e0 = lane <= i ? expf(s0 - m) : 0.0f, e1 = lane + 64 <= i ? expf(s1 - m) : 0.0f;
        const float sum = wave_allsum(e0 + e1);
        ps[wave][lane] = e0;
        ps[wave][lane + 64] = e1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float o = 0.0f;
        for (int j = 0; j <= i; ++j) o = fmaf(ps[wave][j], vs[j][lane], o);
        reinterpret_cast<T*>(a.out)[(long)(r0 + i) * W + h * 64 + lane] = (T)(o / sum);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // every lane has read ps before the next row overwrites it
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// out [rows, ldp]: out[r][c] = W[r][c], zero for c >= cols; transpose: out [cols, rows], out[c][r] = W[r][c]
template <typename T>
__global__ __launch_bounds__(256) void clip_pack_kernel(const float* __restrict__ W, int rows, int cols, int transpose, int ldp,
                                                        T* __restrict__ out) {
    const long total = (long)rows * (transpose ? cols : ldp);
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        if (transpose) {
            out[o] = (T)W[(o % rows) * cols + o / rows];
        } else {
            const long r = o / ldp;
            const int c = (int)(o - r * ldp);
            out[o] = c < cols ? (T)W[r * cols + c] : (T)0.0f;
        }
    }
}

hipError_t launch_clip_pack(const float* W, int rows, int cols, int transpose, int ldp, int fp16, void* out, hipStream_t st) {
    const long total = (long)rows * (transpose ? cols : ldp);
    const int blocks = (int)std::min<long>((total + 255) / 256, 8192);
    if (fp16) clip_pack_kernel<_Float16><<<blocks, 256, 0, st>>>(W, rows, cols, transpose, ldp, reinterpret_cast<_Float16*>(out));
    else clip_pack_kernel<float><<<blocks, 256, 0, st>>>(W, rows, cols, transpose, ldp, reinterpret_cast<float*>(out));
    return hipGetLastError();
}

namespace {

template <typename T>
hipError_t clip_gemm(const void* A, const void* B, const float* bias, void* C, int M, int N, int K, int ldc, int epi, hipStream_t st) {
    ClipGemmArgs g{A, B, bias, C, M, N, K, ldc};
    const dim3 grid((N + CLIP_BN - 1) / CLIP_BN, (M + CLIP_BM - 1) / CLIP_BM);
    if (epi == CLIP_EPI_F32) clip_gemm_kernel<T, CLIP_EPI_F32><<<grid, CLIP_THREADS, 0, st>>>(g);
    else if (epi == CLIP_EPI_GELU) clip_gemm_kernel<T, CLIP_EPI_GELU><<<grid, CLIP_THREADS, 0, st>>>(g);
    else clip_gemm_kernel<T, CLIP_EPI_RESID><<<grid, CLIP_THREADS, 0, st>>>(g);
    return hipGetLastError();
}

template <typename T>
hipError_t clip_ln(int mode, const ClipLnArgs& a, hipStream_t st) {
    const int blocks = (a.rows + 3) / 4;
    if (mode == CLIP_LN_EMBED) clip_ln_kernel<T, CLIP_LN_EMBED, false><<<blocks, CLIP_THREADS, 0, st>>>(a);
    else if (mode == CLIP_LN_POOL) clip_ln_kernel<T, CLIP_LN_POOL, false><<<blocks, CLIP_THREADS, 0, st>>>(a);
    else if (mode == CLIP_LN_PATCH) clip_ln_kernel<T, CLIP_LN_PATCH, true><<<blocks, CLIP_THREADS, 0, st>>>(a);
    else if (a.round_f32) clip_ln_kernel<T, CLIP_LN_ROW, true><<<blocks, CLIP_THREADS, 0, st>>>(a);
    else clip_ln_kernel<T, CLIP_LN_ROW, false><<<blocks, CLIP_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

template <typename T>
hipError_t clip_encode_t(const ClipEncodeArgs& e, hipStream_t st) {
    constexpr int fp16 = sizeof(T) == 2;
    const laff_clip_text& m = *e.model;
    const int W = m.width, R = e.R, N = e.N;
    ClipLnArgs ln{};
    ln.X = e.X;
    ln.out = e.A;
    ln.W = W;
    ln.rows = R;
    ln.stride = 1;
    ln.ids = e.ids;
    ln.row_off = e.row_off;
    ln.N = N;
    ln.V = m.vocab_size;
    ln.ctx = m.context_length;
    ln.tok_emb = m.token_embedding;
    ln.pos_emb = m.positional_embedding;
    ClipAttnArgs at{reinterpret_cast<const float*>(e.big), e.row_off, e.A, W};
    for (int l = 0; l < m.layers; ++l) {
        CLIP_TRY(launch_clip_block_qkv(m.blocks[l], l == 0 ? CLIP_LN_EMBED : CLIP_LN_ROW, ln, e.big, fp16, st));
        clip_attn_kernel<T><<<dim3(N, m.heads), CLIP_THREADS, 0, st>>>(at);
        CLIP_TRY(hipGetLastError());
        CLIP_TRY(launch_clip_block_post(m.blocks[l], ln, e.big, fp16, st));
    }
    ln.gamma = m.ln_final_weight;
    ln.beta = m.ln_final_bias;
    ln.rows = N;
    CLIP_TRY(clip_ln<T>(CLIP_LN_POOL, ln, st));
    return clip_gemm<T>(e.A, m.text_projection, nullptr, e.out, N, m.embed_dim, W, e.ldo, CLIP_EPI_F32, st);
}

}  // namespace

hipError_t launch_clip_encode(const ClipEncodeArgs& e, int fp16, hipStream_t st) {
    return fp16 ? clip_encode_t<_Float16>(e, st) : clip_encode_t<float>(e, st);
}

hipError_t launch_clip_gemm(const void* A, const void* B, const float* bias, void* C, int M, int N, int K, int ldc, int epi, int fp16,
                            hipStream_t st) {
    return fp16 ? clip_gemm<_Float16>(A, B, bias, C, M, N, K, ldc, epi, st) : clip_gemm<float>(A, B, bias, C, M, N, K, ldc, epi, st);
}

hipError_t launch_clip_ln(int mode, const ClipLnArgs& a, int fp16, hipStream_t st) {
    return fp16 ? clip_ln<_Float16>(mode, a, st) : clip_ln<float>(mode, a, st);
}

hipError_t launch_clip_block_qkv(const laff_clip_block& b, int mode, ClipLnArgs ln, void* big, int fp16, hipStream_t st) {
    const int W = ln.W;
    ln.gamma = b.ln_1_weight;
    ln.beta = b.ln_1_bias;
    CLIP_TRY(launch_clip_ln(mode, ln, fp16, st));
    return launch_clip_gemm(ln.out, b.in_proj_weight, b.in_proj_bias, big, ln.rows, 3 * W, W, 3 * W, CLIP_EPI_F32, fp16, st);
}

hipError_t launch_clip_block_post(const laff_clip_block& b, ClipLnArgs ln, void* big, int fp16, hipStream_t st) {
    const int W = ln.W, M = ln.rows, ldx = ln.stride * W;
    CLIP_TRY(launch_clip_gemm(ln.out, b.out_proj_weight, b.out_proj_bias, ln.X, M, W, W, ldx, CLIP_EPI_RESID, fp16, st));
    ln.gamma = b.ln_2_weight;
    ln.beta = b.ln_2_bias;
    CLIP_TRY(launch_clip_ln(CLIP_LN_ROW, ln, fp16, st));
    CLIP_TRY(launch_clip_gemm(ln.out, b.c_fc_weight, b.c_fc_bias, big, M, 4 * W, W, 4 * W, CLIP_EPI_GELU, fp16, st));
    return launch_clip_gemm(big, b.c_proj_weight, b.c_proj_bias, ln.X, M, W, 4 * W, ldx, CLIP_EPI_RESID, fp16, st);
}

}  // namespace laff
