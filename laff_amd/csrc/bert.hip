// bert.hip -- the BERT text encoder (BertTxtEncoder.forward, reference model/model.py:437-466: transformers' BertModel, pooler_output),
// inference only.  Post-LN, bidirectional MHA with head dim 64:
//
//   x = LN_emb(word[id] + type[0] + pos[t])
//   layers x { h = LN_1(x + Wo MHA(x) + bo);  x = LN_2(h + W2 GELU_erf(W1 h + b1) + b2) }
//   out = tanh(Wp x[CLS] + bp)
//
// Ragged rows.  The reference pads every caption to the batch's longest and masks the padded keys, which then weigh exactly 0: a
// caption's rows are its unpadded computation.  So the captions' rows are concatenated without padding; row_off [N+1] gives where each
// starts and the CLS row of caption i is row_off[i].  The last layer runs its queries, attention output, LayerNorms and feed-forward on
// the N CLS rows alone (gathered into a compact [N, W] block; K and V come from every row): exact, as the pooler reads only those rows.
//
// The residual stream x stays fp32 [R, W]; the matrix operands are the encoder's precision T (_Float16 or float).  The GEMM tile and
// the LayerNorm helper are clip_core.h's; the F32 and RESID epilogues run through clip.hip's launch_clip_gemm.  The kernels of this file:
//   bert_gemm_kernel   clip_gemm_tile with BERT's epilogues: + bias, erf-GELU -> T (intermediate.dense), + bias, tanh -> fp32 (pooler)
//   bert_ln_kernel     one wave per row: EMBED (word + type[0] + pos gather, LN_emb), ROW (LN in place), CLS (the gather of the CLS
//                      rows, no LN); each writes the fp32 stream and the operand T, the latter rounded from the fp32 value
//   bert_attn_kernel   softmax(q k^T / 8) v per (caption, head) over key slices of 32 with an online softmax, so neither registers
//                      nor LDS depend on the caption length: fp16 on v_mfma_f32_16x16x32_f16, fp32 on v_mfma_f32_16x16x4_f32
//
// Batch invariance: every reduction's split and order depends on the model's dimensions and the caption's own length only (the GEMM's
// full-K chain per output, the LayerNorm's one-wave butterfly, attention over the caption's own keys in ascending slices), so a
// caption's feature is bitwise the same in any batch and any chunking of it.
#include <algorithm>

#include "clip_core.h"

namespace laff {

constexpr int BERT_THREADS = 256;

struct BertLnArgs {
    float* X;              // the fp32 rows written (every mode)
    void* out;             // [rows, W] operand
    const float* src;      // CLS: the residual stream the CLS rows are read from
    const float* gamma;
    const float* beta;
    float eps;
    int W, rows;
    const int* ids;        // EMBED: [R]
    const int* row_off;    // EMBED, CLS: [N+1]
    int N, V, P;           // EMBED: captions, vocabulary, positions
    const float* word;     // EMBED: [V, W]
    const float* pos;      // EMBED: [P, W]
    const float* type0;    // EMBED: [W]
};

struct BertAttnArgs {
    const float* qkv;      // [R, 3W] fp32: K at column W + 64 h, V at 2W + 64 h
    const float* q;        // query i of caption c at q + (q0 + i) ldq + 64 h; q0 = row_off[c] (all rows) or c (CLS)
    int ldq;
    void* out;             // operand, row q0 + i
    const int* row_off;
    int W, cls;
};

template <typename T, int EPI>
__global__ __launch_bounds__(CLIP_THREADS) void bert_gemm_kernel(ClipGemmArgs g) {
    clip_gemm_tile<T, EPI>(g);
}

template <typename T, int MODE>
__global__ __launch_bounds__(BERT_THREADS) void bert_ln_kernel(BertLnArgs a) {
    const int row = blockIdx.x * (BERT_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;                             // whole waves: the butterflies below see all 64 lanes
    const int W = a.W, nv = W >> 6;
    float* X = a.X + (long)row * W;
    T* out = reinterpret_cast<T*>(a.out) + (long)row * W;
    float x[16];
    if constexpr (MODE == BERT_LN_CLS) {
        const float* s = a.src + (long)a.row_off[row] * W;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < nv) {
                const float v = s[lane + 64 * k];
                X[lane + 64 * k] = v;
                out[lane + 64 * k] = (T)v;
            }
        return;
    } else if constexpr (MODE == BERT_LN_EMBED) {
        int lo = 0, hi = a.N;                              // the caption: the last c with row_off[c] <= row
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.row_off[mid] <= row) lo = mid;
            else hi = mid;
        }
        const int t = row - a.row_off[lo], id = a.ids[row];
        const bool ok = (unsigned)id < (unsigned)a.V && (unsigned)t < (unsigned)a.P;
        const float* we = a.word + (long)(ok ? id : 0) * W;
        const float* pe = a.pos + (long)(ok ? t : 0) * W;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < nv) {
                const int e = lane + 64 * k;               // BertEmbeddings' order: (word + token type) + position
                x[k] = ok ? (we[e] + a.type0[e]) + pe[e] : __builtin_nanf("");   // an id outside the table poisons its row
            }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < nv) x[k] = X[lane + 64 * k];
    }
    clip_layernorm(x, nv, W, lane, a.gamma, a.beta, a.eps, [&](int k, float v) {
        asm("" : "+v"(v));                                 // v stays an fp32 value: the operand is the stream's value, rounded
        X[lane + 64 * k] = v;
        out[lane + 64 * k] = (T)v;
    });
}

// One workgroup per (caption, head); wave w takes the 16-query blocks w, w + 4, ... of the caption and streams its L keys in slices of
// 32 (two 16-key tiles) straight from the fp32 QKV rows (L2-resident: no LDS), with an online softmax in fp32:
//   S^T = K Q^T / 8 per tile (A = 16 keys, B = 16 queries): lane holds query ql = lane & 15 and keys 16 t + 4 grp + r, r = 0..3;
//   the slice max per query (lane-local, then the xor-16 / xor-32 partners), m' = max(m, max), p = exp(s - m'), the lane's partial
//   sum l = l exp(m - m') + sum p, and O (rows: queries 4 grp + r) rescaled by the factor of query 4 grp + r (from lane 4 grp + r);
//   O += P V with the lane's own probabilities as the A operand.  Keys past L are -inf (their V rows clamped to L - 1, weight 0).
//   fp16: K / Q / P / V cast to fp16, 2 MFMAs per S tile over the head dim, one 16x16x32 MFMA per 16 output columns per slice (slot r:
//         key 32 js + 4 grp + r, slot 4 + r: key 32 js + 16 + 4 grp + r, the same keys in both operands).
//   fp32: 16 MFMAs per S tile (MFMA s takes head dim 16 grp + s in k-slot grp of both operands); 8 per 16 output columns per slice
//         (MFMA (t, r) takes key 32 js + 16 t + 4 grp + r in k-slot grp).
// O / l at the end, with l summed over the query's four lanes.  The slices run in ascending order: the reduction order depends on L.
template <typename T>
__global__ __launch_bounds__(BERT_THREADS) void bert_attn_kernel(BertAttnArgs a) {
    constexpr bool F16 = sizeof(T) == 2;
    const int cap = blockIdx.x, h = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ql = lane & 15, grp = lane >> 4;
    const int r0 = a.row_off[cap], L = a.row_off[cap + 1] - r0;
    const int nq = a.cls ? 1 : L, q0 = a.cls ? cap : r0, W = a.W;
    const long ld = 3L * W;
    const float* kb = a.qkv + (long)r0 * ld + W + h * 64;
    const float* vb = kb + W;
    const int ns = (L + 31) >> 5;
    const float ninf = -__builtin_inff();
    for (int qb = wave; qb * 16 < nq; qb += BERT_THREADS / 64) {
        const float* qp = a.q + (long)(q0 + min(qb * 16 + ql, nq - 1)) * a.ldq + h * 64;   // the rows past nq are not stored
        clip_h8 qh[2];
        float qf[16];
        if constexpr (F16) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const clip_f4 x0 = *reinterpret_cast<const clip_f4*>(qp + 32 * s + 8 * grp);
                const clip_f4 x1 = *reinterpret_cast<const clip_f4*>(qp + 32 * s + 8 * grp + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    qh[s][i] = (_Float16)(x0[i] * 0.125f);
                    qh[s][i + 4] = (_Float16)(x1[i] * 0.125f);
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const clip_f4 x = *reinterpret_cast<const clip_f4*>(qp + 16 * grp + 4 * c);
#pragma unroll
                for (int i = 0; i < 4; ++i) qf[4 * c + i] = x[i] * 0.125f;
            }
        }
        clip_f4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = clip_f4{0.0f, 0.0f, 0.0f, 0.0f};
        float m = ninf, l = 0.0f;
        for (int js = 0; js < ns; ++js) {
            clip_f4 sc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float* kp = kb + (long)min(32 * js + 16 * t + ql, L - 1) * ld;
                sc[t] = clip_f4{0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (F16) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const clip_f4 x0 = *reinterpret_cast<const clip_f4*>(kp + 32 * s + 8 * grp);
                        const clip_f4 x1 = *reinterpret_cast<const clip_f4*>(kp + 32 * s + 8 * grp + 4);
                        clip_h8 kh;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            kh[i] = (_Float16)x0[i];
                            kh[i + 4] = (_Float16)x1[i];
                        }
                        sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[s], sc[t], 0, 0, 0);
                    }
                } else {
                    float kf[16];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const clip_f4 x = *reinterpret_cast<const clip_f4*>(kp + 16 * grp + 4 * c);
#pragma unroll
                        for (int i = 0; i < 4; ++i) kf[4 * c + i] = x[i];
                    }
#pragma unroll
                    for (int s = 0; s < 16; ++s) sc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s], qf[s], sc[t], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (32 * js + 16 * t + 4 * grp + r >= L) sc[t][r] = ninf;
            }
            float mx = ninf;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[t][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);                 // finite: key 32 js < L scores every query
            const float alpha = expf(m - mn);              // 0 on the first slice
            m = mn;
            float ps = 0.0f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[t][r] = expf(sc[t][r] - mn);        // exp(-inf) = 0 for the keys past L
                    ps += sc[t][r];
                }
            l = fmaf(l, alpha, ps);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ar = __shfl(alpha, 4 * grp + r);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt][r] *= ar;
            }
            const float* vr[8];                            // the V rows of k-slots 0..7 (F16) / of (t, r) = (j >> 2, j & 3) (fp32)
#pragma unroll
            for (int j = 0; j < 8; ++j) vr[j] = vb + (long)min(32 * js + 16 * (j >> 2) + 4 * grp + (j & 3), L - 1) * ld;
            if constexpr (F16) {
                clip_h8 p;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = (_Float16)sc[0][r];
                    p[r + 4] = (_Float16)sc[1][r];
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    clip_h8 v;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (_Float16)vr[j][16 * dt + ql];
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(p, v, o[dt], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[j >> 2][j & 3], vr[j][16 * dt + ql], o[dt], 0, 0, 0);
            }
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        T* out = reinterpret_cast<T*>(a.out);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float lr = __shfl(l, 4 * grp + r);
            const int i = qb * 16 + 4 * grp + r;           // C/D map: row (query) 4 grp + r, column (head dim) 16 dt + ql
            if (i < nq)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) out[(long)(q0 + i) * W + h * 64 + 16 * dt + ql] = (T)(o[dt][r] / lr);
        }
    }
}

namespace {

template <typename T>
hipError_t bert_gemm(int epi, const void* A, const void* B, const float* bias, void* C, int M, int N, int K, int ldc, hipStream_t st) {
    ClipGemmArgs g{A, B, bias, C, M, N, K, ldc};
    const dim3 grid((N + CLIP_BN - 1) / CLIP_BN, (M + CLIP_BM - 1) / CLIP_BM);
    if (epi == CLIP_EPI_GELU_ERF) bert_gemm_kernel<T, CLIP_EPI_GELU_ERF><<<grid, CLIP_THREADS, 0, st>>>(g);
    else bert_gemm_kernel<T, CLIP_EPI_TANH><<<grid, CLIP_THREADS, 0, st>>>(g);
    return hipGetLastError();
}

template <typename T>
hipError_t bert_ln(int mode, const BertLnArgs& a, hipStream_t st) {
    const int blocks = (a.rows + 3) / 4;
    if (mode == BERT_LN_EMBED) bert_ln_kernel<T, BERT_LN_EMBED><<<blocks, BERT_THREADS, 0, st>>>(a);
    else if (mode == BERT_LN_CLS) bert_ln_kernel<T, BERT_LN_CLS><<<blocks, BERT_THREADS, 0, st>>>(a);
    else bert_ln_kernel<T, BERT_LN_ROW><<<blocks, BERT_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

// x += Wo a + bo;  x = LN_1(x) -> a;  x += W2 GELU_erf(W1 a + b1) + b2;  x = LN_2(x) -> a   over ln.rows rows of x = ln.X, a = ln.out
template <typename T>
hipError_t bert_block_post(const laff_bert_block& b, int I, BertLnArgs ln, void* big, hipStream_t st) {
    constexpr int fp16 = sizeof(T) == 2;
    const int W = ln.W, M = ln.rows;
    CLIP_TRY(launch_clip_gemm(ln.out, b.attn_out_weight, b.attn_out_bias, ln.X, M, W, W, W, CLIP_EPI_RESID, fp16, st));
    ln.gamma = b.ln_1_weight;
    ln.beta = b.ln_1_bias;
    CLIP_TRY(bert_ln<T>(BERT_LN_ROW, ln, st));
    CLIP_TRY(bert_gemm<T>(CLIP_EPI_GELU_ERF, ln.out, b.inter_weight, b.inter_bias, big, M, I, W, I, st));
    CLIP_TRY(launch_clip_gemm(big, b.out_weight, b.out_bias, ln.X, M, W, I, W, CLIP_EPI_RESID, fp16, st));
    ln.gamma = b.ln_2_weight;
    ln.beta = b.ln_2_bias;
    return bert_ln<T>(BERT_LN_ROW, ln, st);
}

template <typename T>
hipError_t bert_attn(const BertAttnArgs& a, int N, int heads, hipStream_t st) {
    bert_attn_kernel<T><<<dim3(N, heads), BERT_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

template <typename T>
hipError_t bert_encode_t(const BertEncodeArgs& e, hipStream_t st) {
    constexpr int fp16 = sizeof(T) == 2;
    const laff_bert_text& m = *e.model;
    const int W = m.width, I = m.intermediate, R = e.R, N = e.N;
    const size_t sz = sizeof(T);
    float* qkv = reinterpret_cast<float*>(e.big);
    BertLnArgs ln{};                                       // every row
    ln.X = e.X;
    ln.out = e.A;
    ln.eps = m.layer_norm_eps;
    ln.W = W;
    ln.rows = R;
    ln.ids = e.ids;
    ln.row_off = e.row_off;
    ln.N = N;
    ln.V = m.vocab_size;
    ln.P = m.max_position;
    ln.word = m.word_embeddings;
    ln.pos = m.position_embeddings;
    ln.type0 = m.token_type_embedding;
    ln.gamma = m.emb_ln_weight;
    ln.beta = m.emb_ln_bias;
    CLIP_TRY(bert_ln<T>(BERT_LN_EMBED, ln, st));
    BertLnArgs cls = ln;                                   // the CLS rows of the last layer: Xc, Ac
    cls.X = e.Xc;
    cls.out = e.Ac;
    cls.src = e.X;
    cls.rows = N;
    for (int l = 0; l < m.layers; ++l) {
        const laff_bert_block& b = m.blocks[l];
        if (l + 1 < m.layers) {
            CLIP_TRY(launch_clip_gemm(e.A, b.qkv_weight, b.qkv_bias, qkv, R, 3 * W, W, 3 * W, CLIP_EPI_F32, fp16, st));
            CLIP_TRY(bert_attn<T>(BertAttnArgs{qkv, qkv, 3 * W, e.A, e.row_off, W, 0}, N, m.heads, st));
            CLIP_TRY(bert_block_post<T>(b, I, ln, e.big, st));
        } else {
            // K and V of every row (weight rows W .. 3W into QKV columns W .. 3W); the rest on the N CLS rows alone
            const char* kvw = reinterpret_cast<const char*>(b.qkv_weight) + (size_t)W * W * sz;
            CLIP_TRY(launch_clip_gemm(e.A, kvw, b.qkv_bias + W, qkv + W, R, 2 * W, W, 3 * W, CLIP_EPI_F32, fp16, st));
            CLIP_TRY(bert_ln<T>(BERT_LN_CLS, cls, st));
            CLIP_TRY(launch_clip_gemm(e.Ac, b.qkv_weight, b.qkv_bias, e.Qc, N, W, W, W, CLIP_EPI_F32, fp16, st));
            CLIP_TRY(bert_attn<T>(BertAttnArgs{qkv, e.Qc, W, e.Ac, e.row_off, W, 1}, N, m.heads, st));
            CLIP_TRY(bert_block_post<T>(b, I, cls, e.big, st));
        }
    }
    return bert_gemm<T>(CLIP_EPI_TANH, e.Ac, m.pooler_weight, m.pooler_bias, e.out, N, W, W, e.ldo, st);
}

}  // namespace

hipError_t launch_bert_encode(const BertEncodeArgs& e, int fp16, hipStream_t st) {
    return fp16 ? bert_encode_t<_Float16>(e, st) : bert_encode_t<float>(e, st);
}

}  // namespace laff
