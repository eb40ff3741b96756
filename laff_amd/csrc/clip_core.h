// clip_core.h -- the device bodies of the transformer core that the CLIP text / image encoders (clip.hip, clip_image.hip) and the
// BERT text encoder (bert.hip) share: the MFMA GEMM tile with its fused epilogues and the one-wave LayerNorm of a row.  Each source
// file instantiates only the epilogues it launches (clip.hip: F32, GELU, RESID; bert.hip: GELU_ERF, TANH), under its own kernel names.
//
// GEMM tile: 128 x 128 outputs per workgroup, 2 x 2 waves of 64 x 64 (4 x 4 MFMA blocks of 16 x 16), K-steps of 128 bytes per row
// (64 halves or 32 floats) staged through two LDS buffers by plain 16-byte loads held in registers across the compute of the step
// before.  LDS image: 16-byte chunk c of row r sits at chunk c ^ (r & 7) of that row.  Rows past M and columns past N are loaded
// from the last valid row / column (every load stays inside its matrix) and not stored.
//   fp16: v_mfma_f32_16x16x32_f16 per 16-byte chunk; lane l holds row l&15, k = 8(l>>4) .. +7 of a 32-wide slice (natural order)
//   fp32: v_mfma_f32_16x16x4_f32 x 4 per 16-byte chunk; component j of lane l is k = 4(l>>4) + j of a 16-wide slice, the same k
//         for both operands, so every product is summed once (the order within the chunk is fixed).
// Each output is one full-K MFMA chain in ascending K-steps from zero in one wave: its value does not depend on M.
#pragma once

#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

constexpr int CLIP_BM = 128, CLIP_BN = 128, CLIP_THREADS = 256;

__device__ __forceinline__ float clip_quick_gelu(float v) { return v / (1.0f + expf(-1.702f * v)); }

template <typename T>
__device__ __forceinline__ clip_f4 clip_mfma_chunk(clip_u4 a, clip_u4 b, clip_f4 acc) {
    if constexpr (sizeof(T) == 2) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(clip_h8, a), __builtin_bit_cast(clip_h8, b), acc, 0, 0, 0);
    } else {
        const clip_f4 af = __builtin_bit_cast(clip_f4, a), bf = __builtin_bit_cast(clip_f4, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], bf[j], acc, 0, 0, 0);
        return acc;
    }
}

// The body of one 128 x 128 output tile (blockIdx.x: column tile, blockIdx.y: row tile) of C = A B^T + bias with epilogue EPI:
// clip_gemm_kernel (clip.hip: F32, GELU, RESID) and bert_gemm_kernel (bert.hip: GELU_ERF, TANH) are thin wrappers around it.
template <typename T, int EPI>
__device__ __forceinline__ void clip_gemm_tile(ClipGemmArgs g) {
    __shared__ clip_u4 lds[2][2][CLIP_BM * 8];               // [stage][A | B][row * 8 + chunk]: 64 KiB
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n0 = blockIdx.x * CLIP_BN, m0 = blockIdx.y * CLIP_BM;
    const int wm = wave >> 1, wn = wave & 1;
    const long rowb = (long)g.K * sizeof(T);               // bytes per operand row (a multiple of 128)
    const int nk = (int)(rowb / 128);
    const char* A = reinterpret_cast<const char*>(g.A);
    const char* B = reinterpret_cast<const char*>(g.B);

    // this thread's four 16-byte chunks of each operand per K-step: rows r0 + 32 i, chunk c (LDS index dst + 256 i)
    const int r0 = tid >> 3, c0 = tid & 7, dst = r0 * 8 + (c0 ^ (r0 & 7));
    long offA[4], offB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        offA[i] = (long)min(m0 + r0 + 32 * i, g.M - 1) * rowb + c0 * 16;
        offB[i] = (long)min(n0 + r0 + 32 * i, g.N - 1) * rowb + c0 * 16;
    }
    clip_u4 ra[4], rb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ra[i] = *reinterpret_cast<const clip_u4*>(A + offA[i]);
        rb[i] = *reinterpret_cast<const clip_u4*>(B + offB[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lds[0][0][dst + 256 * i] = ra[i];
        lds[0][1][dst + 256 * i] = rb[i];
    }

    clip_f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = clip_f4{0.0f, 0.0f, 0.0f, 0.0f};

    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int st = kt & 1;
        if (kt + 1 < nk)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ra[i] = *reinterpret_cast<const clip_u4*>(A + offA[i] + (long)(kt + 1) * 128);
                rb[i] = *reinterpret_cast<const clip_u4*>(B + offB[i] + (long)(kt + 1) * 128);
            }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int c = 4 * s + (lane >> 4);
            clip_u4 a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ra_ = wm * 64 + t * 16 + (lane & 15), rb_ = wn * 64 + t * 16 + (lane & 15);
                a[t] = lds[st][0][ra_ * 8 + (c ^ (ra_ & 7))];
                b[t] = lds[st][1][rb_ * 8 + (c ^ (rb_ & 7))];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = clip_mfma_chunk<T>(a[i], b[j], acc[i][j]);
        }
        if (kt + 1 < nk)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lds[st ^ 1][0][dst + 256 * i] = ra[i];
                lds[st ^ 1][1][dst + 256 * i] = rb[i];
            }
        __syncthreads();
    }

    // C/D map of the 16 x 16 blocks: column lane & 15, row 4 (lane >> 4) + reg
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + j * 16 + (lane & 15);
        if (col >= g.N) continue;
        const float bias = g.bias ? g.bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = m0 + wm * 64 + i * 16 + 4 * (lane >> 4) + reg;
                if (row >= g.M) continue;
                const float v = acc[i][j][reg] + bias;
                const long o = (long)row * g.ldc + col;
                if constexpr (EPI == CLIP_EPI_F32) reinterpret_cast<float*>(g.C)[o] = v;
                else if constexpr (EPI == CLIP_EPI_GELU) reinterpret_cast<T*>(g.C)[o] = (T)clip_quick_gelu(v);
                else if constexpr (EPI == CLIP_EPI_RESID) reinterpret_cast<float*>(g.C)[o] += v;
                else if constexpr (EPI == CLIP_EPI_GELU_ERF)
                    reinterpret_cast<T*>(g.C)[o] = (T)(0.5f * v * (1.0f + erff(v * 0.70710678118654752f)));
                else reinterpret_cast<float*>(g.C)[o] = tanhf(v);                        // CLIP_EPI_TANH
            }
    }
}

// LayerNorm (gamma, beta, eps) of one row held by a wave, element lane + 64 k in x[k]: put(k, y[k]) for each of the lane's elements
template <typename Put>
__device__ __forceinline__ void clip_layernorm(const float (&x)[16], int nv, int W, int lane, const float* gamma, const float* beta,
                                               float eps, Put&& put) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < nv) s += x[k];
    const float mean = wave_allsum(s) / (float)W;
    float q = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < nv) q = fmaf(x[k] - mean, x[k] - mean, q);
    const float rstd = 1.0f / sqrtf(wave_allsum(q) / (float)W + eps);
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < nv) {
            const int e = lane + 64 * k;
            put(k, fmaf((x[k] - mean) * rstd, gamma[e], beta[e]));
        }
}

}  // namespace laff
