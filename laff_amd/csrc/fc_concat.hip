// fc_concat.hip -- the W2VV++ "concat" tower in one launch (laff_fc_concat_act_bn[_grouped]):
//
//     Y[N, D] = bn(act( sum_s X_s . W[:, c_s : c_s + Dk_s]^T + bias ))
//
// The reference concatenates the per-feature inputs (torch.cat) and runs one dense F.linear over the (N, sum Dk) matrix.  Here the
// concatenation is never formed: the K loop of an fp32 MFMA GEMM walks the SEGMENTS, each with its own X pointer / ldx, and reads W in
// place through ldw at the segment's column offset.  A sparse (CSR) segment -- the bag-of-words feature, ~10 entries out of ~10k
// columns -- is not staged at all: after the dense K loop every lane adds the few rows of the transposed column block Wt_s that its
// output row names into the SAME accumulator registers with fp32 FMAs, so bias / activation / BatchNorm see the complete sum.
//
// Tile: 128 rows x 128 columns per 256-thread workgroup, four wavefronts of 64 x 64 (2 x 2 blocks of v_mfma_f32_32x32x2_f32, 64
// accumulator registers), K-step 32 floats, two LDS stages of 2 x 16 KiB (64 KiB: two workgroups per CU).  The LDS image of an operand
// is [row][8 chunks of 16 B] with the chunk index XOR-swizzled by (row >> 1) & 7, the image gemm_nt.hip's tiles use: a ds_read_b128 of
// lane (row, k-half) is conflict-free, and the same image is filled either
//   * by LDS-DMA (global_load_lds_dwordx4, swizzle applied to the SOURCE address) when the segment's rows are 16-byte aligned
//     (base, leading dimension, width and -- for W -- the column offset multiples of 4 floats); a chunk past the segment's end is
//     fetched from a zero word instead, or
//   * through registers with element-wise bounds (any width / alignment: w2v's neighbours of width 30 or 1).
// A K-step never straddles two segments: every segment starts a new step and its last step is zero-filled.
//
// Arithmetic: an fp32 MFMA is a k-ordered fmaf chain, one rounding per product; the chain restarts from zero every K-step and the
// step sums are added up in step order (blocked summation, see the K loop).  The order of the operations of one output element is
// fixed by the segment list alone (dense segments in list order, K-steps ascending; then the sparse segments in list order, entries
// in CSR order), never by the row's position in the batch or by the other rows: rows are
// bitwise independent of the batch they arrive in.  Nothing is allocated, nothing synchronises; vector stores only.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace laff {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CT = 128;                 // tile rows == tile columns
constexpr int CROWB = 128;              // bytes of K per row per K-step (32 floats)
constexpr int COPB = CT * CROWB;        // one operand of one stage
constexpr int CSTAGEB = 2 * COPB;
constexpr int CPITCH = 68;              // epilogue slab: 32 rows x 64 fp32 per wave, padded

__device__ __attribute__((aligned(16))) unsigned int g_concat_zero16[4] = {0, 0, 0, 0};

__device__ __forceinline__ int cswz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// The activation in library precision (ocml tanhf / expf, <= 1 ulp; the division is IEEE): this kernel's error is held against
// 2 x the error of an fp32 CPU evaluation, which leaves no room for the ~2.4e-7 of the v_exp_f32 + v_rcp_f32 form the other FC
// epilogues use.  ~100 VALU instructions per value, issued in the shadow of the sibling workgroup's MFMAs (two workgroups per CU).
__device__ __forceinline__ float concat_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ float concat_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ void concat_wave_lds_fence() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    asm volatile("" ::: "memory");
}

// One operand tile of one K-step: 128 rows x 8 chunks; LDS slot p = row * 8 + cs holds source chunk cswz(row, cs) of that row.
// base: first element of the segment's window in row 0; rows clamp to nrows - 1 (such rows / columns are never stored).
// kel0: first element of the step inside the segment, kvalid: the segment's width.
template <bool FAST>
__device__ __forceinline__ void concat_stage(const float* __restrict__ base, int row0, int nrows, long ld, int kel0, int kvalid,
                                             char* lds_op, unsigned lds_op_addr, int tid) {
#pragma unroll
    for (int it = 0; it < CT * 8 / 256; ++it) {
        const int p = it * 256 + tid;
        const int row = p >> 3, cs = p & 7;
        const int c = cswz(row, cs);
        int gr = row0 + row;
        gr = gr < nrows ? gr : nrows - 1;
        const int k = kel0 + c * 4;
        const float* rowp = base + (long)gr * ld;
        if constexpr (FAST) {
            const void* src = (k + 4 <= kvalid) ? (const void*)(rowp + k) : (const void*)g_concat_zero16;
            const unsigned dst = lds_op_addr + (unsigned)(it * 256 + (tid & ~63)) * 16u;
            unsigned keep;
            asm volatile(
                "s_mov_b32 %0, m0\n\t"
                "s_mov_b32 m0, %2\n\t"
                "s_nop 0\n\t"
                "global_load_lds_dwordx4 %1, off\n\t"
                "s_mov_b32 m0, %0"
                : "=&s"(keep)
                : "v"(src), "s"(__builtin_amdgcn_readfirstlane(dst))
                : "memory");
        } else {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k + j < kvalid) v[j] = rowp[k + j];
            *(float4*)(lds_op + (size_t)p * 16) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

__device__ __forceinline__ f32x4 concat_frag(const char* lds_op, int row, int chunk) {
    return *(const f32x4*)(lds_op + row * CROWB + cswz(row, chunk) * 16);
}

__global__ __launch_bounds__(256, 2) void fc_concat_kernel(const ConcatArgs g) {
    __shared__ __attribute__((aligned(16))) char smem[2 * CSTAGEB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, hh = lane >> 5;

    int pi = 0;
    while (pi + 1 < g.count && (int)blockIdx.x >= g.tile_start[pi + 1]) ++pi;      // block-uniform
    const ConcatProblem& q = g.p[pi];
    const int lin = (int)blockIdx.x - g.tile_start[pi];
    const int tiles_c = (q.D + CT - 1) / CT;
    const int r0 = (lin / tiles_c) * CT, c0 = (lin % tiles_c) * CT;
    const int N = q.N, D = q.D;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);

    // ---- dense segments: the K loop walks (segment, K-step inside it) -------------------------------------------------------------
    int total = 0;                                            // K-steps of all dense segments
    for (int s = 0; s < q.nd; ++s) total += (q.d[s].dk + 31) >> 5;
    int st_seg = 0, st_kin = 0;                               // next step to stage
    auto stage_next = [&](int buf) {
        const ConcatDense& sg = q.d[st_seg];
        char* s = smem + buf * CSTAGEB;
        const unsigned sa = lds0 + (unsigned)buf * CSTAGEB;
        const int k0 = st_kin * 32;
        if (sg.fast & 1) concat_stage<true>(sg.X, r0, N, sg.ldx, k0, sg.dk, s, sa, tid);
        else concat_stage<false>(sg.X, r0, N, sg.ldx, k0, sg.dk, s, sa, tid);
        if (sg.fast & 2) concat_stage<true>(q.W + sg.c0, c0, D, q.ldw, k0, sg.dk, s + COPB, sa + COPB, tid);
        else concat_stage<false>(q.W + sg.c0, c0, D, q.ldw, k0, sg.dk, s + COPB, sa + COPB, tid);
        if (++st_kin == ((sg.dk + 31) >> 5)) { st_kin = 0; ++st_seg; }
    };
    if (total > 0) {
        stage_next(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int kt = 0; kt < total; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < total) stage_next(buf ^ 1);          // lands while this step's MFMAs run
            const char* sx = smem + buf * CSTAGEB;
            const char* sw = sx + COPB;
            // Blocked summation: the 32 products of a K-step are chained from ZERO in a step accumulator (the MFMA's C operand is the
            // inline constant 0 for the step's first instruction), and the step's sum is then added to the running total -- an error
            // of ~(sqrt(32) + sqrt(K / 32)) roundings instead of the ~sqrt(K) of one chain over all of K (K = 12k: 4x smaller), at
            // the price of 64 more registers and 64 v_add_f32 per 64 MFMAs.
            f32x16 stp[2][2];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int chunk = 2 * ks + hh;
                f32x4 fw[2], fx[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    fw[t] = concat_frag(sw, wc * 64 + t * 32 + l31, chunk);
                    fx[t] = concat_frag(sx, wr * 64 + t * 32 + l31, chunk);
                }
#pragma unroll
                for (int tr = 0; tr < 2; ++tr)
#pragma unroll
                    for (int tc = 0; tc < 2; ++tc)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                            stp[tr][tc] = __builtin_amdgcn_mfma_f32_32x32x2f32(fw[tc][e], fx[tr][e], (ks == 0 && e == 0) ? zero : stp[tr][tc], 0, 0, 0);
                        }
            }
#pragma unroll
            for (int tr = 0; tr < 2; ++tr)
#pragma unroll
                for (int tc = 0; tc < 2; ++tc) acc[tr][tc] += stp[tr][tc];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next stage's LDS-DMA has landed ...
            __syncthreads();                                  // ... for every wave, and every wave is done reading this one
        }
    }

    // ---- sparse segments: lane (l31, hh) owns output row (tr, l31) and, per (tc, quad), 4 consecutive columns -----------------------
    for (int s = 0; s < q.ns; ++s) {
        const ConcatSparse& sp = q.s[s];
        const long ldwt = sp.ldwt;
#pragma unroll
        for (int tr = 0; tr < 2; ++tr) {
            const int rr = r0 + wr * 64 + tr * 32 + l31;
            int beg = 0, end = 0;
            if (rr < N) { beg = sp.indptr[rr]; end = sp.indptr[rr + 1]; }
            int wi = 0;
            float vi = 0.0f;
            auto fetch = [&](int p) {                         // ids outside the segment's columns contribute nothing
                wi = 0; vi = 0.0f;
                if (p < end) {
                    wi = sp.indices[p];
                    vi = sp.values ? sp.values[p] : 1.0f;
                    if (wi < 0 || wi >= sp.dk) { wi = 0; vi = 0.0f; }
                }
            };
            fetch(beg);
            for (int p = beg; p < end; ++p) {
                const float* wrow = sp.wt + (long)wi * ldwt;
                const float v = vi;
                fetch(p + 1);                                 // the next entry's id is in flight behind this entry's row loads
#pragma unroll
                for (int tc = 0; tc < 2; ++tc)
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) {
                        const int cc = c0 + wc * 64 + tc * 32 + 8 * qd + 4 * hh;
                        if (cc < D) {                          // D % 4 == 0: the whole quad is inside
                            const float4 w4 = *(const float4*)(wrow + cc);
                            acc[tr][tc][4 * qd + 0] = fmaf(v, w4.x, acc[tr][tc][4 * qd + 0]);
                            acc[tr][tc][4 * qd + 1] = fmaf(v, w4.y, acc[tr][tc][4 * qd + 1]);
                            acc[tr][tc][4 * qd + 2] = fmaf(v, w4.z, acc[tr][tc][4 * qd + 2]);
                            acc[tr][tc][4 * qd + 3] = fmaf(v, w4.w, acc[tr][tc][4 * qd + 3]);
                        }
                    }
            }
        }
    }

    // ---- epilogue: bias -> activation -> folded BatchNorm in the accumulator layout, then through a wave-private LDS slab so that a
    // store instruction writes 4 rows x 256 contiguous bytes --------------------------------------------------------------------------
    float* slab = (float*)smem + wave * (32 * CPITCH);        // the operand ring is free: the K loop ended on a barrier
    const int cw0 = c0 + wc * 64;
    const int act = q.act;
#pragma unroll
    for (int tr = 0; tr < 2; ++tr) {
        const int rbase = r0 + wr * 64 + tr * 32;
#pragma unroll
        for (int tc = 0; tc < 2; ++tc)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int cl = tc * 32 + 8 * qd + 4 * hh;
                const int cc = cw0 + cl;
                float v[4], bb[4] = {0, 0, 0, 0}, ss[4] = {1, 1, 1, 1}, hs[4] = {0, 0, 0, 0};
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[tr][tc][4 * qd + e];
                if (cc < D) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (q.bias) bb[e] = q.bias[cc + e];
                        if (q.bn_scale) { ss[e] = q.bn_scale[cc + e]; hs[e] = q.bn_shift[cc + e]; }
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += bb[e];
                if (act == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = concat_tanh(v[e]);
                } else if (act == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
                } else if (act == 3) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = concat_sigmoid(v[e]);
                }
                if (q.bn_scale) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], ss[e], hs[e]);
                }
                *(float4*)(slab + l31 * CPITCH + cl) = make_float4(v[0], v[1], v[2], v[3]);
            }
        concat_wave_lds_fence();
        const int col4 = (lane & 15) * 4;
        const int gc = cw0 + col4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = (lane >> 4) + 4 * j;
            const float4 v = *(const float4*)(slab + row * CPITCH + col4);
            const int gr = rbase + row;
            if (gr < N && gc < D) *(float4*)(q.Y + (long)gr * q.ldy + gc) = v;
        }
        concat_wave_lds_fence();
    }
}

}  // namespace

hipError_t launch_fc_concat(ConcatArgs& a, hipStream_t st) {
    long tiles = 0;
    for (int i = 0; i < a.count; ++i) {
        a.tile_start[i] = (int)tiles;
        tiles += (long)((a.p[i].N + CT - 1) / CT) * ((a.p[i].D + CT - 1) / CT);
        if (tiles > 0x7fffffffL) return hipErrorInvalidValue;
    }
    a.tile_start[a.count] = (int)tiles;
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(fc_concat_kernel, dim3((unsigned)tiles), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace laff
