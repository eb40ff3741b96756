/*
 * laff_hip.h -- C ABI of liblaff_hip.so: the MI355X (gfx950) kernels behind the LAFF retrieval hot path.
 *
 * The reference (ruc-aimc-lab/LAFF, pure Python/PyTorch) has no FFI layer; its boundary is the nn.Module
 * API in model/model.py.  laff_amd/ keeps that Python surface and calls the entry points below through
 * ctypes.  Each entry point names the reference code it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - every pointer is CALLER-OWNED DEVICE MEMORY (hipMalloc / a torch tensor's data_ptr) unless the
 *     parameter is documented as host memory; the library neither frees nor retains it past the call;
 *   - all matrices are row-major fp32 unless stated; `ld*` = leading dimension in ELEMENTS;
 *   - calls are asynchronous and ordered on the stream bound to the ctx (laff_ctx_set_stream);
 *     only laff_rank_metrics / laff_device_info synchronise;
 *   - return value: 0 = LAFF_OK, negative = error; laff_last_error() returns the thread-local message;
 *   - an EMPTY problem (N = 0 rows / B = 0 videos / Nt = 0 or Nv = 0) is legal everywhere -- the reference meets it as an
 *     empty last batch or an empty query set: the call returns LAFF_OK without launching or touching any pointer;
 *   - a ctx is not thread-safe; distinct ctxs are independent.  No exceptions cross this boundary.
 */
#ifndef LAFF_HIP_H
#define LAFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAFF_ABI_VERSION 47

enum {
    LAFF_OK = 0,
    LAFF_E_ARG = -1,          /* null pointer / negative size / bad enum */
    LAFF_E_SHAPE = -2,        /* shape outside what the kernels support (message says which) */
    LAFF_E_ALIGN = -3,        /* pointer / leading dimension alignment */
    LAFF_E_HIP = -4,          /* a HIP runtime call failed (message carries hipGetErrorString) */
    LAFF_E_UNSUPPORTED = -5
};

/* activation of TransformNet (model/model.py:236-243) */
enum { LAFF_ACT_NONE = 0, LAFF_ACT_TANH = 1, LAFF_ACT_RELU = 2, LAFF_ACT_SIGMOID = 3 };

/* flags of the attention kernels (Attention_1 ctor, model/Attention.py:48-63; Multi_head ctor :489-506) */
enum {
    LAFF_ATT_WITH_AVE = 1,          /* g += gw * mean_L(x)           (Attention.py:94-99) */
    LAFF_ATT_MUL = 2,               /* logits on x * mean_L(x)       (Attention.py:83-86) */
    LAFF_ATT_L2NORM_EACH_HEAD = 4,  /* l2norm(x, dim=3) per head     (Attention.py:522-523) */
    LAFF_ATT_NO_SPLIT_HEAD = 8,     /* every head sees all D columns (Attention.py:520)   */
    LAFF_ATT_JUST_AVERAGE = 16      /* JustAverage: mean over L, no softmax, no norm (Attention.py:35-37) */
};

/* operand precision of the similarity GEMM */
enum {
    LAFF_PREC_FP32 = 0,    /* fp32 MFMA (v_mfma_f32_32x32x2_f32): bit-for-bit an fp32 fma chain          */
    LAFF_PREC_FP16 = 1,    /* one fp16 MFMA pass: MEASURED max |d cos| 8e-5 on 4e8 pairs at d=512; the PROVEN per-pair bound is
                            * band_t + band_v of laff_rank_prepare, 4-5e-4 at d=512 (Cauchy-Schwarz on the operand rounding).  Ranks
                            * from the banded pipeline are exact regardless; a caller that needs every returned score inside 1e-4
                            * takes FP16X3 (what predict() / retrieve() default to) */
    LAFF_PREC_BF16 = 2,    /* one bf16 MFMA pass: ~5e-4 -- for rank-identity workloads only              */
    LAFF_PREC_FP16X3 = 3,  /* fp16 hi+lo split, 3 MFMA passes: ~1e-7                                    */
    LAFF_PREC_BF16X3 = 4   /* bf16 hi+lo split, 3 MFMA passes: ~1e-6                                    */
};

typedef struct laff_ctx laff_ctx;

/* ---- context ------------------------------------------------------------------------------------ */
int laff_abi_version(void);
const char* laff_last_error(void);
/* device: HIP ordinal; hip_stream: hipStream_t (NULL = default stream). */
int laff_ctx_create(int device, void* hip_stream, laff_ctx** out);
int laff_ctx_set_stream(laff_ctx* ctx, void* hip_stream);
int laff_ctx_destroy(laff_ctx* ctx);
/* host out: [0]=CU count, [1]=clock MHz, [2]=LDS bytes per CU-workgroup limit, [3]=wavefront size */
int laff_device_info(laff_ctx* ctx, int out[4]);
/* Measurement aid (no counterpart in the reference): a one-thread launch, ordered on the ctx's stream like every other call and
 * capturable in a HIP graph, that writes the device's constant-rate wall clock (s_memrealtime) to *slot (device memory).  bench.py puts
 * one in front of and behind every launch of a captured step: the differences are the durations of the kernels as the graph runs
 * them (this runtime refuses event-record nodes in a capture).  laff_wall_clock_khz: ticks per millisecond of that clock. */
int laff_stamp(laff_ctx* ctx, unsigned long long* slot /*device*/);
int laff_wall_clock_khz(laff_ctx* ctx, int* khz /*host*/);

/* ---- a1: TransformNet.forward (model/model.py:257-276), eval mode ------------------------------------
 * Y[N,D] = (act(X[N,Dk] . W[D,Dk]^T + bias)) * bn_scale + bn_shift
 * bias / bn_scale / bn_shift may be NULL (absent stage).  bn_* are the folded eval-mode BatchNorm1d:
 * scale = gamma / sqrt(running_var + 1e-5), shift = beta - running_mean * scale.
 * fp32 MFMA; any N, Dk, D >= 1 (16-byte aligned rows take the direct-to-LDS path). */
int laff_fc_act_bn(laff_ctx* ctx, const float* X, int N, int Dk, int ldx, const float* W, int ldw,
                   const float* bias, const float* bn_scale, const float* bn_shift, int D, int act,
                   float* Y, int ldy);

/* The same projection for up to 8 independent features in ONE launch (a3: the per-feature Python loop of
 * VisMutiTransformNet.forward, model/model.py:1807-1827, and the text-side loop :1673-1681). */
typedef struct {
    const float* X; int N, Dk, ldx;
    const float* W; int ldw;
    const float* bias; const float* bn_scale; const float* bn_shift;
    int D, act;
    float* Y; int ldy;
} laff_fc_problem;
int laff_fc_act_bn_grouped(laff_ctx* ctx, const laff_fc_problem* problems /*host array*/, int count);

/* ---- the W2VV++ "concat" towers (VisTransformNet model/model.py:279-308, MultiScaleTxtEncoder + MultiScaleTxtNet :683-726) --------
 * Y[N,D] = (act(sum_s X_s . W[:, col_s : col_s + Dk_s]^T + bias)) * bn_scale + bn_shift          in ONE launch
 * i.e. a1 on torch.cat(X_0 .. X_{n-1}, dim 1) without the concatenated matrix ever existing.  W is [D, K] with rows ldw apart and is
 * read in place at each segment's column window.  A segment is
 *   dense  (X != NULL):  X [N, Dk] fp32, rows ldx >= Dk apart; fp32 MFMA.  16-byte aligned rows (X, ldx, Dk and, for W's window,
 *                        W, ldw, col multiples of 4 floats) take the direct-to-LDS loads, anything else goes through registers;
 *   sparse (X == NULL):  CSR (indptr [N + 1], indices, values | NULL = ones) over Dk columns + Wt = the TRANSPOSED window
 *                        [Dk, ldwt >= D] (one vocabulary entry = one contiguous row, as laff_fc_gather_act_bn takes it); added to the
 *                        same accumulators with fp32 FMAs before bias / activation / BatchNorm.  `indices` are not validated (ids
 *                        outside [0, Dk) contribute nothing); rows may be empty and may repeat a column.
 * fp32-class arithmetic only: there is no 16-bit operand route.  Rows are bitwise independent of the batch they arrive in.
 * Limits: 1 <= nseg <= 8, Dk >= 1, D % 4 == 0, 4 <= D <= 8192, ldy % 4 == 0 and Y / Wt 16-byte aligned, ldwt % 4 == 0, windows inside
 * [0, K) and pairwise disjoint, ldw >= K (LAFF_E_ARG / LAFF_E_SHAPE / LAFF_E_ALIGN before any GPU work).  W may be NULL when every
 * segment is sparse.  N == 0 is a successful no-op.  Allocates nothing, does not synchronise, can be captured in a graph. */
typedef struct {
    const float* X; int ldx;                                      /* dense segment (X == NULL: sparse) */
    const int* indptr; const int* indices; const float* values;   /* sparse segment */
    const float* Wt; int ldwt;
    int Dk;                                                       /* width of the segment */
    int col;                                                      /* first column of its window in W */
} laff_fc_concat_segment;
typedef struct {
    const laff_fc_concat_segment* segments /*host array*/; int nseg;
    int N;
    const float* W; int K, ldw;                                   /* K: columns of W (sum of the widths, or more) */
    const float* bias; const float* bn_scale; const float* bn_shift;
    int D, act;
    float* Y; int ldy;
} laff_fc_concat_problem;
int laff_fc_concat_act_bn(laff_ctx* ctx, const laff_fc_concat_problem* problem);
/* up to 4 problems per launch (both sides' towers of a retrieval run as one launch); more are launched four at a time */
int laff_fc_concat_act_bn_grouped(laff_ctx* ctx, const laff_fc_concat_problem* problems /*host array*/, int count);

/* a1 on the 16-bit matrix pipe with fp32-class accuracy ("fp16x3"): both operands are split once into exact fp16
 * hi + lo parts with a per-row power-of-two scale (laff_split_rows); the GEMM accumulates lo*hi + hi*lo + hi*hi in fp32
 * (fp16 x fp16 products are exact in fp32; the dropped lo*lo term is 2^-22 relative) and the epilogue undoes the scales.
 * 3 MFMA passes at the 2.5 PF fp16 rate instead of one at the 157 TF fp32 rate. */
int laff_split_rows_bytes(int N, int K, size_t* out);            /* bytes of the [2][N][Kp] fp16 operand, Kp = ceil(K/64)*64 */
int laff_split_rows(laff_ctx* ctx, const float* X, int N, int K, int ldx, void* out_hi_lo, float* rscale /*[N]*/);
/* up to 8 matrices in one launch (host arrays of `count` entries) */
int laff_split_rows_grouped(laff_ctx* ctx, int count, const float* const* X, const int* N, const int* K, const int* ldx,
                            void* const* out_hi_lo, float* const* rscale);
typedef struct {
    const void* Xs; const float* x_rscale; int N, Dk;          /* laff_split_rows(X[N,Dk]) */
    const void* Ws; const float* w_rscale;                      /* laff_split_rows(W[D,Dk]) */
    const float* bias; const float* bn_scale; const float* bn_shift;
    int D, act;
    float* Y; int ldy;
} laff_fc_split_problem;
int laff_fc_act_bn_split_grouped(laff_ctx* ctx, const laff_fc_split_problem* problems /*host array*/, int count);

/* The same projection with the INPUT split fused into the GEMM: X stays fp32 in HBM, only its per-row power-of-two scales are
 * computed beforehand (laff_row_scales_grouped: one read of X, N floats out; same scales as laff_split_rows) and the kernel
 * forms the fp16 hi / lo planes on the way into LDS -- laff_split_rows' 2 x N x Kp fp16 planes are never written or re-read.
 * Results are bit-identical to laff_split_rows + laff_fc_act_bn_split_grouped on 256x256 tiles.
 * Needs Dk % 32 == 0, ldx % 4 == 0 and 16-byte aligned X rows; W is split once with laff_split_rows as before. */
int laff_row_scales_grouped(laff_ctx* ctx, int count, const float* const* X, const int* N, const int* K, const int* ldx,
                            float* const* rscale);
typedef struct {
    const float* X; int ldx; const float* x_rscale; int N, Dk;  /* fp32 input + laff_row_scales_grouped(X) */
    const void* Ws; const float* w_rscale;                      /* laff_split_rows(W[D,Dk]) */
    const float* bias; const float* bn_scale; const float* bn_shift;
    int D, act;
    float* Y; int ldy;
} laff_fc_fused_problem;
int laff_fc_act_bn_fused_grouped(laff_ctx* ctx, const laff_fc_fused_problem* problems /*host array*/, int count);

/* Which kernels the three grouped FC entry points above run for a list of problems, in launch order: the answer of the very
 * functions the launches go through (the staging kind of each problem, the grouping by kind and by eight, the 512-big-tile test
 * and the tail split of the split tile, which reads this process's CU count).  Launches nothing, reads no device memory.
 *   family   LAFF_FC_FAMILY_F32 (laff_fc_act_bn_grouped), _SPLIT (laff_fc_act_bn_split_grouped), _FUSED (laff_fc_act_bn_fused_grouped)
 *   shapes   host array; x_aligned / w_aligned stand for 16-byte aligned X / W base pointers (the split operands of the SPLIT
 *            family and Ws of the FUSED one are always aligned; ldx is ignored by SPLIT, ldw by SPLIT and FUSED)
 *   kind     [count] host out: F32: the staging kind 0 / 1 / 2 (registers, LDS-DMA with a K tail, fast LDS-DMA); SPLIT / FUSED:
 *            the tile edge, 128 or 256; -1 for an empty problem (N = 0: in no launch)
 *   launch_of[count] host out: index of the launch that computes the problem, -1 for an empty one
 *   launches [cap] host out, *n_launches of them: the kernel, its problems, its tiles (128 x 128 for F32_* and F16_128, 256 x 256
 *            otherwise) and, for LAFF_FC_KERNEL_X3, the tail split: nbig whole tiles + `quarters` 128 x 128 workgroups (4 per
 *            remaining tile)
 * A problem list the entry point would refuse is refused here with the same code; more than cap launches: LAFF_E_ARG. */
enum { LAFF_FC_FAMILY_F32 = 0, LAFF_FC_FAMILY_SPLIT = 1, LAFF_FC_FAMILY_FUSED = 2 };
enum {
    LAFF_FC_KERNEL_F32_REG = 0,      /* fp32 MFMA, 128 x 128 tiles, operands through registers: unaligned rows / Dk % 4 != 0 */
    LAFF_FC_KERNEL_F32_TAIL = 1,     /* fp32 MFMA, LDS-DMA with a K tail: Dk * 4 % 128 != 0, or an operand span >= 4 GiB     */
    LAFF_FC_KERNEL_F32_GLDS = 2,     /* fp32 MFMA, fast LDS-DMA                                                            */
    LAFF_FC_KERNEL_F16_128 = 3,      /* split operands, 128 x 128 tiles: a launch of < 512 tiles of 256 x 256              */
    LAFF_FC_KERNEL_X3 = 4,           /* split operands, the 256 x 256 hi/lo tile (+ quarter tiles of a sparse last round)   */
    LAFF_FC_KERNEL_X3_FUSED = 5,     /* the same tile with the input split on its way into LDS (any launch size)            */
    LAFF_FC_KERNEL_STRIP = 6,        /* laff_fc_act_bn_strip_grouped, laff_fc_gather_act_bn, laff_fc_concat_act_bn*: one     */
    LAFF_FC_KERNEL_GATHER = 7,       /*   kernel family each; never an answer of laff_fc_route (named for the bindings'      */
    LAFF_FC_KERNEL_CONCAT = 8,       /*   route tables)                                                                      */
    LAFF_FC_KERNEL_F16_256 = 9       /* 16-bit one-plane operands on 256 x 256 tiles: no FC entry point builds such a group   */
};
typedef struct { int N, Dk, D, ldx, ldw; int x_aligned, w_aligned; } laff_fc_shape;
typedef struct { int kernel, count; long long tiles; int nbig; long long quarters; } laff_fc_launch;
int laff_fc_route(laff_ctx* ctx, int family, const laff_fc_shape* shapes /*host*/, int count, int* kind, int* launch_of,
                  laff_fc_launch* launches, int cap, int* n_launches);

/* a1 / a3 in STRIP form for Dk == 512 inputs (TransformNet.forward, model/model.py:257-276; the per-feature loops :1807-1827 and
 * :1673-1681): same arithmetic as the fused-split form above (fp16 hi/lo, three products, fp32 accumulation) with X STATIONARY --
 * a wavefront loads 32 fp32 input rows once, finds their maxima and converts them to hi / lo MFMA fragments in registers (no
 * laff_row_scales_grouped pass, nothing of the split ever in memory); W streams through LDS from an image packed once per model:
 *   laff_fc_strip_pack(W[D,512], bias, bn_scale, bn_shift, act) -> img  (laff_fc_strip_pack_bytes(D) bytes, 16-byte aligned: the hi/lo
 *   fragments of W in LDS order + the per-column epilogue constants with bias, activation and folded BatchNorm pre-combined)
 * Needs Dk == 512, D % 32 == 0, ldx % 4 == 0, 16-byte aligned X; any N, any ldy >= D.  Up to 8 problems per launch; problems of
 * different D or activation kind are launched separately.  |Y - fp64| as the other fp16x3 forms (<= ~1e-6 of the row / weight scale).
 * The kernel exists on two MFMA shapes; LAFF_FC_STRIP_MFMA, read when a ctx is created (process-wide, as LAFF_STRIP), picks: 16 =
 * v_mfma_f32_16x16x32_f16 (default), 32 = v_mfma_f32_32x32x16_f16.  Both laff_fc_strip_pack and laff_fc_act_bn_strip_grouped follow it,
 * and the two image layouts differ (same size): AN IMAGE MUST BE LAUNCHED UNDER THE MODE IT WAS PACKED UNDER -- re-pack after changing
 * the mode.  Results of the two agree to rounding (the MFMA-internal summation order differs), not bit for bit. */
int laff_fc_strip_pack_bytes(int D, int Dk, size_t* out);
int laff_fc_strip_pack(laff_ctx* ctx, const float* W, int ldw, const float* bias, const float* bn_scale, const float* bn_shift, int D,
                       int Dk, int act, void* img);
typedef struct {
    const float* X; int ldx; int N;
    const void* img; int D, act;                                /* laff_fc_strip_pack(...) of this feature's TransformNet */
    float* Y; int ldy;
} laff_fc_strip_problem;
int laff_fc_act_bn_strip_grouped(laff_ctx* ctx, const laff_fc_strip_problem* problems /*host array*/, int count);

/* a1 for a SPARSE input feature (bag-of-words, model/model.py:399-416): X given as CSR (indptr[N+1], indices[nnz],
 * values[nnz] or NULL = all ones) over Dk columns; Wt = W^T [Dk, ldwt >= D] so that one vocabulary entry is one contiguous
 * row.  Y[N,D] = bn(act(sum_j values_j * Wt[indices_j, :] + bias)).  D % 4 == 0, D <= 8192, 16-byte aligned Wt / Y rows. */
int laff_fc_gather_act_bn(laff_ctx* ctx, const int* indptr, const int* indices, const float* values, int N, int Dk,
                          const float* Wt, int ldwt, const float* bias, const float* bn_scale, const float* bn_shift, int D,
                          int act, float* Y, int ldy);

/* ---- 8f-4: training loss -- MarginRankingLoss (loss.py:68-135) per head, summed over heads (model/model.py:2032-2048) ----
 * s = caption embeddings, im = video embeddings, both [B, H, d] fp32 contiguous (H = 1 for a 2-D batch).
 * scores_h = l2norm(im_h) . l2norm(s_h)^T (eps 1e-13, loss.py:30-34); hinge on the margin against the diagonal, row-wise
 * ('i2t'), column-wise ('t2i') or both; max_violation keeps the hardest negative; cost_style sum or mean.
 * Writes loss[0] (device float) and, when non-NULL, the gradients d_s / d_im [B, H, d] of that loss (what autograd gives the
 * reference).  workspace: caller-owned device scratch of laff_margin_loss_workspace_bytes(B, H, d), 16-byte aligned. */
enum { LAFF_LOSS_MAX_VIOLATION = 1, LAFF_LOSS_COST_MEAN = 2, LAFF_LOSS_DIR_I2T = 4, LAFF_LOSS_DIR_T2I = 8 };
int laff_margin_loss_workspace_bytes(int B, int H, int d, size_t* out);
int laff_margin_loss(laff_ctx* ctx, const float* s, const float* im, int B, int H, int d, float margin, unsigned flags,
                     float* loss, float* d_s, float* d_im, void* workspace, size_t workspace_bytes);

/* DualSoftmaxLoss (loss.py:291-310) per head, summed over heads: the criterion of opt.loss == 'dsl' (model/model.py:1992-1993).
 * s, im as above.  M_h = l2norm(s_h) . l2norm(im_h)^T (rows = captions); with A = softmax of M / temp down each column,
 * cal(M) = -sum_i log softmax_row(B * M (.) A)[i][i] and loss_h = (cal(M_h) + cal(M_h^T)) / 2, every softmax taken about its
 * maximum (any temp > 0).  Writes loss[0] and, when non-NULL, d_s / d_im [B, H, d]; with both NULL the call is forward-only and
 * no gradient is formed.  B as laff_margin_loss accepts it, and B == 0 (nothing is touched).  workspace: caller-owned device
 * scratch of laff_dsl_loss_workspace_bytes(B, H, d), 16-byte aligned. */
int laff_dsl_loss_workspace_bytes(int B, int H, int d, size_t* out);
int laff_dsl_loss(laff_ctx* ctx, const float* s, const float* im, int B, int H, int d, float temp, float* loss, float* d_s,
                  float* d_im, void* workspace, size_t workspace_bytes);

/* MarginRankingLossWithScore (loss.py:138-200): the margin ranking loss on a score matrix the caller formed, score [B, ld >= B]
 * fp32 with any row pitch.  cost_s compares along the rows against score[i][i] ('i2t'), cost_im along the columns against
 * score[j][j] ('t2i'), the diagonal cleared; flags are LAFF_LOSS_*.  Writes loss[0] and, when non-NULL, d_score with the pitch of
 * score ([B, ld]; the columns past B are scratch).  B as laff_margin_loss accepts it, and B == 0 (nothing is touched). */
int laff_margin_loss_scores(laff_ctx* ctx, const float* score, int ld, int B, float margin, unsigned flags, float* loss,
                            float* d_score);

/* ---- text tower: the GRU caption encoder (model/model.py:323-396 GruTxtEncoder / BiGruTxtEncoder), inference, one layer ----------
 * torch.nn.GRU arithmetic (gate order r, z, n; h0 = 0) over captions given as token ids, then pooling over each caption's steps:
 *   LAFF_GRU_MEAN      mean of h_t                       -> H columns (bidirectional: forward mean | reverse mean, 2H)
 *   LAFF_GRU_LAST      h at the caption's last token      -> H columns (bidirectional: the forward half only, as the reference)
 *   LAFF_GRU_MEAN_LAST mean | last                        -> 2H columns (unidirectional only; the reference crashes on bigru)
 * The input half is a table lookup: P = we . W_ih^T + b_ih [V, 3H] (build it with laff_fc_act_bn, act none).
 * laff_gru_pack_whh: W_hh [3H, H] contiguous -> the step kernel's layout, 3*H*H floats, 16-byte aligned.
 * laff_gru_encode: the rows are the captions sorted by length, longest first (stable); tokens [T, N] int32 time-major in that order
 * (entries past a row's length are not read), lengths [N] and perm [N] (sorted row -> output row) on the device; batch_sizes [T] is
 * HOST memory: batch_sizes[t] = number of rows with length > t (what torch's PackedSequence holds), batch_sizes[0] = N.
 * One launch per time step (both directions in the same launch); no allocation, no host synchronisation: capturable in a HIP graph.
 * The P_rev / whh_rev / bhh_rev set is read only when bidirectional and pooling is LAFF_GRU_MEAN.  out [N, ldo]: row perm[i] is
 * caption i of the sorted order.  workspace: laff_gru_workspace_bytes(N, H, ...) bytes, 16-byte aligned.
 * Limits: num_layers == 1, H % 32 == 0, 32 <= H <= 2048.  A caption's features do not depend on the rest of its batch (bitwise). */
enum { LAFF_GRU_MEAN = 0, LAFF_GRU_LAST = 1, LAFF_GRU_MEAN_LAST = 2 };
int laff_gru_pack_whh(laff_ctx* ctx, const float* W_hh, int H, float* packed);
int laff_gru_workspace_bytes(int N, int H, int num_layers, int bidirectional, int pooling, size_t* out);
int laff_gru_encode(laff_ctx* ctx, const int* tokens, const int* lengths, const int* perm, const int* batch_sizes /*host*/, int T, int N,
                    int V, int H, int num_layers, int bidirectional, int pooling, const float* P_fwd, const float* whh_fwd,
                    const float* bhh_fwd, const float* P_rev, const float* whh_rev, const float* bhh_rev, float* out, int ldo,
                    void* workspace, size_t workspace_bytes);

/* ---- the GRU caption encoder, differentiable: the training forward and backpropagation through time (fp32, one layer, h0 = 0) ----
 * Packed positions: pos(t, row) = off[t] + row with off the prefix sum of batch_sizes; M = sum of batch_sizes rows in all.
 * laff_gru_gather_rows: X [M, D] = table[ids] (an id outside [0, V) gives a NaN row).  With X = we[tokens in packed order], form
 *   GI = X . W_ih^T + b_ih [M, 3H] per direction with laff_fc_act_bn (act none): the table of this batch only.
 * laff_gru_encode_train: laff_gru_encode with P := GI, V := M and pos [T, N] in place of the tokens (pos[t, row] = off[t] + row for the
 *   active entries; the others are not read).  Same arithmetic, same out.  It also fills reserve (laff_gru_train_reserve_bytes, 16-byte
 *   aligned): per direction the planes r, z, n, q = W_hn h_prev + b_hn and h_prev, [M, H] each, addressed by packed position.
 * laff_gru_pack_whh_t: W_hh [3H, H] -> the backward step's operand layout (the transposed pack), 3*H*H floats, 16-byte aligned.
 * laff_gru_backward: from dout [N, lddo] (the gradient of out, input order) one launch per time step, then the parameter gradients
 *   through laff_fc_backward's launch path and the embedding gradient.  grads_fwd / grads_rev: {dW_ih [3H, we_dim], dW_hh [3H, H],
 *   db_ih [3H], db_hh [3H]} of a direction, HOST arrays of four device pointers, each may be null (not wanted); grads_rev is read only
 *   when bidirectional and pooling is LAFF_GRU_MEAN (under bigru + last the reverse direction has no gradient).  d_we [V, we_dim] or
 *   null: the sum of the rows of dX = dGI . W_ih that share a token, from the token segments seg_off [U + 1], seg_tok [U], seg_pos [M]
 *   (device; distinct token -> its packed positions in ascending order), each segment summed in that order; rows of unused tokens
 *   are zeros.  X is read for dW_ih only, W_ih for d_we only.  workspace: laff_gru_backward_workspace_bytes, 16-byte aligned.
 *   No allocation, no host synchronisation, no atomics: capturable, and two calls give the same bits.
 * laff_gru_backward_plan (host only, no ctx): per launch i in [0, T) whether the saving forward (fwd_big[i]) and the backward
 *   (bwd_big[i]) take the 64 x 32 tile (1) or the 16 x 16 one (0). */
int laff_gru_pack_whh_t(laff_ctx* ctx, const float* W_hh, int H, float* packed);
int laff_gru_gather_rows(laff_ctx* ctx, const float* table, int V, int D, const int* ids, int M, float* X);
int laff_gru_train_reserve_bytes(int M, int H, int num_layers, int bidirectional, int pooling, size_t* out);
int laff_gru_encode_train(laff_ctx* ctx, const int* pos, const int* lengths, const int* perm, const int* batch_sizes /*host*/, int T, int N,
                          int M, int H, int num_layers, int bidirectional, int pooling, const float* GI_fwd, const float* whh_fwd,
                          const float* bhh_fwd, const float* GI_rev, const float* whh_rev, const float* bhh_rev, float* out, int ldo,
                          void* workspace, size_t workspace_bytes, void* reserve, size_t reserve_bytes);
int laff_gru_backward_plan(const int* batch_sizes /*host*/, int T, int H, int bidirectional, int pooling, int* fwd_big, int* bwd_big);
int laff_gru_backward_workspace_bytes(const int* batch_sizes /*host*/, int T, int N, int H, int we_dim, int num_layers, int bidirectional,
                                      int pooling, int want_dwe, size_t* out);
int laff_gru_backward(laff_ctx* ctx, const int* lengths, const int* perm, const int* batch_sizes /*host*/, int T, int N, int M, int H,
                      int we_dim, int num_layers, int bidirectional, int pooling, const float* dout, int lddo, const void* reserve,
                      size_t reserve_bytes, const float* X, const float* wih_fwd, const float* whht_fwd, const float* wih_rev,
                      const float* whht_rev, const int* seg_off, const int* seg_tok, const int* seg_pos, int U, int V, float* d_we,
                      float* const grads_fwd[4] /*host*/, float* const grads_rev[4] /*host*/, void* workspace, size_t workspace_bytes);

/* ---- text tower: the CLIP text encoder (clip.model.CLIP.encode_text, model/clip/model.py:153-206, 245-358), inference -----------
 * token + positional embedding -> layers x ResidualAttentionBlock (pre-LN, causal MHA with head dim 64, QuickGELU MLP of 4 width)
 * -> ln_final -> the row at argmax(ids) -> . text_projection.
 * Captions come RAGGED: caption i is its ids up to and including p_i = argmax(ids_i) (first occurrence: the row the reference pools;
 * <|endoftext|> unless the caption was cut at the context length).  A causal mask keeps the later positions from reaching row p_i,
 * so they are left out.  ids [R] int32 concatenates the captions; row_off [N+1] int32 (row_off[0] = 0, row_off[N] = R, every caption
 * 1 .. context_length rows) is passed TWICE: on the device for the kernels and in HOST memory for the checks (the same values).
 * Weights: the four matrices of every block and text_projection are packed once with laff_clip_pack_weight into the encoder's
 * precision (LAFF_PREC_FP32, or LAFF_PREC_FP16: fp16 operands, fp32 accumulation); in_proj / out_proj / c_fc / c_proj as stored
 * (nn.Linear's [out, in]), text_projection [width, embed] with transpose = 1.  Every other pointer is fp32 on the device.
 * out [N, ldo] fp32: caption i's feature in row i.  workspace: laff_clip_workspace_bytes(R, ...) bytes, 16-byte aligned.
 * Limits: width % 64 == 0, 64 <= width <= 1024, heads * 64 == width, 1 <= context_length <= 77, layers >= 1 (LAFF_E_UNSUPPORTED).
 * No allocation, no host synchronisation: capturable in a HIP graph (one stream, no branches).  A caption's feature does not depend on
 * the rest of its batch (bitwise), so any split of a batch into calls gives the same features. */
typedef struct laff_clip_block {
    const float* ln_1_weight;
    const float* ln_1_bias;
    const void* in_proj_weight;   /* packed [3 width, width] */
    const float* in_proj_bias;
    const void* out_proj_weight;  /* packed [width, width] */
    const float* out_proj_bias;
    const float* ln_2_weight;
    const float* ln_2_bias;
    const void* c_fc_weight;      /* packed [4 width, width] */
    const float* c_fc_bias;
    const void* c_proj_weight;    /* packed [width, 4 width] */
    const float* c_proj_bias;
} laff_clip_block;
typedef struct laff_clip_text {
    int width, layers, heads, embed_dim, context_length, vocab_size;
    const float* token_embedding;       /* [vocab_size, width] */
    const float* positional_embedding;  /* [context_length, width] */
    const laff_clip_block* blocks;      /* HOST array of `layers` blocks (of device pointers) */
    const float* ln_final_weight;
    const float* ln_final_bias;
    const void* text_projection;        /* packed text_projection^T [embed_dim, width] */
} laff_clip_text;
int laff_clip_pack_weight(laff_ctx* ctx, const float* W, int rows, int cols, int transpose, int precision, void* packed);
int laff_clip_workspace_bytes(int R, int N, int width, int precision, size_t* out);
int laff_clip_encode(laff_ctx* ctx, const int* ids, const int* row_off, const int* row_off_host, int N, int R, const laff_clip_text* model,
                     int precision, float* out, int ldo, void* workspace, size_t workspace_bytes);

/* ---- video tower: the CLIP image encoder (clip.model.CLIP.encode_image: VisualTransformer, model/clip/model.py:153-243, 342-343) --
 * Frames [F, 3, R, R] fp32 NCHW (preprocessed as the reference feeds them), g = R / patch_size, L = g^2 + 1 tokens per frame:
 *   x = [class_embedding ; conv1(frame) as g^2 patch rows] + positional_embedding -> ln_pre
 *   -> layers x the text encoder's block (laff_clip_block; full, non-causal attention) -> ln_post(x[class row]) . proj
 * The last block computes queries, out_proj and the MLP for the class rows only (the only rows pooled): exact.
 * Weights: conv1.weight [width, 3, p, p] viewed as [width, 3 p^2] is packed with laff_clip_pack_weight_padded into [width, Kp],
 * Kp = laff_clip_image_kpad(patch_size, precision) (3 p^2 rounded up to 64 halves / 32 floats; the padding is zero and exact);
 * the blocks as for the text encoder; proj [width, embed_dim] with laff_clip_pack_weight(transpose = 1).  Other pointers fp32.
 * out_frames [F, ldo] fp32: frame f's feature in row f.  frame_off [V+1] int32 (frame_off[0] = 0, frame_off[V] = F, every video at
 * least one frame) on the device, and the same values in HOST memory (frame_off_host) for the checks; out_mean [V, ldm] fp32: the mean
 * of video v's frame features, summed in ascending frame order (out_mean may be NULL when V == 0).
 * workspace: laff_clip_image_workspace_bytes(F, ...) bytes, 16-byte aligned.
 * Limits (LAFF_E_UNSUPPORTED): width % 64 == 0, 64 <= width <= 1024, heads * 64 == width, layers >= 1, resolution % patch_size == 0,
 * 2 <= L <= 257 (ViT-B/32, B/16, L/14; L/14@336 with L = 577 is refused); F L <= 4,194,304 token rows per call (LAFF_E_SHAPE).
 * No allocation, no host synchronisation: capturable in a HIP graph.  A frame's feature does not depend on the rest of its batch
 * (bitwise). */
typedef struct laff_clip_visual {
    int width, layers, heads, embed_dim, input_resolution, patch_size;
    const void* conv1_weight;           /* packed [width, Kp] */
    const float* class_embedding;       /* [width] */
    const float* positional_embedding;  /* [L, width] */
    const float* ln_pre_weight;
    const float* ln_pre_bias;
    const laff_clip_block* blocks;      /* HOST array of `layers` blocks (of device pointers) */
    const float* ln_post_weight;
    const float* ln_post_bias;
    const void* proj;                   /* packed proj^T [embed_dim, width] */
} laff_clip_visual;
int laff_clip_pack_weight_padded(laff_ctx* ctx, const float* W, int rows, int cols, int padded_cols, int precision, void* packed);
int laff_clip_image_kpad(int patch_size, int precision, int* out);
int laff_clip_image_workspace_bytes(int F, int width, int input_resolution, int patch_size, int precision, size_t* out);
int laff_clip_image_encode(laff_ctx* ctx, const float* pixels, int F, const int* frame_off, const int* frame_off_host, int V,
                           const laff_clip_visual* model, int precision, float* out_frames, int ldo, float* out_mean, int ldm,
                           void* workspace, size_t workspace_bytes);

/* ---- video tower: frame preprocessing, decoded frames -> the image encoder's pixels (clip._transform, model/clip/clip.py:58-65:
 * Resize(R, BICUBIC), CenterCrop(R), ToTensor, Normalize through torchvision on Pillow; data_provider.py:274-281 the bilinear variant) --
 * frames: F ragged frames as packed HWC uint8 RGB in one buffer of frames_bytes bytes; frame f is `height x width x 3` bytes at byte
 * `offset` of its descriptor (ANY byte offset: the kernel reads bytes).  desc [F] is passed TWICE: on the device for the kernel and in
 * HOST memory (desc_host, the same values) for the checks, like frame_off / frame_off_host above.
 * The resize is Pillow's 8-bit resample bit for bit: horizontal pass -> uint8 -> vertical pass, each
 *   out = clip8((sum_i k_i p_i + 2^21) >> 22)     int32 taps k_i, int32 accumulation, arithmetic shift
 * -- integer multiply-adds only on the device.  The taps come from the caller (laff_amd/frame_prep.py derives them in float64 once
 * per distinct (in, out, filter)), so the filter (bicubic, bilinear, ...) is the caller's choice.  A tap table describes ONE axis of
 * the cropped window, R outputs, as int32 words { K, xmin[R], count[R], taps[K][R] }: output j of the window is
 * sum_{i < count[j]} taps[i][j] * p[xmin[j] + i], 1 <= count[j] <= K, taps[i][j] for i >= count[j] unused.  An axis that is not resized
 * is the identity table (K = 1, xmin[j] = crop + j, taps = 2^22).  htab / vtab of a descriptor are the word indices of the frame's
 * horizontal / vertical table in `taps` (taps_len words; on the device and the same words in HOST memory, taps_host).
 * out_pixels [F, 3, R, R] fp32 = (float(u) / 255.0f - mean[c]) / stdv[c] with true fp32 divides (mean, stdv: host arrays of 3);
 * out_u8 [F, R, R, 3] uint8 (nullable): the resized, cropped image u itself.
 * One launch over (frame, row tile); the uint8 intermediate stays in LDS, so laff_frame_preprocess_workspace_bytes is 0 today and
 * workspace may be NULL (the arguments are kept so that a plan with a workspace does not change the ABI).
 * Limits (LAFF_E_UNSUPPORTED): 1 <= height, width <= 4096; 1 <= R <= 512; F <= 65535 per call; one output row's LDS image,
 * (taps of the row) x R x 3 bytes, at most 65,536 bytes, i.e. a vertical tap count of at most floor(65536 / (3 R)) (97 at R = 224,
 * 42 at R = 512: every short-side resize of a frame up to 4096 px fits, bicubic included).  Every table entry is checked against
 * its frame (xmin >= 0, xmin + count <= width / height; LAFF_E_ARG) before anything is launched.
 * No allocation, no host synchronisation: capturable in a HIP graph.  A frame's output does not depend on the rest of its batch
 * (bitwise). */
typedef struct laff_frame_desc {
    int64_t offset;        /* byte offset of the frame in `frames` */
    int32_t height, width;
    int32_t htab, vtab;    /* word index of the horizontal / vertical tap table in `taps` */
    int32_t reserved[2];   /* 0 */
} laff_frame_desc;
int laff_frame_preprocess_workspace_bytes(int F, int R, size_t* out);
int laff_frame_preprocess(laff_ctx* ctx, const uint8_t* frames, size_t frames_bytes, const laff_frame_desc* desc,
                          const laff_frame_desc* desc_host, int F, int R, const int32_t* taps, const int32_t* taps_host, size_t taps_len,
                          const float* mean, const float* stdv, float* out_pixels, uint8_t* out_u8, void* workspace,
                          size_t workspace_bytes);

/* ---- text tower: the BERT text encoder (BertTxtEncoder.forward: transformers' BertModel pooler_output, model/model.py:437-466) ----
 * Post-LN encoder, inference, eps = layer_norm_eps:
 *   x = LN_emb(word[id] + type[0] + pos[t])
 *   layers x { h = LN_1(x + attention.output.dense(MHA(x)));  x = LN_2(h + output.dense(GELU_erf(intermediate.dense(h)))) }
 *   out = tanh(pooler.dense(x[CLS row]))        (bidirectional MHA with head dim 64, scale 1/8)
 * Captions come RAGGED: caption i is its wordpiece ids [CLS] ... [SEP] without padding.  The reference pads with a key mask that gives
 * padded keys a weight of exactly 0, so each caption's rows equal the unpadded computation.  ids [R] int32 concatenates the captions;
 * row_off [N+1] int32 (row_off[0] = 0, row_off[N] = R, every caption 1 .. max_position rows, at most 512) is passed TWICE: on the
 * device for the kernels and in HOST memory for the checks (the same values).  Caption i's CLS row is row_off[i].
 * The last layer runs its queries, attention output, LayerNorms and feed-forward on the N CLS rows only (K and V from every row).
 * Weights: per layer the query / key / value weights stacked into one [3 width, width] matrix (rows: query, key, value) with its
 * [3 width] bias, attention.output.dense [width, width], intermediate.dense [intermediate, width], output.dense [width, intermediate]
 * and pooler.dense [width, width], each packed once with laff_clip_pack_weight (transpose = 0) into the encoder's precision
 * (LAFF_PREC_FP32, or LAFF_PREC_FP16: fp16 operands, fp32 accumulation, LayerNorm, softmax and residual stream).  Every other
 * pointer is fp32 on the device; token_type_embedding is row 0 of the token-type table.
 * out [N, ldo] fp32: caption i's pooler_output in row i.  workspace: laff_bert_workspace_bytes(R, N, ...) bytes, 16-byte aligned.
 * Limits (LAFF_E_UNSUPPORTED): width % 64 == 0, 64 <= width <= 1024, heads * 64 == width, intermediate % 64 == 0,
 * 1 <= max_position <= 512, layers >= 1; R <= 4,194,304 token rows per call (LAFF_E_SHAPE).
 * No allocation, no host synchronisation: capturable in a HIP graph (one stream, no branches).  A caption's feature does not depend on
 * the rest of its batch (bitwise), so any split of a batch into calls gives the same features. */
typedef struct laff_bert_block {
    const void* qkv_weight;             /* packed [3 width, width]: attention.self.query / key / value weights, stacked */
    const float* qkv_bias;              /* [3 width] */
    const void* attn_out_weight;        /* packed [width, width]: attention.output.dense */
    const float* attn_out_bias;
    const float* ln_1_weight;           /* attention.output.LayerNorm */
    const float* ln_1_bias;
    const void* inter_weight;           /* packed [intermediate, width]: intermediate.dense */
    const float* inter_bias;
    const void* out_weight;             /* packed [width, intermediate]: output.dense */
    const float* out_bias;
    const float* ln_2_weight;           /* output.LayerNorm */
    const float* ln_2_bias;
} laff_bert_block;
typedef struct laff_bert_text {
    int width, layers, heads, intermediate, max_position, vocab_size;
    float layer_norm_eps;
    const float* word_embeddings;       /* [vocab_size, width] */
    const float* position_embeddings;   /* [max_position, width] */
    const float* token_type_embedding;  /* [width]: row 0 of embeddings.token_type_embeddings */
    const float* emb_ln_weight;         /* embeddings.LayerNorm */
    const float* emb_ln_bias;
    const laff_bert_block* blocks;      /* HOST array of `layers` blocks (of device pointers) */
    const void* pooler_weight;          /* packed [width, width] */
    const float* pooler_bias;
} laff_bert_text;
int laff_bert_workspace_bytes(int R, int N, int width, int intermediate, int precision, size_t* out);
int laff_bert_encode(laff_ctx* ctx, const int* ids, const int* row_off, const int* row_off_host, int N, int R, const laff_bert_text* model,
                     int precision, float* out, int ldo, void* workspace, size_t workspace_bytes);

/* ---- text tower: the NetVLAD text encoder (NetVLADTxtEncoder, model/model.py:529-549; NetVLAD.forward, model/Attention.py:862-918) --
 * Per caption, over its word2vec rows x_m: xh_m = x_m / max(|x_m|, 1e-12), a_m = softmax_k(xh_m . fc1_weight[k]) (no bias),
 * u_k = sum_m a_mk xh_m - (sum_m a_mk) centroids[k]; each u_k / max(|u_k|, 1e-12), flattened k-major to K*D values, then the row
 * / max(|row|, 1e-12).
 * Captions come RAGGED: ids [R] int32 (rows of table [V, D]) concatenates the captions' distinct known words; row_off [N+1] int32
 * (row_off[0] = 0, non-decreasing, row_off[N] = R) is passed TWICE: on the device for the kernels and in HOST memory for the checks
 * (the same values).  zero_rows [N] int32 on the device: for a caption without ids, the number of all-zero rows it stands for (the
 * reference's caption whose words are all unknown); ignored for a caption with ids.  A caption with no ids and no zero rows gives a
 * zero row.  fc1_weight and centroids are [K, D] contiguous, read as they are (nothing to pack).
 * out [N, ldo]: caption i's K*D values in row i.  workspace: laff_netvlad_workspace_bytes(R, K) bytes, 16-byte aligned.
 * Limits: 1 <= K <= 64 (LAFF_E_UNSUPPORTED); D % 4 == 0, 4 <= D <= 1024 (LAFF_E_UNSUPPORTED); ldo % 4 == 0; table, centroids, out
 * 16-byte aligned.  An id outside [0, V) makes its caption's row NaN instead of reading past the table.
 * No allocation, no host synchronisation: capturable in a HIP graph.  A caption's row does not depend on the rest of its batch
 * (bitwise). */
int laff_netvlad_workspace_bytes(int R, int K, size_t* out);
int laff_netvlad_encode(laff_ctx* ctx, const float* table, int V, int D, const int* ids, const int* row_off, const int* row_off_host,
                        const int* zero_rows, int N, int R, const float* fc1_weight, const float* centroids, int K, float* out, int ldo,
                        void* workspace, size_t workspace_bytes);

/* ---- the NetVLAD text encoder, differentiable: the saving forward and the gradients of fc1_weight and centroids (fp32) ----------
 * The arguments up to ldo are laff_netvlad_encode's, with its limits and error codes; the word2vec table gets no gradient.
 * laff_netvlad_encode_train: the same out, bit for bit, and reserve (laff_netvlad_train_reserve_bytes(N, R, K) bytes, 16-byte
 *   aligned): the soft assignments [R, K], 1 / max(|x|, eps) [R], per caption max(|u_k|, eps) for every cluster and max(|v|, eps)
 *   [N, K + 1], and which of those norms were clamped [N, K + 1] int32.  The assignments go straight into the reserve, so workspace
 *   is not used: NULL / 0 is fine, a pointer must be 16-byte aligned.
 * laff_netvlad_backward: from out [N, ldo] (the forward's), d_out [N, ldg] (its gradient; ldg % 4 == 0, at least K*D, 16-byte aligned)
 *   and the reserve: d_fc1 [K, D] = sum_r dz_r (x) xh_r and d_centroids [K, D] = - sum_i s_ik du_ik, contiguous and 16-byte aligned;
 *   either may be NULL (not wanted: not formed, not touched).  The clamped norms follow torch: below eps a norm passes no gradient, the
 *   derivative is d / eps.  Every element of a wanted output is written exactly once, zeros included; N = 0 or R = 0 is legal (zeros).
 *   Sums run over token rows / captions in ascending order inside chunks whose boundaries depend on (N, R) alone, then over the chunks in
 *   ascending order: no atomics, two calls give the same bits.  An id outside [0, V) is never read past the table and makes both
 *   gradients NaN.  workspace: laff_netvlad_backward_workspace_bytes(N, R, K, D) bytes, 16-byte aligned.  Three launches.
 * Buffers that are too small are refused by name before any launch.  No allocation, no host synchronisation: capturable. */
int laff_netvlad_train_reserve_bytes(int N, int R, int K, size_t* out);
int laff_netvlad_backward_workspace_bytes(int N, int R, int K, int D, size_t* out);
int laff_netvlad_encode_train(laff_ctx* ctx, const float* table, int V, int D, const int* ids, const int* row_off,
                              const int* row_off_host, const int* zero_rows, int N, int R, const float* fc1_weight,
                              const float* centroids, int K, float* out, int ldo, void* reserve, size_t reserve_bytes, void* workspace,
                              size_t workspace_bytes);
int laff_netvlad_backward(laff_ctx* ctx, const float* table, int V, int D, const int* ids, const int* row_off, const int* row_off_host,
                          const int* zero_rows, int N, int R, const float* fc1_weight, const float* centroids, int K, const float* out,
                          int ldo, const float* d_out, int ldg, const void* reserve, size_t reserve_bytes, float* d_fc1,
                          float* d_centroids, void* workspace, size_t workspace_bytes);

/* ---- a2-a6: stack + Multi_head_MyApply_Attention / Attention_1 / JustAverage ----------------------------
 * (model/model.py:1858-1876, :1663-1705; model/Attention.py:508-531, :78-105)
 * One feature plane per fused feature; nothing is stacked or tiled in memory.
 *   x_l[n, h, c] = act_l( src_l[n, (tile ? c : h*d + c)] ) * scale_l[h*d + c] + shift_l[h*d + c]
 * act (LAFF_ACT_*) lets the producing projection hand over its PRE-activation output (x W^T + b) and leave
 * `tanh -> BatchNorm` of TransformNet (model/model.py:270-275) to this kernel (same v_exp_f32 / v_rcp_f32 arithmetic as the
 * GEMM epilogue: identical bits either way).
 * tile != 0 restates the no-transform branch `x.repeat(1, heads)` + BatchNorm1d(D)
 * (model/model.py:1801-1805, 1822-1823; text side :659-664, 1675-1676): src has d columns. */
typedef struct {
    const float* src;     /* [N, ld] */
    int ld;
    int tile;
    const float* scale;   /* [H*d] or NULL (=1) */
    const float* shift;   /* [H*d] or NULL (=0) */
    int act;              /* LAFF_ACT_* applied to src before the affine (0 = none) */
    /* GATHER plane (src == NULL, wt != NULL): a sparse feature through its FC without materialising the projected plane --
     * value[n, c] = sum_j values[j] * wt[indices[j], c] + bias[c] over the CSR row n (the arithmetic of laff_fc_gather_act_bn),
     * then act and the affine as above.  d <= 512 per head, never tiled. */
    const int* indptr;    /* [N+1] */
    const int* indices;   /* [nnz] */
    const float* values;  /* [nnz] or NULL (all ones) */
    const float* wt;      /* [dk, ldwt] = W^T */
    int ldwt, dk;
    const float* bias;    /* [H*d] or NULL */
    /* optional per-row factor [N] applied after the affine: the inverse row norm of `local_embs = l2norm(local_embs, dim=2)` in the
     * expert-embedding branch (model/model.py:1866-1873, :1686-1694), produced by laff_plane_row_norms; NULL = none.  Not with gather
     * planes. */
    const float* row_scale;
} laff_plane;

/* out[l * N + n] = 1 / (|x_l[n, :]|_2 + 1e-13 + 1e-14) over all H*d columns of plane l as laff_fuse would read it (activation,
 * tiling, affine -- the expert embedding row rides in `shift`): what `l2norm(local_embs, dim=2)` divides by (loss.py:8-13).
 * The planes' own row_scale must be NULL here.  flags: only LAFF_ATT_NO_SPLIT_HEAD matters (d = D columns, one "head"). */
int laff_plane_row_norms(laff_ctx* ctx, const laff_plane* planes /*host array of L*/, int L, int N, int H, int d, unsigned flags,
                         float* out /*[L, N]*/);

/* E[N,H,d] (unit L2 norm per (n,h) unless JUST_AVERAGE).  w [H,d], b [H], gw [H] device arrays.
 * attn_w: optional [N,H,L] softmax weights (the `self.weights` side output, Attention.py:90).
 * L <= 8, d % 4 == 0.  With NO_SPLIT_HEAD every head reads columns [0,d) (d = D). */
int laff_fuse(laff_ctx* ctx, const laff_plane* planes /*host array of L*/, int L, int N, int H, int d,
              const float* w, const float* b, const float* gw, unsigned flags, float* E, float* attn_w);

/* Backward of laff_fuse over PLAIN DENSE planes (no activation, tiling, folded affine, gather or row_scale: in training those are
 * upstream ops with their own autograd).  x / dx: HOST arrays of L device pointers with their row pitches ldx / lddx (elements), so the
 * L slices of a stacked (N, L, H*d) tensor and of its gradient are used in place.  Split heads: plane l holds x_l[n, h*d + c]; with
 * LAFF_ATT_NO_SPLIT_HEAD every head reads columns [0, d) and dx_l is the sum over the heads.  dE [N, lde >= H*d] is the gradient of
 * laff_fuse's E.  The forward is recomputed from the planes (nothing else is saved) and
 *   dx_l [N, lddx_l]  the gradient of every plane, always written;
 *   dw [H, d]         the gradient of w (NULL: not formed), a deterministic two-stage sum over the rows;
 *   db [H]            zeros (softmax does not see a shift of its logits); NULL: not written.
 * gw gets no gradient (the reference reads it through .item(), model/Attention.py:96).  LAFF_ATT_JUST_AVERAGE: dx_l = dE / L, dw = 0.
 * No atomics: two calls on the same inputs give the same bits.  No allocation, no host synchronisation; ordered on the ctx's stream.
 * workspace: caller-owned device scratch of laff_fuse_backward_workspace_bytes(L, N, H, d, flags), 16-byte aligned; only read when dw
 * is given.  Limits as laff_fuse: 1 <= L <= 8, d % 4 == 0, rows 16-byte aligned (pitches % 4 == 0); N == 0 touches nothing. */
int laff_fuse_backward_workspace_bytes(int L, int N, int H, int d, unsigned flags, size_t* out);
int laff_fuse_backward(laff_ctx* ctx, const float* const* x /*host array of L device pointers*/, const int* ldx /*host, L row pitches*/,
                       int L, int N, int H, int d, const float* w /*[H,d]*/, const float* b /*[H]*/, const float* gw /*[H]*/,
                       unsigned flags /*LAFF_ATT_*/, const float* dE /*[N, lde >= H*d]*/, int lde,
                       float* const* dx /*host array of L device pointers*/, const int* lddx /*host, L pitches*/,
                       float* dw /*[H,d], nullable*/, float* db /*[H], nullable*/, void* workspace, size_t workspace_bytes);

/* ---- multi-head self-attention fusion (Multi_head_MyApply_selfAttention, model/Attention.py:317-470) ------------------------- */
/* the token list of a group (row n, head h): the L planes' head slices, optionally with one token in front (T = L + 1) */
enum { LAFF_SA_PREPEND_NONE = 0, LAFF_SA_PREPEND_MAX = 1 /* elementwise max over l */, LAFF_SA_PREPEND_MEAN = 2 /* mean over l */ };
/* what is returned of the T outputs o_i */
enum {
    LAFF_SA_POOL_MEAN = 0,   /* mean over i */
    LAFF_SA_POOL_MAX = 1,    /* elementwise max over i */
    LAFF_SA_POOL_TOKEN = 2,  /* o_token, 0 <= token < T: first / last / second / third and the prepending types */
    LAFF_SA_POOL_ALL = 3     /* every o_i, a stacked (N, L, H*d) tensor (the Attention_1 output type); no prepended token */
};

/* The block over PLAIN DENSE planes, fp32.  x: HOST array of L device pointers with row pitches ldx (elements): plane l holds
 * x_l[n, h*d + c], so the slices of a stacked (N, L, H*d) tensor are read in place.  Per group (n, h), with the tokens u_i of the
 * `prepend` rule:
 *   t_i = u_i / (|u_i| + 1e-13 + 1e-14)  with LAFF_ATT_L2NORM_EACH_HEAD (the only flag read), else u_i
 *   A = softmax_j(s t_i . t_j),  s = (d / H) ^ -0.5 with the INTEGER quotient (Attention.py:402), so d >= H
 *   r_i = sum_j A_ij t_j + t_i;   o_i = gamma (.) (r_i - mean r_i) / sqrt(var r_i + 1e-5) + beta   (biased variance; gamma, beta [d]
 *   are shared by all heads)
 * and E [N, lde >= H*d] receives the pooled rows, or, with LAFF_SA_POOL_ALL, O receives o_l at O[n * ldon + l * ldol + h*d + c].
 * Maxima (LAFF_SA_PREPEND_MAX, LAFF_SA_POOL_MAX): the LOWEST index wins a tie -- a `>` comparison in ascending index; the backward
 * routes the gradient to that index.
 * Backward: recomputes the forward from the planes (nothing else is saved); dE [N, lde] is the gradient of E, or dO that of O in the
 * same stacked layout.  Writes
 *   dx_l [N, lddx_l]    the gradient of every plane, always (through the prepended token and the normalisation as well);
 *   dgamma, dbeta [d]   each on request (NULL: not formed): a deterministic two-stage sum over rows and heads through the workspace.
 * No atomics: two calls give the same bits.  No allocation, no host synchronisation; ordered on the ctx's stream, capturable.
 * workspace: caller-owned device scratch of out[0] bytes of laff_selfattn_fuse_backward_plan, 16-byte aligned, only used when dgamma
 * or dbeta is given.  laff_selfattn_fuse_backward_plan (host only, no ctx): out = {workspace bytes, partial rows = blocks of the launch}.
 * Limits: 1 <= L <= 8, d % 4 == 0, 4 <= d <= 512, H >= 1, H*d <= 8192, d >= H, 16-byte aligned bases, pitches % 4 == 0.  N == 0
 * touches nothing, except zeros to dgamma / dbeta when they are given. */
int laff_selfattn_fuse_backward_plan(int N, int H, int d, int out[2]);
int laff_selfattn_fuse(laff_ctx* ctx, const float* const* x /*host array of L device pointers*/, const int* ldx /*host, L row pitches*/,
                       int L, int N, int H, int d, const float* gamma /*[d]*/, const float* beta /*[d]*/, int prepend /*LAFF_SA_PREPEND_*/,
                       int pool /*LAFF_SA_POOL_*/, int token, unsigned flags, float* E /*[N, lde], pooled*/, int lde,
                       float* O /*stacked, LAFF_SA_POOL_ALL*/, int ldon, int ldol);
int laff_selfattn_fuse_backward(laff_ctx* ctx, const float* const* x, const int* ldx, int L, int N, int H, int d, const float* gamma,
                                const float* beta, int prepend, int pool, int token, unsigned flags, const float* dE, int lde,
                                const float* dO, int ldon, int ldol, float* const* dx /*host array of L device pointers*/,
                                const int* lddx /*host, L pitches*/, float* dgamma /*[d], nullable*/, float* dbeta /*[d], nullable*/,
                                void* workspace, size_t workspace_bytes);

/* Backward of the FC projection A = act(X W^T + bias), the forward laff_fc_act_bn computes without a BatchNorm stage; fp32 MFMA.
 * X [N, ldx >= Dk], W [D, ldw >= Dk], A [N, lda >= D] the SAVED forward output, dA [N, ldda >= D] its gradient.  With
 *   dZ = dA (.) act'(A)      tanh: 1 - A^2   sigmoid: A (1 - A)   relu: A > 0   none: 1
 * the call writes whichever outputs are given (each may be NULL):
 *   dX [N, lddx >= Dk] = dZ W        (reads W, not X)
 *   dW [D, lddw >= Dk] = dZ^T X      (reads X, not W)
 *   db [D]             = sum_n dZ[n, :]
 * dZ is formed while dA and A are loaded and never stored.  Any N >= 0, Dk, D >= 1 and any pitch >= the width; rows that start on
 * 16-byte boundaries (base and pitch % 4 == 0) are read with 16-byte loads, others element by element.  Pointers 4-byte aligned.
 * N == 0: dW and db are set to zero, nothing else is touched.  Where the output tiles alone would not fill the chip a sum is cut into
 * chunks that depend on (N, Dk, D) only: the sum over N of dW and db (1 chunk for N <= 128), the sum over D of dX (1 for D <= 128).
 * With more than one the partial tiles go to `workspace` (16-byte aligned) and are added in chunk order.  No atomics: two calls give
 * the same bits.  No allocation, no host synchronisation; ordered on the ctx's stream, capturable.
 * laff_fc_backward_plan (host only, no ctx): out = {chunks of the dW / db sum, workspace bytes, chunks of the dX sum, tile variants:
 * bit 0 dW and bit 1 dX on 128 x 128 tiles, else 64 x 64}.  The chunks do not depend on want_dx / want_dw; the workspace bytes cover
 * dX's partial tiles with want_dx, dW's and db's with want_dw, and db's alone in any case. */
int laff_fc_backward_plan(int N, int Dk, int D, int want_dx, int want_dw, int out[4]);
int laff_fc_backward(laff_ctx* ctx, const float* X, int N, int Dk, int ldx, const float* W, int ldw, int D, int act /*LAFF_ACT_*/,
                     const float* A, int lda, const float* dA, int ldda, float* dX, int lddx, float* dW, int lddw, float* db,
                     void* workspace, size_t workspace_bytes);

/* Backward of the same projection for a SPARSE X [N, Dk] (the bag-of-words; forward laff_fc_gather_act_bn without a BatchNorm stage, or
 * a CSR segment of laff_fc_concat_act_bn).  A [N, lda >= D] is the SAVED forward output, dA [N, ldda >= D] its gradient, dZ as above:
 *   dW [D, lddw >= Dk]:  dW[d, v] = sum over the entries (n, v) of X of x[n, v] dZ[n, d]      (W's own layout, not the transposed one)
 *   db [D]             = sum_n dZ[n, :]                                                        (there is no dX: counts)
 * X comes in TRANSPOSED (CSC): colptr [Dk + 1] and rows [nnz] int32, values [nnz] fp32 or NULL for all ones; column v owns the entries
 * [colptr[v], colptr[v + 1]), in ascending row order.  A repeated row index inside a column adds up; an entry whose row lies outside
 * [0, N) contributes nothing; entries outside every column's range are never read.  D % 4 == 0, 4 <= D <= 8192; A and dA 16-byte aligned
 * with lda % 4 == ldda % 4 == 0; dW and db 4-byte aligned, any lddw >= Dk.  Either output may be NULL.  The one launch writes EVERY
 * element of the window [D, Dk] of dW and only those (+0.0 in a column without entries; no memset in front), so a call can fill a
 * column window at any offset of a wider gradient.  dW's base and pitch 16-byte aligned and Dk % 4 == 0: 16-byte stores, else 4-byte
 * ones, same bits.  Every element of dW is one fmaf chain over its column's entries in their order, db is summed in an order fixed by
 * N: no atomics, two calls give the same bits.  N == 0 or nnz == 0: dW is set to zero and the pattern is not read (db is zero for
 * N == 0, the sum otherwise).  No workspace, no allocation, no host synchronisation; ordered on the ctx's stream, capturable. */
int laff_fc_gather_backward(laff_ctx* ctx, const int* colptr, const int* rows, const float* values, int nnz, int N, int Dk, int D,
                            int act /*LAFF_ACT_*/, const float* A, int lda, const float* dA, int ldda, float* dW, int lddw, float* db);

/* Backward of the concat layer A = act(sum_s X_s . W[:, col_s : col_s + Dk_s]^T + bias), the forward laff_fc_concat_act_bn computes
 * without a BatchNorm stage; fp32.  A [N, lda >= D] is the SAVED forward output, dA [N, ldda >= D] its gradient, dZ as above.  W is
 * [D, ldw >= K] and dW ONE gradient [D, lddw >= K]; each may be NULL, as may db and every dX:
 *   dW[:, col_s : col_s + Dk_s] = dZ^T X_s     every DENSE segment in ONE launch, X_s read in place, the window written in place: every
 *                                              element of a window exactly once, nothing outside the windows
 *   db [D] = sum_n dZ[n, :]                    once per call: by the dense launch, or by the first CSR segment's when all are CSR
 *   dX_s [N, lddx >= Dk_s] = dZ W[:, window]   every dense segment with dX != NULL in ONE launch, W read in place at the window
 * The segments come as parallel host arrays of nseg entries, segment s being dense (nnz[s] < 0) or sparse (nnz[s] >= 0 entries):
 *   widths[s] = Dk_s, cols[s] = col_s                         both kinds
 *   X[s] [N, ldx[s] >= Dk_s], dX[s] [N, lddx[s] >= Dk_s]      dense (dX[s] NULL: not wanted; X[s] is read for dW only)
 *   colptr[s], rows[s], values[s] (NULL = ones), nnz[s]       sparse: the TRANSPOSED pattern, exactly as laff_fc_gather_backward takes
 *                                                             it; that kernel is issued on the segment's window, one launch each.  A
 *                                                             dX on a sparse segment is refused (counts).
 * (one array per field and no struct: the header's structs are a pinned list, tests/test_cabi.py.)  An array whose kind of segment
 * does not occur may be NULL.  The dense products run laff_fc_backward's tile body on v_mfma_f32_32x32x2_f32: an element is one fmaf
 * chain in k order, and with the same cut it has the bits of laff_fc_backward on the window.  The sum over N of dW and db is not cut at
 * N <= 128; beyond that, and for the sum over D of dX, the cut depends on (N, D, the dense widths) only; partial tiles go to
 * `workspace` (16-byte aligned) and are added in chunk order.  No atomics: two calls give the same bits.  No allocation, no host
 * synchronisation; ordered on the ctx's stream, capturable.
 * Limits, refused by name before any GPU work (a NULL ctx is looked at last): 1 <= nseg <= 8, Dk >= 1, windows inside [0, K) and pairwise
 * disjoint, D % 4 == 0, 4 <= D <= 8192, lddw >= K, a workspace of at least the plan's bytes; pointers 4-byte aligned, and with a sparse
 * segment A / dA 16-byte aligned with lda % 4 == ldda % 4 == 0.  N == 0: the windows of dW and db are set to zero, nothing else is touched.
 * laff_fc_concat_backward_plan (host only, no ctx): widths[s] = Dk_s, kinds[s] = bit 0 sparse | bit 1 dX wanted;
 * out = {chunks of the dW / db sum, workspace bytes, chunks of the dX sum, tile variants: bit 0 dW and bit 1 dX on 128 x 128 tiles}.
 * The bytes come back as an int: a shape whose workspace exceeds INT_MAX bytes is refused by the plan (LAFF_E_SHAPE). */
int laff_fc_concat_backward_plan(int N, int D, const int* widths /*host*/, const int* kinds /*host*/, int nseg, int want_dw, int out[4]);
int laff_fc_concat_backward(laff_ctx* ctx, int nseg, const int* widths /*host*/, const int* cols /*host*/, const int* nnz /*host*/,
                            const float* const* X /*host array of device pointers*/, const int* ldx /*host*/,
                            float* const* dX /*host array of device pointers*/, const int* lddx /*host*/,
                            const int* const* colptr /*host array*/, const int* const* rows /*host array*/,
                            const float* const* values /*host array*/, int N, const float* W, int K, int ldw, int D, int act /*LAFF_ACT_*/,
                            const float* A, int lda, const float* dA, int ldda, float* dW, int lddw, float* db, void* workspace,
                            size_t workspace_bytes);

/* The stage between a projection's activation and its output in training mode (model/model.py:236-243 under .train()): dropout by a
 * counter-based mask, then BatchNorm1d on the batch's statistics; fp32.  A [N, lda >= D] is the activation output.
 *   m[n,c]  = keep(seed, n, c) / (1 - p)     (1 when p == 0: no generator call, seed may be NULL);   U = A (.) m
 *   mean[c] = sum_n U / N      var[c] = sum_n (U - mean)^2 / N (biased)      invstd = 1 / sqrt(var + eps)
 *   Y [N, ldy >= D] = gamma (U - mean) invstd + beta;     save_mean [D] = mean, save_invstd [D] = invstd
 *   running_mean = (1 - momentum) running_mean + momentum mean;   running_var likewise with var N / (N - 1); both updated in place
 * gamma == NULL: no BatchNorm stage, Y = U, no statistics are formed, none of beta / running_* / save_* is read or written.
 * The mask: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (c >> 2, n, 0, 0); element (n, c) takes output word c & 3 and
 * is kept iff word >= (uint32) floor(p * 4294967296.0).  One round: (hi0, lo0) = mulhilo32(0xD2511F53, c0), (hi1, lo1) =
 * mulhilo32(0xCD9E8D57, c2), c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), then k0 += 0x9E3779B9, k1 += 0xBB67AE85; ten rounds.  n and c are
 * the logical row and column: pitch and base address do not enter.  seed: DEVICE pointer to one 64-bit word, read by the kernels (a
 * captured call sees whatever the word holds at replay).  A kept element is A * fp32(1 / (1 - p)), a dropped one +0.0.
 * The variance is the corrected two-pass form on the strip a block keeps in registers; the per-column arithmetic behind the sums runs
 * in float64 and is rounded to fp32 once (Y is formed from the mean's fp32 head and tail; save_mean is the head).  N <= 256: one launch, A is read once.  Larger N: the rows are cut into chunks of 256, each
 * chunk's (mean, M2) goes to `workspace` as float64 and a second launch merges them in chunk order and normalises.
 * Backward: dY [N, lddy >= D], A, p, seed, gamma, save_mean, save_invstd as the forward had and left them; the mask is recomputed.
 *   xhat = (U - mean) invstd      dbeta [D] = sum_n dY      dgamma [D] = sum_n dY (.) xhat
 *   dU   = gamma invstd (dY - dbeta / N - xhat dgamma / N)      (dU = dY without a BatchNorm stage)      dA [N, ldda >= D] = dU (.) m
 * Each of dA, dgamma, dbeta may be NULL (not formed); the others do not change by it.
 * Any D >= 1 and any pitch >= D; bases 4-byte aligned (seed 8-byte).  Rows on 16-byte boundaries (bases, pitches, D % 4 == 0) take the
 * kernels with 16-byte accesses, anything else the element-wise ones: same bits.  No atomics: two calls with one seed give the same
 * bits.  No allocation, no host synchronisation; ordered on the ctx's stream, capturable.  workspace: 16-byte aligned, bytes of the plan.
 * Refused before any GPU work (a NULL ctx is looked at last): N < 0 or D < 1 (LAFF_E_SHAPE); p outside [0, 1), p > 0 with a NULL
 * seed, p == 0 with gamma == NULL (nothing to do), N < 2 with a BatchNorm stage (one value per channel has no variance; N == 0
 * included), eps <= 0, momentum outside [0, 1] (LAFF_E_ARG).  N == 0 without a BatchNorm stage touches nothing.
 * laff_dropout_bn_train_plan (host only, no ctx): out = {row chunks of the column sums (1 without a BatchNorm stage), workspace bytes,
 * launches per direction, rows of a chunk}. */
int laff_dropout_bn_train_plan(int N, int D, int has_bn, int out[4]);
int laff_dropout_bn_train(laff_ctx* ctx, const float* A, int N, int D, int lda, double p, const unsigned long long* seed /*device*/,
                          const float* gamma /*[D], nullable*/, const float* beta /*[D]*/, float* running_mean /*[D]*/,
                          float* running_var /*[D]*/, double momentum, double eps, float* Y, int ldy, float* save_mean /*[D]*/,
                          float* save_invstd /*[D]*/, void* workspace, size_t workspace_bytes);
int laff_dropout_bn_train_backward(laff_ctx* ctx, const float* dY, int lddy, const float* A, int N, int D, int lda, double p,
                                   const unsigned long long* seed /*device*/, const float* gamma /*[D], nullable*/,
                                   const float* save_mean /*[D]*/, const float* save_invstd /*[D]*/, float* dA /*nullable*/, int ldda,
                                   float* dgamma /*[D], nullable*/, float* dbeta /*[D], nullable*/, void* workspace, size_t workspace_bytes);

/* Training-mode BatchNorm1d(H C) over a feature tiled H times, X.repeat(1, H): the no-transform feature of the LAFF towers
 * (TransformNet(fc=False, batch_norm=True)); fp32.  X [N, ldx >= C]; the tiled input is never formed.  The H copies of a column share
 * their batch statistics, which are formed once per input column:
 *   mean[c] = sum_n X / N      var[c] = sum_n (X - mean)^2 / N (biased)      invstd = 1 / sqrt(var + eps)
 *   Y [N, ldy >= H C]:  Y[n, hC+c] = gamma[hC+c] (X[n,c] - mean[c]) invstd[c] + beta[hC+c];   save_mean [C] = mean, save_invstd [C] = invstd
 *   running_mean [H C], running_var [H C]: channel hC+c updated in place as laff_dropout_bn_train updates it (unbiased variance)
 * Backward: dY [N, lddy >= H C], X, gamma, save_mean, save_invstd as the forward had and left them.
 *   xhat = (X - mean) invstd      dbeta[hC+c] = sum_n dY[n,hC+c]      dgamma[hC+c] = sum_n dY[n,hC+c] xhat[n,c]
 *   dU_h = gamma_h invstd (dY_h - dbeta_h / N - xhat dgamma_h / N)      dX [N, lddx >= C] = sum_h dU_h, h ascending
 * Each of dX, dgamma, dbeta may be NULL (not formed); the others do not change by it.
 * The arithmetic and the summation order are those of laff_dropout_bn_train: Y, running_mean, running_var, dgamma and dbeta are
 * bit-identical to laff_dropout_bn_train / _backward with p = 0 on the materialised X.repeat(1, H), and save_mean[c] / save_invstd[c]
 * equal that run's entries hC+c for every h.  N <= 256: one launch per direction; larger N: chunks of 256 rows, float64 partials in
 * `workspace`, a second launch merges them in chunk order.
 * Any C >= 1 and any pitches; bases 4-byte aligned.  Rows on 16-byte boundaries (bases, pitches, C % 4 == 0) take the kernels with
 * 16-byte accesses, anything else the element-wise ones: same bits.  No atomics: two calls give the same bits.  No allocation, no host
 * synchronisation; ordered on the ctx's stream, capturable.  workspace: 16-byte aligned, bytes of the plan (both directions).
 * Refused before any GPU work (a NULL ctx is looked at last): H < 1, C < 1 or N < 0 (LAFF_E_SHAPE); N < 2, NULL gamma, eps <= 0,
 * momentum outside [0, 1] (LAFF_E_ARG).
 * laff_tile_bn_train_plan (host only, no ctx): out = {row chunks, workspace bytes, launches per direction, rows of a chunk}. */
int laff_tile_bn_train_plan(int N, int C, int H, int out[4]);
int laff_tile_bn_train(laff_ctx* ctx, const float* X /*[N, ldx >= C]*/, int N, int C, int ldx, int H, const float* gamma /*[H*C]*/,
                       const float* beta /*[H*C]*/, float* running_mean /*[H*C]*/, float* running_var /*[H*C]*/, double momentum, double eps,
                       float* Y /*[N, ldy >= H*C]*/, int ldy, float* save_mean /*[C]*/, float* save_invstd /*[C]*/, void* workspace,
                       size_t workspace_bytes);
int laff_tile_bn_train_backward(laff_ctx* ctx, const float* dY /*[N, lddy >= H*C]*/, int lddy, const float* X, int N, int C, int ldx, int H,
                                const float* gamma, const float* save_mean, const float* save_invstd, float* dX /*[N, lddx >= C], nullable*/,
                                int lddx, float* dgamma /*[H*C], nullable*/, float* dbeta /*[H*C], nullable*/, void* workspace,
                                size_t workspace_bytes);

/* The expert stage of a LAFF tower in training mode (model/model.py:1848-1873, :1653-1694 of the reference): the expert embedding added
 * to each of the L projected planes and `l2norm(local_embs, dim=2)` after it, written as the stacked tensor the fusion reads in place.
 * One launch for all L planes; fp32.  x: HOST array of L device pointers, x[l] [N, ldx[l] >= D] (ldx a HOST array), D = H d columns.
 * expert [L, lde >= D] or NULL; l2norm 0 / 1; both off is refused (the towers never ask for a plain copy).
 *   v = x[l][n, :] + expert[l, :]   (x without expert)        r = 1 / (sqrt(sum_c v^2) + 1e-13 + 1e-14)   (as laff_plane_row_norms)
 *   Y: element (n, l, c) at n ldn + l ldl + c:  v r, or v without l2norm;      rnorm [L][N] = r  (only with l2norm)
 * Backward: dY in Y's layout (the fusion backward's gradient of the stacked tensor, in place), x, expert, rnorm as the forward had and
 * left them.  With s = sqrt(sum_c v^2) and g = dY[n, l, :]:
 *   dv = r g - v (r^2 / s) (v . g), the second term 0 where s == 0;  dv = g without l2norm
 *   dx[l] [N, lddx[l] >= D] = dv  (every plane, HOST arrays as x / ldx)      d_expert [L, D] dense, or NULL = sum_n dv
 * d_expert is a two-stage sum: each block of the backward launch adds the dv of its 16 rows in ascending order and stores the partial
 * to `workspace` ([blocks][L][D] floats), a second small launch adds the partials in block order.  The block count depends on N only.
 * No atomics: two calls give the same bits.  No allocation, no host synchronisation; ordered on the ctx's stream, capturable (the
 * pointer and pitch arrays are read on the host at the call).  N == 0 touches nothing, except d_expert = 0.
 * Refused before any GPU work (a NULL ctx is looked at last): L outside [1, 8], D % 4 != 0, D < 4, D > 8192, N < 0, a pitch below D,
 * stacked pitches that overlap (LAFF_E_SHAPE); no expert and no l2norm, a NULL array / plane / stacked tensor, l2norm without rnorm,
 * d_expert without expert, a workspace below the plan's bytes when d_expert is asked (LAFF_E_ARG); a base that is not 16-byte aligned
 * or a pitch that is no multiple of 4 floats (LAFF_E_ALIGN).
 * laff_expert_stage_train_plan (host only, no ctx): out = {blocks of the backward launch per plane, workspace bytes}. */
int laff_expert_stage_train_plan(int N, int L, int D, int out[2]);
int laff_expert_stage_train(laff_ctx* ctx, const float* const* x /*host [L]*/, const int* ldx /*host [L]*/, int N, int L, int D,
                            const float* expert /*[L, lde >= D], nullable*/, int lde, int l2norm, float* Y, int ldn, int ldl,
                            float* rnorm /*[L][N], with l2norm*/);
int laff_expert_stage_train_backward(laff_ctx* ctx, const float* dY, int ldn, int ldl, const float* const* x /*host [L]*/,
                                     const int* ldx /*host [L]*/, int N, int L, int D, const float* expert, int lde, int l2norm,
                                     const float* rnorm, float* const* dx /*host [L]*/, const int* lddx /*host [L]*/,
                                     float* d_expert /*[L, D], nullable*/, void* workspace, size_t workspace_bytes);

/* The optimizer step: the global L2 norm of a list of gradients, the clip by it, and Adam / RMSprop with that clip folded in.
 * A tensor list is `count` flat fp32 device tensors of n[i] >= 0 elements, each base 4-byte aligned (nothing stronger is assumed; a
 * launch whose bases are all 16-byte aligned runs the variant with 16-byte accesses).  Pointer arrays and n are HOST arrays.
 *   laff_grad_sqnorm   leaves float64 partial sums of g*g in `workspace` (8-byte aligned, bytes >= 8 * partials of the plan);
 *   laff_grad_scale    total = sqrt(sum of the partials), c = min(1, max_norm / (total + 1e-6)) in float64, c rounded to fp32 once (a NaN
 *                      total gives a NaN c); g *= c in place; (float)total to total_norm_out (device, nullable).  This is
 *                      torch.nn.utils.clip_grad_norm_ with norm_type 2 and error_if_nonfinite=False;
 *   laff_optim_step    the same c when max_norm > 0 (else c = 1, workspace and total_norm_out are not touched), then per element in fp32,
 *                      one rounding per operation, in torch's order:  gh = c g;  gh += weight_decay p  when weight_decay != 0;
 *                        Adam:     m = m + (gh - m)(1 - beta1);  v = beta2 v + ((1 - beta2) gh) gh;
 *                                  p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)),  bc = 1 - beta^step
 *                        RMSprop:  s = alpha s + ((1 - alpha) gh) gh;  p = p - lr (gh / (sqrt(s) + eps))     (momentum 0, not centered)
 *                      with 1 - beta, bc1, bc2 formed in float64 on the host and rounded to fp32 once.  g is NOT written.  total_norm_out
 *                      is stored when max_norm > 0 and at least one tensor is not empty.
 * The norm of a step is over whatever list laff_grad_sqnorm was given (all parameter groups); laff_optim_step may then be called once
 * per group with the same workspace and `partials`.  No atomics: every block re-sums the partials in index order, two calls give the
 * same bits.  The tensor table travels in the launch arguments: no allocation, no copy, no host synchronisation; ordered on the ctx's
 * stream, capturable.  Refused before any GPU work: null pointers with n > 0, n < 0, unknown kind, step < 1, beta outside [0, 1),
 * eps < 0, weight_decay < 0 (LAFF_E_ARG), a workspace too small (LAFF_E_ARG), misaligned pointers (LAFF_E_ALIGN).  n == 0 entries and
 * count == 0 are accepted and do nothing.
 * laff_optim_plan (host only, no ctx): out = {elements of a chunk, tensors of one launch's table, norm launches, partials (workspace =
 * 8 * partials bytes), update launches, blocks a launch has at most}.  laff_optim_last_launches (host only): the launches the calling
 * thread's last laff_grad_sqnorm / laff_grad_scale / laff_optim_step issued, out = {16-byte variant, single-float variant}. */
enum { LAFF_OPT_ADAM = 0, LAFF_OPT_RMSPROP = 1 };
typedef struct { float* p; const float* g; float* s1; float* s2; long long n; } laff_optim_tensor;  /* s2 NULL for RMSprop */
typedef struct { int kind /*LAFF_OPT_*/; double lr, beta1, beta2 /*alpha for RMSprop in beta2*/, eps, weight_decay; long long step; } laff_optim_hyper;
int laff_optim_plan(int count, const long long* n, int out[6]);
int laff_optim_last_launches(int out[2]);
int laff_grad_sqnorm(laff_ctx* ctx, int count, const float* const* g, const long long* n, void* workspace, size_t bytes);
int laff_grad_scale(laff_ctx* ctx, int count, float* const* g, const long long* n, double max_norm, const void* workspace, int partials,
                    float* total_norm_out);
int laff_optim_step(laff_ctx* ctx, const laff_optim_tensor* t /*host array*/, int count, const laff_optim_hyper* h,
                    double max_norm /*<= 0: no clipping*/, const void* workspace, int partials, float* total_norm_out /*nullable*/);

/* laff_fuse that ALSO emits the single-plane 16-bit similarity operand E16[N, H*d] = E * prescale (LAFF_PREC_FP16 or
 * LAFF_PREC_BF16), saving the separate laff_pack_rows pass.  E is already unit-norm per (n,h) to fp32 rounding, so the
 * re-normalisation loss.cosine_sim applies (loss.py:33) is a no-op at 16-bit precision. */
int laff_fuse_packed(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, const float* w, const float* b,
                     const float* gw, unsigned flags, float* E, float* attn_w, void* E16, int precision, float prescale);

/* laff_fuse_packed that ALSO does laff_rank_prepare's work for its rows (split heads of d <= 512): the wavefront that has just produced a
 * row measures the rounding error of the operand it emits (band) and, on the text side, scores the row exactly against its
 * ground-truth video -- the 235 MB that laff_rank_prepare reads back at 40k x 10k are never read.  Two launches, videos first:
 *   side 2 (video rows): band = band_v [((N + 3) & ~3) + ceil(N / 64)], per-column values written;
 *   side 1 (text rows) : band = band_t [N]; Ev / Nv / band_v = the video side's E, row count and band_v (its 64-column block maxima
 *                        are completed here: N * 16 >= Nv); s_gt64 [N] (-inf where gt_col - col0 is outside [0, Nv)), count [N]
 *                        cleared, the header of `pairs` cleared.
 * What the exact-rank pipeline needs afterwards is exactly what laff_rank_prepare leaves behind: laff_sim_gemm_banded and
 * laff_rank_resolve follow unchanged; s_gt64 has the arithmetic of laff_rank_resolve's re-score (equal rows give bit-equal scores).
 * LAFF_E_UNSUPPORTED for shapes this path does not cover (d > 512, unsplit heads, no operand): call laff_rank_prepare instead. */
typedef struct laff_rank_side {
    int side;
    const int* gt_col;
    int col0;
    const float* Ev;
    int Nv;
    double* s_gt64;
    float* band;
    float* band_v;
    int* count;
    unsigned* pairs;
    double* partials;      /* H > 1: scratch [N][H][2] (the per-head terms of a row come from several workgroups; the last arrival sums them */
    unsigned* tickets;     /*        in head order: the arithmetic of laff_rank_resolve's re-score); [N], cleared by the call */
} laff_rank_side;
int laff_fuse_packed_rank(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, const float* w, const float* b,
                          const float* gw, unsigned flags, float* E, float* attn_w, void* E16, int precision, float prescale,
                          const laff_rank_side* rs /* NULL: plain laff_fuse_packed */);

/* ---- a7: per-video frame attention of VisMutiTransformNetPlusFrameFeat (model/model.py:2163-2173) --------
 * V[B,d] = Attention_1 over the Fmax frames of each video; frames[B,Fmax,d] zero padded.
 * lens != NULL: frames >= lens[b] are known zeros and are accounted for analytically (they still take
 * part in the softmax and in mean_L exactly as in the reference, whose mask slice is a no-op);
 * lens == NULL: all Fmax frames are read (needed behind vis_frame_addFC, where padding becomes the bias). */
int laff_frame_fuse(laff_ctx* ctx, const float* frames, const int* lens, int B, int Fmax, int d,
                    const float* w /*[d]*/, const float* b /*[1]*/, const float* gw /*[1]*/, unsigned flags,
                    float* V);
/* the frame features of one tower (same B / Fmax / d / flags / lens, own frames, attention parameters and output) in ONE
 * launch: host arrays of `count` device pointers (gw may be NULL without WITH_AVE) */
int laff_frame_fuse_grouped(laff_ctx* ctx, int count, const float* const* frames, const int* lens, int B, int Fmax, int d,
                            const float* const* w, const float* const* b, const float* const* gw, unsigned flags,
                            float* const* V);
/* the same, fed with the reference's mask_tensor (model/model.py:2156-2160: fp32 (B, ldm >= Fmax), ones for the frames a video has,
 * then zeros) instead of lens: lens[b] = round(sum_f mask[b][f]) is taken inside the launch -- `mask.sum(dim=1).int()` as two
 * framework launches in front of this one was 15 us of a 0.47 ms pass (C3) */
int laff_frame_fuse_grouped_mask(laff_ctx* ctx, int count, const float* const* frames, const float* mask, int ldm, int B, int Fmax,
                                 int d, const float* const* w, const float* const* b, const float* const* gw, unsigned flags,
                                 float* const* V);

/* Backward of laff_frame_fuse_grouped: `count` frame features of one tower (same B / Fmax / d / flags / lens), up to 8 per launch, more
 * in further launches.  Host arrays of `count` device pointers: frames [B, Fmax, d], w [d], b [1], gw [1] (the array may be NULL without
 * WITH_AVE), dV [B, lddv >= d] the gradient of V, dframes [B, Fmax, d], dw [d] and db [1] (either array may be NULL: not formed).
 * lens [B] device int32 or NULL (all Fmax frames real).  The forward is recomputed from the frames (nothing else is saved):
 *   dframes   rows below lens[b]: the gradient; rows at or past it: zeros (the frames there are never read, whatever they hold);
 *             a video with lens[b] == 0 (V = 0) gets zero rows and adds nothing to dw;
 *   dw        a deterministic two-stage sum over the videos: one partial row per (feature, video) in `workspace`, added per feature in a
 *             fixed order by a second small launch; identically zero at Fmax == 1;
 *   db        zeros (softmax does not see a shift of its logits).
 * gw gets no gradient (the reference reads it through .item(), model/Attention.py:96).  No atomics: two calls give the same bits.  No
 * allocation, no host synchronisation; ordered on the ctx's stream, capturable.  workspace: caller-owned device scratch, 16-byte
 * aligned, count * B * d * 4 bytes (laff_frame_fuse_backward_plan), only used when dw is given.
 * Limits: d % 4 == 0, 4 <= d <= 1024, Fmax >= 1, lddv >= d and lddv % 4 == 0 (LAFF_E_SHAPE), flags within WITH_AVE | MUL (LAFF_E_ARG),
 * 16-byte aligned bases (LAFF_E_ALIGN); all refused before any GPU work.  B == 0 or count == 0 touches nothing.
 * laff_frame_fuse_backward_plan (host only, no ctx): out = {workspace bytes, kernel variant = the 256-column chunks a lane owns (1, 2 or
 * 4 for d <= 256 / 512 / 1024), launches of the main kernel (ceil(count / 8)), partial rows of dw per feature (B; 0 without dw)}. */
int laff_frame_fuse_backward_plan(int count, int B, int Fmax, int d, int want_dw, int out[4]);
int laff_frame_fuse_backward(laff_ctx* ctx, int count, const float* const* frames, const int* lens /*NULL: all Fmax*/, int B, int Fmax,
                             int d, const float* const* w, const float* const* b, const float* const* gw /*may be NULL without WITH_AVE*/,
                             unsigned flags, const float* const* dV, int lddv, float* const* dframes, float* const* dw /*may be NULL*/,
                             float* const* db /*may be NULL*/, void* workspace, size_t workspace_bytes);

/* ---- a8: loss.l2norm (loss.py:8-13) + operand packing for the similarity GEMM ---------------------------
 * For each (n,h): y = x / (||x||_2 + eps + 1e-14) if normalize, then y * prescale, converted to `precision`.
 * out layout: FP32 -> float [N, H*d]; FP16/BF16 -> 16-bit [N, H*d]; *X3 -> two planes [2][N, H*d] (hi, lo).
 * laff_packed_bytes gives the size. */
int laff_packed_bytes(int N, int K, int precision, size_t* out);
int laff_pack_rows(laff_ctx* ctx, const float* E, int N, int H, int d, int lde, int normalize, float eps,
                   float prescale, int precision, void* out);

/* ---- a9-a11: loss.cosine_sim + W2VVPP.get_txt2vis_matrix (loss.py:30-34, model/model.py:1003-1016) ------
 * S[Nt,Nv] = scale * T[Nt,K] . V[Nv,K]^T on operands produced by laff_pack_rows (K = H*d, scale = 1/(H*prescale^2)).
 * S may be NULL when only ranks are wanted.  If gt_col != NULL the epilogue also accumulates
 *   count[t] += #{ v : v + col0 != gt_col[t] and S[t,v] > s_gt[t] }   (count must be zeroed by the caller)
 * which is the argsort/label loop of predictor.py:232-244 in count form.  Any K (even for 16-bit
 * operands); K bytes a multiple of 128 takes the fast direct-to-LDS path, other sizes the generic staging paths. */
int laff_sim_gemm(laff_ctx* ctx, const void* T, const void* V, int Nt, int Nv, int K, float scale,
                  int precision, float* S, int lds, const int* gt_col, int col0, const float* s_gt,
                  int* count);

/* The kernel ("route") that laff_sim_gemm / laff_sim_gemm_banded run for a problem, chosen from the shape, the K bytes, the
 * precision, the epilogue and this process's LAFF_STRIP mode and CU count (read when a ctx is created).  Launches nothing.
 * lds: score row pitch in floats, 0 = no scores (a non-zero lds stands for a 16-byte aligned S); count_mode: 0 = none,
 * 1 = the approximate fused count (gt_col + s_gt), 2 = the banded count (pair_cap slots).  *route = one of LAFF_ROUTE_*. */
enum {
    LAFF_ROUTE_TILED128_REG = 0,     /* 128 x 128 tiles, operands staged through registers: K bytes % 16 != 0      */
    LAFF_ROUTE_TILED128_TAIL = 1,    /* 128 x 128 tiles, LDS-DMA with a K tail: K bytes % 128 != 0, or an operand span >= 4 GiB */
    LAFF_ROUTE_TILED128 = 2,         /* 128 x 128 tiles, fast LDS-DMA: fp32, and 16-bit problems of < 512 tiles of 256 x 256 */
    LAFF_ROUTE_TILED256 = 3,         /* 256 x 256 tiles, 8 waves: 16-bit, >= 512 big tiles                        */
    LAFF_ROUTE_TILED256_LONGK = 4,   /* 256 x 256 tiles, 4 waves: 16-bit one plane, >= 4096 big tiles, K bytes >= 8192 */
    LAFF_ROUTE_X3 = 5,               /* the hi/lo split tile: FP16X3 / BF16X3, >= 512 big tiles                   */
    LAFF_ROUTE_STRIP = 6             /* the K = 512 strip kernel (sim_strip.hip)                                   */
};
int laff_sim_gemm_route(laff_ctx* ctx, int Nt, int Nv, int K, int precision, int lds, int count_mode, unsigned pair_cap, int* route);

/* Ground-truth pre-pass for the fused count: s_gt[t] = scale * <T[t], V[gt_col[t]-col0]> on the packed operands
 * (fp32 accumulation of the same 16-bit products), -inf when that column is outside [0,Nv).  When laff_sim_gemm is
 * then called with gt_col/s_gt it writes exactly this value at S[t, gt] so counts and S stay consistent.
 * 16-bit precisions only.  zero_count (nullable, [Nt]) is cleared on the way: it is the accumulator the fused count of
 * laff_sim_gemm adds into (saves a fill launch). */
int laff_row_dot_gt(laff_ctx* ctx, const void* T, const void* V, int Nt, int Nv, int K, float scale, int precision,
                    const int* gt_col, int col0, float* s_gt, int* zero_count);

/* Host-side helper (no device work, any thread): owner[t] = position in the video id list of the prefix of caption id t before its first
 * '#' -- the match predictor.py:241 makes per query (`txt_id.split('#')[0]` looked up in vis_ids).  Both id lists arrive as one UTF-8 blob
 * each, ids separated by '\n', no trailing separator (ids must not contain '\n').  LAFF_E_SHAPE + message when a video id occurs twice
 * or a caption names a video that is not there. */
int laff_match_ids(const char* txt_blob, size_t txt_bytes, int n_txt, const char* vis_blob, size_t vis_bytes, int n_vis, int* owner /*host*/);

/* laff_rank_prepare for ONE side of a sharded pass (laff_amd/dist.py 'video16': the 16-bit text operand is what is all-gathered, the
 * fp32 text rows stay with their owner):
 *   sides = 1, text rows : s_gt64 [Nt] = the exact score of every text against Ev[gt_col - col0] (-inf outside [0, Nv)), band_t [Nt],
 *                          count cleared, list header cleared.  Ev = the fp32 video rows present (V, band_v untouched, may be NULL);
 *   sides = 2, video rows: band_v [((Nv + 3) & ~3) + ceil(Nv / 64)] (Et, T, gt_col, s_gt64, band_t untouched, may be NULL). */
int laff_rank_prepare_part(laff_ctx* ctx, int sides, const float* Et, const float* Ev, const void* T, const void* V, int Nt, int Nv, int H,
                           int d, int precision, float prescale, const int* gt_col, int col0, double* s_gt64, float* band_t, float* band_v,
                           int* zero_count, unsigned* pairs);

/* laff_rank_prepare that PRODUCES one or both GEMM operands on the way (emit: 1 = T, 2 = V, 3 = both): E16 = fp16 / bf16 (E * prescale),
 * no re-normalisation -- what laff_pack_rows(normalize = 0) writes for rows that are unit-norm already (the towers' outputs; gathered
 * embedding rows of a sharded pass, laff_amd/dist.py): one launch and one pass over those rows instead of two.  The operand not named in
 * `emit` is read as in laff_rank_prepare.  Single-plane 16-bit precisions only (LAFF_E_UNSUPPORTED otherwise). */
int laff_rank_prepare_emit(laff_ctx* ctx, int emit, const float* Et, const float* Ev, void* T, void* V, int Nt, int Nv, int H, int d,
                           int precision, float prescale, const int* gt_col, int col0, double* s_gt64, float* band_t, float* band_v,
                           int* zero_count, unsigned* pairs);

/* The listed pairs of a video shard's laff_sim_gemm_banded, exported to the owners of the TEXT rows instead of re-scored here (the exact
 * re-score needs the fp32 text row).  bounds [world + 1] (device): owner o holds text rows [bounds[o], bounds[o + 1]).  out: `world`
 * buckets of `cap` slots {row - bounds[o], col + col0}, unused slots 0xffffffff (the call fills them); fill [world + 1]: pairs per
 * bucket, [world] = 1 if a bucket overflowed (then count[0] is poisoned like an overflowing list).  Behind a 4-word header
 * {0, 0, n_slots, 4} any concatenation of buckets is a list laff_rank_resolve reads.  S (optional): the ground-truth entries take
 * the exact score, as laff_rank_resolve would write them.  predictor.py:232-244 is the loop this pipeline replaces. */
int laff_rank_export_pairs(laff_ctx* ctx, const double* s_gt64, int* count, float* S, int lds, int Nv, unsigned* pairs, unsigned pair_cap,
                           const int* bounds /*device*/, int world, int col0, unsigned* out, unsigned cap, unsigned* fill);

/* ---- a12 made EXACT on a reduced-precision GEMM ------------------------------------------------------------------------------
 * The reference ranks come from fp32 scores (predictor.py:232-244 on model/model.py:1003-1016).  A 16-bit MFMA pass keeps the
 * scores inside the 1e-4 contract but not the ranks, so the fused count is done against a PROVEN error band and the few pairs
 * inside the band are re-scored exactly.  exact(t, v) = (1/H) sum_h <t_h, v_h> / ((|t_h| + eps)(|v_h| + eps)), eps = 1e-13 + 1e-14
 * (loss.py:8-13, 30-34), evaluated in fp64 on the fp32 embeddings; rank = 1 + #{v != gt : exact(t, v) > exact(t, gt)}.
 *
 *   laff_rank_prepare      Et [Nt, H, d], Ev [Nv, H, d]: the fp32 embeddings (rows 16-byte aligned, d % 4 == 0); T, V: the GEMM
 *                          operands made from them (laff_pack_rows / laff_fuse_packed; `precision`, `prescale` as given there).
 *                          Writes s_gt64[t] = exact(t, gt_col[t] - col0) (-inf when that column is outside [0, Nv): another
 *                          shard owns it -- all-reduce MAX the doubles), band_t [Nt] and band_v with
 *                          |S_gemm(t, v) - exact(t, v)| <= band_t[t] + band_v[v]  (measured operand rounding error of both rows by
 *                          Cauchy-Schwarz + the fp32 accumulation bound; behind the per-column values, from offset (Nv + 3) & ~3:
 *                          the maximum of every aligned block of 64 columns, which is what the GEMM epilogue uses -- band_v holds
 *                          ((Nv + 3) & ~3) + ceil(Nv / 64) floats), clears zero_count [Nt] (nullable) and the pair-list header.
 *   laff_sim_gemm_banded   (gt_col, s_gt64, band_t, band_v: 16-byte aligned and readable up to the next multiple of 16 bytes -- the
 *                          kernel fetches them in 16-byte groups by LDS-DMA.)  laff_sim_gemm whose fused count is exact-decidable: count[t] += #{v != gt : S > s_gt + band}, pairs with
 *                          |S - s_gt| <= band are listed in `pairs` (uint32: header {n_extra, overflow, A, w} then pair_cap x
 *                          {row, col}, col shard-local: A slots in per-wavefront segments of w slots -- valid pairs first, unused
 *                          slots have row 0xffffffff -- then n_extra pairs appended by wavefronts whose segment was too small);
 *                          S (nullable) receives (float)s_gt64 at the ground-truth entry -- from the tiled kernels; the K = 512
 *                          strip kernel (LAFF_ROUTE_STRIP) stores its own score there and lists the entry, and laff_rank_resolve
 *                          writes (float)s_gt64 over it.
 *   laff_rank_resolve      re-scores the listed pairs: count[row] += exact > s_gt64[row]; S (nullable) takes the fp32 value of the
 *                          exact score (one ulp above (float)s_gt64 where rounding would hide a strict inequality) so that ranks
 *                          recounted from S equal count + 1.  pair_cap is used in whole groups of four slots (rounded down, >= 4).
 *                          More than pair_cap pairs: pairs[1] = 1 and count[0] is poisoned with -(2^26) -- negative even after an
 *                          int32 all-reduce SUM over <= 16 shards -- which trips the rank < 1 flag of laff_rank_metrics*.
 * After laff_rank_resolve (and an all-reduce SUM of count when videos are sharded) count + 1 are the exact ranks. */
int laff_rank_prepare(laff_ctx* ctx, const float* Et, const float* Ev, const void* T, const void* V, int Nt, int Nv, int H, int d,
                      int precision, float prescale, const int* gt_col, int col0, double* s_gt64, float* band_t, float* band_v,
                      int* zero_count, unsigned* pairs);
int laff_sim_gemm_banded(laff_ctx* ctx, const void* T, const void* V, int Nt, int Nv, int K, float scale, int precision, float* S,
                         int lds, const int* gt_col, int col0, const double* s_gt64, const float* band_t, const float* band_v,
                         int* count, unsigned* pairs, unsigned pair_cap);
int laff_rank_resolve(laff_ctx* ctx, const float* Et, const float* Ev, int Nt, int Nv, int H, int d, const double* s_gt64,
                      int* count, float* S, int lds, unsigned* pairs, unsigned pair_cap);
/* laff_rank_resolve and laff_rank_metrics[_async](count, base) in ONE launch, for passes in which nothing (no all-reduce of the counts)
 * comes between them: the workgroup of the resolve launch that finishes last turns the final counts into ranks (ranks_out, nullable:
 * count + base) and the seven metrics of evaluation.eval (/root/reference/evaluation.py:92-109) -- the label loop + eval of
 * predictor.py:232-246 end in the same kernel that settles the last rank.  out8 (host): 7 metrics + flag as laff_rank_metrics_async.
 *   synchronous == 0: returns at once; when out8 is pinned host memory (hipHostMalloc / hipHostRegister) the device writes it
 *                     directly -- valid after the stream (or the graph the call was captured in) has completed --, otherwise a 64-byte
 *                     copy is queued behind the launch.  Capturable (call it once eagerly first: the ctx allocates its result slots then).
 *   synchronous != 0: waits for the stream; LAFF_E_ARG when the flag is set (a rank < 1: overflowed pair list).
 * The fp64 mean of reciprocals is summed in this one workgroup's fixed order: equal to laff_rank_metrics to rounding (1e-16). */
int laff_rank_resolve_metrics(laff_ctx* ctx, const float* Et, const float* Ev, int Nt, int Nv, int H, int d, const double* s_gt64,
                              int* count, float* S, int lds, unsigned* pairs, unsigned pair_cap, int base, int* ranks_out,
                              double* out8 /*host*/, int synchronous);

/* s_gt[t] = S[t, gt_col[t]-col0] if that column is in [0,Nv) else -inf  (shard-local ground-truth score) */
int laff_gather_gt(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* gt_col, int col0,
                   float* s_gt);
/* count[t] (+)= #{ v in [0,Nv) : v + col0 != gt_col[t] and S[t,v] > s_gt[t] }; accumulate != 0 adds. */
int laff_rank_count(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* gt_col, int col0,
                    const float* s_gt, int* count, int accumulate);
/* Video-to-text direction (predictor.py:262-270): for every text t with owner video gt_col[t]:
 *   count[t] = #{ t' != t : S[t', v] > S[t, v] },  v = gt_col[t] - col0 in [0,Nv)  (others untouched).
 * grp_off[Nv+1] / grp_idx[Nt]: CSR of texts grouped by owner column (local). */
int laff_v2t_count(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* grp_off,
                   const int* grp_idx, int max_group, int* count);

/* The same count made EXACT on the outputs of the exact-rank pipeline (replaces the column argsort of /root/reference/predictor.py:262-270
 * with positions that do not depend on the operand precision of the GEMM):
 *   count[t] = #{ t' != t : exact(t', v) > exact(t, v) },  exact() = the fp64 cosine of the fp32 embeddings (laff_rank_prepare).
 * S must be what laff_sim_gemm_banded (+ laff_rank_resolve) wrote for these operands: every entry within band_t[t'] + band_v[v] of
 * exact(t', v).  Entries further than that from a caption's threshold s_gt64[t] are decided on S; the others are listed as {t', v, t}
 * (3 words each behind a 4-word header {entries wanted, overflow flag, 0, 0}; list_cap entries) and re-scored in fp64 from Et / Ev.
 * count [Nt] is overwritten (0 for texts whose video is not a column of this S).  list[1] != 0 afterwards: the list was too small,
 * count is not valid -- call again with list_cap >= list[0]. */
int laff_v2t_count_exact(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* grp_off, const int* grp_idx,
                         int max_group, const float* Et, const float* Ev, int H, int d, const double* s_gt64,
                         const float* band_t, const float* band_v, int* count, unsigned* list, unsigned list_cap);

/* ---- result lists (predictor.txt2video_write_to_file, predictor.py:53-88): for every row the K best columns, score
 * descending (ties: larger column first = a stable ascending argsort read backwards), instead of a full-matrix argsort.
 * idx_out [Nt,K] int32, val_out [Nt,K] fp32.  1 <= K <= min(Nv, 8192); the row (4 Nv bytes) + 8 K' bytes (K' = K rounded up to
 * 64 / 512 / 2048 / 4096 / 8192) must fit 160 KiB of LDS: wider collections are split by columns and the per-block lists merged with a
 * second call (laff_amd.ops.topk_rows does; LAFF_E_UNSUPPORTED says how many columns fit). */
int laff_topk_rows(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, int K, int* idx_out, float* val_out);

/* ---- retrieval post-processing: k-reciprocal re-ranking (model/ReRank.py:19-104, Zhong et al., CVPR 2017) -------------------------
 * P independent problems per call; a problem is one candidate set given as three SIMILARITY blocks by pointer and pitch: qq [Q, Q],
 * qg [Q, G], gg [G, G] (gg need not be symmetric), N = Q + G items.  The N x N matrix is never concatenated.  All arithmetic fp32:
 *   orig = 2 - 2 [[qq, qg], [qg^T, gg]];  D[i, j] = orig[j, i] / max_k orig[k, i]  (IEEE division)
 *   rank[i] = the k1 + 1 smallest entries of D[i, :], ascending (ties: lower index)
 *   R(i, k) = { j in rank[i][0..k] : i in rank[j][0..k] };  kh = round_half_even(k1 / 2)
 *   E(i) = R(i, k1) + every R(c, kh), c in R(i, k1), with |R(c, kh) & R(i, k1)| > 2/3 |R(c, kh)|  (a set, ascending)
 *   V[i, e] = exp(-D[i, e]) / sum over E(i);  k2 != 1: V[i] <- mean of V[rank[i][0..k2)]
 *   m[i, j] = sum_k min(V[i, k], V[j, k]);  out[i, g] = (1 - m / (2 - m)) (1 - lambda) + D[i, Q + g] lambda   for i < Q, j = Q + g
 * out [Q, ldo] of every problem receives its Q x G block.  workspace: laff_rerank_workspace_bytes(problems, P, k1, k2) bytes, 256-byte
 * aligned; per problem it holds the neighbour lists and the sparse rows of V before and after the query expansion, about
 * 8 N (min(cap, N) + min(k2 cap, N)) bytes with cap = (k1 + 1)(kh + 2) -- 42 MB at N = 3001, k1 = 20, k2 = 6.
 * Limits (LAFF_E_UNSUPPORTED): 1 <= k1 <= 32, 1 <= k2 <= min(8, k1 + 1), Q >= 1, G >= 1, k1 + 1 <= N <= 4096.
 * No allocation, no host synchronisation; problems run 16 to a launch set of four kernels.  A problem's result does not depend on
 * the problems it is batched with (bitwise). */
typedef struct laff_rerank_problem {
    const float* qq; long long ldqq;
    const float* qg; long long ldqg;
    const float* gg; long long ldgg;
    float* out;      long long ldo;
    int Q, G;
} laff_rerank_problem;
int laff_rerank_workspace_bytes(const laff_rerank_problem* problems /*host array; Q and G are read*/, int P, int k1, int k2, size_t* out);
int laff_rerank_run(laff_ctx* ctx, const laff_rerank_problem* problems /*host array*/, int P, int k1, int k2, float lambda_value,
                    void* workspace, size_t workspace_bytes);
/* re_ranking_tkb_simple (model/ReRank.py:107-159) after the two top-K passes (laff_topk_rows): nn [G, k1] int32 = the k1 best columns
 * of every gg row, cand [Q, K] int32 = the K best columns of every qg row.  count [G] int32 receives 1 + the number of rows of nn
 * that hold the column (a histogram pass); out [Q, ldo] receives log(count + 1) at each row's candidate columns and 0 in its other
 * G - K columns.  The caller L2-normalises the rows (loss.l2norm).  An index outside [0, G) is skipped. */
int laff_rerank_tkb(laff_ctx* ctx, const int* nn, int G, int k1, const int* cand, int Q, int K, int* count, float* out, int ldo);

/* ---- the 'hist' measure: generalised Jaccard / histogram intersection (loss.py:43-65, evaluation.py:19-41) ------------------------
 *   S[t, v] = (1 / H) sum_h J(T[t, h, :], V[v, h, :]),   J(x, y) = sum_k min(x_k, y_k) / (sum_k max(x_k, y_k) + eps)
 * the mean over heads of the per-head measure, as the reference's 3-D get_txt2vis_matrix takes it (model/model.py:1008-1014); H = 1 is
 * the plain 2-D case.  T [Nt, H d] and V [Nv, H d] fp32 with row pitches ldt, ldv >= H d; S [Nt, Nv] fp32 with row pitch lds >= Nv,
 * columns Nv .. lds-1 are not written.  Pointers and pitches need 4-byte alignment only (16-byte loads are used where base, pitch and
 * head width allow them; the result does not depend on it).  eps >= 0 is added to the union of every head before the division;
 * eps = 0 gives IEEE results (0 / 0 = NaN, as evaluation.hist_sim).  Inputs may be negative.  Both sums are accumulated in fp32 in
 * one fixed order (no atomics: bitwise reproducible).
 * Refused before any GPU work (LAFF_E_ARG / LAFF_E_SHAPE, the message names the value): null T / V / S when Nt Nv > 0, Nt < 0, Nv < 0,
 * H < 1, d < 1, H d beyond int, ldt / ldv < H d, lds < Nv, eps < 0 or NaN.  Nt == 0 or Nv == 0: returns 0, launches nothing. */
int laff_sim_hist(laff_ctx* ctx, const float* T, long ldt, const float* V, long ldv, int Nt, int Nv, int H, int d, float eps, float* S,
                  long lds);

/* ---- a13: evaluation.eval (evaluation.py:92-109) for single-GT rows ---------------------------------------
 * rank[i] = r[i] + base must be >= 1: pass 1-based ranks with base = 0, or the counts of better-scoring videos that
 * laff_sim_gemm / laff_rank_count produce with base = 1; ranks_out (nullable, [Nq] device) receives the ranks.
 * out7 (host) = r1, r5, r10, medr, meanr, mir, mAP.  Reduced on the device (one small kernel), 56 bytes copied back;
 * synchronises the stream. */
int laff_rank_metrics(laff_ctx* ctx, const int* r, int Nq, int base, int* ranks_out, double out7[7]);
/* Same, without synchronising: out8 is PINNED HOST memory (8 doubles: the 7 metrics + an error flag, 1.0 if a rank < 1 was
 * seen -- the 7 metrics are then NaN -- else 0.0); valid once the stream has been synchronised.  Capturable in a HIP graph.
 * The device writes a pinned (device-addressable) buffer directly from the kernel; any other host pointer gets a 64-byte copy queued
 * behind the launch. */
int laff_rank_metrics_async(laff_ctx* ctx, const int* r, int Nq, int base, int* ranks_out, double* out8_pinned_host);

/* ---- t: a training batch gathered from a device-resident training set in ONE launch (no counterpart in the reference: its
 * PairDataset / collate_pair, data_provider.py:92-152, :621-698, read and stack a batch item by item on the host) -----------------
 * Runs 1 .. LAFF_ASSEMBLE_MAX_JOBS copy jobs over the same B batch rows.  Sources are resident device arrays of 4-byte elements.
 * Every per-batch integer sits in ONE int32 control block [control_len], passed TWICE: on the device for the kernel and in HOST
 * memory for the checks (the same values; the caller uploads it once per batch).  A job names where in the block its integers start.
 *   LAFF_ASSEMBLE_ROWS    dst[b, 0:w] = src[row[b], 0:w]: src [n_src, ld_src >= w], dst [B, ld_dst >= w], row = control + rows_at [B],
 *                         every row[b] in [0, n_src) (a source row may repeat).  Any w >= 1.
 *   LAFF_ASSEMBLE_RAGGED  src [n_items, ld_src >= w] holds n_src segments, segment g the rows [off_src[g], off_src[g + 1]) (off_src
 *                         [n_src + 1] int32 on the device); seg = control + rows_at [B] in [0, n_src).  dst [B, fmax, w] contiguous:
 *                         the first min(len, fmax) rows of segment seg[b], then zeros up to fmax >= 1; a padded row is not read from the
 *                         source.  mask (nullable) [B, fmax] fp32: 1 for a copied row, 0 for a padded one.  Several jobs over the same
 *                         segments give the same mask: pass it to the first and NULL to the others.
 *   LAFF_ASSEMBLE_CSR     the source CSR has n_src rows and n_items entries: off_src = crow_src [n_src + 1], col_src (int32), src =
 *                         val_src (4-byte values).  row = control + rows_at [B]; crow_dst = control + crow_at [B + 1], non-decreasing from
 *                         crow_dst[0] >= 0 with crow_dst[B] <= cap_dst (the entries col_dst and dst = val_dst hold).  The entries of source
 *                         row row[b] go to [crow_dst[b], crow_dst[b + 1]); a range longer than the source row is filled with zeros, a
 *                         shorter one takes the row's first entries.  Empty rows and crow_dst[B] == 0 are legal.
 * The job chooses its access width: 16 bytes a lane where src, dst and both pitches are 16-byte aligned (ragged: w % 4 == 0 too),
 * with the last w % 4 elements of a row copied one by one; 4 bytes a lane otherwise (any 4-byte aligned window of a wider matrix).
 * Every destination element is written exactly once, plain loads and stores, no atomics: two calls give the same bits.  An index read
 * from DEVICE memory (the device copy of control, off_src) that points outside its source is never followed: that row comes out as
 * zeros.  Limits: 1 <= B <= 4096; at most LAFF_ASSEMBLE_MAX_JOBS jobs; a destination of 2^31 elements or more (B * ld_dst,
 * B * fmax * w) is refused by name (LAFF_E_SHAPE); sources are addressed in 64 bits.  All refusals come before the launch, the NULL ctx
 * last.  No allocation, no host synchronisation: capturable in a HIP graph. */
enum { LAFF_ASSEMBLE_ROWS = 0, LAFF_ASSEMBLE_RAGGED = 1, LAFF_ASSEMBLE_CSR = 2 };
#define LAFF_ASSEMBLE_MAX_JOBS 16
#define LAFF_ASSEMBLE_MAX_BATCH 4096
typedef struct laff_assemble_job {
    int kind;               /* LAFF_ASSEMBLE_* */
    int rows_at;            /* index in control of this job's B source indices */
    int crow_at;            /* CSR: index in control of crow_dst [B + 1] */
    int w;                  /* rows, ragged: elements of a row */
    int ld_src;             /* rows, ragged: pitch of src in elements */
    int ld_dst;             /* rows: pitch of dst in elements */
    int n_src;              /* rows: rows of src; ragged: segments; CSR: rows of the source */
    int n_items;            /* ragged: rows of src; CSR: entries of the source */
    int fmax;               /* ragged: rows of a padded batch row */
    int cap_dst;            /* CSR: entries that col_dst / dst hold */
    const void* src;        /* device; CSR: val_src */
    const int* off_src;     /* device; ragged: seg_off; CSR: crow_src */
    const int* col_src;     /* device; CSR */
    void* dst;              /* device; CSR: val_dst */
    int* col_dst;           /* device; CSR */
    float* mask;            /* device; ragged, nullable */
} laff_assemble_job;
int laff_batch_assemble(laff_ctx* ctx, const laff_assemble_job* jobs, int count, int B, const int* control /*device*/,
                        const int* control_host, int control_len);

/* ---- e: the collectives of the sharded path for a host that is not Python (laff_amd/dist.py issues the same three through
 * torch.distributed).  One process per GPU; RCCL is looked up at the first call (a copy already loaded into
 * the process first, then librccl.so / librccl.so.1) -- the library does not link against it, LAFF_E_UNSUPPORTED when there is none.
 * Every call is asynchronous on the stream the comm was created with (the ctx's; laff_comm_set_stream re-binds it).
 *   'video' scheme (the reference's loop model/model.py:1057-1077 sharded by video rows): laff_allgather_rows on the text
 *   embeddings, laff_allreduce_f64_max on s_gt64 (laff_rank_prepare writes -inf for texts whose video lives elsewhere),
 *   laff_allreduce_i32_sum on the counts (the overflow poison -2^26 survives a sum over up to 16 shards). */
#define LAFF_COMM_ID_BYTES 128
typedef struct laff_comm laff_comm;
int laff_comm_unique_id(unsigned char* id /*[LAFF_COMM_ID_BYTES], made by one rank, handed to the others out of band*/);
int laff_comm_init(laff_ctx* ctx, int rank, int world, const unsigned char* id, laff_comm** out);
int laff_comm_set_stream(laff_comm* comm, void* hip_stream);
int laff_comm_destroy(laff_comm* comm);
int laff_allgather_rows(laff_comm* comm, const void* send, void* recv, size_t bytes_per_rank);     /* recv: world x bytes, rank order */
int laff_allreduce_i32_sum(laff_comm* comm, int* buf, size_t n);                                    /* in place */
int laff_allreduce_f64_max(laff_comm* comm, double* buf, size_t n);                                 /* in place */

#ifdef __cplusplus
}
#endif
#endif /* LAFF_HIP_H */
