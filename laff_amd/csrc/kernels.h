// kernels.h -- internal launch interface between api.hip and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/laff_hip.h"

namespace laff {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting: one flag word per kernel instantiation, one bit per device
// ordinal (a second laff_ctx on another GPU of the same process sets it again).  The first launch of an instantiation on a device must
// therefore happen outside a HIP-graph capture (every caller warms up eagerly before it captures).
template <typename K>
static inline hipError_t smem_attr_once(unsigned long long& done, K kernel, int smem) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    // (atomic: two host threads driving two contexts must not lose each other's bit -- a lost bit would repeat the call, possibly
    // inside a capture)
    if (__atomic_load_n(&done, __ATOMIC_ACQUIRE) & bit) return hipSuccess;
    if (smem > 64 * 1024) {
        e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return e;
    }
    __atomic_fetch_or(&done, bit, __ATOMIC_ACQ_REL);
    return hipSuccess;
}

enum { GEMM_F32 = 0, GEMM_F16 = 1, GEMM_BF16 = 2 };

struct GemmArgs {
    const void* R;        // [nR, ldR] rows -> output rows
    const float* Rf;      // x3 fused tile only: the row operand in fp32 [nR, ldRf]; split into hi/lo planes in the kernel
    int ldRf;
    const void* C;        // [nC, ldC] rows -> output columns
    int nR, nC, K;        // K in elements (per segment)
    int ldR, ldC;         // elements
    int nseg;             // 1, or 3 for the hi/lo split (virtual K concatenation)
    long segR[3], segC[3];  // byte offset of the operand plane used by each segment
    float* out;           // [nR, ldo] or null
    int ldo;
    float scale;
    const float* row_scale;   // optional per-output-row / per-output-column factors (operand split scales)
    const float* col_scale;
    // FC epilogue
    const float* bias;
    const float* bn_scale;
    const float* bn_shift;
    int act;
    // fused ground-truth rank count
    const int* gt_col;
    int col0;
    const float* s_gt;
    int* count;
    // exact-rank ("banded") count: definite counts here, pairs inside the error band go to a list for laff_rank_resolve
    const double* s_gt64;     // [nR] exact ground-truth scores (laff_rank_prepare); non-null selects the banded epilogue
    const float* band_r;      // [nR] row part of the band half-width
    const float* band_c;      // [nC] column part
    unsigned* pairs;          // header {count, overflow, 0, 0} + pair_cap x {row, col}
    unsigned pair_cap;
    unsigned long long* trace;   // debug (LAFF_GEMM_TRACE build only): 8 timestamps per workgroup
};

constexpr int MAX_GROUP = 8;
struct GroupedGemmArgs {
    int count;
    int nbig;             // x3 grouped kernel: blocks [0, nbig) run big tiles, the rest quarter tiles of the remaining ones
    int tile_start[MAX_GROUP + 1];
    GemmArgs p[MAX_GROUP];
};

// ---- strip form of the similarity GEMM at K = 512 (sim_strip.hip) ------------------------------------------------------------
constexpr int STRIP_ROWS = 256;          // text rows per strip (4 wavefronts x 64 rows held in registers)
constexpr int STRIP_COLS = 32;           // videos per column block (one 32 KiB ring slot)
constexpr int STRIP_MAX_GROUPS = 2048;   // aligned 64-column groups whose band maxima fit the LDS table (131,072 videos)
constexpr int STRIP_MAX_WG = 512;        // persistent workgroups (one per CU)
constexpr int STRIP_CHUNK = 64;          // entries per chunk of the dump list (a wavefront takes a new chunk with one atomic)
constexpr int STRIP_ENTRY_WORDS = 24;    // one dumped group: {row, colbase, lo, hi | mask16, the row's ground-truth column, 0, 0 | 16 raw accumulators}
struct StripArgs {
    const void* T;            // [nR][512] 16-bit, rows 1,024 bytes apart
    const void* V;            // [nC][512]
    int nR, nC;
    float* out;               // [nR][ldo] or null
    int ldo;
    float scale, inv_scale;
    const int* gt_col;        // banded count (as GemmArgs); count == null: scores only
    int col0;
    const double* s_gt64;
    const float* band_r;
    const float* band_c;
    int* count;
    unsigned* pairs;          // header {chunks taken, flag, NW | 1 << 31, NCH} | NCH per-chunk counts | NCH chunks of STRIP_CHUNK entries
    unsigned pair_cap;
    int nranges;              // == gridDim.x
    unsigned long long* trace;   // debug (LAFF_STRIP_TRACE build only): 64 cycle stamps per workgroup
    unsigned short range_of_wg[STRIP_MAX_WG];
};
extern int g_strip_mode;
bool sim_strip_eligible(const GemmArgs& a, int mode, bool aligned);
hipError_t launch_sim_strip(const GemmArgs& a, int mode, hipStream_t st);

// ---- strip form of the FC projection at K = 512 (fc_strip.hip): X stationary in registers, W streamed from a packed LDS image ----
constexpr int FC_STRIP_ROWS = 128;       // input rows per strip (4 wavefronts x 32 rows held in registers)
constexpr int FC_STRIP_K = 512;
struct FcStripProblem {
    const float* X;           // [N][ldx] fp32, 16-byte aligned rows
    const void* img;          // laff_fc_strip_pack: D / 32 blocks x 2 K-halves x 32 KiB {hi, lo} + [D][4] lane constants
    const float* vec;         // the lane constants inside img
    float* Y;                 // [N][ldy]
    int ldx, ldy, N;
    int unit0;                // first (strip, column block) unit of this problem in the launch (filled by launch_fc_strip)
};
struct FcStripArgs {
    int count;
    int nblk;                 // D / 32, the same for every problem of a launch
    int nranges;              // == gridDim.x
    int total_units;
    unsigned long long* trace;   // debug (LAFF_FCS_TRACE build only): 80 words per workgroup
    FcStripProblem p[MAX_GROUP];
    unsigned short range_of_wg[STRIP_MAX_WG];
};
size_t fc_strip_image_bytes(int D);
size_t fc_strip_vec_offset(int D);
hipError_t launch_fc_strip_pack(const float* W, int ldw, const float* bias, const float* bn_scale, const float* bn_shift, int D, int act,
                                void* img, hipStream_t st);
hipError_t launch_fc_strip(FcStripArgs& a, int act, hipStream_t st);
// The kernel exists on two MFMA shapes: v_mfma_f32_16x16x32_f16 (fc_strip16.hip, the default) and v_mfma_f32_32x32x16_f16
// (fc_strip.hip); what they share is fc_strip_common.h, the one host path is fc_strip.hip's.  g_fc_strip_mfma (16 or 32:
// LAFF_FC_STRIP_MFMA, read when a ctx is created) says which image layout launch_fc_strip_pack writes and which kernel
// launch_fc_strip runs: an image must be launched in the mode it was packed in.
extern int g_fc_strip_mfma;

// ---- concat tower (fc_concat.hip): Y = bn(act(sum_s X_s . W[:, c_s : c_s + Dk_s]^T + bias)), dense + CSR segments, one launch ------
constexpr int CONCAT_MAX_SEG = 8;        // segments per problem, dense and sparse together
constexpr int CONCAT_MAX_GROUP = 4;      // problems per launch (the launch arguments stay below the 4 KiB kernel-argument limit)
struct ConcatDense {
    const float* X;           // [N][ldx] fp32
    int ldx, dk, c0;          // c0: first column of W's window
    int fast;                 // bit 0: X rows take the LDS-DMA path, bit 1: W's window does
};
struct ConcatSparse {
    const int* indptr;        // CSR over dk columns
    const int* indices;
    const float* values;      // null = ones
    const float* wt;          // [dk][ldwt >= D]: the transposed column block
    int ldwt, dk;
};
struct ConcatProblem {
    const float* W;           // [D][ldw], read in place at every dense segment's column offset
    const float* bias;
    const float* bn_scale;
    const float* bn_shift;
    float* Y;                 // [N][ldy]
    int N, D, ldw, ldy, act;
    int nd, ns;               // dense / sparse segments, each in list order
    ConcatDense d[CONCAT_MAX_SEG];
    ConcatSparse s[CONCAT_MAX_SEG];
};
struct ConcatArgs {
    int count;
    int tile_start[CONCAT_MAX_GROUP + 1];     // filled by launch_fc_concat
    ConcatProblem p[CONCAT_MAX_GROUP];
};
hipError_t launch_fc_concat(ConcatArgs& a, hipStream_t st);

// the kernel launch_gemm_nt runs for these arguments (LAFF_ROUTE_*, include/laff_hip.h); launches nothing
int gemm_route(const GemmArgs& a, int mode, bool aligned);
hipError_t launch_gemm_nt(const GemmArgs& a, int mode, bool aligned, hipStream_t st);
// what a grouped FC launch runs (laff_fc_route reports it, the launchers below act on it): kernel = LAFF_FC_KERNEL_*, tiles in that
// kernel's own tile; the split tile's tail split leaves nbig whole 256 x 256 tiles and `quarters` 128 x 128 workgroups
struct GroupedPlan { int kernel; long tiles; int nbig; long quarters; };
bool plan_gemm_nt_grouped_f32(GroupedGemmArgs& g, int staging, GroupedPlan& pl);
bool plan_gemm_nt_grouped_f16(GroupedGemmArgs& g, GroupedPlan& pl);
bool plan_gemm_nt_x3_fused_grouped(GroupedGemmArgs& g, GroupedPlan& pl);
hipError_t launch_gemm_nt_grouped_f32(GroupedGemmArgs& g, int staging, hipStream_t st);
hipError_t launch_gemm_nt_grouped_f16(GroupedGemmArgs& g, hipStream_t st);
hipError_t launch_gemm_nt_x3_fused_grouped(GroupedGemmArgs& g, hipStream_t st);   // fp32 row operand split in the kernel   // fast staging only (packed operands)
int staging_kind(const GemmArgs& a, int esz, bool aligned);
extern int g_num_cus;

constexpr int MAX_L = 8;
struct FuseArgs {
    const float* src[MAX_L];
    const float* scale[MAX_L];
    const float* shift[MAX_L];
    int ld[MAX_L];
    int tile[MAX_L];
    int act[MAX_L];       // LAFF_ACT_* applied to the plane before its affine
    const float* rownorm[MAX_L];      // optional per-row factor [N] applied after the affine (expert-embedding l2norm branch)
    // gather planes (src == null): plane value = sum_j values_j * Wt[indices_j, column] + bias[column]  (sparse bag-of-words FC)
    const int* g_indptr[MAX_L];
    const int* g_indices[MAX_L];
    const float* g_values[MAX_L];     // null = all ones
    const float* g_wt[MAX_L];         // [Dk, g_ldwt], non-null marks a gather plane
    const float* g_bias[MAX_L];
    int g_ldwt[MAX_L], g_dk[MAX_L];
    int head_major;       // block -> (head = b % H, 4 rows): with H == 8 every XCD gathers from its own 512-column slice of Wt
    int L, N, H, d;
    int head_stride;      // d (split heads) or 0 (every head sees all columns)
    const float* w;       // [H, d]
    const float* b;       // [H]
    const float* gw;      // [H]
    unsigned flags;
    float* E;             // [N, H, d]
    float* attn_w;        // [N, H, L] or null
    void* E16;            // optional [N, H*d] 16-bit GEMM operand (E * e16_scale), fp16 or bf16
    int e16_bf16;
    float e16_scale;
    // laff_rank_prepare's work for these rows done by this launch (laff_fuse_packed_rank; heads of d <= 512, E16 given): the wave
    // that has just produced a row measures its operand's rounding error (band) and, on the text side, scores it exactly against its
    // ground-truth video (s_gt64) -- the rows are not read back by a separate launch.  rp_side 0 = off, 1 = text rows, 2 = video rows.
    int rp_side;
    const int* rp_gt;         // side 1: [N] ground-truth column of every text
    int rp_col0, rp_Nv;       // side 1: the videos of this launch's partner are columns [col0, col0 + Nv)
    const float* rp_Ev;       // side 1: their fp32 embeddings [Nv, d] (the E of the side-2 launch, complete before this one starts)
    double* rp_sgt;           // side 1: s_gt64 [N]
    float* rp_band;           // side 1: band_t [N];  side 2: band_v [((N + 3) & ~3) + ceil(N / 64)] (per column; the block maxima are
                              //         finished by the side-1 launch, which runs behind this one)
    float* rp_band_v;         // side 1: the partner's band_v
    int* rp_count;            // side 1: [N], cleared
    unsigned* rp_pairs;       // side 1: pair-list header, cleared
    double* rp_part;          // H > 1: [N][H][2] scratch {head term of the exact score, q_h^2}
    unsigned* rp_ticket;      // H > 1: [N] arrival counters, zero at launch
    float rp_unit, rp_cacc;   // unit roundoff of the operand format, accumulation term of the band (see launch_rank_prepare)
};
hipError_t launch_fuse(const FuseArgs& a, hipStream_t st);
hipError_t launch_plane_row_norms(const FuseArgs& a, float* out /*[L][N]*/, hipStream_t st);

// fuse_bwd.hip: backward of the fusion over plain dense planes (laff_fuse_backward)
struct FuseBwdArgs {
    const float* x[MAX_L];    // [N, ldx]
    float* dx[MAX_L];         // [N, lddx]
    int ldx[MAX_L], lddx[MAX_L];
    int L, N, H, d;
    int head_stride;          // d (split heads) or 0 (every head sees all columns; dx_l is the sum over the heads)
    const float* w;           // [H, d]
    const float* b;           // [H]
    const float* gw;          // [H]
    unsigned flags;
    const float* dE;          // [N, lde >= H * d]
    int lde;
    float* dw_part;           // workspace [H][part_rows][d], or null when dw is not wanted
    int rows_per_block, part_rows;       // filled by launch_fuse_backward from fuse_bwd_plan
};
// how a shape is cut: rows per block (a multiple of 4), row chunks, and the partial rows of dw per head that the workspace holds
void fuse_bwd_plan(int N, int H, int d, unsigned flags, int* rows_per_block, int* chunks, int* part_rows);
hipError_t launch_fuse_backward(FuseBwdArgs& a, float* dw, float* db, hipStream_t st);

// selfattn_fuse.hip: the multi-head self-attention fusion block, forward and backward (laff_selfattn_fuse, laff_selfattn_fuse_backward)
struct SelfAttnArgs {
    const float* x[MAX_L];    // [N, ldx]
    float* dx[MAX_L];         // [N, lddx]                     backward
    int ldx[MAX_L], lddx[MAX_L];
    int L, N, H, d;
    int prepend, pool, token; // LAFF_SA_PREPEND_*, LAFF_SA_POOL_*, the token index of LAFF_SA_POOL_TOKEN
    int l2n;                  // l2norm_each_head
    float scale;              // (d / H) ^ -0.5
    const float* gamma;       // [d]
    const float* beta;        // [d]
    float* E;                 // [N, lde]   pooled output      forward
    const float* dE;          // [N, lde]   its gradient       backward
    int lde;
    float* O;                 // stacked output (LAFF_SA_POOL_ALL): O[n * ldon + l * ldol + h * d + c]
    const float* dO;          // its gradient
    int ldon, ldol;
    float* part;              // workspace [chunks][2 d], or null when neither dgamma nor dbeta is wanted
    int groups_per_block, chunks;        // filled by the launchers from selfattn_plan
};
// how N * H groups are cut: groups per block (a multiple of 4) and blocks = partial rows of dgamma | dbeta
void selfattn_plan(int N, int H, int* groups_per_block, int* chunks);
hipError_t launch_selfattn_fuse(SelfAttnArgs& a, hipStream_t st);
hipError_t launch_selfattn_fuse_backward(SelfAttnArgs& a, float* dgamma, float* dbeta, hipStream_t st);

// fc_bwd.hip: backward of the FC projection A = act(X W^T + bias) (laff_fc_backward)
struct FcBwdArgs {
    const float* X;           // [N, ldx >= Dk]   read for dW
    const float* W;           // [D, ldw >= Dk]   read for dX
    const float* A;           // [N, lda >= D]    the saved forward output
    const float* dA;          // [N, ldda >= D]
    float* dX;                // [N, lddx >= Dk] or null
    float* dW;                // [D, lddw >= Dk] or null
    float* db;                // [D] or null
    int N, Dk, D, ldx, ldw, lda, ldda, lddx, lddw, act;
    unsigned vec;             // 16-byte loads allowed: bit 0 A and dA, bit 1 X, bit 2 W (base aligned and pitch % 4 == 0)
    float* part;              // workspace: [chunks][D][Dk] partial dW, then [chunks][D] partial db; afterwards [chunks_dx][N][Dk] partial dX
    float* part_db;           // filled by launch_fc_backward, as are the four below (from fc_bwd_plan)
    int chunks, chunk_rows;   // dW, db: the cut of the sum over N
    int chunks_dx, chunk_len_dx;         // dX: the cut of the sum over D
};
// how a shape is cut, from (N, Dk, D) alone: per product the edge (64 or 128) of its output tiles and the chunks of its sum (each a
// multiple of 32 long), and the workspace that dW with db, db alone and dX need (0 with one chunk)
struct FcBwdPlan {
    int chunks, chunk_rows, tile_dw;
    int chunks_dx, chunk_len_dx, tile_dx;
    size_t ws_dw, ws_db, ws_dx;
};
void fc_bwd_plan(int N, int Dk, int D, FcBwdPlan* p);
hipError_t launch_fc_backward(const FcBwdArgs& a, hipStream_t st);

// fc_gather_bwd.hip: backward of the FC projection of a sparse X, given transposed (CSC) (laff_fc_gather_backward)
struct FcGatherBwdArgs {
    const int* colptr;        // [Dk + 1]; column v owns the entries [colptr[v], colptr[v + 1]), ascending row order
    const int* rows;          // [nnz] row index of an entry; one outside [0, N) contributes nothing
    const float* values;      // [nnz] or null (all ones)
    const float* A;           // [N, lda >= D]    the saved forward output, rows 16-byte aligned
    const float* dA;          // [N, ldda >= D]   rows 16-byte aligned
    float* dW;                // [D, lddw >= Dk] or null; every element of the window is written
    float* db;                // [D] or null
    int nnz, N, Dk, D, lda, ldda, lddw, act;
};
hipError_t launch_fc_gather_backward(const FcGatherBwdArgs& a, hipStream_t st);

// fc_concat_bwd.hip: backward of the concat layer's dense segments, all of them in one launch per product (laff_fc_concat_backward;
// the CSR segments go through launch_fc_gather_backward on their windows)
struct FcConcatBwdSeg {
    const float* X;           // [N, ldx >= dk]   read for dW, in place
    float* dX;                // [N, lddx >= dk] or null
    int ldx, lddx, dk, col;   // col: first column of the segment's window in W and dW
};
struct FcConcatBwdArgs {
    const float* W;           // [D, ldw >= K]    read for dX, in place at every window
    const float* A;           // [N, lda >= D]    the saved forward output
    const float* dA;          // [N, ldda >= D]
    float* dW;                // [D, lddw >= K] or null; only the dense segments' windows are written
    float* db;                // [D] or null
    int N, D, ldw, lda, ldda, lddw, act;
    int nseg;                 // dense segments, in list order
    FcConcatBwdSeg seg[CONCAT_MAX_SEG];
    float* part;              // workspace, as FcBwdArgs::part with the segments' columns side by side in a partial row
};
// how the dense segments of widths dk[0 .. n) are cut, from (N, D, the widths) alone: as FcBwdPlan, with the products' tiles counted
// over all segments; ws_dx counts the dx_cols columns of the segments that want a dX
void fc_concat_bwd_plan(int N, int D, const int* dk, int n, int dx_cols, FcBwdPlan* p);
hipError_t launch_fc_concat_backward(const FcConcatBwdArgs& a, hipStream_t st);

// bn_train.hip: dropout by a counter-based mask and training-mode BatchNorm1d, forward and backward (laff_dropout_bn_train,
// laff_dropout_bn_train_backward).  One struct for both directions; a direction leaves the other's fields null.
constexpr int BN_TRAIN_ROWS = 256;       // rows of a chunk: the strip of 32 columns that a block keeps in registers
struct BnTrainArgs {
    const float* A;           // [N, lda >= D]    the activation output
    const float* dY;          // backward: [N, lddy >= D]
    float* out;               // forward: Y [N, ldo >= D]; backward: dA [N, ldo >= D] or null
    const unsigned long long* seed;      // device; read only when drop
    const float* gamma;       // [D], null: no BatchNorm stage
    const float* beta;        // forward
    float* running_mean;      // forward, updated in place, as running_var
    float* running_var;
    float* save_mean;         // forward: written; backward: read, as save_invstd
    float* save_invstd;
    float* dgamma;            // backward, [D] or null, as dbeta
    float* dbeta;
    double* part;             // workspace [chunks][2][D]: per chunk (mean, M2) forward, (sum dY, sum dY xhat) backward
    int N, D, lda, lddy, ldo;
    int drop;                 // p > 0
    unsigned thresh;          // an element is kept iff its Philox word >= thresh
    float scale;              // fp32(1 / (1 - p))
    double momentum, eps;
    int fast;                 // rows on 16-byte boundaries (bases and pitches) and D % 4 == 0
};
struct BnTrainPlan {
    int chunks;               // row chunks of the column sums (1 without a BatchNorm stage: nothing is summed)
    int launches;             // per direction: 1, or 2 when the sums are cut
    size_t ws;                // workspace bytes (0 with one chunk)
};
void bn_train_plan(int N, int D, bool has_bn, BnTrainPlan* p);
hipError_t launch_bn_train_forward(const BnTrainArgs& a, hipStream_t st);
hipError_t launch_bn_train_backward(const BnTrainArgs& a, hipStream_t st);

// tile_bn_train.hip: training-mode BatchNorm1d(H C) over X.repeat(1, H) without forming the tiled input (laff_tile_bn_train,
// laff_tile_bn_train_backward).  One struct for both directions, as BnTrainArgs; the statistics are per input column.
struct TileBnTrainArgs {
    const float* X;           // [N, ldx >= C]
    const float* dY;          // backward: [N, lddy >= H C]
    float* Y;                 // forward: [N, ldy >= H C]
    float* dX;                // backward: [N, lddx >= C] or null
    const float* gamma;       // [H C]
    const float* beta;        // forward, [H C]
    float* running_mean;      // forward, [H C], updated in place, as running_var
    float* running_var;
    float* save_mean;         // [C]; forward: written; backward: read, as save_invstd
    float* save_invstd;
    float* dgamma;            // backward, [H C] or null, as dbeta
    float* dbeta;
    double* part;             // workspace: forward [chunks][2][C] (mean, M2); backward [chunks][2][H C] (sum dY, sum dY xhat)
    int N, C, H, ldx, ldy, lddy, lddx;
    double momentum, eps;
    int fast;                 // rows on 16-byte boundaries (bases and pitches) and C % 4 == 0
};
// its plan is bn_train_plan(N, H C, true): the backward's partials; the forward's are 1 / H of them
hipError_t launch_tile_bn_train_forward(const TileBnTrainArgs& a, hipStream_t st);
hipError_t launch_tile_bn_train_backward(const TileBnTrainArgs& a, hipStream_t st);

// expert_train.hip: the expert stage of the towers in training mode (laff_expert_stage_train, laff_expert_stage_train_backward): the
// expert embedding added to each plane and the row norm over all D columns, into / out of the stacked [N, L, D] tensor of the fusion.
// One struct for both directions.
constexpr int EXPERT_MAX_PLANES = 8;
constexpr int EXPERT_ROWS = 16;           // rows of one block of the backward: one partial column sum of d_expert per block
struct ExpertStageArgs {
    const float* x[EXPERT_MAX_PLANES];    // [N, ldx[l] >= D] each
    float* dx[EXPERT_MAX_PLANES];         // backward: [N, lddx[l] >= D] each
    int ldx[EXPERT_MAX_PLANES], lddx[EXPERT_MAX_PLANES];
    const float* expert;                  // [L, lde >= D] or null
    float* Y;                             // forward: element (n, l, c) at n ldn + l ldl + c
    const float* dY;                      // backward: the same layout
    float* rnorm;                         // [L][N]; forward: written, backward: read; null without l2norm
    float* part;                          // backward: [chunks][L][D] partial column sums, or null (d_expert not formed)
    float* d_expert;                      // backward: [L, D] dense, or null
    int N, L, D, lde, l2norm;
    long ldn, ldl;
};
void expert_stage_plan(int N, int L, int D, int* chunks, size_t* ws);
hipError_t launch_expert_stage_forward(const ExpertStageArgs& a, hipStream_t st);
hipError_t launch_expert_stage_backward(const ExpertStageArgs& a, hipStream_t st);

// optim.hip: global-norm clipping and the Adam / RMSprop step over a list of flat fp32 tensors (laff_grad_sqnorm, laff_grad_scale,
// laff_optim_step)
constexpr int OPTIM_CHUNK = 4096;        // elements of one chunk: 256 threads x 4 accesses of 16 bytes
constexpr int OPTIM_TABLE = 72;          // tensors of one launch: the table travels in the launch arguments (72 x 48 bytes)
constexpr int OPTIM_GRID_CAP = 1024;     // blocks of one launch, striding over the chunks; also the partials a norm launch leaves
struct OptimEntry {
    float* p;                 // the parameter (laff_grad_scale: the gradient that is scaled in place)
    const float* g;
    float* s1;                // exp_avg / square_avg
    float* s2;                // exp_avg_sq, Adam only
    long long n;              // elements, > 0
    long long first;          // the tensor's first chunk in the launch
};
struct OptimTable {
    long long chunks;         // of the whole launch
    int count;
    OptimEntry t[OPTIM_TABLE];
};
struct OptimScalars {         // the step's constants, rounded to fp32 once on the host from float64
    float lr, omb1 /*1 - beta1*/, b2 /*beta2, RMSprop's alpha*/, omb2 /*1 - b2*/, eps, wd, bc1, bc2;
};
struct OptimPlan { int launches, partials; };
struct OptimLaunches { int fast, generic; };             // launches issued, by variant
void optim_plan(int count, const long long* n, OptimPlan* p);
hipError_t launch_optim_sqnorm(const laff_optim_tensor* t, int count, double* part, OptimLaunches* done, hipStream_t st);
hipError_t launch_optim_scale(const laff_optim_tensor* t, int count, double max_norm, const double* part, int np, float* total_out,
                              OptimLaunches* done, hipStream_t st);
hipError_t launch_optim_update(const laff_optim_tensor* t, int count, int kind, const OptimScalars& h, double max_norm, const double* part,
                               int np, float* total_out, OptimLaunches* done, hipStream_t st);

struct FrameArgs {
    const float* frames;  // [B, Fmax, d]
    const int* lens;      // [B] or null
    int B, Fmax, d;
    const float* w;
    const float* b;
    const float* gw;
    unsigned flags;
    float* V;             // [B, d]
    const float* mask;    // [B, ldm] or null: the reference's mask_tensor (1.0 per valid frame, a prefix of the row); replaces lens
    int ldm;
};
struct FrameGroup {       // up to 8 frame features of the same shape in ONE launch: block -> (feature, video)
    int count;
    FrameArgs f[8];
};
hipError_t launch_frame_fuse(const FrameGroup& g, hipStream_t st);

// frame_bwd.hip: backward of the frame attention (laff_frame_fuse_backward)
struct FrameBwdArgs {
    const float* frames;  // [B, Fmax, d]
    const float* w;       // [d]
    const float* b;       // [1]
    const float* gw;      // [1] or null without WITH_AVE
    const float* dV;      // [B, lddv]
    float* dframes;       // [B, Fmax, d]
    float* dw;            // [d] or null
    float* db;            // [1] or null
};
struct FrameBwdGroup {    // up to 8 frame features of the same shape in ONE launch: block -> (feature, video)
    int count, B, Fmax, d, lddv;
    unsigned flags;
    const int* lens;      // [B] or null
    float* dw_part;       // workspace [count][B][d]: one partial row of dw per (feature, video); null when dw is not wanted
    FrameBwdArgs f[8];
};
int frame_bwd_variant(int d);            // NCH, the 256-column chunks a lane owns: 1 / 2 / 4
// tail: also run the second launch (dw from the partial rows, db = 0)
hipError_t launch_frame_fuse_backward(const FrameBwdGroup& g, bool tail, hipStream_t st);

hipError_t launch_split_rows_grouped(int count, const float* const* X, const int* N, const int* K, const int* ldx, void* const* out,
                                     float* const* rscale, hipStream_t st);
hipError_t launch_loss_normalize(const float* s, const float* im, int B, int H, int d, int dp, int Bp, float eps, float* XH,
                                 float* XHT, float* nrm, float* npr, hipStream_t st);
hipError_t launch_margin_reduce(const float* S, float* dS, float* dST, float* loss_h, float* loss, int B, int Bp, int H,
                                float margin, int max_violation, int use_s, int use_im, float g_s, float g_im, hipStream_t st);
hipError_t launch_loss_normalize_bwd(const float* XH, const float* G, const float* nrm, const float* npr, int B, int H, int d,
                                     int dp, float* d_s, float* d_im, hipStream_t st);
hipError_t launch_loss_sum_heads(const float* loss_h, int H, float* loss, hipStream_t st);
// loss_dsl.hip: the dual-softmax criterion on S [H][B][Bp] (rows = captions); ST [H][B][Bp] and stat [H][DSL_STAT_ROWS][B] are scratch,
// dS / dST [H][B][Bp] are written (padding columns zeroed) unless both are null
constexpr int DSL_STAT_ROWS = 10;
hipError_t launch_dsl_reduce(const float* S, float* ST, float* stat, float* dS, float* dST, float* loss_h, float* loss, int B, int Bp,
                             int H, float temp, hipStream_t st);
hipError_t launch_fc_gather(const int* indptr, const int* indices, const float* values, int N, int Dk, const float* Wt, int ldwt,
                            const float* bias, const float* bn_scale, const float* bn_shift, int D, int act, float* Y, int ldy,
                            hipStream_t st);
hipError_t launch_pack_rows(const float* E, int N, int H, int d, int lde, int normalize, float eps, float prescale,
                            int precision, void* out, hipStream_t st);

hipError_t launch_row_dot_gt(const void* T, const void* V, int Nt, int Nv, int K, int bf16, int x3, float scale,
                             const int* gt_col, int col0, float* s_gt, int* zero_count, hipStream_t st);
// The constants of the exact-rank error band (rank_prepare_kernel, and fuse_kernel's rp_* rows): the unit roundoff of the operand format,
// and the fp32 accumulation of the exact products: K = H * d terms (3K for a hi/lo split, plus its dropped lo*lo term <= 2^-22), 2^-23
// each (covers round-to-nearest and truncating accumulators), + 2^-20 for the fp32 copy of s_gt64, the scaling and the rounding of the
// accumulator-unit thresholds the GEMM epilogue compares against.
static inline void rank_band_constants(int precision, int H, int d, float* unit, float* c_acc) {
    const bool x3 = precision == LAFF_PREC_FP16X3 || precision == LAFF_PREC_BF16X3;
    const bool bf16 = precision == LAFF_PREC_BF16 || precision == LAFF_PREC_BF16X3;
    *unit = precision == LAFF_PREC_FP32 ? 5.9604645e-8f : (bf16 ? 3.90625e-3f : 4.8828125e-4f);
    *c_acc = (float)((double)H * d * (x3 ? 3.0 : 1.0) * 1.1920929e-7 + 9.5367432e-7 + (x3 ? 2.3841858e-7 : 0.0));
}
hipError_t launch_rank_prepare(const float* Et, const float* Ev, const void* T, const void* V, int Nt, int Nv, int H, int d,
                               int precision, float prescale, const int* gt_col, int col0, double* s_gt64, float* band_t,
                               float* band_v, int* zero_count, unsigned* pairs, int sides, hipStream_t st, int emit = 0);
hipError_t launch_rank_export(const double* s_gt64, int* count, float* S, int lds, unsigned* pairs, unsigned pair_cap, const int* bounds,
                              int world, int col0, unsigned* out, unsigned cap, unsigned* fill, hipStream_t st);
// metrics_n > 0: the block that finishes last also turns the counts into ranks (count + base -> ranks_out) and the seven metrics
// (out8 on the device, host8 = the same in device-addressable host memory or null); ticket: one zero word, left zero
hipError_t launch_rank_resolve(const float* Et, const float* Ev, int Nt, int Nv, int H, int d, const double* s_gt64, int* count,
                               float* S, int lds, unsigned* pairs, unsigned pair_cap, hipStream_t st, int metrics_n = 0, int base = 0,
                               int* ranks_out = nullptr, double* out8 = nullptr, double* host8 = nullptr, unsigned* ticket = nullptr);
// scratch: rank_metrics_scratch_bytes() bytes, zero before the first launch (every launch leaves it zero); not shared by launches in flight
size_t rank_metrics_scratch_bytes();
size_t rank_resolve_ticket_offset();      // where, inside that scratch, the ticket lines of the fused resolve + metrics launch start
// host8: the 8 result doubles also go to this device-addressable host buffer (null: none)
hipError_t launch_rank_metrics(const int* r, int n, int base, int* ranks_out, double* out7, double* err, unsigned* scratch, hipStream_t st,
                               double* host8 = nullptr);
hipError_t launch_gather_gt(const float* S, int Nt, int Nv, int lds, const int* gt_col, int col0, float* s_gt,
                            hipStream_t st);
hipError_t launch_rank_count(const float* S, int Nt, int Nv, int lds, const int* gt_col, int col0, const float* s_gt,
                             int* count, int accumulate, hipStream_t st);
hipError_t launch_topk_rows(const float* S, int Nt, int Nv, int lds, int K, int* idx_out, float* val_out, hipStream_t st);
hipError_t launch_v2t_count(const float* S, int Nt, int Nv, int lds, const int* grp_off, const int* grp_idx,
                            int max_group, int* count, hipStream_t st);
hipError_t launch_v2t_count_exact(const float* S, int Nt, int Nv, int lds, const int* grp_off, const int* grp_idx, int max_group,
                                  const float* Et, const float* Ev, int H, int d, const double* s_gt64, const float* band_t,
                                  const float* band_v, int* count, unsigned* list, unsigned cap, hipStream_t st);

// gru.hip: one direction of a GRU time step (laff_gru_encode)
struct GruDirArgs {
    const float* P;       // [V, 3H]: we . W_ih^T + b_ih
    const float* Wp;      // laff_gru_pack_whh(W_hh)
    const float* bhh;     // [3H]
    const float* h_in;    // packed h_{t-1} (zero for a row that has not started)
    float* h_out;         // packed h_t
    float* sum;           // [Npad, H] running sum of h over the steps taken so far
    int B;                // active rows (a prefix of the length-sorted rows)
    int t;                // token column of this step
    int col0;             // output column of this direction's mean
    float* res;           // saving step only: this direction's reserve, the planes r, z, n, q, h_prev of [M, H] each
    int off;              // saving step only: packed position of this step's row 0 (prefix sum of batch_sizes)
};
struct GruStepArgs {
    GruDirArgs d0, d1;    // d0 forward, d1 reverse (grid.z)
    const int* tokens;    // [T, N] time-major, sorted row order
    const int* lens;      // [N] sorted row order
    const int* perm;      // [N] sorted row -> output row
    int N, H, V, skip_gemm, pooling;
    float* out;
    int ldo;
    int M;                // saving step only: packed rows in all, sum of batch_sizes
};
hipError_t launch_gru_pack_whh(const float* W, int H, float* Wp, hipStream_t st);
// save: the training step (laff_gru_encode_train), which also fills the reserve; the tile rule is the same
hipError_t launch_gru_step(const GruStepArgs& s, int ndirs, hipStream_t st, bool save = false);
// the tile rule of a forward or backward step with B active rows (the larger of the two directions'): true = the 64 x 32 tile
bool gru_step_big(int B, int H, int ndirs);

// gru_bwd.hip: one direction of a backward time step (laff_gru_backward)
struct GruBwdDirArgs {
    const float* WpT;     // laff_gru_pack_whh_t(W_hh)
    const float* res;     // this direction's reserve (r, z, n, q, h_prev planes of [M, H])
    const float* dgh_nb;  // dGH rows of the step that consumed this step's h (its row 0); read for rows < Bnb
    float* dgi;           // dGI rows of this step (its row 0), [B, 3H]
    float* dgh;           // dGH rows of this step
    float* carry;         // [N, H]: dh z of the row's previous backward step, updated in place
    int B, Bnb;           // active rows of this step; rows of it that the consuming step had too (a prefix)
    int t, off, col0;     // token column, packed position of row 0, this direction's column of dout under mean pooling
};
struct GruBwdStepArgs {
    GruBwdDirArgs d0, d1;
    const int* lens;
    const int* perm;
    const float* dout;    // [N, lddo] gradient of the encoder's output, input order
    int lddo, N, H, M, pooling;
};
hipError_t launch_gru_pack_whh_t(const float* W, int H, float* Wp, hipStream_t st);
hipError_t launch_gru_bwd_step(const GruBwdStepArgs& s, int ndirs, hipStream_t st);
// X[m] = table[ids[m]] (NaN for an id outside the table)
hipError_t launch_gru_gather_rows(const float* table, int V, int D, const int* ids, int M, float* X, hipStream_t st);
// d_we[seg_tok[s]] = sum over p in [seg_off[s], seg_off[s+1]) of dX0[seg_pos[p]] (+ dX1[seg_pos[p]]), in that order
hipError_t launch_gru_embed_grad(const float* dX0, const float* dX1, int M, int D, const int* seg_off, const int* seg_tok,
                                 const int* seg_pos, int U, int V, float* d_we, hipStream_t st);

// clip.hip: the CLIP text encoder (laff_clip_encode) and the transformer core it shares with the image encoder (clip_image.hip)
typedef float clip_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 clip_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 clip_h8 __attribute__((ext_vector_type(8)));
typedef unsigned clip_u4 __attribute__((ext_vector_type(4)));   // one 16-byte chunk (not HIP's uint4: a struct that stays in memory)
#define CLIP_TRY(expr)                               \
    do {                                             \
        const hipError_t e_ = (expr);                \
        if (e_ != hipSuccess) return e_;             \
    } while (0)
// epilogues of clip_gemm_tile (clip_core.h): + bias -> fp32, + bias QuickGELU -> operand, + bias added in place to fp32 C; and BERT's
// + bias erf-GELU -> operand, + bias tanh -> fp32
enum { CLIP_EPI_F32 = 0, CLIP_EPI_GELU = 1, CLIP_EPI_RESID = 2, CLIP_EPI_GELU_ERF = 3, CLIP_EPI_TANH = 4 };
enum { CLIP_LN_ROW = 0, CLIP_LN_EMBED = 1, CLIP_LN_POOL = 2, CLIP_LN_PATCH = 3 };
struct ClipGemmArgs {
    const void* A;        // [M, K] operand rows
    const void* B;        // [N, K] packed weight (nn.Linear layout)
    const float* bias;    // [N] or null
    void* C;              // [M, ldc]: fp32 (F32, RESID: added in place) or the operand type (GELU)
    int M, N, K, ldc;
};
struct ClipLnArgs {
    float* X;             // residual stream [*, W]: read (ROW: rows s * stride; POOL), written (EMBED, PATCH)
    const float* gamma;   // the LayerNorm into out
    const float* beta;
    void* out;            // [rows, W] operand
    int W, rows, stride;
    int round_f32;        // ROW: round to fp32 before the operand conversion, as the image tower does (clip_ln_kernel's F32)
    const int* ids;       // EMBED: [R] token ids
    const int* row_off;   // EMBED, POOL: [N+1]
    int N, V, ctx;        // EMBED
    const float* tok_emb; // EMBED: [V, W]
    const float* pos_emb; // EMBED: [ctx, W]; PATCH: [L, W]
    const float* patch;   // PATCH: [F g^2, W] fp32 patch GEMM output
    const float* cls;     // PATCH: [W] class embedding
    const float* pre_gamma;   // PATCH: ln_pre, its output written to X
    const float* pre_beta;
    int L;                // PATCH: tokens per frame
};
struct ClipAttnArgs {
    const float* qkv;     // [R, 3W]
    const int* row_off;   // [N+1]
    void* out;            // [R, W] operand
    int W;
};
struct ClipEncodeArgs {
    const laff_clip_text* model;
    const int* ids;
    const int* row_off;
    int N, R;
    float* X;             // workspace: [R, W] fp32
    void* A;              // workspace: [R, W] operand
    void* big;            // workspace: [R, 3W] fp32 (QKV) / [R, 4W] operand (MLP hidden)
    float* out;
    int ldo;
};
// an fp32 weight [rows, cols] -> operand [rows, ldp], zero columns past cols; transpose: [cols, rows] (ldp unused)
hipError_t launch_clip_pack(const float* W, int rows, int cols, int transpose, int ldp, int fp16, void* out, hipStream_t st);
hipError_t launch_clip_encode(const ClipEncodeArgs& e, int fp16, hipStream_t st);
// C[M, ldc] (+)= A[M, K] . B[N, K]^T + bias with epilogue epi (clip_gemm_kernel); K * operand size a multiple of 128 bytes
hipError_t launch_clip_gemm(const void* A, const void* B, const float* bias, void* C, int M, int N, int K, int ldc, int epi, int fp16,
                            hipStream_t st);
// LayerNorm of a.rows rows into the operand a.out in mode CLIP_LN_* (clip_ln_kernel)
hipError_t launch_clip_ln(int mode, const ClipLnArgs& a, int fp16, hipStream_t st);
// One pre-LN residual block around its attention, which each encoder launches itself (ln: X, out = the operand A, W, rows, stride):
//   launch_clip_block_qkv    A = ln_1(x) (LayerNorm mode `mode`, stride 1);  big = in_proj(A) [rows, 3W] fp32
//   launch_clip_block_post   x += out_proj(A);  A = ln_2(x);  x += c_proj(QuickGELU(c_fc(A)))  on x rows s * stride (ldc = stride W)
hipError_t launch_clip_block_qkv(const laff_clip_block& b, int mode, ClipLnArgs ln, void* big, int fp16, hipStream_t st);
hipError_t launch_clip_block_post(const laff_clip_block& b, ClipLnArgs ln, void* big, int fp16, hipStream_t st);

// clip_image.hip: the CLIP image encoder (laff_clip_image_encode)
constexpr int VIT_MAX_TOKENS = 257;
struct ClipImageArgs {
    const laff_clip_visual* model;
    const float* pixels;  // [F, 3, res, res]
    const int* frame_off; // [V+1] device
    int F, V, Kp;
    float* X;             // workspace: [F L, W] fp32 residual stream
    void* A;              // workspace: [F L, W] operand
    void* big;            // workspace: QKV [F L, 3W] fp32 / MLP hidden [F L, 4W] operand / patch operand + patch GEMM output
    size_t patch_out;     // byte offset of the patch GEMM output [F g^2, W] fp32 inside big
    float* q_cls;         // workspace: [F, W] fp32 (the class rows' queries of the last block)
    void* a_cls;          // workspace: [F, W] operand (the class rows' LayerNorm / attention output)
    float* out;
    int ldo;
    float* out_mean;
    int ldm;
};
hipError_t launch_clip_image_encode(const ClipImageArgs& e, int fp16, hipStream_t st);

// frame_prep.hip: frame preprocessing (laff_frame_preprocess)
constexpr int FRAME_PREP_LDS_BYTES = 64 * 1024;   // the LDS image of one row tile: two blocks per CU
constexpr int FRAME_PREP_MAX_TILE = 16;
struct FramePrepArgs {
    const unsigned char* frames;   // packed HWC uint8 frames
    const laff_frame_desc* desc;   // [F] device
    const int* taps;               // the tap tables, device
    int F, R, tile;                // tile: output rows per block
    float mean[3], stdv[3];
    float* out_pixels;             // [F, 3, R, R] fp32
    unsigned char* out_u8;         // [F, R, R, 3] uint8 or null
};
hipError_t launch_frame_prep(const FramePrepArgs& a, size_t lds_bytes, hipStream_t st);

// bert.hip: the BERT text encoder (laff_bert_encode) on the transformer core of clip_core.h
constexpr int BERT_MAX_POSITION = 512;
enum { BERT_LN_EMBED = 0, BERT_LN_ROW = 1, BERT_LN_CLS = 2 };
struct BertEncodeArgs {
    const laff_bert_text* model;
    const int* ids;
    const int* row_off;
    int N, R;
    float* X;             // workspace: [R, W] fp32 residual stream
    void* A;              // workspace: [R, W] operand
    void* big;            // workspace: [R, 3W] fp32 (QKV) / [R, I] operand (intermediate)
    float* Xc;            // workspace: [N, W] fp32, the CLS rows' residual stream in the last layer
    float* Qc;            // workspace: [N, W] fp32, their queries
    void* Ac;             // workspace: [N, W] operand
    float* out;
    int ldo;
};
hipError_t launch_bert_encode(const BertEncodeArgs& e, int fp16, hipStream_t st);

// netvlad.hip: the NetVLAD text encoder (laff_netvlad_encode)
constexpr int NETVLAD_MAX_K = 64;
constexpr int NETVLAD_MAX_D = 1024;
struct NetvladArgs {
    const float* table;       // [V, D] word2vec rows
    int V, D, K;
    const int* ids;           // [R] table rows, caption i's are ids[row_off[i] .. row_off[i+1])
    const int* row_off;       // [N+1]
    const int* zero_rows;     // [N] zero rows of a caption without known words
    int N, R;
    const float* fc1;         // [K, D]
    const float* centroids;   // [K, D]
    float* assign;            // workspace: [R, K] soft assignments
    float* rnorm;             // workspace: [R] 1 / max(|x|, eps)
    float* out;
    long ldo;
};
hipError_t launch_netvlad_assign(const NetvladArgs& a, hipStream_t st);      // the first of its two launches alone (R > 0)
hipError_t launch_netvlad_encode(const NetvladArgs& a, hipStream_t st);

// netvlad_bwd.hip: the saving forward and the backward of the NetVLAD encoder (laff_netvlad_encode_train, laff_netvlad_backward)
struct NetvladBwdArgs {
    NetvladArgs f;            // the forward's arguments: assign and rnorm are the reserve's, out the forward's output
    const float* den;         // reserve: [N, K + 1] max(|u_k|, eps) for k < K, then max(|v|, eps)
    const int* clamped;       // reserve: [N, K + 1] 1 where that norm was not above eps
    const float* g;           // [N, ldg] the gradient of out
    long ldg;
    float* du;                // workspace: [N, K, D]
    float* mass;              // workspace: [N, K] s_k
    float* dz;                // workspace: [R, K] the gradient of the logits
    float* part_fc1;          // workspace: [chunks_r, K, D] the sums of d_fc1 over rows_per_chunk token rows each
    float* part_cent;         // workspace: [chunks_n, K, D] the sums of d_centroids over caps_per_chunk captions each
    int rows_per_chunk, chunks_r, caps_per_chunk, chunks_n;
    float* d_fc1;             // [K, D] or null
    float* d_cent;            // [K, D] or null
};
// a.assign / a.rnorm are written (the reserve's regions); den / clamped [N, K + 1] as NetvladBwdArgs reads them
hipError_t launch_netvlad_encode_train(const NetvladArgs& a, float* den, int* clamped, hipStream_t st);
hipError_t launch_netvlad_backward(const NetvladBwdArgs& p, hipStream_t st);

// rerank.hip: k-reciprocal re-ranking (laff_rerank_run) and the neighbour-count re-ranking (laff_rerank_tkb)
constexpr int RERANK_MAX_K1 = 32;
constexpr int RERANK_MAX_K2 = 8;
constexpr int RERANK_MAX_N = 4096;        // items of one problem: four N-float rows in 64 KiB of LDS
constexpr int RERANK_MAX_CAP = 608;       // >= (k1 + 1) * (round(k1 / 2) + 2) at k1 = 32 (594): the expansion set's bound
constexpr int RERANK_GROUP = 16;          // problems per launch (the descriptors travel as kernel arguments)
struct RerankProblem {
    const float *qq, *qg, *gg;            // [Q, Q], [Q, G], [G, G] similarities
    float* out;                           // [Q, G]
    long ldqq, ldqg, ldgg, ldo;
    int Q, G;
    int L1, L2;                           // row pitch of the sparse rows: min(cap, N), min(k2 cap, N)
    int* rank;                            // workspace: [N, k1 + 1] neighbour lists, ascending distance
    float* colmax;                        // workspace: [N] column maxima of 2 - 2 x
    int *cnt1, *idx1;                     // workspace: V before query expansion, [N] entries per row, [N, L1] columns (ascending)
    float* val1;                          //            [N, L1] weights
    int *cnt2, *idx2;                     // workspace: V after query expansion, [N, L2] (the same buffers as *1 when k2 == 1)
    float* val2;
};
struct RerankArgs {
    RerankProblem p[RERANK_GROUP];
    int count, k1, k2, kh;                // kh = round_half_even(k1 / 2)
    float lambda;
};
size_t rerank_lds_bytes(int maxN);
hipError_t launch_rerank(const RerankArgs& a, int maxQ, int maxG, int maxN, hipStream_t st);   // the largest Q, G and Q + G of the set
hipError_t launch_rerank_tkb(const int* nn, int G, int k1, const int* cand, int Q, int K, int* count, float* out, long ldo,
                             hipStream_t st);

// sim_hist.hip: the 'hist' measure (laff_sim_hist): S[t, v] = 1/H sum_h sum_k min / (sum_k max + eps), fp32
struct SimHistArgs {
    const float *T, *V;                   // [Nt, H d], [Nv, H d]
    float* S;                             // [Nt, Nv]
    long ldt, ldv, lds;
    int Nt, Nv, H, d;
    float eps;
    int vec;                              // bit 0 / 1: T / V may be read in 16-byte groups (base, pitch and head width allow it)
    unsigned tilesV;                      // tiles along Nv; blockIdx.x = text tile * tilesV + video tile
};
bool sim_hist_tiles(int Nt, int Nv, unsigned* tilesV, unsigned* tiles);    // false: more tiles than a grid holds
hipError_t launch_sim_hist(const SimHistArgs& a, unsigned tiles, hipStream_t st);

// batch_assemble.hip: a training batch gathered from the resident set in one launch (laff_batch_assemble)
constexpr int ASSEMBLE_JOBS = 16;             // jobs of one launch: the table travels in the launch arguments (16 x 96 bytes)
constexpr int ASSEMBLE_THREADS = 256;
constexpr int ASSEMBLE_ITEMS_PER_THREAD = 4;  // a job gets a block per 1024 items ...
constexpr int ASSEMBLE_BLOCK_CAP = 512;       // ... up to this many, which then stride
struct AssembleJob {
    int kind;                 // LAFF_ASSEMBLE_*
    int vec;                  // rows, ragged: 16-byte pieces (bases and pitches allow it); else one element a piece
    int rows_at, crow_at;     // in the control block: the B source indices; CSR: crow_dst [B + 1]
    int w, ld_src, ld_dst;
    int n_src;                // rows of src (rows), segments (ragged), rows of the source CSR
    int n_items;              // ragged: rows of src; CSR: entries of the source
    int fmax;
    int first_block, blocks;  // filled by launch_batch_assemble
    const void* src;          // CSR: val_src
    const int* off_src;       // ragged: seg_off [n_src + 1]; CSR: crow_src [n_src + 1]
    const int* col_src;
    void* dst;                // CSR: val_dst
    int* col_dst;
    float* mask;
};
struct AssembleTable {
    int count, B;
    const int* control;
    AssembleJob j[ASSEMBLE_JOBS];
};
long long assemble_items(const AssembleJob& j, int B);
hipError_t launch_batch_assemble(AssembleTable& t, hipStream_t st);

}  // namespace laff
