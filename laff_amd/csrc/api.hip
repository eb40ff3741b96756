// api.hip -- extern "C" surface of liblaff_hip.so (see include/laff_hip.h for the contract).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"

constexpr int METRIC_SLOTS = 33;

struct laff_ctx {
    int device;
    hipStream_t stream;
    double* d_metrics = nullptr;   // METRIC_SLOTS x (7 doubles + 1 flag: 0.0 / 1.0 = a rank < 1 was seen, metrics are NaN) on the device
    unsigned metrics_slot = 0;     // every laff_rank_metrics_async call takes the next slot: calls captured into different graphs (or in
                                   // flight on different streams) do not share their result buffer
    double* h_metrics = nullptr;   // pinned host mirror
    char* d_mscratch = nullptr;    // METRIC_SLOTS x rank_metrics_scratch_bytes(): the metrics kernel's partials + histograms, kept zero
};

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(LAFF_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

#define CHECK_CTX(ctx) \
    if (!(ctx)) return fail(LAFF_E_ARG, "%s: null ctx", __func__)
#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

int metrics_buffers(laff_ctx* ctx) {
    if (ctx->d_metrics) return LAFF_OK;
    const size_t sb = laff::rank_metrics_scratch_bytes();
    HIP_TRY(hipMalloc((void**)&ctx->d_mscratch, METRIC_SLOTS * sb));
    HIP_TRY(hipMemset(ctx->d_mscratch, 0, METRIC_SLOTS * sb));
    HIP_TRY(hipHostMalloc((void**)&ctx->h_metrics, 8 * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipMalloc((void**)&ctx->d_metrics, METRIC_SLOTS * 8 * sizeof(double)));
    HIP_TRY(hipMemset(ctx->d_metrics, 0, METRIC_SLOTS * 8 * sizeof(double)));
    return LAFF_OK;
}

// slot 0 serves the synchronous calls; every asynchronous one takes the next of the others
size_t next_metrics_slot(laff_ctx* ctx) { return 1 + ctx->metrics_slot++ % (METRIC_SLOTS - 1); }

// A pinned (hipHostMalloc'ed / registered) result buffer is addressable from the device: the finishing workgroup stores the 64 bytes
// there itself and no copy node follows the launch.  Returns that alias, or null (anything else gets the copy).
double* pinned_alias(double* host8) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, host8, 0) == hipSuccess && dp) return (double*)dp;
    (void)hipGetLastError();
    return nullptr;
}

// the synchronous result: slot 0 back to the host, refused with `flagged` when the kernel saw a rank < 1
int metrics_read_back(laff_ctx* ctx, double out7[7], const char* flagged) {
    HIP_TRY(hipMemcpyAsync(ctx->h_metrics, ctx->d_metrics, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->h_metrics[7] != 0.0) return fail(LAFF_E_ARG, "%s", flagged);
    for (int i = 0; i < 7; ++i) out7[i] = ctx->h_metrics[i];
    return LAFF_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }                       // floats: every region of a float workspace starts on 16 bytes
size_t round256(size_t b) { return (b + 255) / 256 * 256; }                 // bytes: every region of a byte workspace starts on 256 bytes

// the workspace holds `need` bytes; then it and the packed operands named with it in `what` (others_aligned) sit on 16 bytes
int check_workspace(const char* fn, const void* workspace, size_t workspace_bytes, size_t need, bool others_aligned, const char* what) {
    if (workspace_bytes < need) return fail(LAFF_E_ARG, "%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes, need);
    if (!aligned16(workspace) || !others_aligned) return fail(LAFF_E_ALIGN, "%s: %s must be 16-byte aligned", fn, what);
    return LAFF_OK;
}
// the same for a workspace that a caller may leave out: a null one is reported as 0 bytes
int need_workspace(const char* fn, const void* workspace, size_t workspace_bytes, size_t need) {
    return check_workspace(fn, workspace, workspace ? workspace_bytes : (size_t)0, need, true, "workspace");
}

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

bool is_x3(int p) { return p == LAFF_PREC_FP16X3 || p == LAFF_PREC_BF16X3; }
int elem_size(int p) { return p == LAFF_PREC_FP32 ? 4 : 2; }
int bad_precision(const char* who, int p) {
    return p < LAFF_PREC_FP32 || p > LAFF_PREC_BF16X3 ? fail(LAFF_E_ARG, "%s: bad precision %d", who, p) : LAFF_OK;
}

// the FC epilogue of `who` (problem i, or the only one when i < 0): the activation code, bn_scale / bn_shift given together and, with
// `align`, bias / bn_scale / bn_shift 16-byte aligned -- in that order
int check_epilogue(const char* who, int i, int act, const float* bias, const float* bn_scale, const float* bn_shift, bool align) {
    char at[96];
    if (i < 0) snprintf(at, sizeof(at), "%s", who);
    else snprintf(at, sizeof(at), "%s: problem %d", who, i);
    if (act < LAFF_ACT_NONE || act > LAFF_ACT_SIGMOID) return fail(LAFF_E_ARG, "%s: bad act %d", at, act);
    if ((bn_scale == nullptr) != (bn_shift == nullptr)) return fail(LAFF_E_ARG, "%s: bn_scale/bn_shift must come together", at);
    if (align && ((bias && !aligned16(bias)) || (bn_scale && (!aligned16(bn_scale) || !aligned16(bn_shift)))))
        return fail(LAFF_E_ALIGN, "%s: bias / bn_scale / bn_shift must be 16-byte aligned", at);
    return LAFF_OK;
}

// a grouped GEMM launch being assembled, with the index each of its problems has in the caller's list
struct FcGroup {
    laff::GroupedGemmArgs ga{};
    int idx[laff::MAX_GROUP];
};

// adds a problem to a grouped GEMM launch and issues the launch once MAX_GROUP are in; the caller launches the rest
template <typename Launch>
hipError_t group_add(FcGroup& g, const laff::GemmArgs& a, int i, Launch launch) {
    g.idx[g.ga.count] = i;
    g.ga.p[g.ga.count++] = a;
    if (g.ga.count < laff::MAX_GROUP) return hipSuccess;
    const hipError_t e = launch(g);
    g.ga.count = 0;
    return e;
}

// laff_split_rows_grouped (out != null) and laff_row_scales_grouped (out == null: per-row scales only, empty matrices skipped):
// each run of up to 8 matrices is checked, then launched at once
int split_rows_by_eight(laff_ctx* ctx, const char* who, int count, const float* const* X, const int* N, const int* K,
                        const int* ldx, void* const* out, float* const* rscale) {
    DeviceGuard g(ctx->device);
    void* const none[8] = {};
    for (int i0 = 0; i0 < count; i0 += 8) {
        const int c = std::min(count - i0, 8);
        for (int i = i0; i < i0 + c; ++i) {
            if (!out && N[i] == 0) continue;
            if (!X[i] || (out && !out[i]) || !rscale[i]) return fail(LAFF_E_ARG, "%s: matrix %d has a null pointer", who, i);
            if (N[i] < 0 || K[i] < 1 || ldx[i] < K[i]) return fail(LAFF_E_SHAPE, "%s: matrix %d bad shape", who, i);
            if (out && !aligned16(out[i])) return fail(LAFF_E_ALIGN, "%s: out %d must be 16-byte aligned", who, i);
        }
        HIP_TRY(laff::launch_split_rows_grouped(c, X + i0, N + i0, K + i0, ldx + i0, out ? out + i0 : none, rscale + i0, ctx->stream));
    }
    return LAFF_OK;
}

}  // namespace

extern "C" {

int laff_abi_version(void) { return LAFF_ABI_VERSION; }

const char* laff_last_error(void) { return g_err.c_str(); }

int laff_ctx_create(int device, void* hip_stream, laff_ctx** out) {
    if (!out) return fail(LAFF_E_ARG, "laff_ctx_create: null out");
    // tuning knobs: process-wide, re-read whenever a ctx is created; an absent variable means the default (not "the last value": a
    // test that set LAFF_STRIP=2, dropped it and made a new ctx used to leave every later bf16 similarity on the strip kernel)
    auto knob = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    laff::g_strip_mode = knob("LAFF_STRIP", 1);
    laff::g_fc_strip_mfma = knob("LAFF_FC_STRIP_MFMA", 16) == 32 ? 32 : 16;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(LAFF_E_ARG, "laff_ctx_create: device %d out of range (%d devices)", device, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(LAFF_E_UNSUPPORTED, "laff_ctx_create: device %d is %s; this library is built for gfx950 only", device,
                    prop.gcnArchName);
    if (prop.multiProcessorCount > 0) laff::g_num_cus = prop.multiProcessorCount;
    laff_ctx* c = new laff_ctx();
    c->device = device;
    c->stream = static_cast<hipStream_t>(hip_stream);
    *out = c;
    return LAFF_OK;
}

/* internal (comm.hip): the ctx's stream and device; the error text of the calling thread */
int laff_ctx_stream_device(laff_ctx* ctx, void** stream, int* device) {
    CHECK_CTX(ctx);
    *stream = (void*)ctx->stream;
    *device = ctx->device;
    return LAFF_OK;
}
void laff_set_error(const char* msg) { g_err = msg ? msg : ""; }

int laff_ctx_set_stream(laff_ctx* ctx, void* hip_stream) {
    CHECK_CTX(ctx);
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    return LAFF_OK;
}

int laff_ctx_destroy(laff_ctx* ctx) {
    if (ctx) {
        if (ctx->d_metrics) (void)hipFree(ctx->d_metrics);
        if (ctx->d_mscratch) (void)hipFree(ctx->d_mscratch);
        if (ctx->h_metrics) (void)hipHostFree(ctx->h_metrics);
    }
    delete ctx;
    return LAFF_OK;
}

namespace {
__global__ void stamp_kernel(unsigned long long* slot) { *slot = wall_clock64(); }
}  // namespace

int laff_stamp(laff_ctx* ctx, unsigned long long* slot) {
    CHECK_CTX(ctx);
    if (!slot) return fail(LAFF_E_ARG, "laff_stamp: null slot");
    DeviceGuard g(ctx->device);
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, ctx->stream, slot);
    HIP_TRY(hipGetLastError());
    return LAFF_OK;
}

int laff_wall_clock_khz(laff_ctx* ctx, int* khz) {
    CHECK_CTX(ctx);
    if (!khz) return fail(LAFF_E_ARG, "laff_wall_clock_khz: null out");
    HIP_TRY(hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, ctx->device));
    return LAFF_OK;
}

int laff_device_info(laff_ctx* ctx, int out[4]) {
    CHECK_CTX(ctx);
    if (!out) return fail(LAFF_E_ARG, "laff_device_info: null out");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    out[0] = prop.multiProcessorCount;
    out[1] = prop.clockRate / 1000;
    out[2] = (int)prop.sharedMemPerBlock;
    out[3] = prop.warpSize;
    return LAFF_OK;
}

static int fc_problem_args(const laff_fc_problem& q, laff::GemmArgs& a, bool& glds, const char* who, int i) {
    if (q.N == 0) { a = laff::GemmArgs{}; glds = true; return LAFF_OK; }      /* empty problem (skipped by the callers) */
    if (!q.X || !q.W || !q.Y) return fail(LAFF_E_ARG, "%s: problem %d: null X/W/Y", who, i);
    if (q.N < 0 || q.Dk < 1 || q.D < 1 || q.ldx < q.Dk || q.ldw < q.Dk || q.ldy < q.D)
        return fail(LAFF_E_SHAPE, "%s: problem %d: bad shape N=%d Dk=%d D=%d ldx=%d ldw=%d ldy=%d", who, i, q.N, q.Dk, q.D, q.ldx, q.ldw,
                    q.ldy);
    if (int rc = check_epilogue(who, i, q.act, q.bias, q.bn_scale, q.bn_shift, true)) return rc;
    a = laff::GemmArgs{};
    a.R = q.X; a.C = q.W; a.nR = q.N; a.nC = q.D; a.K = q.Dk; a.ldR = q.ldx; a.ldC = q.ldw;
    a.nseg = 1; a.segR[0] = a.segC[0] = 0;
    a.out = q.Y; a.ldo = q.ldy; a.scale = 1.0f;
    a.bias = q.bias; a.bn_scale = q.bn_scale; a.bn_shift = q.bn_shift; a.act = q.act;
    glds = aligned16(q.X) && aligned16(q.W) && (q.ldx % 4 == 0) && (q.ldw % 4 == 0) && (q.Dk % 4 == 0);
    return LAFF_OK;
}

int laff_fc_act_bn_grouped(laff_ctx* ctx, const laff_fc_problem* problems, int count);

int laff_fc_act_bn(laff_ctx* ctx, const float* X, int N, int Dk, int ldx, const float* W, int ldw, const float* bias,
                   const float* bn_scale, const float* bn_shift, int D, int act, float* Y, int ldy) {
    CHECK_CTX(ctx);
    laff_fc_problem q{X, N, Dk, ldx, W, ldw, bias, bn_scale, bn_shift, D, act, Y, ldy};
    return laff_fc_act_bn_grouped(ctx, &q, 1);
}

// laff_fc_act_bn_grouped's walk over its problems: launch(group, kind) gets each launch in order (laff_fc_route passes a recorder).
// Problems are grouped by staging kind (see staging_kind), at most MAX_GROUP per launch; kinds (nullable) receives every kind.
extern "C++" {
template <typename Launch>
static int fc_f32_walk(const laff_fc_problem* problems, int count, int* kinds, Launch launch_kind) {
    for (int kind = 2; kind >= 0; --kind) {
        auto launch = [&](FcGroup& g) { return launch_kind(g, kind); };
        FcGroup g;
        for (int i = 0; i < count; ++i) {
            laff::GemmArgs a;
            bool aligned;
            if (int rc = fc_problem_args(problems[i], a, aligned, "laff_fc_act_bn_grouped", i)) return rc;
            if (problems[i].N == 0) continue;
            const int k = laff::staging_kind(a, 4, aligned);
            if (kinds) kinds[i] = k;
            if (k != kind) continue;
            HIP_TRY(group_add(g, a, i, launch));
        }
        if (g.ga.count) HIP_TRY(launch(g));
    }
    return LAFF_OK;
}
}  // extern "C++"

int laff_fc_act_bn_grouped(laff_ctx* ctx, const laff_fc_problem* problems, int count) {
    CHECK_CTX(ctx);
    if (!problems || count < 0) return fail(LAFF_E_ARG, "laff_fc_act_bn_grouped: bad problem list");
    DeviceGuard g(ctx->device);
    return fc_f32_walk(problems, count, nullptr,
                       [&](FcGroup& fg, int kind) { return laff::launch_gemm_nt_grouped_f32(fg.ga, kind, ctx->stream); });
}

/* checks problem i of a concat launch and, when it is not empty, turns it into the kernel's form */
static int fc_concat_problem_args(const laff_fc_concat_problem& q, laff::ConcatProblem& a, const char* who, int i) {
    if (q.N < 0) return fail(LAFF_E_ARG, "%s: problem %d: negative N=%d", who, i, q.N);
    if (q.N == 0) { a = laff::ConcatProblem{}; return LAFF_OK; }              /* empty problem (skipped): pointers may be null */
    if (!q.segments || q.nseg < 1 || q.nseg > laff::CONCAT_MAX_SEG)
        return fail(LAFF_E_ARG, "%s: problem %d: need 1 <= nseg <= %d segments (nseg=%d)", who, i, laff::CONCAT_MAX_SEG, q.nseg);
    if (q.D < 4 || (q.D & 3) || q.D > 8192 || q.ldy < q.D || (q.ldy & 3) || q.K < 1)
        return fail(LAFF_E_SHAPE, "%s: problem %d: need D %% 4 == 0, 4 <= D <= 8192, ldy >= D, ldy %% 4 == 0, K >= 1 (D=%d ldy=%d K=%d)", who,
                    i, q.D, q.ldy, q.K);
    if (int rc = check_epilogue(who, i, q.act, q.bias, q.bn_scale, q.bn_shift, false)) return rc;
    a = laff::ConcatProblem{};
    bool dense = false;
    for (int s = 0; s < q.nseg; ++s) {
        const laff_fc_concat_segment& g = q.segments[s];
        if (g.Dk < 1) return fail(LAFF_E_SHAPE, "%s: problem %d: segment %d has width Dk=%d", who, i, s, g.Dk);
        if (g.col < 0 || (long long)g.col + g.Dk > q.K)
            return fail(LAFF_E_SHAPE, "%s: problem %d: segment %d: columns [%d, %lld) are outside W's K=%d", who, i, s, g.col,
                        (long long)g.col + g.Dk, q.K);
        for (int t = 0; t < s; ++t) {
            const laff_fc_concat_segment& h = q.segments[t];
            if (g.col < h.col + h.Dk && h.col < g.col + g.Dk)
                return fail(LAFF_E_SHAPE, "%s: problem %d: segments %d and %d overlap in W's columns", who, i, t, s);
        }
        if (g.X) {
            if (g.ldx < g.Dk) return fail(LAFF_E_SHAPE, "%s: problem %d: segment %d: ldx=%d < Dk=%d", who, i, s, g.ldx, g.Dk);
            dense = true;
            laff::ConcatDense& d = a.d[a.nd++];
            d.X = g.X; d.ldx = g.ldx; d.dk = g.Dk; d.c0 = g.col;
            d.fast = ((aligned16(g.X) && g.ldx % 4 == 0 && g.Dk % 4 == 0) ? 1 : 0) |
                     ((q.W && aligned16(q.W) && q.ldw % 4 == 0 && g.col % 4 == 0 && g.Dk % 4 == 0) ? 2 : 0);
        } else {
            if (!g.indptr || !g.indices || !g.Wt)
                return fail(LAFF_E_ARG, "%s: problem %d: segment %d: null X and null indptr / indices / Wt", who, i, s);
            if (g.ldwt < q.D || (g.ldwt & 3))
                return fail(LAFF_E_SHAPE, "%s: problem %d: segment %d: need ldwt >= D, ldwt %% 4 == 0 (ldwt=%d D=%d)", who, i, s, g.ldwt, q.D);
            if (!aligned16(g.Wt)) return fail(LAFF_E_ALIGN, "%s: problem %d: segment %d: Wt must be 16-byte aligned", who, i, s);
            laff::ConcatSparse& p = a.s[a.ns++];
            p.indptr = g.indptr; p.indices = g.indices; p.values = g.values; p.wt = g.Wt; p.ldwt = g.ldwt; p.dk = g.Dk;
        }
    }
    if (dense && (q.ldw < q.K)) return fail(LAFF_E_SHAPE, "%s: problem %d: ldw=%d < K=%d", who, i, q.ldw, q.K);
    if ((dense && !q.W) || !q.Y) return fail(LAFF_E_ARG, "%s: problem %d: null W / Y", who, i);
    if (!aligned16(q.Y)) return fail(LAFF_E_ALIGN, "%s: problem %d: Y must be 16-byte aligned", who, i);
    a.W = q.W; a.bias = q.bias; a.bn_scale = q.bn_scale; a.bn_shift = q.bn_shift; a.Y = q.Y;
    a.N = q.N; a.D = q.D; a.ldw = q.ldw; a.ldy = q.ldy; a.act = q.act;
    return LAFF_OK;
}

int laff_fc_concat_act_bn_grouped(laff_ctx* ctx, const laff_fc_concat_problem* problems, int count) {
    if (!problems || count < 0) return fail(LAFF_E_ARG, "laff_fc_concat_act_bn_grouped: bad problem list");
    std::vector<laff::ConcatProblem> live;
    for (int i = 0; i < count; ++i) {               /* every problem is checked before anything is launched */
        laff::ConcatProblem a;
        if (int rc = fc_concat_problem_args(problems[i], a, "laff_fc_concat_act_bn_grouped", i)) return rc;
        if (problems[i].N > 0) live.push_back(a);
    }
    CHECK_CTX(ctx);
    if (live.empty()) return LAFF_OK;
    DeviceGuard g(ctx->device);
    for (size_t i0 = 0; i0 < live.size(); i0 += laff::CONCAT_MAX_GROUP) {
        laff::ConcatArgs ca{};
        ca.count = (int)std::min(live.size() - i0, (size_t)laff::CONCAT_MAX_GROUP);
        for (int j = 0; j < ca.count; ++j) ca.p[j] = live[i0 + j];
        HIP_TRY(laff::launch_fc_concat(ca, ctx->stream));
    }
    return LAFF_OK;
}

int laff_fc_concat_act_bn(laff_ctx* ctx, const laff_fc_concat_problem* problem) {
    if (!problem) return fail(LAFF_E_ARG, "laff_fc_concat_act_bn: null problem");
    return laff_fc_concat_act_bn_grouped(ctx, problem, 1);
}

int laff_fc_gather_act_bn(laff_ctx* ctx, const int* indptr, const int* indices, const float* values, int N, int Dk,
                          const float* Wt, int ldwt, const float* bias, const float* bn_scale, const float* bn_shift, int D,
                          int act, float* Y, int ldy) {
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!indptr || !indices || !Wt || !Y) return fail(LAFF_E_ARG, "laff_fc_gather_act_bn: null argument");
    if (N < 0 || Dk < 1 || D < 4 || (D & 3) || D > 8192 || ldwt < D || (ldwt & 3) || ldy < D || (ldy & 3))
        return fail(LAFF_E_SHAPE, "laff_fc_gather_act_bn: bad shape N=%d Dk=%d D=%d ldwt=%d ldy=%d", N, Dk, D, ldwt, ldy);
    if (int rc = check_epilogue("laff_fc_gather_act_bn", -1, act, bias, bn_scale, bn_shift, false)) return rc;
    if (!aligned16(Wt) || !aligned16(Y)) return fail(LAFF_E_ALIGN, "laff_fc_gather_act_bn: Wt / Y must be 16-byte aligned");
    if (N == 0) return LAFF_OK;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_fc_gather(indptr, indices, values, N, Dk, Wt, ldwt, bias, bn_scale, bn_shift, D, act, Y, ldy, ctx->stream));
    return LAFF_OK;
}

namespace {
struct LossLayout {
    size_t XH, XHT, nrm, npr, S, dS, dST, G, loss_h, total;   // offsets in floats
    int dp, Bp;
};
LossLayout loss_layout(int B, int H, int d) {
    LossLayout L{};
    L.dp = (d + 3) & ~3;
    L.Bp = (B + 3) & ~3;
    size_t o = 0;
    L.XH = o;     o += up4((size_t)2 * H * B * L.dp);
    L.XHT = o;    o += up4((size_t)2 * H * d * L.Bp);
    L.nrm = o;    o += up4((size_t)2 * H * B);
    L.npr = o;    o += up4((size_t)2 * H * B);
    L.S = o;      o += up4((size_t)H * B * L.Bp);
    L.dS = o;     o += up4((size_t)H * B * L.Bp);
    L.dST = o;    o += up4((size_t)H * B * L.Bp);
    L.G = o;      o += up4((size_t)2 * H * B * L.dp);
    L.loss_h = o; o += up4((size_t)H);
    L.total = o;
    return L;
}
// the upper end of the B range of the loss entry points (they share the reduction's shape; each checks its own lower end)
int loss_check_batch(const char* fn, int B) {
    if (B > 16384) return fail(LAFF_E_SHAPE, "%s: bad shape B=%d", fn, B);
    if ((size_t)(2 * B + 16) * sizeof(float) > 64 * 1024) return fail(LAFF_E_UNSUPPORTED, "%s: B=%d exceeds the reduction kernel's LDS budget", fn, B);
    return LAFF_OK;
}
// The pipeline the embedding losses share around their own reduce launch.  `row` says which side's rows are the rows of the score
// matrices, 0 = captions (s), 1 = videos (im); the other side is the column operand.
float* loss_head(float* ws, size_t region, int side, int h, int H, size_t floats) { return ws + region + ((size_t)side * H + h) * floats; }
// normalize both sides, then per head  scores_h [B rows, B columns] = Row^_h . Col^_h^T  into L.S
int loss_scores(laff_ctx* ctx, const float* s, const float* im, int B, int H, int d, const LossLayout& L, float* ws, int row) {
    HIP_TRY(laff::launch_loss_normalize(s, im, B, H, d, L.dp, L.Bp, 1e-13f, ws + L.XH, ws + L.XHT, ws + L.nrm, ws + L.npr, ctx->stream));
    std::vector<laff_fc_problem> probs((size_t)H);
    for (int h = 0; h < H; ++h)
        probs[h] = laff_fc_problem{loss_head(ws, L.XH, row, h, H, (size_t)B * L.dp), B, d, L.dp, loss_head(ws, L.XH, 1 - row, h, H, (size_t)B * L.dp),
                                   L.dp, nullptr, nullptr, nullptr, B, LAFF_ACT_NONE, ws + L.S + (size_t)h * B * L.Bp, L.Bp};
    return laff_fc_act_bn_grouped(ctx, probs.data(), H);
}
// from dS_h = dL/dscores_h in L.dS and its transpose in L.dST, per head  dL/dRow^_h = dS_h . Col^_h  (column operand = Col^_h^T, K = the
// column side's items)  and  dL/dCol^_h = dS_h^T . Row^_h;  then the backward of the normalisation into d_s, d_im
int loss_grads(laff_ctx* ctx, int B, int H, int d, const LossLayout& L, float* ws, int row, float* d_s, float* d_im) {
    std::vector<laff_fc_problem> probs;
    for (int h = 0; h < H; ++h) {
        probs.push_back(laff_fc_problem{ws + L.dS + (size_t)h * B * L.Bp, B, B, L.Bp, loss_head(ws, L.XHT, 1 - row, h, H, (size_t)d * L.Bp), L.Bp,
                                        nullptr, nullptr, nullptr, d, LAFF_ACT_NONE, loss_head(ws, L.G, row, h, H, (size_t)B * L.dp), L.dp});
        probs.push_back(laff_fc_problem{ws + L.dST + (size_t)h * B * L.Bp, B, B, L.Bp, loss_head(ws, L.XHT, row, h, H, (size_t)d * L.Bp), L.Bp,
                                        nullptr, nullptr, nullptr, d, LAFF_ACT_NONE, loss_head(ws, L.G, 1 - row, h, H, (size_t)B * L.dp), L.dp});
    }
    if (int rc = laff_fc_act_bn_grouped(ctx, probs.data(), (int)probs.size())) return rc;
    HIP_TRY(laff::launch_loss_normalize_bwd(ws + L.XH, ws + L.G, ws + L.nrm, ws + L.npr, B, H, d, L.dp, d_s, d_im, ctx->stream));
    return LAFF_OK;
}
// what the LAFF_LOSS_* flags of the margin criteria ask of margin_reduce_kernel
struct MarginFlags {
    int maxv, use_s, use_im;
    float gw;                 // the weight of a hinge term: 1, or the mean's 1 / B (max violation) or 1 / B^2
    MarginFlags(unsigned flags, int B)
        : maxv((flags & LAFF_LOSS_MAX_VIOLATION) ? 1 : 0), use_s((flags & LAFF_LOSS_DIR_I2T) ? 1 : 0), use_im((flags & LAFF_LOSS_DIR_T2I) ? 1 : 0),
          gw(!(flags & LAFF_LOSS_COST_MEAN) ? 1.0f : maxv ? 1.0f / (float)B : 1.0f / ((float)B * (float)B)) {}
};
}  // namespace

int laff_margin_loss_workspace_bytes(int B, int H, int d, size_t* out) {
    if (!out || B < 1 || H < 1 || d < 1) return fail(LAFF_E_ARG, "laff_margin_loss_workspace_bytes: bad args");
    *out = loss_layout(B, H, d).total * sizeof(float);
    return LAFF_OK;
}

int laff_margin_loss(laff_ctx* ctx, const float* s, const float* im, int B, int H, int d, float margin, unsigned flags,
                     float* loss, float* d_s, float* d_im, void* workspace, size_t workspace_bytes) {
    CHECK_CTX(ctx);
    if (!s || !im || !loss || !workspace) return fail(LAFF_E_ARG, "laff_margin_loss: null argument");
    if (B < 1 || H < 1 || d < 1) return fail(LAFF_E_SHAPE, "laff_margin_loss: bad shape B=%d H=%d d=%d", B, H, d);
    // the upper limit of B is a shape error and keeps its place in front of the flags / workspace checks (the order of the error
    // codes is part of the ABI); the LDS budget, an 'unsupported', stays behind them, below
    if (B > 16384) return loss_check_batch("laff_margin_loss", B);
    if (flags & ~15u) return fail(LAFF_E_ARG, "laff_margin_loss: unknown flags 0x%x", flags);
    const LossLayout L = loss_layout(B, H, d);
    if (int rc = need_workspace("laff_margin_loss", workspace, workspace_bytes, L.total * sizeof(float))) return rc;
    if (int rc = loss_check_batch("laff_margin_loss", B)) return rc;
    DeviceGuard g(ctx->device);
    float* ws = (float*)workspace;
    const MarginFlags f(flags, B);
    if (int rc = loss_scores(ctx, s, im, B, H, d, L, ws, 1)) return rc;      // scores_h [B videos, B captions] = I^_h . S^_h^T
    HIP_TRY(laff::launch_margin_reduce(ws + L.S, ws + L.dS, ws + L.dST, ws + L.loss_h, loss, B, L.Bp, H, margin, f.maxv, f.use_s, f.use_im,
                                       f.gw, f.gw, ctx->stream));
    if (!d_s && !d_im) return LAFF_OK;
    return loss_grads(ctx, B, H, d, L, ws, 1, d_s, d_im);
}

namespace {
struct DslLayout {
    LossLayout L;
    size_t ST, stat, total;   // offsets in floats, behind the margin loss's layout
};
DslLayout dsl_layout(int B, int H, int d) {
    DslLayout D{};
    D.L = loss_layout(B, H, d);
    size_t o = D.L.total;
    D.ST = o;   o += up4((size_t)H * B * D.L.Bp);
    D.stat = o; o += up4((size_t)H * laff::DSL_STAT_ROWS * B);
    D.total = o;
    return D;
}
}  // namespace

int laff_dsl_loss_workspace_bytes(int B, int H, int d, size_t* out) {
    if (!out || B < 0 || H < 1 || d < 1) return fail(LAFF_E_ARG, "laff_dsl_loss_workspace_bytes: bad args");
    *out = B ? dsl_layout(B, H, d).total * sizeof(float) : 0;
    return LAFF_OK;
}

int laff_dsl_loss(laff_ctx* ctx, const float* s, const float* im, int B, int H, int d, float temp, float* loss, float* d_s,
                  float* d_im, void* workspace, size_t workspace_bytes) {
    CHECK_CTX(ctx);
    if (B < 0 || H < 1 || d < 1) return fail(LAFF_E_SHAPE, "laff_dsl_loss: bad shape B=%d H=%d d=%d", B, H, d);
    if (int rc = loss_check_batch("laff_dsl_loss", B)) return rc;
    if (!(temp > 0.0f) || !std::isfinite(temp)) return fail(LAFF_E_ARG, "laff_dsl_loss: temp must be positive and finite, got %g", (double)temp);
    if (B == 0) return LAFF_OK;
    if (!s || !im || !loss) return fail(LAFF_E_ARG, "laff_dsl_loss: null argument");
    const DslLayout D = dsl_layout(B, H, d);
    const LossLayout& L = D.L;
    if (int rc = need_workspace("laff_dsl_loss", workspace, workspace_bytes, D.total * sizeof(float))) return rc;
    DeviceGuard g(ctx->device);
    float* ws = (float*)workspace;
    const bool grad = d_s || d_im;
    if (int rc = loss_scores(ctx, s, im, B, H, d, L, ws, 0)) return rc;      // M_h [B captions, B videos] = S^_h . I^_h^T  (cosine_sim(s, im), loss.py:296)
    HIP_TRY(laff::launch_dsl_reduce(ws + L.S, ws + D.ST, ws + D.stat, grad ? ws + L.dS : nullptr, grad ? ws + L.dST : nullptr,
                                    ws + L.loss_h, loss, B, L.Bp, H, temp, ctx->stream));
    if (!grad) return LAFF_OK;
    return loss_grads(ctx, B, H, d, L, ws, 0, d_s, d_im);
}

int laff_margin_loss_scores(laff_ctx* ctx, const float* score, int ld, int B, float margin, unsigned flags, float* loss,
                            float* d_score) {
    CHECK_CTX(ctx);
    if (B < 0 || (B > 0 && ld < B)) return fail(LAFF_E_SHAPE, "laff_margin_loss_scores: bad shape B=%d ld=%d", B, ld);
    if (int rc = loss_check_batch("laff_margin_loss_scores", B)) return rc;
    if (flags & ~15u) return fail(LAFF_E_ARG, "laff_margin_loss_scores: unknown flags 0x%x", flags);
    if (B == 0) return LAFF_OK;
    if (!score || !loss) return fail(LAFF_E_ARG, "laff_margin_loss_scores: null argument");
    DeviceGuard g(ctx->device);
    const MarginFlags f(flags, B);
    // margin_reduce_kernel as it is, one head: the score matrix in place of the GEMM's, its pitch as Bp, no transposed gradient, and
    // loss[0] as the per-head slot that the head sum then copies onto itself
    HIP_TRY(laff::launch_margin_reduce(score, d_score, nullptr, loss, loss, B, ld, 1, margin, f.maxv, f.use_s, f.use_im, f.gw, f.gw, ctx->stream));
    return LAFF_OK;
}

namespace {
// the GRU encoder's limits and workspace: per direction two ping-pong h buffers (packed) and the pooled sums, N rounded up to the
// 64-row tile of the step kernel (its operand reads cover whole tiles; the padding rows stay zero)
int gru_check_size(const char* fn, int H, int num_layers) {
    if (num_layers != 1) return fail(LAFF_E_UNSUPPORTED, "%s: num_layers=%d: only one-layer GRUs are supported (rnn_layer = 1)", fn, num_layers);
    if (H < 32 || H > 2048 || H % 32) return fail(LAFF_E_SHAPE, "%s: H=%d: the hidden size must be a multiple of 32 in [32, 2048]", fn, H);
    return LAFF_OK;
}
int gru_check_mode(const char* fn, int bidirectional, int pooling) {
    if (pooling < LAFF_GRU_MEAN || pooling > LAFF_GRU_MEAN_LAST) return fail(LAFF_E_ARG, "%s: bad pooling %d", fn, pooling);
    if (bidirectional && pooling == LAFF_GRU_MEAN_LAST)
        return fail(LAFF_E_UNSUPPORTED, "%s: bigru_mean_last is not supported (the reference fails on it as well)", fn);
    return LAFF_OK;
}
int gru_dirs(int bidirectional, int pooling) { return bidirectional && pooling == LAFF_GRU_MEAN ? 2 : 1; }
size_t gru_npad(int N) { return ((size_t)N + 63) / 64 * 64; }
}  // namespace

int laff_gru_pack_whh(laff_ctx* ctx, const float* W_hh, int H, float* packed) {
    if (int rc = gru_check_size("laff_gru_pack_whh", H, 1)) return rc;
    if (!W_hh || !packed) return fail(LAFF_E_ARG, "laff_gru_pack_whh: null argument");
    if (!aligned16(packed)) return fail(LAFF_E_ALIGN, "laff_gru_pack_whh: packed must be 16-byte aligned");
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_gru_pack_whh(W_hh, H, packed, ctx->stream));
    return LAFF_OK;
}

int laff_gru_workspace_bytes(int N, int H, int num_layers, int bidirectional, int pooling, size_t* out) {
    if (!out || N < 0) return fail(LAFF_E_ARG, "laff_gru_workspace_bytes: bad args");
    if (int rc = gru_check_size("laff_gru_workspace_bytes", H, num_layers)) return rc;
    if (int rc = gru_check_mode("laff_gru_workspace_bytes", bidirectional, pooling)) return rc;
    *out = (size_t)gru_dirs(bidirectional, pooling) * 3 * gru_npad(N) * H * sizeof(float);
    return LAFF_OK;
}

// laff_gru_encode, and with a reserve laff_gru_encode_train: the same steps with the saving kernel, V = M = sum of batch_sizes
static int gru_encode_run(const char* fn, laff_ctx* ctx, const int* tokens, const int* lengths, const int* perm, const int* batch_sizes,
                          int T, int N, int V, int H, int num_layers, int bidirectional, int pooling, const float* P_fwd,
                          const float* whh_fwd, const float* bhh_fwd, const float* P_rev, const float* whh_rev, const float* bhh_rev,
                          float* out, int ldo, void* workspace, size_t workspace_bytes, bool train, void* reserve, size_t reserve_bytes) {
    // every argument is checked before any GPU work
    if (int rc = gru_check_size(fn, H, num_layers)) return rc;
    if (int rc = gru_check_mode(fn, bidirectional, pooling)) return rc;
    if (N < 0 || T < 0 || V < 1) return fail(LAFF_E_SHAPE, "%s: bad shape N=%d T=%d V=%d", fn, N, T, V);
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    const int ndirs = gru_dirs(bidirectional, pooling);
    if (!tokens || !lengths || !perm || !batch_sizes || !P_fwd || !whh_fwd || !bhh_fwd || !out || !workspace ||
        (ndirs == 2 && (!P_rev || !whh_rev || !bhh_rev)))
        return fail(LAFF_E_ARG, "%s: null argument", fn);
    if (T < 1) return fail(LAFF_E_SHAPE, "%s: T=%d: every caption has at least one token", fn, T);
    const int width = pooling == LAFF_GRU_LAST ? H : (pooling == LAFF_GRU_MEAN_LAST ? 2 * H : ndirs * H);
    if (ldo < width) return fail(LAFF_E_SHAPE, "%s: ldo=%d < output width %d", fn, ldo, width);
    if (batch_sizes[0] != N) return fail(LAFF_E_ARG, "%s: batch_sizes[0]=%d != N=%d", fn, batch_sizes[0], N);
    for (int t = 0; t < T; ++t)
        if (batch_sizes[t] < 1 || (t && batch_sizes[t] > batch_sizes[t - 1]))
            return fail(LAFF_E_ARG, "%s: batch_sizes must be positive and non-increasing (batch_sizes[%d]=%d)", fn, t, batch_sizes[t]);
    const size_t npad = gru_npad(N), plane = npad * H;
    const size_t need = (size_t)ndirs * 3 * plane * sizeof(float);
    if (workspace_bytes < need) return fail(LAFF_E_ARG, "%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes, need);
    if (!aligned16(workspace) || !aligned16(whh_fwd) || (ndirs == 2 && !aligned16(whh_rev)))
        return fail(LAFF_E_ALIGN, "%s: workspace / packed W_hh must be 16-byte aligned", fn);
    std::vector<int> off;
    if (train) {
        long M = 0;
        off.resize(T);
        for (int t = 0; t < T; ++t) {
            off[t] = (int)M;
            M += batch_sizes[t];
        }
        if (M != V) return fail(LAFF_E_ARG, "%s: M=%d but batch_sizes sum to %ld", fn, V, M);
        const size_t rneed = (size_t)ndirs * 5 * M * H * sizeof(float);
        if (!reserve || reserve_bytes < rneed)
            return fail(LAFF_E_ARG, "%s: reserve too small (%zu < %zu bytes)", fn, reserve ? reserve_bytes : (size_t)0, rneed);
        if (!aligned16(reserve)) return fail(LAFF_E_ALIGN, "%s: reserve must be 16-byte aligned", fn);
    }
    if (!ctx) return fail(LAFF_E_ARG, "%s: null ctx", fn);
    DeviceGuard g(ctx->device);
    // h_0 = 0 and the sums start at 0; a reverse-direction row reads its buffer untouched (zero) at its first step
    HIP_TRY(hipMemsetAsync(workspace, 0, need, ctx->stream));
    float* ws = (float*)workspace;
    laff::GruStepArgs a{};
    a.tokens = tokens;
    a.lens = lengths;
    a.perm = perm;
    a.N = N;
    a.H = H;
    a.V = V;
    a.pooling = pooling;
    a.out = out;
    a.ldo = ldo;
    laff::GruDirArgs* dir[2] = {&a.d0, &a.d1};
    const float* P[2] = {P_fwd, P_rev};
    const float* W[2] = {whh_fwd, whh_rev};
    const float* bh[2] = {bhh_fwd, bhh_rev};
    for (int d = 0; d < ndirs; ++d) {
        dir[d]->P = P[d];
        dir[d]->Wp = W[d];
        dir[d]->bhh = bh[d];
        dir[d]->sum = ws + (3 * d + 2) * plane;
        dir[d]->col0 = d * H;
        if (train) dir[d]->res = (float*)reserve + (size_t)d * 5 * V * H;
    }
    if (train) a.M = V;
    for (int i = 0; i < T; ++i) {
        for (int d = 0; d < ndirs; ++d) {
            const int t = d ? T - 1 - i : i;      // the reverse direction walks the same sorted prefix backwards
            dir[d]->t = t;
            dir[d]->B = batch_sizes[t];
            dir[d]->h_in = ws + (3 * d + (i & 1)) * plane;
            dir[d]->h_out = ws + (3 * d + ((i + 1) & 1)) * plane;
            if (train) dir[d]->off = off[t];
        }
        a.skip_gemm = i == 0;                     // h = 0 for every row of the first step of either direction
        HIP_TRY(laff::launch_gru_step(a, ndirs, ctx->stream, train));
    }
    return LAFF_OK;
}

int laff_gru_encode(laff_ctx* ctx, const int* tokens, const int* lengths, const int* perm, const int* batch_sizes, int T, int N, int V,
                    int H, int num_layers, int bidirectional, int pooling, const float* P_fwd, const float* whh_fwd,
                    const float* bhh_fwd, const float* P_rev, const float* whh_rev, const float* bhh_rev, float* out, int ldo,
                    void* workspace, size_t workspace_bytes) {
    return gru_encode_run("laff_gru_encode", ctx, tokens, lengths, perm, batch_sizes, T, N, V, H, num_layers, bidirectional, pooling, P_fwd,
                          whh_fwd, bhh_fwd, P_rev, whh_rev, bhh_rev, out, ldo, workspace, workspace_bytes, false, nullptr, 0);
}

/* ---- the differentiable GRU encoder ---- */
namespace {
// M = sum of batch_sizes after the checks that laff_gru_encode makes of them; < 0: the error code
long gru_packed_rows(const char* fn, const int* batch_sizes, int T, int N) {
    if (!batch_sizes) return fail(LAFF_E_ARG, "%s: null batch_sizes", fn);
    if (T < 1) return fail(LAFF_E_SHAPE, "%s: T=%d: every caption has at least one token", fn, T);
    if (batch_sizes[0] != N) return fail(LAFF_E_ARG, "%s: batch_sizes[0]=%d != N=%d", fn, batch_sizes[0], N);
    long M = 0;
    for (int t = 0; t < T; ++t) {
        if (batch_sizes[t] < 1 || (t && batch_sizes[t] > batch_sizes[t - 1]))
            return fail(LAFF_E_ARG, "%s: batch_sizes must be positive and non-increasing (batch_sizes[%d]=%d)", fn, t, batch_sizes[t]);
        M += batch_sizes[t];
    }
    if (M > INT_MAX / 8) return fail(LAFF_E_SHAPE, "%s: %ld packed rows in one call", fn, M);
    return M;
}

// where laff_gru_backward keeps what in its workspace, in bytes from its start; every region starts on 256 bytes
struct GruBwdLayout {
    size_t carry, dgi, dgh, dx, fc, total;
};
GruBwdLayout gru_bwd_layout(int N, long M, int H, int we_dim, int ndirs, bool want_dwe) {
    GruBwdLayout l{};
    size_t at = 0;
    l.carry = at; at += round256((size_t)ndirs * N * H * sizeof(float));
    l.dgi = at;   at += round256((size_t)ndirs * M * 3 * H * sizeof(float));
    l.dgh = at;   at += round256((size_t)ndirs * M * 3 * H * sizeof(float));
    l.dx = at;    at += want_dwe ? round256((size_t)ndirs * M * we_dim * sizeof(float)) : 0;
    laff::FcBwdPlan hh, ih;
    laff::fc_bwd_plan((int)M, H, 3 * H, &hh);
    laff::fc_bwd_plan((int)M, we_dim, 3 * H, &ih);
    l.fc = at;    at += round256(std::max(std::max(hh.ws_dw, ih.ws_dw), want_dwe ? ih.ws_dx : (size_t)0));
    l.total = at;
    return l;
}

// the arguments of launch_fc_backward for  dZ = dA (.) act'(A),  dW [D, Dk] = dZ^T X,  db = column sums of dZ,  dX = dZ W  (null outputs
// are left out); `vec` allows the 16-byte loads per operand: its base on 16 bytes and its pitch a multiple of 4
laff::FcBwdArgs fc_bwd_args(const float* X, int N, int Dk, int ldx, const float* W, int ldw, int D, int act, const float* A, int lda,
                            const float* dA, int ldda, float* dX, int lddx, float* dW, int lddw, float* db, void* workspace) {
    laff::FcBwdArgs a{};
    a.X = X; a.W = W; a.A = A; a.dA = dA; a.dX = dX; a.dW = dW; a.db = db;
    a.N = N; a.Dk = Dk; a.D = D; a.ldx = ldx; a.ldw = ldw; a.lda = lda; a.ldda = ldda; a.lddx = lddx; a.lddw = lddw; a.act = act;
    a.vec = (aligned16(A) && aligned16(dA) && lda % 4 == 0 && ldda % 4 == 0 ? 1u : 0u) | (X && aligned16(X) && ldx % 4 == 0 ? 2u : 0u) |
            (W && aligned16(W) && ldw % 4 == 0 ? 4u : 0u);
    a.part = (float*)workspace;
    return a;
}
// the GRU's weight gradients: activation none (A = dA), dense rows
hipError_t gru_fc_backward(const float* X, int Dk, const float* W, const float* dA, int M, int D, float* dX, float* dW, float* db,
                           void* fc_ws, hipStream_t st) {
    if (!dX && !dW && !db) return hipSuccess;
    return laff::launch_fc_backward(fc_bwd_args(X, M, Dk, Dk, W, Dk, D, LAFF_ACT_NONE, dA, D, dA, D, dX, Dk, dW, Dk, db, fc_ws), st);
}
}  // namespace

int laff_gru_pack_whh_t(laff_ctx* ctx, const float* W_hh, int H, float* packed) {
    if (int rc = gru_check_size("laff_gru_pack_whh_t", H, 1)) return rc;
    if (!W_hh || !packed) return fail(LAFF_E_ARG, "laff_gru_pack_whh_t: null argument");
    if (!aligned16(packed)) return fail(LAFF_E_ALIGN, "laff_gru_pack_whh_t: packed must be 16-byte aligned");
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_gru_pack_whh_t(W_hh, H, packed, ctx->stream));
    return LAFF_OK;
}

int laff_gru_gather_rows(laff_ctx* ctx, const float* table, int V, int D, const int* ids, int M, float* X) {
    if (V < 1 || D < 1 || M < 0) return fail(LAFF_E_SHAPE, "laff_gru_gather_rows: bad shape V=%d D=%d M=%d", V, D, M);
    if (M == 0) return LAFF_OK;
    if (!table || !ids || !X) return fail(LAFF_E_ARG, "laff_gru_gather_rows: null argument");
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_gru_gather_rows(table, V, D, ids, M, X, ctx->stream));
    return LAFF_OK;
}

int laff_gru_train_reserve_bytes(int M, int H, int num_layers, int bidirectional, int pooling, size_t* out) {
    if (!out || M < 0) return fail(LAFF_E_ARG, "laff_gru_train_reserve_bytes: bad args");
    if (int rc = gru_check_size("laff_gru_train_reserve_bytes", H, num_layers)) return rc;
    if (int rc = gru_check_mode("laff_gru_train_reserve_bytes", bidirectional, pooling)) return rc;
    *out = (size_t)gru_dirs(bidirectional, pooling) * 5 * M * H * sizeof(float);
    return LAFF_OK;
}

int laff_gru_encode_train(laff_ctx* ctx, const int* pos, const int* lengths, const int* perm, const int* batch_sizes, int T, int N, int M,
                          int H, int num_layers, int bidirectional, int pooling, const float* GI_fwd, const float* whh_fwd,
                          const float* bhh_fwd, const float* GI_rev, const float* whh_rev, const float* bhh_rev, float* out, int ldo,
                          void* workspace, size_t workspace_bytes, void* reserve, size_t reserve_bytes) {
    return gru_encode_run("laff_gru_encode_train", ctx, pos, lengths, perm, batch_sizes, T, N, M, H, num_layers, bidirectional, pooling,
                          GI_fwd, whh_fwd, bhh_fwd, GI_rev, whh_rev, bhh_rev, out, ldo, workspace, workspace_bytes, true, reserve,
                          reserve_bytes);
}

int laff_gru_backward_plan(const int* batch_sizes, int T, int H, int bidirectional, int pooling, int* fwd_big, int* bwd_big) {
    const char* fn = "laff_gru_backward_plan";
    if (int rc = gru_check_size(fn, H, 1)) return rc;
    if (int rc = gru_check_mode(fn, bidirectional, pooling)) return rc;
    if (!fwd_big || !bwd_big) return fail(LAFF_E_ARG, "%s: null out", fn);
    const long M = gru_packed_rows(fn, batch_sizes, T, batch_sizes ? batch_sizes[0] : 0);
    if (M < 0) return (int)M;
    const int ndirs = gru_dirs(bidirectional, pooling);
    for (int i = 0; i < T; ++i) {
        /* launch i of the forward: step i with, in a bigru, the reverse direction's step T - 1 - i; launch i of the backward: the same two,
           each walked the other way */
        const int Bf = std::max(batch_sizes[i], ndirs > 1 ? batch_sizes[T - 1 - i] : 0);
        const int Bb = std::max(batch_sizes[T - 1 - i], ndirs > 1 ? batch_sizes[i] : 0);
        fwd_big[i] = laff::gru_step_big(Bf, H, ndirs) ? 1 : 0;
        bwd_big[i] = laff::gru_step_big(Bb, H, ndirs) ? 1 : 0;
    }
    return LAFF_OK;
}

int laff_gru_backward_workspace_bytes(const int* batch_sizes, int T, int N, int H, int we_dim, int num_layers, int bidirectional,
                                      int pooling, int want_dwe, size_t* out) {
    const char* fn = "laff_gru_backward_workspace_bytes";
    if (!out || N < 0 || we_dim < 1) return fail(LAFF_E_ARG, "%s: bad args", fn);
    if (int rc = gru_check_size(fn, H, num_layers)) return rc;
    if (int rc = gru_check_mode(fn, bidirectional, pooling)) return rc;
    if (N == 0) {
        *out = 0;
        return LAFF_OK;
    }
    const long M = gru_packed_rows(fn, batch_sizes, T, N);
    if (M < 0) return (int)M;
    *out = gru_bwd_layout(N, M, H, we_dim, gru_dirs(bidirectional, pooling), want_dwe != 0).total;
    return LAFF_OK;
}

int laff_gru_backward(laff_ctx* ctx, const int* lengths, const int* perm, const int* batch_sizes, int T, int N, int M, int H, int we_dim,
                      int num_layers, int bidirectional, int pooling, const float* dout, int lddo, const void* reserve,
                      size_t reserve_bytes, const float* X, const float* wih_fwd, const float* whht_fwd, const float* wih_rev,
                      const float* whht_rev, const int* seg_off, const int* seg_tok, const int* seg_pos, int U, int V, float* d_we,
                      float* const grads_fwd[4], float* const grads_rev[4], void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_gru_backward";
    if (int rc = gru_check_size(fn, H, num_layers)) return rc;
    if (int rc = gru_check_mode(fn, bidirectional, pooling)) return rc;
    if (N < 0 || M < 0 || we_dim < 1 || U < 0 || V < 1)
        return fail(LAFF_E_SHAPE, "%s: bad shape N=%d M=%d we_dim=%d U=%d V=%d", fn, N, M, we_dim, U, V);
    if (N == 0) return LAFF_OK;
    const int ndirs = gru_dirs(bidirectional, pooling);
    const long Msum = gru_packed_rows(fn, batch_sizes, T, N);
    if (Msum < 0) return (int)Msum;
    if (Msum != M) return fail(LAFF_E_ARG, "%s: M=%d but batch_sizes sum to %ld", fn, M, Msum);
    if (!lengths || !perm || !dout || !reserve || !whht_fwd || !grads_fwd || (ndirs == 2 && (!whht_rev || !grads_rev)) || !workspace)
        return fail(LAFF_E_ARG, "%s: null argument", fn);
    float* const none[4] = {nullptr, nullptr, nullptr, nullptr};
    float* const* G[2] = {grads_fwd, ndirs == 2 ? grads_rev : none};            /* dW_ih, dW_hh, db_ih, db_hh of a direction */
    const float* wih[2] = {wih_fwd, wih_rev};
    const float* whht[2] = {whht_fwd, whht_rev};
    const bool want_dwe = d_we != nullptr;
    bool need_x = false;
    for (int d = 0; d < ndirs; ++d) need_x = need_x || G[d][0];
    if (need_x && !X) return fail(LAFF_E_ARG, "%s: null X (read for dW_ih)", fn);
    if (want_dwe && (!wih_fwd || (ndirs == 2 && !wih_rev) || !seg_off || !seg_tok || !seg_pos))
        return fail(LAFF_E_ARG, "%s: d_we needs W_ih of every direction and the token segments", fn);
    if (U > M) return fail(LAFF_E_ARG, "%s: U=%d distinct tokens in M=%d positions", fn, U, M);
    const int width = pooling == LAFF_GRU_LAST ? H : (pooling == LAFF_GRU_MEAN_LAST ? 2 * H : ndirs * H);
    if (lddo < width) return fail(LAFF_E_SHAPE, "%s: lddo=%d < output width %d", fn, lddo, width);
    const size_t rneed = (size_t)ndirs * 5 * M * H * sizeof(float);
    if (reserve_bytes < rneed) return fail(LAFF_E_ARG, "%s: reserve too small (%zu < %zu bytes)", fn, reserve_bytes, rneed);
    const GruBwdLayout L = gru_bwd_layout(N, M, H, we_dim, ndirs, want_dwe);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, L.total,
                                 aligned16(reserve) && aligned16(whht_fwd) && (ndirs != 2 || aligned16(whht_rev)),
                                 "workspace / reserve / packed W_hh"))
        return rc;
    for (int d = 0; d < ndirs; ++d)
        for (int k = 0; k < 4; ++k)
            if (reinterpret_cast<uintptr_t>(G[d][k]) & 3) return fail(LAFF_E_ALIGN, "%s: the gradients must be 4-byte aligned", fn);
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    char* ws = (char*)workspace;
    float* carry = (float*)(ws + L.carry);
    float* dgi = (float*)(ws + L.dgi);
    float* dgh = (float*)(ws + L.dgh);
    float* dx = want_dwe ? (float*)(ws + L.dx) : nullptr;
    HIP_TRY(hipMemsetAsync(carry, 0, (size_t)ndirs * N * H * sizeof(float), ctx->stream));   // no carry into a row's first backward step
    std::vector<int> off(T);
    for (int t = 0, m = 0; t < T; ++t) {
        off[t] = m;
        m += batch_sizes[t];
    }
    const size_t MH = (size_t)M * H;
    laff::GruBwdStepArgs a{};
    a.lens = lengths;
    a.perm = perm;
    a.dout = dout;
    a.lddo = lddo;
    a.N = N;
    a.H = H;
    a.M = M;
    a.pooling = pooling;
    laff::GruBwdDirArgs* dir[2] = {&a.d0, &a.d1};
    for (int d = 0; d < ndirs; ++d) {
        dir[d]->WpT = whht[d];
        dir[d]->res = (const float*)reserve + (size_t)d * 5 * MH;
        dir[d]->carry = carry + (size_t)d * N * H;
        dir[d]->col0 = d * H;
    }
    for (int i = 0; i < T; ++i) {
        for (int d = 0; d < ndirs; ++d) {
            const int t = d ? i : T - 1 - i;            // each direction walks its own steps backwards
            const int nb = d ? t - 1 : t + 1;           // the step that consumed h_t
            float* gi = dgi + (size_t)d * 3 * MH;
            float* gh = dgh + (size_t)d * 3 * MH;
            dir[d]->t = t;
            dir[d]->off = off[t];
            dir[d]->B = batch_sizes[t];
            dir[d]->Bnb = nb < 0 || nb >= T ? 0 : std::min(batch_sizes[nb], batch_sizes[t]);
            dir[d]->dgh_nb = dir[d]->Bnb ? gh + (size_t)off[nb] * 3 * H : gh;
            dir[d]->dgi = gi + (size_t)off[t] * 3 * H;
            dir[d]->dgh = gh + (size_t)off[t] * 3 * H;
        }
        HIP_TRY(laff::launch_gru_bwd_step(a, ndirs, ctx->stream));
    }
    for (int d = 0; d < ndirs; ++d) {
        const float* gi = dgi + (size_t)d * 3 * MH;
        const float* gh = dgh + (size_t)d * 3 * MH;
        const float* hprev = (const float*)reserve + (size_t)d * 5 * MH + 4 * MH;
        HIP_TRY(gru_fc_backward(hprev, H, nullptr, gh, M, 3 * H, nullptr, G[d][1], G[d][3], ws + L.fc, ctx->stream));
        HIP_TRY(gru_fc_backward(X, we_dim, wih[d], gi, M, 3 * H, want_dwe ? dx + (size_t)d * M * we_dim : nullptr, G[d][0], G[d][2],
                                ws + L.fc, ctx->stream));
    }
    if (want_dwe) {
        /* rows of we that no caption used are zeros; the others are each summed by one workgroup in the host's fixed order */
        HIP_TRY(hipMemsetAsync(d_we, 0, (size_t)V * we_dim * sizeof(float), ctx->stream));
        HIP_TRY(laff::launch_gru_embed_grad(dx, ndirs == 2 ? dx + (size_t)M * we_dim : nullptr, M, we_dim, seg_off, seg_tok, seg_pos, U, V,
                                            d_we, ctx->stream));
    }
    return LAFF_OK;
}

namespace {
// what the ragged entry points share (laff_clip_encode, laff_bert_encode, laff_netvlad_encode, laff_clip_image_encode: items
// concatenated without padding, their [N+1] offsets on the device and on the host, out with a pitch, a byte workspace)
// the token rows one transformer call takes at most: the GEMMs' grid.y = rows / 128 stays well inside its limit
constexpr long MAX_TOKEN_ROWS = 1L << 22;
int check_token_rows(const char* fn, int items, long rows_per_item) {
    if (items * rows_per_item <= MAX_TOKEN_ROWS) return LAFF_OK;
    if (rows_per_item == 1) return fail(LAFF_E_SHAPE, "%s: R=%d: more than 4,194,304 token rows in one call", fn, items);
    return fail(LAFF_E_SHAPE, "%s: F=%d frames of %ld tokens: more than 4,194,304 token rows in one call", fn, items, rows_per_item);
}
// the host copy off[0 .. N] of the offsets `name` ("row_off": rows, "frame_off": frames) of N `item`s in R rows, N and R under the
// letters dims[0] and dims[1]: off[0] = 0, every length in [lo, hi] (hi = INT_MAX: no upper limit, otherwise `limit` names it),
// off[N] = R -- in that order
int check_offsets(const char* fn, const char* name, const char* item, const char* dims, const int* off, int N, int R, int lo, int hi,
                  const char* limit) {
    const int unit = (int)strlen(name) - 4;     /* "row" / "frame" */
    if (off[0] != 0) return fail(LAFF_E_ARG, "%s: %s[0]=%d != 0", fn, name, off[0]);
    for (int i = 0; i < N; ++i) {
        const int L = off[i + 1] - off[i];
        if (L >= lo && L <= hi) continue;
        if (lo == 0 && L < 0) return fail(LAFF_E_ARG, "%s: %s decreases at %s %d (%d -> %d)", fn, name, item, i, off[i], off[i + 1]);
        if (hi == INT_MAX) return fail(LAFF_E_ARG, "%s: %s: %s %d has %d %.*ss (at least %d)", fn, name, item, i, L, unit, name, lo);
        return fail(LAFF_E_ARG, "%s: %s: %s %d has %d %.*ss (%d .. %s=%d)", fn, name, item, i, L, unit, name, lo, limit, hi);
    }
    if (off[N] != R) return fail(LAFF_E_ARG, "%s: %s[%c]=%d != %c=%d", fn, name, dims[0], off[N], dims[1], R);
    return LAFF_OK;
}
// the workspace prefix of the transformer encoders: X [rows, W] fp32 | A [rows, W] operand (sz bytes an element) |
// big [rows, max(3W fp32, big_cols operand)], each region on 256 bytes; total: where an encoder's own regions start.  The CLIP text
// encoder's workspace is this prefix with big_cols = 4W
struct ClipWs {
    size_t x, a, big, total;
};
ClipWs clip_ws(size_t rows, int width, size_t sz, size_t big_cols) {
    const size_t w = (size_t)width;
    ClipWs s;
    s.x = 0;
    s.a = round256(rows * w * 4);
    s.big = s.a + round256(rows * w * sz);
    s.total = s.big + round256(rows * std::max(3 * w * 4, big_cols * sz));
    return s;
}
int clip_precision(const char* fn, int precision, int* fp16) {
    if (precision < LAFF_PREC_FP32 || precision > LAFF_PREC_BF16X3) return fail(LAFF_E_ARG, "%s: unknown precision %d", fn, precision);
    if (precision != LAFF_PREC_FP32 && precision != LAFF_PREC_FP16)
        return fail(LAFF_E_UNSUPPORTED, "%s: precision %d: the CLIP encoder takes LAFF_PREC_FP32 or LAFF_PREC_FP16", fn, precision);
    *fp16 = precision == LAFF_PREC_FP16;
    return LAFF_OK;
}
int clip_check_width(const char* fn, int width) {
    if (width < 64 || width > 1024 || width % 64)
        return fail(LAFF_E_UNSUPPORTED, "%s: width=%d: the width must be a multiple of 64 in [64, 1024]", fn, width);
    return LAFF_OK;
}
int clip_check_heads(const char* fn, int width, int heads) {
    if (heads < 1 || heads * 64 != width)
        return fail(LAFF_E_UNSUPPORTED, "%s: width=%d heads=%d: only a head dim of 64 is supported", fn, width, heads);
    return LAFF_OK;
}
// every block's pointers, then the 16-byte alignment of its packed weights
int clip_check_blocks(const char* fn, const laff_clip_block* blocks, int layers) {
    for (int l = 0; l < layers; ++l) {
        const laff_clip_block& b = blocks[l];
        if (!b.ln_1_weight || !b.ln_1_bias || !b.in_proj_weight || !b.in_proj_bias || !b.out_proj_weight || !b.out_proj_bias ||
            !b.ln_2_weight || !b.ln_2_bias || !b.c_fc_weight || !b.c_fc_bias || !b.c_proj_weight || !b.c_proj_bias)
            return fail(LAFF_E_ARG, "%s: null pointer in block %d", fn, l);
        if (!aligned16(b.in_proj_weight) || !aligned16(b.out_proj_weight) || !aligned16(b.c_fc_weight) || !aligned16(b.c_proj_weight))
            return fail(LAFF_E_ALIGN, "%s: packed weights of block %d must be 16-byte aligned", fn, l);
    }
    return LAFF_OK;
}
int bert_check_blocks(const char* fn, const laff_bert_block* blocks, int layers) {
    for (int l = 0; l < layers; ++l) {
        const laff_bert_block& b = blocks[l];
        if (!b.qkv_weight || !b.qkv_bias || !b.attn_out_weight || !b.attn_out_bias || !b.ln_1_weight || !b.ln_1_bias ||
            !b.inter_weight || !b.inter_bias || !b.out_weight || !b.out_bias || !b.ln_2_weight || !b.ln_2_bias)
            return fail(LAFF_E_ARG, "%s: null pointer in block %d", fn, l);
        if (!aligned16(b.qkv_weight) || !aligned16(b.attn_out_weight) || !aligned16(b.inter_weight) || !aligned16(b.out_weight))
            return fail(LAFF_E_ALIGN, "%s: packed weights of block %d must be 16-byte aligned", fn, l);
    }
    return LAFF_OK;
}
// laff_clip_pack_weight (padded = false, ldp = cols) and laff_clip_pack_weight_padded
int clip_pack(const char* fn, laff_ctx* ctx, const float* W, int rows, int cols, int transpose, bool padded, int ldp, int precision,
              void* packed) {
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    if (!padded && (rows < 1 || cols < 1)) return fail(LAFF_E_SHAPE, "%s: bad shape %d x %d", fn, rows, cols);
    if (padded && (rows < 1 || cols < 1 || ldp < cols))
        return fail(LAFF_E_SHAPE, "%s: bad shape %d x %d padded to %d columns", fn, rows, cols, ldp);
    if (!W || !packed) return fail(LAFF_E_ARG, "%s: null argument", fn);
    if (!aligned16(packed)) return fail(LAFF_E_ALIGN, "%s: packed must be 16-byte aligned", fn);
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_clip_pack(W, rows, cols, transpose, ldp, fp16, packed, ctx->stream));
    return LAFF_OK;
}
}  // namespace

int laff_clip_pack_weight(laff_ctx* ctx, const float* W, int rows, int cols, int transpose, int precision, void* packed) {
    return clip_pack("laff_clip_pack_weight", ctx, W, rows, cols, transpose != 0, false, cols, precision, packed);
}

int laff_clip_workspace_bytes(int R, int N, int width, int precision, size_t* out) {
    const char* fn = "laff_clip_workspace_bytes";
    if (!out || R < 0 || N < 0 || N > R) return fail(LAFF_E_ARG, "%s: bad args", fn);
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    if (int rc = clip_check_width(fn, width)) return rc;
    *out = clip_ws(R, width, fp16 ? 2 : 4, 4 * (size_t)width).total;
    return LAFF_OK;
}

int laff_clip_encode(laff_ctx* ctx, const int* ids, const int* row_off, const int* row_off_host, int N, int R, const laff_clip_text* m,
                     int precision, float* out, int ldo, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_clip_encode";
    // every argument is checked before any GPU work
    if (!m) return fail(LAFF_E_ARG, "%s: null model", fn);
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    if (int rc = clip_check_width(fn, m->width)) return rc;
    if (int rc = clip_check_heads(fn, m->width, m->heads)) return rc;
    if (m->context_length < 1 || m->context_length > 77)
        return fail(LAFF_E_UNSUPPORTED, "%s: context_length=%d: at most 77 positions are supported", fn, m->context_length);
    if (m->layers < 1) return fail(LAFF_E_UNSUPPORTED, "%s: layers=%d: at least one block", fn, m->layers);
    if (m->embed_dim < 1 || m->vocab_size < 1) return fail(LAFF_E_SHAPE, "%s: embed_dim=%d vocab_size=%d", fn, m->embed_dim, m->vocab_size);
    if (N < 0 || R < N) return fail(LAFF_E_SHAPE, "%s: bad shape N=%d R=%d", fn, N, R);
    if (int rc = check_token_rows(fn, R, 1)) return rc;
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch */
    if (!ids || !row_off || !row_off_host || !out || !workspace || !m->token_embedding || !m->positional_embedding || !m->blocks ||
        !m->ln_final_weight || !m->ln_final_bias || !m->text_projection)
        return fail(LAFF_E_ARG, "%s: null argument", fn);
    if (int rc = clip_check_blocks(fn, m->blocks, m->layers)) return rc;
    if (int rc = check_offsets(fn, "row_off", "caption", "NR", row_off_host, N, R, 1, m->context_length, "context_length")) return rc;
    if (ldo < m->embed_dim) return fail(LAFF_E_SHAPE, "%s: ldo=%d < embed_dim=%d", fn, ldo, m->embed_dim);
    const ClipWs ws = clip_ws(R, m->width, fp16 ? 2 : 4, 4 * (size_t)m->width);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, ws.total, aligned16(m->text_projection),
                                 "workspace / packed text_projection"))
        return rc;
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    char* w = (char*)workspace;
    laff::ClipEncodeArgs e{m, ids, row_off, N, R, (float*)(w + ws.x), w + ws.a, w + ws.big, out, ldo};
    HIP_TRY(laff::launch_clip_encode(e, fp16, ctx->stream));
    return LAFF_OK;
}

namespace {
// the CLIP image encoder's workspace: X [F L, W] fp32 | A [F L, W] operand | big [F L, max(3W fp32, 4W operand)], at least the patch
// operand [F g^2, Kp] + the patch GEMM output [F g^2, W] fp32 | q_cls [F, W] fp32 | a_cls [F, W] operand, each region on 256 bytes
int vit_kpad(int patch, int fp16) {
    const int step = fp16 ? 64 : 32;                     // the GEMM's K-step: 128 bytes of a row
    return (3 * patch * patch + step - 1) / step * step;
}
int vit_check_dims(const char* fn, int width, int res, int patch) {
    if (int rc = clip_check_width(fn, width)) return rc;
    if (patch < 1 || res < patch || res % patch)
        return fail(LAFF_E_UNSUPPORTED, "%s: input_resolution=%d patch_size=%d: the resolution must be a multiple of the patch size", fn,
                    res, patch);
    if (patch > 128) return fail(LAFF_E_UNSUPPORTED, "%s: patch_size=%d: at most 128", fn, patch);
    const long g = res / patch, L = g * g + 1;
    if (L < 2 || L > laff::VIT_MAX_TOKENS)
        return fail(LAFF_E_UNSUPPORTED, "%s: %ld tokens per frame (input_resolution=%d patch_size=%d): the attention takes at most %d", fn, L,
                    res, patch, laff::VIT_MAX_TOKENS);
    return LAFF_OK;
}
struct VitWs : ClipWs {
    size_t patch_out, q_cls, a_cls;
};
VitWs vit_ws(int F, int width, int res, int patch, int fp16) {
    const size_t sz = fp16 ? 2 : 4, w = (size_t)width, g = (size_t)(res / patch), np = (size_t)F * g * g;
    VitWs s;
    static_cast<ClipWs&>(s) = clip_ws((size_t)F * (g * g + 1), width, sz, 4 * w);
    s.patch_out = round256(np * (size_t)vit_kpad(patch, fp16) * sz);
    s.q_cls = std::max(s.total, s.big + s.patch_out + round256(np * w * 4));
    s.a_cls = s.q_cls + round256((size_t)F * w * 4);
    s.total = s.a_cls + round256((size_t)F * w * sz);
    return s;
}
}  // namespace

int laff_clip_pack_weight_padded(laff_ctx* ctx, const float* W, int rows, int cols, int padded_cols, int precision, void* packed) {
    return clip_pack("laff_clip_pack_weight_padded", ctx, W, rows, cols, 0, true, padded_cols, precision, packed);
}

int laff_clip_image_kpad(int patch_size, int precision, int* out) {
    const char* fn = "laff_clip_image_kpad";
    if (!out || patch_size < 1 || patch_size > 128) return fail(LAFF_E_ARG, "%s: bad args", fn);
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    *out = vit_kpad(patch_size, fp16);
    return LAFF_OK;
}

int laff_clip_image_workspace_bytes(int F, int width, int input_resolution, int patch_size, int precision, size_t* out) {
    const char* fn = "laff_clip_image_workspace_bytes";
    if (!out || F < 0) return fail(LAFF_E_ARG, "%s: bad args", fn);
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    if (int rc = vit_check_dims(fn, width, input_resolution, patch_size)) return rc;
    *out = vit_ws(F, width, input_resolution, patch_size, fp16).total;
    return LAFF_OK;
}

int laff_clip_image_encode(laff_ctx* ctx, const float* pixels, int F, const int* frame_off, const int* frame_off_host, int V,
                           const laff_clip_visual* m, int precision, float* out_frames, int ldo, float* out_mean, int ldm, void* workspace,
                           size_t workspace_bytes) {
    const char* fn = "laff_clip_image_encode";
    // every argument is checked before any GPU work
    if (!m) return fail(LAFF_E_ARG, "%s: null model", fn);
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    if (int rc = vit_check_dims(fn, m->width, m->input_resolution, m->patch_size)) return rc;
    if (int rc = clip_check_heads(fn, m->width, m->heads)) return rc;
    if (m->layers < 1) return fail(LAFF_E_UNSUPPORTED, "%s: layers=%d: at least one block", fn, m->layers);
    if (m->embed_dim < 1) return fail(LAFF_E_SHAPE, "%s: embed_dim=%d", fn, m->embed_dim);
    if (F < 0 || V < 0 || V > F) return fail(LAFF_E_SHAPE, "%s: bad shape F=%d V=%d", fn, F, V);
    const long L = (long)(m->input_resolution / m->patch_size) * (m->input_resolution / m->patch_size) + 1;
    if (int rc = check_token_rows(fn, F, L)) return rc;
    if (F == 0) return LAFF_OK;                 /* empty problem: nothing to launch */
    if (!pixels || !out_frames || !workspace || (V > 0 && (!frame_off || !frame_off_host || !out_mean)) || !m->conv1_weight ||
        !m->class_embedding || !m->positional_embedding || !m->ln_pre_weight || !m->ln_pre_bias || !m->blocks || !m->ln_post_weight ||
        !m->ln_post_bias || !m->proj)
        return fail(LAFF_E_ARG, "%s: null argument", fn);
    if (int rc = clip_check_blocks(fn, m->blocks, m->layers)) return rc;
    if (V > 0) {
        if (int rc = check_offsets(fn, "frame_off", "video", "VF", frame_off_host, V, F, 1, INT_MAX, nullptr)) return rc;
        if (ldm < m->embed_dim) return fail(LAFF_E_SHAPE, "%s: ldm=%d < embed_dim=%d", fn, ldm, m->embed_dim);
    }
    if (ldo < m->embed_dim) return fail(LAFF_E_SHAPE, "%s: ldo=%d < embed_dim=%d", fn, ldo, m->embed_dim);
    const VitWs ws = vit_ws(F, m->width, m->input_resolution, m->patch_size, fp16);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, ws.total, aligned16(m->proj) && aligned16(m->conv1_weight),
                                 "workspace / packed conv1 / packed proj"))
        return rc;
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    char* w = (char*)workspace;
    laff::ClipImageArgs e{m, pixels, frame_off, F, V, vit_kpad(m->patch_size, fp16), (float*)(w + ws.x), w + ws.a, w + ws.big,
                          ws.patch_out, (float*)(w + ws.q_cls), w + ws.a_cls, out_frames, ldo, out_mean, ldm};
    HIP_TRY(laff::launch_clip_image_encode(e, fp16, ctx->stream));
    return LAFF_OK;
}

int laff_frame_preprocess_workspace_bytes(int F, int R, size_t* out) {
    const char* fn = "laff_frame_preprocess_workspace_bytes";
    if (!out || F < 0) return fail(LAFF_E_ARG, "%s: bad args", fn);
    if (R < 1 || R > 512) return fail(LAFF_E_UNSUPPORTED, "%s: R=%d: 1 .. 512", fn, R);
    *out = 0;                                   /* the intermediate of the two passes stays in LDS */
    return LAFF_OK;
}

namespace {
// one axis' tap table { K, xmin[R], count[R], taps[K][R] } at word `at` of the host copy, checked against the axis' source size
int frame_prep_check_table(const char* fn, int f, const char* axis, const int32_t* taps, size_t taps_len, long at, int R, int in) {
    if (at < 0 || (size_t)at + 1 + 2 * (size_t)R > taps_len)
        return fail(LAFF_E_ARG, "%s: frame %d: %s table at word %ld is outside the %zu words of taps", fn, f, axis, at, taps_len);
    const int32_t* t = taps + at;
    const int K = t[0];
    if (K < 1 || (size_t)at + 1 + (2 + (size_t)K) * R > taps_len)
        return fail(LAFF_E_ARG, "%s: frame %d: %s table with K=%d runs past the %zu words of taps", fn, f, axis, K, taps_len);
    for (int j = 0; j < R; ++j) {
        const int xmin = t[1 + j], n = t[1 + R + j];
        if (xmin < 0 || n < 1 || n > K || (long)xmin + n > in)
            return fail(LAFF_E_ARG, "%s: frame %d: %s table entry %d reads [%d, %d + %d) of %d", fn, f, axis, j, xmin, xmin, n, in);
    }
    return LAFF_OK;
}
}  // namespace

int laff_frame_preprocess(laff_ctx* ctx, const uint8_t* frames, size_t frames_bytes, const laff_frame_desc* desc,
                          const laff_frame_desc* desc_host, int F, int R, const int32_t* taps, const int32_t* taps_host, size_t taps_len,
                          const float* mean, const float* stdv, float* out_pixels, uint8_t* out_u8, void* workspace,
                          size_t workspace_bytes) {
    const char* fn = "laff_frame_preprocess";
    (void)workspace;
    (void)workspace_bytes;
    // every argument is checked before any GPU work
    if (F < 0) return fail(LAFF_E_SHAPE, "%s: F=%d", fn, F);
    if (R < 1 || R > 512) return fail(LAFF_E_UNSUPPORTED, "%s: R=%d: 1 .. 512", fn, R);
    if (F > 65535) return fail(LAFF_E_UNSUPPORTED, "%s: F=%d: at most 65535 frames per call", fn, F);
    if (F == 0) return LAFF_OK;                 /* empty problem: nothing to launch */
    if (!frames || !desc || !desc_host || !taps || !taps_host || !mean || !stdv || !out_pixels)
        return fail(LAFF_E_ARG, "%s: null argument", fn);
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f) || !std::isfinite(stdv[c]) || !std::isfinite(mean[c]))
            return fail(LAFF_E_ARG, "%s: mean[%d]=%g std[%d]=%g: finite, std > 0", fn, c, (double)mean[c], c, (double)stdv[c]);
    // the tallest LDS image over the frames at every tile height: rows [min xmin, max xmin + count) of the tile x R x 3 bytes
    constexpr int NT = 5;                       /* tile heights 16, 8, 4, 2, 1 */
    int need[NT] = {0, 0, 0, 0, 0};
    long last_h = -1, last_v = -1;
    int last_w = -1, last_hh = -1;
    for (int f = 0; f < F; ++f) {
        const laff_frame_desc& d = desc_host[f];
        if (d.height < 1 || d.height > 4096 || d.width < 1 || d.width > 4096)
            return fail(LAFF_E_UNSUPPORTED, "%s: frame %d is %d x %d: each side 1 .. 4096", fn, f, d.height, d.width);
        const size_t bytes = (size_t)d.height * d.width * 3;
        if (d.offset < 0 || (size_t)d.offset > frames_bytes || bytes > frames_bytes - (size_t)d.offset)
            return fail(LAFF_E_ARG, "%s: frame %d at byte %lld with %zu bytes is outside the %zu bytes of frames", fn, f,
                        (long long)d.offset, bytes, frames_bytes);
        if (d.htab != last_h || d.width != last_w) {
            if (int rc = frame_prep_check_table(fn, f, "horizontal", taps_host, taps_len, d.htab, R, d.width)) return rc;
            last_h = d.htab, last_w = d.width;
        }
        if (d.vtab == last_v && d.height == last_hh) continue;      /* the same vertical table: already in `need` */
        if (int rc = frame_prep_check_table(fn, f, "vertical", taps_host, taps_len, d.vtab, R, d.height)) return rc;
        last_v = d.vtab, last_hh = d.height;
        const int32_t* xmin = taps_host + d.vtab + 1;
        const int32_t* cnt = xmin + R;
        for (int t = 0; t < NT; ++t) {
            const int tile = laff::FRAME_PREP_MAX_TILE >> t;
            for (int y0 = 0; y0 < R; y0 += tile) {
                int s0 = xmin[y0], s1 = s0;
                for (int y = y0; y < std::min(R, y0 + tile); ++y) s0 = std::min(s0, xmin[y]), s1 = std::max(s1, xmin[y] + cnt[y]);
                need[t] = std::max(need[t], s1 - s0);
            }
        }
    }
    int pick = -1;
    for (int t = 0; t < NT && pick < 0; ++t)
        if ((size_t)need[t] * R * 3 <= (size_t)laff::FRAME_PREP_LDS_BYTES) pick = t;
    if (pick < 0)
        return fail(LAFF_E_UNSUPPORTED, "%s: %d vertical taps at R=%d need %zu bytes of LDS for one output row (at most %d)", fn,
                    need[NT - 1], R, (size_t)need[NT - 1] * R * 3, laff::FRAME_PREP_LDS_BYTES);
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    laff::FramePrepArgs a{frames, desc, taps, F, R, laff::FRAME_PREP_MAX_TILE >> pick, {mean[0], mean[1], mean[2]},
                          {stdv[0], stdv[1], stdv[2]}, out_pixels, out_u8};
    HIP_TRY(laff::launch_frame_prep(a, (size_t)need[pick] * R * 3, ctx->stream));
    return LAFF_OK;
}

namespace {
// the BERT text encoder's workspace: X [R, W] fp32 | A [R, W] operand | big [R, max(3W fp32, I operand)] | Xc [N, W] fp32 |
// Qc [N, W] fp32 | Ac [N, W] operand, each region on 256 bytes
int bert_check_dims(const char* fn, int width, int intermediate) {
    if (int rc = clip_check_width(fn, width)) return rc;
    if (intermediate < 64 || intermediate % 64)
        return fail(LAFF_E_UNSUPPORTED, "%s: intermediate=%d: the GEMM takes a positive multiple of 64", fn, intermediate);
    return LAFF_OK;
}
struct BertWs : ClipWs {
    size_t xc, qc, ac;
};
BertWs bert_ws(size_t R, size_t N, int width, int intermediate, int fp16) {
    const size_t sz = fp16 ? 2 : 4, w = (size_t)width;
    BertWs s;
    static_cast<ClipWs&>(s) = clip_ws(R, width, sz, (size_t)intermediate);
    s.xc = s.total;
    s.qc = s.xc + round256(N * w * 4);
    s.ac = s.qc + round256(N * w * 4);
    s.total = s.ac + round256(N * w * sz);
    return s;
}
}  // namespace

int laff_bert_workspace_bytes(int R, int N, int width, int intermediate, int precision, size_t* out) {
    const char* fn = "laff_bert_workspace_bytes";
    if (!out || R < 0 || N < 0 || N > R) return fail(LAFF_E_ARG, "%s: bad args", fn);
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    if (int rc = bert_check_dims(fn, width, intermediate)) return rc;
    *out = bert_ws(R, N, width, intermediate, fp16).total;
    return LAFF_OK;
}

int laff_bert_encode(laff_ctx* ctx, const int* ids, const int* row_off, const int* row_off_host, int N, int R, const laff_bert_text* m,
                     int precision, float* out, int ldo, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_bert_encode";
    // every argument is checked before any GPU work
    if (!m) return fail(LAFF_E_ARG, "%s: null model", fn);
    int fp16 = 0;
    if (int rc = clip_precision(fn, precision, &fp16)) return rc;
    if (int rc = bert_check_dims(fn, m->width, m->intermediate)) return rc;
    if (int rc = clip_check_heads(fn, m->width, m->heads)) return rc;
    if (m->max_position < 1 || m->max_position > laff::BERT_MAX_POSITION)
        return fail(LAFF_E_UNSUPPORTED, "%s: max_position=%d: at most %d positions are supported", fn, m->max_position,
                    laff::BERT_MAX_POSITION);
    if (m->layers < 1) return fail(LAFF_E_UNSUPPORTED, "%s: layers=%d: at least one block", fn, m->layers);
    if (m->vocab_size < 1) return fail(LAFF_E_SHAPE, "%s: vocab_size=%d", fn, m->vocab_size);
    if (!(m->layer_norm_eps >= 0.0f) || m->layer_norm_eps > 1.0f)
        return fail(LAFF_E_ARG, "%s: layer_norm_eps=%g: expected a value in [0, 1]", fn, (double)m->layer_norm_eps);
    if (N < 0 || R < N) return fail(LAFF_E_SHAPE, "%s: bad shape N=%d R=%d", fn, N, R);
    if (int rc = check_token_rows(fn, R, 1)) return rc;
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch */
    if (!ids || !row_off || !row_off_host || !out || !workspace || !m->word_embeddings || !m->position_embeddings ||
        !m->token_type_embedding || !m->emb_ln_weight || !m->emb_ln_bias || !m->blocks || !m->pooler_weight || !m->pooler_bias)
        return fail(LAFF_E_ARG, "%s: null argument", fn);
    if (int rc = bert_check_blocks(fn, m->blocks, m->layers)) return rc;
    if (int rc = check_offsets(fn, "row_off", "caption", "NR", row_off_host, N, R, 1, m->max_position, "max_position")) return rc;
    if (ldo < m->width) return fail(LAFF_E_SHAPE, "%s: ldo=%d < width=%d", fn, ldo, m->width);
    const BertWs ws = bert_ws(R, N, m->width, m->intermediate, fp16);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, ws.total, aligned16(m->pooler_weight),
                                 "workspace / packed pooler weight"))
        return rc;
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    char* w = (char*)workspace;
    laff::BertEncodeArgs e{m, ids, row_off, N, R, (float*)(w + ws.x), w + ws.a, w + ws.big, (float*)(w + ws.xc), (float*)(w + ws.qc),
                           w + ws.ac, out, ldo};
    HIP_TRY(laff::launch_bert_encode(e, fp16, ctx->stream));
    return LAFF_OK;
}

namespace {
// the NetVLAD encoder's workspace: soft assignments [R, K] fp32 | 1 / max(|x|, eps) [R] fp32, each region on 256 bytes
size_t netvlad_rnorm_offset(int R, int K) { return round256((size_t)R * K * sizeof(float)); }
size_t netvlad_ws_bytes(int R, int K) { return netvlad_rnorm_offset(R, K) + round256((size_t)R * sizeof(float)); }
int netvlad_check_k(const char* fn, int K) {
    if (K < 1 || K > laff::NETVLAD_MAX_K)
        return fail(LAFF_E_UNSUPPORTED, "%s: K=%d: the number of clusters must be in [1, %d]", fn, K, laff::NETVLAD_MAX_K);
    return LAFF_OK;
}
// what laff_netvlad_encode, laff_netvlad_encode_train and laff_netvlad_backward check alike, in two steps around the empty problem
int netvlad_check_sizes(const char* fn, int V, int D, int N, int R, int K) {
    if (int rc = netvlad_check_k(fn, K)) return rc;
    if (D < 4 || D > laff::NETVLAD_MAX_D || D % 4)
        return fail(LAFF_E_UNSUPPORTED, "%s: D=%d: the word-vector width must be a multiple of 4 in [4, %d]", fn, D, laff::NETVLAD_MAX_D);
    if (N < 0 || R < 0 || V < 1) return fail(LAFF_E_SHAPE, "%s: bad shape N=%d R=%d V=%d", fn, N, R, V);
    return LAFF_OK;
}
// other_null: one of the caller's own pointers is missing
int netvlad_check_batch(const char* fn, const float* table, const int* ids, const int* row_off, const int* row_off_host,
                        const int* zero_rows, int N, int R, const float* fc1_weight, const float* centroids, int K, int D,
                        const float* out, int ldo, bool other_null) {
    if (!table || (R && !ids) || !row_off || !row_off_host || !zero_rows || !fc1_weight || !centroids || !out || other_null)
        return fail(LAFF_E_ARG, "%s: null argument", fn);
    if (int rc = check_offsets(fn, "row_off", "caption", "NR", row_off_host, N, R, 0, INT_MAX, nullptr)) return rc;
    if (ldo < K * D || ldo % 4) return fail(LAFF_E_SHAPE, "%s: ldo=%d: at least K*D=%d and a multiple of 4", fn, ldo, K * D);
    return LAFF_OK;
}
// the training reserve: the forward's workspace (assignments, 1 / max(|x|, eps)) | den [N, K + 1] fp32 | clamped [N, K + 1] int32
struct NetvladReserve {
    size_t rnorm, den, clamped, total;
};
NetvladReserve netvlad_reserve(int N, int R, int K) {
    NetvladReserve s;
    s.rnorm = netvlad_rnorm_offset(R, K);
    s.den = netvlad_ws_bytes(R, K);
    s.clamped = s.den + round256((size_t)N * (K + 1) * sizeof(float));
    s.total = s.clamped + round256((size_t)N * (K + 1) * sizeof(int));
    return s;
}
// the backward's workspace: DU [N, K, D] | s [N, K] | dz [R, K] | the chunk sums of d_fc1 and of d_centroids [chunks, K, D], fp32,
// each region on 256 bytes.  At most 128 chunks each, of at least 64 token rows / 16 captions: a function of (N, R) alone
struct NetvladBwdWs {
    size_t mass, dz, part_fc1, part_cent, total;
    int rows_per_chunk, chunks_r, caps_per_chunk, chunks_n;
};
NetvladBwdWs netvlad_bwd_ws(int N, int R, int K, int D) {
    NetvladBwdWs s;
    s.rows_per_chunk = std::max(64, (R + 127) / 128);
    s.chunks_r = (R + s.rows_per_chunk - 1) / s.rows_per_chunk;
    s.caps_per_chunk = std::max(16, (N + 127) / 128);
    s.chunks_n = (N + s.caps_per_chunk - 1) / s.caps_per_chunk;
    const size_t kd = (size_t)K * D * sizeof(float);
    s.mass = round256((size_t)N * kd);
    s.dz = s.mass + round256((size_t)N * K * sizeof(float));
    s.part_fc1 = s.dz + round256((size_t)R * K * sizeof(float));
    s.part_cent = s.part_fc1 + round256((size_t)s.chunks_r * kd);
    s.total = s.part_cent + round256((size_t)s.chunks_n * kd);
    return s;
}
int check_reserve(const char* fn, size_t reserve_bytes, size_t need) {
    if (reserve_bytes < need) return fail(LAFF_E_ARG, "%s: reserve too small (%zu < %zu bytes)", fn, reserve_bytes, need);
    return LAFF_OK;
}
}  // namespace

int laff_netvlad_workspace_bytes(int R, int K, size_t* out) {
    if (!out || R < 0) return fail(LAFF_E_ARG, "laff_netvlad_workspace_bytes: bad args");
    if (int rc = netvlad_check_k("laff_netvlad_workspace_bytes", K)) return rc;
    *out = netvlad_ws_bytes(R, K);
    return LAFF_OK;
}

int laff_netvlad_encode(laff_ctx* ctx, const float* table, int V, int D, const int* ids, const int* row_off, const int* row_off_host,
                        const int* zero_rows, int N, int R, const float* fc1_weight, const float* centroids, int K, float* out, int ldo,
                        void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_netvlad_encode";
    // every argument is checked before any GPU work
    if (int rc = netvlad_check_sizes(fn, V, D, N, R, K)) return rc;
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch */
    if (int rc = netvlad_check_batch(fn, table, ids, row_off, row_off_host, zero_rows, N, R, fc1_weight, centroids, K, D, out, ldo,
                                     R && !workspace))
        return rc;
    if (int rc = check_workspace(fn, workspace, workspace_bytes, netvlad_ws_bytes(R, K),
                                 aligned16(table) && aligned16(centroids) && aligned16(fc1_weight) && aligned16(out),
                                 "table / fc1_weight / centroids / out / workspace"))
        return rc;
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    float* ws = (float*)workspace;
    laff::NetvladArgs a{table, V, D, K, ids, row_off, zero_rows, N, R, fc1_weight, centroids, ws,
                        (float*)((char*)workspace + netvlad_rnorm_offset(R, K)), out, ldo};
    HIP_TRY(laff::launch_netvlad_encode(a, ctx->stream));
    return LAFF_OK;
}

int laff_netvlad_train_reserve_bytes(int N, int R, int K, size_t* out) {
    if (!out || N < 0 || R < 0) return fail(LAFF_E_ARG, "laff_netvlad_train_reserve_bytes: bad args");
    if (int rc = netvlad_check_k("laff_netvlad_train_reserve_bytes", K)) return rc;
    *out = netvlad_reserve(N, R, K).total;
    return LAFF_OK;
}

int laff_netvlad_backward_workspace_bytes(int N, int R, int K, int D, size_t* out) {
    const char* fn = "laff_netvlad_backward_workspace_bytes";
    if (!out) return fail(LAFF_E_ARG, "%s: bad args", fn);
    if (int rc = netvlad_check_sizes(fn, 1, D, N, R, K)) return rc;
    *out = netvlad_bwd_ws(N, R, K, D).total;
    return LAFF_OK;
}

int laff_netvlad_encode_train(laff_ctx* ctx, const float* table, int V, int D, const int* ids, const int* row_off,
                              const int* row_off_host, const int* zero_rows, int N, int R, const float* fc1_weight,
                              const float* centroids, int K, float* out, int ldo, void* reserve, size_t reserve_bytes, void* workspace,
                              size_t workspace_bytes) {
    const char* fn = "laff_netvlad_encode_train";
    if (int rc = netvlad_check_sizes(fn, V, D, N, R, K)) return rc;
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, nothing to save */
    if (int rc = netvlad_check_batch(fn, table, ids, row_off, row_off_host, zero_rows, N, R, fc1_weight, centroids, K, D, out, ldo,
                                     !reserve))
        return rc;
    const NetvladReserve rs = netvlad_reserve(N, R, K);
    if (int rc = check_reserve(fn, reserve_bytes, rs.total)) return rc;
    /* the assignments go straight into the reserve: the workspace is not used, it may be null */
    if (int rc = check_workspace(fn, workspace, workspace_bytes, 0,
                                 aligned16(table) && aligned16(centroids) && aligned16(fc1_weight) && aligned16(out) && aligned16(reserve),
                                 "table / fc1_weight / centroids / out / reserve / workspace"))
        return rc;
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    char* r = (char*)reserve;
    laff::NetvladArgs a{table, V, D, K, ids, row_off, zero_rows, N, R, fc1_weight, centroids, (float*)r, (float*)(r + rs.rnorm), out, ldo};
    HIP_TRY(laff::launch_netvlad_encode_train(a, (float*)(r + rs.den), (int*)(r + rs.clamped), ctx->stream));
    return LAFF_OK;
}

int laff_netvlad_backward(laff_ctx* ctx, const float* table, int V, int D, const int* ids, const int* row_off, const int* row_off_host,
                          const int* zero_rows, int N, int R, const float* fc1_weight, const float* centroids, int K, const float* out,
                          int ldo, const float* d_out, int ldg, const void* reserve, size_t reserve_bytes, float* d_fc1,
                          float* d_centroids, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_netvlad_backward";
    if (int rc = netvlad_check_sizes(fn, V, D, N, R, K)) return rc;
    if (N > 0) {
        if (int rc = netvlad_check_batch(fn, table, ids, row_off, row_off_host, zero_rows, N, R, fc1_weight, centroids, K, D, out, ldo,
                                         !d_out || !reserve || !workspace))
            return rc;
        if (ldg < K * D || ldg % 4) return fail(LAFF_E_SHAPE, "%s: ldg=%d: at least K*D=%d and a multiple of 4", fn, ldg, K * D);
        if (int rc = check_reserve(fn, reserve_bytes, netvlad_reserve(N, R, K).total)) return rc;
    }
    if (!d_fc1 && !d_centroids) return LAFF_OK; /* nothing wanted: nothing to launch */
    const NetvladBwdWs L = netvlad_bwd_ws(N, R, K, D);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, N > 0 ? L.total : 0,
                                 aligned16(table) && aligned16(centroids) && aligned16(out) && aligned16(d_out) && aligned16(reserve) &&
                                     aligned16(d_fc1) && aligned16(d_centroids),
                                 "table / centroids / out / d_out / reserve / d_fc1 / d_centroids / workspace"))
        return rc;
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    const NetvladReserve rs = netvlad_reserve(N, R, K);
    char* r = (char*)const_cast<void*>(reserve);
    char* w = (char*)workspace;
    laff::NetvladBwdArgs p{};
    p.f = laff::NetvladArgs{table, V, D, K, ids, row_off, zero_rows, N, R, fc1_weight, centroids, (float*)r, (float*)(r + rs.rnorm),
                            const_cast<float*>(out), ldo};
    p.den = (const float*)(r + rs.den);
    p.clamped = (const int*)(r + rs.clamped);
    p.g = d_out;
    p.ldg = ldg;
    p.du = (float*)w;
    p.mass = (float*)(w + L.mass);
    p.dz = (float*)(w + L.dz);
    p.part_fc1 = (float*)(w + L.part_fc1);
    p.part_cent = (float*)(w + L.part_cent);
    p.rows_per_chunk = L.rows_per_chunk;
    p.chunks_r = L.chunks_r;
    p.caps_per_chunk = L.caps_per_chunk;
    p.chunks_n = L.chunks_n;
    p.d_fc1 = d_fc1;
    p.d_cent = d_centroids;
    HIP_TRY(laff::launch_netvlad_backward(p, ctx->stream));
    return LAFF_OK;
}

namespace {
// B entries of the host control block from `at`, each in [0, n): the source indices of job i
int assemble_indices(const char* fn, int i, const int* control_host, int control_len, int at, int B, int n, const char* what) {
    if (at < 0 || (long long)at + B > control_len)
        return fail(LAFF_E_ARG, "%s: job %d: %s [%d, %d) lie outside the control block of %d", fn, i, what, at, at + B, control_len);
    for (int b = 0; b < B; ++b)
        if (control_host[at + b] < 0 || control_host[at + b] >= n)
            return fail(LAFF_E_ARG, "%s: job %d: %s[%d] = %d is outside [0, %d)", fn, i, what, b, control_host[at + b], n);
    return LAFF_OK;
}
}  // namespace

int laff_batch_assemble(laff_ctx* ctx, const laff_assemble_job* jobs, int count, int B, const int* control, const int* control_host,
                        int control_len) {
    const char* fn = "laff_batch_assemble";
    if (count < 1 || count > LAFF_ASSEMBLE_MAX_JOBS)
        return fail(LAFF_E_SHAPE, "%s: %d jobs; a launch takes 1 to %d", fn, count, LAFF_ASSEMBLE_MAX_JOBS);
    if (B < 1 || B > LAFF_ASSEMBLE_MAX_BATCH) return fail(LAFF_E_SHAPE, "%s: B=%d; a batch has 1 to %d rows", fn, B, LAFF_ASSEMBLE_MAX_BATCH);
    if (!jobs || !control || !control_host || control_len < 1) return fail(LAFF_E_ARG, "%s: null jobs / control / control_host", fn);
    if (!aligned4(control)) return fail(LAFF_E_ALIGN, "%s: control must be 4-byte aligned", fn);
    laff::AssembleTable t{};
    t.count = count;
    t.B = B;
    t.control = control;
    for (int i = 0; i < count; ++i) {
        const laff_assemble_job& q = jobs[i];
        laff::AssembleJob& j = t.j[i];
        if (q.kind < LAFF_ASSEMBLE_ROWS || q.kind > LAFF_ASSEMBLE_CSR) return fail(LAFF_E_ARG, "%s: job %d: bad kind %d", fn, i, q.kind);
        if (!q.src || !q.dst) return fail(LAFF_E_ARG, "%s: job %d: null src / dst", fn, i);
        if (!aligned4(q.src) || !aligned4(q.dst)) return fail(LAFF_E_ALIGN, "%s: job %d: src / dst must be 4-byte aligned", fn, i);
        j.kind = q.kind;
        j.rows_at = q.rows_at;
        j.src = q.src;
        j.dst = q.dst;
        if (q.kind == LAFF_ASSEMBLE_CSR) {
            if (q.n_src < 1 || q.n_items < 0 || q.cap_dst < 0)
                return fail(LAFF_E_SHAPE, "%s: job %d: bad CSR sizes n_src=%d n_items=%d cap_dst=%d", fn, i, q.n_src, q.n_items, q.cap_dst);
            if (!q.off_src || !q.col_src || !q.col_dst) return fail(LAFF_E_ARG, "%s: job %d: null crow_src / col_src / col_dst", fn, i);
            if (int rc = assemble_indices(fn, i, control_host, control_len, q.rows_at, B, q.n_src, "row")) return rc;
            if (q.crow_at < 0 || (long long)q.crow_at + B + 1 > control_len)
                return fail(LAFF_E_ARG, "%s: job %d: crow_dst [%d, %d] lies outside the control block of %d", fn, i, q.crow_at,
                            q.crow_at + B, control_len);
            const int* cd = control_host + q.crow_at;
            if (cd[0] < 0) return fail(LAFF_E_ARG, "%s: job %d: crow_dst[0] = %d is negative", fn, i, cd[0]);
            for (int b = 0; b < B; ++b)
                if (cd[b + 1] < cd[b]) return fail(LAFF_E_ARG, "%s: job %d: crow_dst decreases at %d (%d -> %d)", fn, i, b, cd[b], cd[b + 1]);
            if (cd[B] > q.cap_dst) return fail(LAFF_E_ARG, "%s: job %d: crow_dst[B] = %d entries, col_dst / val_dst hold %d", fn, i, cd[B], q.cap_dst);
            j.crow_at = q.crow_at;
            j.n_src = q.n_src;
            j.n_items = q.n_items;
            j.off_src = q.off_src;
            j.col_src = q.col_src;
            j.col_dst = q.col_dst;
            continue;
        }
        const bool ragged = q.kind == LAFF_ASSEMBLE_RAGGED;
        if (q.w < 1 || q.ld_src < q.w || q.n_src < 1 || (!ragged && q.ld_dst < q.w) || (ragged && (q.fmax < 1 || q.n_items < 0)))
            return fail(LAFF_E_SHAPE, "%s: job %d: bad shape w=%d ld_src=%d ld_dst=%d n_src=%d n_items=%d fmax=%d", fn, i, q.w, q.ld_src,
                        q.ld_dst, q.n_src, q.n_items, q.fmax);
        if (ragged && !q.off_src) return fail(LAFF_E_ARG, "%s: job %d: null seg_off", fn, i);
        const long long dst_elems = ragged ? (long long)B * q.fmax * q.w : (long long)B * q.ld_dst;
        if (dst_elems > INT_MAX)
            return fail(LAFF_E_SHAPE, "%s: job %d: a destination of %lld elements overflows 32-bit indexing (%s)", fn, i, dst_elems,
                        ragged ? "B * fmax * w" : "B * ld_dst");
        if (int rc = assemble_indices(fn, i, control_host, control_len, q.rows_at, B, q.n_src, ragged ? "seg" : "row")) return rc;
        j.w = q.w;
        j.ld_src = q.ld_src;
        j.ld_dst = ragged ? q.w : q.ld_dst;
        j.n_src = q.n_src;
        j.n_items = q.n_items;
        j.fmax = ragged ? q.fmax : 1;
        j.off_src = q.off_src;
        j.mask = ragged ? q.mask : nullptr;
        j.vec = aligned16(q.src) && aligned16(q.dst) && q.ld_src % 4 == 0 && j.ld_dst % 4 == 0 && q.w >= 4;
    }
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_batch_assemble(t, ctx->stream));
    return LAFF_OK;
}

namespace {
int rr_round_half_even(int k1) { return (k1 & 1) ? ((k1 / 2) & 1 ? k1 / 2 + 1 : k1 / 2) : k1 / 2; }
// checks k1 / k2 and one problem's sizes; lays the problem's workspace out from `base` (may be null: sizes only); returns the bytes
int rerank_layout(const char* fn, int i, int Q, int G, int k1, int k2, char* base, laff::RerankProblem* d, size_t* bytes) {
    if (k1 < 1 || k1 > laff::RERANK_MAX_K1) return fail(LAFF_E_UNSUPPORTED, "%s: k1=%d: supported 1 <= k1 <= %d", fn, k1, laff::RERANK_MAX_K1);
    if (k2 < 1 || k2 > laff::RERANK_MAX_K2 || k2 > k1 + 1)
        return fail(LAFF_E_UNSUPPORTED, "%s: k2=%d: supported 1 <= k2 <= min(%d, k1 + 1)", fn, k2, laff::RERANK_MAX_K2);
    if (Q < 1 || G < 1) return fail(LAFF_E_UNSUPPORTED, "%s: problem %d: Q=%d G=%d: both at least 1", fn, i, Q, G);
    const long N = (long)Q + G;
    if (N < k1 + 1 || N > laff::RERANK_MAX_N)
        return fail(LAFF_E_UNSUPPORTED, "%s: problem %d: N=Q+G=%ld: supported k1 + 1 = %d <= N <= %d", fn, i, N, k1 + 1, laff::RERANK_MAX_N);
    const int cap = (k1 + 1) * (rr_round_half_even(k1) + 2);
    const int L1 = (int)std::min<long>(cap, N), L2 = k2 == 1 ? L1 : (int)std::min<long>((long)k2 * cap, N);
    size_t o = 0;
    auto take = [&](size_t b) { char* r = base ? base + o : nullptr; o += round256(b); return r; };
    char* rank = take((size_t)N * (k1 + 1) * 4);
    char* colmax = take((size_t)N * 4);
    char* cnt1 = take((size_t)N * 4);
    char* idx1 = take((size_t)N * L1 * 4);
    char* val1 = take((size_t)N * L1 * 4);
    char *cnt2 = cnt1, *idx2 = idx1, *val2 = val1;
    if (k2 != 1) {
        cnt2 = take((size_t)N * 4);
        idx2 = take((size_t)N * L2 * 4);
        val2 = take((size_t)N * L2 * 4);
    }
    if (d) {
        d->L1 = L1; d->L2 = L2;
        d->rank = (int*)rank; d->colmax = (float*)colmax;
        d->cnt1 = (int*)cnt1; d->idx1 = (int*)idx1; d->val1 = (float*)val1;
        d->cnt2 = (int*)cnt2; d->idx2 = (int*)idx2; d->val2 = (float*)val2;
    }
    *bytes = o;
    return LAFF_OK;
}
}  // namespace

int laff_rerank_workspace_bytes(const laff_rerank_problem* problems, int P, int k1, int k2, size_t* out) {
    const char* fn = "laff_rerank_workspace_bytes";
    if (!out || P < 0 || (P && !problems)) return fail(LAFF_E_ARG, "%s: bad args", fn);
    size_t total = 0;
    for (int i = 0; i < P; ++i) {
        size_t b;
        if (int rc = rerank_layout(fn, i, problems[i].Q, problems[i].G, k1, k2, nullptr, nullptr, &b)) return rc;
        total += b;
    }
    *out = total;
    return LAFF_OK;
}

int laff_rerank_run(laff_ctx* ctx, const laff_rerank_problem* problems, int P, int k1, int k2, float lambda_value, void* workspace,
                    size_t workspace_bytes) {
    const char* fn = "laff_rerank_run";
    // every argument is checked before any GPU work
    if (P < 0 || (P && !problems)) return fail(LAFF_E_ARG, "%s: bad args", fn);
    if (!(lambda_value >= 0.0f && lambda_value <= 1.0f)) return fail(LAFF_E_ARG, "%s: lambda_value=%g outside [0, 1]", fn, (double)lambda_value);
    size_t need = 0;
    if (int rc = laff_rerank_workspace_bytes(problems, P, k1, k2, &need)) {
        g_err.replace(0, strlen("laff_rerank_workspace_bytes"), fn);
        return rc;
    }
    if (P == 0) return LAFF_OK;
    for (int i = 0; i < P; ++i) {
        const laff_rerank_problem& q = problems[i];
        if (!q.qq || !q.qg || !q.gg || !q.out) return fail(LAFF_E_ARG, "%s: problem %d has a null pointer", fn, i);
        if (q.ldqq < q.Q || q.ldqg < q.G || q.ldgg < q.G || q.ldo < q.G)
            return fail(LAFF_E_SHAPE, "%s: problem %d: a pitch is shorter than its row (Q=%d G=%d)", fn, i, q.Q, q.G);
    }
    if (!workspace || workspace_bytes < need) return fail(LAFF_E_ARG, "%s: workspace too small (%zu < %zu bytes)", fn, workspace ? workspace_bytes : (size_t)0, need);
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(LAFF_E_ALIGN, "%s: workspace must be 256-byte aligned", fn);
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    char* base = (char*)workspace;
    for (int i0 = 0; i0 < P; i0 += laff::RERANK_GROUP) {
        laff::RerankArgs a{};
        a.count = std::min(P - i0, laff::RERANK_GROUP);
        a.k1 = k1; a.k2 = k2; a.kh = rr_round_half_even(k1); a.lambda = lambda_value;
        int maxQ = 0, maxG = 0, maxN = 0;
        for (int i = 0; i < a.count; ++i) {
            const laff_rerank_problem& q = problems[i0 + i];
            laff::RerankProblem& d = a.p[i];
            d.qq = q.qq; d.qg = q.qg; d.gg = q.gg; d.out = q.out;
            d.ldqq = (long)q.ldqq; d.ldqg = (long)q.ldqg; d.ldgg = (long)q.ldgg; d.ldo = (long)q.ldo;
            d.Q = q.Q; d.G = q.G;
            size_t b;
            (void)rerank_layout(fn, i0 + i, q.Q, q.G, k1, k2, base, &d, &b);
            base += b;
            maxQ = std::max(maxQ, q.Q); maxG = std::max(maxG, q.G); maxN = std::max(maxN, q.Q + q.G);
        }
        // the grids and the LDS rows are sized for the largest Q, G and N = Q + G of the set (each possibly of another problem)
        HIP_TRY(laff::launch_rerank(a, maxQ, maxG, maxN, ctx->stream));
    }
    return LAFF_OK;
}

int laff_rerank_tkb(laff_ctx* ctx, const int* nn, int G, int k1, const int* cand, int Q, int K, int* count, float* out, int ldo) {
    const char* fn = "laff_rerank_tkb";
    if (G < 1 || Q < 0 || k1 < 1 || k1 > G || K < 0 || K > G || ldo < G)
        return fail(LAFF_E_SHAPE, "%s: need 1 <= k1 <= G, 0 <= K <= G, ldo >= G (G=%d Q=%d k1=%d K=%d ldo=%d)", fn, G, Q, k1, K, ldo);
    if (!nn || !count || (Q && (!out || (K && !cand)))) return fail(LAFF_E_ARG, "%s: null argument", fn);
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_rerank_tkb(nn, G, k1, cand, Q, K, count, out, ldo, ctx->stream));
    return LAFF_OK;
}

int laff_sim_hist(laff_ctx* ctx, const float* T, long ldt, const float* V, long ldv, int Nt, int Nv, int H, int d, float eps, float* S,
                  long lds) {
    const char* fn = "laff_sim_hist";
    // every argument is checked before the ctx: a bad call needs no GPU
    if (Nt < 0) return fail(LAFF_E_SHAPE, "%s: Nt=%d is negative", fn, Nt);
    if (Nv < 0) return fail(LAFF_E_SHAPE, "%s: Nv=%d is negative", fn, Nv);
    if (H < 1) return fail(LAFF_E_SHAPE, "%s: H=%d, need H >= 1", fn, H);
    if (d < 1) return fail(LAFF_E_SHAPE, "%s: d=%d, need d >= 1", fn, d);
    const long K = (long)H * d;
    if (K > INT_MAX) return fail(LAFF_E_SHAPE, "%s: H*d=%ld does not fit an int (H=%d d=%d)", fn, K, H, d);
    if (ldt < K) return fail(LAFF_E_SHAPE, "%s: ldt=%ld is shorter than a row (H*d=%ld)", fn, ldt, K);
    if (ldv < K) return fail(LAFF_E_SHAPE, "%s: ldv=%ld is shorter than a row (H*d=%ld)", fn, ldv, K);
    if (lds < Nv) return fail(LAFF_E_SHAPE, "%s: lds=%ld is shorter than a row (Nv=%d)", fn, lds, Nv);
    if (!(eps >= 0.0f)) return fail(LAFF_E_ARG, "%s: eps=%g, need eps >= 0", fn, (double)eps);
    if (Nt == 0 || Nv == 0) return LAFF_OK;                 /* an empty side: nothing to launch, pointers may be null */
    if (!T) return fail(LAFF_E_ARG, "%s: T is null", fn);
    if (!V) return fail(LAFF_E_ARG, "%s: V is null", fn);
    if (!S) return fail(LAFF_E_ARG, "%s: S is null", fn);
    laff::SimHistArgs a{};
    unsigned tiles = 0;
    if (!laff::sim_hist_tiles(Nt, Nv, &a.tilesV, &tiles))
        return fail(LAFF_E_SHAPE, "%s: Nt=%d x Nv=%d is more tiles than one grid holds", fn, Nt, Nv);
    CHECK_CTX(ctx);
    DeviceGuard g(ctx->device);
    a.T = T; a.V = V; a.S = S;
    a.ldt = ldt; a.ldv = ldv; a.lds = lds;
    a.Nt = Nt; a.Nv = Nv; a.H = H; a.d = d;
    a.eps = eps;
    const bool heads16 = H == 1 || d % 4 == 0;              // every head of a row starts on 16 bytes when the row does
    a.vec = (heads16 && aligned16(T) && ldt % 4 == 0 ? 1 : 0) | (heads16 && aligned16(V) && ldv % 4 == 0 ? 2 : 0);
    HIP_TRY(laff::launch_sim_hist(a, tiles, ctx->stream));
    return LAFF_OK;
}

int laff_split_rows_bytes(int N, int K, size_t* out) {
    if (!out || N < 0 || K < 1) return fail(LAFF_E_ARG, "laff_split_rows_bytes: bad args");
    const size_t Kp = (size_t)(K + 63) / 64 * 64;
    *out = 2 * (size_t)N * Kp * 2;
    return LAFF_OK;
}

int laff_split_rows(laff_ctx* ctx, const float* X, int N, int K, int ldx, void* out, float* rscale) {
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    return split_rows_by_eight(ctx, "laff_split_rows", 1, &X, &N, &K, &ldx, &out, &rscale);
}

int laff_split_rows_grouped(laff_ctx* ctx, int count, const float* const* X, const int* N, const int* K, const int* ldx,
                            void* const* out, float* const* rscale) {
    CHECK_CTX(ctx);
    if (count < 0 || (count && (!X || !N || !K || !ldx || !out || !rscale))) return fail(LAFF_E_ARG, "laff_split_rows_grouped: bad argument list");
    return split_rows_by_eight(ctx, "laff_split_rows_grouped", count, X, N, K, ldx, out, rscale);
}

// laff_fc_act_bn_split_grouped's walk over its problems: launch(group) gets each launch in order (laff_fc_route passes a recorder)
extern "C++" {
template <typename Launch>
static int fc_split_walk(const laff_fc_split_problem* problems, int count, Launch launch) {
    FcGroup g;
    for (int i = 0; i < count; ++i) {
        const laff_fc_split_problem& q = problems[i];
        if (!q.Xs || !q.Ws || !q.x_rscale || !q.w_rscale || !q.Y) return fail(LAFF_E_ARG, "laff_fc_act_bn_split_grouped: problem %d has a null operand", i);
        if (q.N < 0 || q.Dk < 1 || q.D < 1 || q.ldy < q.D) return fail(LAFF_E_SHAPE, "laff_fc_act_bn_split_grouped: problem %d bad shape", i);
        if (int rc = check_epilogue("laff_fc_act_bn_split_grouped", i, q.act, q.bias, q.bn_scale, q.bn_shift, true)) return rc;
        if (!aligned16(q.Xs) || !aligned16(q.Ws)) return fail(LAFF_E_ALIGN, "laff_fc_act_bn_split_grouped: problem %d: Xs / Ws must be 16-byte aligned", i);
        const int Kp = (q.Dk + 63) / 64 * 64;
        if ((long long)q.N * Kp * 4 >= (1ll << 32) || (long long)q.D * Kp * 4 >= (1ll << 32))
            return fail(LAFF_E_UNSUPPORTED, "laff_fc_act_bn_split_grouped: problem %d: packed operand exceeds 4 GiB", i);
        if (q.N == 0) continue;
        laff::GemmArgs a{};
        a.R = q.Xs; a.C = q.Ws; a.nR = q.N; a.nC = q.D; a.K = Kp; a.ldR = Kp; a.ldC = Kp;
        a.nseg = 3;                                   // lo*hi, hi*lo (small terms first), hi*hi
        a.segR[0] = (long)q.N * Kp * 2; a.segC[0] = 0;
        a.segR[1] = 0;                  a.segC[1] = (long)q.D * Kp * 2;
        a.segR[2] = 0;                  a.segC[2] = 0;
        a.out = q.Y; a.ldo = q.ldy; a.scale = 1.0f;
        a.row_scale = q.x_rscale; a.col_scale = q.w_rscale;
        a.bias = q.bias; a.bn_scale = q.bn_scale; a.bn_shift = q.bn_shift; a.act = q.act;
        HIP_TRY(group_add(g, a, i, launch));
    }
    if (g.ga.count) HIP_TRY(launch(g));
    return LAFF_OK;
}
}  // extern "C++"

int laff_fc_act_bn_split_grouped(laff_ctx* ctx, const laff_fc_split_problem* problems, int count) {
    CHECK_CTX(ctx);
    if (!problems || count < 0) return fail(LAFF_E_ARG, "laff_fc_act_bn_split_grouped: bad problem list");
    DeviceGuard g(ctx->device);
    return fc_split_walk(problems, count, [&](FcGroup& fg) { return laff::launch_gemm_nt_grouped_f16(fg.ga, ctx->stream); });
}

int laff_row_scales_grouped(laff_ctx* ctx, int count, const float* const* X, const int* N, const int* K, const int* ldx,
                            float* const* rscale) {
    CHECK_CTX(ctx);
    if (count < 0 || (count && (!X || !N || !K || !ldx || !rscale))) return fail(LAFF_E_ARG, "laff_row_scales_grouped: bad argument list");
    return split_rows_by_eight(ctx, "laff_row_scales_grouped", count, X, N, K, ldx, nullptr, rscale);
}

// laff_fc_act_bn_fused_grouped's walk over its problems: launch(group) gets each launch in order (laff_fc_route passes a recorder)
extern "C++" {
template <typename Launch>
static int fc_fused_walk(const laff_fc_fused_problem* problems, int count, Launch launch) {
    FcGroup g;
    for (int i = 0; i < count; ++i) {
        const laff_fc_fused_problem& q = problems[i];
        if (q.N == 0) continue;
        if (!q.X || !q.Ws || !q.x_rscale || !q.w_rscale || !q.Y) return fail(LAFF_E_ARG, "laff_fc_act_bn_fused_grouped: problem %d has a null operand", i);
        if (q.N < 0 || q.Dk < 32 || (q.Dk & 31) || q.D < 1 || q.ldy < q.D || q.ldx < q.Dk || (q.ldx & 3))
            return fail(LAFF_E_SHAPE, "laff_fc_act_bn_fused_grouped: problem %d: need Dk %% 32 == 0, ldx %% 4 == 0 (N=%d Dk=%d D=%d ldx=%d ldy=%d)",
                        i, q.N, q.Dk, q.D, q.ldx, q.ldy);
        if (int rc = check_epilogue("laff_fc_act_bn_fused_grouped", i, q.act, q.bias, q.bn_scale, q.bn_shift, true)) return rc;
        if (!aligned16(q.X) || !aligned16(q.Ws)) return fail(LAFF_E_ALIGN, "laff_fc_act_bn_fused_grouped: problem %d: X / Ws must be 16-byte aligned", i);
        const int Kp = (q.Dk + 63) / 64 * 64;
        if ((long long)q.N * q.ldx * 4 >= (1ll << 32) || (long long)q.D * Kp * 4 >= (1ll << 32))
            return fail(LAFF_E_UNSUPPORTED, "laff_fc_act_bn_fused_grouped: problem %d: operand exceeds 4 GiB", i);
        laff::GemmArgs a{};
        a.Rf = q.X; a.ldRf = q.ldx; a.R = nullptr; a.ldR = 0;
        a.C = q.Ws; a.nR = q.N; a.nC = q.D; a.K = q.Dk; a.ldC = Kp;
        a.nseg = 3;
        a.segC[0] = 0; a.segC[1] = (long)q.D * Kp * 2; a.segC[2] = 0;
        a.out = q.Y; a.ldo = q.ldy; a.scale = 1.0f;
        a.row_scale = q.x_rscale; a.col_scale = q.w_rscale;
        a.bias = q.bias; a.bn_scale = q.bn_scale; a.bn_shift = q.bn_shift; a.act = q.act;
#ifdef LAFF_GEMM_TRACE
        if (const char* e = getenv("LAFF_GEMM_TRACE_PTR")) a.trace = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
        HIP_TRY(group_add(g, a, i, launch));
    }
    if (g.ga.count) HIP_TRY(launch(g));
    return LAFF_OK;
}
}  // extern "C++"

int laff_fc_act_bn_fused_grouped(laff_ctx* ctx, const laff_fc_fused_problem* problems, int count) {
    CHECK_CTX(ctx);
    if (!problems || count < 0) return fail(LAFF_E_ARG, "laff_fc_act_bn_fused_grouped: bad problem list");
    DeviceGuard g(ctx->device);
    return fc_fused_walk(problems, count, [&](FcGroup& fg) { return laff::launch_gemm_nt_x3_fused_grouped(fg.ga, ctx->stream); });
}

int laff_fc_route(laff_ctx* ctx, int family, const laff_fc_shape* shapes, int count, int* kind, int* launch_of, laff_fc_launch* launches,
                  int cap, int* n_launches) {
    CHECK_CTX(ctx);
    if (family < LAFF_FC_FAMILY_F32 || family > LAFF_FC_FAMILY_FUSED) return fail(LAFF_E_ARG, "laff_fc_route: bad family %d", family);
    if (count < 0 || cap < 0 || !n_launches || (count && (!shapes || !kind || !launch_of)) || (cap && !launches))
        return fail(LAFF_E_ARG, "laff_fc_route: bad argument list");
    // stand-ins for the caller's buffers: the choice looks at their alignment and at which are present, never at what they hold
    alignas(16) static char stand_in[32];
    float* const al = (float*)stand_in;
    float* const off = (float*)(stand_in + 4);
    for (int i = 0; i < count; ++i) kind[i] = launch_of[i] = -1;
    int n = 0;
    bool over = false;
    // records one launch the way the launcher of the family plans it
    auto record = [&](FcGroup& g, int stg) {
        laff::GroupedPlan pl;
        const bool ok = family == LAFF_FC_FAMILY_F32     ? laff::plan_gemm_nt_grouped_f32(g.ga, stg, pl)
                        : family == LAFF_FC_FAMILY_SPLIT ? laff::plan_gemm_nt_grouped_f16(g.ga, pl)
                                                         : laff::plan_gemm_nt_x3_fused_grouped(g.ga, pl);
        if (!ok) return hipErrorInvalidValue;
        if (n >= cap) { over = true; return hipSuccess; }
        const bool tile128 = pl.kernel <= LAFF_FC_KERNEL_F16_128;
        for (int j = 0; j < g.ga.count; ++j) {
            launch_of[g.idx[j]] = n;
            if (family != LAFF_FC_FAMILY_F32) kind[g.idx[j]] = tile128 ? 128 : 256;
        }
        launches[n++] = laff_fc_launch{pl.kernel, g.ga.count, pl.tiles, pl.nbig, pl.quarters};
        return hipSuccess;
    };
    int rc = LAFF_OK;
    if (family == LAFF_FC_FAMILY_F32) {
        std::vector<laff_fc_problem> ps((size_t)count);
        for (int i = 0; i < count; ++i) {
            const laff_fc_shape& q = shapes[i];
            ps[i] = laff_fc_problem{q.x_aligned ? al : off, q.N, q.Dk, q.ldx, q.w_aligned ? al : off, q.ldw, nullptr, nullptr, nullptr,
                                    q.D, LAFF_ACT_NONE, al, q.D};
        }
        rc = fc_f32_walk(ps.data(), count, kind, record);
    } else if (family == LAFF_FC_FAMILY_SPLIT) {
        std::vector<laff_fc_split_problem> ps((size_t)count);
        for (int i = 0; i < count; ++i) {
            const laff_fc_shape& q = shapes[i];
            ps[i] = laff_fc_split_problem{al, al, q.N, q.Dk, al, al, nullptr, nullptr, nullptr, q.D, LAFF_ACT_NONE, al, q.D};
        }
        rc = fc_split_walk(ps.data(), count, [&](FcGroup& g) { return record(g, 2); });
    } else {
        std::vector<laff_fc_fused_problem> ps((size_t)count);
        for (int i = 0; i < count; ++i) {
            const laff_fc_shape& q = shapes[i];
            ps[i] = laff_fc_fused_problem{q.x_aligned ? al : off, q.ldx, al, q.N, q.Dk, al, al, nullptr, nullptr, nullptr, q.D,
                                          LAFF_ACT_NONE, al, q.D};
        }
        rc = fc_fused_walk(ps.data(), count, [&](FcGroup& g) { return record(g, 2); });
    }
    if (rc) return rc;
    if (over) return fail(LAFF_E_ARG, "laff_fc_route: more than cap=%d launches", cap);
    *n_launches = n;
    return LAFF_OK;
}

/* host-side helper, no device work: owner[t] = position in the video id list of the prefix of caption id t before its first '#'
 * (predictor.py:241: txt_id.split('#')[0] looked up in vis_ids).  One open-addressing table over the video ids, FNV-1a. */
int laff_match_ids(const char* txt_blob, size_t txt_bytes, int n_txt, const char* vis_blob, size_t vis_bytes, int n_vis, int* owner) {
    if (n_txt < 0 || n_vis < 0 || (n_txt && (!txt_blob || !owner)) || (n_vis && !vis_blob)) return fail(LAFF_E_ARG, "laff_match_ids: bad arguments");
    if (n_txt == 0) return LAFF_OK;
    auto hash = [](const char* p, size_t n) {
        unsigned long long h = 1469598103934665603ull;
        for (size_t i = 0; i < n; ++i) { h ^= (unsigned char)p[i]; h *= 1099511628211ull; }
        return h;
    };
    size_t cap = 16;
    while (cap < 2 * (size_t)n_vis + 2) cap <<= 1;
    struct Slot { const char* p; unsigned len; int idx; };
    std::vector<Slot> table(cap, Slot{nullptr, 0u, -1});
    size_t at = 0;
    for (int v = 0; v < n_vis; ++v) {
        if (at > vis_bytes) return fail(LAFF_E_ARG, "laff_match_ids: the video blob holds fewer than %d ids", n_vis);
        const char* b = vis_blob + at;
        const char* e = (const char*)memchr(b, '\n', vis_bytes - at);
        const size_t len = e ? (size_t)(e - b) : vis_bytes - at;
        at += len + 1;
        size_t s = hash(b, len) & (cap - 1);
        while (table[s].idx >= 0) {
            if (table[s].len == len && memcmp(table[s].p, b, len) == 0)
                return fail(LAFF_E_SHAPE, "laff_match_ids: video id '%.*s' appears twice in vis_ids", (int)len, b);
            s = (s + 1) & (cap - 1);
        }
        table[s] = Slot{b, (unsigned)len, v};
    }
    if (at != vis_bytes + 1 && !(n_vis == 0 && vis_bytes == 0)) return fail(LAFF_E_ARG, "laff_match_ids: the video blob does not hold exactly %d ids", n_vis);
    at = 0;
    for (int t = 0; t < n_txt; ++t) {
        if (at > txt_bytes) return fail(LAFF_E_ARG, "laff_match_ids: the caption blob holds fewer than %d ids", n_txt);
        const char* b = txt_blob + at;
        const char* e = (const char*)memchr(b, '\n', txt_bytes - at);
        const size_t line = e ? (size_t)(e - b) : txt_bytes - at;
        at += line + 1;
        const char* h = (const char*)memchr(b, '#', line);
        const size_t len = h ? (size_t)(h - b) : line;
        size_t s = hash(b, len) & (cap - 1);
        int found = -1;
        while (table[s].idx >= 0) {
            if (table[s].len == len && memcmp(table[s].p, b, len) == 0) { found = table[s].idx; break; }
            s = (s + 1) & (cap - 1);
        }
        if (found < 0) return fail(LAFF_E_SHAPE, "laff_match_ids: caption %d refers to a video that is not in vis_ids: '%.*s'", t, (int)len, b);
        owner[t] = found;
    }
    if (at != txt_bytes + 1) return fail(LAFF_E_ARG, "laff_match_ids: the caption blob does not hold exactly %d ids", n_txt);
    return LAFF_OK;
}

int laff_fc_strip_pack_bytes(int D, int Dk, size_t* out) {
    if (!out || D < 32 || (D & 31)) return fail(LAFF_E_SHAPE, "laff_fc_strip_pack_bytes: D must be a positive multiple of 32 (D=%d)", D);
    if (Dk != laff::FC_STRIP_K) return fail(LAFF_E_SHAPE, "laff_fc_strip_pack_bytes: the strip form takes Dk == 512 (Dk=%d)", Dk);
    *out = laff::fc_strip_image_bytes(D);
    return LAFF_OK;
}

int laff_fc_strip_pack(laff_ctx* ctx, const float* W, int ldw, const float* bias, const float* bn_scale, const float* bn_shift, int D,
                       int Dk, int act, void* img) {
    CHECK_CTX(ctx);
    if (!W || !img) return fail(LAFF_E_ARG, "laff_fc_strip_pack: null W / img");
    if (D < 32 || (D & 31) || Dk != laff::FC_STRIP_K || ldw < Dk)
        return fail(LAFF_E_SHAPE, "laff_fc_strip_pack: need D %% 32 == 0, Dk == 512, ldw >= Dk (D=%d Dk=%d ldw=%d)", D, Dk, ldw);
    if ((long long)D * 2048 >= (1ll << 32)) return fail(LAFF_E_UNSUPPORTED, "laff_fc_strip_pack: image exceeds 4 GiB");
    if (int rc = check_epilogue("laff_fc_strip_pack", -1, act, bias, bn_scale, bn_shift, false)) return rc;
    if (!aligned16(img)) return fail(LAFF_E_ALIGN, "laff_fc_strip_pack: img must be 16-byte aligned");
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_fc_strip_pack(W, ldw, bias, bn_scale, bn_shift, D, act, img, ctx->stream));
    return LAFF_OK;
}

int laff_fc_act_bn_strip_grouped(laff_ctx* ctx, const laff_fc_strip_problem* problems, int count) {
    CHECK_CTX(ctx);
    if (!problems || count < 0) return fail(LAFF_E_ARG, "laff_fc_act_bn_strip_grouped: bad problem list");
    DeviceGuard g(ctx->device);
    auto kind = [](int act) { return act == LAFF_ACT_TANH || act == LAFF_ACT_SIGMOID ? 2 : (act == LAFF_ACT_RELU ? 1 : 0); };
    std::vector<char> done((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        const laff_fc_strip_problem& q = problems[i];
        if (q.N == 0) { done[i] = 1; continue; }
        if (!q.X || !q.img || !q.Y) return fail(LAFF_E_ARG, "laff_fc_act_bn_strip_grouped: problem %d has a null operand", i);
        if (q.N < 0 || q.D < 32 || (q.D & 31) || q.ldy < q.D || q.ldx < laff::FC_STRIP_K || (q.ldx & 3))
            return fail(LAFF_E_SHAPE, "laff_fc_act_bn_strip_grouped: problem %d: need D %% 32 == 0, ldx >= 512, ldx %% 4 == 0 (N=%d D=%d ldx=%d ldy=%d)",
                        i, q.N, q.D, q.ldx, q.ldy);
        if (int rc = check_epilogue("laff_fc_act_bn_strip_grouped", i, q.act, nullptr, nullptr, nullptr, false)) return rc;
        if (!aligned16(q.X) || !aligned16(q.img)) return fail(LAFF_E_ALIGN, "laff_fc_act_bn_strip_grouped: problem %d: 16-byte alignment", i);
        if ((long long)laff::FC_STRIP_ROWS * q.ldy * 4 >= (1ll << 31) || (long long)q.D * 2048 >= (1ll << 32))
            return fail(LAFF_E_UNSUPPORTED, "laff_fc_act_bn_strip_grouped: problem %d: output strip / image exceeds the 32-bit buffer range", i);
    }
    // one launch per (D, activation kind), up to MAX_GROUP problems each
    for (int i = 0; i < count; ++i) {
        if (done[i]) continue;
        laff::FcStripArgs fa{};
        fa.nblk = problems[i].D / 32;
        const int k = kind(problems[i].act);
        for (int j = i; j < count && fa.count < laff::MAX_GROUP; ++j) {
            const laff_fc_strip_problem& q = problems[j];
            if (done[j] || q.D != problems[i].D || kind(q.act) != k) continue;
            laff::FcStripProblem& fp = fa.p[fa.count++];
            fp.X = q.X; fp.img = q.img; fp.vec = (const float*)((const char*)q.img + laff::fc_strip_vec_offset(q.D));
            fp.Y = q.Y; fp.ldx = q.ldx; fp.ldy = q.ldy; fp.N = q.N;
            done[j] = 1;
        }
        HIP_TRY(laff::launch_fc_strip(fa, problems[i].act, ctx->stream));
    }
    return LAFF_OK;
}

int laff_fuse_packed(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, const float* w, const float* b,
                     const float* gw, unsigned flags, float* E, float* attn_w, void* E16, int precision, float prescale);
int laff_fuse_packed_rank(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, const float* w, const float* b,
                          const float* gw, unsigned flags, float* E, float* attn_w, void* E16, int precision, float prescale,
                          const laff_rank_side* rs);

int laff_fuse(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, const float* w, const float* b,
              const float* gw, unsigned flags, float* E, float* attn_w) {
    return laff_fuse_packed(ctx, planes, L, N, H, d, w, b, gw, flags, E, attn_w, nullptr, LAFF_PREC_FP16, 1.0f);
}

// plane descriptors -> FuseArgs (shared by laff_fuse* and laff_plane_row_norms)
static int parse_planes(const laff_plane* planes, int L, int N, int H, int d, unsigned flags, laff::FuseArgs& a, bool& any_gather) {
    if (!planes) return fail(LAFF_E_ARG, "laff_fuse: null planes");
    if (L < 1 || L > laff::MAX_L) return fail(LAFF_E_SHAPE, "laff_fuse: L=%d outside [1,%d]", L, laff::MAX_L);
    if (N < 0 || H < 1 || d < 4 || (d & 3)) return fail(LAFF_E_SHAPE, "laff_fuse: need N>=0, H>=1, d%%4==0 (N=%d H=%d d=%d)", N, H, d);
    const bool nosplit = flags & LAFF_ATT_NO_SPLIT_HEAD;
    any_gather = false;
    for (int l = 0; l < L; ++l) {
        const laff_plane& p = planes[l];
        if ((p.scale == nullptr) != (p.shift == nullptr)) return fail(LAFF_E_ARG, "laff_fuse: plane %d scale/shift must come together", l);
        if (p.act < LAFF_ACT_NONE || p.act > LAFF_ACT_SIGMOID) return fail(LAFF_E_ARG, "laff_fuse: plane %d bad act %d", l, p.act);
        if (p.scale && (!aligned16(p.scale) || !aligned16(p.shift))) return fail(LAFF_E_ALIGN, "laff_fuse: plane %d affine not 16-byte aligned", l);
        a.rownorm[l] = p.row_scale;
        if (!p.src && p.wt) {                          // gather plane
            if (!p.indptr || !p.indices) return fail(LAFF_E_ARG, "laff_fuse: gather plane %d needs indptr / indices", l);
            if (p.tile || nosplit || d > 512) return fail(LAFF_E_UNSUPPORTED, "laff_fuse: gather plane %d needs split heads of d <= 512, not tiled", l);
            if (p.row_scale) return fail(LAFF_E_UNSUPPORTED, "laff_fuse: gather plane %d cannot take a row_scale (project the feature with laff_fc_gather_act_bn first)", l);
            if (p.dk < 1 || p.ldwt < H * d || (p.ldwt & 3)) return fail(LAFF_E_SHAPE, "laff_fuse: gather plane %d: dk=%d ldwt=%d (need >= %d, multiple of 4)", l, p.dk, p.ldwt, H * d);
            if (!aligned16(p.wt) || (p.bias && !aligned16(p.bias))) return fail(LAFF_E_ALIGN, "laff_fuse: gather plane %d not 16-byte aligned", l);
            a.g_indptr[l] = p.indptr; a.g_indices[l] = p.indices; a.g_values[l] = p.values; a.g_wt[l] = p.wt; a.g_bias[l] = p.bias;
            a.g_ldwt[l] = p.ldwt; a.g_dk[l] = p.dk;
            a.scale[l] = p.scale; a.shift[l] = p.shift; a.act[l] = p.act;
            any_gather = true;
            continue;
        }
        if (!p.src) return fail(LAFF_E_ARG, "laff_fuse: plane %d has null src", l);
        if (p.tile && nosplit) return fail(LAFF_E_UNSUPPORTED, "laff_fuse: tiled plane with NO_SPLIT_HEAD");
        const int need = p.tile ? d : (nosplit ? d : H * d);
        if (p.ld < need || (p.ld & 3)) return fail(LAFF_E_SHAPE, "laff_fuse: plane %d ld=%d (need >= %d, multiple of 4)", l, p.ld, need);
        if (!aligned16(p.src)) return fail(LAFF_E_ALIGN, "laff_fuse: plane %d not 16-byte aligned", l);
        a.src[l] = p.src; a.ld[l] = p.ld; a.tile[l] = p.tile; a.scale[l] = p.scale; a.shift[l] = p.shift; a.act[l] = p.act;
    }
    a.L = L; a.N = N; a.H = H; a.d = d; a.head_stride = nosplit ? 0 : d;
    a.flags = flags;
    return LAFF_OK;
}

int laff_fuse_packed(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, const float* w, const float* b,
                     const float* gw, unsigned flags, float* E, float* attn_w, void* E16, int precision, float prescale) {
    return laff_fuse_packed_rank(ctx, planes, L, N, H, d, w, b, gw, flags, E, attn_w, E16, precision, prescale, nullptr);
}

int laff_fuse_packed_rank(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, const float* w, const float* b,
                          const float* gw, unsigned flags, float* E, float* attn_w, void* E16, int precision, float prescale,
                          const laff_rank_side* rs) {
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (rs) {
        if (rs->side != 1 && rs->side != 2) return fail(LAFF_E_ARG, "laff_fuse_packed_rank: side must be 1 (text) or 2 (video)");
        if (!E16 || d > 512 || (flags & LAFF_ATT_NO_SPLIT_HEAD))
            return fail(LAFF_E_UNSUPPORTED, "laff_fuse_packed_rank: needs the 16-bit operand (E16) and split heads of d <= 512 (H=%d d=%d): use laff_rank_prepare", H, d);
        if (H > 1 && (!rs->partials || !rs->tickets)) return fail(LAFF_E_ARG, "laff_fuse_packed_rank: several heads need the partials / tickets scratch");
        if (!rs->band) return fail(LAFF_E_ARG, "laff_fuse_packed_rank: null band");
        if (rs->side == 1) {
            if (!rs->gt_col || !rs->Ev || !rs->s_gt64 || !rs->band_v || !rs->count || !rs->pairs)
                return fail(LAFF_E_ARG, "laff_fuse_packed_rank: the text side needs gt_col, Ev, s_gt64, band_v, count and pairs");
            if (rs->Nv < 1 || (long)N * 16 < rs->Nv)
                return fail(LAFF_E_UNSUPPORTED, "laff_fuse_packed_rank: %d text rows cannot finish the block maxima of %d videos: use laff_rank_prepare", N, rs->Nv);
            if (!aligned16(rs->Ev)) return fail(LAFF_E_ALIGN, "laff_fuse_packed_rank: Ev must be 16-byte aligned");
        }
    }
    if (E16 && precision != LAFF_PREC_FP16 && precision != LAFF_PREC_BF16)
        return fail(LAFF_E_UNSUPPORTED, "laff_fuse_packed: E16 is a single-plane operand (FP16 or BF16), got precision %d", precision);
    if (E16 && !aligned16(E16)) return fail(LAFF_E_ALIGN, "laff_fuse_packed: E16 must be 16-byte aligned");
    if (E16 && (flags & LAFF_ATT_JUST_AVERAGE)) return fail(LAFF_E_UNSUPPORTED, "laff_fuse_packed: JUST_AVERAGE output is not unit-norm");
    if (!planes || !E) return fail(LAFF_E_ARG, "laff_fuse: null planes/E");
    const bool javg = flags & LAFF_ATT_JUST_AVERAGE;
    if (!javg && (!w || !b)) return fail(LAFF_E_ARG, "laff_fuse: null w/b");
    if ((flags & LAFF_ATT_WITH_AVE) && !gw) return fail(LAFF_E_ARG, "laff_fuse: WITH_AVE needs gw");
    if (!aligned16(E) || (w && !aligned16(w))) return fail(LAFF_E_ALIGN, "laff_fuse: E/w must be 16-byte aligned");
    laff::FuseArgs a{};
    bool any_gather = false;
    if (int rc = parse_planes(planes, L, N, H, d, flags, a, any_gather)) return rc;
    a.head_major = any_gather ? 1 : 0;
    a.w = w; a.b = b; a.gw = gw; a.E = E; a.attn_w = attn_w;
    a.E16 = E16; a.e16_bf16 = precision == LAFF_PREC_BF16; a.e16_scale = prescale;
    if (rs) {
        a.rp_side = rs->side; a.rp_gt = rs->gt_col; a.rp_col0 = rs->col0; a.rp_Nv = rs->Nv; a.rp_Ev = rs->Ev; a.rp_sgt = rs->s_gt64;
        a.rp_band = rs->band; a.rp_band_v = rs->band_v; a.rp_count = rs->count; a.rp_pairs = rs->pairs;
        a.rp_part = rs->partials; a.rp_ticket = rs->tickets;
        laff::rank_band_constants(precision, H, d, &a.rp_unit, &a.rp_cacc);
    }
    DeviceGuard g(ctx->device);
    if (rs && H > 1) HIP_TRY(hipMemsetAsync(rs->tickets, 0, (size_t)N * sizeof(unsigned), ctx->stream));
    HIP_TRY(laff::launch_fuse(a, ctx->stream));
    return LAFF_OK;
}

int laff_plane_row_norms(laff_ctx* ctx, const laff_plane* planes, int L, int N, int H, int d, unsigned flags, float* out) {
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!out) return fail(LAFF_E_ARG, "laff_plane_row_norms: null out");
    laff::FuseArgs a{};
    bool any_gather = false;
    if (int rc = parse_planes(planes, L, N, H, d, flags, a, any_gather)) return rc;
    if (any_gather) return fail(LAFF_E_UNSUPPORTED, "laff_plane_row_norms: gather planes are not supported (project the feature first)");
    for (int l = 0; l < L; ++l)
        if (a.rownorm[l]) return fail(LAFF_E_ARG, "laff_plane_row_norms: plane %d already carries a row_scale", l);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_plane_row_norms(a, out, ctx->stream));
    return LAFF_OK;
}

// the shape and flags of laff_fuse_backward and its workspace query
static int fuse_backward_shape(const char* fn, int L, int N, int H, int d, unsigned flags) {
    if (L < 1 || L > laff::MAX_L) return fail(LAFF_E_SHAPE, "%s: L=%d outside [1,%d]", fn, L, laff::MAX_L);
    if (N < 0 || H < 1 || d < 4 || (d & 3)) return fail(LAFF_E_SHAPE, "%s: need N>=0, H>=1, d%%4==0 (N=%d H=%d d=%d)", fn, N, H, d);
    if ((long long)H * d > INT_MAX) return fail(LAFF_E_SHAPE, "%s: H * d = %lld columns", fn, (long long)H * d);
    if (flags & ~31u) return fail(LAFF_E_ARG, "%s: unknown flags 0x%x", fn, flags);
    return LAFF_OK;
}

int laff_fuse_backward_workspace_bytes(int L, int N, int H, int d, unsigned flags, size_t* out) {
    if (!out) return fail(LAFF_E_ARG, "laff_fuse_backward_workspace_bytes: null out");
    if (int rc = fuse_backward_shape("laff_fuse_backward_workspace_bytes", L, N, H, d, flags)) return rc;
    int R = 0, P = 0, rows = 0;
    laff::fuse_bwd_plan(N, H, d, flags, &R, &P, &rows);
    *out = N ? (size_t)H * rows * d * sizeof(float) : 0;
    return LAFF_OK;
}

int laff_fuse_backward(laff_ctx* ctx, const float* const* x, const int* ldx, int L, int N, int H, int d, const float* w, const float* b,
                       const float* gw, unsigned flags, const float* dE, int lde, float* const* dx, const int* lddx, float* dw, float* db,
                       void* workspace, size_t workspace_bytes) {
    CHECK_CTX(ctx);
    if (int rc = fuse_backward_shape("laff_fuse_backward", L, N, H, d, flags)) return rc;
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!x || !ldx || !dx || !lddx || !dE) return fail(LAFF_E_ARG, "laff_fuse_backward: null x / ldx / dx / lddx / dE");
    const bool javg = flags & LAFF_ATT_JUST_AVERAGE, nosplit = flags & LAFF_ATT_NO_SPLIT_HEAD;
    if (!javg && (!w || !b)) return fail(LAFF_E_ARG, "laff_fuse_backward: null w/b");
    if (!javg && (flags & LAFF_ATT_WITH_AVE) && !gw) return fail(LAFF_E_ARG, "laff_fuse_backward: WITH_AVE needs gw");
    if (lde < H * d || (lde & 3)) return fail(LAFF_E_SHAPE, "laff_fuse_backward: lde=%d (need >= %d, multiple of 4)", lde, H * d);
    if (!aligned16(dE) || (w && !aligned16(w)) || (dw && !aligned16(dw)))
        return fail(LAFF_E_ALIGN, "laff_fuse_backward: dE / w / dw must be 16-byte aligned");
    laff::FuseBwdArgs a{};
    const int need = nosplit ? d : H * d;
    for (int l = 0; l < L; ++l) {
        if (!x[l] || !dx[l]) return fail(LAFF_E_ARG, "laff_fuse_backward: plane %d has a null x / dx", l);
        if (ldx[l] < need || (ldx[l] & 3) || lddx[l] < need || (lddx[l] & 3))
            return fail(LAFF_E_SHAPE, "laff_fuse_backward: plane %d ldx=%d lddx=%d (need >= %d, multiples of 4)", l, ldx[l], lddx[l], need);
        if (!aligned16(x[l]) || !aligned16(dx[l])) return fail(LAFF_E_ALIGN, "laff_fuse_backward: plane %d not 16-byte aligned", l);
        a.x[l] = x[l]; a.dx[l] = dx[l]; a.ldx[l] = ldx[l]; a.lddx[l] = lddx[l];
    }
    a.L = L; a.N = N; a.H = H; a.d = d; a.head_stride = nosplit ? 0 : d;
    a.w = w; a.b = b; a.gw = gw; a.flags = flags; a.dE = dE; a.lde = lde;
    if (dw && !javg) {
        int R = 0, P = 0, rows = 0;
        laff::fuse_bwd_plan(N, H, d, flags, &R, &P, &rows);
        const size_t bytes = (size_t)H * rows * d * sizeof(float);
        if (int rc = need_workspace("laff_fuse_backward", workspace, workspace_bytes, bytes)) return rc;
        a.dw_part = (float*)workspace;
    }
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_fuse_backward(a, dw, db, ctx->stream));
    return LAFF_OK;
}

// the shape and mode of laff_selfattn_fuse, its backward and the plan: plain integers, checked before anything else
static int selfattn_shape(const char* fn, int N, int H, int d) {
    if (N < 0 || H < 1) return fail(LAFF_E_SHAPE, "%s: need N>=0, H>=1 (N=%d H=%d)", fn, N, H);
    if (d < 4 || d > 512 || (d & 3)) return fail(LAFF_E_SHAPE, "%s: d=%d per head outside [4,512] or not a multiple of 4", fn, d);
    if ((long long)H * d > 8192) return fail(LAFF_E_SHAPE, "%s: H * d = %lld columns (at most 8192)", fn, (long long)H * d);
    if (d < H) return fail(LAFF_E_SHAPE, "%s: d=%d < H=%d: the scale (d / H) ^ -0.5 divides by zero", fn, d, H);
    if ((long long)N * H > INT_MAX) return fail(LAFF_E_SHAPE, "%s: N * H = %lld groups", fn, (long long)N * H);
    return LAFF_OK;
}

// everything of the two launches but the ctx: fills `a`.  g: E / dE (pooled) and S: O / dO (stacked) are the output of the forward and
// the incoming gradient of the backward.
static int selfattn_check(const char* fn, const float* const* x, const int* ldx, int L, int N, int H, int d, const float* gamma,
                          const float* beta, int prepend, int pool, int token, unsigned flags, const float* g, int lde, const float* S,
                          int ldon, int ldol, const char* gname, const char* sname, laff::SelfAttnArgs& a) {
    if (L < 1 || L > laff::MAX_L) return fail(LAFF_E_SHAPE, "%s: L=%d outside [1,%d]", fn, L, laff::MAX_L);
    if (int rc = selfattn_shape(fn, N, H, d)) return rc;
    if (flags & ~(unsigned)LAFF_ATT_L2NORM_EACH_HEAD) return fail(LAFF_E_ARG, "%s: unknown flags 0x%x", fn, flags);
    if (prepend < LAFF_SA_PREPEND_NONE || prepend > LAFF_SA_PREPEND_MEAN) return fail(LAFF_E_ARG, "%s: unknown prepend %d", fn, prepend);
    if (pool < LAFF_SA_POOL_MEAN || pool > LAFF_SA_POOL_ALL) return fail(LAFF_E_ARG, "%s: unknown pool %d", fn, pool);
    const int T = L + (prepend != LAFF_SA_PREPEND_NONE);
    if (pool == LAFF_SA_POOL_TOKEN && (token < 0 || token >= T)) return fail(LAFF_E_ARG, "%s: token=%d outside [0,%d)", fn, token, T);
    if (pool == LAFF_SA_POOL_ALL && prepend != LAFF_SA_PREPEND_NONE)
        return fail(LAFF_E_ARG, "%s: LAFF_SA_POOL_ALL returns the L planes' tokens: no prepended token", fn);
    a.L = L; a.N = N; a.H = H; a.d = d; a.prepend = prepend; a.pool = pool; a.token = pool == LAFF_SA_POOL_TOKEN ? token : 0;
    a.l2n = (flags & LAFF_ATT_L2NORM_EACH_HEAD) != 0;
    a.scale = 1.0f / sqrtf((float)(d / H));
    a.gamma = gamma; a.beta = beta; a.lde = lde; a.ldon = ldon; a.ldol = ldol;
    if (N == 0) return LAFF_OK;                 /* empty problem: pointers may be null */
    const int D = H * d;
    if (!x || !ldx || !gamma || !beta) return fail(LAFF_E_ARG, "%s: null x / ldx / gamma / beta", fn);
    if (!aligned16(gamma) || !aligned16(beta)) return fail(LAFF_E_ALIGN, "%s: gamma / beta must be 16-byte aligned", fn);
    for (int l = 0; l < L; ++l) {
        if (!x[l]) return fail(LAFF_E_ARG, "%s: plane %d is null", fn, l);
        if (ldx[l] < D || (ldx[l] & 3)) return fail(LAFF_E_SHAPE, "%s: plane %d ldx=%d (need >= %d, a multiple of 4)", fn, l, ldx[l], D);
        if (!aligned16(x[l])) return fail(LAFF_E_ALIGN, "%s: plane %d not 16-byte aligned", fn, l);
        a.x[l] = x[l]; a.ldx[l] = ldx[l];
    }
    if (pool == LAFF_SA_POOL_ALL) {
        if (!S) return fail(LAFF_E_ARG, "%s: null %s", fn, sname);
        const long long ln = ldon, ll = ldol;
        if (ldon < D || ldol < D || ((N - 1) * ln + D > ll && (L - 1) * ll + D > ln && N > 1 && L > 1))
            return fail(LAFF_E_SHAPE, "%s: the pitches of %s (row %d, plane %d) do not hold [N=%d, L=%d, H*d=%d] without overlap", fn, sname,
                        ldon, ldol, N, L, D);
        if ((ldon & 3) || (ldol & 3) || !aligned16(S))
            return fail(LAFF_E_ALIGN, "%s: the rows of %s must be 16-byte aligned (base, row pitch %d, plane pitch %d)", fn, sname, ldon, ldol);
    } else {
        if (!g) return fail(LAFF_E_ARG, "%s: null %s", fn, gname);
        if (lde < D || (lde & 3)) return fail(LAFF_E_SHAPE, "%s: lde=%d (need >= %d, a multiple of 4)", fn, lde, D);
        if (!aligned16(g)) return fail(LAFF_E_ALIGN, "%s: %s must be 16-byte aligned", fn, gname);
    }
    return LAFF_OK;
}

int laff_selfattn_fuse_backward_plan(int N, int H, int d, int out[2]) {
    const char* fn = "laff_selfattn_fuse_backward_plan";
    if (!out) return fail(LAFF_E_ARG, "%s: null out", fn);
    if (int rc = selfattn_shape(fn, N, H, d)) return rc;
    int R = 0, P = 0;
    laff::selfattn_plan(N, H, &R, &P);
    out[0] = N ? P * 2 * d * (int)sizeof(float) : 0;
    out[1] = N ? P : 0;
    return LAFF_OK;
}

int laff_selfattn_fuse(laff_ctx* ctx, const float* const* x, const int* ldx, int L, int N, int H, int d, const float* gamma,
                       const float* beta, int prepend, int pool, int token, unsigned flags, float* E, int lde, float* O, int ldon,
                       int ldol) {
    const char* fn = "laff_selfattn_fuse";
    laff::SelfAttnArgs a{};
    if (int rc = selfattn_check(fn, x, ldx, L, N, H, d, gamma, beta, prepend, pool, token, flags, E, lde, O, ldon, ldol, "E", "O", a)) return rc;
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;
    a.E = E; a.O = O;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_selfattn_fuse(a, ctx->stream));
    return LAFF_OK;
}

int laff_selfattn_fuse_backward(laff_ctx* ctx, const float* const* x, const int* ldx, int L, int N, int H, int d, const float* gamma,
                                const float* beta, int prepend, int pool, int token, unsigned flags, const float* dE, int lde,
                                const float* dO, int ldon, int ldol, float* const* dx, const int* lddx, float* dgamma, float* dbeta,
                                void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_selfattn_fuse_backward";
    laff::SelfAttnArgs a{};
    if (int rc = selfattn_check(fn, x, ldx, L, N, H, d, gamma, beta, prepend, pool, token, flags, dE, lde, dO, ldon, ldol, "dE", "dO", a))
        return rc;
    if (N > 0 && (!dx || !lddx)) return fail(LAFF_E_ARG, "%s: null dx / lddx", fn);
    for (int l = 0; l < L && N > 0; ++l) {
        if (!dx[l]) return fail(LAFF_E_ARG, "%s: plane %d has a null dx", fn, l);
        if (lddx[l] < H * d || (lddx[l] & 3)) return fail(LAFF_E_SHAPE, "%s: plane %d lddx=%d (need >= %d, a multiple of 4)", fn, l, lddx[l], H * d);
        if (!aligned16(dx[l])) return fail(LAFF_E_ALIGN, "%s: dx of plane %d not 16-byte aligned", fn, l);
        a.dx[l] = dx[l]; a.lddx[l] = lddx[l];
    }
    if ((dgamma && !aligned16(dgamma)) || (dbeta && !aligned16(dbeta))) return fail(LAFF_E_ALIGN, "%s: dgamma / dbeta must be 16-byte aligned", fn);
    if ((dgamma || dbeta) && N > 0) {
        int R = 0, P = 0;
        laff::selfattn_plan(N, H, &R, &P);
        if (int rc = need_workspace(fn, workspace, workspace_bytes, (size_t)P * 2 * d * sizeof(float))) return rc;
        a.part = (float*)workspace;
    }
    CHECK_CTX(ctx);
    if (N == 0 && !dgamma && !dbeta) return LAFF_OK;
    a.dE = dE; a.dO = dO;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_selfattn_fuse_backward(a, dgamma, dbeta, ctx->stream));
    return LAFF_OK;
}

static int fc_backward_shape(const char* fn, int N, int Dk, int D) {
    if (N < 0 || Dk < 1 || D < 1) return fail(LAFF_E_SHAPE, "%s: need N>=0, Dk>=1, D>=1 (N=%d Dk=%d D=%d)", fn, N, Dk, D);
    return LAFF_OK;
}

int laff_fc_backward_plan(int N, int Dk, int D, int want_dx, int want_dw, int out[4]) {
    if (!out) return fail(LAFF_E_ARG, "laff_fc_backward_plan: null out");
    if (int rc = fc_backward_shape("laff_fc_backward_plan", N, Dk, D)) return rc;
    laff::FcBwdPlan p;
    laff::fc_bwd_plan(N, Dk, D, &p);
    /* the cuts depend on the shape alone; want_dx / want_dw only say whose partial tiles the workspace has to hold (db's always) */
    const size_t bytes = std::max(want_dx ? p.ws_dx : (size_t)0, want_dw ? p.ws_dw : p.ws_db);
    if (bytes > (size_t)INT_MAX) return fail(LAFF_E_SHAPE, "laff_fc_backward_plan: workspace of %zu bytes", bytes);
    out[0] = p.chunks; out[1] = (int)bytes; out[2] = p.chunks_dx; out[3] = (p.tile_dw == 128 ? 1 : 0) | (p.tile_dx == 128 ? 2 : 0);
    return LAFF_OK;
}

int laff_fc_backward(laff_ctx* ctx, const float* X, int N, int Dk, int ldx, const float* W, int ldw, int D, int act, const float* A, int lda,
                     const float* dA, int ldda, float* dX, int lddx, float* dW, int lddw, float* db, void* workspace,
                     size_t workspace_bytes) {
    CHECK_CTX(ctx);
    const char* fn = "laff_fc_backward";
    if (int rc = fc_backward_shape(fn, N, Dk, D)) return rc;
    if (act < LAFF_ACT_NONE || act > LAFF_ACT_SIGMOID) return fail(LAFF_E_ARG, "%s: bad act %d", fn, act);
    if (dW && lddw < Dk) return fail(LAFF_E_SHAPE, "%s: lddw=%d < Dk=%d", fn, lddw, Dk);
    if (!aligned4(dW) || !aligned4(db)) return fail(LAFF_E_ALIGN, "%s: dW / db must be 4-byte aligned", fn);
    DeviceGuard g(ctx->device);
    if (N == 0) {                                /* the empty sum: zeros in dW and db, nothing else is read or written */
        if (dW) HIP_TRY(hipMemset2DAsync(dW, (size_t)lddw * sizeof(float), 0, (size_t)Dk * sizeof(float), D, ctx->stream));
        if (db) HIP_TRY(hipMemsetAsync(db, 0, (size_t)D * sizeof(float), ctx->stream));
        return LAFF_OK;
    }
    if (!dX && !dW && !db) return LAFF_OK;
    if (!A || !dA || (dW && !X) || (dX && !W)) return fail(LAFF_E_ARG, "%s: null A / dA, X (read for dW) or W (read for dX)", fn);
    if (lda < D || ldda < D || (dW && ldx < Dk) || (dX && (ldw < Dk || lddx < Dk)))
        return fail(LAFF_E_SHAPE, "%s: a row pitch is below the row width (ldx=%d ldw=%d lddx=%d Dk=%d; lda=%d ldda=%d D=%d)", fn, ldx, ldw,
                    lddx, Dk, lda, ldda, D);
    if (!aligned4(X) || !aligned4(W) || !aligned4(A) || !aligned4(dA) || !aligned4(dX))
        return fail(LAFF_E_ALIGN, "%s: X / W / A / dA / dX must be 4-byte aligned", fn);
    laff::FcBwdPlan p;
    laff::fc_bwd_plan(N, Dk, D, &p);
    const size_t need = std::max(dX ? p.ws_dx : (size_t)0, dW ? p.ws_dw : db ? p.ws_db : (size_t)0);
    if (need)
        if (int rc = need_workspace(fn, workspace, workspace_bytes, need)) return rc;
    const laff::FcBwdArgs a = fc_bwd_args(X, N, Dk, ldx, W, ldw, D, act, A, lda, dA, ldda, dX, lddx, dW, lddw, db, need ? workspace : nullptr);
    HIP_TRY(laff::launch_fc_backward(a, ctx->stream));
    return LAFF_OK;
}

int laff_fc_gather_backward(laff_ctx* ctx, const int* colptr, const int* rows, const float* values, int nnz, int N, int Dk, int D, int act,
                            const float* A, int lda, const float* dA, int ldda, float* dW, int lddw, float* db) {
    CHECK_CTX(ctx);
    const char* fn = "laff_fc_gather_backward";
    if (N < 0 || nnz < 0 || Dk < 1 || D < 4 || (D & 3) || D > 8192)
        return fail(LAFF_E_SHAPE, "%s: need N>=0, nnz>=0, Dk>=1, D%%4==0, 4<=D<=8192 (N=%d nnz=%d Dk=%d D=%d)", fn, N, nnz, Dk, D);
    if (act < LAFF_ACT_NONE || act > LAFF_ACT_SIGMOID) return fail(LAFF_E_ARG, "%s: bad act %d", fn, act);
    if (dW && lddw < Dk) return fail(LAFF_E_SHAPE, "%s: lddw=%d < Dk=%d", fn, lddw, Dk);
    if (!aligned4(dW) || !aligned4(db)) return fail(LAFF_E_ALIGN, "%s: dW / db must be 4-byte aligned", fn);
    if (!dW && !db) return LAFF_OK;
    const bool walk = dW && N > 0 && nnz > 0;    /* otherwise dW is the empty sum: zeros, and the pattern is not read */
    if (walk && (!colptr || !rows)) return fail(LAFF_E_ARG, "%s: null colptr / rows", fn);
    if (N > 0) {
        if (!A || !dA) return fail(LAFF_E_ARG, "%s: null A / dA", fn);
        if (lda < D || ldda < D || (lda & 3) || (ldda & 3))
            return fail(LAFF_E_SHAPE, "%s: lda=%d and ldda=%d must be multiples of 4 and at least D=%d", fn, lda, ldda, D);
        if (!aligned16(A) || !aligned16(dA)) return fail(LAFF_E_ALIGN, "%s: A / dA must be 16-byte aligned", fn);
    }
    DeviceGuard g(ctx->device);
    if (dW && !walk) HIP_TRY(hipMemset2DAsync(dW, (size_t)lddw * sizeof(float), 0, (size_t)Dk * sizeof(float), D, ctx->stream));
    if (N == 0) {
        if (db) HIP_TRY(hipMemsetAsync(db, 0, (size_t)D * sizeof(float), ctx->stream));
        return LAFF_OK;
    }
    laff::FcGatherBwdArgs a{};
    a.colptr = colptr; a.rows = rows; a.values = values; a.A = A; a.dA = dA; a.dW = walk ? dW : nullptr; a.db = db;
    a.nnz = nnz; a.N = N; a.Dk = Dk; a.D = D; a.lda = lda; a.ldda = ldda; a.lddw = lddw; a.act = act;
    HIP_TRY(laff::launch_fc_gather_backward(a, ctx->stream));
    return LAFF_OK;
}

/* what the plan and the call of a concat layer's backward refuse first: the number of segments, N and D */
static int fc_concat_backward_shape(const char* fn, int N, int D, int nseg) {
    if (nseg < 1 || nseg > laff::CONCAT_MAX_SEG)
        return fail(LAFF_E_ARG, "%s: need 1 <= nseg <= %d segments (nseg=%d)", fn, laff::CONCAT_MAX_SEG, nseg);
    if (N < 0 || D < 4 || (D & 3) || D > 8192)
        return fail(LAFF_E_SHAPE, "%s: need N >= 0, D %% 4 == 0, 4 <= D <= 8192 (N=%d D=%d)", fn, N, D);
    return LAFF_OK;
}

/* the workspace bytes of the dense launches: dX's partial rows, dW's with db's, or db's alone */
static size_t fc_concat_backward_ws(const laff::FcBwdPlan& p, bool dense, bool dx, bool want_dw) {
    return dense ? std::max(dx ? p.ws_dx : (size_t)0, want_dw ? p.ws_dw : p.ws_db) : 0;
}

int laff_fc_concat_backward_plan(int N, int D, const int* widths, const int* kinds, int nseg, int want_dw, int out[4]) {
    const char* fn = "laff_fc_concat_backward_plan";
    if (!out || !widths || !kinds) return fail(LAFF_E_ARG, "%s: null widths / kinds / out", fn);
    if (int rc = fc_concat_backward_shape(fn, N, D, nseg)) return rc;
    int dk[laff::CONCAT_MAX_SEG], n = 0, dx_cols = 0;
    for (int s = 0; s < nseg; ++s) {
        if (widths[s] < 1) return fail(LAFF_E_SHAPE, "%s: segment %d has width Dk=%d", fn, s, widths[s]);
        if ((kinds[s] & 3) == 3) return fail(LAFF_E_ARG, "%s: segment %d: a CSR segment has no dX", fn, s);
        if (kinds[s] & 1) continue;
        dk[n++] = widths[s];
        if (kinds[s] & 2) dx_cols += widths[s];
    }
    laff::FcBwdPlan p;
    laff::fc_concat_bwd_plan(N, D, dk, n, dx_cols, &p);
    const size_t bytes = fc_concat_backward_ws(p, n > 0, dx_cols > 0, want_dw != 0);
    if (bytes > (size_t)INT_MAX) return fail(LAFF_E_SHAPE, "%s: workspace of %zu bytes", fn, bytes);
    out[0] = p.chunks; out[1] = (int)bytes; out[2] = p.chunks_dx; out[3] = (p.tile_dw == 128 ? 1 : 0) | (p.tile_dx == 128 ? 2 : 0);
    return LAFF_OK;
}

int laff_fc_concat_backward(laff_ctx* ctx, int nseg, const int* widths, const int* cols, const int* nnz, const float* const* X, const int* ldx,
                            float* const* dX, const int* lddx, const int* const* colptr, const int* const* rows, const float* const* values,
                            int N, const float* W, int K, int ldw, int D, int act, const float* A, int lda, const float* dA, int ldda,
                            float* dW, int lddw, float* db, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_fc_concat_backward";
    if (int rc = fc_concat_backward_shape(fn, N, D, nseg)) return rc;
    if (!widths || !cols || !nnz) return fail(LAFF_E_ARG, "%s: null widths / cols / nnz", fn);
    if (K < 1) return fail(LAFF_E_SHAPE, "%s: K=%d", fn, K);
    if (act < LAFF_ACT_NONE || act > LAFF_ACT_SIGMOID) return fail(LAFF_E_ARG, "%s: bad act %d", fn, act);
    /* the call's arrays go straight into the two launchers' forms: the dense segments into a.seg, a sparse one into its gather launch */
    laff::FcConcatBwdArgs a{};
    laff::FcGatherBwdArgs csr[laff::CONCAT_MAX_SEG];
    int csr_col[laff::CONCAT_MAX_SEG], ncsr = 0, dk[laff::CONCAT_MAX_SEG], dx_cols = 0;
    for (int s = 0; s < nseg; ++s) {
        const int w = widths[s], c = cols[s];
        float* const dx = dX ? dX[s] : nullptr;
        if (w < 1) return fail(LAFF_E_SHAPE, "%s: segment %d has width Dk=%d", fn, s, w);
        if (c < 0 || (long long)c + w > K)
            return fail(LAFF_E_SHAPE, "%s: segment %d: columns [%d, %lld) are outside W's K=%d", fn, s, c, (long long)c + w, K);
        for (int t = 0; t < s; ++t)
            if (c < cols[t] + widths[t] && cols[t] < c + w) return fail(LAFF_E_SHAPE, "%s: segments %d and %d overlap in W's columns", fn, t, s);
        if (nnz[s] >= 0) {
            if (dx) return fail(LAFF_E_ARG, "%s: segment %d: a CSR segment has no dX (counts)", fn, s);
            laff::FcGatherBwdArgs& q = csr[ncsr];
            q = laff::FcGatherBwdArgs{};
            q.colptr = colptr ? colptr[s] : nullptr; q.rows = rows ? rows[s] : nullptr; q.values = values ? values[s] : nullptr;
            q.nnz = nnz[s]; q.N = N; q.Dk = w; q.D = D; q.lda = lda; q.ldda = ldda; q.lddw = lddw; q.act = act; q.A = A; q.dA = dA;
            if (dW && N > 0 && q.nnz > 0 && (!q.colptr || !q.rows)) return fail(LAFF_E_ARG, "%s: segment %d: null colptr / rows", fn, s);
            csr_col[ncsr++] = c;
        } else {
            laff::FcConcatBwdSeg& f = a.seg[a.nseg];
            f.X = X ? X[s] : nullptr; f.ldx = ldx ? ldx[s] : 0; f.dX = N > 0 ? dx : nullptr; f.lddx = lddx ? lddx[s] : 0; f.dk = w; f.col = c;
            if (N > 0 && ((dW && f.ldx < w) || (dx && f.lddx < w)))
                return fail(LAFF_E_SHAPE, "%s: segment %d: a row pitch is below Dk=%d (ldx=%d lddx=%d)", fn, s, w, f.ldx, f.lddx);
            if (N > 0 && dW && !f.X) return fail(LAFF_E_ARG, "%s: segment %d: null X (read for dW)", fn, s);
            if (!aligned4(f.X) || !aligned4(dx)) return fail(LAFF_E_ALIGN, "%s: segment %d: X / dX must be 4-byte aligned", fn, s);
            dk[a.nseg++] = w;
            if (dx) dx_cols += w;
        }
    }
    if (dW && lddw < K) return fail(LAFF_E_SHAPE, "%s: lddw=%d < K=%d", fn, lddw, K);
    if (!aligned4(dW) || !aligned4(db) || !aligned4(W)) return fail(LAFF_E_ALIGN, "%s: W / dW / db must be 4-byte aligned", fn);
    laff::FcBwdPlan p;
    laff::fc_concat_bwd_plan(N, D, dk, a.nseg, dx_cols, &p);
    const size_t need = N > 0 ? fc_concat_backward_ws(p, a.nseg > 0, dx_cols > 0, dW != nullptr) : 0;
    if (need && (dW || db || dx_cols))
        if (int rc = need_workspace(fn, workspace, workspace_bytes, need)) return rc;
    if (N > 0 && (dW || db || dx_cols)) {
        if (!A || !dA || (dx_cols && !W)) return fail(LAFF_E_ARG, "%s: null A / dA, or W (read for dX)", fn);
        if (lda < D || ldda < D || (dx_cols && ldw < K))
            return fail(LAFF_E_SHAPE, "%s: a row pitch is below the row width (lda=%d ldda=%d D=%d; ldw=%d K=%d)", fn, lda, ldda, D, ldw, K);
        if (!aligned4(A) || !aligned4(dA)) return fail(LAFF_E_ALIGN, "%s: A / dA must be 4-byte aligned", fn);
        if (ncsr && (!aligned16(A) || !aligned16(dA) || (lda & 3) || (ldda & 3)))
            return fail(LAFF_E_ALIGN, "%s: with a CSR segment A / dA must be 16-byte aligned and lda=%d, ldda=%d multiples of 4", fn, lda, ldda);
    }
    CHECK_CTX(ctx);
    if (!dW && !db && !dx_cols) return LAFF_OK;
    DeviceGuard g(ctx->device);
    if (N == 0) {                                /* the empty sum: zeros in dW's windows and db, nothing else is read or written */
        if (dW)
            for (int s = 0; s < nseg; ++s)
                HIP_TRY(hipMemset2DAsync(dW + cols[s], (size_t)lddw * sizeof(float), 0, (size_t)widths[s] * sizeof(float), D, ctx->stream));
        if (db) HIP_TRY(hipMemsetAsync(db, 0, (size_t)D * sizeof(float), ctx->stream));
        return LAFF_OK;
    }
    /* the dense segments: one launch for dW (with db), one for dX */
    a.W = W; a.A = A; a.dA = dA; a.dW = dW; a.db = db;
    a.N = N; a.D = D; a.ldw = ldw; a.lda = lda; a.ldda = ldda; a.lddw = lddw; a.act = act;
    a.part = need ? (float*)workspace : nullptr;
    HIP_TRY(laff::launch_fc_concat_backward(a, ctx->stream));
    /* the CSR segments: laff_fc_gather_backward's launch on each window; db from the first one when no dense launch formed it */
    for (int i = 0; i < ncsr; ++i) {
        laff::FcGatherBwdArgs& q = csr[i];
        q.db = a.nseg == 0 && i == 0 ? db : nullptr;
        if (!dW && !q.db) continue;
        float* window = dW ? dW + csr_col[i] : nullptr;
        const bool walk = window && q.nnz > 0;   /* otherwise the window is the empty sum: zeros, and the pattern is not read */
        if (window && !walk) HIP_TRY(hipMemset2DAsync(window, (size_t)lddw * sizeof(float), 0, (size_t)q.Dk * sizeof(float), D, ctx->stream));
        if (!walk && !q.db) continue;
        q.dW = walk ? window : nullptr;
        HIP_TRY(laff::launch_fc_gather_backward(q, ctx->stream));
    }
    return LAFF_OK;
}

/* The refusals and steps that the plain and the tiled BatchNorm entry points share; a layer of D columns is planned as
   bn_train_plan(N, D, has_bn), the tiled one with D = H C.  The first three come before CHECK_CTX: the tests call them without a GPU. */
static int bn_plan_out(const char* fn, int N, int D, bool has_bn, int out[4]) {
    laff::BnTrainPlan p;
    laff::bn_train_plan(N, D, has_bn, &p);
    if (p.ws > (size_t)INT_MAX) return fail(LAFF_E_SHAPE, "%s: workspace of %zu bytes", fn, p.ws);
    out[0] = p.chunks; out[1] = (int)p.ws; out[2] = p.launches; out[3] = laff::BN_TRAIN_ROWS;
    return LAFF_OK;
}
static int bn_rows_check(const char* fn, int N, bool batch) {             /* at most one of the two can hold */
    if ((N + laff::BN_TRAIN_ROWS - 1) / laff::BN_TRAIN_ROWS > 65535) return fail(LAFF_E_SHAPE, "%s: N=%d beyond 65535 chunks of rows", fn, N);
    if (batch && N < 2) return fail(LAFF_E_ARG, "%s: batch statistics need N >= 2 rows, got %d", fn, N);
    return LAFF_OK;
}
static int bn_eps_momentum_check(const char* fn, double eps, double momentum) {
    if (!(eps > 0.0)) return fail(LAFF_E_ARG, "%s: eps=%g must be positive", fn, eps);
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(LAFF_E_ARG, "%s: momentum=%g outside [0, 1]", fn, momentum);
    return LAFF_OK;
}
/* the float64 partials of a call in its checked workspace; null where the plan needs none */
static int bn_part(const char* fn, int N, int D, bool has_bn, void* workspace, size_t workspace_bytes, double** part) {
    laff::BnTrainPlan plan;
    laff::bn_train_plan(N, D, has_bn, &plan);
    *part = plan.ws ? (double*)workspace : nullptr;
    return plan.ws ? need_workspace(fn, workspace, workspace_bytes, plan.ws) : LAFF_OK;
}

/* what both directions of the dropout + BatchNorm stage refuse before any GPU work, a null ctx included: the tests need no GPU */
static int dropout_bn_check(const char* fn, int N, int D, double p, const void* seed, bool has_bn) {
    if (N < 0 || D < 1) return fail(LAFF_E_SHAPE, "%s: need N>=0, D>=1 (N=%d D=%d)", fn, N, D);
    if (!(p >= 0.0 && p < 1.0)) return fail(LAFF_E_ARG, "%s: p=%g outside [0, 1)", fn, p);
    if (p > 0.0 && !seed) return fail(LAFF_E_ARG, "%s: p > 0 needs a seed", fn);
    if (p == 0.0 && !has_bn) return fail(LAFF_E_ARG, "%s: p == 0 without a BatchNorm stage (null gamma): nothing to do", fn);
    return bn_rows_check(fn, N, has_bn);
}

/* the dropout side of the arguments: thresh = floor(p 2^32) and fp32(1 / (1 - p)), in double on the host */
static void dropout_bn_mask(laff::BnTrainArgs& a, double p, const unsigned long long* seed) {
    a.drop = p > 0.0;
    a.seed = seed;
    a.thresh = (unsigned)std::floor(p * 4294967296.0);
    a.scale = (float)(1.0 / (1.0 - p));
}
static int dropout_bn_seed_check(const char* fn, const unsigned long long* seed) {
    return (reinterpret_cast<uintptr_t>(seed) & 7) ? fail(LAFF_E_ALIGN, "%s: seed must be 8-byte aligned", fn) : LAFF_OK;
}

int laff_dropout_bn_train_plan(int N, int D, int has_bn, int out[4]) {
    if (!out) return fail(LAFF_E_ARG, "laff_dropout_bn_train_plan: null out");
    if (N < 0 || D < 1) return fail(LAFF_E_SHAPE, "laff_dropout_bn_train_plan: need N>=0, D>=1 (N=%d D=%d)", N, D);
    return bn_plan_out("laff_dropout_bn_train_plan", N, D, has_bn != 0, out);
}

int laff_dropout_bn_train(laff_ctx* ctx, const float* A, int N, int D, int lda, double p, const unsigned long long* seed, const float* gamma,
                          const float* beta, float* running_mean, float* running_var, double momentum, double eps, float* Y, int ldy,
                          float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_dropout_bn_train";
    if (int rc = dropout_bn_check(fn, N, D, p, seed, gamma != nullptr)) return rc;
    if (gamma)
        if (int rc = bn_eps_momentum_check(fn, eps, momentum)) return rc;
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;
    if (!A || !Y) return fail(LAFF_E_ARG, "%s: null A / Y", fn);
    if (gamma && (!beta || !running_mean || !running_var || !save_mean || !save_invstd))
        return fail(LAFF_E_ARG, "%s: a BatchNorm stage needs beta, running_mean, running_var, save_mean and save_invstd", fn);
    if (lda < D || ldy < D) return fail(LAFF_E_SHAPE, "%s: a row pitch is below the row width (lda=%d ldy=%d D=%d)", fn, lda, ldy, D);
    if (!aligned4(A) || !aligned4(Y) || !aligned4(gamma) || !aligned4(beta) || !aligned4(running_mean) || !aligned4(running_var) ||
        !aligned4(save_mean) || !aligned4(save_invstd))
        return fail(LAFF_E_ALIGN, "%s: every fp32 pointer must be 4-byte aligned", fn);
    if (int rc = dropout_bn_seed_check(fn, seed)) return rc;
    laff::BnTrainArgs a{};
    if (int rc = bn_part(fn, N, D, gamma != nullptr, workspace, workspace_bytes, &a.part)) return rc;
    a.A = A; a.out = Y; a.gamma = gamma; a.beta = beta; a.running_mean = running_mean; a.running_var = running_var;
    a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.N = N; a.D = D; a.lda = lda; a.ldo = ldy; a.momentum = momentum; a.eps = eps;
    a.fast = aligned16(A) && aligned16(Y) && lda % 4 == 0 && ldy % 4 == 0 && D % 4 == 0;
    dropout_bn_mask(a, p, seed);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_bn_train_forward(a, ctx->stream));
    return LAFF_OK;
}

int laff_dropout_bn_train_backward(laff_ctx* ctx, const float* dY, int lddy, const float* A, int N, int D, int lda, double p,
                                   const unsigned long long* seed, const float* gamma, const float* save_mean, const float* save_invstd,
                                   float* dA, int ldda, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_dropout_bn_train_backward";
    if (int rc = dropout_bn_check(fn, N, D, p, seed, gamma != nullptr)) return rc;
    CHECK_CTX(ctx);
    if (!gamma && (dgamma || dbeta)) return fail(LAFF_E_ARG, "%s: dgamma / dbeta without a BatchNorm stage (null gamma)", fn);
    if (N == 0 || (!dA && !dgamma && !dbeta)) return LAFF_OK;
    if (!A || !dY) return fail(LAFF_E_ARG, "%s: null A / dY", fn);
    if (gamma && (!save_mean || !save_invstd)) return fail(LAFF_E_ARG, "%s: a BatchNorm stage needs save_mean and save_invstd", fn);
    if (lda < D || lddy < D || (dA && ldda < D))
        return fail(LAFF_E_SHAPE, "%s: a row pitch is below the row width (lda=%d lddy=%d ldda=%d D=%d)", fn, lda, lddy, ldda, D);
    if (!aligned4(A) || !aligned4(dY) || !aligned4(dA) || !aligned4(gamma) || !aligned4(save_mean) || !aligned4(save_invstd) ||
        !aligned4(dgamma) || !aligned4(dbeta))
        return fail(LAFF_E_ALIGN, "%s: every fp32 pointer must be 4-byte aligned", fn);
    if (int rc = dropout_bn_seed_check(fn, seed)) return rc;
    laff::BnTrainArgs a{};
    if (int rc = bn_part(fn, N, D, gamma != nullptr, workspace, workspace_bytes, &a.part)) return rc;
    a.A = A; a.dY = dY; a.out = dA; a.gamma = gamma; a.save_mean = const_cast<float*>(save_mean);
    a.save_invstd = const_cast<float*>(save_invstd); a.dgamma = dgamma; a.dbeta = dbeta;
    a.N = N; a.D = D; a.lda = lda; a.lddy = lddy; a.ldo = ldda;
    a.fast = aligned16(A) && aligned16(dY) && lda % 4 == 0 && lddy % 4 == 0 && D % 4 == 0 && (!dA || (aligned16(dA) && ldda % 4 == 0));
    dropout_bn_mask(a, p, seed);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_bn_train_backward(a, ctx->stream));
    return LAFF_OK;
}

/* what the plan and both directions of the tiled BatchNorm refuse before any GPU work, a null ctx included */
static int tile_bn_check(const char* fn, int N, int C, int H, bool has_gamma, bool batch) {
    if (H < 1 || C < 1 || N < 0) return fail(LAFF_E_SHAPE, "%s: need N>=0, C>=1, H>=1 (N=%d C=%d H=%d)", fn, N, C, H);
    if ((long long)H * C > INT_MAX || H > 65535) return fail(LAFF_E_SHAPE, "%s: H=%d heads of C=%d columns are out of range", fn, H, C);
    if (int rc = bn_rows_check(fn, N, batch)) return rc;
    if (batch && !has_gamma) return fail(LAFF_E_ARG, "%s: null gamma", fn);
    return LAFF_OK;
}

int laff_tile_bn_train_plan(int N, int C, int H, int out[4]) {
    if (!out) return fail(LAFF_E_ARG, "laff_tile_bn_train_plan: null out");
    if (int rc = tile_bn_check("laff_tile_bn_train_plan", N, C, H, true, false)) return rc;
    return bn_plan_out("laff_tile_bn_train_plan", N, H * C, true, out);
}

int laff_tile_bn_train(laff_ctx* ctx, const float* X, int N, int C, int ldx, int H, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, double momentum, double eps, float* Y, int ldy, float* save_mean,
                       float* save_invstd, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_tile_bn_train";
    if (int rc = tile_bn_check(fn, N, C, H, gamma != nullptr, true)) return rc;
    if (int rc = bn_eps_momentum_check(fn, eps, momentum)) return rc;
    CHECK_CTX(ctx);
    if (!X || !Y || !beta || !running_mean || !running_var || !save_mean || !save_invstd)
        return fail(LAFF_E_ARG, "%s: null X / Y / beta / running_mean / running_var / save_mean / save_invstd", fn);
    if (ldx < C || ldy < H * C) return fail(LAFF_E_SHAPE, "%s: a row pitch is below the row width (ldx=%d ldy=%d C=%d H=%d)", fn, ldx, ldy, C, H);
    if (!aligned4(X) || !aligned4(Y) || !aligned4(gamma) || !aligned4(beta) || !aligned4(running_mean) || !aligned4(running_var) ||
        !aligned4(save_mean) || !aligned4(save_invstd))
        return fail(LAFF_E_ALIGN, "%s: every fp32 pointer must be 4-byte aligned", fn);
    laff::TileBnTrainArgs a{};
    if (int rc = bn_part(fn, N, H * C, true, workspace, workspace_bytes, &a.part)) return rc;
    a.X = X; a.Y = Y; a.gamma = gamma; a.beta = beta; a.running_mean = running_mean; a.running_var = running_var;
    a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.N = N; a.C = C; a.H = H; a.ldx = ldx; a.ldy = ldy; a.momentum = momentum; a.eps = eps;
    a.fast = aligned16(X) && aligned16(Y) && ldx % 4 == 0 && ldy % 4 == 0 && C % 4 == 0;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_tile_bn_train_forward(a, ctx->stream));
    return LAFF_OK;
}

int laff_tile_bn_train_backward(laff_ctx* ctx, const float* dY, int lddy, const float* X, int N, int C, int ldx, int H, const float* gamma,
                                const float* save_mean, const float* save_invstd, float* dX, int lddx, float* dgamma, float* dbeta,
                                void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_tile_bn_train_backward";
    if (int rc = tile_bn_check(fn, N, C, H, gamma != nullptr, true)) return rc;
    CHECK_CTX(ctx);
    if (!dX && !dgamma && !dbeta) return LAFF_OK;
    if (!X || !dY || !save_mean || !save_invstd) return fail(LAFF_E_ARG, "%s: null X / dY / save_mean / save_invstd", fn);
    if (ldx < C || lddy < H * C || (dX && lddx < C))
        return fail(LAFF_E_SHAPE, "%s: a row pitch is below the row width (ldx=%d lddy=%d lddx=%d C=%d H=%d)", fn, ldx, lddy, lddx, C, H);
    if (!aligned4(X) || !aligned4(dY) || !aligned4(dX) || !aligned4(gamma) || !aligned4(save_mean) || !aligned4(save_invstd) ||
        !aligned4(dgamma) || !aligned4(dbeta))
        return fail(LAFF_E_ALIGN, "%s: every fp32 pointer must be 4-byte aligned", fn);
    laff::TileBnTrainArgs a{};
    if (int rc = bn_part(fn, N, H * C, true, workspace, workspace_bytes, &a.part)) return rc;
    a.X = X; a.dY = dY; a.dX = dX; a.gamma = gamma; a.save_mean = const_cast<float*>(save_mean);
    a.save_invstd = const_cast<float*>(save_invstd); a.dgamma = dgamma; a.dbeta = dbeta;
    a.N = N; a.C = C; a.H = H; a.ldx = ldx; a.lddy = lddy; a.lddx = lddx;
    a.fast = aligned16(X) && aligned16(dY) && ldx % 4 == 0 && lddy % 4 == 0 && C % 4 == 0 && (!dX || (aligned16(dX) && lddx % 4 == 0));
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_tile_bn_train_backward(a, ctx->stream));
    return LAFF_OK;
}

/* what the plan and both directions of the expert stage refuse before any GPU work, a null ctx included: the tests need no GPU */
static int expert_stage_shape(const char* fn, int N, int L, int D) {
    if (L < 1 || L > laff::EXPERT_MAX_PLANES) return fail(LAFF_E_SHAPE, "%s: need 1 <= L <= %d planes, got %d", fn, laff::EXPERT_MAX_PLANES, L);
    if (D < 4 || D % 4 != 0 || D > 8192) return fail(LAFF_E_SHAPE, "%s: need D %% 4 == 0 and 4 <= D <= 8192, got %d", fn, D);
    if (N < 0) return fail(LAFF_E_SHAPE, "%s: need N >= 0, got %d", fn, N);
    return LAFF_OK;
}
static int expert_stage_check(const char* fn, int N, int L, int D, const float* const* x, const int* ldx, const char* xname,
                              const float* expert, int lde, int l2norm, const float* stacked, int ldn, int ldl, const char* sname,
                              const float* rnorm) {
    if (int rc = expert_stage_shape(fn, N, L, D)) return rc;
    if (!expert && !l2norm) return fail(LAFF_E_ARG, "%s: neither an expert table nor l2norm: a plain copy is not provided", fn);
    if (N == 0) return LAFF_OK;                    /* no rows: nothing is addressed (torch hands null pointers for empty tensors) */
    if (!x || !ldx || !stacked) return fail(LAFF_E_ARG, "%s: null %s / its pitches / %s", fn, xname, sname);
    if (l2norm && !rnorm) return fail(LAFF_E_ARG, "%s: l2norm needs rnorm", fn);
    for (int l = 0; l < L; ++l) {
        if (!x[l]) return fail(LAFF_E_ARG, "%s: null %s[%d]", fn, xname, l);
        if (ldx[l] < D) return fail(LAFF_E_SHAPE, "%s: the row pitch of %s[%d] is below D (%d < %d)", fn, xname, l, ldx[l], D);
        if (ldx[l] % 4 != 0 || !aligned16(x[l]))
            return fail(LAFF_E_ALIGN, "%s: the rows of %s[%d] must be 16-byte aligned (base and pitch %d)", fn, xname, l, ldx[l]);
    }
    if (expert && lde < D) return fail(LAFF_E_SHAPE, "%s: the row pitch of expert is below D (%d < %d)", fn, lde, D);
    if (expert && (lde % 4 != 0 || !aligned16(expert))) return fail(LAFF_E_ALIGN, "%s: the rows of expert must be 16-byte aligned (base and pitch %d)", fn, lde);
    if (ldn < D || ldl < D || !((long long)ldn >= (long long)(L - 1) * ldl + D || (long long)ldl >= (long long)(N > 0 ? N - 1 : 0) * ldn + D))
        return fail(LAFF_E_SHAPE, "%s: the pitches of %s (row %d, plane %d) do not hold [N=%d, L=%d, D=%d] without overlap", fn, sname, ldn, ldl, N, L, D);
    if (ldn % 4 != 0 || ldl % 4 != 0 || !aligned16(stacked))
        return fail(LAFF_E_ALIGN, "%s: the rows of %s must be 16-byte aligned (base, row pitch %d, plane pitch %d)", fn, sname, ldn, ldl);
    if (rnorm && !aligned4(rnorm)) return fail(LAFF_E_ALIGN, "%s: rnorm must be 4-byte aligned", fn);
    return LAFF_OK;
}

int laff_expert_stage_train_plan(int N, int L, int D, int out[2]) {
    const char* fn = "laff_expert_stage_train_plan";
    if (!out) return fail(LAFF_E_ARG, "%s: null out", fn);
    if (int rc = expert_stage_shape(fn, N, L, D)) return rc;
    int chunks;
    size_t ws;
    laff::expert_stage_plan(N, L, D, &chunks, &ws);
    if (ws > (size_t)INT_MAX) return fail(LAFF_E_SHAPE, "%s: workspace of %zu bytes", fn, ws);
    out[0] = chunks; out[1] = (int)ws;
    return LAFF_OK;
}

int laff_expert_stage_train(laff_ctx* ctx, const float* const* x, const int* ldx, int N, int L, int D, const float* expert, int lde,
                            int l2norm, float* Y, int ldn, int ldl, float* rnorm) {
    const char* fn = "laff_expert_stage_train";
    if (int rc = expert_stage_check(fn, N, L, D, x, ldx, "x", expert, lde, l2norm, Y, ldn, ldl, "Y", rnorm)) return rc;
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;
    laff::ExpertStageArgs a{};
    for (int l = 0; l < L; ++l) { a.x[l] = x[l]; a.ldx[l] = ldx[l]; }
    a.expert = expert; a.lde = lde; a.Y = Y; a.rnorm = l2norm ? rnorm : nullptr; a.N = N; a.L = L; a.D = D; a.l2norm = l2norm != 0;
    a.ldn = ldn; a.ldl = ldl;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_expert_stage_forward(a, ctx->stream));
    return LAFF_OK;
}

int laff_expert_stage_train_backward(laff_ctx* ctx, const float* dY, int ldn, int ldl, const float* const* x, const int* ldx, int N, int L,
                                     int D, const float* expert, int lde, int l2norm, const float* rnorm, float* const* dx, const int* lddx,
                                     float* d_expert, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_expert_stage_train_backward";
    if (int rc = expert_stage_check(fn, N, L, D, x, ldx, "x", expert, lde, l2norm, dY, ldn, ldl, "dY", rnorm)) return rc;
    if (N > 0 && (!dx || !lddx)) return fail(LAFF_E_ARG, "%s: null dx / its pitches", fn);
    for (int l = 0; l < L && N > 0; ++l) {
        if (!dx[l]) return fail(LAFF_E_ARG, "%s: null dx[%d]", fn, l);
        if (lddx[l] < D) return fail(LAFF_E_SHAPE, "%s: the row pitch of dx[%d] is below D (%d < %d)", fn, l, lddx[l], D);
        if (lddx[l] % 4 != 0 || !aligned16(dx[l]))
            return fail(LAFF_E_ALIGN, "%s: the rows of dx[%d] must be 16-byte aligned (base and pitch %d)", fn, l, lddx[l]);
    }
    if (d_expert && !expert) return fail(LAFF_E_ARG, "%s: d_expert without an expert table", fn);
    if (d_expert && !aligned16(d_expert)) return fail(LAFF_E_ALIGN, "%s: d_expert must be 16-byte aligned", fn);
    int chunks;
    size_t ws;
    laff::expert_stage_plan(N, L, D, &chunks, &ws);
    if (d_expert && ws)
        if (int rc = need_workspace(fn, workspace, workspace_bytes, ws)) return rc;
    CHECK_CTX(ctx);
    laff::ExpertStageArgs a{};
    for (int l = 0; l < L && N > 0; ++l) { a.x[l] = x[l]; a.ldx[l] = ldx[l]; a.dx[l] = dx[l]; a.lddx[l] = lddx[l]; }
    a.expert = expert; a.lde = lde; a.dY = dY; a.rnorm = l2norm ? const_cast<float*>(rnorm) : nullptr; a.N = N; a.L = L; a.D = D;
    a.l2norm = l2norm != 0; a.ldn = ldn; a.ldl = ldl; a.d_expert = d_expert; a.part = d_expert && ws ? (float*)workspace : nullptr;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_expert_stage_backward(a, ctx->stream));
    return LAFF_OK;
}

static_assert(sizeof(laff_optim_tensor) == 40, "laff_optim_tensor is five 8-byte words (laff_amd/ops.py fills the host array as such)");

/* the launches of the calling thread's last optimizer call, by variant */
static thread_local laff::OptimLaunches g_optim_launches{};

/* a tensor list as the optimizer entry points take it: sizes and 4-byte alignment of `slots` pointers an entry (null only with n == 0) */
static int optim_check_list(const char* fn, const laff_optim_tensor* t, int count, bool want_s1, bool want_s2) {
    if (count < 0) return fail(LAFF_E_ARG, "%s: count=%d", fn, count);
    if (count > 0 && !t) return fail(LAFF_E_ARG, "%s: null tensor list", fn);
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
    for (int i = 0; i < count; ++i) {
        if (t[i].n < 0) return fail(LAFF_E_ARG, "%s: tensor %d has n=%lld", fn, i, t[i].n);
        if (t[i].n == 0) continue;
        if (!t[i].g || (want_s1 && (!t[i].p || !t[i].s1)) || (want_s2 && !t[i].s2))
            return fail(LAFF_E_ARG, "%s: tensor %d has a null pointer with n=%lld", fn, i, t[i].n);
        if (misaligned(t[i].p) || misaligned(t[i].g) || misaligned(t[i].s1) || misaligned(t[i].s2))
            return fail(LAFF_E_ALIGN, "%s: tensor %d: pointers must be 4-byte aligned", fn, i);
    }
    return LAFF_OK;
}

static int optim_check_workspace(const char* fn, const void* workspace, int partials) {
    if (partials < 0) return fail(LAFF_E_ARG, "%s: partials=%d", fn, partials);
    if (partials > 0 && !workspace) return fail(LAFF_E_ARG, "%s: null workspace with %d partials", fn, partials);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(LAFF_E_ALIGN, "%s: workspace must be 8-byte aligned", fn);
    return LAFF_OK;
}

int laff_optim_plan(int count, const long long* n, int out[6]) {
    if (!out) return fail(LAFF_E_ARG, "laff_optim_plan: null out");
    if (count < 0 || (count > 0 && !n)) return fail(LAFF_E_ARG, "laff_optim_plan: count=%d, n %s", count, n ? "given" : "null");
    for (int i = 0; i < count; ++i)
        if (n[i] < 0) return fail(LAFF_E_ARG, "laff_optim_plan: tensor %d has n=%lld", i, n[i]);
    laff::OptimPlan p;
    laff::optim_plan(count, n, &p);
    out[0] = laff::OPTIM_CHUNK; out[1] = laff::OPTIM_TABLE; out[2] = p.launches; out[3] = p.partials; out[4] = p.launches;
    out[5] = laff::OPTIM_GRID_CAP;
    return LAFF_OK;
}

int laff_optim_last_launches(int out[2]) {
    if (!out) return fail(LAFF_E_ARG, "laff_optim_last_launches: null out");
    out[0] = g_optim_launches.fast; out[1] = g_optim_launches.generic;
    return LAFF_OK;
}

int laff_grad_sqnorm(laff_ctx* ctx, int count, const float* const* g, const long long* n, void* workspace, size_t bytes) {
    CHECK_CTX(ctx);
    const char* fn = "laff_grad_sqnorm";
    if (count < 0 || (count > 0 && (!g || !n))) return fail(LAFF_E_ARG, "%s: count=%d with null g or n", fn, count);
    std::vector<laff_optim_tensor> t((size_t)count);
    for (int i = 0; i < count; ++i) t[i] = laff_optim_tensor{nullptr, g[i], nullptr, nullptr, n[i]};
    if (int rc = optim_check_list(fn, t.data(), count, false, false)) return rc;
    laff::OptimPlan p;
    laff::optim_plan(count, n, &p);
    if (bytes < 8 * (size_t)p.partials) return fail(LAFF_E_ARG, "%s: workspace too small (%zu < %zu bytes)", fn, bytes, 8 * (size_t)p.partials);
    if (int rc = optim_check_workspace(fn, workspace, p.partials)) return rc;
    g_optim_launches = {};
    DeviceGuard guard(ctx->device);
    HIP_TRY(laff::launch_optim_sqnorm(t.data(), count, (double*)workspace, &g_optim_launches, ctx->stream));
    return LAFF_OK;
}

int laff_grad_scale(laff_ctx* ctx, int count, float* const* g, const long long* n, double max_norm, const void* workspace, int partials,
                    float* total_norm_out) {
    CHECK_CTX(ctx);
    const char* fn = "laff_grad_scale";
    if (count < 0 || (count > 0 && (!g || !n))) return fail(LAFF_E_ARG, "%s: count=%d with null g or n", fn, count);
    std::vector<laff_optim_tensor> t((size_t)count);
    for (int i = 0; i < count; ++i) t[i] = laff_optim_tensor{g[i], g[i], nullptr, nullptr, n[i]};
    if (int rc = optim_check_list(fn, t.data(), count, false, false)) return rc;
    if (int rc = optim_check_workspace(fn, workspace, partials)) return rc;
    if (reinterpret_cast<uintptr_t>(total_norm_out) & 3) return fail(LAFF_E_ALIGN, "%s: total_norm_out must be 4-byte aligned", fn);
    g_optim_launches = {};
    DeviceGuard guard(ctx->device);
    HIP_TRY(laff::launch_optim_scale(t.data(), count, max_norm, (const double*)workspace, partials, total_norm_out, &g_optim_launches,
                                     ctx->stream));
    return LAFF_OK;
}

int laff_optim_step(laff_ctx* ctx, const laff_optim_tensor* t, int count, const laff_optim_hyper* h, double max_norm, const void* workspace,
                    int partials, float* total_norm_out) {
    CHECK_CTX(ctx);
    const char* fn = "laff_optim_step";
    if (!h) return fail(LAFF_E_ARG, "%s: null hyper-parameters", fn);
    if (h->kind != LAFF_OPT_ADAM && h->kind != LAFF_OPT_RMSPROP) return fail(LAFF_E_ARG, "%s: unknown kind %d", fn, h->kind);
    const bool adam = h->kind == LAFF_OPT_ADAM;
    if (h->step < 1) return fail(LAFF_E_ARG, "%s: step=%lld < 1", fn, h->step);
    if ((adam && !(h->beta1 >= 0.0 && h->beta1 < 1.0)) || !(h->beta2 >= 0.0 && h->beta2 < 1.0))
        return fail(LAFF_E_ARG, "%s: beta1=%g / beta2=%g outside [0, 1)", fn, h->beta1, h->beta2);
    if (!(h->eps >= 0.0)) return fail(LAFF_E_ARG, "%s: eps=%g < 0", fn, h->eps);
    if (!(h->weight_decay >= 0.0)) return fail(LAFF_E_ARG, "%s: weight_decay=%g < 0", fn, h->weight_decay);
    if (int rc = optim_check_list(fn, t, count, true, adam)) return rc;
    const bool clip = max_norm > 0.0;
    if (clip) {
        if (int rc = optim_check_workspace(fn, workspace, partials)) return rc;
        if (reinterpret_cast<uintptr_t>(total_norm_out) & 3) return fail(LAFF_E_ALIGN, "%s: total_norm_out must be 4-byte aligned", fn);
    }
    laff::OptimScalars s{};
    s.lr = (float)h->lr; s.omb1 = (float)(1.0 - h->beta1); s.b2 = (float)h->beta2; s.omb2 = (float)(1.0 - h->beta2);
    s.eps = (float)h->eps; s.wd = (float)h->weight_decay;
    s.bc1 = adam ? (float)(1.0 - std::pow(h->beta1, (double)h->step)) : 1.0f;
    s.bc2 = adam ? (float)(1.0 - std::pow(h->beta2, (double)h->step)) : 1.0f;
    g_optim_launches = {};
    DeviceGuard guard(ctx->device);
    HIP_TRY(laff::launch_optim_update(t, count, h->kind, s, clip ? max_norm : 0.0, clip ? (const double*)workspace : nullptr,
                                      clip ? partials : 0, clip ? total_norm_out : nullptr, &g_optim_launches, ctx->stream));
    return LAFF_OK;
}

static int frame_fuse_grouped(laff_ctx* ctx, int count, const float* const* frames, const int* lens, const float* mask, int ldm, int B, int Fmax,
                              int d, const float* const* w, const float* const* b, const float* const* gw, unsigned flags, float* const* V) {
    CHECK_CTX(ctx);
    if (B == 0 || count == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (count < 0 || !frames || !w || !b || !V) return fail(LAFF_E_ARG, "laff_frame_fuse: null frames/w/b/V");
    if (B < 0 || Fmax < 1 || d < 4 || (d & 3) || d > 1024)
        return fail(LAFF_E_SHAPE, "laff_frame_fuse: need B>=0, Fmax>=1, d%%4==0, d<=1024 (B=%d Fmax=%d d=%d)", B, Fmax, d);
    if (flags & ~(unsigned)(LAFF_ATT_WITH_AVE | LAFF_ATT_MUL)) return fail(LAFF_E_UNSUPPORTED, "laff_frame_fuse: flags 0x%x", flags);
    if ((long)B * (count < 8 ? count : 8) > 0x7fffffffL) return fail(LAFF_E_SHAPE, "laff_frame_fuse: grid too large");
    DeviceGuard g(ctx->device);
    for (int i0 = 0; i0 < count; i0 += 8) {
        laff::FrameGroup grp{};
        grp.count = count - i0 < 8 ? count - i0 : 8;
        for (int i = 0; i < grp.count; ++i) {
            const int k = i0 + i;
            if (!frames[k] || !w[k] || !b[k] || !V[k]) return fail(LAFF_E_ARG, "laff_frame_fuse: feature %d has a null pointer", k);
            if ((flags & LAFF_ATT_WITH_AVE) && (!gw || !gw[k])) return fail(LAFF_E_ARG, "laff_frame_fuse: WITH_AVE needs gw");
            if (!aligned16(frames[k]) || !aligned16(w[k]) || !aligned16(V[k])) return fail(LAFF_E_ALIGN, "laff_frame_fuse: 16-byte alignment");
            grp.f[i] = laff::FrameArgs{frames[k], lens, B, Fmax, d, w[k], b[k], gw ? gw[k] : nullptr, flags, V[k], mask, ldm};
        }
        HIP_TRY(laff::launch_frame_fuse(grp, ctx->stream));
    }
    return LAFF_OK;
}

int laff_frame_fuse_grouped(laff_ctx* ctx, int count, const float* const* frames, const int* lens, int B, int Fmax, int d,
                            const float* const* w, const float* const* b, const float* const* gw, unsigned flags, float* const* V) {
    return frame_fuse_grouped(ctx, count, frames, lens, nullptr, 0, B, Fmax, d, w, b, gw, flags, V);
}

int laff_frame_fuse_grouped_mask(laff_ctx* ctx, int count, const float* const* frames, const float* mask, int ldm, int B, int Fmax, int d,
                                 const float* const* w, const float* const* b, const float* const* gw, unsigned flags, float* const* V) {
    if (B > 0 && count > 0 && (!mask || ldm < Fmax)) return fail(LAFF_E_ARG, "laff_frame_fuse_grouped_mask: mask must be (B, ldm >= Fmax)");
    return frame_fuse_grouped(ctx, count, frames, nullptr, mask, ldm, B, Fmax, d, w, b, gw, flags, V);
}

int laff_frame_fuse(laff_ctx* ctx, const float* frames, const int* lens, int B, int Fmax, int d, const float* w,
                    const float* b, const float* gw, unsigned flags, float* V) {
    return laff_frame_fuse_grouped(ctx, 1, &frames, lens, B, Fmax, d, &w, &b, gw ? &gw : nullptr, flags, &V);
}

// the shape of laff_frame_fuse_backward and its plan: plain integers, checked before anything else
static int frame_backward_shape(const char* fn, int count, int B, int Fmax, int d) {
    if (count < 0 || B < 0 || Fmax < 1 || d < 4 || (d & 3) || d > 1024)
        return fail(LAFF_E_SHAPE, "%s: need count>=0, B>=0, Fmax>=1, d%%4==0, 4<=d<=1024 (count=%d B=%d Fmax=%d d=%d)", fn, count, B, Fmax, d);
    if ((long long)B * (count < 8 ? count : 8) > INT_MAX) return fail(LAFF_E_SHAPE, "%s: grid too large", fn);
    if ((long long)B * Fmax * d > (long long)INT_MAX * 4) return fail(LAFF_E_SHAPE, "%s: a feature of %lld elements", fn, (long long)B * Fmax * d);
    return LAFF_OK;
}

int laff_frame_fuse_backward_plan(int count, int B, int Fmax, int d, int want_dw, int out[4]) {
    if (!out) return fail(LAFF_E_ARG, "laff_frame_fuse_backward_plan: null out");
    if (int rc = frame_backward_shape("laff_frame_fuse_backward_plan", count, B, Fmax, d)) return rc;
    const long long bytes = want_dw ? (long long)count * B * d * (long long)sizeof(float) : 0;
    if (bytes > INT_MAX) return fail(LAFF_E_SHAPE, "laff_frame_fuse_backward_plan: workspace of %lld bytes", bytes);
    out[0] = (int)bytes; out[1] = laff::frame_bwd_variant(d); out[2] = (count + 7) / 8; out[3] = want_dw ? B : 0;
    return LAFF_OK;
}

int laff_frame_fuse_backward(laff_ctx* ctx, int count, const float* const* frames, const int* lens, int B, int Fmax, int d,
                             const float* const* w, const float* const* b, const float* const* gw, unsigned flags, const float* const* dV,
                             int lddv, float* const* dframes, float* const* dw, float* const* db, void* workspace, size_t workspace_bytes) {
    const char* fn = "laff_frame_fuse_backward";
    if (int rc = frame_backward_shape(fn, count, B, Fmax, d)) return rc;
    if (flags & ~(unsigned)(LAFF_ATT_WITH_AVE | LAFF_ATT_MUL)) return fail(LAFF_E_ARG, "%s: unknown flags 0x%x", fn, flags);
    if (lddv < d || (lddv & 3)) return fail(LAFF_E_SHAPE, "%s: lddv=%d (need >= %d, multiple of 4)", fn, lddv, d);
    CHECK_CTX(ctx);
    if (B == 0 || count == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!frames || !w || !b || !dV || !dframes) return fail(LAFF_E_ARG, "%s: null frames / w / b / dV / dframes", fn);
    if ((flags & LAFF_ATT_WITH_AVE) && !gw) return fail(LAFF_E_ARG, "%s: WITH_AVE needs gw", fn);
    for (int k = 0; k < count; ++k) {
        if (!frames[k] || !w[k] || !b[k] || !dV[k] || !dframes[k] || (dw && !dw[k]) || (db && !db[k]))
            return fail(LAFF_E_ARG, "%s: feature %d has a null pointer", fn, k);
        if ((flags & LAFF_ATT_WITH_AVE) && !gw[k]) return fail(LAFF_E_ARG, "%s: WITH_AVE needs gw (feature %d)", fn, k);
        if (!aligned16(frames[k]) || !aligned16(w[k]) || !aligned16(dV[k]) || !aligned16(dframes[k]) || (dw && !aligned16(dw[k])))
            return fail(LAFF_E_ALIGN, "%s: feature %d: frames / w / dV / dframes / dw must be 16-byte aligned", fn, k);
    }
    if (dw)
        if (int rc = need_workspace(fn, workspace, workspace_bytes, (size_t)count * B * d * sizeof(float))) return rc;
    DeviceGuard g(ctx->device);
    for (int i0 = 0; i0 < count; i0 += 8) {
        laff::FrameBwdGroup grp{};
        grp.count = count - i0 < 8 ? count - i0 : 8;
        grp.B = B; grp.Fmax = Fmax; grp.d = d; grp.lddv = lddv; grp.flags = flags; grp.lens = lens;
        grp.dw_part = dw ? (float*)workspace + (size_t)i0 * B * d : nullptr;
        for (int i = 0; i < grp.count; ++i) {
            const int k = i0 + i;
            grp.f[i] = laff::FrameBwdArgs{frames[k], w[k], b[k], gw ? gw[k] : nullptr, dV[k], dframes[k], dw ? dw[k] : nullptr,
                                          db ? db[k] : nullptr};
        }
        HIP_TRY(laff::launch_frame_fuse_backward(grp, dw || db, ctx->stream));
    }
    return LAFF_OK;
}

int laff_packed_bytes(int N, int K, int precision, size_t* out) {
    if (!out || N < 0 || K < 0) return fail(LAFF_E_ARG, "laff_packed_bytes: bad args");
    if (int rc = bad_precision("laff_packed_bytes", precision)) return rc;
    *out = (size_t)N * K * elem_size(precision) * (is_x3(precision) ? 2 : 1);
    return LAFF_OK;
}

int laff_pack_rows(laff_ctx* ctx, const float* E, int N, int H, int d, int lde, int normalize, float eps, float prescale,
                   int precision, void* out) {
    CHECK_CTX(ctx);
    if (N == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!E || !out) return fail(LAFF_E_ARG, "laff_pack_rows: null E/out");
    if (N < 0 || H < 1 || d < 1 || lde < H * d)
        return fail(LAFF_E_SHAPE, "laff_pack_rows: bad shape N=%d H=%d d=%d lde=%d", N, H, d, lde);
    if (int rc = bad_precision("laff_pack_rows", precision)) return rc;
    const bool vec = !(d & 3) && !(lde & 3) && aligned16(E) && aligned16(out);
    if (!vec && precision != LAFF_PREC_FP32)
        return fail(LAFF_E_ALIGN, "laff_pack_rows: 16-bit output needs d%%4==0, lde%%4==0 and 16-byte aligned buffers (d=%d lde=%d)", d, lde);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_pack_rows(E, N, H, d, lde, normalize, eps, prescale, precision, out, ctx->stream));
    return LAFF_OK;
}

// the GemmArgs of a similarity GEMM on laff_pack_rows operands (what laff_sim_gemm launches and laff_sim_gemm_route asks about)
static laff::GemmArgs sim_gemm_args(const void* T, const void* V, int Nt, int Nv, int K, float scale, int precision, float* S, int lds,
                                    const int* gt_col, int col0, const float* s_gt, int* count, const double* s_gt64, const float* band_t,
                                    const float* band_v, unsigned* pairs, unsigned pair_cap) {
    laff::GemmArgs a{};
    a.R = T; a.C = V; a.nR = Nt; a.nC = Nv; a.K = K; a.ldR = K; a.ldC = K;
    const long planeT = (long)Nt * K * 2, planeV = (long)Nv * K * 2;
    if (is_x3(precision)) {
        // virtual K concatenation: lo*hi, hi*lo first (small terms), hi*hi last
        a.nseg = 3;
        a.segR[0] = planeT; a.segC[0] = 0;
        a.segR[1] = 0;      a.segC[1] = planeV;
        a.segR[2] = 0;      a.segC[2] = 0;
    } else {
        a.nseg = 1; a.segR[0] = a.segC[0] = 0;
    }
    a.out = S; a.ldo = lds; a.scale = scale;
    a.gt_col = gt_col; a.col0 = col0; a.s_gt = s_gt; a.count = gt_col ? count : nullptr;
    a.s_gt64 = s_gt64; a.band_r = band_t; a.band_c = band_v; a.pairs = pairs; a.pair_cap = pair_cap;
#ifdef LAFF_GEMM_TRACE
    if (const char* e = getenv("LAFF_GEMM_TRACE_PTR")) a.trace = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
    return a;
}

static int sim_gemm_mode(int precision) {
    if (precision == LAFF_PREC_FP16 || precision == LAFF_PREC_FP16X3) return laff::GEMM_F16;
    if (precision == LAFF_PREC_BF16 || precision == LAFF_PREC_BF16X3) return laff::GEMM_BF16;
    return laff::GEMM_F32;
}

// rows of K elements: 16-byte aligned rows take the direct-to-LDS paths (K bytes a multiple of 128: the fast one),
// anything else is staged through registers with element-wise K bounds
static bool sim_gemm_aligned(int K, int precision) { return ((long)K * elem_size(precision)) % 16 == 0; }

static int sim_gemm_impl(laff_ctx* ctx, const char* who, const void* T, const void* V, int Nt, int Nv, int K, float scale,
                         int precision, float* S, int lds, const int* gt_col, int col0, const float* s_gt, int* count,
                         const double* s_gt64, const float* band_t, const float* band_v, unsigned* pairs, unsigned pair_cap) {
    CHECK_CTX(ctx);
    if (Nt == 0 || Nv == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!T || !V) return fail(LAFF_E_ARG, "%s: null T/V", who);
    if (int rc = bad_precision(who, precision)) return rc;
    if (Nt < 0 || Nv < 0 || K < 1 || ((long)K * elem_size(precision)) % 4)
        return fail(LAFF_E_SHAPE, "%s: K must be positive (and even for 16-bit operands) (Nt=%d Nv=%d K=%d)", who, Nt, Nv, K);
    if (!S && !gt_col) return fail(LAFF_E_ARG, "%s: nothing to produce (S and gt_col both null)", who);
    if (S && lds < Nv) return fail(LAFF_E_SHAPE, "%s: lds=%d < Nv=%d", who, lds, Nv);
    if (gt_col && !count) return fail(LAFF_E_ARG, "%s: gt_col needs count", who);
    if (gt_col && !s_gt && !s_gt64) return fail(LAFF_E_ARG, "%s: gt_col needs the ground-truth scores", who);
    pair_cap &= ~3u;            /* the resolve kernel reads the list four slots at a time: a ragged tail is never used */
    if (s_gt64 && (!gt_col || !band_t || !band_v || !pairs || pair_cap < 4))
        return fail(LAFF_E_ARG, "%s: the banded count needs gt_col, band_t, band_v and a pair list of >= 4 slots", who);
    if (!aligned16(T) || !aligned16(V)) return fail(LAFF_E_ALIGN, "%s: operands must be 16-byte aligned", who);
    if (s_gt64 && (!aligned16(gt_col) || !aligned16(s_gt64) || !aligned16(band_t) || !aligned16(band_v)))
        return fail(LAFF_E_ALIGN, "%s: gt_col, s_gt64, band_t and band_v must be 16-byte aligned (fetched in 16-byte groups)", who);
    const laff::GemmArgs a = sim_gemm_args(T, V, Nt, Nv, K, scale, precision, S, lds, gt_col, col0, s_gt, count, s_gt64, band_t, band_v,
                                           pairs, pair_cap);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_gemm_nt(a, sim_gemm_mode(precision), sim_gemm_aligned(K, precision), ctx->stream));
    return LAFF_OK;
}

int laff_sim_gemm(laff_ctx* ctx, const void* T, const void* V, int Nt, int Nv, int K, float scale, int precision,
                  float* S, int lds, const int* gt_col, int col0, const float* s_gt, int* count) {
    if (gt_col && !s_gt) return fail(LAFF_E_ARG, "laff_sim_gemm: gt_col needs s_gt and count");
    return sim_gemm_impl(ctx, "laff_sim_gemm", T, V, Nt, Nv, K, scale, precision, S, lds, gt_col, col0, s_gt, count, nullptr, nullptr,
                         nullptr, nullptr, 0);
}

int laff_sim_gemm_banded(laff_ctx* ctx, const void* T, const void* V, int Nt, int Nv, int K, float scale, int precision, float* S,
                         int lds, const int* gt_col, int col0, const double* s_gt64, const float* band_t, const float* band_v,
                         int* count, unsigned* pairs, unsigned pair_cap) {
    if (!gt_col || !s_gt64) return fail(LAFF_E_ARG, "laff_sim_gemm_banded: null gt_col / s_gt64");
    return sim_gemm_impl(ctx, "laff_sim_gemm_banded", T, V, Nt, Nv, K, scale, precision, S, lds, gt_col, col0, nullptr, count, s_gt64,
                         band_t, band_v, pairs, pair_cap);
}

int laff_sim_gemm_route(laff_ctx* ctx, int Nt, int Nv, int K, int precision, int lds, int count_mode, unsigned pair_cap, int* route) {
    CHECK_CTX(ctx);
    if (!route) return fail(LAFF_E_ARG, "laff_sim_gemm_route: null route");
    if (int rc = bad_precision("laff_sim_gemm_route", precision)) return rc;
    if (count_mode < 0 || count_mode > 2) return fail(LAFF_E_ARG, "laff_sim_gemm_route: bad count_mode %d", count_mode);
    if (Nt < 1 || Nv < 1 || K < 1 || ((long)K * elem_size(precision)) % 4 || (lds && lds < Nv) || (!lds && !count_mode))
        return fail(LAFF_E_SHAPE, "laff_sim_gemm_route: no launch for Nt=%d Nv=%d K=%d lds=%d count_mode=%d", Nt, Nv, K, lds, count_mode);
    pair_cap &= ~3u;
    if (count_mode == 2 && pair_cap < 4) return fail(LAFF_E_ARG, "laff_sim_gemm_route: the banded count needs a pair list of >= 4 slots");
    // stand-ins for the caller's buffers: the choice looks at which are present and at the alignment of S, never at what they hold
    alignas(16) static char stand_in[16];
    void* p = stand_in;
    const laff::GemmArgs a = sim_gemm_args(p, p, Nt, Nv, K, 1.0f, precision, lds ? (float*)p : nullptr, lds, count_mode ? (const int*)p : nullptr, 0,
                                           count_mode == 1 ? (const float*)p : nullptr, count_mode ? (int*)p : nullptr,
                                           count_mode == 2 ? (const double*)p : nullptr, count_mode == 2 ? (const float*)p : nullptr,
                                           count_mode == 2 ? (const float*)p : nullptr, count_mode == 2 ? (unsigned*)p : nullptr,
                                           count_mode == 2 ? pair_cap : 0);
    *route = laff::gemm_route(a, sim_gemm_mode(precision), sim_gemm_aligned(K, precision));
    return LAFF_OK;
}

// what the three laff_rank_prepare* entry points share behind their own null / empty-problem rules
static int rank_prepare_impl(laff_ctx* ctx, const char* who, int sides, int emit, const float* Et, const float* Ev, const void* T,
                             const void* V, int Nt, int Nv, int H, int d, int precision, float prescale, const int* gt_col, int col0,
                             double* s_gt64, float* band_t, float* band_v, int* zero_count, unsigned* pairs) {
    if (int rc = bad_precision(who, precision)) return rc;
    if (Nt < 0 || Nv < 0 || H < 1 || d < 4 || (d & 3)) return fail(LAFF_E_SHAPE, "%s: need H >= 1, d %% 4 == 0 (Nt=%d Nv=%d H=%d d=%d)", who, Nt, Nv, H, d);
    if (!(prescale > 0.0f)) return fail(LAFF_E_ARG, "%s: prescale must be positive", who);
    if ((Et && !aligned16(Et)) || (Ev && !aligned16(Ev)) || (T && !aligned16(T)) || (V && !aligned16(V)))
        return fail(LAFF_E_ALIGN, "%s: embeddings and operands must be 16-byte aligned", who);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_rank_prepare(Et, Ev, T, V, Nt, Nv, H, d, precision, prescale, gt_col, col0, s_gt64, band_t, band_v, zero_count,
                                      pairs, sides, ctx->stream, emit));
    return LAFF_OK;
}

int laff_rank_prepare(laff_ctx* ctx, const float* Et, const float* Ev, const void* T, const void* V, int Nt, int Nv, int H, int d,
                      int precision, float prescale, const int* gt_col, int col0, double* s_gt64, float* band_t, float* band_v,
                      int* zero_count, unsigned* pairs) {
    CHECK_CTX(ctx);
    if (Nt == 0 && Nv == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if ((Nt > 0 && (!Et || !T || !gt_col || !s_gt64 || !band_t)) || (Nv > 0 && (!Ev || !V || !band_v)))
        return fail(LAFF_E_ARG, "laff_rank_prepare: null argument");
    return rank_prepare_impl(ctx, "laff_rank_prepare", 3, 0, Et, Ev, T, V, Nt, Nv, H, d, precision, prescale, gt_col, col0, s_gt64, band_t,
                             band_v, zero_count, pairs);
}

int laff_rank_prepare_part(laff_ctx* ctx, int sides, const float* Et, const float* Ev, const void* T, const void* V, int Nt, int Nv, int H,
                           int d, int precision, float prescale, const int* gt_col, int col0, double* s_gt64, float* band_t, float* band_v,
                           int* zero_count, unsigned* pairs) {
    CHECK_CTX(ctx);
    if (sides != 1 && sides != 2) return fail(LAFF_E_ARG, "laff_rank_prepare_part: sides must be 1 (text rows) or 2 (video rows)");
    if ((sides == 1 && Nt == 0) || (sides == 2 && Nv == 0)) return LAFF_OK;
    if (sides == 1 && (!Et || !T || !gt_col || !s_gt64 || !band_t || (Nv > 0 && !Ev))) return fail(LAFF_E_ARG, "laff_rank_prepare_part: null argument (text side)");
    if (sides == 2 && (!Ev || !V || !band_v)) return fail(LAFF_E_ARG, "laff_rank_prepare_part: null argument (video side)");
    return rank_prepare_impl(ctx, "laff_rank_prepare_part", sides, 0, Et, Ev, T, V, Nt, Nv, H, d, precision, prescale, gt_col, col0, s_gt64,
                             band_t, band_v, zero_count, pairs);
}

int laff_rank_prepare_emit(laff_ctx* ctx, int emit, const float* Et, const float* Ev, void* T, void* V, int Nt, int Nv, int H, int d,
                           int precision, float prescale, const int* gt_col, int col0, double* s_gt64, float* band_t, float* band_v,
                           int* zero_count, unsigned* pairs) {
    CHECK_CTX(ctx);
    if (emit < 1 || emit > 3) return fail(LAFF_E_ARG, "laff_rank_prepare_emit: emit must be 1 (T), 2 (V) or 3 (both)");
    if (precision != LAFF_PREC_FP16 && precision != LAFF_PREC_BF16)
        return fail(LAFF_E_UNSUPPORTED, "laff_rank_prepare_emit: single-plane 16-bit operands only (precision %d): call laff_pack_rows + laff_rank_prepare", precision);
    if (Nt == 0 || Nv == 0) return LAFF_OK;
    if (!Et || !Ev || !T || !V || !gt_col || !s_gt64 || !band_t || !band_v) return fail(LAFF_E_ARG, "laff_rank_prepare_emit: null argument");
    return rank_prepare_impl(ctx, "laff_rank_prepare_emit", 3, emit, Et, Ev, T, V, Nt, Nv, H, d, precision, prescale, gt_col, col0, s_gt64,
                             band_t, band_v, zero_count, pairs);
}

int laff_rank_export_pairs(laff_ctx* ctx, const double* s_gt64, int* count, float* S, int lds, int Nv, unsigned* pairs, unsigned pair_cap,
                           const int* bounds, int world, int col0, unsigned* out, unsigned cap, unsigned* fill) {
    CHECK_CTX(ctx);
    if (!s_gt64 || !count || !pairs || !bounds || !out || !fill) return fail(LAFF_E_ARG, "laff_rank_export_pairs: null argument");
    pair_cap &= ~3u;
    if (world < 1 || world > 16 || cap < 4 || (cap & 3) || pair_cap < 4) return fail(LAFF_E_SHAPE, "laff_rank_export_pairs: need 1 <= world <= 16, cap %% 4 == 0 (world=%d cap=%u)", world, cap);
    if (S && lds < Nv) return fail(LAFF_E_SHAPE, "laff_rank_export_pairs: lds=%d < Nv=%d", lds, Nv);
    if (!aligned16(out)) return fail(LAFF_E_ALIGN, "laff_rank_export_pairs: out must be 16-byte aligned");
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_rank_export(s_gt64, count, S, lds, pairs, pair_cap, bounds, world, col0, out, cap, fill, ctx->stream));
    return LAFF_OK;
}

// the arguments laff_rank_resolve and laff_rank_resolve_metrics share; pair_cap comes back as whole groups of four slots (as
// laff_sim_gemm_banded uses the list)
static int rank_resolve_checks(const char* who, const float* Et, const float* Ev, int Nt, int Nv, int H, int d, const double* s_gt64,
                               const int* count, const float* S, int lds, const unsigned* pairs, unsigned& pair_cap) {
    if (!Et || !Ev || !s_gt64 || !count || !pairs) return fail(LAFF_E_ARG, "%s: null argument", who);
    pair_cap &= ~3u;
    if (Nt < 0 || Nv < 0 || H < 1 || d < 4 || (d & 3) || pair_cap < 4) return fail(LAFF_E_SHAPE, "%s: bad shape", who);
    if (S && lds < Nv) return fail(LAFF_E_SHAPE, "%s: lds=%d < Nv=%d", who, lds, Nv);
    if (!aligned16(Et) || !aligned16(Ev)) return fail(LAFF_E_ALIGN, "%s: embeddings must be 16-byte aligned", who);
    return LAFF_OK;
}

int laff_rank_resolve(laff_ctx* ctx, const float* Et, const float* Ev, int Nt, int Nv, int H, int d, const double* s_gt64,
                      int* count, float* S, int lds, unsigned* pairs, unsigned pair_cap) {
    CHECK_CTX(ctx);
    if (Nt == 0 || Nv == 0) return LAFF_OK;                 /* empty problem: nothing was listed */
    if (int rc = rank_resolve_checks("laff_rank_resolve", Et, Ev, Nt, Nv, H, d, s_gt64, count, S, lds, pairs, pair_cap)) return rc;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_rank_resolve(Et, Ev, Nt, Nv, H, d, s_gt64, count, S, lds, pairs, pair_cap, ctx->stream));
    return LAFF_OK;
}

int laff_rank_resolve_metrics(laff_ctx* ctx, const float* Et, const float* Ev, int Nt, int Nv, int H, int d, const double* s_gt64,
                              int* count, float* S, int lds, unsigned* pairs, unsigned pair_cap, int base, int* ranks_out, double* out8,
                              int synchronous) {
    CHECK_CTX(ctx);
    if (!out8) return fail(LAFF_E_ARG, "laff_rank_resolve_metrics: null out8");
    if (Nt < 1 || Nv < 1) return fail(LAFF_E_SHAPE, "laff_rank_resolve_metrics: Nt=%d Nv=%d (the metrics of an empty query set are undefined)", Nt, Nv);
    if (int rc = rank_resolve_checks("laff_rank_resolve_metrics", Et, Ev, Nt, Nv, H, d, s_gt64, count, S, lds, pairs, pair_cap)) return rc;
    DeviceGuard g(ctx->device);
    if (int rc = metrics_buffers(ctx)) return rc;
    const size_t si = synchronous ? 0 : next_metrics_slot(ctx);
    double* slot = ctx->d_metrics + 8 * si;
    unsigned* ticket = (unsigned*)(ctx->d_mscratch + si * laff::rank_metrics_scratch_bytes() + laff::rank_resolve_ticket_offset());
    double* host8 = synchronous ? nullptr : pinned_alias(out8);
    HIP_TRY(laff::launch_rank_resolve(Et, Ev, Nt, Nv, H, d, s_gt64, count, S, lds, pairs, pair_cap, ctx->stream, Nt, base, ranks_out, slot,
                                      host8, ticket));
    if (synchronous) {
        if (int rc = metrics_read_back(ctx, out8, "laff_rank_resolve_metrics: a rank < 1 was found (the pair list of laff_sim_gemm_banded "
                                                  "overflowed, or the counts are corrupt)"))
            return rc;
        out8[7] = 0.0;
        return LAFF_OK;
    }
    if (!host8) HIP_TRY(hipMemcpyAsync(out8, slot, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return LAFF_OK;
}

int laff_gather_gt(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* gt_col, int col0, float* s_gt) {
    CHECK_CTX(ctx);
    if (Nt == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!S || !gt_col || !s_gt) return fail(LAFF_E_ARG, "laff_gather_gt: null argument");
    if (Nt < 0 || Nv < 0 || lds < Nv) return fail(LAFF_E_SHAPE, "laff_gather_gt: bad shape");
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_gather_gt(S, Nt, Nv, lds, gt_col, col0, s_gt, ctx->stream));
    return LAFF_OK;
}

int laff_rank_count(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* gt_col, int col0,
                    const float* s_gt, int* count, int accumulate) {
    CHECK_CTX(ctx);
    if (Nt == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!S || !gt_col || !s_gt || !count) return fail(LAFF_E_ARG, "laff_rank_count: null argument");
    if (Nt < 0 || Nv < 0 || lds < Nv) return fail(LAFF_E_SHAPE, "laff_rank_count: bad shape");
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_rank_count(S, Nt, Nv, lds, gt_col, col0, s_gt, count, accumulate, ctx->stream));
    return LAFF_OK;
}

int laff_topk_rows(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, int K, int* idx_out, float* val_out) {
    CHECK_CTX(ctx);
    if (Nt == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!S || !idx_out || !val_out) return fail(LAFF_E_ARG, "laff_topk_rows: null argument");
    if (Nt < 0 || Nv < 1 || lds < Nv || K < 1 || K > Nv || K > 8192) return fail(LAFF_E_SHAPE, "laff_topk_rows: need 1 <= K <= min(Nv, 8192) (Nt=%d Nv=%d K=%d)", Nt, Nv, K);
    {
        const size_t kp = K <= 64 ? 64 : (K <= 512 ? 512 : (K <= 2048 ? 2048 : (K <= 4096 ? 4096 : 8192)));
        if ((size_t)((Nv + 3) & ~3) * 4 + kp * 8 + 256 * 4 + 16 > 160 * 1024)
            return fail(LAFF_E_UNSUPPORTED, "laff_topk_rows: Nv=%d with K=%d does not fit the LDS-resident row (%zu columns at most: split the "
                        "columns and merge the per-block lists, as laff_amd.ops.topk_rows does)", Nv, K, (160 * 1024 - kp * 8 - 1040) / 4);
    }
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_topk_rows(S, Nt, Nv, lds, K, idx_out, val_out, ctx->stream));
    return LAFF_OK;
}

int laff_v2t_count(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* grp_off, const int* grp_idx,
                   int max_group, int* count) {
    CHECK_CTX(ctx);
    if (Nt == 0 || Nv == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!S || !grp_off || !grp_idx || !count) return fail(LAFF_E_ARG, "laff_v2t_count: null argument");
    if (Nt < 0 || Nv < 0 || lds < Nv || max_group < 0) return fail(LAFF_E_SHAPE, "laff_v2t_count: bad shape");
    if (Nt == 0 || Nv == 0 || max_group == 0) return LAFF_OK;
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_v2t_count(S, Nt, Nv, lds, grp_off, grp_idx, max_group, count, ctx->stream));
    return LAFF_OK;
}

int laff_v2t_count_exact(laff_ctx* ctx, const float* S, int Nt, int Nv, int lds, const int* grp_off, const int* grp_idx,
                         int max_group, const float* Et, const float* Ev, int H, int d, const double* s_gt64,
                         const float* band_t, const float* band_v, int* count, unsigned* list, unsigned list_cap) {
    CHECK_CTX(ctx);
    if (Nt == 0 || Nv == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!S || !grp_off || !grp_idx || !count || !Et || !Ev || !s_gt64 || !band_t || !band_v || !list)
        return fail(LAFF_E_ARG, "laff_v2t_count_exact: null argument");
    if (Nt < 0 || Nv < 0 || lds < Nv || max_group < 0 || H < 1 || d < 4 || (d & 3))
        return fail(LAFF_E_SHAPE, "laff_v2t_count_exact: bad shape (Nt=%d Nv=%d lds=%d H=%d d=%d: d must be a multiple of 4)", Nt, Nv, lds, H, d);
    if (!aligned16(Et) || !aligned16(Ev)) return fail(LAFF_E_ALIGN, "laff_v2t_count_exact: embeddings must be 16-byte aligned");
    if (list_cap < 1) return fail(LAFF_E_SHAPE, "laff_v2t_count_exact: list_cap must be >= 1");
    DeviceGuard g(ctx->device);
    if (max_group == 0) {
        HIP_TRY(hipMemsetAsync(count, 0, (size_t)Nt * sizeof(int), ctx->stream));
        HIP_TRY(hipMemsetAsync(list, 0, 16, ctx->stream));
        return LAFF_OK;
    }
    HIP_TRY(laff::launch_v2t_count_exact(S, Nt, Nv, lds, grp_off, grp_idx, max_group, Et, Ev, H, d, s_gt64, band_t, band_v, count, list,
                                         list_cap, ctx->stream));
    return LAFF_OK;
}

int laff_row_dot_gt(laff_ctx* ctx, const void* T, const void* V, int Nt, int Nv, int K, float scale, int precision,
                    const int* gt_col, int col0, float* s_gt, int* zero_count) {
    CHECK_CTX(ctx);
    if (Nt == 0) return LAFF_OK;                 /* empty problem: nothing to launch, pointers may be null */
    if (!T || !V || !gt_col || !s_gt) return fail(LAFF_E_ARG, "laff_row_dot_gt: null argument");
    if (precision < LAFF_PREC_FP16 || precision > LAFF_PREC_BF16X3) return fail(LAFF_E_UNSUPPORTED, "laff_row_dot_gt: 16-bit precisions only (got %d)", precision);
    if (Nt < 0 || Nv < 0 || K < 2 || (K & 1)) return fail(LAFF_E_SHAPE, "laff_row_dot_gt: K must be positive and even (K=%d)", K);
    if (!aligned16(T) || !aligned16(V)) return fail(LAFF_E_ALIGN, "laff_row_dot_gt: operands must be 16-byte aligned");
    const int bf16 = (precision == LAFF_PREC_BF16 || precision == LAFF_PREC_BF16X3);
    DeviceGuard g(ctx->device);
    HIP_TRY(laff::launch_row_dot_gt(T, V, Nt, Nv, K, bf16, is_x3(precision) ? 1 : 0, scale, gt_col, col0, s_gt, zero_count, ctx->stream));
    return LAFF_OK;
}

int laff_rank_metrics_async(laff_ctx* ctx, const int* rank1, int Nq, int base, int* ranks_out, double* out8) {
    CHECK_CTX(ctx);
    if (!rank1 || !out8) return fail(LAFF_E_ARG, "laff_rank_metrics_async: null argument");
    if (Nq < 1) return fail(LAFF_E_SHAPE, "laff_rank_metrics_async: Nq=%d", Nq);
    DeviceGuard g(ctx->device);
    if (int rc = metrics_buffers(ctx)) return rc;
    const size_t si = next_metrics_slot(ctx);
    double* slot = ctx->d_metrics + 8 * si;
    double* host8 = pinned_alias(out8);
    HIP_TRY(laff::launch_rank_metrics(rank1, Nq, base, ranks_out, slot, slot + 7,
                                      (unsigned*)(ctx->d_mscratch + si * laff::rank_metrics_scratch_bytes()), ctx->stream, host8));
    if (!host8) HIP_TRY(hipMemcpyAsync(out8, slot, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return LAFF_OK;
}

int laff_rank_metrics(laff_ctx* ctx, const int* rank1, int Nq, int base, int* ranks_out, double out7[7]) {
    CHECK_CTX(ctx);
    if (!rank1 || !out7) return fail(LAFF_E_ARG, "laff_rank_metrics: null argument");
    if (Nq < 1) return fail(LAFF_E_SHAPE, "laff_rank_metrics: Nq=%d", Nq);
    DeviceGuard g(ctx->device);
    if (int rc = metrics_buffers(ctx)) return rc;
    HIP_TRY(laff::launch_rank_metrics(rank1, Nq, base, ranks_out, ctx->d_metrics, ctx->d_metrics + 7, (unsigned*)ctx->d_mscratch, ctx->stream));
    return metrics_read_back(ctx, out7, "laff_rank_metrics: a rank < 1 was found (ranks must be 1-based; a poisoned count also means the "
                                        "pair list of laff_sim_gemm_banded overflowed)");
}

}  // extern "C"
