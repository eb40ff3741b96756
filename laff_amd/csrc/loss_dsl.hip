// loss_dsl.hip -- dual-softmax loss on the in-batch cosine score matrix, per head, forward + backward, fp32
// (/root/reference/loss.py:291-310 DualSoftmaxLoss, summed over heads as model/model.py:2032-2048 does with any criterion).
//
//   M = l2norm(s) . l2norm(im)^T          rows = captions, columns = videos, n = B, temperature t
//   cal(X):  A[i][j] = exp(X[i][j]/t) / sum_i' exp(X[i'][j]/t)         softmax down each column       (loss.py:304)
//            P       = n * X (.) A
//            cal     = -sum_i (P[i][i] - logsumexp_j P[i][j])          log-softmax along each row     (loss.py:306-309)
//            with G = softmax_row(P) - I:
//            dX[i][j] = n A G + (n/t) A (X G - c[j]),   c[j] = sum_i' A[i'][j] X[i'][j] G[i'][j]
//   loss = (cal(M) + cal(M^T)) / 2
//
// The B x B x d contractions stay on the fp32 MFMA GEMM and the row normalisation on loss.hip; this file is the part between them.
// Like margin_reduce_kernel it is one 1024-thread workgroup per head sweeping the matrix from L2: batches are small, the kernel is
// latency-bound.  A transposed copy of M is made first, so that cal(M^T) is cal(M) with the two copies exchanged and every sweep reads
// rows (coalesced), one wave per row.  Per side w (X_0 = M, X_1 = M^T) three sweeps:
//   1. rows of X_(1-w) = columns of X_w:  amax[j], asum[j]                       (the column softmax of X_w / t)
//   2. rows of X_w:                       pmax[i], psum[i] of P, and the loss term of row i
//   3. rows of X_(1-w) again:             c[j]
// and one more writes dM = (dX_0 + dX_1^T) / 2 and, as a transposed store of the same values, dM^T.  Every softmax and
// log-sum-exp takes its maximum first (a separate pass over the row, which sits in L1), so t = 0.01 (logits of +-100) is as safe as
// t = 1000.  The per-row statistics live in the workspace, not in LDS: B is bounded by the margin loss's range, not by 10 B floats.
#include "kernels.h"
#include "wave_reduce.h"

namespace laff {

namespace {
enum { AMAX = 0, ASUM = 1, PMAX = 2, PSUM = 3, CSUM = 4, STAT_PER_SIDE = 5 };
static_assert(2 * STAT_PER_SIDE == DSL_STAT_ROWS, "stat layout");

struct DslArgs {
    const float* S;       // [H][B][Bp] scores (rows = captions, columns = videos)
    float* ST;            // [H][B][Bp] scratch: the transpose
    float* stat;          // [H][2][STAT_PER_SIDE][B] scratch
    float* dS;            // [H][B][Bp] dLoss/dScores, or null (forward only)
    float* dST;           // [H][B][Bp] its transpose
    float* loss_h;        // [H]
    int B, Bp;
    float temp;
};

// A of one element from its column's statistics
__device__ __forceinline__ float dsl_a(float x, float amax, float asum, float temp) { return expf((x - amax) / temp) / asum; }

// d cal(X_w) / d X_w[ip][ja] for the element value x
__device__ __forceinline__ float dsl_grad(const float* st, int B, float x, int ja, int ip, float n, float temp) {
    const float A = dsl_a(x, st[AMAX * B + ja], st[ASUM * B + ja], temp);
    const float P = x * A * n;
    const float G = expf(P - st[PMAX * B + ip]) / st[PSUM * B + ip] - (ja == ip ? 1.0f : 0.0f);
    return n * A * G + (n / temp) * A * (x * G - st[CSUM * B + ja]);
}
}  // namespace

__global__ __launch_bounds__(1024) void dsl_reduce_kernel(DslArgs a) {
    __shared__ double red[16];
    const int B = a.B, Bp = a.Bp, h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float temp = a.temp, n = (float)B;
    const float* X[2] = {a.S + (long)h * B * Bp, a.ST + (long)h * B * Bp};
    float* XT = a.ST + (long)h * B * Bp;
    float* st[2] = {a.stat + (long)h * DSL_STAT_ROWS * B, a.stat + ((long)h * DSL_STAT_ROWS + STAT_PER_SIDE) * B};

    for (long e = tid; e < (long)B * B; e += 1024) {
        const int i = (int)(e / B), j = (int)(e % B);
        XT[(long)j * Bp + i] = X[0][(long)i * Bp + j];
    }
    __syncthreads();

    // sweep 1: row r of X_(1-w) is column r of X_w
    for (int w = 0; w < 2; ++w)
        for (int r = wave; r < B; r += 16) {
            const float* row = X[1 - w] + (long)r * Bp;
            float m = -INFINITY;
            for (int k = lane; k < B; k += 64) m = fmaxf(m, row[k]);
            m = wave_allmax(m);
            float s = 0.0f;
            for (int k = lane; k < B; k += 64) s += expf((row[k] - m) / temp);
            s = wave_allsum(s);
            if (lane == 0) {
                st[w][AMAX * B + r] = m;
                st[w][ASUM * B + r] = s;
            }
        }
    __syncthreads();

    // sweep 2: row i of X_w -> the row statistics of P and -log softmax_row(P)[i][i]
    // The log-sum-exp of the loss runs in fp64: the 2 B row terms all carry the same sign of the fp32 exp / log's residual bias
    // (~1e-7 each), which adds up to more than an ulp of the loss from B = 65 on; in fp64 the loss keeps only the rounding of P.
    double loss = 0.0;
    for (int w = 0; w < 2; ++w)
        for (int i = wave; i < B; i += 16) {
            const float* row = X[w] + (long)i * Bp;
            float m = -INFINITY;
            for (int j = lane; j < B; j += 64) m = fmaxf(m, row[j] * dsl_a(row[j], st[w][AMAX * B + j], st[w][ASUM * B + j], temp) * n);
            m = wave_allmax(m);
            double s = 0.0;
            for (int j = lane; j < B; j += 64)
                s += exp((double)(row[j] * dsl_a(row[j], st[w][AMAX * B + j], st[w][ASUM * B + j], temp) * n - m));
            s = wave_allsum(s);
            const float pii = row[i] * dsl_a(row[i], st[w][AMAX * B + i], st[w][ASUM * B + i], temp) * n;
            loss += log(s) - (double)(pii - m);
            if (lane == 0) {
                st[w][PMAX * B + i] = m;
                st[w][PSUM * B + i] = (float)s;
            }
        }
    if (lane == 0) red[wave] = loss;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int v = 0; v < 16; ++v) t += red[v];
        a.loss_h[h] = (float)(0.5 * t);
    }
    if (!a.dS) return;

    // sweep 3: c[j] of X_w along row j of X_(1-w)
    for (int w = 0; w < 2; ++w)
        for (int j = wave; j < B; j += 16) {
            const float* row = X[1 - w] + (long)j * Bp;
            const float amax = st[w][AMAX * B + j], asum = st[w][ASUM * B + j];
            float c = 0.0f;
            for (int i = lane; i < B; i += 64) {
                const float x = row[i];
                const float A = dsl_a(x, amax, asum, temp);
                const float G = expf(x * A * n - st[w][PMAX * B + i]) / st[w][PSUM * B + i] - (i == j ? 1.0f : 0.0f);
                c += A * x * G;
            }
            c = wave_allsum(c);
            if (lane == 0) st[w][CSUM * B + j] = c;
        }
    __syncthreads();

    // dM[r][k] = (dX_0[r][k] + dX_1[k][r]) / 2, one wave per row of M; dM^T is the transposed store of the same value (as
    // margin_reduce_kernel forms its dST), the padding columns of both are zeroed
    float* dS = a.dS + (long)h * B * Bp;
    float* dST = a.dST + (long)h * B * Bp;
    for (int r = wave; r < B; r += 16)
        for (int k = lane; k < Bp; k += 64) {
            const long e = (long)r * Bp + k;
            if (k < B) {
                const float x = X[0][e];
                const float g = 0.5f * (dsl_grad(st[0], B, x, k, r, n, temp) + dsl_grad(st[1], B, x, r, k, n, temp));
                dS[e] = g;
                dST[(long)k * Bp + r] = g;
            } else {
                dS[e] = 0.0f;
                dST[e] = 0.0f;
            }
        }
}

hipError_t launch_dsl_reduce(const float* S, float* ST, float* stat, float* dS, float* dST, float* loss_h, float* loss, int B, int Bp,
                             int H, float temp, hipStream_t st) {
    DslArgs a{S, ST, stat, dS, dST, loss_h, B, Bp, temp};
    hipLaunchKernelGGL(dsl_reduce_kernel, dim3(H), dim3(1024), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    return launch_loss_sum_heads(loss_h, H, loss, st);
}

}  // namespace laff
