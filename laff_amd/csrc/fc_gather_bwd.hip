// fc_gather_bwd.hip -- backward of the FC projection A = act(X W^T + bias) of a SPARSE X [N, Dk] for gfx950, fp32:
// laff_fc_gather_backward.
//
//   dZ = dA (.) act'(A)      tanh: 1 - A^2    sigmoid: A (1 - A)    relu: A > 0    none: 1       (A is the SAVED forward output)
//   dW[d, v] = sum over the entries (n, v) of X of x[n, v] dZ[n, d]        db[d] = sum_n dZ[n, d]        (no dX: counts)
//
// X comes in transposed (CSC): column v owns the entries [colptr[v], colptr[v + 1]) of rows / values, in ascending row order.  The work
// is writing dW [D, Dk] once -- 82 MB at 2048 x 10,000 against a few thousand entries -- so this is a store kernel:
//
//   * a block of four wavefronts owns TV = 64 consecutive vocabulary columns x TD = 128 rows d of dW;
//   * a tile without entries (colptr[v0 + TV] == colptr[v0], a block-uniform test) stores zeros at once;
//   * otherwise each wavefront walks the segments of its share of the columns (a quarter of the tile's entries) with the lanes along d (lane l owns d0 + 2 l and d0 + 2 l + 1: a load
//     of A or dA is 512 contiguous bytes), UNR entries in flight, one fmaf chain per element in entry order; the sums go to LDS as
//     [TV][TD + 1] and are written out transposed, the lanes along v: a store instruction covers 256 contiguous bytes of a dW row.
//   * the 16-byte store variant (dW's base and pitch 16-byte aligned, Dk % 4 == 0) and the single-float one are two kernels; they
//     differ in the stores only, so their bits are equal;
//   * db: D / 32 further blocks of the same launch, each 32 columns of dZ summed over the rows by sum_rows_fixed_order_of.
//
// No atomics, and the order of every sum is fixed by the pattern (dW) or by N (db) alone: two calls give the same bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "attn_common.h"
#include "fc_bwd_common.h"
#include "kernels.h"

namespace laff {

namespace {

constexpr int TV = 64, TD = 128, THREADS = 256, WAVES = THREADS / 64, PITCH = TD + 1, UNR = 8, DB_COLS = 4 * DW_LANES;

__device__ __forceinline__ int lane_value(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// A wavefront's share of the tile whose rows start at d0: column sums into tile[column][d - d0], lane l owning d0 + 2 l and
// d0 + 2 l + 1 (8-byte loads; D % 4 == 0, so the pair is inside or outside).  Lane c holds the segment of the
// tile's column c in cpa (start) and cpb (end), clamped to [0, nnz]: whatever colptr holds, nothing outside rows / values is read.
// The tile's entries [tbeg, tend] are cut into four equal pieces and a column belongs to the wavefront whose piece holds its start:
// word frequencies follow a 1 / rank law, and with 16 fixed columns each one wavefront walked a third of a batch's entries while
// three waited.  No step waits for memory per column: the segments come out of cpa / cpb by v_readlane, and the entries' row indices
// and values are held 64 at a time in rj / xj, one entry per lane, and come out the same way -- so every branch is wave-uniform, a
// column without entries costs a few scalar instructions, and the loads of A and dA of UNR entries fly together.
template <int ACT>
__device__ __forceinline__ void walk_columns(const FcGatherBwdArgs& a, int cpa, int cpb, int d0, int wave, int lane, float (*tile)[PITCH]) {
    const int dd = d0 + 2 * lane < a.D ? d0 + 2 * lane : 0;                 // a lane past D reads column 0; its sums are not stored
    const int tbeg = lane_value(cpa, 0), tend = lane_value(cpb, TV - 1);
    const long long len = (long long)tend - tbeg;
    const int lo = tbeg + (int)(len * wave / WAVES), hi = wave == WAVES - 1 ? tend + 1 : tbeg + (int)(len * (wave + 1) / WAVES);
    int cb = lo, rj;                                                        // rj, xj: the entries [cb, cb + 64)
    float xj;
    auto load_entries = [&]() {
        const int j = min(cb + lane, a.nnz - 1);                            // nnz >= 1: the tile is not empty
        rj = a.rows[j];
        xj = a.values ? a.values[j] : 1.0f;
    };
    load_entries();
    for (int c = 0; c < TV; ++c) {
        const int beg = lane_value(cpa, c), end = lane_value(cpb, c);
        if (beg < lo || beg >= hi) continue;                                // another wavefront's column
        float acc0 = 0.f, acc1 = 0.f;
        for (int j0 = beg; j0 < end; j0 += UNR) {
            if (j0 < cb || j0 + UNR > cb + 64) {
                cb = j0;
                load_entries();
            }
            // UNR entries at once: their rows of A and dA are loaded before the first fmaf, which then run in entry order.  Straight
            // line: an entry that does not count (past the segment's end, or a row outside [0, N)) loads row 0 and is dropped by a
            // select -- with a branch around a load, where the two paths meet hipcc waits for the load, one entry at a time.
            float2 s[UNR], g[UNR];
            float x[UNR];
            bool ok[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int n = lane_value(rj, j0 + u - cb);
                x[u] = lane_value(xj, j0 + u - cb);
                ok[u] = j0 + u < end && (unsigned)n < (unsigned)a.N;
                const size_t r = ok[u] ? (size_t)n : 0;                     // N >= 1 here
                s[u] = *(const float2*)(a.A + r * a.lda + dd);
                g[u] = *(const float2*)(a.dA + r * a.ldda + dd);
            }
            __builtin_amdgcn_sched_barrier(0);                              // hipcc otherwise sinks each pair of loads to its fmaf
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const float t0 = fmaf(x[u], dact<ACT>(s[u].x, g[u].x), acc0), t1 = fmaf(x[u], dact<ACT>(s[u].y, g[u].y), acc1);
                acc0 = ok[u] ? t0 : acc0;
                acc1 = ok[u] ? t1 : acc1;
            }
        }
        tile[c][2 * lane] = acc0;
        tile[c][2 * lane + 1] = acc1;
    }
}

// 32 columns of db by one block: dZ's rows are formed on the way and added in the fixed order of sum_rows_fixed_order_of
template <int ACT>
__device__ __forceinline__ float4 db_columns(const FcGatherBwdArgs& a, int col, bool valid, float4 (&sh)[DW_GROUPS][DW_LANES]) {
    return sum_rows_fixed_order_of(
        [&](int r) {
            const float4 s = *(const float4*)(a.A + (size_t)r * a.lda + col), g = *(const float4*)(a.dA + (size_t)r * a.ldda + col);
            return make_float4(dact<ACT>(s.x, g.x), dact<ACT>(s.y, g.y), dact<ACT>(s.z, g.z), dact<ACT>(s.w, g.w));
        },
        valid ? a.N : 0, sh);
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void fc_gather_bwd_kernel(FcGatherBwdArgs a) {
    __shared__ float tile[TV][PITCH];
    __shared__ float4 sh[DW_GROUPS][DW_LANES];
    const int lane = threadIdx.x & 63, wave = pinned(threadIdx.x >> 6);
    const int tiles = a.dW ? ((a.Dk + TV - 1) / TV) * ((a.D + TD - 1) / TD) : 0;

    if ((int)blockIdx.x >= tiles) {                                         // db
        const int col = ((int)blockIdx.x - tiles) * DB_COLS + 4 * (threadIdx.x & (DW_LANES - 1));
        const bool valid = col < a.D;                                       // D % 4 == 0: a lane's four columns are inside or outside
        float4 t;
        switch (a.act) {
            case LAFF_ACT_TANH: t = db_columns<LAFF_ACT_TANH>(a, col, valid, sh); break;
            case LAFF_ACT_SIGMOID: t = db_columns<LAFF_ACT_SIGMOID>(a, col, valid, sh); break;
            case LAFF_ACT_RELU: t = db_columns<LAFF_ACT_RELU>(a, col, valid, sh); break;
            default: t = db_columns<LAFF_ACT_NONE>(a, col, valid, sh); break;
        }
        if (threadIdx.x < DW_LANES && valid) {                              // db's base is 4-byte aligned only
            a.db[col] = t.x;
            a.db[col + 1] = t.y;
            a.db[col + 2] = t.z;
            a.db[col + 3] = t.w;
        }
        return;
    }

    // the rows d vary fastest over the blocks: the tiles of the first vocabulary columns, the frequent words of a vocabulary sorted by
    // count and so the longest walks, start first
    const int tiles_d = (a.D + TD - 1) / TD, v0 = ((int)blockIdx.x / tiles_d) * TV, d0 = ((int)blockIdx.x % tiles_d) * TD;
    // one pair of loads per wavefront brings the 64 segments; the tile is empty when its first start equals its last end
    int cpa = 0, cpb = 0;
    if (a.nnz > 0) {
        cpa = min(max(a.colptr[min(v0 + lane, a.Dk)], 0), a.nnz);
        cpb = min(max(a.colptr[min(v0 + lane + 1, a.Dk)], 0), a.nnz);
    }
    const bool empty = lane_value(cpa, 0) == lane_value(cpb, TV - 1);       // the same in the four wavefronts
    if (!empty) {
        switch (a.act) {
            case LAFF_ACT_TANH: walk_columns<LAFF_ACT_TANH>(a, cpa, cpb, d0, wave, lane, tile); break;
            case LAFF_ACT_SIGMOID: walk_columns<LAFF_ACT_SIGMOID>(a, cpa, cpb, d0, wave, lane, tile); break;
            case LAFF_ACT_RELU: walk_columns<LAFF_ACT_RELU>(a, cpa, cpb, d0, wave, lane, tile); break;
            default: walk_columns<LAFF_ACT_NONE>(a, cpa, cpb, d0, wave, lane, tile); break;
        }
        __syncthreads();
    }

    // the tile transposed, the lanes along v; wavefront w stores the rows d0 + [32 w, 32 w + 32)
    if constexpr (VEC) {
        const int vl = 4 * (lane & 15), v = v0 + vl;                        // Dk % 4 == 0: four columns are inside or outside
#pragma unroll 4
        for (int i = 0; i < TD / WAVES / 4; ++i) {
            const int dl = wave * (TD / WAVES) + 4 * i + (lane >> 4), d = d0 + dl;
            if (d < a.D && v < a.Dk) {
                const float4 t = empty ? zero4() : make_float4(tile[vl][dl], tile[vl + 1][dl], tile[vl + 2][dl], tile[vl + 3][dl]);
                *(float4*)(a.dW + (size_t)d * a.lddw + v) = t;
            }
        }
    } else {
        const int v = v0 + lane;
#pragma unroll 4
        for (int i = 0; i < TD / WAVES; ++i) {
            const int dl = wave * (TD / WAVES) + i, d = d0 + dl;
            if (d < a.D && v < a.Dk) a.dW[(size_t)d * a.lddw + v] = empty ? 0.f : tile[lane][dl];
        }
    }
}

}  // namespace

hipError_t launch_fc_gather_backward(const FcGatherBwdArgs& a, hipStream_t st) {
    const long long tiles = a.dW ? (long long)((a.Dk + TV - 1) / TV) * ((a.D + TD - 1) / TD) : 0;
    const long long blocks = tiles + (a.db ? (a.D + DB_COLS - 1) / DB_COLS : 0);
    if (blocks == 0) return hipSuccess;
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    const bool vec = a.dW && (reinterpret_cast<uintptr_t>(a.dW) & 15) == 0 && a.lddw % 4 == 0 && a.Dk % 4 == 0;
    if (vec) hipLaunchKernelGGL(fc_gather_bwd_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL(fc_gather_bwd_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace laff
