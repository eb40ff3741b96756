// laff_batch_assemble: a training batch gathered from the resident training set in ONE launch.
//
// The launch runs a table of up to ASSEMBLE_JOBS copy jobs; the table travels in the launch arguments.  Every per-batch integer (the
// source row of every batch row, the destination offsets of the CSR rows) sits in one int32 control block that the host uploaded
// once.  Job j owns the blocks [first_block, first_block + blocks) of the grid and strides over its own items with them:
//   rows    dst[b, 0:w] = src[row[b], 0:w]
//   ragged  dst[b, f, 0:w] = src[seg_off[seg[b]] + f, 0:w] for f < len(seg[b]), zeros up to fmax; mask[b, f] = 1 / 0
//   CSR     col_dst / val_dst [crow_dst[b] ...) = the entries of source row row[b]
// These are copies of few bytes (3 MB at the LAFF shape), so the cost is the launch itself: one kernel, plain global loads and stores,
// 16 bytes per lane where the job's bases, pitches and width allow it (`vec`, decided on the host per job), 4 bytes otherwise.  Every
// destination element is written exactly once by exactly one lane: no atomics, two calls give the same bits.  Source addresses are
// formed in 64 bits; every index read from device memory is checked against the source's size before it is used, so a stale control
// block or offset array cannot make the kernel read or write outside its buffers (the affected rows are zeros).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace laff {

namespace {

constexpr int THREADS = ASSEMBLE_THREADS;

// the items [i0, i0 + stride, ...) below n of this job, over the job's own blocks
struct Span {
    unsigned i, n, stride;
};
__device__ __forceinline__ Span span_of(const AssembleJob& j, unsigned n) {
    return Span{(blockIdx.x - (unsigned)j.first_block) * THREADS + threadIdx.x, n, (unsigned)j.blocks * THREADS};
}

// one 16-byte chunk (VEC) or one element of a row: the tail of a row whose width is no multiple of 4 is copied by elements
template <bool VEC>
__device__ __forceinline__ void copy_piece(const unsigned* __restrict__ s, unsigned* __restrict__ d, int c, int w, bool zero) {
    if (VEC) {
        const int e0 = 4 * c;
        if (e0 + 4 <= w) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (!zero) v = *reinterpret_cast<const uint4*>(s + e0);
            *reinterpret_cast<uint4*>(d + e0) = v;
        } else {
            for (int e = e0; e < w; ++e) d[e] = zero ? 0u : s[e];
        }
    } else {
        d[c] = zero ? 0u : s[c];
    }
}

template <bool VEC>
__device__ __forceinline__ void rows_job(const AssembleJob& j, const int* __restrict__ control, int B) {
    const unsigned pieces = VEC ? (unsigned)(j.w + 3) / 4 : (unsigned)j.w;
    const int* __restrict__ row = control + j.rows_at;
    for (Span s = span_of(j, (unsigned)B * pieces); s.i < s.n; s.i += s.stride) {
        const unsigned b = s.i / pieces, c = s.i - b * pieces;
        const int r = row[b];
        const bool bad = (unsigned)r >= (unsigned)j.n_src;
        copy_piece<VEC>((const unsigned*)j.src + (size_t)(bad ? 0 : r) * j.ld_src, (unsigned*)j.dst + (size_t)b * j.ld_dst, (int)c, j.w, bad);
    }
}

template <bool VEC>
__device__ __forceinline__ void ragged_job(const AssembleJob& j, const int* __restrict__ control, int B) {
    const unsigned pieces = VEC ? (unsigned)(j.w + 3) / 4 : (unsigned)j.w;
    const int* __restrict__ seg = control + j.rows_at;
    const unsigned per_b = (unsigned)j.fmax * pieces;
    for (Span s = span_of(j, (unsigned)B * per_b); s.i < s.n; s.i += s.stride) {
        const unsigned b = s.i / per_b, rest = s.i - b * per_b;
        const unsigned f = rest / pieces, c = rest - f * pieces;
        const int g = seg[b];
        long long first = 0;
        int len = 0;
        if ((unsigned)g < (unsigned)j.n_src) {
            first = j.off_src[g];
            const long long end = j.off_src[g + 1];
            if (first >= 0 && end >= first && end <= (long long)j.n_items) len = (int)min(end - first, (long long)j.fmax);
        }
        const bool pad = (int)f >= len;                                   // a padded row is never read from the source
        copy_piece<VEC>((const unsigned*)j.src + (size_t)(pad ? 0 : first + f) * j.ld_src, (unsigned*)j.dst + ((size_t)b * j.fmax + f) * j.w,
                        (int)c, j.w, pad);
        if (j.mask && c == 0) j.mask[(size_t)b * j.fmax + f] = pad ? 0.0f : 1.0f;
    }
}

// 64 lanes a batch row: the entries of a caption's row are few
__device__ __forceinline__ void csr_job(const AssembleJob& j, const int* __restrict__ control, int B) {
    const int* __restrict__ row = control + j.rows_at;
    const int* __restrict__ crow_dst = control + j.crow_at;
    const unsigned lane = threadIdx.x & 63u, groups = THREADS / 64;
    for (unsigned b = (blockIdx.x - (unsigned)j.first_block) * groups + threadIdx.x / 64; b < (unsigned)B; b += (unsigned)j.blocks * groups) {
        const int r = row[b], d0 = crow_dst[b], dn = crow_dst[b + 1] - d0;
        long long s0 = 0;
        int sn = 0;
        if ((unsigned)r < (unsigned)j.n_src) {
            s0 = j.off_src[r];
            const long long end = j.off_src[r + 1];
            if (s0 >= 0 && end >= s0 && end <= (long long)j.n_items) sn = (int)min(end - s0, (long long)dn);
        }
        for (int e = (int)lane; e < dn; e += 64) {                       // entries the source row does not have are written as zeros
            j.col_dst[d0 + e] = e < sn ? j.col_src[s0 + e] : 0;
            ((unsigned*)j.dst)[d0 + e] = e < sn ? ((const unsigned*)j.src)[s0 + e] : 0u;
        }
    }
}

__global__ __launch_bounds__(THREADS) void batch_assemble_kernel(const AssembleTable t) {
    int ji = 0;
    while (ji + 1 < t.count && (int)blockIdx.x >= t.j[ji + 1].first_block) ++ji;
    const AssembleJob& j = t.j[ji];
    if (j.kind == LAFF_ASSEMBLE_ROWS) {
        if (j.vec) rows_job<true>(j, t.control, t.B);
        else rows_job<false>(j, t.control, t.B);
    } else if (j.kind == LAFF_ASSEMBLE_RAGGED) {
        if (j.vec) ragged_job<true>(j, t.control, t.B);
        else ragged_job<false>(j, t.control, t.B);
    } else {
        csr_job(j, t.control, t.B);
    }
}

}  // namespace

static_assert(sizeof(AssembleTable) + 256 <= 4096, "the table and the implicit arguments must fit 4 KiB of launch arguments");

// items of a job as its kernel counts them (at most 2^31 - 1: checked by the caller)
long long assemble_items(const AssembleJob& j, int B) {
    if (j.kind == LAFF_ASSEMBLE_CSR) return (long long)B * 64;
    const long long pieces = j.vec ? (j.w + 3) / 4 : j.w;
    return (long long)B * pieces * (j.kind == LAFF_ASSEMBLE_RAGGED ? j.fmax : 1);
}

hipError_t launch_batch_assemble(AssembleTable& t, hipStream_t st) {
    int grid = 0;
    for (int i = 0; i < t.count; ++i) {
        AssembleJob& j = t.j[i];
        const long long per_block = (long long)THREADS * ASSEMBLE_ITEMS_PER_THREAD;
        long long blocks = (assemble_items(j, t.B) + per_block - 1) / per_block;
        j.blocks = (int)(blocks < 1 ? 1 : blocks > ASSEMBLE_BLOCK_CAP ? ASSEMBLE_BLOCK_CAP : blocks);
        j.first_block = grid;
        grid += j.blocks;
    }
    hipLaunchKernelGGL(batch_assemble_kernel, dim3(grid), dim3(THREADS), 0, st, t);
    return hipGetLastError();
}

}  // namespace laff
