// fc_strip16.hip -- fc_strip.hip's strip kernel (TransformNet.forward for K = 512 inputs: FC -> activation -> folded BatchNorm, X
// stationary in the accumulator registers, W streamed from a packed LDS image) on v_mfma_f32_16x16x32_f16 instead of
// v_mfma_f32_32x32x16_f16: the same flops in the same cycles, at less energy per flop -- the chip holds a higher clock on this shape
// (docs/experiments.md, "fc_strip on 16x16x32 MFMAs"; tools/probe/fcshapeprobe.hip).  Selected by LAFF_FC_STRIP_MFMA (api.hip).
//
// The decomposition is fc_strip.hip's (its header describes it): 4 wavefronts of 32 rows x K = 512 {hi, lo}, the 4 x 32 KiB ring + the
// staging buffer, 8 LDS-DMA pieces per wave and slot, 64 fragment reads per column block of 32 outputs, persistent ranges, the early
// rounds of the next strip, the accumulator-file guard, the three epilogue kinds, the image size and the [D][4] constant table.  What
// the two share as code is fc_strip_common.h; the kernel body is this file's own.  What differs is the fragment geometry:
//   * A (the strip): lane (i = lane & 15, g = lane >> 4) holds rows i and i + 16 of the wave's 32 (row tiles t = 0, 1).  K step J
//     (32 k), row tile t: a[16 J + 8 t .. + 3] = hi halves, a[16 J + 8 t + 4 .. + 7] = lo halves; element e <-> k = 32 J + 4 g +
//     (e & 3) + 16 (e >> 2), so that the four lanes of a row read adjacent 16-byte pieces of it.  One power-of-two scale per row,
//     i.e. two per lane;
//   * B (the W image): per ring slot {plane}{16 fragments = 8 K steps x 2 column tiles u}{64 lanes}{16 bytes}; MFMA column n of tile u
//     is output column 2 n + u of the block, the k order is A's;
//   * per K step twelve MFMAs of 16 cycles: for each product (Xlo.Whi, Xhi.Wlo, Xhi.Whi), column tile u, row tile t:
//     acc[t][u] += ... -- an accumulator comes up every fourth MFMA;
//   * a lane's 16 accumulators are 8 rows (16 t + 4 g + e) x 2 ADJACENT columns: the epilogue stores a dwordx2 per (t, e) -- 4 rows x
//     128 contiguous bytes per instruction, 8 stores per block -- and the lane constants are two 16-byte loads;
//   * the planner gives a 16-cycle MFMA slot at most 8 cycles of epilogue: one or two plain VALU, or one v_exp / v_rcp, or one store.
// An image is read in the geometry it was packed in: fc_strip_pack_kernel<16>'s images are not fc_strip_pack_kernel<32>'s.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fc_strip_common.h"
#include "wave_reduce.h"

namespace laff {

namespace {

using namespace fcs;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// acc (+)= A(strip fragment in a[R .. R + 3]: rows of X) x B(fragment of the W stream: output columns)
template <int R, bool FIRST>
__device__ __forceinline__ void mfma_strip(f32x4& acc, const u32x4& wfrag) {
    if constexpr (FIRST) asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c2:%c3], %1, 0" : "=v"(acc) : "v"(wfrag), "n"(R), "n"(R + 3));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c2:%c3], %1, %0" : "+v"(acc) : "v"(wfrag), "n"(R), "n"(R + 3));
}
// address = voff0 + ROWMUL * ldy4, made right in front of the store (one address register instead of one per accumulator pair)
template <int ROWMUL>
__device__ __forceinline__ void store_row(unsigned& tmp, f32x2 data, unsigned voff0, unsigned ldy4, u32x4 rsrc, unsigned soff) {
    asm volatile("v_mad_u32_u24 %0, %3, %4, %2\n\tbuffer_store_dwordx2 %1, %0, %5, %6 offen nt"
                 : "=&v"(tmp) : "v"(data), "v"(voff0), "s"(ldy4), "n"(ROWMUL), "s"(rsrc), "s"(soff) : "memory");
}

// The schedule of one column block (fc_strip_common.h): a fragment is F = 2 Jl + u (K step Jl of the slot, column tile u), six MFMAs
// behind it: slot sg = 96 H + 6 F + m.  (The MFMAs of a K step's two fragments interleave -- see body -- but the slot of everything
// else is counted per fragment.)  The epilogue's accumulator i = 8 t + 2 e + u is row 16 t + 4 g + e of the wave's 32, column 2 n + u
// of the block, its row scale rs[4 t + e], its lane constants cv[u]; one store (a dwordx2) per pair u = 0, 1.
constexpr Geometry GEOM = {.mfmas = 6, .skip_read_slots = true, .piece_m = 2, .piece_m2 = 4, .cv_loads = 2, .early = 6,
                           .slot_cycles = 8, .cost_valu = 4, .cost_trans = 8, .cost_store = 8};
constexpr int ST_STEP = 2;
constexpr int DRAIN_STORES = 16 / ST_STEP;            // OP_ST items of the stream: what a drain leaves in the vector-memory queue
static_assert(FD < NSETS - 1 && FD % 2 == 0 && BAR_J % 2 == 0, "the barrier sits in front of a K step, whose two fragments are read together");

}  // namespace

template <int ACTK>
__global__ __launch_bounds__(256, 1) void fc_strip16_kernel(const FcStripArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    AgprHold hold;
    agpr_hold_begin(hold);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n15 = lane & 15, g4 = lane >> 4;
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);

    const int nblk = pin_s(a.nblk), count = pin_s(a.count);
    const int nranges = pin_s(a.nranges);
    const long U = (long)pin_s((unsigned)a.total_units);
    const int myrange = a.range_of_wg[blockIdx.x];
    int u0 = pin_s((int)(U * myrange / nranges));              // (U < 2^31: launch_fc_strip)
    const int u1 = pin_s((int)(U * (myrange + 1) / nranges));
    const unsigned img_bytes = (unsigned)nblk * (2u * SLOT);

    constexpr EpiStream STREAM = make_stream<ACTK, ST_STEP>();
    constexpr Plan PLAN = make_plan(GEOM, STREAM);
    static_assert(PLAN.fits, "the epilogue stream does not fit behind the MFMAs of one column block");

    // per-lane constants of the loops
    unsigned lane16 = (unsigned)lane * 16u;
    asm volatile("" : "+v"(lane16));
    const unsigned xa0 = lds0 + lane16, xa1 = lds0 + lane16 + 2u * SLOT;      // fragment addresses: ring slots 0, 1 | 2, 3
    const unsigned wslot = (unsigned)wave * (PIECES * 1024u);                   // this wave's 8 KiB of a slot (LDS and source offset)
    const unsigned ldsw = pin_s(lds0 + wslot);                                  // LDS address of this wave's 8 KiB of ring slot 0
    const unsigned cvoff = (unsigned)n15 * 32u;                                 // the constants of columns 2 n, 2 n + 1: 32 bytes
    int pre_base = -1;           // >= 0: the previous segment's last three bodies brought rounds 0..2 of this segment's strip into buffers (e + pre_base) & 3
    const unsigned m0_keep = m0_get();
#ifdef LAFF_FCS_TRACE
    unsigned long long* const trc = a.trace ? a.trace + (size_t)blockIdx.x * 80 : nullptr;     // (LAFF_FCS_STAMP: fc_strip_common.h)
    int trc_seg = 0;
#endif

    while (u0 < u1) {
        // ---- the segment: column blocks [blk0, blk0 + n) of one strip of one problem --------------------------------------------------
        int p = 0;
        while (p + 1 < count && u0 >= a.p[p + 1].unit0) ++p;
        p = __builtin_amdgcn_readfirstlane(p);
        const int ul = u0 - a.p[p].unit0;
        const int strip = __builtin_amdgcn_readfirstlane(ul / nblk);
        const int blk0 = __builtin_amdgcn_readfirstlane(ul - strip * nblk);
        const int n = __builtin_amdgcn_readfirstlane(std::min(nblk - blk0, u1 - u0));
        u0 += n;
        LAFF_FCS_STAMP(0);
#ifdef LAFF_FCS_TRACE
        if (trc && tid == 0 && trc_seg < 8) trc[64 + trc_seg] = (unsigned long long)n;
#endif
        // The K-eighth ROUNDS the input rows travel in, and their swizzle, are fc_strip.hip's.  xoff(p, strip, xv): the per-lane source
        // offsets (rows beyond the matrix read the last row), relative to the strip's first row.
        auto xoff = [&](int p_, int strip_, unsigned (&xv)[8]) {
            const int N_ = a.p[p_].N, ldx_ = a.p[p_].ldx, r0_ = strip_ * FR;
            int ln = lane;
            asm volatile("" : "+v"(ln));              // made here: hipcc hoists lane-only terms out of the segment loop and keeps them all the way
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int rw = 4 * t + (ln >> 4);                       // row of the wave
                const int r = std::min(r0_ + wave * 32 + rw, N_ - 1) - r0_;
                xv[t] = (unsigned)r * (unsigned)ldx_ * 4u + ((((unsigned)ln & 15u) ^ ((unsigned)rw & 15u)) << 4);
            }
        };
        // the strip whose first three rounds this segment's last three bodies bring in: the next segment's (n >= 2: three bodies exist)
        const bool has_next = u0 < u1 && n >= 2;
        int p2 = p, strip2 = strip;
        if (has_next) {
            p2 = 0;
            while (p2 + 1 < count && u0 >= a.p[p2 + 1].unit0) ++p2;
            p2 = __builtin_amdgcn_readfirstlane(p2);
            strip2 = __builtin_amdgcn_readfirstlane((u0 - a.p[p2].unit0) / nblk);
        }
        unsigned xvn[8];
        xoff(p2, strip2, xvn);
#pragma unroll
        for (int t = 0; t < 8; ++t) asm volatile("" : "+v"(xvn[t]));
        const u32x4 rsrcXn = rebased_rsrc((unsigned long long)a.p[p2].X + (unsigned long long)(strip2 * FR) * (unsigned)a.p[p2].ldx * 4ull,
                                          (unsigned long long)FR * (unsigned)a.p[p2].ldx * 4ull, 0ull);
        const int N = pin_s(a.p[p].N), ldx = pin_s(a.p[p].ldx), ldy = pin_s(a.p[p].ldy);
        const unsigned long long pX = pin_s((unsigned long long)a.p[p].X), pW = pin_s((unsigned long long)a.p[p].img);
        const unsigned long long pVec = pin_s((unsigned long long)a.p[p].vec), pY = pin_s((unsigned long long)a.p[p].Y);
        const int row0 = strip * FR;

        f32x4 acc[2][2][2];              // [set][row tile t][column tile u]
        u32x4 fr[NSETS][2];
        float rs[8];
        f32x2 tt[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
        unsigned ta[4] = {0, 0, 0, 0};
        f32x4 cv[2][2] = {{{0, 0, 0, 0}, {0, 0, 0, 0}}, {{0, 0, 0, 0}, {0, 0, 0, 0}}};      // [set][column u]

        int e_row[2] = {0, 0};           // exponents of this lane's two row maxima: scale 2^(9 - e) in, 2^(e - 9) out
        // ---- the strip: this wave's 32 rows x 512 fp32 -> a[0:255] (raw), eight rounds through four wave-private buffers -- this wave's
        // 8 KiB of each (idle) ring slot; round e lives in buffer (e + base) & 3.  Rounds 0..2 are already there when the previous
        // segment's last bodies brought them (pre_base); up to four rounds are in flight.  The read-back (a round is two K steps jj; chunk
        // cc = 2 jj + t: lane (i, g) takes the 16-byte pieces 8 jj + g and 8 jj + 4 + g of row i + 16 t) folds the row maxima and parks
        // the raw values in the accumulator file.  Within each of ds_read_b128's four lane groups the sixteen lanes have sixteen
        // different i, and g only xors a constant into the swizzled position: sixteen different 16-byte columns, no bank conflict.
        {
            const unsigned long long xbase = pX + (unsigned long long)row0 * (unsigned)ldx * 4ull;
            unsigned xv[8];
            xoff(p, strip, xv);
            const bool pre = pre_base >= 0;
            const int base = pre ? pre_base : 0;
            unsigned XA[8];                            // read-back addresses inside a buffer: (cc, quad) -> row i + 16 t, piece 8 jj + 4 quad + g, swizzled
            {
                unsigned ln = (unsigned)lane;
                asm volatile("" : "+v"(ln));
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    XA[j] = ((ln & 15u) + 16u * (unsigned)((j >> 1) & 1)) * 256u + ((((unsigned)(8 * (j >> 2) + 4 * (j & 1)) + (ln >> 4)) ^ (ln & 15u)) << 4);
            }
            // round -> buffer.  Without early rounds: 0 1 2 3 X 0 1 2 (five in flight).  With them: rounds 0..2 sit in ring slots b0 b1 b2
            // (b_i = (i + base) & 3), round 3 in X, round 4 in b3 (the previous segment's last slot): b0 b1 b2 X b3 b0 b1 X -- round 7 follows
            // round 3, which landed long ago, not round 2, the last one to have been issued.
            auto buf_of = [&](int e) __attribute__((always_inline)) {
                const int ring = pre ? (e < 3 ? e : (e == 4 ? 3 : e - 5)) : (e < 4 ? e : e - 5);
                const bool x = pre ? (e == 3 || e == 7) : e == 4;
                return ldsw + (unsigned)(x ? RING : ((ring + base) & 3)) * (unsigned)SLOT;
            };
            auto issue_round = [&](auto EC) __attribute__((always_inline)) {
                constexpr int e = decltype(EC)::value;
                const unsigned long long ebase = xbase + (unsigned long long)(e * 256);
                const unsigned b = pin_s(buf_of(e));
                static_for<0, 8>([&](auto TC) __attribute__((always_inline)) {
                    constexpr int t = decltype(TC)::value;
                    dma_rows<t * 1024>(xv[t], ebase, b);
                });
            };
            float m0[2] = {0.f, 0.f}, m1[2] = {0.f, 0.f};   // running maxima of |x| over this lane's quarter of its two rows [t]
            u32x4 rq[8];
            auto read_round = [&](auto EC) __attribute__((always_inline)) {
                constexpr int e = decltype(EC)::value;
                const unsigned b = buf_of(e);
                static_for<0, 8>([&](auto JC) __attribute__((always_inline)) { constexpr int j = decltype(JC)::value; lds_read128<0>(rq[j], XA[j] + b); });
                wait_lgkm<0>();
                static_for<0, 8>([&](auto IC) __attribute__((always_inline)) { pin_v(rq[decltype(IC)::value]); });
            };
            auto stash_round = [&](auto EC) __attribute__((always_inline)) {
                constexpr int e = decltype(EC)::value;
                static_for<0, 4>([&](auto CC) __attribute__((always_inline)) {
                    constexpr int cc = decltype(CC)::value;
                    stash_chunk<8 * (4 * e + cc)>(rq[2 * cc], rq[2 * cc + 1], m0[cc & 1], m1[cc & 1]);
                });
            };
            using E0 = std::integral_constant<int, 0>; using E1 = std::integral_constant<int, 1>; using E2 = std::integral_constant<int, 2>;
            using E3 = std::integral_constant<int, 3>; using E4 = std::integral_constant<int, 4>; using E5 = std::integral_constant<int, 5>;
            using E6 = std::integral_constant<int, 6>; using E7 = std::integral_constant<int, 7>;
            if (!pre) {
                issue_round(E0{}); issue_round(E1{}); issue_round(E2{}); issue_round(E3{}); issue_round(E4{});
                wait_vm<32>(); read_round(E0{}); issue_round(E5{}); stash_round(E0{});
                wait_vm<32>(); read_round(E1{}); issue_round(E6{}); stash_round(E1{});
                wait_vm<32>(); read_round(E2{}); issue_round(E7{}); stash_round(E2{});
                wait_vm<32>(); read_round(E3{}); stash_round(E3{});
                wait_vm<24>(); read_round(E4{}); stash_round(E4{});
            } else {
                // The queue holds, oldest first: round 3 and round 0 (tail body 1), round 1 (body 2: 8 pieces, its stores, the two loads of the
                // lane constants), round 2 (body 3: 8 + its stores), round 4 (8, in front of the drain), the drain's stores.  The counts are lower bounds of what was
                // issued behind the round waited for.
                constexpr int DR = DRAIN_STORES, S1 = PLAN.st_half[1];       // (DR = the stores of bodies 2 and 3 together)
                wait_vm<(10 + 8 + DR) + 8 + DR>(); read_round(E0{}); issue_round(E5{}); stash_round(E0{});
                wait_vm<(8 + S1) + 8 + DR + 8>(); read_round(E1{}); issue_round(E6{}); stash_round(E1{});
                read_round(E3{}); issue_round(E7{}); stash_round(E3{});
                wait_vm<8 + DR + 24>(); read_round(E2{}); stash_round(E2{});
                wait_vm<24>(); read_round(E4{}); stash_round(E4{});
            }
            wait_vm<16>(); read_round(E5{}); stash_round(E5{});
            wait_vm<8>(); read_round(E6{}); stash_round(E6{});
            wait_vm<0>(); read_round(E7{}); stash_round(E7{});
#pragma unroll
            for (int t = 0; t < 2; ++t) {              // a row lives in lanes i, i + 16, i + 32, i + 48
                float m = fmaxf(m0[t], m1[t]);
                m = wave_step32<16>(m, [](float x, float y) { return fmaxf(x, y); });
                m = wave_step32<32>(m, [](float x, float y) { return fmaxf(x, y); });
                e_row[t] = split_exponent(m);
            }
            pre_base = has_next ? ((n & 1) ? 2 : 0) : -1;   // where this segment's last three bodies will leave the next strip's rounds 0..2
        }
        __builtin_amdgcn_s_barrier();            // every wave has emptied its staging quarter: the ring may fill
        asm volatile("" ::: "memory");
        LAFF_FCS_STAMP(1);

        // ---- W ring prologue: the segment's first three slots land while the strip is converted.  The image as a raw buffer starting at
        // this wave's 8 KiB of a slot ----
        const u32x4 rsrcW = rebased_rsrc(pW, img_bytes, wslot);
        unsigned soffW = (unsigned)blk0 * (2u * SLOT);                        // image offset of the slot the next pieces belong to
        ring_prologue(lane16, rsrcW, soffW, img_bytes, ldsw);

        // ---- the raw strip is converted in place ----
        LAFF_FCS_STAMP(2);
        {
            const float s0 = pow2f(9 - e_row[0]), s1 = pow2f(9 - e_row[1]);
            asm volatile("s_nop 1" ::: "memory");
            // chunk c = 2 J + t: hi <- a[8 c .. 8 c + 3], lo <- a[8 c + 4 .. 8 c + 7]; halves e = 0 .. 7 <-> raw registers 8 c + e
            static_for<0, 32>([&](auto GC) __attribute__((always_inline)) { convert_chunk_inplace<8 * decltype(GC)::value>((decltype(GC)::value & 1) ? s1 : s0); });
        }
        asm volatile("s_nop 3" ::: "memory");            // v_accvgpr_write -> MFMA reading it
        LAFF_FCS_STAMP(3);
        {
            // the epilogue's row scales: lane (n, g) needs those of rows 16 t + 4 g + e, which lane 4 g + e has for both t
            const float mine0 = pow2f(e_row[0] - 9), mine1 = pow2f(e_row[1] - 9);
#pragma unroll
            for (int i = 0; i < 8; ++i) rs[i] = __shfl((i >> 2) ? mine1 : mine0, 4 * g4 + (i & 3));
        }
        // output addressing: row 16 t + 4 g + e of the wave's 32, columns 2 n, 2 n + 1 of the block, at voff0 + (16 t + e) ldy4
        const unsigned ldy4 = (unsigned)ldy * 4u;
        unsigned voff0 = ((unsigned)(wave * 32 + 4 * g4) * (unsigned)ldy + 2u * (unsigned)n15) * 4u;
        // the output rows of this strip as a raw buffer: rows beyond N are dropped by its bounds check (voff carries the row)
        const u32x4 rsrcY = rebased_rsrc(pY + (unsigned long long)row0 * (unsigned)ldy * 4ull,
                                         ((unsigned long long)(std::min(FR, N - row0) - 1) * (unsigned)ldy + (unsigned)(nblk * 32)) * 4ull, 0ull);
        const u32x4 rsrcNone = {0u, 0u, 0u, 0x00020000u};
        // the lane constants {cs', b', c1, c0} of columns 32 blk + 2 n, + 1: [D][4] floats
        const u32x4 rsrcV = rebased_rsrc(pVec, (unsigned long long)nblk * 512ull, 0ull);

        // everything the prologue loaded is in registers by now: pin hipcc's own waits here, not inside the hand-counted loops
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(rs[i]));
        asm volatile("" : "+v"(voff0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        LAFF_FCS_STAMP(4);
        // fragments 0 .. FD - 1 of the first slot
        static_for<0, FD>([&](auto JC) __attribute__((always_inline)) {
            constexpr int j = decltype(JC)::value;
            lds_read128<j * 1024>(fr[j][0], xa0);
            lds_read128<PLANE + j * 1024>(fr[j][1], xa0);
        });

        // ---- one micro-op of the epilogue of block `blk - 1` (accumulator set Q, lane constants cv[Q]) --------------------------------
        u32x4 rsrcYe = rsrcNone;            // the first body's epilogue runs on nothing: an empty buffer drops its stores
        unsigned soffY = 0u;
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using IM1 = std::integral_constant<int, -1>;
        auto epi_item = [&](auto QC, auto IC, auto DRAIN) __attribute__((always_inline)) {
            constexpr int Q = decltype(QC)::value;
            constexpr EpiOp op = STREAM.op[decltype(IC)::value];
            constexpr int i = op.elem, u = i & 1, e = (i >> 1) & 3, t = i >> 3, k = (i >> 1) & 3;     // tt[k] = the pair (u = 0, 1)
            if constexpr (op.kind == OP_WAITCV) {
                // (drain: the lane constants were the block's first vector-memory operations: 16 pieces and the block's stores came behind
                // them -- a vmcnt(0) here would also wait for the next strip's rows the last bodies have just asked for; DRAIN counts
                // what else was issued)
                if constexpr (decltype(DRAIN)::value >= 0) wait_vm<16 + DRAIN_STORES + decltype(DRAIN)::value>(); else wait_vm<PLAN.vm_cv>();
                asm volatile("" : "+v"(cv[Q][0]), "+v"(cv[Q][1]));
            } else if constexpr (op.kind == OP_MUL) {
                asm volatile("v_mul_f32 %0, %1, %2" : "=v"(tt[k][u]) : "v"(acc[Q][t][u][e]), "v"(rs[4 * t + e]));
            } else if constexpr (op.kind == OP_FMA1) {
                asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(tt[k][u]) : "v"(cv[Q][u].x), "v"(cv[Q][u].y));
            } else if constexpr (op.kind == OP_EXP) {
                asm volatile("v_exp_f32 %0, %0" : "+v"(tt[k][u]));
            } else if constexpr (op.kind == OP_ADD1) {
                asm volatile("v_add_f32 %0, 1.0, %0" : "+v"(tt[k][u]));
            } else if constexpr (op.kind == OP_RCP) {
                asm volatile("v_rcp_f32 %0, %0" : "+v"(tt[k][u]));
            } else if constexpr (op.kind == OP_MAX) {
                asm volatile("v_max_f32 %0, 0, %0" : "+v"(tt[k][u]));
            } else if constexpr (op.kind == OP_FMA2) {
                asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(tt[k][u]) : "v"(cv[Q][u].z), "v"(cv[Q][u].w));
            } else if constexpr (op.kind == OP_ST) {
                store_row<16 * t + e>(ta[k], tt[k], voff0, ldy4, rsrcYe, soffY);
            }
        };

        // ---- one body: half a column block (ring slot 2 PAR + H), see "the schedule of one column block" --------------------------------
        auto body = [&](auto PARC, auto HC, auto XRC, int blk) __attribute__((always_inline)) {
            constexpr int PAR = decltype(PARC)::value, H = decltype(HC)::value, Q = PAR ^ 1;
            constexpr int XR = decltype(XRC)::value;                 // >= 0: the pieces carry round XR of the next strip's rows, not the W stream
            constexpr int RSLOT = 2 * PAR + H;                                   // this body's ring slot
            constexpr int NSLOT_R = (RSLOT + 1) & 3;                             // the next body's
            constexpr int DSLOT = (RSLOT + 3) & 3;                               // the slot refilled here: the previous body's
            const unsigned soff_here = std::min(soffW, img_bytes - SLOT);
            soffW += SLOT;
            if constexpr (H == 0) soffY = (unsigned)(blk - 1) * 128u;
            static_for<0, 16>([&](auto FC) __attribute__((always_inline)) {
                constexpr int F = decltype(FC)::value;                           // fragment of the slot: K step Jl = F >> 1, column tile F & 1
                constexpr int G = 16 * H + F;                                    // fragment of the block: register set G % NSETS
                if constexpr (F == BAR_J) {
                    // (the segment's last body has no next slot to wait for: what is in flight is the next strip's)
                    if constexpr (XR != 2) wait_vm<PLAN.vm_bar[H]>();
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                }
                if constexpr (F % 2 == 0) wait_lgkm<2 * (FD - 2)>();             // the four fragments of this K step have arrived
                __builtin_amdgcn_sched_barrier(0);
                static_for<0, 6>([&](auto MC) __attribute__((always_inline)) {
                    constexpr int m = decltype(MC)::value, SG = 96 * H + 6 * F + m;
                    // the twelve MFMAs of a K step: product by product -- lo.hi, hi.lo (small terms first), hi.hi -- over the four
                    // accumulators (column tile, row tile): an accumulator comes up every fourth MFMA
                    constexpr int s12 = SG % 12, JG = SG / 12, M = s12 / 4, u = (s12 % 4) / 2, t = s12 & 1;
                    constexpr int R = 16 * JG + 8 * t, GS = (2 * JG + u) % NSETS;
                    if constexpr (M == 0) mfma_strip<R + 4, (JG == 0)>(acc[PAR][t][u], fr[GS][0]);
                    else if constexpr (M == 1) mfma_strip<R, false>(acc[PAR][t][u], fr[GS][1]);
                    else mfma_strip<R, false>(acc[PAR][t][u], fr[GS][0]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (m == 0) {
                        // the fragment FD ahead (this slot, or the next one behind the barrier)
                        constexpr int FN = F + FD;
                        constexpr int RS = FN < 16 ? RSLOT : NSLOT_R, FF = FN & 15, GN = (G + FD) % NSETS;
                        constexpr int OFFS = (RS & 1) * SLOT + FF * 1024;
                        if constexpr (RS < 2) {
                            lds_read128<OFFS>(fr[GN][0], xa0);
                            lds_read128<OFFS + PLANE>(fr[GN][1], xa0);
                        } else {
                            lds_read128<OFFS>(fr[GN][0], xa1);
                            lds_read128<OFFS + PLANE>(fr[GN][1], xa1);
                        }
                    }
                    if constexpr (slot_cvload(SG)) {
                        // this block's lane constants (used by its epilogue, in the next block's bodies or in the drain)
                        const unsigned so = (unsigned)blk * 512u;
                        asm volatile("buffer_load_dwordx4 %0, %2, %3, %4 offen\n\tbuffer_load_dwordx4 %1, %2, %3, %4 offen offset:16"
                                     : "=&v"(cv[PAR][0]), "=&v"(cv[PAR][1]) : "v"(cvoff), "s"(rsrcV), "s"(so) : "memory");
                    }
                    if constexpr (XR == 0 && m == 2 && F < 8) {
                        // round 3 of the next strip, to the staging-only buffer (no ring slot: no barrier to respect)
                        dma_piece<XB_OFF + F * 1024>(xvn[F], rsrcXn, 3u * 256u, ldsw);
                    }
                    constexpr int dp = slot_piece(GEOM, SG);
                    if constexpr (dp >= 0) {
                        // the W stream's piece dp of the slot three ahead -- or, in the segment's last three bodies, instruction dp of round
                        // XR of the next strip's rows; same LDS target either way
                        if constexpr (XR >= 0) dma_piece<DSLOT * SLOT + dp * 1024>(xvn[dp], rsrcXn, (unsigned)(256 * XR), ldsw);
                        else dma_piece<DSLOT * SLOT + dp * 1024>(lane16 + (unsigned)(dp * 1024), rsrcW, soff_here, ldsw);
                    }
                    static_for<PLAN.begin[SG], PLAN.begin[SG + 1]>([&](auto IC) __attribute__((always_inline)) {
                        __builtin_amdgcn_sched_barrier(0);
                        epi_item(std::integral_constant<int, Q>{}, IC, IM1{});
                    });
                    __builtin_amdgcn_sched_barrier(0);
                });
            });
        };

        auto drain = [&](auto QC, auto EXTRA, int blk) __attribute__((always_inline)) {
            LAFF_FCS_STAMP(5);
            mfma_drain_nops();
            rsrcYe = rsrcY;
            soffY = (unsigned)blk * 128u;
            static_for<0, STREAM.n>([&](auto IC) __attribute__((always_inline)) { epi_item(QC, IC, EXTRA); });
        };
        // The segment's blocks: a plain loop, then -- when a next segment exists -- its last two blocks as the copies whose last three bodies
        // fetch the next strip's first three rounds (compile-time copies: the plain loop keeps its one branch per two blocks).
        auto plain = [&](auto PARC, int b) __attribute__((always_inline)) {
            body(PARC, I0{}, IM1{}, blk0 + b);
            body(PARC, I1{}, IM1{}, blk0 + b);
        };
        auto tail = [&](auto PARC, int b) __attribute__((always_inline)) {
            constexpr int P = decltype(PARC)::value;
            body(PARC, I0{}, IM1{}, blk0 + b);
            body(PARC, I1{}, I0{}, blk0 + b);
            rsrcYe = rsrcY;
            body(std::integral_constant<int, P ^ 1>{}, I0{}, I1{}, blk0 + b + 1);
            body(std::integral_constant<int, P ^ 1>{}, I1{}, I2{}, blk0 + b + 1);
            // Every wave is done with the ring (the segment's barrier, taken here instead of behind the drain): round 4 goes to the last
            // body's slot and flies while the drain computes.
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            static_for<0, 8>([&](auto TC) __attribute__((always_inline)) {
                constexpr int t = decltype(TC)::value;
                dma_piece<(2 * (P ^ 1) + 1) * SLOT + t * 1024>(xvn[t], rsrcXn, 4u * 256u, ldsw);
            });
            drain(std::integral_constant<int, P ^ 1>{}, std::integral_constant<int, 8>{}, blk0 + b + 1);
        };
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[1][0][0][e] = acc[1][0][1][e] = acc[1][1][0][e] = acc[1][1][1][e] = 0.0f;
        {
            const int m = has_next ? n - 2 : n;          // blocks of the plain loop
            int b = 0, par = 0;                          // par: parity of the block behind the plain loop
            if (m > 0) {
#pragma nounroll
                for (;;) {
                    plain(I0{}, b);
                    rsrcYe = rsrcY;
                    if (++b >= m) { par = 1; break; }
                    plain(I1{}, b);
                    if (++b >= m) { par = 0; break; }
                }
            }
            if (has_next) {
                if (par == 0) tail(I0{}, b); else tail(I1{}, b);
            } else {
                if (par == 1) drain(I0{}, I0{}, blk0 + b - 1); else drain(I1{}, I0{}, blk0 + b - 1);
            }
        }
        // segment end: nothing of this wave may still be in flight towards the fragment registers; vector memory is NOT drained (fc_strip.hip)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int s8 = 0; s8 < NSETS; ++s8) asm volatile("" ::"v"(fr[s8][0]), "v"(fr[s8][1]));
        if (!has_next) __builtin_amdgcn_s_barrier();   // every wave is done with the ring before the next segment's strip staging refills it
        LAFF_FCS_STAMP(6);
#ifdef LAFF_FCS_TRACE
        ++trc_seg;
#endif
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // no LDS-DMA of this workgroup outlives it
    m0_set(m0_keep);
    agpr_hold_end(hold);
}

// (called by launch_fc_strip, fc_strip.hip, which has set up the units and ranges of a)
hipError_t fc_strip16_launch(const FcStripArgs& a, int kind, hipStream_t st) {
    if (kind == ACT_EXP) return fc_strip_launch<fc_strip16_kernel<ACT_EXP>>(a, st);
    if (kind == ACT_RELU) return fc_strip_launch<fc_strip16_kernel<ACT_RELU>>(a, st);
    return fc_strip_launch<fc_strip16_kernel<ACT_LIN>>(a, st);
}

}  // namespace laff
