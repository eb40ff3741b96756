// fc_strip_common.h -- what the two MFMA shapes of the FC strip kernel share (fc_strip.hip: v_mfma_f32_32x32x16_f16, fc_strip16.hip:
// v_mfma_f32_16x16x32_f16): the LDS ring, the accumulator-file guard, the asm wrappers, the input split, the epilogue as a static
// stream of micro-ops, the planner that places that stream behind the MFMAs, the W ring prologue, the pack kernel and the launch of
// one kernel instance.  A shape's file keeps its header comment, mfma_strip, store_row, its Geometry and the kernel; fc_strip.hip
// also has the host path of both.  Internal to those two files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "strip_util.h"

namespace laff {
namespace fcs {

using namespace su;

constexpr int FR = FC_STRIP_ROWS;              // 128 rows per strip: 4 wavefronts x 32
constexpr int SLOT = 32 * 1024;                // one ring slot: 32 columns x 256 k x {hi, lo}
constexpr int PLANE = 16 * 1024;
constexpr int RING = 4;
constexpr int PIECES = 8;                      // 1 KiB LDS-DMA pieces per wave per slot
constexpr int XB_OFF = RING * SLOT;            // a fifth 32 KiB buffer, strip staging only (all of the CU's LDS: 160 KiB)
constexpr int SMEM = XB_OFF + SLOT;
static_assert(SMEM <= 160 * 1024, "LDS budget");

// A FRAGMENT is one 1 KiB read per plane: 32x32x16: a sub-step (16 k) of the block's 32 columns; 16x16x32: a K step (32 k) of one of
// the block's two column tiles.  32 fragments per column block, 16 per ring slot, in either shape.
constexpr int FD = 6;                          // fragment reads run FD fragments ahead,
constexpr int NSETS = 8;                       // into 8 register sets (two planes each; 32 fragments per block: a divisor of 32)
static_assert(32 % NSETS == 0 && FD < NSETS, "the set of a fragment must not depend on the block");
constexpr int BAR_J = 16 - FD;                 // the body's barrier sits in front of this fragment

// ---- all 256 accumulator registers are named literally (the strip).  hipcc must not put anything of its own there (left alone it parks
// long-lived values in a0.. when the 256 architectural registers get tight -- silently overwritten by the strip): 64 dummy quads are
// defined in the accumulator file at kernel entry and "used" at its exit, so the allocator sees every one of them occupied throughout;
// if registers run out it spills to scratch instead, which tools/debug/isa_audit.py reports. ----
struct AgprHold { u32x4 q[64]; };
#define HOLD16(OP, h, b)                                                                                                                  \
    OP(h.q[b], h.q[b + 1], h.q[b + 2], h.q[b + 3], h.q[b + 4], h.q[b + 5], h.q[b + 6], h.q[b + 7], h.q[b + 8], h.q[b + 9], h.q[b + 10], h.q[b + 11], \
       h.q[b + 12], h.q[b + 13], h.q[b + 14], h.q[b + 15])
#define HOLD_DEF(x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, xa, xb, xc, xd, xe, xf)                                                            \
    asm volatile("" : "=a"(x0), "=a"(x1), "=a"(x2), "=a"(x3), "=a"(x4), "=a"(x5), "=a"(x6), "=a"(x7), "=a"(x8), "=a"(x9), "=a"(xa), "=a"(xb), \
                 "=a"(xc), "=a"(xd), "=a"(xe), "=a"(xf))
#define HOLD_USE(x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, xa, xb, xc, xd, xe, xf)                                                            \
    asm volatile("" ::"a"(x0), "a"(x1), "a"(x2), "a"(x3), "a"(x4), "a"(x5), "a"(x6), "a"(x7), "a"(x8), "a"(x9), "a"(xa), "a"(xb), "a"(xc),   \
                 "a"(xd), "a"(xe), "a"(xf))
__device__ __forceinline__ void agpr_hold_begin(AgprHold& h) { HOLD16(HOLD_DEF, h, 0); HOLD16(HOLD_DEF, h, 16); HOLD16(HOLD_DEF, h, 32); HOLD16(HOLD_DEF, h, 48); }
__device__ __forceinline__ void agpr_hold_end(AgprHold& h) { HOLD16(HOLD_USE, h, 0); HOLD16(HOLD_USE, h, 16); HOLD16(HOLD_USE, h, 32); HOLD16(HOLD_USE, h, 48); }

template <int R, int OFF>
__device__ __forceinline__ void agpr_load4(const void* p) {            // a[R .. R + 3] <- 16 bytes at p + OFF
    asm volatile("global_load_dwordx4 a[%c1:%c2], %0, off offset:%c3" ::"v"(p), "n"(R), "n"(R + 3), "n"(OFF) : "memory");
}
template <int R>
__device__ __forceinline__ float agpr_read() {
    float x;
    asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(x) : "n"(R));
    return x;
}
template <int R>
__device__ __forceinline__ void agpr_write(unsigned x) { asm volatile("v_accvgpr_write_b32 a[%c1], %0" ::"v"(x), "n"(R)); }

template <int IMM>
__device__ __forceinline__ void lds_read128(u32x4& d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(IMM));
}

// one 1 KiB piece of the W stream, straight into LDS (lane L lands at M0 base + 16 L; the image is already in LDS order)
template <int LDSOFF>
__device__ __forceinline__ void dma_piece(unsigned voff, u32x4 rsrc, unsigned soff, unsigned m0base) {
    asm volatile("s_add_i32 m0, %3, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds"
                 ::"v"(voff), "s"(rsrc), "s"(soff), "s"(m0base), "n"(LDSOFF) : "memory", "scc");
}

// 1 KiB of input rows straight into LDS (lane L lands at M0 base + LDSOFF + 16 L): scalar base + per-lane 32-bit offset.  (No
// immediate offset: the instruction's offset field moves the LDS address as well as the global one.)
template <int LDSOFF>
__device__ __forceinline__ void dma_rows(unsigned voff, unsigned long long base, unsigned m0base) {
    asm volatile("s_add_i32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 "
                 ::"v"(voff), "s"(base), "s"(m0base), "n"(LDSOFF) : "memory", "scc");
}
// 16 bytes of the LDS staging -> a[R .. R + 3]
template <int R, int IMM>
__device__ __forceinline__ void lds_to_agpr(unsigned addr) {
    asm volatile("ds_read_b128 a[%c1:%c2], %0 offset:%c3" ::"v"(addr), "n"(R), "n"(R + 3), "n"(IMM) : "memory");
}
template <typename T>
__device__ __forceinline__ void pin_v(T& x) { asm volatile("" : "+v"(x)); }

// row maximum -> exponent of the power-of-two scale: same rule as split_rows_kernel (fuse.hip): maximum scaled into [512, 1024)
__device__ __forceinline__ int split_exponent(float m) {
    const int be = (int)((__float_as_uint(m) >> 23) & 0xffu);
    if (!(m > 0.f) || be == 0xff) return 0;
    return max(be - 127, -100);
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }
// one raw chunk (two quads from the staging read-back) -> a[R .. R + 7], its eight values folded into the two running row maxima
template <int R>
__device__ __forceinline__ void stash_chunk(const u32x4& q0, const u32x4& q1, float& m0, float& m1) {
    asm volatile("v_max3_f32 %0, |%2|, |%3|, %0\n\tv_max3_f32 %1, |%4|, |%5|, %1\n\tv_max3_f32 %0, |%6|, |%7|, %0\n\tv_max3_f32 %1, |%8|, |%9|, %1\n\t"
                 "v_accvgpr_write_b32 a[%c10+0], %2\n\tv_accvgpr_write_b32 a[%c10+1], %3\n\tv_accvgpr_write_b32 a[%c10+2], %4\n\t"
                 "v_accvgpr_write_b32 a[%c10+3], %5\n\tv_accvgpr_write_b32 a[%c10+4], %6\n\tv_accvgpr_write_b32 a[%c10+5], %7\n\t"
                 "v_accvgpr_write_b32 a[%c10+6], %8\n\tv_accvgpr_write_b32 a[%c10+7], %9"
                 : "+v"(m0), "+v"(m1) : "v"(q0.x), "v"(q0.y), "v"(q0.z), "v"(q0.w), "v"(q1.x), "v"(q1.y), "v"(q1.z), "v"(q1.w), "n"(R));
}
// a[R .. R + 7] (eight fp32 of one row: two 16-byte pieces of it, see the shape's k order) -> a[R .. R + 3] = their fp16 hi halves,
// a[R + 4 .. R + 7] = the lo halves.
//   hi = f16(x s) (x s is exact: s is a power of two), residual x s - hi exact in fp32, lo = f16(residual): split_rows_kernel's
//   arithmetic (fuse.hip), as one statement with the four pairs' chains interleaved (a dependent VALU pair costs 7 cycles, not 4)
template <int R>
__device__ __forceinline__ void convert_chunk_inplace(float s) {
    float x0, x1, x2, x3, x4, x5, x6, x7;
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    asm volatile(
        "v_accvgpr_read_b32 %0, a[%c17+0]\n\tv_accvgpr_read_b32 %1, a[%c17+1]\n\tv_accvgpr_read_b32 %2, a[%c17+2]\n\tv_accvgpr_read_b32 %3, a[%c17+3]\n\t"
        "v_accvgpr_read_b32 %4, a[%c17+4]\n\tv_accvgpr_read_b32 %5, a[%c17+5]\n\tv_accvgpr_read_b32 %6, a[%c17+6]\n\tv_accvgpr_read_b32 %7, a[%c17+7]\n\t"
        "v_fma_mixlo_f16 %8, %0, %16, 0\n\tv_fma_mixlo_f16 %9, %2, %16, 0\n\tv_fma_mixlo_f16 %10, %4, %16, 0\n\tv_fma_mixlo_f16 %11, %6, %16, 0\n\t"
        "v_fma_mixhi_f16 %8, %1, %16, 0\n\tv_fma_mixhi_f16 %9, %3, %16, 0\n\tv_fma_mixhi_f16 %10, %5, %16, 0\n\tv_fma_mixhi_f16 %11, %7, %16, 0\n\t"
        "v_fma_mix_f32 %0, %0, %16, -%8 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\tv_fma_mix_f32 %2, %2, %16, -%9 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mix_f32 %4, %4, %16, -%10 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\tv_fma_mix_f32 %6, %6, %16, -%11 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mix_f32 %1, %1, %16, -%8 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\tv_fma_mix_f32 %3, %3, %16, -%9 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mix_f32 %5, %5, %16, -%10 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\tv_fma_mix_f32 %7, %7, %16, -%11 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_accvgpr_write_b32 a[%c17+0], %8\n\tv_accvgpr_write_b32 a[%c17+1], %9\n\tv_accvgpr_write_b32 a[%c17+2], %10\n\tv_accvgpr_write_b32 a[%c17+3], %11\n\t"
        "v_cvt_pk_f16_f32 %12, %0, %1\n\tv_cvt_pk_f16_f32 %13, %2, %3\n\tv_cvt_pk_f16_f32 %14, %4, %5\n\tv_cvt_pk_f16_f32 %15, %6, %7\n\t"
        "v_accvgpr_write_b32 a[%c17+4], %12\n\tv_accvgpr_write_b32 a[%c17+5], %13\n\tv_accvgpr_write_b32 a[%c17+6], %14\n\tv_accvgpr_write_b32 a[%c17+7], %15"
        : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3), "=&v"(x4), "=&v"(x5), "=&v"(x6), "=&v"(x7), "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3),
          "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
        : "v"(s), "n"(R));
}
__device__ __forceinline__ void absmax3(float& m, float x, float y) { asm volatile("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(x), "v"(y)); }
// hi = f16(x s) for two values (x s is exact: s is a power of two), the residuals x s - hi (exact in fp32) replace x, lo = f16(residual):
// the arithmetic of split_rows_kernel (fuse.hip)
__device__ __forceinline__ void split_pair(float& x0, float& x1, float s, unsigned& hi, unsigned& lo) {
    asm volatile("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(x0), "v"(s));
    asm volatile("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(x1), "v"(s));
    asm volatile("v_fma_mix_f32 %0, %0, %1, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "+v"(x0) : "v"(s), "v"(hi));
    asm volatile("v_fma_mix_f32 %0, %0, %1, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(x1) : "v"(s), "v"(hi));
    asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(lo) : "v"(x0), "v"(x1));
}

// ---- the epilogue of a column block as a static stream of micro-ops -----------------------------------------------------------------
// Per accumulator i, 16 of them per lane (which row and column that is, and where its row scale rs sits, is the shape's: epi_item):
//   MUL t = acc * rs   FMA1 t = t * c.x + c.y   [EXP t = 2^t   ADD1 t = t + 1   RCP t = 1 / t] | [MAX t = max(t, 0)]   FMA2 t = t * c.z + c.w   ST
// with the lane constants c = {cs', b', c1, c0} of the accumulator's column folded by fc_strip_pack_kernel so that the chain is the
// whole FC epilogue:
//   tanh:    y' = 2 log2(e) (cs acc rs + bias), tanh = 1 - 2 / (2^y' + 1), out = (bn_s + bn_t) + (-2 bn_s) / (2^y' + 1)
//   sigmoid: y' = -log2(e) (...),              out = bn_t + bn_s / (2^y' + 1)
//   relu:    out = bn_s max(y, 0) + bn_t;      none: out = (cs bn_s) acc rs + (bn_s bias + bn_t)   (one fma)
// Elements go in groups of four, stage by stage, so that a dependent pair is four instructions apart (the transcendental ->
// VALU forwarding hazard needs one; hipcc pads nothing inside or between asm statements it cannot see into).  A group ends with its
// stores: one per element (32x32x16: a dword), or one per ST_STEP = 2 elements (16x16x32: a dwordx2 of two adjacent columns).
enum : unsigned char { OP_WAITCV = 0, OP_MUL, OP_FMA1, OP_EXP, OP_ADD1, OP_RCP, OP_MAX, OP_FMA2, OP_ST };
enum { ACT_LIN = 0, ACT_RELU = 1, ACT_EXP = 2 };                 // epilogue kinds (template parameter)
struct EpiOp { unsigned char kind, elem; };
struct EpiStream { EpiOp op[160]; int n; };

template <int ACTK, int ST_STEP>
constexpr EpiStream make_stream() {
    EpiStream s{};
    s.n = 0;
    auto push = [&](unsigned char k, int e) { s.op[s.n++] = EpiOp{k, (unsigned char)e}; };
    push(OP_WAITCV, 0);
    for (int g = 0; g < 4; ++g) {
        auto stage = [&](unsigned char k, int step) { for (int e = 0; e < 4; e += step) push(k, 4 * g + e); };
        stage(OP_MUL, 1);
        stage(OP_FMA1, 1);
        if (ACTK == ACT_EXP) { stage(OP_EXP, 1); stage(OP_ADD1, 1); stage(OP_RCP, 1); stage(OP_FMA2, 1); }
        if (ACTK == ACT_RELU) { stage(OP_MAX, 1); stage(OP_FMA2, 1); }
        stage(OP_ST, ST_STEP);
    }
    return s;
}

// ---- the schedule of one column block: two bodies H = 0, 1 (one ring slot each) of 16 fragments F, MF MFMAs behind each: MFMA issue
// slot sg = 16 MF H + MF F + m ---------------------------------------------------------------------------------------------------------
//   * (F, m = 0): the two fragment reads (hi, lo plane) of the fragment FD ahead -- from F = BAR_J on that is the NEXT ring slot;
//   * in front of fragment BAR_J: counted vmcnt (this wave's pieces of the next slot have landed) + s_barrier (everybody's have, and
//     everybody is done with the previous slot, which the pieces issued right behind the barrier refill -- 4 slots: 3 ahead);
//   * (BAR_J .. 15, m = piece_m) and two m = piece_m2 slots: the 8 DMA pieces;  slot 1 of the block: its lane constants (cv_loads loads);
//     -- in the LAST THREE bodies of a segment those pieces would fetch W slots beyond it: they carry the first three K-eighth rounds
//     of the NEXT strip's input rows instead (same count, same LDS targets: this wave's 8 KiB of the slot being freed); the first of
//     the three also issues round 3 into the staging-only fifth buffer, and round 4 goes into the last body's slot in front of the
//     drain: the strip switch starts with 40 of its 64 KiB per wave in LDS or on the way;
//   * everything else (with skip_read_slots: but the m = 0 slots): the epilogue stream of the previous block, spread evenly by cost,
//     at most slot_cycles per slot where that is set.  It starts behind the block's first fragment (the previous block's last MFMA has
//     retired by then) and ends `early` slots before the block does.
// What a shape sets:
//                       mfmas  skip_read_slots  piece_m  piece_m2  cv_loads  early  slot_cycles  cost_valu  cost_trans  cost_store
//   32x32x16 (fc_strip)   3        false           1        2         1        4     0 (no cap)      1          3           2      (instructions)
//   16x16x32 (fc_strip16) 6        true            2        4         2        6     8               4          8           8      (issue cycles
//     beside a 16-cycle MFMA, which itself holds the vector issue for 8: a slot takes 8 more -- one or two plain VALU, or one v_exp /
//     v_rcp, or one store)
struct Geometry {
    int mfmas;                // MFMAs per fragment; NSLOT = 32 * mfmas issue slots per column block
    bool skip_read_slots;     // the slots with the fragment reads take no epilogue
    int piece_m, piece_m2;    // m of the slots with a DMA piece
    int cv_loads;             // vector-memory operations of a block's lane-constant load
    int early;                // finish the stream this many usable slots early
    int slot_cycles;          // cap of the costs placed in one slot, 0: none
    int cost_valu, cost_trans, cost_store;
    constexpr int nslot() const { return 32 * mfmas; }
    constexpr int op_cost(unsigned char k) const {
        return (k == OP_EXP || k == OP_RCP) ? cost_trans : (k == OP_WAITCV ? 0 : (k == OP_ST ? cost_store : cost_valu));
    }
};
constexpr int MAX_NSLOT = 192;

constexpr int slot_piece(const Geometry& g, int sg) {
    const int F = (sg % (16 * g.mfmas)) / g.mfmas, m = sg % g.mfmas;
    if (m == g.piece_m && F >= BAR_J) return F - BAR_J;          // one per fragment behind the barrier ...
    if (m == g.piece_m2 && F == BAR_J + 1) return 6;             // ... and two fragments with a second one: the four waves leave the barrier
    if (m == g.piece_m2 && F == BAR_J + 4) return 7;             // together, and pieces packed into four fragments queue up in the CU's one TA path
    return -1;
}
constexpr bool slot_cvload(int sg) { return sg == 1; }
struct Plan {
    short begin[MAX_NSLOT + 1];   // slot sg issues the stream's items [begin[sg], begin[sg + 1])
    short vm_bar[2];      // vmcnt operand at the barrier of body H
    short vm_cv;          // vmcnt operand in front of the first use of the previous block's lane constants
    short st_half[2];     // stores of the stream issued in body H
    bool fits;
};
constexpr Plan make_plan(const Geometry& g, const EpiStream& st) {
    Plan p{};
    const int NSLOT = g.nslot();
    int usable = 0, total = 0;
    auto ok = [&](int sg) { return sg >= g.mfmas && !(g.skip_read_slots && sg % g.mfmas == 0) && slot_piece(g, sg) < 0; };
    for (int sg = 0; sg < NSLOT; ++sg) usable += ok(sg) ? 1 : 0;
    for (int i = 0; i < st.n; ++i) total += g.op_cost(st.op[i].kind);
    usable -= g.early;                                  // finish a few slots early
    int at = 0, k = 0, spent = 0;
    for (int sg = 0; sg < NSLOT; ++sg) {
        p.begin[sg] = (short)at;
        if (!ok(sg)) continue;
        ++k;
        const int target = (int)(((long)k * total + usable - 1) / usable);
        int here = 0;
        while (at < st.n && spent < target) {
            const int c = g.op_cost(st.op[at].kind);
            if (g.slot_cycles && here + c > g.slot_cycles) break;
            here += c; spent += c; ++at;
        }
    }
    p.begin[NSLOT] = (short)at;
    p.fits = at == st.n;
    // vector-memory program order over three consecutive identical blocks; the third one is measured
    int vm_n = 0, last_piece[3][2] = {}, cv_ord[3] = {}, bar_at[3][2] = {}, waitcv_at[3] = {};
    for (int blk = 0; blk < 3; ++blk)
        for (int sg = 0; sg < NSLOT; ++sg) {
            const int H = sg / (16 * g.mfmas), F = (sg % (16 * g.mfmas)) / g.mfmas, m = sg % g.mfmas;
            if (F == BAR_J && m == 0) bar_at[blk][H] = vm_n;
            if (slot_cvload(sg)) { vm_n += g.cv_loads; cv_ord[blk] = vm_n; }
            if (slot_piece(g, sg) >= 0) { ++vm_n; last_piece[blk][H] = vm_n; }
            for (int i = p.begin[sg]; i < p.begin[sg + 1]; ++i) {
                if (st.op[i].kind == OP_WAITCV) waitcv_at[blk] = vm_n;
                if (st.op[i].kind == OP_ST) { ++vm_n; if (blk == 2) ++p.st_half[H]; }
            }
        }
    auto clamp = [](int c) { return c < 0 ? 0 : (c > 63 ? 63 : c); };
    // barrier of body (b, H): the pieces of ring slot sigma + 1 were issued in body sigma - 2 = (b - 1, H)
    for (int H = 0; H < 2; ++H) p.vm_bar[H] = (short)clamp(bar_at[2][H] - last_piece[1][H]);
    p.vm_cv = (short)clamp(waitcv_at[2] - cv_ord[1]);
    return p;
}

// W ring prologue: the first three slots of the segment (slot s of the segment = image slot 2 blk0 + s, soffW its image offset); it
// lands while the strip is converted.  rsrcW: the image as a raw buffer starting at this wave's 8 KiB of a slot
__device__ __forceinline__ void ring_prologue(unsigned lane16, u32x4 rsrcW, unsigned& soffW, unsigned img_bytes, unsigned ldsw) {
    static_for<0, 3>([&](auto SC) __attribute__((always_inline)) {
        constexpr int s = decltype(SC)::value;
        static_for<0, PIECES>([&](auto PC) __attribute__((always_inline)) {
            constexpr int P = decltype(PC)::value;
            dma_piece<s * SLOT + P * 1024>(lane16 + (unsigned)(P * 1024), rsrcW, std::min(soffW, img_bytes - SLOT), ldsw);
        });
        soffW += SLOT;
    });
}
// (The other phases that read the same in the two kernel bodies -- the kernel prologue, the segment decode, the row offsets of a
// strip load, the segment end -- stay written out in each: as shared inline functions they changed hipcc's register assignment in
// one kernel or both, and the rule here is that sharing leaves the instructions alone.)

// ---- debug build (LAFF_FCS_TRACE): cycle stamps of wave 0 -- per segment s (up to 8): base 8 s: +0 start, +1 strip in the registers
// (raw), +2 row maxima, +3 converted, +4 ring prologue landed + barrier, +5 block loop done, +6 drained + segment end | [64 + s] = blocks
// of the segment.  (The kernel declares trc and trc_seg.) ----
#ifdef LAFF_FCS_TRACE
#define LAFF_FCS_STAMP(i) do { if (trc && tid == 0 && trc_seg < 8) trc[8 * trc_seg + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define LAFF_FCS_STAMP(i) do {} while (0)
#endif

}  // namespace fcs

// ---- W [D][512] fp32 (+ bias, BatchNorm, activation) -> the LDS image + the lane-constant table -------------------------------------
// One workgroup (256 threads) per output column n: row maximum -> power-of-two scale (as split_rows_kernel), hi / lo halves scattered
// into the image {block n / 32}{K half}{plane}{16 fragments}{64 lanes}{8 halves}, in the MFMA shape's fragment order:
//   32x32x16:  k = 16 j + 4 hh + (pos & 3) + 8 (pos >> 2):  fragment j % 16 (the sub-step),              lane 32 hh + n % 32
//   16x16x32:  k = 32 J + 4 g + (pos & 3) + 16 (pos >> 2):  fragment 2 (J % 8) + (n & 1) (K step, tile),  lane 16 g + (n % 32) / 2
// An image is read in the geometry it was packed in.
template <int MFMA>
__global__ __launch_bounds__(256) void fc_strip_pack_kernel(const float* __restrict__ W, int ldw, const float* __restrict__ bias,
                                                            const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int D,
                                                            int act, _Float16* __restrict__ img, float* __restrict__ vec) {
    using namespace fcs;
    static_assert(MFMA == 32 || MFMA == 16, "the two MFMA shapes");
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (n >= D) return;
    const float x0 = W[(size_t)n * ldw + tid], x1 = W[(size_t)n * ldw + 256 + tid];
    float m = fmaxf(fabsf(x0), fabsf(x1));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const int e = split_exponent(m);
    const float s = pow2f(9 - e), cs = pow2f(e - 9);
    const int blk = n >> 5;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k = t * 256 + tid;
        const float x = (t ? x1 : x0) * s;
        const _Float16 h = (_Float16)x, l = (_Float16)(x - (float)h);
        const int half = k >> 8;
        const size_t base = ((size_t)(blk * 2 + half) * 2) * (PLANE / 2);        // in halves: slot start
        size_t at;                                                                // in halves, inside the plane
        if constexpr (MFMA == 32) {
            const int n31 = n & 31, jj = (k >> 4) & 15, w = k & 15;
            const int hh = (w >> 2) & 1, pos = (w & 3) + 4 * (w >> 3);
            at = (size_t)(jj * 64 + 32 * hh + n31) * 8 + pos;
        } else {
            const int n15 = (n & 31) >> 1, u = n & 1, Jl = (k >> 5) & 7, w = k & 31;
            const int g = (w >> 2) & 3, pos = (w & 3) + 4 * (w >> 4);
            at = (size_t)((2 * Jl + u) * 64 + 16 * g + n15) * 8 + pos;
        }
        img[base + at] = h;
        img[base + PLANE / 2 + at] = l;
    }
    if (tid == 0) {
        const float b = bias ? bias[n] : 0.f, g = bn_scale ? bn_scale[n] : 1.f, t = bn_shift ? bn_shift[n] : 0.f;
        float4 c;
        if (act == LAFF_ACT_TANH) c = make_float4(cs * 2.885390081777927f, b * 2.885390081777927f, -2.f * g, g + t);
        else if (act == LAFF_ACT_SIGMOID) c = make_float4(cs * -1.4426950408889634f, b * -1.4426950408889634f, g, t);
        else if (act == LAFF_ACT_RELU) c = make_float4(cs, b, g, t);
        else c = make_float4(cs * g, fmaf(b, g, t), 0.f, 0.f);
        *(float4*)(vec + 4 * (size_t)n) = c;
    }
}

// ---- host side: one launch per (MFMA shape, epilogue kind); each shape's file picks among its three by kind (ACT_*) -----------------
template <void (*KERNEL)(const FcStripArgs)>
hipError_t fc_strip_launch(const FcStripArgs& a, hipStream_t st) {
    static unsigned long long attr_done = 0;
    if (hipError_t e = smem_attr_once(attr_done, KERNEL, fcs::SMEM); e != hipSuccess) return e;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)a.nranges), dim3(256), fcs::SMEM, st, a);
    return hipGetLastError();
}
hipError_t fc_strip32_launch(const FcStripArgs& a, int kind, hipStream_t st);      // fc_strip.hip
hipError_t fc_strip16_launch(const FcStripArgs& a, int kind, hipStream_t st);      // fc_strip16.hip

}  // namespace laff
