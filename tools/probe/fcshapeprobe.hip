// The FC strip's block loop on the two fp16 MFMA shapes, side by side: does the chip hold a higher clock on v_mfma_f32_16x16x32_f16
// than on v_mfma_f32_32x32x16_f16 when the loop carries what fc_strip_kernel's carries?  (docs/experiments.md, "fc_strip on 16x16x32".)
//
// One wavefront per SIMD (256 threads, 512 registers, all of the CU's LDS), 256 accumulator registers of stationary A (32 rows x
// K = 512, {hi, lo} fp16 halves of random data, a[8 s .. 8 s + 3] hi, a[8 s + 4 .. 8 s + 7] lo), B fragments re-read from LDS by
// ds_read_b128 into rotating register sets a few groups ahead, counted lgkmcnt.  Per column block of 32 outputs the wave's tile is
// 32 x 32 (16 accumulators per lane) in both arms:
//   SHAPE 32: 32 sub-steps of 16 k, three MFMAs 32x32x16 each (lo.hi, hi.lo, hi.hi) into one f32x16               96 MFMAs x 32 cycles
//   SHAPE 16: 16 steps of 32 k x 2 column tiles, per row tile t the same three products into acc[t][u] (f32x4)    192 MFMAs x 16 cycles
//   RD 4: a pair of fragment reads (hi, lo) per 3 resp. 6 MFMAs -- 64 reads per block, what fc_strip_kernel does;
//   RD 2: a pair per K = 32, i.e. per 6 resp. 12 MFMAs -- half the LDS read traffic.
// Two accumulator sets alternate; the tanh epilogue of the previous block (per element v_mul, v_fma, v_exp, v_add, v_rcp, v_fma;
// per store a v_mad for the address: 80 plain VALU, 32 v_exp / v_rcp, 16 dword stores resp. 8 dwordx2 stores, nt, 16 KiB per
// workgroup and block) is spread behind the MFMAs of the current one by a compile-time plan:
//   SHAPE 32: cost-proportional over the slots, at most 24 cycles of issue cost and one v_exp / v_rcp per slot;
//   SHAPE 16: at most 8 cycles per slot (plain 4; v_exp / v_rcp 8, alone; v_mad + store 8, alone), none in a slot with fragment reads.
// All arms run in one process in interleaved rounds; reported per arm: wall time per launch (events) and the in-kernel clock
// (delta s_memtime / delta s_memrealtime x 100 MHz around the block loop, median over workgroups).
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/probe/fcshapeprobe.hip -o fcshapeprobe && ./fcshapeprobe [rounds] [launches] [blocks]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                                       \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess) {                                                                        \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));         \
            exit(1);                                                                                   \
        }                                                                                              \
    } while (0)

constexpr int SMEM = 160 * 1024;          // all of the CU's LDS: one workgroup per CU
constexpr int LO_PLANE = 32 * 1024;       // LDS: hi fragments of group g at 1024 g, lo fragments at LO_PLANE + 1024 g
constexpr int IMG = 64 * 1024;
constexpr int OUT_PER_BLOCK = 16 * 1024;  // 128 rows x 32 columns fp32
constexpr int OUT_RING = 64;              // blocks of output per workgroup before the addresses repeat
constexpr size_t OUT_PER_WG = (size_t)OUT_PER_BLOCK * OUT_RING;

template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}
template <int N>
__device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }

// the accumulator file belongs to the stationary operand: hipcc sees all 256 registers occupied from entry to exit
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

template <int R>
__device__ __forceinline__ void agpr_load4(const void* p) {            // a[R .. R + 3] <- 16 bytes at p + 4 R
    asm volatile("global_load_dwordx4 a[%c1:%c2], %0, off offset:%c3" ::"v"(p), "n"(R), "n"(R + 3), "n"(4 * R) : "memory");
}
template <int R, bool FIRST>
__device__ __forceinline__ void mfma32(f32x16& acc, const u32x4& b) {
    if constexpr (FIRST) asm volatile("v_mfma_f32_32x32x16_f16 %0, a[%c2:%c3], %1, 0" : "=v"(acc) : "v"(b), "n"(R), "n"(R + 3));
    else asm volatile("v_mfma_f32_32x32x16_f16 %0, a[%c2:%c3], %1, %0" : "+v"(acc) : "v"(b), "n"(R), "n"(R + 3));
}
template <int R, bool FIRST>
__device__ __forceinline__ void mfma16(f32x4& acc, const u32x4& b) {
    if constexpr (FIRST) asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c2:%c3], %1, 0" : "=v"(acc) : "v"(b), "n"(R), "n"(R + 3));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c2:%c3], %1, %0" : "+v"(acc) : "v"(b), "n"(R), "n"(R + 3));
}
template <int IMM>
__device__ __forceinline__ void lds_read128(u32x4& d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(IMM));
}

// ---- the epilogue of a block as a static stream, and where its items go ---------------------------------------------------------------
enum : unsigned char { OP_MUL = 0, OP_FMA1, OP_EXP, OP_ADD1, OP_RCP, OP_FMA2, OP_PAD, OP_ST };
struct EpiOp { unsigned char kind, elem; };
struct EpiStream { EpiOp op[160]; int n; };
constexpr int op_cycles(unsigned char k) { return (k == OP_EXP || k == OP_RCP || k == OP_ST) ? 8 : 4; }

template <int SHAPE>
constexpr EpiStream make_stream() {
    EpiStream s{};
    s.n = 0;
    auto push = [&](unsigned char k, int e) { s.op[s.n++] = EpiOp{k, (unsigned char)e}; };
    for (int g = 0; g < 4; ++g) {          // elements in groups of four, stage by stage: a dependent pair is four instructions apart
        auto stage = [&](unsigned char k) { for (int e = 0; e < 4; ++e) push(k, 4 * g + e); };
        stage(OP_MUL); stage(OP_FMA1); stage(OP_EXP); stage(OP_ADD1); stage(OP_RCP); stage(OP_FMA2);
        if (SHAPE == 32) stage(OP_ST);                                                    // 16 x (v_mad + dword store)
        else { push(OP_PAD, 4 * g); push(OP_PAD, 4 * g + 2); push(OP_ST, 4 * g); push(OP_ST, 4 * g + 2); }   // 8 x (v_mad + dwordx2 store)
    }
    return s;
}

template <int SHAPE, int RD>
struct Cfg {
    static constexpr int NSLOT = SHAPE == 32 ? 96 : 192;                       // MFMAs of a block
    static constexpr int MPG = (SHAPE == 32 ? 3 : 6) * (RD == 2 ? 2 : 1);      // MFMAs per pair of fragment reads
    static constexpr int NG = NSLOT / MPG;                                     // read groups of a block
    static constexpr int AHEAD = RD == 4 ? 6 : 3;                              // fragment reads run this many groups ahead,
    static constexpr int NSETS = RD == 4 ? 8 : 4;                              // into this many register sets
    static constexpr int START = SHAPE == 32 ? 3 : 6;                          // the previous block's last MFMA has retired by this slot
    static constexpr int CAP = SHAPE == 32 ? 24 : 8;                           // issue cycles of fillers per slot
    static_assert(NG % NSETS == 0 && AHEAD < NSETS, "the set of a group must not depend on the block");
};
struct Plan { short begin[193]; bool fits; };
template <int SHAPE, int RD>
constexpr Plan make_plan() {
    using C = Cfg<SHAPE, RD>;
    Plan p{};
    const EpiStream st = make_stream<SHAPE>();
    auto ok = [](int sg) { return sg >= C::START && !(SHAPE == 16 && sg % C::MPG == 0); };
    int usable = 0, total = 0;
    for (int sg = 0; sg < C::NSLOT; ++sg) usable += ok(sg) ? 1 : 0;
    for (int i = 0; i < st.n; ++i) total += op_cycles(st.op[i].kind);
    usable -= 4;                                        // finish a few slots early
    int at = 0, k = 0, spent = 0;
    for (int sg = 0; sg < C::NSLOT; ++sg) {
        p.begin[sg] = (short)at;
        if (!ok(sg)) continue;
        ++k;
        const int target = (int)(((long)k * total + usable - 1) / usable);
        int here = 0;
        bool slow = false;
        while (at < st.n && spent < target) {
            const int c = op_cycles(st.op[at].kind);
            const bool s8 = st.op[at].kind == OP_EXP || st.op[at].kind == OP_RCP;
            if (here > 0 && (here + c > C::CAP || (s8 && slow))) break;
            here += c; spent += c; slow = slow || s8; ++at;
        }
    }
    p.begin[C::NSLOT] = (short)at;
    p.fits = at == st.n;
    return p;
}

template <int SHAPE, int RD>
__global__ __launch_bounds__(256, 1) void probe(const unsigned* __restrict__ A, const u32x4* __restrict__ B, char* __restrict__ out,
                                                unsigned long long* __restrict__ stamps, int nblocks) {
    using C = Cfg<SHAPE, RD>;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    AgprHold hold;
    agpr_hold_begin(hold);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr Plan PLAN = make_plan<SHAPE, RD>();
    static_assert(PLAN.fits, "the epilogue stream does not fit behind the MFMAs of one block");

    // the B image -> LDS, the stationary operand -> a[0:255]
    for (int i = tid; i < IMG / 16; i += 256) ((u32x4*)smem)[i] = B[i];
    const unsigned* ap = A + (size_t)tid * 256;
    static_for<0, 64>([&](auto RC) { agpr_load4<4 * decltype(RC)::value>(ap); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
    unsigned xa = lds0 + (unsigned)lane * 16u;
    asm volatile("" : "+v"(xa));
    float rs[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { rs[i] = 2.3841858e-07f * (float)(1 + ((lane + i) & 3)); asm volatile("" : "+v"(rs[i])); }   // 2^-22 ..
    f32x4 cv = {1.0f, 0.1f, -2.0f, 1.0f};
    asm volatile("" : "+v"(cv));
    unsigned ldy4 = 128u;
    asm volatile("" : "+s"(ldy4));
    // SHAPE 32: lane (column n = lane & 31, hh = lane >> 5), accumulator i <-> row 8 (i >> 2) + 4 hh + (i & 3), a dword per store;
    // SHAPE 16: lane (n = lane & 15, g = lane >> 4), columns 2 n + u, rows 16 t + 4 g + e, the two columns in one dwordx2 store
    unsigned voff0 = SHAPE == 32 ? ((unsigned)(wave * 32 + 4 * (lane >> 5)) * 32u + (unsigned)(lane & 31)) * 4u
                                 : ((unsigned)(wave * 32 + 4 * (lane >> 4)) * 32u + 2u * (unsigned)(lane & 15)) * 4u;
    asm volatile("" : "+v"(voff0));
    const unsigned long long out_wg = (unsigned long long)out + (unsigned long long)blockIdx.x * OUT_PER_WG;

    f32x16 acc32[2];
    f32x4 acc16[2][2][2];                    // [set][row tile t][column tile u]
    u32x4 fr[C::NSETS][2];
    float tt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x2 tp[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    unsigned ta[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) acc32[0][e] = acc32[1][e] = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc16[q][0][0][e] = acc16[q][0][1][e] = acc16[q][1][0][e] = acc16[q][1][1][e] = 0.f;

    unsigned long long yb = 0;              // where the stores of the running epilogue go
    auto epi_item = [&acc32, &acc16, &tt, &tp, &ta, &rs, &cv, &voff0, &ldy4, &yb](auto QC, auto IC) {
        constexpr int Q = decltype(QC)::value;
        constexpr EpiOp op = make_stream<SHAPE>().op[decltype(IC)::value];
        constexpr int i = op.elem;
        if constexpr (SHAPE == 32) {
            if constexpr (op.kind == OP_MUL) asm volatile("v_mul_f32 %0, %1, %2" : "=v"(tt[i & 7]) : "v"(acc32[Q][i]), "v"(rs[i]));
            else if constexpr (op.kind == OP_FMA1) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(tt[i & 7]) : "v"(cv.x), "v"(cv.y));
            else if constexpr (op.kind == OP_EXP) asm volatile("v_exp_f32 %0, %0" : "+v"(tt[i & 7]));
            else if constexpr (op.kind == OP_ADD1) asm volatile("v_add_f32 %0, 1.0, %0" : "+v"(tt[i & 7]));
            else if constexpr (op.kind == OP_RCP) asm volatile("v_rcp_f32 %0, %0" : "+v"(tt[i & 7]));
            else if constexpr (op.kind == OP_FMA2) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(tt[i & 7]) : "v"(cv.z), "v"(cv.w));
            else if constexpr (op.kind == OP_ST)
                asm volatile("v_mad_u32_u24 %0, %3, %4, %2\n\tglobal_store_dword %0, %1, %5 nt"
                             : "=&v"(ta[i & 3]) : "v"(tt[i & 7]), "v"(voff0), "s"(ldy4), "n"(8 * (i >> 2) + (i & 3)), "s"(yb) : "memory");
        } else {
            constexpr int u = i & 1, e = (i >> 1) & 3, t = i >> 3, k = (i >> 1) & 3;      // element i: column tile u, register e, row tile t
            if constexpr (op.kind == OP_MUL) asm volatile("v_mul_f32 %0, %1, %2" : "=v"(tp[k][u]) : "v"(acc16[Q][t][u][e]), "v"(rs[i]));
            else if constexpr (op.kind == OP_FMA1) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(tp[k][u]) : "v"(cv.x), "v"(cv.y));
            else if constexpr (op.kind == OP_EXP) asm volatile("v_exp_f32 %0, %0" : "+v"(tp[k][u]));
            else if constexpr (op.kind == OP_ADD1) asm volatile("v_add_f32 %0, 1.0, %0" : "+v"(tp[k][u]));
            else if constexpr (op.kind == OP_RCP) asm volatile("v_rcp_f32 %0, %0" : "+v"(tp[k][u]));
            else if constexpr (op.kind == OP_FMA2) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(tp[k][u]) : "v"(cv.z), "v"(cv.w));
            else if constexpr (op.kind == OP_PAD) asm volatile("v_max_f32 %0, %0, %0" : "+v"(tp[k][1]));
            else if constexpr (op.kind == OP_ST)
                asm volatile("v_mad_u32_u24 %0, %3, %4, %2\n\tglobal_store_dwordx2 %0, %1, %5 nt"
                             : "=&v"(ta[k]) : "v"(tp[k]), "v"(voff0), "s"(ldy4), "n"(16 * t + e), "s"(yb) : "memory");
        }
    };
    auto body = [&](auto PARC, int blk) {
        constexpr int PAR = decltype(PARC)::value, Q = PAR ^ 1;
        yb = out_wg + (unsigned long long)((unsigned)(blk - 1) & (OUT_RING - 1)) * OUT_PER_BLOCK;
        asm volatile("" : "+s"(yb));
        static_for<0, C::NG>([&](auto GC) {
            constexpr int G = decltype(GC)::value;
            // the fragments of this group have arrived (SHAPE 16 with a pair of reads per column tile: both tiles' at the even group)
            if constexpr (SHAPE == 32 || RD == 2) wait_lgkm<2 * (C::AHEAD - 1)>();
            else if constexpr (G % 2 == 0) wait_lgkm<2 * (C::AHEAD - 2)>();
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, C::MPG>([&](auto MC) {
                constexpr int m = decltype(MC)::value, SG = C::MPG * G + m;
                // lo.hi, hi.lo (small terms first), hi.hi
                if constexpr (SHAPE == 32) {
                    constexpr int S = RD == 4 ? G : 2 * G + m / 3, M = m % 3;
                    const u32x4& whi = fr[G % C::NSETS][0];
                    const u32x4& wlo = fr[G % C::NSETS][1];
                    if constexpr (M == 0) mfma32<8 * S + 4, (SG == 0)>(acc32[PAR], whi);
                    else if constexpr (M == 1) mfma32<8 * S, false>(acc32[PAR], wlo);
                    else mfma32<8 * S, false>(acc32[PAR], whi);
                } else {
                    // the twelve MFMAs of a K step go product by product over the four accumulators: an accumulator every fourth MFMA
                    constexpr int J = SG / 12, s12 = SG % 12, M = s12 / 4, u = (s12 % 4) / 2, t = s12 & 1, R = 16 * J + 8 * t;
                    constexpr int FG = RD == 4 ? 2 * J + u : J;                   // the read group of column tile u
                    const u32x4& whi = fr[FG % C::NSETS][0];
                    const u32x4& wlo = fr[FG % C::NSETS][1];
                    if constexpr (M == 0) mfma16<R + 4, (J == 0)>(acc16[PAR][t][u], whi);
                    else if constexpr (M == 1) mfma16<R, false>(acc16[PAR][t][u], wlo);
                    else mfma16<R, false>(acc16[PAR][t][u], whi);
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (m == 0) {
                    constexpr int GN = (G + C::AHEAD) % C::NG, SN = (G + C::AHEAD) % C::NSETS;
                    lds_read128<GN * 1024>(fr[SN][0], xa);
                    lds_read128<LO_PLANE + GN * 1024>(fr[SN][1], xa);
                }
                static_for<PLAN.begin[SG], PLAN.begin[SG + 1]>([&](auto IC) {
                    __builtin_amdgcn_sched_barrier(0);
                    epi_item(std::integral_constant<int, Q>{}, IC);
                });
                __builtin_amdgcn_sched_barrier(0);
            });
        });
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    static_for<0, C::AHEAD>([&](auto GC) {       // fragments of the first groups (behind the stamps: their wait is not the loop's)
        constexpr int g = decltype(GC)::value;
        lds_read128<g * 1024>(fr[g][0], xa);
        lds_read128<LO_PLANE + g * 1024>(fr[g][1], xa);
    });
#pragma nounroll
    for (int b = 0; b < nblocks; b += 2) {
        body(std::integral_constant<int, 0>{}, b);
        body(std::integral_constant<int, 1>{}, b + 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
    for (int s8 = 0; s8 < C::NSETS; ++s8) asm volatile("" ::"v"(fr[s8][0]), "v"(fr[s8][1]));
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) s += acc32[0][e] + acc32[1][e];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        s += acc16[0][0][0][e] + acc16[0][0][1][e] + acc16[0][1][0][e] + acc16[0][1][1][e] + acc16[1][0][0][e] + acc16[1][0][1][e] +
             acc16[1][1][0][e] + acc16[1][1][1][e];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += tt[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) s += tp[i][0] + tp[i][1];
    ((float*)(stamps + 2 * gridDim.x))[(size_t)blockIdx.x * 256 + tid] = s;
    if (tid == 0) {
        stamps[2 * blockIdx.x] = c1 - c0;
        stamps[2 * blockIdx.x + 1] = r1 - r0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    agpr_hold_end(hold);
}

static unsigned short f16_bits(float x) {
    const _Float16 h = (_Float16)x;
    unsigned short b;
    memcpy(&b, &h, 2);
    return b;
}
static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static float uniform(float amp) {          // (-amp, amp)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return amp * ((float)((rng_state >> 40) & 0xffffff) / 8388608.0f - 1.0f);
}
static unsigned pair_bits(float amp) { return (unsigned)f16_bits(uniform(amp)) | ((unsigned)f16_bits(uniform(amp)) << 16); }

struct Arm {
    const char* name;
    void (*kernel)(const unsigned*, const u32x4*, char*, unsigned long long*, int);
    std::vector<double> ms, ghz, cyc;
};

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 12, launches = argc > 2 ? atoi(argv[2]) : 40;
    const int blocks = (argc > 3 ? atoi(argv[3]) : 2048) & ~1;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int G = prop.multiProcessorCount;
    printf("device %s, %d CUs; %d rounds x %d launches x %d blocks per arm\n", prop.name, G, rounds, launches, blocks);

    // hi halves: row maximum scaled into [512, 1024); lo halves: the fp16 residual of such a value
    std::vector<unsigned> hA(256 * 256), hB(IMG / 4);
    for (int t = 0; t < 256; ++t)
        for (int r = 0; r < 256; ++r) hA[t * 256 + r] = pair_bits((r & 4) ? 0.25f : 1024.f);
    for (int i = 0; i < IMG / 4; ++i) hB[i] = pair_bits(i * 4 >= LO_PLANE ? 0.25f : 1024.f);
    unsigned* dA; u32x4* dB; char* dOut; unsigned long long* dStamps;
    const size_t stamp_bytes = (size_t)G * 16 + (size_t)G * 256 * 4;
    CHECK(hipMalloc(&dA, hA.size() * 4));
    CHECK(hipMalloc(&dB, IMG));
    CHECK(hipMalloc(&dOut, (size_t)G * OUT_PER_WG));
    CHECK(hipMalloc(&dStamps, stamp_bytes));
    CHECK(hipMemcpy(dA, hA.data(), hA.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dB, hB.data(), IMG, hipMemcpyHostToDevice));
    CHECK(hipMemset(dOut, 0, (size_t)G * OUT_PER_WG));

    Arm arms[4] = {{"32x32x16, 64 reads/block", probe<32, 4>, {}, {}, {}},
                   {"16x16x32, 64 reads/block", probe<16, 4>, {}, {}, {}},
                   {"32x32x16, 32 reads/block", probe<32, 2>, {}, {}, {}},
                   {"16x16x32, 32 reads/block", probe<16, 2>, {}, {}, {}}};
    for (Arm& a : arms) CHECK(hipFuncSetAttribute((const void*)a.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    auto run = [&](Arm& a, int n, bool record) {
        CHECK(hipEventRecord(e0, 0));
        for (int i = 0; i < n; ++i) hipLaunchKernelGGL(a.kernel, dim3(G), dim3(256), SMEM, 0, dA, dB, dOut, dStamps, blocks);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (!record) return (double)ms;
        std::vector<unsigned long long> h(2 * G);
        CHECK(hipMemcpy(h.data(), dStamps, h.size() * 8, hipMemcpyDeviceToHost));
        std::vector<double> f(G), c(G);
        for (int w = 0; w < G; ++w) { f[w] = (double)h[2 * w] / (double)h[2 * w + 1] * 0.1; c[w] = (double)h[2 * w]; }
        std::sort(f.begin(), f.end());
        std::sort(c.begin(), c.end());
        a.ms.push_back(ms / n);
        a.ghz.push_back(f[G / 2]);
        a.cyc.push_back(c[G / 2] / blocks);
        return (double)ms;
    };
    double warm = 0;                                       // the clock settles under load: > 2 s of back-to-back launches first
    while (warm < 2500.0) for (Arm& a : arms) warm += run(a, 10, false);
    for (int r = 0; r < rounds; ++r) for (Arm& a : arms) run(a, launches, true);

    std::vector<float> sums((size_t)G * 256);
    CHECK(hipMemcpy(sums.data(), (char*)dStamps + (size_t)G * 16, sums.size() * 4, hipMemcpyDeviceToHost));
    double chk = 0;
    for (float x : sums) chk += x;
    auto med = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    auto mn = [](const std::vector<double>& v) { return *std::min_element(v.begin(), v.end()); };
    auto mx = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()); };
    for (Arm& a : arms)
        printf("%-26s wall ms/launch median %.4f min %.4f max %.4f | clock GHz median %.3f min %.3f max %.3f | cycles/block %.0f\n", a.name,
               med(a.ms), mn(a.ms), mx(a.ms), med(a.ghz), mn(a.ghz), mx(a.ghz), med(a.cyc));
    for (int p = 0; p < 4; p += 2)
        printf("%s: 32x32x16 / 16x16x32 wall, median %.4f, min %.4f, slowest 16 vs fastest 32 %.4f\n", p ? "32 reads/block" : "64 reads/block",
               med(arms[p].ms) / med(arms[p + 1].ms), mn(arms[p].ms) / mn(arms[p + 1].ms), mn(arms[p].ms) / mx(arms[p + 1].ms));
    printf("checksum of the last launch's accumulators %.6g\n", chk);
    return 0;
}
