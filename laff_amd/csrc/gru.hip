// gru.hip -- the GRU caption encoder of the text tower: the inference step and its saving variant for training (gru_bwd.hip)
// (reference model/model.py:323-396 GruTxtEncoder / BiGruTxtEncoder: nn.GRU over the embedded caption + mean / last pooling).
//
// torch.nn.GRU arithmetic, gate order r, z, n, h0 = 0:
//   r = sigma(W_ir x + b_ir + W_hr h + b_hr)    z = sigma(W_iz x + b_iz + W_hz h + b_hz)
//   n = tanh(W_in x + b_in + r * (W_hn h + b_hn))                h' = (1 - z) * n + z * h
//
// The input half is a table: x_t = we[token], so W_ih x_t + b_ih is row `token` of P = we . W_ih^T + b_ih [V, 3H], built once per
// weight set by the fp32 GEMM (laff_fc_act_bn); a step gathers three values of it per (row, hidden unit).
//
// The recurrent half is one launch per time step (both directions of a bigru in the same launch, grid.z): over the active prefix
// of the length-sorted rows, gh = h_{t-1} . W_hh^T on v_mfma_f32_16x16x4_f32, and the gate epilogue in the same workgroup: gather
// from P, add b_hh, the gates, h_t to a ping-pong buffer, the pooled sum, and at each row's last step that row's output.  The
// launch boundary orders the steps; workgroups never talk to each other.
//
// A workgroup (4 waves) owns 16*RT rows x 16*UT hidden units, i.e. the r, z and n columns of the same units, so the epilogue has
// all three gates of an element at hand.  The K = H sum is split over the 4 waves by 16-wide chunks (wave w: chunks
// [w*nc/4, (w+1)*nc/4), nc = H/16) and the partials are added in LDS as (p0 + p2) + (p1 + p3).  That split and every MFMA's k
// order depend on H only -- not on RT / UT, the batch or a row's position -- so a caption's features are bitwise the same whatever
// else is in its batch (the tile shape is picked per step from the number of active rows).
//
// Operand layouts (both built so that one wave's float4 load of a 16 x 16 operand block is 1 KB contiguous):
//   packed W_hh: Wp[ut][kc][g][lane][j] = W_hh[g*H + 16*ut + (lane&15)][16*kc + 4*(lane>>4) + j]     (laff_gru_pack_whh)
//   packed h:    Hp[rt][kc][lane][j]    = h[16*rt + (lane&15)][16*kc + 4*(lane>>4) + j]
// MFMA j of chunk kc then takes component j: lane group G = lane>>4 supplies k = 16*kc + 4*G + j for both operands.
#include <algorithm>

#include "kernels.h"

namespace laff {

typedef float gru_f4 __attribute__((ext_vector_type(4)));

constexpr int GRU_THREADS = 256;

__device__ __forceinline__ long gru_h_index(int row, int u, int nc) {
    return ((long)(row >> 4) * nc + (u >> 4)) * 256 + (((row & 15) + 16 * ((u & 15) >> 2)) << 2) + (u & 3);
}

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void gru_pack_whh_kernel(const float* __restrict__ W, int H, float* __restrict__ Wp) {
    const int nc = H >> 4;
    const long total = 3L * H * H;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const int j = (int)(o & 3), lane = (int)((o >> 2) & 63);
        long q = o >> 8;
        const int g = (int)(q % 3);
        q /= 3;
        const int kc = (int)(q % nc), ut = (int)(q / nc);
        Wp[o] = W[(long)(g * H + 16 * ut + (lane & 15)) * H + 16 * kc + 4 * (lane >> 4) + j];
    }
}

// SAVE: the training step (laff_gru_encode_train).  It also stores r, z, n, q = W_hn h + b_hn and h_prev of every active
// element at the row's packed position D.off + row of the reserve; the inference instantiations have none of it.
template <int RT, int UT, bool SAVE = false>
__global__ __launch_bounds__(GRU_THREADS) void gru_step_kernel(GruStepArgs s) {
    const GruDirArgs D = blockIdx.z ? s.d1 : s.d0;
    const int row0 = blockIdx.y * 16 * RT;
    if (row0 >= D.B) return;
    const int H = s.H, nc = H >> 4;
    const int u0 = blockIdx.x * 16 * UT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NA = RT * UT * 3;                 // accumulators per wave: (row tile, unit tile, gate)
    __shared__ gru_f4 red[2][NA][64];

    gru_f4 acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = gru_f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (!s.skip_gemm) {
        const gru_f4* A = reinterpret_cast<const gru_f4*>(D.h_in) + (long)(row0 >> 4) * nc * 64 + lane;
        const gru_f4* W = reinterpret_cast<const gru_f4*>(D.Wp) + (long)(u0 >> 4) * nc * 3 * 64 + lane;
        const int kb = wave * nc / 4, ke = (wave + 1) * nc / 4;
        for (int kc = kb; kc < ke; ++kc) {
            gru_f4 a[RT], b[UT * 3];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) a[rt] = A[((long)rt * nc + kc) * 64];
#pragma unroll
            for (int ut = 0; ut < UT; ++ut)
#pragma unroll
                for (int g = 0; g < 3; ++g) b[ut * 3 + g] = W[(((long)ut * nc + kc) * 3 + g) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int c = 0; c < UT * 3; ++c)
                        acc[rt * UT * 3 + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][j], b[c][j], acc[rt * UT * 3 + c], 0, 0, 0);
        }
    }
    // fixed-order reduction of the 4 K-slices: (p0 + p2) + (p1 + p3); the total ends in red[0]
    if (wave >= 2)
#pragma unroll
        for (int a = 0; a < NA; ++a) red[wave - 2][a][lane] = acc[a];
    __syncthreads();
    if (wave < 2)
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[a] += red[wave][a][lane];
    __syncthreads();
    if (wave == 1)
#pragma unroll
        for (int a = 0; a < NA; ++a) red[0][a][lane] = acc[a];
    __syncthreads();
    if (wave == 0)
#pragma unroll
        for (int a = 0; a < NA; ++a) red[0][a][lane] = acc[a] + red[0][a][lane];
    __syncthreads();

    // gate epilogue: consecutive threads take consecutive hidden units of one row
    const float* red0 = reinterpret_cast<const float*>(&red[0][0][0]);
    for (int e = threadIdx.x; e < 256 * RT * UT; e += GRU_THREADS) {
        const int uu = e % (16 * UT), i = e / (16 * UT);
        const int row = row0 + i;
        if (row >= D.B) break;                      // e grows with i: every later element of this thread is past B too
        const int u = u0 + uu;
        const int cl = (uu & 15) + 16 * ((i & 15) >> 2), reg = i & 3;    // C/D map of 16x16x4: col = lane&15, row = 4*(lane>>4)+reg
        const int a0 = ((i >> 4) * UT + (uu >> 4)) * 3;
        const float gr = red0[((a0 + 0) * 64 + cl) * 4 + reg];
        const float gz = red0[((a0 + 1) * 64 + cl) * 4 + reg];
        const float gn = red0[((a0 + 2) * 64 + cl) * 4 + reg];
        const int tok = s.tokens[(long)D.t * s.N + row];
        float xr = __builtin_nanf(""), xz = xr, xn = xr;       // a token outside the table poisons its row instead of reading past P
        if ((unsigned)tok < (unsigned)s.V) {
            const float* p = D.P + (long)tok * 3 * H + u;
            xr = p[0];
            xz = p[H];
            xn = p[2 * H];
        }
        const float r = gru_sigmoid(xr + (gr + D.bhh[u]));
        const float z = gru_sigmoid(xz + (gz + D.bhh[H + u]));
        const float n = tanhf(xn + r * (gn + D.bhh[2 * H + u]));
        const long hi = gru_h_index(row, u, nc);
        const float hp = D.h_in[hi];
        const float h = fmaf(z, hp - n, n);
        D.h_out[hi] = h;
        if constexpr (SAVE) {
            const long plane = (long)s.M * H;
            float* rs = D.res + ((long)D.off + row) * H + u;
            rs[0] = r;
            rs[plane] = z;
            rs[2 * plane] = n;
            rs[3 * plane] = gn + D.bhh[2 * H + u];
            rs[4 * plane] = hp;
        }
        float sum = 0.0f;
        if (s.pooling != LAFF_GRU_LAST) {
            float* sp = D.sum + (long)row * H + u;
            sum = *sp + h;
            *sp = sum;
        }
        const int len = s.lens[row];
        if (D.t != (blockIdx.z ? 0 : len - 1)) continue;
        const int orow = s.perm[row];
        if ((unsigned)orow >= (unsigned)s.N) continue;
        float* o = s.out + (long)orow * s.ldo;
        if (s.pooling == LAFF_GRU_MEAN) o[D.col0 + u] = sum / (float)len;
        else if (s.pooling == LAFF_GRU_LAST) o[u] = h;
        else {
            o[u] = sum / (float)len;
            o[H + u] = h;
        }
    }
}

hipError_t launch_gru_pack_whh(const float* W, int H, float* Wp, hipStream_t st) {
    const long total = 3L * H * H;
    const int blocks = (int)std::min<long>((total + 255) / 256, 8192);
    gru_pack_whh_kernel<<<blocks, 256, 0, st>>>(W, H, Wp);
    return hipGetLastError();
}

// the 64 x 32 tile loads 5x fewer operand bytes per MFMA; it pays once there are enough of them to fill the device
bool gru_step_big(int B, int H, int ndirs) { return (long)((B + 63) / 64) * (H / 32) * ndirs >= 512; }

hipError_t launch_gru_step(const GruStepArgs& s, int ndirs, hipStream_t st, bool save) {
    const int B = std::max(s.d0.B, ndirs > 1 ? s.d1.B : 0);
    if (gru_step_big(B, s.H, ndirs)) {
        dim3 grid(s.H / 32, (B + 63) / 64, ndirs);
        if (save) gru_step_kernel<4, 2, true><<<grid, GRU_THREADS, 0, st>>>(s);
        else gru_step_kernel<4, 2><<<grid, GRU_THREADS, 0, st>>>(s);
    } else {
        dim3 grid(s.H / 16, (B + 15) / 16, ndirs);
        if (save) gru_step_kernel<1, 1, true><<<grid, GRU_THREADS, 0, st>>>(s);
        else gru_step_kernel<1, 1><<<grid, GRU_THREADS, 0, st>>>(s);
    }
    return hipGetLastError();
}

}  // namespace laff
