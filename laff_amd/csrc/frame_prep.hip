// frame_prep.hip -- frame preprocessing (laff_frame_preprocess): decoded RGB uint8 frames of any size -> the CLIP image encoder's
// [F, 3, R, R] fp32 pixels.  The reference does this per frame in Python through torchvision on Pillow (model/clip/clip.py:58-65:
// Resize(R, BICUBIC), CenterCrop(R), ToTensor, Normalize; data_provider.py:274-281 the bilinear 'slip' variant).
//
// The resize is Pillow's 8-bit resample, reproduced bit for bit: a horizontal pass whose result is rounded to uint8, then a vertical
// pass on that result, each `out = clip8((sum_i k_i p_i + 2^21) >> 22)` with int32 taps k_i that the host derives in float64 once per
// distinct (in, out, filter).  The device does integer multiply-adds only until the final normalise, so nothing depends on the order
// of a floating-point sum: a frame's output is bitwise the same alone, in any batch and under any row tiling.
//
// One launch, one kernel: block (row tile, frame) computes `tile` output rows of the cropped R x R window.
//   phase 1  the source rows the tile's vertical taps touch, [s0, s1), are filtered horizontally at the cropped width into LDS as
//            uint8 [s1 - s0][R][3] -- the uint8 intermediate of the two passes never reaches HBM; only the columns and rows the
//            window depends on are read;
//   phase 2  the vertical pass over LDS; the uint8 result goes to out_u8 [F, R, R, 3] (optional) and
//            (float(u) / 255.0f - mean_c) / std_c, with true fp32 divides, to out_pixels [F, 3, R, R].
// The tap table of an axis holds the R window entries only: { K, xmin[R], count[R], taps[K][R] } int32 (taps transposed, so a wave
// reading tap i of consecutive outputs reads consecutive words).  An axis Pillow skips (in == out) comes as the identity table
// (one tap of 2^22), which the same arithmetic maps to the source byte exactly.
//
// The host (api.hip) picks `tile` in {16, 8, 4, 2, 1} rows, the largest whose LDS image fits FRAME_PREP_LDS_BYTES for every frame of
// the call, and checks every table entry against the frame's size before the launch: the kernel itself reads only
// [xmin, xmin + count) of a row / column it was given.  Frames are read with byte loads: any byte offset is legal.
#include "kernels.h"

namespace laff {

constexpr int FRAME_PREP_THREADS = 256;

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(FRAME_PREP_THREADS) void frame_prep_kernel(FramePrepArgs a) {
    extern __shared__ unsigned char rows[];      // [s1 - s0][R][3] uint8: the horizontally filtered source rows of this tile
    const int R = a.R, f = blockIdx.y;
    const int y0 = blockIdx.x * a.tile, y1 = min(R, y0 + a.tile);
    const laff_frame_desc d = a.desc[f];
    const int* __restrict__ ht = a.taps + d.htab;
    const int* __restrict__ vt = a.taps + d.vtab;
    const int* __restrict__ hxmin = ht + 1;
    const int* __restrict__ hcnt = ht + 1 + R;
    const int* __restrict__ hk = ht + 1 + 2 * R;
    const int* __restrict__ vxmin = vt + 1;
    const int* __restrict__ vcnt = vt + 1 + R;
    const int* __restrict__ vk = vt + 1 + 2 * R;
    int s0 = vxmin[y0], s1 = s0;
    for (int y = y0; y < y1; ++y) {
        s0 = min(s0, vxmin[y]);
        s1 = max(s1, vxmin[y] + vcnt[y]);
    }
    const int nrows = s1 - s0, row_bytes = 3 * R;
    const unsigned char* __restrict__ src = a.frames + d.offset + (long)s0 * d.width * 3;

    // phase 1: horizontal pass, one (source row, output column) per thread, the three channels together
    for (int o = threadIdx.x; o < nrows * R; o += FRAME_PREP_THREADS) {
        const int r = o / R, x = o - r * R;
        const int xm = hxmin[x], n = hcnt[x];
        const unsigned char* __restrict__ p = src + ((long)r * d.width + xm) * 3;
        int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
        for (int i = 0; i < n; ++i) {
            const int k = hk[i * R + x];
            acc0 += k * (int)p[3 * i];
            acc1 += k * (int)p[3 * i + 1];
            acc2 += k * (int)p[3 * i + 2];
        }
        unsigned char* q = rows + r * row_bytes + 3 * x;
        q[0] = (unsigned char)clip8(acc0 >> 22);
        q[1] = (unsigned char)clip8(acc1 >> 22);
        q[2] = (unsigned char)clip8(acc2 >> 22);
    }
    __syncthreads();

    // phase 2: vertical pass over LDS, lanes along (channel, column) so that the fp32 planes are written in whole lines
    float* __restrict__ out = a.out_pixels + (long)f * 3 * R * R;
    unsigned char* __restrict__ out8 = a.out_u8 ? a.out_u8 + (long)f * 3 * R * R : nullptr;
    for (int o = threadIdx.x; o < (y1 - y0) * row_bytes; o += FRAME_PREP_THREADS) {
        const int yy = o / row_bytes, j = o - yy * row_bytes, y = y0 + yy;
        const int c = j / R, x = j - c * R;
        const int n = vcnt[y];
        const unsigned char* __restrict__ p = rows + (vxmin[y] - s0) * row_bytes + 3 * x + c;
        int acc = 1 << 21;
        for (int i = 0; i < n; ++i) acc += vk[i * R + y] * (int)p[i * row_bytes];
        const int u = clip8(acc >> 22);
        if (out8) out8[((long)y * R + x) * 3 + c] = (unsigned char)u;
        const float m = c == 0 ? a.mean[0] : (c == 1 ? a.mean[1] : a.mean[2]);
        const float sd = c == 0 ? a.stdv[0] : (c == 1 ? a.stdv[1] : a.stdv[2]);
        out[((long)c * R + y) * R + x] = ((float)u / 255.0f - m) / sd;
    }
}

hipError_t launch_frame_prep(const FramePrepArgs& a, size_t lds_bytes, hipStream_t st) {
    const dim3 grid((a.R + a.tile - 1) / a.tile, a.F);
    hipLaunchKernelGGL(frame_prep_kernel, grid, dim3(FRAME_PREP_THREADS), lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace laff
