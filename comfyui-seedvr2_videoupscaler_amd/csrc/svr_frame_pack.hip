// Output frames narrowed on the device before they cross PCIe (frameio.py is the specification, bit for bit).
// Streaming kernels: no LDS, no atomics, capped grids with a grid-stride loop.
//   pack8_kernel        rgb8 / bgr8: the clip as ONE flat run of T*H*W*C samples, so a frame start never breaks alignment.  A lane
//                       owns a unit of 16 samples (48 for three-channel bgr8: the smallest run that holds whole pixels AND whole
//                       16-byte stores), read as 16-byte loads and written as 16-byte stores; the samples behind the last whole
//                       unit -- or all of them when a pointer is not 16-byte aligned -- go one by one.
//   pack_yuv_vec_kernel yuv420p10, W % 16 == 0 and 16-byte aligned pointers: a lane owns 16 x 2 pixels = two Y runs of 32 bytes and
//                       8 + 8 chroma samples, every access 16 bytes (rows, planes and frames all start on 16 bytes then).
//   pack_yuv_kernel     yuv420p10, any other geometry: a lane owns one chroma sample and its 2 x 2 pixels, element accesses (a Y
//                       row starts 2 * W bytes after the previous one: off 16 bytes whenever W % 8 != 0).
// Arithmetic: q = rint(clamp(x, 0, 1) * full_scale) in fp32 -- fmaxf(NaN, 0) = 0, so NaN becomes code 0 --, BT.709 limited range
// in exact 64-bit integers (every numerator positive and below 2^62: unsigned division = the specification's floor division).
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

template <int KIND>                                  // SVR_STORE_FP32 / SVR_STORE_BF16
SVR_DEVICE float pack_load(const void* p, int64_t i) {
    if constexpr (KIND == SVR_STORE_FP32) return ((const float*)p)[i];
    else return bf2f(((const bf16_t*)p)[i]);
}

// N consecutive samples (N % 8 == 0) from element index e (16-byte aligned address) as 16-byte loads
template <int KIND, int N>
SVR_DEVICE void pack_load_run(const void* p, int64_t e, float* v) {
#pragma unroll
    for (int k = 0; k < N / 8; ++k) load8<KIND>(p, e + 8 * k, v + 8 * k);
}

SVR_DEVICE uint32_t pack_code(float x, float full_scale) {
    return (uint32_t)__builtin_rintf(fminf(fmaxf(x, 0.f), 1.f) * full_scale);
}

// C == 0: rgb8 (samples in place); C == 3 / 4: bgr8 of C-channel pixels (channels 0 and 2 swapped, a fourth in place)
template <int KIND, int C>
__global__ __launch_bounds__(256) void pack8_kernel(const void* __restrict__ x, unsigned char* __restrict__ out, int64_t n_units,
                                                    int64_t n) {
    constexpr int U = C == 3 ? 48 : 16, CH = C ? C : 1;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t u = first; u < n_units; u += step) {
        float v[U];
        pack_load_run<KIND, U>(x, u * U, v);
        uint32_t w[U / 4];
#pragma unroll
        for (int k = 0; k < U / 4; ++k) w[k] = 0;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int c = C ? j % CH : 1;                                 // (a unit starts on a pixel: U % C == 0)
            const int d = c == 0 ? j + 2 : c == 2 ? j - 2 : j;            // where sample j lands
            w[d / 4] |= pack_code(v[j], 255.f) << (8 * (d % 4));
        }
#pragma unroll
        for (int k = 0; k < U / 16; ++k)
            *(uint4*)(out + u * U + 16 * k) = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
    for (int64_t i = n_units * U + first; i < n; i += step) {
        const int c = C ? (int)(i % CH) : 1;
        const int64_t d = c == 0 ? i + 2 : c == 2 ? i - 2 : i;
        out[d] = (unsigned char)pack_code(pack_load<KIND>(x, i), 255.f);
    }
}

constexpr uint64_t YUV_D = 65535ull * 65536ull;
SVR_DEVICE uint32_t yuv_luma(int r, int g, int b) {
    return 64u + (uint32_t)((876ull * (uint64_t)(13933 * (int64_t)r + 46871 * (int64_t)g + 4732 * (int64_t)b) + YUV_D / 2) / YUV_D);
}
// sr, sg, sb: the sums of the 2 x 2 block's codes
SVR_DEVICE uint32_t yuv_cb(int sr, int sg, int sb) {
    const int64_t m = -7509 * (int64_t)sr - 25259 * (int64_t)sg + 32768 * (int64_t)sb;
    return (uint32_t)((uint64_t)((int64_t)(2050ull * YUV_D) + 896 * m) / (4 * YUV_D));
}
SVR_DEVICE uint32_t yuv_cr(int sr, int sg, int sb) {
    const int64_t m = 32768 * (int64_t)sr - 29763 * (int64_t)sg - 3005 * (int64_t)sb;
    return (uint32_t)((uint64_t)((int64_t)(2050ull * YUV_D) + 896 * m) / (4 * YUV_D));
}

template <int KIND>
__global__ __launch_bounds__(256) void pack_yuv_vec_kernel(const void* __restrict__ x, unsigned short* __restrict__ out, int T, int H,
                                                           int W) {
    const int w16 = W / 16, h2 = (H + 1) / 2, w2 = W / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)h2 * w2, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * h2 * w16;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int sx = (int)(idx % w16), cy = (int)(idx / w16 % h2);
        const int64_t t = idx / w16 / h2;
        int sr[8], sg[8], sb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) sr[k] = sg[k] = sb[k] = 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int y = min(2 * cy + rr, H - 1);                        // (the row beyond an odd H repeats the last one)
            float v[48];
            pack_load_run<KIND, 48>(x, ((t * H + y) * W + sx * 16) * 3, v);
            uint32_t yw[8];
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int r = (int)pack_code(v[3 * p], 65535.f), g = (int)pack_code(v[3 * p + 1], 65535.f),
                          b = (int)pack_code(v[3 * p + 2], 65535.f);
                sr[p / 2] += r; sg[p / 2] += g; sb[p / 2] += b;
                const uint32_t Y = yuv_luma(r, g, b);
                yw[p / 2] = (p & 1) ? (yw[p / 2] | (Y << 16)) : Y;
            }
            if (2 * cy + rr < H) {
                uint4* dst = (uint4*)(out + t * frame + (int64_t)y * W + sx * 16);
                dst[0] = make_uint4(yw[0], yw[1], yw[2], yw[3]);
                dst[1] = make_uint4(yw[4], yw[5], yw[6], yw[7]);
            }
        }
        uint32_t cb[4], cr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cb[k] = yuv_cb(sr[2 * k], sg[2 * k], sb[2 * k]) | (yuv_cb(sr[2 * k + 1], sg[2 * k + 1], sb[2 * k + 1]) << 16);
            cr[k] = yuv_cr(sr[2 * k], sg[2 * k], sb[2 * k]) | (yuv_cr(sr[2 * k + 1], sg[2 * k + 1], sb[2 * k + 1]) << 16);
        }
        unsigned short* c0 = out + t * frame + plane + (int64_t)cy * w2 + sx * 8;
        *(uint4*)c0 = make_uint4(cb[0], cb[1], cb[2], cb[3]);
        *(uint4*)(c0 + cplane) = make_uint4(cr[0], cr[1], cr[2], cr[3]);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void pack_yuv_kernel(const void* __restrict__ x, unsigned short* __restrict__ out, int T, int H,
                                                       int W) {
    const int h2 = (H + 1) / 2, w2 = (W + 1) / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)h2 * w2, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * cplane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int cx = (int)(idx % w2), cy = (int)(idx / w2 % h2);
        const int64_t t = idx / w2 / h2;
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int y = min(2 * cy + rr, H - 1), xx = min(2 * cx + cc, W - 1);   // (beyond the frame: the last row / column)
                const int64_t px = (t * H + y) * W + xx;
                const int r = (int)pack_code(pack_load<KIND>(x, px * 3), 65535.f), g = (int)pack_code(pack_load<KIND>(x, px * 3 + 1), 65535.f),
                          b = (int)pack_code(pack_load<KIND>(x, px * 3 + 2), 65535.f);
                sr += r; sg += g; sb += b;
                if (2 * cy + rr < H && 2 * cx + cc < W) out[t * frame + (int64_t)y * W + xx] = (unsigned short)yuv_luma(r, g, b);
            }
        unsigned short* c0 = out + t * frame + plane + (int64_t)cy * w2 + cx;
        c0[0] = (unsigned short)yuv_cb(sr, sg, sb);
        c0[cplane] = (unsigned short)yuv_cr(sr, sg, sb);
    }
}

}  // namespace svr
