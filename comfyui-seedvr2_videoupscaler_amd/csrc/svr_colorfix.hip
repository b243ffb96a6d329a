// Colour correction after the decode (colorfix.py is the specification; reference: src/utils/color_fix.py).
//   wavelet_kernel      out = clamp(high5(content) + low5(style), -1, 1): the five a-trous levels of BOTH operands in one launch,
//                       a workgroup per (frame, channel, tile) with the tile + its halo staged in LDS             -> [T, H, W, 3]
//   lab_planes_kernel   two [-1, 1] frame sets -> CIELAB (D65), planar [3, T*H*W] each (what the sort wants)
//   lab_merge_kernel    L = c_L w + m_L (1 - w), matched a, b -> sRGB, clamp, * 2 - 1                              -> [T, H, W, 3]
//   chan_stats_kernel / chan_stats_finish_kernel   per (frame, channel) mean and unbiased variance of content and style: fp64
//                       partial sums in a fixed order (as the GroupNorm statistics)                              -> fp32 [T, 3, 4]
//   adain_apply_kernel  (c - mean_c) / sqrt(var_c + eps) * sqrt(var_s + eps) + mean_s                             -> [T, H, W, 3]
// A pixel operand is fp32 and addressed by four element strides (T, C, H, W), so channels-last frames and a sliced [C, T, H, W]
// buffer are read where they lie.  The pyramid is adds and power-of-two scalings only: the wavelet result equals
// colorfix.wavelet_reconstruction bit for bit.  The colour-space kernels keep torch's operation order (no contraction of a
// multiply with the add that follows it; the 3x3 matrices as the fused-multiply-add chain k = 0, 1, 2 that the CPU's sgemm runs).
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

struct PixStrides { int64_t t, c, h, w; };          // element strides of a [T, 3, H, W]-indexed fp32 operand

constexpr int WAVELET_LEVELS = 5;
constexpr int WAVELET_TILE = 64;                    // output tile edge
constexpr int WAVELET_HALO_MAX = 31;                // 1 + 2 + 4 + 8 + 16
constexpr int WAVELET_REGION = WAVELET_TILE + 2 * WAVELET_HALO_MAX;      // 126
constexpr int WAVELET_PITCH = WAVELET_REGION + 1;                        // 127 floats per LDS row
constexpr int WAVELET_THREADS = 1024;               // 32 x 32 lanes; a 32-lane row of consecutive floats is conflict-free
constexpr int WAVELET_OWN = (WAVELET_TILE / 32) * (WAVELET_TILE / 32);   // tile pixels per thread
constexpr int WAVELET_LDS_BYTES = 2 * WAVELET_REGION * WAVELET_PITCH * (int)sizeof(float);   // two planes, 125 KiB

struct WaveletRadii { int r[WAVELET_LEVELS]; };     // min(2^i, max(1, min(H, W) / 8)): colorfix.wavelet_blur

// One operand's pyramid over the region [ry0, ry1) x [rx0, rx1) of the image (the tile + halo, cut to the image) held in ``a``;
// ``b`` takes the vertical pass.  Region bounds ARE the clamp: on an image border they are the image's (replicate padding of
// every level's own input), elsewhere they only bound what a cell beyond the needed box would read.  Level i computes just the box
// the levels after it still need (the tile + the sum of their radii).  WITH_HIGH: high = (high + image) - low for the thread's
// own tile pixels, kept in registers.  On return ``a`` holds the fifth low-pass for the tile (after a barrier).
template <bool WITH_HIGH>
SVR_DEVICE void wavelet_pyramid(float* __restrict__ a, float* __restrict__ b, const WaveletRadii& radii, int halo,
                                int ty0, int ty1, int tx0, int tx1, int ry0, int ry1, int rx0, int rx1,
                                float (&high)[WAVELET_OWN]) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 31, row = threadIdx.x >> 5;
    float prev[WAVELET_OWN];
    if constexpr (WITH_HIGH) {
#pragma unroll
        for (int k = 0; k < WAVELET_OWN; ++k) {
            const int gy = ty0 + row + 32 * (k >> 1), gx = tx0 + lane + 32 * (k & 1);
            high[k] = 0.f;
            prev[k] = (gy < ty1 && gx < tx1) ? a[(gy - ry0) * WAVELET_PITCH + gx - rx0] : 0.f;
        }
    }
    int after = halo;                                             // sum of the radii of the levels still to come
#pragma unroll 1
    for (int lvl = 0; lvl < WAVELET_LEVELS; ++lvl) {
        const int r = radii.r[lvl];
        after -= r;
        const int by0 = max(ty0 - after, ry0), by1 = min(ty1 + after, ry1);
        const int hx0 = max(tx0 - after, rx0), hx1 = min(tx1 + after, rx1);
        const int vx0 = max(hx0 - r, rx0), vx1 = min(hx1 + r, rx1);
        for (int gy = by0 + row; gy < by1; gy += 32) {            // rows y - r, y, y + r
            const int yl = max(gy - r, ry0) - ry0, yh = min(gy + r, ry1 - 1) - ry0, yc = gy - ry0;
            for (int gx = vx0 + lane; gx < vx1; gx += 32) {
                const int x = gx - rx0;
                const float s = a[yl * WAVELET_PITCH + x] + a[yh * WAVELET_PITCH + x];
                b[yc * WAVELET_PITCH + x] = s * 0.25f + 0.5f * a[yc * WAVELET_PITCH + x];
            }
        }
        __syncthreads();
        for (int gy = by0 + row; gy < by1; gy += 32) {            // columns x - r, x, x + r of that result
            const float* v = b + (gy - ry0) * WAVELET_PITCH;
            for (int gx = hx0 + lane; gx < hx1; gx += 32) {
                const int xl = max(gx - r, rx0) - rx0, xh = min(gx + r, rx1 - 1) - rx0, xc = gx - rx0;
                const float s = v[xl] + v[xh];
                a[(gy - ry0) * WAVELET_PITCH + xc] = s * 0.25f + 0.5f * v[xc];
            }
        }
        __syncthreads();
        if constexpr (WITH_HIGH) {
#pragma unroll
            for (int k = 0; k < WAVELET_OWN; ++k) {
                const int gy = ty0 + row + 32 * (k >> 1), gx = tx0 + lane + 32 * (k & 1);
                if (gy < ty1 && gx < tx1) {
                    const float low = a[(gy - ry0) * WAVELET_PITCH + gx - rx0];
                    high[k] = (high[k] + prev[k]) - low;
                    prev[k] = low;
                }
            }
        }
    }
}

SVR_DEVICE void wavelet_stage(float* __restrict__ a, const float* __restrict__ src, PixStrides s, int t, int c,
                              int ry0, int ry1, int rx0, int rx1) {
    const int lane = threadIdx.x & 31, row = threadIdx.x >> 5;
    const float* plane = src + (int64_t)t * s.t + (int64_t)c * s.c;
    for (int gy = ry0 + row; gy < ry1; gy += 32)
        for (int gx = rx0 + lane; gx < rx1; gx += 32)
            a[(gy - ry0) * WAVELET_PITCH + gx - rx0] = plane[(int64_t)gy * s.h + (int64_t)gx * s.w];
}

__global__ __launch_bounds__(WAVELET_THREADS) void wavelet_kernel(const float* __restrict__ content, PixStrides cs,
                                                                  const float* __restrict__ style, PixStrides ss,
                                                                  float* __restrict__ out, PixStrides os, int H, int W,
                                                                  WaveletRadii radii, int halo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* a = (float*)smem;
    float* b = a + WAVELET_REGION * WAVELET_PITCH;
    const int t = blockIdx.z / 3, c = blockIdx.z % 3;
    const int tx0 = blockIdx.x * WAVELET_TILE, ty0 = blockIdx.y * WAVELET_TILE;
    const int tx1 = min(tx0 + WAVELET_TILE, W), ty1 = min(ty0 + WAVELET_TILE, H);
    const int rx0 = max(tx0 - halo, 0), rx1 = min(tx1 + halo, W), ry0 = max(ty0 - halo, 0), ry1 = min(ty1 + halo, H);
    float high[WAVELET_OWN], unused[WAVELET_OWN];
    wavelet_stage(a, content, cs, t, c, ry0, ry1, rx0, rx1);
    __syncthreads();
    wavelet_pyramid<true>(a, b, radii, halo, ty0, ty1, tx0, tx1, ry0, ry1, rx0, rx1, high);
    __syncthreads();                                              // the last own-pixel reads of ``a`` before it is refilled
    wavelet_stage(a, style, ss, t, c, ry0, ry1, rx0, rx1);
    __syncthreads();
    wavelet_pyramid<false>(a, b, radii, halo, ty0, ty1, tx0, tx1, ry0, ry1, rx0, rx1, unused);
    const int lane = threadIdx.x & 31, row = threadIdx.x >> 5;
    float* dst = out + (int64_t)t * os.t + (int64_t)c * os.c;
#pragma unroll
    for (int k = 0; k < WAVELET_OWN; ++k) {
        const int gy = ty0 + row + 32 * (k >> 1), gx = tx0 + lane + 32 * (k & 1);
        if (gy < ty1 && gx < tx1) {
            const float v = high[k] + a[(gy - ry0) * WAVELET_PITCH + gx - rx0];
            dst[(int64_t)gy * os.h + (int64_t)gx * os.w] = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);      // (a NaN stays one)
        }
    }
}

// ---- CIELAB <-> sRGB, the operation order of colorfix.rgb_to_lab / lab_to_rgb ------------------------------------------------
constexpr float LAB_EPS = (float)(6.0 / 29.0);
constexpr float LAB_EPS3 = (float)((6.0 / 29.0) * (6.0 / 29.0) * (6.0 / 29.0));
constexpr float LAB_KAPPA = (float)((29.0 / 3.0) * (29.0 / 3.0) * (29.0 / 3.0));

// one row of ``x @ m.T``: the fp32 fused-multiply-add chain over k = 0, 1, 2 (what the CPU's sgemm computes for these shapes)
SVR_DEVICE float mix_row(float x0, float x1, float x2, float m0, float m1, float m2) {
    return fmaf(x2, m2, fmaf(x1, m1, x0 * m0));
}

SVR_DEVICE void rgb_to_lab_px(const float (&x)[3], float (&lab)[3]) {
#pragma clang fp contract(off)
    float lin[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = (x[c] + 1.0f) * 0.5f;                           // [-1, 1] -> [0, 1]
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        lin[c] = v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f;
    }
    float xyz[3];
    xyz[0] = mix_row(lin[0], lin[1], lin[2], 0.4124564f, 0.3575761f, 0.1804375f) / 0.95047f;
    xyz[1] = mix_row(lin[0], lin[1], lin[2], 0.2126729f, 0.7151522f, 0.0721750f);
    xyz[2] = mix_row(lin[0], lin[1], lin[2], 0.0193339f, 0.1191920f, 0.9503041f) / 1.08883f;
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        f[c] = xyz[c] > LAB_EPS3 ? powf(xyz[c], (float)(1.0 / 3.0)) : (xyz[c] * LAB_KAPPA + 16.0f) / 116.0f;
    lab[0] = f[1] * 116.0f - 16.0f;
    lab[1] = (f[0] - f[1]) * 500.0f;
    lab[2] = (f[1] - f[2]) * 200.0f;
}

SVR_DEVICE float lab_finv(float f) {
#pragma clang fp contract(off)
    return f > LAB_EPS ? f * f * f : (f * 116.0f - 16.0f) / LAB_KAPPA;
}

SVR_DEVICE void lab_to_rgb_px(float L, float A, float B, float (&rgb)[3]) {
#pragma clang fp contract(off)
    const float fy = (L + 16.0f) / 116.0f;
    const float fx = A / 500.0f + fy;
    const float fz = fy - B / 200.0f;
    const float X = lab_finv(fx) * 0.95047f, Y = lab_finv(fy), Z = lab_finv(fz) * 1.08883f;
    float lin[3];
    lin[0] = mix_row(X, Y, Z, 3.2404542f, -1.5371385f, -0.4985314f);
    lin[1] = mix_row(X, Y, Z, -0.9692660f, 1.8760108f, 0.0415560f);
    lin[2] = mix_row(X, Y, Z, 0.0556434f, -0.2040259f, 1.0572252f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = lin[c] > 0.0031308f ? powf(lin[c] < 0.f ? 0.f : lin[c], (float)(1.0 / 2.4)) * 1.055f - 0.055f : lin[c] * 12.92f;
        rgb[c] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    }
}

constexpr int COLORFIX_ROW_PIXELS = 256;            // pixels of one image row per workgroup of the streaming kernels

// blockIdx.x = (frame * H + row) * chunks + chunk of 256 pixels; blockIdx.y = operand (0: base -> c_lab, 1: style -> s_lab)
__global__ __launch_bounds__(COLORFIX_ROW_PIXELS) void lab_planes_kernel(const float* __restrict__ base, PixStrides bs,
                                                                         const float* __restrict__ style, PixStrides ss,
                                                                         float* __restrict__ c_lab, float* __restrict__ s_lab,
                                                                         int H, int W, int chunks, int64_t plane) {
    const int64_t line = blockIdx.x / chunks;
    const int x = (int)(blockIdx.x % chunks) * COLORFIX_ROW_PIXELS + threadIdx.x;
    if (x >= W) return;
    const int t = (int)(line / H), y = (int)(line % H);
    const bool second = blockIdx.y != 0;
    const float* src = second ? style : base;
    const PixStrides s = second ? ss : bs;
    float* dst = second ? s_lab : c_lab;
    const float* px = src + (int64_t)t * s.t + (int64_t)y * s.h + (int64_t)x * s.w;
    const float rgb[3] = {px[0], px[s.c], px[2 * s.c]};
    float lab[3];
    rgb_to_lab_px(rgb, lab);
    const int64_t i = line * W + x;
    dst[i] = lab[0]; dst[plane + i] = lab[1]; dst[2 * plane + i] = lab[2];
}

__global__ __launch_bounds__(COLORFIX_ROW_PIXELS) void lab_merge_kernel(const float* __restrict__ c_L, const float* __restrict__ m_L,
                                                                        const float* __restrict__ m_a, const float* __restrict__ m_b,
                                                                        float w, float one_minus_w, float* __restrict__ out,
                                                                        PixStrides os, int H, int W, int chunks) {
#pragma clang fp contract(off)
    const int64_t line = blockIdx.x / chunks;
    const int x = (int)(blockIdx.x % chunks) * COLORFIX_ROW_PIXELS + threadIdx.x;
    if (x >= W) return;
    const int t = (int)(line / H), y = (int)(line % H);
    const int64_t i = line * W + x;
    float L = c_L[i];
    if (m_L) L = L * w + m_L[i] * one_minus_w;
    float rgb[3];
    lab_to_rgb_px(L, m_a[i], m_b[i], rgb);
    float* px = out + (int64_t)t * os.t + (int64_t)y * os.h + (int64_t)x * os.w;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c * os.c] = rgb[c] * 2.0f - 1.0f;
}

// ---- AdaIN ----------------------------------------------------------------------------------------------------------------------
constexpr int CHAN_STATS_PARTS = 64;                // partial sums per (operand, frame, channel); part p takes rows p, p + 64, ...

// grid (parts, T * 3, 2 operands); partial[((operand * T * 3 + frame * 3 + channel) * parts + part) * 2 + {sum, sum of squares}]
__global__ __launch_bounds__(256) void chan_stats_kernel(const float* __restrict__ content, PixStrides cs,
                                                         const float* __restrict__ style, PixStrides ss, int H, int W,
                                                         double* __restrict__ partial) {
    __shared__ double red_s[256], red_q[256];
    const int t = blockIdx.y / 3, c = blockIdx.y % 3;
    const float* src = blockIdx.z ? style : content;
    const PixStrides s = blockIdx.z ? ss : cs;
    const float* plane = src + (int64_t)t * s.t + (int64_t)c * s.c;
    double sum = 0.0, sq = 0.0;
    for (int y = blockIdx.x; y < H; y += CHAN_STATS_PARTS)
        for (int x = threadIdx.x; x < W; x += 256) {
            const double v = (double)plane[(int64_t)y * s.h + (int64_t)x * s.w];
            sum += v; sq += v * v;
        }
    red_s[threadIdx.x] = sum; red_q[threadIdx.x] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                           // a fixed tree: the same bits on every run
        if ((int)threadIdx.x < o) { red_s[threadIdx.x] += red_s[threadIdx.x + o]; red_q[threadIdx.x] += red_q[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* p = partial + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * CHAN_STATS_PARTS + blockIdx.x) * 2;
        p[0] = red_s[0]; p[1] = red_q[0];
    }
}

// stats[(frame * 3 + channel) * 4 + {mean_c, var_c, mean_s, var_s}] (fp32; the variance unbiased: n - 1)
__global__ __launch_bounds__(256) void chan_stats_finish_kernel(const double* __restrict__ partial, int planes, double n,
                                                                float* __restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;                 // operand * planes + plane
    if (i >= 2 * planes) return;
    const double* p = partial + (int64_t)i * CHAN_STATS_PARTS * 2;
    double sum = 0.0, sq = 0.0;
    for (int k = 0; k < CHAN_STATS_PARTS; ++k) { sum += p[2 * k]; sq += p[2 * k + 1]; }
    const double mean = sum / n;
    float* o = stats + (int64_t)(i % planes) * 4 + (i / planes) * 2;
    o[0] = (float)mean;
    o[1] = (float)((sq - sum * mean) / (n - 1.0));
}

__global__ __launch_bounds__(COLORFIX_ROW_PIXELS) void adain_apply_kernel(const float* __restrict__ content, PixStrides cs,
                                                                          const float* __restrict__ stats, float eps,
                                                                          float* __restrict__ out, PixStrides os, int H, int W,
                                                                          int chunks) {
#pragma clang fp contract(off)
    const int64_t line = blockIdx.x / chunks;
    const int x = (int)(blockIdx.x % chunks) * COLORFIX_ROW_PIXELS + threadIdx.x;
    if (x >= W) return;
    const int t = (int)(line / H), y = (int)(line % H);
    const float* src = content + (int64_t)t * cs.t + (int64_t)y * cs.h + (int64_t)x * cs.w;
    float* dst = out + (int64_t)t * os.t + (int64_t)y * os.h + (int64_t)x * os.w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* st = stats + ((int64_t)t * 3 + c) * 4;
        const float c_std = sqrtf(st[1] + eps), s_std = sqrtf(st[3] + eps);
        dst[c * os.c] = (src[c * cs.c] - st[0]) / c_std * s_std + st[2];
    }
}

}  // namespace svr
