// The HSV half of the colour correction (colorfix.hsv_spec / wavelet_adaptive_spec / hue_match_spec are the specification).
//   hsv_planes_kernel      two [-1, 1] frame sets -> ((x + 1) * 0.5) clamped -> colorfix.rgb_to_hsv: content h, s, v and style h, s
//                          as dense planes [T*H*W] (what the partition and the sort want).  Every operation in torch's order, IEEE
//                          divisions, nothing contracted: the planes equal the CPU run bit for bit.
//   hue-conditional rank matching (svr_hue_match in svr_api.hip), from svr_rank.hip's kernels and one of this file's:
//     a stable partition of (saturation key, flat index) by hue class: ONE radix pass whose digit is the class (rank_hist_kernel /
//     rank_scan_kernel / rank_scatter_kernel with DIGIT = 1), source with indices, reference keys only.  The classes of bin 0
//     (h >= 1, [0, e_1), [e_11, 1)) are digits 0..2, so the reference's bin 0 is one run; the source's bin 0 must stand in the order
//     of the plane (ties go to the lower flat index), which a second partition gives (DIGIT = 2: inside bin 0 first).  The class
//     counts are the scan's totals; the host reads them once and sorts only the bins that qualify, each as the four-pass sort over
//     its run (the runs are read, never written: bins 0 and 11 share pixels), then
//   hue_apply_kernel       out[index[k]] = sorted_reference[(k * (n_r - 1)) / (n_s - 1)] in 64-bit integers: the exact nearest rank.
//   hsv_merge_kernel       colorfix.hsv_to_rgb(h, sat, v) in its operation order, clamped to [0, 1], * 2 - 1        -> [T, H, W, 3]
//   adaptive_blend_kernel  the same HSV pixel blended into the wavelet base: w = sigmoid(sharpness * (sat(content) - sat(style) -
//                          threshold)) where sat(base) - sat(style) > threshold / 2, else 0; out = base * (1 - w) + hsv * w.  The
//                          saturation maps and the mask are exact operations (bit-equal to the CPU's); the sigmoid's expf is not.
// Operand conventions are svr_colorfix.hip's: pixels fp32 by four element strides, planes dense fp32.  Plain vector stores only.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

// ((x + 1) * 0.5).clamp(0, 1)
SVR_DEVICE float hsv_unit(float x) {
#pragma clang fp contract(off)
    const float v = (x + 1.0f) * 0.5f;
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

// colorfix.rgb_to_hsv of one pixel already in [0, 1].  remainder(q, 6) for q in [-1, 1] is q < 0 ? q + 6 : q (-0.0 stays -0.0).
SVR_DEVICE void rgb_to_hsv_px(float r, float g, float b, float& h, float& s, float& v) {
#pragma clang fp contract(off)
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const float rng = maxc - minc;
    const bool colour = rng > 1e-10f;
    const float d = colour ? rng : 1.0f;
    float hh = 0.f;
    if (maxc == r && colour) { const float q = (g - b) / d; hh = q < 0.f ? q + 6.0f : q; }
    if (maxc == g && colour) hh = (b - r) / d + 2.0f;             // the three wheres in order: ties resolve blue > green > red
    if (maxc == b && colour) hh = (r - g) / d + 4.0f;
    s = maxc > 1e-10f ? rng / fmaxf(maxc, 1e-10f) : 0.f;
    h = hh / 6.0f;
    v = maxc;
}

// colorfix.saturation_map of one [-1, 1] pixel (the s of rgb_to_hsv)
SVR_DEVICE float saturation_px(float x0, float x1, float x2) {
#pragma clang fp contract(off)
    const float r = hsv_unit(x0), g = hsv_unit(x1), b = hsv_unit(x2);
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    return maxc > 1e-10f ? (maxc - minc) / fmaxf(maxc, 1e-10f) : 0.f;
}

// colorfix.hsv_to_rgb of one pixel, then clamp(0, 1) * 2 - 1
SVR_DEVICE void hsv_to_pixel(float h, float s, float v, float (&px)[3]) {
#pragma clang fp contract(off)
    const float h6 = h * 6.0f, fl = floorf(h6);
    int sector = (int)((long long)fl % 6);
    if (sector < 0) sector += 6;                                  // torch's % on integers takes the divisor's sign
    const float f = h6 - fl;
    const float p = v * (1.0f - s), q = v * (1.0f - s * f), t = v * (1.0f - s * (1.0f - f));
    float r, g, b;
    switch (sector) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
    const float rgb[3] = {r, g, b};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = rgb[c] < 0.f ? 0.f : (rgb[c] > 1.f ? 1.f : rgb[c]);
        px[c] = x * 2.0f - 1.0f;
    }
}

// blockIdx.x = (frame * H + row) * chunks + chunk of 256 pixels; blockIdx.y = operand (0: content -> h, s, v; 1: style -> h, s)
__global__ __launch_bounds__(COLORFIX_ROW_PIXELS) void hsv_planes_kernel(const float* __restrict__ content, PixStrides cs,
                                                                         const float* __restrict__ style, PixStrides ss,
                                                                         float* __restrict__ c_hsv, float* __restrict__ s_hs,
                                                                         int H, int W, int chunks, int64_t plane) {
    const int64_t line = blockIdx.x / chunks;
    const int x = (int)(blockIdx.x % chunks) * COLORFIX_ROW_PIXELS + threadIdx.x;
    if (x >= W) return;
    const int t = (int)(line / H), y = (int)(line % H);
    const bool second = blockIdx.y != 0;
    const float* src = second ? style : content;
    const PixStrides s = second ? ss : cs;
    const float* px = src + (int64_t)t * s.t + (int64_t)y * s.h + (int64_t)x * s.w;
    float h, sat, v;
    rgb_to_hsv_px(hsv_unit(px[0]), hsv_unit(px[s.c]), hsv_unit(px[2 * s.c]), h, sat, v);
    const int64_t i = line * W + x;
    if (second) {
        s_hs[i] = h; s_hs[plane + i] = sat;
    } else {
        c_hsv[i] = h; c_hsv[plane + i] = sat; c_hsv[2 * plane + i] = v;
    }
}

// out[index[k]] = ref[(k * (n_r - 1)) / (n_s - 1)], n_s >= 2: colorfix.nearest_rank_index.  The quotient is at most n_r - 1.
__global__ __launch_bounds__(256) void hue_apply_kernel(const uint32_t* __restrict__ index, const uint32_t* __restrict__ ref,
                                                        uint32_t n_s, uint32_t n_r, uint32_t* out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_s) return;
    const uint64_t q = (uint64_t)k * (uint64_t)(n_r - 1u) / (uint64_t)(n_s - 1u);
    out[index[k]] = ref[q];
}

__global__ __launch_bounds__(COLORFIX_ROW_PIXELS) void hsv_merge_kernel(const float* __restrict__ h, const float* __restrict__ sat,
                                                                        const float* __restrict__ v, float* __restrict__ out,
                                                                        PixStrides os, int H, int W, int chunks) {
    const int64_t line = blockIdx.x / chunks;
    const int x = (int)(blockIdx.x % chunks) * COLORFIX_ROW_PIXELS + threadIdx.x;
    if (x >= W) return;
    const int t = (int)(line / H), y = (int)(line % H);
    const int64_t i = line * W + x;
    float rgb[3];
    hsv_to_pixel(h[i], sat[i], v[i], rgb);
    float* px = out + (int64_t)t * os.t + (int64_t)y * os.h + (int64_t)x * os.w;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c * os.c] = rgb[c];
}

// thr, half_thr, sharp: threshold, threshold * 0.5 (the product in double) and sharpness, each rounded to fp32 once, as torch rounds
// the Python scalars
__global__ __launch_bounds__(COLORFIX_ROW_PIXELS) void adaptive_blend_kernel(const float* __restrict__ base, PixStrides bs,
                                                                             const float* __restrict__ content, PixStrides cs,
                                                                             const float* __restrict__ style, PixStrides ss,
                                                                             const float* __restrict__ h, const float* __restrict__ sat,
                                                                             const float* __restrict__ v, float thr, float half_thr,
                                                                             float sharp, float* __restrict__ out, PixStrides os,
                                                                             int H, int W, int chunks) {
#pragma clang fp contract(off)
    const int64_t line = blockIdx.x / chunks;
    const int x = (int)(blockIdx.x % chunks) * COLORFIX_ROW_PIXELS + threadIdx.x;
    if (x >= W) return;
    const int t = (int)(line / H), y = (int)(line % H);
    const int64_t i = line * W + x;
    const float* bp = base + (int64_t)t * bs.t + (int64_t)y * bs.h + (int64_t)x * bs.w;
    const float* cp = content + (int64_t)t * cs.t + (int64_t)y * cs.h + (int64_t)x * cs.w;
    const float* sp = style + (int64_t)t * ss.t + (int64_t)y * ss.h + (int64_t)x * ss.w;
    const float b3[3] = {bp[0], bp[bs.c], bp[2 * bs.c]};
    const float s_sat = saturation_px(sp[0], sp[ss.c], sp[2 * ss.c]);
    const float c_sat = saturation_px(cp[0], cp[cs.c], cp[2 * cs.c]);
    const float b_sat = saturation_px(b3[0], b3[1], b3[2]);
    const float arg = sharp * ((c_sat - s_sat) - thr);
    float w = 1.0f / (1.0f + expf(0.0f - arg));
    w = w * ((b_sat - s_sat) > half_thr ? 1.0f : 0.0f);
    w = w < 0.f ? 0.f : (w > 1.f ? 1.f : w);
    float hsv[3];
    hsv_to_pixel(h[i], sat[i], v[i], hsv);
    float* px = out + (int64_t)t * os.t + (int64_t)y * os.h + (int64_t)x * os.w;
    const float keep = 1.0f - w;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c * os.c] = b3[c] * keep + hsv[c] * w;
}

}  // namespace svr
