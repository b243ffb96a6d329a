// Input frames widened on the device after they crossed PCIe packed (frameio_in.py is the specification, bit for bit): the inverse
// of svr_frame_pack.hip.  Streaming kernels: no LDS, no atomics, capped grids with a grid-stride loop.
//   unpack_rgb_kernel      rgb8 / bgr8 / rgb16: the clip as ONE flat run of T*H*W*C samples.  A lane owns a whole number of 16-byte
//                          loads -- 16 samples of 8 bits, 8 of 16 bits, 48 for three-channel bgr8 (the smallest run that holds whole
//                          pixels AND whole 16-byte loads) -- and writes them as 16-byte fp32 stores; the samples behind the last
//                          whole unit -- or all of them when a pointer is not 16-byte aligned -- go one by one.
//   unpack_yuv_vec_kernel  yuv420p8 / yuv420p10, W % 16 == 0 and 16-byte aligned pointers: a lane owns 16 x 2 pixels.  It reads two Y
//                          runs of 16 samples and, per chroma plane, the rows cy - 1, cy, cy + 1 (clamped to the plane) over its 8
//                          columns PLUS the first column of the next unit (clamped to the row: the neighbour across the unit seam
//                          that the odd last pixel of the unit interpolates with), and writes 2 x 16 x 3 fp32 as 16-byte stores.
//                          Rows, planes and frames all start on 16 bytes then (8 for the chroma rows of the 8-bit format, whose
//                          8 samples are one 8-byte load).
//   unpack_yuv_kernel      any other geometry: a lane owns one pixel, element accesses.
// Arithmetic: chroma upsampled bilinearly in integers (MPEG-2 siting: co-sited with even luma columns, midway between luma rows;
// weights over 8), the matrix in exact 64-bit integers, ONE fp32 operation at the end: the IEEE division q / D, the fp32 value nearest
// to it (no reciprocal, no fma: hipcc's default keeps fp32 division correctly rounded).  The numerators of the matrix can be negative:
// they are clamped at zero BEFORE the (unsigned) division, which is what the specification's floor division followed by its clamp
// gives.  A sample above 2^n - 1 (possible in the 16-bit container of the 10-bit format) counts as 2^n - 1, so |num| < 6.1e16 < 2^62
// for any input bytes.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"
#include <type_traits>

namespace svr {

SVR_DEVICE float unpack_unit(uint32_t q, float full_scale) { return (float)q / full_scale; }

// BYTES: 1 (full scale 255) / 2 (65535).  C == 0: samples in place; C == 3 / 4: bgr of C-channel pixels (channels 0 and 2 swapped back)
template <int BYTES, int C>
__global__ __launch_bounds__(256) void unpack_rgb_kernel(const void* __restrict__ packed, float* __restrict__ out, int64_t n_units,
                                                         int64_t n) {
    constexpr int U = BYTES == 2 ? 8 : (C == 3 ? 48 : 16), CH = C ? C : 1, LOADS = U * BYTES / 16;
    constexpr float D = BYTES == 2 ? 65535.f : 255.f;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t u = first; u < n_units; u += step) {
        uint32_t w[4 * LOADS];
#pragma unroll
        for (int k = 0; k < LOADS; ++k) {
            const uint4 v = ((const uint4*)packed)[u * LOADS + k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
        float f[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const uint32_t s = BYTES == 1 ? (w[j / 4] >> (8 * (j % 4))) & 0xffu : (w[j / 2] >> (16 * (j % 2))) & 0xffffu;
            const int c = C ? j % CH : 1;                                 // (a unit starts on a pixel: U % C == 0)
            const int d = c == 0 ? j + 2 : c == 2 ? j - 2 : j;            // where sample j lands
            f[d] = unpack_unit(s, D);
        }
#pragma unroll
        for (int k = 0; k < U / 4; ++k)
            ((float4*)out)[u * (U / 4) + k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
    }
    for (int64_t i = n_units * U + first; i < n; i += step) {
        const uint32_t s = BYTES == 1 ? ((const unsigned char*)packed)[i] : ((const unsigned short*)packed)[i];
        const int c = C ? (int)(i % CH) : 1;
        const int64_t d = c == 0 ? i + 2 : c == 2 ? i - 2 : i;
        out[d] = unpack_unit(s, D);
    }
}

struct YuvCoef { int rv, gu, gv, bu; };                   // the matrix scaled by 2^16 (bt709: 103206, 12276, 30679, 121609)

// BITS 8 / 10 (12: svr_planar.hip); PC: full range (y0 = 0, both excursions 2^n - 1) instead of tv (16 / 219 / 224, shifted for 10 bits)
template <int BITS, int PC>
struct YuvFormat {
    static constexpr int MAXV = (1 << BITS) - 1;
    static constexpr int Y0 = PC ? 0 : 16 << (BITS - 8);
    static constexpr int64_t YS = PC ? MAXV : 219 << (BITS - 8);
    static constexpr int64_t CS = PC ? MAXV : 224 << (BITS - 8);
    static constexpr int MID = 8 << (BITS - 1);
    static constexpr int64_t LUMA = 8 * CS * 65536;       // base = (Y - y0) * LUMA
    static constexpr int64_t DEN = YS * LUMA;
    typedef typename std::conditional<BITS == 8, unsigned char, unsigned short>::type sample_t;
};

// q = clamp(floor((2 num + Den) / (2 Den)), 0, 65535) with num = 65535 * s; a numerator <= 0 gives 0 (floor, then the clamp)
template <class F>
SVR_DEVICE uint32_t yuv_q(int64_t s) {
    const int64_t top = 2 * 65535 * s + F::DEN;
    const uint64_t q = top <= 0 ? 0ull : (uint64_t)top / (uint64_t)(2 * F::DEN);
    return (uint32_t)(q < 65535ull ? q : 65535ull);
}
template <class F>
SVR_DEVICE float yuv_code(int64_t s) { return unpack_unit(yuv_q<F>(s), 65535.f); }

// Y a sample, cb8 / cr8 the upsampled chroma over 8
template <class F>
SVR_DEVICE void yuv_pixel(int Y, int cb8, int cr8, const YuvCoef& k, float* rgb) {
    const int64_t base = (int64_t)(Y - F::Y0) * F::LUMA;
    const int u = cb8 - F::MID, v = cr8 - F::MID;
    rgb[0] = yuv_code<F>(base + (int64_t)(k.rv * v) * F::YS);
    rgb[1] = yuv_code<F>(base - (int64_t)(k.gu * u + k.gv * v) * F::YS);
    rgb[2] = yuv_code<F>(base + (int64_t)(k.bu * u) * F::YS);
}

// N consecutive samples (N * sizeof(sample) a multiple of 8, the address aligned to min(16, that)) clamped to the format's maximum
template <class F, int N>
SVR_DEVICE void yuv_load_run(const typename F::sample_t* p, int* v) {
    constexpr int BYTES = sizeof(typename F::sample_t), WORDS = N * BYTES / 4;
    uint32_t w[WORDS];
    if constexpr (WORDS == 2) {
        const uint2 a = *(const uint2*)p;
        w[0] = a.x; w[1] = a.y;
    } else {
#pragma unroll
        for (int k = 0; k < WORDS / 4; ++k) {
            const uint4 a = ((const uint4*)p)[k];
            w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w;
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const uint32_t s = BYTES == 1 ? (w[j / 4] >> (8 * (j % 4))) & 0xffu : (w[j / 2] >> (16 * (j % 2))) & 0xffffu;
        v[j] = (int)min(s, (uint32_t)F::MAXV);
    }
}

template <int BITS, int PC>
__global__ __launch_bounds__(256) void unpack_yuv_vec_kernel(const void* __restrict__ packed, float* __restrict__ out, int T, int H,
                                                             int W, YuvCoef k) {
    typedef YuvFormat<BITS, PC> F;
    typedef typename F::sample_t S;
    const int w16 = W / 16, h2 = (H + 1) / 2, w2 = W / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)h2 * w2, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * h2 * w16;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int sx = (int)(idx % w16), cy = (int)(idx / w16 % h2);
        const int64_t t = idx / w16 / h2;
        const S* f = (const S*)packed + t * frame;
        // the three chroma rows, vertically interpolated in quarters: top[] for luma row 2 cy, bot[] for 2 cy + 1; index 8 is the
        // first column of the next unit, clamped to the row
        const int rows[3] = {max(cy - 1, 0), cy, min(cy + 1, h2 - 1)};
        const int next = min(sx * 8 + 8, w2 - 1);
        int top[2][9], bot[2][9];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const S* c = f + plane + pl * cplane;
            int r[3][9];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                yuv_load_run<F, 8>(c + (int64_t)rows[i] * w2 + sx * 8, r[i]);
                r[i][8] = min((int)c[(int64_t)rows[i] * w2 + next], F::MAXV);
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                top[pl][i] = r[0][i] + 3 * r[1][i];
                bot[pl][i] = 3 * r[1][i] + r[2][i];
            }
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int y = 2 * cy + rr;
            if (y >= H) break;                                            // (odd H: the last chroma row has one luma row)
            int Y[16];
            yuv_load_run<F, 16>(f + (int64_t)y * W + sx * 16, Y);
            float o[48];
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int* vb = rr ? bot[0] : top[0];
                const int* vr = rr ? bot[1] : top[1];
                // even column: twice the vertical value at p / 2; odd: the sum of the values at p / 2 and p / 2 + 1
                const int cb8 = vb[p / 2] + vb[p / 2 + (p & 1)], cr8 = vr[p / 2] + vr[p / 2 + (p & 1)];
                yuv_pixel<F>(Y[p], cb8, cr8, k, o + 3 * p);
            }
            float4* dst = (float4*)(out + ((t * H + y) * W + sx * 16) * 3);
#pragma unroll
            for (int i = 0; i < 12; ++i) dst[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
        }
    }
}

template <int BITS, int PC>
__global__ __launch_bounds__(256) void unpack_yuv_kernel(const void* __restrict__ packed, float* __restrict__ out, int T, int H,
                                                         int W, YuvCoef k) {
    typedef YuvFormat<BITS, PC> F;
    typedef typename F::sample_t S;
    const int h2 = (H + 1) / 2, w2 = (W + 1) / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)h2 * w2, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * plane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int x = (int)(idx % W), y = (int)(idx / W % H);
        const int64_t t = idx / W / H;
        const S* f = (const S*)packed + t * frame;
        const int j = y >> 1, jo = (y & 1) ? min(j + 1, h2 - 1) : max(j - 1, 0);      // the chroma row and the other one, clamped
        const int c0 = x >> 1, c1 = min(c0 + (x & 1), w2 - 1);                        // the column and (odd x) the next, clamped
        int c8[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const S* c = f + plane + pl * cplane;
            auto at = [&](int row, int col) { return min((int)c[(int64_t)row * w2 + col], F::MAXV); };
            c8[pl] = 3 * at(j, c0) + at(jo, c0) + 3 * at(j, c1) + at(jo, c1);
        }
        float rgb[3];
        yuv_pixel<F>(min((int)f[(int64_t)y * W + x], F::MAXV), c8[0], c8[1], k, rgb);
        float* o = out + idx * 3;
        o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
    }
}

}  // namespace svr
