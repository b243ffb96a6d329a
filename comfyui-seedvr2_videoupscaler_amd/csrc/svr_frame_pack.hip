// Output frames narrowed on the device before they cross PCIe (frameio.py is the specification, bit for bit).
// Streaming kernels: no LDS, no atomics, capped grids with a grid-stride loop.
//   pack8_kernel        rgb8 / bgr8: the clip as ONE flat run of T*H*W*C samples, so a frame start never breaks alignment.  A lane
//                       owns a unit of 16 samples (48 for three-channel bgr8: the smallest run that holds whole pixels AND whole
//                       16-byte stores), read as 16-byte loads and written as 16-byte stores; the samples behind the last whole
//                       unit -- or all of them when a pointer is not 16-byte aligned -- go one by one.
// yuv420p10 has no kernel of its own here: svr_frame_pack_colour.hip's pair, run with the BT.709 limited-range coefficients and
// centre-sited chroma, writes it for svr_pack_frames as for svr_pack_yuv420p10.  It builds on pack_load, pack_load_run, pack_code
// and YUV_D below.
// Arithmetic: q = rint(clamp(x, 0, 1) * full_scale) in fp32 -- fmaxf(NaN, 0) = 0, so NaN becomes code 0.
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

// 8-bit BT.709 luma of the 8-bit codes, weights rounded at 2^16 (shots.luma8): what cut detection and the active area look at
SVR_DEVICE uint32_t luma8(float r, float g, float b) {
    return (13933u * pack_code(r, 255.f) + 46871u * pack_code(g, 255.f) + 4732u * pack_code(b, 255.f) + 32768u) >> 16;
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

constexpr uint64_t YUV_D = 65535ull * 65536ull;      // the yuv420p10 divisor: 16-bit codes times the matrix scale 2^16

}  // namespace svr
