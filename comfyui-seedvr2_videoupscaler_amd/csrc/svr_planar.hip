// Planar YUV -- 4:2:0 / 4:2:2 / 4:4:4 at 8 / 10 / 12 bits -- turned into 16-bit RGB codes (uint16 [T, H, W, 3]: svr_unpack_frames'
// SVR_UNPACK_RGB16 input) on the device, after the planes crossed PCIe as they are stored (planar.py is the specification, bit for
// bit).  Streaming kernels in svr_frame_unpack.hip's idiom, whose YuvFormat, yuv_load_run and yuv_q they share: no LDS, no atomics,
// capped grids with a grid-stride loop, 64-bit indices for anything multiplied by T.
//   planar_vec_kernel   W % 16 == 0 and 16-byte aligned pointers: a lane owns 16 pixels of one row (4:2:2, 4:4:4) or 16 x 2 pixels
//                       (4:2:0, as unpack_yuv_vec_kernel).  It reads Y as 16-sample runs and, per chroma plane and chroma row it
//                       needs, 8 samples PLUS the first column of the next unit, clamped to the row (the neighbour across the unit
//                       seam that the odd last pixel interpolates with) -- 4:4:4: 16 samples and no neighbour -- and writes per row
//                       16 x 3 uint16 = 96 bytes as six 16-byte stores.  Rows, planes and frames all start on 16 bytes then (8 for
//                       the 8-sample chroma runs of the 8-bit formats, which are one 8-byte load).
//   planar_kernel       any other geometry: a lane owns one pixel, element accesses.
// SUB 0 / 1 / 2 = 4:2:0 / 4:2:2 / 4:4:4 (SVR_PLANAR_*); TOPLEFT (4:2:0 only): chroma co-sited with even luma rows instead of midway
// between them.  The vertical value V is in quarters (weights (1, 3) / (3, 1), TOPLEFT (4, 0) / (2, 2), 4:2:2 and 4:4:4: 4 C[y]);
// horizontally an even column (and every 4:4:4 column) takes 2 V, an odd one the sum of its two neighbours: weights over 8.
// Arithmetic: samples clamped to 2^n - 1 AS THEY ARE LOADED, so |cb8 - mid| <= 2^(n+2) and the 32-bit products of yuv_codes
// (123299 * 16384 < 2^31 at 12 bits, bt2020) cannot overflow; the matrix in exact 64-bit integers (2 * 65535 * |s| + Den < 2^61),
// clamped at zero BEFORE the unsigned division.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

// Y a sample, cb8 / cr8 the upsampled chroma over 8 -> three 16-bit codes
template <class F>
SVR_DEVICE void planar_pixel(int Y, int cb8, int cr8, const YuvCoef& k, uint32_t* rgb) {
    const int64_t base = (int64_t)(Y - F::Y0) * F::LUMA;
    const int u = cb8 - F::MID, v = cr8 - F::MID;
    rgb[0] = yuv_q<F>(base + (int64_t)(k.rv * v) * F::YS);
    rgb[1] = yuv_q<F>(base - (int64_t)(k.gu * u + k.gv * v) * F::YS);
    rgb[2] = yuv_q<F>(base + (int64_t)(k.bu * u) * F::YS);
}

// 16 pixels of one row: Y[16], per plane the vertical values v[pl][..] (4:4:4: 16 of them; else 8 and the seam neighbour) -> 96 bytes
template <class F, int SUB>
SVR_DEVICE void planar_store_run(const int* Y, const int* vb, const int* vr, const YuvCoef& k, unsigned short* out) {
    uint32_t o[48];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        int cb8, cr8;
        if constexpr (SUB == SVR_PLANAR_444) {
            cb8 = 2 * vb[p]; cr8 = 2 * vr[p];
        } else {                                                            // even column: twice the value at p / 2; odd: the sum of the two
            cb8 = vb[p / 2] + vb[p / 2 + (p & 1)]; cr8 = vr[p / 2] + vr[p / 2 + (p & 1)];
        }
        planar_pixel<F>(Y[p], cb8, cr8, k, o + 3 * p);
    }
    uint4* dst = (uint4*)out;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        dst[i] = make_uint4(o[8 * i] | o[8 * i + 1] << 16, o[8 * i + 2] | o[8 * i + 3] << 16, o[8 * i + 4] | o[8 * i + 5] << 16,
                            o[8 * i + 6] | o[8 * i + 7] << 16);
}

template <int SUB, int BITS, int PC, int TOPLEFT>
__global__ __launch_bounds__(256) void planar_vec_kernel(const void* __restrict__ planes, unsigned short* __restrict__ out, int T, int H,
                                                         int W, YuvCoef k) {
    typedef YuvFormat<BITS, PC> F;
    typedef typename F::sample_t S;
    constexpr bool V420 = SUB == SVR_PLANAR_420;
    constexpr int NV = SUB == SVR_PLANAR_444 ? 16 : 9;                      // vertical values a unit needs per plane and row
    const int w16 = W / 16, hc = V420 ? (H + 1) / 2 : H, wc = SUB == SVR_PLANAR_444 ? W : W / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)hc * wc, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * hc * w16;                            // (4:2:0: one unit per chroma row; else one per luma row)
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int sx = (int)(idx % w16), cy = (int)(idx / w16 % hc);
        const int64_t t = idx / w16 / hc;
        const S* f = (const S*)planes + t * frame;
        // one chroma row's run for this unit: the samples, and (subsampled columns) the first column of the next unit, clamped
        auto load = [&](const S* c, int row, int* r) {
            if constexpr (SUB == SVR_PLANAR_444) {
                yuv_load_run<F, 16>(c + (int64_t)row * wc + sx * 16, r);
            } else {
                yuv_load_run<F, 8>(c + (int64_t)row * wc + sx * 8, r);
                r[8] = min((int)c[(int64_t)row * wc + min(sx * 8 + 8, wc - 1)], F::MAXV);
            }
        };
        int top[2][NV], bot[2][NV];                                         // V for luma row 2 cy and 2 cy + 1 (4:2:0), or for row cy
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const S* c = f + plane + pl * cplane;
            int r1[NV];
            load(c, cy, r1);
            if constexpr (!V420) {
#pragma unroll
                for (int i = 0; i < NV; ++i) top[pl][i] = 4 * r1[i];
            } else if constexpr (TOPLEFT) {
                int r2[NV];
                load(c, min(cy + 1, hc - 1), r2);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    top[pl][i] = 4 * r1[i];
                    bot[pl][i] = 2 * r1[i] + 2 * r2[i];
                }
            } else {
                int r0[NV], r2[NV];
                load(c, max(cy - 1, 0), r0);
                load(c, min(cy + 1, hc - 1), r2);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    top[pl][i] = r0[i] + 3 * r1[i];
                    bot[pl][i] = 3 * r1[i] + r2[i];
                }
            }
        }
#pragma unroll
        for (int rr = 0; rr < (V420 ? 2 : 1); ++rr) {
            const int y = V420 ? 2 * cy + rr : cy;
            if (y >= H) break;                                              // (odd H: the last chroma row has one luma row)
            int Y[16];
            yuv_load_run<F, 16>(f + (int64_t)y * W + sx * 16, Y);
            planar_store_run<F, SUB>(Y, rr ? bot[0] : top[0], rr ? bot[1] : top[1], k, out + ((t * H + y) * W + sx * 16) * 3);
        }
    }
}

template <int SUB, int BITS, int PC, int TOPLEFT>
__global__ __launch_bounds__(256) void planar_kernel(const void* __restrict__ planes, unsigned short* __restrict__ out, int T, int H, int W,
                                                     YuvCoef k) {
    typedef YuvFormat<BITS, PC> F;
    typedef typename F::sample_t S;
    constexpr bool V420 = SUB == SVR_PLANAR_420;
    const int hc = V420 ? (H + 1) / 2 : H, wc = SUB == SVR_PLANAR_444 ? W : (W + 1) / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)hc * wc, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * plane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int x = (int)(idx % W), y = (int)(idx / W % H);
        const int64_t t = idx / W / H;
        const S* f = (const S*)planes + t * frame;
        // the two chroma rows and their weights in quarters, clamped; the column and (odd x of a subsampled row) the next, clamped
        int j, jo, wj, wo;
        if constexpr (!V420) { j = jo = y; wj = wo = 2; }
        else if constexpr (TOPLEFT) { j = y >> 1; jo = min(j + (y & 1), hc - 1); wj = wo = 2; }
        else { j = y >> 1; jo = (y & 1) ? min(j + 1, hc - 1) : max(j - 1, 0); wj = 3; wo = 1; }
        const int c0 = SUB == SVR_PLANAR_444 ? x : x >> 1, c1 = SUB == SVR_PLANAR_444 ? x : min(c0 + (x & 1), wc - 1);
        int c8[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const S* c = f + plane + pl * cplane;
            auto at = [&](int row, int col) { return min((int)c[(int64_t)row * wc + col], F::MAXV); };
            c8[pl] = wj * at(j, c0) + wo * at(jo, c0) + wj * at(j, c1) + wo * at(jo, c1);
        }
        uint32_t rgb[3];
        planar_pixel<F>(min((int)f[(int64_t)y * W + x], F::MAXV), c8[0], c8[1], k, rgb);
        unsigned short* o = out + idx * 3;
        o[0] = (unsigned short)rgb[0]; o[1] = (unsigned short)rgb[1]; o[2] = (unsigned short)rgb[2];
    }
}

}  // namespace svr
