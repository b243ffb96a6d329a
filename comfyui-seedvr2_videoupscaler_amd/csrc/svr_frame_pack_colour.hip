// The yuv420p10 writer, behind both entry points: svr_pack_yuv420p10 with a choice of matrix, range and chroma siting
// (frameio.pack_yuv420p10_torch is the specification, bit for bit: what an HDR (BT.2020) source is written with), and
// svr_pack_frames' SVR_PACK_YUV420P10 with BT.709, limited range, centre siting (frameio.pack_frames_torch, an independent
// statement of the same integers).  Two shapes, svr_frame_pack.hip's streaming rules (no LDS, no atomics, capped grids with a
// grid-stride loop, no cross-lane traffic) and its pack_load, pack_load_run, pack_code and YUV_D:
//   pack_colour_vec_kernel  W % 16 == 0 and 16-byte aligned pointers: a lane owns 16 x 2 pixels = two Y runs of 32 bytes and 8 + 8
//                           chroma samples, every access of its own run 16 bytes (rows, planes and frames all start on 16 bytes then).
//   pack_colour_kernel      any other geometry: a lane owns one chroma sample and its 2 x 2 pixels, element accesses (a Y row
//                           starts 2 * W bytes after the previous one: off 16 bytes whenever W % 8 != 0).
// Matrix and range arrive as integers in PackCoef (as the unpack's YuvCoef); the siting is a template parameter:
//   LEFT = false  chroma from the 2 x 2 block, weights 1: S = 4.
//   LEFT = true   columns 2k-1, 2k, 2k+1 with weights 1, 2, 1 over the two rows: S = 8.  Column 2k-1 of a lane's FIRST chroma sample
//                 lies one pixel to the left of its run: the lane loads that pixel itself (three elements per row, 1/16 more loads,
//                 from a line its left neighbour streams anyway), so nothing depends on which lane, wave or workgroup holds the
//                 neighbouring run; at column 0 the index clamps to the lane's own first pixel.
// Arithmetic: q = rint(clamp(x, 0, 1) * 65535) in fp32 (NaN -> 0), then exact integers: every numerator is positive and below 2^62,
// so unsigned division is the specification's floor division.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

struct PackCoef { int y0, ys, cs, wr, wg, wb, cb_r, cb_g, cr_g, cr_b; };   // range (10 bits) and the matrix scaled by 2^16

SVR_DEVICE uint32_t colour_luma(int r, int g, int b, const PackCoef& k) {
    // (the weights sum to 65536: the weighted sum is at most 65536 * 65535 < 2^32)
    const uint32_t s = (uint32_t)k.wr * (uint32_t)r + (uint32_t)k.wg * (uint32_t)g + (uint32_t)k.wb * (uint32_t)b;
    return (uint32_t)k.y0 + (uint32_t)(((uint64_t)(uint32_t)k.ys * s + YUV_D / 2) / YUV_D);
}
// m: the chroma row applied to the weighted sums of codes (total weight S); half = 512, top = 1023
template <int S>
SVR_DEVICE uint32_t colour_chroma(int64_t m, int cs) {
    const uint64_t num = (uint64_t)((int64_t)((uint64_t)S * 512ull * YUV_D + (uint64_t)S * (YUV_D / 2)) + (int64_t)cs * m);
    const uint32_t c = (uint32_t)(num / ((uint64_t)S * YUV_D));
    return c < 1023u ? c : 1023u;
}
template <int S>
SVR_DEVICE uint32_t colour_cb(int sr, int sg, int sb, const PackCoef& k) {
    return colour_chroma<S>(k.cb_r * (int64_t)sr + k.cb_g * (int64_t)sg + 32768 * (int64_t)sb, k.cs);
}
template <int S>
SVR_DEVICE uint32_t colour_cr(int sr, int sg, int sb, const PackCoef& k) {
    return colour_chroma<S>(32768 * (int64_t)sr + k.cr_g * (int64_t)sg + k.cr_b * (int64_t)sb, k.cs);
}

template <int KIND, bool LEFT>
__global__ __launch_bounds__(256) void pack_colour_vec_kernel(const void* __restrict__ x, unsigned short* __restrict__ out, int T,
                                                              int H, int W, PackCoef k) {
    constexpr int S = LEFT ? 8 : 4;
    const int w16 = W / 16, h2 = (H + 1) / 2, w2 = W / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)h2 * w2, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * h2 * w16;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int sx = (int)(idx % w16), cy = (int)(idx / w16 % h2);
        const int64_t t = idx / w16 / h2;
        int sr[8], sg[8], sb[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) sr[c] = sg[c] = sb[c] = 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int y = min(2 * cy + rr, H - 1);                        // (the row beyond an odd H repeats the last one)
            const int64_t row = (t * H + y) * W;
            float v[48];
            pack_load_run<KIND, 48>(x, (row + sx * 16) * 3, v);
            if constexpr (LEFT) {                                         // column 2k-1 of the run's first chroma sample
                const int64_t e = (row + max(sx * 16 - 1, 0)) * 3;
                sr[0] += (int)pack_code(pack_load<KIND>(x, e), 65535.f);
                sg[0] += (int)pack_code(pack_load<KIND>(x, e + 1), 65535.f);
                sb[0] += (int)pack_code(pack_load<KIND>(x, e + 2), 65535.f);
            }
            uint32_t yw[8];
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int r = (int)pack_code(v[3 * p], 65535.f), g = (int)pack_code(v[3 * p + 1], 65535.f),
                          b = (int)pack_code(v[3 * p + 2], 65535.f);
                if constexpr (LEFT) {
                    const int wgt = (p & 1) ? 1 : 2;                      // column 2k twice, 2k+1 once ...
                    sr[p / 2] += wgt * r; sg[p / 2] += wgt * g; sb[p / 2] += wgt * b;
                    if ((p & 1) && p < 15) { sr[p / 2 + 1] += r; sg[p / 2 + 1] += g; sb[p / 2 + 1] += b; }   // ... and as the next one's 2k-1
                } else {
                    sr[p / 2] += r; sg[p / 2] += g; sb[p / 2] += b;
                }
                const uint32_t Y = colour_luma(r, g, b, k);
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
        for (int c = 0; c < 4; ++c) {
            cb[c] = colour_cb<S>(sr[2 * c], sg[2 * c], sb[2 * c], k) | (colour_cb<S>(sr[2 * c + 1], sg[2 * c + 1], sb[2 * c + 1], k) << 16);
            cr[c] = colour_cr<S>(sr[2 * c], sg[2 * c], sb[2 * c], k) | (colour_cr<S>(sr[2 * c + 1], sg[2 * c + 1], sb[2 * c + 1], k) << 16);
        }
        unsigned short* c0 = out + t * frame + plane + (int64_t)cy * w2 + sx * 8;
        *(uint4*)c0 = make_uint4(cb[0], cb[1], cb[2], cb[3]);
        *(uint4*)(c0 + cplane) = make_uint4(cr[0], cr[1], cr[2], cr[3]);
    }
}

template <int KIND, bool LEFT>
__global__ __launch_bounds__(256) void pack_colour_kernel(const void* __restrict__ x, unsigned short* __restrict__ out, int T, int H,
                                                          int W, PackCoef k) {
    constexpr int S = LEFT ? 8 : 4;
    const int h2 = (H + 1) / 2, w2 = (W + 1) / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)h2 * w2, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * cplane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int cx = (int)(idx % w2), cy = (int)(idx / w2 % h2);
        const int64_t t = idx / w2 / h2;
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int y = min(2 * cy + rr, H - 1);                        // (beyond the frame: the last row / column)
            const int64_t row = (t * H + y) * W;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int xx = min(2 * cx + cc, W - 1);
                const int64_t px = row + xx;
                const int r = (int)pack_code(pack_load<KIND>(x, px * 3), 65535.f), g = (int)pack_code(pack_load<KIND>(x, px * 3 + 1), 65535.f),
                          b = (int)pack_code(pack_load<KIND>(x, px * 3 + 2), 65535.f);
                const int wgt = LEFT && cc == 0 ? 2 : 1;
                sr += wgt * r; sg += wgt * g; sb += wgt * b;
                if (2 * cy + rr < H && 2 * cx + cc < W) out[t * frame + (int64_t)y * W + xx] = (unsigned short)colour_luma(r, g, b, k);
            }
            if constexpr (LEFT) {                                         // column 2k-1, clamped to the frame
                const int64_t e = (row + max(2 * cx - 1, 0)) * 3;
                sr += (int)pack_code(pack_load<KIND>(x, e), 65535.f);
                sg += (int)pack_code(pack_load<KIND>(x, e + 1), 65535.f);
                sb += (int)pack_code(pack_load<KIND>(x, e + 2), 65535.f);
            }
        }
        unsigned short* c0 = out + t * frame + plane + (int64_t)cy * w2 + cx;
        c0[0] = (unsigned short)colour_cb<S>(sr, sg, sb, k);
        c0[cplane] = (unsigned short)colour_cr<S>(sr, sg, sb, k);
    }
}

}  // namespace svr
