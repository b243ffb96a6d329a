// Output frames written as planar YUV for the encoder: 4:2:0, 4:2:2 or 4:4:4 at 8, 10 or 12 bits, with a choice of matrix, range and
// chroma siting -- svr_pack_planar (planar_out.pack_planar_torch is the specification, bit for bit), the mirror image of
// svr_planar.hip.  Two shapes per instance, svr_frame_pack.hip's streaming rules (no LDS, no atomics, capped grids with a grid-stride
// loop, 64-bit element indices, no cross-lane traffic) and its pack_load, pack_load_run, pack_code and YUV_D; colour_luma is
// svr_frame_pack_colour.hip's, planar_chroma its colour_chroma with half and top as arguments:
//   planar_out_vec_kernel  W % 16 == 0 and 16-byte aligned pointers: a lane owns a run of 16 pixels by the rows of ONE chroma sample
//                          (1 row for 4:2:2 / 4:4:4, 2 for 4:2:0).  Every store of its own run is the widest its bytes allow: a Y row
//                          is 16 bytes (8 bits) or 2 x 16 bytes; the chroma of a run is 16 samples for 4:4:4 (16 or 2 x 16 bytes) and
//                          8 samples otherwise -- 16 bytes at 10 / 12 bits, ONE 8-byte store at 8 bits (rows, planes and frames all
//                          start on 8 bytes then: wc = W / 2 is a multiple of 8).
//   planar_out_kernel      any other geometry: a lane owns one chroma sample and the pixels under it, element accesses.
// Template parameters: KIND (fp32 / bf16 frames), SUB, SIT and WIDE (uint16 samples: 10 and 12 bits; uint8 otherwise).  Matrix, range
// and depth arrive as integers in PlanarOutCoef (y0, ys, cs, half, top and the matrix at 2^16), as PackCoef does.
//   SIT 0 "center"   chroma from the block under the sample, weights 1.
//   SIT 1 "left"     columns 2k-1, 2k, 2k+1 with weights 1, 2, 1.  Column 2k-1 of a lane's FIRST chroma sample lies one pixel to the
//                    left of its run: the lane loads that pixel itself (three elements per row), as pack_colour_vec_kernel does, so
//                    nothing depends on which lane, wave or workgroup holds the neighbouring run; at column 0 the index clamps.
//                    (4:4:4 is SIT 1 with nothing to site: column x alone.)
//   SIT 2 "topleft"  (4:2:0 only) "left", and rows 2j-1, 2j, 2j+1 with weights 1, 2, 1.  Row 2j-1 belongs to the lane above: this lane
//                    reads it itself -- a THIRD row, 1.5 x the loads of "left" (from lines the neighbouring lane streams anyway: L2
//                    serves most of them; profiles/planar_out.txt has the price).  At row 0 the index clamps to row 0.
// What goes wrong here:
//   * registers: the vector shape holds 48 floats of one row plus 3 x 8 (3 x 16 for 4:4:4) integer sums; the rows are taken one after
//     the other so only one is live.  No instance may spill (tests/test_kernel_resources.py looks at every kernel of the library).
//   * the clamp at top is needed at every depth: in "pc" range a saturated blue reaches 2^n.  The sums reach 16 * 65535, well inside
//     32 bits; ys * s reaches 2^44 and cs * m 2^47: both stay in 64 bits.  Every numerator is positive and below 2^62
//     (planar_out.numerator_bounds), so the unsigned division is the specification's floor division.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

struct PlanarOutCoef { PackCoef k; int half, top; };   // k.y0, k.ys, k.cs at the depth of half and top

// m: the chroma row applied to the weighted sums of codes (total weight S)
SVR_DEVICE uint32_t planar_chroma(int64_t m, int S, const PlanarOutCoef& c) {
    const uint64_t num = (uint64_t)((int64_t)((uint64_t)S * (uint64_t)c.half * YUV_D + (uint64_t)S * (YUV_D / 2)) + (int64_t)c.k.cs * m);
    const uint32_t q = (uint32_t)(num / ((uint64_t)S * YUV_D));
    return q < (uint32_t)c.top ? q : (uint32_t)c.top;
}
SVR_DEVICE uint32_t planar_cb(int sr, int sg, int sb, int S, const PlanarOutCoef& c) {
    return planar_chroma(c.k.cb_r * (int64_t)sr + c.k.cb_g * (int64_t)sg + 32768 * (int64_t)sb, S, c);
}
SVR_DEVICE uint32_t planar_cr(int sr, int sg, int sb, int S, const PlanarOutCoef& c) {
    return planar_chroma(32768 * (int64_t)sr + c.k.cr_g * (int64_t)sg + c.k.cr_b * (int64_t)sb, S, c);
}

// total weight of one chroma sample's taps
template <int SUB, int SIT>
constexpr int planar_out_weight() {
    return (SUB != SVR_PLANAR_420 ? 1 : SIT == 2 ? 4 : 2) * (SUB == SVR_PLANAR_444 ? 1 : SIT == 0 ? 2 : 4);
}

// N samples (N = 8 or 16) at element index e of a plane of uint8 / uint16, the address aligned to the bytes of the run
template <bool WIDE, int N>
SVR_DEVICE void planar_out_store(void* out, int64_t e, const uint32_t* q) {
    if constexpr (WIDE) {
        uint4* dst = (uint4*)((unsigned short*)out + e);
#pragma unroll
        for (int k = 0; k < N / 8; ++k)
            dst[k] = make_uint4(q[8 * k] | (q[8 * k + 1] << 16), q[8 * k + 2] | (q[8 * k + 3] << 16), q[8 * k + 4] | (q[8 * k + 5] << 16),
                                q[8 * k + 6] | (q[8 * k + 7] << 16));
    } else {
        uint32_t w[N / 4];
#pragma unroll
        for (int k = 0; k < N / 4; ++k) w[k] = q[4 * k] | (q[4 * k + 1] << 8) | (q[4 * k + 2] << 16) | (q[4 * k + 3] << 24);
        if constexpr (N == 16) *(uint4*)((unsigned char*)out + e) = make_uint4(w[0], w[1], w[2], w[3]);
        else *(uint2*)((unsigned char*)out + e) = make_uint2(w[0], w[1]);
    }
}
template <bool WIDE>
SVR_DEVICE void planar_out_store1(void* out, int64_t e, uint32_t q) {
    if constexpr (WIDE) ((unsigned short*)out)[e] = (unsigned short)q;
    else ((unsigned char*)out)[e] = (unsigned char)q;
}

template <int KIND, int SUB, int SIT, bool WIDE>
__global__ __launch_bounds__(256) void planar_out_vec_kernel(const void* __restrict__ x, void* __restrict__ out, int T, int H, int W,
                                                             PlanarOutCoef c) {
    constexpr bool V2 = SUB == SVR_PLANAR_420, FULL = SUB == SVR_PLANAR_444, LEFT = !FULL && SIT != 0, TOP = V2 && SIT == 2;
    constexpr int S = planar_out_weight<SUB, SIT>(), NC = FULL ? 16 : 8, ROWS = TOP ? 3 : V2 ? 2 : 1;
    const int w16 = W / 16, hc = V2 ? (H + 1) / 2 : H, wc = FULL ? W : W / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)hc * wc, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * hc * w16;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int sx = (int)(idx % w16), cy = (int)(idx / w16 % hc);
        const int64_t t = idx / w16 / hc;
        int sr[NC], sg[NC], sb[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n) sr[n] = sg[n] = sb[n] = 0;
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int dy = TOP ? rr - 1 : rr;                             // TOP: rows 2j-1, 2j, 2j+1 with weights 1, 2, 1
            const int vw = TOP && rr == 1 ? 2 : 1;
            const int y0 = (V2 ? 2 * cy : cy) + dy;
            const int y = min(max(y0, 0), H - 1);                         // (the row above row 0 and beyond an odd H: the nearest one)
            const int64_t row = (t * H + y) * W;
            float v[48];
            pack_load_run<KIND, 48>(x, (row + sx * 16) * 3, v);
            if constexpr (LEFT) {                                         // column 2k-1 of the run's first chroma sample
                const int64_t e = (row + max(sx * 16 - 1, 0)) * 3;
                sr[0] += vw * (int)pack_code(pack_load<KIND>(x, e), 65535.f);
                sg[0] += vw * (int)pack_code(pack_load<KIND>(x, e + 1), 65535.f);
                sb[0] += vw * (int)pack_code(pack_load<KIND>(x, e + 2), 65535.f);
            }
            uint32_t yq[16];
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int r = (int)pack_code(v[3 * p], 65535.f), g = (int)pack_code(v[3 * p + 1], 65535.f),
                          b = (int)pack_code(v[3 * p + 2], 65535.f);
                if constexpr (FULL) {
                    sr[p] += r; sg[p] += g; sb[p] += b;
                } else if constexpr (LEFT) {
                    const int wgt = vw * ((p & 1) ? 1 : 2);               // column 2k twice, 2k+1 once ...
                    sr[p / 2] += wgt * r; sg[p / 2] += wgt * g; sb[p / 2] += wgt * b;
                    if ((p & 1) && p < 15) { sr[p / 2 + 1] += vw * r; sg[p / 2 + 1] += vw * g; sb[p / 2 + 1] += vw * b; }   // ... and as the next one's 2k-1
                } else {
                    sr[p / 2] += vw * r; sg[p / 2] += vw * g; sb[p / 2] += vw * b;
                }
                yq[p] = colour_luma(r, g, b, c.k);
            }
            if (dy >= 0 && y0 < H) planar_out_store<WIDE, 16>(out, t * frame + (int64_t)y * W + sx * 16, yq);   // (its own rows only)
        }
        uint32_t cb[NC], cr[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            cb[n] = planar_cb(sr[n], sg[n], sb[n], S, c);
            cr[n] = planar_cr(sr[n], sg[n], sb[n], S, c);
        }
        const int64_t c0 = t * frame + plane + (int64_t)cy * wc + sx * NC;
        planar_out_store<WIDE, NC>(out, c0, cb);
        planar_out_store<WIDE, NC>(out, c0 + cplane, cr);
    }
}

template <int KIND, int SUB, int SIT, bool WIDE>
__global__ __launch_bounds__(256) void planar_out_kernel(const void* __restrict__ x, void* __restrict__ out, int T, int H, int W,
                                                         PlanarOutCoef c) {
    constexpr bool V2 = SUB == SVR_PLANAR_420, FULL = SUB == SVR_PLANAR_444, LEFT = !FULL && SIT != 0, TOP = V2 && SIT == 2;
    constexpr int S = planar_out_weight<SUB, SIT>(), ROWS = TOP ? 3 : V2 ? 2 : 1, COLS = FULL ? 1 : LEFT ? 3 : 2;
    const int hc = V2 ? (H + 1) / 2 : H, wc = FULL ? W : (W + 1) / 2;
    const int64_t plane = (int64_t)H * W, cplane = (int64_t)hc * wc, frame = plane + 2 * cplane;
    const int64_t total = (int64_t)T * cplane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int cx = (int)(idx % wc), cy = (int)(idx / wc % hc);
        const int64_t t = idx / wc / hc;
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int dy = TOP ? rr - 1 : rr;
            const int vw = TOP && rr == 1 ? 2 : 1;
            const int y0 = (V2 ? 2 * cy : cy) + dy;
            const int y = min(max(y0, 0), H - 1);                         // (beyond the frame: the nearest row / column)
            const int64_t row = (t * H + y) * W;
#pragma unroll
            for (int cc = 0; cc < COLS; ++cc) {
                const int dx = LEFT ? cc - 1 : cc;                        // LEFT: columns 2k-1, 2k, 2k+1 with weights 1, 2, 1
                const int hw = LEFT && cc == 1 ? 2 : 1;
                const int x0 = (FULL ? cx : 2 * cx) + dx;
                const int xx = min(max(x0, 0), W - 1);
                const int64_t e = (row + xx) * 3;
                const int r = (int)pack_code(pack_load<KIND>(x, e), 65535.f), g = (int)pack_code(pack_load<KIND>(x, e + 1), 65535.f),
                          b = (int)pack_code(pack_load<KIND>(x, e + 2), 65535.f);
                sr += vw * hw * r; sg += vw * hw * g; sb += vw * hw * b;
                if (dy >= 0 && y0 < H && dx >= 0 && x0 < W)               // (the pixels under the sample are this lane's to write)
                    planar_out_store1<WIDE>(out, t * frame + (int64_t)y * W + xx, colour_luma(r, g, b, c.k));
            }
        }
        const int64_t c0 = t * frame + plane + (int64_t)cy * wc + cx;
        planar_out_store1<WIDE>(out, c0, planar_cb(sr, sg, sb, S, c));
        planar_out_store1<WIDE>(out, c0 + cplane, planar_cr(sr, sg, sb, S, c));
    }
}

}  // namespace svr
