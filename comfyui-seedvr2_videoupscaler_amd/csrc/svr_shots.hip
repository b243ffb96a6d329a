// Frame signatures for cut detection (shots.py is the specification, bit for bit): per frame a 4 x 4 grid of 64-bin histograms of
// the 8-bit BT.709 luma, int32 [T, 1024] indexed [cell_row * 4 + cell_col][Y8 >> 2].
//   signature_kernel    one workgroup per (frame, band): a band is SIG_BAND_ROWS consecutive pixel rows of ONE cell row (the last band
//                       of a cell row is shorter; a cell row of fewer rows leaves its later bands empty), so a workgroup counts into
//                       4 cell columns x 64 bins = 256 counters.  The band is one dense run of rows * W pixels: a lane owns a unit
//                       of 8 pixels (24 or 32 samples: whole pixels AND whole 16-byte loads in fp32 and in bf16), units placed on
//                       multiples of 8 pixels of the CLIP so that every one starts on 16 bytes; the pixels in front of the band's
//                       first unit and behind its last -- or all of them when the clip's pointer is not 16-byte aligned -- go one by
//                       one.  Counts go into one LDS histogram per wave (ds_add_u32), the four are summed and the non-zero counters
//                       added to the signature with integer global atomics: integer adds commute, two runs give the same bits.
// Contention: a flat frame (letterbox bars, black frames, fades) sends every lane of a wave to ONE counter, which the LDS would
// serialise 64 ways.  signature_count therefore asks first whether the wave's active lanes all hold the same key -- one
// v_readfirstlane, one compare, two ballots -- and then lets the first of them add the lane count once; only a wave that holds
// different keys issues per-lane adds.  Waves never share a histogram, so the worst left is one wave's own spread of keys.
// Arithmetic: q = rint(clamp(x, 0, 1) * 255) in fp32 (pack_code: fmaxf(NaN, 0) = 0), Y8 = (13933 r + 46871 g + 4732 b + 32768) >> 16
// in 32 unsigned bits (at most 255 * 65536 + 32768).  Cell column of x: the number of k in 1..3 with x >= ceil(k W / 4), which is
// (x * 4) / W without the division.  H * W < 2^31 (the host refuses more: the counters are int32), so pixel indices inside a
// band fit 32 bits; the band's place in the clip is 64-bit.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

constexpr int SIG_BAND_ROWS = 16;                    // 16 x 1280 pixels = 80 per lane at 720p; 45 bands per cell row and frame
constexpr int SIG_UNIT = 8;                          // pixels per lane and step on the 16-byte route

SVR_DEVICE uint32_t signature_bin(float r, float g, float b) { return luma8(r, g, b) >> 2; }

// one count for ``key`` in this wave's histogram; call with any set of active lanes
SVR_DEVICE void signature_count(int* hist, uint32_t key) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
    const uint64_t active = __ballot(1), same = __ballot(key == first);
    if (same == active) {                                                       // (wave-uniform branch)
        if ((int)__lane_id() == __ffsll((unsigned long long)active) - 1) atomicAdd(hist + first, __popcll(active));
    } else {
        atomicAdd(hist + key, 1);
    }
}

template <int KIND, int C>                           // SVR_STORE_FP32 / SVR_STORE_BF16; C = 3 or 4 samples per pixel
__global__ __launch_bounds__(256) void signature_kernel(const void* __restrict__ frames, int* __restrict__ sig, int H, int W,
                                                        int bands, int vec) {
    __shared__ int hist[4][256];                     // [wave][cell_col * 64 + bin]
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t t = blockIdx.x / (4 * bands);
    const int b = (int)(blockIdx.x % (4 * bands)), cell_row = b / bands, band = b % bands;
    const int64_t y0 = ((int64_t)cell_row * H + 3) / 4 + (int64_t)band * SIG_BAND_ROWS;       // first pixel row of the band
    const int64_t y_end = ((int64_t)(cell_row + 1) * H + 3) / 4;                              // one past the cell row's last
    if (y0 >= y_end) return;                                                                  // (whole workgroup)
    const int rows = (int)(y_end - y0 < SIG_BAND_ROWS ? y_end - y0 : SIG_BAND_ROWS);
    const int n = rows * W;                                                                   // <= H * W < 2^31
    const int64_t g0 = (t * H + y0) * W;                                                      // the band's first pixel in the clip
    const int c1 = (int)(((int64_t)W + 3) / 4), c2 = (int)((2 * (int64_t)W + 3) / 4), c3 = (int)((3 * (int64_t)W + 3) / 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[k][tid] = 0;
    __syncthreads();
    int* mine = hist[wave];
    // [0, head) one by one, then n_units units, then the rest one by one
    int head = vec ? (int)((SIG_UNIT - g0 % SIG_UNIT) % SIG_UNIT) : n;
    if (head > n) head = n;
    const int n_units = (n - head) / SIG_UNIT;
    for (int u = tid; u < n_units; u += 256) {
        const int p = head + u * SIG_UNIT;
        float v[SIG_UNIT * C];
        pack_load_run<KIND, SIG_UNIT * C>(frames, (g0 + p) * C, v);
        int x = p % W;
#pragma unroll
        for (int j = 0; j < SIG_UNIT; ++j) {
            const int col = (x >= c1) + (x >= c2) + (x >= c3);
            signature_count(mine, (uint32_t)col * 64u + signature_bin(v[j * C], v[j * C + 1], v[j * C + 2]));
            if (++x == W) x = 0;
        }
    }
    const int tail0 = head + n_units * SIG_UNIT;
    for (int i = tid; i < head + (n - tail0); i += 256) {
        const int p = i < head ? i : tail0 + (i - head);
        const int64_t e = (g0 + p) * C;
        const int x = p % W;
        const int col = (x >= c1) + (x >= c2) + (x >= c3);
        signature_count(mine, (uint32_t)col * 64u + signature_bin(pack_load<KIND>(frames, e), pack_load<KIND>(frames, e + 1),
                                                                   pack_load<KIND>(frames, e + 2)));
    }
    __syncthreads();
    const int total = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
    if (total) atomicAdd(sig + t * 1024 + cell_row * 256 + tid, total);                       // t < T, cell_row < 4, tid < 256
}

}  // namespace svr
