// Active-area profile of a clip (active.py is the specification, bit for bit): int32 [H + W], entry y < H the number of pixels of row y
// over ALL frames whose 8-bit BT.709 luma exceeds ``dark``, entry H + x the same for column x.
//   active_profile_kernel   one workgroup per (frame, band): a band is ACT_BAND_ROWS consecutive pixel rows of one frame (the last band
//                           of a frame is shorter), one dense run of rows * W pixels, walked as svr_shots.hip walks its bands: a lane
//                           owns a unit of 8 pixels (24 or 32 samples: whole pixels AND whole 16-byte loads in fp32 and in bf16),
//                           units placed on multiples of 8 pixels of the CLIP so that every one starts on 16 bytes; the pixels in
//                           front of the band's first unit and behind its last -- or all of them when the clip's pointer is not
//                           16-byte aligned -- go one by one.  Counts go into LDS: one counter per row of the band and one per
//                           column below ACT_LDS_COLS (a lane sums a unit's pixels of one row in a register first); the rare column
//                           at or beyond ACT_LDS_COLS is counted straight in global memory.  After a barrier the non-zero counters
//                           are added to the profile with integer global atomics: integer adds commute, two runs give the same bits.
// A pixel with Y8 <= dark adds nothing anywhere: flat bars, black frames and fades cost no LDS traffic and no global atomics, so
// the contention case of svr_shots.hip (every lane of a wave on one counter) does not arise for them.
// Arithmetic: Y8 as in svr_shots.hip (pack_code per channel, the weights sum to 65536).  T * max(H, W) < 2^31 (the host refuses more:
// the counters are int32); a band holds up to ACT_BAND_ROWS * W pixels, so indices inside a band and into the clip are 64-bit.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

constexpr int ACT_BAND_ROWS = 32;                    // 32 x 1280 pixels = 160 per lane at 720p; 23 bands per frame
constexpr int ACT_UNIT = 8;                          // pixels per lane and step on the 16-byte route
constexpr int ACT_LDS_COLS = 4096;                   // columns with an LDS counter (16 KB): every source up to 4096 wide

SVR_DEVICE bool active_lit(float r, float g, float b, uint32_t dark) { return luma8(r, g, b) > dark; }

// one count for column x (x < W)
SVR_DEVICE void active_count_col(int* cols, int* __restrict__ out_cols, int x) {
    if (x < ACT_LDS_COLS) atomicAdd(cols + x, 1);
    else atomicAdd(out_cols + x, 1);
}

template <int KIND, int C>                           // SVR_STORE_FP32 / SVR_STORE_BF16; C = 3 or 4 samples per pixel
__global__ __launch_bounds__(256) void active_profile_kernel(const void* __restrict__ frames, int* __restrict__ out, int H, int W,
                                                             int bands, uint32_t dark, int vec) {
    __shared__ int cols[ACT_LDS_COLS];
    __shared__ int rows_lds[ACT_BAND_ROWS];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x / bands;
    const int y0 = (int)(blockIdx.x % bands) * ACT_BAND_ROWS;                                 // first pixel row of the band; < H
    const int rows = H - y0 < ACT_BAND_ROWS ? H - y0 : ACT_BAND_ROWS;
    const int64_t n = (int64_t)rows * W;
    const int64_t g0 = (t * H + y0) * W;                                                      // the band's first pixel in the clip
    const int lds_cols = W < ACT_LDS_COLS ? W : ACT_LDS_COLS;
    int* out_cols = out + H;
    for (int i = tid; i < lds_cols; i += 256) cols[i] = 0;
    if (tid < ACT_BAND_ROWS) rows_lds[tid] = 0;
    __syncthreads();
    // [0, head) one by one, then n_units units, then the rest one by one
    int64_t head = vec ? (ACT_UNIT - g0 % ACT_UNIT) % ACT_UNIT : n;
    if (head > n) head = n;
    const int64_t n_units = (n - head) / ACT_UNIT;
    for (int64_t u = tid; u < n_units; u += 256) {
        const int64_t p = head + u * ACT_UNIT;
        float v[ACT_UNIT * C];
        pack_load_run<KIND, ACT_UNIT * C>(frames, (g0 + p) * C, v);
        int row = (int)(p / W), x = (int)(p - (int64_t)row * W), cnt = 0;                     // row < rows <= ACT_BAND_ROWS
#pragma unroll
        for (int j = 0; j < ACT_UNIT; ++j) {
            if (active_lit(v[j * C], v[j * C + 1], v[j * C + 2], dark)) {
                active_count_col(cols, out_cols, x);
                ++cnt;
            }
            if (++x == W) {                                                                   // the unit goes on in the next row
                if (cnt) atomicAdd(rows_lds + row, cnt);
                cnt = 0, x = 0, ++row;                                                        // (p + 7 < n: row stays below rows
            }                                                                                 //  while pixels are left)
        }
        if (cnt) atomicAdd(rows_lds + row, cnt);
    }
    const int64_t tail0 = head + n_units * ACT_UNIT;
    for (int64_t i = tid; i < head + (n - tail0); i += 256) {
        const int64_t p = i < head ? i : tail0 + (i - head);
        const int64_t e = (g0 + p) * C;
        if (active_lit(pack_load<KIND>(frames, e), pack_load<KIND>(frames, e + 1), pack_load<KIND>(frames, e + 2), dark)) {
            const int row = (int)(p / W);
            active_count_col(cols, out_cols, (int)(p - (int64_t)row * W));
            atomicAdd(rows_lds + row, 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < lds_cols; i += 256)
        if (cols[i]) atomicAdd(out_cols + i, cols[i]);                                        // i < W
    if (tid < rows && rows_lds[tid]) atomicAdd(out + y0 + tid, rows_lds[tid]);                // y0 + tid < H
}

}  // namespace svr
