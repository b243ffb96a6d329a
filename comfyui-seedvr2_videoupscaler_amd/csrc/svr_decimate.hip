// Decimation on the packed planes (decimate.py is the specification, bit for bit: integers in, integers out): per frame the largest
// block sum of its absolute difference from the frame before it, then of every cycle of five frames the four that are not the
// smallest are copied.  64-bit offsets, capped grids with a grid-stride loop.
//
//   diff_kernel<S, VEC>   ONE launch, plane 0 only; comb_kernel's ownership.  A workgroup owns one band of 32 plane rows of one
//       frame and a run of whole block columns: a lane owns one 16-byte unit (vector route) or one sample column (element route)
//       and walks down the band's rows of F[t] and F[t-1].  A block is 32 s samples wide, a multiple of 16 bytes in every format, so
//       a unit never straddles two block columns and all a lane sums belongs to ONE block: one register, then one LDS atomic per
//       lane.  After a barrier the non-zero block sums go out with integer atomicMax -- it commutes, so two runs give the same
//       bits.  A workgroup's run starts on a block column, so every block is summed by exactly one workgroup and its sum is whole.
//       The caller has zeroed diff; frame 0 of a clip without ``before`` has no predecessor: one lane stores DEC_FIRST there and
//       nothing else touches that entry.  Every frame's plane 0 is read twice, as F[t] and as F[t-1].
//   decimate_select_kernel<S, VEC>   ONE launch over whole frames: an output frame is a contiguous copy of one input frame, in
//       16-byte units where the pointers and the frame's bytes allow, else in elements.  Every lane derives its output frame's
//       source from its cycle's five diffs, read from device memory (stream order after the diffs launch is all it needs).  The
//       lane that owns the first unit of a cycle's first output frame writes drops[c] and adds the cycle to stats (64-bit
//       integer atomic add).
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

constexpr int DEC_BLOCK = 32;                         // decimate.BLOCK: plane rows, and pixel columns, of a block
constexpr int DEC_CYCLE = 5;                          // decimate.CYCLE
constexpr int DEC_LANES = 256;
constexpr int DEC_FIRST = 0x7fffffff;                 // decimate.FIRST: diff[0] of a clip without ``before``

// VEC: a lane owns U = 16 / sizeof(S) samples of a row; else one.  per: lanes per block column (32 s / U, or 32 s); cb: block
// columns per workgroup (DEC_LANES / per); chunks: workgroups per row of blocks.  cols: the row in lane columns (N / U, or N).
// frame: elements per frame.  before: the frame ahead of F[0], or null.
template <class S, int VEC>
__global__ __launch_bounds__(DEC_LANES) void diff_kernel(const S* __restrict__ packed, const S* __restrict__ before, int T, int64_t frame,
                                                          int R, int64_t N, int per, int cb, int chunks, int64_t cols,
                                                          int* __restrict__ diff) {
    constexpr int U = VEC ? 16 / (int)sizeof(S) : 1;
    __shared__ int blocks[DEC_LANES];
    const int lane = threadIdx.x, local = lane / per;
    const int band_rows = (R + DEC_BLOCK - 1) / DEC_BLOCK;
    const int64_t items = (int64_t)T * band_rows * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int chunk = (int)(item % chunks), band = (int)(item / chunks % band_rows), t = (int)(item / chunks / band_rows);
        if (t == 0 && !before) {                                              // (uniform over the workgroup: no barrier is skipped by some)
            if (chunk == 0 && band == 0 && lane == 0) diff[0] = DEC_FIRST;
            continue;
        }
        blocks[lane] = 0;
        __syncthreads();
        const int64_t col = (int64_t)chunk * cb * per + lane;                 // the lane's unit / sample column in the row
        if (local < cb && col < cols) {
            const int r0 = band * DEC_BLOCK, r1 = min(r0 + DEC_BLOCK, R);
            const S* cur = packed + (int64_t)t * frame + col * U;
            const S* prev = (t > 0 ? packed + (int64_t)(t - 1) * frame : before) + col * U;
            int sum = 0;
            for (int r = r0; r < r1; ++r) {
                if constexpr (VEC != 0) {
                    int a[U], b[U];
                    deint_load_unit<S>(cur + (int64_t)r * N, a);
                    deint_load_unit<S>(prev + (int64_t)r * N, b);
#pragma unroll
                    for (int j = 0; j < U; ++j) sum += deint_abs(a[j] - b[j]);
                } else {
                    sum += deint_abs((int)cur[(int64_t)r * N] - (int)prev[(int64_t)r * N]);
                }
            }
            if (sum) atomicAdd(&blocks[local], sum);
        }
        __syncthreads();
        if (lane < cb) {
            const int n = blocks[lane];
            if (n) atomicMax(diff + t, n);
        }
        __syncthreads();                                                      // (the sums are zeroed again at the loop's head)
    }
}

// decimate.drops_torch for cycle c: the first position of the smallest of its five diffs
SVR_DEVICE int dec_drop(const int* __restrict__ diff, int c) {
    const int* d = diff + (int64_t)c * DEC_CYCLE;
    int at = 0, least = d[0];
#pragma unroll
    for (int j = 1; j < DEC_CYCLE; ++j)
        if (d[j] < least) least = d[j], at = j;
    return at;
}

// units: a frame in lane units (frame * sizeof(S) / 16, or frame elements).  n_out = T - T / 5 output frames.  bound: the diff above
// which a dropped frame counts as no duplicate.  drops / stats: null where the caller wants none.
template <class S, int VEC>
__global__ __launch_bounds__(DEC_LANES) void decimate_select_kernel(const S* __restrict__ packed, const int* __restrict__ diff, int T,
                                                                     int64_t frame, int64_t units, int64_t bound, S* __restrict__ out,
                                                                     int* __restrict__ drops, unsigned long long* __restrict__ stats) {
    constexpr int U = VEC ? 16 / (int)sizeof(S) : 1;
    const int cycles = T / DEC_CYCLE;
    const int64_t n_out = (int64_t)T - cycles, total = n_out * units;
    for (int64_t idx = (int64_t)blockIdx.x * DEC_LANES + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * DEC_LANES) {
        const int64_t x = idx % units, o = idx / units;
        int64_t src = o + cycles;                                              // the trailing partial cycle: a copy
        if (o < (int64_t)cycles * (DEC_CYCLE - 1)) {
            const int c = (int)(o / (DEC_CYCLE - 1)), j = (int)(o % (DEC_CYCLE - 1));
            const int drop = dec_drop(diff, c);
            src = (int64_t)c * DEC_CYCLE + j + (j >= drop ? 1 : 0);
            if (j == 0 && x == 0) {
                if (drops) drops[c] = drop;
                if (stats) {
                    atomicAdd(stats + drop, 1ull);
                    if (diff[(int64_t)c * DEC_CYCLE + drop] > bound) atomicAdd(stats + DEC_CYCLE, 1ull);
                }
            }
        }
        const S* from = packed + src * frame + x * U;
        S* to = out + o * frame + x * U;
        if constexpr (VEC != 0) *(uint4*)to = *(const uint4*)from;
        else *to = *from;
    }
}

}  // namespace svr
