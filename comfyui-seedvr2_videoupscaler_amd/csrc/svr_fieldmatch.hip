// Field matching on the packed planes (fieldmatch.py is the specification, bit for bit: integers in, integers out): per frame the
// combing of the three weaves its kept field can make is counted, then every frame is copied row by row from the weave the counts
// choose, or from the deinterlaced frame where none is clean.  64-bit offsets, capped grids with a grid-stride loop.
//
//   comb_kernel<S, VEC>   ONE launch, plane 0 only.  A workgroup owns one block row (16 plane rows) of one frame
//       and a run of whole block columns: a lane owns one 16-byte unit (vector route) or one sample column (element route) and
//       walks down the band's tested rows.  u and l of one tested row are l and u of its neighbours, so the lane keeps l as the
//       next u and reads every F[t] row of the band once; the rows of F[t-1] and F[t+1] are read at the tested rows only.  A block
//       is 16 s samples wide, a multiple of 16 bytes in every format, so a unit never straddles two block columns and all a lane
//       counts belongs to ONE block: three registers, then one LDS atomic per non-zero candidate.  After a barrier the non-zero
//       block counters go out with integer atomicAdd (total) and atomicMax (peak) -- both commute, so two runs give the same bits.
//       A workgroup's run starts on a block column, so every block is counted by exactly one workgroup and its peak is whole.
//   select_kernel<S, VEC>   ONE LAUNCH PER PLANE (svr_deinterlace's rule and routes).  Every lane reads its
//       frame's three peaks from device memory (stream order after the counts launch is all it needs), applies the mode rule and
//       copies 16 bytes or one sample from F[t], F[t-1], F[t+1] or deint[t].  In plane 0's launch the lane that owns the first
//       sample of a frame writes modes[t] and adds the frame to stats (64-bit integer atomic add).
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

constexpr int FM_BLOCK = 16;                          // fieldmatch.BLOCK: plane rows, and pixel columns, of a block
constexpr int FM_LANES = 256;

// sample i is combed: m outside [min(u, l) - thr, max(u, l) + thr]
SVR_DEVICE int fm_combed(int m, int u, int l, int thr) { return (m < min(u, l) - thr || m > max(u, l) + thr) ? 1 : 0; }

// VEC: a lane owns U = 16 / sizeof(S) samples of a row; else one.  per: lanes per block column (16 s / U, or 16 s); cb: block
// columns per workgroup (FM_LANES / per); chunks: workgroups per row of blocks.  cols: the row in lane columns (N / U, or N).
template <class S, int VEC>
__global__ __launch_bounds__(FM_LANES) void comb_kernel(DeintClip<S> clip, int R, int64_t N, int per, int cb, int chunks, int64_t cols,
                                                         int first, int thr, int* __restrict__ cnt) {
    constexpr int U = VEC ? 16 / (int)sizeof(S) : 1;
    __shared__ int blocks[3][FM_LANES];
    const int lane = threadIdx.x, local = lane / per;
    const int band_rows = (R + FM_BLOCK - 1) / FM_BLOCK;
    const int64_t items = (int64_t)clip.T * band_rows * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int chunk = (int)(item % chunks), band = (int)(item / chunks % band_rows), t = (int)(item / chunks / band_rows);
        blocks[0][lane] = 0, blocks[1][lane] = 0, blocks[2][lane] = 0;
        __syncthreads();
        const int64_t col = (int64_t)chunk * cb * per + lane;                 // the lane's unit / sample column in the row
        if (local < cb && col < cols) {
            // the band's tested rows: r % 2 == 1 - first, 1 <= r <= R - 2
            int r = band * FM_BLOCK;
            if (r < 1) r = 1;
            if ((r & 1) == first) ++r;
            const int end = min(band * FM_BLOCK + FM_BLOCK - 1, R - 2);
            if (r <= end) {
                const S* cur = clip.at(t) + col * U;
                const S* prev = clip.at(t - 1) + col * U;
                const S* next = clip.at(t + 1) + col * U;
                int c0 = 0, c1 = 0, c2 = 0;
                if constexpr (VEC != 0) {
                    int u[U], l[U], m[U];
                    deint_load_unit<S>(cur + (int64_t)(r - 1) * N, u);
                    for (; r <= end; r += 2) {
                        deint_load_unit<S>(cur + (int64_t)(r + 1) * N, l);
                        deint_load_unit<S>(cur + (int64_t)r * N, m);
#pragma unroll
                        for (int j = 0; j < U; ++j) c0 += fm_combed(m[j], u[j], l[j], thr);
                        deint_load_unit<S>(prev + (int64_t)r * N, m);
#pragma unroll
                        for (int j = 0; j < U; ++j) c1 += fm_combed(m[j], u[j], l[j], thr);
                        deint_load_unit<S>(next + (int64_t)r * N, m);
#pragma unroll
                        for (int j = 0; j < U; ++j) c2 += fm_combed(m[j], u[j], l[j], thr), u[j] = l[j];
                    }
                } else {
                    int u = cur[(int64_t)(r - 1) * N];
                    for (; r <= end; r += 2) {
                        const int l = cur[(int64_t)(r + 1) * N];
                        c0 += fm_combed(cur[(int64_t)r * N], u, l, thr);
                        c1 += fm_combed(prev[(int64_t)r * N], u, l, thr);
                        c2 += fm_combed(next[(int64_t)r * N], u, l, thr);
                        u = l;
                    }
                }
                if (c0) atomicAdd(&blocks[0][local], c0);
                if (c1) atomicAdd(&blocks[1][local], c1);
                if (c2) atomicAdd(&blocks[2][local], c2);
            }
        }
        __syncthreads();
        if (lane < cb) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int n = blocks[k][lane];
                if (n) {
                    atomicAdd(cnt + ((int64_t)t * 3 + k) * 2, n);
                    atomicMax(cnt + ((int64_t)t * 3 + k) * 2 + 1, n);
                }
            }
        }
        __syncthreads();                                                      // (the counters are zeroed again at the loop's head)
    }
}

// fieldmatch.modes_torch for frame t: peaks against mi * s
SVR_DEVICE int fm_mode(const int* __restrict__ cnt, int t, int64_t bound) {
    const int* c = cnt + (int64_t)t * 6;
    const int pc = c[1], pa = c[3], pb = c[5];
    if (pc <= bound) return 0;
    if (pa <= pb) return pa <= bound ? 1 : 3;
    return pb <= bound ? 2 : 3;
}

// the frame a sample of row r of frame t is copied from: deint[t] in mode 3; F[t] for the kept parity (and the only row of a plane);
// else the frame the mode names
template <class S>
SVR_DEVICE const S* fm_source(const DeintClip<S>& clip, const S* deint, int t, int mode, bool kept) {
    if (mode == 3) return deint + (int64_t)t * clip.frame;
    return clip.at(kept || mode == 0 ? t : mode == 1 ? t - 1 : t + 1);
}

// off / R / N: the plane inside a frame (elements).  cols: N in lane columns (N / U, or N).  modes / stats: written where this is
// plane 0's launch (null otherwise, and where the caller wants none)
template <class S, int VEC>
__global__ __launch_bounds__(FM_LANES) void select_kernel(DeintClip<S> clip, const S* __restrict__ deint, const int* __restrict__ cnt,
                                                           int64_t bound, S* __restrict__ out, int64_t off, int R, int64_t N, int64_t cols,
                                                           int first, int plane0, int* __restrict__ modes,
                                                           unsigned long long* __restrict__ stats) {
    constexpr int U = VEC ? 16 / (int)sizeof(S) : 1;
    const int64_t total = (int64_t)clip.T * R * cols;
    for (int64_t idx = (int64_t)blockIdx.x * FM_LANES + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * FM_LANES) {
        const int64_t x = idx % cols;
        const int r = (int)(idx / cols % R), t = (int)(idx / cols / R);
        const int mode = fm_mode(cnt, t, bound);
        const int64_t at = off + (int64_t)r * N + x * U;
        const S* src = fm_source(clip, deint, t, mode, (r & 1) == first || R == 1) + at;
        S* dst = out + (int64_t)t * clip.frame + at;
        if constexpr (VEC != 0) *(uint4*)dst = *(const uint4*)src;
        else *dst = *src;
        if (plane0 && r == 0 && x == 0) {
            if (modes) modes[t] = mode;
            if (stats) {
                atomicAdd(stats + mode, 1ull);
                if (mode == 3) {
                    atomicAdd(stats + 4, (unsigned long long)cnt[(int64_t)t * 6 + 2]);
                    atomicAdd(stats + 5, (unsigned long long)cnt[(int64_t)t * 6 + 4]);
                }
            }
        }
    }
}

}  // namespace svr
