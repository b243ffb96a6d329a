// Rank matching for the LAB colour transfer (colorfix.sort_key / rank_match_spec are the specification): a stable least-significant-
// digit radix sort of fp32 keys, keys only or key + uint32 source index, and the scatter out[index[k]] = sorted_reference[k].
//
//   key      fp32 -> uint32 in integer arithmetic (no floating-point compare: a denormal mode cannot change it): any NaN ->
//            0x7FC00000, both zeros -> +0.0, then a set sign bit complements the word and a clear one is set.  Unsigned order of the
//            keys = the order of torch.sort(stable=True) on the CPU; a key decodes to its canonical value.
//   digits   8 bits, four passes.  11 + 11 + 10 bits would save one pass of 20 B per pair, but a 2048-digit tile x digit table at a
//            4096-key tile is half the size of the keys themselves and its in-tile counters (one set per wave) no longer fit
//            next to the reorder buffers; with 8 bits the table is 1/16 of the keys and a thread of the workgroup owns a digit.
//   a pass   three plain launches ordered by the stream, nothing waits on another workgroup:
//     rank_hist_kernel     a workgroup counts the digits of RANK_GROUP = 16 consecutive tiles of RANK_TILE = 4096 keys (LDS
//                          counters; a count does not depend on arrival order) -> table[digit][tile], 16 tiles = one 64-byte store
//     rank_scan_kernel     workgroup d turns row d of the table into its exclusive prefix over the tiles, 2048 entries per step with
//                          a carry (any number of tiles in one launch), and leaves the row's sum in totals[d]
//     rank_scatter_kernel  a workgroup walks the same 16 tiles.  Per tile: lane l of wave w holds positions w * 1024 + j * 64 + l,
//                          j = 0..15.  Round j ranks a wave's 64 keys by match masks (eight ballots over the digit's bits, a ninth
//                          over "holds a key") and popcount(mask & lanes below); rounds chain through per-wave digit counters in
//                          LDS; waves through their exclusive sums.  Keys (and indices) are put in tile order into LDS, then stored
//                          as contiguous runs per digit at totals' prefix + table[digit][tile] + place in the run.
//            A lane past the end of the data stays in every ballot and barrier, flagged empty; only whole tiles past the end are
//            left (a workgroup-uniform test before the tile's first barrier).
//   rank_apply_kernel      out[index[k]] = value[k], four consecutive k per lane.
//   DIGIT    where a pass takes its digit from.  0: bits [shift, shift + 8) of the key (the sort).  1 and 2: the hue of the pixel the
//            key belongs to (rank_hue_digit: the hue class, or "outside bin 0"), read from a plane beside the keys: the one-pass
//            stable partitions of the hue-conditional matching (svr_hsv.hip).  Such a pass is a first pass (it makes the key and the
//            index from the element's place), counts and ranks exactly as a sort's pass does, and keeps each key's digit in LDS
//            beside it, since the digit cannot be read back from the key.
// Offsets are uint32: n <= 2^30 (svr_api.hip refuses more), so positions, byte offsets of 4-byte elements and the table's
// 256 * ceil16(tiles) entries all stay below 2^32.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

constexpr int RANK_BITS = 8;
constexpr int RANK_RADIX = 1 << RANK_BITS;          // 256: thread d of a workgroup owns digit d
constexpr int RANK_THREADS = 256;
constexpr int RANK_WAVES = RANK_THREADS / 64;
constexpr int RANK_KPT = 16;                        // keys per thread and tile
constexpr int RANK_TILE = RANK_THREADS * RANK_KPT;  // 4096 keys: one column of the table
constexpr int RANK_WAVE_KEYS = 64 * RANK_KPT;       // 1024 consecutive keys of a tile per wave
constexpr int RANK_GROUP = 16;                      // tiles per workgroup: 16 uint32 counts = one 64-byte piece of a table row
constexpr int RANK_SCAN_STEP = RANK_THREADS * 8;    // table entries per step of the scan (two uint4 per thread)
constexpr int64_t RANK_MAX_N = 1ll << 30;
static int g_rank_launches = 3;                     // svr_set_option("rank_launches"): measurement only, 3 = every launch of a pass
static_assert(RANK_RADIX == RANK_THREADS, "thread d owns digit d");

SVR_DEVICE uint32_t rank_key_bits(uint32_t b) {
    const uint32_t mag = b & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) b = 0x7FC00000u;         // NaN of either sign
    if (mag == 0u) b = 0u;                          // both zeros
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SVR_DEVICE uint32_t rank_value_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// Hue bins of colorfix.hue_match_spec (HUE_EDGES): e_k = float32(k * (1.0 / 12)), the product taken in double as Python takes it; bin k
// = [e_k, e_k+1) in fp32 comparisons, bin 11 ends at 1.0, and bin 0 also holds every h >= e_11 (float32(1 - 1/12) == e_11).  A hue is
// in one CLASS: digit 0: h >= 1.0 (bin 0 only), 1: [0, e_1) (bin 0 only; -0.0 is in it), 2: [e_11, 1.0) (bins 0 and 11), 2 + k: bin k
// of 1..10, 13: no bin (NaN, h < 0).  So the classes of bin 0 are digits 0..2 and stand together after a partition by class.
constexpr int HUE_BINS = 12;
constexpr int HUE_CLASSES = 14;
SVR_DEVICE uint32_t rank_hue_class(float h) {
    if (!(h >= 0.0f)) return 13u;
    if (h >= 1.0f) return 0u;
    uint32_t k = 0;
#pragma unroll
    for (int e = 1; e < HUE_BINS; ++e) k += h >= (float)(e * (1.0 / 12)) ? 1u : 0u;
    return k == 0u ? 1u : (k == 11u ? 2u : k + 2u);
}
// DIGIT 1: the class; DIGIT 2: 0 inside bin 0, 1 outside (a stable partition that leaves bin 0 in the order of the plane)
template <int DIGIT>
SVR_DEVICE uint32_t rank_hue_digit(float h) {
    const uint32_t c = rank_hue_class(h);
    return DIGIT == 1 ? c : (c <= 2u ? 0u : 1u);
}

// exclusive prefix of ``v`` over the workgroup's 256 threads (and the sum of all); wave_tot: RANK_WAVES words of LDS
SVR_DEVICE uint32_t rank_block_scan(uint32_t v, uint32_t* wave_tot, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < RANK_WAVES; ++i) {
        const uint32_t t = wave_tot[i];
        if (i < w) base += t;
        tot += t;
    }
    __syncthreads();                                              // wave_tot is free for the next call
    total = tot;
    return base + inc - v;
}

// grid: ceil(tiles / 16).  table: [256][tiles_p] with tiles_p = tiles rounded up to 16 (the columns past the last tile get zeros).
template <int DIGIT>
__global__ __launch_bounds__(RANK_THREADS) void rank_hist_kernel(const uint32_t* __restrict__ in, const float* __restrict__ hue,
                                                                 uint32_t n, int shift, int first,
                                                                 uint32_t* __restrict__ table, uint32_t tiles_p) {
    __shared__ uint32_t hist[RANK_GROUP * RANK_RADIX];
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < RANK_GROUP; ++i) hist[i * RANK_RADIX + tid] = 0;
    __syncthreads();
    const uint32_t g0 = blockIdx.x * (uint32_t)(RANK_GROUP * RANK_TILE);
#pragma unroll 1
    for (int tt = 0; tt < RANK_GROUP; ++tt) {
        const uint32_t base = g0 + (uint32_t)tt * RANK_TILE;
        if (base >= n) break;                                     // (uniform; no barrier inside the loop)
#pragma unroll
        for (int j = 0; j < RANK_KPT; ++j) {
            const uint32_t g = base + (uint32_t)j * RANK_THREADS + tid;
            if (g < n) {
                uint32_t d;
                if constexpr (DIGIT == 0) {
                    uint32_t k = in[g];
                    if (first) k = rank_key_bits(k);
                    d = (k >> shift) & (RANK_RADIX - 1);
                } else {
                    d = rank_hue_digit<DIGIT>(hue[g]);
                }
                atomicAdd(&hist[tt * RANK_RADIX + d], 1u);
            }
        }
    }
    __syncthreads();
    uint4* row = (uint4*)(table + tid * tiles_p + blockIdx.x * (uint32_t)RANK_GROUP);
#pragma unroll
    for (int q = 0; q < RANK_GROUP / 4; ++q)
        row[q] = make_uint4(hist[(4 * q) * RANK_RADIX + tid], hist[(4 * q + 1) * RANK_RADIX + tid],
                            hist[(4 * q + 2) * RANK_RADIX + tid], hist[(4 * q + 3) * RANK_RADIX + tid]);
}

// grid: 256, workgroup d scans row d in place; totals[d] = the row's sum
__global__ __launch_bounds__(RANK_THREADS) void rank_scan_kernel(uint32_t* __restrict__ table, uint32_t tiles_p,
                                                                 uint32_t* __restrict__ totals) {
    __shared__ uint32_t wave_tot[RANK_WAVES];
    uint32_t* row = table + blockIdx.x * tiles_p;
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < tiles_p; base += RANK_SCAN_STEP) {         // (uniform: every thread meets the scan's barriers)
        const uint32_t i = base + threadIdx.x * 8;
        const bool in = i < tiles_p;                                          // tiles_p % 16 == 0: eight entries or none
        uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
        if (in) { a = *(const uint4*)(row + i); b = *(const uint4*)(row + i + 4); }
        const uint32_t sum = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
        uint32_t total;
        const uint32_t ex = rank_block_scan(sum, wave_tot, total) + carry;
        if (in) {
            uint4 oa, ob;
            oa.x = ex; oa.y = oa.x + a.x; oa.z = oa.y + a.y; oa.w = oa.z + a.z;
            ob.x = oa.w + a.w; ob.y = ob.x + b.x; ob.z = ob.y + b.y; ob.w = ob.z + b.z;
            *(uint4*)(row + i) = oa; *(uint4*)(row + i + 4) = ob;
        }
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// out_mode 0: keys (and indices) as they are, for the next pass; 1: the keys' canonical values (and indices): the last pass of a
// sort; 2: indices only: the last pass over the source plane of a rank matching, whose sorted keys nobody reads
template <bool PAIRS, int DIGIT>
__global__ __launch_bounds__(RANK_THREADS) void rank_scatter_kernel(const uint32_t* __restrict__ in_keys, const uint32_t* __restrict__ in_idx,
                                                                    const float* __restrict__ hue,
                                                                    uint32_t n, int shift, int first, int out_mode,
                                                                    const uint32_t* __restrict__ table, uint32_t tiles_p,
                                                                    const uint32_t* __restrict__ totals,
                                                                    uint32_t* __restrict__ out_keys, uint32_t* __restrict__ out_idx) {
    __shared__ uint32_t skey[RANK_TILE];
    __shared__ uint32_t sidx[PAIRS ? RANK_TILE : 1];
    __shared__ unsigned char sdig[DIGIT ? RANK_TILE : 1];         // DIGIT != 0: the digit of the key at each place of the tile
    __shared__ uint32_t cnt[RANK_WAVES * RANK_RADIX];             // per wave and digit: counts, then the wave's first place in the tile
    __shared__ uint32_t gdelta[RANK_RADIX];                       // per digit: global place - place in the tile
    __shared__ uint32_t wave_tot[RANK_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t* wcnt = cnt + w * RANK_RADIX;
    uint32_t unused;
    const uint32_t dbase = rank_block_scan(totals[tid], wave_tot, unused);    // keys of smaller digits in the whole array
#pragma unroll 1
    for (int tt = 0; tt < RANK_GROUP; ++tt) {
        const uint32_t tile = blockIdx.x * (uint32_t)RANK_GROUP + tt, tbase = tile * (uint32_t)RANK_TILE;
        if (tbase >= n) break;                                    // a whole tile past the end: uniform, before the tile's barriers
        const uint32_t nvalid = min(n - tbase, (uint32_t)RANK_TILE);
        const uint32_t toff = table[tid * tiles_p + tile];        // keys of digit tid in the tiles before this one
#pragma unroll
        for (int i = 0; i < RANK_WAVES; ++i) cnt[i * RANK_RADIX + tid] = 0;
        uint32_t key[RANK_KPT], idx[PAIRS ? RANK_KPT : 1], r[RANK_KPT], dig[DIGIT ? RANK_KPT : 1];
#pragma unroll
        for (int j = 0; j < RANK_KPT; ++j) {
            const uint32_t p = w * RANK_WAVE_KEYS + j * 64 + lane;
            key[j] = 0xFFFFFFFFu;
            if constexpr (PAIRS) idx[j] = 0;
            if constexpr (DIGIT != 0) dig[j] = RANK_RADIX - 1;
            if (p < nvalid) {
                const uint32_t k = in_keys[tbase + p];
                key[j] = first ? rank_key_bits(k) : k;
                if constexpr (PAIRS) idx[j] = first ? tbase + p : in_idx[tbase + p];
                if constexpr (DIGIT != 0) dig[j] = rank_hue_digit<DIGIT>(hue[tbase + p]);
            }
        }
        __syncthreads();                                          // the counters are zero
#pragma unroll
        for (int j = 0; j < RANK_KPT; ++j) {
            uint32_t d = (key[j] >> shift) & (RANK_RADIX - 1);
            if constexpr (DIGIT != 0) d = dig[j];
            const bool valid = w * RANK_WAVE_KEYS + j * 64 + lane < nvalid;
            uint64_t m = __ballot(valid);                         // an empty lane votes in every ballot and is in no mask
#pragma unroll
            for (int b = 0; b < RANK_BITS; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t bal = __ballot(bit);
                m &= bit ? bal : ~bal;
            }
            const uint32_t prev = wcnt[d];                        // keys of digit d in this wave's earlier rounds
            const uint32_t lower = (uint32_t)__popcll(m & below);
            r[j] = prev + lower;
            if (valid && lower == 0) wcnt[d] = prev + (uint32_t)__popcll(m);
            __builtin_amdgcn_wave_barrier();                      // round j + 1 reads what round j stored (same wave: LDS keeps order)
        }
        __syncthreads();
        {
            const uint32_t c0 = cnt[tid], c1 = cnt[RANK_RADIX + tid], c2 = cnt[2 * RANK_RADIX + tid], c3 = cnt[3 * RANK_RADIX + tid];
            static_assert(RANK_WAVES == 4, "four per-wave counters are summed by hand");
            uint32_t total;
            const uint32_t tstart = rank_block_scan((c0 + c1) + (c2 + c3), wave_tot, total);   // (its barriers: all counts are read)
            cnt[tid] = tstart;
            cnt[RANK_RADIX + tid] = tstart + c0;
            cnt[2 * RANK_RADIX + tid] = tstart + c0 + c1;
            cnt[3 * RANK_RADIX + tid] = tstart + c0 + c1 + c2;
            gdelta[tid] = dbase + toff - tstart;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RANK_KPT; ++j) {
            if (w * RANK_WAVE_KEYS + j * 64 + lane < nvalid) {
                uint32_t d = (key[j] >> shift) & (RANK_RADIX - 1);
                if constexpr (DIGIT != 0) d = dig[j];
                const uint32_t at = wcnt[d] + r[j];
                skey[at] = key[j];
                if constexpr (PAIRS) sidx[at] = idx[j];
                if constexpr (DIGIT != 0) sdig[at] = (unsigned char)d;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RANK_KPT; ++j) {
            const uint32_t q = (uint32_t)j * RANK_THREADS + tid;
            if (q < nvalid) {
                const uint32_t k = skey[q];
                uint32_t d = (k >> shift) & (RANK_RADIX - 1);
                if constexpr (DIGIT != 0) d = sdig[q];
                const uint32_t dst = gdelta[d] + q;
                if (out_mode != 2) out_keys[dst] = out_mode ? rank_value_bits(k) : k;
                if constexpr (PAIRS) out_idx[dst] = sidx[q];
            }
        }
        // (the next tile writes cnt after this tile's last read of it, gdelta and skey only behind further barriers)
    }
}

// out[index[k]] = value[k]; a lane takes four consecutive k (index and value 16-byte aligned)
__global__ __launch_bounds__(256) void rank_apply_kernel(const uint32_t* __restrict__ index, const uint32_t* __restrict__ value,
                                                         uint32_t n, uint32_t* out) {
    const uint32_t k4 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (k4 + 4u <= n) {
        const uint4 i = *(const uint4*)(index + k4), v = *(const uint4*)(value + k4);
        out[i.x] = v.x; out[i.y] = v.y; out[i.z] = v.z; out[i.w] = v.w;
    } else {
        for (uint32_t k = k4; k < n; ++k) out[index[k]] = value[k];
    }
}

}  // namespace svr
