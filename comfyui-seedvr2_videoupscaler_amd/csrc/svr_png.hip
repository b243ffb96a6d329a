// PNG output encoded on the device: per frame the zlib stream of pngenc.py (the specification, byte for byte) -- filtered rows,
// one Huffman-only dynamic deflate block per segment of about 64 KiB, an empty stored block behind each so that segments are whole
// bytes.  Three launches:
//   png_filter_kernel   one workgroup per (frame, segment).  A wave takes a row: a first sweep over its pixels sums the five filters'
//                       costs (codes formed from the fp32 / bf16 samples of the pixel, its left, upper and upper-left neighbours),
//                       a wave reduction picks the type, a second sweep stores the filtered bytes to scratch, counts them in the
//                       wave's own LDS histogram and accumulates the segment's Adler-32 partial sums.  Then the workgroup builds the
//                       code in LDS: the 257 counts ranked in parallel, the two-queue tree, the depths and the canonical codes by one
//                       lane (a few hundred serial LDS steps), the counts halved and the tree rebuilt while it is deeper than 15.
//                       Out: the code table (bit-reversed code | length << 16 per symbol), the segment's byte size, its Adler sums.
//   png_scan_kernel     one workgroup per frame: exclusive scan of the segment sizes (offsets, sizes[t]), the Adler partials
//                       combined in order, the stream's 2-byte head and 6-byte tail.
//   png_pack_kernel     one workgroup per (frame, segment): the table in LDS; tiles of 256 lanes x 16 symbols; a workgroup prefix sum
//                       of the lanes' bit counts gives each its bit offset; a lane assembles 32-bit words in a register pair and ORs
//                       them into a zeroed LDS image of the tile (integer OR: order-independent, so the bytes are deterministic);
//                       the tile's whole bytes go to the output, its last partial byte is carried into the next tile.
// svr_png_encode_runs (pngenc.py "Runs": run-length matches at distance 1) puts one launch behind the first and packs differently:
//   png_runs_kernel     one workgroup per (frame, segment): the tokens tile by tile (png_tile_tokens: run starts by a running
//                       maximum over the workgroup, carried from tile to tile; run ends by a look of 258 bytes ahead), their
//                       histogram over 286 symbols in LDS, the second code by the same construction, both bit totals compared:
//                       meta[3] = the choice, meta[0] and the second table for a chosen segment.
//   png_pack_kernel<true>  a chosen segment: the 1222-bit header, the tokens found again tile by tile (nothing but the choice and
//                       the table passes between the launches), a position giving 0 bits, a literal's code, or a match's code,
//                       extra bits and distance bit; any other segment exactly as png_pack_kernel<false>, the literal packer.
// Every indexed per-lane array is fully unrolled (registers) or lives in LDS: no kernel here has a private segment.  Every store to
// ``out`` is guarded by the frame's capacity.  Bytes of ``out`` past sizes[t] are not written.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

constexpr int PNG_SYMS = 257;                      // literals 0..255 and end-of-block
constexpr int PNG_TABLE = 260;                     // table stride in 32-bit words (16-byte multiples)
constexpr uint32_t PNG_ADLER = 65521u;
constexpr int PNG_HEADER_BITS = 1106;
constexpr int PNG_RUN = 16;                        // symbols per lane and tile in png_pack_kernel
constexpr int PNG_TILE = 256 * PNG_RUN;
// The packer's tile image: 7 carried bits + PNG_TILE positions of at most 15 bits + 6 bits.  (A match head takes up to 15 + 5 + 1 =
// 21 bits and the two or more positions it covers none: they make up for it, unless the head is the tile's last position.)
constexpr int PNG_BUF_WORDS = (7 + PNG_TILE * 15 + 6 + 31) / 32 + 1;
constexpr int PNG_RUN_SYMS = 286;                  // with run-length matches: the length symbols 257..285 as well
constexpr int PNG_RUN_TABLE = 288;
constexpr int PNG_RUN_HEADER_BITS = 1222;
constexpr uint32_t PNG_MAX_MATCH = 258u;
// groups of PNG_RUN positions behind a lane's own in which a run's end decides a token: whether 258 bytes are left at position i is
// known from the positions up to i + 257
constexpr int PNG_LOOK = (PNG_RUN - 1 + 257) / PNG_RUN;
constexpr uint32_t PNG_NONE = 0xFFFFFFFFu;

static int g_png_passes = 3;                       // svr_set_option("png_passes"): measurement only, 3 = the whole encoder

struct PngLayout {
    int bpp, stride, R, nseg;
    int64_t filt_off, table_off, meta_off, segoff_off, table2_off, scratch_bytes, capacity;
};

// (pngenc.geometry / frame_bound; the scratch: filtered bytes | tables | {bytes, adler s1, s2, literal data bits -> run block chosen}
// per segment | segment offsets | with runs: the run blocks' tables)
static inline PngLayout png_layout(int64_t T, int64_t H, int64_t W, int C, int depth, bool runs = false) {
    PngLayout L;
    L.bpp = C * depth / 8;
    L.stride = (int)(1 + W * L.bpp);
    L.R = (int)std::max<int64_t>(1, 65536 / L.stride);
    L.nseg = (int)((H + L.R - 1) / L.R);
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    const int64_t segs = T * L.nseg;
    L.filt_off = 0;
    L.table_off = up16(T * H * L.stride);
    L.meta_off = L.table_off + segs * PNG_TABLE * 4;
    L.segoff_off = L.meta_off + segs * 16;
    L.table2_off = up16(L.segoff_off + segs * 8);
    L.scratch_bytes = runs ? L.table2_off + segs * PNG_RUN_TABLE * 4 : L.segoff_off + segs * 8;
    const int64_t full = H / L.R, rest = H - full * L.R;
    auto bound = [](int64_t n) { return 139 + (15 * (n + 1) + 7) / 8 + 5; };
    L.capacity = 2 + full * bound((int64_t)L.R * L.stride) + (rest ? bound(rest * L.stride) : 0) + 6;
    return L;
}

template <int KIND, int DEPTH, int C>
SVR_DEVICE void png_pixel(const void* frames, int64_t px, uint32_t* b) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const uint32_t q = pack_code(pack_load<KIND>(frames, px * C + c), DEPTH == 8 ? 255.f : 65535.f);
        if constexpr (DEPTH == 8) b[c] = q;
        else { b[2 * c] = q >> 8; b[2 * c + 1] = q & 255u; }                 // (big-endian)
    }
}

// the pixel's bytes and those of its left, upper and upper-left neighbours (zero outside the frame)
template <int KIND, int DEPTH, int C>
SVR_DEVICE void png_neighbours(const void* frames, int64_t row_px, int W, int x, bool top, uint32_t* cur, uint32_t* lf, uint32_t* up,
                               uint32_t* ul) {
    constexpr int BPP = C * DEPTH / 8;
#pragma unroll
    for (int k = 0; k < BPP; ++k) lf[k] = up[k] = ul[k] = 0;
    png_pixel<KIND, DEPTH, C>(frames, row_px + x, cur);
    if (x > 0) png_pixel<KIND, DEPTH, C>(frames, row_px + x - 1, lf);
    if (!top) {
        png_pixel<KIND, DEPTH, C>(frames, row_px - W + x, up);
        if (x > 0) png_pixel<KIND, DEPTH, C>(frames, row_px - W + x - 1, ul);
    }
}

SVR_DEVICE uint32_t png_paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

SVR_DEVICE uint32_t png_wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}

// The code of pngenc.code_lengths / canonical_codes over the NS counts ``hist`` (LDS; every thread of the workgroup calls this;
// hist is complete and at least two counts are non-zero): two-queue Huffman over the used symbols, counts halved (rounding up)
// while the tree is deeper than 15.  On return, for everyone: sw[s] = bit-reversed code | length << 16 (0 for an unused symbol);
// for thread 0 the return value is the sum of hist[s] * length[s].  ``sw`` (LDS, 2 NS words) is also the weights' working space:
// the sorted leaves, then the internal nodes.  The function's own arrays are one set per NS, distinct objects (the serial part is
// LDS-latency bound, and the compiler keeps more of it in registers when it knows that the arrays do not overlap).
template <int NS>
SVR_DEVICE uint64_t png_build_code(const uint32_t* hist, uint32_t* sw, int tid) {
    __shared__ uint32_t cnt[NS], len_s[NS];
    __shared__ unsigned short ssym[NS], parent[2 * NS], depth_s[2 * NS];
    __shared__ uint32_t blc[17], nxt[17];
    __shared__ uint32_t ctl[2];
    __syncthreads();
    for (int s = tid; s < NS; s += 256) {
        cnt[s] = hist[s];
        len_s[s] = 0;
    }
    for (;;) {
        __syncthreads();
        for (int s = tid; s < NS; s += 256) {
            const uint32_t c = cnt[s];
            if (c) {
                int rank = 0;
                for (int j = 0; j < NS; ++j) {
                    const uint32_t cj = cnt[j];
                    rank += (cj != 0u && (cj < c || (cj == c && j < s))) ? 1 : 0;
                }
                sw[rank] = c;
                ssym[rank] = (unsigned short)s;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int s = 0; s < NS; ++s) n += cnt[s] != 0u ? 1 : 0;
            int leaf = 0, node = n;                               // (n >= 2: a type byte and the end-of-block symbol)
            for (int q = n; q < 2 * n - 1; ++q) {
                uint32_t w = 0;
                for (int rep = 0; rep < 2; ++rep) {
                    const bool take_leaf = leaf < n && (node >= q || sw[leaf] <= sw[node]);
                    const int pick = take_leaf ? leaf++ : node++;
                    w += sw[pick];
                    parent[pick] = (unsigned short)q;
                }
                sw[q] = w;
            }
            depth_s[2 * n - 2] = 0;
            uint32_t deepest = 0;
            for (int x = 2 * n - 3; x >= 0; --x) {
                const uint32_t d = depth_s[parent[x]] + 1u;
                depth_s[x] = (unsigned short)d;
                if (x < n) deepest = max(deepest, d);
            }
            ctl[0] = (uint32_t)n;
            ctl[1] = deepest;
        }
        __syncthreads();
        if (ctl[1] <= 15u) break;
        for (int s = tid; s < NS; s += 256) {
            const uint32_t c = cnt[s];
            cnt[s] = c ? (c + 1u) >> 1 : 0u;
        }
    }
    for (int i = tid; i < (int)ctl[0]; i += 256) len_s[ssym[i]] = depth_s[i];
    __syncthreads();
    uint64_t total = 0;
    if (tid == 0) {                                               // canonical codes (RFC 1951, 3.2.2), stored bit-reversed
        for (int b = 0; b <= 16; ++b) blc[b] = 0;
        for (int s = 0; s < NS; ++s) blc[len_s[s]] += 1u;
        blc[0] = 0;
        uint32_t code = 0;
        nxt[0] = 0;
        for (int b = 1; b <= 15; ++b) { code = (code + blc[b - 1]) << 1; nxt[b] = code; }
        uint64_t bits = 0;
        for (int s = 0; s < NS; ++s) {
            const uint32_t l = len_s[s];
            uint32_t e = 0;
            if (l) {
                const uint32_t c = nxt[l];
                nxt[l] = c + 1u;
                e = (__brev(c) >> (32u - l)) | (l << 16);
                bits += (uint64_t)hist[s] * l;
            }
            sw[s] = e;
        }
        total = bits;
    }
    __syncthreads();
    return total;
}

template <int KIND, int DEPTH, int C>
__global__ __launch_bounds__(256) void png_filter_kernel(const void* __restrict__ frames, unsigned char* __restrict__ filt,
                                                         uint32_t* __restrict__ table, uint32_t* __restrict__ meta, int H, int W, int R,
                                                         int nseg) {
    constexpr int BPP = C * DEPTH / 8;
    __shared__ uint32_t whist[4][256];
    __shared__ uint32_t hist[PNG_SYMS], sw[2 * PNG_SYMS];
    __shared__ uint32_t adler[2];
    const int seg = (int)(blockIdx.x % (unsigned)nseg);
    const int64_t t = blockIdx.x / (unsigned)nseg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = 1 + W * BPP;
    const int r0 = seg * R, r1 = min(H, r0 + R);
    const uint32_t seglen = (uint32_t)(r1 - r0) * (uint32_t)stride;
    for (int i = tid; i < 4 * 256; i += 256) (&whist[0][0])[i] = 0;
    if (tid < 2) adler[tid] = 0;
    __syncthreads();

    uint64_t s1 = 0, s2 = 0;                                      // sum of bytes; sum of (seglen - position) * byte
    for (int r = r0 + wave; r < r1; r += 4) {
        const int64_t row_px = (t * H + r) * W;
        const bool top = r == 0;
        uint32_t cost[5] = {0, 0, 0, 0, 0};
        for (int x = lane; x < W; x += 64) {
            uint32_t cur[BPP], lf[BPP], up[BPP], ul[BPP];
            png_neighbours<KIND, DEPTH, C>(frames, row_px, W, x, top, cur, lf, up, ul);
#pragma unroll
            for (int k = 0; k < BPP; ++k) {
                const uint32_t pred[5] = {0u, lf[k], up[k], (lf[k] + up[k]) >> 1, png_paeth(lf[k], up[k], ul[k])};
#pragma unroll
                for (int ty = 0; ty < 5; ++ty) {
                    const uint32_t f = (cur[k] - pred[ty]) & 255u;
                    cost[ty] += f < 128u ? f : 256u - f;
                }
            }
        }
        int type = 0;
        uint32_t best = png_wave_sum(cost[0]);
#pragma unroll
        for (int ty = 1; ty < 5; ++ty) {
            const uint32_t c = png_wave_sum(cost[ty]);
            if (c < best) { best = c; type = ty; }                // (a tie keeps the lower type)
        }
        unsigned char* dst = filt + (t * H + r) * (int64_t)stride;
        const uint32_t row_pos = (uint32_t)(r - r0) * (uint32_t)stride;
        if (lane == 0) {
            dst[0] = (unsigned char)type;
            atomicAdd(&whist[wave][type], 1u);
            s1 += (uint32_t)type;
            s2 += (uint64_t)(seglen - row_pos) * (uint32_t)type;
        }
        for (int x = lane; x < W; x += 64) {
            uint32_t cur[BPP], lf[BPP], up[BPP], ul[BPP];
            png_neighbours<KIND, DEPTH, C>(frames, row_px, W, x, top, cur, lf, up, ul);
#pragma unroll
            for (int k = 0; k < BPP; ++k) {
                const uint32_t pred = type == 0 ? 0u : type == 1 ? lf[k] : type == 2 ? up[k] : type == 3 ? (lf[k] + up[k]) >> 1
                                                                                                        : png_paeth(lf[k], up[k], ul[k]);
                const uint32_t f = (cur[k] - pred) & 255u;
                const uint32_t pos = row_pos + 1u + (uint32_t)x * BPP + k;
                dst[1 + (int64_t)x * BPP + k] = (unsigned char)f;
                atomicAdd(&whist[wave][f], 1u);
                s1 += f;
                s2 += (uint64_t)(seglen - pos) * f;
            }
        }
    }
    {
        const uint32_t a = png_wave_sum((uint32_t)(s1 % PNG_ADLER)), b = png_wave_sum((uint32_t)(s2 % PNG_ADLER));
        if (lane == 0) { atomicAdd(&adler[0], a % PNG_ADLER); atomicAdd(&adler[1], b % PNG_ADLER); }
    }
    __syncthreads();
    for (int s = tid; s < PNG_SYMS; s += 256) hist[s] = s < 256 ? whist[0][s] + whist[1][s] + whist[2][s] + whist[3][s] : 1u;
    const uint64_t bits = png_build_code<PNG_SYMS>(hist, sw, tid);
    if (tid == 0) {
        uint32_t* m = meta + ((int64_t)blockIdx.x) * 4;
        m[0] = (uint32_t)((PNG_HEADER_BITS + bits + 3 + 7) / 8 + 4);
        m[1] = adler[0] % PNG_ADLER;
        m[2] = adler[1] % PNG_ADLER;
        m[3] = (uint32_t)bits;                                    // (the literal block's data bits: png_runs_kernel's; < 2^28)
    }
    uint32_t* tab = table + ((int64_t)blockIdx.x) * PNG_TABLE;
    for (int s = tid; s < PNG_TABLE; s += 256) tab[s] = s < PNG_SYMS ? sw[s] : 0u;
}

// ---- run-length matches (pngenc.py "Runs"): the tokens of a tile, the second code, the choice
struct PngTokLds {
    uint32_t first[256 + PNG_LOOK];                               // per group of PNG_RUN positions: its first run start, or PNG_NONE
    uint32_t wmax[4];
};

// the length symbol 257..285 of a match of c = 3..258 bytes, the number of its extra bits and their value (RFC 1951, 3.2.5)
SVR_DEVICE void png_length_symbol(uint32_t c, uint32_t& sym, uint32_t& extra_n, uint32_t& extra_v) {
    const uint32_t m = c - 3u;
    extra_n = (m < 8u || c == PNG_MAX_MATCH) ? 0u : 29u - (uint32_t)__clz(m);      // floor(log2 m) - 2
    extra_v = m & ((1u << extra_n) - 1u);
    sym = c == PNG_MAX_MATCH ? 285u : 257u + 4u * extra_n + (m >> extra_n);
}

// The tokens of the positions [base, base + PNG_TILE) of a segment of n filtered bytes ``src``; every thread of the workgroup
// calls this, tile after tile in ascending order; lane tid owns the positions base + PNG_RUN tid + j.  tok[j]: a literal's byte
// 0..255; 256 + c for the head of a match of c bytes; PNG_NONE for a position that emits nothing (covered by a match, or at /
// past the segment's end).  A position starts a run if it is position 0 or its byte differs from the one before; positions from n
// on count as starts too, so a run ends with the segment whatever follows it in memory.
//   forward   each lane's last start, a workgroup-wide running maximum: the start s of the run a lane's stretch begins in --
//             ``run_start`` carries it from tile to tile, so a run may be as long as the segment;
//   backward  a match covers at most 258 bytes, so min(rem, 258) is enough (rem: the bytes left in the run): a lane looks for the
//             next start in the PNG_LOOK groups behind its own, PNG_LOOK of them lying past the tile (their first starts are
//             found by the first PNG_LOOK lanes).
// With o = i - s and q = (o - 1) % 258 the specification's c is min(258, rem + q).
SVR_DEVICE void png_tile_tokens(const unsigned char* __restrict__ src, uint32_t n, uint32_t base, int tid, PngTokLds& L,
                                uint32_t& run_start, uint32_t* tok) {
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t i0 = base + (uint32_t)tid * PNG_RUN;
    uint32_t b[PNG_RUN + 1];
    b[0] = (i0 > 0u && i0 <= n) ? src[i0 - 1u] : 0u;
    uint32_t starts = 0;                                          // bit j: position i0 + j starts a run
#pragma unroll
    for (int j = 0; j < PNG_RUN; ++j) {
        const uint32_t i = i0 + j;
        b[j + 1] = i < n ? src[i] : 0u;
        if (i == 0u || i >= n || b[j + 1] != b[j]) starts |= 1u << j;
    }
    __syncthreads();                                              // (the tile before is done with L)
    L.first[tid] = starts ? i0 + (uint32_t)__ffs((int)starts) - 1u : PNG_NONE;
    if (tid < PNG_LOOK) {
        const uint32_t h0 = base + PNG_TILE + (uint32_t)tid * PNG_RUN;
        uint32_t f = PNG_NONE;
        for (int j = PNG_RUN - 1; j >= 0; --j) {                  // (descending: the first start is the last one assigned)
            const uint32_t i = h0 + j;
            if (i >= n || src[i] != src[i - 1u]) f = i;
        }
        L.first[256 + tid] = f;
    }
    uint32_t v = starts ? i0 + (32u - (uint32_t)__clz(starts)) : 0u;      // 1 + the lane's last start
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v = max(v, o);
    }
    if (lane == 63) L.wmax[wave] = v;
    uint32_t enter = (uint32_t)__shfl_up((int)v, 1);
    if (lane == 0) enter = 0u;
    __syncthreads();
    uint32_t last = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const uint32_t x = L.wmax[w]; last = max(last, x); if (w < wave) enter = max(enter, x); }
    uint32_t s = enter ? enter - 1u : run_start;
    run_start = last ? last - 1u : run_start;
    uint32_t next = i0 + PNG_RUN * (PNG_LOOK + 1);                // the next start behind the lane's stretch (>= 258 away if none)
#pragma unroll
    for (int g = PNG_LOOK; g >= 1; --g) { const uint32_t f = L.first[tid + g]; if (f != PNG_NONE) next = f; }
    uint32_t rem[PNG_RUN];
#pragma unroll
    for (int j = PNG_RUN - 1; j >= 0; --j) {
        rem[j] = next - (i0 + j);
        if ((starts >> j) & 1u) next = i0 + j;
    }
#pragma unroll
    for (int j = 0; j < PNG_RUN; ++j) {
        const uint32_t i = i0 + j;
        if ((starts >> j) & 1u) s = i;
        const uint32_t o = i - s, q = o ? (o - 1u) % PNG_MAX_MATCH : 0u;
        uint32_t t = PNG_NONE;
        if (i < n) {
            if (o == 0u || rem[j] + q < 3u) t = b[j + 1];
            else if (q == 0u) t = 256u + min(rem[j], PNG_MAX_MATCH);
        }
        tok[j] = t;
    }
}

// One workgroup per (frame, segment), behind png_filter_kernel: the histogram of the tokens over 286 symbols, the second code, the
// choice.  In: meta[3] = the literal block's data bits.  Out: meta[3] = 1 if the segment is written as a run block -- then meta[0] is
// that block's size and table2 its code --, else 0 and nothing else changes.
__global__ __launch_bounds__(256) void png_runs_kernel(const unsigned char* __restrict__ filt, uint32_t* __restrict__ table2,
                                                       uint32_t* __restrict__ meta, int H, int stride, int R, int nseg) {
    __shared__ PngTokLds tl;
    __shared__ uint32_t whist[4][PNG_RUN_SYMS];
    __shared__ uint32_t hist[PNG_RUN_SYMS], sw[2 * PNG_RUN_SYMS], chosen_s;
    const int seg = (int)(blockIdx.x % (unsigned)nseg);
    const int64_t t = blockIdx.x / (unsigned)nseg;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int r0 = seg * R, r1 = min(H, r0 + R);
    const uint32_t n = (uint32_t)(r1 - r0) * (uint32_t)stride;
    const unsigned char* src = filt + (t * H + r0) * (int64_t)stride;
    for (int i = tid; i < 4 * PNG_RUN_SYMS; i += 256) (&whist[0][0])[i] = 0;
    __syncthreads();
    uint32_t run_start = 0;
    for (uint32_t base = 0; base < n; base += PNG_TILE) {
        uint32_t tok[PNG_RUN];
        png_tile_tokens(src, n, base, tid, tl, run_start, tok);
#pragma unroll
        for (int j = 0; j < PNG_RUN; ++j) {
            if (tok[j] == PNG_NONE) continue;
            uint32_t sym = tok[j], en, ev;
            if (sym >= 256u) png_length_symbol(sym - 256u, sym, en, ev);
            atomicAdd(&whist[wave][sym], 1u);
        }
    }
    __syncthreads();
    for (int s = tid; s < PNG_RUN_SYMS; s += 256) hist[s] = s == 256 ? 1u : whist[0][s] + whist[1][s] + whist[2][s] + whist[3][s];
    __syncthreads();
    uint32_t matches = 0, extra = 0;                              // (every thread sums the 29 counts: the branch below is uniform)
    for (int s = 257; s < PNG_RUN_SYMS; ++s) {
        const uint32_t c = hist[s];
        matches += c;
        extra += c * ((s < 265 || s == 285) ? 0u : (uint32_t)(s - 261) >> 2);
    }
    uint32_t* m = meta + ((int64_t)blockIdx.x) * 4;
    if (matches == 0u) {
        if (tid == 0) m[3] = 0;
        return;
    }
    const uint64_t bits = png_build_code<PNG_RUN_SYMS>(hist, sw, tid);
    if (tid == 0) {
        const uint64_t bits_runs = PNG_RUN_HEADER_BITS + bits + extra + matches, bits_lit = (uint64_t)PNG_HEADER_BITS + m[3];
        const bool chosen = bits_runs < bits_lit;
        if (chosen) m[0] = (uint32_t)((bits_runs + 3 + 7) / 8 + 4);
        m[3] = chosen ? 1u : 0u;
        chosen_s = chosen ? 1u : 0u;
    }
    __syncthreads();
    if (chosen_s) {
        uint32_t* tab = table2 + ((int64_t)blockIdx.x) * PNG_RUN_TABLE;
        for (int s = tid; s < PNG_RUN_TABLE; s += 256) tab[s] = s < PNG_RUN_SYMS ? sw[s] : 0u;
    }
}

// one workgroup per frame: segment offsets, sizes[t], the Adler-32 and the stream's head and tail
__global__ __launch_bounds__(256) void png_scan_kernel(const uint32_t* __restrict__ meta, int64_t* __restrict__ segoff,
                                                       unsigned char* __restrict__ out, int64_t cap, int64_t* __restrict__ sizes, int H,
                                                       int stride, int R, int nseg) {
    __shared__ uint64_t pbytes[256];
    __shared__ uint32_t pl[256], pa[256], pb[256], fin[2];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x;
    const int chunk = (nseg + 255) / 256, lo = min(nseg, tid * chunk), hi = min(nseg, lo + chunk);
    const uint32_t* m = meta + t * nseg * 4;
    uint64_t bytes = 0, l = 0, a = 0, b = 0;                      // this chunk's (length, byte sum, weighted sum), modulo 65521
    for (int s = lo; s < hi; ++s) {
        const uint64_t ls = (uint64_t)(min(H, (s + 1) * R) - s * R) * (uint64_t)stride % PNG_ADLER;
        bytes += m[4 * s];
        b = (b + ls * a + m[4 * s + 2]) % PNG_ADLER;              // (the bytes before gain this segment's length in weight)
        a = (a + m[4 * s + 1]) % PNG_ADLER;
        l = (l + ls) % PNG_ADLER;
    }
    pbytes[tid] = bytes; pl[tid] = (uint32_t)l; pa[tid] = (uint32_t)a; pb[tid] = (uint32_t)b;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0, L = 0, A = 0, B = 0;
        for (int i = 0; i < 256; ++i) {
            const uint64_t nb = pbytes[i];
            pbytes[i] = run;
            run += nb;
            B = (B + (uint64_t)pl[i] * A + pb[i]) % PNG_ADLER;
            A = (A + pa[i]) % PNG_ADLER;
            L = (L + pl[i]) % PNG_ADLER;
        }
        fin[0] = (uint32_t)((1u + A) % PNG_ADLER);                // Adler-32 starts from A = 1, B = 0
        fin[1] = (uint32_t)((L + B) % PNG_ADLER);
        const int64_t total = 2 + (int64_t)run + 6;
        sizes[t] = total;
        unsigned char* o = out + t * cap;
        if (total <= cap) {
            o[0] = 0x78; o[1] = 0x01;
            unsigned char* tail = o + 2 + run;
            tail[0] = 0x03; tail[1] = 0x00;
            tail[2] = (unsigned char)(fin[1] >> 8); tail[3] = (unsigned char)(fin[1] & 255u);
            tail[4] = (unsigned char)(fin[0] >> 8); tail[5] = (unsigned char)(fin[0] & 255u);
        }
    }
    __syncthreads();
    int64_t off = 2 + (int64_t)pbytes[tid];
    for (int s = lo; s < hi; ++s) {
        segoff[t * nseg + s] = off;
        off += m[4 * s];
    }
}

// RUNS: a segment whose meta[3] is set (png_runs_kernel) is written as a run block from table2; the others, and every segment
// without RUNS, as the literal block from table.  An entry e[j] of the tile is value | bits << SH: 16 + 15 bits without RUNS, up
// to 21 bits of value (code, extra bits, the distance bit 0) with them.
template <bool RUNS>
__global__ __launch_bounds__(256) void png_pack_kernel(const unsigned char* __restrict__ filt, const uint32_t* __restrict__ table,
                                                       const uint32_t* __restrict__ table2, const uint32_t* __restrict__ meta,
                                                       const int64_t* __restrict__ segoff, unsigned char* __restrict__ out, int64_t cap,
                                                       int H, int stride, int R, int nseg) {
    constexpr uint32_t SH = RUNS ? 24u : 16u, MASK = (1u << SH) - 1u;
    __shared__ uint32_t tab[RUNS ? PNG_RUN_TABLE : PNG_TABLE];
    __shared__ uint32_t buf[PNG_BUF_WORDS];
    __shared__ uint32_t wsum[4];
    __shared__ PngTokLds tl;
    const int seg = (int)(blockIdx.x % (unsigned)nseg);
    const int64_t t = blockIdx.x / (unsigned)nseg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = seg * R, r1 = min(H, r0 + R);
    const int64_t n = (int64_t)(r1 - r0) * stride;                // the segment's bytes; symbol n is the end of the block
    const unsigned char* src = filt + (t * H + r0) * (int64_t)stride;
    const int64_t off0 = segoff[blockIdx.x];
    unsigned char* dst = out + t * cap + off0;
    const int64_t room = cap - off0;                              // no store at or beyond dst[room]
    const bool runs = RUNS && meta[(int64_t)blockIdx.x * 4 + 3] != 0u;       // (uniform over the workgroup)
    if (runs) for (int i = tid; i < PNG_RUN_TABLE; i += 256) tab[i] = table2[(int64_t)blockIdx.x * PNG_RUN_TABLE + i];
    else for (int i = tid; i < PNG_TABLE; i += 256) tab[i] = table[(int64_t)blockIdx.x * PNG_TABLE + i];
    for (int i = tid; i < PNG_BUF_WORDS; i += 256) buf[i] = 0;
    __syncthreads();

    // whole bytes of buf (bits [0, carried + added)) -> dst at byte ``at``; the partial last byte carried to byte 0 of a zeroed buf
    auto flush = [&](int64_t at, uint32_t carried, uint32_t added) {
        const uint32_t end = carried + added, nfull = end >> 3;
        const uint32_t carry = (end & 7u) ? (buf[nfull >> 2] >> (8u * (nfull & 3u))) & 255u : 0u;
        for (uint32_t j = tid; j < nfull; j += 256)
            if (at + j < room) dst[at + j] = (unsigned char)((buf[j >> 2] >> (8u * (j & 3u))) & 255u);
        __syncthreads();
        for (uint32_t w = tid; w <= ((end + 31u) >> 5) && w < (uint32_t)PNG_BUF_WORDS; w += 256) buf[w] = w == 0 ? carry : 0u;
        __syncthreads();
    };

    // the block header: 17 bits, nineteen 3-bit lengths (4 for the code-length symbols 0..15: all but the first three in the
    // transmitted order), 258 lengths as 4-bit codes (symbol v has code v: written bit-reversed) -- 287 in a run block: HLIT = 29,
    // 286 lengths and the one distance code's length 1
    const int nsyms = runs ? PNG_RUN_SYMS : PNG_SYMS, header_bits = runs ? PNG_RUN_HEADER_BITS : PNG_HEADER_BITS;
    if (tid == 19) atomicOr(&buf[0], (1u << 2) | (runs ? 29u << 3 : 0u) | (15u << 13));      // BTYPE = 10 (its high bit), HLIT, HCLEN = 15
    if (tid >= 3 && tid < 19) { const uint32_t bit = 17u + 3u * tid + 2u; atomicOr(&buf[bit >> 5], 1u << (bit & 31u)); }
    for (int i = tid; i < nsyms + 1; i += 256) {
        const uint32_t l = i < nsyms ? tab[i] >> 16 : (runs ? 1u : 0u);
        const uint32_t v = __brev(l) >> 28, bit = 74u + 4u * i, sh = bit & 31u;
        if (v) {
            atomicOr(&buf[bit >> 5], v << sh);
            if (sh > 28u) atomicOr(&buf[(bit >> 5) + 1], v >> (32u - sh));
        }
    }
    __syncthreads();
    flush(0, 0u, (uint32_t)header_bits);
    int64_t bitpos = header_bits;
    uint32_t run_start = 0;

    for (int64_t base = 0; base <= n; base += PNG_TILE) {
        const int64_t i0 = base + (int64_t)tid * PNG_RUN;
        uint32_t e[PNG_RUN], nb = 0;
        if (runs) {
            uint32_t tok[PNG_RUN];
            png_tile_tokens(src, (uint32_t)n, (uint32_t)base, tid, tl, run_start, tok);
#pragma unroll
            for (int j = 0; j < PNG_RUN; ++j) {
                uint32_t v = 0, bits = 0;
                if (tok[j] < 256u || i0 + j == n) {
                    const uint32_t c = tab[i0 + j == n ? 256u : tok[j]];
                    v = c & 0xFFFFu;
                    bits = c >> 16;
                } else if (tok[j] != PNG_NONE) {
                    uint32_t sym, en, ev;
                    png_length_symbol(tok[j] - 256u, sym, en, ev);
                    const uint32_t c = tab[sym];
                    v = (c & 0xFFFFu) | (ev << (c >> 16));
                    bits = (c >> 16) + en + 1u;
                }
                e[j] = v | (bits << SH);
                nb += bits;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PNG_RUN; ++j) {
                const int64_t i = i0 + j;
                const uint32_t c = i < n ? tab[src[i]] : (i == n ? tab[256] : 0u);
                e[j] = RUNS ? (c & 0xFFFFu) | (c >> 16 << SH) : c;
                nb += c >> 16;
            }
        }
        uint32_t v = nb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)v, d);
            if (lane >= d) v += o;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint32_t x = wsum[w]; total += x; if (w < wave) before += x; }
        const uint32_t carried = (uint32_t)(bitpos & 7);
        const uint32_t pos = carried + before + v - nb;
        uint32_t word = pos >> 5, fill = pos & 31u;
        uint64_t acc = 0;
#pragma unroll
        for (int j = 0; j < PNG_RUN; ++j) {
            acc |= (uint64_t)(e[j] & MASK) << fill;
            fill += e[j] >> SH;
            if (fill >= 32u) {
                if (word < (uint32_t)PNG_BUF_WORDS) atomicOr(&buf[word], (uint32_t)acc);
                ++word;
                acc >>= 32;
                fill -= 32u;
            }
        }
        if (fill && word < (uint32_t)PNG_BUF_WORDS) atomicOr(&buf[word], (uint32_t)acc);
        __syncthreads();
        flush(bitpos >> 3, carried, total);
        bitpos += total;
    }
    if (tid == 0) {                                               // the empty stored block: 000, padding, 00 00 FF FF
        const int64_t p = bitpos >> 3, end = (bitpos + 3 + 7) >> 3;
        if (p < room) dst[p] = (unsigned char)(buf[0] & 255u);
        if (end > p + 1 && p + 1 < room) dst[p + 1] = 0;
        if (end + 3 < room) { dst[end] = 0; dst[end + 1] = 0; dst[end + 2] = 0xFF; dst[end + 3] = 0xFF; }
    }
}

}  // namespace svr
