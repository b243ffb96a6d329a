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
constexpr int PNG_BUF_WORDS = PNG_TILE * 15 / 32 + 2;      // 7 carried bits + PNG_TILE symbols of at most 15 bits

static int g_png_passes = 3;                       // svr_set_option("png_passes"): measurement only, 3 = the whole encoder

struct PngLayout {
    int bpp, stride, R, nseg;
    int64_t filt_off, table_off, meta_off, segoff_off, scratch_bytes, capacity;
};

// (pngenc.geometry / frame_bound; the scratch: filtered bytes | tables | {bytes, adler s1, s2, 0} per segment | segment offsets)
static inline PngLayout png_layout(int64_t T, int64_t H, int64_t W, int C, int depth) {
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
    L.scratch_bytes = L.segoff_off + segs * 8;
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

template <int KIND, int DEPTH, int C>
__global__ __launch_bounds__(256) void png_filter_kernel(const void* __restrict__ frames, unsigned char* __restrict__ filt,
                                                         uint32_t* __restrict__ table, uint32_t* __restrict__ meta, int H, int W, int R,
                                                         int nseg) {
    constexpr int BPP = C * DEPTH / 8;
    __shared__ uint32_t whist[4][256];
    __shared__ uint32_t hist[PNG_SYMS], cnt[PNG_SYMS], len_s[PNG_SYMS];
    __shared__ uint32_t sw[2 * PNG_SYMS];                         // weights: the sorted leaves, then the internal nodes
    __shared__ unsigned short ssym[PNG_SYMS], parent[2 * PNG_SYMS], depth_s[2 * PNG_SYMS];
    __shared__ uint32_t blc[17], nxt[17];
    __shared__ uint32_t adler[2], ctl[2];
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
    for (int s = tid; s < PNG_SYMS; s += 256) {
        const uint32_t c = s < 256 ? whist[0][s] + whist[1][s] + whist[2][s] + whist[3][s] : 1u;
        hist[s] = cnt[s] = c;
        len_s[s] = 0;
    }

    // the code: two-queue Huffman over the used symbols, counts halved (rounding up) while the tree is deeper than 15
    for (;;) {
        __syncthreads();
        for (int s = tid; s < PNG_SYMS; s += 256) {
            const uint32_t c = cnt[s];
            if (c) {
                int rank = 0;
                for (int j = 0; j < PNG_SYMS; ++j) {
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
            for (int s = 0; s < PNG_SYMS; ++s) n += cnt[s] != 0u ? 1 : 0;
            int leaf = 0, node = n;                               // (n >= 2: a type byte and the end-of-block symbol)
            for (int k = n; k < 2 * n - 1; ++k) {
                uint32_t w = 0;
                for (int rep = 0; rep < 2; ++rep) {
                    const bool take_leaf = leaf < n && (node >= k || sw[leaf] <= sw[node]);
                    const int pick = take_leaf ? leaf++ : node++;
                    w += sw[pick];
                    parent[pick] = (unsigned short)k;
                }
                sw[k] = w;
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
        for (int s = tid; s < PNG_SYMS; s += 256) {
            const uint32_t c = cnt[s];
            cnt[s] = c ? (c + 1u) >> 1 : 0u;
        }
    }
    for (int i = tid; i < (int)ctl[0]; i += 256) len_s[ssym[i]] = depth_s[i];
    __syncthreads();
    uint32_t* tab = table + ((int64_t)blockIdx.x) * PNG_TABLE;
    if (tid == 0) {                                               // canonical codes (RFC 1951, 3.2.2), stored bit-reversed
        for (int b = 0; b <= 16; ++b) blc[b] = 0;
        for (int s = 0; s < PNG_SYMS; ++s) blc[len_s[s]] += 1u;
        blc[0] = 0;
        uint32_t code = 0;
        nxt[0] = 0;
        for (int b = 1; b <= 15; ++b) { code = (code + blc[b - 1]) << 1; nxt[b] = code; }
        uint64_t bits = 0;
        for (int s = 0; s < PNG_SYMS; ++s) {
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
        uint32_t* m = meta + ((int64_t)blockIdx.x) * 4;
        m[0] = (uint32_t)((PNG_HEADER_BITS + bits + 3 + 7) / 8 + 4);
        m[1] = adler[0] % PNG_ADLER;
        m[2] = adler[1] % PNG_ADLER;
        m[3] = 0;
    }
    __syncthreads();
    for (int s = tid; s < PNG_TABLE; s += 256) tab[s] = s < PNG_SYMS ? sw[s] : 0u;
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

__global__ __launch_bounds__(256) void png_pack_kernel(const unsigned char* __restrict__ filt, const uint32_t* __restrict__ table,
                                                       const int64_t* __restrict__ segoff, unsigned char* __restrict__ out, int64_t cap,
                                                       int H, int stride, int R, int nseg) {
    __shared__ uint32_t tab[PNG_TABLE];
    __shared__ uint32_t buf[PNG_BUF_WORDS];
    __shared__ uint32_t wsum[4];
    const int seg = (int)(blockIdx.x % (unsigned)nseg);
    const int64_t t = blockIdx.x / (unsigned)nseg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = seg * R, r1 = min(H, r0 + R);
    const int64_t n = (int64_t)(r1 - r0) * stride;                // the segment's bytes; symbol n is the end of the block
    const unsigned char* src = filt + (t * H + r0) * (int64_t)stride;
    const int64_t off0 = segoff[blockIdx.x];
    unsigned char* dst = out + t * cap + off0;
    const int64_t room = cap - off0;                              // no store at or beyond dst[room]
    for (int i = tid; i < PNG_TABLE; i += 256) tab[i] = table[(int64_t)blockIdx.x * PNG_TABLE + i];
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
    // transmitted order), 258 lengths as 4-bit codes (symbol v has code v: written bit-reversed)
    if (tid == 19) atomicOr(&buf[0], (1u << 2) | (15u << 13));    // BTYPE = 10 (its high bit), HCLEN = 15
    if (tid >= 3 && tid < 19) { const uint32_t bit = 17u + 3u * tid + 2u; atomicOr(&buf[bit >> 5], 1u << (bit & 31u)); }
    for (int i = tid; i < 258; i += 256) {
        const uint32_t l = i < PNG_SYMS ? tab[i] >> 16 : 0u;
        const uint32_t v = __brev(l) >> 28, bit = 74u + 4u * i, sh = bit & 31u;
        if (v) {
            atomicOr(&buf[bit >> 5], v << sh);
            if (sh > 28u) atomicOr(&buf[(bit >> 5) + 1], v >> (32u - sh));
        }
    }
    __syncthreads();
    flush(0, 0u, PNG_HEADER_BITS);
    int64_t bitpos = PNG_HEADER_BITS;

    for (int64_t base = 0; base <= n; base += PNG_TILE) {
        const int64_t i0 = base + (int64_t)tid * PNG_RUN;
        uint32_t e[PNG_RUN], nb = 0;
#pragma unroll
        for (int j = 0; j < PNG_RUN; ++j) {
            const int64_t i = i0 + j;
            e[j] = i < n ? tab[src[i]] : (i == n ? tab[256] : 0u);
            nb += e[j] >> 16;
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
            acc |= (uint64_t)(e[j] & 0xFFFFu) << fill;
            fill += e[j] >> 16;
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
