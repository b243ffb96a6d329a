"""PNG output encoded where the frames live: the zlib stream, stated once, in plain Python / numpy / torch.

This module is the specification of the kernels in csrc/svr_png.hip (equal BYTE FOR BYTE: ``HipOps.encode_png`` against
``encode_frames_spec``), as frameio.py is for the pack kernels, plus the host-side PNG plumbing of the command line (framing, a
16-bit reader, a general writer for frames that are not on a device).  Any device.

``frames`` [T, H, W, C], fp32 or bf16, C = 3 or 4; ``depth`` 8 or 16.  Samples are frameio.codes(frames, 255.0 | 65535.0) -- its
NaN / +-inf rules included --, 16-bit samples stored big-endian.  bpp = C * depth / 8 bytes per pixel, stride = 1 + W * bpp bytes
per filtered row.  Every frame is independent: one zlib stream each.

Filtering   Per row one of the PNG filter types 0..4 (None, Sub, Up, Average, Paeth) exactly as the PNG specification defines them:
            the row before row 0 and the bytes left of byte ``bpp`` are zero, Average uses floor((a + b) / 2), Paeth breaks ties
            in the order a, b, c.  The chosen type minimises the sum over the row's filtered bytes f of (f < 128 ? f : 256 - f); a
            tie goes to the lowest type.  The filtered row is the type byte followed by the W * bpp filtered bytes.
Segments    R = max(1, 65536 // stride) rows per segment; segment s covers rows [s R, min(H, (s + 1) R)) (the last may be ragged).
            A segment is one deflate block -- and the unit of parallel work on the device.
Lengths     Per segment the histogram of its bytes (type bytes included) over symbols 0..255, plus symbol 256 (end of block) with
            count 1.  Huffman lengths by the two-queue construction: the used symbols as leaves sorted by (count, symbol), internal
            nodes in creation order, each pick takes the smaller weight and a tie goes to the leaf queue.  If the deepest leaf is
            below 16 bits those are the lengths; otherwise every non-zero count c becomes (c + 1) >> 1, the tree is rebuilt, and so
            on.  (A single used symbol cannot occur: symbol 256 is always there beside at least one type byte.)  Codes are
            canonical (RFC 1951, 3.2.2).
Block bits  LSB-first packing, Huffman codes bit-reversed, as deflate requires:
              1. BFINAL = 0, BTYPE = 10 (dynamic), HLIT = 0 (257 codes), HDIST = 0 (1 code), HCLEN = 15 (all 19 lengths);
              2. the nineteen 3-bit code-length-code lengths in the order 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14,
                 1, 15: 4 for the symbols 0..15, 0 for 16, 17, 18 -- a complete code in which symbol v has the 4-bit code v;
              3. 258 lengths, each as that 4-bit code: the 257 literal / end-of-block lengths, then ONE distance length of 0 (no
                 distance code exists and none is used: the stream holds literals only);
              4. the segment's bytes, then symbol 256;
              5. an empty stored block, so that segments are byte-aligned and concatenate: bits 000, zero padding to the next
                 byte, then 00 00 FF FF.
            The header (1. to 3.) is HEADER_BITS = 1106 bits.
Stream      78 01, the segments in order, 03 00 (a final empty fixed block), the Adler-32 of all filtered bytes, big-endian.
File        signature, IHDR(W, H, depth, colour type 2 | 6, 0, 0, 0), ONE IDAT, IEND; chunk CRCs by zlib.crc32 on the host.
Capacity    A segment of n filtered bytes takes at most segment_bound(n) = 139 + ceil(15 (n + 1) / 8) + 5 bytes with any code
            limited to 15 bits: it takes exactly ceil((1106 + data bits + 3) / 8) + 4 with data bits <= 15 (n + 1), and
            ceil(1109 / 8) = 139.  A frame takes at most frame_bound(H, W, C, depth) = 2 + the sum of its segments' bounds + 6.  Both
            are asserted here.

Without ``runs`` there are no LZ77 matches and no run lengths: Huffman-only output floors at one bit per byte, so a flat frame
compresses 8 : 1 and no better.

Runs        ``runs=True`` (RUNS is the switch the command line reads) changes a segment's deflate block and nothing else: filtering,
            segments, the Adler-32, 78 01 ... 03 00, the empty stored block behind every segment and the framing stay.  Matches are
            runs of one byte at DISTANCE 1 only -- a scan, not a string search; other distances would need only more distance
            codes, and there are still no general matches.
Tokens      The segment's n filtered bytes, type bytes included, split into maximal runs of equal bytes; matches never leave the
            segment.  Position i lies in the run [s, s + L) and has o = i - s.  o = 0: a literal.  o >= 1: with k = (o - 1) // 258,
            j = (o - 1) % 258 and c = min(258, L - 1 - 258 k): c < 3 -> a literal; else j = 0 -> a match of length c at distance 1;
            else the position emits nothing.  So a run of L <= 3 is all literals; a longer one is a literal, (L - 1) // 258 matches
            of 258 and a remainder that is one match if it is >= 3 and one or two literals otherwise.  (With rem = s + L - i the
            bytes left in the run: L - 1 - 258 k = rem + j, so a position's token follows from o and min(rem, 258) alone.)
Code        The histogram over symbols 0..285: the literals that are emitted, symbol 256 with count 1, the length symbols 257..285
            (RFC 1951, 3.2.5) of the matches.  Lengths by code_lengths, fed 286 counts; codes canonical.  The distance alphabet has
            ONE code, symbol 0 (distance 1), of length 1.
Run block     1. BFINAL = 0, BTYPE = 10, HLIT = 29 (286 codes), HDIST = 0, HCLEN = 15;
              2. the same nineteen 3-bit code-length-code lengths;
              3. 286 length nibbles, then one distance nibble for length 1;
              4. the tokens in order: a literal is its code; a match is the length symbol's code, its extra bits (c - base, least
                 significant bit first), then the one distance bit 0;
              5. symbol 256, then the empty stored block.
            The header is RUN_HEADER_BITS = 17 + 57 + 4 * 287 = 1222 bits; the data bits stay <= 15 (n + 1): a match costs at most
            15 + 5 + 1 = 21 bits and covers at least 3 bytes.
Choice      Per segment: bits_lit = 1106 + sum hist_lit len_lit, bits_runs = 1222 + sum hist_runs len_runs + the extra bits + the
            number of matches.  The run block is written iff the segment has at least one match and bits_runs < bits_lit, strictly;
            otherwise the segment is the literal block, byte for byte.  So no stream is longer than the literal one --
            segment_bound and frame_bound hold unchanged, asserted here -- and a frame without a useful run gives the same bytes.
"""
import struct
import zlib

import numpy as np
import torch

from . import frameio

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS = 1106
RUN_HEADER_BITS = 1222
MAX_BITS = 15
SEGMENT_BYTES = 65536
MAX_MATCH = 258
# RFC 1951, 3.2.5: the base length and the number of extra bits of the length symbols 257..285
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
# The switch the command line reads (inference_cli.py's writer factory): png output is written with run-length matches.
RUNS = True
LITERAL, MATCH, COVERED = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------- geometry
def geometry(H: int, W: int, C: int, depth: int):
    """-> (bpp, stride, R, segments); raises for a channel count or depth the stream does not take."""
    if C not in (3, 4):
        raise ValueError(f"C must be 3 or 4, got C = {C}")
    if depth not in (8, 16):
        raise ValueError(f"depth must be 8 or 16, got {depth}")
    if H < 1 or W < 1:
        raise ValueError(f"need H >= 1 and W >= 1, got {H} x {W}")
    bpp = C * depth // 8
    stride = 1 + W * bpp
    R = max(1, SEGMENT_BYTES // stride)
    return bpp, stride, R, -(-H // R)


def segment_bound(n: int) -> int:
    return 139 + (15 * (n + 1) + 7) // 8 + 5


def frame_bound(H: int, W: int, C: int, depth: int) -> int:
    """Bytes that hold the zlib stream of any frame of this geometry (the per-frame capacity of HipOps.encode_png's ``out``)."""
    _, stride, R, nseg = geometry(H, W, C, depth)
    return 2 + sum(segment_bound((min(H, (s + 1) * R) - s * R) * stride) for s in range(nseg)) + 6


# ---------------------------------------------------------------------------------------------------------------- filtering
def sample_bytes(samples: np.ndarray, depth: int) -> np.ndarray:
    """samples [H, W, C] (integers) -> uint8 [H, W * bpp], 16-bit samples big-endian"""
    H = samples.shape[0]
    if depth == 8:
        return np.ascontiguousarray(samples.astype(np.uint8)).reshape(H, -1)
    return np.ascontiguousarray(samples.astype(">u2")).view(np.uint8).reshape(H, -1)


def filter_candidates(samples: np.ndarray, depth: int) -> np.ndarray:
    """-> int32 [5, H, W * bpp]: every row filtered with each of the five types"""
    bpp = samples.shape[2] * depth // 8
    raw = sample_bytes(samples, depth).astype(np.int32)
    a, b, c = np.zeros_like(raw), np.zeros_like(raw), np.zeros_like(raw)
    a[:, bpp:] = raw[:, :-bpp]
    b[1:] = raw[:-1]
    c[1:, bpp:] = raw[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([raw, raw - a, raw - b, raw - ((a + b) >> 1), raw - paeth]) & 255


def filter_rows(samples: np.ndarray, depth: int) -> np.ndarray:
    """samples [H, W, C] -> uint8 [H, stride]: per row the chosen type byte and the filtered bytes"""
    cand = filter_candidates(samples, depth)
    H = cand.shape[1]
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)
    ftype = cost.argmin(axis=0)                                              # (the first minimum: a tie goes to the lowest type)
    out = np.empty((H, 1 + cand.shape[2]), dtype=np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = cand[ftype, np.arange(H)]
    return out


def unfilter(data, W: int, H: int, C: int, depth: int) -> np.ndarray:
    """The decoder: H * stride filtered bytes -> samples uint8 / uint16 [H, W, C].  Rows of type 0, 1, 2 in numpy; Average and
    Paeth rows pixel by pixel (each byte depends on the one before)."""
    bpp, stride, _, _ = geometry(H, W, C, depth)
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    if data.size != H * stride:
        raise ValueError(f"{H} rows of {stride} bytes are {H * stride} bytes, got {data.size}")
    rows = data.reshape(H, stride)
    out = np.zeros((H, W * bpp), dtype=np.uint8)
    prev = np.zeros(W * bpp, dtype=np.uint8)
    for y in range(H):
        ftype, f = int(rows[y, 0]), rows[y, 1:]
        if ftype == 0:
            cur = f.copy()
        elif ftype == 1:
            cur = (np.cumsum(f.reshape(W, bpp).astype(np.int64), axis=0) & 255).astype(np.uint8).reshape(-1)
        elif ftype == 2:
            cur = f + prev
        elif ftype in (3, 4):
            fl, up = f.reshape(W, bpp).astype(np.int32), prev.reshape(W, bpp).astype(np.int32)
            res = np.zeros((W, bpp), dtype=np.int32)
            left, upleft = np.zeros(bpp, dtype=np.int32), np.zeros(bpp, dtype=np.int32)
            for x in range(W):
                if ftype == 3:
                    pred = (left + up[x]) >> 1
                else:
                    p = left + up[x] - upleft
                    pa, pb, pc = abs(p - left), abs(p - up[x]), abs(p - upleft)
                    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up[x], upleft))
                left = (fl[x] + pred) & 255
                upleft = up[x]
                res[x] = left
            cur = res.astype(np.uint8).reshape(-1)
        else:
            raise ValueError(f"row {y}: filter type {ftype}")
        out[y] = prev = cur
    if depth == 8:
        return out.reshape(H, W, C)
    return out.view(">u2").astype(np.uint16).reshape(H, W, C)


# ---------------------------------------------------------------------------------------------------------------- code lengths
def tree_lengths(counts):
    """Huffman lengths of the used symbols by the two-queue construction, NOT limited: leaves sorted by (count, symbol), internal
    nodes in creation order, the smaller weight first, a tie to the leaf queue."""
    used = sorted((int(c), s) for s, c in enumerate(counts) if c > 0)
    n = len(used)
    if n < 2:
        raise ValueError("a Huffman code needs at least two used symbols")
    w = [c for c, _ in used] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    leaf, node = 0, n                                                        # the heads of the two queues
    for k in range(n, 2 * n - 1):
        for _ in range(2):
            if leaf < n and (node >= k or w[leaf] <= w[node]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, node = node, node + 1
            w[k] += w[pick]
            parent[pick] = k
    depth = [0] * (2 * n - 1)
    for x in range(2 * n - 3, -1, -1):
        depth[x] = depth[parent[x]] + 1
    lengths = [0] * len(counts)
    for i, (_, s) in enumerate(used):
        lengths[s] = depth[i]
    return lengths


def code_lengths(counts):
    """tree_lengths, limited to 15 bits: while the deepest leaf is above 15, every non-zero count c becomes (c + 1) >> 1."""
    counts = [int(c) for c in counts]
    while True:
        lengths = tree_lengths(counts)
        if max(lengths) <= MAX_BITS:
            return lengths
        counts = [(c + 1) >> 1 if c > 0 else 0 for c in counts]


def canonical_codes(lengths):
    """RFC 1951, 3.2.2: -> codes (as written there: most significant bit first; 0 for an unused symbol)"""
    bl_count = [0] * (MAX_BITS + 2)
    for n in lengths:
        if n:
            bl_count[n] += 1
    code, next_code = 0, [0] * (MAX_BITS + 2)
    for bits in range(1, MAX_BITS + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            codes[s] = next_code[n]
            next_code[n] += 1
    return codes


def reverse_bits(v: int, n: int) -> int:
    r = 0
    for _ in range(n):
        r, v = (r << 1) | (v & 1), v >> 1
    return r


# ---------------------------------------------------------------------------------------------------------------- the stream
def _pack_bits(values: np.ndarray, nbits: np.ndarray) -> (np.ndarray, int):
    """tokens (value, bit count), each written least significant bit first -> (uint8 bytes, zero-padded; total bits)"""
    starts = np.cumsum(nbits) - nbits
    total = int(nbits.sum())
    bits = np.zeros((total + 7) // 8 * 8, dtype=np.uint8)
    for k in range(int(nbits.max())):
        m = nbits > k
        bits[starts[m] + k] = (values[m] >> k) & 1
    return np.packbits(bits, bitorder="little"), total


def length_symbol(c: int):
    """A match length 3..258 -> (its symbol 257..285, the number of extra bits, their value c - base); 258 is symbol 285."""
    if not 3 <= c <= MAX_MATCH:
        raise ValueError(f"a match is 3..{MAX_MATCH} bytes long, got {c}")
    k = 28 if c == MAX_MATCH else max(i for i, b in enumerate(LENGTH_BASE[:28]) if b <= c)
    return 257 + k, LENGTH_EXTRA[k], c - LENGTH_BASE[k]


def segment_tokens(data):
    """One segment's filtered bytes -> (kind, length), int64 [n] each: per position LITERAL, MATCH (a match head; ``length`` its
    length, 0 elsewhere) or COVERED (the position emits nothing), by the token rule of the docstring."""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    n = data.size
    i = np.arange(n, dtype=np.int64)
    first = np.ones(n, dtype=bool)
    first[1:] = data[1:] != data[:-1]
    s = np.maximum.accumulate(np.where(first, i, 0))                         # the start of the position's run
    starts = np.flatnonzero(first)
    run_len = np.diff(np.append(starts, n))
    L = run_len[np.cumsum(first) - 1]
    o = i - s
    k, j = (o - 1) // MAX_MATCH, (o - 1) % MAX_MATCH
    c = np.minimum(MAX_MATCH, L - 1 - MAX_MATCH * k)
    kind = np.where((o == 0) | (c < 3), LITERAL, np.where(j == 0, MATCH, COVERED)).astype(np.int64)
    return kind, np.where(kind == MATCH, c, 0).astype(np.int64)


def _bit_reversed_code(hist):
    lengths = code_lengths(hist)
    rev = np.array([reverse_bits(c, l) for c, l in zip(canonical_codes(lengths), lengths)], dtype=np.int64)
    return lengths, rev, np.array(lengths, dtype=np.int64)


def _finish_block(head_v, head_n, values, nbits, rev, lens):
    values = np.concatenate([np.array(head_v, dtype=np.int64), values, rev[256:257], np.zeros(1, dtype=np.int64)])
    nbits = np.concatenate([np.array(head_n, dtype=np.int64), nbits, lens[256:257], np.full(1, 3, dtype=np.int64)])
    packed, _ = _pack_bits(values, nbits)
    return packed.tobytes() + b"\x00\x00\xff\xff"


def segment_choice(data) -> bool:
    """Whether ``runs=True`` writes this segment as a run block: it has a match and bits_runs < bits_lit."""
    return _encode_segment(data, True)[1]


def _encode_segment(data, runs):
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    n = data.size
    hist = np.bincount(data, minlength=256).tolist() + [1]
    lengths, rev, lens = _bit_reversed_code(hist)
    bits_lit = HEADER_BITS + sum(h * l for h, l in zip(hist, lengths))
    head_v = [0, 2, 0, 0, 15] + [0 if s > 15 else 4 for s in CLC_ORDER] + [reverse_bits(l, 4) for l in lengths] + [0]
    head_n = [1, 2, 5, 5, 4] + [3] * 19 + [4] * 258
    assert sum(head_n) == HEADER_BITS
    literal = _finish_block(head_v, head_n, rev[data], lens[data], rev, lens)
    assert len(literal) == (bits_lit + 3 + 7) // 8 + 4 and len(literal) <= segment_bound(n), (len(literal), segment_bound(n))
    if not runs:
        return literal, False
    kind, length = segment_tokens(data)
    heads = np.flatnonzero(kind == MATCH)
    if heads.size == 0:
        return literal, False
    sym, extra_n, extra_v = (np.array(v, dtype=np.int64) for v in zip(*(length_symbol(int(c)) for c in length[heads])))
    lit = data[kind == LITERAL]
    hist_r = (np.bincount(lit, minlength=256).tolist() + [1] + np.bincount(sym - 257, minlength=29).tolist())
    lengths_r, rev_r, lens_r = _bit_reversed_code(hist_r)
    bits_runs = RUN_HEADER_BITS + sum(h * l for h, l in zip(hist_r, lengths_r)) + int(extra_n.sum()) + heads.size
    if not bits_runs < bits_lit:
        return literal, False
    head_v = [0, 2, 29, 0, 15] + [0 if s > 15 else 4 for s in CLC_ORDER] + [reverse_bits(l, 4) for l in lengths_r] + [reverse_bits(1, 4)]
    head_n = [1, 2, 5, 5, 4] + [3] * 19 + [4] * 287
    assert sum(head_n) == RUN_HEADER_BITS
    emit = kind != COVERED
    values, nbits = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    values[kind == LITERAL], nbits[kind == LITERAL] = rev_r[lit], lens_r[lit]
    values[heads] = rev_r[sym] | (extra_v << lens_r[sym])                   # (the distance bit behind them is 0)
    nbits[heads] = lens_r[sym] + extra_n + 1
    assert int(nbits.sum()) + int(lens_r[256]) <= MAX_BITS * (n + 1)
    out = _finish_block(head_v, head_n, values[emit], nbits[emit], rev_r, lens_r)
    assert len(out) == (bits_runs + 3 + 7) // 8 + 4 and len(out) <= len(literal), (len(out), len(literal))
    return out, True


def encode_segment(data, runs: bool = False) -> bytes:
    """One segment's filtered bytes -> its deflate block and the empty stored block behind it (whole bytes)."""
    return _encode_segment(data, runs)[0]


def encode_filtered(filtered: np.ndarray, runs: bool = False) -> bytes:
    """uint8 [H, stride] filtered rows -> the frame's zlib stream"""
    H, stride = filtered.shape
    R = max(1, SEGMENT_BYTES // stride)
    parts = [b"\x78\x01"] + [encode_segment(filtered[r:r + R].tobytes(), runs) for r in range(0, H, R)]
    parts += [b"\x03\x00", struct.pack(">I", zlib.adler32(filtered.tobytes()) & 0xFFFFFFFF)]
    return b"".join(parts)


def frame_samples(frames: torch.Tensor, depth: int) -> np.ndarray:
    """frameio.codes as integers: uint8 / uint16 [T, H, W, C] on the host"""
    if frames.dim() != 4 or frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames must be [T, H, W, C] in fp32 or bf16, got {tuple(frames.shape)} {frames.dtype}")
    geometry(frames.shape[1], frames.shape[2], frames.shape[3], depth)
    q = frameio.codes(frames, 255.0 if depth == 8 else 65535.0).to(torch.int32).cpu().numpy()
    return q.astype(np.uint8 if depth == 8 else np.uint16)


def encode_frames_spec(frames: torch.Tensor, depth: int = 8, runs: bool = False):
    """-> list of T ``bytes``: one zlib stream per frame"""
    q = frame_samples(frames, depth)
    T, H, W, C = q.shape
    bound = frame_bound(H, W, C, depth)
    streams = [encode_filtered(filter_rows(q[t], depth), runs) for t in range(T)]
    assert all(len(s) <= bound for s in streams), (max(map(len, streams)), bound)
    return streams


# ---------------------------------------------------------------------------------------------------------------- files
def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def png_parts(stream, W: int, H: int, C: int, depth: int):
    """-> (head, tail): the bytes of the file in front of and behind the stream, which a writer puts out as it is (any object with
    the buffer protocol: no copy of a 4K frame's tens of megabytes for the sake of a concatenation)."""
    geometry(H, W, C, depth)
    view = memoryview(stream).cast("B")
    ihdr = struct.pack(">IIBBBBB", W, H, depth, 2 if C == 3 else 6, 0, 0, 0)
    head = SIGNATURE + _chunk(b"IHDR", ihdr) + struct.pack(">I", len(view)) + b"IDAT"
    tail = struct.pack(">I", zlib.crc32(view, zlib.crc32(b"IDAT")) & 0xFFFFFFFF) + _chunk(b"IEND", b"")
    return head, tail


def png_file(stream, W: int, H: int, C: int, depth: int) -> bytes:
    """A frame's zlib stream framed as a PNG file: signature, IHDR, one IDAT, IEND."""
    head, tail = png_parts(stream, W, H, C, depth)
    return head + bytes(memoryview(stream).cast("B")) + tail


def write_png(path: str, samples: np.ndarray):
    """The host writer for frames that are not on a device: samples uint8 / uint16 [H, W, 3 | 4], filtered as above, then a general
    deflate (zlib level 6) -- the one place that is not the kernel's stream, and need not equal its bytes."""
    if samples.ndim != 3 or samples.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"samples must be uint8 or uint16 [H, W, C], got {samples.dtype} {samples.shape}")
    H, W, C = samples.shape
    depth = 8 * samples.dtype.itemsize
    stream = zlib.compress(filter_rows(samples, depth).tobytes(), 6)
    with open(path, "wb") as f:
        f.write(png_file(stream, W, H, C, depth))


def png_header(path: str):
    """-> (W, H, depth, colour type, interlace) of a PNG file, None for anything else"""
    try:
        with open(path, "rb") as f:
            head = f.read(33)
    except OSError:
        return None
    if len(head) < 33 or head[:8] != SIGNATURE or head[12:16] != b"IHDR":
        return None
    W, H, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", head[16:29])
    return W, H, depth, ctype, interlace


def read_png16(path: str):
    """A non-interlaced PNG of bit depth 16 and colour type 2 (RGB) or 6 (RGBA) -> uint16 [H, W, 3 | 4]; None for everything else
    (PIL cannot return 16-bit RGB: it reduces such a file to 8 bits)."""
    info = png_header(path)
    if info is None or info[2] != 16 or info[3] not in (2, 6) or info[4] != 0:
        return None
    W, H, _, ctype, _ = info
    with open(path, "rb") as f:
        blob = f.read()
    pos, idat = 8, []
    while pos + 8 <= len(blob):
        n, kind = struct.unpack(">I4s", blob[pos:pos + 8])
        if kind == b"IDAT":
            idat.append(blob[pos + 8:pos + 8 + n])
        elif kind == b"IEND":
            break
        pos += 12 + n
    return unfilter(zlib.decompress(b"".join(idat)), W, H, 3 if ctype == 2 else 4, 16)
