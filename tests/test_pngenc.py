"""-m "not gpu": pngenc.py, the specification of csrc/svr_png.hip -- the stream's validity (zlib and PIL decode it to the samples of
frameio.codes), the filter rule against a byte-by-byte evaluation of the PNG specification, the length-limited code, the capacity
bounds, a size guard against a silently flat code, the 16-bit reader / host writer --, and the command line's png route: 16-bit files
for sources deeper than 8 bits, today's bytes for everything else, FrameSink's encoded route with a stand-in backend."""
import io
import os
import random
import shutil
import struct
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import sub
from frame_unpack_cases import fake_video, random_packed, stand_ins
from test_stream import cli, rig  # noqa: F401 (fixtures)

# (T, H, W, C, depth); the last has three segments: stride 301, R = 217, the final segment 66 rows
SHAPES = [(1, 1, 1, 3, 8), (2, 3, 5, 3, 8), (1, 2, 2, 4, 8), (3, 17, 33, 3, 16), (1, 5, 40, 4, 16), (1, 500, 100, 3, 8)]
FIB = [1, 1]
while len(FIB) < 24:
    FIB.append(FIB[-1] + FIB[-2])


def clip(T, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, H, W, C, generator=g) * 1.2 - 0.1


def synthetic(H=300, W=400):
    """0.5 + 0.3 sin(x / 9) + 0.2 cos(y / 7) plus N(0, 0.01): smooth with noise, what a decoded frame looks like to a filter"""
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    base = (0.5 + 0.3 * torch.sin(xx / 9) + 0.2 * torch.cos(yy / 7))[..., None].expand(H, W, 3)
    return (base + torch.randn(H, W, 3, generator=g) * 0.01)[None].contiguous()


def reference_filters(raw, bpp):
    """The PNG specification byte by byte: raw uint8 [H, n] -> five filtered versions [5, H, n] (int)."""
    H, n = raw.shape
    out = np.zeros((5, H, n), dtype=np.int64)
    for y in range(H):
        for i in range(n):
            x = int(raw[y, i])
            a = int(raw[y, i - bpp]) if i >= bpp else 0
            b = int(raw[y - 1, i]) if y > 0 else 0
            c = int(raw[y - 1, i - bpp]) if (y > 0 and i >= bpp) else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            paeth = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            for ty, pred in enumerate((0, a, b, (a + b) // 2, paeth)):
                out[ty, y, i] = (x - pred) % 256
    return out


# ---------------------------------------------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_is_valid_and_decodes_to_the_codes(shape):
    pngenc, frameio = sub("pngenc"), sub("frameio")
    T, H, W, C, depth = shape
    x = clip(T, H, W, C, seed=sum(shape))
    streams = pngenc.encode_frames_spec(x, depth)
    assert len(streams) == T
    q = frameio.codes(x, 255.0 if depth == 8 else 65535.0).to(torch.int32).numpy()
    bpp, stride, R, nseg = pngenc.geometry(H, W, C, depth)
    if shape == SHAPES[-1]:
        assert (R, nseg, H - (nseg - 1) * R) == (217, 3, 66)
    for t, s in enumerate(streams):
        assert len(s) <= pngenc.frame_bound(H, W, C, depth)
        filtered = zlib.decompress(s)
        assert filtered == pngenc.filter_rows(q[t], depth).tobytes() and len(filtered) == H * stride
        back = pngenc.unfilter(filtered, W, H, C, depth)
        assert back.dtype == (np.uint8 if depth == 8 else np.uint16) and np.array_equal(back.astype(np.int32), q[t])
        img = Image.open(io.BytesIO(pngenc.png_file(s, W, H, C, depth)))
        img.load()
        assert img.size == (W, H)
        if depth == 8:
            want = frameio.pack_frames_torch(x[t:t + 1], "rgb8")[0].numpy()
            assert img.mode == ("RGB" if C == 3 else "RGBA") and np.array_equal(np.asarray(img), want)
    # bf16 frames: the same statement through frameio.codes
    xb = x.to(torch.bfloat16)
    qb = frameio.codes(xb, 255.0 if depth == 8 else 65535.0).to(torch.int32).numpy()
    assert zlib.decompress(pngenc.encode_frames_spec(xb, depth)[0]) == pngenc.filter_rows(qb[0], depth).tobytes()


def test_non_finite_samples_follow_frameio_codes():
    pngenc = sub("pngenc")
    x = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.5, 2.0]).reshape(1, 1, 2, 3)
    assert pngenc.frame_samples(x, 8).flatten().tolist() == [0, 255, 0, 0, 128, 255]
    assert pngenc.frame_samples(x, 16).flatten().tolist() == [0, 65535, 0, 0, 32768, 65535]
    for kw, word in ((dict(C=2), "C must be"), (dict(depth=12), "depth must be"), (dict(H=0), "H >= 1")):
        args = dict(H=4, W=4, C=3, depth=8)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            pngenc.geometry(**args)


# ---------------------------------------------------------------------------------------------------------------- filters
@pytest.mark.parametrize("C,depth", [(3, 8), (4, 8), (3, 16), (4, 16)])
def test_filters_and_their_choice_against_the_png_specification(C, depth):
    pngenc = sub("pngenc")
    rng = np.random.default_rng(C * depth)
    top = 256 if depth == 8 else 65536
    q = rng.integers(0, top, (9, 7, C))
    q[3] = q[2]                                                              # a row equal to the one above: Up gives zeros
    q[5, :, :] = q[5, :1, :]                                                 # a flat row: Sub gives zeros after the first pixel
    q[7] = (q[6] + 3) % top
    bpp = C * depth // 8
    raw = pngenc.sample_bytes(q, depth)
    assert raw.shape == (9, 7 * bpp)
    if depth == 16:
        assert raw[0, 0] == q[0, 0, 0] >> 8 and raw[0, 1] == q[0, 0, 0] & 255          # big-endian
    want = reference_filters(raw, bpp)
    assert np.array_equal(pngenc.filter_candidates(q, depth), want)
    # the edges, said directly: on row 0 Average predicts floor(a / 2) and Paeth predicts a; at the left edge of a later row Average
    # predicts floor(b / 2) and Paeth predicts b; the first pixel of row 0 is unpredicted by all five
    r = raw.astype(np.int64)
    assert np.array_equal(want[3, 0, bpp:], (r[0, bpp:] - r[0, :-bpp] // 2) % 256) and np.array_equal(want[4, 0], want[1, 0])
    assert np.array_equal(want[3, 4, :bpp], (r[4, :bpp] - r[3, :bpp] // 2) % 256) and np.array_equal(want[4, 4, :bpp], want[2, 4, :bpp])
    assert all(np.array_equal(want[ty, 0, :bpp], r[0, :bpp]) for ty in range(5))
    cost = np.where(want < 128, want, 256 - want).sum(axis=2)
    rows = pngenc.filter_rows(q, depth)
    for y in range(9):
        ty = int(rows[y, 0])
        assert cost[ty, y] == cost[:, y].min() and all(cost[k, y] > cost[ty, y] for k in range(ty)), y
        assert np.array_equal(rows[y, 1:], want[ty, y])
    assert rows[3, 0] == 2 and rows[5, 0] in (1, 4)


def test_a_tie_between_filters_goes_to_the_lowest_type():
    pngenc = sub("pngenc")
    flat = np.full((1, 4, 3), 10)                 # row 0, every byte 10: None 120 = Up 120, Sub 30 = Paeth 30, Average 30 + 9 * 5
    cand = pngenc.filter_candidates(flat, 8)
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)[:, 0].tolist()
    assert cost == [120, 30, 120, 75, 30]
    assert pngenc.filter_rows(flat, 8)[0, 0] == 1                            # Sub, not Paeth
    assert pngenc.filter_rows(np.zeros((2, 3, 4), dtype=np.int64), 16)[:, 0].tolist() == [0, 0]      # all five cost 0: None


# ---------------------------------------------------------------------------------------------------------------- code lengths
def kraft(lengths):
    return sum(Fraction(1, 2 ** n) for n in lengths if n)


def assert_prefix_free(lengths, codes):
    words = sorted(format(c, f"0{n}b") for c, n in zip(codes, lengths) if n)
    assert len(set(words)) == len(words)
    for a, b in zip(words, words[1:]):
        assert not b.startswith(a), (a, b)


def test_a_tree_deeper_than_15_is_rebuilt_from_halved_counts():
    pngenc = sub("pngenc")
    assert max(pngenc.tree_lengths(FIB)) == 23                               # Fibonacci counts: the most lopsided tree
    lengths = pngenc.code_lengths(FIB)
    assert max(lengths) <= 15 and kraft(lengths) == 1 and all(n > 0 for n in lengths)
    assert_prefix_free(lengths, pngenc.canonical_codes(lengths))
    # the rule itself: halve (rounding up) until the plain tree fits
    counts = list(FIB)
    while max(pngenc.tree_lengths(counts)) > 15:
        counts = [(c + 1) >> 1 for c in counts]
    assert lengths == pngenc.tree_lengths(counts) and counts != FIB
    # one more symbol of count 1 (a segment's end of block) splits the chain into two interleaved ones: such a histogram needs no limit
    assert max(pngenc.tree_lengths(FIB + [1])) == 13
    pow2 = [2 ** (17 - v) for v in range(18)] + [1]                          # ... counts that each exceed the sum of the smaller ones do
    assert max(pngenc.tree_lengths(pow2)) == 18 and max(pngenc.code_lengths(pow2)) == 15 and kraft(pngenc.code_lengths(pow2)) == 1
    # ties: equal counts are ordered by symbol, a leaf goes before an internal node of the same weight
    assert pngenc.tree_lengths([1, 1, 1, 1]) == [2, 2, 2, 2] and pngenc.tree_lengths([1, 1, 2]) == [2, 2, 1]
    assert pngenc.tree_lengths([0, 5, 0, 1]) == [0, 1, 0, 1]
    with pytest.raises(ValueError, match="two used symbols"):
        pngenc.tree_lengths([0, 3, 0])


def test_random_histograms_give_complete_codes_of_at_most_15_bits():
    pngenc = sub("pngenc")
    rng = random.Random(7)
    limited = 0
    for k in range(200):
        kind = k % 4
        if kind == 0:
            hist = [rng.randint(0, 300) for _ in range(256)]
        elif kind == 1:
            hist = [int(65536 * 0.5 ** rng.uniform(0, 30)) for _ in range(256)]          # many magnitudes: deep trees
        elif kind == 2:
            hist = [0] * 256
            for s in rng.sample(range(256), rng.randint(1, 40)):
                hist[s] = rng.randint(1, 70000)
        else:
            hist = [int(1.6 ** (i % 40)) if rng.random() < 0.8 else 0 for i in range(256)]
        hist.append(1)
        if sum(c > 0 for c in hist) < 2:
            hist[0] = 1
        limited += max(pngenc.tree_lengths(hist)) > 15
        lengths = pngenc.code_lengths(hist)
        assert len(lengths) == 257 and max(lengths) <= 15 and kraft(lengths) == 1
        assert all((n > 0) == (c > 0) for n, c in zip(lengths, hist))
        assert_prefix_free(lengths, pngenc.canonical_codes(lengths))
    assert limited >= 20                                                     # the limit was exercised, not only stated


def test_capacity_bounds_hold_for_the_worst_code():
    """A segment whose every byte carries a 15-bit code cannot exist, but nothing longer than 15 bits can: the bound is from the limit."""
    pngenc = sub("pngenc")
    assert pngenc.HEADER_BITS == 1106 and pngenc.segment_bound(0) == 139 + 2 + 5
    for n in (1, 7, 8, 9, 301, 65536, 65601):
        assert pngenc.segment_bound(n) >= (1106 + 15 * (n + 1) + 3 + 7) // 8 + 4
    vals = np.concatenate([np.full(c, v) for v, c in enumerate(FIB)])
    np.random.default_rng(1).shuffle(vals)
    seg = pngenc.encode_segment(vals.astype(np.uint8).tobytes())
    assert len(seg) <= pngenc.segment_bound(vals.size)
    assert seg[-4:] == b"\x00\x00\xff\xff"
    assert zlib.decompressobj(-15).decompress(seg + b"\x03\x00") == vals.astype(np.uint8).tobytes()      # (a raw deflate stream)
    assert pngenc.frame_bound(500, 100, 3, 8) == 2 + 2 * pngenc.segment_bound(217 * 301) + pngenc.segment_bound(66 * 301) + 6
    assert pngenc.frame_bound(3, 8200, 4, 16) == 2 + 3 * pngenc.segment_bound(65601) + 6


def test_size_stays_near_a_general_deflate_on_a_decoded_looking_frame():
    pngenc = sub("pngenc")
    x = synthetic()
    file = pngenc.png_file(pngenc.encode_frames_spec(x, 8)[0], 400, 300, 3, 8)
    ref = io.BytesIO()
    Image.fromarray(pngenc.frame_samples(x, 8)[0]).save(ref, format="PNG")
    raw, pil = 300 * 400 * 3, len(ref.getvalue())
    print(f"file {len(file)} B = {len(file) / raw:.4f} of raw, {len(file) / pil:.4f} x PIL's {pil} B")
    assert len(file) <= 0.75 * raw and len(file) <= 1.05 * pil
    # out of scope, stated: no run lengths, so a flat frame floors at one bit per byte
    flat = pngenc.encode_frames_spec(torch.full((1, 64, 64, 4), 0.25), 8)[0]
    assert 64 * 65 * 4 // 8 < len(flat) < 64 * 65 * 4 // 8 + 200


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_entry_points_agree_with_the_specification_and_refuse_before_any_launch():
    """svr_png_encode_bytes states pngenc.frame_bound; svr_png_encode refuses bad arguments on the host with a message naming the
    argument.  No device is needed: nothing is launched."""
    import ctypes
    import re
    from conftest import ROOT
    pngenc, hip_lib = sub("pngenc"), sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    for T, H, W, C, depth in SHAPES + [(1, 2, 4112, 3, 8), (1, 3, 8200, 4, 16), (17, 2160, 3840, 3, 8), (2, 2160, 3840, 4, 16), (1, 1, 87381, 3, 8)]:
        scratch, cap = ctypes.c_int64(0), ctypes.c_int64(0)
        assert L.svr_png_encode_bytes(T, H, W, C, depth, ctypes.byref(scratch), ctypes.byref(cap)) == 0
        _, stride, _, nseg = pngenc.geometry(H, W, C, depth)
        assert cap.value == pngenc.frame_bound(H, W, C, depth)
        assert scratch.value >= T * H * stride + T * nseg * (257 * 4 + 16 + 8)           # filtered bytes, tables, sizes and sums, offsets
    for args, word in (((1, 4, 4, 2, 8), b"C must be 3 or 4"), ((1, 4, 4, 3, 12), b"depth must be 8 or 16"), ((0, 4, 4, 3, 8), b"T >= 1"),
                       ((1, 0, 4, 3, 8), b"H >= 1"), ((1, 4, 2 ** 23, 3, 8), b"W must stay below"), ((1, 2 ** 25, 4, 3, 8), b"H must not exceed")):
        assert L.svr_png_encode_bytes(*args, None, None) != 0
        assert b"svr_png_encode_bytes" in L.svr_last_error() and word in L.svr_last_error(), L.svr_last_error()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    need, cap = ctypes.c_int64(0), ctypes.c_int64(0)
    assert L.svr_png_encode_bytes(1, 4, 6, 3, 8, ctypes.byref(need), ctypes.byref(cap)) == 0
    order = ("frames", "kind", "T", "H", "W", "C", "depth", "scratch", "nscratch", "out", "cap", "sizes", "stream")

    def call(**kw):
        a = dict(frames=p, kind=1, T=1, H=4, W=6, C=3, depth=8, scratch=p, nscratch=need.value, out=p, cap=cap.value, sizes=p, stream=None)
        a.update(kw)
        return L.svr_png_encode(*[a[k] for k in order])

    odd = lambda n: ctypes.c_void_p(base + n)
    for kw, word in ((dict(frames=None), b"frames"), (dict(scratch=None), b"scratch"), (dict(out=None), b"out"), (dict(sizes=None), b"sizes"),
                     (dict(kind=2), b"x_kind"), (dict(C=2), b"C must be 3 or 4"), (dict(C=5), b"C must be 3 or 4"), (dict(depth=12), b"depth must be 8 or 16"),
                     (dict(depth=0), b"depth must be 8 or 16"), (dict(T=0), b"T >= 1"), (dict(W=-1), b"W >= 1"),
                     (dict(nscratch=need.value - 1), b"scratch_bytes"), (dict(nscratch=0), b"scratch_bytes"), (dict(cap=cap.value - 1), b"out_capacity"),
                     (dict(frames=odd(2)), b"frames"), (dict(scratch=odd(8)), b"scratch"), (dict(sizes=odd(4)), b"sizes")):
        assert call(**kw) != 0
        msg = L.svr_last_error()
        assert b"svr_png_encode:" in msg and word in msg, (kw, msg)
    # header, ctypes table and build list know the entry points; the ABI stays 9
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    for name, n_args in (("svr_png_encode", 13), ("svr_png_encode_bytes", 7)):
        decl = re.search(rf"int {name}\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == n_args == len(hip_lib.SYMBOLS[name][1])
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert '#include "svr_png.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert os.path.join(hip_lib.CSRC, "svr_png.hip") in hip_lib.sources()


# ---------------------------------------------------------------------------------------------------------------- files
def hand_made_png(W, H, depth, ctype, interlace, body):
    chunk = lambda kind, data: struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace))
            + chunk(b"IDAT", zlib.compress(body)) + chunk(b"IEND", b""))


def test_sixteen_bit_files_round_trip_and_everything_else_is_left_to_pil(tmp_path):
    pngenc = sub("pngenc")
    rng = np.random.default_rng(3)
    for C in (3, 4):
        q = rng.integers(0, 65536, (11, 13, C)).astype(np.uint16)
        q[4] = q[3]
        path = str(tmp_path / f"deep{C}.png")
        pngenc.write_png(path, q)
        back = pngenc.read_png16(path)
        assert back.dtype == np.uint16 and np.array_equal(back, q)
        assert pngenc.png_header(path) == (13, 11, 16, 2 if C == 3 else 6, 0)
        img = Image.open(path)
        assert img.size == (13, 11)
        q8 = (q >> 8).astype(np.uint8)                                       # the host writer at depth 8: PIL reads the same pixels
        pngenc.write_png(path, q8)
        assert np.array_equal(np.asarray(Image.open(path)), q8) and pngenc.read_png16(path) is None
    # several IDAT chunks, as other writers produce them
    q = rng.integers(0, 65536, (5, 6, 3)).astype(np.uint16)
    whole = pngenc.png_file(zlib.compress(pngenc.filter_rows(q, 16).tobytes()), 6, 5, 3, 16)
    at = whole.index(b"IDAT") - 4
    n, = struct.unpack(">I", whole[at:at + 4])
    body = whole[at + 8:at + 8 + n]
    chunk = lambda data: struct.pack(">I", len(data)) + b"IDAT" + data + struct.pack(">I", zlib.crc32(b"IDAT" + data) & 0xFFFFFFFF)
    (tmp_path / "split.png").write_bytes(whole[:at] + chunk(body[:7]) + chunk(body[7:]) + whole[at + 12 + n:])
    assert np.array_equal(pngenc.read_png16(str(tmp_path / "split.png")), q)
    # not for this reader: interlaced, 8-bit, greyscale, something that is no png, a missing file
    (tmp_path / "interlaced.png").write_bytes(hand_made_png(2, 2, 16, 2, 1, b"\0" * 64))
    (tmp_path / "grey16.png").write_bytes(hand_made_png(2, 2, 16, 0, 0, b"\0" * 10))
    Image.fromarray(rng.integers(0, 256, (4, 4, 3)).astype(np.uint8)).save(tmp_path / "rgb8.png")
    Image.fromarray(rng.integers(0, 256, (4, 4)).astype(np.uint8)).save(tmp_path / "grey8.png")
    (tmp_path / "text.png").write_bytes(b"not a png at all, but longer than a header would be........")
    for name in ("interlaced.png", "grey16.png", "rgb8.png", "grey8.png", "text.png", "missing.png"):
        assert pngenc.read_png16(str(tmp_path / name)) is None, name
    with pytest.raises(ValueError, match="samples must be"):
        pngenc.write_png(str(tmp_path / "x.png"), np.zeros((2, 2, 3), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- command line
@pytest.fixture()
def identity(cli, monkeypatch):  # noqa: F811
    """the engines' work replaced by the identity: what reaches the writer is what the reader produced"""
    monkeypatch.setattr(cli, "run", lambda args, frames, eng=None, **kw: (frames, 0))
    monkeypatch.setattr(cli, "run_stream", lambda args, chunks, eng=None: chunks)
    return cli


def pil_bytes(arr):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


@pytest.mark.parametrize("C", [3, 4])
def test_a_sixteen_bit_still_leaves_as_a_sixteen_bit_file_with_its_samples(identity, tmp_path, C):
    pngenc = sub("pngenc")
    q = np.random.default_rng(C).integers(0, 65536, (6, 9, C)).astype(np.uint16)
    q[0, 0] = 65535
    q[0, 1] = 0
    pngenc.write_png(str(tmp_path / "in.png"), q)
    frames, _ = identity.load_frames(str(tmp_path / "in.png"))
    assert frames.dtype == torch.float32 and tuple(frames.shape) == (1, 6, 9, C)
    assert torch.equal(frames, sub("frameio_in").unit(torch.from_numpy(q.astype(np.int64)), 65535)[None])
    assert identity.main([str(tmp_path / "in.png"), "--output", str(tmp_path / "out.png")]) == 0
    assert pngenc.png_header(str(tmp_path / "out.png")) == (9, 6, 16, 2 if C == 3 else 6, 0)
    assert np.array_equal(pngenc.read_png16(str(tmp_path / "out.png")), q)


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_a_ten_bit_video_leaves_as_sixteen_bit_files(identity, tmp_path, monkeypatch, chunked):
    pngenc, fin, frameio = sub("pngenc"), sub("frameio_in"), sub("frameio")
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    packed = random_packed("yuv420p10", 7, 8, 10, 3, seed=8)
    fake_video(tmp_path / "clip.mkv", packed, "yuv420p10le", 10, 8, color_space="bt709", color_range="tv")
    tail = ["--chunk_size", "3"] if chunked else []
    assert identity.main([str(tmp_path / "clip.mkv"), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "out")] + tail) == 0
    want = frameio.codes(fin.unpack_frames_torch(packed, "yuv420p10", 7, 8, 10, 3, "bt709", "tv"), 65535.0).to(torch.int32).numpy()
    assert sorted(os.listdir(tmp_path / "out")) == [f"frame_{i:06d}.png" for i in range(7)]
    for i in range(7):
        path = str(tmp_path / "out" / f"frame_{i:06d}.png")
        assert pngenc.png_header(path) == (10, 8, 16, 2, 0)
        assert np.array_equal(pngenc.read_png16(path).astype(np.int32), want[i]), i


def test_eight_bit_sources_leave_as_the_bytes_pil_writes_today(identity, tmp_path, monkeypatch):
    fin, frameio = sub("frameio_in"), sub("frameio")
    rng = np.random.default_rng(5)
    # an 8-bit still
    q = rng.integers(0, 256, (6, 9, 3)).astype(np.uint8)
    Image.fromarray(q).save(tmp_path / "in.png")
    assert identity.output_depth(str(tmp_path / "in.png")) == 8
    assert identity.main([str(tmp_path / "in.png"), "--output", str(tmp_path / "out.png")]) == 0
    assert (tmp_path / "out.png").read_bytes() == pil_bytes(q)
    # a .npy
    x = torch.rand(3, 8, 10, 3)
    np.save(tmp_path / "clip.npy", x.numpy())
    want = frameio.pack_frames_torch(x, "rgb8").numpy()
    for n, tail in enumerate(([], ["--chunk_size", "2"])):
        assert identity.main([str(tmp_path / "clip.npy"), "--output_format", "png", "--output", str(tmp_path / f"npy{n}")] + tail) == 0
        for i in range(3):
            assert (tmp_path / f"npy{n}" / f"frame_{i:06d}.png").read_bytes() == pil_bytes(want[i]), (n, i)
    # a yuv420p video through ffmpeg
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    packed = random_packed("yuv420p8", 4, 8, 10, 3, seed=9)
    fake_video(tmp_path / "clip.mp4", packed, "yuv420p", 10, 8, color_space="bt709", color_range="tv")
    assert identity.main([str(tmp_path / "clip.mp4"), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "vid")]) == 0
    want = frameio.pack_frames_torch(fin.unpack_frames_torch(packed, "yuv420p8", 4, 8, 10, 3, "bt709", "tv"), "rgb8").numpy()
    for i in range(4):
        assert (tmp_path / "vid" / f"frame_{i:06d}.png").read_bytes() == pil_bytes(want[i]), i
    # the depth rule
    info = lambda pix: dict(pix_fmt=pix, height=1080, width=16, color_space=None, color_range=None)
    assert [identity.output_depth("c.mkv", info(p)) for p in ("yuv420p", "yuv420p10le", "yuv444p12le", "rgb24", "yuva420p")] == [8, 16, 16, 8, 8]
    assert identity.output_depth("clip.npy") == 8 and identity.output_depth("clip.mp4") == 8 and identity.output_depth("photo.jpg") == 8


class SpecOps:
    """A stand-in backend whose encode_png IS the specification, on the host: (out uint8 [T, cap], sizes int64 [T])."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def encode_png(self, frames, depth=8, out=None, sizes=None):
        pngenc = sub("pngenc")
        T, H, W, C = frames.shape
        streams = pngenc.encode_frames_spec(frames, depth)
        out = torch.full((T, pngenc.frame_bound(H, W, C, depth)), 0xA5, dtype=torch.uint8)
        for t, s in enumerate(streams):
            out[t, :len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
        self.calls.append((tuple(frames.shape), depth))
        return out, torch.tensor([len(s) for s in streams], dtype=torch.int64)


@pytest.mark.parametrize("depth", [8, 16])
def test_sink_hands_encoded_streams_to_the_writer(cli, tmp_path, depth):  # noqa: F811
    pngenc = sub("pngenc")
    chunks = [clip(t, 6, 16, 4, seed=30 + t) for t in (3, 1, 2)]
    seen = []

    class Watching(cli.PngWriter):
        def write_streams(self, streams, height, width, channels):
            seen.append([len(s) for s in streams])
            super().write_streams(streams, height, width, channels)

        def write(self, arr, height, width):
            raise AssertionError("the encoded route hands over streams, not frames")

    ops = SpecOps()
    sink = cli.FrameSink(Watching(str(tmp_path / "out"), depth=depth), ops)
    for c in chunks:
        sink.put(c)
    sink.close()
    assert ops.calls == [((t, 6, 16, 4), depth) for t in (3, 1, 2)] and sink.frames == 6
    want = [s for c in chunks for s in pngenc.encode_frames_spec(c, depth)]
    assert [n for part in seen for n in part] == [len(s) for s in want]      # only sizes[t] bytes of each slot reached the writer
    for i, s in enumerate(want):
        assert (tmp_path / "out" / f"frame_{i:06d}.png").read_bytes() == pngenc.png_file(s, 16, 6, 4, depth), i
    # a single image job goes to the path itself
    sink = cli.FrameSink(cli.PngWriter(str(tmp_path / "one" / "still.png"), single=True, depth=depth), SpecOps())
    sink.put(chunks[1])
    sink.close()
    assert (tmp_path / "one" / "still.png").read_bytes() == pngenc.png_file(want[3], 16, 6, 4, depth)
    # a backend without the encoder, a writer that takes no streams: the routes of before
    plain = cli.FrameSink(cli.PngWriter(str(tmp_path / "plain")))
    plain.put(chunks[0])
    plain.close()
    packed = sub("frameio").pack_frames_torch(chunks[0], "rgb8").numpy()
    assert (tmp_path / "plain" / "frame_000000.png").read_bytes() == pil_bytes(packed[0])
    with pytest.raises(ValueError, match="depth"):
        cli.PngWriter(str(tmp_path / "bad"), depth=12)


def test_a_writer_exception_on_the_encoded_route_surfaces_at_the_next_put(cli, tmp_path):  # noqa: F811
    class Full(cli.PngWriter):
        def write_streams(self, streams, height, width, channels):
            raise OSError("No space left on device")

    sink = cli.FrameSink(Full(str(tmp_path / "out")), SpecOps())
    sink.put(clip(2, 4, 5, 3, seed=1))
    # the next put that meets the failure raises it: at the latest the third, which has to wait for the buffer of the first
    with pytest.raises(RuntimeError, match="writing frames failed: OSError: No space left"):
        for _ in range(3):
            sink.put(clip(1, 4, 5, 3, seed=2))
    sink.close(quiet=True)
