"""-m "not gpu": the run-length stream of pngenc.py (``runs=True``) -- the token rule on raw segments, the length symbols against
the RFC 1951 table, validity (zlib, PIL and read_png16 decode it to the samples of frameio.codes), never longer than the literal
stream, equal to it where no run pays, the per-segment choice, two size conditions --, and the command line's hand-over: a writer
with ``runs`` asks the backend for such streams, one without makes the call of before."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import sub
from test_pngenc import SHAPES, clip, synthetic
from test_stream import cli, rig  # noqa: F401 (fixtures)

# RFC 1951, 3.2.5, written out: symbol -> (extra bits, the lengths it covers)
RFC_LENGTHS = {257: (0, 3, 3), 258: (0, 4, 4), 259: (0, 5, 5), 260: (0, 6, 6), 261: (0, 7, 7), 262: (0, 8, 8), 263: (0, 9, 9),
               264: (0, 10, 10), 265: (1, 11, 12), 266: (1, 13, 14), 267: (1, 15, 16), 268: (1, 17, 18), 269: (2, 19, 22),
               270: (2, 23, 26), 271: (2, 27, 30), 272: (2, 31, 34), 273: (3, 35, 42), 274: (3, 43, 50), 275: (3, 51, 58),
               276: (3, 59, 66), 277: (4, 67, 82), 278: (4, 83, 98), 279: (4, 99, 114), 280: (4, 115, 130), 281: (5, 131, 162),
               282: (5, 163, 194), 283: (5, 195, 226), 284: (5, 227, 257), 285: (0, 258, 258)}


def run_tokens(L):
    """The rule, run by run: (kind, length) of the L positions of one maximal run."""
    pngenc = sub("pngenc")
    out = [(pngenc.LITERAL, 0)]
    left = L - 1
    while left >= 3:
        c = min(258, left)
        out += [(pngenc.MATCH, c)] + [(pngenc.COVERED, 0)] * (c - 1)
        left -= c
    return out + [(pngenc.LITERAL, 0)] * left


def sprite(depth_seed=0):
    g = torch.Generator().manual_seed(5 + depth_seed)
    x = torch.zeros(1, 128, 128, 4)
    x[0, 30:80, 30:80] = torch.rand(50, 50, 4, generator=g)
    return x


def letterboxed():
    x = clip(1, 270, 480, 3, seed=11)
    x[0, :34] = 0.0
    x[0, -34:] = 0.0
    return x


def mixed():
    """120 x 600 x 3 at depth 8: stride 1801, R = 36, four segments; rows 0..35 zero (segment 0 is one run), the rest noise."""
    x = clip(1, 120, 600, 3, seed=12)
    x[0, :36] = 0.0
    return x


# (name, frames, depth): the issue's table, both depths where it lists them
FRAMES = [("constant", torch.full((1, 64, 64, 4), 0.5), 8), ("zeros", torch.zeros(1, 9, 21, 3), 8), ("sprite8", sprite(), 8),
          ("sprite16", sprite(), 16), ("letterbox", letterboxed(), 8), ("flat_row", torch.full((1, 1, 70000, 3), 0.25), 8),
          ("noise", clip(1, 40, 50, 3, seed=13), 8), ("smooth_noise", synthetic(), 8), ("mixed", mixed(), 8)]


# ---------------------------------------------------------------------------------------------------------------- tokens
@pytest.mark.parametrize("L", list(range(1, 12)) + list(range(258, 263)) + list(range(516, 521)) + [775])
def test_tokens_of_two_runs_around_a_separator(L):
    pngenc = sub("pngenc")
    data = bytes([7]) * L + bytes([9]) + bytes([7]) * L
    kind, length = pngenc.segment_tokens(data)
    want = run_tokens(L) + run_tokens(1) + run_tokens(L)
    assert list(zip(kind.tolist(), length.tolist())) == want
    # what the tokens say is the segment: literals copy a byte, a match repeats the byte before it
    back = []
    for i, (k, c) in enumerate(want):
        if k == pngenc.LITERAL:
            back.append(data[i])
        elif k == pngenc.MATCH:
            back += [back[-1]] * c
    assert bytes(back) == data
    for runs in (False, True):
        assert zlib.decompress(b"\x78\x01" + pngenc.encode_segment(data, runs) + b"\x03\x00" +
                               zlib.adler32(data).to_bytes(4, "big")) == data


def test_length_symbols_against_the_rfc_table():
    pngenc = sub("pngenc")
    seen = set()
    for c in range(3, 259):
        sym, extra_n, extra_v = pngenc.length_symbol(c)
        n, lo, hi = RFC_LENGTHS[sym]
        assert extra_n == n and lo <= c <= hi and extra_v == c - lo and 0 <= extra_v < (1 << n), c
        seen.add(sym)
    assert seen == set(RFC_LENGTHS) and pngenc.length_symbol(258) == (285, 0, 0) and pngenc.length_symbol(257) == (284, 5, 30)
    for bad in (2, 259):
        with pytest.raises(ValueError):
            pngenc.length_symbol(bad)


@pytest.mark.parametrize("seed", range(6))
def test_random_segments_decode_and_never_grow(seed):
    pngenc = sub("pngenc")
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 4000))
    mean = (1.5, 4.0, 30.0, 400.0, 2.0, 90.0)[seed]
    parts, total = [], 0
    while total < n:
        L = min(int(rng.geometric(1.0 / mean)), n - total)
        parts.append(np.full(L, rng.integers(0, 4), dtype=np.uint8))
        total += L
    data = np.concatenate(parts).tobytes()
    lit, run = pngenc.encode_segment(data), pngenc.encode_segment(data, runs=True)
    for block in (lit, run):
        assert zlib.decompress(b"\x78\x01" + block + b"\x03\x00" + zlib.adler32(data).to_bytes(4, "big")) == data
    assert len(run) <= len(lit) <= pngenc.segment_bound(len(data))
    assert pngenc.encode_segment(data, runs=False) == lit


# ---------------------------------------------------------------------------------------------------------------- frames
def assert_valid(x, depth, tmp_path):
    pngenc, frameio = sub("pngenc"), sub("frameio")
    T, H, W, C = x.shape
    q = frameio.codes(x, 255.0 if depth == 8 else 65535.0).to(torch.int32).numpy()
    lit, run = pngenc.encode_frames_spec(x, depth), pngenc.encode_frames_spec(x, depth, runs=True)
    assert pngenc.encode_frames_spec(x, depth, runs=False) == lit
    for t in range(T):
        assert zlib.decompress(run[t]) == pngenc.filter_rows(q[t], depth).tobytes()
        assert len(run[t]) <= len(lit[t]) <= pngenc.frame_bound(H, W, C, depth)
        blob = pngenc.png_file(run[t], W, H, C, depth)
        if depth == 8:
            img = Image.open(io.BytesIO(blob))
            assert img.mode == ("RGB" if C == 3 else "RGBA") and np.array_equal(np.asarray(img), q[t].astype(np.uint8))
        else:
            (tmp_path / "deep.png").write_bytes(blob)
            assert np.array_equal(pngenc.read_png16(str(tmp_path / "deep.png")).astype(np.int32), q[t])
    return lit, run


@pytest.mark.parametrize("name,x,depth", FRAMES, ids=[f[0] for f in FRAMES])
def test_frames_decode_and_never_grow(name, x, depth, tmp_path):
    assert_valid(x, depth, tmp_path)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_literal_suite_s_shapes(shape, tmp_path):
    T, H, W, C, depth = shape
    assert_valid(clip(T, H, W, C, seed=sum(shape)), depth, tmp_path)
    assert_valid(torch.zeros(T, H, W, C), depth, tmp_path)


def test_pure_noise_gives_the_literal_bytes():
    pngenc = sub("pngenc")
    for shape in ((1, 40, 50, 3, 8), (2, 31, 8, 3, 8), (1, 1, 1, 3, 8), (1, 30, 40, 4, 16)):
        x = torch.rand(*shape[:4], generator=torch.Generator().manual_seed(sum(shape)))      # (inside [0, 1): no clamped neighbours)
        assert pngenc.encode_frames_spec(x, shape[4], runs=True) == pngenc.encode_frames_spec(x, shape[4])


def test_size_conditions():
    pngenc = sub("pngenc")
    size = lambda x, runs: len(pngenc.encode_frames_spec(x, 8, runs=runs)[0])
    flat = torch.full((1, 64, 64, 4), 0.5)
    assert 4 * size(flat, True) <= size(flat, False)
    assert size(sprite(), True) <= 0.7 * size(sprite(), False)


def test_the_choice_differs_between_the_segments_of_one_frame():
    pngenc = sub("pngenc")
    x = mixed()
    assert pngenc.geometry(120, 600, 3, 8)[1:] == (1801, 36, 4)
    rows = pngenc.filter_rows(pngenc.frame_samples(x, 8)[0], 8)
    segs = [rows[r:r + 36].tobytes() for r in range(0, 120, 36)]
    assert [pngenc.segment_choice(s) for s in segs] == [True, False, False, False]
    assert segs[0] == bytes(36 * 1801)
    kind, length = pngenc.segment_tokens(segs[0])
    assert int((kind == pngenc.MATCH).sum()) == -(-(36 * 1801 - 1) // 258) and int(length.sum()) == 36 * 1801 - 1
    lit, run = (pngenc.encode_filtered(rows, r) for r in (False, True))
    parts = [pngenc.encode_segment(s, True) for s in segs]
    assert run == b"\x78\x01" + b"".join(parts) + lit[-6:]
    assert [parts[i] == pngenc.encode_segment(segs[i]) for i in range(4)] == [False, True, True, True]
    # a segment with matches that do not pay: incidental short runs in noise over eight values
    rng = np.random.default_rng(3)
    data = rng.integers(0, 8, 3000).astype(np.uint8).tobytes()
    assert (pngenc.segment_tokens(data)[0] == pngenc.MATCH).any() and not pngenc.segment_choice(data)
    assert pngenc.encode_segment(data, True) == pngenc.encode_segment(data)


# ---------------------------------------------------------------------------------------------------------------- command line
class RunsOps:
    """A stand-in backend whose encode_png IS the specification, on the host, and takes ``runs``."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def encode_png(self, frames, depth=8, out=None, sizes=None, **kw):
        pngenc = sub("pngenc")
        T, H, W, C = frames.shape
        streams = pngenc.encode_frames_spec(frames, depth, **kw)
        out = torch.full((T, pngenc.frame_bound(H, W, C, depth)), 0xA5, dtype=torch.uint8)
        for t, s in enumerate(streams):
            out[t, :len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
        self.calls.append((tuple(frames.shape), depth, kw))
        return out, torch.tensor([len(s) for s in streams], dtype=torch.int64)


def bordered(T, seed):
    x = clip(T, 12, 20, 4, seed=seed)
    x[:, :3] = 0.0
    x[:, -3:] = 0.0
    x[:, :, :4] = 0.0
    x[:, :, -4:] = 0.0
    return x


@pytest.mark.parametrize("depth", [8, 16])
def test_a_writer_with_runs_asks_for_run_streams(cli, tmp_path, depth):  # noqa: F811
    pngenc = sub("pngenc")
    chunks = [bordered(t, seed=50 + t) for t in (2, 1)]
    ops = RunsOps()
    sink = cli.FrameSink(cli.PngWriter(str(tmp_path / "runs"), depth=depth, runs=True), ops)
    for c in chunks:
        sink.put(c)
    sink.close()
    assert ops.calls == [((t, 12, 20, 4), depth, dict(runs=True)) for t in (2, 1)]
    want = [s for c in chunks for s in pngenc.encode_frames_spec(c, depth, runs=True)]
    lit = [s for c in chunks for s in pngenc.encode_frames_spec(c, depth)]
    assert all(len(w) < len(l) for w, l in zip(want, lit))
    for i, s in enumerate(want):
        assert (tmp_path / "runs" / f"frame_{i:06d}.png").read_bytes() == pngenc.png_file(s, 20, 12, 4, depth), i
    # the default writer makes the call of before: no ``runs`` argument reaches the backend
    ops = RunsOps()
    sink = cli.FrameSink(cli.PngWriter(str(tmp_path / "plain"), depth=depth), ops)
    sink.put(chunks[0])
    sink.close()
    assert ops.calls == [((2, 12, 20, 4), depth, {})]
    for i in range(2):
        assert (tmp_path / "plain" / f"frame_{i:06d}.png").read_bytes() == pngenc.png_file(lit[i], 20, 12, 4, depth), i


def test_the_writer_factory_reads_the_switch(cli, tmp_path, monkeypatch):  # noqa: F811
    pngenc = sub("pngenc")
    assert isinstance(pngenc.RUNS, bool)
    for value in (True, False):
        monkeypatch.setattr(pngenc, "RUNS", value)
        w = cli.open_writer("png", str(tmp_path / "w"), 30.0, depth=16)
        assert isinstance(w, cli.PngWriter) and w.runs is value and w.depth == 16
    assert cli.PngWriter(str(tmp_path / "d")).runs is False
