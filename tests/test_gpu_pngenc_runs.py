"""-m gpu: svr_png_encode_runs (csrc/svr_png.hip) through HipOps.encode_png(..., runs=True) against its specification
pngenc.encode_frames_spec(..., runs=True) -- EQUAL byte for byte, ``sizes`` included, fp32 and bf16 input --, what lies past a
stream, the refusals of the new entry point, and the command line's hand-over with a writer that asks for runs.

``out`` and ``sizes`` live in tests/guarded_out.py buffers and the guards must stay intact.  Bytes of a frame's slot past sizes[t]
are NOT written by the kernels: they must still hold the poison byte 0xA5 after the call.

The shapes are the smallest at which the run stream can go wrong: one run across every row of a segment (and longer than 64 KiB,
many packer tiles long), a run that must stop at a segment's end although the byte value goes on, run lengths on every side of
the 258-byte match limit, a match head on the last position of a packer tile (4096 positions: 256 lanes x 16), segments of both
kinds in one launch."""
import io
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from guarded_out import GUARD_BYTE, guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
TILE = 4096                                                                  # positions per tile of the bit packer


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def clip(T, H, W, C, seed):
    """random values in [-0.1, 1.1] with the rounding ties (k + 0.5) / 255 and (k + 0.5) / 65535 scattered in"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(T, H, W, C, generator=g) * 1.2 - 0.1
    flat = x.view(-1)
    n = flat.numel()
    k8 = torch.randint(0, 255, (n,), generator=g).double()
    k16 = torch.randint(0, 65535, (n,), generator=g).double()
    pick = torch.rand(n, generator=g)
    flat[:] = torch.where(pick < 0.15, ((k8 + 0.5) / 255).float(), torch.where(pick < 0.3, ((k16 + 0.5) / 65535).float(), flat))
    return x


def encode(hip, x_dev, depth, bufs=None, runs=True):
    """-> (out uint8 [T, cap] and sizes on the host, the guarded buffers): guards asserted"""
    pngenc = sub("pngenc")
    T, H, W, C = x_dev.shape
    cap = pngenc.frame_bound(H, W, C, depth)
    assert hip.encode_png_bytes(T, H, W, C, depth, runs=runs)[1] == cap
    g_out, g_sizes = bufs or (guarded((T, cap), torch.uint8), guarded((T,), torch.int64))
    out, sizes = hip.encode_png(x_dev, depth, out=g_out.t, sizes=g_sizes.t, runs=runs)
    torch.cuda.synchronize()
    assert out is g_out.t and sizes is g_sizes.t
    name = f"encode_png runs {tuple(x_dev.shape)} {x_dev.dtype} depth {depth}"
    g_out.assert_guards(name)
    g_sizes.assert_guards(name)
    out, sizes = out.cpu(), sizes.cpu()
    for t in range(T):
        assert 0 < int(sizes[t]) <= cap, (name, t, int(sizes[t]))
    return out, sizes, (g_out, g_sizes)


def assert_equals_the_specification(hip, x, depth, want=None):
    """-> the specification's streams (``want``: computed before, shared)"""
    pngenc = sub("pngenc")
    want = want or pngenc.encode_frames_spec(x, depth, runs=True)
    out, sizes, _ = encode(hip, x.cuda(), depth)
    for t, w in enumerate(want):
        n = int(sizes[t])
        got = out[t, :n].numpy().tobytes()
        first = next((i for i in range(min(n, len(w))) if got[i] != w[i]), None)
        assert n == len(w) and got == w, (tuple(x.shape), x.dtype, depth, t, n, len(w), first)
        assert bool((out[t, n:] == GUARD_BYTE).all()), (t, "bytes past sizes[t] were written")
    return want


def segments(x, depth):
    """-> per frame the list of its segments' filtered bytes"""
    pngenc = sub("pngenc")
    _, H, W, C = x.shape
    R = pngenc.geometry(H, W, C, depth)[2]
    return [[rows[r:r + R].tobytes() for r in range(0, H, R)]
            for rows in (pngenc.filter_rows(q, depth) for q in pngenc.frame_samples(x, depth))]


# ---------------------------------------------------------------------------------------------------------------- 1: no match chosen
@DTYPES
def test_without_a_useful_run_the_bytes_are_the_literal_ones(hip, dtype):
    pngenc = sub("pngenc")
    for shape in ((1, 1, 1, 3, 8), (2, 31, 8, 3, 8)):
        x = clip(*shape[:4], seed=sum(shape)).to(dtype)
        assert not any(pngenc.segment_choice(s) for f in segments(x, 8) for s in f)
        want = assert_equals_the_specification(hip, x, 8)
        assert want == pngenc.encode_frames_spec(x, 8)
        out, sizes, _ = encode(hip, x.cuda(), 8, runs=False)
        assert [out[t, :int(sizes[t])].numpy().tobytes() for t in range(shape[0])] == want
    scratch_lit, cap_lit = hip.encode_png_bytes(2, 31, 8, 3, 8)
    scratch_run, cap_run = hip.encode_png_bytes(2, 31, 8, 3, 8, runs=True)
    assert cap_run == cap_lit and scratch_run > scratch_lit


# ---------------------------------------------------------------------------------------------------------------- 2 .. 5: flat frames
# zeros: the whole segment is one run crossing every row (9 x 64 = 576 bytes -> 258 + 258 + 59); constant RGBA; 500 x 100: three
# segments, the last ragged, a run must stop at a segment's end although the byte value goes on; 3 x 8200 x 4 at depth 16: stride
# 65 601, R = 1, one run longer than 64 KiB and sixteen packer tiles long
FLAT = [(2, 9, 21, 3, 8, 0.0), (1, 9, 21, 4, 16, 0.0), (1, 64, 64, 4, 8, 0.5), (1, 500, 100, 3, 8, 0.0), (1, 3, 8200, 4, 16, 0.0)]


@DTYPES
@pytest.mark.parametrize("case", FLAT, ids=lambda c: "x".join(map(str, c[:5])))
def test_flat_frames(hip, case, dtype):
    pngenc = sub("pngenc")
    T, H, W, C, depth, value = case
    x = torch.full((T, H, W, C), value, dtype=dtype)
    segs = segments(x, depth)[0]
    assert all(pngenc.segment_choice(s) for s in segs)
    if case == FLAT[0]:
        kind, length = pngenc.segment_tokens(segs[0])
        assert len(segs) == 1 and length[kind == pngenc.MATCH].tolist() == [258, 258, 59]
    if case == FLAT[3]:                                                      # every byte is zero: the runs end with the segments
        assert segs == [bytes(217 * 301), bytes(217 * 301), bytes(66 * 301)]
    if case == FLAT[4]:
        assert segs == [bytes(65601)] * 3
    want = assert_equals_the_specification(hip, x, depth)
    assert all(len(w) < len(l) for w, l in zip(want, pngenc.encode_frames_spec(x, depth)))


# ---------------------------------------------------------------------------------------------------------------- 6: match lengths
def piecewise_row(C, W):
    """One row of W pixels at depth 8, piecewise constant: a channel toggles between 60 and 130 where the Sub-filtered row is to
    hold a non-zero byte, so the row's filtered bytes are the type byte, pixel 0, and zero runs of CHOSEN lengths between single
    non-zero bytes (filtered byte 1 + C p + c is channel c of pixel p).  The lengths: 1..5 and (L - 1) % 258 in {0, 1, 2, 3, 257}
    on both sides of one and two whole matches; a run that starts at position 4094, so that its first match head is the last
    position of the packer's first tile and the match lies in the next; a run of 600 across position 8192; the rest of the row."""
    plan = [1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 516, 517, 518, 519, 520, ("at", TILE - 2), 300, 775, 259, 260, 261, 262, 258,
            ("at", 2 * TILE - 192), 600]
    n = 1 + C * W
    pos, nonzero = 1 + C, []                                                 # the first zero lies behind pixel 0
    for item in plan:
        L = item[1] - 1 - pos if isinstance(item, tuple) else item
        assert L >= 1
        nonzero.append(pos + L)
        pos += L + 1
    assert pos + 300 < n
    q = np.full((W, C), 60, dtype=np.int64)
    for b in nonzero:
        p, c = divmod(b - 1, C)
        q[p:, c] = 190 - q[p, c]
    return torch.from_numpy(q / 255.0).float().reshape(1, 1, W, C)


@DTYPES
@pytest.mark.parametrize("C", [3, 4])
def test_match_lengths_around_the_limit_and_a_head_on_a_tile_s_last_position(hip, C, dtype):
    pngenc = sub("pngenc")
    x = piecewise_row(C, 4200).to(dtype)
    (seg,), = segments(x, 8)
    data = np.frombuffer(seg, dtype=np.uint8)
    assert data[0] == 1 and pngenc.segment_choice(seg)                       # Sub is chosen, and the run block
    kind, length = pngenc.segment_tokens(seg)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], (data == 0).astype(np.int8), [0]])))
    zero_runs = (edges[1::2] - edges[0::2]).tolist()
    assert {1, 2, 3, 4, 5} <= set(zero_runs)
    for k in (1, 2):                                                         # one and two whole matches in front of the remainder
        assert {0, 1, 2, 3} <= {(L - 1) % 258 for L in zero_runs if (L - 1) // 258 == k}, (k, zero_runs)
    assert {258, 516, 775} <= set(zero_runs)                                 # (L - 1) % 258 = 257: the remainder is one short of a match
    heads = np.flatnonzero(kind == pngenc.MATCH)
    assert kind[TILE - 1] == pngenc.MATCH and length[TILE - 1] == 258        # a head on the last position of a packer tile
    assert any(h < 2 * TILE <= h + length[h] for h in heads)                 # a match across a tile boundary
    assert any(h // 16 != (h + length[h] - 1) // 16 for h in heads)          # ... and across the lanes' stretches
    assert {3, 4, 257, 258} <= set(length[heads].tolist())
    assert_equals_the_specification(hip, x, 8)


# ---------------------------------------------------------------------------------------------------------------- 7: both kinds of segment
def mixed():
    """two frames of 120 x 600 x 3: stride 1801, R = 36, four segments each; zero rows 0..35 in one and 72..107 in the other"""
    x = clip(2, 120, 600, 3, seed=12)
    x[0, :36] = 0.0
    x[1, 72:108] = 0.0
    return x


@DTYPES
def test_segments_with_different_choices_in_one_launch(hip, dtype):
    pngenc = sub("pngenc")
    x = mixed().to(dtype)
    chosen = [[pngenc.segment_choice(s) for s in f] for f in segments(x, 8)]
    assert chosen == [[True, False, False, False], [False, False, True, False]]
    assert_equals_the_specification(hip, x, 8)


# ---------------------------------------------------------------------------------------------------------------- 8: buffers reused
def test_a_second_call_into_the_same_buffers_gives_the_same_bytes(hip):
    x = mixed().cuda()
    out1, sizes1, bufs = encode(hip, x, 8)
    out2, sizes2, _ = encode(hip, x, 8, bufs)
    assert torch.equal(sizes1, sizes2) and torch.equal(out1, out2)
    # ... and a shorter stream into them leaves the longer one's tail alone (nothing past sizes[t] is written)
    out3, sizes3, _ = encode(hip, torch.zeros_like(x), 8, bufs)
    for t in range(2):
        n1, n3 = int(sizes1[t]), int(sizes3[t])
        assert n3 < n1 // 20 and torch.equal(out3[t, n3:], out1[t, n3:])
    # without buffers the op allocates them
    out, sizes = hip.encode_png(x, 8, runs=True)
    assert out.dtype == torch.uint8 and sizes.dtype == torch.int64 and torch.equal(sizes.cpu(), sizes1)
    assert all(torch.equal(out[t, :int(sizes1[t])].cpu(), out1[t, :int(sizes1[t])]) for t in range(2))


# ---------------------------------------------------------------------------------------------------------------- 9: refusals
def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    pngenc = sub("pngenc")
    x = torch.zeros(2, 6, 8, 3, device="cuda")
    cap = pngenc.frame_bound(6, 8, 3, 8)
    out, sizes = guarded((2, cap), torch.uint8), guarded((2,), torch.int64)
    with pytest.raises(ValueError, match="C must be 3 or 4"):
        hip.encode_png(torch.rand(2, 6, 8, 2, device="cuda"), runs=True)
    with pytest.raises(ValueError, match="depth must be 8 or 16"):
        hip.encode_png(x, 12, runs=True)
    with pytest.raises(ValueError, match="out must be"):
        hip.encode_png(x, 8, out=torch.empty(2, cap - 1, dtype=torch.uint8, device="cuda"), runs=True)
    with pytest.raises(ValueError, match="sizes must be"):
        hip.encode_png(x, 8, sizes=torch.empty(2, dtype=torch.int32, device="cuda"), runs=True)
    with pytest.raises(ValueError, match="depth must be 8 or 16"):
        hip.encode_png_bytes(2, 6, 8, 3, 12, runs=True)
    # the C entry point itself, device pointers: the message names the entry point and the argument
    L = hip.lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    need, cap_c = hip.encode_png_bytes(2, 6, 8, 3, 8, runs=True)
    assert cap_c == cap and need > hip.encode_png_bytes(2, 6, 8, 3, 8)[0]
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda **kw: L.svr_png_encode_runs(*[{**dict(frames=p(x), kind=1, T=2, H=6, W=8, C=3, depth=8, scratch=p(scratch), nscratch=need,
                                                        out=p(out.t), cap=cap, sizes=p(sizes.t), stream=None), **kw}[k]
                                                for k in ("frames", "kind", "T", "H", "W", "C", "depth", "scratch", "nscratch", "out", "cap", "sizes", "stream")])
    # (the literal call's scratch is too small for this one)
    for kw, word in ((dict(C=2), b"C must be 3 or 4"), (dict(depth=12), b"depth must be 8 or 16"), (dict(T=0), b"T >= 1"),
                     (dict(nscratch=need - 1), b"scratch_bytes"), (dict(nscratch=hip.encode_png_bytes(2, 6, 8, 3, 8)[0]), b"scratch_bytes"),
                     (dict(cap=cap - 1), b"out_capacity"), (dict(kind=2), b"x_kind"), (dict(frames=None), b"frames"),
                     (dict(sizes=None), b"sizes"), (dict(out=None), b"out"), (dict(scratch=ctypes.c_void_p(scratch.data_ptr() + 4)), b"scratch")):
        assert call(**kw) != 0
        msg = L.svr_last_error()
        assert b"svr_png_encode_runs:" in msg and word in msg, msg
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    sizes.assert_guards("refused calls")
    assert bool(out.poisoned().all()) and bool(sizes.poisoned().all())       # nothing was launched: the payloads are untouched


# ---------------------------------------------------------------------------------------------------------------- 10: command line
@pytest.mark.parametrize("depth", [8, 16])
def test_frame_sink_writes_device_frames_with_runs(hip, tmp_path, depth):
    """A small RGBA clip with a transparent border through FrameSink(PngWriter(runs=True), ops=HipOps): each file is the framed run
    stream of the specification, smaller than the literal one, and decodes -- by PIL at depth 8, by pngenc.read_png16 at depth 16 --
    to the corresponding pack of the frames."""
    import importlib.util
    from PIL import Image
    pngenc, frameio = sub("pngenc"), sub("frameio")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_png_runs", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    chunks = [clip(t, 20, 36, 4, seed=40 + t) for t in (2, 1)]
    for c in chunks:
        c[:, :6] = c[:, -6:] = 0.0
        c[:, :, :9] = c[:, :, -9:] = 0.0
    sink = cli.FrameSink(cli.PngWriter(str(tmp_path / "out"), depth=depth, runs=True), hip)
    for c in chunks:
        sink.put(c.cuda())
    sink.close()
    frames = torch.cat(chunks)
    want, lit = pngenc.encode_frames_spec(frames, depth, runs=True), pngenc.encode_frames_spec(frames, depth)
    assert sorted(os.listdir(tmp_path / "out")) == [f"frame_{i:06d}.png" for i in range(3)]
    for i in range(3):
        path = tmp_path / "out" / f"frame_{i:06d}.png"
        assert len(want[i]) < len(lit[i])
        assert path.read_bytes() == pngenc.png_file(want[i], 36, 20, 4, depth), i
        if depth == 8:
            img = Image.open(io.BytesIO(path.read_bytes()))
            assert img.mode == "RGBA" and np.array_equal(np.asarray(img), frameio.pack_frames_torch(frames[i:i + 1], "rgb8")[0].numpy())
        else:
            codes = frameio.codes(frames[i], 65535.0).to(torch.int32).numpy()
            assert np.array_equal(pngenc.read_png16(str(path)).astype(np.int32), codes)
