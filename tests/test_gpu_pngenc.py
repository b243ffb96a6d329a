"""-m gpu: csrc/svr_png.hip through HipOps.encode_png against its specification pngenc.encode_frames_spec -- EQUAL byte for byte,
``sizes`` included, fp32 and bf16 input (a mismatch is a finding, not a tolerance) --, what lies past a stream, the refusals, and
the command line's hand-over (FrameSink + PngWriter) with frames on the device.

``out`` and ``sizes`` live in tests/guarded_out.py buffers and the guards must stay intact.  Bytes of a frame's slot past sizes[t]
are NOT written by the kernels: they must still hold the poison byte 0xA5 after the call."""
import io
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from guarded_out import GUARD_BYTE, guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
# (T, H, W, C, depth).  The CPU suite's shapes (the last: three segments, a ragged one); rows that cross a wave's 64 lanes and a
# workgroup's 256 (1040 and 4112 pixels); stride 65 601 > 65 536: R = 1 and a row longer than a segment's nominal size (and than
# one 4096-symbol tile of the bit packer, sixteen times over); frames that start off 16 bytes
SHAPES = [(1, 1, 1, 3, 8), (2, 3, 5, 3, 8), (1, 2, 2, 4, 8), (3, 17, 33, 3, 16), (1, 5, 40, 4, 16), (1, 500, 100, 3, 8),
          (1, 2, 1040, 3, 8), (1, 2, 4112, 3, 8), (1, 3, 8200, 4, 16), (2, 31, 8, 3, 8)]
FIB = [1, 1]
while len(FIB) < 24:
    FIB.append(FIB[-1] + FIB[-2])


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


def encode(hip, x_dev, depth, bufs=None):
    """-> (out uint8 [T, cap] and sizes on the host, the guarded buffers): guards asserted, the bytes past each stream still poison"""
    pngenc = sub("pngenc")
    T, H, W, C = x_dev.shape
    cap = pngenc.frame_bound(H, W, C, depth)
    assert hip.encode_png_bytes(T, H, W, C, depth)[1] == cap
    g_out, g_sizes = bufs or (guarded((T, cap), torch.uint8), guarded((T,), torch.int64))
    out, sizes = hip.encode_png(x_dev, depth, out=g_out.t, sizes=g_sizes.t)
    torch.cuda.synchronize()
    assert out is g_out.t and sizes is g_sizes.t
    name = f"encode_png {tuple(x_dev.shape)} {x_dev.dtype} depth {depth}"
    g_out.assert_guards(name)
    g_sizes.assert_guards(name)
    out, sizes = out.cpu(), sizes.cpu()
    for t in range(T):
        assert 0 < int(sizes[t]) <= cap, (name, t, int(sizes[t]))
    return out, sizes, (g_out, g_sizes)


def assert_equals_the_specification(hip, x, depth, x_dev=None):
    pngenc = sub("pngenc")
    want = pngenc.encode_frames_spec(x, depth)
    out, sizes, bufs = encode(hip, x.cuda() if x_dev is None else x_dev, depth)
    for t, w in enumerate(want):
        n = int(sizes[t])
        got = out[t, :n].numpy().tobytes()
        first = next((i for i in range(min(n, len(w))) if got[i] != w[i]), None)
        assert n == len(w) and got == w, (tuple(x.shape), x.dtype, depth, t, n, len(w), first)
        assert bool((out[t, n:] == GUARD_BYTE).all()), (t, "bytes past sizes[t] were written")
    return bufs


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, dtype):
    T, H, W, C, depth = shape
    assert_equals_the_specification(hip, clip(T, H, W, C, seed=sum(shape)).to(dtype), depth)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_a_dense_view_four_bytes_into_an_allocation(hip, dtype):
    x = clip(2, 31, 8, 3, seed=4).to(dtype)
    store = torch.empty(x.numel() + 4 // x.element_size(), dtype=dtype, device="cuda")
    shifted = store[4 // x.element_size():].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    assert_equals_the_specification(hip, x, 8, shifted)
    assert_equals_the_specification(hip, x, 16, shifted)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_special_content(hip, dtype):
    assert_equals_the_specification(hip, torch.zeros(2, 9, 21, 3, dtype=dtype), 8)
    assert_equals_the_specification(hip, torch.zeros(1, 9, 21, 4, dtype=dtype), 16)
    rgba = clip(1, 12, 30, 4, seed=2)
    rgba[..., 3] = 1.0
    for depth in (8, 16):
        assert_equals_the_specification(hip, rgba.to(dtype), depth)
    x = clip(1, 16, 64, 3, seed=9)
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    g = torch.Generator().manual_seed(10)
    where = torch.randperm(x.numel(), generator=g)[:400]
    x.view(-1)[where] = specials[torch.arange(400) % 4]
    for depth in (8, 16):
        assert_equals_the_specification(hip, x.to(dtype), depth)
        assert_equals_the_specification(hip, x[:, :5, :7].contiguous().to(dtype), depth)


def test_the_length_limit_path(hip):
    """A single-row frame at depth 8 for which the specification picks filter 0 -- verified here on the CPU --, so that the
    segment's histogram is the row's own value counts plus the type byte (on value 0) and the end of block, and whose first tree is
    deeper than 15 -- verified too: the device halves the counts and rebuilds, as the specification does.

    The row: 1 x 87381 x 3, the values 0..17 with counts 2^17..2^0 (3 * 87381 = 2^18 - 1), shuffled with a fixed seed: every count
    exceeds the sum of all smaller ones, so the tree is one chain of depth 18 whatever the two extra symbols do.  Counts
    F(1)..F(24) on the values 0..23 (1 x 40464 x 3) do NOT give such a tree once those two symbols are in: the weights 1, 1, 1, 2,
    3, 5, ... -- wherever the type byte's + 1 falls -- merge into two interleaved chains of depth 13 (asserted below), and with the
    frequent values small or large the cheapest filter is not reliably 0 either.  That frame is encoded as well, equal byte for
    byte, with whatever filter and depth the specification gives it."""
    pngenc = sub("pngenc")
    vals = torch.cat([torch.full((2 ** (17 - v),), float(v)) for v in range(18)])
    assert vals.numel() == 3 * 87381
    vals = vals[torch.randperm(vals.numel(), generator=torch.Generator().manual_seed(1))]
    x = (vals / 255.0).reshape(1, 1, 87381, 3)
    rows = pngenc.filter_rows(pngenc.frame_samples(x, 8)[0], 8)
    assert rows[0, 0] == 0
    hist = np.bincount(rows.reshape(-1), minlength=256).tolist() + [1]
    assert hist[:18] == [2 ** 17 + 1] + [2 ** (17 - v) for v in range(1, 18)] and sum(hist[18:]) == 1
    assert max(pngenc.tree_lengths(hist)) == 18 and max(pngenc.code_lengths(hist)) == 15
    assert_equals_the_specification(hip, x, 8)
    assert_equals_the_specification(hip, x.to(BF16), 8)
    for k in range(24):
        counts = list(FIB)
        counts[k] += 1
        assert max(pngenc.tree_lengths(counts + [1])) == 13
    vals = torch.cat([torch.full((c,), float(v)) for v, c in enumerate(FIB)])
    assert vals.numel() == 3 * 40464
    vals = vals[torch.randperm(vals.numel(), generator=torch.Generator().manual_seed(1))]
    assert_equals_the_specification(hip, (vals / 255.0).reshape(1, 1, 40464, 3), 8)


def test_a_second_call_into_the_same_buffers_gives_the_same_bytes(hip):
    x = clip(2, 40, 50, 3, seed=6).cuda()
    out1, sizes1, bufs = encode(hip, x, 8)
    out2, sizes2, _ = encode(hip, x, 8, bufs)
    assert torch.equal(sizes1, sizes2) and torch.equal(out1, out2)
    # ... and a shorter stream into them leaves the longer one's tail alone (nothing past sizes[t] is written)
    out3, sizes3, _ = encode(hip, torch.zeros_like(x), 8, bufs)
    for t in range(2):
        n1, n3 = int(sizes1[t]), int(sizes3[t])
        assert n3 < n1 and torch.equal(out3[t, n3:], out1[t, n3:])
    # without buffers the op allocates them
    out, sizes = hip.encode_png(x, 8)
    assert out.dtype == torch.uint8 and sizes.dtype == torch.int64 and torch.equal(sizes.cpu(), sizes1)
    assert all(torch.equal(out[t, :int(sizes1[t])].cpu(), out1[t, :int(sizes1[t])]) for t in range(2))


def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    pngenc = sub("pngenc")
    x = torch.rand(2, 6, 8, 3, device="cuda")
    cap = pngenc.frame_bound(6, 8, 3, 8)
    out, sizes = guarded((2, cap), torch.uint8), guarded((2,), torch.int64)
    with pytest.raises(ValueError, match="C must be 3 or 4"):
        hip.encode_png(torch.rand(2, 6, 8, 2, device="cuda"))
    with pytest.raises(ValueError, match="depth must be 8 or 16"):
        hip.encode_png(x, 12)
    with pytest.raises(ValueError, match="at least one pixel"):
        hip.encode_png(x[:0])
    with pytest.raises(ValueError, match="out must be"):
        hip.encode_png(x, 8, out=torch.empty(2, cap - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        hip.encode_png(x, 8, out=torch.empty(1, cap, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        hip.encode_png(x, 8, out=torch.empty(2, cap, dtype=torch.int8, device="cuda"))
    with pytest.raises(ValueError, match="sizes must be"):
        hip.encode_png(x, 8, sizes=torch.empty(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="frames must be contiguous"):
        hip.encode_png(torch.rand(2, 6, 8, 4, device="cuda")[..., :3])
    with pytest.raises(ValueError, match="frames must be contiguous"):
        hip.encode_png(x[:, ::2])
    with pytest.raises(ValueError, match="fp32 or bf16"):
        hip.encode_png(x.half())
    with pytest.raises(ValueError, match="frames must live on"):
        hip.encode_png(x.cpu())
    # the C entry point itself, device pointers: the message names the argument
    L = hip.lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    need, cap_c = hip.encode_png_bytes(2, 6, 8, 3, 8)
    assert cap_c == cap
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda **kw: L.svr_png_encode(*[{**dict(frames=p(x), kind=1, T=2, H=6, W=8, C=3, depth=8, scratch=p(scratch), nscratch=need,
                                                   out=p(out.t), cap=cap, sizes=p(sizes.t), stream=None), **kw}[k]
                                           for k in ("frames", "kind", "T", "H", "W", "C", "depth", "scratch", "nscratch", "out", "cap", "sizes", "stream")])
    for kw, word in ((dict(C=2), b"C must be 3 or 4"), (dict(depth=12), b"depth must be 8 or 16"), (dict(T=0), b"T >= 1"),
                     (dict(nscratch=need - 1), b"scratch_bytes"), (dict(cap=cap - 1), b"out_capacity"), (dict(kind=2), b"x_kind"),
                     (dict(frames=None), b"frames"), (dict(sizes=None), b"sizes"), (dict(scratch=ctypes.c_void_p(scratch.data_ptr() + 4)), b"scratch")):
        assert call(**kw) != 0
        msg = L.svr_last_error()
        assert b"svr_png_encode" in msg and word in msg, msg
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    sizes.assert_guards("refused calls")
    assert bool(out.poisoned().all()) and bool(sizes.poisoned().all())       # nothing was launched: the payloads are untouched


@pytest.mark.parametrize("depth", [8, 16])
def test_frame_sink_writes_device_frames_as_png_files(hip, tmp_path, depth):
    """A small clip on the device through FrameSink(PngWriter, ops=HipOps): each file is the framed stream of the specification and
    decodes -- by PIL at depth 8, by pngenc.read_png16 at depth 16 -- to the corresponding pack of the frames."""
    import importlib.util
    from PIL import Image
    pngenc, frameio = sub("pngenc"), sub("frameio")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_png", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    chunks = [clip(t, 20, 36, 4, seed=40 + t) for t in (3, 1, 2)]
    sink = cli.FrameSink(cli.PngWriter(str(tmp_path / "out"), depth=depth), hip)
    for c in chunks:
        sink.put(c.cuda())
    sink.close()
    assert all(b is None or b.is_pinned() for b in sink.buffers) and any(b is not None for b in sink.buffers)
    frames = torch.cat(chunks)
    want = pngenc.encode_frames_spec(frames, depth)
    assert sorted(os.listdir(tmp_path / "out")) == [f"frame_{i:06d}.png" for i in range(6)]
    for i in range(6):
        path = tmp_path / "out" / f"frame_{i:06d}.png"
        assert path.read_bytes() == pngenc.png_file(want[i], 36, 20, 4, depth), i
        if depth == 8:
            img = Image.open(io.BytesIO(path.read_bytes()))
            assert img.mode == "RGBA" and np.array_equal(np.asarray(img), frameio.pack_frames_torch(frames[i:i + 1], "rgb8")[0].numpy())
        else:
            codes = frameio.codes(frames[i], 65535.0).to(torch.int32).numpy()
            assert np.array_equal(pngenc.read_png16(str(path)).astype(np.int32), codes)
