"""-m gpu: csrc/svr_frame_pack_colour.hip through HipOps.pack_yuv420p10 against its specification frameio.pack_yuv420p10_torch --
EQUAL, every matrix x range x siting, fp32 and bf16 input (integer results: a mismatch is a finding, not a tolerance) --, special
inputs, other layouts and entry points, and its refusals.

Outputs live in tests/guarded_out.py buffers and the guards must stay intact.  As in tests/test_gpu_frame_pack.py the uint16
payload is not asked for left-over poison (0xA5A5 is out of a 10-bit plane's range, but the comparison with the specification is
the check that every element was written; the payload starts as 0xA5 bytes, never as a previous result)."""
import ctypes
import itertools

import pytest
import torch

from conftest import sub
from guarded_out import guarded
from test_gpu_frame_pack import clip, same

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
COMBOS = list(itertools.product(("bt709", "bt601", "bt2020"), ("tv", "pc"), ("center", "left")))
# [T, H, W]: tests/test_gpu_frame_pack.py's shapes (samples below one vector, odd and even H and W, W a multiple of 16 and not, frame
# starts off 16 bytes, the 16-byte kernel with an odd H and several frames), and two rows of the 16-byte kernel that cross a wave
# (64 lanes x 16 px = 1024) and a workgroup (256 lanes x 16 px = 4096) boundary: where a left neighbour that came from another lane
# could go wrong
SHAPES = [(1, 1, 1), (1, 1, 5), (2, 3, 5), (1, 2, 2), (1, 5, 4), (3, 17, 33), (1, 16, 64), (1, 64, 66), (2, 31, 8), (2, 5, 32), (1, 1, 16),
          (1, 2, 1040), (1, 2, 4112)]
GREEN = {("bt2020", "tv"): (658, 189, 100), ("bt601", "tv"): (578, 215, 137), ("bt709", "tv"): (691, 167, 105), ("bt709", "pc"): (732, 118, 47),
         ("bt2020", "pc"): (694, 143, 42)}


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def run_kernel(hip, x, matrix, range_, siting):
    frameio = sub("frameio")
    T, H, W, C = x.shape
    g = guarded(frameio.packed_shape(T, H, W, C, "yuv420p10"), torch.uint16)
    out = hip.pack_yuv420p10(x if x.is_cuda else x.cuda(), matrix, range_, siting, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"pack_yuv420p10 {matrix} {range_} {siting} {tuple(x.shape)} {x.dtype}")
    return out.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, dtype):
    frameio = sub("frameio")
    x = clip(*shape, 3, seed=sum(shape) + 3).to(dtype)
    dev = x.cuda()
    for matrix, range_, siting in COMBOS:
        want = frameio.pack_yuv420p10_torch(x, matrix, range_, siting)
        got = run_kernel(hip, dev, matrix, range_, siting)
        assert same(got, want), (matrix, range_, siting, int((got.to(torch.int32) != want.to(torch.int32)).sum()))
    # the planes of today's format, from the other kernel
    assert same(run_kernel(hip, dev, "bt709", "tv", "center"), hip.pack_frames(dev, "yuv420p10").cpu())


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_non_finite_and_negative_zero(hip, dtype):
    frameio = sub("frameio")
    x = clip(1, 16, 64, 3, seed=9)
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    g = torch.Generator().manual_seed(10)
    where = torch.randperm(x.numel(), generator=g)[:400]
    x.view(-1)[where] = specials[torch.arange(400) % 4]
    x = x.to(dtype)
    for src in (x, x[:, :5, :7].contiguous()):                                # the 16-byte kernel and the element-wise one
        for matrix, range_, siting in COMBOS:
            assert same(run_kernel(hip, src, matrix, range_, siting), frameio.pack_yuv420p10_torch(src, matrix, range_, siting)), (matrix, range_, siting)
    one = specials[:3].reshape(1, 1, 1, 3).to(dtype)                          # NaN -> 0, +inf -> full scale, -inf -> 0: green
    for (matrix, range_), green in GREEN.items():
        for siting in ("center", "left"):
            assert tuple(run_kernel(hip, one, matrix, range_, siting).flatten().tolist()) == green, (matrix, range_, siting)


def test_output_allocated_by_the_op_and_an_unaligned_view(hip):
    """Without ``out`` the op allocates; frames that start 4 bytes into an allocation (a dense view) take the element-wise route
    and give the same bytes."""
    frameio = sub("frameio")
    x = clip(2, 6, 16, 3, seed=4)
    store = torch.empty(x.numel() + 1, device="cuda")
    shifted = store[1:].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    for matrix, range_, siting in COMBOS:
        want = frameio.pack_yuv420p10_torch(x, matrix, range_, siting)
        got = hip.pack_yuv420p10(x.cuda(), matrix, range_, siting)
        assert got.dtype == torch.uint16 and got.is_cuda and same(got.cpu(), want), (matrix, range_, siting)
        assert same(hip.pack_yuv420p10(shifted, matrix, range_, siting).cpu(), want), (matrix, range_, siting)
    assert same(hip.pack_yuv420p10(x.cuda()).cpu(), frameio.pack_frames_torch(x, "yuv420p10"))          # (the defaults)
    assert same(frameio.pack_yuv420p10(x.cuda(), "bt2020", "tv", "left", ops=hip).cpu(), frameio.pack_yuv420p10_torch(x, "bt2020", "tv", "left"))


def test_frame_sink_packs_device_frames_as_the_writer_asks(hip):
    """The command line's hand-over with frames on the GPU and a writer that asks for BT.2020 tv planes with left-sited chroma."""
    import importlib.util
    import os
    from conftest import ROOT
    frameio = sub("frameio")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_colour_sink", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    seen = []

    class Keep:
        fmt, alpha, pack = "yuv420p10", False, ("bt2020", "tv", "left")

        def write(self, arr, height, width):
            seen.append((arr.copy(), height, width))

        def close(self):
            pass

    chunks = [clip(t, 6, 16, 3, seed=20 + t) for t in (3, 1, 2)]
    sink = cli.FrameSink(Keep(), hip)
    for c in chunks:
        sink.put(c.cuda())
    sink.close()
    assert len(seen) == 3 and all(b.is_pinned() for b in sink.buffers)
    for c, (arr, h, w) in zip(chunks, seen):
        assert (h, w) == (6, 16) and same(torch.from_numpy(arr), frameio.pack_yuv420p10_torch(c, "bt2020", "tv", "left"))


def test_refusals_name_the_argument_and_launch_nothing(hip):
    hip_lib = sub("hip_lib")
    x = torch.rand(2, 6, 8, 3, device="cuda")
    shape = (2, 48 + 24)
    out = guarded(shape, torch.uint16)
    with pytest.raises(ValueError, match="frames must live on"):
        hip.pack_yuv420p10(x.cpu(), "bt2020", "tv", "left", out=out.t)
    with pytest.raises(ValueError, match="frames must be contiguous"):
        hip.pack_yuv420p10(torch.rand(2, 6, 8, 4, device="cuda")[..., :3], "bt2020", "tv", "left", out=out.t)
    with pytest.raises(ValueError, match="frames must be contiguous"):
        hip.pack_yuv420p10(torch.rand(2, 12, 8, 3, device="cuda")[:, ::2], "bt2020", "tv", "left", out=out.t)
    with pytest.raises(ValueError, match="C = 3"):
        hip.pack_yuv420p10(torch.rand(2, 6, 8, 4, device="cuda"), "bt2020", "tv", "left", out=out.t)
    with pytest.raises(ValueError, match="frames must be"):
        hip.pack_yuv420p10(x.half(), "bt2020", "tv", "left", out=out.t)
    for bad in (torch.empty(2, 48 + 23, dtype=torch.uint16, device="cuda"), torch.empty(shape, dtype=torch.int16, device="cuda"),
                torch.empty(shape, dtype=torch.uint16), torch.empty(2, 2 * (48 + 24), dtype=torch.uint16, device="cuda")[:, ::2]):
        with pytest.raises(ValueError, match="out must"):
            hip.pack_yuv420p10(x, "bt2020", "tv", "left", out=bad)
    for kw, word in ((dict(matrix="bt2100"), "matrix"), (dict(range_="full"), "range_"), (dict(siting="topleft"), "siting")):
        with pytest.raises(ValueError, match=word):
            hip.pack_yuv420p10(x, out=out.t, **kw)
    # the C entry point itself, device pointers: bad codes and a wrong out_bytes, the message names the argument
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L, need = hip.lib, 2 * 2 * (48 + 24)
    for codes, word in (((3, 0, 1), b"matrix"), ((-1, 0, 1), b"matrix"), ((2, 2, 1), b"range"), ((2, 0, 2), b"siting"), ((2, 0, -1), b"siting")):
        assert L.svr_pack_yuv420p10(p(x), 1, 2, 6, 8, *codes, p(out.t), need, None) != 0
        assert word in L.svr_last_error() and b"svr_pack_yuv420p10" in L.svr_last_error()
    assert L.svr_pack_yuv420p10(p(x), 2, 2, 6, 8, 2, 0, 1, p(out.t), need, None) != 0 and b"x_kind" in L.svr_last_error()
    for nbytes in (need - 2, need + 16, need // 2, 0):
        assert L.svr_pack_yuv420p10(p(x), 1, 2, 6, 8, 2, 0, 1, p(out.t), nbytes, None) != 0
        assert b"out_bytes" in L.svr_last_error()
    with pytest.raises(hip_lib.HipLibraryError, match="out_bytes"):
        hip_lib.check(L.svr_pack_yuv420p10(p(x), 1, 2, 6, 8, 2, 0, 1, p(out.t), 5, None), "svr_pack_yuv420p10")
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was launched: the payload is untouched
