"""-m gpu: csrc/svr_planar_out.hip through HipOps.pack_planar against its specification planar_out.pack_planar_torch -- EQUAL, every
(sub, siting, bits) instance, fp32 and bf16 input (integer results: a mismatch is a finding, not a tolerance) --, the yuv420p10 kernel
on the device, special inputs, other layouts, the command line's hand-over and the refusals.

Outputs live in tests/guarded_out.py buffers and the guards are asserted after every launch.  As in tests/test_gpu_colour_out.py the
payload is not asked for left-over poison (0xA5 is a valid 8-bit sample; the comparison with the specification is the check that every
element was written: the payload starts as 0xA5 bytes, never as a previous result)."""
import ctypes
import itertools

import pytest
import torch

from conftest import sub
from guarded_out import guarded
from test_gpu_colour_out import SHAPES
from test_gpu_frame_pack import clip, same

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SITINGS = {"420": ("center", "left", "topleft"), "422": ("center", "left"), "444": ("left",)}
INSTANCES = [(s, siting, bits) for s in ("420", "422", "444") for siting in SITINGS[s] for bits in (8, 10, 12)]
COLOURS = list(itertools.product(("bt709", "bt601", "bt2020"), ("tv", "pc")))
# the vector shape with H = 1, an odd H, and a first chroma row whose upper neighbour clamps next to ones whose does not
TOPLEFT_SHAPES = [(1, 1, 32), (1, 3, 16), (2, 4, 48)]
# the green of (NaN, +inf, -inf) -> (0, 65535, 0), worked out with Fractions in tests/test_planar_out.py::check_value
GREEN = {(8, "bt709", "tv"): (173, 42, 26), (10, "bt709", "tv"): (691, 167, 105), (12, "bt2020", "tv"): (2632, 756, 400),
         (10, "bt2020", "pc"): (694, 143, 42)}


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def run_kernel(hip, x, s, bits, matrix, range_, siting):
    planar = sub("planar")
    T, H, W, _ = x.shape
    g = guarded(planar.planar_shape(T, H, W, s), planar.planar_dtype(bits))
    out = hip.pack_planar(x if x.is_cuda else x.cuda(), s, bits, matrix, range_, siting, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"pack_planar {s} {bits} {matrix} {range_} {siting} {tuple(x.shape)} {x.dtype}")
    return out.cpu()


def differing(got, want):
    return int((got.to(torch.int32) != want.to(torch.int32)).sum())


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + TOPLEFT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, dtype):
    planar_out = sub("planar_out")
    x = clip(*shape, 3, seed=sum(shape) + 5).to(dtype)
    dev = x.cuda()
    for n, (s, siting, bits) in enumerate(INSTANCES):
        if shape in TOPLEFT_SHAPES and siting != "topleft":
            continue
        matrix, range_ = COLOURS[(n + sum(shape)) % 6]                         # (the templates do not depend on them)
        want = planar_out.pack_planar_torch(x, s, bits, matrix, range_, siting)
        got = run_kernel(hip, dev, s, bits, matrix, range_, siting)
        assert same(got, want), (s, siting, bits, matrix, range_, differing(got, want))
        if s == "420" and bits == 10 and siting != "topleft":                  # the yuv420p10 kernel, on the device
            assert same(got, hip.pack_yuv420p10(dev, matrix, range_, siting).cpu()), (siting, matrix, range_)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 16, 64), (3, 17, 33)], ids=["vector", "element"])
def test_every_matrix_and_range(hip, shape, dtype):
    planar_out = sub("planar_out")
    x = clip(*shape, 3, seed=41).to(dtype)
    dev = x.cuda()
    for (matrix, range_), (s, siting, bits) in itertools.product(COLOURS, INSTANCES):
        want = planar_out.pack_planar_torch(x, s, bits, matrix, range_, siting)
        got = run_kernel(hip, dev, s, bits, matrix, range_, siting)
        assert same(got, want), (s, siting, bits, matrix, range_, differing(got, want))


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_non_finite_and_negative_zero(hip, dtype):
    planar_out = sub("planar_out")
    x = clip(1, 16, 64, 3, seed=9)
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    g = torch.Generator().manual_seed(10)
    where = torch.randperm(x.numel(), generator=g)[:400]
    x.view(-1)[where] = specials[torch.arange(400) % 4]
    x = x.to(dtype)
    for src in (x, x[:, :5, :7].contiguous()):                                # the vector shape and the element shape
        for n, (s, siting, bits) in enumerate(INSTANCES):
            matrix, range_ = COLOURS[n % 6]
            want = planar_out.pack_planar_torch(src, s, bits, matrix, range_, siting)
            got = run_kernel(hip, src, s, bits, matrix, range_, siting)
            assert same(got, want), (s, siting, bits, matrix, range_, differing(got, want))
    one = specials[:3].reshape(1, 1, 1, 3).to(dtype)                          # NaN -> 0, +inf -> full scale, -inf -> 0: green
    for (bits, matrix, range_), green in GREEN.items():
        for s, siting, b in INSTANCES:
            if b == bits:
                assert tuple(run_kernel(hip, one, s, bits, matrix, range_, siting).flatten().tolist()) == green, (s, siting, bits)


def test_output_allocated_by_the_op_and_an_unaligned_view(hip):
    """Without ``out`` the op allocates; frames that start 4 bytes into an allocation (a dense view) take the element route; both
    give the guarded run's bytes.  (2, 6, 16): at 8 bits the chroma rows of 4:2:0 / 4:2:2 are single 8-byte stores, every other one
    off 16 bytes."""
    planar_out, planar = sub("planar_out"), sub("planar")
    x = clip(2, 6, 16, 3, seed=4)
    store = torch.empty(x.numel() + 1, device="cuda")
    shifted = store[1:].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    for n, (s, siting, bits) in enumerate(INSTANCES):
        matrix, range_ = COLOURS[n % 6]
        want = planar_out.pack_planar_torch(x, s, bits, matrix, range_, siting)
        got = hip.pack_planar(x.cuda(), s, bits, matrix, range_, siting)
        assert got.dtype == planar.planar_dtype(bits) and got.is_cuda and same(got.cpu(), want), (s, siting, bits)
        assert same(hip.pack_planar(shifted, s, bits, matrix, range_, siting).cpu(), want), (s, siting, bits)
        assert same(run_kernel(hip, x, s, bits, matrix, range_, siting), want), (s, siting, bits)
    assert same(planar_out.pack_planar(x.cuda(), "422", 8, "bt601", "pc", "center", ops=hip).cpu(),
                planar_out.pack_planar_torch(x, "422", 8, "bt601", "pc", "center"))


def test_frame_sink_packs_device_frames_as_the_writer_asks(hip):
    """The command line's hand-over with frames on the GPU and a writer whose ``planes`` names the planes."""
    import importlib.util
    import os
    from conftest import ROOT
    planar_out = sub("planar_out")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_planar_sink", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    for planes in (("422", 10, "bt2020", "tv", "left"), ("420", 8, "bt709", "tv", "left")):
        seen = []

        class Keep:
            fmt, alpha, pack = "bgr8", False, None

            def write(self, arr, height, width):
                seen.append((arr.copy(), height, width))

            def close(self):
                pass

        Keep.planes = planes
        chunks = [clip(t, 6, 16, 3, seed=20 + t) for t in (3, 1, 2)]
        sink = cli.FrameSink(Keep(), hip)
        for c in chunks:
            sink.put(c.cuda())
        sink.close()
        assert len(seen) == 3 and all(b.is_pinned() for b in sink.buffers)
        for c, (arr, h, w) in zip(chunks, seen):
            assert (h, w) == (6, 16) and same(torch.from_numpy(arr), planar_out.pack_planar_torch(c, *planes)), planes


def test_refusals_name_the_argument_and_launch_nothing(hip):
    hip_lib = sub("hip_lib")
    x = torch.rand(2, 6, 8, 3, device="cuda")
    shape = (2, 48 + 48)                                                       # 4:2:2
    out = guarded(shape, torch.uint16)
    call = lambda frames=x, s="422", bits=10, matrix="bt2020", range_="tv", siting="left", o=out.t: hip.pack_planar(
        frames, s, bits, matrix, range_, siting, out=o)
    with pytest.raises(ValueError, match="frames must live on"):
        call(x.cpu())
    with pytest.raises(ValueError, match="frames must be contiguous"):
        call(torch.rand(2, 6, 8, 4, device="cuda")[..., :3])
    with pytest.raises(ValueError, match="frames must be contiguous"):
        call(torch.rand(2, 12, 8, 3, device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="C = 3"):
        call(torch.rand(2, 6, 8, 4, device="cuda"))
    with pytest.raises(ValueError, match="frames must be"):
        call(x.half())
    for bad in (torch.empty(2, 48 + 47, dtype=torch.uint16, device="cuda"), torch.empty(shape, dtype=torch.uint8, device="cuda"),
                torch.empty(shape, dtype=torch.uint16), torch.empty(2, 2 * (48 + 48), dtype=torch.uint16, device="cuda")[:, ::2],
                torch.empty(2, 48 + 24, dtype=torch.uint16, device="cuda")):   # (the last: 4:2:0's shape)
        with pytest.raises(ValueError, match="out must"):
            call(o=bad)
    for kw, word in ((dict(s="411"), "sub"), (dict(bits=9), "bits"), (dict(matrix="bt2100"), "matrix"), (dict(range_="full"), "range_"),
                     (dict(siting="topleft"), "siting"), (dict(s="444", siting="center"), "siting"), (dict(siting="top"), "siting")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    # the C entry point itself, device pointers: bad codes and a wrong out_bytes, the message names the argument
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L, need = hip.lib, 2 * 2 * (48 + 48)
    good = (1, 10, 2, 0, 1)                                                    # sub, bits, matrix, range, siting
    for at, code, word in ((0, 3, b"sub"), (0, -1, b"sub"), (1, 9, b"bits"), (1, 16, b"bits"), (2, 3, b"matrix"), (2, -1, b"matrix"),
                           (3, 2, b"range"), (4, 3, b"siting"), (4, -1, b"siting"), (4, 2, b"siting")):   # (the last: topleft for 4:2:2)
        codes = good[:at] + (code,) + good[at + 1:]
        assert L.svr_pack_planar(p(x), 1, 2, 6, 8, *codes, p(out.t), need, None) != 0
        assert word in L.svr_last_error() and b"svr_pack_planar" in L.svr_last_error(), L.svr_last_error()
    assert L.svr_pack_planar(p(x), 1, 2, 6, 8, 2, 10, 2, 0, 0, p(out.t), 2 * 2 * 144, None) != 0     # center for 4:4:4
    assert b"siting" in L.svr_last_error()
    assert L.svr_pack_planar(p(x), 2, 2, 6, 8, *good, p(out.t), need, None) != 0 and b"x_kind" in L.svr_last_error()
    for nbytes in (need - 2, need + 16, need // 2, 2 * 2 * (48 + 24), 0):      # (need // 2: the 8-bit planes' size)
        assert L.svr_pack_planar(p(x), 1, 2, 6, 8, *good, p(out.t), nbytes, None) != 0
        assert b"out_bytes" in L.svr_last_error()
    assert L.svr_pack_planar(p(x), 1, 2, 6, 8, 1, 8, 2, 0, 1, p(out.t), need, None) != 0 and b"out_bytes" in L.svr_last_error()
    with pytest.raises(hip_lib.HipLibraryError, match="out_bytes"):
        hip_lib.check(L.svr_pack_planar(p(x), 1, 2, 6, 8, *good, p(out.t), 5, None), "svr_pack_planar")
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was launched: the payload is untouched
