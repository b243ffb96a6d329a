"""-m gpu: csrc/svr_active.hip through HipOps.active_profile against its specification active.profile_torch -- EQUAL, fp32 and bf16
input (integer counts: a mismatch is a finding, not a tolerance) --, its refusals, and pipeline.upscale(area=...) on the device.

Outputs live in tests/guarded_out.py buffers, pre-filled with garbage (the 0xA5 bytes of the payload: -1515870811 per counter), and
the guards must stay intact: the call itself has to bring the profile to zero before it counts."""
import pytest
import torch

from conftest import sub
from guarded_out import guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
PARAMS = dict(dark=8, specks=0, skew=4, margin=2, gain=6)
# (T, H, W, C): the smallest shapes at which the geometry can go wrong
SHAPES = [
    (2, 4, 4, 4),        # alpha ignored
    (3, 19, 23, 3),      # nothing aligned
    (1, 130, 7, 4),      # more rows than a band (five bands of 32, the last of two rows), narrow: a unit of 8 pixels spans rows
    (2, 64, 260, 3),     # a row wider than one pass of the workgroup
    (3, 5, 5, 3),        # frames that start off 16 bytes
    (2, 36, 300, 3),     # a band of more than 256 units (the unit loop goes round) and a second band of four rows
]
# beyond the issue's list: columns at and beyond the LDS counters (4096), which are counted in global memory
EXTRA_SHAPES = [(1, 3, 4100, 3)]
DARKS = (0, 8, 254, 255)


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def clip(T, H, W, C, seed):
    """A letterboxed random field: values in [-0.1, 1.1] with the rounding ties (k + 0.5) / 255 and the greys just at and above the
    thresholds of DARKS scattered in; black rows at the top and the bottom, a black column band on the left."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(T, H, W, C, generator=g) * 1.2 - 0.1
    flat = x.view(-1)
    k8 = torch.randint(0, 255, (flat.numel(),), generator=g).double()
    flat[:] = torch.where(torch.rand(flat.numel(), generator=g) < 0.2, ((k8 + 0.5) / 255).float(), flat)
    grey = torch.tensor([0, 1, 8, 9, 254, 255])[torch.randint(0, 6, (T, H, W), generator=g)].double() / 255
    x[:] = torch.where((torch.rand(T, H, W, generator=g) < 0.3)[..., None], grey.float()[..., None].expand(T, H, W, C), x)
    x[:, :H // 5] = 0.0
    x[:, H - H // 6:] = 0.0
    x[:, :, :W // 7] = 0.0
    return x


def run_kernel(hip, x, dark):
    H, W = x.shape[1], x.shape[2]
    g = guarded((H + W,), torch.int32)
    assert bool(g.poisoned().all())                                            # garbage in: every counter starts at 0xA5A5A5A5
    out = hip.active_profile(x.cuda(), dark, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"active_profile {tuple(x.shape)} {x.dtype} dark={dark}")
    return out.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + EXTRA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, dtype):
    active = sub("active")
    T, H, W, C = shape
    x = clip(*shape, seed=sum(shape)).to(dtype)
    for dark in DARKS:
        want = active.profile_torch(x, dark)
        got = run_kernel(hip, x, dark)
        assert got.dtype == torch.int32 and torch.equal(got, want), (dark, int((got != want).sum()))
        assert int(got[:H].sum()) == int(got[H:].sum())
    assert int(want.sum()) == 0                                                # dark = 255 counts nothing
    want = active.profile_torch(x, 8)
    assert int(want.sum()) > 0
    assert torch.equal(run_kernel(hip, x, 8), run_kernel(hip, x, 8))           # two calls: the same bits
    # frames 4 bytes into an allocation: the element-wise route gives the same counts
    store = torch.empty(x.numel() + 2, dtype=dtype, device="cuda")
    shifted = store[4 // x.element_size():][:x.numel()].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    assert torch.equal(hip.active_profile(shifted, 8).cpu(), want)
    assert torch.equal(active.profile(x.cuda(), 8, hip).cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_dark_and_flat_clips(hip, dtype):
    """An all-dark clip gives all zeros (nothing is added anywhere); a flat lit one gives T W per row and T H per column."""
    for T, H, W in ((2, 64, 260), (3, 19, 23)):
        for v in (0.0, 8 / 255):
            assert run_kernel(hip, torch.full((T, H, W, 3), v).to(dtype), 8).tolist() == [0] * (H + W)
        for v in (9 / 255, 1.0):
            assert run_kernel(hip, torch.full((T, H, W, 3), v).to(dtype), 8).tolist() == [T * W] * H + [T * H] * W


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_non_finite_negative_and_large_values(hip, dtype):
    active = sub("active")
    x = clip(1, 64, 260, 3, seed=9)
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.5, 1.5, -0.0])
    where = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(10))[:3000]
    x.view(-1)[where] = specials[torch.arange(3000) % 6]
    x = x.to(dtype)
    for src in (x, x[:, :19, :23].contiguous()):
        assert torch.equal(run_kernel(hip, src, 8), active.profile_torch(src, 8))
    for v, lit in ((float("nan"), 0), (float("inf"), 1), (-float("inf"), 0), (-0.5, 0), (1.5, 1)):
        assert run_kernel(hip, torch.full((1, 4, 5, 3), v, dtype=dtype), 8).tolist() == [5 * lit] * 4 + [4 * lit] * 5, v


def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    x = torch.rand(2, 6, 8, 4, device="cuda")
    out = guarded((14,), torch.int32)
    cases = [
        (lambda: hip.active_profile(x.cpu(), 8, out=out.t), "frames must live on"),
        (lambda: hip.active_profile(x.half(), 8, out=out.t), "fp32 or bf16"),
        (lambda: hip.active_profile(x[..., :3], 8, out=out.t), "frames must be contiguous"),
        (lambda: hip.active_profile(x[:, :, ::2], 8, out=out.t[:10]), "frames must be contiguous"),
        (lambda: hip.active_profile(x[..., :2].contiguous(), 8, out=out.t), "C = 3 or 4"),
        (lambda: hip.active_profile(x, -1, out=out.t), "dark must be"),
        (lambda: hip.active_profile(x, 256, out=out.t), "dark must be"),
        (lambda: hip.active_profile(x, 8.0, out=out.t), "dark must be"),
        (lambda: hip.active_profile(x, 8, out=torch.empty(13, dtype=torch.int32, device="cuda")), "out must be"),
        (lambda: hip.active_profile(x, 8, out=torch.empty(2, 7, dtype=torch.int32, device="cuda")), "out must be"),
        (lambda: hip.active_profile(x, 8, out=torch.empty(14, dtype=torch.int64, device="cuda")), "out must be"),
        (lambda: hip.active_profile(x, 8, out=out.t.cpu()), "out must live on"),
        (lambda: hip.active_profile(torch.empty((1 << 16, 1 << 15, 1, 3), device="meta"), 8, out=out.t), r"T \* max\(H, W\)"),
    ]
    for call, word in cases:
        with pytest.raises(ValueError, match=word):
            call()
    # the C entry point itself, device pointers: the message names the argument
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = hip.lib
    for args, word in (((p(x), 1, 2, 6, 8, 4, 8, p(out.t), 14 * 4 - 4, None), b"out_bytes"),
                       ((p(x), 1, 2, 6, 8, 4, 8, p(out.t), 15 * 4, None), b"out_bytes"),
                       ((p(x), 1, 2, 0, 8, 4, 8, p(out.t), 8 * 4, None), b"H must"),
                       ((p(x), 1, 2, 6, 0, 4, 8, p(out.t), 6 * 4, None), b"W must"),
                       ((p(x), 1, 0, 6, 8, 4, 8, p(out.t), 14 * 4, None), b"T >= 1"),
                       ((p(x), 1, 2, 6, 8, 5, 8, p(out.t), 14 * 4, None), b"C must"),
                       ((p(x), 2, 2, 6, 8, 4, 8, p(out.t), 14 * 4, None), b"kind"),
                       ((p(x), 1, 2, 6, 8, 4, 256, p(out.t), 14 * 4, None), b"dark"),
                       ((p(x), 1, 2, 6, 8, 4, -1, p(out.t), 14 * 4, None), b"dark"),
                       ((None, 1, 2, 6, 8, 4, 8, p(out.t), 14 * 4, None), b"frames"),
                       ((p(x), 1, 2, 6, 8, 4, 8, None, 14 * 4, None), b"out is"),
                       ((p(x), 1, 1 << 16, 6, 1 << 15, 4, 8, p(out.t), (6 + (1 << 15)) * 4, None), b"T * max(H, W)"),
                       ((p(x), 1, 1 << 16, 1 << 15, 8, 4, 8, p(out.t), (8 + (1 << 15)) * 4, None), b"T * max(H, W)")):
        assert L.svr_active_profile(*args) != 0
        assert word in L.svr_last_error() and b"svr_active_profile" in L.svr_last_error(), (word, L.svr_last_error())
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was enqueued: the payload is untouched


def test_letterboxed_clip_through_upscale_on_the_device(hip):
    """upscale(area=Rule) on the kernels is the composition of the device's own upscale(crop, target_size=...) and the canvas, same
    bits (the kernels are deterministic); the same through upscale_stream."""
    from test_active import canvas_of, letterboxed
    from test_stream import tiny_runner
    pipeline, active = sub("pipeline"), sub("active")
    runner, text = tiny_runner(hip, vae_channels=(128, 128, 128, 128)), sub("weights").synth_text_embedding().cuda()
    frames = letterboxed(channels=3).cuda()
    kw = dict(resolution=48, batch_size=5, color_correction="wavelet", temporal_overlap=1, prepend_frames=1)
    rule = active.Rule(**PARAMS)
    assert rule.area(hip.active_profile(frames, 8).tolist(), 6, 32, 40) == (4, 28, 0, 40)
    got = pipeline.upscale(frames, runner, text, area=rule, **kw)
    want = canvas_of(frames)
    want[:, 6:42] = pipeline.upscale(frames[:, 4:28].contiguous(), runner, text, target_size=(36, 60), **kw)
    assert got.shape == want.shape == (6, 48, 60, 3) and torch.equal(got, want)
    parts = list(pipeline.upscale_stream(iter([frames[:5], frames[5:]]), runner, text, area=rule, **kw))
    ctx = canvas_of(frames[4:6])
    ctx[:, 6:42] = pipeline.upscale(frames[4:6, 4:28].contiguous(), runner, text, target_size=(36, 60), **{**kw, "prepend_frames": 0})
    assert torch.equal(parts[0], pipeline.upscale(frames[:5], runner, text, area=rule, **kw))
    assert torch.equal(parts[0][:, 6:42], pipeline.upscale(frames[:5, 4:28].contiguous(), runner, text, target_size=(36, 60), **kw))
    assert torch.equal(parts[1], ctx[1:])
