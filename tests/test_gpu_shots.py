"""-m gpu: csrc/svr_shots.hip through HipOps.frame_signatures against its specification shots.signatures_torch -- EQUAL, fp32 and bf16
input (integer counts: a mismatch is a finding, not a tolerance) --, its refusals, and pipeline.upscale_shots on the device.

Outputs live in tests/guarded_out.py buffers, pre-filled with garbage (the 0xA5 bytes of the payload: -1515870811 per counter), and
the guards must stay intact: the call itself has to bring the signature to zero before it counts."""
import pytest
import torch

from conftest import sub
from guarded_out import guarded
from shot_clips import assert_precondition, shot_clip

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
# (T, H, W, C): the smallest shapes at which the geometry can go wrong
SHAPES = [
    (2, 4, 4, 4),        # one pixel per cell, alpha ignored
    (3, 19, 23, 3),      # ragged cells
    (1, 130, 7, 4),      # rows outnumber a lane's columns; three bands of 16 rows per cell row, the last of one row
    (2, 64, 260, 3),     # a row wider than one pass of a workgroup
]
# beyond the issue's list: a band of more than 256 units of 8 pixels (the unit loop goes round), frames that start off 8 pixels
EXTRA_SHAPES = [(2, 36, 300, 3), (3, 5, 5, 3)]


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def clip(T, H, W, C, seed):
    """random values in [-0.1, 1.1] with the rounding ties (k + 0.5) / 255 scattered in"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(T, H, W, C, generator=g) * 1.2 - 0.1
    flat = x.view(-1)
    k8 = torch.randint(0, 255, (flat.numel(),), generator=g).double()
    flat[:] = torch.where(torch.rand(flat.numel(), generator=g) < 0.2, ((k8 + 0.5) / 255).float(), flat)
    return x


def run_kernel(hip, x):
    g = guarded((x.shape[0], 1024), torch.int32)
    assert bool(g.poisoned().all())                                            # garbage in: every counter starts at 0xA5A5A5A5
    out = hip.frame_signatures(x.cuda(), out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"frame_signatures {tuple(x.shape)} {x.dtype}")
    return out.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + EXTRA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, dtype):
    shots = sub("shots")
    x = clip(*shape, seed=sum(shape)).to(dtype)
    want = shots.signatures_torch(x)
    got = run_kernel(hip, x)
    assert got.dtype == torch.int32 and torch.equal(got, want), int((got != want).sum())
    assert got.sum(dim=1).tolist() == [shape[1] * shape[2]] * shape[0]
    assert torch.equal(run_kernel(hip, x), got)                                # two calls: the same bits
    # frames 4 bytes into an allocation: the element-wise route gives the same counts
    store = torch.empty(x.numel() + 2, dtype=dtype, device="cuda")
    shifted = store[4 // x.element_size():][:x.numel()].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    assert torch.equal(hip.frame_signatures(shifted).cpu(), want)
    assert torch.equal(shots.signatures(x.cuda(), hip).cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_flat_frames_put_one_bin_per_cell_at_the_cells_pixel_count(hip, dtype):
    """Every lane on one counter: the contention case.  Black, a grey and white; 64 x 260 (whole bands through the 16-byte route)
    and 19 x 23 (ragged cells)."""
    for H, W in ((64, 260), (19, 23)):
        values = torch.tensor([0.0, 0.5, 1.0])
        x = values.view(3, 1, 1, 1).expand(3, H, W, 3).contiguous().to(dtype)
        got = run_kernel(hip, x).view(3, 4, 4, 64)
        rows = torch.tensor([sum(1 for y in range(H) if (y * 4) // H == r) for r in range(4)])
        cols = torch.tensor([sum(1 for c in range(W) if (c * 4) // W == k) for k in range(4)])
        for t, b in enumerate((0, 128 >> 2, 63)):                              # 0.5 * 255 = 127.5 -> 128 (ties to even)
            want = torch.zeros(4, 4, 64, dtype=torch.int32)
            want[:, :, b] = (rows[:, None] * cols[None, :]).to(torch.int32)
            assert torch.equal(got[t], want), (H, W, t)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_non_finite_negative_and_large_values(hip, dtype):
    shots = sub("shots")
    x = clip(1, 64, 260, 3, seed=9)
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.5, 1.5, -0.0])
    where = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(10))[:3000]
    x.view(-1)[where] = specials[torch.arange(3000) % 6]
    x = x.to(dtype)
    for src in (x, x[:, :19, :23].contiguous()):
        assert torch.equal(run_kernel(hip, src), shots.signatures_torch(src))
    for v, b in ((float("nan"), 0), (float("inf"), 63), (-float("inf"), 0), (-0.5, 0), (1.5, 63)):
        got = run_kernel(hip, torch.full((1, 4, 4, 3), v, dtype=dtype)).view(16, 64)
        assert got[:, b].tolist() == [1] * 16 and int(got.sum()) == 16, v


def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    x = torch.rand(2, 6, 8, 4, device="cuda")
    out = guarded((2, 1024), torch.int32)
    cases = [
        (lambda: hip.frame_signatures(x.cpu(), out=out.t), "frames must live on"),
        (lambda: hip.frame_signatures(x.half(), out=out.t), "fp32 or bf16"),
        (lambda: hip.frame_signatures(x[:, :3].contiguous(), out=out.t[:2]), "H >= 4"),
        (lambda: hip.frame_signatures(x[..., :3], out=out.t), "frames must be contiguous"),
        (lambda: hip.frame_signatures(x[:, ::2], out=out.t), "H >= 4|contiguous"),
        (lambda: hip.frame_signatures(x[:, :, ::2], out=out.t), "frames must be contiguous"),
        (lambda: hip.frame_signatures(x, out=torch.empty(2, 1023, dtype=torch.int32, device="cuda")), "out must be"),
        (lambda: hip.frame_signatures(x, out=torch.empty(3, 1024, dtype=torch.int32, device="cuda")), "out must be"),
        (lambda: hip.frame_signatures(x, out=torch.empty(2, 1024, dtype=torch.int64, device="cuda")), "out must be"),
        (lambda: hip.frame_signatures(x, out=out.t.cpu()), "out must live on"),
    ]
    for call, word in cases:
        with pytest.raises(ValueError, match=word):
            call()
    # the C entry point itself, device pointers: the message names the argument
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = hip.lib
    for args, word in (((p(x), 1, 2, 6, 8, 4, p(out.t), 2 * 4096 - 4, None), b"sig_bytes"),
                       ((p(x), 1, 2, 6, 8, 4, p(out.t), 4096, None), b"sig_bytes"),
                       ((p(x), 1, 2, 3, 16, 4, p(out.t), 2 * 4096, None), b"H must"),
                       ((p(x), 1, 2, 16, 3, 4, p(out.t), 2 * 4096, None), b"W must"),
                       ((p(x), 1, 0, 6, 8, 4, p(out.t), 0, None), b"T >= 1"),
                       ((p(x), 1, 2, 6, 8, 5, p(out.t), 2 * 4096, None), b"C must"),
                       ((p(x), 2, 2, 6, 8, 4, p(out.t), 2 * 4096, None), b"kind"),
                       ((None, 1, 2, 6, 8, 4, p(out.t), 2 * 4096, None), b"frames"),
                       ((p(x), 1, 2, 6, 8, 4, None, 2 * 4096, None), b"sig is"),
                       ((p(x), 1, 2, 1 << 16, 1 << 15, 4, p(out.t), 2 * 4096, None), b"H * W")):
        assert L.svr_frame_signatures(*args) != 0
        assert word in L.svr_last_error() and b"svr_frame_signatures" in L.svr_last_error(), (word, L.svr_last_error())
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was enqueued: the payload is untouched


def test_two_shot_clip_through_upscale_shots_on_the_device(hip):
    """A two-shot clip through pipeline.upscale_shots with a detector, on the kernels: the per-shot pipeline.upscale calls, same bits
    (the kernels are deterministic); the precondition is asserted with the torch statement on the device."""
    from test_stream import tiny_runner
    pipeline, shots = sub("pipeline"), sub("shots")
    runner, text = tiny_runner(hip, vae_channels=(128, 128, 128, 128)), sub("weights").synth_text_embedding().cuda()
    frames = shot_clip(24, 40, [6, 5], seed=11).cuda()                         # (the frame size of the pipeline goldens)
    assert_precondition(shots, frames, [6])
    kw = dict(resolution=48, batch_size=5, color_correction="wavelet", temporal_overlap=1, prepend_frames=1)
    det = shots.Detector(percent=30, ratio=3, window=8, min_shot=3)
    got = pipeline.upscale_shots(frames, runner, text, cuts=det, **kw)
    want = torch.cat([pipeline.upscale(frames[a:b], runner, text, **kw) for a, b in ((0, 6), (6, 11))])
    assert det.count == 11 and got.shape == want.shape and got.shape[0] == 11 and torch.equal(got, want)
    # the same through the stream, the cut inside the second chunk
    det = shots.Detector(percent=30, ratio=3, window=8, min_shot=3)
    parts = list(pipeline.upscale_stream(iter([frames[:5], frames[5:]]), runner, text, cuts=det, **kw))
    ctx = pipeline.upscale(frames[4:6], runner, text, **{**kw, "prepend_frames": 0})[1:]
    assert torch.equal(parts[0], pipeline.upscale(frames[:5], runner, text, **kw))
    assert torch.equal(parts[1], torch.cat([ctx, want[6:]]))
