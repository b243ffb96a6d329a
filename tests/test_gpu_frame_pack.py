"""-m gpu: csrc/svr_frame_pack.hip through HipOps.pack_frames against its specification frameio.pack_frames_torch -- EQUAL, every
format, fp32 and bf16 input (integer results: a mismatch is a finding, not a tolerance) --, its refusals, and pipeline.upscale_stream
on the device: bit-equal to the per-chunk calls, device memory bounded by one chunk.

Outputs live in tests/guarded_out.py buffers and the guards must stay intact.  The uint8 / uint16 payloads are written everywhere
but are not asked for left-over poison: the poison byte 0xA5 = 165 (0xA5A5 as a 10-bit plane value is out of range, but the check
would say nothing the comparison does not) is a legitimate code, as test_gpu_alpha.py notes for the edge map -- the comparison with
the specification is the check that every element was written, and the payload starts as 0xA5 bytes, never as a previous result."""
import pytest
import torch

from conftest import sub
from guarded_out import guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FORMATS = ("rgb8", "bgr8", "yuv420p10")
# [T, H, W]: the smallest shapes that reach every seam -- sample counts below one 16-byte vector (1,1,1: 3 samples; 1,1,5: 15) and
# off a multiple of 16 / 48, odd and even H and W (chroma rows / columns that repeat the last one), W a multiple of 8 and not, of
# 16 (the 16-byte yuv kernel: 1,16,64) and not (1,64,66), frame starts off 16 bytes (2,3,5: 45 bytes / 62 bytes per frame; 2,31,8).
SHAPES = [(1, 1, 1), (1, 1, 5), (2, 3, 5), (1, 2, 2), (1, 5, 4), (3, 17, 33), (1, 16, 64), (1, 64, 66), (2, 31, 8)]
# beyond the issue's list: the 16-byte yuv kernel with an odd H (its second row repeats the first) and several frames
EXTRA_SHAPES = [(2, 5, 32), (1, 1, 16)]


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


def run_kernel(hip, x, fmt):
    frameio = sub("frameio")
    T, H, W, C = x.shape
    g = guarded(frameio.packed_shape(T, H, W, C, fmt), frameio.packed_dtype(fmt))
    out = hip.pack_frames(x.cuda(), fmt, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"pack_frames {fmt} {tuple(x.shape)} {x.dtype}")
    return out.cpu()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.uint16 else a,
                                                                     b.view(torch.int16) if b.dtype == torch.uint16 else b)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + EXTRA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, dtype):
    frameio = sub("frameio")
    for C in (3, 4):
        x = clip(*shape, C, seed=sum(shape) + C).to(dtype)
        for fmt in FORMATS:
            if fmt == "yuv420p10" and C == 4:
                continue
            want = frameio.pack_frames_torch(x, fmt)
            got = run_kernel(hip, x, fmt)
            assert same(got, want), (fmt, C, int((got.to(torch.int32) != want.to(torch.int32)).sum()))


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_non_finite_and_negative_zero(hip, dtype):
    frameio = sub("frameio")
    x = clip(1, 16, 64, 3, seed=9)
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    g = torch.Generator().manual_seed(10)
    where = torch.randperm(x.numel(), generator=g)[:400]
    x.view(-1)[where] = specials[torch.arange(400) % 4]
    x = x.to(dtype)
    for src in (x, x[:, :5, :7].contiguous()):                                # the 16-byte kernels and the element-wise ones
        for fmt in FORMATS:
            assert same(run_kernel(hip, src, fmt), frameio.pack_frames_torch(src, fmt)), fmt
    one = specials[:3].reshape(1, 1, 1, 3).to(dtype)
    assert run_kernel(hip, one, "rgb8").flatten().tolist() == [0, 255, 0]
    assert run_kernel(hip, one, "yuv420p10").flatten().tolist() == [691, 167, 105]


# (Y, Cb, Cr) of the flat frames black, blue, green, cyan, red, magenta, yellow, white: BT.709, limited range
CORNER_CODES = [(64, 512, 512), (127, 960, 471), (691, 167, 105), (754, 615, 64), (250, 409, 960), (313, 857, 919), (877, 64, 553),
                (940, 512, 512)]


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_cube_corners_reach_the_chroma_extremes(hip, dtype):
    """Every pixel one of the eight corners of the RGB cube: chroma reaches 64 and 960, where the shared kernel's clamp at 1023 and
    its rounding constant S * 512 * D + S * D / 2 must give what the BT.709 statement's 2050 * D gives.  (1, 2, 16) and (2, 5, 32)
    take the 16-byte route, (1, 3, 5) and (1, 1, 1) the element-wise one."""
    frameio = sub("frameio")
    corners = torch.tensor([[r, g, b] for r in (0., 1.) for g in (0., 1.) for b in (0., 1.)])
    g = torch.Generator().manual_seed(31)
    for shape in [(1, 2, 16), (2, 5, 32), (1, 3, 5), (1, 1, 1)]:
        x = corners[torch.randint(0, 8, shape, generator=g)].to(dtype)
        assert same(run_kernel(hip, x, "yuv420p10"), frameio.pack_frames_torch(x, "yuv420p10")), shape
    flat = corners.view(8, 1, 1, 3).expand(8, 2, 2, 3).contiguous().to(dtype)
    got = run_kernel(hip, flat, "yuv420p10")                                   # per frame: 4 Y, 1 Cb, 1 Cr
    assert got.to(torch.int32).tolist() == [[y] * 4 + [cb, cr] for y, cb, cr in CORNER_CODES]


def test_output_allocated_by_the_op_and_an_unaligned_view(hip):
    """Without ``out`` the op allocates; frames that start 4 bytes into an allocation (a dense view: frames[1:] of a one-pixel
    first frame would be 12 bytes in) take the element-wise route and give the same bytes."""
    frameio = sub("frameio")
    x = clip(2, 6, 16, 3, seed=4)
    want = {fmt: frameio.pack_frames_torch(x, fmt) for fmt in FORMATS}
    store = torch.empty(x.numel() + 1, device="cuda")
    shifted = store[1:].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    for fmt in FORMATS:
        assert same(hip.pack_frames(x.cuda(), fmt).cpu(), want[fmt]), fmt
        assert same(hip.pack_frames(shifted, fmt).cpu(), want[fmt]), fmt


def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    hip_lib = sub("hip_lib")
    x = torch.rand(2, 6, 8, 4, device="cuda")
    out = guarded((2, 6, 8, 4), torch.uint8)
    with pytest.raises(ValueError, match="C = 3"):
        hip.pack_frames(x, "yuv420p10")
    with pytest.raises(ValueError, match="frames must be contiguous"):
        hip.pack_frames(x[..., :3], "rgb8")
    with pytest.raises(ValueError, match="frames must be contiguous"):
        hip.pack_frames(x[:, ::2], "rgb8")
    with pytest.raises(ValueError, match="out must be"):
        hip.pack_frames(x, "rgb8", out=torch.empty(2, 6, 8, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        hip.pack_frames(x, "rgb8", out=torch.empty(2, 6, 8, 4, dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError, match="frames must live on"):
        hip.pack_frames(x.cpu(), "rgb8")
    with pytest.raises(ValueError, match="fmt"):
        hip.pack_frames(x, "rgb10")
    # the C entry point itself: a wrong out_bytes and C = 4 for yuv420p10, device pointers, the message names the argument
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = hip.lib
    for nbytes in (2 * 6 * 8 * 4 - 1, 2 * 6 * 8 * 4 + 16, 2 * 6 * 8 * 3):
        assert L.svr_pack_frames(p(x), 1, 2, 6, 8, 4, 0, p(out.t), nbytes, None) != 0
        assert b"out_bytes" in L.svr_last_error()
    assert L.svr_pack_frames(p(x), 1, 2, 6, 8, 4, 2, p(out.t), 2 * 2 * (48 + 24), None) != 0
    assert b"C must be 3" in L.svr_last_error()
    with pytest.raises(hip_lib.HipLibraryError, match="out_bytes"):
        hip_lib.check(L.svr_pack_frames(p(x), 1, 2, 6, 8, 4, 1, p(out.t), 5, None), "svr_pack_frames")
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was launched: the payload is untouched


# ---------------------------------------------------------------------------------------------------------------- streaming
@pytest.fixture(scope="module")
def tiny(hip):
    from test_stream import tiny_runner
    return tiny_runner(hip, vae_channels=(128, 128, 128, 128)), sub("weights").synth_text_embedding().cuda()


KW = dict(resolution=32, batch_size=5, color_correction="wavelet")


def test_stream_equals_the_per_chunk_calls_bit_for_bit(hip, tiny):
    """13 frames of 16 x 20 in chunks of 5 with an overlap of 2: each yielded chunk is pipeline.upscale of (context + chunk) with the
    context trimmed, same bits (the kernels are deterministic), and packs to the specification's bytes."""
    pipeline, frameio = sub("pipeline"), sub("frameio")
    runner, text = tiny
    g = torch.Generator().manual_seed(5)
    frames = torch.rand(13, 16, 20, 3, generator=g).cuda()
    chunks = [frames[i:i + 5] for i in range(0, 13, 5)]
    got = list(pipeline.upscale_stream(iter(chunks), runner, text, temporal_overlap=2, prepend_frames=1, **KW))
    assert [o.shape[0] for o in got] == [5, 5, 3]
    for k, o in enumerate(got):
        ctx = 0 if k == 0 else 2
        whole = torch.cat([chunks[k - 1][-ctx:], chunks[k]]) if ctx else chunks[k]
        want = pipeline.upscale(whole, runner, text, temporal_overlap=2, prepend_frames=1 if k == 0 else 0, **KW)[ctx:]
        assert o.shape == want.shape and torch.equal(o, want), k
        for fmt in FORMATS:
            assert same(frameio.pack_frames(o.contiguous(), fmt, hip).cpu(), frameio.pack_frames_torch(o.cpu().contiguous(), fmt)), (k, fmt)


def test_stream_memory_does_not_grow_with_the_clip(hip, tiny):
    """Peak device memory over 30 frames in chunks of 5 against the same over 10 frames in chunks of 5, each yielded chunk packed
    and dropped: what the generator may keep between chunks is the raw input tail (``temporal_overlap`` frames, part of one input
    chunk), and the caching allocator may split blocks differently by less than that -- so the longer clip may exceed the shorter by
    at most the bytes of ONE input chunk (5 x 16 x 20 x 3 fp32 = 19 200).  A condition from what may be kept, not a measurement:
    one retained OUTPUT chunk (5 x 32 x 40 x 3 fp32 = 76 800 bytes) per chunk would exceed it at the first."""
    pipeline, frameio = sub("pipeline"), sub("frameio")
    runner, text = tiny
    g = torch.Generator().manual_seed(6)
    host = torch.rand(30, 16, 20, 3, generator=g)

    def peak(n):
        def chunks():
            for i in range(0, n, 5):
                yield host[i:i + 5].cuda()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        sizes = []
        for out in pipeline.upscale_stream(chunks(), runner, text, temporal_overlap=2, **KW):
            packed = frameio.pack_frames(out.contiguous(), "yuv420p10", hip)
            sizes.append(tuple(packed.shape))
            del out, packed
        torch.cuda.synchronize()
        assert len(sizes) == n // 5
        return torch.cuda.max_memory_allocated()

    peak(10)                                                                   # (first use: kernels loaded, allocator warm)
    short, long_ = peak(10), peak(30)
    one_input_chunk = 5 * 16 * 20 * 3 * 4
    print(f"peak over 10 frames {short} B, over 30 frames {long_} B, one input chunk {one_input_chunk} B")
    assert long_ <= short + one_input_chunk


def test_frame_sink_packs_device_frames_through_the_runners_backend(hip):
    """The command line's hand-over with frames on the GPU: packed by ``ops`` there, through the two pinned buffers, to the writer
    thread in order; without a backend device frames are refused, not converted some other way."""
    import importlib.util
    import os
    from conftest import ROOT
    frameio = sub("frameio")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_sink", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    seen = []

    class Keep:
        fmt, alpha = "yuv420p10", False

        def write(self, arr, height, width):
            seen.append((arr.copy(), height, width))

        def close(self):
            pass

    chunks = [clip(t, 6, 16, 3, seed=20 + t) for t in (3, 3, 1, 2)]
    sink = cli.FrameSink(Keep(), hip)
    for c in chunks:
        sink.put(c.cuda())
    sink.close()
    assert len(seen) == 4 and all(b.is_pinned() for b in sink.buffers)
    for c, (arr, h, w) in zip(chunks, seen):
        assert (h, w) == (6, 16) and same(torch.from_numpy(arr), frameio.pack_frames_torch(c, "yuv420p10"))
    sink = cli.FrameSink(Keep())
    with pytest.raises(ValueError, match="ops"):
        sink.put(chunks[0].cuda())
    sink.close()
