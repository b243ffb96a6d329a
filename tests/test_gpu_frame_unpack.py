"""-m gpu: csrc/svr_frame_unpack.hip through HipOps.unpack_frames against its specification frameio_in.unpack_frames_torch -- EQUAL,
every format, both matrices, both ranges (every result is an integer code over a full scale and ONE fp32 division: a mismatch is a
finding, not a tolerance) --, every rgb code on the device, unaligned views, its refusals, and the command line's FrameSource feeding
pipeline.upscale_stream on the device.

Outputs live in tests/guarded_out.py buffers: the guards must stay intact and NO poison may be left -- the output is fp32 and the
poison a NaN pattern no division produces, so unlike the pack's integer payload the left-over check means something here."""
import importlib.util
import os
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from frame_unpack_cases import SHAPES, YUV, channel_counts, fake_video, random_packed, stand_ins
from guarded_out import guarded

pytestmark = pytest.mark.gpu
FORMATS = ("rgb8", "bgr8", "rgb16", "yuv420p8", "yuv420p10")


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def settings(fmt):
    """(matrix, range_) pairs a format distinguishes"""
    return [(m, r) for m in ("bt709", "bt601") for r in ("tv", "pc")] if fmt in YUV else [("bt709", "tv")]


def run_kernel(hip, packed, fmt, T, H, W, C, matrix, range_):
    g = guarded((T, H, W, C), torch.float32)
    out = hip.unpack_frames(packed.cuda(), fmt, T, H, W, C, matrix, range_, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    name = f"unpack_frames {fmt} {(T, H, W, C)} {matrix} {range_}"
    g.assert_guards(name)
    g.assert_written(name)
    return out.cpu()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, fmt):
    fin = sub("frameio_in")
    T, H, W = shape
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        for matrix, range_ in settings(fmt):
            want = fin.unpack_frames_torch(packed, fmt, T, H, W, C, matrix, range_)
            got = run_kernel(hip, packed, fmt, T, H, W, C, matrix, range_)
            assert got.shape == want.shape and torch.equal(got, want), (C, matrix, range_, int((got != want).sum()))


def test_every_rgb_code_on_the_device(hip):
    """All 65 536 rgb16 codes and all 256 rgb8 codes in one 256 x 256 frame each, against the CPU specification (which
    tests/test_frame_unpack.py holds against exact fractions): the device's fp32 division is the nearest value for every code."""
    fin = sub("frameio_in")
    q = torch.arange(65536, dtype=torch.int64)
    wide = q.to(torch.uint16).reshape(1, 256, 256, 1).expand(1, 256, 256, 3).contiguous()
    assert torch.equal(run_kernel(hip, wide, "rgb16", 1, 256, 256, 3, "bt709", "tv"), fin.unpack_frames_torch(wide, "rgb16", 1, 256, 256, 3))
    narrow = (q % 256).to(torch.uint8).reshape(1, 256, 256, 1).expand(1, 256, 256, 4).contiguous()
    for fmt in ("rgb8", "bgr8"):
        assert torch.equal(run_kernel(hip, narrow, fmt, 1, 256, 256, 4, "bt709", "tv"), fin.unpack_frames_torch(narrow, fmt, 1, 256, 256, 4))
    # 10-bit samples the container can hold and no decoder writes: they count as 1023
    wild = random_packed("rgb16", 2, 6, 16, 3, seed=1).reshape(2, -1)[:, :6 * 16 + 2 * 3 * 8].contiguous()
    assert torch.equal(run_kernel(hip, wild, "yuv420p10", 2, 6, 16, 3, "bt709", "tv"), fin.unpack_frames_torch(wild, "yuv420p10", 2, 6, 16, 3))


def test_output_allocated_by_the_op_and_an_unaligned_view(hip):
    """Without ``out`` the op allocates; a packed view that starts 2 or 4 bytes into an allocation takes the element route and gives
    the same values, and so does an output 4 bytes off (the vector kernels need both ends on 16 bytes)."""
    fin = sub("frameio_in")
    T, H, W = 2, 6, 16
    for fmt in FORMATS:
        C = 3
        packed = random_packed(fmt, T, H, W, C, seed=4)
        for matrix, range_ in settings(fmt)[:1] + settings(fmt)[-1:]:
            want = fin.unpack_frames_torch(packed, fmt, T, H, W, C, matrix, range_)
            assert torch.equal(hip.unpack_frames(packed.cuda(), fmt, T, H, W, C, matrix, range_).cpu(), want), fmt
            size = packed.element_size()
            for off in (2, 4):
                store = torch.empty(packed.numel() + off // size, dtype=packed.dtype, device="cuda")
                shifted = store[off // size:].view(packed.shape)
                shifted.copy_(packed)
                assert shifted.is_contiguous() and shifted.data_ptr() % 16 == off
                g = guarded((T, H, W, C), torch.float32)
                hip.unpack_frames(shifted, fmt, T, H, W, C, matrix, range_, out=g.t)
                torch.cuda.synchronize()
                g.assert_guards(fmt)
                g.assert_written(fmt)
                assert torch.equal(g.t.cpu(), want), (fmt, off)
            # the output off 16 bytes: a view one element into a guarded payload
            g = guarded((T * H * W * C + 1,), torch.float32)
            out = g.t[1:].view(T, H, W, C)
            hip.unpack_frames(packed.cuda(), fmt, T, H, W, C, matrix, range_, out=out)
            torch.cuda.synchronize()
            g.assert_guards(fmt)
            assert torch.equal(out.cpu(), want) and bool(g.poisoned()[0]) and not bool(g.poisoned()[1:].any()), fmt


def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    hip_lib = sub("hip_lib")
    packed = random_packed("rgb8", 2, 6, 8, 4, seed=0).cuda()
    planes = random_packed("yuv420p10", 2, 6, 8, 3, seed=0).cuda()
    out = guarded((2, 6, 8, 4), torch.float32)
    with pytest.raises(ValueError, match="C = 3"):
        hip.unpack_frames(planes, "yuv420p10", 2, 6, 8, 4, out=out.t)
    with pytest.raises(ValueError, match="fmt"):
        hip.unpack_frames(packed, "rgb10", 2, 6, 8, 4, out=out.t)
    with pytest.raises(ValueError, match="matrix"):
        hip.unpack_frames(packed, "rgb8", 2, 6, 8, 4, matrix="bt2020", out=out.t)
    with pytest.raises(ValueError, match="range_"):
        hip.unpack_frames(packed, "rgb8", 2, 6, 8, 4, range_="full", out=out.t)
    with pytest.raises(ValueError, match="packed must be torch.uint16"):
        hip.unpack_frames(packed, "rgb16", 2, 6, 8, 4, out=out.t)
    with pytest.raises(ValueError, match="packed must hold"):
        hip.unpack_frames(packed, "rgb8", 2, 6, 9, 4, out=out.t)
    with pytest.raises(ValueError, match="packed must be contiguous"):
        hip.unpack_frames(torch.cat([packed, packed], dim=3)[..., ::2], "rgb8", 2, 6, 8, 4, out=out.t)
    with pytest.raises(ValueError, match="packed must live on"):
        hip.unpack_frames(packed.cpu(), "rgb8", 2, 6, 8, 4, out=out.t)
    with pytest.raises(ValueError, match="out must be"):
        hip.unpack_frames(packed[..., :3].contiguous(), "rgb8", 2, 6, 8, 3, out=out.t)
    with pytest.raises(ValueError, match="out must be"):
        hip.unpack_frames(packed, "rgb8", 2, 6, 8, 4, out=torch.empty(2, 6, 8, 4, dtype=torch.bfloat16, device="cuda"))
    # the C entry point itself, device pointers: wrong byte counts, C = 4 for the planes, an unknown matrix
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = hip.lib
    n = 2 * 6 * 8 * 4
    for nin, nout, word in ((n - 1, 4 * n, b"packed_bytes"), (n + 16, 4 * n, b"packed_bytes"), (n, 4 * n - 4, b"out_bytes"), (n, n, b"out_bytes")):
        assert L.svr_unpack_frames(p(packed), nin, 0, 2, 6, 8, 4, 0, 0, p(out.t), nout, None) != 0
        assert word in L.svr_last_error()
    assert L.svr_unpack_frames(p(planes), 2 * 2 * (48 + 24), 2, 2, 6, 8, 4, 0, 0, p(out.t), 4 * n, None) != 0
    assert b"C must be 3" in L.svr_last_error()
    with pytest.raises(hip_lib.HipLibraryError, match="matrix"):
        hip_lib.check(L.svr_unpack_frames(p(packed), n, 0, 2, 6, 8, 4, 7, 0, p(out.t), 4 * n, None), "svr_unpack_frames")
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was launched: the payload is untouched


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_frame_source_feeds_the_stream_on_the_device(hip, tmp_path):
    """A stand-in ffmpeg emits 13 yuv420p10 frames of 16 x 20; FrameSource in chunks of 5 (5, 5, 3) into pipeline.upscale_stream
    equals upscale_stream fed the specification's frames, bit for bit; the reader's two host buffers are pinned."""
    from test_stream import tiny_runner
    fin, pipeline = sub("frameio_in"), sub("pipeline")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_source", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    runner, text = tiny_runner(hip, vae_channels=(128, 128, 128, 128)), sub("weights").synth_text_embedding().cuda()
    kw = dict(resolution=32, batch_size=5, color_correction="wavelet", temporal_overlap=2, prepend_frames=1)
    ffprobe, ffmpeg = stand_ins(str(tmp_path / "bin"))
    packed = random_packed("yuv420p10", 13, 16, 20, 3, seed=7)
    clip = tmp_path / "clip.mkv"
    fake_video(clip, packed, "yuv420p10le", 20, 16, rate="25/1", color_space="bt709", color_range="tv")
    info = cli.probe_video(ffprobe, str(clip))
    assert info["fps"] == Fraction(25) and cli.route_input(info) == ("yuv420p10le", "yuv420p10", 3, "bt709", "tv")
    src = cli.FrameSource(ffmpeg, str(clip), info, 5, ops=hip, device="cuda:0")
    assert len(src.buffers) == 2 and all(b.is_pinned() for b in src.buffers)
    seen = []

    def chunks():
        for c in src.chunks():
            assert c.is_cuda and c.dtype == torch.float32
            seen.append(c.cpu())
            yield c

    got = [o.cpu() for o in pipeline.upscale_stream(chunks(), runner, text, **kw)]
    frames = fin.unpack_frames_torch(packed, "yuv420p10", 13, 16, 20, 3, "bt709", "tv")
    assert [c.shape[0] for c in seen] == [5, 5, 3] and torch.equal(torch.cat(seen), frames)
    want = [o.cpu() for o in pipeline.upscale_stream((frames[i:i + 5].cuda() for i in range(0, 13, 5)), runner, text, **kw)]
    assert len(got) == len(want) == 3
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), k
    assert not src.thread.is_alive()
