"""-m gpu: csrc/svr_deinterlace.hip through HipOps.deinterlace against its specification deinterlace.deinterlace_torch -- EQUAL, every
format and channel count, both orders, both rates, every kind of context (integers in, integers out: a mismatch is a finding, not a
tolerance) --, the alignment routes, its refusals, and the command line's FrameSource(fields=...) feeding pipeline.upscale_stream on
the device.

Outputs live in tests/guarded_out.py buffers and the guards must stay intact.  The payload's poison is the byte 0xA5, which a
result can equal: the left-over check is made on clips whose samples all lie BELOW 0xA5 (0xA5A5 for the 16-bit formats) -- every
result lies between the smallest and the largest input, so no result is the poison there."""
import importlib.util
import os
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from deinterlace_cases import CONTEXTS, FORMATS, SHAPES, channel_counts, context, random_packed
from frame_unpack_cases import fake_video, stand_ins
from guarded_out import guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def dev(t):
    return None if t is None else t.cuda()


def run_kernel(hip, packed, fmt, T, H, W, C, order, rate, before=None, after=None, written=False):
    n_out = T * (2 if rate == "field" else 1)
    g = guarded((n_out,) + tuple(packed.shape[1:]), packed.dtype)
    out = hip.deinterlace(packed.cuda(), fmt, T, H, W, C, order, rate, before=dev(before), after=dev(after), out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    name = f"deinterlace {fmt} {(T, H, W, C)} {order} {rate}"
    g.assert_guards(name)
    if written:
        g.assert_written(name)
    return out.cpu()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(hip, shape, fmt):
    de = sub("deinterlace")
    T, H, W = shape
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        for n, kind in enumerate(CONTEXTS):
            before, after = context(kind, fmt, H, W, C, seed=n)
            for order in de.ORDERS:
                for rate in de.RATES:
                    want = de.deinterlace_torch(packed, fmt, T, H, W, C, order, rate, before, after)
                    got = run_kernel(hip, packed, fmt, T, H, W, C, order, rate, before, after)
                    assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), \
                        (C, kind, order, rate, int((got.to(torch.int32) != want.to(torch.int32)).sum()))


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_output_sample_is_written(hip, fmt):
    """Samples below the poison pattern: no result can equal it, so a sample that still holds it was never stored.  (2, 5, 32): the
    vector route for the luma plane and the RGB formats, the element route for the 8-bit chroma planes; (3, 17, 33): the element
    route everywhere."""
    de = sub("deinterlace")
    for T, H, W in ((2, 5, 32), (3, 17, 33)):
        C = channel_counts(fmt)[-1]
        packed = random_packed(fmt, T, H, W, C, seed=9)
        packed = (packed.to(torch.int64) % (0xA5 if packed.dtype == torch.uint8 else 0x3FF)).to(packed.dtype)
        for rate in de.RATES:
            want = de.deinterlace_torch(packed, fmt, T, H, W, C, "bff", rate)
            assert torch.equal(run_kernel(hip, packed, fmt, T, H, W, C, "bff", rate, written=True), want), (fmt, rate)


def test_output_allocated_by_the_op_and_unaligned_views(hip):
    """Without ``out`` the op allocates; a packed view, a context frame or an output that starts 2 or 4 bytes into an allocation
    takes the element route and gives the same bits."""
    de = sub("deinterlace")
    T, H, W = 3, 6, 32
    for fmt in FORMATS:
        C = 3
        packed = random_packed(fmt, T, H, W, C, seed=4)
        before, after = context("both", fmt, H, W, C, seed=5)
        want = de.deinterlace_torch(packed, fmt, T, H, W, C, "tff", "field", before, after)
        got = hip.deinterlace(packed.cuda(), fmt, T, H, W, C, "tff", "field", before=before.cuda(), after=after.cuda())
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want), fmt
        size = packed.element_size()

        def shifted(t, off):
            store = torch.empty(t.numel() + off // size, dtype=t.dtype, device="cuda")
            view = store[off // size:].view(t.shape)
            view.copy_(t)
            assert view.is_contiguous() and view.data_ptr() % 16 == off
            return view

        for off in (2, 4):
            for which in ("packed", "before", "after"):
                ops = dict(packed=packed.cuda(), before=before.cuda(), after=after.cuda())
                ops[which] = shifted(ops[which], off)
                g = guarded(want.shape, want.dtype)
                hip.deinterlace(ops["packed"], fmt, T, H, W, C, "tff", "field", before=ops["before"], after=ops["after"], out=g.t)
                torch.cuda.synchronize()
                g.assert_guards(fmt)
                assert torch.equal(g.t.cpu(), want), (fmt, off, which)
            # the output off 16 bytes: a view ``off`` bytes into a guarded payload
            g = guarded((want.numel() + off // size,), want.dtype)
            out = g.t[off // size:].view(want.shape)
            hip.deinterlace(packed.cuda(), fmt, T, H, W, C, "tff", "field", before=before.cuda(), after=after.cuda(), out=out)
            torch.cuda.synchronize()
            g.assert_guards(fmt)
            assert torch.equal(out.cpu(), want) and bool(g.poisoned()[:off // size].all()), (fmt, off)


def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    hip_lib = sub("hip_lib")
    packed = random_packed("rgb8", 2, 6, 8, 4, seed=0).cuda()
    planes = random_packed("yuv420p10", 2, 6, 8, 3, seed=0).cuda()
    frame = packed[0].clone()
    out = guarded((4, 6, 8, 4), torch.uint8)
    call = lambda *a, **kw: hip.deinterlace(*a, **{"out": out.t, **kw})
    with pytest.raises(ValueError, match="deinterlace: .*C = 3"):
        call(planes, "yuv420p10", 2, 6, 8, 4, "tff", "field")
    with pytest.raises(ValueError, match="deinterlace: fmt"):
        call(packed, "rgb10", 2, 6, 8, 4, "tff", "field")
    with pytest.raises(ValueError, match="deinterlace: order"):
        call(packed, "rgb8", 2, 6, 8, 4, "top", "field")
    with pytest.raises(ValueError, match="deinterlace: rate"):
        call(packed, "rgb8", 2, 6, 8, 4, "tff", "double")
    with pytest.raises(ValueError, match="packed must be torch.uint16"):
        call(packed, "rgb16", 2, 6, 8, 4, "tff", "field")
    with pytest.raises(ValueError, match="packed must hold"):
        call(packed, "rgb8", 2, 6, 9, 4, "tff", "field")
    with pytest.raises(ValueError, match="before must hold"):
        call(packed, "rgb8", 2, 6, 8, 4, "tff", "field", before=packed)
    with pytest.raises(ValueError, match="after must be torch.uint8"):
        call(packed, "rgb8", 2, 6, 8, 4, "tff", "field", after=frame.to(torch.int16))
    with pytest.raises(ValueError, match="packed must be contiguous"):
        call(torch.cat([packed, packed], dim=3)[..., ::2], "rgb8", 2, 6, 8, 4, "tff", "field")
    with pytest.raises(ValueError, match="after must be contiguous"):
        call(packed, "rgb8", 2, 6, 8, 4, "tff", "field", after=torch.cat([frame, frame], dim=2)[..., ::2])
    with pytest.raises(ValueError, match="packed must live on"):
        call(packed.cpu(), "rgb8", 2, 6, 8, 4, "tff", "field")
    with pytest.raises(ValueError, match="before must live on"):
        call(packed, "rgb8", 2, 6, 8, 4, "tff", "field", before=frame.cpu())
    with pytest.raises(ValueError, match="out must be"):
        call(packed, "rgb8", 2, 6, 8, 4, "tff", "frame")                                   # (out holds 4 frames, the rate gives 2)
    with pytest.raises(ValueError, match="out must be"):
        hip.deinterlace(packed, "rgb8", 2, 6, 8, 4, "tff", "field", out=torch.empty(4, 6, 8, 4, dtype=torch.int16, device="cuda"))
    # the C entry point itself, device pointers: wrong byte counts, C = 4 for the planes, unknown ids, an output over an input
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = hip.lib
    n = 2 * 6 * 8 * 4
    for nin, nout, word in ((n - 1, 2 * n, b"packed_bytes is 383, the format needs exactly 384"),
                            (n, n, b"out_bytes is 384, the format and rate need exactly 768"), (n, 2 * n + 1, b"out_bytes")):
        assert L.svr_deinterlace(p(packed), nin, None, None, 0, 2, 6, 8, 4, 0, 1, p(out.t), nout, None) != 0
        assert word in L.svr_last_error(), L.svr_last_error()
    assert L.svr_deinterlace(p(planes), 2 * 2 * (48 + 24), None, None, 2, 2, 6, 8, 4, 0, 1, p(out.t), 2 * n, None) != 0
    assert b"C must be 3" in L.svr_last_error()
    with pytest.raises(hip_lib.HipLibraryError, match="order must be"):
        hip_lib.check(L.svr_deinterlace(p(packed), n, None, None, 0, 2, 6, 8, 4, 2, 1, p(out.t), 2 * n, None), "svr_deinterlace")
    with pytest.raises(hip_lib.HipLibraryError, match="rate must be"):
        hip_lib.check(L.svr_deinterlace(p(packed), n, None, None, 0, 2, 6, 8, 4, 0, 2, p(out.t), 2 * n, None), "svr_deinterlace")
    # an output that overlaps the clip, through HipOps and through the entry point: the payload holds the clip itself, then
    store = guarded((3 * n,), torch.uint8)
    store.t[:n].copy_(packed.reshape(-1))
    inside = store.t[:n].view(2, 6, 8, 4)
    kept = store.t.clone()
    with pytest.raises(hip_lib.HipLibraryError, match="out overlaps packed"):
        hip.deinterlace(inside, "rgb8", 2, 6, 8, 4, "tff", "field", out=store.t[n - 16:3 * n - 16].view(4, 6, 8, 4))
    with pytest.raises(hip_lib.HipLibraryError, match="out overlaps before"):
        hip.deinterlace(packed, "rgb8", 2, 6, 8, 4, "tff", "field", before=store.t[:n // 2].view(6, 8, 4), out=store.t[:2 * n].view(4, 6, 8, 4))
    assert L.svr_deinterlace(p(packed), n, None, p(store.t[2 * n:]), 0, 2, 6, 8, 4, 0, 1, p(store.t[n:]), 2 * n, None) != 0
    assert b"out overlaps after" in L.svr_last_error()
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    store.assert_guards("refused calls")
    assert bool(out.poisoned().all()) and torch.equal(store.t, kept)                   # nothing was launched: the payloads are untouched


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_frame_source_deinterlaces_on_the_device_and_feeds_the_stream(hip, tmp_path):
    """A stand-in ffmpeg emits 13 yuv420p10 frames of 16 x 20; FrameSource(fields=("tff", "field")) in chunks of 5 gives 10, 10 and
    6 frames that equal the specification applied to the whole clip, bit for bit, and pipeline.upscale_stream fed by it equals
    upscale_stream fed the specification's frames; the reader's two host buffers are pinned."""
    from test_stream import tiny_runner
    fin, de, pipeline = sub("frameio_in"), sub("deinterlace"), sub("pipeline")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_fields", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    runner, text = tiny_runner(hip, vae_channels=(128, 128, 128, 128)), sub("weights").synth_text_embedding().cuda()
    kw = dict(resolution=32, batch_size=5, color_correction="wavelet", temporal_overlap=2, prepend_frames=1)
    ffprobe, ffmpeg = stand_ins(str(tmp_path / "bin"))
    packed = random_packed("yuv420p10", 13, 16, 20, 3, seed=7)
    clip = tmp_path / "clip.mkv"
    fake_video(clip, packed, "yuv420p10le", 20, 16, rate="25/1", color_space="bt709", color_range="tv")
    info = cli.probe_video(ffprobe, str(clip))
    src = cli.FrameSource(ffmpeg, str(clip), info, 5, ops=hip, device="cuda:0", fields=("tff", "field"))
    assert len(src.buffers) == 2 and all(b.is_pinned() for b in src.buffers) and src.fps == Fraction(50)
    seen = []

    def chunks():
        for c in src.chunks():
            assert c.is_cuda and c.dtype == torch.float32
            seen.append(c.cpu())
            yield c

    got = [o.cpu() for o in pipeline.upscale_stream(chunks(), runner, text, **kw)]
    frames = fin.unpack_frames_torch(de.deinterlace_torch(packed, "yuv420p10", 13, 16, 20, 3, "tff", "field"), "yuv420p10", 26, 16, 20, 3,
                                     "bt709", "tv")
    assert [c.shape[0] for c in seen] == [10, 10, 6] and torch.equal(torch.cat(seen), frames)
    want = [o.cpu() for o in pipeline.upscale_stream((frames[i:i + 10].cuda() for i in range(0, 26, 10)), runner, text, **kw)]
    assert len(got) == len(want) == 3
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), k
    assert not src.thread.is_alive()
