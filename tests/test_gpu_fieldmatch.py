"""-m gpu: csrc/svr_fieldmatch.hip through HipOps.comb_counts / HipOps.field_select against its specification fieldmatch.py -- EQUAL,
every format and channel count, both orders, every kind of context (integers in, integers out: a mismatch is a finding, not a
tolerance) --, crafted counts that force every mode and tie, the alignment routes, determinism, the refusals, and the command
line's FrameSource(fields=("tff", "match")) feeding pipeline.upscale_stream on the device.

Outputs live in tests/guarded_out.py buffers and the guards must stay intact.  The payload's poison is the byte 0xA5, which a
copied sample can equal: the left-over check is made on clips whose samples all lie BELOW 0xA5 (0xA5A5 for the 16-bit formats) --
every output sample is a stored sample or a deinterlaced one, which lies between the smallest and the largest input."""
import ctypes
import importlib.util
import os
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from fieldmatch_cases import (CONTEXTS, FORMATS, MI, ORDERS, SHAPES, THR, channel_counts, context, crafted_counts, interlace, packed_clip,
                              pictures, random_packed, telecine)
from frame_unpack_cases import fake_video, stand_ins
from guarded_out import guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def dev(t):
    return None if t is None else t.cuda()


def step(fmt, C):
    return 1 if fmt in ("yuv420p8", "yuv420p10") else C


def run_counts(hip, packed, fmt, T, H, W, C, order, thr, before=None, after=None):
    g = guarded((T, 3, 2), torch.int32)
    out = hip.comb_counts(packed.cuda(), fmt, T, H, W, C, order, thr, before=dev(before), after=dev(after), out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"comb_counts {fmt} {(T, H, W, C)} {order}")
    g.assert_written(f"comb_counts {fmt} {(T, H, W, C)} {order}")               # (the call zeroes every counter: no poison is left)
    return out.cpu()


def run_select(hip, packed, deint, cnt, fmt, T, H, W, C, order, mi, before=None, after=None, written=False, side=True):
    """-> (frames, modes, stats): modes / stats None where ``side`` is False (NULL pointers)"""
    g = guarded(tuple(packed.shape), packed.dtype)
    gm, gs = guarded((T,), torch.int32), guarded((6,), torch.int64, init=torch.tensor([5, 0, 7, 0, 11, 0], device="cuda"))
    out = hip.field_select(packed.cuda(), deint.cuda(), cnt.cuda(), fmt, T, H, W, C, order, mi, before=dev(before), after=dev(after),
                           out=g.t, modes=gm.t if side else None, stats=gs.t if side else None)
    torch.cuda.synchronize()
    assert out is g.t
    name = f"field_select {fmt} {(T, H, W, C)} {order}"
    for b in (g, gm, gs):
        b.assert_guards(name)
    if written:
        g.assert_written(name)
    if not side:
        assert bool(gm.poisoned().all()) and gs.t.tolist() == [5, 0, 7, 0, 11, 0]                     # untouched
        return out.cpu(), None, None
    gm.assert_written(name)
    return out.cpu(), gm.t.cpu(), gs.t.cpu() - torch.tensor([5, 0, 7, 0, 11, 0])                       # (stats is ADDED to)


def spec_stats(fm, modes, cnt):
    st = fm.Stats()
    st.add(modes, cnt)
    return st.counts


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_specification_on_random_clips(hip, shape, fmt):
    """Random samples: nearly every sample is combed at a small thr, so the peaks sit at a block's capacity.  The select kernel is fed
    the counts kernel's own output, with a bound that splits the peaks the clip has."""
    fm, de = sub("fieldmatch"), sub("deinterlace")
    T, H, W = shape
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        s = step(fmt, C)
        for n, kind in enumerate(CONTEXTS):
            before, after = context(kind, fmt, H, W, C, seed=n)
            for order in ORDERS:
                thr = (3, 90, 200, 40)[n]
                want = fm.comb_counts_torch(packed, fmt, T, H, W, C, order, thr, before, after)
                got = run_counts(hip, packed, fmt, T, H, W, C, order, thr, before, after)
                assert torch.equal(got, want), (C, kind, order, got.tolist(), want.tolist())
                mi = int(want[:, :, 1].max()) // (2 * s)
                modes = fm.modes_torch(want, mi, s)
                deint = de.deinterlace_torch(packed, fmt, T, H, W, C, order, "frame", before, after)
                frames, gm, gs = run_select(hip, packed, deint, got, fmt, T, H, W, C, order, mi, before, after)
                assert torch.equal(gm, modes) and torch.equal(gs, spec_stats(fm, modes, want)), (C, kind, order)
                assert torch.equal(frames, fm.select_torch(packed, deint, modes, fmt, T, H, W, C, order, before, after)), (C, kind, order)


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernels_equal_the_specification_on_the_builders_clips(hip, fmt):
    """Sparse counts: a telecined clip followed by an interlaced one at the property geometry, the test's own thr / mi; the whole
    front through HipOps equals the specification, modes and stats included."""
    fm = sub("fieldmatch")
    for (R, N, speed), order in (((18, 40, 2), "tff"), ((34, 70, 3), "bff")):
        P = pictures(14, R, N, speed, seed=3)
        clip = torch.cat([packed_clip(P[:8], fmt, lambda pl: telecine(pl, order)[0]), packed_clip(P[8:], fmt, lambda pl: interlace(pl, order))])
        T = clip.shape[0]
        frames, modes, cnt = fm.field_match_torch(clip, fmt, T, R, N, 3, order, THR, MI)
        assert {0, 1, 3} <= set(modes.tolist())
        assert torch.equal(run_counts(hip, clip, fmt, T, R, N, 3, order, THR), cnt), (R, N)
        st = fm.Stats("cuda:0")
        g = guarded(tuple(clip.shape), clip.dtype)
        out = fm.field_match(clip.cuda(), fmt, T, R, N, 3, order, THR, MI, ops=hip, out=g.t, stats=st)
        torch.cuda.synchronize()
        g.assert_guards(fmt)
        assert out is g.t and torch.equal(out.cpu(), frames) and torch.equal(st.counts.cpu(), spec_stats(fm, modes, cnt)), (R, N)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_select_on_crafted_counts_takes_every_mode_and_tie(hip, shape, fmt):
    """The counts are crafted, so the four modes and the three ties occur at every shape whatever the clip holds (7 frames: one of
    each row of fieldmatch_cases.crafted_counts).  modes and stats are written when given and untouched when NULL."""
    fm, de = sub("fieldmatch"), sub("deinterlace")
    _, H, W = shape
    T = 7
    for C in channel_counts(fmt):
        s = step(fmt, C)
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        cnt, want_modes = crafted_counts(T, 5, s)
        for n, (kind, order) in enumerate(zip(CONTEXTS, ORDERS * 2)):
            before, after = context(kind, fmt, H, W, C, seed=n)
            deint = de.deinterlace_torch(packed, fmt, T, H, W, C, order, "frame", before, after)
            want = fm.select_torch(packed, deint, torch.tensor(want_modes, dtype=torch.int32), fmt, T, H, W, C, order, before, after)
            frames, gm, gs = run_select(hip, packed, deint, cnt, fmt, T, H, W, C, order, 5, before, after)
            assert gm.tolist() == want_modes == fm.modes_torch(cnt, 5, s).tolist()
            assert torch.equal(gs, spec_stats(fm, gm, cnt)) and gs[:4].tolist() == [1, 3, 1, 2]
            assert torch.equal(frames, want), (C, kind, order)
            bare, _, _ = run_select(hip, packed, deint, cnt, fmt, T, H, W, C, order, 5, before, after, side=False)
            assert torch.equal(bare, want), (C, kind, order)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_output_sample_is_written(hip, fmt):
    """Samples below the poison pattern: no output sample can equal it, so one that still holds it was never stored.  (7, 5, 32): the
    vector route for the luma plane and the RGB formats, the element route for the 8-bit chroma planes; (7, 17, 33): the element
    route everywhere."""
    fm, de = sub("fieldmatch"), sub("deinterlace")
    for T, H, W in ((7, 5, 32), (7, 17, 33)):
        C = channel_counts(fmt)[-1]
        packed = random_packed(fmt, T, H, W, C, seed=9)
        packed = (packed.to(torch.int64) % (0xA5 if packed.dtype == torch.uint8 else 0x3FF)).to(packed.dtype)
        cnt, want_modes = crafted_counts(T, 5, step(fmt, C))
        deint = de.deinterlace_torch(packed, fmt, T, H, W, C, "bff", "frame")
        want = fm.select_torch(packed, deint, torch.tensor(want_modes, dtype=torch.int32), fmt, T, H, W, C, "bff")
        frames, _, _ = run_select(hip, packed, deint, cnt, fmt, T, H, W, C, "bff", 5, written=True)
        assert torch.equal(frames, want), (fmt, T, H, W)


def shifted(t, off):
    """a dense copy of t that starts ``off`` bytes past a 16-byte boundary"""
    size = t.element_size()
    store = torch.empty(t.numel() + 16 // size, dtype=t.dtype, device="cuda")
    view = store[off // size:off // size + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == off
    return view


def test_unaligned_views_give_the_same_bits_and_two_runs_agree(hip):
    """Without ``out`` the ops allocate; a view 2 or 4 bytes off a 16-byte boundary, for each operand in turn, takes the element
    route and gives the same bits; two runs of comb_counts give the same bits (integer atomics commute)."""
    fm, de = sub("fieldmatch"), sub("deinterlace")
    T, H, W = 7, 18, 32
    for fmt in FORMATS:
        C = 3
        packed = random_packed(fmt, T, H, W, C, seed=4)
        before, after = context("both", fmt, H, W, C, seed=5)
        want_cnt = fm.comb_counts_torch(packed, fmt, T, H, W, C, "tff", 40, before, after)
        cnt, want_modes = crafted_counts(T, 5, step(fmt, C))
        deint = de.deinterlace_torch(packed, fmt, T, H, W, C, "tff", "frame", before, after)
        want = fm.select_torch(packed, deint, torch.tensor(want_modes, dtype=torch.int32), fmt, T, H, W, C, "tff", before, after)
        base = dict(packed=packed.cuda(), before=before.cuda(), after=after.cuda(), deint=deint.cuda(), cnt=cnt.cuda())
        runs = [hip.comb_counts(base["packed"], fmt, T, H, W, C, "tff", 40, before=base["before"], after=base["after"]) for _ in range(2)]
        assert runs[0].dtype == torch.int32 and torch.equal(runs[0], runs[1]) and torch.equal(runs[0].cpu(), want_cnt), fmt
        got = hip.field_select(base["packed"], base["deint"], base["cnt"], fmt, T, H, W, C, "tff", 5, before=base["before"], after=base["after"])
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want), fmt
        size = packed.element_size()
        for off in (2, 4):
            for which in ("packed", "before", "after"):
                ops = dict(base)
                ops[which] = shifted(ops[which], off)
                got = hip.comb_counts(ops["packed"], fmt, T, H, W, C, "tff", 40, before=ops["before"], after=ops["after"])
                assert torch.equal(got.cpu(), want_cnt), (fmt, off, which)
            for which in ("packed", "before", "after", "deint", "cnt"):
                if which == "cnt" and off % 4:                                     # (int32: 4 bytes off is its smallest offset)
                    continue
                ops = dict(base)
                ops[which] = shifted(ops[which], off)
                g = guarded(want.shape, want.dtype)
                hip.field_select(ops["packed"], ops["deint"], ops["cnt"], fmt, T, H, W, C, "tff", 5, before=ops["before"], after=ops["after"], out=g.t)
                torch.cuda.synchronize()
                g.assert_guards(fmt)
                assert torch.equal(g.t.cpu(), want), (fmt, off, which)
            # the output off 16 bytes: a view ``off`` bytes into a guarded payload
            g = guarded((want.numel() + off // size,), want.dtype)
            out = g.t[off // size:].view(want.shape)
            hip.field_select(base["packed"], base["deint"], base["cnt"], fmt, T, H, W, C, "tff", 5, before=base["before"], after=base["after"], out=out)
            torch.cuda.synchronize()
            g.assert_guards(fmt)
            assert torch.equal(out.cpu(), want) and bool(g.poisoned()[:off // size].all()), (fmt, off)


def test_refusals_name_the_argument_and_launch_nothing(hip):
    hip_lib, fm = sub("hip_lib"), sub("fieldmatch")
    packed = random_packed("rgb8", 2, 6, 8, 4, seed=0).cuda()
    planes = random_packed("yuv420p10", 2, 6, 8, 3, seed=0).cuda()
    frame = packed[0].clone()
    deint, cnt = packed.clone(), torch.zeros(2, 3, 2, dtype=torch.int32, device="cuda")
    out, gc = guarded((2, 6, 8, 4), torch.uint8), guarded((2, 3, 2), torch.int32)
    counts = lambda *a, **kw: hip.comb_counts(*a, **{"out": gc.t, **kw})
    select = lambda *a, **kw: hip.field_select(*a, **{"out": out.t, **kw})
    with pytest.raises(ValueError, match="comb_counts: .*C = 3"):
        counts(planes, "yuv420p10", 2, 6, 8, 4, "tff", 12)
    with pytest.raises(ValueError, match="comb_counts: fmt"):
        counts(packed, "rgb10", 2, 6, 8, 4, "tff", 12)
    with pytest.raises(ValueError, match="comb_counts: order"):
        counts(packed, "rgb8", 2, 6, 8, 4, "top", 12)
    with pytest.raises(ValueError, match="comb_counts: thr must be an integer in 0..255"):
        counts(packed, "rgb8", 2, 6, 8, 4, "tff", 256)
    with pytest.raises(ValueError, match="comb_counts: packed must be torch.uint16"):
        counts(packed, "rgb16", 2, 6, 8, 4, "tff", 12)
    with pytest.raises(ValueError, match="comb_counts: packed must hold"):
        counts(packed, "rgb8", 2, 6, 9, 4, "tff", 12)
    with pytest.raises(ValueError, match="comb_counts: before must hold"):
        counts(packed, "rgb8", 2, 6, 8, 4, "tff", 12, before=packed)
    with pytest.raises(ValueError, match="comb_counts: packed must be contiguous"):
        counts(torch.cat([packed, packed], dim=3)[..., ::2], "rgb8", 2, 6, 8, 4, "tff", 12)
    with pytest.raises(ValueError, match="comb_counts: after must live on"):
        counts(packed, "rgb8", 2, 6, 8, 4, "tff", 12, after=frame.cpu())
    with pytest.raises(ValueError, match="comb_counts: out must be"):
        hip.comb_counts(packed, "rgb8", 2, 6, 8, 4, "tff", 12, out=torch.empty(2, 3, 2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="comb_counts: out must be"):
        hip.comb_counts(packed, "rgb8", 2, 6, 8, 4, "tff", 12, out=torch.empty(3, 3, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="field_select: order"):
        select(packed, deint, cnt, "rgb8", 2, 6, 8, 4, "top", 5)
    with pytest.raises(ValueError, match="field_select: mi must be a non-negative integer"):
        select(packed, deint, cnt, "rgb8", 2, 6, 8, 4, "tff", -1)
    with pytest.raises(ValueError, match="field_select: deint must be torch.uint8"):
        select(packed, deint.to(torch.int16), cnt, "rgb8", 2, 6, 8, 4, "tff", 5)
    with pytest.raises(ValueError, match="field_select: deint must hold"):
        select(packed, deint[:1], cnt, "rgb8", 2, 6, 8, 4, "tff", 5)
    with pytest.raises(ValueError, match="field_select: cnt must be torch.int32"):
        select(packed, deint, cnt.long(), "rgb8", 2, 6, 8, 4, "tff", 5)
    with pytest.raises(ValueError, match="field_select: cnt must be"):
        select(packed, deint, cnt[:1], "rgb8", 2, 6, 8, 4, "tff", 5)
    with pytest.raises(ValueError, match="field_select: deint must live on"):
        select(packed, deint.cpu(), cnt, "rgb8", 2, 6, 8, 4, "tff", 5)
    with pytest.raises(ValueError, match="field_select: modes must hold 2 elements"):
        select(packed, deint, cnt, "rgb8", 2, 6, 8, 4, "tff", 5, modes=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="field_select: stats must be torch.int64"):
        select(packed, deint, cnt, "rgb8", 2, 6, 8, 4, "tff", 5, stats=torch.zeros(6, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="field_select: out must be"):
        hip.field_select(packed, deint, cnt, "rgb8", 2, 6, 8, 4, "tff", 5, out=torch.empty(4, 6, 8, 4, dtype=torch.uint8, device="cuda"))

    class Failing:
        def comb_counts(self, *a, **kw):
            raise hip_lib.HipLibraryError("library failed")
        field_select = comb_counts

    with pytest.raises(hip_lib.HipLibraryError, match="library failed"):                 # (no fall-back from a failing library)
        fm.field_match(packed, "rgb8", 2, 6, 8, 4, "tff", 12, 5, ops=Failing())
    # the C entry points themselves, device pointers: wrong byte counts, unknown ids, an output over an input
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = hip.lib
    n = 2 * 6 * 8 * 4
    for nin, ncnt, word in ((n - 1, 48, b"packed_bytes is 383, the format needs exactly 384"),
                            (n, 24, b"cnt_bytes is 24, int32 [T, 3, 2] needs exactly 48")):
        assert L.svr_comb_counts(p(packed), nin, None, None, 0, 2, 6, 8, 4, 0, 12, p(gc.t), ncnt, None) != 0
        assert word in L.svr_last_error(), L.svr_last_error()
    assert L.svr_comb_counts(p(packed), n, None, None, 0, 2, 6, 8, 4, 0, 300, p(gc.t), 48, None) != 0
    assert b"thr must lie in 0..255" in L.svr_last_error()
    assert L.svr_field_select(p(packed), n, None, None, p(deint), n, p(cnt), 48, 0, 2, 6, 8, 4, 0, 5, p(out.t), n + 1, None, None, None) != 0
    assert b"out_bytes is 385, the format needs exactly 384" in L.svr_last_error()
    with pytest.raises(hip_lib.HipLibraryError, match="order must be"):
        hip_lib.check(L.svr_field_select(p(packed), n, None, None, p(deint), n, p(cnt), 48, 0, 2, 6, 8, 4, 2, 5, p(out.t), n, None, None, None),
                      "svr_field_select")
    # outputs that overlap an input, through HipOps: the payload holds the clip itself, then
    store = guarded((3 * n,), torch.uint8)
    store.t[:n].copy_(packed.reshape(-1))
    inside = store.t[:n].view(2, 6, 8, 4)
    kept = store.t.clone()
    with pytest.raises(hip_lib.HipLibraryError, match="out overlaps packed"):
        hip.field_select(inside, deint, cnt, "rgb8", 2, 6, 8, 4, "tff", 5, out=store.t[n - 16:2 * n - 16].view(2, 6, 8, 4))
    with pytest.raises(hip_lib.HipLibraryError, match="out overlaps deint"):
        hip.field_select(packed, inside, cnt, "rgb8", 2, 6, 8, 4, "tff", 5, out=store.t[n - 16:2 * n - 16].view(2, 6, 8, 4))
    with pytest.raises(hip_lib.HipLibraryError, match="out overlaps before"):
        hip.field_select(packed, deint, cnt, "rgb8", 2, 6, 8, 4, "tff", 5, before=store.t[:n // 2].view(6, 8, 4), out=inside)
    with pytest.raises(hip_lib.HipLibraryError, match="cnt overlaps packed"):
        hip.comb_counts(inside, "rgb8", 2, 6, 8, 4, "tff", 12, out=store.t[n - 16:n + 32].view(torch.int32).view(2, 3, 2))
    with pytest.raises(hip_lib.HipLibraryError, match="modes overlaps cnt"):
        select(packed, deint, cnt, "rgb8", 2, 6, 8, 4, "tff", 5, modes=cnt.view(-1)[4:6])
    torch.cuda.synchronize()
    for g in (out, gc, store):
        g.assert_guards("refused calls")
    assert bool(out.poisoned().all()) and bool(gc.poisoned().all()) and torch.equal(store.t, kept)      # nothing was launched
    assert torch.equal(deint, packed) and not cnt.any()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_frame_source_matches_fields_on_the_device_and_feeds_the_stream(hip, tmp_path):
    """A stand-in ffmpeg emits 13 yuv420p10 frames of 18 x 40 (10 telecined, 3 interlaced); FrameSource(fields=("tff", "match")) in
    chunks of 5 equals the specification applied to the whole clip, bit for bit; pipeline.upscale_stream fed by it equals
    upscale_stream fed the specification's frames; field_stats.report() equals the counts of the specification's modes."""
    from test_stream import tiny_runner
    fin, fm, pipeline = sub("frameio_in"), sub("fieldmatch"), sub("pipeline")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_fieldmatch", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    runner, text = tiny_runner(hip, vae_channels=(128, 128, 128, 128)), sub("weights").synth_text_embedding().cuda()
    kw = dict(resolution=32, batch_size=5, color_correction="wavelet", temporal_overlap=2, prepend_frames=1)
    ffprobe, ffmpeg = stand_ins(str(tmp_path / "bin"))
    P = pictures(14, 18, 40, 2, seed=3)
    packed = torch.cat([packed_clip(P[:8], "yuv420p10", lambda pl: telecine(pl, "tff")[0]),
                        packed_clip(P[8:], "yuv420p10", lambda pl: interlace(pl, "tff"))])
    clip = tmp_path / "clip.mkv"
    fake_video(clip, packed, "yuv420p10le", 40, 18, rate="25/1", color_space="bt709", color_range="tv")
    info = cli.probe_video(ffprobe, str(clip))
    src = cli.FrameSource(ffmpeg, str(clip), info, 5, ops=hip, device="cuda:0", fields=("tff", "match"), match=dict(thr=THR, mi=MI))
    assert len(src.buffers) == 2 and all(b.is_pinned() for b in src.buffers) and src.fps == Fraction(25)
    assert src.field_stats.counts.is_cuda
    seen = []

    def chunks():
        for c in src.chunks():
            assert c.is_cuda and c.dtype == torch.float32
            seen.append(c.cpu())
            yield c

    got = [o.cpu() for o in pipeline.upscale_stream(chunks(), runner, text, **kw)]
    matched, modes, cnt = fm.field_match_torch(packed, "yuv420p10", 13, 18, 40, 3, "tff", THR, MI)
    assert modes.tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 3, 3, 3]
    frames = fin.unpack_frames_torch(matched, "yuv420p10", 13, 18, 40, 3, "bt709", "tv")
    assert [c.shape[0] for c in seen] == [5, 5, 3] and torch.equal(torch.cat(seen), frames)
    want = [o.cpu() for o in pipeline.upscale_stream((frames[i:i + 5].cuda() for i in range(0, 13, 5)), runner, text, **kw)]
    assert len(got) == len(want) == 3
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), k
    whole = fm.Stats()
    whole.add(modes, cnt)
    report = src.field_stats.report()
    assert report == whole.report() and [report[k] for k in ("stored", "prev", "next", "deinterlaced")] == [6, 4, 0, 3]
    assert not src.thread.is_alive()
