"""-m gpu: csrc/svr_decimate.hip through HipOps.frame_diffs / HipOps.decimate_select against its specification decimate.py -- EQUAL,
every shape, format and channel count, with and without ``before`` (integers in, integers out: a mismatch is a finding, not a
tolerance) --, crafted diffs that put the drop at every position and tie, the alignment routes, determinism, the telecine property
on the device, and the command line's FrameSource(fields=("tff", "decimate")) feeding pipeline.upscale_stream on the device.

Outputs live in tests/guarded_out.py buffers and the guards must stay intact.  The payload's poison is the byte 0xA5, which a
copied sample can equal: the left-over check is made on clips whose samples all lie BELOW 0xA5 (0xA5A5 for the 16-bit formats) --
every output sample is a stored sample."""
import importlib.util
import os
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from decimate_cases import (FIRST, FORMATS, GEOMETRIES, MI, ORDERS, SHAPES, SHIFT, THR, channel_counts, crafted_diffs, interlace, packed_clip,
                            pictures, random_packed, telecine)
from frame_unpack_cases import fake_video, stand_ins
from guarded_out import guarded

pytestmark = pytest.mark.gpu
DUP = 64                                              # the tests' own parameter (never decimate.DEFAULTS)
START = [5, 0, 7, 0, 11, 3]                           # what stats holds before a call: it is ADDED to


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def dev(t):
    return None if t is None else t.cuda()


def step(fmt, C):
    return 1 if fmt in ("yuv420p8", "yuv420p10") else C


def run_diffs(hip, packed, fmt, T, H, W, C, before=None):
    g = guarded((T,), torch.int32)
    out = hip.frame_diffs(dev(packed), fmt, T, H, W, C, before=dev(before), out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"frame_diffs {fmt} {(T, H, W, C)}")
    return out.cpu()


def run_select(hip, packed, diff, fmt, T, H, W, C, dup, written=False, side=True):
    """-> (frames, drops, stats): drops / stats None where ``side`` is False (NULL pointers)"""
    g = guarded((T - T // 5,) + tuple(packed.shape[1:]), packed.dtype)
    gd, gs = guarded((T // 5,), torch.int32), guarded((6,), torch.int64, init=torch.tensor(START, device="cuda"))
    out = hip.decimate_select(dev(packed), dev(diff), fmt, T, H, W, C, dup, out=g.t, drops=gd.t if side else None, stats=gs.t if side else None)
    torch.cuda.synchronize()
    assert out is g.t
    name = f"decimate_select {fmt} {(T, H, W, C)}"
    for b in (g, gd, gs):
        b.assert_guards(name)
    if written:
        g.assert_written(name)
    if not side:
        assert bool(gd.poisoned().all()) and gs.t.tolist() == START                                  # untouched
        return out.cpu(), None, None
    gd.assert_written(name)
    return out.cpu(), gd.t.cpu(), gs.t.cpu() - torch.tensor(START)


def spec_stats(dec, drops, diff, dup, s, shift):
    st = dec.Stats()
    st.add(drops, diff, dup, s, shift)
    return st.counts


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_specification_on_random_clips(hip, shape, fmt):
    """Random samples over the whole code range: block sums near a block's capacity.  The select kernel is fed the diff kernel's own
    output, with a bound that splits the diffs the clip has; drops and stats present, then NULL."""
    dec = sub("decimate")
    T, H, W = shape
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        s = step(fmt, C)
        for before in (None, random_packed(fmt, 1, H, W, C, seed=77)):
            want_frames, want_drops, want = dec.decimate_torch(packed, fmt, T, H, W, C, before)
            got = run_diffs(hip, packed, fmt, T, H, W, C, before)
            assert torch.equal(got, want), (C, before is None, got.tolist(), want.tolist())
            dup = min((int(want[1:].max()) >> SHIFT[fmt]) // (2 * s), 2 ** 18) if T > 1 else 0
            frames, drops, stats = run_select(hip, packed, got, fmt, T, H, W, C, dup)
            assert torch.equal(drops, want_drops) and torch.equal(stats, spec_stats(dec, want_drops, want, dup, s, SHIFT[fmt])), (C, before is None)
            assert torch.equal(frames, want_frames), (C, before is None)
            bare, _, _ = run_select(hip, packed, got, fmt, T, H, W, C, dup, side=False)
            assert torch.equal(bare, want_frames), (C, before is None)


@pytest.mark.parametrize("fmt", FORMATS)
def test_select_on_crafted_diffs_drops_at_every_position_and_tie(hip, fmt):
    """The diffs are crafted, so every position, both kinds of tie, the sentinel and both sides of the bound occur whatever the clip
    holds: 43 frames -- the eight rows of decimate_cases.crafted_diffs and a three-frame tail -- and T on both sides of one cycle."""
    dec = sub("decimate")
    for T, H, W in ((43, 5, 32), (43, 3, 7), (4, 5, 32), (5, 3, 7), (9, 5, 32)):
        for C in channel_counts(fmt):
            s = step(fmt, C)
            packed = random_packed(fmt, T, H, W, C, seed=T + C)
            diff, want_drops = crafted_diffs(T, (DUP * s) << SHIFT[fmt])
            want = dec.select_torch(packed, torch.tensor(want_drops, dtype=torch.int32), fmt, T, H, W, C)
            frames, drops, stats = run_select(hip, packed, diff, fmt, T, H, W, C, DUP)
            assert drops.tolist() == want_drops == dec.drops_torch(diff).tolist(), (T, C)
            assert torch.equal(stats, spec_stats(dec, drops, diff, DUP, s, SHIFT[fmt])), (T, C)
            if T == 43:
                assert stats.tolist() == [2, 2, 1, 1, 2, 5]
            assert torch.equal(frames, want), (T, C)
            bare, _, _ = run_select(hip, packed, diff, fmt, T, H, W, C, DUP, side=False)
            assert torch.equal(bare, want), (T, C)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_output_sample_is_written(hip, fmt):
    """Samples below the poison pattern: no output sample can equal it, so one that still holds it was never stored.  (11, 5, 32):
    the vector route; (11, 17, 33): an odd frame size, the element route."""
    dec = sub("decimate")
    for T, H, W in ((11, 5, 32), (11, 17, 33)):
        C = channel_counts(fmt)[-1]
        packed = random_packed(fmt, T, H, W, C, seed=9)
        packed = (packed.to(torch.int64) % (0xA5 if packed.dtype == torch.uint8 else 0x3FF)).to(packed.dtype)
        diff, want_drops = crafted_diffs(T, 0)
        want = dec.select_torch(packed, torch.tensor(want_drops, dtype=torch.int32), fmt, T, H, W, C)
        frames, _, _ = run_select(hip, packed, diff, fmt, T, H, W, C, DUP, written=True)
        assert torch.equal(frames, want), (fmt, T, H, W)
        g = guarded((T,), torch.int32)                                            # the diffs: every entry is zeroed, then written
        hip.frame_diffs(packed.cuda(), fmt, T, H, W, C, out=g.t)
        torch.cuda.synchronize()
        g.assert_guards(fmt)
        assert torch.equal(g.t.cpu(), dec.diffs_torch(packed, fmt, T, H, W, C)) and g.t[0] == FIRST


def shifted(t, off):
    """a dense copy of t that starts ``off`` bytes past a 16-byte boundary"""
    size = t.element_size()
    store = torch.empty(t.numel() + 16 // size, dtype=t.dtype, device="cuda")
    view = store[off // size:off // size + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == off
    return view


def test_unaligned_views_give_the_same_bits_and_two_runs_agree(hip):
    """Without ``out`` the ops allocate; a view one element (and 4 bytes) off a 16-byte boundary, for each operand in turn, takes the
    element route and gives the same bits; two runs of frame_diffs give the same bits (integer max commutes)."""
    dec = sub("decimate")
    T, H, W = 7, 34, 32
    for fmt in FORMATS:
        C = 3
        packed = random_packed(fmt, T, H, W, C, seed=4)
        before = random_packed(fmt, 1, H, W, C, seed=5)[0]
        want_diff = dec.diffs_torch(packed, fmt, T, H, W, C, before)
        diff, want_drops = crafted_diffs(T, 0)
        want = dec.select_torch(packed, torch.tensor(want_drops, dtype=torch.int32), fmt, T, H, W, C)
        base = dict(packed=packed.cuda(), before=before.cuda(), diff=diff.cuda())
        runs = [hip.frame_diffs(base["packed"], fmt, T, H, W, C, before=base["before"]) for _ in range(2)]
        assert runs[0].dtype == torch.int32 and torch.equal(runs[0], runs[1]) and torch.equal(runs[0].cpu(), want_diff), fmt
        got = hip.decimate_select(base["packed"], base["diff"], fmt, T, H, W, C, DUP)
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want), fmt
        size = packed.element_size()
        for off in (size, 4):                                                      # one element; and int32's smallest offset
            for which in ("packed", "before"):
                ops = dict(base)
                ops[which] = shifted(ops[which], off)
                got = hip.frame_diffs(ops["packed"], fmt, T, H, W, C, before=ops["before"])
                assert torch.equal(got.cpu(), want_diff), (fmt, off, which)
            for which in ("packed", "diff"):
                if which == "diff" and off % 4:
                    continue
                ops = dict(base)
                ops[which] = shifted(ops[which], off)
                g = guarded(want.shape, want.dtype)
                hip.decimate_select(ops["packed"], ops["diff"], fmt, T, H, W, C, DUP, out=g.t)
                torch.cuda.synchronize()
                g.assert_guards(fmt)
                assert torch.equal(g.t.cpu(), want), (fmt, off, which)
            # the output off 16 bytes: a view ``off`` bytes into a guarded payload
            g = guarded((want.numel() + off // size,), want.dtype)
            out = g.t[off // size:].view(want.shape)
            hip.decimate_select(base["packed"], base["diff"], fmt, T, H, W, C, DUP, out=out)
            torch.cuda.synchronize()
            g.assert_guards(fmt)
            assert torch.equal(out.cpu(), want) and bool(g.poisoned()[:off // size].all()), (fmt, off)


def test_refusals_name_the_argument_and_launch_nothing(hip):
    hip_lib, dec = sub("hip_lib"), sub("decimate")
    packed = random_packed("rgb8", 5, 6, 8, 4, seed=0).cuda()
    diff = torch.zeros(5, dtype=torch.int32, device="cuda")
    out, gd = guarded((4, 6, 8, 4), torch.uint8), guarded((5,), torch.int32)
    with pytest.raises(ValueError, match="frame_diffs: fmt"):
        hip.frame_diffs(packed, "rgb10", 5, 6, 8, 4, out=gd.t)
    with pytest.raises(ValueError, match="frame_diffs: packed must hold"):
        hip.frame_diffs(packed, "rgb8", 5, 6, 9, 4, out=gd.t)
    with pytest.raises(ValueError, match="frame_diffs: before must hold"):
        hip.frame_diffs(packed, "rgb8", 5, 6, 8, 4, before=packed, out=gd.t)
    with pytest.raises(ValueError, match="frame_diffs: before must live on"):
        hip.frame_diffs(packed, "rgb8", 5, 6, 8, 4, before=packed[0].cpu(), out=gd.t)
    with pytest.raises(ValueError, match="frame_diffs: out must be"):
        hip.frame_diffs(packed, "rgb8", 5, 6, 8, 4, out=torch.empty(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="decimate_select: dup must be an integer in 0..262144"):
        hip.decimate_select(packed, diff, "rgb8", 5, 6, 8, 4, 2 ** 18 + 1, out=out.t)
    with pytest.raises(ValueError, match="decimate_select: diff must be torch.int32"):
        hip.decimate_select(packed, diff.long(), "rgb8", 5, 6, 8, 4, DUP, out=out.t)
    with pytest.raises(ValueError, match="decimate_select: diff must be"):
        hip.decimate_select(packed, diff[:4], "rgb8", 5, 6, 8, 4, DUP, out=out.t)
    with pytest.raises(ValueError, match="decimate_select: out must be"):
        hip.decimate_select(packed, diff, "rgb8", 5, 6, 8, 4, DUP, out=torch.empty(5, 6, 8, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="decimate_select: drops must hold 1 elements"):
        hip.decimate_select(packed, diff, "rgb8", 5, 6, 8, 4, DUP, out=out.t, drops=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="decimate_select: stats must be torch.int64"):
        hip.decimate_select(packed, diff, "rgb8", 5, 6, 8, 4, DUP, out=out.t, stats=torch.zeros(6, dtype=torch.int32, device="cuda"))
    with pytest.raises(hip_lib.HipLibraryError, match="drops overlaps diff"):
        hip.decimate_select(packed, diff, "rgb8", 5, 6, 8, 4, DUP, out=out.t, drops=diff[2:3])
    with pytest.raises(hip_lib.HipLibraryError, match="out overlaps packed"):
        hip.decimate_select(packed, diff, "rgb8", 5, 6, 8, 4, DUP, out=packed[:4])

    class Failing:
        def frame_diffs(self, *a, **kw):
            raise hip_lib.HipLibraryError("library failed")
        decimate_select = frame_diffs

    with pytest.raises(hip_lib.HipLibraryError, match="library failed"):                 # (no fall-back from a failing library)
        dec.decimate(packed, "rgb8", 5, 6, 8, 4, DUP, ops=Failing())
    torch.cuda.synchronize()
    for g in (out, gd):
        g.assert_guards("refused calls")
    assert bool(out.poisoned().all()) and bool(gd.poisoned().all()) and not diff.any()    # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_matched_telecined_clip_comes_back_as_its_pictures_on_the_device(hip, fmt):
    """Field matching and decimation through HipOps, stats included: 15 telecined frames -> the 12 pictures, bit for bit, the drop at
    position 2 of every cycle, no dropped frame over the bound."""
    dec, fm = sub("decimate"), sub("fieldmatch")
    for (R, N, speed), order in zip(GEOMETRIES, ORDERS):
        P = pictures(12, R, N, speed, seed=N)
        prog = packed_clip(P, fmt)
        tele = packed_clip(P, fmt, lambda pl: telecine(pl, order)[0]).cuda()
        matched = fm.field_match(tele, fmt, 15, R, N, 3, order, THR, MI, ops=hip)
        st = dec.Stats("cuda:0")
        g = guarded(tuple(prog.shape), prog.dtype)
        out = dec.decimate(matched, fmt, 15, R, N, 3, DUP, ops=hip, out=g.t, stats=st)
        torch.cuda.synchronize()
        g.assert_guards(fmt)
        assert out is g.t and torch.equal(out.cpu(), prog), (R, N, order)
        assert st.report() == dict(cycles=3, positions=[0, 0, 3, 0, 0], not_duplicates=0)
        drops = torch.empty(3, dtype=torch.int32, device="cuda")
        hip.decimate_select(matched, hip.frame_diffs(matched, fmt, 15, R, N, 3), fmt, 15, R, N, 3, DUP, drops=drops)
        assert drops.tolist() == [2, 2, 2]


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_frame_source_decimates_on_the_device_and_feeds_the_stream(hip, tmp_path):
    """A stand-in ffmpeg emits 23 yuv420p10 frames of 18 x 40 (20 telecined from 16 pictures, 3 interlaced);
    FrameSource(fields=("tff", "decimate")) in buffers of 4 -- every cycle but the first is completed by carried frames -- equals the specification applied to the whole clip, bit for bit;
    pipeline.upscale_stream fed by it equals upscale_stream fed the specification's frames in the same chunks; both reports equal
    the specification's."""
    from test_stream import tiny_runner
    fin, fm, dec, pipeline = sub("frameio_in"), sub("fieldmatch"), sub("decimate"), sub("pipeline")
    spec = importlib.util.spec_from_file_location("svr_cli_gpu_decimate", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    runner, text = tiny_runner(hip, vae_channels=(128, 128, 128, 128)), sub("weights").synth_text_embedding().cuda()
    kw = dict(resolution=32, batch_size=5, color_correction="wavelet", temporal_overlap=2, prepend_frames=1)
    ffprobe, ffmpeg = stand_ins(str(tmp_path / "bin"))
    P = pictures(22, 18, 40, 2, seed=3)
    packed = torch.cat([packed_clip(P[:16], "yuv420p10", lambda pl: telecine(pl, "tff")[0]),
                        packed_clip(P[16:], "yuv420p10", lambda pl: interlace(pl, "tff"))])
    clip = tmp_path / "clip.mkv"
    fake_video(clip, packed, "yuv420p10le", 40, 18, rate="25/1", color_space="bt709", color_range="tv")
    info = cli.probe_video(ffprobe, str(clip))
    src = cli.FrameSource(ffmpeg, str(clip), info, 4, ops=hip, device="cuda:0", fields=("tff", "decimate"), match=dict(thr=THR, mi=MI),
                          decimate=dict(dup=DUP))
    assert len(src.buffers) == 2 and all(b.is_pinned() for b in src.buffers) and src.fps == Fraction(20)
    assert src.decimate_stats.counts.is_cuda and src.field_stats.counts.is_cuda
    seen = []

    def chunks():
        for c in src.chunks():
            assert c.is_cuda and c.dtype == torch.float32 and c.shape[0] > 0
            seen.append(c.cpu())
            yield c

    got = [o.cpu() for o in pipeline.upscale_stream(chunks(), runner, text, **kw)]
    matched, modes, cnt = fm.field_match_torch(packed, "yuv420p10", 23, 18, 40, 3, "tff", THR, MI)
    kept, drops, diff = dec.decimate_torch(matched, "yuv420p10", 23, 18, 40, 3)
    assert drops.tolist() == [2, 2, 2, 2]
    frames = fin.unpack_frames_torch(kept, "yuv420p10", 19, 18, 40, 3, "bt709", "tv")
    assert [c.shape[0] for c in seen] == [4, 4, 4, 4, 3] and torch.equal(torch.cat(seen), frames)
    want = [o.cpu() for o in pipeline.upscale_stream((frames[a:b].cuda() for a, b in ((0, 4), (4, 8), (8, 12), (12, 16), (16, 19))), runner, text, **kw)]
    assert len(got) == len(want) == 5
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), k
    whole, fwhole = dec.Stats(), fm.Stats()
    whole.add(drops, diff, DUP, 1, 2)
    fwhole.add(modes, cnt)
    assert src.decimate_stats.report() == whole.report() == dict(cycles=4, positions=[0, 0, 4, 0, 0], not_duplicates=0)
    assert src.field_stats.report() == fwhole.report()
    assert not src.thread.is_alive()
