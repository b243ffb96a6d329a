"""-m "not gpu": decimation (decimate.py, the specification of csrc/svr_decimate.hip) -- the torch statements against a restatement of
the text in plain integers, value cases, the drop rule on crafted diffs, the properties (a field-matched telecined clip comes back
as its film pictures bit for bit, a static clip as any four of five, any split equals the whole) --, the command line's reader
behind FrameSource(fields=(order, "decimate")) and the decimate.ENABLED switch against stand-ins for the two executables, and the
C ABI's refusals.  NOT covered anywhere: a real ffmpeg, real footage."""
import os
import re
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from decimate_cases import (FIRST, FORMATS, GEOMETRIES, MI, ORDERS, SHAPES, SHIFT, THR, channel_counts, crafted_diffs, interlace,
                            loop_drops, loop_frame_diffs, loop_select, loop_stats, packed_clip, pictures, random_packed, telecine)
from frame_unpack_cases import calls, fake_video, stand_ins
from test_deinterlace import tagged
from test_frame_unpack import identity  # noqa: F401 (fixture)
from test_refusal_messages import Ptr, call
from test_stream import cli, rig  # noqa: F401 (fixtures)

DUP = 64                                              # the tests' own parameter (never decimate.DEFAULTS)


def step(fmt, C):
    return 1 if fmt in ("yuv420p8", "yuv420p10") else C


# ---------------------------------------------------------------------------------------------------------------- specification
def test_module_surface_and_the_shipped_switch():
    dec, fm, de = sub("decimate"), sub("fieldmatch"), sub("deinterlace")
    assert dec.ENABLED is False and dec.RATE == "decimate" and dec.CYCLE == 5 and dec.BLOCK == 32 and dec.FIRST == FIRST
    assert "dup" in dec.DEFAULTS and len(dec.DEFAULTS) == 1
    assert dec.RATE not in de.RATES and dec.RATE != fm.RATE and dec.planes is de.planes
    for word in ("SYNTHETIC", "NOT MET REAL FOOTAGE", "No test depends on", "3:2 cycles of five only", "one drop per cycle, duplicate or not",
                 "plane 0 decides", "--skip_first_frames", "trailing partial cycle is kept whole", "no scene-change handling",
                 "tagged progressive", "one GPU", "FIRST position", "no mirror", "informational only"):
        assert word.lower() in dec.__doc__.lower(), word
    assert "no decimation" in fm.__doc__ and "decimate.py" in fm.__doc__
    st = dec.Stats()
    assert st.counts.dtype == torch.int64 and tuple(st.counts.shape) == (6,) and not st.counts.any()
    assert st.report() == dict(cycles=0, positions=[0, 0, 0, 0, 0], not_duplicates=0)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"decimate"' in entry


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_equals_the_loop_restatement(shape, fmt):
    """Random clips over the whole code range, every channel count, with and without ``before``: diffs, drops, select and stats."""
    dec = sub("decimate")
    T, H, W = shape
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        s = step(fmt, C)
        for before in (None, random_packed(fmt, 1, H, W, C, seed=77)):
            got = dec.diffs_torch(packed, fmt, T, H, W, C, before)
            want = loop_frame_diffs(packed, fmt, T, H, W, C, before)
            assert got.dtype == torch.int32 and tuple(got.shape) == (T,) and torch.equal(got, want), (C, before is None)
            assert (got[0] == FIRST) == (before is None)
            drops = dec.drops_torch(got)
            assert drops.dtype == torch.int32 and drops.tolist() == loop_drops(want.tolist()) and len(drops) == T // 5
            out = dec.select_torch(packed, drops, fmt, T, H, W, C)
            assert out.dtype == packed.dtype and out.shape == (T - T // 5,) + packed.shape[1:] and out.is_contiguous()
            assert torch.equal(out, loop_select(packed, drops.tolist(), T)), (C, before is None)
            frames, drops2, diff2 = dec.decimate_torch(packed, fmt, T, H, W, C, before)
            assert torch.equal(frames, out) and torch.equal(drops2, drops) and torch.equal(diff2, got)
            dup = int(want[1:].max()) >> SHIFT[fmt] if T > 1 else 0
            dup = min(dup // (2 * s), 2 ** 18)                                  # (a bound that splits the diffs the clip has)
            st = dec.Stats()
            st.add(drops, got, dup, s, SHIFT[fmt])
            assert st.counts.tolist() == loop_stats(drops.tolist(), want.tolist(), dup, s, SHIFT[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_value_cases_at_the_ends_of_each_code_range(fmt):
    """Two frames, all zero and all ``top``: every block sum is its sample count times top -- the largest possible one, 32 * 32 * 4 *
    65535, with C = 4 in rgb16 --; a partial block counts its own samples only; one sample off by one code gives 1; 10-bit samples
    above 1023 are used as stored."""
    dec = sub("decimate")
    top = 255 if SHIFT[fmt] == 0 else 65535

    def clip_of(rows, like):
        """int rows [T, frame] -> a packed clip of like's dtype and frame shape (built wide: torch has few uint16 ops)"""
        return torch.tensor(rows, dtype=torch.int32).to(like.dtype).reshape((len(rows),) + tuple(like.shape[1:]))

    for C in channel_counts(fmt):
        s = step(fmt, C)
        for H, W, full in ((32, 32, 32 * 32), (40, 70, 32 * 32), (7, 5, 35), (33, 31, 32 * 31)):
            like = random_packed(fmt, 2, H, W, C, seed=0)
            n = like.numel() // 2
            want = full * s * top
            assert want < 2 ** 31
            for rows in ([[0] * n, [top] * n], [[top] * n, [0] * n]):
                frames = clip_of(rows, like)
                diff = dec.diffs_torch(frames, fmt, 2, H, W, C)
                assert diff.tolist() == [FIRST, want] == loop_frame_diffs(frames, fmt, 2, H, W, C).tolist(), (fmt, C, H, W)
            last = [0] * n
            last[H * W * s - 1] = 1                                              # plane 0's last sample, off by one code
            one = clip_of([[0] * n, last], like)
            assert dec.diffs_torch(one, fmt, 2, H, W, C).tolist() == [FIRST, 1]
            assert dec.diffs_torch(one[1:], fmt, 1, H, W, C, before=one[0]).tolist() == [1]
            assert dec.diffs_torch(one[:1], fmt, 1, H, W, C, before=one[0]).tolist() == [0]
            if fmt == "rgb16" and C == 4 and (H, W) == (32, 32):
                assert want == 32 * 32 * 4 * 65535 == 268431360                  # the largest block sum there is
    if fmt in ("yuv420p8", "yuv420p10"):
        like = random_packed(fmt, 2, 4, 4, 3, seed=0)
        if fmt == "yuv420p10":                                                   # samples above 1023 are used as stored
            assert dec.diffs_torch(clip_of([[1023] * 24, [4000] * 16 + [1023] * 8], like), fmt, 2, 4, 4, 3).tolist() == [FIRST, 16 * (4000 - 1023)]
        # chroma decides nothing
        assert dec.diffs_torch(clip_of([[7] * 24, [7] * 16 + [200] * 8], like), fmt, 2, 4, 4, 3).tolist() == [FIRST, 0]


def test_drops_on_crafted_diffs_and_the_stats_bound():
    dec = sub("decimate")
    for s, shift, dup in ((1, 0, 0), (3, 0, 64), (4, 8, 1024), (1, 2, 2 ** 18)):
        bound = (dup * s) << shift
        for T in (1, 4, 5, 9, 40, 43):
            diff, want = crafted_diffs(T, bound)
            drops = dec.drops_torch(diff)
            assert drops.tolist() == want == loop_drops(diff.tolist()), (T, s)
            st = dec.Stats()
            st.add(drops, diff, dup, s, shift)
            assert st.counts.tolist() == loop_stats(want, diff.tolist(), dup, s, shift)
            assert st.report() == dict(cycles=T // 5, positions=st.counts.tolist()[:5], not_duplicates=st.counts.tolist()[5])
        diff, want = crafted_diffs(40, bound)
        assert set(want) == {0, 1, 2, 3, 4} and loop_stats(want, diff.tolist(), dup, s, shift) == [2, 2, 1, 1, 2, 5]
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(1, 5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="diff must be torch.int32"):
            dec.drops_torch(bad)


# ---------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("R,N,speed", GEOMETRIES)
def test_a_matched_telecined_clip_comes_back_as_its_pictures(R, N, speed, fmt):
    dec, fm = sub("decimate"), sub("fieldmatch")
    for order in ORDERS:
        P = pictures(12, R, N, speed, seed=N)
        prog = packed_clip(P, fmt)
        tele = packed_clip(P, fmt, lambda pl: telecine(pl, order)[0])
        matched = fm.field_match_torch(tele, fmt, 15, R, N, 3, order, THR, MI)[0]
        frames, drops, diff = dec.decimate_torch(matched, fmt, 15, R, N, 3)
        print(fmt, order, diff.tolist())
        assert drops.tolist() == [2, 2, 2] and torch.equal(frames, prog), (order, drops.tolist())
        d = diff.tolist()
        assert d[0] == FIRST and all(d[t] == 0 for t in (2, 7, 12)) and all(d[t] >= 1000 << SHIFT[fmt] for t in range(1, 15) if t % 5 != 2)
        st = dec.Stats()
        st.add(drops, diff, DUP, 3 if fmt in ("rgb8", "bgr8", "rgb16") else 1, SHIFT[fmt])
        assert st.report() == dict(cycles=3, positions=[0, 0, 3, 0, 0], not_duplicates=0)
        # a clip that was not telecined loses a frame per cycle all the same, and says so
        st = dec.Stats()
        frames, drops, diff = dec.decimate_torch(prog[:10].contiguous(), fmt, 10, R, N, 3)
        st.add(drops, diff, DUP, 3 if fmt in ("rgb8", "bgr8", "rgb16") else 1, SHIFT[fmt])
        assert frames.shape[0] == 8 and st.report()["cycles"] == 2 == st.report()["not_duplicates"]
        # static: any four of five of its identical frames
        image = random_packed(fmt, 1, R, N, 3, seed=R)
        still = image.expand(7, *image.shape[1:]).contiguous()
        frames, drops, diff = dec.decimate_torch(still, fmt, 7, R, N, 3)
        assert torch.equal(frames, still[:6]) and drops.tolist() == [1] and diff.tolist() == [FIRST, 0, 0, 0, 0, 0, 0]
        assert dec.drops_torch(dec.diffs_torch(still, fmt, 7, R, N, 3, before=image)).tolist() == [0]


def test_any_split_with_its_true_before_equals_the_whole():
    """diff[t] depends on frames t - 1 and t only: the diffs of any split are the whole's, so a caller that cuts at cycle boundaries,
    or carries the frames short of a cycle, gets the whole's frames."""
    dec, fm = sub("decimate"), sub("fieldmatch")
    fmt, R, N = "yuv420p8", 18, 40
    P = pictures(16, R, N, 2, seed=5)
    clip = torch.cat([packed_clip(P[:12], fmt, lambda pl: telecine(pl, "tff")[0]), packed_clip(P[12:], fmt)])
    T = clip.shape[0]
    assert T == 19
    clip = fm.field_match_torch(clip, fmt, T, R, N, 3, "tff", THR, MI)[0]
    whole, drops, diff = dec.decimate_torch(clip, fmt, T, R, N, 3)
    assert drops.tolist() == [2, 2, 2] and whole.shape[0] == 16
    for cuts in ((5,), (10, 15), (5, 10, 15), (3, 7), (2,), tuple(range(1, T)), (T - 1,), (4, 6, 11, 18)):
        edges = [0, *cuts, T]
        parts = [dec.diffs_torch(clip[a:b].contiguous(), fmt, b - a, R, N, 3, clip[a - 1] if a else None) for a, b in zip(edges[:-1], edges[1:])]
        assert torch.equal(torch.cat(parts), diff), cuts
        assert torch.equal(dec.select_torch(clip, dec.drops_torch(torch.cat(parts)), fmt, T, R, N, 3), whole), cuts
        if all(c % 5 == 0 for c in cuts):                                       # cut at cycle boundaries: the parts are the whole's frames
            frames = [dec.decimate_torch(clip[a:b].contiguous(), fmt, b - a, R, N, 3, clip[a - 1] if a else None)[0]
                      for a, b in zip(edges[:-1], edges[1:])]
            assert torch.equal(torch.cat(frames), whole), cuts
    assert torch.equal(dec.select_torch(clip, dec.drops_torch(diff), fmt, T, R, N, 3), whole)


def test_arguments_are_refused_by_name_and_the_front_composes_the_steps():
    dec = sub("decimate")
    packed = random_packed("rgb8", 7, 4, 6, 3, seed=0)
    ok = dict(packed=packed, fmt="rgb8", T=7, H=4, W=6, C=3)
    for change, word in ((dict(fmt="rgb10"), "fmt must be"), (dict(C=2), "C = 3 or 4"), (dict(T=0, packed=packed[:0]), "T, H, W must be positive"),
                         (dict(packed=packed.to(torch.int16)), "packed must be torch.uint8"), (dict(W=7), "packed must hold 588 samples"),
                         (dict(before=packed), "before must hold the 72 samples of one rgb8 frame"),
                         (dict(before=packed[0].to(torch.int32)), "before must be torch.uint8"), (dict(fmt="yuv420p8", C=4), "yuv420p8 takes C = 3")):
        with pytest.raises(ValueError, match=re.escape(word)):
            dec.diffs_torch(**{**ok, **change})
        with pytest.raises(ValueError, match=re.escape(word)):
            dec.decimate(**{**ok, **change}, dup=DUP)
    for bad in (-1, 2 ** 18 + 1, 1.0, None, True):
        with pytest.raises(ValueError, match=re.escape("dup must be an integer in 0..262144")):
            dec.decimate(**ok, dup=bad)
    for out in (torch.empty(7, 4, 6, 3, dtype=torch.uint8), torch.empty(6, 4, 6, 3, dtype=torch.int16), torch.empty(6, 4, 6, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=re.escape("out must be torch.uint8 (6, 4, 6, 3)")):
            dec.decimate(**ok, dup=DUP, out=out)
    with pytest.raises(ValueError, match="drops must be torch.int32"):
        dec.select_torch(**ok, drops=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="drops must be torch.int32"):
        dec.select_torch(**ok, drops=torch.zeros(2, dtype=torch.int32))
    # the front: the torch statements without ops, ``out`` filled, ``stats`` added to; dup = 0 and 2^18 are taken
    want, drops, diff = dec.decimate_torch(**ok)
    out, st = torch.empty_like(want), dec.Stats()
    assert dec.decimate(**ok, dup=0, out=out, stats=st) is out and torch.equal(out, want) and torch.equal(dec.decimate(**ok, dup=2 ** 18), want)
    dec.decimate(**ok, dup=0, stats=st)
    assert st.counts.tolist() == [2 * n for n in loop_stats(drops.tolist(), diff.tolist(), 0, 3, 0)] and st.counts[5] == 2

    # a backend that has the two ops is used -- and handed the diffs and the stats tensor; one that fails raises
    class Double:
        def __init__(self):
            self.seen = []

        def frame_diffs(self, packed, fmt, T, H, W, C, before=None):
            self.seen.append("frame_diffs")
            return dec.diffs_torch(packed, fmt, T, H, W, C, before)

        def decimate_select(self, packed, diff_, fmt, T, H, W, C, dup, out=None, drops=None, stats=None):
            self.seen.append("decimate_select")
            assert torch.equal(diff_, diff) and stats is st2.counts and dup == DUP
            return dec.select_torch(packed, dec.drops_torch(diff_), fmt, T, H, W, C)

    double, st2 = Double(), dec.Stats()
    assert torch.equal(dec.decimate(**ok, dup=DUP, ops=double, stats=st2), want) and double.seen == ["frame_diffs", "decimate_select"]

    class Failing(Double):
        def frame_diffs(self, *a, **kw):
            raise RuntimeError("library failed")

    with pytest.raises(RuntimeError, match="library failed"):
        dec.decimate(**ok, dup=DUP, ops=Failing())

    class Half:                                                                 # (one op of the two: the torch statements)
        frame_diffs = Failing.frame_diffs

    assert torch.equal(dec.decimate(**ok, dup=DUP, ops=Half()), want)


# ---------------------------------------------------------------------------------------------------------------- reader
T_, H_, W_ = 23, 18, 40


def source_clip(fmt, order):
    """23 frames of the property geometry: 20 telecined frames from 16 pictures, then 3 interlaced ones"""
    P = pictures(22, H_, W_, 2, seed=3)
    return torch.cat([packed_clip(P[:16], fmt, lambda pl: telecine(pl, order)[0]), packed_clip(P[16:], fmt, lambda pl: interlace(pl, order))])


def spec_of_the_whole(fmt, order, matrix):
    """-> (the 19 fp32 frames, the decimation report, the field-matching report) of the specification on the whole clip"""
    fin, fm, dec = sub("frameio_in"), sub("fieldmatch"), sub("decimate")
    packed = source_clip(fmt, order)
    matched, modes, cnt = fm.field_match_torch(packed, fmt, T_, H_, W_, 3, order, THR, MI)
    frames, drops, diff = dec.decimate_torch(matched, fmt, T_, H_, W_, 3)
    assert drops.tolist() == [2, 2, 2, 2] and frames.shape[0] == 19
    st, fst = dec.Stats(), fm.Stats()
    st.add(drops, diff, DUP, 1 if "yuv" in fmt else 3, SHIFT[fmt])
    fst.add(modes, cnt)
    return fin.unpack_frames_torch(frames, fmt, 19, H_, W_, 3, matrix, "tv"), st.report(), fst.report()


def decimate_source(cli, tmp_path, fmt, pix, order, chunk, **kw):
    _, ffmpeg = stand_ins(str(tmp_path / "bin"))
    clip = tmp_path / f"clip_{fmt}.mkv"
    fake_video(clip, source_clip(fmt, order), pix, W_, H_)
    info = dict(width=W_, height=H_, fps=Fraction(30000, 1001), pix_fmt=pix, color_space=None, color_range=None, has_audio=False)
    return cli.FrameSource(ffmpeg, str(clip), info, chunk, fields=(order, "decimate"), **kw)


@pytest.mark.parametrize("fmt,pix,order", [("yuv420p10", "yuv420p10le", "tff"), ("yuv420p8", "yuv420p", "bff"), ("rgb8", "rgb24", "tff")])
def test_source_chunks_equal_the_specification_applied_to_the_whole_clip(cli, tmp_path, fmt, pix, order):
    want, report, field_report = spec_of_the_whole(fmt, order, "bt601")
    assert report == dict(cycles=4, positions=[0, 0, 4, 0, 0], not_duplicates=0) and field_report["deinterlaced"] == 3
    sizes = {}
    for chunk in (1, 2, 4, 5, 7, 23, 30):
        src = decimate_source(cli, tmp_path, fmt, pix, order, chunk, match=dict(thr=THR, mi=MI), decimate=dict(dup=DUP))
        assert src.fps == Fraction(24000, 1001) and isinstance(src.fps, Fraction)
        assert src.match == dict(thr=THR, mi=MI) and src.decimate == dict(dup=DUP)
        got = list(src.chunks())
        sizes[chunk] = [c.shape[0] for c in got]
        assert all(c.shape[0] > 0 and c.dtype == torch.float32 and c.shape[1:] == (H_, W_, 3) for c in got), chunk    # nothing is yielded empty
        assert torch.equal(torch.cat(got), want), chunk
        assert src.decimate_stats.report() == report and src.field_stats.report() == field_report, chunk
        assert not src.thread.is_alive() and src.proc.returncode == 0
    # whole cycles only, then the partial cycle as it is; buffers of 7 complete one, one and two cycles; one buffer -> everything
    assert sizes[1] == sizes[2] == sizes[4] == sizes[5] == [4, 4, 4, 4, 3] and sizes[7] == [4, 4, 8, 3] and sizes[23] == sizes[30] == [19], sizes


def test_source_takes_the_defaults_and_other_sources_have_no_decimation(cli, tmp_path):
    dec, fm = sub("decimate"), sub("fieldmatch")
    src = decimate_source(cli, tmp_path, "yuv420p8", "yuv420p", "tff", 5)
    assert src.decimate == dec.DEFAULTS and src.decimate is not dec.DEFAULTS and src.match == fm.DEFAULTS
    assert src.decimate_stats is not None and src.field_stats is not None
    src.close()
    _, ffmpeg = stand_ins(str(tmp_path / "bin"))
    info = dict(width=W_, height=H_, fps=Fraction(25), pix_fmt="yuv420p", color_space=None, color_range=None, has_audio=False)
    for fields in (None, ("tff", "match"), ("tff", "frame")):
        src = cli.FrameSource(ffmpeg, str(tmp_path / "clip_yuv420p8.mkv"), info, 5, fields=fields)
        assert src.decimate_stats is None and src.decimate is None and src.fps == Fraction(25)
        src.close()
    for fields in (("top", "decimate"), ("tff", "decimated")):
        with pytest.raises(ValueError, match="fields must be"):
            cli.FrameSource("ffmpeg", "x.mkv", info, 5, fields=fields)


# ---------------------------------------------------------------------------------------------------------------- command line
def run_main(cli, tmp_path, monkeypatch, chunked, field_order):
    """the 23 yuv420p frames at 25 fps, woven tff, tagged, through the identity "engines" into the stand-in encoder -> (its argv, its
    stdin, the packed clip)"""
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    packed = source_clip("yuv420p8", "tff")
    src, out = tmp_path / "clip.mkv", tmp_path / "out.mp4"
    tagged(src, packed, "yuv420p", W_, H_, field_order=field_order, rate="25/1", color_space="bt709", color_range="tv")
    tail = ["--chunk_size", "5"] if chunked else []
    assert cli.main([str(src), "--video_backend", "ffmpeg", "--output", str(out)] + tail) == 0
    return open(str(out) + ".args").read().split("\n"), out.read_bytes(), packed


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_cli_decimates_a_tagged_source_where_the_switch_is_on_and_says_so_once(identity, tmp_path, monkeypatch, capsys, chunked):
    dec, fm, de, frameio = sub("decimate"), sub("fieldmatch"), sub("deinterlace"), sub("frameio")
    monkeypatch.setattr(dec, "ENABLED", True)
    monkeypatch.setattr(dec, "DEFAULTS", dict(dup=DUP))                        # (the test's own parameters, not the shipped ones)
    monkeypatch.setattr(fm, "DEFAULTS", dict(thr=THR, mi=MI))
    monkeypatch.setattr(fm, "ENABLED", True)                                   # (decimation takes precedence over both)
    monkeypatch.setattr(de, "ENABLED", True)
    argv, piped, packed = run_main(identity, tmp_path, monkeypatch, chunked, "tt")
    want, report, _ = spec_of_the_whole("yuv420p8", "tff", "bt709")
    assert piped == frameio.pack_frames_torch(want, "bgr8").numpy().tobytes() and len(piped) == 19 * H_ * W_ * 3
    assert argv[argv.index("-r") + 1] == "20"
    captured = capsys.readouterr()
    assert "Warning" not in captured.err
    lines = captured.out.splitlines()
    said = [n for n, line in enumerate(lines) if "Decimation" in line]
    matched = [n for n, line in enumerate(lines) if "Field matching" in line]
    assert len(said) == 1 and len(matched) == 1 and said[0] == matched[0] + 1, captured.out
    assert "4 cycles of five frames" in lines[said[0]] and "0 / 0 / 4 / 0 / 0" in lines[said[0]] and "telecined" not in lines[said[0]]
    assert [line.split()[0] for line in calls(str(tmp_path / "bin"))] == ["ffprobe", "ffmpeg", "ffmpeg"]


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_cli_with_the_switch_off_is_todays(identity, tmp_path, monkeypatch, capsys, chunked):
    fin, dec, fm, de, frameio = sub("frameio_in"), sub("decimate"), sub("fieldmatch"), sub("deinterlace"), sub("frameio")
    assert dec.ENABLED is False and fm.ENABLED is False and de.ENABLED is False
    argv, piped, packed = run_main(identity, tmp_path, monkeypatch, chunked, "tt")
    captured = capsys.readouterr()
    lines = [line for line in captured.err.splitlines() if "interlaced" in line]
    assert len(lines) == 1 and lines[0] == ("Warning: the source is tagged interlaced (field_order tt); deinterlacing is off, the frames "
                                            "are upscaled as stored")
    assert "Decimation" not in captured.out and "Field matching" not in captured.out
    today = frameio.pack_frames_torch(fin.unpack_frames_torch(packed, "yuv420p8", T_, H_, W_, 3, "bt709", "tv"), "bgr8").numpy().tobytes()
    assert piped == today and argv[argv.index("-r") + 1] == "25"
    # fieldmatch.ENABLED alone means what it meant
    monkeypatch.setattr(fm, "ENABLED", True)
    monkeypatch.setattr(fm, "DEFAULTS", dict(thr=THR, mi=MI))
    argv1, piped1, _ = run_main(identity, tmp_path, monkeypatch, chunked, "tt")
    matched = fm.field_match_torch(packed, "yuv420p8", T_, H_, W_, 3, "tff", THR, MI)[0]
    assert piped1 == frameio.pack_frames_torch(fin.unpack_frames_torch(matched, "yuv420p8", T_, H_, W_, 3, "bt709", "tv"), "bgr8").numpy().tobytes()
    out = capsys.readouterr().out
    assert argv1 == argv and "Field matching" in out and "Decimation" not in out
    monkeypatch.setattr(fm, "ENABLED", False)
    # a source without an order is today's whatever the switch says: the same bytes and argv, no warning, no summary
    for enabled in (False, True):
        monkeypatch.setattr(dec, "ENABLED", enabled)
        for tag in (None, "progressive"):
            argv2, piped2, _ = run_main(identity, tmp_path, monkeypatch, chunked, tag)
            captured = capsys.readouterr()
            assert argv2 == argv and piped2 == today and "Warning" not in captured.err and "Decimation" not in captured.out


def test_source_fields_precedence_and_the_summary_line(cli, monkeypatch, capsys):
    dec, fm, de = sub("decimate"), sub("fieldmatch"), sub("deinterlace")
    assert cli.source_fields("tt", 0) is None and "Warning" in capsys.readouterr().err
    monkeypatch.setattr(fm, "ENABLED", True)
    assert cli.source_fields("tt", 0) == ("tff", "match")                      # fieldmatch.ENABLED alone: as before
    monkeypatch.setattr(dec, "ENABLED", True)
    assert cli.source_fields("tt", 0) == ("tff", "decimate") and cli.source_fields("bt", 1) == ("bff", "decimate")
    monkeypatch.setattr(fm, "ENABLED", False)
    monkeypatch.setattr(de, "ENABLED", True)
    assert cli.source_fields("bb", 0) == ("bff", "decimate")
    assert cli.source_fields("progressive", 0) is None and cli.source_fields(None, 0) is None and capsys.readouterr().err == ""
    monkeypatch.setattr(dec, "ENABLED", False)
    assert cli.source_fields("bb", 0) == ("bff", de.RATE)
    st = dec.Stats()
    for counts, doubt in (([1, 2, 30, 4, 5, 0], False), ([1, 2, 30, 4, 5, 21], False), ([1, 2, 30, 4, 5, 22], True), ([0, 0, 0, 0, 0, 0], False),
                          ([3, 0, 0, 0, 0, 3], True)):
        st.counts.copy_(torch.tensor(counts))
        line = cli.decimate_summary(st)
        assert line.startswith("Decimation: ") and "\n" not in line and f"{sum(counts[:5])} cycles of five frames" in line
        assert " / ".join(map(str, counts[:5])) in line and f"{counts[5]} of the dropped frames were not duplicates" in line
        assert ("does not look telecined" in line) == doubt, line


# ---------------------------------------------------------------------------------------------------------------- C ABI
p, q, w = Ptr(0), Ptr(1 << 16), Ptr(1 << 17)            # operands 64 KiB apart (a 5-frame 4 x 6 rgb8 clip with C = 3 is 360 bytes)
FMT = "fmt must be SVR_UNPACK_RGB8, SVR_UNPACK_BGR8, SVR_UNPACK_RGB16, SVR_UNPACK_YUV420P8 or SVR_UNPACK_YUV420P10"
# (packed, packed_bytes, before, fmt, T, H, W, C, diff, diff_bytes, stream) -> svr_last_error()
DIFF_ROWS = [
    ((None, 144, None, 0, 2, 4, 6, 3, q, 8, None), "packed is a null pointer"),
    ((p, 144, None, 0, 2, 4, 6, 3, None, 8, None), "diff is a null pointer"),
    ((p, 144, None, 0, 0, 4, 6, 3, q, 8, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, 0, 2, 0, 6, 3, q, 8, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, 0, 2, 4, -1, 3, q, 8, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, 0, 2, 1 << 20, 1 << 20, 3, q, 8, None), "T * H * W must not exceed 2^40 pixels"),
    ((p, 144, None, 5, 2, 4, 6, 3, q, 8, None), FMT),
    ((p, 144, None, -1, 2, 4, 6, 3, q, 8, None), FMT),
    ((p, 144, None, 0, 2, 4, 6, 2, q, 8, None), "C must be 3 or 4"),
    ((p, 144, None, 4, 2, 4, 6, 4, q, 8, None), "C must be 3 for the yuv420p formats"),
    ((p + 1, 288, None, 3, 2, 4, 6, 3, q, 8, None), "packed is not aligned to 2 bytes"),
    ((p, 144, p + 4097, 2, 2, 4, 6, 3, q, 8, None), "before is not aligned to 2 bytes"),
    ((p, 144, None, 0, 2, 4, 6, 3, q + 2, 8, None), "diff is not aligned to 4 bytes"),
    ((p, 143, None, 0, 2, 4, 6, 3, q, 8, None), "packed_bytes is 143, the format needs exactly 144"),
    ((p, 144, None, 3, 2, 4, 6, 3, q, 8, None), "packed_bytes is 144, the format needs exactly 288"),
    ((p, 108, None, 2, 2, 3, 5, 3, q, 7, None), "diff_bytes is 7, int32 [T] needs exactly 8"),
    ((p, 144, None, 0, 2, 4, 6, 3, q, 12, None), "diff_bytes is 12, int32 [T] needs exactly 8"),
    ((p, 144, None, 0, 2, 4, 6, 3, p + 140, 8, None), "diff overlaps packed"),
    ((p + 4, 144, None, 0, 2, 4, 6, 3, p, 8, None), "diff overlaps packed"),
    ((p, 144, q + 4, 0, 2, 4, 6, 3, q, 8, None), "diff overlaps before"),
    ((p, 144, q + (-68), 0, 2, 4, 6, 3, q, 8, None), "diff overlaps before"),
    # two faults: which one is reported
    ((None, 143, None, 9, 0, 4, 6, 3, None, 8, None), "packed is a null pointer"),
    ((p, 143, None, 9, 2, 4, 6, 2, q + 2, 8, None), FMT),
    ((p, 143, None, 0, 2, 4, 6, 3, q + 2, 7, None), "diff is not aligned to 4 bytes"),
    ((p, 143, None, 0, 2, 4, 6, 3, p, 7, None), "packed_bytes is 143, the format needs exactly 144"),
]
# (packed, packed_bytes, diff, diff_bytes, fmt, T, H, W, C, dup, out, out_bytes, drops, stats, stream)
d, m, st = Ptr(3 << 15), Ptr(5 << 15), Ptr(6 << 15)
SELECT_ROWS = [
    ((None, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, None, None, None), "packed is a null pointer"),
    ((p, 360, None, 20, 0, 5, 4, 6, 3, 64, q, 288, None, None, None), "diff is a null pointer"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, None, 288, None, None, None), "out is a null pointer"),
    ((p, 360, d, 20, 0, 0, 4, 6, 3, 64, q, 288, None, None, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 360, d, 20, 0, 5, 1 << 20, 1 << 20, 3, 64, q, 288, None, None, None), "T * H * W must not exceed 2^40 pixels"),
    ((p, 360, d, 20, 7, 5, 4, 6, 3, 64, q, 288, None, None, None), FMT),
    ((p, 360, d, 20, 3, 5, 4, 6, 5, 64, q, 288, None, None, None), "C must be 3 or 4"),
    ((p, 360, d, 20, 2, 5, 4, 6, 4, 64, q, 288, None, None, None), "C must be 3 for the yuv420p formats"),
    ((p + 1, 720, d, 20, 3, 5, 4, 6, 3, 64, q, 576, None, None, None), "packed is not aligned to 2 bytes"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, -1, q, 288, None, None, None), "dup must lie in 0..262144"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 262145, q, 288, None, None, None), "dup must lie in 0..262144"),
    ((p, 720, d, 20, 3, 5, 4, 6, 3, 64, q + 1, 576, None, None, None), "out is not aligned to 2 bytes"),
    ((p, 360, d + 2, 20, 0, 5, 4, 6, 3, 64, q, 288, None, None, None), "diff is not aligned to 4 bytes"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, m + 2, None, None), "drops is not aligned to 4 bytes"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, None, st + 4, None), "stats is not aligned to 8 bytes"),
    ((p, 359, d, 20, 0, 5, 4, 6, 3, 64, q, 288, None, None, None), "packed_bytes is 359, the format needs exactly 360"),
    ((p, 360, d, 16, 0, 5, 4, 6, 3, 64, q, 288, None, None, None), "diff_bytes is 16, int32 [T] needs exactly 20"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 360, None, None, None), "out_bytes is 360, the T - T / 5 frames need exactly 288"),
    ((p, 288, d, 16, 0, 4, 4, 6, 3, 64, q, 216, None, None, None), "out_bytes is 216, the T - T / 5 frames need exactly 288"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, p + 359, 288, None, None, None), "out overlaps packed"),
    ((p, 360, q + 284, 20, 0, 5, 4, 6, 3, 64, q, 288, None, None, None), "out overlaps diff"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, p + 356, None, None), "drops overlaps packed"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, d + 16, None, None), "drops overlaps diff"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, q + 284, None, None), "drops overlaps out"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, None, p + 352, None), "stats overlaps packed"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, None, d + (-40), None), "stats overlaps diff"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, None, q + 280, None), "stats overlaps out"),
    ((p, 360, d, 20, 0, 5, 4, 6, 3, 64, q, 288, m, m, None), "stats overlaps drops"),
    # two faults: which one is reported
    ((p, 359, None, 20, 9, 5, 4, 6, 3, -6, q, 288, None, None, None), "diff is a null pointer"),
    ((p, 359, d, 20, 0, 5, 4, 6, 3, -6, q, 288, m + 2, None, None), "dup must lie in 0..262144"),
    ((p, 359, d, 21, 0, 5, 4, 6, 3, 64, p, 288, None, None, None), "packed_bytes is 359, the format needs exactly 360"),
]


def test_every_refusal_message_of_the_entry_points_is_exact():
    """Every argument is validated on the host before anything is enqueued, so a host buffer stands in for device memory."""
    L = sub("hip_lib").lib()
    for fn, rows in (("svr_frame_diffs", DIFF_ROWS), ("svr_decimate_select", SELECT_ROWS)):
        for args, message in rows:
            assert L.svr_set_option(b"no_such_key", 0) != 0         # (a known message first: an accepted call would leave it standing)
            assert call(L, fn, args) == -1, (fn, args)
            assert L.svr_last_error().decode() == f"{fn}: {message}", (fn, args)


def test_header_ctypes_table_and_build_list_know_the_entry_points():
    hip_lib = sub("hip_lib")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert {"svr_frame_diffs", "svr_decimate_select"} <= declared and declared == set(hip_lib.SYMBOLS)
    for fn, n in (("svr_frame_diffs", 11), ("svr_decimate_select", 15)):
        decl = re.search(rf"int {fn}\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == n == len(hip_lib.SYMBOLS[fn][1]), fn
        assert re.search(rf"^ \*   {fn}\s+\S", src, flags=re.M), fn                                   # the operand-layout table
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert re.search(r"v9, additive: \+ svr_frame_diffs\(\) / svr_decimate_select\(\).*?New symbols only", src, flags=re.S)
    api = open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert '#include "svr_decimate.hip"' in api and api.index('#include "svr_fieldmatch.hip"') < api.index('#include "svr_decimate.hip"')
    assert os.path.join(hip_lib.CSRC, "svr_decimate.hip") in hip_lib.sources()            # (the loader's source hash covers it)
    lib = hip_lib.lib()
    assert lib.svr_abi_version() == 9 and hasattr(lib, "svr_frame_diffs") and hasattr(lib, "svr_decimate_select")
    ops = sub("ops")
    assert hasattr(ops.HipOps, "frame_diffs") and hasattr(ops.HipOps, "decimate_select")
    from ops_reference import TorchOps
    assert not hasattr(TorchOps, "frame_diffs") and not hasattr(TorchOps, "decimate_select")              # as with field matching
