"""-m "not gpu": field matching (fieldmatch.py, the specification of csrc/svr_fieldmatch.hip) -- the torch statements against a
per-sample restatement of the text, value cases, the properties (a progressive clip and a telecined clip come back bit for bit, an
interlaced clip comes back deinterlaced, a static clip as stored, a wrong order is contradicted by the two sums), the mode rule on
crafted counts --, the command line's reader behind FrameSource(fields=(order, "match")) and the fieldmatch.ENABLED switch against
stand-ins for the two executables, and the C ABI's refusals.  NOT covered anywhere: a real ffmpeg, real footage."""
import os
import re
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from fieldmatch_cases import (CONTEXTS, FORMATS, GEOMETRIES, MI, ORDERS, SHAPES, SHIFT, THR, channel_counts, context, crafted_counts,
                              cut_planes, interlace, loop_comb_counts, loop_counts, loop_modes, loop_select, packed_clip, pictures,
                              random_packed, telecine)
from frame_unpack_cases import calls, fake_video, stand_ins
from test_deinterlace import tagged
from test_frame_unpack import identity  # noqa: F401 (fixture)
from test_refusal_messages import Ptr, call
from test_stream import cli, rig  # noqa: F401 (fixtures)


def step(fmt, C):
    return 1 if fmt in ("yuv420p8", "yuv420p10") else C


# ---------------------------------------------------------------------------------------------------------------- specification
def test_module_surface_and_the_shipped_switch():
    fm, de = sub("fieldmatch"), sub("deinterlace")
    assert fm.ENABLED is False and fm.RATE == "match" and fm.DEFAULTS == dict(thr=10, mi=24) and fm.BLOCK == 16
    assert de.RATES == ("frame", "field") and fm.RATE not in de.RATES and fm.ORDERS == de.ORDERS
    for word in ("SYNTHETIC", "No test depends on", "no decimation", "tagged progressive", "plane 0 decides", "noise above thr",
                 "reported, not corrected", "one order per clip", "tie between the neighbours", "AGREES", "CONTRADICTS"):
        assert word.lower() in fm.__doc__.lower(), word
    assert "fieldmatch" in de.__doc__
    st = fm.Stats()
    assert st.counts.dtype == torch.int64 and tuple(st.counts.shape) == (6,) and not st.counts.any()
    assert st.report() == dict(stored=0, prev=0, next=0, deinterlaced=0, sum_prev=0, sum_next=0, verdict="says nothing about")
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"fieldmatch"' in entry


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_equals_the_loop_restatement(shape, fmt):
    """Random clips over the whole code range (nearly every sample combed at a small thr, few at a large one): counts, modes and
    select, for every channel count, both orders and every kind of context.  Select is also fed modes that walk through 0..3,
    whatever the counts say."""
    fm, de = sub("fieldmatch"), sub("deinterlace")
    T, H, W = shape
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        s = step(fmt, C)
        assert de.planes(fmt, H, W, C)[0][3] == s
        for n, kind in enumerate(CONTEXTS):
            before, after = context(kind, fmt, H, W, C, seed=n)
            for order in ORDERS:
                thr = (3, 90, 200, 40)[n]
                got = fm.comb_counts_torch(packed, fmt, T, H, W, C, order, thr, before, after)
                want = loop_comb_counts(packed, fmt, T, H, W, C, order, thr, before, after)
                assert got.dtype == torch.int32 and tuple(got.shape) == (T, 3, 2) and torch.equal(got, want), (C, kind, order)
                mi = int(want[:, :, 1].max()) // (2 * s)                       # (a bound that splits the peaks the clip has)
                modes = fm.modes_torch(got, mi, s)
                assert modes.dtype == torch.int32 and modes.tolist() == loop_modes(want.tolist(), mi, s), (C, kind, order)
                deint = de.deinterlace_torch(packed, fmt, T, H, W, C, order, "frame", before, after)
                for m in (modes, torch.tensor([(t + n) % 4 for t in range(T)], dtype=torch.int32)):
                    out = fm.select_torch(packed, deint, m, fmt, T, H, W, C, order, before, after)
                    assert out.dtype == packed.dtype and out.shape == packed.shape and out.is_contiguous()
                    assert torch.equal(out, loop_select(packed, deint, m.tolist(), fmt, T, H, W, C, order, before, after)), (C, kind, order)
                frames, modes2, cnt2 = fm.field_match_torch(packed, fmt, T, H, W, C, order, thr, mi, before, after)
                assert torch.equal(cnt2, got) and torch.equal(modes2, modes)
                assert torch.equal(frames, fm.select_torch(packed, deint, modes, fmt, T, H, W, C, order, before, after))


def test_planes_without_a_tested_row_count_nothing():
    fm = sub("fieldmatch")
    for fmt, (T, H, W) in (("rgb8", (2, 2, 9)), ("yuv420p10", (2, 2, 9)), ("rgb16", (3, 1, 8)), ("yuv420p8", (1, 1, 16))):
        packed = random_packed(fmt, T, H, W, 3, seed=1)
        for order in ORDERS:
            cnt = fm.comb_counts_torch(packed, fmt, T, H, W, 3, order, 0)
            assert not cnt.any() and fm.modes_torch(cnt, 0, 1).tolist() == [0] * T
            frames, _, _ = fm.field_match_torch(packed, fmt, T, H, W, 3, order, 0, 0)
            assert torch.equal(frames, packed)
    # three rows: "tff" tests row 1, "bff" has none (row 2 has no row below it)
    packed = random_packed("yuv420p8", 2, 3, 5, 3, seed=2)
    assert fm.comb_counts_torch(packed, "yuv420p8", 2, 3, 5, 3, "tff", 0).any()
    assert not fm.comb_counts_torch(packed, "yuv420p8", 2, 3, 5, 3, "bff", 0).any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_value_cases_thresholds_and_the_ends_of_the_code_range(fmt):
    """One tested row (H = 3, "tff") of hand-made samples: u and l at the ends of the container's range, m exactly at, and one code
    beyond, min(u, l) - thr' and max(u, l) + thr'; thr in {0, 12, 255}.  10-bit samples above 1023 are used as stored."""
    fm = sub("fieldmatch")
    top = 255 if SHIFT[fmt] == 0 else 65535
    H, W, C = 3, 16, 3
    s = step(fmt, C)
    N = W * s
    for thr in (0, 12, 255):
        t_ = thr << SHIFT[fmt]
        # per sample (u, l, m, combed)
        cases = [(0, 0, 0, False), (top, top, top, False), (0, top, top // 2, False), (top, 0, 0, False)]
        if t_ < top:
            cases += [(0, 0, t_, False), (0, 0, t_ + 1, True), (top, top, top - t_, False), (top, top, top - t_ - 1, True),
                      (t_, top, 0, False), (t_ + 1, top, 0, True)]
        if fmt == "yuv420p10":
            cases += [(1023, 1023, 1023 + t_, False), (1023, 1023, 1024 + t_, True), (2000, 3000, 3001 + t_, True), (2000, 3000, 3000 + t_, False)]
        cases = (cases * N)[:N]
        frame = torch.tensor([[c[0] for c in cases], [c[2] for c in cases], [c[1] for c in cases]], dtype=torch.int64)
        numel = random_packed(fmt, 1, H, W, C, seed=0).numel()
        flat = torch.zeros(numel, dtype=torch.int64)
        flat[:3 * N] = frame.reshape(-1)
        packed = flat.to(torch.uint16 if SHIFT[fmt] else torch.uint8).reshape(random_packed(fmt, 1, H, W, C, seed=0).shape)
        cnt = fm.comb_counts_torch(packed, fmt, 1, H, W, C, "tff", thr)
        want = sum(c[3] for c in cases)
        assert cnt[0, 0].tolist() == [want, want] and (want > 0 or thr == 255), (fmt, thr)    # (W = 16 pixels: one block)
        assert cnt[0, 1].tolist() == cnt[0, 0].tolist() == cnt[0, 2].tolist()                 # (a one-frame clip is its own neighbour)
        assert torch.equal(cnt, loop_comb_counts(packed, fmt, 1, H, W, C, "tff", thr))


def test_mode_rule_on_crafted_counts():
    fm = sub("fieldmatch")
    for s in (1, 3, 4):
        for mi in (0, 6, 24):
            b = mi * s
            rows = [((b, 999, 999), 0), ((b + 1, 999, 999), 3), ((0, 0, 0), 0), ((b + 1, b, b), 1), ((b + 1, b + 1, b + 1), 3),
                    ((b + 1, b, b + 1), 1), ((b + 1, b + 1, b), 2), ((b + 1, b + 5, b + 2), 3), ((b + 1, 0, 0), 1), ((b + 1, 1, 0), 2),
                    ((b + 1, b, b + 900), 1), ((b + 1, b + 900, b), 2)]
            cnt = torch.zeros(len(rows), 3, 2, dtype=torch.int32)
            for t, (peaks, _) in enumerate(rows):
                cnt[t, :, 1] = torch.tensor(peaks, dtype=torch.int32)
                cnt[t, :, 0] = 7777                                            # (the totals decide nothing)
            assert fm.modes_torch(cnt, mi, s).tolist() == [m for _, m in rows] == loop_modes(cnt.tolist(), mi, s), (s, mi)
        cnt, modes = crafted_counts(9, 5, s)
        assert fm.modes_torch(cnt, 5, s).tolist() == modes == loop_modes(cnt.tolist(), 5, s) and set(modes) == {0, 1, 2, 3}
    for bad in (-1, 1.5, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="mi must be a non-negative integer"):
            fm.modes_torch(torch.zeros(1, 3, 2, dtype=torch.int32), bad, 1)
    with pytest.raises(ValueError, match="cnt must be torch.int32"):
        fm.modes_torch(torch.zeros(1, 3, 2, dtype=torch.int64), 1, 1)


# ---------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("R,N,speed", GEOMETRIES)
def test_geometry_progressive_peaks_lie_under_the_bound_and_mixed_peaks_over_it(R, N, speed):
    """With the restatement alone (s = 1): every stored progressive picture has peak <= MI, every mixed frame peak > MI."""
    for order in ORDERS:
        P = pictures(8, R, N, speed, seed=R)
        frames, src = telecine(P, order)
        cnt = loop_counts(frames.tolist(), R, N, 1, order, THR)
        mixed = [t for t in range(10) if t % 5 in (2, 3)]
        print(order, [c[0][1] for c in cnt])
        assert src == [0, 1, 1, 2, 3, 4, 5, 5, 6, 7]
        assert all((cnt[t][0][1] > MI) == (t in mixed) for t in range(10)), cnt
        assert all(c[0][1] <= MI for c in loop_counts(P.tolist(), R, N, 1, order, THR))
        woven = interlace(pictures(12, R, N, speed, seed=R + 1), order)
        assert all(min(c[k][1] for k in range(3)) > MI for c in loop_counts(woven.tolist(), R, N, 1, order, THR))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("R,N,speed", GEOMETRIES)
def test_progressive_telecined_interlaced_and_static_clips(R, N, speed, fmt):
    fm, de = sub("fieldmatch"), sub("deinterlace")
    for order in ORDERS:
        P = pictures(8, R, N, speed, seed=N)
        # progressive: bit-identical, all modes 0
        prog = packed_clip(P, fmt)
        out, modes, _ = fm.field_match_torch(prog, fmt, 8, R, N, 3, order, THR, MI)
        assert torch.equal(out, prog) and modes.tolist() == [0] * 8, (order, "progressive")
        # telecined: every frame comes back as the picture its first field shows, nothing is deinterlaced
        src = telecine(P, order)[1]
        tele = packed_clip(P, fmt, lambda pl: telecine(pl, order)[0])
        out, modes, _ = fm.field_match_torch(tele, fmt, 10, R, N, 3, order, THR, MI)
        assert modes.tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 1, 0] and 3 not in modes.tolist(), (order, modes.tolist())
        for t in range(10):
            assert torch.equal(out[t], prog[src[t]]), (order, t)
        # interlaced, motion in every frame: the deinterlaced clip, all modes 3
        G = pictures(24, R, N, speed, seed=N + 1)
        woven = packed_clip(G, fmt, lambda pl: interlace(pl, order))
        out, modes, _ = fm.field_match_torch(woven, fmt, 12, R, N, 3, order, THR, MI)
        assert modes.tolist() == [3] * 12 and torch.equal(out, de.deinterlace_torch(woven, fmt, 12, R, N, 3, order, "frame")), order
        # ... read with the WRONG order: the previous frame's other field is three field times away, the next frame's one
        other = ORDERS[1 - ORDERS.index(order)]
        right, wrong = fm.Stats(), fm.Stats()
        fm.field_match(woven, fmt, 12, R, N, 3, order, THR, MI, stats=right)
        fm.field_match(woven, fmt, 12, R, N, 3, other, THR, MI, stats=wrong)
        r, w = right.report(), wrong.report()
        print(fmt, order, r, w)
        assert r["deinterlaced"] == 12 and r["sum_prev"] < r["sum_next"] and r["verdict"] == "agrees with"
        assert w["deinterlaced"] > 0 and w["sum_prev"] > w["sum_next"] and w["verdict"] == "contradicts"
        # static: as stored, whatever the picture holds
        image = random_packed(fmt, 1, R, N, 3, seed=R)
        still = image.expand(4, *image.shape[1:]).contiguous()
        assert torch.equal(fm.field_match_torch(still, fmt, 4, R, N, 3, order, THR, MI)[0], still), (order, "static")


def test_any_split_with_its_true_neighbours_equals_the_whole():
    fm = sub("fieldmatch")
    fmt, R, N = "yuv420p8", 18, 40
    P = pictures(12, R, N, 2, seed=5)
    clip = torch.cat([packed_clip(P[:8], fmt, lambda pl: telecine(pl, "tff")[0]), packed_clip(P[8:], fmt, lambda pl: interlace(pl, "tff"))])
    T = clip.shape[0]
    whole, modes, _ = fm.field_match_torch(clip, fmt, T, R, N, 3, "tff", THR, MI)
    assert {0, 1, 3} <= set(modes.tolist())
    for cuts in ((3, 5), (2,), tuple(range(1, T)), (T - 1,)):
        edges = [0, *cuts, T]
        parts = []
        for a, b in zip(edges[:-1], edges[1:]):
            before = clip[a - 1] if a > 0 else (clip[1] if b - a == 1 else None)
            after = clip[b] if b < T else (clip[T - 2] if b - a == 1 else None)
            parts.append(fm.field_match_torch(clip[a:b].contiguous(), fmt, b - a, R, N, 3, "tff", THR, MI, before, after)[0])
        assert torch.equal(torch.cat(parts), whole), cuts


def test_arguments_are_refused_by_name_and_the_front_composes_the_steps():
    fm, de = sub("fieldmatch"), sub("deinterlace")
    packed = random_packed("rgb8", 2, 4, 6, 3, seed=0)
    ok = dict(packed=packed, fmt="rgb8", T=2, H=4, W=6, C=3, order="tff", thr=12)
    for change, word in ((dict(fmt="rgb10"), "fmt must be"), (dict(C=2), "C = 3 or 4"), (dict(order="top"), "order must be one of"),
                         (dict(T=0, packed=packed[:0]), "T, H, W must be positive"), (dict(packed=packed.to(torch.int16)), "packed must be torch.uint8"),
                         (dict(W=7), "packed must hold 168 samples"), (dict(before=packed), "before must hold the 72 samples of one rgb8 frame"),
                         (dict(after=packed[0].to(torch.int32)), "after must be torch.uint8"), (dict(fmt="yuv420p8", C=4), "yuv420p8 takes C = 3"),
                         (dict(thr=-1), "thr must be an integer in 0..255"), (dict(thr=256), "thr must be an integer in 0..255"),
                         (dict(thr=1.0), "thr must be an integer in 0..255")):
        with pytest.raises(ValueError, match=re.escape(word)):
            fm.comb_counts_torch(**{**ok, **change})
        with pytest.raises(ValueError, match=re.escape(word)):
            fm.field_match(**{**ok, **change}, mi=3)
    big = torch.empty(1, 1, 1, 1, dtype=torch.uint8)                            # (expanded: a view, no memory)
    with pytest.raises(ValueError, match=re.escape("H * W * C must not exceed 2^31 samples (the counters are int32)")):
        fm.check_arguments(big.expand(1, 2 ** 15, 2 ** 15, 3), "rgb8", 1, 2 ** 15, 2 ** 15, 3, "tff", 12)
    with pytest.raises(ValueError, match="mi must be a non-negative integer"):
        fm.field_match(**ok, mi=-1)
    deint = de.deinterlace_torch(packed, "rgb8", 2, 4, 6, 3, "tff", "frame")
    with pytest.raises(ValueError, match="modes must be torch.int32"):
        fm.select_torch(packed, deint, torch.zeros(2, dtype=torch.int64), "rgb8", 2, 4, 6, 3, "tff")
    with pytest.raises(ValueError, match="deint must be torch.uint8"):
        fm.select_torch(packed, deint[:1], torch.zeros(2, dtype=torch.int32), "rgb8", 2, 4, 6, 3, "tff")
    # the front: the torch statements without ops, ``out`` checked and filled, ``stats`` added to
    want, modes, cnt = fm.field_match_torch(**ok, mi=3)
    out, st = torch.empty_like(want), fm.Stats()
    assert fm.field_match(**ok, mi=3, out=out, stats=st) is out and torch.equal(out, want) and torch.equal(fm.field_match(**ok, mi=3), want)
    fm.field_match(**ok, mi=3, stats=st)
    m = modes.tolist()
    sums = [2 * sum(int(cnt[t, k, 0]) for t in range(2) if m[t] == 3) for k in (1, 2)]
    assert st.counts.tolist() == [2 * m.count(v) for v in range(4)] + sums
    with pytest.raises(ValueError, match="out must be"):
        fm.field_match(**ok, mi=3, out=torch.empty(2, 4, 6, 4, dtype=torch.uint8))

    # a backend that has the two ops is used -- and handed the deinterlaced clip, the counts and the stats tensor; one that fails raises
    class Double:
        def __init__(self):
            self.seen = []

        def comb_counts(self, packed, fmt, T, H, W, C, order, thr, before=None, after=None):
            self.seen.append("comb_counts")
            return fm.comb_counts_torch(packed, fmt, T, H, W, C, order, thr, before, after)

        def field_select(self, packed, deint, cnt, fmt, T, H, W, C, order, mi, before=None, after=None, out=None, modes=None, stats=None):
            self.seen.append("field_select")
            assert torch.equal(deint, de.deinterlace_torch(packed, fmt, T, H, W, C, order, "frame", before, after)) and stats is st2.counts
            return fm.select_torch(packed, deint, fm.modes_torch(cnt, mi, 3), fmt, T, H, W, C, order, before, after)

    double, st2 = Double(), fm.Stats()
    assert torch.equal(fm.field_match(**ok, mi=3, ops=double, stats=st2), want) and double.seen == ["comb_counts", "field_select"]

    class Failing(Double):
        def comb_counts(self, *a, **kw):
            raise RuntimeError("library failed")

    with pytest.raises(RuntimeError, match="library failed"):
        fm.field_match(**ok, mi=3, ops=Failing())


# ---------------------------------------------------------------------------------------------------------------- reader
def match_source(cli, tmp_path, fmt, pix, order, chunk, match=None, R=18, N=40):
    """a 13-frame clip of the property geometry -- 10 telecined frames, then 3 interlaced ones -- behind the stand-in ffmpeg"""
    _, ffmpeg = stand_ins(str(tmp_path / "bin"))
    clip = tmp_path / f"clip_{fmt}.mkv"
    P = pictures(14, R, N, 2, seed=3)
    packed = torch.cat([packed_clip(P[:8], fmt, lambda pl: telecine(pl, order)[0]), packed_clip(P[8:], fmt, lambda pl: interlace(pl, order))])
    fake_video(clip, packed, pix, N, R)
    info = dict(width=N, height=R, fps=Fraction(30000, 1001), pix_fmt=pix, color_space=None, color_range=None, has_audio=False)
    return cli.FrameSource(ffmpeg, str(clip), info, chunk, fields=(order, "match"), match=match), packed, clip


@pytest.mark.parametrize("fmt,pix", [("yuv420p10", "yuv420p10le"), ("yuv420p8", "yuv420p"), ("rgb8", "rgb24")])
@pytest.mark.parametrize("order", ORDERS)
def test_source_chunks_equal_the_specification_applied_to_the_whole_clip(cli, tmp_path, fmt, pix, order):
    fin, fm = sub("frameio_in"), sub("fieldmatch")
    src, packed, clip = match_source(cli, tmp_path, fmt, pix, order, 5, dict(thr=THR, mi=MI))
    assert src.fps == Fraction(30000, 1001) and isinstance(src.fps, Fraction) and src.match == dict(thr=THR, mi=MI)
    got = list(src.chunks())
    assert [c.shape[0] for c in got] == [5, 5, 3] and all(c.dtype == torch.float32 and c.shape[1:] == (18, 40, 3) for c in got)
    frames, modes, cnt = fm.field_match_torch(packed, fmt, 13, 18, 40, 3, order, THR, MI)
    assert modes.tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 3, 3, 3]
    want = fin.unpack_frames_torch(frames, fmt, 13, 18, 40, 3, "bt601", "tv")
    assert torch.equal(torch.cat(got), want)
    whole = fm.Stats()
    whole.add(modes, cnt)
    assert src.field_stats.report() == whole.report() and whole.report()["deinterlaced"] == 3
    argv = open(str(clip) + ".args").read().split("\n")
    assert argv == ["-loglevel", "error", "-noautorotate", "-i", str(clip), "-map", "0:v:0", "-f", "rawvideo", "-pix_fmt", pix, "-"]
    assert not src.thread.is_alive() and src.proc.returncode == 0
    for chunk in (1, 4, 13, 20):
        src, _, _ = match_source(cli, tmp_path, fmt, pix, order, chunk, dict(thr=THR, mi=MI))
        assert torch.equal(torch.cat(list(src.chunks())), want), chunk
        assert src.field_stats.report() == whole.report(), chunk


def test_source_takes_the_defaults_where_no_parameters_are_given_and_refuses_other_rates(cli, tmp_path):
    fm = sub("fieldmatch")
    src, _, _ = match_source(cli, tmp_path, "yuv420p8", "yuv420p", "tff", 5)
    assert src.match == fm.DEFAULTS and src.match is not fm.DEFAULTS and src.field_stats is not None
    src.close()
    info = dict(width=2, height=2, fps=Fraction(24), pix_fmt="yuv420p")
    for fields in (("top", "match"), ("tff", "matched"), ("tff", "double")):
        with pytest.raises(ValueError, match="fields must be"):
            cli.FrameSource("ffmpeg", "x.mkv", info, 5, fields=fields)


# ---------------------------------------------------------------------------------------------------------------- command line
T_, H_, W_ = 13, 18, 40


def run_main(cli, tmp_path, monkeypatch, chunked, field_order):
    """13 yuv420p frames of 18 x 40 at 25 fps (10 telecined, 3 interlaced, woven tff), tagged, through the identity "engines" into the
    stand-in encoder -> (its argv, its stdin, the packed clip)"""
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    P = pictures(14, H_, W_, 2, seed=3)
    packed = torch.cat([packed_clip(P[:8], "yuv420p8", lambda pl: telecine(pl, "tff")[0]),
                        packed_clip(P[8:], "yuv420p8", lambda pl: interlace(pl, "tff"))])
    src, out = tmp_path / "clip.mkv", tmp_path / "out.mp4"
    tagged(src, packed, "yuv420p", W_, H_, field_order=field_order, rate="25/1", color_space="bt709", color_range="tv")
    tail = ["--chunk_size", "5"] if chunked else []
    assert cli.main([str(src), "--video_backend", "ffmpeg", "--output", str(out)] + tail) == 0
    return open(str(out) + ".args").read().split("\n"), out.read_bytes(), packed


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_cli_matches_a_tagged_source_where_the_switch_is_on_and_says_so_once(identity, tmp_path, monkeypatch, capsys, chunked):
    fin, fm, de, frameio = sub("frameio_in"), sub("fieldmatch"), sub("deinterlace"), sub("frameio")
    monkeypatch.setattr(fm, "ENABLED", True)
    monkeypatch.setattr(fm, "DEFAULTS", dict(thr=THR, mi=MI))                  # (the test's own parameters, not the shipped ones)
    monkeypatch.setattr(de, "ENABLED", True)                                   # (field matching takes precedence)
    argv, piped, packed = run_main(identity, tmp_path, monkeypatch, chunked, "tt")
    frames, modes, _ = fm.field_match_torch(packed, "yuv420p8", T_, H_, W_, 3, "tff", THR, MI)
    want = fin.unpack_frames_torch(frames, "yuv420p8", T_, H_, W_, 3, "bt709", "tv")
    assert piped == frameio.pack_frames_torch(want, "bgr8").numpy().tobytes() and len(piped) == T_ * H_ * W_ * 3
    assert argv[argv.index("-r") + 1] == "25"
    captured = capsys.readouterr()
    assert "Warning" not in captured.err
    lines = [line for line in captured.out.splitlines() if "Field matching" in line]
    assert len(lines) == 1, captured.out
    n = [modes.tolist().count(v) for v in range(4)]
    assert n[0] > 0 and n[1] > 0 and n[3] > 0 and sum(n) == T_
    assert f"(tff): {n[0]} frames as stored, {n[1]} matched to the previous frame, {n[2]} matched to the next, {n[3]} deinterlaced" in lines[0]
    assert "agrees with the field_order tag" in lines[0]
    assert [line.split()[0] for line in calls(str(tmp_path / "bin"))] == ["ffprobe", "ffmpeg", "ffmpeg"]


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_cli_with_the_switch_off_is_todays(identity, tmp_path, monkeypatch, capsys, chunked):
    fin, fm, de, frameio = sub("frameio_in"), sub("fieldmatch"), sub("deinterlace"), sub("frameio")
    assert fm.ENABLED is False and de.ENABLED is False
    argv, piped, packed = run_main(identity, tmp_path, monkeypatch, chunked, "tt")
    captured = capsys.readouterr()
    lines = [line for line in captured.err.splitlines() if "interlaced" in line]
    assert len(lines) == 1 and lines[0] == ("Warning: the source is tagged interlaced (field_order tt); deinterlacing is off, the frames "
                                            "are upscaled as stored")
    assert "Field matching" not in captured.out
    today = frameio.pack_frames_torch(fin.unpack_frames_torch(packed, "yuv420p8", T_, H_, W_, 3, "bt709", "tv"), "bgr8").numpy().tobytes()
    assert piped == today and argv[argv.index("-r") + 1] == "25"
    # deinterlace.ENABLED alone means what it meant
    monkeypatch.setattr(de, "ENABLED", True)
    argv1, piped1, _ = run_main(identity, tmp_path, monkeypatch, chunked, "tt")
    fields = fin.unpack_frames_torch(de.deinterlace_torch(packed, "yuv420p8", T_, H_, W_, 3, "tff", "field"), "yuv420p8", 2 * T_, H_, W_, 3,
                                     "bt709", "tv")
    assert piped1 == frameio.pack_frames_torch(fields, "bgr8").numpy().tobytes() and argv1[argv1.index("-r") + 1] == "50"
    assert "Field matching" not in capsys.readouterr().out
    monkeypatch.setattr(de, "ENABLED", False)
    # a source without an order is today's either way: the same bytes and argv, no warning, no summary
    for enabled in (False, True):
        monkeypatch.setattr(fm, "ENABLED", enabled)
        for tag in (None, "progressive"):
            argv2, piped2, _ = run_main(identity, tmp_path, monkeypatch, chunked, tag)
            captured = capsys.readouterr()
            assert argv2 == argv and piped2 == today and "Warning" not in captured.err and "Field matching" not in captured.out


def test_source_fields_and_the_summary_line(cli, monkeypatch, capsys):
    fm, de = sub("fieldmatch"), sub("deinterlace")
    assert cli.source_fields("tt", 0) is None and "Warning" in capsys.readouterr().err
    monkeypatch.setattr(fm, "ENABLED", True)
    assert cli.source_fields("tt", 0) == ("tff", "match") and cli.source_fields("bt", 1) == ("bff", "match")
    assert cli.source_fields("progressive", 0) is None and cli.source_fields(None, 0) is None and capsys.readouterr().err == ""
    monkeypatch.setattr(fm, "ENABLED", False)
    monkeypatch.setattr(de, "ENABLED", True)
    assert cli.source_fields("bb", 0) == ("bff", de.RATE)
    st = fm.Stats()
    for counts, word in (([4, 3, 2, 1, 10, 20], "agrees with"), ([4, 3, 2, 1, 20, 10], "contradicts"), ([9, 1, 0, 0, 0, 0], "says nothing about")):
        st.counts.copy_(torch.tensor(counts))
        line = cli.field_summary(st, "bff")
        assert f"{counts[0]} frames as stored, {counts[1]} matched to the previous frame, {counts[2]} matched to the next, {counts[3]} deinterlaced" in line
        assert f"{counts[4]} : {counts[5]}" in line and f"which {word} the field_order tag" in line and "(bff)" in line and "\n" not in line


# ---------------------------------------------------------------------------------------------------------------- C ABI
p, q, w = Ptr(0), Ptr(1 << 16), Ptr(1 << 17)            # three operands 64 KiB apart (a 2-frame 4 x 6 rgb8 clip with C = 3 is 144 bytes)
FMT = "fmt must be SVR_UNPACK_RGB8, SVR_UNPACK_BGR8, SVR_UNPACK_RGB16, SVR_UNPACK_YUV420P8 or SVR_UNPACK_YUV420P10"
# (packed, packed_bytes, before, after, fmt, T, H, W, C, order, thr, cnt, cnt_bytes, stream) -> svr_last_error()
COMB_ROWS = [
    ((None, 144, None, None, 0, 2, 4, 6, 3, 0, 12, q, 48, None), "packed is a null pointer"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 12, None, 48, None), "cnt is a null pointer"),
    ((p, 144, None, None, 0, 0, 4, 6, 3, 0, 12, q, 48, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, None, 0, 2, 0, 6, 3, 0, 12, q, 48, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, None, 0, 2, 4, -1, 3, 0, 12, q, 48, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, None, 0, 2, 1 << 20, 1 << 20, 3, 0, 12, q, 48, None), "T * H * W must not exceed 2^40 pixels"),
    ((p, 144, None, None, 5, 2, 4, 6, 3, 0, 12, q, 48, None), FMT),
    ((p, 144, None, None, -1, 2, 4, 6, 3, 0, 12, q, 48, None), FMT),
    ((p, 144, None, None, 0, 2, 4, 6, 2, 0, 12, q, 48, None), "C must be 3 or 4"),
    ((p, 144, None, None, 4, 2, 4, 6, 4, 0, 12, q, 48, None), "C must be 3 for the yuv420p formats"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 2, 12, q, 48, None), "order must be SVR_FIELD_TFF or SVR_FIELD_BFF"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, -1, 12, q, 48, None), "order must be SVR_FIELD_TFF or SVR_FIELD_BFF"),
    ((p + 1, 288, None, None, 3, 2, 4, 6, 3, 0, 12, q, 48, None), "packed is not aligned to 2 bytes"),
    ((p, 144, p + 4097, None, 2, 2, 4, 6, 3, 0, 12, q, 48, None), "before is not aligned to 2 bytes"),
    ((p, 144, None, p + 4097, 2, 2, 4, 6, 3, 0, 12, q, 48, None), "after is not aligned to 2 bytes"),
    ((p, 144, None, None, 0, 1, 1 << 15, 1 << 15, 3, 0, 12, q, 24, None), "H * W * C must not exceed 2^31 samples (the counters are int32)"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, -1, q, 48, None), "thr must lie in 0..255"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 256, q, 48, None), "thr must lie in 0..255"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 12, q + 2, 48, None), "cnt is not aligned to 4 bytes"),
    ((p, 143, None, None, 0, 2, 4, 6, 3, 0, 12, q, 48, None), "packed_bytes is 143, the format needs exactly 144"),
    ((p, 144, None, None, 3, 2, 4, 6, 3, 0, 12, q, 48, None), "packed_bytes is 144, the format needs exactly 288"),
    ((p, 108, None, None, 2, 2, 3, 5, 3, 0, 12, q, 47, None), "cnt_bytes is 47, int32 [T, 3, 2] needs exactly 48"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 12, q, 24, None), "cnt_bytes is 24, int32 [T, 3, 2] needs exactly 48"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 1, 12, p + 140, 48, None), "cnt overlaps packed"),
    ((p + 44, 144, None, None, 0, 2, 4, 6, 3, 1, 12, p, 48, None), "cnt overlaps packed"),
    ((p, 144, q + 44, None, 0, 2, 4, 6, 3, 0, 12, q, 48, None), "cnt overlaps before"),
    ((p, 144, None, q + (-68), 0, 2, 4, 6, 3, 0, 12, q, 48, None), "cnt overlaps after"),
    # two faults: which one is reported
    ((None, 143, None, None, 9, 0, 4, 6, 3, 0, 999, None, 48, None), "packed is a null pointer"),
    ((p, 143, None, None, 9, 2, 4, 6, 3, 7, 999, q, 48, None), FMT),
    ((p, 143, None, None, 0, 2, 4, 6, 3, 0, 999, q, 47, None), "thr must lie in 0..255"),
    ((p, 143, None, None, 0, 2, 4, 6, 3, 0, 12, p, 47, None), "packed_bytes is 143, the format needs exactly 144"),
]
# (packed, packed_bytes, before, after, deint, deint_bytes, cnt, cnt_bytes, fmt, T, H, W, C, order, mi, out, out_bytes, modes, stats, stream)
d, c, m, st = Ptr(1 << 15), Ptr(3 << 15), Ptr(5 << 15), Ptr(6 << 15)
SELECT_ROWS = [
    ((None, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "packed is a null pointer"),
    ((p, 144, None, None, None, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "deint is a null pointer"),
    ((p, 144, None, None, d, 144, None, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "cnt is a null pointer"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, None, 144, None, None, None), "out is a null pointer"),
    ((p, 144, None, None, d, 144, c, 48, 0, 0, 4, 6, 3, 0, 6, q, 144, None, None, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 1 << 20, 1 << 20, 3, 0, 6, q, 144, None, None, None), "T * H * W must not exceed 2^40 pixels"),
    ((p, 144, None, None, d, 144, c, 48, 7, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), FMT),
    ((p, 144, None, None, d, 144, c, 48, 3, 2, 4, 6, 5, 0, 6, q, 144, None, None, None), "C must be 3 or 4"),
    ((p, 144, None, None, d, 144, c, 48, 2, 2, 4, 6, 4, 0, 6, q, 144, None, None, None), "C must be 3 for the yuv420p formats"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 2, 6, q, 144, None, None, None), "order must be SVR_FIELD_TFF or SVR_FIELD_BFF"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, -1, q, 144, None, None, None), "mi must not be negative"),
    ((p + 1, 288, None, None, d, 288, c, 48, 3, 2, 4, 6, 3, 0, 6, q, 288, None, None, None), "packed is not aligned to 2 bytes"),
    ((p, 288, p + 4097, None, d, 288, c, 48, 3, 2, 4, 6, 3, 0, 6, q, 288, None, None, None), "before is not aligned to 2 bytes"),
    ((p, 288, None, p + 4097, d, 288, c, 48, 3, 2, 4, 6, 3, 0, 6, q, 288, None, None, None), "after is not aligned to 2 bytes"),
    ((p, 288, None, None, d + 1, 288, c, 48, 3, 2, 4, 6, 3, 0, 6, q, 288, None, None, None), "deint is not aligned to 2 bytes"),
    ((p, 288, None, None, d, 288, c, 48, 3, 2, 4, 6, 3, 0, 6, q + 1, 288, None, None, None), "out is not aligned to 2 bytes"),
    ((p, 144, None, None, d, 144, c + 2, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "cnt is not aligned to 4 bytes"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, m + 2, None, None), "modes is not aligned to 4 bytes"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, st + 4, None), "stats is not aligned to 8 bytes"),
    ((p, 143, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "packed_bytes is 143, the format needs exactly 144"),
    ((p, 144, None, None, d, 145, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "deint_bytes is 145, the format needs exactly 144"),
    ((p, 144, None, None, d, 144, c, 24, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "cnt_bytes is 24, int32 [T, 3, 2] needs exactly 48"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 288, None, None, None), "out_bytes is 288, the format needs exactly 144"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, p + 143, 144, None, None, None), "out overlaps packed"),
    ((p, 144, q + 143, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "out overlaps before"),
    ((p, 144, None, q + (-71), d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "out overlaps after"),
    ((p, 144, None, None, q + 100, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "out overlaps deint"),
    ((p, 144, None, None, d, 144, q + 140, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, None, None), "out overlaps cnt"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, p + 140, None, None), "modes overlaps packed"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, c + 44, None, None), "modes overlaps cnt"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, q + 140, None, None), "modes overlaps out"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, d + 136, None), "stats overlaps deint"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, None, q + 136, None), "stats overlaps out"),
    ((p, 144, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, 6, q, 144, m, m, None), "stats overlaps modes"),
    # two faults: which one is reported
    ((p, 143, None, None, None, 144, c, 48, 9, 2, 4, 6, 3, 0, -6, q, 144, None, None, None), "deint is a null pointer"),
    ((p, 143, None, None, d, 144, c, 48, 0, 2, 4, 6, 3, 0, -6, q, 144, None, None, None), "mi must not be negative"),
    ((p, 143, None, None, d, 145, c, 48, 0, 2, 4, 6, 3, 0, 6, p, 144, None, None, None), "packed_bytes is 143, the format needs exactly 144"),
]


def test_every_refusal_message_of_the_entry_points_is_exact():
    """Every argument is validated on the host before anything is enqueued, so a host buffer stands in for device memory."""
    L = sub("hip_lib").lib()
    for fn, rows in (("svr_comb_counts", COMB_ROWS), ("svr_field_select", SELECT_ROWS)):
        for args, message in rows:
            assert L.svr_set_option(b"no_such_key", 0) != 0         # (a known message first: an accepted call would leave it standing)
            assert call(L, fn, args) == -1, (fn, args)
            assert L.svr_last_error().decode() == f"{fn}: {message}", (fn, args)


def test_header_ctypes_table_and_build_list_know_the_entry_points():
    hip_lib = sub("hip_lib")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert {"svr_comb_counts", "svr_field_select"} <= declared and declared == set(hip_lib.SYMBOLS)
    for fn, n in (("svr_comb_counts", 14), ("svr_field_select", 20)):
        decl = re.search(rf"int {fn}\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == n == len(hip_lib.SYMBOLS[fn][1]), fn
        assert re.search(rf"^ \*   {fn}\s+\S", src, flags=re.M), fn                                   # the operand-layout table
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert re.search(r"v9, additive: \+ svr_comb_counts\(\) / svr_field_select\(\).*?New symbols only", src, flags=re.S)
    api = open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert '#include "svr_fieldmatch.hip"' in api and api.index('#include "svr_deinterlace.hip"') < api.index('#include "svr_fieldmatch.hip"')
    assert os.path.join(hip_lib.CSRC, "svr_fieldmatch.hip") in hip_lib.sources()          # (the loader's source hash covers it)
    lib = hip_lib.lib()
    assert lib.svr_abi_version() == 9 and hasattr(lib, "svr_comb_counts") and hasattr(lib, "svr_field_select")
