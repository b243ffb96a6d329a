"""-m "not gpu": the deinterlacing rule (deinterlace.py, the specification of csrc/svr_deinterlace.hip) -- the vectorised torch
against a per-sample restatement of the text, the check values that pin the text, static clips, kept rows and range, any split
equal to the whole, moving bars and a moving diagonal --, the command line's reader behind FrameSource(fields=...) and the
deinterlace.ENABLED switch against stand-ins for the two executables, and the C ABI's refusals.  NOT covered anywhere: a real ffmpeg,
a real interlaced recording."""
import json
import os
import re
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from deinterlace_cases import (CONTEXTS, FORMATS, SHAPES, as_gray_rgb, channel_counts, context, formula_clip, loop_deinterlace, loop_plane,
                               moving_bar, moving_diagonal, random_packed, weave)
from frame_unpack_cases import calls, fake_video, stand_ins
from test_frame_unpack import identity  # noqa: F401 (fixture)
from test_refusal_messages import Ptr, call
from test_stream import cli, rig  # noqa: F401 (fixtures)

ORDERS, RATES = ("tff", "bff"), ("frame", "field")
LOOP_CAP = 6000                                       # samples per frame above which the loop restatement is not run


# ---------------------------------------------------------------------------------------------------------------- specification
def test_module_surface_and_the_shipped_switch():
    de, fin = sub("deinterlace"), sub("frameio_in")
    assert de.ORDERS == ORDERS and de.RATES == RATES and de.ENABLED is False and de.RATE == "field"
    for word in ("mis-tag", "synthetic", "comb detection", "telecine", "one-frame clip"):
        assert word in de.__doc__, word
    assert de.planes("rgb16", 5, 7, 4) == [(0, 5, 28, 4)] and de.planes("bgr8", 5, 7, 3) == [(0, 5, 21, 3)]
    assert de.planes("yuv420p10", 5, 7, 3) == [(0, 5, 7, 1), (35, 3, 4, 1), (47, 3, 4, 1)]
    for fmt in fin.FORMATS:
        for C in channel_counts(fmt):
            off, R, N, _ = de.planes(fmt, 5, 7, C)[-1]                           # the last plane ends where the frame ends
            assert off + R * N == random_packed(fmt, 1, 5, 7, C, seed=0).numel()
    for tag, order in (("tt", "tff"), ("tb", "tff"), ("bb", "bff"), ("bt", "bff"), ("progressive", None), ("unknown", None), ("", None),
                       (None, None)):
        assert de.field_order(tag) == order, tag


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] * s[2] * 4 <= LOOP_CAP], ids=lambda s: "x".join(map(str, s)))
def test_torch_equals_the_loop_restatement(shape, fmt):
    """Random clips over the whole code range; every channel count, both orders, both rates, every kind of context."""
    de = sub("deinterlace")
    T, H, W = shape
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=sum(shape) + C)
        for n, kind in enumerate(CONTEXTS):
            before, after = context(kind, fmt, H, W, C, seed=n)
            for order in ORDERS:
                for rate in RATES:
                    got = de.deinterlace_torch(packed, fmt, T, H, W, C, order, rate, before, after)
                    want = loop_deinterlace(packed, fmt, T, H, W, C, order, rate, before, after)
                    assert got.dtype == packed.dtype and got.shape == want.shape and got.is_contiguous()
                    assert got.shape[0] == T * (2 if rate == "field" else 1) and got.shape[1:] == packed.shape[1:]
                    assert torch.equal(got, want), (C, kind, order, rate)


def luma_only(F, H, W):
    """a list-of-lists plane as the Y plane of a yuv420p8 clip whose chroma is zero (static: it comes back zero, sums are the Y plane's)"""
    T = len(F)
    y = torch.tensor(F, dtype=torch.int64).reshape(T, H * W)
    return torch.cat([y, torch.zeros(T, 2 * ((H + 1) // 2) * ((W + 1) // 2), dtype=torch.int64)], dim=1).to(torch.uint8)


def test_check_values_pin_the_text():
    """Figures from a loop prototype of exactly the rule's text, written when the rule was drafted, before any of this code: the
    loop restatement here and the torch statement (one plane with s = 1 = the Y plane of a yuv420p8 clip; s = 3 = an rgb8 clip)
    both give them."""
    de = sub("deinterlace")
    total = lambda frames: sum(v for f in frames for row in f for v in row)
    T, R, N = 3, 6, 11
    F = formula_clip(T, R, N)
    assert F[1][2][3] == (37 + 66 + 45 + 6 + 202 + 87) % 256
    clip = luma_only(F, R, N)
    sums = {("tff", "frame"): 24596, ("tff", "field"): 48187, ("bff", "frame"): 23649, ("bff", "field"): 48323}
    for (order, rate), want in sums.items():
        assert total(loop_plane(F, R, N, 1, order, rate)) == want, (order, rate)
        assert int(de.deinterlace_torch(clip, "yuv420p8", T, R, N, 3, order, rate).long().sum()) == want, (order, rate)
    rows = {(2, 1): [141, 58, 113, 162, 141, 226, 65, 68, 141, 138, 145], (3, 2): [117, 173, 239, 73, 33, 27, 133, 79, 77, 85, 103]}
    loop = loop_plane(F, R, N, 1, "tff", "field")
    spec = de.deinterlace_torch(clip, "yuv420p8", T, R, N, 3, "tff", "field")[:, :R * N].reshape(2 * T, R, N)
    for (o, r), want in rows.items():
        assert loop[o][r] == want and spec[o, r].tolist() == want, (o, r)
    assert total(loop_plane(F, R, N, 1, "tff", "field", F[2], F[0])) == 48495
    assert int(de.deinterlace_torch(clip, "yuv420p8", T, R, N, 3, "tff", "field", clip[2], clip[0]).long().sum()) == 48495
    T, R, N = 2, 5, 33
    G = formula_clip(T, R, N)
    assert total(loop_plane(G, R, N, 3, "bff", "field")) == 78600 and total(loop_plane(G, R, N, 1, "bff", "field")) == 78511
    rgb = torch.tensor(G, dtype=torch.int64).to(torch.uint8).reshape(T, R, N // 3, 3)
    assert int(de.deinterlace_torch(rgb, "rgb8", T, R, N // 3, 3, "bff", "field").long().sum()) == 78600
    assert int(de.deinterlace_torch(luma_only(G, R, N), "yuv420p8", T, R, N, 3, "bff", "field").long().sum()) == 78511


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_static_clip_comes_back_exactly(fmt):
    de = sub("deinterlace")
    for T, H, W in ((1, 5, 9), (2, 6, 7), (4, 17, 33), (3, 1, 8), (3, 2, 2)):
        for C in channel_counts(fmt):
            image = random_packed(fmt, 1, H, W, C, seed=H + W)
            clip = image.expand(T, *image.shape[1:]).contiguous()
            for order in ORDERS:
                for rate in RATES:
                    out = de.deinterlace_torch(clip, fmt, T, H, W, C, order, rate)
                    assert torch.equal(out, image.expand(out.shape[0], *image.shape[1:])), (T, H, W, C, order, rate)


@pytest.mark.parametrize("fmt", FORMATS)
def test_kept_rows_are_the_source_rows_and_results_stay_in_range(fmt):
    de = sub("deinterlace")
    T, H, W = 4, 9, 12
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=C)
        # a narrow band of codes: min / max of the inputs is then a real bound, not the container's
        packed = (packed.to(torch.int64) % 97 + 300 * (packed.element_size() - 1) + 50).to(packed.dtype)
        lo, hi = int(packed.to(torch.int64).min()), int(packed.to(torch.int64).max())
        for order in ORDERS:
            for rate in RATES:
                out = de.deinterlace_torch(packed, fmt, T, H, W, C, order, rate).to(torch.int64).reshape(-1, packed[0].numel())
                assert int(out.min()) >= lo and int(out.max()) <= hi
                src = packed.to(torch.int64).reshape(T, -1)
                for o in range(out.shape[0]):
                    t, k = (o // 2, o % 2) if rate == "field" else (o, 0)
                    p = (0 if order == "tff" else 1) ^ k
                    for off, R, N, _ in de.planes(fmt, H, W, C):
                        got, want = out[o, off:off + R * N].reshape(R, N), src[t, off:off + R * N].reshape(R, N)
                        assert torch.equal(got[p::2], want[p::2]), (order, rate, o, off)


@pytest.mark.parametrize("fmt", FORMATS)
def test_any_split_with_its_true_neighbours_equals_the_whole(fmt):
    """A part inside the clip gets the frames next to it.  A part at an end of the clip gets no frame on that side and mirrors on
    its own -- which is the whole clip's mirror as long as the part has two frames; a ONE-frame part at an end has nothing of its
    own to mirror and is handed the clip's mirror frame (F[1] ahead of the first frame, F[T-2] behind the last), as FrameSource does."""
    de = sub("deinterlace")
    T, H, W = 7, 6, 11
    for C in channel_counts(fmt):
        packed = random_packed(fmt, T, H, W, C, seed=11)

        def neighbours(a, b):
            before = packed[a - 1] if a > 0 else (packed[1] if b - a == 1 else None)
            after = packed[b] if b < T else (packed[T - 2] if b - a == 1 else None)
            return dict(before=before, after=after)

        for order in ORDERS:
            for rate in RATES:
                whole = de.deinterlace_torch(packed, fmt, T, H, W, C, order, rate)
                for cuts in ((3, 5), (2,), (1,), (1, 2, 3, 4, 5, 6), (6,)):
                    edges = [0, *cuts, T]
                    parts = [de.deinterlace_torch(packed[a:b].contiguous(), fmt, b - a, H, W, C, order, rate, **neighbours(a, b))
                             for a, b in zip(edges[:-1], edges[1:])]
                    assert torch.equal(torch.cat(parts), whole), (C, order, rate, cuts)


@pytest.mark.parametrize("width,speed", [(6, 4), (3, 5), (10, 2), (2, 7), (5, 5), (8, 3)])
def test_a_moving_bar_comes_back_field_by_field(width, speed):
    """10 fields of a vertical bar moving right, woven into 5 frames: field rate returns the fields' own pictures, frame rate every
    other one, in both orders; deinterlaced in the wrong order it does not."""
    de = sub("deinterlace")
    g = moving_bar(width, speed)
    for order in ORDERS:
        frames = as_gray_rgb(weave(g, order))
        out = de.deinterlace_torch(frames, "rgb8", 5, 8, 96, 3, order, "field")
        assert torch.equal(out, as_gray_rgb(g)), order
        assert torch.equal(de.deinterlace_torch(frames, "rgb8", 5, 8, 96, 3, order, "frame"), as_gray_rgb(g[0::2])), order
        other = ORDERS[1 - ORDERS.index(order)]
        assert not torch.equal(de.deinterlace_torch(frames, "rgb8", 5, 8, 96, 3, other, "field"), as_gray_rgb(g))


def test_a_moving_diagonal_is_closer_than_the_woven_frame():
    """8 fields of a slanted bar moving right: every output is closer to its field's picture than the woven frame it came from, by
    more than a factor of two (mean absolute error 0.33 inside the clip and 1.16 at its ends against 5.94 woven; the half is a
    margin over those figures, not a tuned bound)."""
    de = sub("deinterlace")
    g = moving_diagonal()
    woven = weave(g, "tff")
    frames = torch.cat([woven.reshape(4, -1), torch.full((4, 2 * 6 * 48), 128, dtype=torch.uint8)], dim=1)       # yuv420p8, flat chroma
    out = de.deinterlace_torch(frames, "yuv420p8", 4, 12, 96, 3, "tff", "field")[:, :12 * 96].reshape(8, 12, 96)
    mae = lambda a, b: float((a.to(torch.int64) - b.to(torch.int64)).abs().double().mean())
    for n in range(8):
        print(f"field {n}: deinterlaced {mae(out[n], g[n]):.3f}, woven {mae(woven[n // 2], g[n]):.3f}")
        assert mae(out[n], g[n]) < 0.5 * mae(woven[n // 2], g[n]), n


def test_arguments_are_refused_by_name():
    de = sub("deinterlace")
    packed = random_packed("rgb8", 2, 4, 6, 3, seed=0)
    ok = dict(packed=packed, fmt="rgb8", T=2, H=4, W=6, C=3, order="tff", rate="field")
    for change, word in ((dict(fmt="rgb10"), "fmt must be"), (dict(C=2), "C = 3 or 4"), (dict(order="top"), "order must be one of"),
                         (dict(rate="double"), "rate must be one of"), (dict(T=0, packed=packed[:0]), "T, H, W must be positive"),
                         (dict(packed=packed.to(torch.int16)), "packed must be torch.uint8"), (dict(W=7), "packed must hold 168 samples"),
                         (dict(before=packed), "before must hold the 72 samples of one rgb8 frame"),
                         (dict(after=packed[0].to(torch.int32)), "after must be torch.uint8"),
                         (dict(fmt="yuv420p8", C=4), "yuv420p8 takes C = 3")):
        with pytest.raises(ValueError, match=re.escape(word)):
            de.check_arguments(**{**ok, **change})
        with pytest.raises(ValueError, match=re.escape(word)):
            de.deinterlace_torch(**{**ok, **change})
    assert de.check_arguments(**ok, before=packed[0], after=packed[1].reshape(-1)) == (2, 4, 6, 3)
    # deinterlace(): the torch statement without ops, ``out`` checked and filled; a backend that has the op is used and may raise
    want = de.deinterlace_torch(**ok)
    out = torch.empty_like(want)
    assert de.deinterlace(**ok, out=out) is out and torch.equal(out, want) and torch.equal(de.deinterlace(**ok), want)
    with pytest.raises(ValueError, match="out must be"):
        de.deinterlace(**ok, out=torch.empty(2, 4, 6, 3, dtype=torch.uint8))

    class Failing:
        def deinterlace(self, *a, **kw):
            raise RuntimeError("library failed")

    with pytest.raises(RuntimeError, match="library failed"):
        de.deinterlace(**ok, ops=Failing())


# ---------------------------------------------------------------------------------------------------------------- reader
def tagged(path, packed, pix_fmt, width, height, field_order=None, **kw):
    """frame_unpack_cases.fake_video plus the field_order tag its canned ffprobe answer does not carry"""
    fake_video(path, packed, pix_fmt, width, height, **kw)
    answer = json.load(open(str(path) + ".json"))
    if field_order is not None:
        answer["streams"][0]["field_order"] = field_order
    json.dump(answer, open(str(path) + ".json", "w"))


def test_probe_dictionaries_do_not_change_for_a_tagged_file(cli, tmp_path):
    ffprobe, _ = stand_ins(str(tmp_path / "bin"))
    clip = tmp_path / "clip.mkv"
    answers = []
    for tag in (None, "tt", "bb", "progressive"):
        tagged(clip, None, "yuv420p", 720, 576, field_order=tag, rate="25/1", audio=True, color_space="bt470bg", color_range="tv")
        answers.append((cli.probe_video(ffprobe, str(clip)), cli.probe_colour(ffprobe, str(clip)), cli.probe_source(ffprobe, str(clip))))
        v, streams = cli.probe_stream(ffprobe, str(clip))
        assert v.get("field_order") == tag and len(streams) == 2 and cli.source_tags(v, streams) == answers[-1][2]
    assert answers[0][0] == dict(width=720, height=576, fps=Fraction(25), pix_fmt="yuv420p", color_space="bt470bg", color_range="tv",
                                 has_audio=True)
    assert answers[0][1] == dict(color_space="bt470bg", color_primaries=None, color_transfer=None, color_range="tv", chroma_location=None)
    assert all(a == answers[0] and a[2] == (a[0], a[1]) for a in answers)


def field_source(cli, tmp_path, fmt, pix, C, fields, T=13, H=5, W=7, chunk=5, **video_kw):
    _, ffmpeg = stand_ins(str(tmp_path / "bin"))
    clip = tmp_path / f"clip_{fmt}.mkv"
    packed = random_packed(fmt, T, H, W, C, seed=T + H + W)
    fake_video(clip, packed, pix, W, H, **video_kw)
    info = dict(width=W, height=H, fps=Fraction(30000, 1001), pix_fmt=pix, color_space=None, color_range=None, has_audio=False)
    return cli.FrameSource(ffmpeg, str(clip), info, chunk, fields=fields), packed, clip


@pytest.mark.parametrize("fmt,pix,C", [("yuv420p10", "yuv420p10le", 3), ("yuv420p8", "yuv420p", 3), ("rgb8", "rgba", 4)])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("rate", RATES)
def test_source_chunks_equal_the_specification_applied_to_the_whole_clip(cli, tmp_path, fmt, pix, C, order, rate):
    """13 frames of 5 x 7 in chunks of 5: every buffer is deinterlaced between its true neighbours, so the chunks are the whole
    clip's result, 5 + 5 + 3 frames in frame rate and 10 + 10 + 6 in field rate; the decoder's command is today's."""
    fin, de = sub("frameio_in"), sub("deinterlace")
    src, packed, clip = field_source(cli, tmp_path, fmt, pix, C, (order, rate))
    k = 2 if rate == "field" else 1
    assert src.fps == k * Fraction(30000, 1001) and isinstance(src.fps, Fraction)
    got = list(src.chunks())
    assert [c.shape[0] for c in got] == [5 * k, 5 * k, 3 * k] and all(c.dtype == torch.float32 and c.shape[1:] == (5, 7, C) for c in got)
    want = fin.unpack_frames_torch(de.deinterlace_torch(packed, fmt, 13, 5, 7, C, order, rate), fmt, 13 * k, 5, 7, C, "bt601", "tv")
    assert torch.equal(torch.cat(got), want)
    argv = open(str(clip) + ".args").read().split("\n")
    assert argv == ["-loglevel", "error", "-noautorotate", "-i", str(clip), "-map", "0:v:0", "-f", "rawvideo", "-pix_fmt", pix, "-"]
    assert not src.thread.is_alive() and src.proc.returncode == 0
    # any chunk size gives the same frames, a chunk of one frame and one that holds the clip included
    for chunk in (1, 4, 13, 20):
        src, _, _ = field_source(cli, tmp_path, fmt, pix, C, (order, rate), chunk=chunk)
        assert torch.equal(torch.cat(list(src.chunks())), want), chunk


def test_source_without_fields_is_todays_and_an_early_close_ends_the_reader(cli, tmp_path):
    fin = sub("frameio_in")
    src, packed, _ = field_source(cli, tmp_path, "yuv420p8", "yuv420p", 3, None)
    assert src.fps == Fraction(30000, 1001) and src.fields is None
    got = list(src.chunks())
    assert [c.shape[0] for c in got] == [5, 5, 3] and torch.equal(torch.cat(got), fin.unpack_frames_torch(packed, "yuv420p8", 13, 5, 7, 3, "bt601", "tv"))
    with pytest.raises(ValueError, match="fields must be"):
        cli.FrameSource("ffmpeg", "x.mkv", dict(width=2, height=2, fps=Fraction(24), pix_fmt="yuv420p"), 5, fields=("top", "field"))
    # the caller stops after the first chunk of a clip that never ends: the decoder is terminated, the thread ends
    src, _, _ = field_source(cli, tmp_path, "rgb16", "rgb48le", 3, ("bff", "field"), endless=True)
    stream = src.chunks()
    assert next(stream).shape[0] == 10
    stream.close()
    assert not src.thread.is_alive() and src.proc.returncode is not None
    # an empty stream is still "No frames to process"
    src, _, _ = field_source(cli, tmp_path, "yuv420p8", "yuv420p", 3, ("tff", "frame"), T=0)
    with pytest.raises(ValueError, match="No frames to process"):
        list(src.chunks())


# ---------------------------------------------------------------------------------------------------------------- command line
T, H, W = 13, 8, 10


def run_main(cli, tmp_path, monkeypatch, chunked, field_order):
    """13 yuv420p frames of 8 x 10 at 25 fps, tagged, through the identity "engines" into the stand-in encoder -> (its argv, its
    stdin, the packed clip, the output path)"""
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    packed = random_packed("yuv420p8", T, H, W, 3, seed=7)
    src, out = tmp_path / "clip.mkv", tmp_path / "out.mp4"
    tagged(src, packed, "yuv420p", W, H, field_order=field_order, rate="25/1", color_space="bt709", color_range="tv")
    tail = ["--chunk_size", "5"] if chunked else []
    assert cli.main([str(src), "--video_backend", "ffmpeg", "--output", str(out)] + tail) == 0
    return open(str(out) + ".args").read().split("\n"), out.read_bytes(), packed, out


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
@pytest.mark.parametrize("tag,order", [("tt", "tff"), ("bt", "bff")])
def test_cli_deinterlaces_a_tagged_source_where_the_switch_is_on(identity, tmp_path, monkeypatch, capsys, chunked, tag, order):
    fin, de, frameio = sub("frameio_in"), sub("deinterlace"), sub("frameio")
    monkeypatch.setattr(de, "ENABLED", True)
    argv, piped, packed, out = run_main(identity, tmp_path, monkeypatch, chunked, tag)
    frames = fin.unpack_frames_torch(de.deinterlace_torch(packed, "yuv420p8", T, H, W, 3, order, "field"), "yuv420p8", 2 * T, H, W, 3,
                                     "bt709", "tv")
    assert piped == frameio.pack_frames_torch(frames, "bgr8").numpy().tobytes() and len(piped) == 26 * H * W * 3
    assert argv[argv.index("-r") + 1] == "50"
    assert "Warning" not in capsys.readouterr().err
    log = calls(str(tmp_path / "bin"))
    assert [line.split()[0] for line in log] == ["ffprobe", "ffmpeg", "ffmpeg"]          # ONE probe, the decoder, the encoder


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_cli_with_the_switch_off_warns_once_and_writes_todays_output(identity, tmp_path, monkeypatch, capsys, chunked):
    fin, de, frameio = sub("frameio_in"), sub("deinterlace"), sub("frameio")
    assert de.ENABLED is False
    argv, piped, packed, out = run_main(identity, tmp_path, monkeypatch, chunked, "tt")
    err = capsys.readouterr().err
    lines = [line for line in err.splitlines() if "interlaced" in line]
    assert len(lines) == 1 and lines[0].startswith("Warning: ") and "field_order tt" in lines[0] and "as stored" in lines[0]
    today = frameio.pack_frames_torch(fin.unpack_frames_torch(packed, "yuv420p8", T, H, W, 3, "bt709", "tv"), "bgr8").numpy().tobytes()
    assert piped == today and argv[argv.index("-r") + 1] == "25"
    # no tag, and a progressive one: the same bytes and argv, no warning
    for tag in (None, "progressive"):
        argv2, piped2, _, _ = run_main(identity, tmp_path, monkeypatch, chunked, tag)
        assert argv2 == argv and piped2 == today and "Warning" not in capsys.readouterr().err
    # ... and with the switch ON a source without an order is today's as well
    monkeypatch.setattr(de, "ENABLED", True)
    argv3, piped3, _, _ = run_main(identity, tmp_path, monkeypatch, chunked, "progressive")
    assert argv3 == argv and piped3 == today and "Warning" not in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------- C ABI
p, q = Ptr(0), Ptr(1 << 16)                     # two operands 64 KiB apart (a 2-frame 4 x 6 rgb8 clip with C = 3 is 144 bytes)
FMT = "fmt must be SVR_UNPACK_RGB8, SVR_UNPACK_BGR8, SVR_UNPACK_RGB16, SVR_UNPACK_YUV420P8 or SVR_UNPACK_YUV420P10"
# (packed, packed_bytes, before, after, fmt, T, H, W, C, order, rate, out, out_bytes, stream) -> svr_last_error()
DEINT_ROWS = [
    ((None, 144, None, None, 0, 2, 4, 6, 3, 0, 1, q, 288, None), "packed is a null pointer"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 1, None, 288, None), "out is a null pointer"),
    ((p, 144, None, None, 0, 0, 4, 6, 3, 0, 1, q, 288, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, None, 0, 2, 0, 6, 3, 0, 1, q, 288, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, None, 0, 2, 4, -1, 3, 0, 1, q, 288, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 144, None, None, 0, 2, 1 << 20, 1 << 20, 3, 0, 1, q, 288, None), "T * H * W must not exceed 2^40 pixels"),
    ((p, 144, None, None, 5, 2, 4, 6, 3, 0, 1, q, 288, None), FMT),
    ((p, 144, None, None, -1, 2, 4, 6, 3, 0, 1, q, 288, None), FMT),
    ((p, 144, None, None, 0, 2, 4, 6, 2, 0, 1, q, 288, None), "C must be 3 or 4"),
    ((p, 144, None, None, 3, 2, 4, 6, 5, 0, 1, q, 288, None), "C must be 3 or 4"),
    ((p, 144, None, None, 2, 2, 4, 6, 4, 0, 1, q, 288, None), "C must be 3 for the yuv420p formats"),
    ((p, 144, None, None, 4, 2, 4, 6, 4, 0, 1, q, 288, None), "C must be 3 for the yuv420p formats"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 2, 1, q, 288, None), "order must be SVR_FIELD_TFF or SVR_FIELD_BFF"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, -1, 1, q, 288, None), "order must be SVR_FIELD_TFF or SVR_FIELD_BFF"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 2, q, 288, None), "rate must be SVR_DEINT_FRAME or SVR_DEINT_FIELD"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, -1, q, 288, None), "rate must be SVR_DEINT_FRAME or SVR_DEINT_FIELD"),
    ((p + 1, 288, None, None, 3, 2, 4, 6, 3, 0, 1, q, 576, None), "packed is not aligned to 2 bytes"),
    ((p, 144, p + 4097, None, 2, 2, 4, 6, 3, 0, 1, q, 288, None), "before is not aligned to 2 bytes"),
    ((p, 144, None, p + 4097, 2, 2, 4, 6, 3, 0, 1, q, 288, None), "after is not aligned to 2 bytes"),
    ((p, 144, None, None, 2, 2, 4, 6, 3, 0, 1, q + 1, 288, None), "out is not aligned to 2 bytes"),
    ((p, 143, None, None, 0, 2, 4, 6, 3, 0, 1, q, 288, None), "packed_bytes is 143, the format needs exactly 144"),
    ((p, 144, None, None, 1, 2, 4, 6, 4, 0, 1, q, 288, None), "packed_bytes is 144, the format needs exactly 192"),
    ((p, 144, None, None, 3, 2, 4, 6, 3, 0, 1, q, 576, None), "packed_bytes is 144, the format needs exactly 288"),
    ((p, 0, None, None, 4, 2, 3, 5, 3, 0, 1, q, 108, None), "packed_bytes is 0, the format needs exactly 54"),
    ((p, 108, None, None, 2, 2, 3, 5, 3, 0, 0, q, 54, None), "out_bytes is 54, the format and rate need exactly 108"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 1, q, 144, None), "out_bytes is 144, the format and rate need exactly 288"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 0, q, 288, None), "out_bytes is 288, the format and rate need exactly 144"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 1, 1, p + 143, 288, None), "out overlaps packed"),
    ((p + 287, 144, None, None, 0, 2, 4, 6, 3, 1, 1, p, 288, None), "out overlaps packed"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 1, 0, p, 144, None), "out overlaps packed"),
    ((p, 144, q + 287, None, 0, 2, 4, 6, 3, 0, 1, q, 288, None), "out overlaps before"),
    ((p, 144, None, q + (-71), 0, 2, 4, 6, 3, 0, 1, q, 288, None), "out overlaps after"),
    # two faults: which one is reported
    ((None, 143, None, None, 9, 0, 4, 6, 3, 0, 1, None, 288, None), "packed is a null pointer"),
    ((p, 143, None, None, 9, 2, 4, 6, 3, 7, 1, q, 288, None), FMT),
    ((p, 143, None, None, 0, 2, 4, 6, 3, 7, 7, q, 288, None), "order must be SVR_FIELD_TFF or SVR_FIELD_BFF"),
    ((p, 143, None, None, 0, 2, 4, 6, 3, 0, 1, p, 287, None), "packed_bytes is 143, the format needs exactly 144"),
    ((p, 144, None, None, 0, 2, 4, 6, 3, 0, 1, p, 287, None), "out_bytes is 287, the format and rate need exactly 288"),
]


def test_every_refusal_message_of_the_entry_point_is_exact():
    """Every argument is validated on the host before the first launch, so a host buffer stands in for device memory."""
    L = sub("hip_lib").lib()
    for args, message in DEINT_ROWS:
        assert L.svr_set_option(b"no_such_key", 0) != 0             # (a known message first: an accepted call would leave it standing)
        assert call(L, "svr_deinterlace", args) == -1, args
        assert L.svr_last_error().decode() == "svr_deinterlace: " + message, args


def test_header_ctypes_table_and_build_list_know_the_entry_point():
    hip_lib, de = sub("hip_lib"), sub("deinterlace")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert "svr_deinterlace" in declared and declared == set(hip_lib.SYMBOLS)
    decl = re.search(r"int svr_deinterlace\(([^;]*)\);", src).group(1)
    assert len(decl.split(",")) == 14 == len(hip_lib.SYMBOLS["svr_deinterlace"][1])
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert re.search(r"v9, additive: \+ svr_deinterlace\(\).*?A new symbol only", src, flags=re.S)
    assert re.search(r"^ \*   svr_deinterlace\s+element alignment is enough", src, flags=re.M)          # the operand-layout table
    for table, prefix in ((hip_lib.FIELD_ORDERS, "SVR_FIELD_"), (hip_lib.DEINT_RATES, "SVR_DEINT_")):
        for name, code in table.items():
            assert re.search(rf"#define {prefix}{name.upper()}\s+{code}\b", src), name
    assert tuple(hip_lib.FIELD_ORDERS) == de.ORDERS and tuple(hip_lib.DEINT_RATES) == de.RATES
    assert [hip_lib.FIELD_ORDERS[o] for o in de.ORDERS] == [0, 1] and [hip_lib.DEINT_RATES[r] for r in de.RATES] == [0, 1]
    assert '#include "svr_deinterlace.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert os.path.join(hip_lib.CSRC, "svr_deinterlace.hip") in hip_lib.sources()         # (the loader's source hash covers it)
