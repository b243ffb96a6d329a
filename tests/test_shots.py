"""-m "not gpu": shot-aware batching -- shots.py (the signature, the distance and the rule, in exact integers), pipeline.upscale_shots
and pipeline.upscale_stream(cuts=...) against the per-shot / per-piece pipeline.upscale calls they stand for (bit for bit, on the fp32
torch double of the C ABI), and the command line behind the shots.ENABLED switch.  Every test passes its detector parameters
explicitly; none reads shots.DEFAULTS."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from ops_reference import TorchOps
from shot_clips import assert_precondition, cuts_of, shot_clip
from test_stream import tiny_runner

PARAMS = dict(percent=30, ratio=3, window=8, min_shot=3)


# ---------------------------------------------------------------------------------------------------------------- signature
def test_luma_check_values():
    shots = sub("shots")
    px = lambda *rgb: int(shots.luma8(torch.tensor(rgb, dtype=torch.float32).view(1, 1, 1, 3)))
    assert [px(1, 1, 1), px(0, 0, 0), px(1, 0, 0), px(0, 1, 0), px(0, 0, 1)] == [255, 0, 54, 182, 18]
    assert 13933 + 46871 + 4732 == 65536 and (shots.GRID, shots.BINS) == (4, 64)


def naive_signatures(frames):
    """per pixel, in Python integers; the codes from frameio.codes"""
    T, H, W, _ = frames.shape
    q = sub("frameio").codes(frames[..., :3], 255.0).to(torch.int64).tolist()
    sig = [[0] * 1024 for _ in range(T)]
    for t in range(T):
        for y in range(H):
            for x in range(W):
                r, g, b = q[t][y][x]
                y8 = (13933 * r + 46871 * g + 4732 * b + 32768) >> 16
                sig[t][(((y * 4) // H) * 4 + (x * 4) // W) * 64 + (y8 >> 2)] += 1
    return torch.tensor(sig, dtype=torch.int32)


@pytest.mark.parametrize("shape", [(2, 19, 23, 3), (2, 4, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_signatures_equal_a_per_pixel_loop(shape):
    shots = sub("shots")
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(sum(shape))) * 1.2 - 0.1
    for src in (x, x.to(torch.bfloat16)):
        sig = shots.signatures_torch(src)
        assert sig.dtype == torch.int32 and tuple(sig.shape) == (shape[0], 1024)
        assert torch.equal(sig, naive_signatures(src))
        assert sig.sum(dim=1).tolist() == [shape[1] * shape[2]] * shape[0]
        assert torch.equal(shots.signatures(src), sig) and torch.equal(shots.signatures(src, ops=object()), sig)
    if shape[-1] == 4:                                       # the fourth channel is ignored
        assert torch.equal(shots.signatures_torch(x), shots.signatures_torch(x[..., :3].contiguous()))
    # a bf16 clip is read as the values it holds
    assert torch.equal(shots.signatures_torch(x.to(torch.bfloat16)), shots.signatures_torch(x.to(torch.bfloat16).float()))


def test_non_finite_negative_and_large_values_follow_frameio_codes():
    shots = sub("shots")
    flat = lambda v: torch.full((1, 5, 6, 3), v)
    bins = lambda sig: sorted(set((sig[0].nonzero().flatten() % 64).tolist()))
    for v, want in ((float("nan"), 0), (float("inf"), 63), (-float("inf"), 0), (-0.3, 0), (1.7, 63), (-0.0, 0)):
        for dtype in (torch.float32, torch.bfloat16):
            sig = shots.signatures_torch(flat(v).to(dtype))
            assert bins(sig) == [want] and int(sig.sum()) == 30, (v, dtype)
    x = torch.rand(1, 19, 23, 3, generator=torch.Generator().manual_seed(1))
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.5, 1.5])
    x.view(-1)[torch.randperm(x.numel(), generator=torch.Generator().manual_seed(2))[:200]] = specials[torch.arange(200) % 5]
    assert torch.equal(shots.signatures_torch(x), naive_signatures(x))


def test_refusals_name_the_argument():
    shots = sub("shots")
    for shape, dtype, word in (((2, 3, 8, 3), torch.float32, "H >= 4"), ((2, 8, 3, 3), torch.float32, "W >= 4"),
                               ((0, 8, 8, 3), torch.float32, "T >= 1"), ((1, 8, 8, 2), torch.float32, "C = 3 or 4"),
                               ((1, 8, 8, 3), torch.float16, "fp32 or bf16"), ((8, 8, 3), torch.float32, r"\[T, H, W, 3 \| 4\]")):
        with pytest.raises(ValueError, match=word):
            shots.signatures_torch(torch.zeros(shape, dtype=dtype))
    for name in PARAMS:
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match=name):
                shots.Detector(**{**PARAMS, name: bad})
    with pytest.raises(ValueError, match="sig_chunk"):
        shots.Detector(**PARAMS).feed(torch.zeros(2, 1024, dtype=torch.int64))
    for total, cuts in ((5, [0]), (5, [5]), (5, [3, 3]), (5, [4, 2]), (0, [])):
        with pytest.raises(ValueError, match="cuts|total"):
            shots.split(total, cuts)
    assert shots.split(5, []) == [(0, 5)] and shots.split(9, [2, 8]) == [(0, 2), (2, 8), (8, 9)]


# ---------------------------------------------------------------------------------------------------------------- the rule
HW = 1000                                                    # 2 H W = 2000: percent 30 asks for D >= 600


def sig_sequence(dists):
    """int32 [len(dists) + 1, 1024] of frames of HW pixels whose consecutive distances are ``dists`` (even numbers): the mass
    a[t] of counter 1 moves by dists[t] / 2, down where there is room and up where not"""
    a, rows = 0, [[HW, 0]]
    for d in dists:
        assert d % 2 == 0 and 0 <= d <= 2 * HW
        a = a - d // 2 if a - d // 2 >= 0 else a + d // 2
        assert 0 <= a <= HW
        rows.append([HW - a, a])
    sig = torch.zeros(len(rows), 1024, dtype=torch.int32)
    sig[:, :2] = torch.tensor(rows, dtype=torch.int32)
    assert sub("shots").distances(sig).tolist() == list(dists)
    return sig


RULE_TABLE = [
    # (name, parameters that differ from percent 30 / ratio 3 / window 4 / min_shot 3, distances of frames 1.., cuts)
    ("(a) alone refuses: 25 % of 2 H W with (b) and (c) met", {}, [10, 10, 10, 500, 10], []),
    ("(a) met at exactly percent", {}, [10, 10, 10, 600, 10], [4]),
    ("(b) alone refuses: below ratio * max(hist)", {}, [300, 300, 300, 898, 10], []),
    ("(b) met at exactly ratio * max(hist)", {}, [300, 300, 300, 900, 10], [4]),
    ("(b) looks at the maximum of hist, not the last entry", {}, [10, 300, 10, 800], []),
    ("(c) alone refuses: the shot before is too short", {}, [10, 800, 10, 10], []),
    ("(c) met at exactly min_shot frames", {}, [10, 10, 800, 10], [3]),
    ("an empty hist passes (b)", {"min_shot": 1}, [2000], [1]),
    ("a zero maximum passes (b)", {}, [0, 0, 0, 2000], [4]),
    ("hist is cleared on a cut: 700 < 3 * 400 would refuse", {}, [400, 400, 400, 1300, 100, 100, 700], [4, 7]),
    ("hist keeps window entries: the 400 has left", {}, [400, 10, 10, 10, 10, 700], [6]),
    ("... and still counts one frame earlier", {}, [400, 10, 10, 10, 700], []),
    ("flash: one cut, the way back refused by (c), then muted", {}, [10, 10, 10, 1980, 1980, 10, 10, 10, 1980], [4]),
    ("flash: heard again once window frames have passed", {}, [10, 10, 10, 1980, 1980, 10, 10, 10, 10, 1980], [4, 10]),
]


@pytest.mark.parametrize("name,params,dists,cuts", RULE_TABLE, ids=[r[0] for r in RULE_TABLE])
def test_rule_table(name, params, dists, cuts):
    shots = sub("shots")
    p = {**dict(percent=30, ratio=3, window=4, min_shot=3), **params}
    sig = sig_sequence(dists)
    assert shots.Detector(**p).feed(sig) == cuts
    det = shots.Detector(**p)                                # frame by frame: the same
    assert [c for t in range(sig.shape[0]) for c in det.feed(sig[t:t + 1])] == cuts


def test_streaming_equals_whole_on_a_synthetic_clip():
    shots = sub("shots")
    lengths = [12, 15, 13]
    clip = shot_clip(19, 23, lengths, seed=4)
    assert_precondition(shots, clip, cuts_of(lengths))
    sig = shots.signatures_torch(clip)
    whole = shots.Detector(**PARAMS).feed(sig)
    assert whole == cuts_of(lengths) == [12, 27]
    for n in (1, 7, 13, 40):
        det = shots.Detector(**PARAMS)
        assert [c for i in range(0, 40, n) for c in det.feed(sig[i:i + n])] == whole, n
        assert det.count == 40
    big = shot_clip(32, 48, [6, 6], seed=5)
    assert_precondition(shots, big, [6])
    assert shots.Detector(**PARAMS).feed(shots.signatures_torch(big)) == [6]


# ---------------------------------------------------------------------------------------------------------------- planning
KW = dict(resolution=16, batch_size=5, color_correction="lab")


@pytest.fixture(scope="module")
def rig():
    return tiny_runner(TorchOps("cpu", act_dtype=torch.float32)), sub("weights").synth_text_embedding().float()


def chunked(frames, n=5):
    return [frames[i:i + n] for i in range(0, frames.shape[0], n)]


def test_upscale_shots_is_the_concatenation_of_the_per_shot_calls(rig):
    pipeline, shots = sub("pipeline"), sub("shots")
    runner, text = rig
    lengths = [6, 7]
    clip = shot_clip(19, 23, lengths, seed=6, channels=4)
    assert_precondition(shots, clip, [6])
    kw = dict(prepend_frames=2, temporal_overlap=1, **KW)
    want = torch.cat([pipeline.upscale(clip[a:b], runner, text, **kw) for a, b in ((0, 6), (6, 13))])
    assert want.shape[0] == 13 and want.shape[1] == 16 and want.shape[3] == 4
    for cuts in ([6], shots.Detector(**PARAMS)):
        got = pipeline.upscale_shots(clip, runner, text, cuts=cuts, **kw)
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert not torch.equal(want, pipeline.upscale(clip, runner, text, **kw))               # (the cut changes the batches)
    for name, value in (("batch_filter", lambda i: True), ("exchange_heads", lambda *a: {}), ("return_spans", True)):
        with pytest.raises(ValueError, match=name):
            pipeline.upscale_shots(clip, runner, text, cuts=[6], **{name: value}, **kw)
        with pytest.raises(ValueError, match=name):
            list(pipeline.upscale_stream([clip], runner, text, cuts=[6], **{name: value}, **kw))
    with pytest.raises(ValueError, match="cuts"):
        pipeline.upscale_shots(clip, runner, text, cuts=[13], **kw)


def test_stream_with_a_detector_on_a_clip_without_cuts_is_the_stream_without_one(rig):
    pipeline, shots = sub("pipeline"), sub("shots")
    runner, text = rig
    clip = shot_clip(19, 23, [13], seed=7)
    assert_precondition(shots, clip, [])
    kw = dict(temporal_overlap=2, prepend_frames=1, **KW)
    plain = list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, **kw))
    det = shots.Detector(**PARAMS)
    got = list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, cuts=det, **kw))
    assert det.count == 13 and [o.shape[0] for o in got] == [5, 5, 3]
    assert all(torch.equal(a, b) for a, b in zip(got, plain))
    assert all(torch.equal(a, b) for a, b in zip(pipeline.upscale_stream(iter(chunked(clip)), runner, text, cuts=[], **kw), plain))


# 16 frames in chunks of 5, temporal_overlap 2, prepend_frames 1.  Per chunk the pieces (first context frame, first frame, one past
# the last, prepend_frames) the stream must be the ``upscale`` of, written by hand from the rule of upscale_stream's docstring.
STREAM_CASES = {
    # a cut inside a chunk (7) and on a chunk's first frame (10)
    "inside, first frame": ([7, 3, 6], True, [[(0, 0, 5, 1)], [(3, 5, 7, 0), (7, 7, 10, 1)], [(10, 10, 15, 1)], [(13, 15, 16, 0)]]),
    # a cut on a chunk's first frame (5) and one frame after one (11)
    "first frame, one after": ([5, 6, 5], False, [[(0, 0, 5, 1)], [(5, 5, 10, 1)], [(8, 10, 11, 0), (11, 11, 15, 1)], [(13, 15, 16, 0)]]),
    # a cut on a chunk's last frame (9): the next chunk's context is one frame, not two
    "context shortened": ([9, 7], True, [[(0, 0, 5, 1)], [(3, 5, 9, 0), (9, 9, 10, 1)], [(9, 10, 15, 0)], [(13, 15, 16, 0)]]),
}


@pytest.mark.parametrize("case", list(STREAM_CASES))
def test_stream_ends_batches_and_contexts_at_the_cuts(rig, case):
    pipeline, shots = sub("pipeline"), sub("shots")
    runner, text = rig
    lengths, with_detector, plan = STREAM_CASES[case]
    cuts = cuts_of(lengths)
    clip = shot_clip(19, 23, lengths, seed=8)
    assert_precondition(shots, clip, cuts)
    source = shots.Detector(**PARAMS) if with_detector else cuts
    got = list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, temporal_overlap=2, prepend_frames=1, cuts=source, **KW))
    assert [o.shape[0] for o in got] == [5, 5, 5, 1]
    for k, pieces in enumerate(plan):
        want = torch.cat([pipeline.upscale(clip[c:b], runner, text, temporal_overlap=2, prepend_frames=p, **KW)[a - c:]
                          for c, a, b, p in pieces])
        assert torch.equal(got[k], want), (case, k)
    for c, a, b, p in (piece for pieces in plan for piece in pieces):      # the table itself: no piece or context across a cut
        assert not any(c < cut < b for cut in cuts) and (p == 1) == (a == 0 or a in cuts)


def test_no_encoder_call_holds_two_shots_and_no_context_reaches_behind_a_cut(rig, monkeypatch):
    """Flat frames that carry their index, (i + 1) / 32, through the resize and the [-1, 1] transform: every vae_encode call of the
    stream is read back as the set of clip frames it holds (padding frames repeat frames of the same call)."""
    pipeline, shots = sub("pipeline"), sub("shots")
    runner, text = rig
    cuts, total = [7, 10, 11, 14], 16
    clip = ((torch.arange(total, dtype=torch.float32) + 1) / 32).view(total, 1, 1, 1).expand(total, 19, 23, 3).contiguous()
    calls, real = [], runner.vae_encode

    def recording(xs):
        for x in xs:                                         # [3, T', H', W'] in [-1, 1]
            idx = ((x[0, :, 0, 0].float() + 1) / 2 * 32).round().to(torch.int64) - 1          # (the top-left pixel: never padding)
            calls.append(sorted(set(idx.tolist())))
        return real(xs)

    monkeypatch.setattr(runner, "vae_encode", recording)
    got = list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, temporal_overlap=2, prepend_frames=1, cuts=cuts,
                                       **{**KW, "color_correction": "none"}))
    assert [o.shape[0] for o in got] == [5, 5, 5, 1] and calls
    spans = shots.split(total, cuts)
    shot_of = lambda i: next(k for k, (a, b) in enumerate(spans) if a <= i < b)
    for frames in calls:
        assert all(0 <= i < total for i in frames)
        assert len({shot_of(i) for i in frames}) == 1, frames                    # one shot per call
        assert frames[0] >= spans[shot_of(frames[-1])][0], frames                # no frame from before the cut
    assert sorted(set(i for frames in calls for i in frames)) == list(range(total))
    assert [3, 4, 5, 6] in calls and [14, 15] in calls       # contexts are there: two frames for (5, 7), ONE behind the cut at 14
    assert not any(13 in frames and 15 in frames for frames in calls)


# ---------------------------------------------------------------------------------------------------------------- CLI
@pytest.fixture()
def cli(rig, monkeypatch):
    runner, text = rig
    spec = importlib.util.spec_from_file_location("svr_cli_shots", os.path.join(ROOT, "inference_cli.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    itf = sub("interfaces")
    monkeypatch.setattr(itf, "get_runner", lambda *a, **k: runner)
    monkeypatch.setattr(itf, "load_text_embedding", lambda device, model_dir=None: text)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    return mod


ARGS = ["--resolution", "16", "--batch_size", "5", "--temporal_overlap", "2", "--prepend_frames", "1"]


def test_the_shipped_switch_is_off():
    shots = sub("shots")
    assert shots.ENABLED is False and set(shots.DEFAULTS) == set(PARAMS)


def test_cli_goes_through_the_shots_when_the_switch_is_on(cli, rig, tmp_path, monkeypatch):
    pipeline, shots = sub("pipeline"), sub("shots")
    runner, text = rig
    clip = shot_clip(19, 23, [7, 6], seed=9)
    assert_precondition(shots, clip, [7])
    np.save(tmp_path / "clip.npy", clip.numpy())
    kw = cli.engines(cli.build_parser().parse_args(["x.npy"] + ARGS))[2]
    whole = pipeline.upscale_shots(clip, runner, text, cuts=[7], **kw)
    streamed = torch.cat(list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, cuts=[7], **kw)))
    run = lambda name, *extra: cli.main([str(tmp_path / "clip.npy"), "--output", str(tmp_path / name)] + ARGS + list(extra))
    # off (as shipped): today's bytes
    assert run("off.pt") == 0
    assert torch.equal(torch.load(tmp_path / "off.pt", weights_only=True), pipeline.upscale(clip, runner, text, **kw))
    monkeypatch.setattr(shots, "ENABLED", True)
    monkeypatch.setattr(shots, "DEFAULTS", dict(PARAMS))
    assert run("whole.pt") == 0 and run("stream.pt", "--chunk_size", "5") == 0
    assert torch.equal(torch.load(tmp_path / "whole.pt", weights_only=True), whole)
    assert torch.equal(torch.load(tmp_path / "stream.pt", weights_only=True), streamed)
    assert not torch.equal(whole, torch.load(tmp_path / "off.pt", weights_only=True))


def test_cli_with_several_ranks_warns_once_and_behaves_as_today(cli, rig, monkeypatch, capsys):
    pipeline, shots, dist_mod = sub("pipeline"), sub("shots"), sub("dist")
    runner, text = rig
    clip = shot_clip(19, 23, [7, 6], seed=9)
    real = cli.engines

    def engines(args):
        r, t, kw, _, _ = real(args)
        return r, t, kw, 0, 2

    monkeypatch.setattr(cli, "engines", engines)
    monkeypatch.setattr(dist_mod, "upscale_sharded", lambda frames, r, t, gather="all", **kw: pipeline.upscale(frames, r, t, **kw))
    monkeypatch.setattr(shots, "ENABLED", True)
    monkeypatch.setattr(shots, "DEFAULTS", dict(PARAMS))
    args = cli.build_parser().parse_args(["x.npy", "--chunk_size", "5"] + ARGS)
    got = list(cli.run_stream(args, iter(chunked(clip))))
    kw = real(args)[2]
    want = list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, **kw))         # no cuts: batches by arithmetic alone
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))
    out, _ = cli.run(args, clip)
    assert torch.equal(out, pipeline.upscale(clip, runner, text, **kw))
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "shot-aware batching serves one GPU" in err
