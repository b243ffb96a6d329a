"""-m "not gpu": the active picture area -- active.py (the profile, the rule and the output rectangle, in exact integers),
pipeline.upscale(target_size=...) and pipeline.upscale(area=...) against the composition they stand for (bit for bit, on the fp32
torch double of the C ABI), their composition with upscale_stream and upscale_shots, and the command line behind the
active.ENABLED switch.  Every test passes its rule parameters explicitly; none reads active.DEFAULTS."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from ops_reference import TorchOps
from test_stream import tiny_runner

PARAMS = dict(dark=8, specks=0, skew=4, margin=2, gain=6)
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- profile
def naive_profile(frames, dark):
    """per pixel, in Python integers; the codes from frameio.codes"""
    T, H, W, _ = frames.shape
    q = sub("frameio").codes(frames[..., :3], 255.0).to(torch.int64).tolist()
    out = [0] * (H + W)
    for t in range(T):
        for y in range(H):
            for x in range(W):
                r, g, b = q[t][y][x]
                if ((13933 * r + 46871 * g + 4732 * b + 32768) >> 16) > dark:
                    out[y] += 1
                    out[H + x] += 1
    return torch.tensor(out, dtype=torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 4, 4, 4), (3, 19, 23, 3), (1, 130, 7, 4)], ids=lambda s: "x".join(map(str, s)))
def test_profile_equals_a_per_pixel_loop(shape, dtype):
    active = sub("active")
    T, H, W, C = shape
    x = (torch.rand(*shape, generator=torch.Generator().manual_seed(sum(shape))) * 1.2 - 0.1)
    x[:, :H // 4] = 0.0                                      # a bar, and values around the thresholds scattered into the rest
    x.view(-1)[::7] = 9 / 255
    x.view(-1)[3::11] = 8 / 255
    x = x.to(dtype)
    for dark in (0, 8, 254, 255):
        got = active.profile_torch(x, dark)
        assert got.dtype == torch.int32 and tuple(got.shape) == (H + W,)
        assert torch.equal(got, naive_profile(x, dark)), dark
        assert int(got[:H].sum()) == int(got[H:].sum())
        assert torch.equal(active.profile(x, dark), got) and torch.equal(active.profile(x, dark, ops=object()), got)
    assert int(active.profile_torch(x, 255).sum()) == 0
    if C == 4:                                               # the fourth channel is ignored
        assert torch.equal(active.profile_torch(x, 8), active.profile_torch(x[..., :3].contiguous(), 8))


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_grey_at_the_threshold_is_dark_and_one_code_above_is_not(dtype):
    """A grey k / 255 has Y8 == k (in bf16 too: the rounded value still rounds to code k), so dark / 255 is not counted and
    (dark + 1) / 255 is."""
    active = sub("active")
    T, H, W = 2, 3, 5
    for dark in (0, 8, 254):
        at = torch.full((T, H, W, 3), dark / 255).to(dtype)
        above = torch.full((T, H, W, 3), (dark + 1) / 255).to(dtype)
        assert active.profile_torch(at, dark).tolist() == [0] * (H + W)
        assert active.profile_torch(above, dark).tolist() == [T * W] * H + [T * H] * W
    assert active.profile_torch(torch.ones(T, H, W, 3, dtype=dtype), 255).tolist() == [0] * (H + W)


def test_non_finite_negative_and_large_values_follow_frameio_codes():
    active = sub("active")
    flat = lambda v: torch.full((1, 5, 6, 3), v)
    for v, lit in ((float("nan"), False), (float("inf"), True), (-float("inf"), False), (-0.3, False), (1.7, True), (-0.0, False)):
        for dtype in (torch.float32, BF16):
            p = active.profile_torch(flat(v).to(dtype), 8)
            assert p.tolist() == ([6] * 5 + [5] * 6 if lit else [0] * 11), (v, dtype)
    x = torch.rand(1, 19, 23, 3, generator=torch.Generator().manual_seed(1))
    specials = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.5, 1.5])
    x.view(-1)[torch.randperm(x.numel(), generator=torch.Generator().manual_seed(2))[:200]] = specials[torch.arange(200) % 5]
    for dark in (0, 100, 254):
        assert torch.equal(active.profile_torch(x, dark), naive_profile(x, dark))


def test_refusals_name_the_argument():
    active = sub("active")
    for shape, dtype, word in (((2, 0, 8, 3), torch.float32, "H >= 1"), ((2, 8, 0, 3), torch.float32, "W >= 1"),
                               ((0, 8, 8, 3), torch.float32, "T >= 1"), ((1, 8, 8, 2), torch.float32, "C = 3 or 4"),
                               ((1, 8, 8, 3), torch.float16, "fp32 or bf16"), ((8, 8, 3), torch.float32, r"\[T, H, W, 3 \| 4\]")):
        for call in (active.profile_torch, active.profile):
            with pytest.raises(ValueError, match=word):
                call(torch.zeros(shape, dtype=dtype), 8)
    with pytest.raises(ValueError, match=r"T \* max\(H, W\)"):
        active.check_frames(torch.empty((1 << 16, 1 << 15, 1, 3), device="meta"))
    active.check_frames(torch.empty(((1 << 16) - 1, 1 << 15, 1, 3), device="meta"))
    for bad in (-1, 256, 8.0, True, None):
        with pytest.raises(ValueError, match="dark"):
            active.profile_torch(torch.zeros(1, 4, 4, 3), bad)
        with pytest.raises(ValueError, match="dark"):
            active.Rule(**{**PARAMS, "dark": bad})
    for name in ("specks", "skew", "margin", "gain"):
        for bad in (-1, 2.0, True, None):
            with pytest.raises(ValueError, match=name):
                active.Rule(**{**PARAMS, name: bad})
    active.Rule(0, 0, 0, 0, 0)                               # zeros are values
    with pytest.raises(ValueError, match="profile"):
        active.Rule(**PARAMS).area([0] * 10, 1, 4, 5)
    with pytest.raises(ValueError, match="area"):
        active.out_rect((4, 4, 0, 8), 8, 8, 16, 16)
    with pytest.raises(ValueError, match="TH"):
        active.out_rect((0, 8, 0, 8), 8, 8, 15, 16)


# ---------------------------------------------------------------------------------------------------------------- the rule
T0, H0, W0 = 6, 32, 40                                       # the rule table's clip: T W = 240 per row, T H = 192 per column
FULL = (0, H0, 0, W0)


def bars(top=0, bottom=0, left=0, right=0, rows=None, cols=None):
    """The profile of black bars of these sizes around a picture with every pixel lit; ``rows`` / ``cols``: {line: count} on top."""
    r = [0 if (y < top or y >= H0 - bottom) else T0 * (W0 - left - right) for y in range(H0)]
    c = [0 if (x < left or x >= W0 - right) else T0 * (H0 - top - bottom) for x in range(W0)]
    for y, n in (rows or {}).items():
        r[y] = n
    for x, n in (cols or {}).items():
        c[x] = n
    return r + c


BAR_ROWS = list(range(6)) + list(range(26, 32))
RULE_TABLE = [
    # name, parameters over PARAMS, profile, expected area -- written by hand from the seven steps of active.py's docstring
    ("symmetric letterbox", {}, bars(6, 6), (4, 28, 0, 40)),
    ("pillarbox", {}, bars(0, 0, 8, 8), (0, 32, 6, 34)),
    ("both, one line apart", {}, bars(6, 5, 8, 7), (4, 29, 6, 35)),
    ("skew of exactly `skew` passes", {}, bars(8, 4), (6, 30, 0, 40)),
    ("a skew beyond `skew` drops the rows only", {}, bars(10, 2, 8, 8), (0, 32, 6, 34)),
    ("a skew beyond `skew` drops the columns only", {}, bars(6, 6, 9, 2), (4, 28, 0, 40)),
    ("a skewed axis alone: nothing to crop", {}, bars(10, 2), FULL),
    ("everything dark", {}, [0] * (H0 + W0), FULL),
    ("all rows dark, columns lit (inconsistent on purpose)", {}, [0] * H0 + [192] * W0, FULL),
    ("interior dark lines mean nothing", {}, bars(6, 6, rows={15: 0, 16: 0}, cols={20: 0}), (4, 28, 0, 40)),
    ("a saving of 6.25 % passes gain = 6", dict(margin=0), bars(1, 1), (1, 31, 0, 40)),
    ("a saving of 6.25 % is below gain = 7", dict(margin=0, gain=7), bars(1, 1), FULL),
    ("a picture of 16 lines is cropped to", dict(margin=0), bars(8, 8), (8, 24, 0, 40)),
    ("a picture of 14 lines is not", dict(margin=0), bars(9, 9), FULL),
    ("a picture of 14 columns is not", dict(margin=0), bars(0, 0, 13, 13), FULL),
    # specks = 12500 ppm of T W = 240 pixels: 3 bright pixels in a row are tolerated (3e6 <= 3e6), 4 are not
    ("specks tolerates exactly its count", dict(specks=12500), bars(6, 6, rows={y: 3 for y in BAR_ROWS}), (4, 28, 0, 40)),
    ("and not one more: that line ends the bar", dict(specks=12500), bars(6, 6, rows={**{y: 3 for y in BAR_ROWS}, 5: 4}), (3, 28, 0, 40)),
    ("and not one more, every bar line: no bars", dict(specks=12500), bars(6, 6, rows={y: 4 for y in BAR_ROWS}), FULL),
    # the columns' own denominator, T H = 192: 12500 ppm tolerate 2 (2e6 <= 2.4e6), not 3
    ("specks for a column counts T H", dict(specks=12500), bars(0, 0, 8, 8, cols={x: 2 for x in list(range(8)) + list(range(32, 40))}),
     (0, 32, 6, 34)),
    ("specks for a column, one more", dict(specks=12500), bars(0, 0, 8, 8, cols={x: 3 for x in list(range(8)) + list(range(32, 40))}), FULL),
    ("margin clipped at the frame edge", {}, bars(1, 1, 8, 8), (0, 32, 6, 34)),
    ("margin keeps lines of the bar", dict(margin=5), bars(6, 6), (1, 31, 0, 40)),
    ("one bright pixel in one frame's bar keeps that bar: row 2", {}, bars(6, 6, rows={2: 1}), (0, 28, 0, 40)),
    ("one bright pixel in row 0: the skew test then drops the axis", {}, bars(6, 6, rows={0: 1}), FULL),
]


@pytest.mark.parametrize("name,over,profile,want", RULE_TABLE, ids=[r[0] for r in RULE_TABLE])
def test_rule_table(name, over, profile, want):
    active = sub("active")
    rule = active.Rule(**{**PARAMS, **over})
    assert rule.area(profile, T0, H0, W0) == want
    assert rule.area(profile, T0, H0, W0) == want            # stateless


def test_rule_on_a_real_profile_with_one_bright_pixel():
    active = sub("active")
    clip = letterboxed(channels=3)
    rule = active.Rule(**PARAMS)
    assert rule.area(active.profile_torch(clip, 8).tolist(), 6, 32, 40) == (4, 28, 0, 40)
    clip[3, 2, 17] = 1.0                                     # one pixel of one frame, in the top bar
    assert rule.area(active.profile_torch(clip, 8).tolist(), 6, 32, 40) == (0, 28, 0, 40)


# ---------------------------------------------------------------------------------------------------------------- the rectangle
def test_out_rect_is_even_contains_the_scaled_area_and_is_less_than_two_pixels_off():
    active, transforms = sub("active"), sub("transforms")
    rng = random.Random(5)
    for H in (32, 480, 720, 1080):
        for W in (H * 16 // 9, H, (H * 3) // 4 + 1):
            for res in (48, 720, 1080, 2160):
                TH, TW = transforms.true_target_dims(H, W, res)
                assert TH % 2 == 0 and TW % 2 == 0
                assert active.out_rect((0, H, 0, W), H, W, TH, TW) == (0, TH, 0, TW)
                for _ in range(25):
                    y0, x0 = rng.randrange(0, H - 16), rng.randrange(0, W - 16)
                    y1, x1 = rng.randrange(y0 + 16, H + 1), rng.randrange(x0 + 16, W + 1)
                    oy0, oy1, ox0, ox1 = active.out_rect((y0, y1, x0, x1), H, W, TH, TW)
                    for o0, o1, a0, a1, n, tn in ((oy0, oy1, y0, y1, H, TH), (ox0, ox1, x0, x1, W, TW)):
                        assert o0 % 2 == 0 and o1 % 2 == 0 and 0 <= o0 < o1 <= tn
                        assert o0 * n <= a0 * tn < (o0 + 2) * n          # o0 <= a0 tn / n < o0 + 2, in integers
                        assert (o1 - 2) * n < a1 * tn <= o1 * n          # o1 - 2 < a1 tn / n <= o1


# ---------------------------------------------------------------------------------------------------------------- pipeline
KW = dict(resolution=48, batch_size=5, temporal_overlap=1, color_correction="lab")


def letterboxed(channels=3, frames=6, seed=3):
    """``frames`` frames of 32 x 40: rows 6..25 random in [0.1, 1] (luma code 26 and up), the rest 0; alpha random everywhere"""
    g = torch.Generator().manual_seed(seed)
    clip = torch.zeros(frames, 32, 40, channels)
    clip[:, 6:26, :, :3] = torch.rand(frames, 20, 40, 3, generator=g) * 0.9 + 0.1
    if channels == 4:
        clip[..., 3] = torch.rand(frames, 32, 40, generator=g)
    return clip


def full_picture(channels=3, frames=6, seed=4):
    return torch.rand(frames, 32, 40, channels, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


@pytest.fixture(scope="module")
def rig():
    return tiny_runner(TorchOps("cpu", act_dtype=torch.float32)), sub("weights").synth_text_embedding().float()


def canvas_of(clip, resolution=48, max_resolution=0):
    """the statement of upscale's docstring, for the output dtype fp32"""
    transforms = sub("transforms")
    th, tw = transforms.true_target_dims(clip.shape[1], clip.shape[2], resolution, max_resolution)
    y = transforms.side_resize(clip.permute(0, 3, 1, 2).float(), resolution, max_resolution).clamp(0, 1)[..., :th, :tw]
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("channels,prepend", [(3, 0), (4, 0), (3, 1), (4, 1)], ids=["rgb", "rgba", "rgb-prepend", "rgba-prepend"])
def test_area_is_the_picture_alone_inside_a_plain_resize(rig, channels, prepend):
    pipeline, active = sub("pipeline"), sub("active")
    runner, text = rig
    clip = letterboxed(channels)
    kw = dict(prepend_frames=prepend, **KW)
    prof = active.profile_torch(clip, 8).tolist()
    assert prof[:32] == [0] * 6 + [240] * 20 + [0] * 6 and prof[32:] == [120] * 40
    rule = active.Rule(**PARAMS)
    assert rule.area(prof, 6, 32, 40) == (4, 28, 0, 40) and active.out_rect((4, 28, 0, 40), 32, 40, 48, 60) == (6, 42, 0, 60)
    got = pipeline.upscale(clip, runner, text, area=rule, **kw)
    assert tuple(got.shape) == (6, 48, 60, channels) and got.dtype == torch.float32
    inner = pipeline.upscale(clip[:, 4:28].contiguous(), runner, text, target_size=(36, 60), **kw)
    assert tuple(inner.shape) == (6, 36, 60, channels)
    assert torch.equal(got[:, 6:42], inner)
    canvas = canvas_of(clip)
    assert torch.equal(got[:, :6], canvas[:, :6]) and torch.equal(got[:, 42:], canvas[:, 42:])
    assert torch.equal(pipeline.upscale(clip, runner, text, area=(4, 28, 0, 40), **kw), got)
    if channels == 3 and prepend == 0:                       # and it is not what the whole frame gives
        assert not torch.equal(got[:, 6:42], pipeline.upscale(clip, runner, text, **kw)[:, 6:42])


def test_a_full_frame_area_and_target_size_of_the_side_rule_are_the_plain_call(rig):
    pipeline, active, transforms = sub("pipeline"), sub("active"), sub("transforms")
    runner, text = rig
    clip = full_picture(4)
    kw = dict(prepend_frames=1, **KW)
    plain = pipeline.upscale(clip, runner, text, **kw)
    assert torch.equal(pipeline.upscale(clip, runner, text, area=(0, 32, 0, 40), **kw), plain)
    assert torch.equal(pipeline.upscale(clip, runner, text, area=active.Rule(**PARAMS), **kw), plain)
    assert transforms.resized_output_size(32, 40, 48) == (48, 60)
    assert torch.equal(pipeline.upscale(clip, runner, text, target_size=(48, 60), max_resolution=0, **kw), plain)
    # a size of its own: the transform goes straight there and the frames are trimmed to it
    out = pipeline.upscale(clip[:2], runner, text, target_size=(38, 50), **kw)
    assert tuple(out.shape) == (2, 38, 50, 4)
    x = torch.rand(3, 3, 20, 24)
    direct = transforms.video_transform(x, 0, 0, size=(38, 50))
    assert tuple(direct.shape) == (3, 3, 48, 64)
    want = torch.nn.functional.interpolate(x, size=[38, 50], mode="bicubic", align_corners=False, antialias=True).clamp(0, 1)
    assert torch.equal(direct[:, :, :38, :50], ((want - 0.5) / 0.5).permute(1, 0, 2, 3)) and bool((direct[:, :, 38:] == -1).all())
    plan = pipeline.BatchPlan(0, 3, 0)
    assert pipeline.transformed_shape(clip, plan, 48, size=(38, 50)) == (3, 5, 48, 64)
    assert tuple(pipeline.prepare_batch(clip, plan, 48, size=(38, 50)).shape) == (3, 5, 48, 64)


def test_pipeline_refusals_name_the_argument(rig):
    pipeline, active = sub("pipeline"), sub("active")
    runner, text = rig
    clip = letterboxed()
    for name, value in (("batch_filter", lambda i: True), ("exchange_heads", lambda *a: {}), ("return_spans", True)):
        with pytest.raises(ValueError, match=name):
            pipeline.upscale(clip, runner, text, area=active.Rule(**PARAMS), **{name: value}, **KW)
        with pytest.raises(ValueError, match=name):
            pipeline.upscale(clip, runner, text, target_size=(36, 60), **{name: value}, **KW)
    with pytest.raises(ValueError, match="target_size"):
        pipeline.upscale(clip, runner, text, area=(4, 28, 0, 40), target_size=(36, 60), **KW)
    for bad in ((35, 60), (36, 0), (36, 60.0), (36,), 36, (-2, 60), (True, 60)):
        with pytest.raises(ValueError, match="target_size"):
            pipeline.upscale(clip, runner, text, target_size=bad, **KW)
    for bad in ((4, 28, 0), (-1, 28, 0, 40), (4, 33, 0, 40), (28, 4, 0, 40), (4, 19, 0, 40), (4, 28, 30, 40), (4, 28, 0, 41),
                (4.0, 28, 0, 40), "rule", (4, 28, 5, 5)):
        with pytest.raises(ValueError, match="area"):
            pipeline.upscale(clip, runner, text, area=bad, **KW)


def test_a_rule_costs_one_read_back_of_the_backends_profile(rig, monkeypatch):
    """The profile goes through the runner's backend where it has one (here: a recording stand-in on the CPU double) and is taken of
    the frames the call received, before prepend_frames."""
    pipeline, active = sub("pipeline"), sub("active")
    runner, text = rig
    clip = letterboxed()
    seen = []

    def active_profile(frames, dark):
        seen.append((tuple(frames.shape), dark))
        return active.profile_torch(frames, dark)

    monkeypatch.setattr(runner.dit.ops, "active_profile", active_profile, raising=False)
    got = pipeline.upscale(clip, runner, text, area=active.Rule(**{**PARAMS, "dark": 9}), prepend_frames=1, **KW)
    assert seen == [((6, 32, 40, 3), 9)]
    monkeypatch.delattr(runner.dit.ops, "active_profile")
    assert torch.equal(got, pipeline.upscale(clip, runner, text, area=(4, 28, 0, 40), prepend_frames=1, **KW))


# ---------------------------------------------------------------------------------------------------------------- composition
def chunked(frames, n=5):
    return [frames[i:i + n] for i in range(0, frames.shape[0], n)]


def test_stream_serves_the_area_per_context_and_chunk(rig):
    pipeline, active = sub("pipeline"), sub("active")
    runner, text = rig
    clip = letterboxed(frames=8, seed=5)
    rule = active.Rule(**PARAMS)
    kw = dict(prepend_frames=1, **KW)
    got = list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, area=rule, **kw))
    assert [tuple(o.shape) for o in got] == [(5, 48, 60, 3), (3, 48, 60, 3)]
    assert torch.equal(got[0], pipeline.upscale(clip[:5], runner, text, area=rule, **kw))
    assert torch.equal(got[1], pipeline.upscale(clip[4:], runner, text, area=rule, **{**kw, "prepend_frames": 0})[1:])
    assert torch.equal(got[1][:, 6:42], pipeline.upscale(clip[4:, 4:28].contiguous(), runner, text, target_size=(36, 60),
                                                         **{**kw, "prepend_frames": 0})[1:])


def test_shots_serve_the_area_per_shot(rig):
    """The second shot has no bars: the first is cropped, the second is not."""
    pipeline, active = sub("pipeline"), sub("active")
    runner, text = rig
    clip = torch.cat([letterboxed(frames=6, seed=6), full_picture(frames=5, seed=7)])
    rule = active.Rule(**PARAMS)
    got = pipeline.upscale_shots(clip, runner, text, cuts=[6], area=rule, **KW)
    first, second = pipeline.upscale(clip[:6], runner, text, area=rule, **KW), pipeline.upscale(clip[6:], runner, text, **KW)
    assert torch.equal(got, torch.cat([first, second]))
    assert torch.equal(first[:, 6:42], pipeline.upscale(clip[:6, 4:28].contiguous(), runner, text, target_size=(36, 60), **KW))
    assert not torch.equal(first, pipeline.upscale(clip[:6], runner, text, **KW))
    # the whole clip as one call would see lit rows everywhere: no area
    assert rule.area(active.profile_torch(clip, 8).tolist(), 11, 32, 40) == (0, 32, 0, 40)


# ---------------------------------------------------------------------------------------------------------------- CLI
@pytest.fixture()
def cli(rig, monkeypatch):
    runner, text = rig
    spec = importlib.util.spec_from_file_location("svr_cli_active", os.path.join(ROOT, "inference_cli.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    itf = sub("interfaces")
    monkeypatch.setattr(itf, "get_runner", lambda *a, **k: runner)
    monkeypatch.setattr(itf, "load_text_embedding", lambda device, model_dir=None: text)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    return mod


ARGS = ["--resolution", "48", "--batch_size", "5", "--temporal_overlap", "1", "--prepend_frames", "1"]


def test_the_shipped_switch_is_off():
    active = sub("active")
    assert active.ENABLED is False and set(active.DEFAULTS) == set(PARAMS)


def test_cli_passes_a_rule_on_all_three_routes_when_the_switch_is_on(cli, rig, tmp_path, monkeypatch):
    pipeline, active, shots = sub("pipeline"), sub("active"), sub("shots")
    runner, text = rig
    clip = letterboxed(frames=8, seed=8)
    np.save(tmp_path / "clip.npy", clip.numpy())
    kw = cli.engines(cli.build_parser().parse_args(["x.npy"] + ARGS))[2]
    rule = active.Rule(**PARAMS)
    whole = pipeline.upscale(clip, runner, text, area=rule, **kw)
    streamed = torch.cat(list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, area=rule, **kw)))
    run = lambda name, *extra: cli.main([str(tmp_path / "clip.npy"), "--output", str(tmp_path / name)] + ARGS + list(extra))
    # off (as shipped): today's bytes
    assert run("off.pt") == 0
    off = torch.load(tmp_path / "off.pt", weights_only=True)
    assert torch.equal(off, pipeline.upscale(clip, runner, text, **kw)) and not torch.equal(off, whole)
    monkeypatch.setattr(active, "ENABLED", True)
    monkeypatch.setattr(active, "DEFAULTS", dict(PARAMS))
    assert run("whole.pt") == 0 and run("stream.pt", "--chunk_size", "5") == 0
    assert torch.equal(torch.load(tmp_path / "whole.pt", weights_only=True), whole)
    assert torch.equal(torch.load(tmp_path / "stream.pt", weights_only=True), streamed)
    # the shots route: the keyword reaches upscale_shots next to the detector
    seen, real = [], pipeline.upscale_shots

    def recording(frames, r, t, **kwargs):
        seen.append(kwargs)
        return real(frames, r, t, **kwargs)

    monkeypatch.setattr(pipeline, "upscale_shots", recording)
    monkeypatch.setattr(shots, "ENABLED", True)
    monkeypatch.setattr(shots, "DEFAULTS", dict(percent=30, ratio=3, window=8, min_shot=3))
    assert run("shots.pt") == 0
    assert len(seen) == 1 and isinstance(seen[0]["cuts"], shots.Detector) and isinstance(seen[0]["area"], active.Rule)
    assert vars(seen[0]["area"]) == PARAMS
    assert torch.equal(torch.load(tmp_path / "shots.pt", weights_only=True), whole)          # (no cut in this clip)


def test_cli_with_several_ranks_warns_once_and_behaves_as_today(cli, rig, monkeypatch, capsys):
    pipeline, active, dist_mod = sub("pipeline"), sub("active"), sub("dist")
    runner, text = rig
    clip = letterboxed(frames=8, seed=8)
    real = cli.engines

    def engines(args):
        r, t, kw, _, _ = real(args)
        return r, t, kw, 0, 2

    monkeypatch.setattr(cli, "engines", engines)
    monkeypatch.setattr(dist_mod, "upscale_sharded", lambda frames, r, t, gather="all", **kw: pipeline.upscale(frames, r, t, **kw))
    monkeypatch.setattr(active, "ENABLED", True)
    monkeypatch.setattr(active, "DEFAULTS", dict(PARAMS))
    args = cli.build_parser().parse_args(["x.npy", "--chunk_size", "5"] + ARGS)
    got = list(cli.run_stream(args, iter(chunked(clip))))
    kw = real(args)[2]
    want = list(pipeline.upscale_stream(iter(chunked(clip)), runner, text, **kw))           # no area: the whole frame
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want))
    out, _ = cli.run(args, clip)
    assert torch.equal(out, pipeline.upscale(clip, runner, text, **kw))
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "the active picture area serves one GPU" in err
