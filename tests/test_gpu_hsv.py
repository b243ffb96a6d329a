"""-m gpu: the HSV kernels (csrc/svr_hsv.hip, the partitions of csrc/svr_rank.hip) against colorfix.py, their specification.

  hsv_planes / hsv_merge   bit-equal to the CPU run of colorfix.rgb_to_hsv / hsv_to_rgb, random pixels and a crafted set, dense operands
                           and the pipeline's two views, every output in a poisoned, guarded canvas
  hue_match                bit-equal to colorfix.hue_match_spec on the same planes: unequal bins, heavy ties, a run across the tile and
                           the 16-tile workgroup, bins at 100 / 101 pixels, empty bins, the wrap class, hues at every edge, in place
  correct(.., "hsv")       bit-equal to colorfix.hsv_spec on the CPU
  wavelet_adaptive         the mask exact; the blend against an fp64 evaluation with a MEASURED bound: twice the largest error of the CPU's
                           fp32 expression against the same fp64 values (the factor allows an exp that rounds differently but as well)
  pipeline.upscale         hsv and wavelet_adaptive over toy-width engines against the same call with the torch route forced

Figures measured on MI355X are in profiles/colorfix.txt."""
import functools

import pytest
import torch

from conftest import sub
from guarded_out import Pool
from test_hsv_match import MIN_PIXEL_CASES, _pair, _planes

pytestmark = pytest.mark.gpu
F32 = torch.float32
INF = float("inf")


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def _bits_equal(got, want):
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def _pipeline_views(content, style):
    """content as ``final[w0:w1]`` (channels last), style as a [:, :, :H, :W] slice of a larger [C, T, H + 3, W + 5] buffer whose
    padding holds NaN (tests/test_gpu_colorfix.py)"""
    T, _, H, W = content.shape
    frames = content.permute(0, 2, 3, 1).contiguous().cuda()
    big = torch.full((3, T, H + 3, W + 5), float("nan"), device="cuda")
    big[:, :, :H, :W] = style.permute(1, 0, 2, 3).cuda()
    return frames.permute(0, 3, 1, 2), big.permute(1, 0, 2, 3)[:, :, :H, :W]


def _to01(x):
    return ((x + 1.0) * 0.5).clamp(0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------- conversions
def _crafted():
    """[-1, 1] pixels [n, 3]: greys, black, white, the six primaries and secondaries, two-channel ties (every pair, as maximum and
    as minimum), -1 and 1, out of range, +-inf, and the smallest ranges fp32 inputs can reach: one fp32 step above -1 is 2^-24, so
    after (x + 1) * 0.5 the range next to the 1e-10 guard is 2^-25 (above it) or 0 (below it)."""
    up = torch.nextafter(torch.tensor(-1.0), torch.tensor(0.0)).item()            # -1 + 2^-24
    dn = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)).item()
    px = [(g, g, g) for g in (-1.0, -0.5, 0.0, 0.3, 1.0, up, dn)]
    px += [(r, g, b) for r in (-1.0, 1.0) for g in (-1.0, 1.0) for b in (-1.0, 1.0)]
    for hi, lo in ((0.5, -0.2), (-0.2, 0.5), (1.0, -1.0), (-1.0, 1.0), (0.25, 0.125)):
        px += [(hi, hi, lo), (hi, lo, hi), (lo, hi, hi)]
    px += [(1.5, -2.0, 0.3), (3.0, 3.0, -3.0), (-1.25, 0.0, 7.0), (INF, 0.0, -INF), (INF, INF, 0.2), (-INF, -INF, -INF), (0.1, -INF, INF)]
    px += [(up, -1.0, -1.0), (-1.0, up, -1.0), (-1.0, -1.0, up), (up, up, -1.0), (up, -1.0, up), (-1.0, up, up)]
    # red maximum with green a step below blue: (g - b) / d is a tiny negative, + 6 rounds to 6.0 and h to 1.0
    px += [(0.5, -0.5, -0.5 + 2.0 ** -24), (0.5, -0.5 + 2.0 ** -24, -0.5), (1.0, up, -1.0), (1.0, -1.0, up)]
    return torch.tensor(px, dtype=F32)


@functools.lru_cache(maxsize=None)
def _frames(T, H, W):
    g = torch.Generator().manual_seed(T * 1000 + W)
    x = torch.rand(T * H * W, 3, generator=g) * 2.4 - 1.2                          # some channels out of range
    crafted = _crafted()
    k = min(crafted.shape[0], T * H * W)
    x[:k] = crafted[torch.randperm(crafted.shape[0], generator=g)[:k]]             # (the 37 x 131 case holds all of them)
    y = (torch.rand(T * H * W, 3, generator=g) * 2 - 1) * 0.7
    y[-k:] = crafted[:k]
    frames = lambda v: v.reshape(T, H, W, 3).permute(0, 3, 1, 2).contiguous()
    return frames(x), frames(y)


@pytest.mark.parametrize("layout", ["dense", "pipeline"])
@pytest.mark.parametrize("T,H,W", [(1, 5, 9), (2, 37, 131), (1, 1, 257)])
def test_hsv_planes_and_merge_equal_the_cpu_run_bit_for_bit(hip, T, H, W, layout):
    cf = sub("colorfix")
    content, style = _frames(T, H, W)
    n = T * H * W
    assert (T, H, W) != (2, 37, 131) or n >= _crafted().shape[0]
    planes = lambda x: cf.rgb_to_hsv(_to01(x)).permute(1, 0, 2, 3).reshape(3, -1).contiguous()
    want_c, want_s = planes(content), planes(style)[:2].contiguous()
    assert torch.isfinite(want_c).all() and torch.isfinite(want_s).all()
    c, s = (content.cuda(), style.cuda()) if layout == "dense" else _pipeline_views(content, style)
    pool = Pool()
    c_hsv, s_hs = hip.hsv_planes(c, s, c_hsv=pool(3, n, dtype=F32), s_hs=pool(2, n, dtype=F32))
    torch.cuda.synchronize()
    pool.check(f"hsv_planes {T}x{H}x{W} {layout}")
    for name, got, want in (("content", c_hsv, want_c), ("style", s_hs, want_s)):
        bad = got.cpu().view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), (name, int(bad.sum()), bad.nonzero()[0].tolist())
    fresh = hip.hsv_planes(c, s)
    assert _bits_equal(fresh[0], want_c) and _bits_equal(fresh[1], want_s)

    # merge: the planes above with the saturation as it is, then replaced by random ones (what the matching does to it)
    g = torch.Generator().manual_seed(7)
    for sat in (want_c[1], torch.rand(n, generator=g), torch.full((n,), 1.0), torch.zeros(n)):
        hsv = torch.stack([want_c[0].reshape(T, H, W), sat.reshape(T, H, W), want_c[2].reshape(T, H, W)], dim=1)
        want = cf.hsv_to_rgb(hsv).clamp(0.0, 1.0) * 2.0 - 1.0
        out = pool(T, 3, H, W, dtype=F32) if layout == "dense" else pool(T, H, W, 3, dtype=F32).permute(0, 3, 1, 2)
        got = hip.hsv_merge(c_hsv[0], sat.cuda(), c_hsv[2], (T, H, W), out=out)
        torch.cuda.synchronize()
        pool.check(f"hsv_merge {T}x{H}x{W} {layout}")
        assert got.data_ptr() == out.data_ptr() and _bits_equal(got, want)
    assert _bits_equal(hip.hsv_merge(c_hsv[0], c_hsv[1], c_hsv[2], (T, H, W)), cf.hsv_to_rgb(
        torch.stack([want_c[k].reshape(T, H, W) for k in range(3)], dim=1)).clamp(0.0, 1.0) * 2.0 - 1.0)


# ---------------------------------------------------------------------------------------------------------------- hue_match
def _pad(h, s, n):
    """planes lengthened to n with pixels of no bin (NaN hue): both sides of a call hold one number of pixels"""
    k = n - h.numel()
    return torch.cat([h, torch.full((k,), float("nan"))]), torch.cat([s, torch.rand(k, generator=torch.Generator().manual_seed(k))])


def _frame_planes(hip, content, style):
    """the device's own planes, copied to the CPU"""
    c_hsv, s_hs = hip.hsv_planes(content.cuda(), style.cuda())
    return c_hsv[0].cpu(), c_hsv[1].cpu(), s_hs[0].cpu(), s_hs[1].cpu()


def _match_cases(hip):
    cf = sub("colorfix")
    cases = {}
    content, style = _pair(3, 96, 160)
    cases["random_frames_unequal_bins"] = _frame_planes(hip, content, style)
    q = lambda x: (x * 127.5).round() / 127.5
    content, style = _pair(2, 64, 96, seed=21)
    cases["quantised_frames_heavy_ties"] = _frame_planes(hip, q(content), q(style))
    g = torch.Generator().manual_seed(31)
    n = 256 * 257                                                 # one bin: a run across the 4096-key tile and the 16-tile workgroup
    one = lambda lo: (lo + torch.rand(n, generator=g) * 0.02, (torch.rand(n, generator=g) * 255).round() / 255)
    cases["one_bin_256x257"] = one(0.30) + one(0.31)
    cases["bin_0_from_three_classes"] = (
        torch.tensor([0.95, 0.01, 1.0, 0.02, 0.99, 1.5, cf.HUE_EDGES[11], 0.0, -0.0])[torch.randint(0, 9, (n,), generator=g)],
        (torch.rand(n, generator=g) * 15).round() / 15) + one(0.93)
    for name, (c_counts, s_counts, _) in MIN_PIXEL_CASES.items():
        c_h, c_s = _planes(cf, c_counts, 1)
        s_h, s_s = _planes(cf, s_counts, 2)
        m = max(c_h.numel(), s_h.numel())
        cases["counts_" + name] = _pad(c_h, c_s, m) + _pad(s_h, s_s, m)
    edges = []
    for e in list(cf.HUE_EDGES) + [cf.HUE_WRAP_EDGE]:
        t = torch.tensor(e, dtype=F32)
        edges += [torch.nextafter(t, torch.tensor(-INF)).item(), e, torch.nextafter(t, torch.tensor(INF)).item()]
    edges = torch.tensor(edges + [-0.0, float("nan"), 2.0, -0.5], dtype=F32)
    n = 3 * 4096 + 5
    planted = lambda: (edges[torch.randint(0, edges.numel(), (n,), generator=g)], (torch.rand(n, generator=g) * 31).round() / 31)
    cases["hues_at_every_edge"] = planted() + planted()
    return cases


CASE_NAMES = ["random_frames_unequal_bins", "quantised_frames_heavy_ties", "one_bin_256x257", "bin_0_from_three_classes",
              "hues_at_every_edge"] + ["counts_" + k for k in sorted(MIN_PIXEL_CASES)]


@functools.lru_cache(maxsize=None)
def _cases_and_specs():
    hip = sub("ops").HipOps("cuda:0")
    cf = sub("colorfix")
    cases = _match_cases(hip)
    assert sorted(cases) == sorted(CASE_NAMES)
    return {k: (v, cf.hue_match_spec(*v)) for k, v in cases.items()}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_hue_match_equals_the_specification_bit_for_bit(hip, name):
    cf = sub("colorfix")
    (c_h, c_s, s_h, s_s), want = _cases_and_specs()[name]
    n = c_h.numel()
    qualifying = [k for k in range(12) if int(cf.hue_bin_mask(c_h, k).sum()) > 100 and int(cf.hue_bin_mask(s_h, k).sum()) > 100]
    print(f"hue_match {name}: n = {n}, qualifying bins {qualifying}, {int((want != c_s).sum())} saturations move")
    if name == "random_frames_unequal_bins":
        assert qualifying == list(range(12))
        assert all(int(cf.hue_bin_mask(c_h, k).sum()) != int(cf.hue_bin_mask(s_h, k).sum()) for k in range(12))
    dev = [t.cuda() for t in (c_h, c_s, s_h, s_s)]
    pool = Pool()
    got = hip.hue_match(*dev, out=pool(n, dtype=F32))
    torch.cuda.synchronize()
    pool.check(f"hue_match {name}")
    bad = got.cpu().view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[0].tolist())
    for t, src in zip(dev, (c_h, c_s, s_h, s_s)):                 # the inputs are not modified
        assert _bits_equal(t, src)
    again = hip.hue_match(*dev)                                   # a second run, the buffer HipOps allocates itself
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    in_place = pool(n, dtype=F32, init=dev[1])                    # out = c_s itself, inside guards
    res = hip.hue_match(dev[0], in_place, dev[2], dev[3], out=in_place)
    torch.cuda.synchronize()
    pool.check(f"hue_match {name} in place", written=False)
    assert res.data_ptr() == in_place.data_ptr() and _bits_equal(res, want)


# ---------------------------------------------------------------------------------------------------------------- composed
@functools.lru_cache(maxsize=None)
def _spec(method):
    cf = sub("colorfix")
    content, style = _pair(3, 96, 160)
    return {"hsv": cf.hsv_spec, "wavelet_adaptive": cf.wavelet_adaptive_spec}[method](content.clone(), style.clone())


@pytest.mark.parametrize("layout", ["dense", "pipeline"])
def test_correct_hsv_equals_the_specification_bit_for_bit(hip, layout):
    cf = sub("colorfix")
    content, style = _pair(3, 96, 160)
    c, s = (content.cuda(), style.cuda()) if layout == "dense" else _pipeline_views(content, style)
    assert cf.HSV_MATCH and cf.routes_to_device(c, s, "hsv", hip)
    got = cf.correct(c, s, "hsv", ops=hip)
    want = _spec("hsv")
    assert got.is_cuda and got.shape == want.shape and got.dtype == want.dtype
    bad = got.cpu() != want
    assert not bool(bad.any()), (int(bad.sum()), float((got.cpu() - want).abs().max()))
    assert _bits_equal(got, want)
    d = (got.cpu() - cf.METHODS["hsv"](content, style)).abs()     # for orientation: the torch route on the CPU
    print(f"correct('hsv') {layout}: against METHODS on the CPU: share off by more than 2e-5: {float((d > 2e-5).float().mean()):.3e}, "
          f"max {float(d.max()):.3e}")


@pytest.mark.parametrize("layout", ["dense", "pipeline"])
def test_adaptive_blend_mask_exact_and_weight_within_the_measured_bound(hip, layout):
    cf = sub("colorfix")
    content, style = _pair(3, 96, 160)
    T, _, H, W = content.shape
    threshold, sharpness = 0.15, 5.0
    base = cf.wavelet_reconstruction(content, style)              # (the kernel's result is this bit for bit: test_gpu_colorfix.py)
    hsv = _spec("hsv")
    w32, mask = cf.adaptive_weight(base, content, style, threshold, sharpness)
    cpu = base * (1.0 - w32) + hsv * w32                          # the CPU's fp32 torch expression
    sat = cf.saturation_map                                       # exact operations: the same bits on both sides
    w64 = torch.sigmoid(sharpness * (sat(content).double() - sat(style).double() - threshold)) * mask.double()
    want = base.double() * (1.0 - w64) + hsv.double() * w64
    bound = 2.0 * float((cpu.double() - want).abs().max())
    c, s = (content.cuda(), style.cuda()) if layout == "dense" else _pipeline_views(content, style)
    assert cf.routes_to_device(c, s, "wavelet_adaptive", hip)
    got = cf.correct(c, s, "wavelet_adaptive", ops=hip).cpu()
    worst = float((got.double() - want).abs().max())
    print(f"wavelet_adaptive {layout}: max |error| vs fp64: CPU fp32 {bound / 2:.3e}, device {worst:.3e} (bound {bound:.3e}); "
          f"mask set at {float(mask.float().mean()):.3f} of the pixels")
    assert torch.isfinite(got).all() and 0.05 < float(mask.float().mean()) < 0.95
    # the mask: outside it w == 0 and the base passes through; inside it w > 0 moves every channel whose two sources differ
    outside = (~mask).expand_as(base)
    assert torch.equal(got[outside], (base * 1.0 + hsv * 0.0)[outside])
    moved = mask.expand_as(base) & ((hsv - base).abs() > 1e-3)
    assert int(moved.sum()) > 1000 and bool((got[moved] != base[moved]).all())
    assert worst <= bound, (worst, bound)
    d = (got - _spec("wavelet_adaptive")).abs()
    print(f"wavelet_adaptive {layout}: against wavelet_adaptive_spec on the CPU: {int((d > 0).sum())} values differ, max {float(d.max()):.3e}")


@pytest.fixture(scope="module")
def toy_runner(hip):
    config, weights, dit, vae, runner = (sub(n) for n in ("config", "weights", "dit", "vae", "runner"))
    dcfg, vcfg = config.DIT_TINY, config.VAEConfig(block_out_channels=(128, 128, 128, 128))
    r = runner.VideoDiffusionInfer(runner.default_config(dcfg, vcfg))
    r.dit = dit.NaDiTEngine(dcfg, weights.synth_dit_state_dict(dcfg, seed=21), hip)
    r.vae = vae.VideoVAEEngine(vcfg, weights.synth_vae_state_dict(vcfg, seed=22), hip)
    return r, weights.synth_text_embedding().cuda()


@pytest.mark.parametrize("method", ["hsv", "wavelet_adaptive"])
def test_pipeline_upscale_against_the_torch_route(toy_runner, monkeypatch, method):
    """pipeline.upscale over toy-width HIP engines (the test of tests/test_gpu_colorfix.py for these two methods): phase 4 on the
    kernels against the same call with colorfix.correct forced to impl="torch", within that file's composed caps."""
    cf, pipeline = sub("colorfix"), sub("pipeline")
    r, txt = toy_runner
    images = torch.rand(9, 24, 40, 3, generator=torch.Generator().manual_seed(4)).cuda()
    kw = dict(resolution=48, batch_size=5, uniform_batch_size=True, temporal_overlap=2, color_correction=method)
    routed, real = [], cf.correct

    def spy(content, style, m, ops=None, impl="auto"):
        routed.append(cf.routes_to_device(content, style, m, ops) and cf._hsv_on_kernels(content, ops))
        return real(content, style, m, ops=ops, impl=impl)

    monkeypatch.setattr(cf, "correct", spy)
    got = pipeline.upscale(images, r, txt, **kw)
    assert routed and all(routed)                                  # every span went to the kernels
    monkeypatch.setattr(cf, "correct", lambda content, style, m, ops=None, impl="auto": real(content, style, m, ops=ops, impl="torch"))
    want = pipeline.upscale(images, r, txt, **kw)
    assert got.shape == want.shape and got.dtype == want.dtype and torch.isfinite(got).all()
    d = (got.cpu() - want.cpu()).abs()
    share, worst = float((d > 2e-5).float().mean()), float(d.max())
    print(f"pipeline.upscale '{method}': kernels vs torch route: share off by more than 2e-5: {share:.3e}, max {worst:.3e}")
    assert share < 5e-3 and worst < 5e-3, (share, worst)
