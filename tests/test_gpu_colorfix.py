"""-m gpu: the colour-correction kernels (csrc/svr_colorfix.hip) against colorfix.py, their specification.

  wavelet      bit-equal to the CPU run of colorfix.wavelet_reconstruction (adds and power-of-two scalings only), dense operands and
               the pipeline's two views, every output in a poisoned, guarded canvas
  LAB          svr_lab_planes / svr_lab_merge against an fp64 restatement of the formulas; the bound is MEASURED: twice the largest
               error of the CPU's fp32 rgb_to_lab / lab_to_rgb against the same fp64 values (the factor allows a libm whose pow
               rounds differently but as well)
  AdaIN        2e-5 from the CPU run (the bound tests/test_gpu_parity.py holds the torch route to), statistics 1e-6 relative
  composed     lab and wavelet_adaptive through colorfix.correct against their CPU run with the bounds of
               test_colour_modes_on_the_device_equal_their_cpu_run; pipeline.upscale over toy-width engines against the same call
               with the torch route forced

Figures measured on MI355X are in profiles/colorfix.txt."""
import functools

import pytest
import torch

from conftest import sub
from guarded_out import Pool

pytestmark = pytest.mark.gpu

WAVELET_CASES = [(1, 5, 9), (2, 37, 131), (1, 136, 129), (3, 96, 160), (1, 200, 333)]     # radius cap 1, 4, 16 (exactly), 12, none


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


@functools.lru_cache(maxsize=None)
def _pair(T, H, W, seed=11):
    g = torch.Generator().manual_seed(seed)
    content = (torch.rand(T, 3, H, W, generator=g) * 2 - 1) * 0.9
    style = (torch.rand(T, 3, H, W, generator=g) * 2 - 1) * 0.6 + 0.1
    return content, style


@functools.lru_cache(maxsize=None)
def _cpu(method, T, H, W):
    content, style = _pair(T, H, W)
    return sub("colorfix").METHODS[method](content.clone(), style.clone())


def _pipeline_views(content, style):
    """content as ``final[w0:w1]`` (channels last), style as the pipeline's reference: a [:, :, :H, :W] slice of a larger
    [C, T, H + 3, W + 5] buffer whose padding holds NaN"""
    T, _, H, W = content.shape
    frames = content.permute(0, 2, 3, 1).contiguous().cuda()
    big = torch.full((3, T, H + 3, W + 5), float("nan"), device="cuda")
    big[:, :, :H, :W] = style.permute(1, 0, 2, 3).cuda()
    return frames.permute(0, 3, 1, 2), big.permute(1, 0, 2, 3)[:, :, :H, :W]


def _close_share(got, want):
    d = (got.cpu() - want).abs()
    return float((d > 2e-5).float().mean()), float(d.max())


# ---------------------------------------------------------------------------------------------------------------- wavelet
@pytest.mark.parametrize("layout", ["dense", "pipeline"])
@pytest.mark.parametrize("T,H,W", WAVELET_CASES)
def test_wavelet_equals_the_cpu_run_bit_for_bit(hip, T, H, W, layout):
    content, style = _pair(T, H, W)
    want = _cpu("wavelet", T, H, W)
    pool = Pool()
    if layout == "dense":
        c, s, out = content.cuda(), style.cuda(), pool(T, 3, H, W, dtype=torch.float32)
    else:
        c, s = _pipeline_views(content, style)
        out = pool(T, H, W, 3, dtype=torch.float32).permute(0, 3, 1, 2)
    got = hip.wavelet_reconstruct(c, s, out=out)
    torch.cuda.synchronize()
    pool.check(f"wavelet {T}x{H}x{W} {layout}")
    assert got.data_ptr() == out.data_ptr() and got.shape == want.shape
    bad = got.cpu() != want
    assert not bool(bad.any()), (int(bad.sum()), [int(i) for i in bad.nonzero()[0]], float((got.cpu() - want).abs().max()))
    assert torch.equal(got.cpu(), want)
    fresh = hip.wavelet_reconstruct(c, s)                         # the buffer HipOps allocates itself
    assert torch.equal(fresh.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------- LAB
_RGB2XYZ = [[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]]
_XYZ2RGB = [[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]]
_EPS, _KAPPA = 6.0 / 29.0, (29.0 / 3.0) ** 3


def _rgb_to_lab64(rgb):
    """[N, 3] sRGB in [0, 1], fp64 -> CIELAB (D65), fp64: the formulas of colorfix.rgb_to_lab restated"""
    lin = torch.where(rgb > 0.04045, ((rgb + 0.055) / 1.055) ** 2.4, rgb / 12.92)
    xyz = lin @ torch.tensor(_RGB2XYZ, dtype=torch.float64).T
    xyz = xyz / torch.tensor([0.95047, 1.0, 1.08883], dtype=torch.float64)
    f = torch.where(xyz > _EPS ** 3, xyz.clamp(min=0) ** (1.0 / 3.0), (xyz * _KAPPA + 16.0) / 116.0)
    return torch.stack([f[:, 1] * 116.0 - 16.0, (f[:, 0] - f[:, 1]) * 500.0, (f[:, 1] - f[:, 2]) * 200.0], dim=1)


def _lab_to_rgb64(lab):
    """[N, 3] CIELAB, fp64 -> sRGB clamped to [0, 1], fp64: colorfix.lab_to_rgb restated"""
    fy = (lab[:, 0] + 16.0) / 116.0
    fx, fz = lab[:, 1] / 500.0 + fy, fy - lab[:, 2] / 200.0
    inv = lambda f: torch.where(f > _EPS, f ** 3, (f * 116.0 - 16.0) / _KAPPA)
    xyz = torch.stack([inv(fx) * 0.95047, inv(fy), inv(fz) * 1.08883], dim=1)
    lin = xyz @ torch.tensor(_XYZ2RGB, dtype=torch.float64).T
    rgb = torch.where(lin > 0.0031308, lin.clamp(min=0) ** (1.0 / 2.4) * 1.055 - 0.055, lin * 12.92)
    return rgb.clamp(0.0, 1.0)


@functools.lru_cache(maxsize=None)
def _lab_frames():
    """[-1, 1] frames [2, 3, 40, 77]: random pixels, then the corner values -- 0, 1, beyond both, 0.04045 and the cube-root knee
    (grey 0.0922 has Y = (6/29)^3) each with the fp32 values around them, grey ramps across both knees"""
    T, H, W = 2, 40, 77
    g = torch.Generator().manual_seed(5)
    c01 = torch.rand(T * H * W, 3, generator=g)
    ulps = torch.arange(-4, 5, dtype=torch.float32) * 2.0 ** -27
    knee = float((_EPS ** 3) ** (1 / 2.4) * 1.055 - 0.055)
    special = [torch.tensor([0.0, 1.0, -0.25, 1.5, 0.5, 2.0 ** -20]), 0.04045 + ulps, knee + ulps * 2, torch.linspace(0.040, 0.041, 64),
               torch.linspace(knee - 2e-3, knee + 2e-3, 64), torch.linspace(0, 1, 256)]
    grey = torch.cat(special).float()
    n = grey.numel()
    c01[:n] = grey[:, None]                                       # grey pixels
    c01[n:2 * n, 0] = grey                                        # one channel at the corner value, the others random
    c01[2 * n:3 * n, 2] = grey
    x = (c01 * 2.0 - 1.0).reshape(T, H, W, 3).permute(0, 3, 1, 2).contiguous()
    return x, T, H, W


def test_lab_planes_against_the_fp64_formulas(hip):
    cf = sub("colorfix")
    x, T, H, W = _lab_frames()
    x2 = x.flip(1) * 0.7                                          # a second operand for the style slot
    n = T * H * W
    worst_cpu, worst_dev = 0.0, 0.0
    c_view, s_view = _pipeline_views(x, x2)
    pool = Pool()
    c_lab, s_lab = hip.lab_planes(c_view, s_view, c_lab=pool(3, n, dtype=torch.float32), s_lab=pool(3, n, dtype=torch.float32))
    torch.cuda.synchronize()
    pool.check("lab_planes")
    for name, frames, got in (("base", x, c_lab), ("style", x2, s_lab)):
        c32 = ((frames + 1.0) * 0.5).clamp(0.0, 1.0)
        want = _rgb_to_lab64(c32.permute(0, 2, 3, 1).reshape(-1, 3).double()).T                    # [3, n]
        cpu = cf.rgb_to_lab(c32).permute(1, 0, 2, 3).reshape(3, -1)
        e_cpu, e_dev = (cpu.double() - want).abs().amax(dim=1), (got.cpu().double() - want).abs().amax(dim=1)
        print(f"lab_planes {name}: max |error| vs fp64 per plane (L, a, b): CPU fp32 {[f'{v:.3e}' for v in e_cpu.tolist()]}, "
              f"device {[f'{v:.3e}' for v in e_dev.tolist()]}")
        worst_cpu, worst_dev = max(worst_cpu, float(e_cpu.max())), max(worst_dev, float(e_dev.max()))
    print(f"lab_planes: max |error| vs fp64: CPU fp32 {worst_cpu:.3e}, device {worst_dev:.3e} (bound {2 * worst_cpu:.3e})")
    assert worst_dev <= 2 * worst_cpu, (worst_dev, worst_cpu)


@pytest.mark.parametrize("weight", [0.8, 1.0])
def test_lab_merge_against_the_fp64_formulas(hip, weight):
    cf = sub("colorfix")
    x, T, H, W = _lab_frames()
    n = T * H * W
    g = torch.Generator().manual_seed(6)
    c32 = ((x + 1.0) * 0.5).clamp(0.0, 1.0)
    lab = _rgb_to_lab64(c32.permute(0, 2, 3, 1).reshape(-1, 3).double())                           # in gamut, corners included
    lab[n // 2:] += (torch.rand(n - n // 2, 3, generator=g).double() - 0.5) * torch.tensor([10.0, 40.0, 40.0])   # and beyond it
    c_L, m_a, m_b = (lab[:, k].float().contiguous() for k in range(3))
    m_L = (c_L + (torch.rand(n, generator=g) - 0.5) * 8.0).contiguous()
    if weight < 1.0:
        L64 = c_L.double() * weight + m_L.double() * (1.0 - weight)
        L32 = c_L * weight + m_L * (1.0 - weight)                                                  # as lab_color_transfer states it
    else:
        L64, L32 = c_L.double(), c_L
    want = (_lab_to_rgb64(torch.stack([L64, m_a.double(), m_b.double()], dim=1)) * 2.0 - 1.0).reshape(T, H, W, 3)
    cpu = (cf.lab_to_rgb(torch.stack([L32.reshape(T, H, W), m_a.reshape(T, H, W), m_b.reshape(T, H, W)], dim=1)) * 2.0 - 1.0)
    pool = Pool()
    out = pool(T, H, W, 3, dtype=torch.float32).permute(0, 3, 1, 2)
    poison = torch.full((n,), float("nan"), device="cuda")         # w >= 1: m_L is not read
    got = hip.lab_merge(c_L.cuda(), m_L.cuda() if weight < 1.0 else poison, m_a.cuda(), m_b.cuda(), weight, (T, H, W), out=out)
    torch.cuda.synchronize()
    pool.check(f"lab_merge w={weight}")
    e_cpu = float((cpu.permute(0, 2, 3, 1).double() - want).abs().max())
    e_dev = float((got.cpu().permute(0, 2, 3, 1).double() - want).abs().max())
    print(f"lab_merge w={weight}: max |error| vs fp64: CPU fp32 {e_cpu:.3e}, device {e_dev:.3e} (bound {2 * e_cpu:.3e})")
    assert torch.isfinite(got).all()
    assert e_dev <= 2 * e_cpu, (e_dev, e_cpu)


# ---------------------------------------------------------------------------------------------------------------- AdaIN
def test_adain_and_its_statistics(hip):
    T, H, W = 3, 96, 160
    content, style = _pair(T, H, W)
    c_view, s_view = _pipeline_views(content, style)
    stats = hip.chan_stats(c_view, s_view).cpu().double()
    flat_c, flat_s = content.double().reshape(T, 3, -1), style.double().reshape(T, 3, -1)
    want = torch.stack([flat_c.mean(2), flat_c.var(2), flat_s.mean(2), flat_s.var(2)], dim=2)      # (unbiased: torch's default)
    rel = ((stats - want).abs() / want.abs()).max()
    print(f"chan_stats: max relative error vs fp64 {float(rel):.3e}")
    assert float(rel) < 1e-6
    pool = Pool()
    for c, s, out in ((c_view, s_view, pool(T, H, W, 3, dtype=torch.float32).permute(0, 3, 1, 2)),
                      (content.cuda(), style.cuda(), pool(T, 3, H, W, dtype=torch.float32))):
        got = hip.adain(c, s, out=out)
        torch.cuda.synchronize()
        d = float((got.cpu() - _cpu("adain", T, H, W)).abs().max())
        print(f"adain: max |device - CPU| {d:.3e}")
        assert d < 2e-5, d
    pool.check("adain")


# ---------------------------------------------------------------------------------------------------------------- composed
@pytest.mark.parametrize("method", ["lab", "wavelet_adaptive", "wavelet", "adain"])
def test_correct_on_the_device_equals_the_cpu_run(hip, method):
    """The (3, 3, 96, 160) inputs and the bounds of test_colour_modes_on_the_device_equal_their_cpu_run: the rank-based modes may
    exchange the matched values of pixels tied within fp32 rounding; a share above the cap means a wrong operation order."""
    cf = sub("colorfix")
    content, style = _pair(3, 96, 160)
    want = _cpu(method, 3, 96, 160)
    c, s = content.cuda(), style.cuda()
    assert cf.routes_to_device(c, s, method, hip)
    got = cf.correct(c, s, method, ops=hip)
    assert got.is_cuda and got.shape == want.shape and got.dtype == want.dtype and torch.isfinite(got).all()
    share, worst = _close_share(got, want)
    print(f"correct('{method}') device vs CPU: share off by more than 2e-5: {share:.3e}, max {worst:.3e}")
    if method == "wavelet":
        assert torch.equal(got.cpu(), want)
    elif method == "adain":
        assert worst < 2e-5
    else:
        assert share < 5e-3 and worst < 5e-3, (share, worst)


@pytest.fixture(scope="module")
def toy_runner(hip):
    config, weights, dit, vae, runner = (sub(n) for n in ("config", "weights", "dit", "vae", "runner"))
    dcfg, vcfg = config.DIT_TINY, config.VAEConfig(block_out_channels=(128, 128, 128, 128))
    r = runner.VideoDiffusionInfer(runner.default_config(dcfg, vcfg))
    r.dit = dit.NaDiTEngine(dcfg, weights.synth_dit_state_dict(dcfg, seed=21), hip)
    r.vae = vae.VideoVAEEngine(vcfg, weights.synth_vae_state_dict(vcfg, seed=22), hip)
    return r, weights.synth_text_embedding().cuda()


@pytest.mark.parametrize("method", ["wavelet", "lab"])
def test_pipeline_upscale_against_the_torch_route(toy_runner, monkeypatch, method):
    """pipeline.upscale over toy-width HIP engines: phase 4 on the kernels against the same call with colorfix.correct forced to
    impl="torch" (the code of before): bit-equal for wavelet, within the composed bounds for lab."""
    cf, pipeline = sub("colorfix"), sub("pipeline")
    r, txt = toy_runner
    images = torch.rand(9, 24, 40, 3, generator=torch.Generator().manual_seed(4)).cuda()
    kw = dict(resolution=48, batch_size=5, uniform_batch_size=True, temporal_overlap=2, color_correction=method)
    routed, real = [], cf.correct

    def spy(content, style, m, ops=None, impl="auto"):
        routed.append(cf.routes_to_device(content, style, m, ops))
        return real(content, style, m, ops=ops, impl=impl)

    monkeypatch.setattr(cf, "correct", spy)
    got = pipeline.upscale(images, r, txt, **kw)
    assert routed and all(routed)                                  # every span went to the kernels
    monkeypatch.setattr(cf, "correct", lambda content, style, m, ops=None, impl="auto": real(content, style, m, ops=ops, impl="torch"))
    want = pipeline.upscale(images, r, txt, **kw)
    assert got.shape == want.shape and got.dtype == want.dtype and torch.isfinite(got).all()
    share, worst = _close_share(got, want.cpu())
    print(f"pipeline.upscale '{method}': kernels vs torch route: share off by more than 2e-5: {share:.3e}, max {worst:.3e}")
    if method == "wavelet":
        assert torch.equal(got, want)
    else:
        assert share < 5e-3 and worst < 5e-3, (share, worst)
