"""-m gpu: the alpha kernels (csrc/svr_alpha.hip through HipOps.alpha_upscale) against the fixture recorded from the reference's
code (tests/golden/recorded_alpha.pt; tests/alpha_reference.py says what it pins and what it cannot: the reference's functions
PLUS a numpy stand-in for their two OpenCV calls).  Reads only tests/golden.

Bounds: edge bytes EQUAL (integer arithmetic; a mismatch is a finding, not a tolerance).  Output within 4 E of the fp64 result
outside the fragile mask, E = max |fp32 - fp64| of the same arithmetic on the same input (recorded per fixture case; measured with
alpha.py's restatement where the input is not a fixture's): the kernels are a second realisation of what the fp32 run realises.

Measured on MI355X (max error / bound per case): profiles/alpha_parity.txt, rewritten when SVR_ALPHA_PARITY_OUT names a file."""
import os

import pytest
import torch

import alpha_reference as ar
from conftest import sub
from guarded_out import guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_measured = []


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


@pytest.fixture(scope="module")
def cases():
    return ar.load_cases()


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    path = os.environ.get("SVR_ALPHA_PARITY_OUT")
    if path and _measured:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_alpha.py on MI355X: max |kernel - fp64 reference| outside the fragile mask, per case\n")
            f.write("# case                      matte   rgb    max error   bound (4 E)  edge bytes\n")
            for row in _measured:
                f.write("%-27s %-7s %-6s %.3e   %.3e    %s\n" % row)


def run_kernels(hip, rgb, alpha_lo, base=None):
    """Both outputs in guarded buffers (tests/guarded_out.py).  The alpha is poisoned with NaN and must be written everywhere; the
    guard byte 0xA5 = 165 is a legitimate edge byte, so the edge map is not asked for left-over poison -- the tests compare it with
    the reference's map byte for byte."""
    shape = tuple(rgb.shape[:3])
    g_out, g_edge = guarded(shape, torch.float32), guarded(shape, torch.uint8)
    out = hip.alpha_upscale(rgb.cuda(), alpha_lo.cuda(), out=g_out.t, base=None if base is None else base.cuda(), edge_out=g_edge.t)
    torch.cuda.synchronize()
    assert out is g_out.t
    g_out.assert_guards("alpha_upscale out")
    g_out.assert_written("alpha_upscale out")
    g_edge.assert_guards("alpha_upscale edge_out")
    return out.cpu(), g_edge.t.cpu()


def restatement_pair(rgb, alpha_lo, base=None):
    """(fp64 result, E = max |fp32 - fp64| outside the fragile mask, fragile mask, edge bytes) of alpha.py on this input."""
    alpha = sub("alpha")
    p64 = {}
    r64 = alpha.upscale_alpha_torch(rgb, alpha_lo, base=base, parts=p64, dtype=torch.float64)
    r32 = alpha.upscale_alpha_torch(rgb, alpha_lo, base=base)
    fragile = alpha.fragile_pixels(p64["q"], p64["n"], p64["is_binary"])
    return r64, float((r32.double() - r64).abs()[~fragile].max()), fragile, p64["edge"]


@pytest.mark.parametrize("kind", ar.MATTES)
@pytest.mark.parametrize("name", list(ar.CASES))
def test_kernels_equal_the_reference_fixture(hip, cases, name, kind):
    """Every fixture case on its recorded bicubic base (torch's interpolation is not under test here), fp32 and bf16 RGB.  The bf16
    run is compared with the restatement on the widened input."""
    c, m = cases[name], cases[name][kind]
    out, edge = run_kernels(hip, c["rgb"], m["alpha_lo"], m["base"])
    err = float((out.double() - m["ref64"]).abs()[~m["fragile"]].max())
    same = torch.equal(edge, c["edge"])
    print(f"{name} {kind} fp32: max error {err:.3e}, bound {ar.bound(m):.3e}, edge bytes equal: {same}")
    _measured.append((name, kind, "fp32", err, ar.bound(m), "equal" if same else "DIFFER"))
    assert same, int((edge != c["edge"]).sum())
    assert float(m["fragile"].float().mean()) <= 1e-3
    assert err <= ar.bound(m)
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0

    rgb16 = c["rgb"].to(BF16)
    want, E, fragile, want_edge = restatement_pair(rgb16.float(), m["alpha_lo"], m["base"])
    out, edge = run_kernels(hip, rgb16, m["alpha_lo"], m["base"])
    err = float((out.double() - want).abs()[~fragile].max())
    same = torch.equal(edge, want_edge)
    print(f"{name} {kind} bf16: max error {err:.3e}, bound {4 * E:.3e}, edge bytes equal: {same}")
    _measured.append((name, kind, "bf16", err, 4 * E, "equal" if same else "DIFFER"))
    assert same, int((edge != want_edge).sum())
    assert float(fragile.float().mean()) <= 1e-2
    assert err <= 4 * E


@pytest.mark.parametrize("kind", ar.MATTES)
def test_full_op_with_its_own_bicubic_base_and_run_to_run_bits(hip, cases, kind):
    """HipOps.alpha_upscale including the bicubic base (torch on the device) on the ragged multi-tile case: same bound, and the
    same bits on a second run (integer atomics only)."""
    c, m = cases["ragged_70x118"], cases["ragged_70x118"][kind]
    out, edge = run_kernels(hip, c["rgb"], m["alpha_lo"])
    again, edge_again = run_kernels(hip, c["rgb"], m["alpha_lo"])
    err = float((out.double() - m["ref64"]).abs()[~m["fragile"]].max())
    print(f"ragged_70x118 {kind} full op: max error {err:.3e}, bound {ar.bound(m):.3e}")
    _measured.append(("ragged_70x118 (full op)", kind, "fp32", err, ar.bound(m), "equal" if torch.equal(edge, c["edge"]) else "DIFFER"))
    assert torch.equal(edge, c["edge"])
    assert err <= ar.bound(m)
    assert torch.equal(out, again) and torch.equal(edge, edge_again)


def test_frame_maxima_do_not_leak_across_frames(hip, cases):
    """The frame with the largest edge maximum placed LAST: replacing it leaves the earlier frames' edge maps and alpha unchanged
    (as long as the batch statistics stay what they were: the replacement keeps the sign of min(rgb) and the matte)."""
    c = cases["tile_edge_33x37"]
    a = c["binary"]["alpha_lo"]
    rgb = c["rgb"][[1, 2, 0]].contiguous()                                 # contrast 0.12, 0.5, 1.0: Sobel maxima 404, 5650, 23130
    a = a[[1, 2, 0]].contiguous()
    out, edge = run_kernels(hip, rgb, a)
    assert torch.equal(edge, c["edge"][[1, 2, 0]])
    other = rgb.clone()
    other[2] = (other[2] * 0.3).roll(5, dims=1)
    out2, edge2 = run_kernels(hip, other, a)
    assert torch.equal(edge2[:2], edge[:2]) and torch.equal(out2[:2], out[:2])
    assert not torch.equal(edge2[2], edge[2])
    assert int(edge2[2].max()) == 255 and int(edge[0].max()) == 255


def test_constant_frame(hip):
    """max n == 0 (the reference divides 0 by 0): edge map 0, alpha finite and in [0, 1]; a constant frame next to a textured
    one keeps its zero edge map."""
    rgb = torch.full((2, 35, 41, 3), -0.5)
    rgb[1] = ar.scene("tile_edge_33x37")[0][0, :, :, :].mean() + torch.linspace(-0.4, 0.4, 41)[None, :, None]
    for a in (torch.ones(2, 9, 11), torch.linspace(0, 1, 2 * 9 * 11).reshape(2, 9, 11)):
        out, edge = run_kernels(hip, rgb, a)
        assert int(edge[0].max()) == 0 and int(edge[1].max()) == 255
        assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0


def test_pipeline_rgba_over_the_kernels(hip):
    """pipeline.upscale over HipOps, tiny configs, a 4-channel clip: RGB bit-equal to the RGB-only call, alpha within the bound of
    the restatement applied to the same frames (the spans' decoded frames before colour correction)."""
    from test_alpha import _tiny_runner, rgba_clip
    pipeline, alpha, weights = sub("pipeline"), sub("alpha"), sub("weights")
    r = _tiny_runner(hip, vae_channels=(128, 128, 128, 128))          # (the reduced VAE of tests/golden/pipeline_small.pt)
    clip = rgba_clip(frames=6, h=24, w=40).cuda()                      # (the frame size of the pipeline goldens)
    text = weights.synth_text_embedding().cuda()
    kw = dict(resolution=48, batch_size=5, temporal_overlap=1, color_correction="lab")
    calls = []
    real = alpha.upscale_alpha
    alpha.upscale_alpha = lambda rgb, a, ops=None: calls.append((rgb.clone(), a.clone())) or real(rgb, a, ops)
    try:
        out = pipeline.upscale(clip, r, text, **kw)
    finally:
        alpha.upscale_alpha = real
    rgb_only = pipeline.upscale(clip[..., :3].contiguous(), r, text, **kw)
    assert out.shape == rgb_only.shape[:3] + (4,) and torch.equal(out[..., :3], rgb_only)
    assert len(calls) == 2 and sum(c[0].shape[0] for c in calls) == 6
    pos = 0
    for rgb, a in calls:
        assert rgb.dtype == torch.float32 and rgb.shape[-1] == 3
        want, E, fragile, _ = restatement_pair(rgb.cpu(), a.cpu())
        got = out[pos:pos + rgb.shape[0], ..., 3].double().cpu()
        err = float((got - want).abs()[~fragile].max())
        print(f"pipeline span at frame {pos}: max error {err:.3e}, bound {4 * E:.3e}, fragile {float(fragile.float().mean()):.2%}")
        assert float(fragile.float().mean()) <= 1e-2
        assert err <= 4 * E
        pos += rgb.shape[0]
    assert float(out[..., 3].min()) >= 0 and float(out[..., 3].max()) <= 1 and float(out[..., 3].std()) > 0.1
