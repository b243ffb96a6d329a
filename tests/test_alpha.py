"""-m "not gpu": edge-guided alpha upscaling -- alpha.py's torch restatement against the fixture recorded from the reference's code
(tests/alpha_reference.py: the reference's four functions PLUS a numpy stand-in for the two OpenCV calls they make, which is the
fixture's limitation), the border semantics of the guided filter, RGBA through pipeline.upscale, the C ABI's refusals, the CLI."""
import ctypes
import os
import shutil

import pytest
import torch

import alpha_reference as ar
from conftest import ROOT, sub
from ops_reference import TorchOps

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def cases():
    return ar.load_cases()


@pytest.mark.parametrize("kind", ar.MATTES)
@pytest.mark.parametrize("name", list(ar.CASES))
def test_restatement_equals_the_reference(cases, name, kind):
    """Edge bytes EQUAL; output within 4 E of the reference in fp64 outside the fragile mask (E = max |ref32 - ref64| of the case:
    the restatement is a second fp32 realisation of the same arithmetic).  Runs the reference live where its source is present."""
    alpha = sub("alpha")
    c, m = cases[name], cases[name][kind]
    parts = {}
    out = alpha.upscale_alpha_torch(c["rgb"], m["alpha_lo"], parts=parts)
    assert out.dtype == torch.float32 and out.shape == m["ref32"].shape
    assert parts["is_binary"] == (kind == "binary")
    assert parts["neg0"] == (name != "unit_range_20x24") and parts["neg1"] == (name == "overshoot_20x24")
    assert torch.equal(parts["edge"], c["edge"])
    assert torch.equal(parts["base"], m["base"])
    assert float(m["fragile"].float().mean()) <= 1e-3
    err = (out.double() - m["ref64"]).abs()[~m["fragile"]]
    print(f"{name} {kind}: E {m['E']:.2e}, max error {float(err.max()):.2e}")
    assert float(err.max()) <= ar.bound(m)
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


def test_double_normalisation_changes_the_edge_map(cases):
    """With pixels below -1 the edge detector's image is normalised twice (the reference tests min < 0 again on the normalised
    frames): the recorded edge bytes are those of the twice-normalised image, not of the once-normalised one."""
    alpha = sub("alpha")
    c = cases["overshoot_20x24"]
    once = alpha.edge_bytes(alpha.sobel_energy(c["rgb"], True, False))
    twice = alpha.edge_bytes(alpha.sobel_energy(c["rgb"], True, True))
    assert torch.equal(twice, c["edge"]) and not torch.equal(once, c["edge"])


def test_constant_frame_has_no_edges_and_a_finite_alpha():
    alpha = sub("alpha")
    rgb = torch.full((1, 6, 9, 3), 0.25)
    for a in (torch.ones(1, 3, 4), torch.linspace(0, 1, 12).reshape(1, 3, 4)):
        parts = {}
        out = alpha.upscale_alpha_torch(rgb, a, parts=parts)
        assert int(parts["edge"].max()) == 0 and bool(torch.isfinite(out).all())
        assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


def test_guided_filter_border_semantics():
    """avg_pool2d pads with zeros and divides by (2r + 1)^2 everywhere, and the second pooling sees a and b as zero outside the
    image.  So a uniform alpha of 1 comes out BELOW 1 at the border (a corner's window holds 9 of 25 taps, twice over), and is 1
    only where the window fits: where every (a, b) under the pixel's window came from a full window, i.e. 2r from the border -- on
    the 5 x 7 case nowhere, on a 13 x 15 frame with r = 2 exactly in rows 4..8, columns 4..10."""
    alpha = sub("alpha")
    guide = (ar.scene("tiny_5x7")[0].mean(dim=-1) + 1) / 2
    ring = torch.ones(5, 7, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    for r in (2, 3):
        q = alpha.guided_filter(guide, torch.ones(1, 5, 7), r)[0]
        assert bool((q[ring] < 1 - 1e-2).all()), q
        assert bool(((q - 1).abs() > 1e-3).all()), q
        assert float(q[0, 0]) < 0.5 and float(q[-1, -1]) < 0.5
    y, x = torch.meshgrid(torch.arange(13.0), torch.arange(15.0), indexing="ij")
    guide = (0.5 + 0.3 * torch.sin(0.4 * x) * torch.cos(0.3 * y))[None]
    q = alpha.guided_filter(guide, torch.ones(1, 13, 15), 2)[0]
    fits = torch.zeros(13, 15, dtype=torch.bool)
    fits[4:9, 4:11] = True
    assert bool(((q[fits] - 1).abs() < 1e-5).all()), q
    assert bool(((q[~fits] - 1).abs() > 1e-5).all()), q
    ring = torch.ones(13, 15, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert bool((q[ring] < 1 - 1e-2).all()), q


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _tiny_runner(ops, vae_channels=None):
    """``vae_channels``: the device kernels serve GroupNorm widths of 128 and up (svr_groupnorm_stats), so the GPU test takes the
    reduced VAE of the pipeline goldens, (128, 128, 128, 128), instead of VAE_TINY's 64-channel stages."""
    config, weights, dit, vae, runner = (sub(n) for n in ("config", "weights", "dit", "vae", "runner"))
    dcfg = config.DIT_TINY
    vcfg = config.VAE_TINY if vae_channels is None else config.VAEConfig(block_out_channels=tuple(vae_channels))
    r = runner.VideoDiffusionInfer(runner.default_config(dcfg, vcfg))
    r.dit = dit.NaDiTEngine(dcfg, weights.synth_dit_state_dict(dcfg), ops)
    r.vae = vae.VideoVAEEngine(vcfg, weights.synth_vae_state_dict(vcfg), ops)
    return r


def rgba_clip(frames=7, h=16, w=20, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(frames, h, w, 3, generator=g)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    a = torch.stack([(((y - h / 2) ** 2 + (x - w / 2 - t) ** 2).sqrt() < h / 3).float() for t in range(frames)])
    return torch.cat([rgb, a.unsqueeze(-1)], dim=-1)


def test_pipeline_rgba_on_the_torch_double():
    """[T, H, W, 4] in -> [T, H', W', 4] out: RGB bit-equal to the three-channel call, alpha = upscale_alpha of each span's frames
    BEFORE colour correction and the input alpha of the same clip frames (prepend_frames pads alpha like RGB); with batch_filter
    and return_spans, owned spans equal the single-rank result and everything else is zero."""
    pipeline, alpha, weights = sub("pipeline"), sub("alpha"), sub("weights")
    r = _tiny_runner(TorchOps("cpu", act_dtype=torch.float32))
    clip = rgba_clip()
    text = weights.synth_text_embedding().float()
    kw = dict(resolution=32, batch_size=5, temporal_overlap=1, prepend_frames=1, color_correction="wavelet")
    calls = []
    real = alpha.upscale_alpha
    alpha.upscale_alpha = lambda rgb, a, ops=None: calls.append((rgb.clone(), a.clone())) or real(rgb, a, ops)
    try:
        out = pipeline.upscale(clip, r, text, **kw)
    finally:
        alpha.upscale_alpha = real
    rgb_only = pipeline.upscale(clip[..., :3].contiguous(), r, text, **kw)
    assert out.shape == rgb_only.shape[:3] + (4,) and out.dtype == rgb_only.dtype
    assert torch.equal(out[..., :3], rgb_only)
    # the frames the alpha saw are the decoded, blended, not yet colour-corrected ones: clamped and mapped to [0, 1] they are the
    # output of the same run without colour correction
    plain = pipeline.upscale(clip[..., :3].contiguous(), r, text, **{**kw, "color_correction": "none"})
    padded_alpha = sub("transforms").pad_video_temporal(clip, count=1, temporal_dim=0, prepend=True)[..., 3]   # alpha padded like RGB
    assert torch.equal(padded_alpha[0], clip[1, ..., 3])
    seen, want, pos = [], [], 0
    assert len(calls) == 2                                                           # 8 frames, batches of 5 with overlap 1
    for rgb, a in calls:
        assert rgb.shape[-1] == 3 and a.shape[0] == rgb.shape[0]
        assert torch.equal(a, padded_alpha[pos:pos + a.shape[0]])
        seen.append(rgb)
        want.append(alpha.upscale_alpha_torch(rgb, a))
        pos += a.shape[0]
    assert torch.equal(torch.cat(seen)[1:].clamp(-1, 1).mul(0.5).add(0.5), plain)
    assert torch.equal(out[..., 3], torch.cat(want)[1:])
    assert float(out[..., 3].min()) >= 0 and float(out[..., 3].max()) <= 1 and float(out[..., 3].std()) > 0.1
    # data parallelism over batches (no overlap: a blend across ranks needs dist.py's head exchange): each rank's owned spans equal
    # the single-rank frames in all four channels, everything else stays zero
    kw0 = {**kw, "temporal_overlap": 0}
    single = pipeline.upscale(clip, r, text, **kw0)
    for rank in (0, 1):
        part, spans = pipeline.upscale(clip, r, text, batch_filter=lambda i, rank=rank: i % 2 == rank, return_spans=True, **kw0)
        assert part.shape == single.shape and list(spans) == [rank]
        owned = torch.zeros(single.shape[0], dtype=torch.bool)
        for a0, a1 in spans.values():
            owned[a0:a1] = True
        assert bool(owned.any()) and float(part[~owned].abs().max()) == 0.0
        assert torch.equal(part[owned], single[owned])
    with pytest.raises(ValueError):
        pipeline.upscale(torch.rand(2, 16, 16, 5), r, text, **kw)


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_alpha_entry_points_refuse_invalid_arguments_before_any_launch():
    """In the pattern of test_cabi.py::test_entry_points_refuse_invalid_arguments_before_any_launch: null pointers, H < 2, W < 2,
    T < 1, an unknown dtype code and a short workspace are refused on the host (non-zero, a message naming the entry point)."""
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = L.svr_alpha_workspace_bytes(1, 4, 4)
    assert need == (4 + 4 + 16) * 4 and L.svr_alpha_workspace_bytes(3, 33, 37) == (4 + 4 + 3 * 33 * 37) * 4
    assert L.svr_alpha_workspace_bytes(0, 4, 4) == 0 and L.svr_alpha_workspace_bytes(1, 1, 4) == 0
    stats = lambda alpha=p, n=12, rgb=p, T=1, H=4, W=4, ld=3, kind=1, ws=p, nbytes=need: \
        L.svr_alpha_stats(alpha, n, rgb, T, H, W, ld, kind, ws, nbytes, None)
    edges = lambda rgb=p, T=1, H=4, W=4, ld=3, kind=1, ws=p, nbytes=need: L.svr_alpha_edges(rgb, T, H, W, ld, kind, ws, nbytes, None)
    refine = lambda rgb=p, base=p, out=p, edge=None, T=1, H=4, W=4, ld=3, kind=1, n=12, ws=p, nbytes=need: \
        L.svr_alpha_refine(rgb, base, out, edge, T, H, W, ld, kind, n, ws, nbytes, None)
    cases = []
    for name, fn in (("svr_alpha_stats", stats), ("svr_alpha_edges", edges), ("svr_alpha_refine", refine)):
        cases += [(name, lambda fn=fn: fn(rgb=None)), (name, lambda fn=fn: fn(ws=None)), (name, lambda fn=fn: fn(H=1)),
                  (name, lambda fn=fn: fn(W=1)), (name, lambda fn=fn: fn(T=0)), (name, lambda fn=fn: fn(kind=2)),
                  (name, lambda fn=fn: fn(kind=7)), (name, lambda fn=fn: fn(nbytes=need - 4)), (name, lambda fn=fn: fn(ld=2))]
    cases += [("svr_alpha_stats", lambda: stats(alpha=None)), ("svr_alpha_stats", lambda: stats(n=0)),
              ("svr_alpha_refine", lambda: refine(base=None)), ("svr_alpha_refine", lambda: refine(out=None)),
              ("svr_alpha_refine", lambda: refine(n=0))]
    for name, call in cases:
        assert call() != 0, name
        assert name.encode() in L.svr_last_error(), (name, L.svr_last_error())


def test_header_and_ctypes_table_agree_on_the_alpha_entry_points():
    import re
    hip_lib = sub("hip_lib")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = sorted(set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M)))
    assert sorted(hip_lib.SYMBOLS) == declared
    assert {"svr_alpha_workspace_bytes", "svr_alpha_stats", "svr_alpha_edges", "svr_alpha_refine"} <= set(declared)
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9


def test_upscale_alpha_uses_the_backend_and_never_falls_back():
    """ops.alpha_upscale where the backend has it -- and its failure propagates; the restatement only for a backend without."""
    alpha, hip_lib = sub("alpha"), sub("hip_lib")
    rgb, mattes = ar.scene("tiny_5x7")

    class Failing:
        def alpha_upscale(self, rgb, a):
            raise hip_lib.HipLibraryError("svr_alpha_stats failed")

    with pytest.raises(hip_lib.HipLibraryError):
        alpha.upscale_alpha(rgb, mattes["soft"], Failing())
    assert torch.equal(alpha.upscale_alpha(rgb, mattes["soft"], TorchOps("cpu")), alpha.upscale_alpha_torch(rgb, mattes["soft"]))


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_keeps_the_alpha_channel(tmp_path, capsys):
    import importlib.util
    import numpy as np
    from PIL import Image
    spec = importlib.util.spec_from_file_location("svr_cli_alpha", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rgba = (rgba_clip(frames=1, h=9, w=11)[0] * 255).round().to(torch.uint8).numpy()
    Image.fromarray(rgba, "RGBA").save(tmp_path / "cutout.png")
    Image.fromarray(rgba[..., :3], "RGB").save(tmp_path / "opaque.png")
    frames, _ = cli.load_frames(str(tmp_path / "cutout.png"))
    assert frames.shape == (1, 9, 11, 4) and frames.dtype == torch.float32
    assert np.array_equal((frames[0] * 255).round().to(torch.uint8).numpy(), rgba)
    assert cli.load_frames(str(tmp_path / "opaque.png"))[0].shape == (1, 9, 11, 3)
    cli.save_frames(frames, str(tmp_path / "out.png"), "png")
    back = Image.open(tmp_path / "out.png")
    assert back.mode == "RGBA" and np.array_equal(np.asarray(back), rgba)
    cli.save_frames(torch.cat([frames, frames]), str(tmp_path / "dir"), "png")
    assert Image.open(tmp_path / "dir" / "frame_000001.png").mode == "RGBA"
    # four-channel tensors keep their alpha too; three-channel ones are untouched
    torch.save(frames, tmp_path / "clip.pt")
    np.save(tmp_path / "clip.npy", frames.numpy())
    assert torch.equal(cli.load_frames(str(tmp_path / "clip.pt"))[0], frames)
    assert torch.equal(cli.load_frames(str(tmp_path / "clip.npy"))[0], frames)
    torch.save(frames[..., :3].contiguous(), tmp_path / "rgb.pt")
    assert cli.load_frames(str(tmp_path / "rgb.pt"))[0].shape[-1] == 3


def test_node_still_refuses_rgba_and_says_where_it_works():
    itf = sub("interfaces")
    with pytest.raises(NotImplementedError, match="pipeline.upscale"):
        itf.SeedVR2VideoUpscaler.execute(torch.zeros(1, 8, 8, 4), {}, {}, 42)
