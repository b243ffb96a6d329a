"""-m gpu: every launch of small ENGINE runs against the per-element bounds of tests/local_error.py (tests/launch_audit.py).

One engine forward per scenario over ``audited(HipOps)``, ``assert_clean()`` at the end.  The scenarios are the smallest at which the
engines still issue every form; the channel widths are production's (spatial sizes are what makes them cheap -- narrower widths would
move the launches onto other kernel instances).  The coverage tests at the end assert the forms and kernel classes on the records, so
the audit cannot pass by auditing nothing: a missing form is a failure.  They take the records of the scenario tests where those ran
in this process and run the scenarios themselves where not.

With SVR_LOCAL_ERROR_LOG=<file> every scenario appends its worst err / bound per (op, kernel class) there
(profiles/launch_audit_headroom.txt is made from such a log -- a record, never an input to a tolerance)."""
import time

import pytest
import torch

import launch_audit as la
from conftest import sub

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

_state = {}


def _once(key, make):
    if key not in _state:
        _state[key] = make()
    return _state[key]


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ scenarios
def _dit_cfg(name):
    config = sub("config")
    return {"3b_tiny": config.DIT_TINY, "7b_tiny": config.DIT_7B_TINY,
            # the block mix of tests/test_gpu_fullscale.py (i) -- MM, shared with shifted windows, final video-only -- at full width
            "3b_wide": config.DiTConfig(num_layers=3, mm_layers=1),
            "7b_wide": config.DiTConfig(vid_dim=3072, heads=24, num_layers=2, mm_layers=2, mlp_type="normal", rope_type="rope3d",
                                        out_norm=False, last_vid_only=False)}[name]


def _run_dit(name, store):
    weights, dit = sub("weights"), sub("dit")
    cfg = _dit_cfg(name)
    sd = _once(("dit_sd", name), lambda: weights.synth_dit_state_dict(cfg, seed=5))
    ops = la.audited(sub("ops").HipOps)("cuda:0")
    eng = dit.NaDiTEngine(cfg, sd, ops, hid_store=store)
    vid = _randn(3, 16, 24, 33, seed=1).to(BF16).cuda()                 # 288 video tokens
    txt = weights.synth_text_embedding().cuda()                         # 58 text rows
    out = eng.forward(vid, txt, 1000.0, x_t=vid[..., :16].contiguous())
    assert bool(torch.isfinite(out.float()).all()) and eng.overflow_reruns == 0
    return ops


def _vae_engine(regime):
    config, weights, vae = sub("config"), sub("weights"), sub("vae")
    sd = _once("vae_sd", lambda: weights.synth_vae_state_dict(config.VAE_V3, seed=7))
    ops = la.audited(sub("ops").HipOps)("cuda:0")
    return ops, vae.VideoVAEEngine(config.VAE_V3, sd, ops, **dict(regime))


TILED = dict(tiled=True, tile_size=(32, 32), tile_overlap=(16, 16))
VAE_RUNS = {
    # slices of 5 + 4 frames, one-frame slices at the deepest level, strided convs with and without a carried halo, frames of 16x24,
    # 8x12 and 4x6 voxels below one patch
    "encode_sliced": lambda eng: eng.encode(_randn(3, 9, 32, 48, seed=4).clamp(-1, 1).cuda(), frames_per_slice=4),
    # the causal-head pair, quad sub-pixel launches with shared statistics, carried halos, 24 tokens per frame: fused attention
    "decode_sliced": lambda eng: eng.decode(_randn(3, 4, 6, 16, seed=3).to(BF16).cuda(), latents_per_slice=1),
    # 64 tokens per frame: mid-block attention as GEMM -> softmax_rows -> GEMM
    "decode_unsliced": lambda eng: eng.decode(_randn(2, 8, 8, 16, seed=5).to(BF16).cuda()),
    "encode_tiled": lambda eng: eng.encode(_randn(3, 5, 48, 64, seed=6).clamp(-1, 1).cuda(), **TILED),
    "decode_tiled": lambda eng: eng.decode(_randn(2, 6, 8, 16, seed=8).to(BF16).cuda(), keep_frames=3, **TILED),
}
DEFAULT, FP32_BF16 = (), (("trunk_store", "fp32"), ("branch_store", "bf16"))
VAE_SCENARIOS = [("encode_sliced", DEFAULT), ("decode_sliced", DEFAULT), ("encode_sliced", FP32_BF16), ("decode_sliced", FP32_BF16),
                 ("decode_unsliced", DEFAULT), ("encode_tiled", DEFAULT), ("decode_tiled", DEFAULT)]
DIT_SCENARIOS = [(n, s) for n in ("3b_tiny", "7b_tiny") for s in ("h16", "fp32", "bf16")] + [("3b_wide", "h16"), ("7b_wide", "h16")]


def _run_vae(run, regime):
    ops, eng = _vae_engine(regime)
    out = VAE_RUNS[run](eng)
    assert bool(torch.isfinite(out.float()).all()) and eng.overflow_reruns == 0
    return ops


def scenario(kind, a, b):
    """The audited ops of one scenario, run once per process."""
    def make():
        t0 = time.perf_counter()
        ops = _run_dit(a, b) if kind == "dit" else _run_vae(a, b)
        torch.cuda.synchronize()
        name = f"{kind} {a} {b if kind == 'dit' else '/'.join(v for _, v in b) or 'default'}"
        print(f"[launch_audit] {name}: {len(ops.records)} launches audited in {time.perf_counter() - t0:.1f} s")
        ops.log_headroom(name)
        return ops
    return _once((kind, a, b), make)


# ------------------------------------------------------------------------------------------------ every launch inside its bounds
@pytest.mark.parametrize("cfg,store", DIT_SCENARIOS, ids=[f"{n}-{s}" for n, s in DIT_SCENARIOS])
def test_dit_forward_launches_are_inside_their_bounds(cfg, store):
    ops = scenario("dit", cfg, store)
    ops.assert_clean()
    assert {r.op for r in ops.records} == {"patchify", "gemm", "ada_combine", "rmsnorm_mod", "qknorm_rope", "attn_varlen", "rows_mean",
                                           "unpatchify_euler"}
    missing = [k for k, v in la.dit_forms(ops.records).items() if not v
               and k not in ("SwiGLU GEMM", "tanh-GELU GEMM", "GEMM with resid is out and h16 output")]
    assert not missing, missing
    assert not any(r.kernel_class == "invalid" for r in ops.records)


@pytest.mark.parametrize("run,regime", VAE_SCENARIOS, ids=[f"{r}-{'_'.join(v for _, v in g) or 'default'}" for r, g in VAE_SCENARIOS])
def test_vae_launches_are_inside_their_bounds(run, regime):
    ops = scenario("vae", run, regime)
    ops.assert_clean()
    assert {"gemm", "groupnorm_stats", "groupnorm_apply"} <= {r.op for r in ops.records}
    assert not any(r.kernel_class == "invalid" for r in ops.records)


# ------------------------------------------------------------------------------------------------ coverage: nothing audited, nothing proven
def test_dit_scenarios_cover_the_engine_forms():
    records = [r for n, s in DIT_SCENARIOS for r in scenario("dit", n, s).records]
    missing = [k for k, v in la.dit_forms(records).items() if not v]
    assert not missing, f"forms no DiT scenario issued: {missing}"
    assert not any(r.kernel_class == "invalid" for r in records)


def test_vae_scenarios_cover_the_engine_forms_and_kernel_classes():
    records = [r for run, g in VAE_SCENARIOS for r in scenario("vae", run, g).records]
    gemms = [r for r in records if r.op == "gemm"]
    classes = {r.kernel_class for r in gemms}
    assert "invalid" not in classes
    assert {"conv_halo", "conv_thin_in", "conv_generic", "conv_thinout", "conv_subpixel", "gemm"} <= classes, classes
    missing = [k for k, v in la.vae_forms(records).items() if not v]
    assert not missing, f"forms no VAE scenario issued: {missing}"
    assert any(r.op == "attn_varlen" and r.flags["head_dim"] == 512 for r in records)        # the fused head_dim-512 kernel
    for cls in la.FUSING_CLASSES:                      # one launch that DELIVERED fused statistics per class that can fuse them
        assert any(r.kernel_class == cls and r.flags["stats_asked"] and r.flags["stats_delivered"] for r in gemms), cls
    assert any(r.op == "gn_shared_stats" and r.flags["stats_delivered"] for r in records)
    assert any(r.flags["quad"] and r.kernel_class == "conv_subpixel" for r in gemms)
