"""-m "not gpu": the launch audit of tests/launch_audit.py, proven on the CPU double of the C ABI.

  * Clean run: over ``TorchOps("cpu", act_dtype=bf16)`` every launch of DIT_TINY, DIT_7B_TINY (h16 and bf16 stream) and of a
    (128, 128, 256, 256) VAE (sliced encode / decode, un-sliced decode, tiled encode / decode) is inside its bound -- the references
    take the engines' own launches (row-offset views, in-place residuals, phase scatter, carried halos) without an exception and
    with no false alarm, so the same audit over HipOps (tests/test_gpu_launch_audit.py) judges the kernels, not itself.
  * Fault injection: an ops double corrupts exactly ONE launch of an engine run -- one 16-byte chunk of one output row of a
    mid-network conv / GEMM, the fused statistics of two frames exchanged, one window's attention rows written one row off.  The
    audit names that launch, and only that launch, by sequence number and op; the engine-level metric the engine tests assert
    (2e-2 for the VAE, 8e-3 for the DiT, against the un-faulted run) sees neither the chunk faults nor the exchanged statistics
    (2.0e-3 and 3.2e-3 on the VAE, 2.4e-3 on the DiT; the shifted window, 1.7e-2, it would see).  That is the gap, as a test.
  * Coverage of forms: the flags recorded on the CPU runs show every form the engines are known to issue (kernel classes are a GPU
    matter), so an engine change that stops issuing one is noticed where there is no GPU."""
import pytest
import torch

import launch_audit as la
from conftest import sub, rel_err
from ops_reference import TorchOps

BF16 = torch.bfloat16
VAE_TOL, DIT_TOL = 2e-2, 8e-3          # tests/test_gpu_wide_trunk.py: the engines against their CPU emulation
VAE_WIDTHS = (128, 128, 256, 256)
TILED = dict(tiled=True, tile_size=(32, 32), tile_overlap=(16, 16))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the scenarios
@pytest.fixture(scope="module")
def vae_sd():
    config, weights = sub("config"), sub("weights")
    cfg = config.VAEConfig(block_out_channels=VAE_WIDTHS)
    return cfg, weights.synth_vae_state_dict(cfg, seed=7)


def run_dit(ops, cfg, store):
    weights, dit = sub("weights"), sub("dit")
    vid = _randn(3, 16, 24, 33, seed=1).to(BF16)
    eng = dit.NaDiTEngine(cfg, weights.synth_dit_state_dict(cfg, seed=5), ops, hid_store=store)
    return eng.forward(vid, weights.synth_text_embedding(), 1000.0, x_t=vid[..., :16].contiguous()).float()


def vae_decode_sliced(eng):
    return eng.decode(_randn(3, 4, 6, 16, seed=3).to(BF16), latents_per_slice=1).float()


def vae_encode_sliced(eng):
    return eng.encode(_randn(3, 9, 32, 48, seed=4).clamp(-1, 1), frames_per_slice=4).float()


def vae_decode_small(eng):
    """three one-latent slices of 4 x 4 latents: the clip's head, the two head patterns of the second latent, the steady state"""
    return eng.decode(_randn(3, 4, 4, 16, seed=9).to(BF16), latents_per_slice=1).float()


def run_vae_all(ops, cfg, sd):
    eng = sub("vae").VideoVAEEngine(cfg, sd, ops)
    vae_encode_sliced(eng)
    vae_decode_sliced(eng)
    eng.decode(_randn(1, 8, 8, 16, seed=5).to(BF16))                                   # 64 tokens per frame: attention as GEMMs
    eng.encode(_randn(3, 1, 40, 48, seed=6).clamp(-1, 1), **TILED)                      # 2 x 2 overlapping tiles
    eng.decode(_randn(2, 5, 6, 16, seed=8).to(BF16), keep_frames=3, **TILED)            # 2 x 2 tiles, the last slice trimmed


# ------------------------------------------------------------------------------------------------ clean runs, coverage of forms
@pytest.fixture(scope="module")
def dit_clean():
    config = sub("config")
    runs = {}
    for name, cfg in (("3b", config.DIT_TINY), ("7b", config.DIT_7B_TINY)):
        for store in ("h16", "bf16"):
            ops = la.audited(TorchOps)("cpu", act_dtype=BF16)
            runs[name, store] = (ops, run_dit(ops, cfg, store))
    return runs


@pytest.fixture(scope="module")
def vae_clean(vae_sd):
    ops = la.audited(TorchOps)("cpu", act_dtype=BF16)
    run_vae_all(ops, *vae_sd)
    return ops


@pytest.fixture(scope="module")
def vae_fusing_clean(vae_sd):
    """a sliced decode over the double that fuses statistics and takes quad launches, as HipOps does"""
    ops = la.audited(la.FusingTorchOps)("cpu", act_dtype=BF16)
    return ops, vae_decode_small(sub("vae").VideoVAEEngine(*vae_sd, ops))


def test_audited_class_is_constructed_like_its_base_and_records_kernel_class_none():
    cls = la.audited(TorchOps)
    assert issubclass(cls, TorchOps) and cls is la.audited(TorchOps)
    ops = cls("cpu", act_dtype=BF16)
    assert ops.act_dtype == BF16 and ops.records == [] and not hasattr(ops, "gn_shared_stats")     # (the engine's probe for shared statistics)
    assert hasattr(la.audited(la.FusingTorchOps)("cpu"), "gn_shared_stats")
    A, W = _randn(5, 64, seed=1).to(BF16), _randn(128, 64, seed=2).to(BF16)
    ops.gemm(A, W, ops.empty(5, 128), N=128, K=64)
    assert [(r.seq, r.op, r.kernel_class) for r in ops.records] == [(0, "gemm", None)] and ops.assert_clean() == 1


def test_dit_launches_are_inside_their_bounds_on_the_cpu_double(dit_clean):
    for (name, store), (ops, out) in dit_clean.items():
        assert ops.assert_clean() == len(ops.records) > 0 and bool(torch.isfinite(out).all())
        assert all(r.kernel_class is None and 0.0 <= r.worst <= 1.0 for r in ops.records)


def test_vae_launches_are_inside_their_bounds_on_the_cpu_double(vae_clean, vae_fusing_clean):
    assert vae_clean.assert_clean() > 600
    assert vae_fusing_clean[0].assert_clean() > 150


def test_dit_runs_issue_the_engine_forms(dit_clean):
    records = [r for ops, _ in dit_clean.values() for r in ops.records]
    missing = [k for k, v in la.dit_forms(records).items() if not v]
    assert not missing, missing
    for (name, store), (ops, _) in dit_clean.items():
        forms = la.dit_forms(ops.records)
        assert forms["GEMM with resid is out and h16 output"] == (store == "h16")
        assert forms["SwiGLU GEMM"] == (name == "3b") and forms["tanh-GELU GEMM"] == (name == "7b")


def test_vae_runs_issue_the_engine_forms(vae_clean, vae_fusing_clean):
    forms = la.vae_forms(vae_clean.records)
    # the plain double has no fragment-ordered weights and fuses nothing: its phase launches are single and share no buffer
    missing = [k for k, v in forms.items() if not v and k not in ("quad phase launch", "phase launches sharing one statistics buffer")]
    assert not missing, missing
    assert not any(r.flags.get("stats_delivered") for r in vae_clean.records)                    # (None is recorded, not failed)
    fused = la.vae_forms(vae_fusing_clean[0].records)
    assert fused["quad phase launch"] and fused["phase launches sharing one statistics buffer"]
    recs = vae_fusing_clean[0].records
    assert any(r.op == "gn_shared_stats" and r.flags["stats_delivered"] and len(r.flags["launches"]) >= 1 for r in recs)
    assert any(r.op == "gemm" and r.flags["stats_delivered"] and not r.flags["shared"] for r in recs)
    assert any(r.op == "gemm" and r.flags["stats_delivered"] and r.flags["quad"] for r in recs)


# ------------------------------------------------------------------------------------------------ fault injection
class _Faulty:
    """Corrupts the result of ONE launch: ``fault`` = (sequence number, fn(out, result, kwargs) -> result or None)."""
    fault = None

    def _hit(self, depth):
        return self.fault is not None and self._depth == depth and len(self.records) - 1 == self.fault[0]

    def gemm(self, A, W, out, **kw):
        res = super().gemm(A, W, out, **kw)
        if self._hit(1):                                  # (the outermost call: the audit has counted it in)
            new = self.fault[1](out, res, kw)
            res = res if new is None else new
        return res

    def attn_varlen(self, qkv, out, seq_rows, out_rows, cu, *args):
        res = super().attn_varlen(qkv, out, seq_rows, out_rows, cu, *args)
        if self._hit(0):
            self.fault[1](out, res, dict(out_rows=out_rows, cu=cu))
        return res


class FaultyTorchOps(_Faulty, TorchOps):
    pass


class FaultyFusingOps(_Faulty, la.FusingTorchOps):
    pass


def chunk_from_the_row_above(out, res, kw):
    """one 16-byte chunk (8 two-byte elements) of one row holds the row above's values"""
    o2 = out.reshape(-1, out.shape[-1])
    assert o2.data_ptr() == out.data_ptr() and out.element_size() == 2
    r = o2.shape[0] // 2 + 1
    assert not torch.equal(o2[r, 8:16], o2[r - 1, 8:16])
    o2[r, 8:16] = o2[r - 1, 8:16]


def two_frames_exchanged(out, res, kw):
    o, stats = res
    return o, stats[[1, 0] + list(range(2, stats.shape[0]))].contiguous()


def window_one_row_off(out, res, kw):
    cu = kw["cu"].tolist()
    rows = kw["out_rows"][cu[1]:cu[2]].long()
    out[rows] = out[rows].roll(1, dims=0)


def audit_names(ops, seq, op):
    """the audit fails exactly the faulted launch and names it"""
    assert [(r.seq, r.op) for r in ops.failed()] == [(seq, op)], [r.describe() for r in ops.failed()]
    with pytest.raises(AssertionError, match=rf"1 of {len(ops.records)} audited launches .*\n  launch #{seq} {op} "):
        ops.assert_clean()
    return ops.failed()[0]


def test_vae_faults_in_one_launch_are_named_and_the_engine_metric_does_not_see_them(vae_sd, vae_fusing_clean):
    clean_ops, clean = vae_fusing_clean
    dec = clean_ops.records
    third = dec[len(dec) // 3: 2 * len(dec) // 3]                       # the middle third of the decoder
    convs = [r for r in third if r.op == "gemm" and r.flags["taps"] == (3, 3, 3) and not r.flags["phase"]]
    fused = [r for r in third if r.op == "gemm" and r.flags["stats_delivered"] and not r.flags["shared"] and r.shapes["out"][0] >= 2]
    assert convs and fused
    cases = {"chunk": (convs[len(convs) // 2], chunk_from_the_row_above), "statistics": (fused[len(fused) // 2], two_frames_exchanged)}
    seen = {}
    for name, (target, fn) in cases.items():
        ops = la.audited(FaultyFusingOps)("cpu", act_dtype=BF16)
        ops.fault = (target.seq, fn)
        out = vae_decode_small(sub("vae").VideoVAEEngine(*vae_sd, ops))
        rec = audit_names(ops, target.seq, "gemm")
        seen[name] = rel_err(out, clean)
        print(f"VAE decode, {name} fault in {rec.describe()}: engine-level rel_err against the un-faulted run {seen[name]:.3e}")
        assert seen[name] > 0.0                                         # (the fault did reach the output)
        if name == "chunk":
            assert "in 1 rows" in rec.failures[0] and rec.worst > 1.0
        else:
            assert "fused GroupNorm statistics" in rec.failures[0] and rec.worst <= 1.0      # (the conv's own output is clean)
    assert seen["chunk"] < VAE_TOL and seen["statistics"] < VAE_TOL       # the engine test would have passed both


def test_dit_faults_in_one_launch_are_named_and_the_engine_metric_does_not_see_them(dit_clean):
    config = sub("config")
    clean_ops, clean = dit_clean["3b", "h16"]
    recs = clean_ops.records
    third = recs[len(recs) // 3: 2 * len(recs) // 3]
    gemms = [r for r in third if r.op == "gemm" and r.flags["epilogue"] == "swiglu" and r.flags["M"] > 58]
    attns = [r for r in third if r.op == "attn_varlen"]
    assert gemms and attns and attns[0].flags["windows"] >= 2
    seen = {}
    for name, (target, fn) in {"chunk": (gemms[0], chunk_from_the_row_above), "attention": (attns[0], window_one_row_off)}.items():
        ops = la.audited(FaultyTorchOps)("cpu", act_dtype=BF16)
        ops.fault = (target.seq, fn)
        out = run_dit(ops, config.DIT_TINY, "h16")
        rec = audit_names(ops, target.seq, target.op)
        seen[name] = rel_err(out, clean)
        print(f"DiT forward, {name} fault in {rec.describe()}: engine-level rel_err against the un-faulted run {seen[name]:.3e}")
        assert seen[name] > 0.0 and rec.worst > 1.0
    assert seen["chunk"] < DIT_TOL
