"""-m gpu: the kernels on data OUTSIDE the zero-mean, unit-scale Gaussians of the other kernel tests (tests/conditioning_cases.py).

  A. GroupNorm COMPOSED (statistics pass -> apply pass, and the statistics fused into the conv epilogues -> apply pass) against a
     two-pass fp64 reference of the stored values, on groups whose mean dominates their spread (rho = |mean| / std up to 1024):
     the variance the apply pass forms is E[x^2] - mean^2, so the sums must carry rho^2 more digits than the variance needs.
     le.check_groupnorm_variance states the requirement on the statistics (2^-9 (var + eps)), le.check_groupnorm on the output.
  B. Epilogues with a ZERO operand: the accumulator is exactly 0 and the stored value is store(epilogue(bias, resid)) -- a function
     stated exactly here, swept over rounding ties, overflow, the subnormal range of h16 and the saturation points of the fast
     activations, on every kernel class (asserted through record_kernel_class).
  C. The row-normalising kernels and the row softmax at the magnitudes the wide residual stream allows.
  D. Both window-attention kernels on STEERED scores (attn_score_cases): the running maximum growing by just under and just over
     the 2^6 of the window kernel's deferred rescale, rows of one query block that disagree about rescaling, weight on the key the
     ragged last tile duplicates, exponents down to -80 and scores of +-115 log2 units, the text rows' norm at the window's end --
     at lengths on both sides of a key tile and of the row table, head_dim 128 and 512, against le.check_attn per element.
     tests/test_local_error.py proves on the CPU that the correct algorithm passes these cases and a missing mask, a stale O and a
     stale l fail them.

Every tensor a svr_* entry point writes comes from tests/guarded_out.py: guard bytes around a payload poisoned with NaN (``init=``
where the launch gets a view that leaves the buffer's last row out, or works in place)."""
import functools
import math

import pytest
import torch

import local_error as le
from conditioning_cases import (offset_groups, scaled_rows, bias_sweep, act_sweep, zero_operand_problem, attn_score_cases, ROW_KINDS,
                                OPTION_DEFAULTS, STORE_KINDS, ZERO_OPERAND_CASES, ATTN_SCORE_CASES)
from conftest import sub
from guarded_out import Pool, guarded
from ops_reference import H16, H16_SCALE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_RESID_GATE, EPI_SWIGLU, _ld, _st

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
KINDS = [BF16, H16, F32]
KIND_IDS = ["bf16", "h16", "fp32"]
EPS = 1e-6
G = 32


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def rnd(*shape, scale=1.0, seed=0, dtype=BF16):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    v = torch.randn(*shape, generator=g, device="cuda") * scale
    return (v * H16_SCALE).to(H16) if dtype == H16 else v.to(dtype)


def nans(*shape, dtype=BF16):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def checked(g, tag):
    """a guarded buffer after the launch that owns all of it: guards intact, no poison left -> its tensor"""
    g.assert_guards(tag)
    g.assert_written(tag)
    return g.t


def gamma_beta(C):
    return rnd(C, dtype=F32, seed=1) + 1, rnd(C, dtype=F32, seed=2)


def all_of(checks):
    """Run every check (each prints its figure), then fail with all the messages: one parametrised case reports every ratio."""
    errs = []
    for fn in checks:
        try:
            fn()
        except AssertionError as e:
            errs.append(str(e))
    assert not errs, "\n".join(errs)


# ================================================================== A. GroupNorm, composed
def _composed(hip, x, stats, tag, silus=(True, False)):
    """check_groupnorm_variance on ``stats`` and groupnorm_apply fed with them against the two-pass reference -> list of checks"""
    T, H, W, C = x.shape
    gamma, beta = gamma_beta(C)
    checks = [lambda: le.check_groupnorm_variance(stats, x, G, EPS, name=f"variance {tag}")]
    for silu in silus:
        g = guarded((T + 1, H, W, C), BF16, init=nans(T + 1, H, W, C))
        out = g.t
        hip.groupnorm_apply(x, out[:T], stats, gamma, beta, G, EPS, silu)
        assert bool(torch.isnan(out[T]).all()) and not bool(torch.isnan(out[:T].float()).any()), tag
        g.assert_guards(f"groupnorm_apply {tag}")
        checks.append(lambda out=out, silu=silu: le.check_groupnorm(out[:T], x, gamma, beta, G, EPS, silu, name=f"composed {tag} silu {silu}"))
    return checks


# 37 x 41 = 1517 rows: one ragged row block; 3 x 683 = 2049: two blocks, the second with ONE row; 64 x 64 = 4096: two full blocks
GN_HW = [(37, 41), (3, 683), (64, 64)]


@pytest.mark.parametrize("rho", [0.5, 16.0, 256.0, 1024.0])
@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("H,W", GN_HW, ids=[f"HW{h * w}" for h, w in GN_HW])
def test_groupnorm_composed_on_offset_groups(hip, H, W, kind, C, rho):
    """groupnorm_stats -> groupnorm_apply on x = std (rho_tg + N(0, 1)), std 1 and 2^-6, every (frame, group) at another rho_tg
    between 9/16 rho and rho (offset_groups), both SiLU settings."""
    checks = []
    for std in (1.0, 2.0 ** -6):
        x = offset_groups(2, H, W, C, G, rho, std, kind, "cuda")
        g = guarded((2, G, 2), F64)
        hip.groupnorm_stats(x, g.t, G)
        stats = checked(g, "groupnorm_stats")
        checks += _composed(hip, x, stats, f"rho {rho} std {std}")
    all_of(checks)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("H,W", [(37, 41), (3, 683)], ids=["HW1517", "HW2049"])
def test_groupnorm_constant_groups(hip, H, W, kind):
    """Groups constant at 0, at 1000 and at -3e5 among ordinary ones: their variance is 0 exactly, the sums cancel completely.
    The clamp var >= 0 must hold (a rounding residue below zero would put a NaN into rstd), the output is finite and the
    normalised value is act(beta) within the bound."""
    T, C = 2, 128
    x = _ld(offset_groups(T, H, W, C, G, 0.5, 1.0, F32, "cuda"))
    const = ((3, 0.0), (4, 1000.0), (17, -3e5), (31, 1000.0))
    for g, v in const:
        x[..., g * 4:g * 4 + 4] = v
    x = _st(x, torch.empty(0, dtype=kind, device="cuda"))                         # (names the storage kind: no entry point writes it)
    mean, var = le.two_pass_moments(x, G)
    assert bool((var[:, [g for g, _ in const]] == 0).all())
    gs = guarded((T, G, 2), F64)
    hip.groupnorm_stats(x, gs.t, G)
    stats = checked(gs, "groupnorm_stats")
    gamma, beta = gamma_beta(C)
    checks = _composed(hip, x, stats, "constant groups")
    for silu in (True, False):
        go = guarded((T, H, W, C), BF16)
        hip.groupnorm_apply(x, go.t, stats, gamma, beta, G, EPS, silu)
        out = checked(go, "groupnorm_apply")
        assert bool(torch.isfinite(out.float()).all())
        b = torch.nn.functional.silu(beta.double()) if silu else beta.double()
        want, _ = le.groupnorm_reference(x, gamma, beta, G, EPS, silu)
        for g, _ in const:
            assert torch.allclose(want[..., g * 4:g * 4 + 4], b[g * 4:g * 4 + 4].expand(T, H, W, 4), rtol=1e-14 if silu else 0.0, atol=0.0)
        if not silu:                          # the group at 0: x a + b with x = 0 and mean = 0 is beta -- bit-exact
            assert torch.equal(out[..., 12:16], beta[12:16].to(BF16).expand(T, H, W, 4))
    all_of(checks)


def test_groupnorm_statistics_of_a_frame_do_not_depend_on_the_clip_at_rho_256(hip):
    """The slicing invariance of the statistics pass (a frame handed over alone == the same frame inside a clip, bit for bit;
    two launches bit-identical), re-asserted on offset data: an accumulation scheme chosen for accuracy must keep it."""
    for kind in KINDS:
        for H, W in ((3, 683), (64, 64)):
            x = offset_groups(3, H, W, 128, G, 256.0, 1.0, kind, "cuda")
            gout = Pool()
            stats, again = (gout(3, G, 2, dtype=F64) for _ in range(2))
            hip.groupnorm_stats(x, stats, G)
            hip.groupnorm_stats(x, again, G)
            assert torch.equal(stats, again)
            for t in range(3):
                one = gout(1, G, 2, dtype=F64)
                hip.groupnorm_stats(x[t:t + 1].contiguous(), one, G)
                assert torch.equal(one[0], stats[t]), (kind, H, W, t)
            gout.check("groupnorm_stats")


def _group_bias(free, rho, To):
    """bias [C] = rho_g s_g: s_g the measured std of group g of the bias-free output (frame 0), rho_g = rho (1 - (g % 8) / 16)
    with alternating sign"""
    _, var = le.two_pass_moments(free[:1], G)
    g = torch.arange(G, device="cuda")
    r = rho * (1.0 - (g % 8).double() / 16.0) * (1.0 - 2.0 * (g % 2))
    return (r * var[0].sqrt()).repeat_interleave(free.shape[-1] // G).float().contiguous()


def _fused_case(hip, launch, C, kind, rho, tag):
    """``launch(bias, out) -> stats``: a conv launch with fused statistics.  Bias-free first (measures s), then with bias = rho s:
    the statistics against the two-pass reference OF THE TENSOR THE LAUNCH STORED, the apply pass fed with them, and two launches
    bit-identical in output and statistics."""
    free = launch(torch.zeros(C, device="cuda"), None)[0]
    bias = _group_bias(free, rho, free.shape[0])
    out, stats = launch(bias, None)
    out2, stats2 = launch(bias, None)
    assert stats is not None and torch.equal(stats, stats2) and torch.equal(out, out2), tag
    assert out.dtype == kind and bool(torch.isfinite(_ld(out)).all())
    all_of(_composed(hip, out, stats, f"{tag} rho {rho}"))


@pytest.mark.parametrize("rho", [0.5, 16.0, 256.0, 1024.0])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_conv_halo_fused_statistics_on_offset_outputs(hip, kind, rho):
    """LDS-halo conv 128 -> 128, T 3, 37 x 70 (ragged patches), its default variant (register-streamed weights, 8 rows)."""
    packing, opsmod = sub("packing"), sub("ops")
    T, H, W, C = 3, 37, 70, 128
    x = rnd(T, H, W, C)
    Wp = packing.pack_conv3d(rnd(C, C, 3, 3, 3, scale=1.0 / math.sqrt(C * 27), seed=2), "cuda")
    Wf = hip.pack_conv_frag(Wp, 3, C, C)
    geom = opsmod.Conv3dGeom(T, H, W, C, T, H, W, (3, 3, 3), (1, 1, 1), (2, 1, 1), None)

    def launch(bias, _):
        g = guarded((T, H, W, C), kind)
        hip.record_kernel_class = True
        try:
            res = hip.gemm(x, Wp, g.t, N=C, K=Wp.shape[1], bias=bias, conv=geom, ldc=C, W_frag=Wf, gn_groups=G, out_f32=kind != BF16)
            assert hip.last_kernel_class == "conv_halo"
        finally:
            hip.record_kernel_class = False
        checked(g, "conv_halo")
        return res
    _fused_case(hip, launch, C, kind, rho, "conv_halo")


@pytest.mark.parametrize("rho", [0.5, 16.0, 256.0, 1024.0])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_conv_thin_input_fused_statistics_on_offset_outputs(hip, kind, rho):
    """The thin-input variant (RGB padded to 4 channels -> 128), 3 x 21 x 70."""
    packing, opsmod = sub("packing"), sub("ops")
    T, H, W, C = 3, 21, 70, 128
    x = rnd(T, H, W, 4)
    x[..., 3] = 0
    Wp = packing.pack_conv3d(rnd(C, 3, 3, 3, 3, scale=1.0 / math.sqrt(81), seed=2), "cuda", 4)
    geom = opsmod.Conv3dGeom(T, H, W, 4, T, H, W, (3, 3, 3), (1, 1, 1), (2, 1, 1), None)

    def launch(bias, _):
        g = guarded((T, H, W, C), kind)
        hip.record_kernel_class = True
        try:
            res = hip.gemm(x, Wp, g.t, N=C, K=Wp.shape[1], bias=bias, conv=geom, ldc=C, gn_groups=G, out_f32=kind != BF16)
            assert hip.last_kernel_class == "conv_thin_in"
        finally:
            hip.record_kernel_class = False
        checked(g, "conv_thin_in")
        return res
    _fused_case(hip, launch, C, kind, rho, "conv_thin_in")


@pytest.mark.parametrize("rho", [0.5, 16.0, 256.0, 1024.0])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_conv_subpixel_fused_statistics_on_offset_outputs(hip, kind, rho):
    """The sub-pixel upsampler kernel, 3 x 9 x 11, 128 -> 128, quad launch: the four phases share one partial buffer; every phase
    (and its border voxels) gets the same bias."""
    packing, opsmod = sub("packing"), sub("ops")
    T, H, W, C, kt = 3, 9, 11, 128, 3
    x = rnd(T, H, W, C)
    wts = []
    for ph, (py, px) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        Wp = packing.pack_conv3d(rnd(C, C, kt, 2, 2, scale=1.0 / math.sqrt(C * 4 * kt), seed=20 + ph), "cuda")
        wts.append((py, px, Wp, hip.pack_conv_frag(Wp, kt, C, C, taps=(2, 2))))
    geom = opsmod.Conv3dGeom(T, H, W, C, T, H, W, (kt, 2, 2), (1, 1, 1), (kt - 1, 1, 1), None)

    def launch(bias, _):
        g = guarded((T, 2 * H, 2 * W, C), kind)                                     # (poisoned: the quad launch owns all four phases)
        out = g.t
        bb = bias[None, :].expand(3, C).contiguous()
        quad = [(py, px, Wp, bias, bb, Wf) for py, px, Wp, Wf in wts]
        shared = {"frames": T, "frame0": 0}
        hip.record_kernel_class = True
        try:
            hip.gemm(x, wts[0][2], out, N=C, K=wts[0][2].shape[1], bias=bias, conv=geom, W_frag=wts[0][3],
                     phase=opsmod.PhaseScatter(0, 0, bb, 1, quad=quad), gn_groups=G, gn_shared=shared, out_f32=kind != BF16)
            assert hip.last_kernel_class == "conv_subpixel"
        finally:
            hip.record_kernel_class = False
        return checked(g, "conv_subpixel quad"), hip.gn_shared_stats(shared)
    _fused_case(hip, launch, C, kind, rho, "conv_subpixel quad")


# ================================================================== B. epilogues with a zero operand
DENORMAL = 2.0 ** -126                  # results in fp32's denormal range may be flushed (le.gemm_reference(abs_err=))
H16_TOP = 65504.0 * 64.0 * (1.0 - 2.0 ** -11)     # below it an h16 store cannot overflow; bf16's top is fp32's


class ZeroLaunch:
    """One ZERO_OPERAND_CASES launch on the device: A = 0, so what is stored is store(epilogue(bias, resid))."""

    def __init__(self, hip, name):
        self.hip, self.name, self.spec = hip, name, ZERO_OPERAND_CASES[name]

        def frag(kind, W, spec):
            if kind == "gemm":
                return hip.pack_gemm_frag(W)
            Cin, Cout, k = spec["conv"][:3]
            return hip.pack_conv_frag(W, k[0], Cin, Cout, taps=(3, 3) if kind == "conv33" else (2, 2))
        self.A, self.W, self.kw, self.shape = zero_operand_problem(self.spec, sub("ops"), "cuda", frag)
        assert self.kw.get("W_frag", 0) is not None
        self.N = self.kw["N"]
        self.M = math.prod(self.shape) // self.N

    def __call__(self, kind, cls=None, **epi):
        """-> the [M, N] view of the tensor the launch stored (NaN before it), after asserting the kernel class"""
        hip, g = self.hip, guarded(self.shape, kind)
        out = g.t
        for k, v in {**OPTION_DEFAULTS, **self.spec.get("options", {})}.items():
            hip.set_option(k, v)
        hip.record_kernel_class = True
        try:
            hip.gemm(self.A, self.W, out, out_f32=kind != BF16, **self.kw, **epi)
            assert hip.last_kernel_class == (cls or self.spec["cls"]), (self.name, hip.last_kernel_class)
        finally:
            hip.record_kernel_class = False
            for k, v in OPTION_DEFAULTS.items():
                hip.set_option(k, v)
        return checked(g, f"{self.name} {kind}").reshape(self.M, self.N)

    def vectors(self, sweep):
        """the sweep tiled over N; N shorter than the sweep: one launch per piece (the last one wraps around)"""
        n = sweep.numel()
        if self.N >= n:
            return [sweep.repeat(-(-self.N // n))[:self.N].contiguous()]
        return [sweep.roll(-s)[:self.N].contiguous() for s in range(0, n, self.N)]


@pytest.fixture(scope="module")
def zero_launch(hip):
    made = {}
    return lambda name: made[name] if name in made else made.setdefault(name, ZeroLaunch(hip, name))


def assert_same_bits(got, want, tag):
    raw = torch.int16 if got.element_size() == 2 else torch.int32
    g, w = got.view(raw), want.expand_as(got).contiguous().view(raw)
    if not torch.equal(g, w):
        r, c = (int(i[0]) for i in torch.nonzero(g != w, as_tuple=True))
        raise AssertionError(f"{tag}: {int((g != w).sum())} of {g.numel()} stored values differ; first at row {r}, column {c}: got bits "
                             f"{int(g[r, c]) & 0xffffffff:#x} ({float(_ld(got)[r, c])!r}), want {int(w[r, c]) & 0xffffffff:#x} "
                             f"({float(_ld(want.expand_as(got))[r, c])!r})")


def stored(values, kind):
    return _st(values, torch.empty(0, dtype=kind, device=values.device))            # (names the storage kind: no entry point writes it)


@pytest.mark.parametrize("name", list(ZERO_OPERAND_CASES))
def test_zero_operand_bias_store_is_bit_exact(zero_launch, name):
    """EPI_BIAS: stored == bf16(bias) | half(bias 2^-6) | bias, torch's round-to-nearest-even conversions, on rounding ties with
    even and odd lower neighbours, at the overflow thresholds and in h16's subnormal range (bias_sweep).  The accumulator is +0,
    so a bias of -0 is stored as 0 + (-0) = +0."""
    L = zero_launch(name)
    for bias in L.vectors(bias_sweep("cuda")):
        for kn, kind in STORE_KINDS.items():
            got = L(kind, bias=bias)
            assert_same_bits(got, stored(0.0 + bias, kind)[None, :], f"{name} bias -> {kn}")


def test_zero_operand_persistent_gemm_with_fragment_ordered_weights(zero_launch):
    """gemm_persistent with W_frag (weights streamed to registers) stores the same bits as without."""
    L = zero_launch("gemm_persistent")
    Lf = ZeroLaunch(L.hip, "gemm_persistent")
    Lf.kw["W_frag"] = L.hip.pack_gemm_frag(L.W)
    assert Lf.kw["W_frag"] is not None
    bias = L.vectors(bias_sweep("cuda"))[0]
    for kn, kind in STORE_KINDS.items():
        a, b = L(kind, bias=bias), Lf(kind, bias=bias)
        assert_same_bits(b, stored(0.0 + bias, kind)[None, :], f"gemm_persistent W_frag bias -> {kn}")
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    acts = act_sweep("cuda").repeat(L.N // 32)
    for epi in (EPI_BIAS_SILU, EPI_BIAS_GELU):
        a, b = L(BF16, bias=acts, epilogue=epi), Lf(BF16, bias=acts, epilogue=epi)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("name", [n for n, s in ZERO_OPERAND_CASES.items() if s.get("pairs") != ()])
def test_zero_operand_residual_add_is_bit_exact(zero_launch, name):
    """EPI_RESID_GATE without a gate: stored == store((0 + bias) + resid), ONE fp32 add, for every (output, residual) storage kind
    the class has a form for.  Residual rows in turn: -bias (cancels to 0 where the residual's format holds the bias exactly),
    +bias (doubles: overflows the h16 store at the top of the sweep), the sweep shifted by one and by seven columns."""
    L = zero_launch(name)
    pairs = L.spec.get("pairs") or [(o, r) for o in STORE_KINDS for r in STORE_KINDS]
    row = torch.arange(L.M, device="cuda")[:, None] % 4
    saw_zero = saw_inf = False
    for bias in L.vectors(bias_sweep("cuda")):
        b = bias[None, :]
        rv = torch.where(row == 0, -b, torch.where(row == 1, b, torch.where(row == 2, b.roll(1, 1), -b.roll(7, 1)))).contiguous()
        for on, rn in pairs:
            resid = stored(rv, STORE_KINDS[rn]).reshape(L.shape)
            got = L(STORE_KINDS[on], bias=bias, epilogue=EPI_RESID_GATE, resid=resid, ldr=L.N)
            want = stored((0.0 + b) + _ld(resid).reshape(L.M, L.N), STORE_KINDS[on])
            assert not bool(torch.isnan(_ld(got)).any())
            assert_same_bits(got, want, f"{name} {rn} residual -> {on}")
            saw_zero, saw_inf = saw_zero or bool((_ld(got)[0::4] == 0).any()), saw_inf or bool(torch.isinf(_ld(got)).any())
    assert saw_zero and saw_inf                                 # pairs that cancelled to 0, pairs that overflowed the store


ACT_CASES = [(n, e) for n, s in ZERO_OPERAND_CASES.items() for e in s["acts"]]


def _act_checks(got, want, bound, mask, bias, kind, tag):
    """No NaN; inside the bound wherever the exact result fits the output format; arguments <= -100 give +-0, arguments >= 100
    give the argument itself (rounded to the format: possibly inf)."""
    v = _ld(got)
    assert not bool(torch.isnan(v).any()), tag
    fits = want.abs() < (H16_TOP if kind == H16 else 3.3e38)
    le.check(tag, got, want, bound, mask & fits.reshape(mask.shape))
    assert bool((v[:, bias <= -100.0] == 0).all()), tag
    big = bias >= 100.0
    assert_same_bits(got[:, big], stored(bias[big], kind)[None, :], tag + ", arguments >= 100")


@pytest.mark.parametrize("name,epi", ACT_CASES, ids=[f"{n}-{'silu' if e == EPI_BIAS_SILU else 'gelu'}" for n, e in ACT_CASES])
def test_zero_operand_fast_activations(zero_launch, name, epi):
    """EPI_BIAS_SILU / EPI_BIAS_GELU at act(bias), bias over +-{0, 2^-130, 1e-30, 1e-3, 1, 10, 20, 80, 87, 88.7, 89, 100, 1e4, 1e19,
    3e38}: v_exp_f32 saturating to inf and to 0, v_rcp_f32 of inf, x^3 overflowing inside the GELU polynomial.  The kernel class that
    serves the launch is the one the case names -- the LDS-halo kernel has no GELU: such a launch must reach a kernel that has."""
    L = zero_launch(name)
    cls = L.spec["acts"][epi]
    kinds = [STORE_KINDS[k] for k in L.spec.get("act_kinds", STORE_KINDS)]
    for bias in L.vectors(act_sweep("cuda")):
        for kind in kinds:
            if cls == "error":
                with pytest.raises(Exception):
                    L(kind, bias=bias, epilogue=epi)
                continue
            got = L(kind, cls=cls, bias=bias, epilogue=epi)
            ref_kw = {k: v for k, v in L.kw.items() if k in ("N", "K", "conv")}
            want, bound, mask = le.gemm_reference(L.A, L.W, got.reshape(L.shape), bias=bias, epilogue=epi, abs_err=DENORMAL, **ref_kw)
            _act_checks(got, want.reshape(L.M, L.N), bound.reshape(L.M, L.N), mask.reshape(L.M, L.N), bias, kind, f"{name} epilogue {epi} -> {kind}")


@pytest.mark.parametrize("name", ["gemm_epi_direct", "gemm_epi_lds", "gemm_persistent"])
def test_swiglu_on_exact_accumulators(zero_launch, name):
    """EPI_SWIGLU has no bias: the sweep comes through the operand.  A has a single 1 per row (column 3; every third row all zero),
    W holds the sweep in that column, so the accumulator of column n IS W[n, 3] (bf16-exact values).  Gate columns: the activation
    sweep; in columns: 1 and -0.5.  silu(gate) * in against le.check_gemm, no NaN, gates <= -100 give +-0, gates >= 100 give
    gate * in exactly; all-zero rows give silu(0) * 0 = 0.  With and without the fragment-ordered weights: the same bits."""
    L = zero_launch(name)
    M, N, K = L.spec["mnk"]
    hip = L.hip
    A = torch.zeros(M, K, device="cuda", dtype=BF16)
    A[torch.arange(M, device="cuda") % 3 != 2, 3] = 1.0
    W = L.W.clone()
    sweep = act_sweep("cuda").to(BF16).float()                                     # (2^-130 is a bf16 denormal: an MFMA may flush it)
    grp = torch.arange(N // 32, device="cuda")
    gate = sweep.repeat(N // 64).reshape(N // 32, 16)                              # group g: sweep[16 (g % 2) ..]
    inn = torch.where((grp // 2) % 2 == 0, 1.0, -0.5)[:, None].expand(N // 32, 16)
    W[:N, 3] = torch.stack([gate, inn], dim=1).reshape(N).to(BF16)
    outs, gout = [], Pool()
    for frag in ([None, hip.pack_gemm_frag(W)] if name == "gemm_persistent" else [None]):
        out = gout(M, N // 2, dtype=BF16)
        for k, v in {**OPTION_DEFAULTS, **L.spec.get("options", {})}.items():
            hip.set_option(k, v)
        hip.record_kernel_class = True
        try:
            hip.gemm(A, W, out, N=N, K=K, epilogue=EPI_SWIGLU, W_frag=frag)
            assert hip.last_kernel_class == L.spec["cls"]
        finally:
            hip.record_kernel_class = False
            for k, v in OPTION_DEFAULTS.items():
                hip.set_option(k, v)
        outs.append(out)
    out = outs[0]
    assert all(torch.equal(o.view(torch.int16), out.view(torch.int16)) for o in outs[1:])
    assert not bool(torch.isnan(out.float()).any())
    le.check_gemm(out, A, W, N=N, K=K, epilogue=EPI_SWIGLU, abs_err=DENORMAL, name=f"{name} swiglu")
    gout.check(f"{name} swiglu")
    g, i = gate.reshape(-1), inn.reshape(-1)
    live = out[torch.arange(M, device="cuda") % 3 != 2]
    assert bool((out[2::3] == 0).all()) and bool((live[:, g <= -100.0] == 0).all())
    assert_same_bits(live[:, g >= 100.0], (g * i)[g >= 100.0].to(BF16)[None, :], f"{name} swiglu, gates >= 100")


@pytest.mark.parametrize("kind", [F32, BF16], ids=["fp32", "bf16"])
def test_groupnorm_apply_silu_over_the_activation_sweep(hip, kind):
    """groupnorm_apply's SiLU on the same arguments: statistics that say mean 0, var + eps = 1 (rstd rounds to 1.0f), gamma 1,
    beta 0 -> y = silu(x), x the activation sweep along the channels."""
    T, H, W, C = 1, 2, 3, 128
    sweep = act_sweep("cuda").repeat(C // 32)
    x = stored(sweep.expand(T, H, W, C).contiguous(), kind)
    n = H * W * (C // G)
    stats = torch.zeros(T, G, 2, device="cuda", dtype=F64)
    stats[..., 1] = n * (1.0 - float(torch.tensor(EPS, dtype=F32)))
    gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    g = guarded((T, H, W, C), BF16)
    hip.groupnorm_apply(x, g.t, stats, gamma, beta, G, EPS, True)
    out = checked(g, "groupnorm_apply silu sweep")
    want, bound = le.groupnorm_apply_reference(x, stats, gamma, beta, G, EPS, True)
    xv = _ld(x)[0, 0, 0]
    _act_checks(out.reshape(-1, C), want.reshape(-1, C), (bound + DENORMAL).reshape(-1, C), torch.ones(H * W, C, dtype=torch.bool, device="cuda"),
                xv, BF16, f"groupnorm_apply silu, {kind} input")


# ================================================================== C. row-normalising kernels, softmax
@pytest.mark.parametrize("dim", [2560, 8])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_rmsnorm_mod_at_the_magnitudes_of_the_wide_stream(hip, kind, dim):
    """Rows scaled by 2^-20, 1 and 2^21, rows with one channel x300, all-zero rows, alone in their 4-row block and mixed within
    one (scaled_rows).  An all-zero row gives ``shift`` exactly (0 without one)."""
    x, which = scaled_rows(dim, kind, "cuda")
    w, sc, sh = (rnd(dim, dtype=F32, seed=s) for s in (1, 2, 3))
    for kw in (dict(), dict(scale=sc, shift=sh), dict(w=w, scale=sc, shift=sh)):
        g = guarded((x.shape[0] + 1, dim), BF16, init=nans(x.shape[0] + 1, dim))
        out = g.t
        hip.rmsnorm_mod(x, out[:-1], 1e-5, **kw)
        assert bool(torch.isnan(out[-1]).all()) and bool(torch.isfinite(out[:-1].float()).all())
        g.assert_guards("rmsnorm_mod")
        zero = (le.values(x) == 0).all(dim=1)
        assert bool(zero[which == 4].all())
        want0 = (sh if "shift" in kw else torch.zeros(dim, device="cuda")).to(BF16)
        assert torch.equal(out[:-1][zero], want0.expand(int(zero.sum()), dim))
        for k, name in enumerate(ROW_KINDS):
            le.check_rmsnorm_mod(out[:-1][which == k], x[which == k], 1e-5, name=f"rmsnorm_mod rows {name} {sorted(kw)}", **kw)


def _rope_tables(n_pos, n_freq):
    ang = torch.arange(n_pos, dtype=F32)[:, None] * (10000.0 ** (-torch.arange(n_freq, dtype=F32) / max(n_freq, 1)))[None, :]
    return ang.cos().cuda().contiguous(), ang.sin().cuda().contiguous()


def test_qknorm_rope_at_the_magnitudes_of_the_wide_stream(hip):
    """heads 3 (one trimmed slot of the four-heads walk); the same row kinds, per row of qkv (bf16).  All-zero rows stay zero."""
    heads, n_pos, n_freq = 3, 64, 21
    qkv, which = scaled_rows(3 * heads * 128, BF16, "cuda")
    rows = qkv.shape[0]
    r = torch.arange(rows)
    pos = torch.stack([r % 7, (r * 7) % n_pos, (r * 13 + 5) % n_pos], -1).to(torch.int16).cuda()
    cos, sin = _rope_tables(n_pos, n_freq)
    wq, wk = rnd(128, dtype=F32, seed=1) + 1, rnd(128, dtype=F32, seed=2) + 1
    g = guarded(qkv.shape, BF16, init=qkv)                                         # (in place: q and k rewritten, V left alone)
    got = g.t
    hip.qknorm_rope(got, heads, pos, 2, cos, sin, wq, wk, 1e-5)
    g.assert_guards("qknorm_rope")
    assert torch.equal(got[:, 2 * heads * 128:], qkv[:, 2 * heads * 128:])
    assert bool(torch.isfinite(got.float()).all())
    assert bool((got[which == 4][:, :2 * heads * 128] == 0).all())
    for k, name in enumerate(ROW_KINDS):
        le.check_qknorm_rope(got[which == k], qkv[which == k], heads, pos[which == k], 2, cos, sin, wq, wk, 1e-5, name=f"qknorm_rope rows {name}")


@pytest.mark.parametrize("cols", [64, 16388])
def test_softmax_rows_wide_score_ranges(hip, cols):
    """Rows whose SCALED scores span +-1e4 (almost every exp2 argument saturates), rows of equal scores (large and small), one
    dominant score in the last column of the last float4."""
    scale = 0.044
    g = torch.Generator(device="cuda").manual_seed(cols)
    S = torch.randn(6, cols, device="cuda", generator=g) * 30.0
    span = torch.linspace(-1e4, 1e4, cols, device="cuda") / scale
    S[0] = span[torch.randperm(cols, device="cuda", generator=g)]
    S[1] = span                                                                    # ascending: the maximum comes last
    S[2] = 1e4 / scale                                                             # equal scores at the top of the range
    S[3] = -1e4 / scale
    S[4, -1] = 1e4 / scale                                                         # one dominant score, last column
    g = guarded((7, cols), BF16, init=nans(7, cols))
    P = g.t
    hip.softmax_rows(S, P[:6], scale)
    assert bool(torch.isnan(P[6]).all()) and bool(torch.isfinite(P[:6].float()).all())
    g.assert_guards("softmax_rows")
    le.check_softmax_rows(P[:6], S, scale, name=f"softmax_rows cols {cols}")
    assert torch.equal(P[2], P[3]) and float(P[4, -1]) == 1.0 and float(P[4, :-1].float().abs().max()) == 0.0


# ================================================================== D. window attention on steered score ranges
@pytest.fixture(params=[0, pytest.param(1, marks=pytest.mark.variants)], ids=["attn_win", "attn_gen1"])
def attn_impl(request, hip):
    """0 = the second-generation window kernel wherever it applies (head_dim 128, windows <= 2048 rows), 1 = the first kernel
    everywhere (as in tests/test_gpu_kernels.py)."""
    hip.set_option("attn_impl", request.param)
    yield request.param
    hip.set_option("attn_impl", 0)


@functools.lru_cache(maxsize=None)
def _score_cases(L, D):
    return attn_score_cases(L, D, 64 if D == 128 else 32, "cuda")


def _score_launch(hip, request, case, L, D, heads, attn_impl=None):
    """One launch of two windows: the case, and the case with its key and value rows in reversed order (a rising profile falls, the
    tail's weight moves to the head of the window).  Head 0 carries the case, a second head plain N(0, 1) data: state leaking between
    (window, head) pairs of very different range shows.  seq_rows and out_rows are permutations (a real gather and scatter).
    check_attn on every element (a non-finite one fails in it), three more launches bit-identical, guards and poison; under
    -m variants the window kernel's build variants store the same bits."""
    q, k, v = _score_cases(L, D)[case]
    plain = lambda j: rnd(2 * L, D, seed=17 * j + L)
    cols = [torch.cat([q, q]), torch.cat([k, k.flip(0)]), torch.cat([v, v.flip(0)])]
    logical = torch.cat([torch.stack([c] + [plain(3 * j + h) for h in range(1, heads)], dim=1).reshape(2 * L, heads * D)
                         for j, c in enumerate(cols)], dim=1)                       # [2 L, (q | k | v) x heads x D]
    g = torch.Generator().manual_seed(L + D)
    seq_rows = torch.randperm(2 * L, generator=g).to(torch.int32).cuda()
    out_rows = torch.randperm(2 * L, generator=g).to(torch.int32).cuda()
    qkv = torch.empty_like(logical)
    qkv[seq_rows.long()] = logical
    cu = torch.tensor([0, L, 2 * L], dtype=torch.int32, device="cuda")
    scale = 1.0 / math.sqrt(D)
    gout = Pool()
    out = gout(2 * L, heads * D, dtype=BF16)
    launch = lambda o: hip.attn_varlen(qkv, o, seq_rows, out_rows, cu, L, heads, D, scale)
    launch(out)
    for _ in range(3):
        assert torch.equal(launch(gout.like(out)), out)
    gout.check(f"attn_varlen {case}")
    if attn_impl == 0 and D == 128 and "variants" in (request.config.getoption("-m") or ""):
        for variant in (1, 3, 4):
            hip.set_option("attn_variant", variant)
            try:
                other = launch(gout.like(out))
            finally:
                hip.set_option("attn_variant", 0)
            assert torch.equal(other, out), variant
            gout.check(f"attn_varlen {case} variant {variant}")
    le.check_attn(out, qkv, seq_rows, out_rows, cu, heads, D, scale, name=f"attn_varlen {case} L {L} D {D}")


@pytest.mark.parametrize("case", ATTN_SCORE_CASES)
def test_attn_steered_scores(hip, request, attn_impl, case):
    """D = 128, L = 259 (four full key tiles and one of 3 keys; two 128-query tiles and a ragged one): every case of
    attn_score_cases, on both kernels."""
    _score_launch(hip, request, case, 259, 128, 2, attn_impl)


# 67: one full tile + 3 keys; 33: one ragged tile, the waves past the first two hold only clamped queries; 2048: the longest row
# table, 32 tiles; 2049: one row more -- served by the first-generation kernel whatever attn_impl says
@pytest.mark.parametrize("case,L", [(c, L) for L in (67, 33, 2048, 2049) for c in ("stairs", "tail_pair", "text_tail")
                                    if c != "text_tail" or L >= 64])
def test_attn_steered_scores_other_lengths(hip, request, attn_impl, case, L):
    _score_launch(hip, request, case, L, 128, 2, attn_impl)


@pytest.mark.parametrize("case,L", [(c, L) for L in (131, 35) for c in ATTN_SCORE_CASES if c != "text_tail" or L >= 64])
def test_attn_steered_scores_head_dim_512(hip, request, case, L):
    """The VAE form: one head of 512, the first-generation kernel's <512, 1, 32> instantiation (32-key tiles, 64-query blocks):
    131 = four tiles + 3 keys, 35 = one tile + 3."""
    _score_launch(hip, request, case, L, 512, 1)
