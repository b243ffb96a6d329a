"""-m "not gpu": the per-element checker of tests/local_error.py, proven on the CPU.

  * No false alarms: a correct implementation -- the fp32 restatement of tests/ops_reference.py with one rounding into the output's
    storage format -- stays inside every bound, for every op family, at the launch-geometry shapes of tests/test_gpu_side_kernels.py
    scaled to CPU size and at the small GEMM / conv / attention cases of tests/test_gpu_kernels.py.
  * Fault injection: a local fault put into a correct result fails the checker while the global metric the kernel tests used alone so
    far (||got - want|| / ||want|| < 2.5e-3, 4e-3 for attention) still passes -- the gap this checker closes.
  * The engines' glue kernels (ada_combine, patchify, im2col_causal, blend_accumulate, blend_finalize, affine_slice): the restatement
    is inside each bound (bit equality for pure data movement), a single-element or single-chunk fault is outside it, and the global
    metric lets that fault pass.
  * Attention on steered score ranges (conditioning_cases.attn_score_cases): the flash ALGORITHM of both kernels
    (tests/attn_emulation.py: key tiles, clamped and masked tail, one rescale vote per query block, deferral) is inside the bound on
    every case, and with the mask missing, O stale or l stale it is rejected on every case that can see the fault."""
import functools
import math

import pytest
import torch

import local_error as le
from attn_emulation import flash_emulation
from conditioning_cases import offset_groups, scaled_rows, act_sweep, attn_score_cases, ROW_KINDS, ATTN_SCORE_CASES
from conftest import sub, rel_err
from ops_reference import TorchOps, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_RESID_GATE, EPI_SWIGLU, H16, H16_SCALE, _ld, _st

BF16, F32 = torch.bfloat16, torch.float32
TOL_BF16, TOL_ATTN = 2.5e-3, 4e-3
STORES = [BF16, H16, F32]
ref = TorchOps("cpu", act_dtype=F32)


def rnd(*shape, scale=1.0, seed=0, dtype=BF16):
    g = torch.Generator().manual_seed(seed + sum(shape))
    v = torch.randn(*shape, generator=g) * scale
    return (v * H16_SCALE).to(H16) if dtype == H16 else v.to(dtype)


def must_fail(fn):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    assert "mod 256" in msg and "mod 16" in msg and "row-relative" in msg, msg
    return msg


def conv_weight(Cout, Cin, k, seed=2):
    w5 = rnd(Cout, Cin, *k, scale=1.0 / math.sqrt(Cin * k[0] * k[1] * k[2]), seed=seed)
    return w5, w5.permute(0, 2, 3, 4, 1).reshape(Cout, -1).contiguous()        # [N, (kt, kh, kw, Cin)]: the packed K order


# ------------------------------------------------------------------------------------------------ no false alarms
@pytest.mark.parametrize("out_dt", STORES, ids=["bf16", "h16", "fp32"])
@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (257, 64, 192), (1, 2560, 256), (513, 384, 64), (257, 64, 2560), (58, 256, 6912)])
def test_gemm_bias_is_inside_its_bounds(M, N, K, out_dt):
    A, W, bias = rnd(M, K), rnd(N, K, scale=1.0 / math.sqrt(K), seed=1), rnd(N, dtype=F32, seed=3)
    out = ref.gemm(A, W, torch.empty(M, N, dtype=out_dt), N=N, K=K, bias=bias)
    assert le.check_gemm(out, A, W, N=N, K=K, bias=bias) <= 1.0


@pytest.mark.parametrize("out_dt", STORES, ids=["bf16", "h16", "fp32"])
def test_gemm_epilogues_are_inside_their_bounds(out_dt):
    M, N, K = 777, 512, 320
    A, W = rnd(M, K), rnd(N, K, scale=1.0 / math.sqrt(K), seed=1)
    bias, gate = rnd(N, dtype=F32, seed=3), rnd(N, dtype=F32, seed=4)
    for res_dt in STORES:
        resid = rnd(M, N, seed=5, dtype=res_dt)
        for epi, kw in ((EPI_BIAS_SILU, {}), (EPI_BIAS_GELU, {}), (EPI_RESID_GATE, dict(gate=gate, resid=resid)),
                        (EPI_RESID_GATE, dict(resid=resid)), (EPI_RESID_GATE, dict(gate=gate))):
            kw = dict(N=N, K=K, bias=bias, epilogue=epi, **kw)
            out = ref.gemm(A, W, torch.empty(M, N, dtype=out_dt), **kw)
            le.check_gemm(out, A, W, name=f"epilogue {epi}", **kw)
    Hd = 768                                                              # SwiGLU: 16 gate | 16 in columns interleaved
    wg, wi = rnd(Hd, K, scale=1 / 16, seed=7), rnd(Hd, K, scale=1 / 16, seed=8)
    Wsw = torch.stack([wg.reshape(Hd // 16, 16, K), wi.reshape(Hd // 16, 16, K)], dim=1).reshape(2 * Hd, K)
    out = ref.gemm(A, Wsw, torch.empty(M, Hd, dtype=out_dt), N=2 * Hd, K=K, epilogue=EPI_SWIGLU)
    le.check_gemm(out, A, Wsw, N=2 * Hd, K=K, epilogue=EPI_SWIGLU, name="swiglu")
    closed = torch.nn.functional.silu(A.double() @ wg.double().t()) * (A.double() @ wi.double().t())
    assert rel_err(le.gemm_reference(A, Wsw, out, N=2 * Hd, K=K, epilogue=EPI_SWIGLU)[0], closed) < 1e-12


CONVS = [  # Cin, Cout, k, stride, pad(lo, hi), T, H, W, halo frames  (the small rows of CONV_CASES in tests/test_gpu_kernels.py)
    (128, 128, (3, 3, 3), (1, 1, 1), (1, 1), 3, 10, 12, 0),
    (128, 128, (3, 3, 3), (1, 1, 1), (1, 1), 2, 9, 7, 2),
    (256, 256, (3, 3, 3), (2, 2, 2), (0, 1), 4, 12, 10, 1),
    (128, 128, (1, 3, 3), (1, 2, 2), (0, 1), 3, 14, 16, 0),
    (512, 256, (1, 1, 1), (1, 1, 1), (0, 0), 3, 6, 5, 0),
    (128, 3, (3, 3, 3), (1, 1, 1), (1, 1), 3, 9, 11, 2),
    (4, 128, (3, 3, 3), (1, 1, 1), (1, 1), 3, 21, 30, 0),
]


def conv_problem(case, res_dt=BF16):
    ops = sub("ops")
    Cin, Cout, k, stride, (plo, phi), T, H, W, hf = case
    x = rnd(T, H, W, Cin)
    halo = rnd(hf, H, W, Cin, seed=9) if hf else None
    w5, Wp = conv_weight(Cout, Cin, k)
    pt = hf if hf else k[0] - 1
    To, Ho, Wo = (T + pt - k[0]) // stride[0] + 1, (H + plo + phi - k[1]) // stride[1] + 1, (W + plo + phi - k[2]) // stride[2] + 1
    geom = ops.Conv3dGeom(T, H, W, Cin, To, Ho, Wo, k, stride, (pt, plo, plo), halo)
    kw = dict(N=Cout, K=Wp.shape[1], bias=rnd(Cout, dtype=F32, seed=3), conv=geom, epilogue=EPI_RESID_GATE,
              resid=rnd(To, Ho, Wo, Cout, seed=11, dtype=res_dt))
    return x, w5, Wp, kw, (To, Ho, Wo, Cout)


@pytest.mark.parametrize("out_dt", STORES, ids=["bf16", "h16", "fp32"])
@pytest.mark.parametrize("case", CONVS)
def test_conv_is_inside_its_bounds(case, out_dt):
    x, w5, Wp, kw, shape = conv_problem(case, res_dt=out_dt)
    out = ref.gemm(x, Wp, torch.empty(shape, dtype=out_dt), **kw)
    assert le.check_gemm(out, x, Wp, **kw) <= 1.0
    # the fp64 reference is F.conv3d in double on the padded input the fp32 restatement builds: restated here from the 5-d weights
    g = kw["conv"]
    head = g.halo.double() if g.halo is not None else x[:1].double().expand(g.pad[0], *x.shape[1:])
    xin = torch.cat([head, x.double()], 0).permute(3, 0, 1, 2)[None] if g.pad[0] else x.double().permute(3, 0, 1, 2)[None]
    xin = torch.nn.functional.pad(xin, (case[4][0], case[4][1], case[4][0], case[4][1]))
    y = torch.nn.functional.conv3d(xin, w5.double(), kw["bias"].double(), stride=case[3])[0].permute(1, 2, 3, 0) + le.values(kw["resid"])
    assert rel_err(le.gemm_reference(x, Wp, out, **kw)[0], y) < 1e-12


@pytest.mark.parametrize("rz,drop", [(1, False), (2, False), (2, True)])
def test_pixel_shuffle_index_map_is_inside_its_bounds(rz, drop):
    ops = sub("ops")
    F_, H, W, Cc = 3, 5, 6, 64
    x, Wp = rnd(F_ * H * W, Cc), rnd(4 * rz * Cc, Cc, scale=1 / 8, seed=1)
    kw = dict(N=4 * rz * Cc, K=Cc, M=F_ * H * W, bias=rnd(4 * rz * Cc, dtype=F32, seed=3), ps=ops.PixelShuffleGeom(F_, H, W, rz, Cc, drop))
    out = ref.gemm(x, Wp, torch.empty(F_ * rz - (1 if drop else 0), 2 * H, 2 * W, Cc, dtype=BF16), **kw)
    le.check_gemm(out, x, Wp, **kw)
    must_fail(lambda: le.check_gemm(out.roll(1, dims=2), x, Wp, **kw))             # a wrong index map is not inside them


@pytest.mark.parametrize("kt,ts,hf", [(3, 1, 0), (2, 2, 1)])
def test_phase_scatter_writes_its_phase_only(kt, ts, hf):
    ops = sub("ops")
    T, H, W, Cin, Cout = 3, 7, 9, 64, 128
    x = rnd(T, H, W, Cin)
    halo = rnd(hf, H, W, Cin, seed=9) if hf else None
    pt = hf if hf else kt - 1
    To = T + pt - kt + 1
    out = torch.full((To * ts, 2 * H, 2 * W, Cout), float("nan"), dtype=BF16)
    for ph, (py, px) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        _, Wp = conv_weight(Cout, Cin, (kt, 2, 2), seed=20 + ph)
        geom = ops.Conv3dGeom(T, H, W, Cin, To, H, W, (kt, 2, 2), (1, 1, 1), (pt, 1 - py, 1 - px), halo)
        kw = dict(N=Cout, K=Wp.shape[1], bias=rnd(Cout, dtype=F32, seed=30 + ph), conv=geom,
                  phase=ops.PhaseScatter(py, px, rnd(3, Cout, dtype=F32, seed=40 + ph), ts))
        before = out.clone()
        ref.gemm(x, Wp, out, **kw)
        le.check_gemm(out, x, Wp, before=before, **kw)
        if ph == 0:                                                                # a launch that also touches another phase's voxel
            stray = out.clone()
            stray[0, 0, 1, 5] = 1.0
            with pytest.raises(AssertionError, match="not its own"):
                le.check_gemm(stray, x, Wp, before=before, **kw)


@pytest.mark.parametrize("lens,heads,D", [([135, 64, 1, 200, 129], 3, 128), ([64, 128, 192, 63, 65, 2, 1], 2, 128), ([100, 33, 257], 1, 512),
                                          ([640], 1, 128), ([300, 300, 77], 5, 128)])
def test_attention_is_inside_its_bounds(lens, heads, D):
    n_rows = 700
    qkv = rnd(n_rows, 3 * heads * D)
    g = torch.Generator().manual_seed(0)
    seq_rows = torch.cat([torch.randint(0, n_rows, (L,), generator=g) for L in lens]).int()
    total = sum(lens)
    out_rows = torch.randperm(total + 9, generator=g)[:total].int()
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    out = torch.full((total + 9, heads * D), 7.0, dtype=BF16)
    before = out.clone()
    ref.attn_varlen(qkv, out, seq_rows, out_rows, cu, max(lens), heads, D, 1.0 / math.sqrt(D))
    assert le.check_attn(out, qkv, seq_rows, out_rows, cu, heads, D, 1.0 / math.sqrt(D), before=before) <= 1.0


# (kt, qblock, defer, D, L): the second-generation window kernel (one vote per 32-query wave, deferral 2^6), the first-generation
# kernel (no deferral) at head_dim 128 and in its head_dim 512 instantiation (32-key tiles); then two more lengths of the first:
# 32 tiles, and one full tile plus 3 keys
ATTN_GEOMETRIES = {"win": (64, 32, 6.0, 128, 259), "gen1": (64, 128, None, 128, 259), "gen1_d512": (32, 64, None, 512, 131),
                   "win_2048": (64, 32, 6.0, 128, 2048), "win_67": (64, 32, 6.0, 128, 67)}
ATTN_SCORE_ITEMS = [(g, c) for g in ("win", "gen1", "gen1_d512") for c in ATTN_SCORE_CASES] + [("win_2048", "stairs"), ("win_67", "step_above")]
STALE_VISIBLE = ("step_above", "stairs", "rows_disagree", "one_row_votes", "tail_pair", "hot_gauss", "text_tail")


@functools.lru_cache(maxsize=None)
def _score_cases(geometry):
    kt, _, _, D, L = ATTN_GEOMETRIES[geometry]
    return attn_score_cases(L, D, kt)


@functools.lru_cache(maxsize=None)
def score_problem(geometry, case):
    """-> (q, k, v, scale, (want, bound, mask)): the fp64 reference of one case, computed once and shared by the tests below"""
    _, _, _, D, L = ATTN_GEOMETRIES[geometry]
    q, k, v = _score_cases(geometry)[case]
    rows, cu, scale = torch.arange(L, dtype=torch.int32), torch.tensor([0, L], dtype=torch.int32), 1.0 / math.sqrt(D)
    return q, k, v, scale, le.attn_reference(torch.cat([q, k, v], dim=1), torch.empty(L, D, dtype=BF16), rows, rows, cu, 1, D, scale)


def emulate(geometry, case, fault=None, decisions=None):
    kt, qblock, defer, _, _ = ATTN_GEOMETRIES[geometry]
    q, k, v, scale, _ = score_problem(geometry, case)
    return flash_emulation(q, k, v, scale, kt=kt, qblock=qblock, defer=defer, fault=fault, decisions=decisions)


@pytest.mark.parametrize("geometry,case", ATTN_SCORE_ITEMS)
def test_attention_algorithm_is_inside_its_bounds_on_steered_scores(geometry, case):
    """The flash algorithm of both kernels (tests/attn_emulation.py) on the score-range cases of conditioning_cases.attn_score_cases:
    inside attn_reference's bound on every element -- the bound itself, not a measured share of it.  The deferred and the forced
    branch are both taken where the case says so (step_below: [rescale, defer, ...]; step_above: [rescale, rescale, defer, ...];
    stairs: in turn)."""
    decisions = []
    out = emulate(geometry, case, decisions=decisions)
    assert le.check(f"attention emulation {geometry} {case}", out, *score_problem(geometry, case)[4]) <= 1.0
    if ATTN_GEOMETRIES[geometry][2] is not None:
        took = ["rescale" if bool(d.all()) else "defer" if not bool(d.any()) else "mixed" for d in decisions]
        want = {"step_below": ["rescale"] + ["defer"] * (len(took) - 1), "step_above": ["rescale", "rescale"] + ["defer"] * (len(took) - 2),
                "stairs": ["rescale", "defer"] * (len(took) // 2) + ["rescale"] * (len(took) % 2), "rows_disagree": ["rescale"] * len(took)}
        # (the first 8 tiles: bf16 moves g = 5.75 tile by up to 5.75 tile 2^-9, so from tile 11 on a step may measure more than 6)
        if case in want:
            assert took[:8] == want[case][:8], (case, took)


@pytest.mark.parametrize("geometry,case", ATTN_SCORE_ITEMS)
def test_attention_faults_are_rejected_on_steered_scores(geometry, case):
    """Each way the online softmax can be broken fails the per-element check on the cases that can see it:
      * the -inf mask of the ragged tile missing: every case but ramp_down (whose last tile weighs 2^-80), wherever L has a ragged tile;
      * O, or l, not multiplied by alpha at a rescale: every case whose running maximum moves after tile 0 (a first-generation
        geometry rescales on every tile, but with alpha = 1 on the flat cases).
    At deferral 2^6, step_below with a stale O PASSES (no rescale after tile 0: the fault has nothing to act on) while step_above
    fails: the two cases differ in the branch the block takes."""
    kt, _, defer, _, L = ATTN_GEOMETRIES[geometry]
    ref3 = score_problem(geometry, case)[4]
    visible = {"nomask": case != "ramp_down" and L % kt != 0, "stale_o": case in STALE_VISIBLE, "stale_l": case in STALE_VISIBLE}
    for fault, seen in visible.items():
        if seen:
            must_fail(lambda: le.check(f"{geometry} {case} {fault}", emulate(geometry, case, fault), *ref3))
    if defer is not None and case == "step_below":
        assert le.check(f"{geometry} step_below stale_o", emulate(geometry, case, "stale_o"), *ref3) <= 1.0


@pytest.mark.parametrize("kind", STORES, ids=["bf16", "h16", "fp32"])
@pytest.mark.parametrize("rows,dim", [(37, 8), (33, 520), (1000, 2560), (19, 3072), (21, 4096)])
def test_rmsnorm_mod_is_inside_its_bounds(rows, dim, kind):
    ramp = torch.logspace(-2, 2, rows)[:, None]                                    # per-row magnitudes 0.01 .. 100
    x = _st(rnd(rows, dim, dtype=F32) * ramp, torch.empty(0, dtype=kind))
    w, sc, sh = (rnd(dim, dtype=F32, seed=s) for s in (1, 2, 3))
    for kw in (dict(), dict(scale=sc, shift=sh), dict(w=w, scale=sc, shift=sh)):
        out = ref.rmsnorm_mod(x, torch.empty(rows, dim, dtype=BF16), 1e-5, **kw)
        assert le.check_rmsnorm_mod(out, x, 1e-5, **kw) <= 1.0


@pytest.mark.parametrize("kind", STORES, ids=["bf16", "h16", "fp32"])
@pytest.mark.parametrize("dim", [2560, 8])
def test_rmsnorm_mod_is_inside_its_bounds_at_the_magnitudes_of_the_wide_stream(dim, kind):
    """Rows scaled by 2^-20 / 1 / 2^21, one channel x300, all zero, alone and mixed in a 4-row block (scaled_rows): the fp32
    arithmetic of the restatement stays inside the (relative) bound at every magnitude -- the inputs of the GPU test are ones a
    correct fp32 kernel survives."""
    x, which = scaled_rows(dim, kind)
    w, sc, sh = (rnd(dim, dtype=F32, seed=s) for s in (1, 2, 3))
    for kw in (dict(), dict(scale=sc, shift=sh), dict(w=w, scale=sc, shift=sh)):
        out = ref.rmsnorm_mod(x, torch.empty(x.shape[0], dim, dtype=BF16), 1e-5, **kw)
        for k, name in enumerate(ROW_KINDS):
            assert le.check_rmsnorm_mod(out[which == k], x[which == k], 1e-5, name=f"rmsnorm_mod rows {name}", **kw) <= 1.0
        assert torch.equal(out[which == 4], (sh if "shift" in kw else torch.zeros(dim)).to(BF16).expand(int((which == 4).sum()), dim))


def rope_tables(n_pos, n_freq):
    ang = torch.arange(n_pos, dtype=F32)[:, None] * (10000.0 ** (-torch.arange(n_freq, dtype=F32) / n_freq))[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


@pytest.mark.parametrize("heads,n_freq", [(1, 21), (3, 10), (5, 1), (20, 21), (24, 10)])
def test_qknorm_rope_is_inside_its_bounds(heads, n_freq):
    rows, n_pos = 211, 40
    qkv = rnd(rows, 3 * heads * 128, scale=3.0)
    pos = torch.stack([torch.arange(rows) % 7, torch.arange(rows) % 31, torch.arange(rows) % n_pos], -1).to(torch.int16)
    cos, sin = rope_tables(n_pos, n_freq)
    wq, wk = rnd(128, dtype=F32, seed=1) + 1, rnd(128, dtype=F32, seed=2) + 1
    got = ref.qknorm_rope(qkv.clone(), heads, pos, 5, cos, sin, wq, wk, 1e-5)
    assert le.check_qknorm_rope(got, qkv, heads, pos, 5, cos, sin, wq, wk, 1e-5) <= 1.0
    # positions that leave the table are clamped by the kernel: the reference takes the clamped rows (the fp32 restatement would
    # wrap or raise, so the clamped positions are handed to it)
    far = pos.clone()
    far[::3, 0] -= 9
    far[1::3, 0] += n_pos
    clamped = far.clone()
    clamped[:, 0] = (far[:, 0].long() + 5).clamp(0, n_pos - 1).to(torch.int16) - 5
    got = ref.qknorm_rope(qkv.clone(), heads, clamped, 5, cos, sin, wq, wk, 1e-5)
    le.check_qknorm_rope(got, qkv, heads, far, 5, cos, sin, wq, wk, 1e-5, name="qknorm_rope clamped")
    touched = got.clone()
    touched[7, 2 * heads * 128 + 3] += 1
    with pytest.raises(AssertionError, match="V columns"):
        le.check_qknorm_rope(touched, qkv, heads, pos, 5, cos, sin, wq, wk, 1e-5)


def test_qknorm_rope_is_inside_its_bounds_at_the_magnitudes_of_the_wide_stream():
    heads, n_pos, n_freq = 3, 64, 21
    qkv, which = scaled_rows(3 * heads * 128, BF16)
    r = torch.arange(qkv.shape[0])
    pos = torch.stack([r % 7, (r * 7) % n_pos, (r * 13 + 5) % n_pos], -1).to(torch.int16)
    cos, sin = rope_tables(n_pos, n_freq)
    wq, wk = rnd(128, dtype=F32, seed=1) + 1, rnd(128, dtype=F32, seed=2) + 1
    got = ref.qknorm_rope(qkv.clone(), heads, pos, 2, cos, sin, wq, wk, 1e-5)
    assert bool((got[which == 4][:, :2 * heads * 128] == 0).all())
    for k, name in enumerate(ROW_KINDS):
        assert le.check_qknorm_rope(got[which == k], qkv[which == k], heads, pos[which == k], 2, cos, sin, wq, wk, 1e-5,
                                    name=f"qknorm_rope rows {name}") <= 1.0


@pytest.mark.parametrize("kind", STORES, ids=["bf16", "h16", "fp32"])
@pytest.mark.parametrize("HW,C,groups", [((1, 2047), 128, 32), ((1, 2049), 256, 32), ((3, 1367), 512, 32), ((1, 4097), 128, 16),
                                         ((1, 2048), 128, 8), ((13, 17), 192, 32), ((9, 11), 320, 32), ((7, 5), 24, 3)])
def test_groupnorm_is_inside_its_bounds(HW, C, groups, kind):
    T = 2
    x = _st(rnd(T, *HW, C, scale=1.5, dtype=F32) + 0.7, torch.empty(0, dtype=kind))
    gamma, beta = rnd(C, dtype=F32, seed=1) + 1, rnd(C, dtype=F32, seed=2)
    stats = ref.groupnorm_stats(x, torch.empty(T, groups, 2, dtype=torch.float64), groups)
    if 256 % (C // 8) == 0:                                                        # (the C svr_groupnorm_stats accepts)
        assert le.check_groupnorm_stats(stats, x, groups) <= 1.0
        xg = _ld(x).reshape(T, -1, groups, C // groups)                            # fp32 sums, as the kernel's threads form them
        f32 = torch.stack([xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))], -1)
        assert le.check_groupnorm_stats(f32.double(), x, groups, name="groupnorm_stats fp32 sums") <= 1.0
    for silu in (True, False):
        out = ref.groupnorm_apply(x, torch.empty(T, *HW, C, dtype=BF16), stats, gamma, beta, groups, 1e-6, silu)
        assert le.check_groupnorm_apply(out, x, stats, gamma, beta, groups, 1e-6, silu) <= 1.0
        assert le.check_groupnorm_apply(out, x, stats, gamma, beta, groups, 1e-6, silu, slab_rows=1, name="slabs") <= 1.0


def stats_in_kernel_order(x, groups, acc=F32):
    """groupnorm_stats_kernel's summation order restated (csrc/svr_elementwise.hip): blocks of 2048 rows; thread (row lane j,
    chunk c) of a block walks the rows r0 + j, r0 + j + rstep, ... (rstep = 256 / (C / 8)) and keeps, per 4-channel quad, a
    running sum  s += ((f0 + f1) + f2) + f3  and  q += ((f0 f0 + f1 f1) + f2 f2) + f3 f3  in ``acc`` precision; everything behind
    the thread (row lanes, quads of a group, blocks) is added in fp64.  acc = fp32: the arithmetic of the kernel as it was;
    acc = fp64: the same order with fp64 accumulators.  -> stats [T, groups, 2] fp64."""
    T, H, W, C = x.shape
    HW, rstep = H * W, 256 // (C // 8)
    f = _ld(x).reshape(T, HW, C // 4, 4).to(acc)
    out = torch.zeros(T, C // 4, 2, dtype=torch.float64)
    for r0 in range(0, HW, le.GN_ROWS_PER_BLOCK):
        blk = f[:, r0:r0 + le.GN_ROWS_PER_BLOCK]
        pad = -blk.shape[1] % rstep
        blk = torch.nn.functional.pad(blk, (0, 0, 0, 0, 0, pad)).reshape(T, -1, rstep, C // 4, 4)        # [T, trip, row lane, quad, 4]
        s = torch.zeros(T, rstep, C // 4, dtype=acc)
        q = torch.zeros(T, rstep, C // 4, dtype=acc)
        for trip in range(blk.shape[1]):
            v = blk[:, trip]
            s = s + (((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])
            q = q + (((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) + v[..., 3] * v[..., 3])
        out += torch.stack([s.double().sum(1), q.double().sum(1)], -1)
    return out.reshape(T, groups, -1, 2).sum(2)


@pytest.mark.parametrize("kind", STORES, ids=["bf16", "h16", "fp32"])
@pytest.mark.parametrize("H,W", [(37, 41), (64, 64)])
def test_groupnorm_variance_check_rejects_fp32_stage_on_offset_data(H, W, kind):
    """check_groupnorm_variance on the statistics kernel's summation order, C = 128, 32 groups, x = std (rho + N(0, 1)):
    with the fp32 per-thread stage (up to 512 terms) the variance E[x^2] - mean^2 is inside 2^-9 (var + eps) up to rho = 16 and
    OUTSIDE it at rho = 256 and 1024 (the checker sees what the sums-relative bound of check_groupnorm_stats accepts -- that one
    passes throughout); with fp64 accumulators in the same order it is inside at every rho.  What survives is therefore decided
    by the accumulator format alone, not by the reference arithmetic."""
    T, C, G = 2, 128, 32
    for std in (1.0, 2.0 ** -6):
        for rho in (0.5, 16.0, 256.0, 1024.0):
            x = offset_groups(T, H, W, C, G, rho, std, kind)
            tag = f"rho {rho} std {std}"
            wide = stats_in_kernel_order(x, G, torch.float64)
            assert le.check_groupnorm_variance(wide, x, G, 1e-6, name=f"fp64 accumulators {tag}") <= 1.0
            narrow = stats_in_kernel_order(x, G, F32)
            assert le.check_groupnorm_stats(narrow, x, G, name=f"fp32 stage, sums {tag}") <= 1.0
            if rho <= 16:
                assert le.check_groupnorm_variance(narrow, x, G, 1e-6, name=f"fp32 stage {tag}") <= 1.0
            else:
                with pytest.raises(AssertionError, match="rho = ") as e:
                    le.check_groupnorm_variance(narrow, x, G, 1e-6, name=f"fp32 stage {tag}")
                assert "two-pass variance" in str(e.value) and "group" in str(e.value)


@pytest.mark.parametrize("kind", STORES, ids=["bf16", "h16", "fp32"])
def test_groupnorm_composed_reference_on_offset_and_constant_groups(kind):
    """groupnorm_reference (two-pass statistics) accepts the fp32 restatement of the apply pass fed with exact fp64 sums, at
    every rho, and rejects it when fed with the fp32-stage statistics at rho = 1024; groups constant at 0 / 1000 / -3e5 have
    variance 0 exactly and normalise to act(beta)."""
    T, H, W, C, G = 2, 37, 41, 128, 32
    gamma, beta = rnd(C, dtype=F32, seed=1) + 1, rnd(C, dtype=F32, seed=2)
    for rho in (0.5, 16.0, 256.0, 1024.0):
        x = offset_groups(T, H, W, C, G, rho, 1.0, kind)
        stats = ref.groupnorm_stats(x, torch.empty(T, G, 2, dtype=torch.float64), G)
        assert le.check_groupnorm_variance(stats, x, G, 1e-6) <= 1.0
        for silu in (True, False):
            out = ref.groupnorm_apply(x, torch.empty(T, H, W, C, dtype=BF16), stats, gamma, beta, G, 1e-6, silu)
            assert le.check_groupnorm(out, x, gamma, beta, G, 1e-6, silu) <= 1.0
    bad = stats_in_kernel_order(x, G, F32)                                         # rho = 1024
    out = ref.groupnorm_apply(x, torch.empty(T, H, W, C, dtype=BF16), bad, gamma, beta, G, 1e-6, False)
    le.check_groupnorm_apply(out, x, bad, gamma, beta, G, 1e-6, False)            # the reference from the given statistics cannot see it
    must_fail(lambda: le.check_groupnorm(out, x, gamma, beta, G, 1e-6, False))
    x = offset_groups(T, H, W, C, G, 0.5, 1.0, F32)
    for g, v in ((3, 0.0), (4, 1000.0), (17, -3e5)):
        x[:, :, :, g * 4:g * 4 + 4] = v
    x = _st(x, torch.empty(0, dtype=kind))
    stats = ref.groupnorm_stats(x, torch.empty(T, G, 2, dtype=torch.float64), G)
    assert le.check_groupnorm_variance(stats, x, G, 1e-6) <= 1.0
    mean, var = le.two_pass_moments(x, G)
    assert bool((var[:, [3, 4, 17]] == 0).all())
    for silu in (True, False):
        want, _ = le.groupnorm_reference(x, gamma, beta, G, 1e-6, silu)
        b = beta.double()
        for g in (3, 4, 17):
            act_b = (torch.nn.functional.silu(b) if silu else b)[g * 4:g * 4 + 4].expand(T, H, W, 4)
            assert torch.allclose(want[..., g * 4:g * 4 + 4], act_b, rtol=1e-14 if silu else 0.0, atol=0.0)
        out = ref.groupnorm_apply(x, torch.empty(T, H, W, C, dtype=BF16), stats, gamma, beta, G, 1e-6, silu)
        assert le.check_groupnorm(out, x, gamma, beta, G, 1e-6, silu) <= 1.0


@pytest.mark.parametrize("cols", [4, 260, 16384, 16388])
def test_softmax_rows_is_inside_its_bounds(cols):
    S = torch.randn(6, cols, generator=torch.Generator().manual_seed(cols)) * 30.0
    S[1, -1] = 400.0                                                               # the maximum is the last element
    S[2] = 3.25                                                                    # a row of equal values
    P = ref.softmax_rows(S, torch.empty(6, cols, dtype=BF16), 0.044)
    assert le.check_softmax_rows(P, S, 0.044) <= 1.0


@pytest.mark.parametrize("cols", [64, 16388])
def test_softmax_rows_is_inside_its_bounds_on_wide_score_ranges(cols):
    scale = 0.044
    S = torch.randn(5, cols, generator=torch.Generator().manual_seed(cols)) * 30.0
    S[0] = torch.linspace(-1e4, 1e4, cols) / scale                                # scaled scores span +-1e4
    S[1], S[2] = 1e4 / scale, -1e4 / scale                                         # rows of equal scores
    S[3, -1] = 1e4 / scale                                                         # one dominant score in the last column
    P = ref.softmax_rows(S, torch.empty(5, cols, dtype=BF16), scale)
    assert le.check_softmax_rows(P, S, scale) <= 1.0


@pytest.mark.parametrize("out_dt", STORES, ids=["bf16", "h16", "fp32"])
def test_activation_sweep_restatement_is_inside_its_bounds(out_dt):
    """The zero-operand activation launches of tests/test_gpu_conditioning.py, restated: A = 0, bias = the activation sweep.  The
    fp32 restatement is inside check_gemm's bound with the 2^-126 absolute term wherever the exact result fits the output format;
    a restatement that flushes results in fp32's denormal range is inside it too -- and outside it without the term."""
    M, N, K = 5, 256, 64
    A, W = torch.zeros(M, K, dtype=BF16), rnd(N, K, seed=1)
    bias = act_sweep().repeat(N // 32)
    for epi in (EPI_BIAS_SILU, EPI_BIAS_GELU):
        kw = dict(N=N, K=K, bias=bias, epilogue=epi)
        out = ref.gemm(A, W, torch.empty(M, N, dtype=out_dt), **kw)
        want, bound, mask = le.gemm_reference(A, W, out, abs_err=2.0 ** -126, **kw)
        fits = want.abs() < (65504.0 * 64 * (1 - 2.0 ** -11) if out_dt == H16 else 3.3e38)
        assert not bool(torch.isnan(_ld(out)).any())
        assert le.check(f"epilogue {epi}", out, want, bound, mask & fits) <= 1.0
        if out_dt == F32:
            flushed = torch.where(out.abs() < 2.0 ** -126, torch.zeros_like(out), out)
            assert not torch.equal(flushed, out)
            assert le.check(f"epilogue {epi}, flushed", flushed, want, bound, mask & fits) <= 1.0
            want, bound, mask = le.gemm_reference(A, W, out, **kw)
            must_fail(lambda: le.check(f"epilogue {epi}, flushed, no absolute term", flushed, want, bound, mask & fits))


def test_rows_mean_and_unpatchify_are_inside_their_bounds():
    for n_groups, dim in ((7, 2560), (1, 520)):
        src = rnd(n_groups * 58, dim)
        dst = ref.rows_mean(src, torch.empty(58, dim, dtype=BF16), n_groups, 58)
        le.check("rows_mean", dst, *le.rows_mean_reference(src, n_groups, 58))
    pred, x_t = rnd(3 * 4 * 6, 96), rnd(3, 8, 12, 16, seed=4)                      # a padded prediction: stride(0) > 4C
    for xt in (x_t, None):
        o = ref.unpatchify_euler(pred, xt, torch.empty(3, 8, 12, 16, dtype=BF16))
        le.check("unpatchify_euler", o, *le.unpatchify_euler_reference(pred, xt, o.shape))


# ------------------------------------------------------------------------------------------------ fault injection
def test_fault_fragment_from_the_row_above():
    """One 16-byte store (8 bf16) of the last row holds the row above's values: 8 of 768 000 elements."""
    M, N, K = 1000, 768, 256
    A, W, bias = rnd(M, K), rnd(N, K, scale=1.0 / math.sqrt(K), seed=1), rnd(N, dtype=F32, seed=3)
    out = ref.gemm(A, W, torch.empty(M, N, dtype=BF16), N=N, K=K, bias=bias)
    want32 = ref.gemm(A, W, torch.empty(M, N), N=N, K=K, bias=bias)
    le.check_gemm(out, A, W, N=N, K=K, bias=bias)
    out[M - 1, N - 8:] = out[M - 2, N - 8:]
    assert rel_err(out.float(), want32) < TOL_BF16                                 # the global metric does not see it
    msg = must_fail(lambda: le.check_gemm(out, A, W, N=N, K=K, bias=bias))
    assert "in 1 rows" in msg and f"row {M - 1} " in msg


def test_fault_one_row_scaled():
    """One row 3 % too large (a stale 1 / rms): worst row error 3e-2 against 1.7e-3 clean, global metric 1.9e-3."""
    rows, dim = 1000, 2560
    x = rnd(rows, dim, scale=2.0)
    sc, sh = rnd(dim, dtype=F32, seed=2), rnd(dim, dtype=F32, seed=3)
    out = ref.rmsnorm_mod(x, torch.empty(rows, dim, dtype=BF16), 1e-5, scale=sc)
    want32 = ref.rmsnorm_mod(x, torch.empty(rows, dim), 1e-5, scale=sc)
    le.check_rmsnorm_mod(out, x, 1e-5, scale=sc)
    out[617] = (out[617].float() * 1.03).to(BF16)
    assert rel_err(out.float(), want32) < TOL_BF16
    msg = must_fail(lambda: le.check_rmsnorm_mod(out, x, 1e-5, scale=sc))
    assert "in 1 rows" in msg and "row 617 " in msg


def test_fault_two_rows_swapped():
    """Two rows of a row-normalised output exchanged (a wave serving the wrong slot of its pipeline).  RMSNorm removes a row's
    magnitude, so the two rows are made alike up to 2 % noise and a factor 1.5: after the norm they differ by 2 % per element -- five
    times the bf16 rounding, and still invisible in the global metric."""
    rows, dim = 1000, 2560
    x = rnd(rows, dim, scale=2.0, dtype=F32)
    x[401] = 1.5 * x[400] + 0.02 * 2.0 * rnd(dim, dtype=F32, seed=5)
    x = x.to(BF16)
    out = ref.rmsnorm_mod(x, torch.empty(rows, dim, dtype=BF16), 1e-5)
    want32 = ref.rmsnorm_mod(x, torch.empty(rows, dim), 1e-5)
    le.check_rmsnorm_mod(out, x, 1e-5)
    out[[400, 401]] = out[[401, 400]]
    assert rel_err(out.float(), want32) < TOL_BF16
    msg = must_fail(lambda: le.check_rmsnorm_mod(out, x, 1e-5))
    assert "in 2 rows" in msg


def test_fault_corner_voxel_missing_one_tap():
    """The corner voxel (0, 0, 0) of a 3x3x3 conv output lacks its centre tap in all 128 channels (a halo predicate off by one)."""
    case = (128, 128, (3, 3, 3), (1, 1, 1), (1, 1), 3, 32, 80, 0)
    x, w5, Wp, kw, shape = conv_problem(case)
    want32 = ref.gemm(x, Wp, torch.empty(shape), **kw)
    out = want32.to(BF16)
    le.check_gemm(out, x, Wp, **kw)
    faulty = want32.clone()
    faulty[0, 0, 0] -= x[0, 0, 0].float() @ w5[:, :, 2, 1, 1].float().t()
    out = faulty.to(BF16)
    assert rel_err(out.float(), want32) < TOL_BF16
    msg = must_fail(lambda: le.check_gemm(out, x, Wp, **kw))
    assert "in 1 rows" in msg and "row 0 " in msg


def test_fault_groupnorm_sum_missing_one_block():
    """One group's sums lack the contribution of one 2048-row block of 128 (a partial that was never added).  The statistics check
    sees it; so does the apply output per element, while the global metric of the apply output -- all that sees fused statistics
    that are only ever consumed -- stays under its limit."""
    T, H, W, C, G = 1, 128, 2048, 32, 8
    x = (rnd(T, H, W, C, scale=1.5, dtype=F32) + 0.1).to(BF16)
    gamma, beta = rnd(C, dtype=F32, seed=1) + 1, rnd(C, dtype=F32, seed=2)
    stats = ref.groupnorm_stats(x, torch.empty(T, G, 2, dtype=torch.float64), G)
    le.check_groupnorm_stats(stats, x, G)
    blk = x[:, 17].double().reshape(T, W, G, C // G)                               # block 17 = rows 17 * 2048 ..
    bad = stats.clone()
    bad[:, 5, 0] -= blk[:, :, 5].sum(dim=(1, 2))
    bad[:, 5, 1] -= blk[:, :, 5].pow(2).sum(dim=(1, 2))
    must_fail(lambda: le.check_groupnorm_stats(bad, x, G))
    want32 = ref.groupnorm_apply(x, torch.empty(T, H, W, C), stats, gamma, beta, G, 1e-6, False)
    out = ref.groupnorm_apply(x, torch.empty(T, H, W, C, dtype=BF16), bad, gamma, beta, G, 1e-6, False)
    assert rel_err(out.float(), want32) < TOL_BF16
    must_fail(lambda: le.check_groupnorm_apply(out, x, stats, gamma, beta, G, 1e-6, False))


def test_fault_attention_row_without_its_last_key_tile():
    """One query row of one head computed over the first 576 of its 640 keys (the last 64-key tile skipped)."""
    heads, D, L = 16, 128, 640
    qkv = rnd(2 * L, 3 * heads * D)
    rows = torch.arange(2 * L, dtype=torch.int32)
    cu = torch.tensor([0, L, 2 * L], dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    want32 = ref.attn_varlen(qkv, torch.zeros(2 * L, heads * D), rows, rows, cu, L, heads, D, scale)
    out = want32.to(BF16)
    le.check_attn(out, qkv, rows, rows, cu, heads, D, scale)
    q3 = qkv.float().reshape(2 * L, 3, heads, D)
    r, h = L + 321, 9
    p = torch.softmax((q3[r, 0, h] @ q3[L:2 * L - 64, 1, h].t()) * scale, dim=-1)
    out[r, h * D:(h + 1) * D] = (p @ q3[L:2 * L - 64, 2, h]).to(BF16)
    assert rel_err(out.float(), want32) < TOL_ATTN
    msg = must_fail(lambda: le.check_attn(out, qkv, rows, rows, cu, heads, D, scale))
    assert "in 1 rows" in msg and f"row {r} " in msg


def test_fault_attention_ragged_tile_unmasked_in_one_query_block():
    """hot_gauss (scores of +-100 log2 units, near one-hot rows), L = 259: ONE 32-query block -- one wave of the window kernel, rows
    160 .. 191 -- computes its last tile without the -inf mask, so the 61 clamped copies of key 258 count.  Only a row that gives that
    key some weight moves at all, and only a little: the global metric stays at 1.4e-3 of its 4e-3 while one row leaves its bound.
    (With the fault in every block no steered case stays under the global limit: the smallest figure is 2e-2, hot_gauss.)"""
    q, k, v, scale, ref3 = score_problem("win", "hot_gauss")
    out, bad = emulate("win", "hot_gauss"), emulate("win", "hot_gauss", "nomask")
    le.check("attention hot_gauss", out, *ref3)
    out[160:192] = bad[160:192]
    assert rel_err(out.float(), ref3[0]) < TOL_ATTN
    msg = must_fail(lambda: le.check("attention hot_gauss, one block unmasked", out, *ref3))
    assert "in 1 rows" in msg


# ------------------------------------------------------------------------------------------------ the engines' glue kernels
def next_bf16(t):
    """the neighbouring bf16 value (one unit in the last place away)"""
    return (t.view(torch.int16) + 1).view(BF16)


def test_ada_combine_is_inside_its_bounds_and_one_element_is_not():
    dim, n_vec = 2560, 14
    emb, params = rnd(dim * 6, scale=2.0), rnd(n_vec, dim, seed=1)
    slots = torch.tensor([v % 6 for v in range(n_vec)], dtype=torch.int32)
    out = ref.ada_combine(emb, params, slots, torch.empty(n_vec, dim))
    assert le.check_ada_combine(out, emb, params, slots) <= 1.0
    clean = out.clone()
    out[9, 1303] *= 1.0 + 2.0 ** -18                                               # 64 fp32 ulps on one element
    assert rel_err(out, clean) < TOL_BF16
    msg = must_fail(lambda: le.check_ada_combine(out, emb, params, slots))
    assert "1 of" in msg and "row 9 " in msg
    out = clean.clone()
    out[5] = clean[4]                                                              # a vector read through its neighbour's slot
    assert "in 1 rows" in must_fail(lambda: le.check_ada_combine(out, emb, params, slots))


def test_data_movement_is_checked_bit_for_bit():
    """patchify and im2col_causal: no arithmetic, so the bound is zero -- on the bit patterns.  One element one bf16 step off, or a
    pad column holding -0.0, passes the global metric (the second is invisible to ANY comparison of values)."""
    ops = sub("ops")
    vid = rnd(3, 8, 12, 33)
    out = ref.patchify(vid, torch.empty(3 * 4 * 6, 192, dtype=BF16))
    want = le.patchify_reference(vid, out)
    assert le.check_bits("patchify", out, want) == 0.0 and bool((want[:, 132:] == 0).all())
    one_off = out.clone()
    one_off[40, 77:78] = next_bf16(out[40, 77:78])
    assert rel_err(one_off.float(), want.float()) < TOL_BF16
    with pytest.raises(AssertionError, match="1 of .* row 40 .* column 77 "):
        le.check_bits("patchify", one_off, want)
    pad = out.clone()
    pad[71, 191] = -0.0
    assert rel_err(pad.float(), want.float()) == 0.0 and torch.equal(pad, want)    # (value comparisons: all blind)
    with pytest.raises(AssertionError, match="row 71 .* column 191 "):
        le.check_bits("patchify", pad, want)
    for T, hf, stride in ((3, 0, (1, 1, 1)), (1, 2, (1, 1, 1)), (4, 1, (2, 2, 2))):
        H, W, Cin, k = 6, 10, 16, (3, 3, 3)
        x, halo = rnd(T, H, W, Cin), (rnd(hf, H, W, Cin, seed=9) if hf else None)
        pt = hf if hf else 2
        plo, phi = (1, 1) if stride == (1, 1, 1) else (0, 1)
        To, Ho, Wo = (T + pt - 3) // stride[0] + 1, (H + plo + phi - 3) // stride[1] + 1, (W + plo + phi - 3) // stride[2] + 1
        geom = ops.Conv3dGeom(T, H, W, Cin, To, Ho, Wo, k, stride, (pt, plo, plo), halo)
        cols = ref.im2col_causal(x, torch.empty(To * Ho * Wo, 448, dtype=BF16), geom)
        want = le.im2col_causal_reference(x, cols, geom)
        assert le.check_bits("im2col_causal", cols, want) == 0.0 and bool((want[:, 432:] == 0).all())
        # the rows ARE the conv's operand: a GEMM over them is the conv (the index map is the one gemm_reference uses)
        w5, Wp = conv_weight(64, Cin, k)
        Wpad = torch.cat([Wp, torch.zeros(64, 16, dtype=BF16)], 1)
        assert rel_err(cols.double() @ Wpad.double().t(), le.gemm_reference(x, Wp, torch.empty(To, Ho, Wo, 64, dtype=F32), N=64, K=432,
                                                                             conv=geom)[0].reshape(-1, 64)) < 1e-12
        tap = cols.clone()
        tap[To * Ho * Wo - 1, 16:32] = cols[To * Ho * Wo - 2, 16:32]               # one tap's 32 bytes from the voxel before
        with pytest.raises(AssertionError, match=f"row {To * Ho * Wo - 1} "):
            le.check_bits("im2col_causal", tap, want)


@pytest.mark.parametrize("case", CONVS)
def test_conv_by_taps_is_the_fp64_conv(case):
    """The tap-by-tap matmul form gemm_acc takes for the fp64 reference on a device == F.conv3d in fp64."""
    from ops_reference import conv_by_taps, conv_padded_input, gemm_acc
    x, w5, Wp, kw, shape = conv_problem(case)
    g = kw["conv"]
    got = conv_by_taps(conv_padded_input(x, g, torch.float64), Wp[:kw["N"]].double(), g, kw["N"])
    assert rel_err(got, gemm_acc(x, Wp, N=kw["N"], K=kw["K"], conv=g, dtype=torch.float64)) < 1e-13


def blend_problem(T=3, C=16, H=64, W=96, h=9, w=12, y0=7, x0=16):
    vae = sub("vae")
    tile = rnd(T, h, w, C, scale=0.5)
    acc, cnt = rnd(T, H, W, C, dtype=F32, seed=1), rnd(H, W, dtype=F32, seed=2).abs() + 0.5
    wy = vae._edge_weights(h, 4, True, False, vae._cos_ramp(4))
    wx = vae._edge_weights(w, 4, True, True, vae._cos_ramp(4))
    return tile, acc, cnt, wy, wx, y0, x0


def test_blend_accumulate_is_inside_its_bounds_and_local_faults_are_not():
    tile, acc0, cnt0, wy, wx, y0, x0 = blend_problem()
    acc, cnt = acc0.clone(), cnt0.clone()
    ref.blend_accumulate(tile, acc, cnt, wy, wx, y0, x0)
    args = (tile, acc0, cnt0, wy, wx, y0, x0)
    assert le.check_blend_accumulate(acc, cnt, *args) <= 1.0
    (wa, ba, ma), (wc, bc, mc) = le.blend_accumulate_reference(*args)
    assert int(ma.sum()) == tile.numel() and int(mc.sum()) == 9 * 12
    # one element of one voxel never received its tile: 1 of 294 912 elements
    bad = acc.clone()
    bad[1, y0 + 3, x0 + 5, 6] = acc0[1, y0 + 3, x0 + 5, 6]
    assert rel_err(bad, wa.where(ma, acc0.double())) < TOL_BF16
    msg = must_fail(lambda: le.check_blend_accumulate(bad, cnt, *args))
    assert "1 of" in msg and "in 1 rows" in msg
    # the weight counted once per FRAME instead of once per pixel
    cnt_T = cnt0.clone()
    cnt_T[y0:y0 + 9, x0:x0 + 12] += 3 * (wy[:, None] * wx[None, :])
    must_fail(lambda: le.check_blend_accumulate(acc, cnt_T, *args))
    # a tile one column too wide: the extra column is not the launch's own
    wide = acc.clone()
    wide[:, y0:y0 + 9, x0 - 1] += 1.0
    with pytest.raises(AssertionError, match="not its own"):
        le.check_blend_accumulate(wide, cnt, *args)


def test_blend_finalize_and_affine_slice_are_inside_their_bounds_and_local_faults_are_not():
    T, H, W, C, c_take = 3, 20, 28, 32, 16
    acc = rnd(T, H, W, C, dtype=F32, scale=3.0)
    cnt = rnd(H, W, dtype=F32, seed=2).abs() + 0.25
    cnt[3, 4] = 0.0                                                                # (never covered: the 1e-6 floor)
    for scale, shift in ((0.9152, 0.0), (1.0, 0.0), (1.0 / 0.9152, 0.3)):
        out = ref.blend_finalize(acc, cnt, torch.empty(T, H, W, c_take, dtype=BF16), scale, shift)
        assert le.check_blend_finalize(out, acc, cnt, scale, shift) <= 1.0
        want = le.blend_finalize_reference(acc, cnt, c_take, scale, shift)[0]
        bad = out.clone()
        bad[2, 11, 13, 8:16] = (out[2, 11, 13, 8:16].float() * 1.02).to(BF16)      # one 16-byte store 2 % off (its neighbour's weight sum)
        assert rel_err(bad.float(), want) < TOL_BF16
        msg = must_fail(lambda: le.check_blend_finalize(bad, acc, cnt, scale, shift))
        assert "in 1 rows" in msg
    inp = rnd(T, H, W, C, scale=2.0)
    for scale, shift in ((0.9152, 0.0), (1.0 / 0.9152, -0.0), (1.7, 0.3)):
        out = ref.affine_slice(inp, torch.empty(T, H, W, c_take, dtype=BF16), scale, shift)
        assert le.check_affine_slice(out, inp, scale, shift) <= 1.0
        want = le.affine_slice_reference(inp, c_take, scale, shift)[0]
        bad = out.clone()
        bad[1, 7, 9, :8] = (out[1, 7, 9, :8].float() * 1.02).to(BF16)              # one 16-byte store 2 % off (a stale scale)
        assert rel_err(bad.float(), want) < TOL_BF16
        assert "in 1 rows" in must_fail(lambda: le.check_affine_slice(bad, inp, scale, shift))
    # a scale applied in bf16 instead of fp32 (0.9152 -> 0.9141): every element 1.2e-3 off, under the 2.5e-3 of the global metric
    scale = 0.9152
    out = ref.affine_slice(inp, torch.empty(T, H, W, c_take, dtype=BF16), float(torch.tensor(scale).to(BF16)), 0.0)
    assert rel_err(out.float(), le.affine_slice_reference(inp, c_take, scale, 0.0)[0]) < TOL_BF16
    must_fail(lambda: le.check_affine_slice(out, inp, scale, 0.0))
