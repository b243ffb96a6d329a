"""-m gpu: the lane maps of conv_halo2_kernel on v_mfma_f32_16x16x32_bf16 -- halo-row fragments as two 16-voxel halves, weight
fragments as two 16-cout halves (from the fragment-ordered copy and from the LDS ring), accumulators parked as four consecutive
couts of one voxel -- at the smallest shapes where each of them can go wrong:

  ragged     128 -> 128, 3x3x3, 2 x 17 x 33, a carried halo of two frames: two patch rows and two patch columns, the second of each
             ragged, so both 16-voxel halves meet an image edge
  one_n_tile 256 -> 128, 1x3x3, 2 x 9 x 31: one cout tile, eight channel slices
  three_n    128 -> 384, 3x3x3, 2 x 8 x 64: three cout tiles
  head       128 -> 128, 2x3x3, 1 x 16 x 32: one input frame (the causal head form)

Every case runs with bf16, h16 and fp32 outputs and a residual of each kind, fused GroupNorm statistics on.  Checked: every element
inside local_error.check_gemm's bound against the fp64 result; the statistics against an fp64 reduction of the stored tensor (the
measure of test_gpu_wide_trunk.py), for each of the three kernels; three launches bit-identical, statistics included; the outputs
of the LDS-weight kernel, 4 rows per wave and 8 rows per wave bit-identical to each other; guards and poison of every output buffer.

Statistics groups: 32, except where a group of Cout / 32 channels would straddle the kernel's 128-cout tiles (384 couts: 12 per
group) -- there the library declines 32 groups (asserted) and the case runs with groups of four channels."""
import math

import pytest
import torch

import local_error as le
from conftest import sub, rel_err
from guarded_out import Pool
from ops_reference import TorchOps, EPI_RESID_GATE, H16, H16_SCALE

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
WIDE = (F32, H16)
CONV_ROWS_DEFAULT = 8

CASES = {
    # Cin, Cout, kt, T, H, W, halo frames
    "ragged": (128, 128, 3, 2, 17, 33, 2),
    "one_n_tile": (256, 128, 1, 2, 9, 31, 0),
    "three_n": (128, 384, 3, 2, 8, 64, 0),
    "head": (128, 128, 2, 1, 16, 32, 0),
}
KINDS = [(BF16, BF16), (H16, H16), (F32, F32), (BF16, H16), (H16, F32), (F32, BF16)]
KIND_IDS = ["bf16_out_bf16_resid", "h16_out_h16_resid", "f32_out_f32_resid", "bf16_out_h16_resid", "h16_out_f32_resid",
            "f32_out_bf16_resid"]


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


@pytest.fixture(scope="module")
def ref():
    return TorchOps("cuda:0", act_dtype=torch.float32)


def rnd(*shape, scale=1.0, seed=0, dtype=BF16):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    v = torch.randn(*shape, generator=g, device="cuda") * scale
    return (v * H16_SCALE).to(H16) if dtype == H16 else v.to(dtype)      # (h16: the stored half is x * 2^-6)


_inputs = {}


def _case_inputs(hip, name):
    """operands of a case, made once and left unchanged: x, halo, packed weights, fragment-ordered weights, bias, geometry"""
    if name not in _inputs:
        packing, opsmod = sub("packing"), sub("ops")
        Cin, Cout, kt, T, H, W, hf = CASES[name]
        x = rnd(T, H, W, Cin)
        halo = rnd(hf, H, W, Cin, seed=9) if hf else None
        w5 = rnd(Cout, Cin, kt, 3, 3, scale=1.0 / math.sqrt(Cin * kt * 9), seed=2)
        Wp = packing.pack_conv3d(w5, "cuda")
        pt = hf if hf else kt - 1
        To = T + pt - kt + 1
        geom = opsmod.Conv3dGeom(T, H, W, Cin, To, H, W, (kt, 3, 3), (1, 1, 1), (pt, 1, 1), halo)
        _inputs[name] = (x, Wp, hip.pack_conv_frag(Wp, kt, Cin, Cout), rnd(Cout, dtype=F32, seed=3), geom, To)
    return _inputs[name]


@pytest.mark.parametrize("out_dt,res_dt", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_conv_halo_mfma16_lane_maps(hip, ref, name, out_dt, res_dt):
    Cin, Cout, kt, T, H, W, hf = CASES[name]
    x, Wp, Wf, bias, geom, To = _case_inputs(hip, name)
    resid = rnd(To, H, W, Cout, seed=11, dtype=res_dt)
    kw = dict(N=Cout, K=Wp.shape[1], bias=bias, conv=geom, ldc=Cout, ldr=Cout, resid=resid, epilogue=EPI_RESID_GATE)
    wide = out_dt in WIDE
    groups = 32
    gout = Pool()
    if 128 % (Cout // 32) != 0:
        _, none = hip.gemm(x, Wp, gout(To, H, W, Cout, dtype=out_dt), gn_groups=32, out_f32=wide, W_frag=Wf, **kw)
        assert none is None
        groups = Cout // 4
    outs, stats = {}, {}
    try:
        for mode, rows, frag in (("lds_weights", CONV_ROWS_DEFAULT, None), ("rows4", 4, Wf), ("rows8", 8, Wf)):
            hip.set_option("conv_rows", rows)
            for rep in range(3):
                out = gout(To, H, W, Cout, dtype=out_dt)
                got, st = hip.gemm(x, Wp, out, gn_groups=groups, out_f32=wide, W_frag=frag, **kw)
                assert got is out and st is not None and st.shape == (To, groups, 2)
                if rep == 0:
                    outs[mode], stats[mode] = out, st.clone()
                else:
                    assert torch.equal(out, outs[mode]), f"{mode}: launch {rep} differs from launch 0"
                    assert torch.equal(st, stats[mode]), f"{mode}: statistics of launch {rep} differ from launch 0"
    finally:
        hip.set_option("conv_rows", CONV_ROWS_DEFAULT)
    torch.cuda.synchronize()
    for mode in ("lds_weights", "rows4"):
        assert torch.equal(outs[mode], outs["rows8"]), f"{mode} and rows8 differ"
    out = outs["rows8"]
    le.check_gemm(out, x, Wp, name=f"conv mfma16 {name}", **kw)
    # (the three kernels add the same stored values in their own fixed orders -- other patch heights, other thread counts -- so
    # their fp64 sums of fp32 outputs may differ in the last bits: each is held to the reduction of the stored tensor instead)
    ws = ref.groupnorm_stats(out, torch.empty(To, groups, 2, device="cuda", dtype=torch.float64), groups)    # reference buffer
    for mode, st in stats.items():
        e0, e1 = rel_err(st[..., 0], ws[..., 0]), rel_err(st[..., 1], ws[..., 1])
        print(f"[mfma16] {name} {mode}: statistics rel err sum {e0:.3e} sumsq {e1:.3e}")
        assert e0 < 1e-5 and e1 < 1e-6, mode
    gout.check(f"conv mfma16 {name}")
