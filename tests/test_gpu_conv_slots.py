"""-m gpu: the K loop of the 8-row LDS-halo conv kernel (conv_halo2_kernel<16, 3>) with one MFMA slot per side operation -- every
halo-row read pair, weight load, halo-piece address and LDS-DMA issue behind four MFMAs of its own, counted waits unchanged -- at
the smallest shapes where a mis-counted wait or a read moved in front of its register's last MFMA can still go wrong:

  shortest loops   Cin = 64 with kt = 1, 2, 3: nA = 2, 4, 6 A steps, so the prologue, the last step's zero-page staging and the drain
                   are most of the loop; Cin = 128 with kt = 3 (nA = 12)
  geometries       T = 2 with 16 x 32 (exactly one patch) and 17 x 33 (four patches, three of them almost empty); Cout = 128, 256
  store kinds      a plain bf16 store, and an h16 store with an h16 residual and fused GroupNorm statistics

Per case: the 8-row kernel equals the 4-row kernel (conv_rows 4: the quarter-burst schedule it was derived from) and the LDS-ring
kernel (conv_impl 3) bit for bit, statistics included (sums of 16-bit stored values in fixed orders), and every element stays inside
local_error.check_gemm's bound.  That bound is taken against the fp64 result of the same conv (ops_reference.conv_by_taps: F.conv3d's
sums in another order); an fp32 F.conv3d lies inside the same bound of that fp64 result, so holding the kernel to the fp64 one asks
no less.  Race screen: T = 3, 64 x 96, 256 -> 256 and 64 -> 128, kt = 3 -- eight launches, each bit-identical to the first."""
import math

import pytest
import torch

import local_error as le
from conftest import sub
from guarded_out import Pool
from ops_reference import EPI_BIAS, EPI_RESID_GATE, H16
from test_gpu_conv_mfma16 import rnd

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
CONV_ROWS_DEFAULT, CONV_IMPL_DEFAULT = 8, 0

LOOPS = {"cin64_kt1": (64, 1), "cin64_kt2": (64, 2), "cin64_kt3": (64, 3), "cin128_kt3": (128, 3)}
GEOMS = {"one_patch": (2, 16, 32), "four_patches": (2, 17, 33)}
COUTS = (128, 256)
KINDS = {"bf16_plain": (BF16, None), "h16_resid_stats": (H16, H16)}
# (kernel, conv_rows, conv_impl): the kernel under test last, its two references first
KERNELS = (("lds_ring", CONV_ROWS_DEFAULT, 3), ("rows4", 4, 0), ("rows8", 8, 0))


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


_inputs = {}


def _operands(hip, Cin, Cout, kt, T, H, W):
    """operands of a shape, made once and left unchanged: x, packed weights, fragment-ordered weights, bias, geometry, To"""
    key = (Cin, Cout, kt, T, H, W)
    if key not in _inputs:
        packing, opsmod = sub("packing"), sub("ops")
        x = rnd(T, H, W, Cin)
        w5 = rnd(Cout, Cin, kt, 3, 3, scale=1.0 / math.sqrt(Cin * kt * 9), seed=2)
        Wp = packing.pack_conv3d(w5, "cuda")
        geom = opsmod.Conv3dGeom(T, H, W, Cin, T, H, W, (kt, 3, 3), (1, 1, 1), (kt - 1, 1, 1), None)
        Wf = hip.pack_conv_frag(Wp, kt, Cin, Cout)
        assert Wf is not None
        _inputs[key] = (x, Wp, Wf, rnd(Cout, dtype=F32, seed=3), geom, T)
    return _inputs[key]


def _launch(hip, gout, ops, kind, Cout, groups=32):
    """one launch of the case's conv under the options set by the caller -> (out, stats or None, keywords for the reference)"""
    x, Wp, Wf, bias, geom, To = ops
    out_dt, res_dt = KINDS[kind]
    kw = dict(N=Cout, K=Wp.shape[1], bias=bias, conv=geom, ldc=Cout)
    if res_dt is not None:
        kw.update(ldr=Cout, resid=rnd(To, geom.H, geom.W, Cout, seed=11, dtype=res_dt), epilogue=EPI_RESID_GATE)
    else:
        kw.update(epilogue=EPI_BIAS)
    out = gout(To, geom.H, geom.W, Cout, dtype=out_dt)
    if res_dt is None:
        got, st = hip.gemm(x, Wp, out, out_f32=False, W_frag=Wf, **kw), None
    else:
        got, st = hip.gemm(x, Wp, out, gn_groups=groups, out_f32=True, W_frag=Wf, **kw)
        assert st is not None and st.shape == (To, groups, 2)
    assert got is out
    return out, st, kw


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("loop", list(LOOPS))
def test_conv_slots_short_loops(hip, loop, geom, Cout, kind):
    (Cin, kt), (T, H, W) = LOOPS[loop], GEOMS[geom]
    ops = _operands(hip, Cin, Cout, kt, T, H, W)
    gout = Pool()
    outs, stats, kw = {}, {}, None
    try:
        for name, rows, impl in KERNELS:
            hip.set_option("conv_rows", rows)
            hip.set_option("conv_impl", impl)
            outs[name], stats[name], kw = _launch(hip, gout, ops, kind, Cout)
    finally:
        hip.set_option("conv_rows", CONV_ROWS_DEFAULT)
        hip.set_option("conv_impl", CONV_IMPL_DEFAULT)
    torch.cuda.synchronize()
    raw = torch.int16
    for name in ("lds_ring", "rows4"):
        diff = int((outs[name].view(raw) != outs["rows8"].view(raw)).sum())
        sdiff = 0 if stats[name] is None else int((stats[name].view(torch.int64) != stats["rows8"].view(torch.int64)).sum())
        print(f"[conv_slots] {loop} {geom} Cout {Cout} {kind}: rows8 vs {name}: {diff} output elements, {sdiff} statistics differ")
        assert diff == 0, f"rows8 and {name} differ in {diff} output elements"
        assert sdiff == 0, f"rows8 and {name} differ in {sdiff} statistics"
    le.check_gemm(outs["rows8"], ops[0], ops[1], name=f"conv slots {loop} {geom} {Cout} {kind}", **kw)
    gout.check(f"conv slots {loop} {geom} {Cout} {kind}")


@pytest.mark.parametrize("Cin,Cout", [(256, 256), (64, 128)], ids=["256_to_256", "64_to_128"])
def test_conv_slots_race_screen(hip, Cin, Cout):
    """eight launches in a row of the 8-row kernel (h16 store, h16 residual, fused statistics): each bit-identical to the first"""
    ops = _operands(hip, Cin, Cout, 3, 3, 64, 96)
    gout = Pool()
    first, first_st = None, None
    for rep in range(8):
        out, st, _ = _launch(hip, gout, ops, "h16_resid_stats", Cout)
        if rep == 0:
            first, first_st = out, st.clone()
        else:
            assert torch.equal(out.view(torch.int16), first.view(torch.int16)), f"launch {rep} differs from launch 0"
            assert torch.equal(st.view(torch.int64), first_st.view(torch.int64)), f"statistics of launch {rep} differ from launch 0"
    torch.cuda.synchronize()
    gout.check(f"conv slots race {Cin} -> {Cout}")
