"""-m "not gpu": the geometry table of tests/geometry_cases.py, checked without a device.

  * Routing: every row, filled into svr_gemm_args from shape-only tensors, is served by the kernel class it names (the library's own
    routing function, as tests/test_cabi.py asks it); the table reaches every SVR_KERNEL_* class and every kernel instance, and
    every axis value meets every instance that can take it.
  * Reference: local_error.gemm_reference (fp64) on every conv row equals F.conv3d over the explicitly built causal head and zero
    padding -- the single-frame, two-tap and sub-halo-ring geometries are new for the reference too.
  * No false alarms: the checks the GPU sweep applies to a launch (bounds, bits of the voxels it does not own, guards, left-over
    poison), applied here to a correct implementation on the same data."""
import ctypes
import os
import shutil

import pytest
import torch
import torch.nn.functional as F

import geometry_cases as gc
import local_error as le
from conftest import sub, rel_err
from guarded_out import guarded
from ops_reference import TorchOps

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
ALL_ROWS = gc.CONV_ROWS + gc.GENERIC_CONV_ROWS
cpu_ops = TorchOps("cpu", act_dtype=torch.float32)


def _meta_frag(*args):
    W = args[1] if len(args) > 1 else args[0]
    return torch.empty(W.numel(), dtype=torch.bfloat16, device="meta")


class _Router:
    """svr_gemm_kernel_class on shape-only tensors, under a row's options (restored afterwards)"""

    def __init__(self):
        self.hip_lib, self.ops = sub("hip_lib"), sub("ops")
        self.hip_lib.build()
        self.L = self.hip_lib.lib()

    def cls(self, A, W, out, kw, options, gn=0):
        """-> kernel class; self.gn_blocks: partial blocks per output frame of the fused statistics (``gn`` groups)"""
        for k, v in {**gc.OPTION_DEFAULTS, **options}.items():
            assert self.L.svr_set_option(k.encode(), v) == 0, k
        try:
            a, _ = self.ops.fill_gemm_args(A, W, out, ptr=lambda t: 0x100000, zeros_ptr=0x100000, **kw)
            code = self.L.svr_gemm_kernel_class(ctypes.byref(a))
            a.gn_groups = gn
            self.gn_blocks = int(self.L.svr_gemm_gn_blocks(ctypes.byref(a))) if gn else None
            return self.hip_lib.KERNEL_CLASSES.get(code, "error: " + self.L.svr_last_error().decode())
        finally:
            for k, v in gc.OPTION_DEFAULTS.items():
                self.L.svr_set_option(k.encode(), v)


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_every_row_routes_to_the_kernel_class_it_names():
    """(SVR_KERNEL_GEMM_PERSISTENT depends on the CU count of the current device: without a device the library reads 256, the
    MI355X's count, so the 240- / 256-tile boundary rows are classified here as they are on the device.)"""
    r = _Router()
    packing = sub("packing")
    seen = set()
    for row in ALL_ROWS:
        inst = gc.INSTANCES.get(row.inst, dict(cls="conv_generic", options={}))
        p = gc.conv_problem(row, r.ops, packing, "meta", frag=_meta_frag)
        out = torch.empty(p.out_shape, dtype=p.out_dtype, device="meta")
        for ln in p.launches:
            got = r.cls(p.x, ln.W, out, ln.kw, inst["options"], gn=row.gn)
            assert got == inst["cls"], (gc.row_id(row), got)
            seen.add(got)
            if row.gn:          # the patch height of the instance that serves the row, as far as the library lets it be seen
                patches = -(-row.H // inst["patch_rows"]) * -(-row.W // 32)
                assert r.gn_blocks == (4 * patches if row.sub else patches), (gc.row_id(row), r.gn_blocks)
    for inst, H, W, bands in gc.BAND_CASES:
        p = gc.conv_problem(gc.band_row(inst, H, W), r.ops, packing, "meta", frag=_meta_frag)
        for band in bands:
            for ln in p.launches:
                got = r.cls(p.x, ln.W, torch.empty(p.out_shape, dtype=p.out_dtype, device="meta"), ln.kw,
                            {**gc.INSTANCES[inst]["options"], "conv_band": band})
                assert got == gc.INSTANCES[inst]["cls"], (inst, H, band, got)
    for case in gc.GEMM_CASES + [gc.EMPTY_GEMM]:
        A, W, kw, shape, dt = gc.gemm_problem(case, packing, "meta", frag=_meta_frag)
        got = r.cls(A, W, torch.empty(shape, dtype=dt, device="meta"), kw, {})
        assert got == case.cls, (gc.gemm_id(case), got)
        seen.add(got)
    assert seen == set(r.hip_lib.KERNEL_CLASSES.values()), sorted(set(r.hip_lib.KERNEL_CLASSES.values()) - seen)
    print("kernel classes reached:", sorted(seen))


def test_the_table_covers_every_instance_and_every_axis_value():
    rows = gc.CONV_ROWS
    assert 60 <= len(rows) <= 90
    assert len({gc.row_id(r) for r in rows}) == len(rows)
    assert {r.inst for r in rows} == set(gc.INSTANCES)
    assert all((r.H, r.W) in gc.HW and r.tk in gc.TK and r.H <= 48 and r.W <= 70 for r in rows)
    report = []
    for name, inst in gc.INSTANCES.items():
        mine = [r for r in rows if r.inst == name]
        axes = {
            "H x W": ({(r.H, r.W) for r in mine}, set(gc.HW)),
            "T / kt / pt / halo": ({r.tk for r in mine}, set(gc.TK)),
            "Cin": ({r.Cin for r in mine}, set(inst["cins"])),
            "N": ({r.N for r in mine}, set(inst["ns"])),
            "output kind": ({r.out for r in mine}, set(gc.OUT_KINDS)),
            "residual kind": ({r.resid for r in mine}, set(inst["resids"])),
        }
        if name in ("halo16_lds", "halo16_wreg8", "halo8_wreg4", "thin_in", "conv_sub"):      # the instances with fused statistics
            axes["gn_groups"] = ({r.gn for r in mine}, {0, 32})
        if name == "conv_sub":
            axes["launch form"] = ({r.sub[0] for r in mine}, {"phase", "quad"})
            axes["t_stride"] = ({r.sub[1] for r in mine}, {1, 2})
            axes["bias_border"] = ({r.sub[2] for r in mine}, {True, False})
            axes["launch form x fused statistics"] = ({(r.sub[0], r.gn) for r in mine}, {(f, n) for f in ("phase", "quad") for n in (0, 32)})
        for axis, (have, want) in axes.items():
            assert have >= want, (name, axis, sorted(want - have, key=str))
        report.append(f"{name}: {len(mine)} rows")
        for r in mine:
            kt = gc.TK[r.tk][1]
            assert (r.resid is not None) == (r.epi == "resid"), gc.row_id(r)
            assert not r.gn or (r.N // 32 in (4, 8, 16) and r.N % 32 == 0), gc.row_id(r)         # fused statistics exist for these N
            if name == "thinout4":
                assert gc.thinout4_serves(r.Cin, kt, r.N), gc.row_id(r)
            if name == "thinout32":
                assert not gc.thinout4_serves(r.Cin, kt, r.N), gc.row_id(r)
            assert (r.sub is not None) == (name == "conv_sub")
    # the 4-cout kernel's LDS rule really does turn some N <= 4 launches over to the 32-cout kernel, and the table holds one
    assert any(r.inst == "thinout32" and r.N <= 4 for r in rows)
    print("instances covered:", "; ".join(report))


_conv_cache = {}


def _conv3d_restatement(p, ln, phase):
    """What one (phase of a) launch computes, from F.conv3d on the explicitly built input: [To, H, W, N] fp64 before the store."""
    py, px, w5, bias, bb = phase
    g = ln.kw["conv"]
    T, H, W, Cin = g.T, g.H, g.W, g.Cin
    kt, pt = g.k[0], g.pad[0]
    x = p.x.double()
    head = p.halo.double()[-pt:] if p.halo is not None else x[:1].expand(pt, H, W, Cin)
    xin = torch.cat([head, x], 0) if pt else x
    xin = xin[..., :w5.shape[1]].permute(3, 0, 1, 2)[None]                         # (thin input: the three real channels)
    pads = (1, 1, 1, 1) if py is None else (1 - px, px, 1 - py, py)
    key = (H, W, T, kt, pt, p.halo is not None, Cin, w5.shape[0], ln.frame0, py, px, w5.shape[3])
    if key not in _conv_cache:                                                     # (rows that differ only in kernel instance,
        _conv_cache[key] = F.conv3d(F.pad(xin, pads), w5.double())[0].permute(1, 2, 3, 0)     # kinds or epilogue share the conv)
    y = _conv_cache[key]                                                           # [To, H, W, N]
    assert y.shape[0] == g.To
    b = bias.double().expand(g.To, H, W, -1).clone()
    if bb is not None:
        rb, cb = (H - 1 if py else 0), (W - 1 if px else 0)
        b[:, rb] = bb[0].double()
        b[:, :, cb] = bb[1].double()
        b[:, rb, cb] = bb[2].double()
    y = y + b
    if ln.kw.get("epilogue") == gc.EPI_BIAS_SILU:
        y = F.silu(y)
    elif ln.kw.get("epilogue") == gc.EPI_BIAS_GELU:
        y = F.gelu(y, approximate="tanh")
    if ln.kw.get("resid") is not None:
        y = y + le.values(ln.kw["resid"])
    return y


@pytest.mark.parametrize("row", ALL_ROWS, ids=[gc.row_id(r) for r in ALL_ROWS])
def test_fp64_reference_equals_conv3d_on_the_explicit_input(row):
    """The reference the GPU sweep compares against, on the row's own data -- and the sweep's own checks on a correct
    implementation (the fp32 restatement of tests/ops_reference.py, one rounding into the output's format, writing a guarded,
    poisoned buffer): no false alarm on any row, every launch leaves the voxels of the other launches bit-untouched, together they
    leave no poison."""
    opsmod, packing = sub("ops"), sub("packing")
    p = gc.conv_problem(row, opsmod, packing, "cpu", frag=lambda kind, W, kt, Cin, N: torch.empty(W.numel(), dtype=torch.bfloat16))
    g = guarded(p.out_shape, p.out_dtype, device="cpu")
    written = torch.zeros(p.out_shape, dtype=torch.bool)
    for ln in p.launches:
        view = g.t[ln.frame0:]
        want, bound, mask = le.gemm_reference(p.x, ln.W, view, **ln.kw)
        assert bool((bound[mask] > 0).all()) and bool(torch.isfinite(want[mask]).all())
        assert not bool((written[ln.frame0:] & mask).any())                        # no voxel belongs to two launches
        written[ln.frame0:] |= mask
        ts = row.sub[1] if row.sub else 1
        for phase in ln.phases:
            y = _conv3d_restatement(p, ln, phase)
            got = want if phase[0] is None else want[::ts, phase[0]::2, phase[1]::2]
            assert got.shape == y.shape
            assert rel_err(got, y) < 1e-12, (gc.row_id(row), phase[:2])
        before = g.t.clone()
        cpu_ops.gemm(p.x, ln.W, view, **ln.kw)
        assert le.check(gc.row_id(row), view, want, bound, mask, before[ln.frame0:]) <= 1.0
    assert bool(written.all())                                                      # together the launches own the whole output
    g.assert_written(gc.row_id(row))
    g.assert_guards(gc.row_id(row))
