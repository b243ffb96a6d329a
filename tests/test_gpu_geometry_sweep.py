"""-m gpu: the tile-edge geometries of tests/geometry_cases.py on the device.  Every launch writes a guarded, poisoned buffer
(tests/guarded_out.py): an element that is never stored stays NaN and fails its bound, a store outside the tensor fails the guards.

  * conv family: each row against the fp64 reference and the derived per-element bounds of tests/local_error.py, the kernel class the
    library reports for the launch, the guards, and -- where the row asks for them -- the fused GroupNorm statistics against those of
    the tensor that was stored.  Sub-pixel rows: every launch leaves the voxels of the other phases bit-untouched, together the
    launches leave no poison in the dense output.
  * conv_band: bit-identical outputs for every band height (the option permutes the tile order only).
  * plain GEMM: one K tile under 256 x 256 tiles, both sides of the 255 / 256-tile routing boundary, N % 8 != 0 (served by the
    direct epilogue, W padded to 128 rows -- not refused).
  * window attention: (window, head) pair counts of 1 and 7 modulo the 8 XCDs, an overstated max_len; attn_impl 1 under `variants`.

No tolerance of its own: value checks are local_error's bounds, containment and option invariance are bit comparisons.
Measured item times: profiles/geometry_sweep.txt."""
import contextlib
import math

import pytest
import torch

import geometry_cases as gc
import local_error as le
from conftest import sub
from guarded_out import guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ALL_ROWS = gc.CONV_ROWS + gc.GENERIC_CONV_ROWS


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


@contextlib.contextmanager
def options(hip, opts, record=True):
    """the row's library options and the kernel-class record, both put back afterwards"""
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        hip.record_kernel_class, hip.last_kernel_class = record, None
        yield
    finally:
        hip.record_kernel_class = False
        for k in opts:
            hip.set_option(k, gc.OPTION_DEFAULTS[k])


def conv_frag(hip):
    return lambda kind, W, kt, Cin, N: hip.pack_conv_frag(W, kt, Cin, N, taps=(3, 3) if kind == "conv33" else (2, 2))


def run_conv_row(hip, row, g, opts, cls, check=True):
    """The launches of ``row`` into the guarded buffer ``g`` -> fused statistics (or None).  ``check``: every launch against its
    bounds (and the elements it does not own against their bits before it)."""
    opsmod, packing = sub("ops"), sub("packing")
    p = gc.conv_problem(row, opsmod, packing, "cuda", frag=conv_frag(hip))
    assert tuple(g.t.shape) == p.out_shape and g.t.dtype == p.out_dtype
    stats = None
    shared = {"frames": p.out_shape[0]} if (row.gn and row.sub) else None
    with options(hip, opts):
        for i, ln in enumerate(p.launches):
            view = g.t[ln.frame0:]
            before = g.t.clone() if check else None
            if ln.kw.get("W_frag", 0) is None:
                raise AssertionError(f"{gc.row_id(row)}: no fragment-ordered weight copy for this geometry")
            if row.sub:
                if shared is not None:
                    shared["frame0"] = ln.frame0
                hip.gemm(p.x, ln.W, view, gn_groups=row.gn, gn_shared=shared, **ln.kw)
            elif row.gn:
                _, stats = hip.gemm(p.x, ln.W, view, gn_groups=row.gn, **ln.kw)
            else:
                hip.gemm(p.x, ln.W, view, **ln.kw)
            assert hip.last_kernel_class == cls, (gc.row_id(row), hip.last_kernel_class)
            g.assert_guards(f"{gc.row_id(row)} launch {i}")
            if check:
                le.check_gemm(view, p.x, ln.W, before=before[ln.frame0:], name=f"{gc.row_id(row)} launch {i}", **ln.kw)
        if shared is not None:
            stats = hip.gn_shared_stats(shared)
    return stats


@pytest.mark.parametrize("row", ALL_ROWS, ids=[gc.row_id(r) for r in ALL_ROWS])
def test_conv_geometry(hip, row):
    inst = gc.INSTANCES.get(row.inst, dict(cls="conv_generic", options={}))
    T, kt, pt, hf = gc.temporal(row.tk)
    ts = row.sub[1] if row.sub else 1
    shape = ((T + pt - kt + 1) * ts, 2 * row.H, 2 * row.W, row.N) if row.sub else (T + pt - kt + 1, row.H, row.W, row.N)
    g = guarded(shape, gc.STORE_KINDS[row.out])
    stats = run_conv_row(hip, row, g, inst["options"], inst["cls"])
    g.assert_written(gc.row_id(row))                     # (sub-pixel rows: the phases together own the dense output)
    if row.gn:
        assert stats is not None and tuple(stats.shape) == (shape[0], row.gn, 2), gc.row_id(row)
        le.check_groupnorm_stats(stats, g.t, row.gn, name=f"{gc.row_id(row)} fused statistics")


@pytest.mark.parametrize("inst,H,W,bands", gc.BAND_CASES, ids=[f"{c[0]}-H{c[1]}" for c in gc.BAND_CASES])
def test_conv_band_changes_the_tile_order_only(hip, inst, H, W, bands):
    row = gc.band_row(inst, H, W)
    T, kt, pt, _ = gc.temporal(row.tk)
    shape = (T + pt - kt + 1, 2 * H, 2 * W, row.N) if row.sub else (T + pt - kt + 1, H, W, row.N)
    outs = {}
    for band in bands:
        g = guarded(shape, BF16)
        run_conv_row(hip, row, g, {**gc.INSTANCES[inst]["options"], "conv_band": band}, gc.INSTANCES[inst]["cls"], check=band == 1)
        g.assert_written(f"{inst} H {H} conv_band {band}")
        outs[band] = g
    for band in bands:
        assert torch.equal(outs[band].t, outs[1].t), (inst, H, band)
        outs[band].assert_guards(f"{inst} H {H} conv_band {band}")


@pytest.mark.parametrize("case", gc.GEMM_CASES, ids=[gc.gemm_id(c) for c in gc.GEMM_CASES])
def test_gemm_geometry(hip, case):
    A, W, kw, shape, dt = gc.gemm_problem(case, sub("packing"), "cuda", frag=hip.pack_gemm_frag)
    assert not case.frag or kw["W_frag"] is not None
    g = guarded(shape, dt)
    with options(hip, {}):
        hip.gemm(A, W, g.t, **kw)
        assert hip.last_kernel_class == case.cls, hip.last_kernel_class
    g.assert_guards(gc.gemm_id(case))
    le.check_gemm(g.t, A, W, name=gc.gemm_id(case), **kw)


def test_empty_gemm_launches_nothing(hip):
    """M = 0: SVR_KERNEL_NONE -- the call succeeds and the output keeps its bits."""
    A, W, kw, shape, dt = gc.gemm_problem(gc.EMPTY_GEMM, sub("packing"), "cuda")
    g = guarded(shape, dt)
    with options(hip, {}):
        hip.gemm(A, W, g.t, **kw)
        assert hip.last_kernel_class == "none"
    torch.cuda.synchronize()
    g.assert_guards("empty GEMM")
    assert bool(g.poisoned().all())


@pytest.mark.parametrize("attn_impl", [0, pytest.param(1, marks=pytest.mark.variants)], ids=["attn_win", "attn_gen1"])
@pytest.mark.parametrize("name,lens,heads,max_len", gc.ATTN_CASES, ids=[c[0] for c in gc.ATTN_CASES])
def test_attn_geometry(hip, attn_impl, name, lens, heads, max_len):
    D, n_rows = 128, 400
    gen = torch.Generator().manual_seed(len(lens) + heads)
    qkv = torch.randn(n_rows, 3 * heads * D, generator=gen).to(BF16).cuda()
    total = sum(lens)
    seq_rows = torch.cat([torch.randint(0, n_rows, (L,), generator=gen) for L in lens]).to(torch.int32).cuda()
    out_rows = torch.arange(total, dtype=torch.int32).cuda()
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32).cuda()
    scale = 1.0 / math.sqrt(D)
    g = guarded((total, heads * D), BF16)
    with options(hip, {"attn_impl": attn_impl}, record=False):
        hip.attn_varlen(qkv, g.t, seq_rows, out_rows, cu, max_len or max(lens), heads, D, scale)
    g.assert_guards(name)
    le.check_attn(g.t, qkv, seq_rows, out_rows, cu, heads, D, scale, name=f"attn {name}")
