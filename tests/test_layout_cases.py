"""-m "not gpu": the layout table of tests/layout_cases.py against the library's host rules, without a device.

  * Every accepted GEMM / conv row, filled into svr_gemm_args through ops.fill_gemm_args from shape-only windows with fake
    pointers at the row's alignment, is served by the kernel class the row names (svr_gemm_kernel_class: the library's own routing
    function) -- and its dense twin, under the twin's options, by the same class.
  * Every refused row returns -1 with a message that names the operand.  Nothing is launched: a refusal happens before any launch,
    and the accepted rows of the other entry points are asked with empty shapes (rows = 0 / n_seq = 0), which validate the layout
    and return.
  * The table itself: every pitch of an accepted row covers its extent, every window lies inside its canvas, the groups (a), (b),
    (c) of the issue are all there for every GEMM shape that has them."""
import ctypes
import os
import shutil

import pytest
import torch

import geometry_cases as gc
import layout_cases as lc
from conftest import sub

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
FAKE = 0x10000000            # a 256-byte aligned fake device address


def _meta_frag(*args):
    W = args[1] if len(args) > 1 else args[0]
    return torch.empty(W.numel(), dtype=torch.bfloat16, device="meta")


def _win(rows, n, place, dtype):
    flat = torch.empty(lc.flat_elems(rows, n, place, dtype), dtype=dtype, device="meta")
    return lc.window(flat, rows, n, place)[1]


@pytest.fixture(scope="module")
def router():
    hip_lib, ops = sub("hip_lib"), sub("ops")
    hip_lib.build()
    L = hip_lib.lib()

    class Router:
        def cls(self, A, W, out, kw, options, ptr=lc.fake_ptr, zeros_ptr=FAKE):
            """-> (class name or "refused", message)"""
            for k, v in {**gc.OPTION_DEFAULTS, **options}.items():
                assert L.svr_set_option(k.encode(), v) == 0, k
            try:
                a, _ = ops.fill_gemm_args(A, W, out, ptr=ptr, zeros_ptr=zeros_ptr, **kw)
                code = int(L.svr_gemm_kernel_class(ctypes.byref(a)))
                return ("refused", L.svr_last_error().decode()) if code == -1 else (hip_lib.KERNEL_CLASSES[code], "")
            finally:
                for k, v in gc.OPTION_DEFAULTS.items():
                    L.svr_set_option(k.encode(), v)

    r = Router()
    r.L, r.ops, r.packing = L, ops, sub("packing")
    return r


def _gemm_windows(r, row):
    """(A window, W, C window, keywords with the residual window) of a GEMM row on shape-only tensors"""
    A, W, kw = lc.gemm_operands(row, r.packing, "meta", frag=_meta_frag)
    Aw = _win(row.M, row.K, row.A, lc.BF16)
    Cw = _win(row.M, lc.out_cols(row), row.C, lc.STORE_KINDS[row.out])
    kw = dict(kw)
    if row.resid == "inplace":
        assert row.R == row.C
        kw["resid"] = Cw
    elif row.resid:
        kw["resid"] = _win(row.M, row.N, row.R, lc.STORE_KINDS[row.resid])
    return A, Aw, W, Cw, kw


@needs_hipcc
@pytest.mark.parametrize("row", lc.GEMM_ROWS, ids=[lc.gemm_id(r) for r in lc.GEMM_ROWS])
def test_gemm_row_routes_to_its_class(router, row):
    A, Aw, W, Cw, kw = _gemm_windows(router, row)
    got, msg = router.cls(Aw, W, Cw, kw, {})
    assert got == row.cls, (lc.gemm_id(row), got, msg)
    # the dense twin the GPU sweep compares bits with: the same class under gemm_w4 = 0 where the row left the persistent kernel
    dense_kw = lc.gemm_operands(row, router.packing, "meta", frag=_meta_frag)[2]
    dense = torch.empty(row.M, lc.out_cols(row), dtype=lc.STORE_KINDS[row.out], device="meta")
    got_dense, _ = router.cls(A, W, dense, dense_kw, {} if row.cls == "gemm_persistent" else {"gemm_w4": 0})
    assert got_dense == row.cls, (lc.gemm_id(row), got_dense)
    if row.tag.startswith("b-"):          # (b): the persistent kernel is ineligible -- the dense launch of the big shape is its
        assert router.cls(A, W, dense, dense_kw, {})[0] == ("gemm_persistent" if (row.M, row.N, row.K) == lc.S_PERS else "gemm")


@needs_hipcc
@pytest.mark.parametrize("row,named", lc.GEMM_REFUSED, ids=[r.tag for r, _ in lc.GEMM_REFUSED])
def test_gemm_refused_row_names_its_operand(router, row, named):
    A, Aw, W, Cw, kw = _gemm_windows(router, row)
    ptr = lc.fake_ptr
    if row.tag == lc.W_OFF:
        ptr = lambda t: lc.fake_ptr(t) + (8 if t is W else 0)
    got, msg = router.cls(Aw, W, Cw, kw, {}, ptr=ptr)
    assert got == "refused" and named in msg, (row.tag, got, msg)
    # ... and svr_gemm_bf16 itself refuses it before any launch (no device here: a launch would fail differently)
    a, _ = router.ops.fill_gemm_args(Aw, W, Cw, ptr=ptr, zeros_ptr=FAKE, **kw)
    assert router.L.svr_gemm_bf16(ctypes.byref(a), None) == -1 and named in router.L.svr_last_error().decode()


def _conv_windows(r, c):
    p, ln = lc.conv_launch(c, r.ops, r.packing, "meta", frag=_meta_frag)
    M, N = p.out_shape[0] * p.out_shape[1] * p.out_shape[2], p.out_shape[3]
    kw = {k: v for k, v in ln.kw.items() if k not in ("ldc", "ldr")}
    Cw = _win(M, N, c.C, p.out_dtype)
    if c.R is not None:
        kw["resid"] = _win(M, N, c.R, ln.kw["resid"].dtype)
    return p, ln, Cw, kw


@needs_hipcc
@pytest.mark.parametrize("c", lc.CONV_ROWS, ids=[lc.conv_id(c) for c in lc.CONV_ROWS])
def test_conv_row_routes_to_its_class(router, c):
    p, ln, Cw, kw = _conv_windows(router, c)
    got, msg = router.cls(p.x, ln.W, Cw, kw, c.options)
    assert got == c.cls, (lc.conv_id(c), got, msg)
    dense = torch.empty(p.out_shape, dtype=p.out_dtype, device="meta")
    assert router.cls(p.x, ln.W, dense, ln.kw, c.twin_options)[0] == c.cls, lc.conv_id(c)
    if c.row.gn:                          # the strided launch produces the fused statistics of the dense one
        a, _ = router.ops.fill_gemm_args(p.x, ln.W, Cw, ptr=lc.fake_ptr, zeros_ptr=FAKE, **kw)
        d, _ = router.ops.fill_gemm_args(p.x, ln.W, dense, ptr=lc.fake_ptr, zeros_ptr=FAKE, **ln.kw)
        a.gn_groups = d.gn_groups = c.row.gn
        for k, v in c.options.items():
            router.L.svr_set_option(k.encode(), v)
        try:
            blocks = int(router.L.svr_gemm_gn_blocks(ctypes.byref(a)))
            assert blocks > 0 and blocks == int(router.L.svr_gemm_gn_blocks(ctypes.byref(d)))
        finally:
            for k, v in gc.OPTION_DEFAULTS.items():
                router.L.svr_set_option(k.encode(), v)


@needs_hipcc
@pytest.mark.parametrize("c,named", lc.CONV_REFUSED, ids=[c.tag for c, _ in lc.CONV_REFUSED])
def test_conv_refused_row_names_its_operand(router, c, named):
    p, ln, Cw, kw = _conv_windows(router, c)
    knobs = {k: c.options[k] for k in lc.POINTER_KNOBS if k in c.options}
    options = {k: v for k, v in c.options.items() if k not in lc.POINTER_KNOBS}
    ptr = lambda t: lc.fake_ptr(t) + (knobs.get("A_off", 0) if t is p.x else knobs.get("halo_off", 0) if t is p.halo else 0)
    got, msg = router.cls(p.x, ln.W, Cw, kw, options, ptr=ptr, zeros_ptr=FAKE + knobs.get("zeros_off", 0))
    assert got == "refused" and named in msg, (c.tag, got, msg)


@needs_hipcc
def test_attention_layouts_are_validated_before_any_launch(router):
    """Accepted rows: an empty call (n_seq = 0) with the row's layout returns 0; refused rows: -1 and the operand's name, with the
    real window count too (refused before any launch)."""
    L = router.L
    for r in lc.ATTN_ROWS:
        n_q, n_o = 3 * r.heads * r.D, r.heads * r.D
        args = (FAKE + r.Q.off + 2 * r.Q.c0, n_q + r.Q.extra, FAKE + r.O.off + 2 * r.O.c0, n_o + r.O.extra)
        assert L.svr_attn_varlen(args[0], args[1], args[2], args[3], None, None, None, 0, max(r.lens), r.heads, r.D, 0.1, None) == 0, \
            (r.name, L.svr_last_error().decode())
    for name, heads, D, ld_qkv, q_off, ld_out, o_off, named in lc.ATTN_REFUSED:
        for n_seq in (0, 3):
            rc = L.svr_attn_varlen(FAKE + q_off, ld_qkv, FAKE + o_off, ld_out, FAKE, FAKE, FAKE, n_seq, 130, heads, D, 0.1, None)
            assert rc == -1 and named in L.svr_last_error().decode(), (name, rc, L.svr_last_error().decode())


@needs_hipcc
def test_side_kernel_layouts_are_validated_before_any_launch(router):
    L = router.L
    for cols, _ in lc.SOFTMAX_ROWS:
        S, Pp = FAKE + 4 * lc.SOFTMAX_S.c0, FAKE + 2 * lc.SOFTMAX_P.c0
        assert L.svr_softmax_rows(S, Pp, 0, cols, cols + lc.SOFTMAX_S.extra, cols + lc.SOFTMAX_P.extra, 1.0, None) == 0, L.svr_last_error().decode()
    for name, cols, ld_s, s_off, ld_p, p_off, named in lc.SOFTMAX_REFUSED:
        rc = L.svr_softmax_rows(FAKE + s_off, FAKE + p_off, 4, cols, ld_s, ld_p, 1.0, None)
        assert rc == -1 and named in L.svr_last_error().decode(), (name, rc, L.svr_last_error().decode())
    assert L.svr_rmsnorm_mod(FAKE, FAKE, 0, 64, 1e-6, None, None, None, 0, None) == 0
    for name, x_off, y_off, named in lc.RMSNORM_REFUSED:
        for rows in (0, 4):
            rc = L.svr_rmsnorm_mod(FAKE + x_off, FAKE + y_off, rows, 64, 1e-6, None, None, None, 0, None)
            assert rc == -1 and named in L.svr_last_error().decode(), (name, rc, L.svr_last_error().decode())
    # svr_unpatchify_euler makes element accesses only: the pitch rule is its whole layout contract
    u = lc.UNPATCHIFY
    assert L.svr_unpatchify_euler(FAKE, 4 * u["C"] - 1, None, FAKE, 0, u["H"], u["W"], u["C"], None) == -1
    assert "ldp" in L.svr_last_error().decode()
    assert L.svr_unpatchify_euler(FAKE + 2 * u["pred"].c0, 4 * u["C"] + u["pred"].extra, None, FAKE, 0, u["H"], u["W"], u["C"], None) == 0


def test_the_table_holds_what_the_contract_lists():
    """Accepted rows: windows inside their canvases, pitches that cover their extents; groups (a), (b), (c) present for every
    GEMM shape; every conv class and both attention head sizes reached; unique ids."""
    for rows, ident in ((lc.GEMM_ROWS, lc.gemm_id), (lc.CONV_ROWS, lc.conv_id)):
        assert len({ident(r) for r in rows}) == len(rows), [ident(r) for r in rows if [ident(q) for q in rows].count(ident(r)) > 1]
    for r in lc.GEMM_ROWS:
        for pl in (r.A, r.C, r.R):
            assert pl is None or (0 <= pl.c0 <= pl.extra and pl.off >= 0), lc.gemm_id(r)
        assert (r.R is not None) == (r.resid is not None) and (r.resid is None or r.epi == "resid"), lc.gemm_id(r)
    shapes = {(lc.S_NARROW, False), (lc.S_WIDE, False), (lc.S_PERS, False), (lc.S_PERS, True)}
    for tag in ("a-ldc8", "a-ldc72-resid", "a-inplace", "b-ldc4"):
        assert {((r.M, r.N, r.K), r.frag) for r in lc.GEMM_ROWS if r.tag == tag} == shapes, tag
    for tag in ("b-c-off8", "b-resid-off8"):
        assert {(r.M, r.N, r.K) for r in lc.GEMM_ROWS if r.tag == tag} == {lc.S_NARROW, lc.S_WIDE, lc.S_PERS}, tag
    assert all(r.cls == "gemm" for r in lc.GEMM_ROWS if r.tag.startswith("b-"))
    c_rows = [r for r in lc.GEMM_ROWS if r.tag.startswith("c-")]
    assert {r.epi for r in c_rows} >= {"bias", "resid", "swiglu", "gelu"} and {r.out for r in c_rows} == {"bf16", "fp32", "h16"}
    assert {r.resid for r in c_rows if r.epi == "resid"} >= {"bf16", "fp32", "h16", "inplace"}
    pers_h16 = {(r.epi, r.resid) for r in c_rows if r.cls == "gemm_persistent" and r.out == "h16"}
    assert pers_h16 >= {("bias", None), ("resid", "h16")}                          # the two h16 forms the persistent kernel serves
    assert {r.C.extra + r.N for r in c_rows if (r.M, r.N, r.K) == lc.S_ODD} == {16, 20}
    assert {c.cls for c in lc.CONV_ROWS} == {"conv_halo", "conv_thin_in", "conv_thinout", "conv_generic"}
    assert {c.row.inst for c in lc.CONV_ROWS if c.cls == "conv_halo"} >= {"halo16_lds", "halo16_wreg8"}
    assert any(c.taps == 2 and c.cls == "conv_generic" for c in lc.CONV_ROWS)
    assert any(c.options.get("conv_thinout4") == 0 for c in lc.CONV_ROWS)
    for c in lc.CONV_ROWS:
        assert 0 <= c.C.c0 <= c.C.extra and (c.R is None) == (c.row.resid is None), lc.conv_id(c)
    assert {r.D for r in lc.ATTN_ROWS} == {128, 512} and {r.Q.extra for r in lc.ATTN_ROWS} == {8, 264}
    assert {tuple(r.lens) for r in lc.ATTN_ROWS} >= {tuple(c[1]) for c in gc.ATTN_CASES}
    assert all(r.Q.c0 % 8 == 0 and r.Q.extra % 8 == 0 and r.O.c0 % 4 == 0 and r.O.extra % 4 == 0 for r in lc.ATTN_ROWS)
    assert {c for c, _ in lc.SOFTMAX_ROWS} == {260, 16384, 16388, 65536}
