"""-m gpu: the layout table of tests/layout_cases.py on the device -- strided and offset operands through the C ABI
(ops.fill_gemm_args with an injected ``chk`` for svr_gemm_bf16, hip_lib.lib() for the other entry points; HipOps itself keeps
refusing non-contiguous tensors).

Outputs.  Every output canvas is a guarded, poisoned buffer (tests/guarded_out.py) wider than the operand.  After the launch
  * the window is checked against the fp64 reference of the DENSE operands with tests/local_error.py's bounds (no tolerance here);
  * every element of the canvas outside the window still holds its poison bits (a store into the pitch gap, or before the
    window's first column, fails this), and the guards are intact;
Inputs.  Input canvases hold NaN outside their windows: a read from a gap column reaches the output as a non-finite value and
fails its bound.
Bit equality.  A row's window equals, bit for bit, the dense launch of the same problem under the options that give it the same
kernel class (gemm_w4 = 0 for the rows that leave the persistent kernel, conv_impl = 1 / conv_sub = 0 for the rows that leave the
halo / sub-pixel kernels, attn_impl = 1 for the output rows the window kernel's 16-byte stores cannot take):
tests/test_gpu_kernels.py::test_gemm_epilogue_paths_bit_identical holds the two epilogue paths of gemm_kernel to bit identity, and
a pitch changes addresses, never arithmetic.
Kernel class.  The class the library reports for the real launch (real pointers) is the row's.

Refused rows are never launched (tests/test_layout_cases.py).  Measured item times: profiles/layout_sweep.txt."""
import contextlib
import ctypes
import math

import pytest
import torch

import geometry_cases as gc
import layout_cases as lc
import local_error as le
from conftest import sub
from guarded_out import guarded

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


@contextlib.contextmanager
def options(hip, opts, record=True):
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        hip.record_kernel_class, hip.last_kernel_class = record, None
        yield
    finally:
        hip.record_kernel_class = False
        for k in opts:
            hip.set_option(k, gc.OPTION_DEFAULTS[k])


def chk(t, dtype=None, name="tensor"):
    """HipOps._chk without the contiguity rule: the windows of this sweep are views"""
    assert t.device.type == "cuda" and (dtype is None or t.dtype == dtype), name
    return t


def nan_canvas(dense2d, place):
    """the input ``dense2d`` as a window of a canvas that holds NaN everywhere else"""
    rows, n = dense2d.shape
    flat = torch.full((lc.flat_elems(rows, n, place, dense2d.dtype),), float("nan"), dtype=dense2d.dtype, device="cuda")
    assert flat.data_ptr() % lc.ALIGN == 0
    _, win = lc.window(flat, rows, n, place)
    win.copy_(dense2d)
    return win


class OutCanvas:
    """a guarded, poisoned canvas with the output window ``.win``; ``init``: the window starts as that tensor (in-place residuals)"""

    def __init__(self, rows, n, place, dtype, init=None):
        self.rows, self.n, self.place = rows, n, place
        self.g = guarded((lc.flat_elems(rows, n, place, dtype),), dtype)
        self.canvas, self.win = lc.window(self.g.t, rows, n, place)
        if init is not None:
            self.win.copy_(init.reshape(rows, n))

    def check(self, name):
        """guards intact, every element outside the window still poison -> the window as a dense tensor"""
        torch.cuda.synchronize()
        self.g.assert_guards(name)
        outside = torch.ones(self.g.t.numel(), dtype=torch.bool, device="cuda")
        e0, ld = self.place.off // self.g.t.element_size(), self.n + self.place.extra
        outside[e0:e0 + self.rows * ld].view(self.rows, ld)[:, self.place.c0:self.place.c0 + self.n] = False
        stray = outside & ~self.g.poisoned()
        if bool(stray.any()):
            i = int(stray.nonzero()[0]) - e0
            raise AssertionError(f"{name}: the launch wrote {int(stray.sum())} canvas elements outside its window; the first at row "
                                 f"{i // ld}, canvas column {i % ld} (window: columns {self.place.c0} .. {self.place.c0 + self.n - 1} of {ld})")
        return self.win.contiguous()


def same_bits(a, b):
    raw = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(raw) == b.contiguous().view(raw)).all())


# ------------------------------------------------------------------------------------------------ plain GEMM
_gemm_cache = {}


def _cached(kind, key, make):
    if (kind, key) not in _gemm_cache:
        _gemm_cache[kind, key] = make()
    return _gemm_cache[kind, key]


def _gemm_key(row):
    return (row.M, row.N, row.K, row.out, row.epi, row.out if row.resid == "inplace" else row.resid)


@pytest.mark.parametrize("row", lc.GEMM_ROWS, ids=[lc.gemm_id(r) for r in lc.GEMM_ROWS])
def test_gemm_layout(hip, row):
    name = lc.gemm_id(row)
    L, opsmod, hip_lib = hip.lib, sub("ops"), sub("hip_lib")
    # dense operands, fp64 reference and dense twin: once per problem, shared by the rows that differ in placement only
    A, W, kw = _cached("operands", _gemm_key(row) + (row.frag,),
                       lambda: lc.gemm_operands(row, sub("packing"), "cuda", frag=hip.pack_gemm_frag))
    assert not row.frag or kw["W_frag"] is not None
    M, NC, dt = row.M, lc.out_cols(row), lc.STORE_KINDS[row.out]
    resid = kw.get("resid")

    def twin():
        g = guarded((M, NC), dt)
        with options(hip, {} if row.cls == "gemm_persistent" else {"gemm_w4": 0}):
            hip.gemm(A, W, g.t, **kw)
            assert hip.last_kernel_class == row.cls, hip.last_kernel_class
        torch.cuda.synchronize()
        g.assert_guards(name + " dense twin")
        return g.t.clone()
    dense = _cached("twin", _gemm_key(row) + (row.frag, row.cls), twin)
    want, bound, mask = _cached("reference", _gemm_key(row), lambda: le.gemm_reference(A, W, dense, **kw))

    out = OutCanvas(M, NC, row.C, dt, init=resid if row.resid == "inplace" else None)
    kwl = dict(kw)
    if row.resid:
        kwl["resid"] = out.win if row.resid == "inplace" else nan_canvas(resid, row.R)
    a, _ = opsmod.fill_gemm_args(nan_canvas(A, row.A), W, out.win, chk=chk, zeros_ptr=hip.zeros.data_ptr(), **kwl)
    assert (a.lda, a.ldc) == (row.K + row.A.extra, NC + row.C.extra) and (not row.resid or a.ldr == row.N + row.R.extra)
    assert hip_lib.KERNEL_CLASSES.get(int(L.svr_gemm_kernel_class(ctypes.byref(a)))) == row.cls, L.svr_last_error().decode()
    hip_lib.check(L.svr_gemm_bf16(ctypes.byref(a), hip._stream()), "svr_gemm_bf16")
    got = out.check(name)
    le.check(name, got, want, bound, mask)
    assert same_bits(got, dense), f"{name}: differs from the dense launch in {int((got != dense).sum())} elements"


# ------------------------------------------------------------------------------------------------ conv family
def conv_frag(hip):
    return lambda kind, W, kt, Cin, N: hip.pack_conv_frag(W, kt, Cin, N, taps=(3, 3) if kind == "conv33" else (2, 2))


@pytest.mark.parametrize("c", lc.CONV_ROWS, ids=[lc.conv_id(c) for c in lc.CONV_ROWS])
def test_conv_layout(hip, c):
    name = lc.conv_id(c)
    L, opsmod, hip_lib = hip.lib, sub("ops"), sub("hip_lib")
    p, ln = lc.conv_launch(c, opsmod, sub("packing"), "cuda", frag=conv_frag(hip))
    assert ln.kw.get("W_frag", 0) is not None, name
    To, N = p.out_shape[0], p.out_shape[3]
    M = To * p.out_shape[1] * p.out_shape[2]
    gn = c.row.gn
    out = OutCanvas(M, N, c.C, p.out_dtype)
    kw = {k: v for k, v in ln.kw.items() if k not in ("ldc", "ldr")}
    if c.R is not None:
        kw["resid"] = nan_canvas(ln.kw["resid"].reshape(M, N), c.R)
    stats = partial = None
    with options(hip, c.options, record=False):
        a, _ = opsmod.fill_gemm_args(p.x, ln.W, out.win, chk=chk, zeros_ptr=hip.zeros.data_ptr(), **kw)
        assert a.ldc == N + c.C.extra and (c.R is None or a.ldr == N + c.R.extra)
        if gn:
            a.gn_groups = gn
            nblk = int(L.svr_gemm_gn_blocks(ctypes.byref(a)))
            assert nblk > 0, name
            partial = guarded((To * nblk * gn * 2,), torch.float64)
            a.gn_partial = partial.t.data_ptr()
        assert hip_lib.KERNEL_CLASSES.get(int(L.svr_gemm_kernel_class(ctypes.byref(a)))) == c.cls, L.svr_last_error().decode()
        hip_lib.check(L.svr_gemm_bf16(ctypes.byref(a), hip._stream()), "svr_gemm_bf16")
        if gn:
            stats = torch.empty(To, gn, 2, dtype=torch.float64, device="cuda")
            hip_lib.check(L.svr_groupnorm_reduce(partial.t.data_ptr(), stats.data_ptr(), To, nblk, gn, hip._stream()), "svr_groupnorm_reduce")
    got = out.check(name).view(p.out_shape)
    le.check_gemm(got, p.x, ln.W, name=name, **ln.kw)
    if gn:
        partial.assert_guards(name + " statistics")
        partial.assert_written(name + " statistics")
        le.check_groupnorm_stats(stats, got, gn, name=name + " fused statistics")
    # the dense twin, under the options that give it the row's class
    g2 = guarded(p.out_shape, p.out_dtype)
    with options(hip, c.twin_options):
        r2 = hip.gemm(p.x, ln.W, g2.t, gn_groups=gn, **ln.kw)
        assert hip.last_kernel_class == c.cls, hip.last_kernel_class
    torch.cuda.synchronize()
    g2.assert_guards(name + " dense twin")
    assert same_bits(got, g2.t), f"{name}: differs from the dense launch in {int((got != g2.t).sum())} elements"
    if gn:
        assert torch.equal(stats, r2[1]), name + ": fused statistics differ from the dense launch's"


# ------------------------------------------------------------------------------------------------ window attention
ATTN_PARAMS = [pytest.param(r, 0, id=r.name) for r in lc.ATTN_ROWS] + \
              [pytest.param(r, 1, id=r.name + "-attn_gen1", marks=pytest.mark.variants) for r in lc.ATTN_ROWS if r.D == 128 and r.twin_impl is None]


@pytest.mark.parametrize("row,attn_impl", ATTN_PARAMS)
def test_attn_layout(hip, row, attn_impl):
    L, hip_lib = hip.lib, sub("hip_lib")
    D, heads, n_rows = row.D, row.heads, 400
    gen = torch.Generator().manual_seed(len(row.lens) + heads + D)
    qkv = torch.randn(n_rows, 3 * heads * D, generator=gen).to(BF16).cuda()
    total = sum(row.lens)
    seq_rows = torch.cat([torch.randint(0, n_rows, (n,), generator=gen) for n in row.lens]).to(torch.int32).cuda()
    n_out = total + 13
    out_rows = torch.randperm(n_out, generator=gen)[:total].to(torch.int32).cuda()             # scattered: 13 rows belong to nobody
    cu = torch.tensor([0] + list(torch.tensor(row.lens).cumsum(0)), dtype=torch.int32).cuda()
    scale, max_len = 1.0 / math.sqrt(D), row.max_len or max(row.lens)
    Qw = nan_canvas(qkv, row.Q)
    out = OutCanvas(n_out, heads * D, row.O, BF16)
    with options(hip, {"attn_impl": attn_impl}, record=False):
        hip_lib.check(L.svr_attn_varlen(Qw.data_ptr(), Qw.stride(0), out.win.data_ptr(), out.win.stride(0), seq_rows.data_ptr(),
                                        out_rows.data_ptr(), cu.data_ptr(), len(row.lens), max_len, heads, D, scale, hip._stream()),
                      "svr_attn_varlen")
    got = out.check(row.name)
    untouched = guarded((n_out, heads * D), BF16)
    le.check_attn(got, qkv, seq_rows, out_rows, cu, heads, D, scale, name=f"attn {row.name}", before=untouched.t)
    g2 = guarded((n_out, heads * D), BF16)
    with options(hip, {"attn_impl": attn_impl if row.twin_impl is None else row.twin_impl}, record=False):
        hip.attn_varlen(qkv, g2.t, seq_rows, out_rows, cu, max_len, heads, D, scale)
    torch.cuda.synchronize()
    g2.assert_guards(row.name + " dense twin")
    assert same_bits(got, g2.t), f"attn {row.name}: differs from the dense launch"


# ------------------------------------------------------------------------------------------------ side kernels
@pytest.mark.parametrize("cols,rows", lc.SOFTMAX_ROWS, ids=[f"cols{c}" for c, _ in lc.SOFTMAX_ROWS])
def test_softmax_rows_layout(hip, cols, rows):
    L, hip_lib = hip.lib, sub("hip_lib")
    S = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(cols)) * 3).cuda()
    Sw = nan_canvas(S, lc.SOFTMAX_S)
    out = OutCanvas(rows, cols, lc.SOFTMAX_P, BF16)
    assert (Sw.stride(0), out.win.stride(0)) == (cols + 4, cols + 12)
    hip_lib.check(L.svr_softmax_rows(Sw.data_ptr(), out.win.data_ptr(), rows, cols, Sw.stride(0), out.win.stride(0), 0.7, hip._stream()),
                  "svr_softmax_rows")
    got = out.check(f"softmax_rows {cols}")
    le.check_softmax_rows(got, S, 0.7, name=f"softmax_rows {cols} strided")
    g2 = guarded((rows, cols), BF16)
    hip.softmax_rows(S, g2.t, 0.7)
    torch.cuda.synchronize()
    assert same_bits(got, g2.t)


def test_unpatchify_euler_offset_prediction(hip):
    """ldp wider than 4 C behind a base offset of an odd number of elements: the kernel makes element accesses only"""
    L, hip_lib = hip.lib, sub("hip_lib")
    u = lc.UNPATCHIFY
    T, H, W, C = u["T"], u["H"], u["W"], u["C"]
    gen = torch.Generator().manual_seed(5)
    pred = torch.randn(T * (H // 2) * (W // 2), 4 * C, generator=gen).to(BF16).cuda()
    x_t = torch.randn(T, H, W, C, generator=gen).to(BF16).cuda()
    Pw = nan_canvas(pred, u["pred"])
    for xt in (x_t, None):
        g = guarded((T, H, W, C), BF16)
        hip_lib.check(L.svr_unpatchify_euler(Pw.data_ptr(), Pw.stride(0), None if xt is None else xt.data_ptr(), g.t.data_ptr(), T, H, W, C,
                                             hip._stream()), "svr_unpatchify_euler")
        torch.cuda.synchronize()
        g.assert_guards("unpatchify_euler")
        le.check("unpatchify_euler offset ldp", g.t, *le.unpatchify_euler_reference(pred, xt, g.t.shape))
        g2 = guarded((T, H, W, C), BF16)
        hip.unpatchify_euler(pred, xt, g2.t)
        assert same_bits(g.t, g2.t)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_alpha_rgba_view_equals_contiguous_rgb(hip, dtype):
    """svr_alpha_* with ld_px = 4 (the first three channels of an RGBA tensor whose fourth holds NaN) against ld_px = 3 on a contiguous
    copy: same bits in the alpha and in the edge bytes."""
    al = lc.ALPHA
    T, H, W, s = al["T"], al["H"], al["W"], al["scale"]
    gen = torch.Generator().manual_seed(11)
    rgba = (torch.rand(T, H, W, 4, generator=gen) * 2 - 1).to(dtype).cuda()
    rgba[..., 3] = float("nan")
    alpha_lo = torch.rand(T, H // s, W // s, generator=gen).cuda()
    outs = []
    for rgb in (rgba[..., :3], rgba[..., :3].contiguous()):
        g, e = guarded((T, H, W), F32), guarded((T, H, W), torch.uint8)
        hip.alpha_upscale(rgb, alpha_lo, out=g.t, edge_out=e.t)
        torch.cuda.synchronize()
        g.assert_guards("alpha_upscale"); e.assert_guards("alpha_upscale edges")
        g.assert_written("alpha_upscale")
        assert bool(torch.isfinite(g.t).all())
        outs.append((g.t.clone(), e.t.clone()))
    assert rgba[..., :3].stride(2) == 4 and same_bits(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ the thin-output weight
@pytest.mark.parametrize("thinout4", [1, 0], ids=["conv_thinout4_kernel", "conv_thinout_kernel"])
def test_thin_output_conv_takes_an_exact_weight(hip, thinout4):
    """ABI v9: a thin-output conv with N <= 4 couts accepts an exact [N, K] weight.  An exact [3, K] weight under conv_thinout4 1
    (the 4-cout kernel) and 0 (the 32-cout kernel), against local_error's bounds and the launch with the 128-row padded weight.

    The weight sits inside a larger buffer of this test's own, 32 * K elements of NaN behind it, so that no kernel reads outside
    the test's allocation whatever it stages.  A value test cannot see the over-read itself: the couts 3 .. 31 that the staged rows
    would feed are never stored (epilogue_store masks n >= N), so NaN in them changes nothing.  That conv_thinout_kernel forms no
    source address past row N - 1 of W (rows >= N come from the zero page, as in conv_thinout4_kernel) is verified by reading
    its staging code (csrc/svr_conv_thinout.hip: `wreal ? W row : g.zeros`)."""
    opsmod, packing, hip_lib, L = sub("ops"), sub("packing"), sub("hip_lib"), hip.lib
    row = gc.R("thinout4", 21, 70, "T3_kt3", 128, 3, "bf16", None, 0, "bias")
    p = gc.conv_problem(row, opsmod, packing, "cuda")
    ln = p.launches[0]
    K, N = ln.W.shape[1], 3
    buf = torch.full(((N + 32) * K,), float("nan"), dtype=BF16, device="cuda")
    W3 = buf[:N * K].view(N, K)
    W3.copy_(ln.W[:N])
    with options(hip, {"conv_thinout4": thinout4}, record=False):
        g = guarded(p.out_shape, p.out_dtype)
        # (fill_gemm_args wants the 128-row padded shape of the product's weights: the exact tensor goes in by pointer)
        a, _ = opsmod.fill_gemm_args(p.x, ln.W, g.t, chk=chk, zeros_ptr=hip.zeros.data_ptr(), **ln.kw)
        a.W = W3.data_ptr()
        assert hip_lib.KERNEL_CLASSES.get(int(L.svr_gemm_kernel_class(ctypes.byref(a)))) == "conv_thinout"
        hip_lib.check(L.svr_gemm_bf16(ctypes.byref(a), hip._stream()), "svr_gemm_bf16")
        torch.cuda.synchronize()
        g.assert_guards("exact [3, K] weight")
        le.check_gemm(g.t, p.x, ln.W, name=f"thin output, exact weight, conv_thinout4 {thinout4}", **ln.kw)
        g2 = guarded(p.out_shape, p.out_dtype)
        hip.gemm(p.x, ln.W, g2.t, **ln.kw)
        torch.cuda.synchronize()
        assert same_bits(g.t, g2.t)
