"""-m gpu: the DiT kernels on tensors past 2^32 elements (and, for the fp32 stream, past 2^32 bytes) -- the sizes of BASELINE config 5
(the 65-frame 7B clip: qkv [550 858, 9 216] = 5.08e9 elements, h1 [550 858, 12 288] = 6.77e9, an fp32 residual stream of 6.8e9 bytes),
which bench.py times and nothing checked.  tests/test_gpu_fullscale.py stops at 2.24e9 elements / 2.99e9 bytes: a row offset formed
in unsigned 32 bits, or a 32-bit product widened afterwards, is still exact there.

tests/index_width_cases.py holds the case table (config 5's widths on the smallest ragged row counts behind each line: M12 = 352 013
rows for the widths 12 288 and fp32 3 072, M9 = 468 500 for 9 216; its docstring derives them) and the block-wise checkers:

  1. GEMM whose OUTPUT passes 2^32 elements -- the qkv form and the bias + tanh-GELU mlp-in form -- on the three main loops production
     can select: gemm_w4r_kernel (W_frag given), gemm_w4q_kernel (no W_frag), gemm_kernel (svr_set_option("gemm_w4", 0));
  2. GEMM whose INPUT passes 2^32 elements (the mlp-out read side: K = 12 288), with and without W_frag;
  3. the residual stream past 2^32 bytes updated in place by the gate + residual epilogue, fp32 and h16;
  4. a 58-row launch into the last rows of a qkv-sized buffer: a view whose BASE lies past element 2^32, as the 7B engine's text-row
     launches have (no shared blocks);
  5. rmsnorm_mod reading the fp32 (then h16) stream; 6. qknorm_rope in place, with the 3B table form and the rope3d form, and on the
     58-row view; 7. attn_varlen gathering windows from below, across and behind the line, on both attention kernels.

Every output comes from tests/guarded_out.py (guards and poison are checked over the whole tensor), EVERY row is compared -- in blocks
of 16 384 rows against local_error's fp64 reference: per element against its derived bound, per block against the project's rel_err
bounds (2.5e-3 behind a bf16 store, 1e-3 behind an fp32 / h16 store, 4e-3 behind attention) -- and the checker's element count is
compared with the tensor's.  Each GEMM launch asserts the kernel class that served it.  With SVR_INDEX_WIDTH_LOG=<file> every case
appends its worst err / bound, kernel class, peak memory and wall time there (profiles/index_width.txt)."""
import contextlib
import math
import time

import pytest
import torch

import index_width_cases as iw
from conftest import sub
from guarded_out import Pool
from ops_reference import EPI_BIAS_GELU, EPI_RESID_GATE, H16

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
GEMM_W4_DEFAULT = 1               # the library's default for svr_set_option("gemm_w4", ...)
LOOP_CLASS = {"w4r": "gemm_persistent", "w4q": "gemm_persistent", "gemm_kernel": "gemm"}


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


@pytest.fixture(scope="module")
def cfg():
    return sub("config").DIT_7B


def _free():
    import gc
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def give_the_memory_back():
    """the cases share the allocator's cached blocks (Clock); the module returns them when its last test is done"""
    yield
    _free()


@pytest.fixture(scope="module")
def qkv9(cfg):
    """the [M9, 9 216] qkv operand of cases 6 and 7: READ-ONLY (case 6 works on guarded copies of it)"""
    c = iw.case(cfg, "qknorm_rope")
    t = iw.fill_rows(torch.empty(c.rows, c.width, dtype=BF16, device="cuda"), seed=9)
    yield t
    del t
    _free()


@pytest.fixture(scope="module")
def h1_in(cfg):
    """the [M12, 12 288] activation of case 2: READ-ONLY"""
    c = iw.case(cfg, "gemm_in_mlp_out")
    t = iw.fill_rows(torch.empty(c.rows, c.width, dtype=BF16, device="cuda"), seed=12)
    yield t
    del t
    _free()


class Clock:
    """wall time and peak device memory of one case, for the record"""

    def __init__(self):
        # (the caching allocator keeps its blocks from case to case -- every case needs the same few GB of fp64 temporaries; with
        # the cache emptied before each case, one case or another of a run took 3-5 s instead of 0.5 s -- and the module gives
        # them back at its end: give_the_memory_back)
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()

    def record(self, name, tally, kernel):
        torch.cuda.synchronize()
        iw.record_run(name, tally, kernel, torch.cuda.max_memory_allocated(), time.perf_counter() - self.t0)


@contextlib.contextmanager
def main_loop(hip, loop):
    """route the next launches to one of the three main loops; the options go back in ``finally``"""
    hip.record_kernel_class, hip.last_kernel_class = True, None
    hip.set_option("gemm_w4", 0 if loop == "gemm_kernel" else GEMM_W4_DEFAULT)
    try:
        yield
    finally:
        hip.set_option("gemm_w4", GEMM_W4_DEFAULT)
        hip.record_kernel_class, hip.last_kernel_class = False, None


def vec(n, seed, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, generator=g, device="cuda") + shift


def weight(N, K, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return sub("packing").pack_matrix(torch.randn(N, K, generator=g, device="cuda") / math.sqrt(K), "cuda")


def gemm_launch(hip, gout, loop, A, W, Wf, M, **kw):
    """one launch on ``loop`` into a fresh guarded [M, N] bf16 tensor; the kernel class is asserted"""
    out = gout(M, kw["N"], dtype=BF16)
    with main_loop(hip, loop):
        hip.gemm(A, W, out, W_frag=Wf if loop == "w4r" else None, **kw)
        assert hip.last_kernel_class == LOOP_CLASS[loop], (loop, hip.last_kernel_class)
    return out


# ------------------------------------------------------------------ 1. GEMM, output past 2^32 elements
@pytest.mark.parametrize("loop", ["w4r", "w4q", "gemm_kernel"])
@pytest.mark.parametrize("form", ["gemm_out_qkv", "gemm_out_mlp_in"])
def test_gemm_output_past_2_32_elements(hip, cfg, form, loop):
    """[M9, 9 216] plain (the 7B qkv form) and [M12, 12 288] with bias + tanh-GELU (the 7B mlp-in form); K = 192.  The w4q case
    also runs the launch on gemm_w4r_kernel: the two main loops give the same bits (the existing contract)."""
    c = iw.case(cfg, form)
    M, N, K = c.rows, c.N, c.K
    assert M * N > iw.LINE and loop in c.variants
    clock = Clock()
    A = iw.fill_rows(torch.empty(M, K, dtype=BF16, device="cuda"), seed=3)
    W = weight(N, K)
    Wf = hip.pack_gemm_frag(W)
    kw = dict(N=N, K=K)
    if form == "gemm_out_mlp_in":
        kw.update(bias=vec(N, 4), epilogue=EPI_BIAS_GELU)
    gout = Pool()
    out = gemm_launch(hip, gout, loop, A, W, Wf, M, **kw)
    if loop == "w4q":
        assert iw.check_rows_equal(gemm_launch(hip, gout, "w4r", A, W, Wf, M, **kw), out, name=f"{form}: w4r against w4q") == M
    tally = iw.check_gemm_rows(out, A, W, tol=iw.TOL_BF16, name=f"{form}[{loop}]", **kw)
    assert tally.rows == M and tally.elements == M * N
    gout.check(f"{form}[{loop}]")
    clock.record(f"{form}[{loop}]", tally, LOOP_CLASS[loop])


# ------------------------------------------------------------------ 2. GEMM, input past 2^32 elements
@pytest.mark.parametrize("loop", ["w4r", "w4q"])
def test_gemm_input_past_2_32_elements(hip, cfg, h1_in, loop):
    """A = [M12, 12 288] (the 7B mlp-out read side: the hazard is the input's row pitch), N = 512, bias, bf16 store."""
    c = iw.case(cfg, "gemm_in_mlp_out")
    M, N, K = c.rows, c.N, c.K
    assert tuple(h1_in.shape) == (M, K) and M * K > iw.LINE
    clock = Clock()
    W = weight(N, K)
    Wf = hip.pack_gemm_frag(W)
    kw = dict(N=N, K=K, bias=vec(N, 4))
    gout = Pool()
    out = gemm_launch(hip, gout, loop, h1_in, W, Wf, M, **kw)
    if loop == "w4q":
        assert iw.check_rows_equal(gemm_launch(hip, gout, "w4r", h1_in, W, Wf, M, **kw), out, name="gemm_in_mlp_out: w4r against w4q") == M
    tally = iw.check_gemm_rows(out, h1_in, W, tol=iw.TOL_BF16, name=f"gemm_in_mlp_out[{loop}]", **kw)
    assert tally.rows == M and tally.elements == M * N
    gout.check(f"gemm_in_mlp_out[{loop}]")
    clock.record(f"gemm_in_mlp_out[{loop}]", tally, LOOP_CLASS[loop])


# ------------------------------------------------------------------ 3. GEMM, wide stream past 2^32 bytes, in place
@pytest.mark.parametrize("kind", [F32, H16], ids=["fp32", "h16"])
def test_gemm_stream_past_2_32_bytes_in_place(hip, cfg, kind):
    """gate * (acc + bias) + residual into the stream itself (C aliases resid): [M12, 3 072] fp32 = 4.33e9 bytes, then the h16 kind
    on the same rows.  The checker reads the residual from the copy made before the launch, block by block."""
    c = iw.case(cfg, "gemm_stream")
    M, N, K = c.rows, c.N, c.K
    assert kind != F32 or M * N * 4 > iw.LINE
    clock = Clock()
    A = iw.fill_rows(torch.empty(M, K, dtype=BF16, device="cuda"), seed=3)
    W = weight(N, K)
    kw = dict(N=N, K=K, bias=vec(N, 4), gate=vec(N, 5), epilogue=EPI_RESID_GATE)
    before = iw.fill_rows(torch.empty(M, N, dtype=kind, device="cuda"), seed=6, scale=2.0)
    gout = Pool()
    hid = gout(M, N, dtype=kind, init=before)
    with main_loop(hip, "w4r"):
        hip.gemm(A, W, hid, resid=hid, out_f32=True, W_frag=hip.pack_gemm_frag(W), **kw)
        assert hip.last_kernel_class == "gemm_persistent"
    name = f"gemm_stream[{'fp32' if kind == F32 else 'h16'}]"
    tally = iw.check_gemm_rows(hid, A, W, tol=iw.TOL_WIDE, name=name, resid=before, **kw)
    assert tally.rows == M and tally.elements == M * N
    gout.check(name)
    clock.record(name, tally, "gemm_persistent")


# ------------------------------------------------------------------ 4. GEMM on a view whose base is past the line
def test_gemm_into_a_view_whose_base_is_past_2_32_elements(hip, cfg):
    """58 rows into out[M9 - 58:] of a poisoned [M9, 9 216] buffer (the 7B engine's text-row launch into qkv[N:]): the 58 rows are
    checked, every other element still holds the poison, the guards are intact."""
    c = iw.case(cfg, "gemm_view")
    M, N, K, rows = c.rows, c.N, c.K, c.view_rows
    r0 = M - rows
    assert r0 * N > iw.LINE
    clock = Clock()
    A = iw.fill_rows(torch.empty(rows, K, dtype=BF16, device="cuda"), seed=3)
    W = weight(N, K)
    gout = Pool()
    out = gout(M, N, dtype=BF16)
    with main_loop(hip, "w4q"):
        hip.gemm(A, W, out[r0:], N=N, K=K)
        assert hip.last_kernel_class == "gemm"             # (36 output tiles: below the persistent kernel's 256)
    tally = iw.check_gemm_rows(out[r0:], A, W, tol=iw.TOL_BF16, name="gemm_view", N=N, K=K, row0=r0)
    assert tally.rows == rows and tally.elements == rows * N
    assert iw.check_rows_poisoned(out[:r0], name="gemm_view: rows in front of the view") == r0
    gout.check("gemm_view", written=False)
    clock.record("gemm_view", tally, "gemm")


# ------------------------------------------------------------------ 5. rmsnorm_mod
@pytest.mark.parametrize("kind", [F32, H16], ids=["fp32", "h16"])
def test_rmsnorm_mod_stream_past_2_32_bytes(hip, cfg, kind):
    c = iw.case(cfg, "rmsnorm_mod")
    M, dim = c.rows, c.width
    assert kind != F32 or M * dim * 4 > iw.LINE
    clock = Clock()
    x = iw.fill_rows(torch.empty(M, dim, dtype=kind, device="cuda"), seed=6, scale=2.0)
    kw = dict(scale=vec(dim, 2, shift=1.0), shift=vec(dim, 3))
    gout = Pool()
    out = gout(M, dim, dtype=BF16)
    hip.rmsnorm_mod(x, out, cfg.norm_eps, **kw)
    name = f"rmsnorm_mod[{'fp32' if kind == F32 else 'h16'}]"
    tally = iw.check_rmsnorm_rows(out, x, cfg.norm_eps, tol=iw.TOL_BF16, name=name, **kw)
    assert tally.rows == M and tally.elements == M * dim
    gout.check(name)
    clock.record(name, tally, "rmsnorm_mod_kernel")


# ------------------------------------------------------------------ 6. qknorm_rope
def rope_form(form, rows):
    """(pos int16 [rows, 3], t_offset, cos, sin): ``table_3b`` -- the 3B form, 21 frequencies per axis on a table indexed by
    position, t_offset = 58; ``rope3d`` -- the 7B form, 3 x 10 frequencies (pairs 30 .. 63 pass through) on a table of
    linspace(-1, 1) values with row 0 = angle 0.  Positions are random int16 from 8 rows in front of the table to 8 rows behind it
    (the kernel clamps them, and so does the reference)."""
    config = sub("config")
    if form == "table_3b":
        n_pos, n_freq, t_offset = 512, config.DIT_3B.rope_freqs, iw.TXT_ROWS
        ang = torch.arange(n_pos, dtype=F32)[:, None] * (10000.0 ** (-torch.arange(n_freq, dtype=F32) / n_freq))[None, :]
    else:
        n_pos, n_freq, t_offset = 300, config.DIT_7B.rope_freqs, 0
        values = torch.cat([torch.zeros(1), torch.linspace(-1, 1, steps=n_pos - 1)])
        ang = values[:, None] * (torch.linspace(1.0, 128.0, n_freq) * math.pi)[None, :]
    assert n_freq == (21 if form == "table_3b" else 10)
    g = torch.Generator(device="cuda").manual_seed(13)
    pos = torch.randint(-8, n_pos + 8, (rows, 3), generator=g, device="cuda").to(torch.int16)
    return pos, t_offset, ang.cos().cuda().contiguous(), ang.sin().cuda().contiguous()


@pytest.mark.parametrize("form", ["table_3b", "rope3d"])
def test_qknorm_rope_in_place_past_2_32_elements(hip, cfg, qkv9, form):
    c = iw.case(cfg, "qknorm_rope")
    M, heads = c.rows, cfg.heads
    assert tuple(qkv9.shape) == (M, 3 * heads * 128) and qkv9.numel() > iw.LINE
    clock = Clock()
    pos, t_offset, cos, sin = rope_form(form, M)
    wq, wk = vec(128, 1, shift=1.0), vec(128, 2, shift=1.0)
    gout = Pool()
    got = gout.like(qkv9, init=qkv9)
    hip.qknorm_rope(got, heads, pos, t_offset, cos, sin, wq, wk, cfg.norm_eps)
    tally = iw.check_qknorm_rows(got, qkv9, heads, pos, t_offset, cos, sin, wq, wk, cfg.norm_eps, tol=iw.TOL_BF16, name=f"qknorm_rope[{form}]")
    assert tally.rows == M and tally.elements == qkv9.numel()
    gout.check(f"qknorm_rope[{form}]")
    clock.record(f"qknorm_rope[{form}]", tally, "qknorm_rope_kernel")


def test_qknorm_rope_on_the_text_rows_behind_2_32_elements(hip, cfg, qkv9):
    """the 58-row call on qkv[M9 - 58:] (the engine's text rows: rope3d table, positions 0): those rows are checked, everything in
    front of them keeps its bits."""
    c = iw.case(cfg, "qknorm_rope_view")
    M, heads, rows = c.rows, cfg.heads, c.view_rows
    r0 = M - rows
    assert r0 * c.width > iw.LINE
    clock = Clock()
    pos, t_offset, cos, sin = rope_form("rope3d", rows)
    wq, wk = vec(128, 1, shift=1.0), vec(128, 2, shift=1.0)
    gout = Pool()
    got = gout.like(qkv9, init=qkv9)
    hip.qknorm_rope(got[r0:], heads, pos, t_offset, cos, sin, wq, wk, cfg.norm_eps)
    tally = iw.check_qknorm_rows(got[r0:], qkv9[r0:], heads, pos, t_offset, cos, sin, wq, wk, cfg.norm_eps, tol=iw.TOL_BF16,
                                 name="qknorm_rope_view", row0=r0)
    assert tally.rows == rows and tally.elements == rows * c.width
    assert iw.check_rows_equal(got[:r0], qkv9[:r0], name="qknorm_rope_view: rows in front of the view") == r0
    gout.check("qknorm_rope_view")
    clock.record("qknorm_rope_view", tally, "qknorm_rope_kernel")


# ------------------------------------------------------------------ 7. attn_varlen gathering across the line
@pytest.mark.parametrize("variant", ["first_generation", "window"])
def test_attn_varlen_gathers_rows_across_2_32_elements(hip, cfg, qkv9, variant):
    """Three windows over the [M9, 9 216] qkv, 24 heads of 128: video rows only from behind row 466 033, alternately from below and
    behind it, only from below; each followed by the last 58 rows.  Video lengths 2 083 / 2 083 / 641: the longest window has 2 141
    rows > 2 048, so the launch runs on the first-generation kernel, the route config 5 takes; 1 990 / 1 157 / 19 (2 048 / 1 215 /
    77 with the text rows): the window kernel, its row table full."""
    c = iw.case(cfg, "attn_varlen")
    heads, D = cfg.heads, cfg.head_dim
    seq, cu = iw.attn_windows(c.rows, iw.line_row(c.width), iw.ATTN_LENS[variant])
    cu_l = cu.tolist()
    max_len = max(b - a for a, b in zip(cu_l, cu_l[1:]))
    assert (max_len > iw.AW_MAXL) == (variant == "first_generation")
    clock = Clock()
    total = seq.numel()
    out_rows = torch.randperm(total + 16, generator=torch.Generator().manual_seed(2))[:total].to(torch.int32).cuda()
    seq, cu = seq.cuda(), cu.cuda()
    scale = 1.0 / math.sqrt(D)
    before = torch.full((total + 16, heads * D), 7.0, device="cuda", dtype=BF16)
    gout = Pool()
    outs = []
    for _ in range(2):
        out = gout(total + 16, heads * D, dtype=BF16, init=before)
        hip.attn_varlen(qkv9, out, seq, out_rows, cu, max_len, heads, D, scale)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])                    # two launches, the same bits
    tally = iw.check_attn_windows(outs[0], qkv9, seq, out_rows, cu, heads, D, scale, tol=iw.TOL_ATTN, name=f"attn_varlen[{variant}]",
                                  before=before)
    assert tally.elements == total * heads * D
    gout.check(f"attn_varlen[{variant}]")
    clock.record(f"attn_varlen[{variant}]", tally, "attn_kernel" if variant == "first_generation" else "attn_win_kernel")
