"""-m "not gpu": the case table and the block-wise checkers of tests/index_width_cases.py, proven on the CPU.

  * Sizes: the DiT tensor sizes of BASELINE configs 3 and 5, computed from config.DIT_3B / DIT_7B on their token grids, say why
    each case of tests/test_gpu_index_width.py exists -- config 5's qkv and h1 pass 2^32 elements and its fp32 stream 2^32 bytes,
    no config-3 tensor passes 2^32 elements -- and every case of the table passes the line it names, by about 2 500 ragged rows,
    at a width that comes from the config.
  * Checkers: over TorchOps("cpu") at small sizes (blocks of 64 rows) each block-wise checker accepts the correct result and counts
    every element; over a double whose result is correct but whose rows m >= m_wrap are stored at (or read from) m - m_wrap --
    what a row offset wrapped at 32 bits does -- each one fails and names the first wrong row."""
import math
import re

import pytest
import torch

import index_width_cases as iw
import local_error as le
from conftest import sub
from guarded_out import Pool
from ops_reference import TorchOps, EPI_BIAS, EPI_BIAS_GELU, EPI_RESID_GATE, H16, H16_SCALE

BF16, F32 = torch.bfloat16, torch.float32
BLOCK = 64


# ------------------------------------------------------------------------------------------------ sizes
def _sizes(name):
    config = sub("config")
    cfg_name, frames, height, width = iw.CLIPS[name]
    return iw.dit_tensors(getattr(config, cfg_name), iw.token_grid(frames, height, width))


def test_clips_are_the_benchmark_workloads():
    import bench
    for name, (cfg_name, frames, height, width) in iw.CLIPS.items():
        assert tuple(bench.WORKLOADS[name][:3]) == (frames, height, width)
    assert iw.token_grid(*iw.CLIPS["cfg5"][1:]) == (17, 135, 240) and iw.token_grid(*iw.CLIPS["cfg3"][1:]) == (9, 135, 240)
    assert iw.TXT_ROWS == sub("weights").synth_text_embedding().shape[0]


def test_config5_passes_the_lines_and_config3_does_not():
    c5, c3 = _sizes("cfg5"), _sizes("cfg3")
    assert c5["qkv"][:2] == (550858, 9216) and c5["h1"][:2] == (550858, 12288)
    for t in ("qkv", "h1"):
        assert c5[t][0] * c5[t][1] > iw.LINE
    assert c5["hid_fp32"][0] * c5["hid_fp32"][1] * c5["hid_fp32"][2] > iw.LINE
    for t, (rows, cols, _) in c3.items():
        assert rows * cols < iw.LINE, t                                             # no config-3 tensor passes 2^32 elements,
    assert c3["qkv"][0] * c3["qkv"][1] > 2 ** 31                                    # though its qkv passes 2^31 elements
    assert c3["hid_fp32"][0] * c3["hid_fp32"][1] * 4 < iw.LINE                      # and no fp32 trunk tensor 2^32 bytes
    # nothing else of config 5 is past 2^32 elements: the table covers the tensors that are
    assert sorted(t for t, (rows, cols, _) in c5.items() if rows * cols > iw.LINE) == ["h1", "qkv"]


def test_every_case_passes_the_line_it_names_at_a_config_width():
    config = sub("config")
    cfg = config.DIT_7B
    w = iw.widths(cfg)
    assert w == {"qkv": 9216, "h1": 12288, "hid": 3072}
    c5 = _sizes("cfg5")
    assert (w["qkv"], w["h1"], w["hid"]) == (c5["qkv"][1], c5["h1"][1], c5["hid_fp32"][1])
    table = iw.cases(cfg)
    assert len({c.name for c in table}) == len(table) == 9
    for c in table:
        assert c.width == w[c.width_of], c.name
        unit = c.elem_bytes if c.line == "bytes" else 1
        boundary = iw.line_row(c.width, unit)
        assert boundary * c.width * unit <= iw.LINE < (boundary + 1) * c.width * unit
        assert c.offset_of_last_launch_row() > iw.LINE, c.name                      # the tensor's end (a view's base) is behind the line
        behind = c.rows - boundary
        assert 2400 <= behind <= 2600 and c.rows % iw.PANEL and c.rows % 8, c.name  # ragged, about 2 500 rows behind
        first_whole = -(-(boundary + 1) // iw.PANEL)                                # the first panel wholly behind the line
        assert c.rows // iw.PANEL - first_whole >= 4, c.name                        # several whole panels, then the ragged one
        assert c.rows <= c5[{"hid": "hid_fp32"}.get(c.width_of, c.width_of)][0]     # never more rows than the clip has
        if c.op == "gemm":
            assert c.K % 64 == 0 and c.K >= 192 and c.N % 256 == 0
            assert (c.K == w["h1"] and c.N == 512) if c.tensor == "A" else (c.K == 192 and c.N == c.width), c.name
    assert (iw.M12, iw.M9) == (352013, 468500)
    assert iw.line_row(12288) == iw.line_row(3072, 4) == 349525 and iw.line_row(9216) == 466033
    # the persistent GEMM kernel takes a launch from 256 output tiles on: every full-size GEMM case has them
    assert all(-(-c.rows // 256) * (c.N // 256) >= 256 for c in table if c.op == "gemm" and not c.view_rows)


def test_attention_windows_straddle_the_line():
    boundary = iw.line_row(9216)
    for variant, lens in iw.ATTN_LENS.items():
        seq, cu = iw.attn_windows(iw.M9, boundary, lens)
        cu_l = cu.tolist()
        longest = max(b - a for a, b in zip(cu_l, cu_l[1:]))
        assert (longest > iw.AW_MAXL) == (variant == "first_generation") and (variant != "window" or longest == iw.AW_MAXL)
        wins = [seq[a:b].long() for a, b in zip(cu_l, cu_l[1:])]
        for wdw in wins:
            assert wdw[-iw.TXT_ROWS:].tolist() == list(range(iw.M9 - iw.TXT_ROWS, iw.M9)) and len(set(wdw.tolist())) == len(wdw)
        v0, v1, v2 = (wdw[:-iw.TXT_ROWS] for wdw in wins)
        assert int(v0.min()) > boundary and int(v2.max()) < boundary
        assert int(v1[0::2].max()) < boundary < int(v1[1::2].min()) and int(seq.max()) == iw.M9 - 1
    assert [l + iw.TXT_ROWS for l in iw.ATTN_LENS["window"]] == [2048, 1215, 77] and iw.ATTN_LENS["first_generation"] == (2083, 2083, 641)


# ------------------------------------------------------------------------------------------------ checkers
def rnd(*shape, scale=1.0, seed=0, dtype=BF16):
    g = torch.Generator().manual_seed(seed + sum(shape))
    v = torch.randn(*shape, generator=g) * scale
    return (v * H16_SCALE).to(H16) if dtype == H16 else v.to(dtype)


class WrappingTorchOps(TorchOps):
    """The result is correct, but a row offset wrapped: with ``wrap = ("store", m_wrap)`` the rows m >= m_wrap of the output land
    at m - m_wrap (rows 0 .. M - m_wrap - 1 then hold the LATER rows' results, rows from m_wrap on are never written); with
    ("load", m_wrap) the rows m >= m_wrap of the input are read from m - m_wrap."""

    def __init__(self, wrap, **kw):
        super().__init__("cpu", **kw)
        self.mode, self.m_wrap = wrap

    def _loaded(self, x):
        if self.mode != "load":
            return x
        x = x.clone()
        x[self.m_wrap:] = x[:x.shape[0] - self.m_wrap]
        return x

    def _stored(self, out, res):
        if self.mode != "store":
            out.copy_(res)
            return out
        out[:self.m_wrap] = res[:self.m_wrap]
        out[:res.shape[0] - self.m_wrap] = res[self.m_wrap:]
        return out

    def gemm(self, A, W, out, **kw):
        res = super().gemm(self._loaded(A), W, torch.empty_like(out), **kw)        # (resid is read before out is written, as in place)
        return self._stored(out, res)

    def rmsnorm_mod(self, x, out, eps, **kw):
        return self._stored(out, super().rmsnorm_mod(self._loaded(x), torch.empty_like(out), eps, **kw))

    def qknorm_rope(self, qkv, heads, pos, *args):
        res = super().qknorm_rope(self._loaded(qkv), heads, pos, *args)             # (TorchOps.qknorm_rope returns a new tensor's rows
        return self._stored(qkv, res.clone())                                       # through copy_: keep the launch in place)

    def attn_varlen(self, qkv, out, seq_rows, *args):
        if self.mode == "load":
            seq_rows = torch.where(seq_rows >= self.m_wrap, seq_rows - self.m_wrap, seq_rows)
        return super().attn_varlen(qkv, out, seq_rows, *args)


def wrong_row(fn):
    """the checker fails and names its first wrong row -> that row"""
    with pytest.raises(AssertionError) as e:
        fn()
    m = re.search(r"first wrong row (\d+)", str(e.value))
    assert m, str(e.value)
    return int(m.group(1))


GEMM_FORMS = {
    "plain_bf16": (BF16, dict()),
    "bias_gelu_bf16": (BF16, dict(bias=True, epilogue=EPI_BIAS_GELU)),
    "stream_fp32": (F32, dict(bias=True, gate=True, epilogue=EPI_RESID_GATE)),
    "stream_h16": (H16, dict(bias=True, gate=True, epilogue=EPI_RESID_GATE)),
}


@pytest.mark.parametrize("form", sorted(GEMM_FORMS))
def test_gemm_checker_accepts_the_result_and_names_a_wrapped_row(form):
    M, N, K, m_wrap = 300, 256, 192, 203                   # 300 rows = four blocks of 64 and a ragged one; the wrap inside block 3
    out_dt, spec = GEMM_FORMS[form]
    A, W = rnd(M, K), rnd(N, K, scale=1.0 / math.sqrt(K), seed=1)
    kw = dict(N=N, K=K, epilogue=spec.get("epilogue", EPI_BIAS))
    if spec.get("bias"):
        kw["bias"] = rnd(N, dtype=F32, seed=3)
    if spec.get("gate"):
        kw["gate"] = rnd(N, dtype=F32, seed=4)
    stream = rnd(M, N, seed=5, dtype=out_dt) if spec.get("gate") else None
    tol = iw.TOL_BF16 if out_dt == BF16 else iw.TOL_WIDE
    gout = Pool("cpu")

    def run(ops):
        out = gout(M, N, dtype=out_dt, init=stream)                                # (the stream: updated in place, C aliases resid)
        ops.gemm(A, W, out, resid=out if stream is not None else None, **kw)
        return out

    tally = iw.check_gemm_rows(run(TorchOps("cpu")), A, W, tol=tol, name=form, resid=stream, block=BLOCK, **kw)
    assert tally.rows == M and tally.elements == M * N and 0.0 < tally.worst <= 1.0 and 0.0 < tally.rel < tol
    stored = run(WrappingTorchOps(("store", m_wrap)))
    assert wrong_row(lambda: iw.check_gemm_rows(stored, A, W, tol=tol, name=form, resid=stream, block=BLOCK, **kw)) == 0
    loaded = run(WrappingTorchOps(("load", m_wrap)))
    assert wrong_row(lambda: iw.check_gemm_rows(loaded, A, W, tol=tol, name=form, resid=stream, block=BLOCK, **kw)) == m_wrap
    if stream is None:                                     # the rows the wrapped store never reached still hold the poison: named as well
        assert wrong_row(lambda: iw.check_gemm_rows(stored[m_wrap:], A[m_wrap:], W, tol=tol, name=form, block=BLOCK, row0=m_wrap, **kw)) == m_wrap
    gout.check("gemm checker", written=False)


def test_gemm_checker_on_a_view_counts_from_the_views_first_row():
    M, N, K, rows = 300, 256, 192, 58
    A, W = rnd(rows, K), rnd(N, K, scale=1.0 / math.sqrt(K), seed=1)
    gout = Pool("cpu")
    out = gout(M, N, dtype=BF16)
    TorchOps("cpu").gemm(A, W, out[M - rows:], N=N, K=K)
    tally = iw.check_gemm_rows(out[M - rows:], A, W, tol=iw.TOL_BF16, name="view", N=N, K=K, block=BLOCK, row0=M - rows)
    assert tally.elements == rows * N
    assert iw.check_rows_poisoned(out[:M - rows], name="view", block=BLOCK) == M - rows
    out[M - rows + 7] = out[M - rows + 6]
    assert wrong_row(lambda: iw.check_gemm_rows(out[M - rows:], A, W, tol=iw.TOL_BF16, name="view", N=N, K=K, block=BLOCK,
                                                row0=M - rows)) == M - rows + 7
    out[131, 5] = 0.25                                                             # one element of a row no launch owns
    assert wrong_row(lambda: iw.check_rows_poisoned(out[:M - rows], name="view", block=BLOCK)) == 131
    gout.check("gemm view checker", written=False)


@pytest.mark.parametrize("kind", [F32, H16], ids=["fp32", "h16"])
def test_rmsnorm_checker_accepts_the_result_and_names_a_wrapped_row(kind):
    M, dim, m_wrap = 300, 256, 203
    x = rnd(M, dim, scale=2.0, dtype=kind)
    kw = dict(scale=rnd(dim, dtype=F32, seed=2), shift=rnd(dim, dtype=F32, seed=3))
    gout = Pool("cpu")
    run = lambda ops: ops.rmsnorm_mod(x, gout(M, dim, dtype=BF16), 1e-5, **kw)
    tally = iw.check_rmsnorm_rows(run(TorchOps("cpu")), x, 1e-5, tol=iw.TOL_BF16, name="rmsnorm", block=BLOCK, **kw)
    assert tally.rows == M and tally.elements == M * dim and 0.0 < tally.worst <= 1.0
    for mode, first in (("store", 0), ("load", m_wrap)):
        bad = run(WrappingTorchOps((mode, m_wrap)))
        assert wrong_row(lambda: iw.check_rmsnorm_rows(bad, x, 1e-5, tol=iw.TOL_BF16, name="rmsnorm", block=BLOCK, **kw)) == first
    gout.check("rmsnorm checker", written=False)


@pytest.mark.parametrize("heads,n_freq,t_offset", [(3, 21, 58), (2, 10, 0)], ids=["table_3b", "rope3d"])
def test_qknorm_checker_accepts_the_result_and_names_a_wrapped_row(heads, n_freq, t_offset):
    M, n_pos, m_wrap = 300, 40, 203
    qkv = rnd(M, 3 * heads * 128)
    g = torch.Generator().manual_seed(2)
    pos = torch.randint(0, n_pos, (M, 3), generator=g).to(torch.int16)             # (inside the table: TorchOps does not clamp)
    ang = torch.arange(n_pos + t_offset, dtype=F32)[:, None] * (10000.0 ** (-torch.arange(n_freq, dtype=F32) / n_freq))[None, :]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    wq, wk = rnd(128, dtype=F32, seed=1) + 1, rnd(128, dtype=F32, seed=2) + 1
    args = (heads, pos, t_offset, cos, sin, wq, wk, 1e-5)
    gout = Pool("cpu")
    run = lambda ops: ops.qknorm_rope(gout.like(qkv, init=qkv), *args)
    tally = iw.check_qknorm_rows(run(TorchOps("cpu")), qkv, *args, tol=iw.TOL_BF16, name="qknorm", block=BLOCK)
    assert tally.rows == M and tally.elements == qkv.numel() and 0.0 < tally.worst <= 1.0
    for mode, first in (("store", 0), ("load", m_wrap)):
        bad = run(WrappingTorchOps((mode, m_wrap)))
        assert wrong_row(lambda: iw.check_qknorm_rows(bad, qkv, *args, tol=iw.TOL_BF16, name="qknorm", block=BLOCK)) == first
    # the 58-row launch on a view: everything in front of it bit-unchanged, or the first changed row is named
    part = gout.like(qkv, init=qkv)
    TorchOps("cpu").qknorm_rope(part[M - 58:], heads, pos[M - 58:], *args[2:])
    assert iw.check_rows_equal(part[:M - 58], qkv[:M - 58], name="qknorm view", block=BLOCK) == M - 58
    iw.check_qknorm_rows(part[M - 58:], qkv[M - 58:], heads, pos[M - 58:], *args[2:], tol=iw.TOL_BF16, name="qknorm view", block=BLOCK, row0=M - 58)
    part[M - 58 - 203 % 58 - 1, 17] += 1
    assert wrong_row(lambda: iw.check_rows_equal(part[:M - 58], qkv[:M - 58], name="qknorm view", block=BLOCK)) == M - 58 - 203 % 58 - 1
    gout.check("qknorm checker", written=False)


def test_attention_checker_accepts_the_result_and_names_a_wrapped_row():
    heads, D, rows, boundary = 2, 128, 400, 203
    qkv = rnd(rows, 3 * heads * D)
    seq, cu = iw.attn_windows(rows, boundary, (41, 30, 17), txt_rows=5)
    total = seq.numel()
    out_rows = torch.randperm(total + 16, generator=torch.Generator().manual_seed(3))[:total].to(torch.int32)
    scale = 1.0 / math.sqrt(D)
    gout = Pool("cpu")
    before = torch.full((total + 16, heads * D), 7.0, dtype=BF16)

    def run(ops):
        out = gout(total + 16, heads * D, dtype=BF16, init=before)
        return ops.attn_varlen(qkv, out, seq, out_rows, cu, 46, heads, D, scale)

    kw = dict(tol=iw.TOL_ATTN, name="attn", before=before)
    tally = iw.check_attn_windows(run(TorchOps("cpu")), qkv, seq, out_rows, cu, heads, D, scale, **kw)
    assert tally.elements == total * heads * D and 0.0 < tally.worst <= 1.0
    bad = run(WrappingTorchOps(("load", boundary + 1)))                             # every row behind the line is read from the front
    with pytest.raises(AssertionError, match=r"first wrong row \d+ .*is the query at qkv row \d+"):
        iw.check_attn_windows(bad, qkv, seq, out_rows, cu, heads, D, scale, **kw)
    # window 2 reads rows below the line only: none of its video rows is wrong, every row of windows 0 and 1 is (their keys moved)
    _, _, mask = le.attn_reference(qkv, bad, seq, out_rows, cu, heads, D, scale)
    good = run(TorchOps("cpu"))
    w2 = out_rows[cu[2]:cu[3] - 5].long()
    assert not torch.equal(bad[out_rows[:cu[2]].long()], good[out_rows[:cu[2]].long()]) and bool(mask[w2].all())
    stray = run(TorchOps("cpu"))
    free = sorted(set(range(total + 16)) - set(out_rows.tolist()))
    stray[free[3], 9] = 1.0                                                        # a row no window owns
    with pytest.raises(AssertionError, match="not its own"):
        iw.check_attn_windows(stray, qkv, seq, out_rows, cu, heads, D, scale, **kw)
    gout.check("attention checker", written=False)


def test_fill_rows_is_blockwise_and_seeded():
    a = iw.fill_rows(torch.empty(150, 16, dtype=BF16), seed=5, block=BLOCK)
    b = iw.fill_rows(torch.empty(150, 16, dtype=BF16), seed=5, block=BLOCK)
    h = iw.fill_rows(torch.empty(150, 16, dtype=H16), seed=5, scale=2.0, block=BLOCK)
    assert torch.equal(a, b) and not torch.equal(a[:64], a[64:128]) and 0.5 < float(a.float().std()) < 1.5
    assert 1.5 < float(le.values(h).std()) < 2.5


def test_record_run_appends_one_line(tmp_path, monkeypatch):
    log = tmp_path / "log.txt"
    monkeypatch.setenv("SVR_INDEX_WIDTH_LOG", str(log))
    t = iw.Tally("x", 1e-3)
    t.worst, t.rel, t.rows, t.elements = 0.5, 2e-4, 3, 12
    iw.record_run("case[variant]", t, "gemm_persistent", 8.7e9, 1.25)
    fields = log.read_text().rstrip("\n").split("\t")
    assert fields[1:5] == ["case[variant]", "0.5000", "rel_err 2.000e-04 / 0.001", "gemm_persistent"] and fields[-2:] == ["peak 8.70 GB", "1.25 s"]
