"""TEST INFRASTRUCTURE: the DiT kernels on tensors whose row offsets pass 2^32 -- the case table and the block-wise checkers of
tests/test_gpu_index_width.py (tests/test_index_width_cases.py proves both on the CPU).

Why these sizes.  BASELINE config 5 (65 frames 2160 x 3840, the 7B model: bench.py's ``cfg5``) has a token grid of 17 x 135 x 240 =
550 800 video rows + 58 text rows.  ``NaDiTEngine._forward`` allocates for the whole clip, without row chunking,

    qkv [550 858, 3 * 24 * 128 = 9 216]  = 5.08e9 elements        h1 [550 858, 4 * 3 072 = 12 288] = 6.77e9 elements

both past 2^32 ELEMENTS, and on the fp32 re-run of an overflowed h16 stream a residual stream [550 858, 3 072] fp32 of 6.8e9 BYTES.
Config 3 (the 3B model at 291 658 rows, tests/test_gpu_fullscale.py) reaches 2.24e9 elements and 2.99e9 bytes: past 2^31 elements
and 2^32 bytes of a 2-byte tensor, but a row offset formed in UNSIGNED 32 bits -- or a 32-bit product widened afterwards -- is
still exact there.  An index slip of that kind needs the crossing, not the workload, so the cases keep config 5's WIDTHS (they come
from config.DIT_7B, never from a literal) and take the smallest ragged row counts behind the line:

    LINE // 12 288 = 349 525 = LINE // (3 072 * 4)      the row in which a [., 12 288] 2-byte tensor passes element 2^32 and a
                                                        [., 3 072] fp32 tensor byte 2^32
    LINE // 9 216  = 466 033                            the same for a [., 9 216] tensor

    M12 = 352 013 = 349 525 + 2 488 rows:  row panels of 256 start at 1 365 * 256 = 349 440 (the panel the line falls into);
                                           panels 1 366 .. 1 374 (nine) lie wholly behind it, panel 1 375 is ragged (13 rows)
    M9  = 468 500 = 466 033 + 2 467 rows:  the line falls into panel 1 820; panels 1 821 .. 1 829 wholly behind, panel 1 830
                                           ragged (20 rows)

Neither is a multiple of 256 (nor of 8: rmsnorm_mod's and qknorm_rope's row groups are ragged too), and each tensor ends about
2 500 rows -- several whole GEMM row panels and a ragged one -- behind its line.  K is 192 (three K tiles of 64: the persistent
kernels' two-tiles-ahead cursor wraps across an output tile) wherever the hazard is the OUTPUT's addressing: no kernel's store
address depends on K.  Two exceptions: the case whose hazard is the row pitch of the INPUT keeps K = 12 288 (with a narrow N = 512,
two column tiles), and the fp32 stream has to pass 2^32 bytes, so it keeps N = 3 072.  The largest tensor is then 352 013 x 12 288
bf16 = 8.65 GB.

Nothing here is fitted to a kernel: the bounds are the project's own (tests/test_gpu_kernels.py: rel_err <= 2.5e-3 behind a bf16
store, <= 1e-3 behind an fp32 / h16 store, <= 4e-3 behind attention; and the per-element bounds tests/local_error.py derives from
unit roundoffs), and the sizes are the arithmetic above.

The checkers walk a tensor in row blocks of at most BLOCK_ROWS rows -- the fp64 temporaries of a block are 1.6 GB each, an fp32
or fp64 copy of a whole tensor is never made -- and put EVERY row through local_error's reference of the op: per element against
its derived bound (local_error.check) and per block against the rel_err bound.  A failure names the first wrong row of the whole
tensor.  Each returns a Tally whose ``elements`` the caller compares with the tensor's size: no element is left out.

Imports torch only; any device."""
import dataclasses
import os

import torch

import local_error as le
from guarded_out import POISON
from ops_reference import H16, H16_SCALE

LINE = 2 ** 32
TXT_ROWS = 58                     # rows of the text stream (weights.synth_text_embedding; the engine appends them to every window)
BLOCK_ROWS = 16384
PANEL = 256                       # rows of a GEMM output tile (csrc/svr_gemm.hip: W4_T, BM)
M12, M9 = 352013, 468500
TOL_BF16, TOL_WIDE, TOL_ATTN = 2.5e-3, 1e-3, 4e-3
CLIPS = {"cfg3": ("DIT_3B", 33, 2160, 3840), "cfg5": ("DIT_7B", 65, 2160, 3840)}      # bench.py WORKLOADS: frames, height, width


def token_grid(frames, height, width):
    """(t, h, w) of the DiT's rows: the VAE's causal 4x temporal and 8x spatial compression, then 1 x 2 x 2 patches."""
    return (frames - 1) // 4 + 1, height // 8 // 2, width // 8 // 2


def dit_tensors(cfg, grid, txt_rows=TXT_ROWS):
    """name -> (rows, columns, bytes per element) of the tensors NaDiTEngine._forward allocates over all R rows of a clip."""
    t, h, w = grid
    R = t * h * w + txt_rows
    inner = cfg.heads * cfg.head_dim
    return {"hid_fp32": (R, cfg.vid_dim, 4), "hid_h16": (R, cfg.vid_dim, 2), "xn": (R, cfg.vid_dim, 2), "qkv": (R, 3 * inner, 2),
            "att": (R, inner, 2), "h1": (R, cfg.mlp_hidden, 2)}


def widths(cfg):
    """the three row widths of the cases, from the model config"""
    return {"qkv": 3 * cfg.heads * cfg.head_dim, "h1": cfg.mlp_hidden, "hid": cfg.vid_dim}


def line_row(width, elem_bytes=1):
    """the row of a dense [., width] tensor in which element (elem_bytes = 1) or byte offset 2^32 falls"""
    return LINE // (width * elem_bytes)


@dataclasses.dataclass(frozen=True)
class Case:
    """One case of tests/test_gpu_index_width.py.  ``tensor``: the operand behind the line, [rows, width] of ``elem_bytes`` bytes;
    ``line``: what it passes -- "elements" (2^32 elements) or "bytes" (2^32 bytes); ``view_rows`` > 0: the launch works on the
    last ``view_rows`` rows only, so it is the view's BASE that has to lie behind the line; ``width_of``: the config-derived
    width (widths()).  N, K: the GEMM's; ``variants``: what the test is parametrised over."""
    name: str
    op: str
    tensor: str
    rows: int
    width: int
    elem_bytes: int
    line: str
    width_of: str
    N: int = 0
    K: int = 0
    view_rows: int = 0
    variants: tuple = ()

    def offset_of_last_launch_row(self):
        """offset (in the unit of ``line``) of the first row the launch touches last: the tensor's end, or the view's base"""
        rows = self.rows - self.view_rows if self.view_rows else self.rows
        return rows * self.width * (self.elem_bytes if self.line == "bytes" else 1)


def cases(cfg):
    """The table, for the 7B config ``cfg`` (config.DIT_7B).  The h16 variants of the two stream cases run the same rows on the
    2-byte stream (2.16e9 bytes: past 2^31 bytes only) -- they share the fp32 kind's addressing code and its instances differ; the
    line a case NAMES is the one its first variant passes."""
    w = widths(cfg)
    return (
        Case("gemm_out_qkv", "gemm", "C", M9, w["qkv"], 2, "elements", "qkv", N=w["qkv"], K=192, variants=("w4r", "w4q", "gemm_kernel")),
        Case("gemm_out_mlp_in", "gemm", "C", M12, w["h1"], 2, "elements", "h1", N=w["h1"], K=192, variants=("w4r", "w4q", "gemm_kernel")),
        Case("gemm_in_mlp_out", "gemm", "A", M12, w["h1"], 2, "elements", "h1", N=512, K=w["h1"], variants=("w4r", "w4q")),
        Case("gemm_stream", "gemm", "C = resid", M12, w["hid"], 4, "bytes", "hid", N=w["hid"], K=192, variants=("fp32", "h16")),
        Case("gemm_view", "gemm", "C", M9, w["qkv"], 2, "elements", "qkv", N=w["qkv"], K=192, view_rows=TXT_ROWS),
        Case("rmsnorm_mod", "rmsnorm_mod", "x", M12, w["hid"], 4, "bytes", "hid", variants=("fp32", "h16")),
        Case("qknorm_rope", "qknorm_rope", "qkv", M9, w["qkv"], 2, "elements", "qkv", variants=("table_3b", "rope3d")),
        Case("qknorm_rope_view", "qknorm_rope", "qkv", M9, w["qkv"], 2, "elements", "qkv", view_rows=TXT_ROWS),
        Case("attn_varlen", "attn_varlen", "qkv", M9, w["qkv"], 2, "elements", "qkv", variants=("first_generation", "window")),
    )


def case(cfg, name):
    return {c.name: c for c in cases(cfg)}[name]


# window lengths of the two attention launches (video rows of the three windows; every window then takes the TXT_ROWS last rows):
# 2 083 + 58 > 2 048 rows sends the whole launch to the first-generation kernel, as config 5's windows do; 2 048 / 1 215 / 77 rows
# INCLUDING the text rows is the longest launch the window kernel's row table takes
ATTN_LENS = {"first_generation": (2083, 2083, 641), "window": (2048 - TXT_ROWS, 1215 - TXT_ROWS, 77 - TXT_ROWS)}
AW_MAXL = 2048                    # csrc/svr_attn_win.hip


def attn_windows(rows, boundary, lens, txt_rows=TXT_ROWS, seed=1):
    """seq_rows / cu (int32, CPU) of three windows over a [rows, .] qkv whose line falls into row ``boundary``: window 0 draws its
    video rows only from BEHIND the boundary row, window 1 alternates rows below and behind it, window 2 only from below; each is
    followed by the last ``txt_rows`` rows, as the engine appends its text rows.  No row repeats inside a window."""
    g = torch.Generator().manual_seed(seed)
    n_vid = rows - txt_rows
    behind = lambda n: boundary + 1 + torch.randperm(n_vid - boundary - 1, generator=g)[:n]
    below = lambda n: torch.randperm(boundary, generator=g)[:n]
    txt = torch.arange(n_vid, rows)
    L0, L1, L2 = lens
    assert n_vid - boundary - 1 >= L0, "not enough rows behind the line for window 0"
    mixed = torch.empty(L1, dtype=torch.long)             # below, behind, below, behind, ... (odd L1: one more from below)
    mixed[0::2], mixed[1::2] = below(L1 - L1 // 2), behind(L1 // 2)
    parts = [behind(L0), txt, mixed, txt, below(L2), txt]
    cu = torch.tensor([0, L0 + txt_rows, L0 + L1 + 2 * txt_rows, L0 + L1 + L2 + 3 * txt_rows], dtype=torch.int32)
    return torch.cat(parts).to(torch.int32), cu


# ------------------------------------------------------------------------------------------------ inputs, in row blocks
def fill_rows(t, seed, scale=1.0, block=BLOCK_ROWS):
    """seeded N(0, scale^2) into the [rows, cols] tensor ``t`` (bf16, fp32 or h16: the half holds x * 2^-6), a row block at a time"""
    g = torch.Generator(device=t.device).manual_seed(seed)
    for r0 in range(0, t.shape[0], block):
        r1 = min(r0 + block, t.shape[0])
        v = torch.randn(r1 - r0, t.shape[1], generator=g, device=t.device) * scale
        t[r0:r1] = (v * H16_SCALE).to(H16) if t.dtype == H16 else v.to(t.dtype)
    return t


# ------------------------------------------------------------------------------------------------ the block-wise checkers
class Tally:
    """What a block-wise checker saw: worst |err| / bound, worst rel_err of a block, rows and elements compared."""

    def __init__(self, name, tol):
        self.name, self.tol = name, tol
        self.worst, self.rel, self.rows, self.elements = 0.0, 0.0, 0, 0


def _first_row(bad_rows, r0):
    return r0 + int(bad_rows.nonzero()[0])


def _block(tally, r0, got, want, bound, mask=None, before=None):
    """one block of rows r0 .. r0 + len(got): every element against its bound (local_error.check), the block against tally.tol"""
    rows = got.shape[0]
    tag = f"{tally.name} rows {r0}..{r0 + rows}"
    try:
        worst = le.check(tag, got, want, bound, mask, before)
    except AssertionError as e:
        _, ratio = le.worst_ratio(got, want, bound, mask)
        bad = (ratio.reshape(rows, -1) > 1.0).any(dim=1)
        if not bool(bad.any()):                           # (a stray write outside the mask: local_error.check's own message)
            raise
        raise AssertionError(f"{tally.name}: first wrong row {_first_row(bad, r0)} ({int(bad.sum())} wrong rows among rows "
                             f"{r0}..{r0 + rows}); {e}") from None
    diff = le.values(got).reshape(want.shape) - want
    ref = want
    if mask is not None:
        diff, ref = torch.where(mask, diff, torch.zeros_like(diff)), torch.where(mask, want, torch.zeros_like(want))
    rel = float(diff.norm() / ref.norm().clamp_min(1e-30))
    assert rel < tally.tol, f"{tag}: rel_err {rel:.3e} is not below {tally.tol}"
    tally.worst, tally.rel = max(tally.worst, worst), max(tally.rel, rel)
    tally.rows += rows
    tally.elements += int(mask.sum()) if mask is not None else got.numel()
    return tally


def _blocks(rows, block):
    return [(r0, min(r0 + block, rows)) for r0 in range(0, rows, block)]


def check_gemm_rows(got, A, W, *, tol, name, resid=None, block=BLOCK_ROWS, row0=0, **kw):
    """Every row of ``got`` [M, N] = the plain GEMM ``gemm(A, W, got, **kw)`` wrote (keywords as HipOps.gemm: N, K, bias, epilogue,
    gate), against local_error.gemm_reference on the same rows of A.  ``resid``: the residual AS IT WAS BEFORE an in-place launch
    (the ``before=`` copy of the stream), taken in the same blocks.  ``row0``: the number the first row has in messages."""
    tally = Tally(name, tol)
    assert got.dim() == 2 and A.shape[0] == got.shape[0] and (resid is None or resid.shape[0] == got.shape[0])
    for r0, r1 in _blocks(got.shape[0], block):
        want, bound, _ = le.gemm_reference(A[r0:r1], W, got[r0:r1], resid=None if resid is None else resid[r0:r1], **kw)
        _block(tally, row0 + r0, got[r0:r1], want, bound)
    return tally


def check_rmsnorm_rows(got, x, eps, *, tol, name, w=None, scale=None, shift=None, block=BLOCK_ROWS):
    """every row of ``got`` = rmsnorm_mod(x) against local_error.rmsnorm_mod_reference"""
    tally = Tally(name, tol)
    assert got.shape == x.shape
    for r0, r1 in _blocks(got.shape[0], block):
        want, bound = le.rmsnorm_mod_reference(x[r0:r1], eps, w, scale, shift, got.dtype)
        _block(tally, r0, got[r0:r1], want, bound)
    return tally


def check_qknorm_rows(got, before, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps, *, tol, name, block=BLOCK_ROWS, row0=0):
    """every row of ``got`` = qknorm_rope in place on ``before``: q and k against local_error.qknorm_rope_reference, the V third
    bit-equal to ``before`` (tally.elements counts all three thirds)."""
    tally = Tally(name, tol)
    n = 2 * heads * 128
    assert got.shape == before.shape and pos.shape[0] == got.shape[0]
    for r0, r1 in _blocks(got.shape[0], block):
        v_diff = (got[r0:r1, n:] != before[r0:r1, n:]).any(dim=1)
        assert not bool(v_diff.any()), f"{name}: V columns were written; first wrong row {_first_row(v_diff, row0 + r0)}"
        want, bound = le.qknorm_rope_reference(before[r0:r1], heads, pos[r0:r1], t_offset, cos_tab, sin_tab, wq, wk, eps)
        _block(tally, row0 + r0, got[r0:r1, :n], want, bound)
        tally.elements += (r1 - r0) * (got.shape[1] - n)
    return tally


def _raw(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_rows_equal(got, want, *, name, block=BLOCK_ROWS, row0=0):
    """``got`` holds the BITS of ``want``, row block by row block; a failure names the first differing row.  -> rows compared"""
    assert got.shape == want.shape and got.dtype == want.dtype
    for r0, r1 in _blocks(got.shape[0], block):
        diff = (_raw(got[r0:r1]) != _raw(want[r0:r1])).reshape(r1 - r0, -1).any(dim=1)
        assert not bool(diff.any()), f"{name}: {int(diff.sum())} rows among rows {row0 + r0}..{row0 + r1} differ; first wrong row {_first_row(diff, row0 + r0)}"
    return got.shape[0]


def check_rows_poisoned(t, *, name, block=BLOCK_ROWS):
    """every element of ``t`` (rows of a guarded_out payload that no launch may have touched) still holds the poison pattern"""
    view, pattern = POISON[t.dtype]
    for r0, r1 in _blocks(t.shape[0], block):
        hit = (t[r0:r1].view(view) != pattern).reshape(r1 - r0, -1).any(dim=1)
        assert not bool(hit.any()), f"{name}: {int(hit.sum())} rows among rows {r0}..{r1} were written; first wrong row {_first_row(hit, r0)}"
    return t.shape[0]


def check_attn_windows(got, qkv, seq_rows, out_rows, cu, heads, head_dim, scale, *, tol, name, before=None):
    """``got`` = attn_varlen's output [rows', heads * head_dim] against local_error.attn_reference.  The reference reads the qkv
    rows the windows name -- gathered once with torch into a compact tensor (``qkv`` as a whole is never converted) -- and every
    row of ``got`` no window owns must hold the bits of ``before``.  A failure names the first wrong OUTPUT row and the qkv row it
    was computed from."""
    tally = Tally(name, tol)
    used, compact_rows = torch.unique(seq_rows.long(), return_inverse=True)
    want, bound, mask = le.attn_reference(qkv[used], got, compact_rows.to(torch.int32), out_rows, cu, heads, head_dim, scale)
    try:
        _block(tally, 0, got, want, bound, mask, before)
    except AssertionError as e:
        _, ratio = le.worst_ratio(got, want, bound, mask)
        bad = (ratio > 1.0).any(dim=1)
        if not bool(bad.any()):
            raise
        o = int(bad.nonzero()[0])
        src = seq_rows[(out_rows.long() == o).nonzero()[0]]
        raise AssertionError(f"{e} [output row {o} is the query at qkv row {int(src)}]") from None
    assert tally.elements == seq_rows.numel() * heads * head_dim
    return tally


# ------------------------------------------------------------------------------------------------ the record of a run
def record_run(case_name, tally, kernel, peak_bytes, seconds):
    """One line per case and variant -- worst err / bound, worst block rel_err against its bound, the kernel class that served the
    launch, peak device memory, wall time -- printed, and appended to the file SVR_INDEX_WIDTH_LOG names (profiles/index_width.txt
    is made from such a log: a record, never an input to a tolerance)."""
    tid = os.environ.get("PYTEST_CURRENT_TEST", "-").split(" ")[0]
    line = (f"{tid}\t{case_name}\t{tally.worst:.4f}\trel_err {tally.rel:.3e} / {tally.tol:g}\t{kernel}\t"
            f"{tally.rows} rows {tally.elements} elements\tpeak {peak_bytes / 1e9:.2f} GB\t{seconds:.2f} s")
    print(f"[index_width] {line}")
    log = os.environ.get("SVR_INDEX_WIDTH_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
