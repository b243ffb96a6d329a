"""Field matching: per stored frame, the combing of the three weaves its kept field can make is counted, the first clean weave is
taken, and only a frame with no clean weave is deinterlaced -- on the packed planes, in exact integers, stated once in plain torch.

DVD, DV and broadcast captures mix three kinds of frame inside one clip: truly interlaced video, progressive film stored as two
fields of one instant, and telecined film, where two frames in five are woven from two different film pictures.  Deinterlacing all
of them (deinterlace.py) costs every progressive frame half its vertical detail; leaving them all alone makes the model sharpen the
combs.  A weave is a copy of stored rows, so a progressive or telecined picture comes back bit for bit.

This module is the specification of the kernels in csrc/svr_fieldmatch.hip (equal bit for bit: integers in, integers out, no
tolerance) and the path taken when ``ops`` has no ``comb_counts`` / ``field_select`` (the torch double of the C ABI that drives the
CPU tests).  Any device.  Like deinterlace.py it runs BEFORE frameio_in.unpack_frames.

Formats, shapes, dtypes, ``planes()``, the ``before`` / ``after`` context and the mirror at the clip's ends (F[-1] := F[min(1, T-1)],
F[T] := F[max(T-2, 0)]) are deinterlace.py's.  p = ORDERS.index(order) is the parity of the kept (first) field: 0 for "tff".

comb counts   ``comb_counts_torch(packed, fmt, T, H, W, C, order, thr, before=None, after=None)`` -> int32 [T, 3, 2].
              Only plane 0 is read: Y for the 4:2:0 formats, the interleaved plane for rgb8 / bgr8 / rgb16: R = H rows of N samples
              with column step s (``planes(fmt, H, W, C)[0]``).
              thr' = thr << shift, shift = 0 for the 8-bit formats, 2 for yuv420p10, 8 for rgb16; thr in 0..255.  Samples are used
              as stored (a 10-bit sample above 1023 is not clamped).
              Tested rows: the r with r % 2 == 1 - p and 1 <= r <= R - 2 (rows of the OTHER field that have a kept row on either
              side).  Candidate k takes row r from X_0 = F[t] ("cur"), X_1 = F[t-1] ("prev"), X_2 = F[t+1] ("next").
              With u = F[t][r-1][i], l = F[t][r+1][i], m = X_k[r][i], sample i of row r is COMBED iff
                  m < min(u, l) - thr'   or   m > max(u, l) + thr'
              Blocks are BLOCK = 16 plane rows by 16 PIXEL columns: block row r // 16, block column (i // s) // 16.
              cnt[t][k] = (total, peak): the number of combed samples of the frame, and the largest count of any one block (at
              most 128 s: eight tested rows of 16 s samples).  A plane with R < 3 has no tested row: all counts are zero.
              Refused by name: thr outside 0..255, H * W * C > 2^31 (the counters are int32), and deinterlace.check_arguments'
              refusals for the arguments shared with it.
modes         ``modes_torch(cnt, mi, s)`` -> int32 [T], from the three peaks pc = cnt[t][0][1], pa = cnt[t][1][1], pb = cnt[t][2][1]:
                  0 (as stored)             if pc <= mi * s
                  else (q, m) = (pa, 1) if pa <= pb else (pb, 2);   m if q <= mi * s, else 3 (deinterlace)
              mi is a non-negative integer: the combed samples one block may hold per channel before the weave counts as combed.
              A stored frame that is clean is never touched; a tie between the neighbours goes to the previous frame.
select        ``select_torch(packed, deint, modes, fmt, T, H, W, C, order, before=None, after=None)`` -> T packed frames.  In EVERY
              plane (chroma row r belongs to field r % 2, as in deinterlace.py):
                  rows of parity p, and the only row of a plane with R == 1: copied from F[t];
                  the other rows: copied from F[t], F[t-1], F[t+1] for modes 0, 1, 2;
                  mode 3: the whole frame is deint[t], deint = deinterlace_torch(..., order, "frame", before, after).
front         ``field_match(packed, fmt, T, H, W, C, order, thr, mi, before=None, after=None, ops=None, out=None, stats=None)`` -> the
              progressive packed clip: deinterlace.deinterlace(..., "frame"), the counts, the modes and the select.  Through
              ``ops.comb_counts`` / ``ops.field_select`` (HipOps: csrc/svr_fieldmatch.hip) where the backend has them -- a failing
              library raises, there is no fall-back from it --, else the torch statements.  ``field_match_torch`` is the three
              statements composed, -> (frames, modes, cnt).  No host synchronisation: every frame is deinterlaced whether or not a
              mode-3 frame turns up, because finding that out would be a read-back.
stats         ``Stats(device)`` holds ONE int64 [6] tensor on the device: entries 0..3 the number of frames per mode, entries 4 and 5
              the sums of total_prev = cnt[t][1][0] and total_next = cnt[t][2][0] over the mode-3 frames.  ``field_match`` adds to it
              on the device; ``Stats.report()`` is the feature's only read-back, ONE ``.tolist()``, called once per job.
              Why the two sums: in truly interlaced motion the previous frame's other field lies one field time from the kept field
              if the order is right and three field times if it is wrong, so sum_prev < sum_next AGREES with the order that was
              used and sum_prev > sum_next CONTRADICTS it.  (A prototype of this rule on a smooth textured object moving over a
              static gradient, 12 frames: right order 188 : 340 and 1209 : 1378, wrong order 406 : 174 and 1440 : 1137.)  The line is
              informational; nothing acts on it.

``ENABLED`` is False, ``RATE`` = "match" is the rate name FrameSource takes next to deinterlace.RATES, ``DEFAULTS`` = dict(thr=10,
mi=24) are the two parameters the command line takes when ``ENABLED`` is set (inference_cli.py reads the switch as it reads
deinterlace.ENABLED; there is no flag: the flag set equals the reference's).  thr = 10 lies above the grain and the quantisation
noise of a clean 8-bit source and far below a field comb across an edge; mi = 24 asks for three combed samples in each of a
block's eight tested rows.  Both come from SYNTHETIC clips only (tests/fieldmatch_cases.py) -- THEY HAVE NOT MET REAL FOOTAGE -- and
that is why ``ENABLED = False`` ships: turning it on waits for someone who has measured them on real clips.  No test depends on
DEFAULTS.
Known limits:
  * no decimation: a telecined clip keeps its one repeated picture in five, and its frame rate -- decimate.py, the stage that runs
    after this one, drops that picture;
  * a source tagged progressive is not examined;
  * plane 0 decides for all planes;
  * noise above thr reads as combing;
  * a wrong order is reported, not corrected;
  * one order per clip; one GPU.
"""
import torch

from . import deinterlace
from .deinterlace import ORDERS, planes

BLOCK = 16
ENABLED = False
RATE = "match"
DEFAULTS = dict(thr=10, mi=24)
_SHIFT = {"rgb8": 0, "bgr8": 0, "yuv420p8": 0, "yuv420p10": 2, "rgb16": 8}


def check_arguments(packed, fmt, T, H, W, C, order, thr, before=None, after=None):
    """deinterlace.check_arguments' refusals for the shared arguments, then thr and the int32 counters; -> the packed shape."""
    shape = deinterlace.check_arguments(packed, fmt, T, H, W, C, order, "frame", before, after)
    if not isinstance(thr, int) or isinstance(thr, bool) or not 0 <= thr <= 255:
        raise ValueError(f"thr must be an integer in 0..255, got {thr!r}")
    if H * W * C > 2 ** 31:
        raise ValueError(f"H * W * C must not exceed 2^31 samples (the counters are int32), got {H} * {W} * {C}")
    return shape


def check_mi(mi):
    if not isinstance(mi, int) or isinstance(mi, bool) or not 0 <= mi < 2 ** 31:
        raise ValueError(f"mi must be a non-negative integer (below 2^31), got {mi!r}")
    return mi


def _context(packed, T, before, after):
    """-> [T + 2, frame]: F[-1] .. F[T] in the packed dtype"""
    F = packed.reshape(T, -1)
    first = before.reshape(1, -1) if before is not None else F[min(1, T - 1)][None]
    last = after.reshape(1, -1) if after is not None else F[max(T - 2, 0)][None]
    return torch.cat([first, F, last])


def comb_counts_torch(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, order: str, thr: int,
                      before: torch.Tensor = None, after: torch.Tensor = None) -> torch.Tensor:
    check_arguments(packed, fmt, T, H, W, C, order, thr, before, after)
    dev = packed.device
    cnt = torch.zeros((T, 3, 2), dtype=torch.int32, device=dev)
    _, R, N, s = planes(fmt, H, W, C)[0]
    p = ORDERS.index(order)
    if R - 1 <= 1 + p:                                                           # no tested row (R < 3; R == 3 and p == 1)
        return cnt
    r = torch.arange(1 + p, R - 1, 2, device=dev)                                # r % 2 == 1 - p, 1 <= r <= R - 2
    X = _context(packed, T, before, after)[:, :R * N].to(torch.int32).reshape(T + 2, R, N)
    cur = X[1:T + 1]
    u, l = cur[:, r - 1], cur[:, r + 1]
    t_ = thr << _SHIFT[fmt]
    lo, hi = torch.minimum(u, l) - t_, torch.maximum(u, l) + t_
    n_bc = ((N // s) + BLOCK - 1) // BLOCK
    n_blocks = ((R + BLOCK - 1) // BLOCK) * n_bc
    block = ((r // BLOCK)[:, None] * n_bc + ((torch.arange(N, device=dev) // s) // BLOCK)[None, :]).reshape(-1)
    for k, Xk in enumerate((cur, X[0:T], X[2:T + 2])):
        m = Xk[:, r]
        combed = ((m < lo) | (m > hi)).reshape(T, -1).to(torch.int32)
        per_block = torch.zeros((T, n_blocks), dtype=torch.int32, device=dev).index_add_(1, block, combed)
        cnt[:, k, 0] = per_block.sum(dim=1)
        cnt[:, k, 1] = per_block.max(dim=1).values
    return cnt


def modes_torch(cnt: torch.Tensor, mi: int, s: int) -> torch.Tensor:
    check_mi(mi)
    if cnt.dtype != torch.int32 or cnt.dim() != 3 or tuple(cnt.shape[1:]) != (3, 2):
        raise ValueError(f"cnt must be torch.int32 [T, 3, 2], got {cnt.dtype} {tuple(cnt.shape)}")
    bound = mi * s
    pc, pa, pb = (cnt[:, k, 1].to(torch.int64) for k in range(3))
    three = torch.full_like(pc, 3)
    prev = torch.where(pa <= bound, torch.ones_like(pc), three)
    nxt = torch.where(pb <= bound, torch.full_like(pc, 2), three)
    mode = torch.where(pc <= bound, torch.zeros_like(pc), torch.where(pa <= pb, prev, nxt))
    return mode.to(torch.int32)


def select_torch(packed: torch.Tensor, deint: torch.Tensor, modes: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, order: str,
                 before: torch.Tensor = None, after: torch.Tensor = None) -> torch.Tensor:
    shape = deinterlace.check_arguments(packed, fmt, T, H, W, C, order, "frame", before, after)
    if deint.dtype != packed.dtype or deint.numel() != packed.numel():
        raise ValueError(f"deint must be {packed.dtype} {tuple(shape)}, got {deint.dtype} {tuple(deint.shape)}")
    if modes.dtype != torch.int32 or tuple(modes.shape) != (T,):
        raise ValueError(f"modes must be torch.int32 {(T,)}, got {modes.dtype} {tuple(modes.shape)}")
    dev = packed.device
    X = _context(packed, T, before, after).to(torch.int32)                       # (torch has few uint16 ops: widened, as frameio_in does)
    p = ORDERS.index(order)
    kept = torch.zeros(X.shape[1], dtype=torch.bool, device=dev)                 # the samples that are F[t]'s whatever the mode
    for off, R, N, _ in planes(fmt, H, W, C):
        rows = torch.arange(R, device=dev)
        kept[off:off + R * N] = ((rows % 2 == p) | (R == 1))[:, None].expand(R, N).reshape(-1)
    m = modes.to(torch.int64)
    source = torch.arange(T, device=dev) + torch.tensor([1, 0, 2, 1], device=dev)[m]          # X's index of F[t], F[t-1], F[t+1]
    woven = torch.where(kept[None], X[1:T + 1], X[source])
    out = torch.where((m == 3)[:, None], deint.reshape(T, -1).to(torch.int32), woven)
    return out.to(packed.dtype).reshape(shape)


def field_match_torch(packed, fmt, T, H, W, C, order, thr, mi, before=None, after=None):
    """The three statements composed -> (the progressive packed clip, modes int32 [T], cnt int32 [T, 3, 2])."""
    check_mi(mi)
    cnt = comb_counts_torch(packed, fmt, T, H, W, C, order, thr, before, after)
    modes = modes_torch(cnt, mi, planes(fmt, H, W, C)[0][3])
    deint = deinterlace.deinterlace_torch(packed, fmt, T, H, W, C, order, "frame", before, after)
    return select_torch(packed, deint, modes, fmt, T, H, W, C, order, before, after), modes, cnt


class Stats:
    """What field matching did to a job's frames, kept on the device: ``counts`` int64 [6] = frames as stored, matched to the
    previous, matched to the next, deinterlaced, then the sums of total_prev and total_next over the deinterlaced frames."""

    def __init__(self, device="cpu"):
        self.counts = torch.zeros(6, dtype=torch.int64, device=device)

    def add(self, modes: torch.Tensor, cnt: torch.Tensor):
        """the torch statement of what svr_field_select adds; no host synchronisation"""
        m = modes.to(torch.int64)
        per_mode = (m[:, None] == torch.arange(4, device=m.device)[None, :]).sum(dim=0)
        sums = (cnt[:, 1:3, 0].to(torch.int64) * (m == 3)[:, None]).sum(dim=0)
        self.counts += torch.cat([per_mode, sums]).to(self.counts.device)

    def report(self):
        """-> dict(stored, prev, next, deinterlaced, sum_prev, sum_next, verdict): the ONE read-back.  verdict: what the two sums
        say about the order that was used: "agrees with" | "contradicts" | "says nothing about"."""
        stored, prev, nxt, deint, sum_prev, sum_next = self.counts.tolist()
        verdict = "agrees with" if sum_prev < sum_next else "contradicts" if sum_prev > sum_next else "says nothing about"
        return dict(stored=stored, prev=prev, next=nxt, deinterlaced=deint, sum_prev=sum_prev, sum_next=sum_next, verdict=verdict)


def field_match(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, order: str, thr: int, mi: int,
                before: torch.Tensor = None, after: torch.Tensor = None, ops=None, out: torch.Tensor = None, stats: Stats = None) -> torch.Tensor:
    """The progressive packed clip (see the module's text).  ``out``: a tensor of the packed dtype and shape; ``stats``: a Stats on
    the clip's device, added to."""
    check_mi(mi)
    if ops is not None and hasattr(ops, "comb_counts") and hasattr(ops, "field_select"):
        check_arguments(packed, fmt, T, H, W, C, order, thr, before, after)
        deint = deinterlace.deinterlace(packed, fmt, T, H, W, C, order, "frame", before=before, after=after, ops=ops)
        cnt = ops.comb_counts(packed, fmt, T, H, W, C, order, thr, before=before, after=after)
        return ops.field_select(packed, deint, cnt, fmt, T, H, W, C, order, mi, before=before, after=after, out=out,
                                stats=None if stats is None else stats.counts)
    frames, modes, cnt = field_match_torch(packed, fmt, T, H, W, C, order, thr, mi, before, after)
    if stats is not None:
        stats.add(modes, cnt)
    if out is None:
        return frames
    if out.dtype != frames.dtype or tuple(out.shape) != tuple(frames.shape):
        raise ValueError(f"out must be {frames.dtype} {tuple(frames.shape)}, got {out.dtype} {tuple(out.shape)}")
    out.copy_(frames)
    return out
