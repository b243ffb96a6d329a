"""Decimation: of every five frames of a 3:2 telecined clip the one that repeats its predecessor is dropped -- on the packed planes,
in exact integers, stated once in plain torch.

Field matching (fieldmatch.py) gives a telecined clip's film pictures back bit for bit, but four pictures still occupy five frames:
one picture in every cycle is shown twice, the motion stutters and the model is paid for a frame that holds nothing new.  This
module measures, per frame, how much it differs from the frame before it, drops the frame of each cycle of five that differs
least and keeps the other four in their order: 4/5 of the frames, at 4/5 of the frame rate.

This module is the specification of the kernels in csrc/svr_decimate.hip (equal bit for bit: integers in, integers out, no
tolerance) and the path taken when ``ops`` has no ``frame_diffs`` / ``decimate_select`` (the torch double of the C ABI that drives
the CPU tests).  Any device.  It runs AFTER field matching and BEFORE frameio_in.unpack_frames.

Formats, shapes, dtypes and ``planes()`` are deinterlace.py's.  T frames F[0..T-1] come in -- normally field matching's output --;
``before`` is the frame ahead of F[0], or None at the clip's start.

diffs         ``diffs_torch(packed, fmt, T, H, W, C, before=None)`` -> int32 [T].
              Only plane 0 is read: Y for the 4:2:0 formats, the interleaved plane for rgb8 / bgr8 / rgb16: R = H rows of N samples
              with column step s (``planes(fmt, H, W, C)[0]``).  Samples are used as stored.
              Blocks are BLOCK = 32 plane rows by 32 PIXEL columns: block row r // 32, block column (i // s) // 32; the blocks at
              the right and the bottom edge are partial.
              diff[t] = the largest, over the blocks, of the block's sum of |F[t][r][i] - F[t-1][r][i]|.  A block sum is at most
              32 * 32 * 4 * 65535 < 2^31: int32 holds it.
              diff[0] compares F[0] with ``before``.  Without ``before`` diff[0] = 2^31 - 1 (``FIRST``): the clip's first frame is
              never the repeated one while any other frame of its cycle is smaller.
              No mirror and no ``after``: diff[t] depends on frames t - 1 and t only, which is what makes any split of a clip, each
              part with its true ``before``, equal the whole.
drops         ``drops_torch(diff)`` -> int32 [T // 5]: per WHOLE cycle c the position 0..4 of the smallest of diff[5c .. 5c + 4].
              A tie goes to the FIRST position.
select        ``select_torch(packed, drops, fmt, T, H, W, C)`` -> T - T // 5 packed frames: every whole cycle loses the frame its
              drop names and keeps the others in their order; the T % 5 frames of a trailing partial cycle are copied; T < 5 is a
              copy.
front         ``decimate(packed, fmt, T, H, W, C, dup, before=None, ops=None, out=None, stats=None)`` -> the decimated packed clip.
              Through ``ops.frame_diffs`` / ``ops.decimate_select`` (HipOps: csrc/svr_decimate.hip) where the backend has both -- a
              failing library raises, there is no fall-back from it --, else the torch statements.  ``decimate_torch`` is the three
              statements composed, -> (frames, drops, diff).  No host synchronisation.
stats         ``Stats(device)`` holds ONE int64 [6] tensor on the device: entries 0..4 the number of cycles whose drop was at that
              position, entry 5 the number of dropped frames with diff > bound, bound = dup * s << shift (shift as in fieldmatch.py:
              0 for the 8-bit formats, 2 for yuv420p10, 8 for rgb16).  ``dup`` is the block difference PER CHANNEL, in 8-bit
              codes, up to which a frame counts as a repeat: an integer in 0..2^18.  ``add(drops, diff, dup, s, shift)`` is the
              torch statement of what the select kernel adds; ``report()`` is the feature's only read-back, ONE ``.tolist()``,
              called once per job -> dict(cycles, positions, not_duplicates).
              Entry 5 is informational only: a frame is dropped in EVERY whole cycle whatever ``dup`` says, because the writer's
              frame rate is constant.  A clip that was not telecined therefore shows as not_duplicates ~ cycles.

``ENABLED`` is False, ``RATE`` = "decimate" is the rate name FrameSource takes next to deinterlace.RATES and fieldmatch.RATE,
``CYCLE`` = 5, ``DEFAULTS`` = dict(dup=1024) -- one code per pixel over a full block -- is the parameter the command line takes when
``ENABLED`` is set (inference_cli.py reads the switch as it reads fieldmatch.ENABLED, over which it takes precedence; there is no
flag: the flag set equals the reference's).  DEFAULTS comes from SYNTHETIC clips only (tests/fieldmatch_cases.py: the duplicate's
difference is exactly 0 there, its neighbours' are in the thousands) -- IT HAS NOT MET REAL FOOTAGE -- and that is why
``ENABLED = False`` ships: turning it on waits for someone who has measured it on real clips.  No test depends on DEFAULTS.
Known limits:
  * 3:2 cycles of five only;
  * one drop per cycle, duplicate or not;
  * plane 0 decides;
  * cycles are counted from the first frame kept after --skip_first_frames;
  * a trailing partial cycle is kept whole, so the video can outlast copied audio by up to 4 / (5 fps) s;
  * no scene-change handling;
  * a source tagged progressive is not examined;
  * one GPU.
"""
import torch

from . import deinterlace, fieldmatch
from .deinterlace import planes

BLOCK = 32
CYCLE = 5
ENABLED = False
RATE = "decimate"
DEFAULTS = dict(dup=1024)
FIRST = 2 ** 31 - 1                                   # diff[0] of a clip without ``before``
DUP_MAX = 2 ** 18
_SHIFT = fieldmatch._SHIFT


def check_dup(dup):
    if not isinstance(dup, int) or isinstance(dup, bool) or not 0 <= dup <= DUP_MAX:
        raise ValueError(f"dup must be an integer in 0..{DUP_MAX}, got {dup!r}")
    return dup


def check_arguments(packed, fmt, T, H, W, C, dup=0, before=None, out=None):
    """deinterlace.check_arguments' refusals for the shared arguments, then dup and ``out``; -> the packed shape of the T frames."""
    shape = deinterlace.check_arguments(packed, fmt, T, H, W, C, "tff", "frame", before, None)
    check_dup(dup)
    if out is not None:
        want = (T - T // CYCLE,) + tuple(shape[1:])
        if out.dtype != packed.dtype or tuple(out.shape) != want:
            raise ValueError(f"out must be {packed.dtype} {want}, got {out.dtype} {tuple(out.shape)}")
    return shape


def _check_diff(diff, T):
    if diff.dtype != torch.int32 or tuple(diff.shape) != (T,):
        raise ValueError(f"diff must be torch.int32 {(T,)}, got {diff.dtype} {tuple(diff.shape)}")


def diffs_torch(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, before: torch.Tensor = None) -> torch.Tensor:
    check_arguments(packed, fmt, T, H, W, C, before=before)
    dev = packed.device
    _, R, N, s = planes(fmt, H, W, C)[0]
    F = packed.reshape(T, -1)[:, :R * N].to(torch.int32)                         # (torch has few uint16 ops: widened, as frameio_in does)
    diff = torch.full((T,), FIRST, dtype=torch.int32, device=dev)
    if before is not None:
        F = torch.cat([before.reshape(1, -1)[:, :R * N].to(torch.int32), F])
    if F.shape[0] < 2:
        return diff
    n_bc = ((N // s) + BLOCK - 1) // BLOCK
    n_blocks = ((R + BLOCK - 1) // BLOCK) * n_bc
    block = ((torch.arange(R, device=dev) // BLOCK)[:, None] * n_bc + ((torch.arange(N, device=dev) // s) // BLOCK)[None, :]).reshape(-1)
    delta = (F[1:] - F[:-1]).abs()
    sums = torch.zeros((delta.shape[0], n_blocks), dtype=torch.int32, device=dev).index_add_(1, block, delta)
    diff[T - delta.shape[0]:] = sums.max(dim=1).values
    return diff


def drops_torch(diff: torch.Tensor) -> torch.Tensor:
    if diff.dtype != torch.int32 or diff.dim() != 1:
        raise ValueError(f"diff must be torch.int32 [T], got {diff.dtype} {tuple(diff.shape)}")
    n = diff.shape[0] // CYCLE
    d = diff[:n * CYCLE].reshape(n, CYCLE)
    position = torch.arange(CYCLE, device=diff.device)[None, :].expand(n, CYCLE)
    smallest = d == d.min(dim=1, keepdim=True).values
    return torch.where(smallest, position, torch.full_like(position, CYCLE)).min(dim=1).values.to(torch.int32)    # the FIRST of a tie


def _sources(drops, T):
    """int64 [T - T // 5]: the input frame every output frame is a copy of"""
    n = T // CYCLE
    o = torch.arange(T - n, device=drops.device)
    c = torch.clamp(o // (CYCLE - 1), max=max(n - 1, 0))
    j = o % (CYCLE - 1)
    d = drops.to(torch.int64)[c] if n else torch.zeros_like(o)
    return torch.where(o < (CYCLE - 1) * n, CYCLE * c + j + (j >= d).to(torch.int64), o + n)


def select_torch(packed: torch.Tensor, drops: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int) -> torch.Tensor:
    shape = check_arguments(packed, fmt, T, H, W, C)
    if drops.dtype != torch.int32 or tuple(drops.shape) != (T // CYCLE,):
        raise ValueError(f"drops must be torch.int32 {(T // CYCLE,)}, got {drops.dtype} {tuple(drops.shape)}")
    return packed.reshape((T,) + tuple(shape[1:]))[_sources(drops, T)].contiguous()


def decimate_torch(packed, fmt, T, H, W, C, before=None):
    """The three statements composed -> (the decimated packed clip, drops int32 [T // 5], diff int32 [T])."""
    diff = diffs_torch(packed, fmt, T, H, W, C, before)
    drops = drops_torch(diff)
    return select_torch(packed, drops, fmt, T, H, W, C), drops, diff


class Stats:
    """What decimation did to a job's cycles, kept on the device: ``counts`` int64 [6] = the cycles whose drop was at position 0, 1,
    2, 3, 4, then the dropped frames whose diff lay above the bound (frames that were no repeats)."""

    def __init__(self, device="cpu"):
        self.counts = torch.zeros(6, dtype=torch.int64, device=device)

    def add(self, drops: torch.Tensor, diff: torch.Tensor, dup: int, s: int, shift: int):
        """the torch statement of what svr_decimate_select adds; no host synchronisation"""
        check_dup(dup)
        n = drops.shape[0]
        d = drops.to(torch.int64)
        per_position = (d[:, None] == torch.arange(CYCLE, device=d.device)[None, :]).sum(dim=0)
        dropped = diff[:n * CYCLE].reshape(n, CYCLE).to(torch.int64).gather(1, d[:, None])[:, 0]
        over = (dropped > (dup * s << shift)).sum().reshape(1)
        self.counts += torch.cat([per_position, over]).to(self.counts.device)

    def report(self):
        """-> dict(cycles, positions, not_duplicates): the ONE read-back"""
        counts = self.counts.tolist()
        return dict(cycles=sum(counts[:CYCLE]), positions=counts[:CYCLE], not_duplicates=counts[CYCLE])


def decimate(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, dup: int, before: torch.Tensor = None, ops=None,
             out: torch.Tensor = None, stats: Stats = None) -> torch.Tensor:
    """The decimated packed clip, T - T // 5 frames (see the module's text).  ``out``: a tensor of the packed dtype and that shape;
    ``stats``: a Stats on the clip's device, added to."""
    check_arguments(packed, fmt, T, H, W, C, dup, before, out)
    if ops is not None and hasattr(ops, "frame_diffs") and hasattr(ops, "decimate_select"):
        diff = ops.frame_diffs(packed, fmt, T, H, W, C, before=before)
        return ops.decimate_select(packed, diff, fmt, T, H, W, C, dup, out=out, stats=None if stats is None else stats.counts)
    frames, drops, diff = decimate_torch(packed, fmt, T, H, W, C, before)
    if stats is not None:
        stats.add(drops, diff, dup, planes(fmt, H, W, C)[0][3], _SHIFT[fmt])
    if out is None:
        return frames
    out.copy_(frames)
    return out
