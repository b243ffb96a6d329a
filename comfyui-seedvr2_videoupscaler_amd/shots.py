"""Hard cuts found on the device, so that no batch spans one: the frame signature, its distance and the rule, in plain torch.

A batch is one 3D-window-attention call and one causal VAE pass, and the 4n+1 rule packs four frames into one latent frame: a
batch that spans a cut mixes two shots inside one latent frame and one attention window, and the frames on either side ghost into
each other.  pipeline.upscale_shots and pipeline.upscale_stream(cuts=...) end batches at the cuts found here.

This module is the specification of csrc/svr_shots.hip (HipOps.frame_signatures; equal bit for bit: integer results, no tolerance)
and the path taken when ``ops`` has no ``frame_signatures`` (the fp32 torch double of the C ABI that drives the CPU tests).  Any
device.  Everything is exact integers.

Luma        ``frames`` [T, H, W, 3 | 4], fp32 or bf16, nominally in [0, 1]; a fourth channel is ignored.
                q  = frameio.codes(frames[..., :3], 255.0)        round_half_even(clamp(float(x), 0, 1) * 255); NaN -> 0, +inf -> 255,
                                                                  -inf -> 0 (frameio's rules)
                Y8 = (13933 r + 46871 g + 4732 b + 32768) >> 16   the BT.709 luma weights of frameio's "yuv420p10"; they sum to
                                                                  65536, so Y8 lies in 0..255
            white -> 255, black -> 0, pure red -> 54, pure green -> 182, pure blue -> 18.

Signature   GRID = 4, BINS = 64.  Pixel row y lies in cell row (y * 4) // H, pixel column x in cell column (x * 4) // W; the bin
            is Y8 >> 2.  ``signatures_torch(frames) -> int32 [T, 1024]``, indexed [cell_row * 4 + cell_col][bin]: the number of
            pixels of that frame with that cell and bin.  Every row sums to H * W.  T >= 1, H >= 4 and W >= 4 are required (every
            cell holds a pixel); anything else raises a ValueError that names the argument.

Distance    D[t] = sum |sig[t] - sig[t - 1]| as int64, in [0, 2 H W]; the first frame of a clip has none.  A histogram per cell
            and not per frame: a cut between two shots of the same overall brightness still moves mass between cells; bins four
            codes wide and cells a quarter of the frame: grain and slow motion move little of it.

Detector    ``Detector(percent, ratio, window, min_shot)``, four positive integers, holds
                since   frames since the last cut or the clip's start
                hist    the distances of at most ``window`` preceding non-cut frames
                prev    the previous frame's signature
            Frame t >= 1 starts a new shot iff all three hold:
                (a)  D[t] * 100 >= percent * 2 * H * W       enough of the frame changed
                (b)  D[t] >= ratio * max(hist)               and far more than this shot's own motion (an empty hist or a zero
                                                             maximum passes)
                (c)  since >= min_shot                       and the shot before it is long enough to be a batch
            On a cut hist is cleared and since becomes 1 once frame t is counted; otherwise D[t] is appended to hist, its oldest
            entry dropped beyond ``window``, and since is incremented.  The clip's first frame only sets prev and since = 1.
            ``feed(sig_chunk) -> list[int]``: the absolute frame indices that start a shot.  It reads the chunk's distances (and
            H * W, the first row's sum) back with ONE ``.tolist()`` -- the only host synchronisation of the feature.
            The rule looks backwards only, on purpose: feeding a clip chunk by chunk, in any chunking, gives exactly the cuts of
            feeding it whole, so a streamed clip is cut where the whole clip would be.

Known limits
  * A one-frame flash yields one cut (at the flash) and then mutes detection for ``window`` frames: the way back is refused by (c),
    its distance enters hist, and (b) holds every later frame against it until it leaves.
  * Two shots with the same block histograms are missed, which leaves today's behaviour (a batch across the cut).
  * Hard cuts only: a dissolve or fade spreads its distance over many frames and passes neither (a) nor (b).

DEFAULTS / ENABLED   ``DEFAULTS`` are the four parameters the command line takes when ``ENABLED`` is set (inference_cli.py reads
the switch as it reads pngenc.RUNS; there is no flag: the flag set equals the reference's).  min_shot = 5 is the smallest 4n+1
batch with more than one latent frame.  The other three come from SYNTHETIC evidence only (tests/test_shots.py: random fields
panned one pixel a frame measure 4-13 % of 2 H W at 19 x 23 and 32 x 48, a cut between disjoint luma ranges 100 %): percent = 35
lies more than twice above the pans and far below a cut, ratio = 3 asks a cut to be three times the shot's own motion where the
clips show a factor of seven and more, window = 8 remembers two latent frames of motion.  THEY HAVE NOT MET REAL FOOTAGE -- there
is no detector in the reference to compare with either -- and that is why ``ENABLED = False`` ships: turning it on waits for
someone who has measured them on real clips.  No test depends on DEFAULTS.
"""
from collections import deque
from typing import List, Sequence, Tuple

import torch

from . import frameio

GRID = 4
BINS = 64
SIG = GRID * GRID * BINS                   # 1024 counters per frame
DEFAULTS = dict(percent=35, ratio=3, window=8, min_shot=5)
ENABLED = False                            # the switch inference_cli.py reads; see the docstring before setting it


def check_frames(frames: torch.Tensor):
    """The refusals shared by the torch statement and HipOps.frame_signatures' callers, each naming its argument."""
    if frames.dim() != 4 or frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames must be [T, H, W, 3 | 4] in fp32 or bf16, got {tuple(frames.shape)} {frames.dtype}")
    T, H, W, C = frames.shape
    if C not in (3, 4):
        raise ValueError(f"frames must have C = 3 or 4 channels, got C = {C}")
    if T < 1:
        raise ValueError(f"frames must hold T >= 1 frames, got T = {T}")
    if H < GRID or W < GRID:
        raise ValueError(f"frames must have H >= {GRID} and W >= {GRID} (every cell holds a pixel), got H = {H}, W = {W}")


def luma8(frames: torch.Tensor) -> torch.Tensor:
    """Y8 of the docstring, int64 [..., H, W] from [..., H, W, >= 3]."""
    q = frameio.codes(frames[..., :3], 255.0).to(torch.int64)
    return (13933 * q[..., 0] + 46871 * q[..., 1] + 4732 * q[..., 2] + 32768) >> 16


def signatures_torch(frames: torch.Tensor) -> torch.Tensor:
    check_frames(frames)
    T, H, W, _ = frames.shape
    dev = frames.device
    row = (torch.arange(H, device=dev) * GRID) // H
    col = (torch.arange(W, device=dev) * GRID) // W
    key = (row[:, None] * GRID + col[None, :]) * BINS + (luma8(frames) >> 2)                 # [T, H, W]
    key = key + torch.arange(T, device=dev)[:, None, None] * SIG
    return torch.bincount(key.reshape(-1), minlength=T * SIG).view(T, SIG).to(torch.int32)


def signatures(frames: torch.Tensor, ops=None) -> torch.Tensor:
    """int32 [T, 1024].  ``ops.frame_signatures`` (HipOps: csrc/svr_shots.hip) where the backend has it -- a failing library raises,
    there is no fall-back from it -- else the torch statement above."""
    if ops is not None and hasattr(ops, "frame_signatures"):
        check_frames(frames)
        return ops.frame_signatures(frames)
    return signatures_torch(frames)


def distances(sig: torch.Tensor) -> torch.Tensor:
    """int64 [T - 1]: D[t] for t = 1 .. T - 1 of consecutive signatures."""
    s = sig.to(torch.int64)
    return (s[1:] - s[:-1]).abs().sum(dim=1)


class Detector:
    def __init__(self, percent: int, ratio: int, window: int, min_shot: int):
        for name, v in (("percent", percent), ("ratio", ratio), ("window", window), ("min_shot", min_shot)):
            if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        self.percent, self.ratio, self.window, self.min_shot = percent, ratio, window, min_shot
        self.since = 0                     # frames since the last cut or the clip's start
        self.hist = deque(maxlen=window)   # distances of the preceding non-cut frames
        self.prev = None                   # the previous frame's signature, int32 [1024]
        self.count = 0                     # frames fed so far = the absolute index of the next one

    def step(self, d: int, hw: int) -> bool:
        """The rule on one distance (frame t >= 1 of the clip); -> whether the frame starts a shot."""
        cut = (d * 100 >= self.percent * 2 * hw
               and (not self.hist or max(self.hist) == 0 or d >= self.ratio * max(self.hist))
               and self.since >= self.min_shot)
        if cut:
            self.hist.clear()
            self.since = 1
        else:
            self.hist.append(d)
            self.since += 1
        return cut

    def feed(self, sig_chunk: torch.Tensor) -> List[int]:
        if sig_chunk.dim() != 2 or sig_chunk.shape[1] != SIG or sig_chunk.shape[0] < 1 or sig_chunk.dtype != torch.int32:
            raise ValueError(f"sig_chunk must be int32 [t >= 1, {SIG}], got {sig_chunk.dtype} {tuple(sig_chunk.shape)}")
        first = self.prev is None
        full = sig_chunk if first else torch.cat([self.prev[None].to(sig_chunk.device), sig_chunk])
        *dist, hw = torch.cat([distances(full), sig_chunk[0].sum(dtype=torch.int64)[None]]).tolist()       # the one read-back
        cuts = []
        if first:
            self.since = 1
        for i, d in enumerate(dist):
            if self.step(d, hw):
                cuts.append(self.count + i + (1 if first else 0))
        self.prev = sig_chunk[-1].clone()
        self.count += sig_chunk.shape[0]
        return cuts


def split(total: int, cuts: Sequence[int]) -> List[Tuple[int, int]]:
    """[(a, b), ...]: the shots of a clip of ``total`` frames whose frames ``cuts`` (strictly increasing, each in 1 .. total - 1)
    start a shot."""
    if total < 1:
        raise ValueError(f"total must be at least 1, got {total}")
    cuts = [int(c) for c in cuts]
    if any(c <= 0 or c >= total for c in cuts) or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"cuts must be strictly increasing frame indices in 1 .. {total - 1}, got {cuts}")
    edges = [0] + cuts + [total]
    return list(zip(edges[:-1], edges[1:]))
