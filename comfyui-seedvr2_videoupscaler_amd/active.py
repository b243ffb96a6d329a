"""The active picture area of a letterboxed or pillarboxed clip, found on the device, so that only the picture is upscaled: the
profile, the rule and the output rectangle, in plain torch and plain integers.

A 2.39:1 film in a 16:9 container is a quarter black bars, and so is 4:3 material in 16:9.  Encode, DiT and decode scale with
the pixel count, so the engine spends that quarter on flat black; the antialiased bicubic of the input transform rings across the
hard bar edge into the picture, and the colour-correction statistics are taken over pixels that are not picture.
pipeline.upscale(area=...) crops to the area found here, upscales the picture alone and puts it into a plain resize of the frame.

This module is the specification of csrc/svr_active.hip (HipOps.active_profile; equal bit for bit: integer results, no tolerance)
and the path taken when ``ops`` has no ``active_profile`` (the fp32 torch double of the C ABI that drives the CPU tests).  Any
device.  Everything is exact integers.

Profile     ``frames`` [T, H, W, 3 | 4], fp32 or bf16, nominally in [0, 1]; a fourth channel is ignored.  Y8 = shots.luma8(frames):
            frameio.codes(., 255.0) per channel (NaN -> 0, +inf -> 255, -inf -> 0), then the BT.709 weights; a grey pixel k / 255
            has Y8 == k exactly.  ``profile_torch(frames, dark) -> int32 [H + W]``: entry y < H is the number of pixels (t, x) of
            row y with Y8 > dark over ALL frames, entry H + x the same for column x; both halves have the same sum.  ``dark`` is
            an integer in 0..255 (255 counts nothing).  T, H, W >= 1 and T * max(H, W) < 2^31 (the counters are int32) are
            required; anything else raises a ValueError that names the argument.

Rule        ``Rule(dark, specks, skew, margin, gain)``, five non-negative integers, stateless.
            ``area(profile, T, H, W) -> (y0, y1, x0, x1)`` in input pixels, from the profile as a list of H + W integers:
              1. a row is DARK iff count * 1_000_000 <= specks * T * W (a column: T * H): ``specks`` is the share of a line, in
                 parts per million, that may be brighter than ``dark`` -- compression noise, a dead pixel -- without the line
                 counting as picture;
              2. top, bottom, left, right: the lengths of the leading and trailing runs of dark lines; a dark line inside the
                 picture means nothing;
              3. top + bottom >= H or left + right >= W: the full frame (a black or faded-out clip; there is nothing to find);
              4. per axis on its own, abs(top - bottom) > skew sets both to 0, likewise left and right: bars are symmetric, a dark
                 sky is not;
              5. ``margin`` lines of each bar stay with the picture: y0 = max(top - margin, 0), y1 = min(H - bottom + margin, H),
                 the columns likewise (a soft bar edge, and room for the resize kernel's support);
              6. a picture under 16 lines or columns: the full frame;
              7. (H W - area) * 100 < gain * H W: the full frame -- a second resize is not worth a sliver.
            The full frame is (0, H, 0, W).

Rectangle   ``out_rect(area, H, W, TH, TW) -> (oy0, oy1, ox0, ox1)`` for the output size (TH, TW) = transforms.true_target_dims(...),
            both even:  oy0 = 2 * ((y0 * TH) // (2 * H)),  oy1 = min(TH, 2 * -((-y1 * TH) // (2 * H))),  the columns likewise: the
            even rectangle that contains the scaled area, each edge less than 2 output pixels from its exact place, the whole
            output for the whole frame.  The crop is resized to exactly this rectangle: a scale error of under 2 pixels per side
            is the stated price of even sizes.

Known limits
  * Dark bars only: coloured or blurred-fill bars are picture to the rule.
  * A subtitle, a logo or one bright pixel (specks = 0) in a bar keeps that bar for that call, which is safe: the call is then
    today's, or crops less.
  * A Rule sees one call's frames: neighbouring chunks of a stream, or neighbouring shots, may choose different areas.
  * One GPU only; the ComfyUI node is untouched.

DEFAULTS / ENABLED   ``DEFAULTS`` are the five parameters the command line takes when ``ENABLED`` is set (inference_cli.py reads
the switch as it reads shots.ENABLED; there is no flag: the flag set equals the reference's).  They come from SYNTHETIC evidence
only (tests/test_active.py: exact black bars around random fields): dark = 8 is half of video black (code 16) and above the codes
a lossy encoder leaves in a bar, specks = 0 lets one bright pixel keep its bar, skew = 4 allows an odd bar height and an
off-by-a-few authoring error and no more, margin = 2 keeps the bar edge out of the crop's border, gain = 6 asks for a saving that
pays for the second resize.  The rule is conservative on purpose: a miss costs time, a false hit costs picture.  THEY HAVE NOT MET
REAL FOOTAGE -- there is nothing in the reference to compare with either -- and that is why ``ENABLED = False`` ships: turning it
on waits for someone who has run it over real clips.  No test depends on DEFAULTS.
"""
from typing import List, Sequence, Tuple

import torch

from . import shots

DEFAULTS = dict(dark=8, specks=0, skew=4, margin=2, gain=6)
ENABLED = False                            # the switch inference_cli.py reads; see the docstring before setting it
MIN_SIDE = 16                              # a picture smaller than this is not cropped to (rule 6; upscale's area= asks the same)


def check_frames(frames: torch.Tensor):
    """The refusals shared by the torch statement and HipOps.active_profile's callers, each naming its argument."""
    if frames.dim() != 4 or frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames must be [T, H, W, 3 | 4] in fp32 or bf16, got {tuple(frames.shape)} {frames.dtype}")
    T, H, W, C = frames.shape
    if C not in (3, 4):
        raise ValueError(f"frames must have C = 3 or 4 channels, got C = {C}")
    if T < 1 or H < 1 or W < 1:
        raise ValueError(f"frames must hold T >= 1 frames of H >= 1 rows and W >= 1 columns, got T = {T}, H = {H}, W = {W}")
    if T * max(H, W) >= 1 << 31:
        raise ValueError(f"frames of T * max(H, W) = {T * max(H, W)}; the int32 counters hold fewer than 2^31")


def check_dark(dark):
    if isinstance(dark, bool) or not isinstance(dark, int) or not 0 <= dark <= 255:
        raise ValueError(f"dark must be an integer in 0..255, got {dark!r}")


def profile_torch(frames: torch.Tensor, dark: int) -> torch.Tensor:
    check_frames(frames)
    check_dark(dark)
    lit = shots.luma8(frames) > dark                                                         # [T, H, W]
    return torch.cat([lit.sum(dim=(0, 2)), lit.sum(dim=(0, 1))]).to(torch.int32)


def profile(frames: torch.Tensor, dark: int, ops=None) -> torch.Tensor:
    """int32 [H + W].  ``ops.active_profile`` (HipOps: csrc/svr_active.hip) where the backend has it -- a failing library raises,
    there is no fall-back from it -- else the torch statement above."""
    if ops is not None and hasattr(ops, "active_profile"):
        check_frames(frames)
        check_dark(dark)
        return ops.active_profile(frames, dark)
    return profile_torch(frames, dark)


def _runs(dark_lines: Sequence[bool]) -> Tuple[int, int]:
    """(leading, trailing) run lengths of True"""
    n = len(dark_lines)
    lead = next((i for i, d in enumerate(dark_lines) if not d), n)
    trail = next((i for i, d in enumerate(reversed(dark_lines)) if not d), n)
    return lead, trail


class Rule:
    def __init__(self, dark: int, specks: int, skew: int, margin: int, gain: int):
        check_dark(dark)
        for name, v in (("specks", specks), ("skew", skew), ("margin", margin), ("gain", gain)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
        self.dark, self.specks, self.skew, self.margin, self.gain = dark, specks, skew, margin, gain

    def area(self, profile: List[int], T: int, H: int, W: int) -> Tuple[int, int, int, int]:
        if T < 1 or H < 1 or W < 1:
            raise ValueError(f"T, H and W must be at least 1, got T = {T}, H = {H}, W = {W}")
        if len(profile) != H + W:
            raise ValueError(f"profile must hold H + W = {H + W} counts, got {len(profile)}")
        full = (0, H, 0, W)
        top, bottom = _runs([int(c) * 1_000_000 <= self.specks * T * W for c in profile[:H]])
        left, right = _runs([int(c) * 1_000_000 <= self.specks * T * H for c in profile[H:]])
        if top + bottom >= H or left + right >= W:
            return full
        if abs(top - bottom) > self.skew:
            top = bottom = 0
        if abs(left - right) > self.skew:
            left = right = 0
        y0, y1 = max(top - self.margin, 0), min(H - bottom + self.margin, H)
        x0, x1 = max(left - self.margin, 0), min(W - right + self.margin, W)
        if y1 - y0 < MIN_SIDE or x1 - x0 < MIN_SIDE:
            return full
        if (H * W - (y1 - y0) * (x1 - x0)) * 100 < self.gain * H * W:
            return full
        return (y0, y1, x0, x1)


def out_rect(area: Tuple[int, int, int, int], H: int, W: int, TH: int, TW: int) -> Tuple[int, int, int, int]:
    y0, y1, x0, x1 = (int(v) for v in area)
    if TH < 2 or TW < 2 or TH % 2 or TW % 2:
        raise ValueError(f"TH and TW must be even and positive, got TH = {TH}, TW = {TW}")
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError(f"area must satisfy 0 <= y0 < y1 <= H = {H} and 0 <= x0 < x1 <= W = {W}, got {(y0, y1, x0, x1)}")
    return (2 * ((y0 * TH) // (2 * H)), min(TH, 2 * -((-y1 * TH) // (2 * H))),
            2 * ((x0 * TW) // (2 * W)), min(TW, 2 * -((-x1 * TW) // (2 * W))))
