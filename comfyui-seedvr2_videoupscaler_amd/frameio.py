"""Output frames narrowed for the encoder: the packed formats, stated once, in plain torch.

This module is the specification of the kernels in csrc/svr_frame_pack.hip and, for "yuv420p10", of csrc/svr_frame_pack_colour.hip
run with the BT.709 limited-range constants and centre-sited chroma (equal bit for bit: integer results, no tolerance) and
the path taken when ``ops`` has no ``pack_frames`` (the fp32 torch double of the C ABI that drives the CPU tests).  Any device.

``frames`` [T, H, W, C], fp32 or bf16, nominally in [0, 1], C = 3 or 4.

  "rgb8" / "bgr8"   uint8 [T, H, W, C]: round_half_even(clamp(float(x), 0, 1) * 255.0) in fp32 -- what the command line's writers
                    have always computed on the host.  "bgr8" swaps channels 0 and 2 (OpenCV's and ffmpeg's bgr24 order); a fourth
                    channel stays in place (BGRA).
  "yuv420p10"       C = 3.  uint16 [T, H*W + 2*h2*w2], h2 = ceil(H/2), w2 = ceil(W/2): per frame the Y plane row-major, then Cb,
                    then Cr -- ffmpeg's ``yuv420p10le`` rawvideo layout.  BT.709, limited range, in exact integers:
                        q  = round_half_even(clamp(float(x), 0, 1) * 65535.0) as int64              D = 65535 * 65536
                        Y  = 64 + (876 * (13933 r + 46871 g + 4732 b) + D/2) // D                   per pixel
                        Cb = (2048 D + 896 * (-7509 sr - 25259 sg + 32768 sb) + 2 D) // (4 D)       sr, sg, sb: the sums of q over
                        Cr = (2048 D + 896 * (32768 sr - 29763 sg - 3005 sb) + 2 D) // (4 D)        the 2 x 2 block
                    (the BT.709 luma weights 0.2126 / 0.7152 / 0.0722 and the chroma rows scaled by 65536; 876 = 940 - 64 and
                    896 = 960 - 64 the 10-bit excursions; a block's rows and columns beyond the frame repeat the last one).  Every
                    numerator is positive and below 2^62, so truncating and floor division agree.  Y 64..940, Cb / Cr 64..960;
                    white (940, 512, 512), black (64, 512, 512), red (250, 409, 960), green (691, 167, 105), blue (127, 960, 471).

``pack_yuv420p10_torch(frames, matrix, range_, siting)``: the same planes, uint16 [T, H*W + 2*h2*w2] from C = 3, for any of three
matrices, two ranges and two chroma sitings -- what an HDR (BT.2020) source is written with.  csrc/svr_frame_pack_colour.hip is its
kernel, equal bit for bit.  With q and D as above, half = 512, top = 1023:

  range_    "tv": y0 = 64, ys = 876, cs = 896;  "pc": y0 = 0, ys = cs = 1023  (frameio_in.yuv_constants(10, range_)).
  matrix    Kr / Kb exact decimals: "bt709" 0.2126 / 0.0722, "bt601" 0.299 / 0.114, "bt2020" 0.2627 / 0.0593; Kg = 1 - Kr - Kb.
            Every weight rounded to nearest at 2^16: luma (Kr, Kg, Kb); the Cb row (-Kr, -Kg, .) / (2 (1 - Kb)) with 32768 for B; the
            Cr row (., -Kg, -Kb) / (2 (1 - Kr)) with 32768 for R.  The luma weights must sum to 65536: a deficit goes to green
            (bt2020: 44433 -> 44434).  Each chroma row then sums to 0.  As (wr, wg, wb | cb_r, cb_g | cr_g, cr_b):
                bt709    13933, 46871, 4732 |  -7509, -25259 | -29763, -3005      (the constants of "yuv420p10" above)
                bt601    19595, 38470, 7471 | -11058, -21710 | -27439, -5329
                bt2020   17216, 44434, 3886 |  -9151, -23617 | -30133, -2635
  luma      Y  = y0 + (ys * (wr r + wg g + wb b) + D/2) // D                                         per pixel
  siting    sr, sg, sb: weighted sums of q with total weight S, indices clamped to the frame.
            "center"  rows 2j, 2j+1, columns 2k, 2k+1, all weights 1: S = 4 -- the 2 x 2 block of "yuv420p10" above.
            "left"    rows 2j, 2j+1 with weight 1, columns 2k-1, 2k, 2k+1 with weights 1, 2, 1: S = 8 -- chroma co-sited with even
                      luma columns, the H.264 / HEVC default and the siting frameio_in.upsample_chroma assumes.
  chroma    Cb = clamp((S half D + cs * (cb_r sr + cb_g sg + 32768 sb) + S D/2) // (S D), 0, top)
            Cr = clamp((S half D + cs * (32768 sr + cr_g sg + cr_b sb) + S D/2) // (S D), 0, top)
            Every numerator is positive (S half D > cs * 32768 * S * 65535 in both ranges) and below 2^62: unsigned division is the
            floor division.  The clamp at top is needed: in "pc" range a saturated blue reaches 1024 without it.

("bt709", "tv", "center") is "yuv420p10" bit for bit.  Check values (Y, Cb, Cr) of a flat frame, either siting: every tv case white
(940, 512, 512), black (64, 512, 512), grey 0.5 (502, 512, 512); every pc case white (1023, 512, 512), black (0, 512, 512);
                 red               green             blue
  bt2020 tv   (294, 387, 960)   (658, 189, 100)   (116, 960, 476)
  bt601 tv    (326, 361, 960)   (578, 215, 137)   (164, 960, 439)
  bt709 tv    (250, 409, 960)   (691, 167, 105)   (127, 960, 471)
  bt709 pc    (217, 395, 1023)  (732, 118, 47)    (74, 1023, 465)
  bt2020 pc   (269, 369, 1023)  (694, 143, 42)    (61, 1023, 471)
Why "left": a decoder that is told nothing assumes it, and a centre-sited plane read that way is shifted by half a luma pixel -- on a
horizontal colour ramp, bt2020 tv, through frameio_in.upsample_chroma: R error 4.96e-3, B 5.77e-3 (quantisation bounds 1.42e-3 and
1.65e-3) for "center", 1.24e-3 and 1.58e-3 for "left" (tests/test_colour_out.py).

Non-finite input, explicitly: NaN -> code 0 (the kernels' fmaxf(NaN, 0) = 0), +inf -> full scale, -inf -> 0, in every format.
"""
from fractions import Fraction

import torch

FORMATS = ("rgb8", "bgr8", "yuv420p10")
YUV_D = 65535 * 65536


def packed_dtype(fmt: str) -> torch.dtype:
    return torch.uint16 if fmt == "yuv420p10" else torch.uint8


def packed_shape(T: int, H: int, W: int, C: int, fmt: str):
    """Shape of the packed clip; raises for an unknown format or a channel count the format does not take."""
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {FORMATS}, got {fmt!r}")
    if fmt == "yuv420p10":
        if C != 3:
            raise ValueError(f"yuv420p10 takes C = 3 (it has no alpha plane), got C = {C}")
        return (T, H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2))
    if C not in (3, 4):
        raise ValueError(f"{fmt} takes C = 3 or 4, got C = {C}")
    return (T, H, W, C)


def codes(frames: torch.Tensor, full_scale: float) -> torch.Tensor:
    """round_half_even(clamp(float(x), 0, 1) * full_scale), fp32 holding integers; NaN -> 0 said here, not left to a cast."""
    x = frames.float()
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    return (x.clamp(0, 1) * full_scale).round()


def _floor_div(a: torch.Tensor, b: int) -> torch.Tensor:
    return torch.div(a, b, rounding_mode="floor")


def pack_frames_torch(frames: torch.Tensor, fmt: str) -> torch.Tensor:
    if frames.dim() != 4 or frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames must be [T, H, W, C] in fp32 or bf16, got {tuple(frames.shape)} {frames.dtype}")
    T, H, W, C = frames.shape
    shape = packed_shape(T, H, W, C, fmt)
    if fmt != "yuv420p10":
        q = codes(frames, 255.0).to(torch.uint8)
        if fmt == "bgr8":
            q = q[..., [2, 1, 0] + ([3] if C == 4 else [])]
        return q.contiguous()
    q = codes(frames, 65535.0).to(torch.int64)
    r, g, b = q[..., 0], q[..., 1], q[..., 2]
    Y = 64 + _floor_div(876 * (13933 * r + 46871 * g + 4732 * b) + YUV_D // 2, YUV_D)
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    rows = torch.arange(2 * h2, device=q.device).clamp(max=H - 1)        # beyond the frame: the last row / column again
    cols = torch.arange(2 * w2, device=q.device).clamp(max=W - 1)
    s = q[:, rows][:, :, cols].reshape(T, h2, 2, w2, 2, 3).sum(dim=(2, 4))
    sr, sg, sb = s[..., 0], s[..., 1], s[..., 2]
    Cb = _floor_div(2048 * YUV_D + 896 * (-7509 * sr - 25259 * sg + 32768 * sb) + 2 * YUV_D, 4 * YUV_D)
    Cr = _floor_div(2048 * YUV_D + 896 * (32768 * sr - 29763 * sg - 3005 * sb) + 2 * YUV_D, 4 * YUV_D)
    out = torch.cat([Y.reshape(T, -1), Cb.reshape(T, -1), Cr.reshape(T, -1)], dim=1).to(torch.uint16)
    assert tuple(out.shape) == shape
    return out


def pack_frames(frames: torch.Tensor, fmt: str, ops=None, out: torch.Tensor = None) -> torch.Tensor:
    """The packed clip.  ``ops.pack_frames`` (HipOps: csrc/svr_frame_pack.hip) where the backend has it -- a failing library
    raises, there is no fall-back from it -- else the torch statement above.  ``out``: a tensor of the packed shape and dtype."""
    if ops is not None and hasattr(ops, "pack_frames"):
        return ops.pack_frames(frames, fmt, out=out)
    packed = pack_frames_torch(frames, fmt)
    if out is None:
        return packed
    if out.dtype != packed.dtype or tuple(out.shape) != tuple(packed.shape):
        raise ValueError(f"out must be {packed.dtype} {tuple(packed.shape)}, got {out.dtype} {tuple(out.shape)}")
    out.copy_(packed)
    return out


# ---------------------------------------------------------------------------------------------------------------- colour out
KR_KB = {"bt709": ("0.2126", "0.0722"), "bt601": ("0.299", "0.114"), "bt2020": ("0.2627", "0.0593")}      # exact decimals
YUV_RANGES = ("tv", "pc")
SITINGS = ("center", "left")


def _nearest(f: Fraction) -> int:
    return (2 * f.numerator + f.denominator) // (2 * f.denominator)


def yuv_matrix(matrix: str):
    """-> (wr, wg, wb, cb_r, cb_g, cr_g, cr_b): the module docstring's weights at 2^16, from the exact decimal Kr, Kb."""
    kr, kb = (Fraction(k) for k in KR_KB[matrix])
    kg = 1 - kr - kb
    wr, wg, wb = (_nearest(k * 65536) for k in (kr, kg, kb))
    wg += 65536 - (wr + wg + wb)                                               # (the deficit goes to green)
    cb_r, cb_g = (_nearest(-k / (2 * (1 - kb)) * 65536) for k in (kr, kg))
    cr_g, cr_b = (_nearest(-k / (2 * (1 - kr)) * 65536) for k in (kg, kb))
    return wr, wg, wb, cb_r, cb_g, cr_g, cr_b


def check_colour(matrix: str, range_: str, siting: str):
    """The refusals shared by the torch statement and HipOps.pack_yuv420p10, each naming its argument."""
    if matrix not in KR_KB:
        raise ValueError(f"matrix must be one of {tuple(KR_KB)}, got {matrix!r}")
    if range_ not in YUV_RANGES:
        raise ValueError(f"range_ must be one of {YUV_RANGES}, got {range_!r}")
    if siting not in SITINGS:
        raise ValueError(f"siting must be one of {SITINGS}, got {siting!r}")


def pack_yuv420p10_torch(frames: torch.Tensor, matrix: str = "bt709", range_: str = "tv", siting: str = "center") -> torch.Tensor:
    if frames.dim() != 4 or frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames must be [T, H, W, C] in fp32 or bf16, got {tuple(frames.shape)} {frames.dtype}")
    check_colour(matrix, range_, siting)
    T, H, W, C = frames.shape
    shape = packed_shape(T, H, W, C, "yuv420p10")
    wr, wg, wb, cb_r, cb_g, cr_g, cr_b = yuv_matrix(matrix)
    y0, ys, cs = (64, 876, 896) if range_ == "tv" else (0, 1023, 1023)
    half, top = 512, 1023
    q = codes(frames, 65535.0).to(torch.int64)
    r, g, b = q[..., 0], q[..., 1], q[..., 2]
    Y = y0 + _floor_div(ys * (wr * r + wg * g + wb * b) + YUV_D // 2, YUV_D)
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    rows = torch.arange(2 * h2, device=q.device).clamp(max=H - 1)              # beyond the frame: the last row / column again
    k2 = 2 * torch.arange(w2, device=q.device)
    taps = ((0, 1), (1, 1)) if siting == "center" else ((-1, 1), (0, 2), (1, 1))        # (column offset, weight)
    S = 2 * sum(w for _, w in taps)
    v = q[:, rows].reshape(T, h2, 2, W, 3).sum(dim=2)                          # [T, h2, W, 3]: the two rows
    s = sum(w * v[:, :, (k2 + d).clamp(0, W - 1)] for d, w in taps)            # [T, h2, w2, 3]
    sr, sg, sb = s[..., 0], s[..., 1], s[..., 2]
    Cb = _floor_div(S * half * YUV_D + cs * (cb_r * sr + cb_g * sg + 32768 * sb) + S * YUV_D // 2, S * YUV_D).clamp(0, top)
    Cr = _floor_div(S * half * YUV_D + cs * (32768 * sr + cr_g * sg + cr_b * sb) + S * YUV_D // 2, S * YUV_D).clamp(0, top)
    out = torch.cat([Y.reshape(T, -1), Cb.reshape(T, -1), Cr.reshape(T, -1)], dim=1).to(torch.uint16)
    assert tuple(out.shape) == shape
    return out


def pack_yuv420p10(frames: torch.Tensor, matrix: str = "bt709", range_: str = "tv", siting: str = "center", ops=None,
                   out: torch.Tensor = None) -> torch.Tensor:
    """The planes.  ``ops.pack_yuv420p10`` (HipOps: csrc/svr_frame_pack_colour.hip) where the backend has it -- a failing library
    raises, there is no fall-back from it -- else the torch statement above.  ``out``: a uint16 tensor of the packed shape."""
    if ops is not None and hasattr(ops, "pack_yuv420p10"):
        return ops.pack_yuv420p10(frames, matrix, range_, siting, out=out)
    packed = pack_yuv420p10_torch(frames, matrix, range_, siting)
    if out is None:
        return packed
    if out.dtype != packed.dtype or tuple(out.shape) != tuple(packed.shape):
        raise ValueError(f"out must be {packed.dtype} {tuple(packed.shape)}, got {out.dtype} {tuple(out.shape)}")
    out.copy_(packed)
    return out
