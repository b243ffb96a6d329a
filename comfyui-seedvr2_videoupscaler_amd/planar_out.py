"""Output frames written as planar YUV -- 4:2:0, 4:2:2 or 4:4:4 at 8, 10 or 12 bits, BT.709 / BT.601 / BT.2020 -- for the encoder: the
mirror image of planar.py, stated once, in plain torch.

This module is the specification of the kernels in csrc/svr_planar_out.hip (equal bit for bit: integer results, no tolerance) and the
path taken when ``ops`` has no ``pack_planar`` (the torch double of the C ABI that drives the CPU tests).  Any device.  ``ENABLED``
(off as shipped): whether inference_cli.route_output routes an mp4 output here at all.

``pack_planar_torch(frames, sub, bits, matrix, range_, siting)``: ``frames`` [T, H, W, 3], fp32 or bf16, nominally in [0, 1] -> the
planes per frame, Y then Cb then Cr, in planar.planar_shape's layout and planar.planar_dtype's type (uint8 at 8 bits, uint16 at 10 and
12): ffmpeg's ``yuv4??p`` / ``yuv4??p10le`` / ``yuv4??p12le`` rawvideo, and what planar.planar_codes_torch reads back.

  sub       one of planar.SUBS; ``bits`` one of planar.BITS (n below); ``matrix`` a key of frameio.KR_KB; ``range_`` one of
            frameio.YUV_RANGES.
  siting    "420": "center", "left" or "topleft";  "422": "center" or "left";  "444": "left" only (it has nothing to site) -- SITINGS.
  codes     q = frameio.codes(frames, 65535.0) as int64 (NaN -> 0, +inf -> full scale, -inf -> 0, as every other format);
            D = frameio.YUV_D;  (wr, wg, wb, cb_r, cb_g, cr_g, cr_b) = frameio.yuv_matrix(matrix);
            (y0, ys, cs, _) = planar.yuv_constants(bits, range_);  half = 2^(n-1), top = 2^n - 1.
  luma      Y  = y0 + (ys * (wr r + wg g + wb b) + D/2) // D                                         per pixel
  chroma    sr, sg, sb: weighted sums of q, total weight S = Sv * Sh, indices clamped to the frame:
              vertical    422 / 444: row y, weight 1 (Sv = 1)
                          420 "center" / "left": rows 2j, 2j+1, weights 1, 1 (Sv = 2)
                          420 "topleft": rows 2j-1, 2j, 2j+1, weights 1, 2, 1 (Sv = 4)
              horizontal  444: column x, weight 1 (Sh = 1)
                          420 / 422 "center": columns 2k, 2k+1, weights 1, 1 (Sh = 2)
                          420 / 422 "left", 420 "topleft": columns 2k-1, 2k, 2k+1, weights 1, 2, 1 (Sh = 4)
            Cb = clamp((S half D + cs (cb_r sr + cb_g sg + 32768 sb) + S D/2) // (S D), 0, top)
            Cr = clamp((S half D + cs (32768 sr + cr_g sg + cr_b sb) + S D/2) // (S D), 0, top)
  bounds    S is 1, 2, 4, 8 or 16.  Over every depth, matrix, range and S the smallest chroma numerator any input can give is
            4 294 901 760 = D > 0 (8 bits, "pc", S = 1: a chroma row's negative weights sum to -32768) and the largest is
            281 470 681 743 360 = 65536 D < 2^62 (12 bits, "pc", S = 16); the luma numerator lies between D/2 and ys * D + D/2.  So a
            kernel's unsigned 64-bit division IS the floor division (``numerator_bounds`` computes both ends in Python integers and
            tests/test_planar_out.py asserts them for every combination).  The clamp at top is needed at every depth: in "pc" range a
            saturated blue reaches 2^n without it.

("420", 10, m, r, "center" | "left") is frameio.pack_yuv420p10_torch(frames, m, r, siting) bit for bit.  Check values (Y, Cb, Cr) of a
flat frame, any siting of the sub: bt709 tv 8 bits white (235, 128, 128), black (16, 128, 128), red (63, 102, 240), green (173, 42, 26),
blue (32, 240, 118); bt601 tv 8 bits red (81, 90, 240); bt2020 tv 12 bits red (1176, 1548, 3840), green (2632, 756, 400), blue
(464, 3840, 1904); bt709 pc 8 bits blue (18, 255, 116) -- the clamp; the 10-bit rows are frameio's.
"""
import torch

from . import frameio, planar

ENABLED = False                                          # inference_cli.route_output routes nothing while this is off
SITINGS = {"420": ("center", "left", "topleft"), "422": ("center", "left"), "444": ("left",)}


def pix_fmt(sub: str, bits: int) -> str:
    """ffmpeg's name of the planes: yuv420p, yuv422p10le, yuv444p12le ..."""
    check_arguments(sub, bits, "bt709", "tv", "left")
    return f"yuv{sub}p" + ("" if bits == 8 else f"{bits}le")


def check_arguments(sub, bits, matrix, range_, siting):
    """The refusals shared by the torch statement and HipOps.pack_planar, each naming its argument."""
    if sub not in planar.SUBS:
        raise ValueError(f"sub must be one of {planar.SUBS}, got {sub!r}")
    if bits not in planar.BITS:
        raise ValueError(f"bits must be one of {planar.BITS}, got {bits!r}")
    if matrix not in frameio.KR_KB:
        raise ValueError(f"matrix must be one of {tuple(frameio.KR_KB)}, got {matrix!r}")
    if range_ not in frameio.YUV_RANGES:
        raise ValueError(f"range_ must be one of {frameio.YUV_RANGES}, got {range_!r}")
    if siting not in SITINGS[sub]:
        raise ValueError(f"siting must be one of {SITINGS[sub]} for sub {sub!r}, got {siting!r}")


def check_channels(C: int):
    if C != 3:
        raise ValueError(f"planar output takes C = 3 (it has no alpha plane), got C = {C}")


def taps(sub: str, siting: str):
    """-> (vertical step, ((row offset, weight), ...), horizontal step, ((column offset, weight), ...)) of one chroma sample"""
    three = ((-1, 1), (0, 2), (1, 1))
    vertical = (1, ((0, 1),)) if sub != "420" else (2, three if siting == "topleft" else ((0, 1), (1, 1)))
    horizontal = (1, ((0, 1),)) if sub == "444" else (2, ((0, 1), (1, 1)) if siting == "center" else three)
    return vertical + horizontal


def total_weight(sub: str, siting: str) -> int:
    _, v, _, h = taps(sub, siting)
    return sum(w for _, w in v) * sum(w for _, w in h)


def numerator_bound(bits: int, matrix: str, range_: str, S: int):
    """-> (smallest, largest) chroma numerator any codes can give at total weight S, in Python integers"""
    _, _, _, cb_r, cb_g, cr_g, cr_b = frameio.yuv_matrix(matrix)
    _, _, cs, _ = planar.yuv_constants(bits, range_)
    full, D = S * 65535, frameio.YUV_D
    fixed = S * (1 << (bits - 1)) * D + S * D // 2
    ends = []
    for row in ((cb_r, cb_g, 32768), (32768, cr_g, cr_b)):                     # (linear in the sums: the ends sit at the corners)
        ends += [fixed + cs * full * sum(w for w in row if w < 0), fixed + cs * full * sum(w for w in row if w > 0)]
    return min(ends), max(ends)


def numerator_bounds():
    """-> (smallest, largest) chroma numerator over every depth, matrix, range and S: what a kernel's unsigned 64 bits have to hold"""
    every = [numerator_bound(bits, matrix, range_, S) for bits in planar.BITS for matrix in frameio.KR_KB
             for range_ in frameio.YUV_RANGES for S in (1, 2, 4, 8, 16)]
    return min(lo for lo, _ in every), max(hi for _, hi in every)


def pack_planar_torch(frames: torch.Tensor, sub: str, bits: int, matrix: str = "bt709", range_: str = "tv",
                      siting: str = "left") -> torch.Tensor:
    if frames.dim() != 4 or frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames must be [T, H, W, C] in fp32 or bf16, got {tuple(frames.shape)} {frames.dtype}")
    check_arguments(sub, bits, matrix, range_, siting)
    T, H, W, C = frames.shape
    check_channels(C)
    if T < 1 or H < 1 or W < 1:
        raise ValueError(f"frames must hold at least one pixel, got {tuple(frames.shape)}")
    shape = planar.planar_shape(T, H, W, sub)
    hc, wc = planar.chroma_dims(sub, H, W)
    D = frameio.YUV_D
    wr, wg, wb, cb_r, cb_g, cr_g, cr_b = frameio.yuv_matrix(matrix)
    y0, ys, cs, _ = planar.yuv_constants(bits, range_)
    half, top = 1 << (bits - 1), (1 << bits) - 1
    q = frameio.codes(frames, 65535.0).to(torch.int64)
    r, g, b = q[..., 0], q[..., 1], q[..., 2]
    Y = y0 + frameio._floor_div(ys * (wr * r + wg * g + wb * b) + D // 2, D)
    vstep, vtaps, hstep, htaps = taps(sub, siting)
    S = total_weight(sub, siting)
    j, k = vstep * torch.arange(hc, device=q.device), hstep * torch.arange(wc, device=q.device)
    v = sum(w * q[:, (j + d).clamp(0, H - 1)] for d, w in vtaps)              # [T, hc, W, 3]
    s = sum(w * v[:, :, (k + d).clamp(0, W - 1)] for d, w in htaps)           # [T, hc, wc, 3]
    sr, sg, sb = s[..., 0], s[..., 1], s[..., 2]
    Cb = frameio._floor_div(S * half * D + cs * (cb_r * sr + cb_g * sg + 32768 * sb) + S * D // 2, S * D).clamp(0, top)
    Cr = frameio._floor_div(S * half * D + cs * (32768 * sr + cr_g * sg + cr_b * sb) + S * D // 2, S * D).clamp(0, top)
    out = torch.cat([Y.reshape(T, -1), Cb.reshape(T, -1), Cr.reshape(T, -1)], dim=1).to(torch.int32).to(planar.planar_dtype(bits))
    assert tuple(out.shape) == shape
    return out


def pack_planar(frames: torch.Tensor, sub: str, bits: int, matrix: str = "bt709", range_: str = "tv", siting: str = "left", ops=None,
                out: torch.Tensor = None) -> torch.Tensor:
    """The planes.  ``ops.pack_planar`` (HipOps: csrc/svr_planar_out.hip) where the backend has it -- a failing library raises, there
    is no fall-back from it -- else the torch statement above.  ``out``: a tensor of the planes' shape and dtype."""
    if ops is not None and hasattr(ops, "pack_planar"):
        return ops.pack_planar(frames, sub, bits, matrix, range_, siting, out=out)
    packed = pack_planar_torch(frames, sub, bits, matrix, range_, siting)
    if out is None:
        return packed
    if out.dtype != packed.dtype or tuple(out.shape) != tuple(packed.shape):
        raise ValueError(f"out must be {packed.dtype} {tuple(packed.shape)}, got {out.dtype} {tuple(out.shape)}")
    out.copy_(packed)
    return out
