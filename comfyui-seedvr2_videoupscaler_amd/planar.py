"""Planar YUV as a decoder emits it -- 4:2:0, 4:2:2 or 4:4:4 at 8, 10 or 12 bits, BT.709 / BT.601 / BT.2020 -- turned into 16-bit RGB
codes: frameio_in.py's "rgb16" format, stated once, in plain torch.  The stage between the upload and everything else: deinterlace,
field matching, decimation and frameio_in.unpack_frames all take "rgb16" as they always did.

This module is the specification of the kernels in csrc/svr_planar.hip (equal bit for bit: every result is an integer code, no
tolerance) and the path taken when ``ops`` has no ``planar_codes`` (the torch double of the C ABI that drives the CPU tests).  Any
device.  ``ENABLED`` (off as shipped): whether inference_cli.route_planar routes a source here at all.

``planar_codes_torch(planes, sub, bits, T, H, W, matrix, range_, siting)`` -> uint16 [T, H, W, 3].

  layout    ``sub`` "420" | "422" | "444", ``bits`` 8 (uint8) | 10 | 12 (uint16: the little-endian containers).  ``planes`` holds, per
            frame, Y [H, W], then Cb, then Cr, each [hc, wc] row-major:  420 hc = ceil(H/2), wc = ceil(W/2);  422 hc = H,
            wc = ceil(W/2);  444 hc = H, wc = W.  A sample above 2^bits - 1 -- the container has room for it, a decoder never writes
            it -- counts as 2^bits - 1, so the bounds below hold for any bytes.
  chroma    cb8, cr8: the plane C at every luma position in integers, weights summing to 8, indices clamped to the plane.
            Vertically V, in quarters:
              422 / 444            row y takes 4 C[y]
              420 "left"           (MPEG-2 / H.264 / HEVC default: midway between luma rows; frameio_in.upsample_chroma) row 2j takes
                                   C[j-1] + 3 C[j], row 2j+1 takes 3 C[j] + C[j+1]
              420 "topleft"        (HDR10 / UHD: co-sited with even luma rows) row 2j takes 4 C[j], row 2j+1 takes
                                   2 C[j] + 2 C[min(j+1, hc-1)]
            Horizontally:
              420 / 422            (co-sited with even luma columns) column 2k takes 2 V[k], column 2k+1 takes V[k] + V[min(k+1, wc-1)]
              444                  column x takes 2 V[x]
            ``siting`` is "left" or "topleft" for 420 and "left" only for 422 and 444 (which have nothing to site vertically).
            For 422 and 444 an output row depends on its own input row alone: the field structure of an interlaced source survives.
  matrix    frameio_in.yuv_codes' formula as it stands, n = bits:  tv: y0 = 16 << (n-8), ys = 219 << (n-8), cs = 224 << (n-8);
            pc: y0 = 0, ys = cs = 2^n - 1;  mid = 8 * 2^(n-1), u = cb8 - mid, v = cr8 - mid
              Den   = ys * 8 * cs * 65536                   base = (Y - y0) * 8 * cs * 65536
              s_R = base + rv * v * ys      s_G = base - (gu * u + gv * v) * ys      s_B = base + bu * u * ys
              q   = clamp(floor((2 * 65535 * s + Den) / (2 * Den)), 0, 65535)        (round half up of 65535 s / Den)
            ``matrix`` "bt709" | "bt601" | "bt2020" (non-constant luminance).  rv, gu, gv, bu = 2 (1 - Kr), 2 (1 - Kb) Kb / Kg,
            2 (1 - Kr) Kr / Kg, 2 (1 - Kb), each rounded at 2^16 from the exact decimal Kr, Kb of frameio.KR_KB:
              bt709 103206, 12276, 30679, 121609      bt601 91881, 22553, 46802, 116130      bt2020 96639, 10784, 37444, 123299
            (the first two rows are frameio_in.MATRICES').
  bounds    |u|, |v| <= 8 * 2^(n-1) = 16384 at 12 bits (the samples are clamped FIRST), so the 32-bit products bu * u (at most
            123299 * 16384 < 2.03e9) and gu * u + gv * v (at most 48228 * 16384 < 7.91e8) stay below 2^31: a kernel keeps the clamp
            ahead of them.  The worst case is 12 bits, bt2020, pc: |s| <= 4095 * 8 * 4095 * 65536 + 123299 * 16384 * 4095 < 1.71e13,
            so 2 * 65535 * |s| + Den < 2.25e18 < 2^61 = 0.25 * 2^63 (``numerator_bound`` computes it in Python integers and
            tests/test_planar.py asserts it for every matrix, range and depth).  Numerators CAN be negative: the division is a
            FLOOR division -- a kernel with a truncating or unsigned division clamps at zero before it divides.

Check values (tests/test_planar.py): tv (235, 128, 128) << (n-8) -> (65535, 65535, 65535) and (16, 128, 128) << (n-8) -> (0, 0, 0),
every matrix and depth; pc (2^n - 1, mid, mid) -> white.  For sub "420", siting "left", 8 / 10 bits, bt709 / bt601
frameio_in.unpack_frames_torch(planar_codes_torch(p, ...), "rgb16", ...) IS frameio_in.unpack_frames_torch(p, "yuv420p8" | "yuv420p10",
...), bit for bit.
"""
from fractions import Fraction

import torch

from . import frameio, frameio_in

ENABLED = False                                          # inference_cli.route_planar routes nothing while this is off
SUBS = ("420", "422", "444")
BITS = (8, 10, 12)
RANGES = frameio_in.RANGES
SITINGS = {"420": ("left", "topleft"), "422": ("left",), "444": ("left",)}


def _matrix(name: str):
    """rv, gu, gv, bu at 2^16 from the exact decimal Kr, Kb (frameio.KR_KB), rounded as frameio.yuv_matrix rounds"""
    kr, kb = (Fraction(k) for k in frameio.KR_KB[name])
    kg = 1 - kr - kb
    return tuple(frameio._nearest(f * 65536) for f in (2 * (1 - kr), 2 * (1 - kb) * kb / kg, 2 * (1 - kr) * kr / kg, 2 * (1 - kb)))


MATRICES = {name: _matrix(name) for name in ("bt709", "bt601", "bt2020")}      # rv, gu, gv, bu


def yuv_constants(bits: int, range_: str):
    """-> (y0, ys, cs, mid): frameio_in.yuv_constants' shifts, for 8, 10 and 12 bits"""
    if range_ == "tv":
        return 16 << (bits - 8), 219 << (bits - 8), 224 << (bits - 8), 8 << (bits - 1)
    return 0, (1 << bits) - 1, (1 << bits) - 1, 8 << (bits - 1)


def numerator_bound(bits: int, matrix: str, range_: str) -> int:
    """The largest 2 * 65535 * |s| + Den any samples can give (Python integers): what a kernel's 64-bit numerator has to hold."""
    rv, gu, gv, bu = MATRICES[matrix]
    y0, ys, cs, mid = yuv_constants(bits, range_)
    top = (1 << bits) - 1
    base = max(top - y0, y0) * 8 * cs * 65536
    return 2 * 65535 * (base + max(rv, gu + gv, bu) * mid * ys) + ys * 8 * cs * 65536


def chroma_dims(sub: str, H: int, W: int):
    """-> (hc, wc) of one chroma plane"""
    return ((H + 1) // 2 if sub == "420" else H), (W if sub == "444" else (W + 1) // 2)


def planar_dtype(bits: int) -> torch.dtype:
    return torch.uint8 if bits == 8 else torch.uint16


def planar_shape(T: int, H: int, W: int, sub: str):
    """Shape of the planes of a clip; raises for an unknown subsampling."""
    if sub not in SUBS:
        raise ValueError(f"sub must be one of {SUBS}, got {sub!r}")
    hc, wc = chroma_dims(sub, H, W)
    return (T, H * W + 2 * hc * wc)


def frame_bytes(H: int, W: int, sub: str, bits: int) -> int:
    if bits not in BITS:
        raise ValueError(f"bits must be one of {BITS}, got {bits!r}")
    return planar_shape(1, H, W, sub)[1] * (1 if bits == 8 else 2)


def check_arguments(planes, sub, bits, T, H, W, matrix, range_, siting):
    """The refusals shared by the torch statement and HipOps.planar_codes, each naming its argument; -> the planes' shape."""
    shape = planar_shape(T, H, W, sub)
    if bits not in BITS:
        raise ValueError(f"bits must be one of {BITS}, got {bits!r}")
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {tuple(MATRICES)}, got {matrix!r}")
    if range_ not in RANGES:
        raise ValueError(f"range_ must be one of {RANGES}, got {range_!r}")
    if siting not in SITINGS[sub]:
        raise ValueError(f"siting must be one of {SITINGS[sub]} for sub {sub!r}, got {siting!r}")
    if T < 1 or H < 1 or W < 1:
        raise ValueError(f"T, H, W must be positive, got T = {T}, H = {H}, W = {W}")
    if planes.dtype != planar_dtype(bits):
        raise ValueError(f"planes must be {planar_dtype(bits)} for {bits} bits, got {planes.dtype}")
    if planes.numel() != shape[0] * shape[1]:
        raise ValueError(f"planes must hold {shape[0] * shape[1]} samples ({tuple(shape)}) for sub {sub!r} at T, H, W = {T}, {H}, {W}, "
                         f"got {tuple(planes.shape)}")
    return shape


def upsample_chroma(c, sub: str, siting: str, H: int, W: int):
    """int64 [T, hc, wc] -> [T, H, W]: the chroma plane at every luma position, times 8 (the module docstring's V, then columns)."""
    hc, wc = c.shape[1], c.shape[2]
    y = torch.arange(H, device=c.device)
    if sub != "420":
        v = 4 * c
    elif siting == "left":
        j = y // 2
        v = 3 * c[:, j] + c[:, torch.where(y % 2 == 0, j - 1, j + 1).clamp(0, hc - 1)]
    else:
        j = y // 2
        v = 2 * c[:, j] + 2 * c[:, (j + y % 2).clamp(max=hc - 1)]
    if sub == "444":
        return 2 * v
    x = torch.arange(W, device=c.device)
    k = x // 2
    return v[:, :, k] + v[:, :, (k + x % 2).clamp(max=wc - 1)]


def yuv_codes(Y, cb8, cr8, bits: int, matrix: str, range_: str):
    """frameio_in.yuv_codes with this module's three matrices and three depths: int64 tensors -> (R, G, B) 16-bit codes."""
    rv, gu, gv, bu = MATRICES[matrix]
    y0, ys, cs, mid = yuv_constants(bits, range_)
    den = ys * 8 * cs * 65536
    base = (Y - y0) * (8 * cs * 65536)
    u, v = cb8 - mid, cr8 - mid

    def code(s):                                     # (floor division: the numerator can be negative)
        return torch.div(2 * 65535 * s + den, 2 * den, rounding_mode="floor").clamp(0, 65535)
    return code(base + rv * v * ys), code(base - (gu * u + gv * v) * ys), code(base + bu * u * ys)


def planar_codes_torch(planes: torch.Tensor, sub: str, bits: int, T: int, H: int, W: int, matrix: str = "bt709", range_: str = "tv",
                       siting: str = "left") -> torch.Tensor:
    check_arguments(planes, sub, bits, T, H, W, matrix, range_, siting)
    hc, wc = chroma_dims(sub, H, W)
    s = planes.reshape(T, -1).to(torch.int64).clamp(max=(1 << bits) - 1)
    Y = s[:, :H * W].reshape(T, H, W)
    cb8 = upsample_chroma(s[:, H * W:H * W + hc * wc].reshape(T, hc, wc), sub, siting, H, W)
    cr8 = upsample_chroma(s[:, H * W + hc * wc:].reshape(T, hc, wc), sub, siting, H, W)
    q = torch.stack(yuv_codes(Y, cb8, cr8, bits, matrix, range_), dim=-1)
    return q.to(torch.int32).to(torch.uint16).contiguous()


def planar_codes(planes: torch.Tensor, sub: str, bits: int, T: int, H: int, W: int, matrix: str = "bt709", range_: str = "tv",
                 siting: str = "left", ops=None, out: torch.Tensor = None) -> torch.Tensor:
    """The rgb16 codes.  ``ops.planar_codes`` (HipOps: csrc/svr_planar.hip) where the backend has it -- a failing library raises,
    there is no fall-back from it -- else the torch statement above.  ``out``: a uint16 tensor [T, H, W, 3]."""
    if ops is not None and hasattr(ops, "planar_codes"):
        return ops.planar_codes(planes, sub, bits, T, H, W, matrix, range_, siting, out=out)
    codes = planar_codes_torch(planes, sub, bits, T, H, W, matrix, range_, siting)
    if out is None:
        return codes
    if out.dtype != torch.uint16 or tuple(out.shape) != (T, H, W, 3):
        raise ValueError(f"out must be torch.uint16 {(T, H, W, 3)}, got {out.dtype} {tuple(out.shape)}")
    out.copy_(codes)
    return out
