"""Input frames as a decoder emits them, widened to fp32: the packed formats, stated once, in plain torch.  The inverse of frameio.py.

This module is the specification of the kernels in csrc/svr_frame_unpack.hip (equal bit for bit: every result is an integer code
over a full scale, no tolerance) and the path taken when ``ops`` has no ``unpack_frames`` (the fp32 torch double of the C ABI that
drives the CPU tests).  Any device.

``unpack_frames_torch(packed, fmt, T, H, W, C, matrix, range_)`` -> fp32 [T, H, W, C], nominally in [0, 1].  With h2 = ceil(H/2),
w2 = ceil(W/2):

  "rgb8" / "bgr8"   uint8 [T, H, W, C], C = 3 or 4 (ffmpeg's rgb24 / rgba, bgr24 / bgra): q the stored sample, D = 255.  "bgr8" swaps
                    channels 0 and 2 back; a fourth channel stays in place.
  "rgb16"           uint16 [T, H, W, C], C = 3 or 4 (rgb48le / rgba64le): q the stored sample, D = 65535.
  "yuv420p8"        C = 3.  uint8 [T, H*W + 2*h2*w2]: per frame the Y plane row-major, then Cb, then Cr (yuv420p / yuvj420p rawvideo,
                    frameio.py's plane layout).  D = 65535.
  "yuv420p10"       the same layout in uint16 (yuv420p10le).  A sample above 1023 -- the container has room for it, a decoder never
                    writes it -- counts as 1023, so the bound on the numerators below holds for any bytes.

Every value is the fp32 number nearest to q / D: ONE floating-point operation, after exact integers.  (Not q * (1 / D): that is not
the nearest value, a kernel contracted to fma would differ again, and on a GPU torch divides a tensor by a Python scalar exactly
that way -- hence the division by a TENSOR below, in fp64: 53 >= 2 * 24 + 2 bits, so rounding twice is harmless.)

The yuv formats, ``matrix`` "bt709" | "bt601", ``range_`` "tv" | "pc", n = 8 or 10 bits:

  chroma    4:2:0 with the MPEG-2 / H.264 / HEVC default siting: co-sited with even luma columns, midway between luma rows.
            Upsampled bilinearly in integers, indices clamped to the plane.  Vertically, in quarters: luma row 2j takes
            C[j-1] + 3 C[j], row 2j+1 takes 3 C[j] + C[j+1].  Horizontally: column 2k takes twice the vertical value at k, column
            2k+1 the sum of the values at k and k+1.  That is cb8, cr8: weights summing to 8.
  constants tv: y0 = 16 << (n-8), ys = 219 << (n-8), cs = 224 << (n-8);  pc: y0 = 0, ys = cs = 2^n - 1.  mid = 8 * 2^(n-1),
            u = cb8 - mid, v = cr8 - mid.  Coefficients rounded at 2^16 from the exact decimal Kr, Kb (as the pack's luma weights):
            bt709 rv = 103206, bu = 121609, gv = 30679, gu = 12276;  bt601 rv = 91881, bu = 116130, gv = 46802, gu = 22553.
  matrix    Den   = ys * 8 * cs * 65536
            base  = (Y - y0) * 8 * cs * 65536
            num_R = 65535 * (base + rv * v * ys)
            num_G = 65535 * (base - (gu * u + gv * v) * ys)
            num_B = 65535 * (base + bu * u * ys)
            q     = clamp(floor((2 * num + Den) / (2 * Den)), 0, 65535)
            Every |num| is below 6.1e16 < 2^62.  Numerators CAN be negative (Y below y0, saturated chroma): the division is a
            FLOOR division -- a kernel with a truncating or unsigned division must clamp at zero before it divides.

Check values (16-bit codes; tests/test_frame_unpack.py), 10-bit tv bt709 unless said:
  (940, 512, 512) -> white (65535, 65535, 65535)      (64, 512, 512) -> (0, 0, 0)      (502, 512, 512) -> (32768, 32768, 32768)
  the pack's red (250, 409, 960) -> (65517, 0, 0)     green (691, 167, 105) -> (27, 65535, 83)     blue (127, 960, 471) -> (0, 0, 65517)
  8-bit tv (235, 128, 128), 8-bit pc (255, 128, 128), 10-bit pc (1023, 512, 512) -> white
"""
import torch

FORMATS = ("rgb8", "bgr8", "rgb16", "yuv420p8", "yuv420p10")
MATRICES = {"bt709": (103206, 12276, 30679, 121609), "bt601": (91881, 22553, 46802, 116130)}      # rv, gu, gv, bu
RANGES = ("tv", "pc")
_BITS = {"yuv420p8": 8, "yuv420p10": 10}


def packed_dtype(fmt: str) -> torch.dtype:
    return torch.uint16 if fmt in ("rgb16", "yuv420p10") else torch.uint8


def packed_shape(T: int, H: int, W: int, C: int, fmt: str):
    """Shape of the packed clip; raises for an unknown format or a channel count the format does not take."""
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {FORMATS}, got {fmt!r}")
    if fmt in _BITS:
        if C != 3:
            raise ValueError(f"{fmt} takes C = 3 (it has no alpha plane), got C = {C}")
        return (T, H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2))
    if C not in (3, 4):
        raise ValueError(f"{fmt} takes C = 3 or 4, got C = {C}")
    return (T, H, W, C)


def frame_bytes(H: int, W: int, C: int, fmt: str) -> int:
    n = 1
    for s in packed_shape(1, H, W, C, fmt):
        n *= s
    return n * (2 if packed_dtype(fmt) == torch.uint16 else 1)


def check_arguments(packed, fmt, T, H, W, C, matrix, range_):
    """The refusals shared by the torch statement and HipOps.unpack_frames, each naming its argument; -> the packed shape."""
    shape = packed_shape(T, H, W, C, fmt)
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {tuple(MATRICES)}, got {matrix!r}")
    if range_ not in RANGES:
        raise ValueError(f"range_ must be one of {RANGES}, got {range_!r}")
    if T < 1 or H < 1 or W < 1:
        raise ValueError(f"T, H, W must be positive, got T = {T}, H = {H}, W = {W}")
    if packed.dtype != packed_dtype(fmt):
        raise ValueError(f"packed must be {packed_dtype(fmt)} for {fmt}, got {packed.dtype}")
    numel = 1
    for s in shape:
        numel *= s
    if packed.numel() != numel:
        raise ValueError(f"packed must hold {numel} samples ({tuple(shape)}) for {fmt} at T, H, W, C = {T}, {H}, {W}, {C}, "
                         f"got {tuple(packed.shape)}")
    return shape


def yuv_constants(bits: int, range_: str):
    """-> (y0, ys, cs, mid)"""
    if range_ == "tv":
        return 16 << (bits - 8), 219 << (bits - 8), 224 << (bits - 8), 8 << (bits - 1)
    return 0, (1 << bits) - 1, (1 << bits) - 1, 8 << (bits - 1)


def yuv_codes(Y, cb8, cr8, bits: int, matrix: str = "bt709", range_: str = "tv"):
    """The matrix of the module docstring on int64 tensors: Y a sample, cb8 / cr8 the upsampled chroma over 8 -> (R, G, B) 16-bit codes."""
    rv, gu, gv, bu = MATRICES[matrix]
    y0, ys, cs, mid = yuv_constants(bits, range_)
    den = ys * 8 * cs * 65536
    base = (Y - y0) * (8 * cs * 65536)
    u, v = cb8 - mid, cr8 - mid

    def code(s):                                     # (floor division: the numerator can be negative)
        return torch.div(2 * 65535 * s + den, 2 * den, rounding_mode="floor").clamp(0, 65535)
    return code(base + rv * v * ys), code(base - (gu * u + gv * v) * ys), code(base + bu * u * ys)


def upsample_chroma(c, H: int, W: int):
    """int64 [T, h2, w2] -> [T, H, W]: the chroma plane at every luma position, times 8."""
    h2, w2 = c.shape[1], c.shape[2]
    y = torch.arange(H, device=c.device)
    j = y // 2
    other = torch.where(y % 2 == 0, j - 1, j + 1).clamp(0, h2 - 1)
    v = 3 * c[:, j] + c[:, other]                                          # [T, H, w2], in quarters
    x = torch.arange(W, device=c.device)
    k = x // 2
    return v[:, :, k] + v[:, :, (k + x % 2).clamp(max=w2 - 1)]


def unit(q, D: int):
    """The fp32 value nearest to q / D (q int64): through fp64, divided by a TENSOR (see the module docstring)."""
    return (q.double() / torch.full((), float(D), dtype=torch.float64, device=q.device)).float()


def unpack_frames_torch(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, matrix: str = "bt709",
                        range_: str = "tv") -> torch.Tensor:
    check_arguments(packed, fmt, T, H, W, C, matrix, range_)
    if fmt not in _BITS:
        q = packed.reshape(T, H, W, C).to(torch.int64)
        if fmt == "bgr8":
            q = q[..., [2, 1, 0] + ([3] if C == 4 else [])]
        return unit(q, 65535 if fmt == "rgb16" else 255).contiguous()
    bits = _BITS[fmt]
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    s = packed.reshape(T, -1).to(torch.int64).clamp(max=(1 << bits) - 1)
    Y = s[:, :H * W].reshape(T, H, W)
    cb8 = upsample_chroma(s[:, H * W:H * W + h2 * w2].reshape(T, h2, w2), H, W)
    cr8 = upsample_chroma(s[:, H * W + h2 * w2:].reshape(T, h2, w2), H, W)
    return unit(torch.stack(yuv_codes(Y, cb8, cr8, bits, matrix, range_), dim=-1), 65535).contiguous()


def unpack_frames(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, matrix: str = "bt709", range_: str = "tv",
                  ops=None, out: torch.Tensor = None) -> torch.Tensor:
    """The fp32 frames.  ``ops.unpack_frames`` (HipOps: csrc/svr_frame_unpack.hip) where the backend has it -- a failing library
    raises, there is no fall-back from it -- else the torch statement above.  ``out``: an fp32 tensor [T, H, W, C]."""
    if ops is not None and hasattr(ops, "unpack_frames"):
        return ops.unpack_frames(packed, fmt, T, H, W, C, matrix, range_, out=out)
    frames = unpack_frames_torch(packed, fmt, T, H, W, C, matrix, range_)
    if out is None:
        return frames
    if out.dtype != torch.float32 or tuple(out.shape) != (T, H, W, C):
        raise ValueError(f"out must be torch.float32 {(T, H, W, C)}, got {out.dtype} {tuple(out.shape)}")
    out.copy_(frames)
    return out
