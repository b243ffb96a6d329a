"""Output frames narrowed for the encoder: the packed formats, stated once, in plain torch.

This module is the specification of the kernels in csrc/svr_frame_pack.hip (equal bit for bit: integer results, no tolerance) and
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

Non-finite input, explicitly: NaN -> code 0 (the kernels' fmaxf(NaN, 0) = 0), +inf -> full scale, -inf -> 0, in every format.
"""
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
