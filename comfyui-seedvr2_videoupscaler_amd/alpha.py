"""Edge-guided alpha upscaling: the reference's ``edge_guided_alpha_upscale(method='guided')`` restated once, in plain torch.

Reference: src/core/alpha_upscaling.py:289-438 (with detect_edges_batch :125-188 and the guided filter :191-286).  The input's
alpha channel is upsampled (bicubic, antialiased) and refined by a guided filter whose guide is the UPSCALED RGB; for a binary
matte the result is then snapped / sharpened around a Sobel edge map of the upscaled frames.

This module is the specification of the kernels in csrc/svr_alpha.hip and the path taken when ``ops`` has no ``alpha_upscale``
(the fp32 torch double of the C ABI that drives the CPU tests).  No cv2, no numpy round trip, any device.  What the reference
computes through OpenCV on the host is restated as exact integer arithmetic:

  * batch statistics over ONE call (the frames of one written span):
      is_binary = (count(a < 0.1) + count(a > 0.9)) / numel > 0.95     (fp32; counts converted before the addition)
      neg0 = min(rgb) < 0 -> the frames are normalised (x + 1) / 2;  neg1 = min(rgb) < -1 -> detect_edges_batch tests
      min < 0 AGAIN on the normalised frames, so with decoder overshoot below -1 the edge detector's image is normalised twice
      (the guided filter's guide once).  Reproduced, not repaired.
  * edge map: u = trunc(clip(x * 255, 0, 255)) in fp32; gray = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's 8-bit
    RGB2GRAY); 3x3 Sobel with BORDER_REFLECT_101; n = sx^2 + sy^2 (int, <= 2 080 800); e = trunc(sqrt(n) / sqrt(max n) * 255) in
    fp64 in THIS order (at exact ties it differs from sqrt(n / max n)); edge = e / 255 in fp32.  A constant frame (0 / 0 in the
    reference) is defined as e = 0.
  * guided filter: radius 2 (binary) / 3, eps 0.002; box means are avg_pool2d with zero padding and a fixed divisor, and the
    second pooling sees a and b as zero outside the image -- so a uniform alpha of 1 comes out BELOW 1 at the border.
"""
import torch
import torch.nn.functional as F

EPS = 0.002


def batch_flags(rgb_thwc: torch.Tensor, alpha_lo: torch.Tensor):
    """-> (is_binary, neg0, neg1) as Python bools (the kernels keep them on the device)."""
    a = alpha_lo.float().flatten()
    near_zero = (a < 0.1).sum().float()
    near_one = (a > 0.9).sum().float()
    is_binary = bool((near_zero + near_one) / a.numel() > 0.95)
    lo = rgb_thwc.float().min()
    return is_binary, bool(lo < 0), bool(lo < -1)


def sobel_energy(rgb_thwc: torch.Tensor, neg0: bool, neg1: bool) -> torch.Tensor:
    """n = sx^2 + sy^2 of the 8-bit gray frames, int32 [T, H, W]."""
    x = rgb_thwc.float()
    if neg0:
        x = (x + 1) / 2
    if neg1:
        x = (x + 1) / 2
    u = (x * 255).clamp(0, 255).to(torch.int32)                          # (.to(int) truncates, as astype(uint8) on [0, 255])
    gray = (4899 * u[..., 0] + 9617 * u[..., 1] + 1868 * u[..., 2] + 8192) >> 14
    g = F.pad(gray.float().unsqueeze(1), (1, 1, 1, 1), mode="reflect").squeeze(1).to(torch.int32)   # reflect = REFLECT_101
    H, W = gray.shape[1:]
    win = lambda dy, dx: g[:, dy:dy + H, dx:dx + W]
    sx = (win(0, 2) + 2 * win(1, 2) + win(2, 2)) - (win(0, 0) + 2 * win(1, 0) + win(2, 0))
    sy = (win(2, 0) + 2 * win(2, 1) + win(2, 2)) - (win(0, 0) + 2 * win(0, 1) + win(0, 2))
    return sx * sx + sy * sy


def edge_bytes(n: torch.Tensor, nmax: torch.Tensor = None) -> torch.Tensor:
    """(edge / edge.max() * 255).astype(uint8) per frame from n [T, H, W]; ``nmax`` [T, 1, 1]: the frames' maxima (default: of n)."""
    if nmax is None:
        nmax = n.amax(dim=(1, 2), keepdim=True)
    e = (n.double().sqrt() / nmax.double().sqrt() * 255.0)
    return torch.where(nmax > 0, e, torch.zeros_like(e)).to(torch.uint8)


def guided_filter(guide: torch.Tensor, src: torch.Tensor, radius: int, eps: float = EPS) -> torch.Tensor:
    """guide, src [T, H, W] -> [T, H, W]; _apply_guided_filter's operation order."""
    I, p = guide.unsqueeze(1), src.unsqueeze(1)
    box = lambda x: F.avg_pool2d(x, kernel_size=2 * radius + 1, stride=1, padding=radius)
    mean_I, mean_p = box(I), box(p)
    var = box(I * I) - mean_I * mean_I
    cov = box(I * p) - mean_I * mean_p
    a = cov / (var + eps)
    b = mean_p - a * mean_I
    return (box(a) * I + box(b)).squeeze(1)


def binary_tail(q: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    """Steps 3-8 of the reference for a binary matte: q the guided filter's output, n the Sobel energy, both [T, H, W].
    (The 3x3 max-pool runs on n: the edge byte is monotone in it.)"""
    nmax = n.amax(dim=(1, 2), keepdim=True)
    edge = edge_bytes(n, nmax).float() / 255.0
    pooled = F.max_pool2d(n.float().unsqueeze(1), kernel_size=3, stride=1, padding=1).squeeze(1).to(n.dtype)   # (n < 2^24: exact)
    zone = edge_bytes(pooled, nmax).float() / 255.0
    contrast = torch.sigmoid((q - 0.5) * 12.0)
    strength = torch.clamp(edge / 0.25, 0, 1)
    in_edges = q * (1 - strength) + contrast * strength
    out = torch.where(zone < 0.05, (q > 0.5).float(), in_edges)
    out = torch.where(zone < 0.03, (out > 0.5).float(), out)
    snap = (out > 0.3) & (out < 0.7) & ~(edge > 0.15)
    return torch.where(snap, (out > 0.5).float(), out)


def bicubic_base(alpha_lo: torch.Tensor, H: int, W: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """alpha [T, h, w] -> [T, H, W] fp32: the reference's step 1 (the input transform uses the same op)."""
    return F.interpolate(alpha_lo.to(dtype).unsqueeze(1), size=(H, W), mode="bicubic", align_corners=False,
                         antialias=True).clamp(0, 1).squeeze(1)


def fragile_pixels(q: torch.Tensor, n: torch.Tensor, is_binary: bool, shift: float = 1e-4, moved: float = 1e-3) -> torch.Tensor:
    """Pixels whose result a shift of the guided filter's output by +-``shift`` moves by more than ``moved``: the ones that sit on
    one of the tail's thresholds (a flip moves a pixel by tenths; the smooth part by at most 3 * shift, the sigmoid's slope).  What
    a comparison of two realisations of this arithmetic has to leave out; none for a soft matte, whose tail is the identity."""
    if not is_binary:
        return torch.zeros_like(q, dtype=torch.bool)
    mid = binary_tail(q, n).clamp(0, 1)
    return ((binary_tail(q + shift, n).clamp(0, 1) - mid).abs() > moved) | ((binary_tail(q - shift, n).clamp(0, 1) - mid).abs() > moved)


def upscale_alpha_torch(rgb_thwc: torch.Tensor, alpha_lo: torch.Tensor, base: torch.Tensor = None, parts: dict = None,
                        dtype: torch.dtype = torch.float32):
    """rgb [T, H, W, 3] (upscaled, [-1, 1] or [0, 1]), alpha_lo [T, h, w] in [0, 1] -> alpha [T, H, W] in [0, 1].
    ``base``: a precomputed bicubic base; ``parts`` (a dict) receives the intermediate results (edge bytes, n, q, flags);
    ``dtype``: fp32 as the reference computes, or fp64 for the floating-point part (base, guide, guided filter, tail) -- the
    batch statistics and the edge map are integer results of the fp32 input and do not change with it."""
    rgb = rgb_thwc[..., :3].float()
    T, H, W, _ = rgb.shape
    if H < 2 or W < 2:
        raise ValueError("alpha upscaling needs frames of at least 2 x 2 pixels (the Sobel border reflects)")
    is_binary, neg0, neg1 = batch_flags(rgb, alpha_lo)
    n = sobel_energy(rgb, neg0, neg1)
    if base is None:
        base = bicubic_base(alpha_lo.float(), H, W, dtype)
    x = rgb.to(dtype)
    if neg0:
        x = (x + 1) / 2
    guide = (x[..., 0] + x[..., 1] + x[..., 2]) / 3
    q = guided_filter(guide, base.to(dtype), 2 if is_binary else 3)
    out = binary_tail(q, n) if is_binary else q
    if parts is not None:
        parts.update(is_binary=is_binary, neg0=neg0, neg1=neg1, n=n, edge=edge_bytes(n), base=base, q=q)
    return out.clamp(0, 1)


def upscale_alpha(rgb_thwc: torch.Tensor, alpha_lo: torch.Tensor, ops=None) -> torch.Tensor:
    """The alpha of one batch of upscaled frames.  ``ops.alpha_upscale`` (HipOps: csrc/svr_alpha.hip) where the backend has it --
    a failing library raises, there is no fall-back from it -- else the torch restatement above."""
    if ops is not None and hasattr(ops, "alpha_upscale"):
        return ops.alpha_upscale(rgb_thwc, alpha_lo)
    return upscale_alpha_torch(rgb_thwc, alpha_lo)
