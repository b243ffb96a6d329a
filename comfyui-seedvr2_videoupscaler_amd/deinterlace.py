"""Interlaced sources: the two fields of a woven frame turned into progressive frames, on the packed planes as the decoder emits
them, in exact integers, stated once in plain torch.

This module is the specification of the kernels in csrc/svr_deinterlace.hip (equal bit for bit: integers in, integers out, no
tolerance) and the path taken when ``ops`` has no ``deinterlace`` (the torch double of the C ABI that drives the CPU tests).  Any
device.  It runs BEFORE frameio_in.unpack_frames, on 1.5 to 6 bytes per pixel instead of the 12 of the fp32 frames, plane by plane:
the chroma planes of interlaced 4:2:0 have their own field structure (chroma row r belongs to field r % 2), which is lost once
unpack has interpolated chroma rows across the two fields; a 10-bit source keeps its 10 bits.

``deinterlace_torch(packed, fmt, T, H, W, C, order, rate, before=None, after=None)`` -> the packed clip of T (``rate`` "frame") or
2T (``rate`` "field") frames, same dtype and layout.  Formats, shapes and dtypes are frameio_in's.

planes    ``planes(fmt, H, W, C)`` -> [(offset, rows R, samples per row N, step s)] in elements of one frame.  rgb8 / bgr8 / rgb16:
          one plane (0, H, W*C, C) -- the neighbour COLUMN of a sample is s = C elements away.  yuv420p8 / yuv420p10, h2 =
          ceil(H/2), w2 = ceil(W/2): Y (0, H, W, 1), Cb (H*W, h2, w2, 1), Cr (H*W + h2*w2, h2, w2, 1).  In every plane row r
          belongs to field r % 2.  Samples are used as stored (a 10-bit sample above 1023 is not clamped); every result lies
          between the smallest and the largest input sample, so the container never overflows.
order     "tff": the first field in time is the even rows (parity 0); "bff": parity 1.
rate      "frame": output t keeps the first field of frame t.  "field": output 2t keeps the first field of frame t, output 2t + 1
          the second.
context   ``before`` / ``after``: one packed frame each, the frame ahead of the clip and the frame behind it (streaming).  Where
          none is given F[-1] := F[min(1, T-1)] and F[T] := F[max(T-2, 0)]: a MIRROR, not a clamp -- a clamp would manufacture
          "static" evidence and weave the first and the last field of a moving clip.

The rule, per plane, for the output that keeps parity p of frame t, k = 0 if that is the frame's first field, else 1.  Integers of
at least 32 bits; >> is an arithmetic shift of a non-negative number.
  rows r with r % 2 == p, and the only row of a plane with R == 1: copied from cur = F[t].
  every other row r, per sample i:
    up = r-1 if r >= 1 else r+1;  dn = r+1 if r+1 < R else r-1;  P = F[t-1], Nx = F[t+1];  B = F[t-1+k], A = F[t+k] (the fields
    of the missing parity just before and just after the kept one);  c = cur[up][i], e = cur[dn][i]
    temporal   d  = (B[r][i] + A[r][i]) >> 1
               t0 = |B[r][i] - A[r][i]| >> 1
               t1 = (|P[up][i] - c| + |P[dn][i] - e|) >> 1
               t2 = (|Nx[up][i] - c| + |Nx[dn][i] - e|) >> 1
               diff = max(t0, t1, t2)
    spatial    sp = (c + e) >> 1.  Only where i - 3s >= 0 and i + 3s <= N - 1, the edge search:
               score(j) = sum over q in {-1, 0, 1} of |cur[up][i + (q+j)s] - cur[dn][i + (q-j)s]|
               pred(j)  = (cur[up][i + js] + cur[dn][i - js]) >> 1
               best = score(0) - 1;  two passes, (j1, j2) = (-1, -2) then (1, 2):  if score(j1) < best: best = score(j1),
               sp = pred(j1), and ONLY then, if score(j2) < best: best = score(j2), sp = pred(j2)
    result     min(max(sp, d - diff), d + diff)
A motion-adaptive, edge-directed rule of the yadif family WITHOUT its spatial-interlacing check: with that check left out a static
picture comes back exactly (diff = 0 there, the result is d = the stored row).  The rule is defined by this text; it is not claimed
equal to any ffmpeg filter's bytes.

``ENABLED`` is False: the command line deinterlaces (in ``RATE``) only where this switch is set and ffprobe's field_order tag names
an order (``field_order``).  It ships off because
  * encoders mis-tag progressive material as interlaced often enough, and deinterlacing such a clip costs vertical detail wherever
    something moves;
  * nothing here checks the tag against the picture;
  * the rule has met synthetic clips only (tests/test_deinterlace.py), no broadcast capture, DVD or DV tape.
Known limits:
  * no comb detection: a progressive clip tagged interlaced is treated as interlaced, an interlaced one tagged progressive is
    upscaled as stored (the command line says so once);
  * no telecine / pulldown handling: 3:2 material comes out with its repeated fields interpolated, not matched;
  * a one-frame clip has no temporal neighbour but itself and comes back woven;
  * the field order is taken for the whole clip; a stream that changes order midway is not followed.
fieldmatch.py answers the first two: it counts the combing of every stored frame and hands only the frames without a clean weave to
the rule above.
"""
import torch

from . import frameio_in

ORDERS = ("tff", "bff")
RATES = ("frame", "field")
ENABLED = False
RATE = "field"
_YUV = ("yuv420p8", "yuv420p10")


def planes(fmt: str, H: int, W: int, C: int):
    """-> [(offset, rows, samples per row, step)] of one packed frame, in elements"""
    if fmt in _YUV:
        h2, w2 = (H + 1) // 2, (W + 1) // 2
        return [(0, H, W, 1), (H * W, h2, w2, 1), (H * W + h2 * w2, h2, w2, 1)]
    return [(0, H, W * C, C)]


def field_order(tag):
    """ffprobe's field_order -> "tff" | "bff" | None (progressive, unknown, absent)."""
    return {"tt": "tff", "tb": "tff", "bb": "bff", "bt": "bff"}.get(tag)


def check_arguments(packed, fmt, T, H, W, C, order, rate, before=None, after=None):
    """The refusals shared by the torch statement and HipOps.deinterlace, each naming its argument; -> the packed shape."""
    shape = frameio_in.packed_shape(T, H, W, C, fmt)
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    if rate not in RATES:
        raise ValueError(f"rate must be one of {RATES}, got {rate!r}")
    if T < 1 or H < 1 or W < 1:
        raise ValueError(f"T, H, W must be positive, got T = {T}, H = {H}, W = {W}")
    dtype = frameio_in.packed_dtype(fmt)
    if packed.dtype != dtype:
        raise ValueError(f"packed must be {dtype} for {fmt}, got {packed.dtype}")
    numel = 1
    for s in shape:
        numel *= s
    if packed.numel() != numel:
        raise ValueError(f"packed must hold {numel} samples ({tuple(shape)}) for {fmt} at T, H, W, C = {T}, {H}, {W}, {C}, "
                         f"got {tuple(packed.shape)}")
    for name, frame in (("before", before), ("after", after)):
        if frame is None:
            continue
        if frame.dtype != dtype:
            raise ValueError(f"{name} must be {dtype} for {fmt}, got {frame.dtype}")
        if frame.numel() != numel // T:
            raise ValueError(f"{name} must hold the {numel // T} samples of one {fmt} frame at H, W, C = {H}, {W}, {C}, "
                             f"got {tuple(frame.shape)}")
    return shape


def _plane(X, R: int, N: int, s: int, p0: int, fields: int):
    """X int32 [T + 2, R, N]: the plane of F[-1] .. F[T] -> int32 [T, fields, R, N]"""
    T = X.shape[0] - 2
    cur, P, Nx = X[1:T + 1], X[0:T], X[2:T + 2]
    if R == 1:
        return cur[:, None].expand(T, fields, R, N)
    r = torch.arange(R, device=X.device)
    up = torch.where(r >= 1, r - 1, r + 1)
    dn = torch.where(r + 1 < R, r + 1, r - 1)
    c, e = cur[:, up], cur[:, dn]
    # spatial prediction: the same for both fields of a frame (only the rows that use it differ)
    sp = (c + e) >> 1
    if N >= 6 * s + 1:
        pad = torch.nn.functional.pad
        cu, ce = pad(c, (3 * s, 3 * s)), pad(e, (3 * s, 3 * s))
        at = lambda x, m: x[..., (3 + m) * s:(3 + m) * s + N]                   # x[i + m s]
        score = lambda j: sum((at(cu, q + j) - at(ce, q - j)).abs() for q in (-1, 0, 1))
        pred = lambda j: (at(cu, j) + at(ce, -j)) >> 1
        best, found = score(0) - 1, sp
        for j1, j2 in ((-1, -2), (1, 2)):
            s1 = score(j1)
            m1 = s1 < best
            best, found = torch.where(m1, s1, best), torch.where(m1, pred(j1), found)
            s2 = score(j2)
            m2 = m1 & (s2 < best)
            best, found = torch.where(m2, s2, best), torch.where(m2, pred(j2), found)
        i = torch.arange(N, device=X.device)
        sp = torch.where((i - 3 * s >= 0) & (i + 3 * s <= N - 1), found, sp)
    t1 = ((P[:, up] - c).abs() + (P[:, dn] - e).abs()) >> 1
    t2 = ((Nx[:, up] - c).abs() + (Nx[:, dn] - e).abs()) >> 1
    outs = []
    for k in range(fields):
        B, A = (P, cur) if k == 0 else (cur, Nx)
        d = (B + A) >> 1
        diff = torch.maximum(torch.maximum((B - A).abs() >> 1, t1), t2)
        new = torch.minimum(torch.maximum(sp, d - diff), d + diff)
        keep = (r % 2 == (p0 if k == 0 else 1 - p0))[None, :, None]
        outs.append(torch.where(keep, cur, new))
    return torch.stack(outs, dim=1)


def deinterlace_torch(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, order: str, rate: str,
                      before: torch.Tensor = None, after: torch.Tensor = None) -> torch.Tensor:
    shape = check_arguments(packed, fmt, T, H, W, C, order, rate, before, after)
    fields = 2 if rate == "field" else 1
    F = packed.reshape(T, -1)
    first = before.reshape(1, -1) if before is not None else F[min(1, T - 1)][None]
    last = after.reshape(1, -1) if after is not None else F[max(T - 2, 0)][None]
    X = torch.cat([first, F, last]).to(torch.int32)                             # (torch has few uint16 ops: widened, as frameio_in does)
    out = torch.empty((T, fields, F.shape[1]), dtype=torch.int32, device=packed.device)
    for off, R, N, s in planes(fmt, H, W, C):
        out[:, :, off:off + R * N] = _plane(X[:, off:off + R * N].reshape(T + 2, R, N), R, N, s, ORDERS.index(order),
                                            fields).reshape(T, fields, R * N)
    return out.to(packed.dtype).reshape((T * fields,) + tuple(shape[1:]))


def deinterlace(packed: torch.Tensor, fmt: str, T: int, H: int, W: int, C: int, order: str, rate: str, before: torch.Tensor = None,
                after: torch.Tensor = None, ops=None, out: torch.Tensor = None) -> torch.Tensor:
    """The progressive packed clip.  ``ops.deinterlace`` (HipOps: csrc/svr_deinterlace.hip) where the backend has it -- a failing
    library raises, there is no fall-back from it -- else the torch statement above.  ``out``: a tensor of the packed dtype and the
    shape of the result."""
    if ops is not None and hasattr(ops, "deinterlace"):
        return ops.deinterlace(packed, fmt, T, H, W, C, order, rate, before=before, after=after, out=out)
    frames = deinterlace_torch(packed, fmt, T, H, W, C, order, rate, before, after)
    if out is None:
        return frames
    if out.dtype != frames.dtype or tuple(out.shape) != tuple(frames.shape):
        raise ValueError(f"out must be {frames.dtype} {tuple(frames.shape)}, got {out.dtype} {tuple(out.shape)}")
    out.copy_(frames)
    return out
