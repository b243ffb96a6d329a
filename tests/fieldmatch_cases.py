"""TEST INFRASTRUCTURE shared by tests/test_fieldmatch.py and tests/test_gpu_fieldmatch.py: a per-sample restatement of field
matching in plain Python integers (written from the text of fieldmatch.py's docstring, sharing no code with the torch statement),
the clip builders -- progressive, 3:2 telecined and interlaced clips of a smooth textured object moving over a static gradient --
and the shape list.

The property geometry.  Noise is at most +-3 codes, so a sample of a progressive picture differs from its vertical neighbours'
range by at most 6 + the picture's own vertical slope (1 code a row): far under THR = 12, every progressive peak is 0 <= MI * s.
A mixed frame's two fields show the object SPEED = 2 .. 3 columns apart: along each of its two vertical edges (contrast >= 35
codes) every tested row has SPEED combed pixels; the object spans at least 4 tested rows of one block row at 18 x 40, so a block
holds at least 8 s > MI * s = 6 s combed samples.  8 x 32 and 6 x 20 are too small (the combed counts stay under MI): 18 x 40 is the
smallest shape of the property tests."""
import itertools

import torch

from deinterlace_cases import (CONTEXTS, FORMATS, SHAPES as DEINT_SHAPES, channel_counts, context, plane_list, random_packed,  # noqa: F401
                               weave)

# deinterlace_cases' shapes ((2, 2, 9) and the one-row planes among them: no tested row; (3, 17, 33): two block rows, the second with
# one row, three block columns, the last with one pixel), plus: a third block row and rows of whole 16-byte units (3, 34, 48), and
# the property geometry (5, 18, 40), and a row of 33 block columns (2, 5, 528): on the vector route a workgroup of the counts kernel
# owns at most 32 block columns of an rgb16 row with C = 4, so that row takes two workgroups
SHAPES = DEINT_SHAPES + [(3, 34, 48), (5, 18, 40), (2, 5, 528)]
ORDERS = ("tff", "bff")
THR, MI = 12, 6                                       # the property tests' own parameters (never fieldmatch.DEFAULTS)
GEOMETRIES = ((18, 40, 2), (34, 70, 3))               # rows, columns, columns the object moves per picture
SHIFT = {"rgb8": 0, "bgr8": 0, "yuv420p8": 0, "yuv420p10": 2, "rgb16": 8}


# ---------------------------------------------------------------------------------------------------------------- restatement
def _frame(F, j, before, after):
    T = len(F)
    if j < 0:
        return before if before is not None else F[min(1, T - 1)]
    if j >= T:
        return after if after is not None else F[max(T - 2, 0)]
    return F[j]


def loop_counts(F, R, N, s, order, thr_code, before=None, after=None):
    """F: T frames of plane 0, each R rows of N ints -> [T][3][2]: (total, peak) of the candidates cur, prev, next."""
    p = ORDERS.index(order)
    out = []
    for t in range(len(F)):
        cur = F[t]
        per_frame = []
        for X in (cur, _frame(F, t - 1, before, after), _frame(F, t + 1, before, after)):
            blocks = {}
            for r in range(1, R - 1):
                if r % 2 != 1 - p:
                    continue
                for i in range(N):
                    u, l, m = cur[r - 1][i], cur[r + 1][i], X[r][i]
                    if m < min(u, l) - thr_code or m > max(u, l) + thr_code:
                        key = (r // 16, (i // s) // 16)
                        blocks[key] = blocks.get(key, 0) + 1
            per_frame.append([sum(blocks.values()), max(blocks.values(), default=0)])
        out.append(per_frame)
    return out


def loop_modes(cnt, mi, s):
    modes = []
    for (_, pc), (_, pa), (_, pb) in cnt:
        if pc <= mi * s:
            modes.append(0)
            continue
        q, m = (pa, 1) if pa <= pb else (pb, 2)
        modes.append(m if q <= mi * s else 3)
    return modes


def loop_select_plane(F, D, modes, R, order, before=None, after=None):
    """one plane: F the stored frames, D the deinterlaced ones (lists of rows) -> the output frames"""
    p = ORDERS.index(order)
    out = []
    for t, mode in enumerate(modes):
        if mode == 3:
            out.append([list(row) for row in D[t]])
            continue
        other = _frame(F, t + (0, -1, 1)[mode], before, after)
        out.append([list(F[t][r]) if (r % 2 == p or R == 1) else list(other[r]) for r in range(R)])
    return out


def cut_planes(packed, fmt, T, H, W, C):
    """packed [T, ...] (or one frame, T = 1) -> per plane of plane_list: (R, N, s, [T frames of R rows of N ints])"""
    flat = packed.reshape(T, -1).to(torch.int64).tolist()
    return [(R, N, s, [[f[off + r * N:off + (r + 1) * N] for r in range(R)] for f in flat]) for off, R, N, s in plane_list(fmt, H, W, C)]


def loop_comb_counts(packed, fmt, T, H, W, C, order, thr, before=None, after=None):
    """-> int32 [T, 3, 2] through loop_counts (plane 0 only)"""
    R, N, s, F = cut_planes(packed, fmt, T, H, W, C)[0]
    ctx = [None if x is None else cut_planes(x, fmt, 1, H, W, C)[0][3][0] for x in (before, after)]
    return torch.tensor(loop_counts(F, R, N, s, order, thr << SHIFT[fmt], *ctx), dtype=torch.int32).reshape(T, 3, 2)


def loop_select(packed, deint, modes, fmt, T, H, W, C, order, before=None, after=None):
    """-> a tensor like packed through loop_select_plane, plane by plane; ``modes`` a list of ints"""
    stored, dei = cut_planes(packed, fmt, T, H, W, C), cut_planes(deint, fmt, T, H, W, C)
    ctx = [None if x is None else cut_planes(x, fmt, 1, H, W, C) for x in (before, after)]
    frames = [[] for _ in range(T)]
    for n, ((R, _, _, F), (_, _, _, D)) in enumerate(zip(stored, dei)):
        res = loop_select_plane(F, D, modes, R, order, *[None if x is None else x[n][3][0] for x in ctx])
        for t in range(T):
            frames[t] += list(itertools.chain.from_iterable(res[t]))
    return torch.tensor(frames, dtype=torch.int64).to(packed.dtype).reshape(packed.shape)


# ---------------------------------------------------------------------------------------------------------------- clips
def pictures(n, R, N, speed, seed=0, width=10):
    """n progressive pictures, uint8 [n, R, N]: a textured object ``width`` columns wide over the middle half of the rows, moving
    ``speed`` columns a picture (wrapping around), over the static gradient 30 + column + row; noise of at most +-3 codes."""
    g = torch.Generator().manual_seed(seed)
    rows, cols = torch.arange(R)[:, None], torch.arange(N)[None, :]
    ground = (30 + cols + rows).expand(R, N)
    inside_rows = (rows >= R // 4) & (rows < R - R // 4)
    out = []
    for k in range(n):
        rel = (cols - (3 + k * speed)) % N
        picture = torch.where(inside_rows & (rel < width), 200 + 3 * rel - rows, ground)
        out.append(picture + torch.randint(-3, 4, (R, N), generator=g))
    return torch.stack(out).clamp(0, 255).to(torch.uint8)


def telecine(P, order):
    """3:2 pulldown of the pictures P [4 m, R, N]: per four pictures A B C D the frames A, B, B|C, C|D, D (a mixed frame keeps its
    first field from the earlier picture) -> (frames [5 m, R, N], src: the picture every frame's FIRST field shows)."""
    first, second, src = [], [], []
    for a in range(0, P.shape[0] - 3, 4):
        first += [a, a + 1, a + 1, a + 2, a + 3]
        second += [a, a + 1, a + 2, a + 3, a + 3]
        src += [a, a + 1, a + 1, a + 2, a + 3]
    fields = torch.stack([P[first], P[second]], dim=1).reshape(-1, *P.shape[1:])
    return weave(fields, order), src


def interlace(G, order):
    """every picture of G [2 T, R, N] is one field -> T woven frames"""
    return weave(G, order)


def picture_planes(P, fmt):
    """the pictures as the planes of a packed format, every plane int64 [n, rows, samples]: the RGB formats carry the picture in all
    of C = 3 channels; the 4:2:0 formats carry it as Y, its even rows and columns as Cb and 255 minus that as Cr; the 16-bit
    containers scale by 2^shift"""
    P = P.to(torch.int64) << SHIFT[fmt]
    if fmt in ("yuv420p8", "yuv420p10"):
        cb = P[:, ::2, ::2]
        return [P, cb, (255 << SHIFT[fmt]) - cb]
    return [P[..., None].expand(*P.shape, 3).reshape(P.shape[0], P.shape[1], -1)]


def packed_clip(P, fmt, build=lambda plane: plane):
    """``build`` (plane pictures -> plane frames: telecine, interlace or nothing) applied to every plane of the pictures -> the
    packed clip (C = 3) in fmt's dtype and shape"""
    planes_ = [build(pl) for pl in picture_planes(P, fmt)]
    T, H, W = planes_[0].shape[0], P.shape[1], P.shape[2]
    dtype = torch.uint16 if SHIFT[fmt] else torch.uint8
    flat = torch.cat([pl.reshape(T, -1) for pl in planes_], dim=1)
    return flat.to(dtype).reshape((T, H, W, 3) if len(planes_) == 1 else (T, -1))


def crafted_counts(T, mi, s):
    """int32 [T, 3, 2] whose peaks walk through the four modes and the three ties, whatever a clip holds: per frame (pc, pa, pb)"""
    b = mi * s
    rows = [(b, b + 9, b + 9),                          # pc == bound: as stored
            (b + 1, b, b + 5),                          # prev alone under the bound
            (b + 1, b + 5, b),                          # next alone under the bound
            (b + 1, b + 2, b + 3),                      # both over: deinterlace
            (b + 1, b, b),                              # a tie under the bound: prev
            (b + 1, b + 4, b + 4),                      # a tie over the bound: deinterlace
            (b + 7, 0, 0)]                              # a tie at zero: prev
    cnt = torch.zeros(T, 3, 2, dtype=torch.int32)
    for t in range(T):
        for k, peak in enumerate(rows[t % len(rows)]):
            cnt[t, k, 1] = peak
            cnt[t, k, 0] = 3 * peak + 100 * k + t       # totals that differ per candidate (the stats sums can tell them apart)
    return cnt, [(0, 1, 2, 3, 1, 3, 1)[t % 7] for t in range(T)]
