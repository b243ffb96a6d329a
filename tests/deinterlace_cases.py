"""TEST INFRASTRUCTURE shared by tests/test_deinterlace.py and tests/test_gpu_deinterlace.py: a per-sample restatement of the
deinterlacing rule in plain Python integers (written from the text of deinterlace.py's docstring, sharing no code with the
vectorised torch), clip builders and the shape list."""
import itertools

import torch

from conftest import sub
from frame_unpack_cases import SHAPES as UNPACK_SHAPES, channel_counts, random_packed  # noqa: F401 (re-exported)

# frame_unpack_cases' shapes (samples fewer than one vector, rows off 16 bytes, odd heights, chroma planes of one row), plus: seven
# columns, where only the middle one runs the edge search (4, 6, 7); five frames, so that an interior frame has two real
# neighbours on either side (5, 4, 23); and a plane all of whose computed rows are border rows (2, 2, 9)
SHAPES = UNPACK_SHAPES + [(4, 6, 7), (5, 4, 23), (2, 2, 9)]
FORMATS = ("rgb8", "bgr8", "rgb16", "yuv420p8", "yuv420p10")
CONTEXTS = ("none", "before", "after", "both")


def loop_plane(F, R, N, s, order, rate, before=None, after=None):
    """F: T frames, each R rows of N ints -> the output frames (lists of rows of ints) of ONE plane with column step s."""
    T = len(F)

    def frame(j):
        if j < 0:
            return before if before is not None else F[min(1, T - 1)]
        if j >= T:
            return after if after is not None else F[max(T - 2, 0)]
        return F[j]

    first = 0 if order == "tff" else 1
    out = []
    for t in range(T):
        for k in ((0, 1) if rate == "field" else (0,)):
            p = first if k == 0 else 1 - first
            cur, P, Nx, B, A = frame(t), frame(t - 1), frame(t + 1), frame(t - 1 + k), frame(t + k)
            rows = []
            for r in range(R):
                if r % 2 == p or R == 1:
                    rows.append(list(cur[r]))
                    continue
                up = r - 1 if r >= 1 else r + 1
                dn = r + 1 if r + 1 < R else r - 1
                row = []
                for i in range(N):
                    c, e = cur[up][i], cur[dn][i]
                    d = (B[r][i] + A[r][i]) >> 1
                    t0 = abs(B[r][i] - A[r][i]) >> 1
                    t1 = (abs(P[up][i] - c) + abs(P[dn][i] - e)) >> 1
                    t2 = (abs(Nx[up][i] - c) + abs(Nx[dn][i] - e)) >> 1
                    diff = max(t0, t1, t2)
                    sp = (c + e) >> 1
                    if i - 3 * s >= 0 and i + 3 * s <= N - 1:
                        def score(j):
                            return sum(abs(cur[up][i + (q + j) * s] - cur[dn][i + (q - j) * s]) for q in (-1, 0, 1))

                        def pred(j):
                            return (cur[up][i + j * s] + cur[dn][i - j * s]) >> 1
                        best = score(0) - 1
                        for j1, j2 in ((-1, -2), (1, 2)):
                            if score(j1) < best:
                                best, sp = score(j1), pred(j1)
                                if score(j2) < best:
                                    best, sp = score(j2), pred(j2)
                    row.append(min(max(sp, d - diff), d + diff))
                rows.append(row)
            out.append(rows)
    return out


def plane_list(fmt, H, W, C):
    """the planes of the rule's text, restated: (offset, rows, samples per row, step)"""
    if fmt in ("yuv420p8", "yuv420p10"):
        h2, w2 = -(-H // 2), -(-W // 2)
        return [(0, H, W, 1), (H * W, h2, w2, 1), (H * W + h2 * w2, h2, w2, 1)]
    return [(0, H, W * C, C)]


def loop_deinterlace(packed, fmt, T, H, W, C, order, rate, before=None, after=None):
    """The packed clip through loop_plane, plane by plane -> a tensor of packed's dtype, [T or 2T, ...]."""
    flat = packed.reshape(T, -1).to(torch.int64).tolist()
    ctx = [None if x is None else x.reshape(-1).to(torch.int64).tolist() for x in (before, after)]
    n_out = T * (2 if rate == "field" else 1)
    out = [[0] * len(flat[0]) for _ in range(n_out)]
    for off, R, N, s in plane_list(fmt, H, W, C):
        cut = lambda f: [f[off + r * N:off + (r + 1) * N] for r in range(R)]
        res = loop_plane([cut(f) for f in flat], R, N, s, order, rate, *[None if x is None else cut(x) for x in ctx])
        for o in range(n_out):
            out[o][off:off + R * N] = list(itertools.chain.from_iterable(res[o]))
    shape = (n_out,) + tuple(packed.shape[1:])
    return torch.tensor(out, dtype=torch.int64).to(packed.dtype).reshape(shape)


def context(kind, fmt, H, W, C, seed):
    """-> (before, after): random single frames or None, by ``kind`` of CONTEXTS"""
    before = random_packed(fmt, 1, H, W, C, seed + 1000) if kind in ("before", "both") else None
    after = random_packed(fmt, 1, H, W, C, seed + 2000) if kind in ("after", "both") else None
    return before, after


def formula_clip(T, R, N):
    """the clip of the check values: F[t][r][i] = (37 t^2 + 11 r i + 5 i^2 + 3 r + 101 t r + 29 t i) mod 256"""
    return [[[(37 * t * t + 11 * r * i + 5 * i * i + 3 * r + 101 * t * r + 29 * t * i) % 256 for i in range(N)] for r in range(R)]
            for t in range(T)]


def weave(fields, order):
    """fields g[0], g[1], ... (uint8 [n, R, N], each a whole picture at its instant) -> n // 2 woven frames: frame t takes the rows
    of its first field's parity from g[2t] and the others from g[2t + 1]."""
    first = 0 if order == "tff" else 1
    frames = fields[1::2].clone()
    frames[:, first::2] = fields[0::2, first::2]
    return frames


def moving_bar(width, speed, n=10, R=8, N=96):
    g = torch.full((n, R, N), 40, dtype=torch.uint8)
    for k in range(n):
        g[k, :, 4 + k * speed:4 + k * speed + width] = 200
    return g


def moving_diagonal(n=8, R=12, N=96):
    g = torch.full((n, R, N), 30, dtype=torch.uint8)
    for k in range(n):
        for r in range(R):
            x0 = 10 + 3 * k + r
            g[k, r, x0:x0 + 12] = 220
    return g


def as_gray_rgb(planes_):
    """uint8 [T, R, N] -> an rgb8 clip with C = 3 whose three channels all hold the plane: [T, R, N, 3]"""
    return planes_[..., None].expand(*planes_.shape, 3).contiguous()


def spec():
    return sub("deinterlace")
