"""TEST INFRASTRUCTURE shared by tests/test_decimate.py and tests/test_gpu_decimate.py: a restatement of decimation in plain Python
integers (written from the text of decimate.py's docstring, sharing no code with the torch statement), crafted diffs, and the shape
list.  The clip builders (progressive pictures, 3:2 telecine, interlaced video) are fieldmatch_cases'.

The property geometry is fieldmatch_cases': after field matching a telecined clip's frames are its pictures A, B, B, C, D per
cycle, so the frame at position 2 equals its predecessor (difference exactly 0) while every other frame shows the object SPEED
columns further on, across two vertical edges of >= 35 codes contrast over at least 9 rows: a block difference in the thousands."""
import torch

from fieldmatch_cases import (FORMATS, GEOMETRIES, MI, ORDERS, SHAPES as MATCH_SHAPES, SHIFT, THR, channel_counts, cut_planes,  # noqa: F401
                              interlace, packed_clip, pictures, random_packed, telecine)

# fieldmatch_cases' shapes (one-row planes, rows off 16 bytes, (2, 5, 528): 17 block columns, so that on the vector route a row of
# rgb16 with C = 4 -- 16 block columns a workgroup -- takes two workgroups), plus: a second block row of one row and a third block
# column of 6 pixels (6, 33, 70); two cycles and a one-frame tail (11, 18, 40); and T on both sides of one cycle and of two
SHAPES = MATCH_SHAPES + [(6, 33, 70), (11, 18, 40), (1, 6, 20), (4, 6, 20), (5, 6, 20), (9, 6, 20)]
FIRST = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------------------- restatement
def loop_diffs(F, R, N, s, before=None):
    """F: T frames of plane 0, each R rows of N ints -> [T]: the largest 32 x 32-pixel block sum of |F[t] - F[t-1]|"""
    out = []
    for t in range(len(F)):
        prev = F[t - 1] if t > 0 else before
        if prev is None:
            out.append(FIRST)
            continue
        blocks = {}
        for r in range(R):
            for i in range(N):
                key = (r // 32, (i // s) // 32)
                blocks[key] = blocks.get(key, 0) + abs(F[t][r][i] - prev[r][i])
        out.append(max(blocks.values()))
    return out


def loop_drops(diff):
    drops = []
    for c in range(len(diff) // 5):
        cycle = diff[5 * c:5 * c + 5]
        at = 0
        for j in range(1, 5):
            if cycle[j] < cycle[at]:                    # (strictly: the first of a tie stays)
                at = j
        drops.append(at)
    return drops


def loop_kept(drops, T):
    """the input frame every output frame is"""
    kept = [t for t in range(T) if t // 5 >= len(drops) or t % 5 != drops[t // 5]]
    assert len(kept) == T - T // 5
    return kept


def loop_stats(drops, diff, dup, s, shift):
    counts = [0] * 6
    for c, d in enumerate(drops):
        counts[d] += 1
        if diff[5 * c + d] > ((dup * s) << shift):
            counts[5] += 1
    return counts


def loop_frame_diffs(packed, fmt, T, H, W, C, before=None):
    """-> int32 [T] through loop_diffs (plane 0 only)"""
    R, N, s, F = cut_planes(packed, fmt, T, H, W, C)[0]
    ctx = None if before is None else cut_planes(before, fmt, 1, H, W, C)[0][3][0]
    return torch.tensor(loop_diffs(F, R, N, s, ctx), dtype=torch.int32)


def loop_select(packed, drops, T):
    return packed[loop_kept(drops, T)]


# ---------------------------------------------------------------------------------------------------------------- crafted diffs
def crafted_diffs(T, bound):
    """int32 [T] and the drops they ask for: cycles whose smallest diff sits at each of the positions 0..4, two- and five-way ties,
    the sentinel at frame 0, dropped values on both sides of ``bound`` (at it: a duplicate; one above: not one)"""
    b = bound
    rows = [((FIRST, b + 5, b, b + 7, b + 9), 2),                   # the sentinel never wins; the drop AT the bound
            ((b + 1, b + 5, b + 3, b + 7, b + 9), 0),               # position 0, one above the bound
            ((b + 9, 0, b + 3, b + 7, b + 9), 1),
            ((b + 9, b + 5, b + 3, b, b + 9), 3),
            ((b + 9, b + 5, b + 3, b + 7, b + 2), 4),               # position 4, above the bound
            ((b + 4, b + 2, b + 8, b + 2, b + 6), 1),               # a two-way tie: the first
            ((b + 6, b + 6, b + 6, b + 6, b + 6), 0),               # a five-way tie: the first
            ((FIRST, FIRST, FIRST, FIRST, FIRST - 1), 4)]
    diff = [FIRST] * T
    for c in range(T // 5):
        diff[5 * c:5 * c + 5] = rows[c % len(rows)][0]
    for t in range(T // 5 * 5, T):
        diff[t] = t                                                 # (a partial cycle's diffs decide nothing)
    return torch.tensor(diff, dtype=torch.int32), [rows[c % len(rows)][1] for c in range(T // 5)]
