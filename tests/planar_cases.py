"""TEST INFRASTRUCTURE shared by tests/test_planar.py and tests/test_gpu_planar.py: the shapes, the settings planar.py distinguishes,
random planes, an independent per-pixel statement of planar.py's docstring in Python integers / Fractions, the torch chain a
FrameSource on the planar route has to equal, and the stand-in executables of tests/frame_unpack_cases.py."""
import importlib.util
import os
from fractions import Fraction

import torch

from conftest import ROOT, sub
from frame_unpack_cases import fake_video, raw_bytes, stand_ins  # noqa: F401 (re-exported)

# [T, H, W]: fewer samples than one vector (1,1,1; 1,1,5), chroma rows and columns that clamp on all four sides (1,2,2; 1,3,3; 2,3,5),
# one and several 16-pixel units per row = the seam neighbour and the row end (1,1,16; 2,5,32; 1,4,32; 2,5,48), odd H in the 4:2:0
# vector kernel (2,5,32; 2,5,48), W off a multiple of 16 (2,4,18; 3,17,33), frame starts off 16 bytes (2,3,5; 2,4,18; 3,17,33)
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 2, 2), (1, 3, 3), (2, 3, 5), (1, 1, 16), (2, 5, 32), (1, 4, 32), (2, 5, 48), (2, 4, 18), (3, 17, 33)]
SMALL = SHAPES[:5]                               # what the per-pixel statement is run on
SUBS = ("420", "422", "444")
BITS = (8, 10, 12)
MATRICES = ("bt709", "bt601", "bt2020")
RANGES = ("tv", "pc")
KR_KB = {"bt709": ("0.2126", "0.0722"), "bt601": ("0.299", "0.114"), "bt2020": ("0.2627", "0.0593")}      # restated, not imported


def sitings(sub_):
    return ("left", "topleft") if sub_ == "420" else ("left",)


def shape_id(s):
    return "x".join(map(str, s))


def random_planes(sub_, bits, T, H, W, seed, whole_container=False):
    """Random samples over 0..2^bits - 1 -- far outside the nominal range, so the matrix meets negative numerators and both clamps --
    or (``whole_container``, 10 / 12 bits) over 0..65535: the samples a decoder never writes, which count as 2^bits - 1."""
    planar = sub("planar")
    g = torch.Generator().manual_seed(seed)
    top = 65536 if whole_container and bits > 8 else 1 << bits
    return torch.randint(0, top, planar.planar_shape(T, H, W, sub_), generator=g).to(torch.int32).to(planar.planar_dtype(bits))


def coefficients(matrix):
    """2 (1 - Kr), 2 (1 - Kb) Kb / Kg, 2 (1 - Kr) Kr / Kg, 2 (1 - Kb) rounded half up at 2^16, from the exact decimals"""
    kr, kb = (Fraction(k) for k in KR_KB[matrix])
    kg = 1 - kr - kb
    half_up = lambda f: (2 * f.numerator + f.denominator) // (2 * f.denominator)
    return tuple(half_up(f * 65536) for f in (2 * (1 - kr), 2 * (1 - kb) * kb / kg, 2 * (1 - kr) * kr / kg, 2 * (1 - kb)))


def pixel_statement(planes, sub_, bits, T, H, W, matrix, range_, siting):
    """planar.py's docstring, one pixel at a time in Python integers and Fractions -> nested lists [T][H][W][3]"""
    hc = (H + 1) // 2 if sub_ == "420" else H
    wc = W if sub_ == "444" else (W + 1) // 2
    top = (1 << bits) - 1
    rv, gu, gv, bu = coefficients(matrix)
    if range_ == "tv":
        y0, ys, cs = 16 << (bits - 8), 219 << (bits - 8), 224 << (bits - 8)
    else:
        y0, ys, cs = 0, top, top
    mid = 8 << (bits - 1)
    den = ys * 8 * cs * 65536
    flat = [[min(int(v), top) for v in frame] for frame in planes.reshape(T, -1).to(torch.int64).tolist()]
    out = []
    for t in range(T):
        f = flat[t]
        luma = lambda y, x: f[y * W + x]

        def eight(pl, y, x):
            c = lambda r, k: f[H * W + pl * hc * wc + min(max(r, 0), hc - 1) * wc + min(max(k, 0), wc - 1)]

            def v(k):                                            # the vertical value in quarters at chroma column k
                if sub_ != "420":
                    return 4 * c(y, k)
                j = y // 2
                if siting == "left":
                    return c(j - 1, k) + 3 * c(j, k) if y % 2 == 0 else 3 * c(j, k) + c(j + 1, k)
                return 4 * c(j, k) if y % 2 == 0 else 2 * c(j, k) + 2 * c(j + 1, k)
            if sub_ == "444":
                return 2 * v(x)
            return 2 * v(x // 2) if x % 2 == 0 else v(x // 2) + v(x // 2 + 1)

        def code(s):                                             # round half up of 65535 s / Den, clamped
            q = Fraction(65535 * s, den) + Fraction(1, 2)
            return min(max(q.numerator // q.denominator, 0), 65535)
        rows = []
        for y in range(H):
            row = []
            for x in range(W):
                base = (luma(y, x) - y0) * 8 * cs * 65536
                u, v_ = eight(0, y, x) - mid, eight(1, y, x) - mid
                row.append([code(base + rv * v_ * ys), code(base - (gu * u + gv * v_) * ys), code(base + bu * u * ys)])
            rows.append(row)
        out.append(rows)
    return out


def load_cli(name="svr_cli_planar"):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "inference_cli.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------------- FrameSource
THR, MI, DUP = 10, 24, 1024
SOURCE_T, SOURCE_H, SOURCE_W = 13, 6, 10


def source_planes(sub_, bits, seed=3):
    return random_planes(sub_, bits, SOURCE_T, SOURCE_H, SOURCE_W, seed)


def chain_of_the_whole(planes, sub_, bits, matrix, range_, siting, fields):
    """the existing torch chain applied to planar_codes_torch of the whole clip as "rgb16" -> fp32 frames"""
    planar, fin = sub("planar"), sub("frameio_in")
    T, H, W = SOURCE_T, SOURCE_H, SOURCE_W
    codes = planar.planar_codes_torch(planes, sub_, bits, T, H, W, matrix, range_, siting)
    n = T
    if fields is not None:
        order, rate = fields
        if rate in ("match", "decimate"):
            codes = sub("fieldmatch").field_match_torch(codes, "rgb16", T, H, W, 3, order, THR, MI)[0]
            if rate == "decimate":
                codes = sub("decimate").decimate_torch(codes, "rgb16", T, H, W, 3)[0]
                n = T - T // 5
        else:
            codes = sub("deinterlace").deinterlace_torch(codes, "rgb16", T, H, W, 3, order, rate)
            n = T * (2 if rate == "field" else 1)
    return fin.unpack_frames_torch(codes.reshape(n, H, W, 3), "rgb16", n, H, W, 3)


def planar_source(cli, directory, planes, pix, chunk, fields=None, color_space="bt709", color_range="tv", chroma_location=None, **kw):
    """a FrameSource over the stand-in ffmpeg for ``planes`` as a ``pix`` "video" -> (source, the decoder's argument file)"""
    ffprobe, ffmpeg = stand_ins(os.path.join(str(directory), "bin"))
    clip = os.path.join(str(directory), f"clip_{pix}.mkv")
    fake_video(clip, planes, pix, SOURCE_W, SOURCE_H, rate="30000/1001", color_space=color_space, color_range=color_range)
    info, colour = cli.probe_source(ffprobe, clip)
    colour = dict(colour, chroma_location=chroma_location)       # (fake_video's ffprobe answer has no such tag)
    src = cli.FrameSource(ffmpeg, clip, info, chunk, fields=fields, match=dict(thr=THR, mi=MI), decimate=dict(dup=DUP), colour=colour, **kw)
    return src, clip + ".args"
