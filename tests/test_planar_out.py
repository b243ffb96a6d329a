"""-m "not gpu": planar output -- planar_out.pack_planar_torch (the specification of csrc/svr_planar_out.hip) against the yuv420p10
statement it extends, check values worked out here from Fractions, its integer bounds, the ingest side read back (planar.py), what the
sitings mean to that reader, the edge clamps by hand, the refusals; the header, the ctypes table and the build list; and the command
line: route_output, FFmpegWriter(planes=), and both ends through the stand-in ffprobe / ffmpeg of tests/frame_unpack_cases.py with the
switch on and off."""
import itertools
import os
import re
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from test_colour_out import BT709_TAGS, H, T, W, run_cli, ten_bit_argv
from test_frame_unpack import TODAY, identity  # noqa: F401 (identity: fixture)
from test_gpu_frame_pack import clip, same
from test_stream import cli, rig  # noqa: F401 (fixtures)

KR_KB = {"bt709": ("0.2126", "0.0722"), "bt601": ("0.299", "0.114"), "bt2020": ("0.2627", "0.0593")}
MATRICES, RANGES, SUBS, BITS = tuple(KR_KB), ("tv", "pc"), ("420", "422", "444"), (8, 10, 12)
SITINGS = {"420": ("center", "left", "topleft"), "422": ("center", "left"), "444": ("left",)}
WEIGHT = {("420", "center"): 4, ("420", "left"): 8, ("420", "topleft"): 16, ("422", "center"): 2, ("422", "left"): 4, ("444", "left"): 1}
COLOURS = {"white": (1, 1, 1), "black": (0, 0, 0), "red": (1, 0, 0), "green": (0, 1, 0), "blue": (0, 0, 1), "yellow": (1, 1, 0),
           "grey": (0.5, 0.5, 0.5)}


def constants(bits, range_):
    return (16 << (bits - 8), 219 << (bits - 8), 224 << (bits - 8)) if range_ == "tv" else (0, (1 << bits) - 1, (1 << bits) - 1)


def planes(packed, s, Hh, Ww):
    """[T, H*W + 2*hc*wc] -> int64 Y [T, H, W], Cb, Cr [T, hc, wc]"""
    hc, wc = ((Hh + 1) // 2 if s == "420" else Hh), (Ww if s == "444" else (Ww + 1) // 2)
    p = packed.to(torch.int64)
    n = p.shape[0]
    return (p[:, :Hh * Ww].reshape(n, Hh, Ww), p[:, Hh * Ww:Hh * Ww + hc * wc].reshape(n, hc, wc), p[:, Hh * Ww + hc * wc:].reshape(n, hc, wc))


def half_up(f):
    return (2 * f.numerator + f.denominator) // (2 * f.denominator)


def check_value(rgb, bits, matrix, range_):
    """(Y, Cb, Cr) of a flat colour in Fractions: the forward matrix from the exact decimal Kr, Kb with every weight rounded at 2^16 as
    the specification defines them (the luma deficit to green), applied to the colour itself -- no codes, no sums, no S --, rounded
    half up and clamped"""
    kr, kb = (Fraction(k) for k in KR_KB[matrix])
    kg = 1 - kr - kb
    at16 = lambda f: Fraction(half_up(f * 65536), 65536)
    wr, wg, wb = at16(kr), at16(kg), at16(kb)
    wg += 1 - (wr + wg + wb)
    cb_row = (at16(-kr / (2 * (1 - kb))), at16(-kg / (2 * (1 - kb))), Fraction(1, 2))
    cr_row = (Fraction(1, 2), at16(-kg / (2 * (1 - kr))), at16(-kb / (2 * (1 - kr))))
    rgb = [Fraction(v) for v in rgb]
    y0, ys, cs = constants(bits, range_)
    dot = lambda row: sum(w * v for w, v in zip(row, rgb))
    chroma = lambda row: min(max(half_up((1 << (bits - 1)) + cs * dot(row)), 0), (1 << bits) - 1)
    return y0 + half_up(ys * dot((wr, wg, wb))), chroma(cb_row), chroma(cr_row)


def bounds(bits, matrix, range_):
    """half a code of Y and half a code of each chroma plane at n bits through the inverse matrix (tests/test_colour_out.py::bounds
    with the depth's excursions): derived from the specification, not measured"""
    kr, kb = (float(k) for k in KR_KB[matrix])
    kg = 1 - kr - kb
    _, ys, cs = constants(bits, range_)
    return (0.5 / ys + 2 * (1 - kr) * 0.5 / cs, 0.5 / ys + (2 * (1 - kb) * kb / kg + 2 * (1 - kr) * kr / kg) * 0.5 / cs,
            0.5 / ys + 2 * (1 - kb) * 0.5 / cs)


def flat(rgb, Tn=1, Hh=4, Ww=6):
    return torch.tensor(rgb, dtype=torch.float32).expand(Tn, Hh, Ww, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------- specification
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_420_at_ten_bits_is_the_yuv420p10_statement(dtype):
    planar_out, frameio = sub("planar_out"), sub("frameio")
    for n, shape in enumerate([(1, 1, 1), (2, 3, 5), (1, 5, 4), (3, 17, 33), (1, 16, 64)]):
        x = clip(*shape, 3, seed=50 + n).to(dtype)
        for m, r, s in itertools.product(MATRICES, RANGES, ("center", "left")):
            assert same(planar_out.pack_planar_torch(x, "420", 10, m, r, s), frameio.pack_yuv420p10_torch(x, m, r, s)), (shape, m, r, s)
    assert planar_out.ENABLED is False                                         # ships off


def test_check_values_of_flat_frames():
    planar_out, planar = sub("planar_out"), sub("planar")
    named = {(8, "bt709", "tv"): dict(white=(235, 128, 128), black=(16, 128, 128), red=(63, 102, 240), green=(173, 42, 26), blue=(32, 240, 118)),
             (8, "bt601", "tv"): dict(red=(81, 90, 240)),
             (12, "bt2020", "tv"): dict(red=(1176, 1548, 3840), green=(2632, 756, 400), blue=(464, 3840, 1904)),
             (8, "bt709", "pc"): dict(blue=(18, 255, 116)),                     # (the clamp: 255.5 rounds to 256 without it)
             # frameio's docstring, the 10-bit rows
             (10, "bt2020", "tv"): dict(red=(294, 387, 960), green=(658, 189, 100), blue=(116, 960, 476), white=(940, 512, 512), black=(64, 512, 512)),
             (10, "bt601", "tv"): dict(red=(326, 361, 960), green=(578, 215, 137), blue=(164, 960, 439)),
             (10, "bt709", "tv"): dict(red=(250, 409, 960), green=(691, 167, 105), blue=(127, 960, 471)),
             (10, "bt709", "pc"): dict(red=(217, 395, 1023), green=(732, 118, 47), blue=(74, 1023, 465), white=(1023, 512, 512), black=(0, 512, 512)),
             (10, "bt2020", "pc"): dict(red=(269, 369, 1023), green=(694, 143, 42), blue=(61, 1023, 471))}
    for (bits, matrix, range_), rows in named.items():
        for colour, want in rows.items():
            assert check_value(COLOURS[colour], bits, matrix, range_) == want, (bits, matrix, range_, colour)
            for s in SUBS:
                for siting in SITINGS[s]:                                      # identical for every siting: independent of S
                    out = planar_out.pack_planar_torch(flat(COLOURS[colour], 2, 3, 5), s, bits, matrix, range_, siting)
                    assert out.dtype == planar.planar_dtype(bits) and tuple(out.shape) == planar.planar_shape(2, 3, 5, s)
                    Y, cb, cr = planes(out, s, 3, 5)
                    assert (set(Y.flatten().tolist()), set(cb.flatten().tolist()), set(cr.flatten().tolist())) == tuple({v} for v in want), \
                        (bits, matrix, range_, colour, s, siting)


def test_numerator_bounds_hold_for_every_combination():
    planar_out = sub("planar_out")
    every = []
    for bits, matrix, range_, S in itertools.product(BITS, MATRICES, RANGES, (1, 2, 4, 8, 16)):
        lo, hi = planar_out.numerator_bound(bits, matrix, range_, S)
        assert 0 < lo <= hi < 2 ** 62, (bits, matrix, range_, S, lo, hi)
        every.append((lo, hi))
    assert planar_out.numerator_bounds() == (min(lo for lo, _ in every), max(hi for _, hi in every)) == (4294901760, 281470681743360)
    assert "4 294 901 760" in planar_out.__doc__ and "281 470 681 743 360" in planar_out.__doc__
    assert {(s, siting): planar_out.total_weight(s, siting) for s in SUBS for siting in SITINGS[s]} == WEIGHT
    assert planar_out.SITINGS == SITINGS


def test_flat_frames_survive_the_round_trip_through_the_ingest_side():
    """pack, then planar.planar_codes_torch: every channel within the quantisation bound the matrix gives at n bits"""
    planar_out, planar, frameio = sub("planar_out"), sub("planar"), sub("frameio")
    worst = {bits: 0.0 for bits in BITS}
    for s, bits, matrix, range_ in itertools.product(SUBS, BITS, MATRICES, RANGES):
        bound = bounds(bits, matrix, range_)
        for colour, rgb in COLOURS.items():
            x = flat(rgb, 1, 3, 5)
            for siting in planar.SITINGS[s]:                                   # (what the reader takes)
                back = planar.planar_codes_torch(planar_out.pack_planar_torch(x, s, bits, matrix, range_, siting), s, bits, 1, 3, 5, matrix,
                                                 range_, siting)
                err = (back.to(torch.int32).double() - frameio.codes(x, 65535.0).double()).abs().amax(dim=(0, 1, 2)) / 65535.0
                for c in range(3):
                    assert float(err[c]) <= bound[c], (s, bits, matrix, range_, siting, colour, c, float(err[c]), bound[c])
                worst[bits] = max(worst[bits], float(err.max()))
    print("worst round-trip error at 8 / 10 / 12 bits:", worst)


def ramp(vertical):
    """64 samples: R rising, G falling, B constant, along the width (4 rows) or the height (4 columns)"""
    i = torch.arange(64, dtype=torch.float64) / 63
    line = torch.stack([0.2 + 0.6 * i, 0.8 - 0.6 * i, torch.full_like(i, 0.5)], dim=-1).float()
    return (line[None, :, None, :].expand(1, 64, 4, 3) if vertical else line[None, None, :, :].expand(1, 4, 64, 3)).contiguous()


@pytest.mark.parametrize("bits", BITS)
def test_siting_means_what_the_reader_assumes(bits):
    planar_out, planar, frameio = sub("planar_out"), sub("planar"), sub("frameio")
    bound = bounds(bits, "bt2020", "tv")

    def error(x, s, packed_as, read_as, vertical):
        _, Hh, Ww, _ = x.shape
        back = planar.planar_codes_torch(planar_out.pack_planar_torch(x, s, bits, "bt2020", "tv", packed_as), s, bits, 1, Hh, Ww, "bt2020",
                                         "tv", read_as)
        err = (back.to(torch.int32).double() - frameio.codes(x, 65535.0).double()).abs() / 65535.0
        err = err[:, 4:-4] if vertical else err[:, :, 4:-4]                    # (at the frame's edge the reader's clamp dominates)
        return [float(e) for e in err.amax(dim=(0, 1, 2))]

    cases = [("420", "left", "center", "left", False), ("422", "left", "center", "left", False), ("420", "topleft", "left", "topleft", True)]
    for s, matched, other, read_as, vertical in cases:
        x = ramp(vertical)
        good, bad = error(x, s, matched, read_as, vertical), error(x, s, other, read_as, vertical)
        print(bits, s, matched, "matched", good, "mismatched", bad, "bound", bound)
        for c in range(3):
            assert good[c] <= bound[c], (s, matched, c, good, bound)
        assert max(good) < max(bad) and good[0] < bad[0] and good[1] < bad[1], (s, matched, good, bad)


def chroma_by_hand(sums, S, bits, matrix, range_):
    frameio = sub("frameio")
    _, _, _, cb_r, cb_g, cr_g, cr_b = frameio.yuv_matrix(matrix)
    _, _, cs = constants(bits, range_)
    D, half, top = 65535 * 65536, 1 << (bits - 1), (1 << bits) - 1
    sr, sg, sb = sums
    cb = (S * half * D + cs * (cb_r * sr + cb_g * sg + 32768 * sb) + S * D // 2) // (S * D)
    cr = (S * half * D + cs * (32768 * sr + cr_g * sg + cr_b * sb) + S * D // 2) // (S * D)
    return min(max(cb, 0), top), min(max(cr, 0), top)


def test_edge_weights_and_clamps_by_hand():
    planar_out, frameio = sub("planar_out"), sub("frameio")
    x = clip(1, 3, 3, 3, seed=77)
    q = frameio.codes(x, 65535.0).to(torch.int64)[0]                           # [3, 3, 3]
    px = lambda y, xx: tuple(int(v) for v in q[y, xx])
    add = lambda *terms: tuple(sum(w * p[c] for w, p in terms) for c in range(3))

    def chroma(s, siting, bits=10, m="bt2020", r="tv", frames=x):
        _, cb, cr = planes(planar_out.pack_planar_torch(frames, s, bits, m, r, siting), s, frames.shape[1], frames.shape[2])
        return lambda j, k: (int(cb[0, j, k]), int(cr[0, j, k]))

    by_hand = lambda sums, S: chroma_by_hand(sums, S, 10, "bt2020", "tv")
    # 4:2:2 left: column -1 clamps at column 0; the column beyond an odd W repeats the last one
    got = chroma("422", "left")
    assert got(1, 0) == by_hand(add((3, px(1, 0)), (1, px(1, 1))), 4)
    assert got(1, 1) == by_hand(add((1, px(1, 1)), (3, px(1, 2))), 4)
    # 4:2:2 center: columns 2, 3 -> 2, 2
    assert chroma("422", "center")(2, 1) == by_hand(add((2, px(2, 2))), 2)
    # 4:2:0 left, chroma row 1 of an odd H: rows 2, 3 -> 2, 2
    assert chroma("420", "left")(1, 0) == by_hand(add((6, px(2, 0)), (2, px(2, 1))), 8)
    assert chroma("420", "center")(1, 1) == by_hand(add((4, px(2, 2))), 4)
    # 4:2:0 topleft: row -1 clamps at row 0 (weights 1, 2, 1 -> 3, 1), row 3 repeats row 2 (1, 2, 1 over rows 1, 2, 2 -> 1, 3)
    got = chroma("420", "topleft")
    assert got(0, 0) == by_hand(add((9, px(0, 0)), (3, px(0, 1)), (3, px(1, 0)), (1, px(1, 1))), 16)
    assert got(1, 1) == by_hand(add((1, px(1, 1)), (3, px(1, 2)), (3, px(2, 1)), (9, px(2, 2))), 16)
    assert got(0, 1) == by_hand(add((3, px(0, 1)), (9, px(0, 2)), (1, px(1, 1)), (3, px(1, 2))), 16)
    assert chroma("444", "left")(2, 1) == by_hand(px(2, 1), 1)
    # H = 1 and W = 1: every tap is the one row / column there is
    row, col = x[:, :1].contiguous(), x[:, :, :1].contiguous()
    assert chroma("420", "topleft", frames=row)(0, 1) == by_hand(add((4, px(0, 1)), (12, px(0, 2))), 16)
    assert chroma("420", "topleft", frames=col)(1, 0) == by_hand(add((4, px(1, 0)), (12, px(2, 0))), 16)
    assert chroma("420", "left", frames=x[:, :1, :1].contiguous())(0, 0) == by_hand(add((8, px(0, 0))), 8)
    for s in SUBS:                                                             # luma: per pixel, whatever the sub
        Y, _, _ = planes(planar_out.pack_planar_torch(x, s, 12, "bt601", "pc", "left"), s, 3, 3)
        wr, wg, wb = frameio.yuv_matrix("bt601")[:3]
        r, g, b = px(2, 1)
        assert int(Y[0, 2, 1]) == (4095 * (wr * r + wg * g + wb * b) + 65535 * 32768) // (65535 * 65536)


def test_refusals_name_their_argument():
    planar_out = sub("planar_out")
    x = torch.rand(2, 4, 6, 3)
    good = dict(sub="422", bits=10, matrix="bt2020", range_="tv", siting="left")
    for kw, word in ((dict(sub="411"), "sub must be"), (dict(bits=9), "bits must be"), (dict(matrix="bt2100"), "matrix must be"),
                     (dict(range_="full"), "range_ must be"), (dict(siting="topleft"), "siting must be"), (dict(siting="top"), "siting must be"),
                     (dict(sub="444", siting="center"), "siting must be"), (dict(sub="420", siting="bottom"), "siting must be")):
        args = dict(good, **kw)
        with pytest.raises(ValueError, match=word):
            planar_out.pack_planar_torch(x, **args)
        with pytest.raises(ValueError, match=word):
            planar_out.pack_planar(x, **args)
    with pytest.raises(ValueError, match="C = 3"):
        planar_out.pack_planar_torch(torch.rand(1, 4, 6, 4), **good)
    with pytest.raises(ValueError, match="frames must be"):
        planar_out.pack_planar_torch(x.double(), **good)
    with pytest.raises(ValueError, match="frames must be"):
        planar_out.pack_planar_torch(x[0], **good)
    with pytest.raises(ValueError, match="at least one pixel"):
        planar_out.pack_planar_torch(torch.zeros(0, 4, 6, 3), **good)
    for out in (torch.zeros(2, 48, dtype=torch.int16), torch.zeros(2, 47, dtype=torch.uint16), torch.zeros(2, 48, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            planar_out.pack_planar(x, out=out, **good)
    assert [planar_out.pix_fmt(s, b) for s, b in (("420", 8), ("422", 10), ("444", 12), ("420", 10), ("444", 8))] == \
        ["yuv420p", "yuv422p10le", "yuv444p12le", "yuv420p10le", "yuv444p"]
    with pytest.raises(ValueError, match="bits must be"):
        planar_out.pix_fmt("420", 16)
    # a HipOps that was never initialised: refused in Python, in clip_args' order, before the library is touched
    mod = sub("ops")
    shell = object.__new__(mod.HipOps)
    shell.device = torch.device("cpu")
    refused = lambda frames, **kw: str(pytest.raises(ValueError, shell.pack_planar, frames, **dict(good, **kw)).value)
    assert refused(x.half()) == "pack_planar: frames must be [T, H, W, C] in fp32 or bf16, got (2, 4, 6, 3) torch.float16"
    assert refused(torch.zeros(0, 4, 6, 2), sub="411") == f"pack_planar: sub must be one of {('420', '422', '444')}, got '411'"
    assert refused(torch.zeros(0, 4, 6, 2), siting="topleft") == "pack_planar: siting must be one of ('center', 'left') for sub '422', got 'topleft'"
    assert refused(torch.zeros(0, 4, 6, 2)) == "pack_planar: planar output takes C = 3 (it has no alpha plane), got C = 2"
    assert refused(torch.zeros(0, 4, 6, 3)) == "pack_planar: frames must hold at least one pixel, got (0, 4, 6, 3)"
    assert refused(torch.zeros(2, 4, 12, 3)[:, :, ::2]) == "pack_planar: frames must be contiguous"
    assert refused(torch.zeros(2, 4, 6, 3, device="meta")) == "pack_planar: frames must live on cpu, got meta"
    assert refused(x, out=torch.zeros(2, 47, dtype=torch.uint16)) == "pack_planar: out must be (2, 48), got (2, 47)"
    assert "out must be torch.uint16" in refused(x, out=torch.zeros(2, 48, dtype=torch.uint8))


def test_pack_planar_uses_the_backend_and_never_falls_back():
    planar_out, hip_lib = sub("planar_out"), sub("hip_lib")
    from ops_reference import TorchOps
    x = clip(2, 5, 7, 3, seed=3)

    class Failing:
        def pack_planar(self, *a, **k):
            raise hip_lib.HipLibraryError("svr_pack_planar failed")

    class Marking:
        def pack_planar(self, frames, s, bits, matrix, range_, siting, out=None):
            return ("backend", s, bits, matrix, range_, siting, out)

    with pytest.raises(hip_lib.HipLibraryError):
        planar_out.pack_planar(x, "422", 10, "bt2020", "tv", "left", ops=Failing())
    assert planar_out.pack_planar(x, "444", 8, "bt601", "pc", "left", ops=Marking()) == ("backend", "444", 8, "bt601", "pc", "left", None)
    assert not hasattr(TorchOps("cpu"), "pack_planar")
    want = planar_out.pack_planar_torch(x, "420", 12, "bt2020", "tv", "topleft")
    assert same(planar_out.pack_planar(x, "420", 12, "bt2020", "tv", "topleft", ops=TorchOps("cpu")), want)
    out = torch.zeros(want.shape, dtype=torch.uint16)
    assert planar_out.pack_planar(x, "420", 12, "bt2020", "tv", "topleft", out=out) is out and same(out, want)


def test_header_ctypes_tables_and_build_list_know_the_entry_point():
    hip_lib, planar_out = sub("hip_lib"), sub("planar_out")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert "svr_pack_planar" in declared and declared == set(hip_lib.SYMBOLS)
    decl = re.search(r"int svr_pack_planar\(([^;]*)\);", src).group(1)
    assert len(decl.split(",")) == 13 == len(hip_lib.SYMBOLS["svr_pack_planar"][1])
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert re.search(r"v9, additive: \+ svr_pack_planar\(\).*?A new symbol only", src, flags=re.S)
    codes = dict(center="SVR_COLOUR_SITING_CENTER", left="SVR_COLOUR_SITING_LEFT", topleft="SVR_PLANAR_SITING_TOPLEFT")
    for name, code in hip_lib.PLANAR_OUT_SITINGS.items():
        assert re.search(rf"#define {codes[name]}\s+{code}\b", src), name
    assert set(hip_lib.PLANAR_OUT_SITINGS) == {s for sitings in planar_out.SITINGS.values() for s in sitings}
    assert hip_lib.COLOUR_SITINGS == {"center": 0, "left": 1} and hip_lib.PLANAR_SITINGS == {"left": 1, "topleft": 2}    # (gained nothing)
    api = open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert '#include "svr_planar_out.hip"' in api and "int svr_pack_planar(" in api
    assert os.path.join(hip_lib.CSRC, "svr_planar_out.hip") in hip_lib.sources()        # (the loader's source hash covers it)
    entry = api[api.index("int svr_pack_planar("):]
    assert "pack_refusal(e, frames" in entry[:entry.index("\n}\n")]            # the shared refusal path


# ---------------------------------------------------------------------------------------------------------------- command line
def test_route_output(cli, monkeypatch):
    planar_out = sub("planar_out")
    tags = lambda **kw: dict(dict.fromkeys(cli.COLOUR_FIELDS), **kw)
    info = lambda pix: dict(width=1920, height=1080, pix_fmt=pix)
    hdr = tags(color_space="bt2020nc", color_primaries="bt2020", color_transfer="smpte2084")
    sources = [info("yuv422p10le"), info("yuv420p"), info("yuv444p12le"), None]
    assert planar_out.ENABLED is False
    for source, colour, ten in itertools.product(sources, (None, tags(), hdr), (False, True)):
        assert cli.route_output(source, colour, "ffmpeg", ten) is None         # the switch is off
    monkeypatch.setattr(planar_out, "ENABLED", True)
    table = {"yuv420p": "420", "yuvj420p": "420", "yuv420p10le": "420", "yuv420p12le": "420", "yuv422p": "422", "yuvj422p": "422",
             "yuv422p10le": "422", "yuv422p12le": "422", "yuv444p": "444", "yuvj444p": "444", "yuv444p10le": "444", "yuv444p12le": "444",
             "nv12": "420", "rgb24": "420", "yuva444p": "420", "gbrp": "420", None: "420"}
    assert set(table) - {"nv12", "rgb24", "yuva444p", "gbrp", None} == set(cli.PLANAR_420) | set(cli.PLANAR_SOURCES)
    for pix, s in table.items():
        assert cli.route_output(info(pix), tags(), "ffmpeg", False) == (s, 8, "bt709", "tv", "left"), pix
        assert cli.route_output(info(pix), tags(), "ffmpeg", True) == (s, 12 if pix and pix.endswith("12le") else 10, "bt709", "tv", "left"), pix
    assert cli.route_output(None, None, "ffmpeg", False) == ("420", 8, "bt709", "tv", "left")       # not read through ffprobe
    assert cli.route_output(None, None, "ffmpeg", True) == ("420", 10, "bt709", "tv", "left")
    # HDR: bt2020 with --10bit, BT.709 (and output_colour's warning, main's to print) without
    assert cli.route_output(info("yuv422p10le"), hdr, "ffmpeg", True) == ("422", 10, "bt2020", "tv", "left")
    assert cli.route_output(info("yuv420p12le"), hdr, "ffmpeg", True) == ("420", 12, "bt2020", "tv", "left")
    assert cli.route_output(info("yuv420p10le"), hdr, "ffmpeg", False) == ("420", 8, "bt709", "tv", "left")
    assert "--10bit" in cli.output_colour(hdr, "ffmpeg", False)[1]
    # topleft only for 4:2:0
    top = dict(hdr, chroma_location="topleft")
    assert cli.route_output(info("yuv420p10le"), top, "ffmpeg", True) == ("420", 10, "bt2020", "tv", "topleft")
    assert cli.route_output(info("yuv420p"), tags(chroma_location="topleft"), "ffmpeg", False) == ("420", 8, "bt709", "tv", "topleft")
    assert cli.route_output(info("yuv422p10le"), top, "ffmpeg", True) == ("422", 10, "bt2020", "tv", "left")
    assert cli.route_output(info("yuv444p"), top, "ffmpeg", True) == ("444", 10, "bt2020", "tv", "left")
    assert cli.route_output(info("yuv420p"), tags(chroma_location="center"), "ffmpeg", False)[4] == "left"
    # bt2020c and the OpenCV backend: today's route, with the existing warnings
    bt2020c = tags(color_space="bt2020c", color_primaries="bt2020", color_transfer="smpte2084")
    assert cli.route_output(info("yuv420p10le"), bt2020c, "ffmpeg", True) is None and "bt2020c" in cli.output_colour(bt2020c, "ffmpeg", True)[1]
    for ten in (False, True):
        assert cli.route_output(info("yuv422p10le"), hdr, "opencv", ten) is None and "OpenCV" in cli.output_colour(hdr, "opencv", ten)[1]
        assert cli.route_output(None, None, "opencv", ten) is None


def test_ffmpeg_writer_states_the_planes_it_is_fed(cli):
    head = lambda pix: ["ffmpeg", "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", pix, "-s", "1920x1080", "-r", "24"]
    w = cli.FFmpegWriter("ffmpeg", "o.mp4", 24.0, ten_bit=True, planes=("422", 10, "bt709", "tv", "left"))
    tags = ["-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv", "-chroma_sample_location", "left"]
    assert w.command(1080, 1920) == head("yuv422p10le") + tags + ["-i", "-", "-c:v", "libx265", "-pix_fmt", "yuv422p10le", "-preset", "medium",
                                                                  "-crf", "12"] + tags + ["o.mp4"]
    assert w.planes == ("422", 10, "bt709", "tv", "left")
    w = cli.FFmpegWriter("ffmpeg", "o.mp4", 24.0, planes=("444", 8, "bt709", "tv", "left"))
    tags = ["-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv"]
    assert w.command(1080, 1920) == head("yuv444p") + tags + ["-i", "-", "-c:v", "libx264", "-pix_fmt", "yuv444p", "-preset", "medium",
                                                              "-crf", "12"] + tags + ["o.mp4"]
    colour = cli.output_colour(dict(color_transfer="smpte2084", color_primaries="bt2020"))[0]
    w = cli.FFmpegWriter("ffmpeg", "o.mp4", Fraction(24000, 1001), ten_bit=True, audio=("in.mkv", 0.5), colour=colour,
                         planes=("420", 12, "bt2020", "tv", "topleft"))
    tags = ["-colorspace", "bt2020nc", "-color_primaries", "bt2020", "-color_trc", "smpte2084", "-color_range", "tv",
            "-chroma_sample_location", "topleft"]
    assert w.command(1080, 1920) == head("yuv420p12le")[:-1] + ["24000/1001"] + tags + [
        "-i", "-", "-ss", "0.500000", "-i", "in.mkv", "-map", "0:v:0", "-map", "1:a?", "-c:a", "copy", "-shortest", "-c:v", "libx265",
        "-pix_fmt", "yuv420p12le", "-preset", "medium", "-crf", "12"] + tags + ["o.mp4"]
    # planes=None: today's commands
    w = cli.FFmpegWriter("ffmpeg", "o.mp4", 30.0)
    assert w.planes is None and w.command(8, 10) == ["ffmpeg"] + TODAY + ["o.mp4"]
    assert cli.FFmpegWriter("ffmpeg", "o.mp4", 30.0, planes=None).command(8, 10) == ["ffmpeg"] + TODAY + ["o.mp4"]
    w = cli.FFmpegWriter("ffmpeg", "o.mp4", 24.0, ten_bit=True, colour=colour)
    hdr = ["-colorspace", "bt2020nc", "-color_primaries", "bt2020", "-color_trc", "smpte2084", "-color_range", "tv", "-chroma_sample_location", "left"]
    assert w.planes is None and w.command(8, 10) == ["ffmpeg"] + ten_bit_argv(hdr, "10x8", "24", "o.mp4")
    assert cli.FFmpegWriter("ffmpeg", "o.mp4", 24.0, ten_bit=True).command(8, 10) == ["ffmpeg"] + ten_bit_argv(BT709_TAGS, "10x8", "24", "o.mp4")


def test_sink_hands_a_writer_with_planes_those_planes(cli):
    planar_out, frameio = sub("planar_out"), sub("frameio")
    x = clip(3, 5, 7, 3, seed=12)

    def through(**attrs):
        seen = []
        writer = type("Keep", (), dict(fmt="bgr8", alpha=False, write=lambda self, arr, h, w: seen.append(arr.copy()), close=lambda self: None,
                                       **attrs))()
        sink = cli.FrameSink(writer)
        sink.put(x)
        sink.close()
        return torch.from_numpy(seen[0])

    for planes_ in (("422", 10, "bt2020", "tv", "left"), ("420", 8, "bt709", "tv", "left"), ("444", 12, "bt601", "pc", "left")):
        assert same(through(planes=planes_), planar_out.pack_planar_torch(x, *planes_)), planes_
    assert same(through(), frameio.pack_frames_torch(x, "bgr8")) and same(through(planes=None), frameio.pack_frames_torch(x, "bgr8"))


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_cli_pipes_the_planes_with_the_switch_on_and_todays_bytes_with_it_off(identity, tmp_path, monkeypatch, chunked):
    planar_out, frameio = sub("planar_out"), sub("frameio")
    assert planar_out.ENABLED is False
    # switch off: today's argv and bytes -- existing behaviour did not move
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, ["--10bit"], pix="yuv422p10le")
    assert argv == ten_bit_argv(BT709_TAGS, "10x8", "24", out)
    assert piped == frameio.pack_frames_torch(frames, "yuv420p10").numpy().astype("<u2").tobytes()
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, [], pix="yuv420p", fmt="yuv420p8")
    assert argv == TODAY[:10] + ["24"] + TODAY[11:] + [str(out)]
    assert piped == frameio.pack_frames_torch(frames, "bgr8").numpy().tobytes()
    # switch on: a yuv422p10le source with --10bit leaves as 4:2:2 at 10 bits
    monkeypatch.setattr(planar_out, "ENABLED", True)
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, ["--10bit"], pix="yuv422p10le")
    tags = BT709_TAGS + ["-chroma_sample_location", "left"]
    assert argv == (["-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "yuv422p10le", "-s", "10x8", "-r", "24"] + tags
                    + ["-i", "-", "-c:v", "libx265", "-pix_fmt", "yuv422p10le", "-preset", "medium", "-crf", "12"] + tags + [str(out)])
    assert piped == planar_out.pack_planar_torch(frames, "422", 10, "bt709", "tv", "left").numpy().astype("<u2").tobytes()
    assert len(piped) == T * H * W * 2 * 2
    # ... and an untagged 8-bit source without --10bit as 4:2:0 at 8 bits: 1.5 bytes a pixel, no scale filter
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, [], pix="yuv420p", fmt="yuv420p8")
    assert argv == (["-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "yuv420p", "-s", "10x8", "-r", "24"] + tags
                    + ["-i", "-", "-c:v", "libx264", "-pix_fmt", "yuv420p", "-preset", "medium", "-crf", "12"] + tags + [str(out)])
    assert piped == planar_out.pack_planar_torch(frames, "420", 8, "bt709", "tv", "left").numpy().tobytes()
    assert 2 * len(piped) == 3 * T * H * W
