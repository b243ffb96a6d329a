"""-m "not gpu": colour out -- frameio.pack_yuv420p10_torch (the yuv420p10 planes with a chosen matrix, range and chroma siting: the
specification of csrc/svr_frame_pack_colour.hip) against today's format, its constants recomputed from the decimal Kr / Kb, its
check values, an fp64 inverse written here (the unpack has no bt2020) and frameio_in's chroma upsampler; the C entry point's
refusals; and the command line: which sources are written as BT.2020 with left-sited chroma, with which tags, and that every other
source gets the command and the bytes it always got (ffprobe and ffmpeg replaced by tests/frame_unpack_cases.py's stand-ins)."""
import ctypes
import json
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from frame_unpack_cases import calls, fake_video, random_packed, stand_ins
from test_frame_unpack import TODAY, identity  # noqa: F401 (identity: fixture)
from test_gpu_frame_pack import EXTRA_SHAPES, SHAPES, clip, same
from test_stream import cli, rig  # noqa: F401 (fixtures)

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
KR_KB = {"bt709": ("0.2126", "0.0722"), "bt601": ("0.299", "0.114"), "bt2020": ("0.2627", "0.0593")}
MATRICES, RANGES, SITINGS = tuple(KR_KB), ("tv", "pc"), ("center", "left")
TABLE = {"bt709": (13933, 46871, 4732, -7509, -25259, -29763, -3005), "bt601": (19595, 38470, 7471, -11058, -21710, -27439, -5329),
         "bt2020": (17216, 44434, 3886, -9151, -23617, -30133, -2635)}


def planes(packed, H, W):
    """uint16 [T, H*W + 2*h2*w2] -> int64 Y [T, H, W], Cb, Cr [T, h2, w2]"""
    T, h2, w2 = packed.shape[0], (H + 1) // 2, (W + 1) // 2
    s = packed.to(torch.int64)
    return (s[:, :H * W].reshape(T, H, W), s[:, H * W:H * W + h2 * w2].reshape(T, h2, w2), s[:, H * W + h2 * w2:].reshape(T, h2, w2))


def constants(range_):
    return (64, 876, 896) if range_ == "tv" else (0, 1023, 1023)


def inverse(Y, cb, cr, matrix, range_):
    """fp64 R, G, B from fp64 Y, Cb, Cr at the same positions: the textbook inverse with the exact decimal Kr, Kb"""
    kr, kb = (float(k) for k in KR_KB[matrix])
    kg = 1 - kr - kb
    y0, ys, cs = constants(range_)
    y, u, v = (Y - y0) / ys, (cb - 512) / cs, (cr - 512) / cs
    return y + 2 * (1 - kr) * v, y - (2 * (1 - kb) * kb / kg) * u - (2 * (1 - kr) * kr / kg) * v, y + 2 * (1 - kb) * u


def bounds(matrix, range_):
    """half a code of Y and half a code of each chroma plane through the inverse: derived from the specification, not measured"""
    kr, kb = (float(k) for k in KR_KB[matrix])
    kg = 1 - kr - kb
    _, ys, cs = constants(range_)
    return (0.5 / ys + 2 * (1 - kr) * 0.5 / cs, 0.5 / ys + (2 * (1 - kb) * kb / kg + 2 * (1 - kr) * kr / kg) * 0.5 / cs,
            0.5 / ys + 2 * (1 - kb) * 0.5 / cs)


# ---------------------------------------------------------------------------------------------------------------- specification
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bt709_tv_center_is_todays_format_bit_for_bit(dtype):
    frameio = sub("frameio")
    for shape in SHAPES + EXTRA_SHAPES:
        x = clip(*shape, 3, seed=sum(shape) + 3).to(dtype)
        got = frameio.pack_yuv420p10_torch(x, "bt709", "tv", "center")
        assert same(got, frameio.pack_frames_torch(x, "yuv420p10")), shape
        assert same(frameio.pack_yuv420p10_torch(x), got)                      # (the defaults)


def test_constants_are_the_decimal_kr_kb_rounded_at_2_to_16():
    frameio = sub("frameio")
    nearest = lambda f: (2 * f.numerator + f.denominator) // (2 * f.denominator)     # (floor of f + 1/2, exact)
    for matrix, (kr, kb) in KR_KB.items():
        kr, kb = Fraction(kr), Fraction(kb)
        kg = 1 - kr - kb
        wr, wg, wb = nearest(kr * 65536), nearest(kg * 65536), nearest(kb * 65536)
        wg += 65536 - (wr + wg + wb)
        cb = (nearest(-kr / (2 * (1 - kb)) * 65536), nearest(-kg / (2 * (1 - kb)) * 65536))
        cr = (nearest(-kg / (2 * (1 - kr)) * 65536), nearest(-kb / (2 * (1 - kr)) * 65536))
        assert (wr, wg, wb) + cb + cr == TABLE[matrix] == frameio.yuv_matrix(matrix), matrix
        assert wr + wg + wb == 65536 and sum(cb) + 32768 == 0 and sum(cr) + 32768 == 0, matrix
    assert nearest(Fraction("0.678") * 65536) == 44433                         # bt2020's green before the deficit goes to it
    fin = sub("frameio_in")
    for range_ in RANGES:
        assert fin.yuv_constants(10, range_)[:3] == constants(range_)
    assert tuple(frameio.KR_KB) == MATRICES and frameio.YUV_RANGES == RANGES and frameio.SITINGS == SITINGS
    assert frameio.FORMATS == ("rgb8", "bgr8", "yuv420p10")                    # the new planes are no new format


CHECK = {("bt2020", "tv"): ((294, 387, 960), (658, 189, 100), (116, 960, 476)), ("bt601", "tv"): ((326, 361, 960), (578, 215, 137), (164, 960, 439)),
         ("bt709", "tv"): ((250, 409, 960), (691, 167, 105), (127, 960, 471)), ("bt709", "pc"): ((217, 395, 1023), (732, 118, 47), (74, 1023, 465)),
         ("bt2020", "pc"): ((269, 369, 1023), (694, 143, 42), (61, 1023, 471))}


@pytest.mark.parametrize("siting", SITINGS)
def test_check_values_of_the_specification(siting):
    frameio = sub("frameio")

    def flat(colour, matrix, range_):
        x = torch.tensor(colour, dtype=torch.float32).expand(1, 2, 2, 3).contiguous()
        out = frameio.pack_yuv420p10_torch(x, matrix, range_, siting)[0].tolist()
        assert out[:4] == [out[0]] * 4
        return out[0], out[4], out[5]

    for matrix in MATRICES:
        assert flat((1, 1, 1), matrix, "tv") == (940, 512, 512) and flat((0, 0, 0), matrix, "tv") == (64, 512, 512)
        assert flat((0.5, 0.5, 0.5), matrix, "tv") == (502, 512, 512)
        assert flat((1, 1, 1), matrix, "pc") == (1023, 512, 512) and flat((0, 0, 0), matrix, "pc") == (0, 512, 512)
    for (matrix, range_), (red, green, blue) in CHECK.items():
        assert flat((1, 0, 0), matrix, range_) == red and flat((0, 1, 0), matrix, range_) == green, (matrix, range_)
        assert flat((0, 0, 1), matrix, range_) == blue, (matrix, range_)
    # non-finite input as in every format: NaN -> 0, +inf -> full scale, -inf -> 0
    assert flat((float("nan"), float("inf"), -float("inf")), "bt2020", "tv") == (658, 189, 100)


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("range_", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_round_trip_of_flat_frames_stays_within_the_quantisation_bound(matrix, range_, siting):
    """4096 random colours, one per 2 x 2 frame, inverted in fp64 here: per channel within half a code of Y and of each chroma plane
    through the inverse (bounds()), plus 2/65535 for the 16-bit codes the planes are computed from."""
    frameio = sub("frameio")
    g = torch.Generator().manual_seed(11)
    colours = torch.rand(4096, 1, 1, 3, generator=g)
    x = colours.expand(4096, 2, 2, 3).contiguous()
    Y, cb, cr = planes(frameio.pack_yuv420p10_torch(x, matrix, range_, siting), 2, 2)
    assert bool((Y == Y[:, :1, :1]).all())
    rgb = inverse(Y[:, 0, 0].double(), cb[:, 0, 0].double(), cr[:, 0, 0].double(), matrix, range_)
    for c, (got, bound) in enumerate(zip(rgb, bounds(matrix, range_))):
        err = float((got - colours[:, 0, 0, c].double()).abs().max())
        print(f"{matrix} {range_} {siting} channel {c}: max error {err:.3e}, bound {bound:.3e} + 2/65535")
        assert err <= bound + 2 / 65535, (c, err, bound)
    if siting == "left":                                                       # flat frames: the same codes for both sitings
        assert same(frameio.pack_yuv420p10_torch(x, matrix, range_, "left"), frameio.pack_yuv420p10_torch(x, matrix, range_, "center"))


def test_left_siting_is_what_the_unpack_upsampler_assumes_and_center_is_not():
    """A horizontal colour ramp (R 0.2 -> 0.8, G 0.4, B 0.7 -> 0.3 over 64 columns), packed as BT.2020 tv, its chroma upsampled by
    frameio_in.upsample_chroma (co-sited with even luma columns) and inverted in fp64, columns 2..61: "left" stays within the bounds
    of the flat-frame test; "center" -- the same samples half a luma pixel to the right -- exceeds them on R and B."""
    frameio, fin = sub("frameio"), sub("frameio_in")
    H, W = 8, 64
    x = torch.empty(1, H, W, 3)
    x[..., 0] = torch.linspace(0.2, 0.8, W)
    x[..., 1] = 0.4
    x[..., 2] = torch.linspace(0.7, 0.3, W)
    limit = [b + 2 / 65535 for b in bounds("bt2020", "tv")]
    errs = {}
    for siting in SITINGS:
        Y, cb, cr = planes(frameio.pack_yuv420p10_torch(x, "bt2020", "tv", siting), H, W)
        cb8, cr8 = fin.upsample_chroma(cb, H, W).double() / 8, fin.upsample_chroma(cr, H, W).double() / 8
        rgb = inverse(Y.double(), cb8, cr8, "bt2020", "tv")
        errs[siting] = [float((rgb[c] - x[..., c].double()).abs()[:, :, 2:62].max()) for c in range(3)]
        print(f"{siting}: max error R {errs[siting][0]:.3e} G {errs[siting][1]:.3e} B {errs[siting][2]:.3e}; limits "
              + " ".join(f"{v:.3e}" for v in limit))
    assert all(e <= v for e, v in zip(errs["left"], limit)), errs
    assert errs["center"][0] > limit[0] and errs["center"][2] > limit[2], errs


def test_left_siting_weights_and_clamps_at_the_frame_edges():
    """An impulse in one column: column 2k gets weight 2 of 8 per row in sample k, an odd column weight 1 in both neighbours; the
    columns beyond either edge repeat the edge (odd W: the last sample is 1 + 2 + 1 of [W-2, W-1, W-1])."""
    frameio = sub("frameio")
    for W in (5, 6):
        for col in range(W):
            x = torch.zeros(1, 2, W, 3)
            x[0, :, col, 2] = 1.0                                              # blue: Cb rises by 448 * weight / 8 above 512
            _, cb, _ = planes(frameio.pack_yuv420p10_torch(x, "bt709", "tv", "left"), 2, W)
            w2 = (W + 1) // 2
            want = [0] * w2
            for k in range(w2):
                for d, wgt in ((-1, 1), (0, 2), (1, 1)):
                    if min(max(2 * k + d, 0), W - 1) == col:
                        want[k] += 2 * wgt                                     # (two rows)
            assert sum(want) > 0 and [round((int(c) - 512) / 448 * 8) for c in cb[0, 0]] == want, (W, col, cb, want)


def test_refusals_name_the_argument():
    frameio = sub("frameio")
    x = torch.rand(1, 4, 6, 3)
    for kw, word in ((dict(matrix="bt2100"), "matrix"), (dict(range_="full"), "range_"), (dict(siting="topleft"), "siting")):
        with pytest.raises(ValueError, match=word):
            frameio.pack_yuv420p10_torch(x, **kw)
        with pytest.raises(ValueError, match=word):
            frameio.pack_yuv420p10(x, **kw)
    with pytest.raises(ValueError, match="C = 3"):
        frameio.pack_yuv420p10_torch(torch.rand(1, 4, 6, 4), "bt2020", "tv", "left")
    with pytest.raises(ValueError, match="fp32 or bf16"):
        frameio.pack_yuv420p10_torch(x.double(), "bt2020", "tv", "left")
    with pytest.raises(ValueError, match="fp32 or bf16"):
        frameio.pack_yuv420p10_torch(x[0], "bt2020", "tv", "left")
    for out in (torch.zeros(1, 24 + 12, dtype=torch.int16), torch.zeros(1, 24 + 11, dtype=torch.uint16), torch.zeros(24 + 12, dtype=torch.uint16)):
        with pytest.raises(ValueError, match="out must be"):
            frameio.pack_yuv420p10(x, "bt2020", "tv", "left", out=out)


def test_pack_yuv420p10_uses_the_backend_and_never_falls_back():
    frameio, hip_lib = sub("frameio"), sub("hip_lib")
    from ops_reference import TorchOps
    x = torch.rand(1, 3, 5, 3)

    class Failing:
        def pack_yuv420p10(self, *a, **k):
            raise hip_lib.HipLibraryError("svr_pack_yuv420p10 failed")

    class Marking:
        def pack_yuv420p10(self, frames, matrix, range_, siting, out=None):
            return ("backend", matrix, range_, siting, out)

    with pytest.raises(hip_lib.HipLibraryError):
        frameio.pack_yuv420p10(x, "bt2020", "tv", "left", ops=Failing())
    assert frameio.pack_yuv420p10(x, "bt601", "pc", "left", ops=Marking()) == ("backend", "bt601", "pc", "left", None)
    assert not hasattr(TorchOps("cpu"), "pack_yuv420p10")
    want = frameio.pack_yuv420p10_torch(x, "bt2020", "tv", "left")
    assert same(frameio.pack_yuv420p10(x, "bt2020", "tv", "left", ops=TorchOps("cpu")), want)
    out = torch.zeros(1, 15 + 2 * 2 * 3, dtype=torch.uint16)
    assert frameio.pack_yuv420p10(x, "bt2020", "tv", "left", out=out) is out and same(out, want)


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_entry_point_refuses_invalid_arguments_before_any_launch():
    """Null pointers, an unknown dtype, matrix, range or siting code, empty dimensions, an out_bytes that is not exactly the planes'
    size, a misaligned pointer: refused on the host with a message naming the argument.  No device is needed: nothing is launched."""
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    call = lambda frames=p, kind=1, T=1, H=4, W=6, matrix=2, range_=0, siting=1, out=p, nbytes=None: L.svr_pack_yuv420p10(
        frames, kind, T, H, W, matrix, range_, siting, out, 2 * T * (H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)) if nbytes is None else nbytes,
        None)
    cases = [(lambda: call(frames=None), b"frames"), (lambda: call(out=None), b"out"), (lambda: call(kind=2), b"x_kind"),
             (lambda: call(kind=-1), b"x_kind"), (lambda: call(T=0), b"T >= 1"), (lambda: call(H=0), b"H >= 1"), (lambda: call(W=-3), b"W >= 1"),
             (lambda: call(matrix=3), b"matrix"), (lambda: call(matrix=-1), b"matrix"), (lambda: call(range_=2), b"range"),
             (lambda: call(range_=-1), b"range"), (lambda: call(siting=2), b"siting"), (lambda: call(siting=-1), b"siting"),
             (lambda: call(nbytes=71), b"out_bytes"), (lambda: call(nbytes=73), b"out_bytes"), (lambda: call(nbytes=0), b"out_bytes"),
             (lambda: call(nbytes=2 * 24), b"out_bytes"), (lambda: call(H=5, W=7, nbytes=2 * (35 + 2 * 2 * 3)), b"out_bytes"),
             (lambda: call(T=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, nbytes=8), b"T * H * W"),
             (lambda: call(T=2 ** 21, H=2 ** 10, W=2 ** 10, nbytes=8), b"T * H * W"),
             (lambda: call(frames=ctypes.c_void_p(base + 2)), b"frames"), (lambda: call(kind=0, frames=ctypes.c_void_p(base + 1)), b"frames"),
             (lambda: call(out=ctypes.c_void_p(base + 1)), b"out")]
    for fn, word in cases:
        assert fn() != 0
        msg = L.svr_last_error()
        assert b"svr_pack_yuv420p10" in msg and word in msg, msg


def test_header_ctypes_tables_and_build_list_know_the_entry_point():
    hip_lib, frameio, fin = sub("hip_lib"), sub("frameio"), sub("frameio_in")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert "svr_pack_yuv420p10" in declared and declared == set(hip_lib.SYMBOLS)
    decl = re.search(r"int svr_pack_yuv420p10\(([^;]*)\);", src).group(1)
    assert len(decl.split(",")) == 11 == len(hip_lib.SYMBOLS["svr_pack_yuv420p10"][1])
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert re.search(r"v9, additive: \+ svr_pack_yuv420p10\(\).*?A new symbol only", src, flags=re.S)
    for table, prefix in ((hip_lib.COLOUR_MATRICES, "SVR_COLOUR_MATRIX_"), (hip_lib.COLOUR_RANGES, "SVR_COLOUR_RANGE_"),
                          (hip_lib.COLOUR_SITINGS, "SVR_COLOUR_SITING_")):
        for name, code in table.items():
            assert re.search(rf"#define {prefix}{name.upper()}\s+{code}\b", src), name
    assert tuple(hip_lib.COLOUR_MATRICES) == tuple(frameio.KR_KB) and tuple(hip_lib.COLOUR_RANGES) == frameio.YUV_RANGES
    assert tuple(hip_lib.COLOUR_SITINGS) == frameio.SITINGS
    # the tables that existed gained nothing: the input side has no bt2020
    assert hip_lib.YUV_MATRICES == {"bt709": 0, "bt601": 1} and tuple(fin.MATRICES) == ("bt709", "bt601")
    assert hip_lib.PACK_FORMATS == {"rgb8": 0, "bgr8": 1, "yuv420p10": 2} and not re.search(r"#define SVR_MATRIX_BT2020", src)
    api = open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert '#include "svr_frame_pack_colour.hip"' in api
    assert os.path.join(hip_lib.CSRC, "svr_frame_pack_colour.hip") in hip_lib.sources()   # (the loader's source hash covers it)
    for matrix, row in TABLE.items():                                          # the entry point's constants are the specification's
        assert ", ".join(map(str, row)) in api, matrix


# ---------------------------------------------------------------------------------------------------------------- command line
def test_probe_colour_reads_the_five_tags_and_probe_video_is_unchanged(cli, tmp_path):
    ffprobe, _ = stand_ins(str(tmp_path / "bin"))
    path = tmp_path / "clip.mkv"
    tagged(path, None, "yuv420p10le", 1920, 1080, rate="30000/1001", audio=True, color_space="bt2020nc", color_range="tv",
           color_primaries="bt2020", color_transfer="smpte2084", chroma_location="left")
    assert cli.probe_colour(ffprobe, str(path)) == dict(color_space="bt2020nc", color_primaries="bt2020", color_transfer="smpte2084",
                                                        color_range="tv", chroma_location="left")
    assert cli.probe_video(ffprobe, str(path)) == dict(width=1920, height=1080, fps=Fraction(30000, 1001), pix_fmt="yuv420p10le",
                                                       color_space="bt2020nc", color_range="tv", has_audio=True)
    tagged(path, None, "yuv420p", 640, 360, color_primaries="unknown", color_transfer="unspecified", chroma_location="")
    assert cli.probe_colour(ffprobe, str(path)) == dict(color_space=None, color_primaries=None, color_transfer=None, color_range=None,
                                                        chroma_location=None)
    assert cli.probe_video(ffprobe, str(path)) == dict(width=640, height=360, fps=Fraction(24), pix_fmt="yuv420p", color_space=None,
                                                       color_range=None, has_audio=False)
    assert len(calls(str(tmp_path / "bin"))) == 4                              # one ffprobe run per call
    with pytest.raises(RuntimeError, match="ffprobe exited with status"):
        cli.probe_colour(ffprobe, str(tmp_path / "missing.mkv"))


def test_output_colour_routes_hdr_sources_and_warns(cli):
    tags = lambda **kw: dict(dict.fromkeys(cli.COLOUR_FIELDS), **kw)
    bt2020 = dict(matrix="bt2020", range_="tv", siting="left")
    assert cli.output_colour(tags(color_space="bt2020nc", color_primaries="bt2020", color_transfer="smpte2084")) == (
        dict(bt2020, primaries="bt2020", trc="smpte2084"), None)
    assert cli.output_colour(tags(color_transfer="arib-std-b67")) == (dict(bt2020, primaries="bt2020", trc="arib-std-b67"), None)
    assert cli.output_colour(tags(color_primaries="bt2020")) == (dict(bt2020, primaries="bt2020", trc="bt709"), None)
    assert cli.output_colour(tags(color_space="bt2020nc", color_transfer="bt2020-10")) == (dict(bt2020, primaries="bt2020", trc="bt2020-10"), None)
    assert cli.output_colour(tags(color_transfer="smpte2084", color_primaries="smpte432", color_range="pc"))[0] == dict(
        bt2020, primaries="smpte432", trc="smpte2084")                         # (the planes are tv whatever the source's range)
    # not HDR: BT.709 as always, nothing said
    for kw in ({}, dict(color_space="bt709", color_primaries="bt709", color_transfer="bt709"), dict(color_space="smpte170m"),
               dict(color_transfer="bt2020-10"), dict(chroma_location="topleft")):
        assert cli.output_colour(tags(**kw)) == (None, None), kw
    assert cli.output_colour(None) == (None, None) and cli.output_colour(None, "opencv", False) == (None, None)
    # the three warnings: one line each, BT.709 output
    hdr = tags(color_space="bt2020nc", color_primaries="bt2020", color_transfer="smpte2084")
    for args, word in (((tags(color_space="bt2020c", color_primaries="bt2020", color_transfer="smpte2084"),), "bt2020c"),
                       ((hdr, "ffmpeg", False), "--10bit"), ((hdr, "opencv", True), "OpenCV"), ((hdr, "opencv", False), "OpenCV")):
        out, warning = cli.output_colour(*args)
        assert out is None and warning.startswith("Warning: ") and word in warning and "\n" not in warning, args


def tagged(path, packed, pix_fmt, width, height, color_primaries=None, color_transfer=None, chroma_location=None, **kw):
    """frame_unpack_cases.fake_video plus the tags its canned ffprobe answer does not carry"""
    fake_video(path, packed, pix_fmt, width, height, **kw)
    answer = json.load(open(str(path) + ".json"))
    for key, value in (("color_primaries", color_primaries), ("color_transfer", color_transfer), ("chroma_location", chroma_location)):
        if value is not None:
            answer["streams"][0][key] = value
    json.dump(answer, open(str(path) + ".json", "w"))


def ten_bit_argv(tags, size, rate, out):
    return (["-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "yuv420p10le", "-s", size, "-r", rate] + tags + ["-i", "-", "-c:v", "libx265",
            "-pix_fmt", "yuv420p10le", "-preset", "medium", "-crf", "12"] + tags + [str(out)])


BT709_TAGS = ["-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv"]
T, H, W = 13, 8, 10


def run_cli(cli, tmp_path, monkeypatch, chunked, flags, pix="yuv420p10le", fmt="rgb16", **tags):
    """13 frames of 8 x 10 through the identity "engines" into the stand-in encoder -> (its argv, its stdin, the frames it was
    handed by the reader's specification, stderr's lines are the caller's to read)"""
    fin = sub("frameio_in")
    bin_ = str(tmp_path / "bin")
    ffprobe, _ = stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    packed = random_packed(fmt, T, H, W, 3, seed=7)
    src, out = tmp_path / "clip.mkv", tmp_path / "out.mp4"
    tagged(src, packed, pix, W, H, **tags)
    before = cli.probe_video(ffprobe, str(src))
    assert before == dict(width=W, height=H, fps=Fraction(24), pix_fmt=pix, color_space=tags.get("color_space"),
                          color_range=tags.get("color_range"), has_audio=False)
    tail = ["--chunk_size", "5"] if chunked else []
    assert cli.main([str(src), "--video_backend", "ffmpeg", "--output", str(out)] + flags + tail) == 0
    matrix = "bt709" if tags.get("color_space") == "bt709" else "bt601"        # (height 8, nothing said: bt601; rgb16 ignores it)
    frames = fin.unpack_frames_torch(packed, fmt, T, H, W, 3, matrix, "tv")
    return open(str(out) + ".args").read().split("\n"), out.read_bytes(), frames, out


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
@pytest.mark.parametrize("trc", ["smpte2084", "arib-std-b67"])
def test_cli_writes_an_hdr_source_as_bt2020_left_sited_and_tagged(identity, tmp_path, monkeypatch, capsys, chunked, trc):
    frameio = sub("frameio")
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, ["--10bit"], color_space="bt2020nc", color_range="tv",
                                       color_primaries="bt2020", color_transfer=trc, chroma_location="left")
    tags = ["-colorspace", "bt2020nc", "-color_primaries", "bt2020", "-color_trc", trc, "-color_range", "tv", "-chroma_sample_location", "left"]
    assert argv == ten_bit_argv(tags, "10x8", "24", out)                       # the five tags on the raw input side and on the output side
    assert piped == frameio.pack_yuv420p10_torch(frames, "bt2020", "tv", "left").numpy().astype("<u2").tobytes()
    assert piped != frameio.pack_frames_torch(frames, "yuv420p10").numpy().astype("<u2").tobytes()
    assert "Warning" not in capsys.readouterr().err
    log = calls(str(tmp_path / "bin"))
    assert [line.split()[0] for line in log] == ["ffprobe", "ffprobe", "ffmpeg", "ffmpeg"]      # (the test's own probe, main's ONE, decoder, encoder)


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
@pytest.mark.parametrize("tags", [dict(color_space="bt709", color_range="tv", color_primaries="bt709", color_transfer="bt709", chroma_location="left"), {}],
                         ids=["bt709", "untagged"])
def test_cli_writes_every_other_source_as_it_always_did(identity, tmp_path, monkeypatch, capsys, chunked, tags):
    frameio = sub("frameio")
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, ["--10bit"], fmt="yuv420p10", **tags)
    assert argv == ten_bit_argv(BT709_TAGS, "10x8", "24", out)
    assert piped == frameio.pack_frames_torch(frames, "yuv420p10").numpy().astype("<u2").tobytes()
    assert "Warning" not in capsys.readouterr().err
    # a source that is not read through ffprobe: a .npy of the same frames
    np.save(tmp_path / "clip.npy", frames.numpy())
    tail = ["--chunk_size", "5"] if chunked else []
    assert identity.main([str(tmp_path / "clip.npy"), "--video_backend", "ffmpeg", "--10bit", "--output_format", "mp4", "--output", str(out)] + tail) == 0
    assert open(str(out) + ".args").read().split("\n") == ten_bit_argv(BT709_TAGS, "10x8", "30", out)
    assert out.read_bytes() == piped


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_cli_warns_once_and_writes_todays_output(identity, tmp_path, monkeypatch, capsys, chunked):
    frameio = sub("frameio")
    # constant-luminance BT.2020 with --10bit: today's 10-bit BT.709 command and bytes
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, ["--10bit"], color_space="bt2020c", color_range="tv",
                                       color_primaries="bt2020", color_transfer="smpte2084")
    assert argv == ten_bit_argv(BT709_TAGS, "10x8", "24", out)
    assert piped == frameio.pack_frames_torch(frames, "yuv420p10").numpy().astype("<u2").tobytes()
    err = capsys.readouterr().err.splitlines()
    assert len(err) == 1 and err[0].startswith("Warning: ") and "bt2020c" in err[0], err
    # an HDR source without --10bit: today's 8-bit command and bytes
    argv, piped, frames, out = run_cli(identity, tmp_path, monkeypatch, chunked, [], color_space="bt2020nc", color_range="tv",
                                       color_primaries="bt2020", color_transfer="smpte2084")
    assert argv == TODAY[:10] + ["24"] + TODAY[11:] + [str(out)]
    assert piped == frameio.pack_frames_torch(frames, "bgr8").numpy().tobytes()
    err = capsys.readouterr().err.splitlines()
    assert len(err) == 1 and err[0].startswith("Warning: ") and "--10bit" in err[0], err
    # the same source into png files: no video is written, nothing to warn about
    assert identity.main([str(tmp_path / "clip.mkv"), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "png")]
                         + (["--chunk_size", "5"] if chunked else [])) == 0
    assert len(os.listdir(tmp_path / "png")) == T and capsys.readouterr().err == ""


def test_sink_asks_the_writer_how_to_pack(cli):
    """A writer whose ``pack`` names (matrix, range_, siting) is handed those planes; one without the attribute, or with None, is
    packed by its ``fmt`` exactly as before."""
    frameio = sub("frameio")
    x = clip(3, 5, 7, 3, seed=12)

    def through(**attrs):
        seen = []
        writer = type("Keep", (), dict(fmt="yuv420p10", alpha=False, write=lambda self, arr, h, w: seen.append(arr.copy()),
                                       close=lambda self: None, **attrs))()
        sink = cli.FrameSink(writer)
        sink.put(x)
        sink.close()
        return torch.from_numpy(seen[0])

    assert same(through(pack=("bt2020", "tv", "left")), frameio.pack_yuv420p10_torch(x, "bt2020", "tv", "left"))
    assert same(through(pack=("bt601", "pc", "center")), frameio.pack_yuv420p10_torch(x, "bt601", "pc", "center"))
    assert same(through(), frameio.pack_frames_torch(x, "yuv420p10")) and same(through(pack=None), frameio.pack_frames_torch(x, "yuv420p10"))
    w = cli.FFmpegWriter("ffmpeg", "o.mp4", 24.0, ten_bit=True, colour=cli.output_colour(dict(color_transfer="smpte2084"))[0])
    assert w.pack == ("bt2020", "tv", "left") and w.fmt == "yuv420p10"
    assert cli.FFmpegWriter("ffmpeg", "o.mp4", 24.0, ten_bit=True).pack is None
    assert cli.FFmpegWriter("ffmpeg", "o.mp4", 24.0, ten_bit=False, colour=dict(matrix="bt2020", range_="tv", siting="left", primaries="bt2020",
                                                                               trc="smpte2084")).pack is None      # (8 bits: ffmpeg converts bgr24)
