"""-m "not gpu": the packed input formats (frameio_in.py, the specification of csrc/svr_frame_unpack.hip) -- every code decoded to
the nearest fp32 value, the check values of its docstring, the integer matrix against exact fractions, the chroma siting, the round
trip with the shipped pack --, the C ABI's refusals, and the command line's ffmpeg reader (probe, routing, FrameSource, audio
passthrough) against stand-ins for the two executables (tests/frame_unpack_cases.py).  NOT covered anywhere: a real ffmpeg."""
import ctypes
import os
import random
import re
import shutil
import signal
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from frame_unpack_cases import SHAPES, calls, channel_counts, fake_video, random_packed, stand_ins
from test_stream import ARGS, KW, cli, rig, split  # noqa: F401 (cli, rig: fixtures)

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def nearest_fp32(q, D):
    """float(Fraction(q, D)) is the correctly rounded double; numpy rounds it once more to fp32: 53 >= 2 * 24 + 2 bits"""
    return np.float32(float(Fraction(q, D)))


# ---------------------------------------------------------------------------------------------------------------- specification
def test_every_rgb_code_decodes_to_the_nearest_fp32_value():
    fin = sub("frameio_in")
    for fmt, D, dtype in (("rgb8", 255, torch.uint8), ("bgr8", 255, torch.uint8), ("rgb16", 65535, torch.uint16)):
        n = D + 1
        assert n % 4 == 0
        q = torch.arange(n, dtype=torch.int64)
        got = fin.unpack_frames_torch(q.to(dtype).reshape(1, 1, n // 4, 4), fmt, 1, 1, n // 4, 4)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, n // 4, 4) and got.is_contiguous()
        want = torch.from_numpy(np.array([nearest_fp32(int(v), D) for v in q], dtype=np.float32)).reshape(1, 1, n // 4, 4)
        if fmt == "bgr8":
            want = want[..., [2, 1, 0, 3]]
        assert torch.equal(got, want), fmt
    # the trap the specification avoids: q * (1 / D) is NOT the nearest value for every code
    q = torch.arange(65536, dtype=torch.float32)
    assert not torch.equal(q * torch.tensor(1.0 / 65535, dtype=torch.float32), fin.unit(q.long(), 65535))


CHECK_VALUES = [  # (bits, range_, (Y, Cb, Cr), 16-bit codes)
    (10, "tv", (940, 512, 512), (65535, 65535, 65535)), (10, "tv", (64, 512, 512), (0, 0, 0)),
    (10, "tv", (502, 512, 512), (32768, 32768, 32768)), (10, "tv", (250, 409, 960), (65517, 0, 0)),
    (10, "tv", (691, 167, 105), (27, 65535, 83)), (10, "tv", (127, 960, 471), (0, 0, 65517)),
    (8, "tv", (235, 128, 128), (65535, 65535, 65535)), (8, "pc", (255, 128, 128), (65535, 65535, 65535)),
    (10, "pc", (1023, 512, 512), (65535, 65535, 65535))]


def test_check_values_of_the_specification():
    fin = sub("frameio_in")
    for bits, range_, yuv, codes in CHECK_VALUES:
        fmt, dtype = ("yuv420p8", torch.uint8) if bits == 8 else ("yuv420p10", torch.uint16)
        want = torch.tensor([nearest_fp32(c, 65535) for c in codes])
        one = fin.unpack_frames_torch(torch.tensor([yuv], dtype=torch.int64).to(dtype), fmt, 1, 1, 1, 3, "bt709", range_)
        assert torch.equal(one.flatten(), want), (bits, range_, yuv, (one.flatten() * 65535).tolist())
        # a flat 2 x 2 block: the four pixels share the chroma sample, every interpolation weight falls on it
        flat = torch.tensor([[yuv[0]] * 4 + [yuv[1], yuv[2]]], dtype=torch.int64).to(dtype)
        four = fin.unpack_frames_torch(flat, fmt, 1, 2, 2, 3, "bt709", range_)
        assert torch.equal(four.reshape(4, 3), want.expand(4, 3)), (bits, range_, yuv)
    assert fin.yuv_constants(10, "tv") == (64, 876, 896, 4096) and fin.yuv_constants(8, "pc") == (0, 255, 255, 1024)


def test_coefficients_are_the_decimal_constants_rounded_at_2_to_16():
    fin = sub("frameio_in")
    for name, kr, kb in (("bt709", Fraction(2126, 10000), Fraction(722, 10000)), ("bt601", Fraction(299, 1000), Fraction(114, 1000))):
        kg = 1 - kr - kb
        exact = (2 * (1 - kr), 2 * (1 - kb) * kb / kg, 2 * (1 - kr) * kr / kg, 2 * (1 - kb))          # rv, gu, gv, bu
        assert fin.MATRICES[name] == tuple(round(c * 65536) for c in exact), name


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("range_", ["tv", "pc"])
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
def test_formula_equals_its_evaluation_in_exact_fractions(bits, range_, matrix):
    """300 random (Y, cb8, cr8) over the whole code range plus the corners of it: q = clamp(floor(num / Den + 1/2), 0, 65535) with
    num / Den evaluated as a Fraction.  The corners make numerators negative (Y = 0 with saturated chroma) and push them past full
    scale."""
    import math
    fin = sub("frameio_in")
    rng = random.Random(bits * 7 + len(range_) + len(matrix))
    top = (1 << bits) - 1
    cases = [(rng.randint(0, top), rng.randint(0, 8 * top), rng.randint(0, 8 * top)) for _ in range(300)]
    cases += [(y, cb, cr) for y in (0, top) for cb in (0, 8 * top) for cr in (0, 8 * top)]
    rv, gu, gv, bu = fin.MATRICES[matrix]
    y0, ys, cs, mid = fin.yuv_constants(bits, range_)
    Y, cb8, cr8 = (torch.tensor(c, dtype=torch.int64) for c in zip(*cases))
    got = torch.stack(fin.yuv_codes(Y, cb8, cr8, bits, matrix, range_), dim=-1).tolist()
    negative = 0
    for (y, cb, cr), codes in zip(cases, got):
        u, v = cb - mid, cr - mid
        luma = Fraction(y - y0, ys)
        exact = (luma + Fraction(rv * v, 8 * cs * 65536), luma - Fraction(gu * u + gv * v, 8 * cs * 65536), luma + Fraction(bu * u, 8 * cs * 65536))
        negative += sum(e < 0 for e in exact)
        want = [min(max(math.floor(65535 * e + Fraction(1, 2)), 0), 65535) for e in exact]
        assert codes == want, (y, cb, cr)
    assert negative > 20


def test_chroma_impulse_spreads_with_the_weights_of_the_siting():
    """One chroma sample of 1 at (1, 1) of a 3 x 3 plane (a 6 x 6 frame): vertically 1, 3 | 3, 1 quarters over luma rows 1..4,
    horizontally 1, 2, 1 over columns 1..3 -- co-sited with the even column 2, midway between rows 2 and 3."""
    fin = sub("frameio_in")
    c = torch.zeros(1, 3, 3, dtype=torch.int64)
    c[0, 1, 1] = 1
    want = torch.zeros(6, 6, dtype=torch.int64)
    want[1:5, 1:4] = torch.tensor([1, 3, 3, 1])[:, None] * torch.tensor([1, 2, 1])[None, :]
    assert torch.equal(fin.upsample_chroma(c, 6, 6)[0], want) and int(want.sum()) == 32
    # a flat plane stays flat, times 8, at every size: the weights sum to 8 also where the indices clamp
    for H, W in ((6, 6), (5, 5), (1, 1), (2, 7), (7, 2)):
        flat = torch.full((1, (H + 1) // 2, (W + 1) // 2), 5, dtype=torch.int64)
        assert torch.equal(fin.upsample_chroma(flat, H, W), torch.full((1, H, W), 40, dtype=torch.int64)), (H, W)
    # odd H and W (5 x 5 over the same 3 x 3 plane): an impulse in the LAST chroma row / column.  Rows 4 (= 2j, takes C[1] + 3 C[2])
    # and 3 (= 2j + 1 of the row above, takes C[2] once); column 4 (even: twice the value) and 3 (odd: the sum with column k + 1)
    c = torch.zeros(1, 3, 3, dtype=torch.int64)
    c[0, 2, 2] = 1
    want = torch.zeros(5, 5, dtype=torch.int64)
    want[3:5, 3:5] = torch.tensor([1, 3])[:, None] * torch.tensor([1, 2])[None, :]
    assert torch.equal(fin.upsample_chroma(c, 5, 5)[0], want)
    # even sizes: the last luma row 2j + 1 asks for C[j + 1] beyond the plane and takes C[j] again (3 + 1 = 4 quarters); the odd
    # last column asks for k + 1 beyond the row and takes k again (1 + 1 = 2)
    assert torch.equal(fin.upsample_chroma(c, 6, 6)[0, 3:, 3:], torch.tensor([1, 3, 4])[:, None] * torch.tensor([1, 2, 2])[None, :])
    # ... and the first row 2j = 0 asks for C[-1] and takes C[0] again
    c = torch.zeros(1, 3, 3, dtype=torch.int64)
    c[0, 0, 0] = 1
    assert torch.equal(fin.upsample_chroma(c, 6, 6)[0, :3, :3], torch.tensor([4, 3, 1])[:, None] * torch.tensor([2, 1, 0])[None, :])


def test_round_trip_with_the_shipped_pack_stays_within_the_two_quantisation_steps():
    """unpack(pack(x, yuv420p10)) on flat 2 x 2 frames of 4 000 seeded random colours plus the eight cube corners.  The bound is
    DERIVED, not fitted: half a 10-bit luma step (0.5 / 876), half a chroma step carried through the matrix row (c * 0.5 / 896 with
    c = 2 (1 - Kr) = 1.5748 for R, 2 (1 - Kb) = 1.8556 for B, their Kr / Kg, Kb / Kg weighted sum 0.6554 bounding G), and 2 / 65535
    for the two roundings to 16-bit codes: 1.48e-3, 0.97e-3, 1.64e-3."""
    fin, frameio = sub("frameio_in"), sub("frameio")
    g = torch.Generator().manual_seed(0)
    colours = torch.cat([torch.rand(4000, 3, generator=g), torch.tensor([[r, gg, b] for r in (0.0, 1.0) for gg in (0.0, 1.0) for b in (0.0, 1.0)])])
    x = colours[:, None, None, :].expand(-1, 2, 2, 3).contiguous()
    T = x.shape[0]
    back = fin.unpack_frames_torch(frameio.pack_frames_torch(x, "yuv420p10"), "yuv420p10", T, 2, 2, 3)
    dev = (back.double() - x.double()).abs().amax(dim=(0, 1, 2))
    bound = [0.5 / 876 + c * 0.5 / 896 + 2 / 65535 for c in (1.5748, 0.6554, 1.8556)]
    print("max deviation R, G, B:", [f"{float(d):.3e}" for d in dev], "bounds:", [f"{b:.3e}" for b in bound])
    for d, b in zip(dev.tolist(), bound):
        assert d <= b


def test_eight_bit_round_trip_is_exact():
    fin, frameio = sub("frameio_in"), sub("frameio")
    for C in (3, 4):
        codes = random_packed("rgb8", 2, 5, 7, C, seed=C)
        for fmt in ("rgb8", "bgr8"):
            x = fin.unpack_frames_torch(codes, fmt, 2, 5, 7, C)
            assert torch.equal(frameio.pack_frames_torch(x, fmt), codes), (fmt, C)
        # bgr8 is rgb8 with channels 0 and 2 swapped, a fourth in place
        order = [2, 1, 0] + ([3] if C == 4 else [])
        assert torch.equal(fin.unpack_frames_torch(codes, "bgr8", 2, 5, 7, C), fin.unpack_frames_torch(codes, "rgb8", 2, 5, 7, C)[..., order])


def test_ten_bit_samples_beyond_1023_count_as_1023():
    fin = sub("frameio_in")
    p = random_packed("yuv420p10", 1, 3, 5, 3, seed=1)
    wild = p.clone()
    wild.view(torch.int16)[p.view(torch.int16) >= 1000] = -1                 # (0xffff)
    capped = p.clone()
    capped.view(torch.int16)[p.view(torch.int16) >= 1000] = 1023
    assert torch.equal(fin.unpack_frames_torch(wild, "yuv420p10", 1, 3, 5, 3), fin.unpack_frames_torch(capped, "yuv420p10", 1, 3, 5, 3))


def test_refusals_name_the_argument():
    fin = sub("frameio_in")
    p = random_packed("yuv420p10", 1, 4, 6, 3, seed=0)
    for kw, word in ((dict(fmt="yuv422p"), "fmt"), (dict(matrix="bt2020"), "matrix"), (dict(range_="full"), "range_"), (dict(C=4), "C = 3"),
                     (dict(H=5), "packed must hold"), (dict(T=0), "T, H, W"), (dict(fmt="yuv420p8"), "packed must be torch.uint8")):
        args = dict(fmt="yuv420p10", T=1, H=4, W=6, C=3, matrix="bt709", range_="tv")
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            fin.unpack_frames_torch(p, **args)
    with pytest.raises(ValueError, match="C = 3 or 4"):
        fin.unpack_frames_torch(torch.zeros(1, 2, 2, 2, dtype=torch.uint8), "rgb8", 1, 2, 2, 2)
    with pytest.raises(ValueError, match="packed must be torch.uint16"):
        fin.unpack_frames_torch(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), "rgb16", 1, 2, 2, 3)
    assert fin.frame_bytes(5, 7, 3, "yuv420p10") == 2 * (35 + 2 * 3 * 4) and fin.frame_bytes(5, 7, 4, "rgb16") == 5 * 7 * 4 * 2


def test_unpack_frames_uses_the_backend_and_never_falls_back():
    fin, hip_lib = sub("frameio_in"), sub("hip_lib")
    from ops_reference import TorchOps
    p = random_packed("rgb8", 1, 3, 5, 3, seed=2)

    class Failing:
        def unpack_frames(self, *a, **k):
            raise hip_lib.HipLibraryError("svr_unpack_frames failed")

    class Marking:
        def unpack_frames(self, packed, fmt, T, H, W, C, matrix, range_, out=None):
            return ("backend", fmt, (T, H, W, C), matrix, range_, out)

    with pytest.raises(hip_lib.HipLibraryError):
        fin.unpack_frames(p, "rgb8", 1, 3, 5, 3, ops=Failing())
    assert fin.unpack_frames(p, "bgr8", 1, 3, 5, 3, "bt601", "pc", ops=Marking()) == ("backend", "bgr8", (1, 3, 5, 3), "bt601", "pc", None)
    assert not hasattr(TorchOps("cpu"), "unpack_frames")
    want = fin.unpack_frames_torch(p, "rgb8", 1, 3, 5, 3)
    assert torch.equal(fin.unpack_frames(p, "rgb8", 1, 3, 5, 3, ops=TorchOps("cpu")), want)
    out = torch.zeros(1, 3, 5, 3)
    assert fin.unpack_frames(p, "rgb8", 1, 3, 5, 3, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError, match="out"):
        fin.unpack_frames(p, "rgb8", 1, 3, 5, 3, out=torch.zeros(1, 3, 5, 4))


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_unpack_entry_point_refuses_invalid_arguments_before_any_launch():
    """Null pointers, non-positive sizes, unknown format / matrix / range codes, a channel count the format does not take, byte
    counts that are not exactly the format's, misaligned pointers: refused on the host with a message naming the argument.  No
    device is needed: nothing is launched."""
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    F = hip_lib.UNPACK_FORMATS

    def size(fmt, T, H, W, C):
        if fmt in (F["yuv420p8"], F["yuv420p10"]):
            n = T * (H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2))
        else:
            n = T * H * W * C
        return n * (2 if fmt in (F["rgb16"], F["yuv420p10"]) else 1)

    def call(packed=p, nin=None, fmt=0, T=1, H=4, W=6, C=3, matrix=0, range_=0, out=p, nout=None):
        return L.svr_unpack_frames(packed, size(fmt, T, H, W, C) if nin is None else nin, fmt, T, H, W, C, matrix, range_, out,
                                   4 * T * H * W * C if nout is None else nout, None)

    yuv10 = F["yuv420p10"]
    cases = [(lambda: call(packed=None), b"packed"), (lambda: call(out=None), b"out"), (lambda: call(T=0), b"T >= 1"),
             (lambda: call(H=0), b"H >= 1"), (lambda: call(W=-3), b"W >= 1"), (lambda: call(fmt=5), b"fmt"), (lambda: call(fmt=-1), b"fmt"),
             (lambda: call(C=2), b"C must be"), (lambda: call(C=5, fmt=F["rgb16"]), b"C must be"), (lambda: call(C=4, fmt=yuv10), b"C must be 3"),
             (lambda: call(C=4, fmt=F["yuv420p8"], nin=36), b"C must be 3"), (lambda: call(matrix=2), b"matrix"), (lambda: call(matrix=-1), b"matrix"),
             (lambda: call(range_=2), b"range"), (lambda: call(nin=71), b"packed_bytes"), (lambda: call(nin=73), b"packed_bytes"),
             (lambda: call(nin=0), b"packed_bytes"), (lambda: call(fmt=yuv10, nin=36), b"packed_bytes"), (lambda: call(fmt=F["rgb16"], nin=72), b"packed_bytes"),
             (lambda: call(nout=287), b"out_bytes"), (lambda: call(nout=72), b"out_bytes"), (lambda: call(nout=0), b"out_bytes"),
             (lambda: call(fmt=yuv10, nout=4 * 36), b"out_bytes"),
             (lambda: call(T=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, nin=8, nout=8), b"T * H * W"),
             (lambda: call(T=2 ** 21, H=2 ** 10, W=2 ** 10, nin=8, nout=8), b"T * H * W"),
             (lambda: call(fmt=yuv10, packed=ctypes.c_void_p(base + 1)), b"packed"), (lambda: call(fmt=F["rgb16"], packed=ctypes.c_void_p(base + 3)), b"packed"),
             (lambda: call(out=ctypes.c_void_p(base + 2)), b"out"), (lambda: call(out=ctypes.c_void_p(base + 1)), b"out")]
    for fn, word in cases:
        assert fn() != 0
        msg = L.svr_last_error()
        assert b"svr_unpack_frames" in msg and word in msg, msg


def test_header_ctypes_table_and_build_list_know_the_entry_point():
    hip_lib, fin = sub("hip_lib"), sub("frameio_in")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert "svr_unpack_frames" in declared and "svr_unpack_frames" in hip_lib.SYMBOLS and declared == set(hip_lib.SYMBOLS)
    decl = re.search(r"int svr_unpack_frames\(([^;]*)\);", src).group(1)
    assert len(decl.split(",")) == 12 == len(hip_lib.SYMBOLS["svr_unpack_frames"][1])
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert re.search(r"v9, additive: \+ svr_unpack_frames\(\).*?A new symbol only", src, flags=re.S)
    for name, code in hip_lib.UNPACK_FORMATS.items():
        assert re.search(rf"#define SVR_UNPACK_{name.upper()}\s+{code}\b", src), name
    assert set(hip_lib.UNPACK_FORMATS) == set(fin.FORMATS)
    for name, code in hip_lib.PACK_FORMATS.items():                          # the pack's ids did not move, and the shared formats share them
        assert re.search(rf"#define SVR_PACK_{name.upper()}\s+{code}\b", src) and hip_lib.UNPACK_FORMATS[name] == code
    assert hip_lib.PACK_FORMATS == {"rgb8": 0, "bgr8": 1, "yuv420p10": 2}
    for table, prefix in ((hip_lib.YUV_MATRICES, "SVR_MATRIX_"), (hip_lib.YUV_RANGES, "SVR_RANGE_")):
        for name, code in table.items():
            assert re.search(rf"#define {prefix}{name.upper()}\s+{code}\b", src), name
    assert tuple(hip_lib.YUV_MATRICES) == tuple(fin.MATRICES) and tuple(hip_lib.YUV_RANGES) == fin.RANGES
    assert '#include "svr_frame_unpack.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert os.path.join(hip_lib.CSRC, "svr_frame_unpack.hip") in hip_lib.sources()        # (the loader's source hash covers it)


# ---------------------------------------------------------------------------------------------------------------- reader
def test_probe_reads_the_first_video_stream(cli, tmp_path):
    ffprobe, _ = stand_ins(str(tmp_path / "bin"))
    clip = tmp_path / "clip.mkv"
    fake_video(clip, None, "yuv420p10le", 1920, 1080, rate="30000/1001", audio=True, color_space="bt709", color_range="tv")
    info = cli.probe_video(ffprobe, str(clip))
    assert info == dict(width=1920, height=1080, fps=Fraction(30000, 1001), pix_fmt="yuv420p10le", color_space="bt709", color_range="tv",
                        has_audio=True)
    fake_video(clip, None, "yuv420p", 640, 360)
    info = cli.probe_video(ffprobe, str(clip))
    assert info["fps"] == 24 and info["color_space"] is None and info["color_range"] is None and info["has_audio"] is False
    assert len(calls(str(tmp_path / "bin"))) == 2
    with pytest.raises(RuntimeError, match="ffprobe exited with status"):
        cli.probe_video(ffprobe, str(tmp_path / "missing.mkv"))                # (the stand-in has no answer for it and dies)


def test_routing_follows_the_pix_fmt_table(cli):
    info = lambda pix, h=1080, space=None, rng=None: dict(pix_fmt=pix, height=h, width=16, color_space=space, color_range=rng)
    route = cli.route_input
    # planar 4:2:0 of 8 / 10 bits: the planes as they are
    assert route(info("yuv420p")) == ("yuv420p", "yuv420p8", 3, "bt709", "tv")
    assert route(info("yuv420p", rng="pc")) == ("yuv420p", "yuv420p8", 3, "bt709", "pc")
    assert route(info("yuvj420p")) == ("yuvj420p", "yuv420p8", 3, "bt709", "pc")
    assert route(info("yuvj420p", rng="tv")) == ("yuvj420p", "yuv420p8", 3, "bt709", "pc")
    assert route(info("yuv420p10le")) == ("yuv420p10le", "yuv420p10", 3, "bt709", "tv")
    assert route(info("yuv420p10le", rng="pc")) == ("yuv420p10le", "yuv420p10", 3, "bt709", "pc")
    # the matrix: color_space, else by height
    assert route(info("yuv420p", h=719))[3] == "bt601" and route(info("yuv420p", h=720))[3] == "bt709"
    assert route(info("yuv420p", space="smpte170m"))[3] == "bt601" and route(info("yuv420p", space="bt470bg"))[3] == "bt601"
    assert route(info("yuv420p", h=480, space="bt709"))[3] == "bt709"
    # a matrix the kernel does not have: ffmpeg converts, at full depth
    assert route(info("yuv420p10le", space="bt2020nc"))[:3] == ("rgb48le", "rgb16", 3)
    assert route(info("yuv420p", space="bt2020nc"))[:3] == ("rgb48le", "rgb16", 3)
    # every other format of at most 8 bits: rgb24, rgba with alpha
    for pix in ("yuv422p", "yuv444p", "yuvj444p", "nv12", "bgr24", "gray", "pal8", "gbrp"):
        assert route(info(pix))[:3] == ("rgb24", "rgb8", 3), pix
    for pix in ("rgba", "bgra", "argb", "yuva420p", "yuva444p", "gbrap", "ya8"):
        assert route(info(pix))[:3] == ("rgba", "rgb8", 4), pix
    # everything else, names the table does not know included: rgb48le, rgba64le with alpha
    for pix in ("yuv422p10le", "yuv444p12le", "yuv420p12le", "gbrp10le", "rgb48le", "gray16le", "p010le", "some_future_format", ""):
        assert route(info(pix))[:3] == ("rgb48le", "rgb16", 3), pix
    for pix in ("yuva444p10le", "yuva420p10le", "gbrap12le", "rgba64le", "ya16le"):
        assert route(info(pix))[:3] == ("rgba64le", "rgb16", 4), pix


def source_case(cli, tmp_path, fmt, pix, T=13, H=5, W=7, C=3, chunk=5, skip=0, cap=0, **video_kw):
    _, ffmpeg = stand_ins(str(tmp_path / "bin"))
    clip = tmp_path / f"clip_{fmt}.mkv"
    packed = random_packed(fmt, T, H, W, C, seed=T + H + W) if T else None
    fake_video(clip, packed, pix, W, H, **video_kw)
    info = dict(width=W, height=H, fps=Fraction(24), pix_fmt=pix, color_space=video_kw.get("color_space"),
                color_range=video_kw.get("color_range"), has_audio=False)
    return cli.FrameSource(ffmpeg, str(clip), info, chunk, skip, cap), packed, clip


@pytest.mark.parametrize("fmt,pix,C,kw", [("yuv420p10", "yuv420p10le", 3, {}), ("yuv420p8", "yuv420p", 3, dict(color_range="pc")),
                                          ("yuv420p8", "yuvj420p", 3, dict(color_space="bt709")), ("rgb8", "yuv444p", 3, {}),
                                          ("rgb8", "yuva420p", 4, {}), ("rgb16", "yuv422p10le", 3, {}), ("rgb16", "gbrap12le", 4, {})])
def test_source_chunks_equal_the_specification_applied_to_the_emitted_bytes(cli, tmp_path, fmt, pix, C, kw):
    """13 frames of 5 x 7 (odd: the chroma planes are 3 x 4) in chunks of 5: 5, 5 and a short last chunk of 3."""
    fin = sub("frameio_in")
    src, packed, clip = source_case(cli, tmp_path, fmt, pix, C=C, **kw)
    assert (src.fmt, src.C) == (fmt, C)
    got = list(src.chunks())
    assert [tuple(c.shape) for c in got] == [(5, 5, 7, C), (5, 5, 7, C), (3, 5, 7, C)] and all(c.dtype == torch.float32 for c in got)
    matrix = "bt709" if kw.get("color_space") else "bt601"                   # (height 5, nothing said: bt601)
    range_ = "pc" if (pix == "yuvj420p" or kw.get("color_range") == "pc") else "tv"
    want = fin.unpack_frames_torch(packed, fmt, 13, 5, 7, C, matrix, range_)
    assert torch.equal(torch.cat(got), want)
    argv = open(str(clip) + ".args").read().split("\n")
    raw = {("yuv420p10", 3): "yuv420p10le", ("yuv420p8", 3): pix, ("rgb8", 3): "rgb24", ("rgb8", 4): "rgba", ("rgb16", 3): "rgb48le",
           ("rgb16", 4): "rgba64le"}[(fmt, C)]
    assert argv == ["-loglevel", "error", "-noautorotate", "-i", str(clip), "-map", "0:v:0", "-f", "rawvideo", "-pix_fmt", raw, "-"]
    assert not src.thread.is_alive() and src.proc.returncode == 0
    assert not any(b.is_pinned() for b in src.buffers) and len(src.buffers) == 2       # (host frames: nothing to pin for)


def test_source_skips_caps_and_terminates_the_decoder(cli, tmp_path):
    fin = sub("frameio_in")
    # skip 2, cap 7 of 13: frames 2..8 as 5 + 2; the decoder would go on for ever and is terminated
    src, packed, _ = source_case(cli, tmp_path, "yuv420p10", "yuv420p10le", skip=2, cap=7, endless=True)
    got = list(src.chunks())
    assert [c.shape[0] for c in got] == [5, 2]
    assert torch.equal(torch.cat(got), fin.unpack_frames_torch(packed, "yuv420p10", 13, 5, 7, 3, "bt601", "tv")[2:9])
    assert src.proc.returncode == -signal.SIGTERM and not src.thread.is_alive()
    # a cap beyond the clip, a skip larger than a chunk: what is there, 13 - 6 = 7 frames as 5 + 2
    src, packed, _ = source_case(cli, tmp_path, "rgb8", "rgb24", skip=6, cap=50)
    got = list(src.chunks())
    assert [c.shape[0] for c in got] == [5, 2] and torch.equal(torch.cat(got), fin.unpack_frames_torch(packed, "rgb8", 13, 5, 7, 3)[6:])
    # the caller stops early: the decoder is terminated, the thread ends
    src, _, _ = source_case(cli, tmp_path, "rgb16", "rgb48le", endless=True)
    stream = src.chunks()
    assert next(stream).shape[0] == 5
    stream.close()
    assert not src.thread.is_alive() and src.proc.returncode is not None


def test_source_reports_an_empty_stream_a_short_frame_and_a_failing_decoder(cli, tmp_path):
    src, _, _ = source_case(cli, tmp_path, "yuv420p8", "yuv420p", T=0)
    with pytest.raises(ValueError, match="No frames to process"):
        list(src.chunks())
    src, _, _ = source_case(cli, tmp_path, "yuv420p8", "yuv420p", T=3, skip=3)            # everything skipped
    with pytest.raises(ValueError, match="No frames to process"):
        list(src.chunks())
    src, _, _ = source_case(cli, tmp_path, "rgb8", "rgb24", fail="clip.mkv: moov atom not found\n")
    with pytest.raises(RuntimeError, match="ffmpeg exited with status 3.*moov atom not found"):
        list(src.chunks())
    assert not src.thread.is_alive()
    src, _, clip = source_case(cli, tmp_path, "rgb16", "rgb48le", T=2)
    with open(str(clip) + ".raw", "ab") as f:
        f.write(b"\0" * 10)
    with pytest.raises(RuntimeError, match="ended inside a frame"):
        list(src.chunks())
    with pytest.raises(ValueError, match="chunk_size"):
        cli.FrameSource("ffmpeg", "x.mkv", dict(width=2, height=2, fps=Fraction(24), pix_fmt="yuv420p"), 0)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_reads_a_video_through_ffmpeg_in_chunks(cli, rig, tmp_path, monkeypatch):
    """13 yuv420p frames of 8 x 10 in chunks of 5 through the tiny runner into png files: the files are the packed stream of the
    specification's frames."""
    from PIL import Image
    fin, frameio, pipeline = sub("frameio_in"), sub("frameio"), sub("pipeline")
    runner, text, _ = rig
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    packed = random_packed("yuv420p8", 13, 8, 10, 3, seed=3)
    fake_video(tmp_path / "clip.mp4", packed, "yuv420p", 10, 8, color_space="bt709", color_range="tv")
    assert cli.main([str(tmp_path / "clip.mp4"), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "out")] + ARGS) == 0
    frames = fin.unpack_frames_torch(packed, "yuv420p8", 13, 8, 10, 3, "bt709", "tv")
    want = torch.cat([frameio.pack_frames_torch(o, "rgb8") for o in
                      pipeline.upscale_stream(iter(split(frames, 5)), runner, text, temporal_overlap=2, prepend_frames=1, **KW)]).numpy()
    assert sorted(os.listdir(tmp_path / "out")) == [f"frame_{i:06d}.png" for i in range(13)]
    for i in range(13):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"frame_{i:06d}.png")), want[i]), i
    log = calls(bin_)
    assert len(log) == 2 and log[0].startswith("ffprobe ") and log[1].startswith("ffmpeg ")          # one probe, one decoder


@pytest.fixture()
def identity(cli, monkeypatch):
    """the engines' work replaced by the identity: what reaches the writer is what the reader produced"""
    monkeypatch.setattr(cli, "run", lambda args, frames, eng=None, **kw: (frames, 0))
    monkeypatch.setattr(cli, "run_stream", lambda args, chunks, eng=None: chunks)
    return cli


TODAY = ["-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "bgr24", "-s", "10x8", "-r", "30", "-i", "-", "-vf",
         "scale=out_color_matrix=bt709:out_range=tv", "-c:v", "libx264", "-pix_fmt", "yuv420p", "-preset", "medium", "-crf", "12",
         "-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv"]


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_writer_copies_the_audio_of_a_video_source_and_only_of_one(identity, tmp_path, monkeypatch, chunked):
    cli, fin, frameio = identity, sub("frameio_in"), sub("frameio")
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    packed = random_packed("yuv420p10", 40, 8, 10, 3, seed=4)
    clip, out = tmp_path / "clip.mkv", tmp_path / "out.mp4"
    fake_video(clip, packed, "yuv420p10le", 10, 8, rate="30000/1001", audio=True, color_space="bt709")
    tail = ["--chunk_size", "16"] if chunked else []
    assert cli.main([str(clip), "--video_backend", "ffmpeg", "--output", str(out), "--skip_first_frames", "3", "--load_cap", "35"] + tail) == 0
    frames = fin.unpack_frames_torch(packed, "yuv420p10", 40, 8, 10, 3, "bt709", "tv")[3:38]
    assert out.read_bytes() == frameio.pack_frames_torch(frames, "bgr8").numpy().tobytes()
    argv = open(str(out) + ".args").read().split("\n")
    i = argv.index("-i")
    assert argv[i:i + 6] == ["-i", "-", "-ss", f"{3 * 1001 / 30000:.6f}", "-i", str(clip)]
    assert argv[argv.index("-r") + 1] == "30000/1001"
    assert argv[i + 8:i + 15] == ["-map", "0:v:0", "-map", "1:a?", "-c:a", "copy", "-shortest"] and argv[-1] == str(out)
    # without the four additions it is today's command
    rest = argv[:i + 2] + argv[i + 6:i + 8] + argv[i + 15:]
    assert rest == TODAY[:10] + ["30000/1001"] + TODAY[11:] + [str(out)]
    # the same source without an audio stream, and a .npy source: today's command, argument for argument
    fake_video(clip, packed, "yuv420p10le", 10, 8, rate="30/1", color_space="bt709")
    assert cli.main([str(clip), "--video_backend", "ffmpeg", "--output", str(out)] + tail) == 0
    assert open(str(out) + ".args").read().split("\n") == TODAY + [str(out)]
    np.save(tmp_path / "clip.npy", frames[:4].numpy())
    assert cli.main([str(tmp_path / "clip.npy"), "--video_backend", "ffmpeg", "--output_format", "mp4", "--output", str(out)] + tail) == 0
    assert open(str(out) + ".args").read().split("\n") == TODAY + [str(out)]
    # a video source with audio whose output is not the ffmpeg writer's: nothing to copy it into
    fake_video(clip, packed[:4].contiguous(), "yuv420p10le", 10, 8, audio=True)
    assert cli.main([str(clip), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "png")] + tail) == 0
    assert len(os.listdir(tmp_path / "png")) == 4


def test_cli_looks_for_ffprobe_and_ffmpeg_before_the_engines(cli, tmp_path, monkeypatch):
    clip = tmp_path / "clip.mp4"
    fake_video(clip, random_packed("yuv420p8", 2, 8, 10, 3, seed=5), "yuv420p", 10, 8)
    os.makedirs(tmp_path / "empty")
    monkeypatch.setenv("PATH", str(tmp_path / "empty"))
    with pytest.raises(RuntimeError, match="ffmpeg executable"):
        cli.main([str(clip), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "o")])
    assert cli.calls == []
    # ffmpeg alone is not enough to READ a video
    _, ffmpeg = stand_ins(str(tmp_path / "bin"))
    os.symlink(ffmpeg, tmp_path / "empty" / "ffmpeg")
    with pytest.raises(RuntimeError, match="ffprobe executable"):
        cli.main([str(clip), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "o")])
    assert cli.calls == [] and calls(str(tmp_path / "bin")) == []
    # a file ffprobe refuses is reported before the engines too
    monkeypatch.setenv("PATH", str(tmp_path / "bin"))
    os.remove(str(clip) + ".json")
    with pytest.raises(RuntimeError, match="ffprobe exited"):
        cli.main([str(clip), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / "o")])
    assert cli.calls == []


def test_opencv_backend_never_starts_either_executable(identity, tmp_path, monkeypatch):
    """--video_backend opencv (the default): a video goes to cv2.VideoCapture as before -- which is missing here or finds no frame in
    the stand-in file --, a tensor input keeps its reader under either backend; ffprobe and ffmpeg are on PATH and never run."""
    cli = identity
    bin_ = str(tmp_path / "bin")
    stand_ins(bin_)
    monkeypatch.setenv("PATH", bin_ + os.pathsep + os.environ.get("PATH", ""))
    clip = tmp_path / "clip.mp4"
    fake_video(clip, random_packed("yuv420p8", 2, 8, 10, 3, seed=6), "yuv420p", 10, 8, audio=True)
    for tail in ([], ["--chunk_size", "5"], ["--video_backend", "opencv"]):
        with pytest.raises((RuntimeError, ValueError)) as e:
            cli.main([str(clip), "--output_format", "png", "--output", str(tmp_path / "o")] + tail)
        assert "ffmpeg" not in str(e.value) and "ffprobe" not in str(e.value)
    x = torch.rand(3, 8, 10, 3)
    np.save(tmp_path / "clip.npy", x.numpy())
    for n, tail in enumerate(([], ["--chunk_size", "2"])):
        assert cli.main([str(tmp_path / "clip.npy"), "--video_backend", "ffmpeg", "--output_format", "png", "--output", str(tmp_path / f"p{n}")] + tail) == 0
        assert len(os.listdir(tmp_path / f"p{n}")) == 3
    assert calls(bin_) == []
