"""planar.py without a GPU: the torch statement against an independent per-pixel statement, its anchor to frameio_in's yuv420p
formats, check values, the siting rows, its refusals; the C entry point's declaration and refusal messages; inference_cli's
route_planar table, the shipped switch, and FrameSource on the planar route against stand-ins for the two executables."""
import os
import re
from fractions import Fraction

import pytest
import torch

from conftest import ROOT, sub
from planar_cases import (BITS, DUP, MATRICES, MI, RANGES, SMALL, SOURCE_H, SOURCE_T, SOURCE_W, SUBS, THR, chain_of_the_whole, coefficients,
                          load_cli, pixel_statement, planar_source, random_planes, shape_id, sitings, source_planes)
from test_refusal_messages import Ptr, call


@pytest.fixture(scope="module")
def cli():
    return load_cli()


def flat_planes(sub_, bits, T, H, W, y, cb, cr):
    planar = sub("planar")
    hc, wc = planar.chroma_dims(sub_, H, W)
    one = torch.cat([torch.full((H * W,), y), torch.full((hc * wc,), cb), torch.full((hc * wc,), cr)])
    return one.repeat(T, 1).to(torch.int32).to(planar.planar_dtype(bits))


# ---------------------------------------------------------------------------------------------------------------- the statement
def test_module_surface_matrices_and_the_integer_bound():
    planar, fin = sub("planar"), sub("frameio_in")
    assert planar.ENABLED is False                                             # ships off
    assert planar.MATRICES["bt2020"] == (96639, 10784, 37444, 123299)
    assert {m: planar.MATRICES[m] for m in fin.MATRICES} == fin.MATRICES       # the rule reproduces the two existing rows
    assert all(planar.MATRICES[m] == coefficients(m) for m in MATRICES)
    assert set(fin.MATRICES) == {"bt709", "bt601"}                             # ... which nobody edited
    for bits in (8, 10):
        for r in RANGES:
            assert planar.yuv_constants(bits, r) == fin.yuv_constants(bits, r)
    assert planar.yuv_constants(12, "tv") == (256, 3504, 3584, 16384) and planar.yuv_constants(12, "pc") == (0, 4095, 4095, 16384)
    for bits in BITS:
        for m in MATRICES:
            rv, gu, gv, bu = planar.MATRICES[m]
            span = 8 << (bits - 1)                                             # |u|, |v| after the sample clamp
            assert bu * span < 2 ** 31 and (gu + gv) * span < 2 ** 31 and rv * span < 2 ** 31
            for r in RANGES:
                assert planar.numerator_bound(bits, m, r) < 2 ** 61
    assert planar.planar_shape(2, 5, 7, "420") == (2, 35 + 2 * 3 * 4) and planar.planar_shape(2, 5, 7, "422") == (2, 35 + 2 * 5 * 4)
    assert planar.planar_shape(2, 5, 7, "444") == (2, 105)
    assert planar.frame_bytes(5, 7, "422", 8) == 75 and planar.frame_bytes(5, 7, "422", 12) == 150
    assert planar.planar_dtype(8) == torch.uint8 and planar.planar_dtype(10) == planar.planar_dtype(12) == torch.uint16


@pytest.mark.parametrize("sub_", SUBS)
@pytest.mark.parametrize("shape", SMALL, ids=shape_id)
def test_torch_equals_the_per_pixel_statement(shape, sub_):
    planar = sub("planar")
    T, H, W = shape
    for bits in BITS:
        for k, (matrix, range_, siting) in enumerate((m, r, s) for m in MATRICES for r in RANGES for s in sitings(sub_)):
            planes = random_planes(sub_, bits, T, H, W, seed=sum(shape) + bits + k, whole_container=(k == 0))
            got = planar.planar_codes_torch(planes, sub_, bits, T, H, W, matrix, range_, siting)
            assert got.dtype == torch.uint16 and tuple(got.shape) == (T, H, W, 3) and got.is_contiguous()
            assert got.to(torch.int64).tolist() == pixel_statement(planes, sub_, bits, T, H, W, matrix, range_, siting), (bits, matrix, range_, siting)


@pytest.mark.parametrize("bits,fmt", [(8, "yuv420p8"), (10, "yuv420p10")])
def test_anchor_to_the_existing_specification(bits, fmt):
    """420 / left IS frameio_in's yuv420p format: codes, then the rgb16 unpack, equal its unpack of the planes, bit for bit."""
    planar, fin = sub("planar"), sub("frameio_in")
    for T, H, W in [(2, 3, 5), (1, 4, 32), (3, 17, 33)]:
        for k, (matrix, range_) in enumerate((m, r) for m in ("bt709", "bt601") for r in RANGES):
            planes = random_planes("420", bits, T, H, W, seed=k, whole_container=(k == 1))
            codes = planar.planar_codes_torch(planes, "420", bits, T, H, W, matrix, range_, "left")
            assert torch.equal(fin.unpack_frames_torch(codes, "rgb16", T, H, W, 3), fin.unpack_frames_torch(planes, fmt, T, H, W, 3, matrix, range_))


def test_check_values_white_black_and_the_bt2020_primaries():
    planar, frameio = sub("planar"), sub("frameio")
    T, H, W = 1, 4, 6
    for sub_ in SUBS:
        for bits in BITS:
            sh = bits - 8
            for matrix in MATRICES:
                for siting in sitings(sub_):
                    run = lambda y, c, r: planar.planar_codes_torch(flat_planes(sub_, bits, T, H, W, y, c, c), sub_, bits, T, H, W, matrix, r, siting)
                    assert bool((run(235 << sh, 128 << sh, "tv") == 65535).all()) and bool((run(16 << sh, 128 << sh, "tv") == 0).all())
                    assert bool((run((1 << bits) - 1, 1 << (bits - 1), "pc") == 65535).all()) and bool((run(0, 1 << (bits - 1), "pc") == 0).all())
    # The primaries as the pack emits them (10 bits, tv, bt2020).  The bound is DERIVED: the pack rounds Y, Cb and Cr to the nearest
    # 10-bit code, so each is off by at most half a step; through R = (Y - y0) / ys + rv (Cr - 512) / cs (and alike for G, B) that
    # is 65535 * (0.5 / 876 + k * 0.5 / 896) codes with k = rv, gu + gv, bu over 2^16, plus half a code for this side's own rounding,
    # plus 2 codes for the coefficients both sides round at 2^16 (eleven of them, each off by at most 2^-17 of full scale: under
    # a fifth of a code apiece).  A clamp to 0..65535 only moves a value towards the true one, which lies inside.
    rv, gu, gv, bu = planar.MATRICES["bt2020"]
    bound = [65535 * (Fraction(1, 2 * 876) + Fraction(k, 65536) * Fraction(1, 2 * 896)) + Fraction(1, 2) + 2 for k in (rv, gu + gv, bu)]
    assert all(50 < b < 128 for b in bound)                                    # (about 93.8, 66.8 and 108.7 codes of 65535: a 10-bit step is 64)
    for colour in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
        frames = torch.tensor(colour, dtype=torch.float32).expand(1, 4, 6, 3).contiguous()
        planes = frameio.pack_yuv420p10_torch(frames, "bt2020", "tv", "left")
        codes = planar.planar_codes_torch(planes, "420", 10, 1, 4, 6, "bt2020", "tv", "left").to(torch.int64)
        for ch in range(3):
            err = (codes[..., ch] - int(colour[ch] * 65535)).abs().max().item()
            assert err <= bound[ch], (colour, ch, err)


def test_flat_chroma_knows_no_siting_and_a_vertical_step_tells_left_from_topleft():
    planar = sub("planar")
    T, H, W = 1, 8, 6
    g = torch.Generator().manual_seed(0)
    luma = torch.randint(64, 941, (H * W,), generator=g)
    results = []
    for sub_ in SUBS:
        hc, wc = planar.chroma_dims(sub_, H, W)
        planes = torch.cat([luma, torch.full((hc * wc,), 400), torch.full((hc * wc,), 600)]).reshape(1, -1).to(torch.int32).to(torch.uint16)
        for siting in sitings(sub_):
            results.append(planar.planar_codes_torch(planes, sub_, 10, T, H, W, "bt2020", "tv", siting))
    assert len(results) == 4 and all(torch.equal(results[0], r) for r in results[1:])
    # chroma rows 0, 1 hold 400 and rows 2, 3 hold 600.  "left": luma row 3 takes 3 C[1] + C[2] and row 4 takes C[1] + 3 C[2];
    # "topleft": row 3 takes 2 C[1] + 2 C[2] and row 4 takes 4 C[2].  Every other row sees one value under both sitings.
    cb = torch.tensor([400, 400, 600, 600]).repeat_interleave(3)
    planes = torch.cat([torch.full((H * W,), 502), cb, torch.full((12,), 512)]).reshape(1, -1).to(torch.int32).to(torch.uint16)
    left = planar.planar_codes_torch(planes, "420", 10, T, H, W, "bt709", "tv", "left")
    topleft = planar.planar_codes_torch(planes, "420", 10, T, H, W, "bt709", "tv", "topleft")
    differing = sorted(set((left != topleft).nonzero()[:, 1].tolist()))
    assert differing == [3, 4]
    blue = lambda codes: codes[0, :, 0, 2].to(torch.int64)
    assert bool((blue(left)[3] < blue(topleft)[3]).item()) and bool((blue(left)[4] < blue(topleft)[4]).item())     # (3a + b < 2a + 2b; a + 3b < 4b)


def test_arguments_are_refused_by_name():
    planar = sub("planar")
    p8, p10 = random_planes("422", 8, 2, 4, 6, 0), random_planes("422", 10, 2, 4, 6, 0)
    ok = lambda **kw: planar.check_arguments(**{**dict(planes=p10, sub="422", bits=10, T=2, H=4, W=6, matrix="bt709", range_="tv", siting="left"), **kw})
    assert ok() == (2, 48)
    for kw, message in ((dict(sub="411"), r"sub must be one of \('420', '422', '444'\), got '411'"),
                        (dict(bits=16), r"bits must be one of \(8, 10, 12\), got 16"),
                        (dict(matrix="bt2020c"), r"matrix must be one of \('bt709', 'bt601', 'bt2020'\), got 'bt2020c'"),
                        (dict(range_="full"), r"range_ must be one of \('tv', 'pc'\), got 'full'"),
                        (dict(siting="center"), r"siting must be one of \('left',\) for sub '422', got 'center'"),
                        (dict(siting="topleft"), r"siting must be one of \('left',\) for sub '422', got 'topleft'"),
                        (dict(sub="444", siting="topleft", planes=torch.zeros(144, dtype=torch.uint16)), r"siting must be one of \('left',\) for sub '444'"),
                        (dict(sub="420", siting="top", planes=torch.zeros(72, dtype=torch.uint16)), r"siting must be one of \('left', 'topleft'\) for sub '420', got 'top'"),
                        (dict(T=0), "T, H, W must be positive"), (dict(H=-1), "T, H, W must be positive"), (dict(W=0), "T, H, W must be positive"),
                        (dict(planes=p8), "planes must be torch.uint16 for 10 bits, got torch.uint8"),
                        (dict(planes=p10, bits=8), "planes must be torch.uint8 for 8 bits, got torch.uint16"),
                        (dict(W=7), r"planes must hold 120 samples \(\(2, 60\)\) for sub '422' at T, H, W = 2, 4, 7, got \(2, 48\)")):
        with pytest.raises(ValueError, match=message):
            ok(**kw)
    with pytest.raises(ValueError, match="bits must be one of"):
        planar.frame_bytes(4, 6, "422", 9)
    with pytest.raises(ValueError, match="sub must be one of"):
        planar.frame_bytes(4, 6, "440", 8)
    # the front: without ops the statement; ``out`` is checked and filled
    out = torch.zeros((2, 4, 6, 3), dtype=torch.uint16)
    want = planar.planar_codes_torch(p10, "422", 10, 2, 4, 6)
    assert planar.planar_codes(p10, "422", 10, 2, 4, 6, out=out) is out and torch.equal(out, want)
    assert torch.equal(planar.planar_codes(p10, "422", 10, 2, 4, 6, ops=object()), want)
    with pytest.raises(ValueError, match="out must be torch.uint16"):
        planar.planar_codes(p10, "422", 10, 2, 4, 6, out=torch.zeros((2, 4, 6, 3), dtype=torch.int16))

    class Failing:
        def planar_codes(self, *a, **k):
            raise RuntimeError("the library failed")
    with pytest.raises(RuntimeError, match="the library failed"):             # no fall-back from a backend that has the method
        planar.planar_codes(p10, "422", 10, 2, 4, 6, ops=Failing())


# ---------------------------------------------------------------------------------------------------------------- C ABI
p, q = Ptr(0), Ptr(1 << 16)
MATRIX = "matrix must be SVR_COLOUR_MATRIX_BT709, SVR_COLOUR_MATRIX_BT601 or SVR_COLOUR_MATRIX_BT2020"
# (planes, planes_bytes, sub, bits, T, H, W, matrix, range, siting, out, out_bytes, stream); a 2 x 4 x 6 clip: 422 has 96 samples
ROWS = [
    ((None, 96, 1, 8, 2, 4, 6, 0, 0, 1, q, 288, None), "planes is a null pointer"),
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 1, None, 288, None), "out is a null pointer"),
    ((p, 96, 1, 8, 0, 4, 6, 0, 0, 1, q, 288, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 96, 1, 8, 2, -4, 6, 0, 0, 1, q, 288, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 96, 1, 8, 2, 4, 0, 0, 0, 1, q, 288, None), "need T >= 1, H >= 1, W >= 1"),
    ((p, 96, 1, 8, 2, 1 << 20, 1 << 20, 0, 0, 1, q, 288, None), "T * H * W must not exceed 2^40 pixels"),
    ((p, 96, 3, 8, 2, 4, 6, 0, 0, 1, q, 288, None), "sub must be SVR_PLANAR_420, SVR_PLANAR_422 or SVR_PLANAR_444"),
    ((p, 96, -1, 8, 2, 4, 6, 0, 0, 1, q, 288, None), "sub must be SVR_PLANAR_420, SVR_PLANAR_422 or SVR_PLANAR_444"),
    ((p, 96, 1, 9, 2, 4, 6, 0, 0, 1, q, 288, None), "bits must be 8, 10 or 12"),
    ((p, 96, 1, 16, 2, 4, 6, 0, 0, 1, q, 288, None), "bits must be 8, 10 or 12"),
    ((p, 96, 1, 8, 2, 4, 6, 3, 0, 1, q, 288, None), MATRIX),
    ((p, 96, 1, 8, 2, 4, 6, -1, 0, 1, q, 288, None), MATRIX),
    ((p, 96, 1, 8, 2, 4, 6, 0, 2, 1, q, 288, None), "range must be SVR_COLOUR_RANGE_TV or SVR_COLOUR_RANGE_PC"),
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 0, q, 288, None), "siting must be SVR_PLANAR_SITING_LEFT or SVR_PLANAR_SITING_TOPLEFT"),
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 3, q, 288, None), "siting must be SVR_PLANAR_SITING_LEFT or SVR_PLANAR_SITING_TOPLEFT"),
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 2, q, 288, None), "siting SVR_PLANAR_SITING_TOPLEFT is for SVR_PLANAR_420 only"),
    ((p, 144, 2, 8, 2, 4, 6, 0, 0, 2, q, 288, None), "siting SVR_PLANAR_SITING_TOPLEFT is for SVR_PLANAR_420 only"),
    ((p + 1, 192, 1, 10, 2, 4, 6, 0, 0, 1, q, 288, None), "planes is not aligned to 2 bytes"),
    ((p + 1, 192, 1, 12, 2, 4, 6, 0, 0, 1, q, 288, None), "planes is not aligned to 2 bytes"),
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 1, q + 1, 288, None), "out is not aligned to 2 bytes"),
    ((p, 95, 1, 8, 2, 4, 6, 0, 0, 1, q, 288, None), "planes_bytes is 95, the format needs exactly 96"),
    ((p, 96, 0, 8, 2, 4, 6, 0, 0, 1, q, 288, None), "planes_bytes is 96, the format needs exactly 72"),
    ((p, 96, 2, 8, 2, 4, 6, 0, 0, 1, q, 288, None), "planes_bytes is 96, the format needs exactly 144"),
    ((p, 96, 1, 10, 2, 4, 6, 0, 0, 1, q, 288, None), "planes_bytes is 96, the format needs exactly 192"),
    ((p, 55, 0, 8, 2, 3, 5, 0, 0, 2, q, 180, None), "planes_bytes is 55, the format needs exactly 54"),      # odd sizes: 2 * (15 + 2 * 2 * 3)
    ((p, 90, 1, 8, 2, 3, 5, 0, 0, 1, q, 180, None), "planes_bytes is 90, the format needs exactly 66"),      # 2 * (15 + 2 * 3 * 3)
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 1, q, 287, None), "out_bytes is 287, uint16 [T, H, W, 3] needs exactly 288"),
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 1, q, 144, None), "out_bytes is 144, uint16 [T, H, W, 3] needs exactly 288"),
    ((p, 96, 1, 8, 2, 4, 6, 0, 0, 1, p + 94, 288, None), "out overlaps planes"),
    ((p + 286, 96, 1, 8, 2, 4, 6, 0, 0, 1, p, 288, None), "out overlaps planes"),
    # two faults: which one is reported
    ((None, 95, 7, 9, 0, 4, 6, 0, 0, 1, None, 288, None), "planes is a null pointer"),
    ((p, 95, 7, 9, 2, 4, 6, 9, 0, 1, q, 288, None), "sub must be SVR_PLANAR_420, SVR_PLANAR_422 or SVR_PLANAR_444"),
    ((p, 95, 1, 8, 2, 4, 6, 0, 0, 1, q + 1, 288, None), "out is not aligned to 2 bytes"),
    ((p, 95, 1, 8, 2, 4, 6, 0, 0, 1, p, 287, None), "planes_bytes is 95, the format needs exactly 96"),
]


def test_every_refusal_message_of_the_entry_point_is_exact():
    """Every argument is validated on the host before the launch, so a host buffer stands in for device memory."""
    L = sub("hip_lib").lib()
    for args, message in ROWS:
        assert L.svr_set_option(b"no_such_key", 0) != 0          # (a known message first: an accepted call would leave it standing)
        assert call(L, "svr_planar_codes", args) == -1, args
        assert L.svr_last_error().decode() == f"svr_planar_codes: {message}", args


def test_header_ctypes_table_and_build_list_know_the_entry_point():
    hip_lib = sub("hip_lib")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert "svr_planar_codes" in declared and declared == set(hip_lib.SYMBOLS)
    decl = re.search(r"int svr_planar_codes\(([^;]*)\);", src).group(1)
    assert len(decl.split(",")) == 13 == len(hip_lib.SYMBOLS["svr_planar_codes"][1])
    assert re.search(r"^ \*   svr_planar_codes\s+\S", src, flags=re.M)                       # the operand-layout table
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    assert re.search(r"v9, additive: \+ svr_planar_codes\(\).*?A new symbol only", src, flags=re.S)
    for name, table in (("SVR_PLANAR_", hip_lib.PLANAR_SUBS), ("SVR_PLANAR_SITING_", hip_lib.PLANAR_SITINGS)):
        for key, value in table.items():
            assert re.search(rf"#define {name}{key.upper()}\s+{value}\b", src), (name, key)
    assert hip_lib.COLOUR_MATRICES["bt2020"] == 2 and re.search(r"#define SVR_COLOUR_MATRIX_BT2020 2\b", src)
    api = open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert api.index('#include "svr_frame_unpack.hip"') < api.index('#include "svr_planar.hip"')
    assert os.path.join(hip_lib.CSRC, "svr_planar.hip") in hip_lib.sources()                 # (the loader's source hash covers it)
    lib = hip_lib.lib()
    assert lib.svr_abi_version() == 9 and hasattr(lib, "svr_planar_codes")
    assert hasattr(sub("ops").HipOps, "planar_codes")
    from ops_reference import TorchOps
    assert not hasattr(TorchOps, "planar_codes")                                             # as with the stages after it


# ---------------------------------------------------------------------------------------------------------------- routing
def info_of(pix, height=1080, **kw):
    return dict(width=16, height=height, fps=Fraction(25), pix_fmt=pix, color_space=kw.get("color_space"), color_range=kw.get("color_range"),
                has_audio=False)


def test_route_planar_follows_its_table(cli, monkeypatch):
    planar = sub("planar")
    assert cli.route_planar(info_of("yuv422p10le")) is None                    # the switch is off
    monkeypatch.setattr(planar, "ENABLED", True)
    always = {"yuv422p": ("422", 8, "tv"), "yuvj422p": ("422", 8, "pc"), "yuv444p": ("444", 8, "tv"), "yuvj444p": ("444", 8, "pc"),
              "yuv422p10le": ("422", 10, "tv"), "yuv444p10le": ("444", 10, "tv"), "yuv420p12le": ("420", 12, "tv"),
              "yuv422p12le": ("422", 12, "tv"), "yuv444p12le": ("444", 12, "tv")}
    for pix, (sub_, bits, range_) in always.items():
        assert cli.route_planar(info_of(pix), None, None) == (pix, sub_, bits, "bt709", range_, "left"), pix
        assert cli.route_planar(info_of(pix, color_space="bt2020nc"), {}, None) == (pix, sub_, bits, "bt2020", range_, "left"), pix
    # route_input's own two: only with a BT.2020 matrix or top-left chroma
    for pix, bits in (("yuv420p", 8), ("yuv420p10le", 10)):
        assert cli.route_planar(info_of(pix, color_space="bt709"), dict(chroma_location="left"), None) is None
        assert cli.route_planar(info_of(pix), None, None) is None
        assert cli.route_planar(info_of(pix, color_space="bt2020nc"), dict(chroma_location="left"), None) == (pix, "420", bits, "bt2020", "tv", "left")
        assert cli.route_planar(info_of(pix, color_space="bt2020nc"), dict(chroma_location="topleft"), None) == (pix, "420", bits, "bt2020", "tv", "topleft")
        assert cli.route_planar(info_of(pix, color_space="smpte170m"), dict(chroma_location="topleft"), None) == (pix, "420", bits, "bt601", "tv", "topleft")
    assert cli.route_planar(info_of("yuvj420p", color_space="bt2020nc"), dict(chroma_location="topleft"), None) is None      # not in the list
    # not routed: alpha, bt2020c, a matrix outside the table, names outside the list, interlaced 4:2:0
    for pix in ("yuva422p", "yuva444p10le", "yuva420p", "gbrap", "rgba", "nv12", "p010le", "yuv411p", "yuv410p", "yuv440p", "yuv422p16le", "gbrp", "", None):
        assert cli.route_planar(info_of(pix, color_space="bt709"), None, None) is None, pix
    for space in ("bt2020c", "smpte240m", "ycgco", "fcc", "gbr"):
        assert cli.route_planar(info_of("yuv422p10le", color_space=space), None, None) is None, space
    for fields in (("tff", "frame"), ("bff", "match"), ("tff", "decimate")):
        assert cli.route_planar(info_of("yuv420p12le"), None, fields) is None
        assert cli.route_planar(info_of("yuv420p10le", color_space="bt2020nc"), dict(chroma_location="topleft"), fields) is None
        assert cli.route_planar(info_of("yuv422p10le"), None, fields) == ("yuv422p10le", "422", 10, "bt709", "tv", "left")
        assert cli.route_planar(info_of("yuv444p"), None, fields) == ("yuv444p", "444", 8, "bt709", "tv", "left")
    # the matrix: MATRIX_OF plus bt2020nc; an absent tag: route_input's height rule.  The range: color_range; yuvj* is pc.  The siting
    assert cli.route_planar(info_of("yuv422p", color_space="smpte170m"))[3] == "bt601" and cli.route_planar(info_of("yuv422p", color_space="bt470bg"))[3] == "bt601"
    assert cli.route_planar(info_of("yuv422p", height=576))[3] == "bt601" and cli.route_planar(info_of("yuv422p", height=720))[3] == "bt709"
    assert cli.route_planar(info_of("yuv422p", color_range="pc"))[4] == "pc" and cli.route_planar(info_of("yuv422p", color_range="jpeg"))[4] == "pc"
    assert cli.route_planar(info_of("yuv422p", color_range="tv"))[4] == "tv" and cli.route_planar(info_of("yuvj444p", color_range="tv"))[4] == "pc"
    assert cli.route_planar(info_of("yuv420p12le"), dict(chroma_location="topleft"))[5] == "topleft"
    assert cli.route_planar(info_of("yuv420p12le"), dict(chroma_location="center"))[5] == "left"
    assert cli.route_planar(info_of("yuv422p10le"), dict(chroma_location="topleft"))[5] == "left"                              # (nothing to site vertically)
    # the depth of what is written
    assert cli.output_depth("a.mkv", info_of("yuv422p")) == 8 and cli.output_depth("a.mkv", info_of("yuv422p10le")) == 16
    assert cli.output_depth("a.mkv", info_of("yuv444p12le"), None, ("tff", "match")) == 16
    assert cli.output_depth("a.mkv", info_of("yuv420p", color_space="bt2020nc"), {}, None) == 8
    monkeypatch.setattr(planar, "ENABLED", False)
    assert cli.output_depth("a.mkv", info_of("yuv422p")) == 8 and cli.output_depth("a.mkv", info_of("yuv422p10le")) == 16      # route_input's


def test_with_the_switch_off_the_source_is_route_inputs(cli, tmp_path):
    assert sub("planar").ENABLED is False
    planes = source_planes("422", 10)
    src, args = planar_source(cli, tmp_path, planes, "yuv422p10le", 5)
    try:
        info = info_of("yuv422p10le", color_space="bt709", color_range="tv")
        assert (src.raw, src.fmt, src.C, src.matrix, src.range_) == cli.route_input(info) == ("rgb48le", "rgb16", 3, "bt709", "tv")
        assert src.planar is None and src.frame_bytes == SOURCE_H * SOURCE_W * 6
        assert src.command("ffmpeg", "x.mkv") == ["ffmpeg", "-loglevel", "error", "-noautorotate", "-i", "x.mkv", "-map", "0:v:0", "-f", "rawvideo",
                                                 "-pix_fmt", "rgb48le", "-"]
    finally:
        src.close()


SOURCES = [("yuv422p10le", "422", 10, None, dict()),
           ("yuv422p10le", "422", 10, ("tff", "frame"), dict()),
           ("yuv422p10le", "422", 10, ("tff", "decimate"), dict()),
           ("yuv420p10le", "420", 10, None, dict(color_space="bt2020nc", chroma_location="topleft"))]


@pytest.mark.parametrize("pix,sub_,bits,fields,tags", SOURCES, ids=lambda v: "-".join(v) if isinstance(v, tuple) else None)
def test_source_chunks_equal_the_chain_applied_to_the_codes_of_the_whole_clip(cli, tmp_path, monkeypatch, pix, sub_, bits, fields, tags):
    planar = sub("planar")
    monkeypatch.setattr(planar, "ENABLED", True)
    planes = source_planes(sub_, bits)
    matrix = "bt2020" if tags.get("color_space") == "bt2020nc" else "bt709"
    siting = tags.get("chroma_location", "left")
    want = chain_of_the_whole(planes, sub_, bits, matrix, "tv", siting, fields)
    n = SOURCE_T - SOURCE_T // 5 if fields and fields[1] == "decimate" else SOURCE_T
    assert want.shape == (n, SOURCE_H, SOURCE_W, 3) and want.dtype == torch.float32
    for chunk in (1, 4, 5):
        src, args = planar_source(cli, tmp_path, planes, pix, chunk, fields=fields, **tags)
        assert src.planar == (sub_, bits, matrix, "tv", siting) and (src.raw, src.fmt, src.C) == (pix, "rgb16", 3)
        assert src.frame_bytes == planar.frame_bytes(SOURCE_H, SOURCE_W, sub_, bits) and all(b.numel() == chunk * src.frame_bytes for b in src.buffers)
        got = list(src.chunks())
        assert all(c.dtype == torch.float32 and c.shape[1:] == (SOURCE_H, SOURCE_W, 3) for c in got)
        assert torch.equal(torch.cat(got), want), chunk
        asked = open(args).read().split("\n")
        assert asked[asked.index("-pix_fmt") + 1] == pix                       # the decoder was asked for the source's own format
        assert not src.thread.is_alive() and src.proc.returncode == 0
        if fields and fields[1] == "decimate":
            assert src.match == dict(thr=THR, mi=MI) and src.decimate == dict(dup=DUP) and src.decimate_stats is not None
    info = info_of(pix, height=SOURCE_H, color_space=tags.get("color_space", "bt709"))
    assert cli.output_depth("clip.mkv", info, dict(chroma_location=tags.get("chroma_location")), fields) == 16
    assert cli.output_depth("clip.mkv", info_of("yuv422p", height=SOURCE_H), None, fields) == 8
