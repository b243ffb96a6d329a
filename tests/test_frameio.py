"""-m "not gpu": the packed output formats (frameio.py, the specification of csrc/svr_frame_pack.hip): rgb8 / bgr8 against the
expression the command line's writers computed on the host, yuv420p10 against the fp64 BT.709 matrix and its fixed points, the
plane layout for odd sizes, non-finite input, the C ABI's refusals, the dispatch rule (backend or specification, no fall-back)."""
import ctypes
import os
import shutil

import pytest
import torch

from conftest import ROOT, sub

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def host_expression(frames):
    """what inference_cli.save_frames computed before the formats had a module of their own"""
    return (frames.float().clamp(0, 1) * 255.0).round().to(torch.uint8)


def tie_values(scale=255):
    """(k + 0.5) / scale for every k: where round-half-even and round-half-up part"""
    return (torch.arange(scale, dtype=torch.float64) + 0.5).div(scale).float()


def test_rgb8_equals_the_host_expression_on_random_ties_and_out_of_range_input():
    frameio = sub("frameio")
    g = torch.Generator().manual_seed(0)
    ties = tie_values()
    assert ties.numel() % 3 == 0
    for x in (torch.rand(2, 5, 7, 3, generator=g), torch.rand(2, 5, 7, 4, generator=g) * 1.2 - 0.1, ties.reshape(1, 5, 17, 3),
              torch.tensor([-3.0, -0.0, 0.0, 1.0, 1.0 + 1e-6, 7.5]).reshape(1, 1, 2, 3)):
        for src in (x, x.to(torch.bfloat16)):
            got = frameio.pack_frames_torch(src, "rgb8")
            assert got.dtype == torch.uint8 and got.shape == src.shape and got.is_contiguous()
            assert torch.equal(got, host_expression(src))
            bgr = frameio.pack_frames_torch(src, "bgr8")
            order = [2, 1, 0] + ([3] if x.shape[-1] == 4 else [])
            assert torch.equal(bgr, got[..., order])
    # where the fp32 product x * 255 IS k + 0.5 (most k), the code is the even neighbour
    exact = ties * 255.0 == torch.arange(255, dtype=torch.float32) + 0.5
    assert int(exact.sum()) > 100
    codes = frameio.pack_frames_torch(ties.reshape(1, 5, 17, 3), "rgb8").flatten()
    assert bool((codes[exact] % 2 == 0).all())


def test_non_finite_input_is_defined():
    frameio = sub("frameio")
    x = torch.tensor([float("nan"), float("inf"), -float("inf")]).reshape(1, 1, 1, 3)
    assert frameio.pack_frames_torch(x, "rgb8").flatten().tolist() == [0, 255, 0]
    assert frameio.pack_frames_torch(x, "bgr8").flatten().tolist() == [0, 255, 0]
    assert frameio.pack_frames_torch(x.to(torch.bfloat16), "rgb8").flatten().tolist() == [0, 255, 0]
    # q = (0, 65535, 0): pure green
    assert frameio.pack_frames_torch(x, "yuv420p10").flatten().tolist() == [691, 167, 105]
    nan = torch.full((1, 2, 2, 3), float("nan"))
    assert frameio.pack_frames_torch(nan, "yuv420p10").flatten().tolist() == [64] * 4 + [512, 512]


def bt709_fp64(rgb):
    """limited-range 10-bit BT.709 of fp64 R'G'B' in [0, 1], unrounded: (Y, Cb, Cr)"""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = 0.2126 * r + 0.7152 * g + 0.0722 * b
    return 64 + 876 * y, 512 + 896 * (b - y) / 1.8556, 512 + 896 * (r - y) / 1.5748


def test_yuv420p10_fixed_points_and_range():
    frameio = sub("frameio")
    px = lambda *c: torch.tensor(c, dtype=torch.float32).reshape(1, 1, 1, 3)
    want = {(1, 1, 1): (940, 512, 512), (0, 0, 0): (64, 512, 512), (1, 0, 0): (250, 409, 960), (0, 1, 0): (691, 167, 105),
            (0, 0, 1): (127, 960, 471)}
    for c, yuv in want.items():
        assert tuple(frameio.pack_frames_torch(px(*c), "yuv420p10").flatten().tolist()) == yuv, c
        # a 2 x 2 block of the colour: four equal Y, the same chroma
        out = frameio.pack_frames_torch(px(*c).expand(1, 2, 2, 3).contiguous(), "yuv420p10").flatten().tolist()
        assert out == [yuv[0]] * 4 + [yuv[1], yuv[2]], c
    g = torch.Generator().manual_seed(1)
    x = torch.rand(3, 18, 22, 3, generator=g) * 1.2 - 0.1
    x[0, :6] = torch.tensor([0.0, 1.0])[torch.randint(0, 2, (6, 22, 3), generator=g)]            # the cube's corners
    out = frameio.pack_frames_torch(x, "yuv420p10").to(torch.int64)
    Y, C = out[:, :18 * 22], out[:, 18 * 22:]
    assert int(Y.min()) >= 64 and int(Y.max()) <= 940 and int(C.min()) >= 64 and int(C.max()) <= 960


def _luma_case():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 16, 24, 3, generator=g) * 1.1 - 0.05
    x[0, :2] = torch.tensor([0.0, 1.0])[torch.randint(0, 2, (2, 24, 3), generator=g)]              # corners of the cube
    out = sub("frameio").pack_frames_torch(x, "yuv420p10").to(torch.float64)
    q = sub("frameio").codes(x, 65535.0).double() / 65535.0                    # the quantised input the integers start from
    return out, q


def test_yuv420p10_luma_within_0_501_of_the_fp64_bt709_value():
    """|Y - fp64 value| <= 0.501 on 768 random pixels, corners of the cube included.  The fp64 value is the format's own luma row --
    BT.709 as the format defines it, weights 13933 / 46871 / 4732 over 65536, applied to the codes q -- evaluated in fp64 without
    the final rounding: the integer arithmetic may be half a code from it and no more.  This guards the rounding (the + D/2, the
    floor division, the 64-bit products); that the row IS BT.709 is the next test's matter, since the decimal constants
    0.2126 / 0.7152 / 0.0722 lie up to 0.35 / 65536 from the row, i.e. up to 0.0047 of a code, and 0.501 cannot hold against them
    for any implementation of the row."""
    out, q = _luma_case()
    r, g, b = q[..., 0], q[..., 1], q[..., 2]
    own = 64 + 876 * (13933 * r + 46871 * g + 4732 * b) / 65536
    err = (out[:, :16 * 24].reshape(2, 16, 24) - own).abs().max()
    print(f"max |Y - fp64 value of the format's luma row| = {float(err):.6f}")
    assert float(err) <= 0.501


def test_yuv420p10_luma_and_chroma_within_the_derived_bounds():
    """Against Kr = 0.2126, Kb = 0.0722 in fp64 the weight rounding to 2^-16 comes on top of the rounding's half code: at most
    876 * 0.3533 / 65536 = 0.0047 (luma: 13932.95 / 46871.35 / 4731.70 stated as 13933 / 46871 / 4732) and 896 * 0.41 / 65536 =
    0.0056 (chroma rows: -7508.6 / -25259.4 / 32768 and 32768 / -29763.3 / -3004.7 stated as integers), so 0.5048 and 0.5057.
    Chroma is that of the block's MEAN colour."""
    out, q = _luma_case()
    Y = out[:, :16 * 24].reshape(2, 16, 24)
    y64, _, _ = bt709_fp64(q)
    print(f"max |Y - decimal BT.709| = {float((Y - y64).abs().max()):.4f}")
    assert float((Y - y64).abs().max()) <= 0.5048
    mean = q.reshape(2, 8, 2, 12, 2, 3).mean(dim=(2, 4))
    _, cb64, cr64 = bt709_fp64(mean)
    cb = out[:, 16 * 24:16 * 24 + 96].reshape(2, 8, 12)
    cr = out[:, 16 * 24 + 96:].reshape(2, 8, 12)
    print(f"max |Cb - fp64| = {float((cb - cb64).abs().max()):.4f}, max |Cr - fp64| = {float((cr - cr64).abs().max()):.4f}")
    assert float((cb - cb64).abs().max()) <= 0.5057 and float((cr - cr64).abs().max()) <= 0.5057


def test_yuv420p10_planes_for_odd_sizes_repeat_the_last_row_and_column():
    frameio = sub("frameio")
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 5, 7, 3, generator=g)
    out = frameio.pack_frames_torch(x, "yuv420p10")
    assert out.dtype == torch.uint16 and tuple(out.shape) == (2, 5 * 7 + 2 * 3 * 4) and out.is_contiguous()
    padded = torch.cat([x, x[:, -1:]], dim=1)
    padded = torch.cat([padded, padded[:, :, -1:]], dim=2)                     # 6 x 8: the frame with its last row / column repeated
    ref = frameio.pack_frames_torch(padded, "yuv420p10").to(torch.int64)
    got = out.to(torch.int64)
    assert torch.equal(got[:, :35].reshape(2, 5, 7), ref[:, :48].reshape(2, 6, 8)[:, :5, :7])
    assert torch.equal(got[:, 35:], ref[:, 48:])
    one = frameio.pack_frames_torch(x[:1, :1, :1].contiguous(), "yuv420p10")
    assert tuple(one.shape) == (1, 3)
    assert frameio.packed_shape(1, 1, 1, 3, "yuv420p10") == (1, 3) and frameio.packed_shape(2, 4, 6, 4, "bgr8") == (2, 4, 6, 4)


def test_formats_refuse_what_they_cannot_carry():
    frameio = sub("frameio")
    with pytest.raises(ValueError, match="C = 3"):
        frameio.pack_frames_torch(torch.rand(1, 2, 2, 4), "yuv420p10")
    with pytest.raises(ValueError, match="fmt"):
        frameio.pack_frames_torch(torch.rand(1, 2, 2, 3), "rgb16")
    with pytest.raises(ValueError, match="C = 3 or 4"):
        frameio.pack_frames_torch(torch.rand(1, 2, 2, 2), "rgb8")
    with pytest.raises(ValueError):
        frameio.pack_frames_torch(torch.rand(2, 2, 3), "rgb8")
    with pytest.raises(ValueError):
        frameio.pack_frames_torch(torch.rand(1, 2, 2, 3).double(), "rgb8")


def test_pack_frames_uses_the_backend_and_never_falls_back():
    frameio, hip_lib = sub("frameio"), sub("hip_lib")
    from ops_reference import TorchOps
    x = torch.rand(1, 3, 5, 3)

    class Failing:
        def pack_frames(self, frames, fmt, out=None):
            raise hip_lib.HipLibraryError("svr_pack_frames failed")

    class Marking:
        def pack_frames(self, frames, fmt, out=None):
            return ("backend", fmt, out)

    with pytest.raises(hip_lib.HipLibraryError):
        frameio.pack_frames(x, "rgb8", Failing())
    assert frameio.pack_frames(x, "bgr8", Marking(), out=None) == ("backend", "bgr8", None)
    assert not hasattr(TorchOps("cpu"), "pack_frames")
    assert torch.equal(frameio.pack_frames(x, "rgb8", TorchOps("cpu")), frameio.pack_frames_torch(x, "rgb8"))
    out = torch.zeros(1, 15 + 2 * 2 * 3, dtype=torch.uint16)
    assert frameio.pack_frames(x, "yuv420p10", None, out=out) is out
    assert torch.equal(out, frameio.pack_frames_torch(x, "yuv420p10"))
    with pytest.raises(ValueError, match="out"):
        frameio.pack_frames(x, "rgb8", None, out=out)


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_pack_entry_point_refuses_invalid_arguments_before_any_launch():
    """Null pointers, an unknown dtype or format code, empty dimensions, a channel count the format does not take, an out_bytes
    that is not exactly the format's size, a misaligned pointer: refused on the host with a message naming the argument."""
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    call = lambda frames=p, kind=1, T=1, H=4, W=6, C=3, fmt=0, out=p, nbytes=None: L.svr_pack_frames(
        frames, kind, T, H, W, C, fmt, out, (T * H * W * C if fmt != 2 else 2 * T * (H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)))
        if nbytes is None else nbytes, None)
    cases = [(lambda: call(frames=None), b"frames"), (lambda: call(out=None), b"out"), (lambda: call(kind=2), b"x_kind"),
             (lambda: call(kind=-1), b"x_kind"), (lambda: call(T=0), b"T >= 1"), (lambda: call(H=0), b"H >= 1"),
             (lambda: call(W=-3), b"W >= 1"), (lambda: call(fmt=3), b"fmt"), (lambda: call(fmt=-1), b"fmt"),
             (lambda: call(C=2), b"C must be"), (lambda: call(C=5, fmt=1), b"C must be"), (lambda: call(C=4, fmt=2), b"C must be 3"),
             (lambda: call(nbytes=71), b"out_bytes"), (lambda: call(nbytes=73), b"out_bytes"), (lambda: call(nbytes=0), b"out_bytes"),
             (lambda: call(fmt=2, nbytes=2 * 24), b"out_bytes"), (lambda: call(fmt=2, nbytes=74), b"out_bytes"),
             (lambda: call(T=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, nbytes=8), b"T * H * W"), (lambda: call(T=2 ** 21, H=2 ** 10, W=2 ** 10, nbytes=8), b"T * H * W"),
             (lambda: call(frames=ctypes.c_void_p(base + 2)), b"frames"), (lambda: call(fmt=2, out=ctypes.c_void_p(base + 1)), b"out")]
    for fn, word in cases:
        assert fn() != 0
        msg = L.svr_last_error()
        assert b"svr_pack_frames" in msg and word in msg, msg


def test_header_ctypes_table_and_build_list_know_the_entry_point():
    import re
    hip_lib = sub("hip_lib")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert "svr_pack_frames" in declared and "svr_pack_frames" in hip_lib.SYMBOLS
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    for name, code in hip_lib.PACK_FORMATS.items():
        assert re.search(rf"#define SVR_PACK_{name.upper()}\s+{code}\b", src), name
    assert tuple(hip_lib.PACK_FORMATS) == sub("frameio").FORMATS
    assert '#include "svr_frame_pack.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
