"""ops.clip_args: the checks every entry point that reads a clip makes first, with each caller's own words -- without a GPU.

The callers are driven through a HipOps that was never initialised (its device set to the CPU): every call below is refused in
Python, before the library is touched.  The expected texts are the ones these callers raised when each spelled the checks out
itself."""
import pytest
import torch

from conftest import sub

CPU = torch.device("cpu")
GOOD = torch.zeros(2, 4, 6, 3)


@pytest.fixture(scope="module")
def ops():
    mod = sub("ops")
    shell = object.__new__(mod.HipOps)
    shell.device = CPU
    return shell


# caller -> how it is called with a clip
CALLERS = {
    "frame_signatures": lambda ops, x: ops.frame_signatures(x),
    "active_profile": lambda ops, x: ops.active_profile(x, 16),
    "encode_png": lambda ops, x: ops.encode_png(x),
    "pack_frames": lambda ops, x: ops.pack_frames(x, "rgb8"),
    "pack_yuv420p10": lambda ops, x: ops.pack_yuv420p10(x),
}
SIZES = {
    "frame_signatures": "frames must hold T >= 1 frames of H >= 4, W >= 4",
    "active_profile": "frames must hold T >= 1 frames of H >= 1, W >= 1",
    "encode_png": "frames must hold at least one pixel",
    "pack_frames": "frames must hold at least one pixel",
    "pack_yuv420p10": "frames must hold at least one pixel",
}
TWO_CHANNELS = {
    "frame_signatures": "frames must have C = 3 or 4, got C = 2",
    "active_profile": "frames must have C = 3 or 4, got C = 2",
    "encode_png": "C must be 3 or 4, got C = 2",
    "pack_frames": "rgb8 takes C = 3 or 4, got C = 2",
    "pack_yuv420p10": "yuv420p10 takes C = 3 (it has no alpha plane), got C = 2",
}


def refused(call, ops, x):
    with pytest.raises(ValueError) as e:
        call(ops, x)
    return str(e.value)


@pytest.mark.parametrize("name", sorted(CALLERS))
def test_each_caller_keeps_its_words(ops, name):
    call = CALLERS[name]
    assert refused(call, ops, torch.zeros(2, 4, 6)) == f"{name}: frames must be [T, H, W, C] in fp32 or bf16, got (2, 4, 6) torch.float32"
    assert refused(call, ops, GOOD.to(torch.float16)) == f"{name}: frames must be [T, H, W, C] in fp32 or bf16, got (2, 4, 6, 3) torch.float16"
    assert refused(call, ops, GOOD.to(torch.uint8)) == f"{name}: frames must be [T, H, W, C] in fp32 or bf16, got (2, 4, 6, 3) torch.uint8"
    assert refused(call, ops, torch.zeros(2, 4, 6, 2)) == f"{name}: {TWO_CHANNELS[name]}"
    for shape in ((0, 4, 6, 3), (2, 0, 6, 3), (2, 4, 0, 3)):
        assert refused(call, ops, torch.zeros(shape, dtype=torch.bfloat16)) == f"{name}: {SIZES[name]}, got {shape}"
    assert refused(call, ops, torch.zeros(2, 4, 12, 3)[:, :, ::2]) == f"{name}: frames must be contiguous"
    assert refused(call, ops, GOOD.permute(0, 2, 1, 3)) == f"{name}: frames must be contiguous"
    assert refused(call, ops, torch.zeros(2, 4, 6, 3, device="meta")) == f"{name}: frames must live on cpu, got meta"


def test_frame_signatures_needs_four_rows_and_columns(ops):
    for shape in ((1, 3, 4, 3), (1, 4, 3, 4)):
        assert refused(CALLERS["frame_signatures"], ops, torch.zeros(shape)) == \
            f"frame_signatures: frames must hold T >= 1 frames of H >= 4, W >= 4, got {shape}"
    # (one row or column is a clip to the others)
    assert refused(CALLERS["active_profile"], ops, torch.zeros(1, 1, 1, 3, device="meta")) == "active_profile: frames must live on cpu, got meta"


def test_the_fault_reported_first_stays_the_same(ops):
    """Rank and dtype, then the channel count, then a caller's codes, then the sizes, then a caller's limits, then device and layout."""
    frameio = sub("frameio")
    empty, sparse = torch.zeros(0, 4, 6, 3), torch.zeros(2, 4, 12, 3)[:, :, ::2]
    assert refused(lambda o, x: o.encode_png(x, depth=7), ops, torch.zeros(2, 4, 6, 2)) == "encode_png: C must be 3 or 4, got C = 2"
    assert refused(lambda o, x: o.encode_png(x, depth=7), ops, empty) == "encode_png: depth must be 8 or 16, got 7"
    assert refused(lambda o, x: o.pack_frames(x, "rgb9"), ops, empty) == f"pack_frames: fmt must be one of {frameio.FORMATS}, got 'rgb9'"
    assert refused(lambda o, x: o.pack_frames(x, "yuv420p10"), ops, torch.zeros(0, 4, 6, 4)) == \
        "pack_frames: yuv420p10 takes C = 3 (it has no alpha plane), got C = 4"
    assert refused(lambda o, x: o.pack_yuv420p10(x, matrix="bt470"), ops, torch.zeros(0, 4, 6, 2)) == \
        f"pack_yuv420p10: matrix must be one of {tuple(frameio.KR_KB)}, got 'bt470'"
    assert refused(lambda o, x: o.pack_yuv420p10(x, siting="top"), ops, sparse) == \
        f"pack_yuv420p10: siting must be one of {frameio.SITINGS}, got 'top'"
    assert refused(lambda o, x: o.active_profile(x, 256), ops, empty) == \
        "active_profile: frames must hold T >= 1 frames of H >= 1, W >= 1, got (0, 4, 6, 3)"
    assert refused(lambda o, x: o.active_profile(x, 256), ops, sparse) == "active_profile: dark must be an integer in 0..255, got 256"
    assert refused(lambda o, x: o.active_profile(x, True), ops, GOOD) == "active_profile: dark must be an integer in 0..255, got True"
    wide = torch.zeros(1, 1, 3, device="meta").expand(1 << 16, 1 << 15, 1, 3)               # T * max(H, W) = 2^31, no storage
    assert refused(lambda o, x: o.active_profile(x, 256), ops, wide) == \
        f"active_profile: frames of T * max(H, W) = {1 << 31}; the int32 counters hold fewer than 2^31"
    large = torch.zeros(1, 1, 3, device="meta").expand(1, 1 << 16, 1 << 15, 3)              # H * W = 2^31
    assert refused(CALLERS["frame_signatures"], ops, large) == \
        f"frame_signatures: frames of H * W = {1 << 31} pixels; the int32 counters hold fewer than 2^31"
    assert refused(lambda o, x: o.active_profile(x, 16), ops, large) == "active_profile: frames must live on cpu, got meta"


def test_clip_args_returns_the_geometry_and_the_store_kind():
    ops_mod = sub("ops")
    assert ops_mod.clip_args("f", GOOD, CPU) == (2, 4, 6, 3, ops_mod.STORE_FP32)
    assert ops_mod.clip_args("f", torch.zeros(1, 4, 4, 4, dtype=torch.bfloat16), CPU, min_hw=4) == (1, 4, 4, 4, ops_mod.STORE_BF16)
    assert ops_mod.clip_args("f", torch.zeros(1, 1, 1, 7), CPU, channels=None) == (1, 1, 1, 7, ops_mod.STORE_FP32)
    seen = []
    ops_mod.clip_args("f", GOOD, CPU, before=lambda *a: seen.append(("before", a)), after=lambda *a: seen.append(("after", a)))
    assert seen == [("before", (2, 4, 6, 3)), ("after", (2, 4, 6, 3))]
    with pytest.raises(ValueError, match="^f: mine$"):
        ops_mod.clip_args("f", GOOD, CPU, after=lambda *a: "mine")


def test_out_is_allocated_or_checked(ops):
    out = ops._out("f", None, (2, 3), torch.int32)
    assert out.shape == (2, 3) and out.dtype == torch.int32 and out.device == CPU
    assert ops._out("f", out, (2, 3), torch.int32) is out
    with pytest.raises(ValueError, match=r"^f: out must be \(2, 4\) for rgb8, got \(2, 3\)$"):
        ops._out("f", out, (2, 4), torch.int32, suffix=" for rgb8")
    with pytest.raises(ValueError, match="^f: out must be torch.int64, got torch.int32$"):
        ops._out("f", out, (2, 3), torch.int64)
    with pytest.raises(ValueError, match="^f: out must be contiguous$"):
        ops._out("f", torch.zeros(3, 2, dtype=torch.int32).t(), (2, 3), torch.int32)
    # the callers' words for a wrong ``out``
    assert refused(lambda o, x: o.frame_signatures(x, out=torch.zeros(2, 1000, dtype=torch.int32)), ops, GOOD) == \
        "frame_signatures: out must be (2, 1024), got (2, 1000)"
    assert refused(lambda o, x: o.active_profile(x, 16, out=torch.zeros(11, dtype=torch.int32)), ops, GOOD) == \
        "active_profile: out must be (10,), got (11,)"
    assert refused(lambda o, x: o.pack_frames(x, "bgr8", out=torch.zeros(2, 4, 6, 4, dtype=torch.uint8)), ops, GOOD) == \
        "pack_frames: out must be (2, 4, 6, 3) for bgr8, got (2, 4, 6, 4)"
    assert refused(lambda o, x: o.pack_yuv420p10(x, out=torch.zeros(2, 35, dtype=torch.uint16)), ops, GOOD) == \
        "pack_yuv420p10: out must be (2, 36), got (2, 35)"
    assert refused(lambda o, x: o.pack_frames(x, "rgb8", out=torch.zeros(2, 4, 6, 3, dtype=torch.int8)), ops, GOOD) == \
        "pack_frames: out must be torch.uint8, got torch.int8"
