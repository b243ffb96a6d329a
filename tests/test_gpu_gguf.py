"""-m gpu: csrc/svr_gguf.hip through HipOps.dequant_gguf against its specification gguf.dequantize_torch and against the reference's
recorded fp32 results -- BIT PATTERNS, every type, bf16 and fp32 output (d * sc * q is exact in fp32 and the one subtraction rounds
once: a mismatch is a finding, not a tolerance) --, its operand rules and refusals, and a tiny GGUF checkpoint through
checkpoint.build_engines(HipOps): the state dict made on the device and one forward of its engine, bit for bit.

Outputs live in tests/guarded_out.py buffers: the guards must stay intact and no poison may be left (every scale of the test blocks
is finite, so no result is a NaN, and the poison patterns are NaNs)."""
import pytest
import torch

from conftest import sub
from guarded_out import guarded
from gguf_fixtures import random_blocks, recorded, tiny_dit_gguf

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAMES = ("Q8_0", "Q4_K", "Q5_K", "Q6_K")
# 1, 2: below one workgroup; 9: all eight 16-byte phases of the 34- and 210-byte blocks and the wrap; 67: off every
# lanes-per-block (4, 32) and blocks-per-workgroup (64, 8) multiple
COUNTS = (1, 2, 9, 67)


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def type_id(name):
    return getattr(sub("gguf"), name)


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def swept_count(name):
    """A block count at which the capped grid sweeps three times, the last one ragged.  The launcher caps the grid at 8 workgroups
    per compute unit, a workgroup is 256 lanes and a lane owns 8 outputs: one sweep is CUs * 8 * 256 * 8 outputs = CUs * 64 blocks
    of 256 (CUs * 512 Q8_0 blocks of 32) -- 16 384 (131 072) on the 256 CUs of an MI355X.  Twice that plus 37 blocks: two full sweeps
    and a third of 37 * 32 = 1 184 lanes (4 workgroups and 160 lanes of a fifth; Q8_0: 148 lanes).  fp32 output: 34 MB."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = sub("gguf").TYPES[type_id(name)][1]
    return 2 * (cus * 8 * 256 * 8 // per) + 37


_cases = {}


def case(name, n):
    """(blocks, the specification's fp32 result), computed once on the host and shared by both output kinds; never modified"""
    if (name, n) not in _cases:
        gguf = sub("gguf")
        blocks = random_blocks(type_id(name), n, seed=17 * type_id(name) + n % 1000)
        _cases[(name, n)] = (blocks, gguf.dequantize_torch(blocks, type_id(name), torch.float32))
    return _cases[(name, n)]


def run_kernel(hip, blocks_dev, name, dtype):
    gguf = sub("gguf")
    _, per, size, _ = gguf.TYPES[type_id(name)]
    g = guarded((blocks_dev.numel() // size, per), dtype)
    out = hip.dequant_gguf(blocks_dev, type_id(name), dtype, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    what = f"dequant_gguf {name} {blocks_dev.numel() // size} blocks -> {dtype}"
    g.assert_guards(what)
    g.assert_written(what)
    return out.cpu()


def mismatches(got, want):
    return int((bits(got) != bits(want)).sum())


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", COUNTS + ("swept",))
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_specification_bit_for_bit(hip, name, n, dtype):
    blocks, want32 = case(name, swept_count(name) if n == "swept" else n)
    want = want32 if dtype == torch.float32 else want32.to(BF16)
    got = run_kernel(hip, blocks.cuda(), name, dtype)
    assert same_bits(got, want), (name, n, mismatches(got, want))


@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_recorded_reference_bit_for_bit(hip, name):
    """the reference's own fp32 block functions (tests/golden/recorded_gguf_dequant.pt): special scales (+-0, the smallest fp16
    subnormal, the largest finite fp16, negative), six-bit scales all 63 / all 0, Q6_K sub-scales -128 / 127"""
    rec = recorded()[name]
    blocks, want = rec["blocks"].cuda(), rec["fp32"]
    got = run_kernel(hip, blocks, name, torch.float32)
    assert same_bits(got, want), mismatches(got, want)
    got = run_kernel(hip, blocks, name, BF16)
    assert same_bits(got, want.to(BF16)), mismatches(got, want.to(BF16))


@pytest.mark.parametrize("name", NAMES)
def test_storage_offset_views_and_the_output_the_op_allocates(hip, name):
    """A view 32 bytes into a larger buffer is read in place; views 1, 2 and 16 bytes in are not 32-byte aligned and go through the
    copy: the same bits every time.  Without ``out`` the op allocates [n_blocks, block size]."""
    gguf = sub("gguf")
    blocks, want32 = case(name, 9)
    want = want32.to(BF16)
    flat = blocks.reshape(-1)
    store = torch.zeros(flat.numel() + 96, dtype=torch.uint8, device="cuda")
    assert store.data_ptr() % 32 == 0
    for off in (32, 1, 2, 16):
        view = store[off:off + flat.numel()]
        view.copy_(flat)
        assert view.is_contiguous() and view.data_ptr() % 32 == off % 32
        assert same_bits(run_kernel(hip, view, name, BF16), want), off
        assert same_bits(run_kernel(hip, view.view(9, -1), name, torch.float32), want32), off
    out = hip.dequant_gguf(blocks.cuda(), type_id(name))
    assert out.dtype == BF16 and tuple(out.shape) == (9, gguf.TYPES[type_id(name)][1]) and same_bits(out.cpu(), want)


def test_refusals_name_the_argument_and_launch_nothing(hip):
    import ctypes
    gguf = sub("gguf")
    blocks = random_blocks(gguf.Q4_K, 4, 1).cuda()
    out = guarded((4, 256), BF16)
    with pytest.raises(ValueError, match="blocks must be contiguous"):
        hip.dequant_gguf(blocks[::2], gguf.Q4_K, out=out.t)
    with pytest.raises(ValueError, match="blocks must be contiguous"):
        hip.dequant_gguf(torch.zeros(4, 288, dtype=torch.uint8, device="cuda")[:, :144], gguf.Q4_K, out=out.t)
    with pytest.raises(ValueError, match="blocks must be torch.uint8"):
        hip.dequant_gguf(blocks.view(torch.int8), gguf.Q4_K, out=out.t)
    with pytest.raises(ValueError, match="whole Q4_K blocks of 144 bytes"):
        hip.dequant_gguf(blocks.reshape(-1)[:-1], gguf.Q4_K)
    with pytest.raises(ValueError, match="whole Q6_K blocks of 210 bytes"):
        hip.dequant_gguf(blocks, gguf.Q6_K)
    with pytest.raises(ValueError, match="whole Q8_0 blocks"):
        hip.dequant_gguf(blocks[:0], gguf.Q8_0)
    with pytest.raises(ValueError, match="blocks must live on"):
        hip.dequant_gguf(blocks.cpu(), gguf.Q4_K, out=out.t)
    with pytest.raises(ValueError, match="Q4_0"):
        hip.dequant_gguf(blocks, 2, out=out.t)
    with pytest.raises(ValueError, match="F16"):
        hip.dequant_gguf(blocks, gguf.F16, out=out.t)
    with pytest.raises(ValueError, match="out_dtype"):
        hip.dequant_gguf(blocks, gguf.Q4_K, torch.float16)
    with pytest.raises(ValueError, match="out must be"):
        hip.dequant_gguf(blocks, gguf.Q4_K, out=torch.empty(1024, dtype=BF16, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        hip.dequant_gguf(blocks, gguf.Q4_K, out=torch.empty(3, 256, dtype=BF16, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        hip.dequant_gguf(blocks, gguf.Q4_K, BF16, out=torch.empty(4, 256, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="out must be contiguous"):
        hip.dequant_gguf(blocks, gguf.Q4_K, out=torch.empty(4, 512, dtype=BF16, device="cuda")[:, ::2])
    # the C entry point itself, on device pointers
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    L = hip.lib
    for nbytes in (4 * 512 - 2, 4 * 512 + 16, 4 * 1024):
        assert L.svr_dequant_gguf(p(blocks), gguf.Q4_K, 4, p(out.t), 0, nbytes, None) != 0 and b"out_bytes" in L.svr_last_error()
    assert L.svr_dequant_gguf(p(blocks, 16), gguf.Q4_K, 3, p(out.t), 0, 3 * 512, None) != 0 and b"aligned" in L.svr_last_error()
    assert L.svr_dequant_gguf(p(blocks), gguf.Q4_K, 4, p(out.t, 8), 0, 4 * 512, None) != 0 and b"aligned" in L.svr_last_error()
    assert L.svr_dequant_gguf(p(blocks), 2, 4, p(out.t), 0, 4 * 512, None) != 0 and b"ggml_type" in L.svr_last_error()
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was launched: the payload is untouched


@pytest.mark.parametrize("family", ["3b", "7b"])
def test_tiny_gguf_checkpoint_through_build_engines_on_the_device(hip, tmp_path, family, monkeypatch):
    """The file goes to the device in staging pieces (made small here: several pieces, both buffers reused, a ragged last one), is
    expanded there, and gives the specification's state dict; the engine built from the file and the engine built from that state
    dict run the same kernels on the same weights: one forward, equal bit for bit."""
    gguf, ck, config, dit = sub("gguf"), sub("checkpoint"), sub("config"), sub("dit")
    cfg = config.DIT_TINY if family == "3b" else config.DIT_7B_TINY
    path = str(tmp_path / f"seedvr2_ema_{family}-Q4_K_M.gguf")
    want, types = tiny_dit_gguf(path, cfg, seed=21)
    assert {gguf.Q4_K, gguf.Q5_K, gguf.Q6_K, gguf.Q8_0, gguf.F16, gguf.F32} <= set(types.values())
    monkeypatch.setattr(gguf, "STAGING_BYTES", 300007)
    got = ck.load_state_dict(path, ops=hip)
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].is_cuda and same_bits(got[k].cpu(), v), (k, gguf.type_name(types[k]))
    assert ck.detect_dit_config(got) is (config.DIT_3B if family == "3b" else config.DIT_7B)
    eng, _ = ck.build_engines(hip, dit_path=path, dit_cfg=cfg)
    twin = dit.NaDiTEngine(cfg, ck.prepare_dit_state_dict(dict(want), cfg), hip)
    g = torch.Generator().manual_seed(0)
    vid, txt = torch.randn(3, 16, 24, 33, generator=g).to(BF16).cuda(), sub("weights").synth_text_embedding().cuda()
    a, b = eng.forward(vid, txt, 1000.0), twin.forward(vid, txt, 1000.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a.float()).all()) and same_bits(a.cpu(), b.cpu())
