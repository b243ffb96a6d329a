"""-m "not gpu": GGUF checkpoints (gguf.py: reader, writer, the specification of csrc/svr_gguf.hip, the loader) -- the
specification against the reference's own block functions at fp32, BIT FOR BIT (recorded in tests/golden/recorded_gguf_dequant.pt
by tools/make_gguf_golden.py, and live where the reference checkout is mounted), against hand-encoded blocks, the file format's
round trips and refusals, a tiny DiT checkpoint through checkpoint / interfaces, the C entry point's refusals."""
import ctypes
import os
import shutil
import struct
import typing

import pytest
import torch

from conftest import ROOT, sub
from gguf_fixtures import random_blocks, recorded, tiny_dit_gguf
from ops_reference import TorchOps
from oracle import reference_loader as rl

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
REFERENCE_FILE = "src/optimization/gguf_dequant.py"
NAMES = ("Q8_0", "Q4_K", "Q5_K", "Q6_K")


def type_id(name):
    return getattr(sub("gguf"), name)


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- specification
@pytest.mark.parametrize("name", NAMES)
def test_specification_equals_the_recorded_reference_bit_for_bit(name):
    gguf = sub("gguf")
    rec = recorded()[name]
    blocks, want = rec["blocks"], rec["fp32"]
    assert tuple(blocks.shape) == (75, gguf.TYPES[type_id(name)][2]) and want.dtype == torch.float32
    assert same_bits(gguf.dequantize_torch(blocks, type_id(name), torch.float32), want)
    assert same_bits(gguf.dequantize_torch(blocks, type_id(name), torch.bfloat16), want.to(torch.bfloat16))
    assert same_bits(gguf.dequantize_torch(blocks.reshape(-1), type_id(name)), want.to(torch.bfloat16))      # flat bytes, default dtype


@pytest.mark.skipif(not os.path.exists(os.path.join(rl.REFERENCE_ROOT, REFERENCE_FILE)), reason="the reference checkout is not mounted")
@pytest.mark.parametrize("name", NAMES)
def test_specification_equals_the_reference_functions_on_20000_random_blocks(name):
    gguf = sub("gguf")
    ns = {"torch": torch, "QK_K": 256, "K_SCALE_SIZE": 12, "Optional": typing.Optional, "Tuple": typing.Tuple, "List": typing.List}
    rl._extract(REFERENCE_FILE, ["to_uint32", "split_block_dims", "get_scale_min"] + [f"dequantize_blocks_{n}" for n in NAMES], ns)
    _, per, size, _ = gguf.TYPES[type_id(name)]
    blocks = random_blocks(type_id(name), 20000, seed=7)
    want = ns[f"dequantize_blocks_{name}"](blocks.clone(), per, size, torch.float32)
    assert bool(torch.isfinite(want).all())
    assert same_bits(gguf.dequantize_torch(blocks, type_id(name), torch.float32), want)
    assert same_bits(gguf.dequantize_torch(blocks, type_id(name), torch.bfloat16), want.to(torch.bfloat16))


def half_bytes(x):
    return list(struct.pack("<e", x))


def k_scale_bytes(sc, m):
    """the 12 scale bytes of a Q4_K / Q5_K block from eight six-bit scales and mins: bytes 0-3 the low scales with the top two bits
    of scales 4-7 above them, bytes 4-7 the same for the mins, bytes 8-11 the low nibbles of scale (low) and min (high) 4-7"""
    out = [0] * 12
    for j in range(4):
        out[j] = sc[j] | ((sc[j + 4] >> 4) << 6)
        out[j + 4] = m[j] | ((m[j + 4] >> 4) << 6)
        out[j + 8] = (sc[j + 4] & 15) | ((m[j + 4] & 15) << 4)
    return out


SC = [1, 2, 3, 5, 17, 33, 47, 63]
MN = [0, 1, 2, 4, 16, 32, 48, 63]


def test_hand_encoded_q8_0_block():
    gguf = sub("gguf")
    q = [8 * e - 128 for e in range(32)]                                     # -128 .. 120
    block = half_bytes(0.25) + [v & 0xFF for v in q]
    want = [0.25 * v for v in q]
    got = gguf.dequantize_torch(torch.tensor(block, dtype=torch.uint8), gguf.Q8_0, torch.float32)
    assert got.shape == (1, 32) and got[0].tolist() == want


@pytest.mark.parametrize("name", ["Q4_K", "Q5_K"])
def test_hand_encoded_q4_k_and_q5_k_blocks(name):
    """d = 0.5, dmin = 0.25, scales and mins that use all six bits on either side of j = 4, q[e] a fixed pattern over the whole range:
    every product and the difference are exact, so the 256 expected values are plain arithmetic."""
    gguf = sub("gguf")
    top = 16 if name == "Q4_K" else 32
    q = [(7 * e + 3) % top for e in range(256)]
    qs, qh = [0] * 128, [0] * 32
    for e in range(256):
        j, l = e // 32, e % 32
        qs[32 * (e // 64) + l] |= (q[e] & 15) << (4 * (j % 2))
        qh[l] |= (q[e] >> 4) << j
    block = half_bytes(0.5) + half_bytes(0.25) + k_scale_bytes(SC, MN) + (qh if name == "Q5_K" else []) + qs
    assert len(block) == gguf.TYPES[type_id(name)][2]
    want = [0.5 * SC[e // 32] * q[e] - 0.25 * MN[e // 32] for e in range(256)]
    got = gguf.dequantize_torch(torch.tensor(block, dtype=torch.uint8), type_id(name), torch.float32)
    assert got.shape == (1, 256) and got[0].tolist() == want
    assert min(want) < 0 < max(want) and len(set(q)) == top


def test_hand_encoded_q6_k_block():
    gguf = sub("gguf")
    q = [(5 * e + 1) % 64 - 32 for e in range(256)]                          # -32 .. 31
    scales = [-128, -77, -33, -8, -1, 0, 1, 2, 3, 7, 19, 45, 64, 99, 126, 127]
    ql, qh = [0] * 128, [0] * 64
    for e in range(256):
        h, r, l = e // 128, (e % 128) // 32, e % 32
        six = q[e] + 32
        ql[64 * h + 32 * (r & 1) + l] |= (six & 15) << (4 * (r >> 1))
        qh[32 * h + l] |= (six >> 4) << (2 * r)
    block = ql + qh + [s & 0xFF for s in scales] + half_bytes(-0.125)
    assert len(block) == 210
    want = [-0.125 * scales[e // 16] * q[e] for e in range(256)]
    got = gguf.dequantize_torch(torch.tensor(block, dtype=torch.uint8), gguf.Q6_K, torch.float32)
    assert got.shape == (1, 256) and got[0].tolist() == want
    assert len(set(q)) == 64


def test_zero_signs_follow_the_expression_order():
    """(d * sc) * q - dmin * m: -0 * q - (+0) = -0, +0 - (+0) = +0, and a zero quant under a negative d keeps the minus sign"""
    gguf = sub("gguf")
    sign = lambda x: [v < 0 for v in bits(x).flatten().tolist()]
    for d, expect_negative in ((0.0, False), (-0.0, True)):
        block = half_bytes(d) + half_bytes(0.0) + k_scale_bytes(SC, MN) + [0x11] * 128
        got = gguf.dequantize_torch(torch.tensor(block, dtype=torch.uint8), gguf.Q4_K, torch.float32)
        assert float(got.abs().max()) == 0 and sign(got) == [expect_negative] * 256
    got = gguf.dequantize_torch(torch.tensor(half_bytes(-1.0) + [0] * 32, dtype=torch.uint8), gguf.Q8_0, torch.float32)
    assert float(got.abs().max()) == 0 and sign(got) == [True] * 32


def test_dequantize_refuses_what_it_cannot_read():
    gguf = sub("gguf")
    with pytest.raises(ValueError, match="Q4_0"):
        gguf.dequantize_torch(torch.zeros(18, dtype=torch.uint8), 2)
    with pytest.raises(ValueError, match="F16"):
        gguf.dequantize_torch(torch.zeros(32, dtype=torch.uint8), gguf.F16)
    with pytest.raises(ValueError, match="multiple of 144"):
        gguf.dequantize_torch(torch.zeros(143, dtype=torch.uint8), gguf.Q4_K)
    with pytest.raises(ValueError, match="uint8"):
        gguf.dequantize_torch(torch.zeros(144, dtype=torch.int8), gguf.Q4_K)
    with pytest.raises(ValueError, match="out_dtype"):
        gguf.dequantize_torch(torch.zeros(144, dtype=torch.uint8), gguf.Q4_K, torch.float16)


# ---------------------------------------------------------------------------------------------------------------- reader / writer
ALL_VALUE_TYPES = {
    "t.u8": (0, 200), "t.i8": (1, -100), "t.u16": (2, 60000), "t.i16": (3, -30000), "t.u32": (4, 4000000000), "t.i32": (5, -2000000000),
    "t.f32": (6, 0.5), "t.bool": (7, True), "t.str": (8, "héllo GGUF"), "t.u64": (10, 2 ** 63 + 5), "t.i64": (11, -2 ** 62),
    "t.f64": (12, 1e-300), "t.arr_i32": (9, (5, [1, -2, 3])), "t.arr_str": (9, (8, ["a", "", "tokens and more tokens"])),
    "t.arr_f32": (9, (6, [0.25, -1.5])), "t.arr_bool": (9, (7, [True, False, True])), "t.arr_empty": (9, (4, [])),
    "t.arr_nested": (9, (9, [(5, [1, 2]), (8, ["x"])])), "inferred.int": 7, "inferred.str": "s", "inferred.list": [4, 5],
}


def sample_tensors(gguf, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = [("plain.f32", gguf.F32, (3, 5), torch.randn(3, 5, generator=g)),
         ("plain.f16", gguf.F16, (7,), torch.randn(7, generator=g).to(torch.float16)),
         ("plain.bf16", gguf.BF16, (2, 3, 4), torch.randn(2, 3, 4, generator=g).to(torch.bfloat16)),
         ("q.q8_0", gguf.Q8_0, (3, 64), random_blocks(gguf.Q8_0, 6, seed + 1)),
         ("q.q4_k", gguf.Q4_K, (2, 512), random_blocks(gguf.Q4_K, 4, seed + 2)),
         ("q.q5_k", gguf.Q5_K, (3, 256), random_blocks(gguf.Q5_K, 3, seed + 3)),
         ("q.q6_k", gguf.Q6_K, (5, 2, 256), random_blocks(gguf.Q6_K, 10, seed + 4))]
    return t


@pytest.mark.parametrize("alignment", [32, 64])
@pytest.mark.parametrize("version", [2, 3])
def test_round_trip_of_every_type_with_every_metadata_value_type(tmp_path, alignment, version):
    gguf = sub("gguf")
    path = str(tmp_path / "all.gguf")
    tensors = sample_tensors(gguf)
    meta = dict(ALL_VALUE_TYPES)
    meta["general.alignment"] = (gguf.U32, alignment)
    gguf.write_gguf(path, tensors, meta, version=version)
    assert open(path, "rb").read(8) == b"GGUF" + struct.pack("<I", version)
    got_meta, infos = gguf.read_gguf(path)
    assert got_meta["general.alignment"] == alignment and got_meta["t.str"] == "héllo GGUF" and got_meta["t.bool"] is True
    assert got_meta["t.u64"] == 2 ** 63 + 5 and got_meta["t.i64"] == -2 ** 62 and got_meta["t.f64"] == 1e-300 and got_meta["t.i8"] == -100
    assert got_meta["t.arr_i32"] == [1, -2, 3] and got_meta["t.arr_str"] == ["a", "", "tokens and more tokens"]
    assert got_meta["t.arr_bool"] == [True, False, True] and got_meta["t.arr_empty"] == [] and got_meta["t.arr_nested"] == [[1, 2], ["x"]]
    assert got_meta["inferred.int"] == 7 and got_meta["inferred.str"] == "s" and got_meta["inferred.list"] == [4, 5]
    assert len(got_meta) == len(meta)
    assert [i.name for i in infos] == [t[0] for t in tensors]
    for info, (name, ggml_type, shape, data) in zip(infos, tensors):
        assert info.ggml_type == ggml_type and info.shape == tuple(shape) and info.ne == tuple(reversed(shape))     # reversed on disk
        assert info.offset % alignment == 0 and info.data.dtype == torch.uint8
        assert torch.equal(info.data, data.contiguous().reshape(-1).view(torch.uint8)), name
    sd = gguf.load_state_dict(path)
    for name, ggml_type, shape, data in tensors:
        if ggml_type in gguf.QUANTISED:
            assert same_bits(sd[name], gguf.dequantize_torch(data, ggml_type, torch.bfloat16).reshape(shape)), name
        else:
            assert same_bits(sd[name], data), name
    assert sub("checkpoint").to_compute_dtype(sd)["plain.f32"].dtype == torch.bfloat16


def test_comfy_orig_shape_is_the_logical_shape(tmp_path):
    gguf = sub("gguf")
    path = str(tmp_path / "orig.gguf")
    blocks = random_blocks(gguf.Q4_K, 12, 3)
    gguf.write_gguf(path, [("conv.weight", gguf.Q4_K, (12, 256), blocks), ("other", gguf.Q8_0, (2, 32), random_blocks(gguf.Q8_0, 2, 4))],
                    {"comfy.gguf.orig_shape.conv.weight": (gguf.ARRAY, (gguf.I32, [4, 3, 16, 16]))})
    _, infos = gguf.read_gguf(path)
    assert infos[0].shape == (4, 3, 16, 16) and infos[0].ne == (256, 12) and infos[1].shape == (2, 32)
    sd = gguf.load_state_dict(path)
    assert same_bits(sd["conv.weight"], gguf.dequantize_torch(blocks, gguf.Q4_K).reshape(4, 3, 16, 16))
    gguf.write_gguf(path, [("conv.weight", gguf.Q4_K, (12, 256), blocks)],
                    {"comfy.gguf.orig_shape.conv.weight": (gguf.ARRAY, (gguf.I32, [5, 3, 16, 16]))})
    with pytest.raises(ValueError, match=r"orig\.gguf.*conv\.weight.*Q4_K"):
        gguf.read_gguf(path)


def patched(path, find, replace, at=0):
    raw = bytearray(open(path, "rb").read())
    i = raw.index(find) + at
    raw[i:i + len(replace)] = replace
    open(path, "wb").write(bytes(raw))


def test_every_unreadable_file_is_a_value_error_naming_the_path_and_the_tensor(tmp_path):
    gguf, ck = sub("gguf"), sub("checkpoint")
    path = str(tmp_path / "bad.gguf")
    write = lambda: gguf.write_gguf(path, [("first", gguf.F32, (4,), torch.zeros(4)),
                                           ("blocks.0.w", gguf.Q4_K, (2, 256), random_blocks(gguf.Q4_K, 2, 0))])
    for loader in (gguf.read_gguf, gguf.load_state_dict, ck.load_state_dict):
        with pytest.raises(ValueError, match="absent.gguf"):
            loader(str(tmp_path / "absent.gguf"))
    with pytest.raises(ValueError, match="bad.gguf"):                             # a directory: unreadable
        os.mkdir(path)
        gguf.read_gguf(path)
    os.rmdir(path)
    open(path, "wb").write(b"")
    with pytest.raises(ValueError, match="bad.gguf"):
        gguf.read_gguf(path)
    write()
    patched(path, b"GGUF", b"GGML")
    with pytest.raises(ValueError, match="bad.gguf.*magic"):
        gguf.read_gguf(path)
    write()
    patched(path, b"GGUF", struct.pack("<I", 1), at=4)
    with pytest.raises(ValueError, match="bad.gguf.*version 1"):
        gguf.read_gguf(path)
    write()
    patched(path, b"GGUF", struct.pack(">I", 3), at=4)
    with pytest.raises(ValueError, match="bad.gguf.*big-endian"):
        gguf.read_gguf(path)
    write()
    whole = open(path, "rb").read()
    open(path, "wb").write(whole[:-1])                                            # the last tensor loses its last byte
    with pytest.raises(ValueError, match=r"bad\.gguf.*blocks\.0\.w.*Q4_K.*past the end"):
        gguf.read_gguf(path)
    open(path, "wb").write(whole[:40])                                            # the header itself is cut
    with pytest.raises(ValueError, match=r"bad\.gguf.*ends inside its header"):
        gguf.read_gguf(path)
    write()
    name = struct.pack("<Q", 10) + b"blocks.0.w"
    patched(path, name, struct.pack("<IQQ", 2, 128, 4), at=len(name))             # ne = (128, 4): the same 512 elements
    with pytest.raises(ValueError, match=r"bad\.gguf.*blocks\.0\.w.*Q4_K.*ne\[0\] = 128.*256"):
        gguf.read_gguf(path)
    gguf.write_gguf(path, [("twin_a", gguf.F32, (4,), torch.zeros(4)), ("twin_b", gguf.F32, (4,), torch.ones(4))])
    patched(path, b"twin_b", b"twin_a")
    with pytest.raises(ValueError, match=r"bad\.gguf.*duplicate.*twin_a"):
        gguf.read_gguf(path)
    for type_id_, type_name_ in ((2, "Q4_0"), (10, "Q2_K"), (11, "Q3_K"), (20, "IQ4_NL"), (99, "ggml type 99")):
        write()
        patched(path, name, struct.pack("<I", type_id_), at=len(name) + 4 + 16)
        with pytest.raises(ValueError, match=rf"bad\.gguf.*blocks\.0\.w.*unsupported.*{type_name_}"):
            gguf.load_state_dict(path)


# ---------------------------------------------------------------------------------------------------------------- checkpoint / interfaces
@pytest.fixture(scope="module")
def tiny_files(tmp_path_factory):
    """path, the specification's state dict and the ggml type of every tensor: DIT_TINY plain and with the ComfyUI prefix, DIT_7B_TINY"""
    config = sub("config")
    d = tmp_path_factory.mktemp("gguf")
    out = {}
    for key, cfg, fname, prefix in (("3b", config.DIT_TINY, "seedvr2_ema_3b-Q4_K_M.gguf", ""),
                                    ("3b_prefixed", config.DIT_TINY, "prefixed.gguf", "model.diffusion_model."),
                                    ("7b", config.DIT_7B_TINY, "seedvr2_ema_7b-Q4_K_M.gguf", "")):
        path = str(d / fname)
        want, types = tiny_dit_gguf(path, cfg, seed=21, prefix=prefix)
        out[key] = (path, cfg, want, types)
    return out


@pytest.mark.parametrize("key", ["3b", "3b_prefixed", "7b"])
def test_tiny_dit_checkpoint_as_gguf_loads_to_the_specifications_state_dict(tiny_files, key):
    gguf, ck = sub("gguf"), sub("checkpoint")
    path, cfg, want, types = tiny_files[key]
    used = set(types.values())
    assert {gguf.Q4_K, gguf.Q5_K, gguf.Q6_K, gguf.Q8_0, gguf.F16, gguf.F32} <= used, used          # the mixture real files have
    got = ck.prepare_dit_state_dict(ck.load_state_dict(path), cfg)
    assert set(got) == set(want)
    for k, v in want.items():
        expect = v if k.endswith("rope.rope.freqs") else v.to(torch.bfloat16)
        assert same_bits(got[k], expect), k
    assert got["blocks.0.attn.rope.rope.freqs"].dtype == torch.float32
    assert all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    values = torch.cat([v.float().flatten() for k, v in got.items() if types[k] in gguf.QUANTISED])
    assert 0.005 < float(values.std()) < 0.2                                                       # scales in a sane range


def test_engine_from_a_gguf_file_equals_the_engine_from_its_state_dict(tiny_files):
    ck, dit = sub("checkpoint"), sub("dit")
    path, cfg, want, _ = tiny_files["3b"]
    ops = TorchOps("cpu", act_dtype=torch.float32)
    g = torch.Generator().manual_seed(0)
    vid, txt = torch.randn(2, 8, 12, 33, generator=g), torch.randn(58, 5120, generator=g)
    a = dit.NaDiTEngine(cfg, ck.prepare_dit_state_dict(dict(want), cfg), ops).forward(vid, txt, 1000.0)
    b = dit.NaDiTEngine(cfg, ck.prepare_dit_state_dict(ck.load_state_dict(path), cfg), ops).forward(vid, txt, 1000.0)
    eng, _ = ck.build_engines(ops, dit_path=path, dit_cfg=cfg)                        # (TorchOps has no dequant_gguf: the torch statement)
    assert not hasattr(ops, "dequant_gguf")
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, eng.forward(vid, txt, 1000.0))


def test_resolve_model_and_family_detection_accept_gguf(tiny_files):
    interfaces, ck, config = sub("interfaces"), sub("checkpoint"), sub("config")
    path3, _, _, _ = tiny_files["3b"]
    path7, _, _, _ = tiny_files["7b"]
    assert "seedvr2_ema_3b-Q4_K_M.gguf" in interfaces.DIT_MODELS
    assert interfaces.resolve_model(os.path.basename(path3), os.path.dirname(path3)) == path3
    assert interfaces.resolve_model(path7) == path7
    with pytest.raises(FileNotFoundError):
        interfaces.resolve_model("seedvr2_ema_3b-Q8_0.gguf", os.path.dirname(path3))
    assert ck.detect_dit_config(ck.load_state_dict(path7)) is config.DIT_7B
    assert ck.detect_dit_config(ck.load_state_dict(path3)) is config.DIT_3B
    assert ck.detect_dit_config(ck.load_state_dict(tiny_files["3b_prefixed"][0])) is config.DIT_3B


def test_load_uses_the_backend_and_never_falls_back(tiny_files):
    gguf, hip_lib = sub("gguf"), sub("hip_lib")
    path = tiny_files["3b"][0]

    class Failing:
        device = torch.device("cpu")

        def dequant_gguf(self, blocks, ggml_type, out_dtype=torch.bfloat16, out=None):
            raise hip_lib.HipLibraryError("svr_dequant_gguf failed")

    calls = []

    class Marking(Failing):
        def dequant_gguf(self, blocks, ggml_type, out_dtype=torch.bfloat16, out=None):
            calls.append((ggml_type, blocks.numel()))
            return gguf.dequantize_torch(blocks, ggml_type, out_dtype)

    staged = gguf._to_device_staged
    gguf._to_device_staged = lambda mm, start, stop, device: torch.frombuffer(mm, dtype=torch.uint8)[start:stop].clone()
    try:
        with pytest.raises(hip_lib.HipLibraryError):
            gguf.load_state_dict(path, ops=Failing())
        got = gguf.load_state_dict(path, ops=Marking())
    finally:
        gguf._to_device_staged = staged
    want = gguf.load_state_dict(path)
    assert len(calls) == sum(1 for t in tiny_files["3b"][3].values() if t in gguf.QUANTISED) > 10
    assert set(got) == set(want) and all(same_bits(got[k], want[k]) for k in want)


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_dequant_entry_point_refuses_invalid_arguments_before_any_launch():
    """Null pointers, a type outside the four, a bad out_kind, block counts below one or beyond 2^40 elements, an out_bytes that is
    not exactly what the type and count need, misaligned pointers: refused on the host, the message names the argument."""
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 32
    p = ctypes.c_void_p(base)
    per = {8: 32, 12: 256, 13: 256, 14: 256}

    def call(blocks=p, ggml_type=12, n=2, out=p, kind=0, nbytes=None):
        need = n * per.get(ggml_type, 256) * (4 if kind == 1 else 2)
        return L.svr_dequant_gguf(blocks, ggml_type, n, out, kind, need if nbytes is None else nbytes, None)

    cases = [(lambda: call(blocks=None), b"blocks"), (lambda: call(out=None), b"out"),
             (lambda: call(ggml_type=0), b"ggml_type"), (lambda: call(ggml_type=2), b"ggml_type"), (lambda: call(ggml_type=30), b"ggml_type"),
             (lambda: call(ggml_type=-1), b"ggml_type"), (lambda: call(kind=2), b"out_kind"), (lambda: call(kind=-1), b"out_kind"),
             (lambda: call(n=0), b"n_blocks"), (lambda: call(n=-5), b"n_blocks"), (lambda: call(n=2 ** 32 + 1), b"2^40"),
             (lambda: call(ggml_type=8, n=2 ** 35 + 1), b"2^40"), (lambda: call(n=2 ** 62), b"2^40"),
             (lambda: call(nbytes=1023), b"out_bytes"), (lambda: call(nbytes=1025), b"out_bytes"), (lambda: call(nbytes=0), b"out_bytes"),
             (lambda: call(kind=1, nbytes=1024), b"out_bytes"), (lambda: call(ggml_type=8, nbytes=1024), b"out_bytes"),
             (lambda: call(blocks=ctypes.c_void_p(base + 16)), b"aligned"), (lambda: call(blocks=ctypes.c_void_p(base + 2)), b"aligned"),
             (lambda: call(out=ctypes.c_void_p(base + 8)), b"aligned"), (lambda: call(out=ctypes.c_void_p(base + 2)), b"aligned")]
    for i, (fn, word) in enumerate(cases):
        assert fn() != 0, i
        msg = L.svr_last_error()
        assert b"svr_dequant_gguf" in msg and word in msg, (i, msg)
    for i, (fn, _) in enumerate(cases[-4:]):                                      # and which pointer it was
        assert fn() != 0 and (b"blocks" if i < 2 else b"out") in L.svr_last_error()


def test_header_ctypes_table_and_build_list_know_the_entry_point():
    import re
    hip_lib, gguf = sub("hip_lib"), sub("gguf")
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M))
    assert "svr_dequant_gguf" in declared and "svr_dequant_gguf" in hip_lib.SYMBOLS
    assert len(hip_lib.SYMBOLS["svr_dequant_gguf"][1]) == 7
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9
    for name in NAMES:
        assert re.search(rf"#define SVR_GGML_{name}\s+{type_id(name)}\b", src), name
    assert '#include "svr_gguf.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert os.path.join(hip_lib.CSRC, "svr_gguf.hip") in hip_lib.sources()                   # the build id covers it
    assert {gguf.TYPES[t][0] for t in gguf.QUANTISED} == set(NAMES)
