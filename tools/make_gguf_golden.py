"""Record the reference's own fp32 GGUF dequantisation: tests/golden/recorded_gguf_dequant.pt (build machine only: needs the
reference checkout).  Per type (Q8_0, Q4_K, Q5_K, Q6_K) 75 blocks, uint8 [75, type size], and the fp32 result of the reference's
``dequantize_blocks_<T>(blocks, block size, type size, torch.float32)`` (src/optimization/gguf_dequant.py), obtained with
oracle.reference_loader._extract -- the unmodified function text, run; nothing of it is stored.

Blocks: random bytes with the fp16 scale fields forced finite; blocks whose scale is +0, -0, the smallest fp16 subnormal, the largest
finite fp16 and a negative value; for the K types one block with every six-bit scale and min at 63 and one with all at 0; for Q6_K
sub-scales -128 and 127.    python tools/make_gguf_golden.py"""
import importlib
import os
import sys
import typing

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
OUT = os.path.join(ROOT, "tests", "golden", "recorded_gguf_dequant.pt")
N_BLOCKS = 75
SPECIAL_HALVES = (0x0000, 0x8000, 0x0001, 0x7BFF, 0xC2A0)       # +0, -0, smallest subnormal, largest finite, -3.3125


def half_fields(ggml_type, gguf):
    """byte offsets of the fp16 fields of a block"""
    return {gguf.Q8_0: (0,), gguf.Q4_K: (0, 2), gguf.Q5_K: (0, 2), gguf.Q6_K: (208,)}[ggml_type]


def force_finite(blocks, fields):
    """an fp16 whose exponent is all ones (inf / NaN) gets exponent bit 14 cleared: every field finite, everything else random"""
    for at in fields:
        hi = blocks[:, at + 1]
        bad = (hi & 0x7C) == 0x7C
        blocks[:, at + 1] = torch.where(bad, hi & 0xBF, hi)
    return blocks


def set_half(blocks, row, at, bits):
    blocks[row, at], blocks[row, at + 1] = bits & 0xFF, bits >> 8


def make_blocks(ggml_type, gguf, seed):
    size = gguf.TYPES[ggml_type][2]
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, 256, (N_BLOCKS, size), generator=g, dtype=torch.int64).to(torch.uint8)
    fields = half_fields(ggml_type, gguf)
    force_finite(blocks, fields)
    row = 0
    for bits in SPECIAL_HALVES:                                  # every scale field of the block takes the special value
        for at in fields:
            set_half(blocks, row, at, bits)
        row += 1
    if len(fields) == 2:                                         # d special, dmin random and the other way round
        for bits in SPECIAL_HALVES:
            set_half(blocks, row, fields[0], bits)
            set_half(blocks, row + 1, fields[1], bits)
            row += 2
    if ggml_type in (gguf.Q4_K, gguf.Q5_K):
        blocks[row, 4:16] = 0xFF                                 # all six-bit scales and mins 63
        blocks[row + 1, 4:16] = 0
        row += 2
    if ggml_type == gguf.Q6_K:
        blocks[row, 192:208] = 0x80                              # -128
        blocks[row + 1, 192:208] = 0x7F                          # 127
        blocks[row + 2, 192:208] = torch.tensor([0x80, 0x7F] * 8, dtype=torch.uint8)
        row += 3
    assert row <= N_BLOCKS
    return blocks


def reference_functions():
    from oracle import reference_loader as rl
    if not rl.available():
        raise SystemExit("the reference checkout is not available here")
    ns = {"torch": torch, "QK_K": 256, "K_SCALE_SIZE": 12, "Optional": typing.Optional, "Tuple": typing.Tuple, "List": typing.List}
    rl._extract("src/optimization/gguf_dequant.py",
                ["to_uint32", "split_block_dims", "get_scale_min", "dequantize_blocks_Q8_0", "dequantize_blocks_Q4_K",
                 "dequantize_blocks_Q5_K", "dequantize_blocks_Q6_K"], ns)
    return ns


def main():
    gguf = importlib.import_module(f"{PKG}.gguf")
    ns = reference_functions()
    table = {}
    for i, ggml_type in enumerate(gguf.QUANTISED):
        name, per, size, _ = gguf.TYPES[ggml_type]
        blocks = make_blocks(ggml_type, gguf, seed=100 + i)
        want = ns[f"dequantize_blocks_{name}"](blocks.clone(), per, size, torch.float32)
        assert want.dtype == torch.float32 and tuple(want.shape) == (N_BLOCKS, per) and bool(torch.isfinite(want).all()), name
        table[name] = {"blocks": blocks, "fp32": want.contiguous().clone()}
        print(f"{name}: {N_BLOCKS} blocks of {size} bytes -> fp32 {tuple(want.shape)}, |x| up to {float(want.abs().max()):.4g}")
    torch.save(table, OUT)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
