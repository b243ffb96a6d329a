"""TEST INFRASTRUCTURE shared by tests/test_gguf.py and tests/test_gpu_gguf.py: random valid GGUF blocks, the recorded reference
results, and a tiny DiT checkpoint written as a GGUF file whose weights ARE the specification's values (no quantiser needed)."""
import os

import torch

from conftest import GOLDEN, sub

HALF_FIELDS = {8: (0,), 12: (0, 2), 13: (0, 2), 14: (208,)}          # byte offsets of the fp16 fields, by ggml type


def recorded():
    """name -> {"blocks": uint8 [75, type size], "fp32": the reference's own fp32 result} (tools/make_gguf_golden.py)"""
    return torch.load(os.path.join(GOLDEN, "recorded_gguf_dequant.pt"), weights_only=True)


def random_blocks(ggml_type, n, seed):
    """random bytes; an fp16 scale field that came out inf / NaN gets an exponent bit cleared: every scale finite"""
    gguf = sub("gguf")
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, 256, (n, gguf.TYPES[ggml_type][2]), generator=g, dtype=torch.int64).to(torch.uint8)
    for at in HALF_FIELDS[ggml_type]:
        hi = blocks[:, at + 1]
        blocks[:, at + 1] = torch.where((hi & 0x7C) == 0x7C, hi & 0xBF, hi)
    return blocks


def weight_blocks(ggml_type, n, seed):
    """random blocks with scales in a sane range: values of a few hundredths, like a trained layer's"""
    gguf = sub("gguf")
    blocks = random_blocks(ggml_type, n, seed)
    g = torch.Generator().manual_seed(seed + 1)
    u = torch.rand(n, generator=g) + 0.5
    d, dmin = {gguf.Q8_0: (5e-4, None), gguf.Q4_K: (1e-4, 7.5e-4), gguf.Q5_K: (5e-5, 7.5e-4), gguf.Q6_K: (3e-5, None)}[ggml_type]
    fields = HALF_FIELDS[ggml_type]
    blocks[:, fields[0]:fields[0] + 2] = (u * d).to(torch.float16).view(torch.uint8).reshape(n, 2)
    if dmin is not None:
        blocks[:, fields[1]:fields[1] + 2] = (u * dmin).to(torch.float16).view(torch.uint8).reshape(n, 2)
    return blocks


def tiny_dit_gguf(path, cfg, seed, prefix=""):
    """A DiT of ``cfg`` as a GGUF file with the mixture real files have: matrices whose input width is a multiple of 256 as
    Q4_K / Q5_K / Q6_K in rotation, a multiple of 32 as Q8_0, any other as F16; vectors (and the fp32 RoPE freqs) as F32.  The tiny
    configs have no width that is a multiple of 32 only (256, 1024, 5120 and the 132 of the patch embedding), so Q8_0 takes every
    fourth turn of the rotation as well: all four kernels see a real tensor.
    -> the state dict the file stands for, by the specification: quantised tensors dequantize_torch(blocks) as bf16, F16 / F32
    tensors in their own dtype -- and name -> ggml type."""
    gguf, weights = sub("gguf"), sub("weights")
    template = weights.synth_dit_state_dict(cfg, seed=seed)
    k_types = (gguf.Q4_K, gguf.Q5_K, gguf.Q6_K, gguf.Q8_0)
    tensors, want, turn = [], {}, 0
    for i, (name, v) in enumerate(template.items()):
        shape = tuple(v.shape)
        if v.dim() == 2 and shape[1] % 32 == 0:
            if shape[1] % 256 == 0:
                ggml_type, turn = k_types[turn % 4], turn + 1
            else:
                ggml_type = gguf.Q8_0
            blocks = weight_blocks(ggml_type, v.numel() // gguf.TYPES[ggml_type][1], seed=1000 * seed + i)
            tensors.append((prefix + name, ggml_type, shape, blocks))
            want[name] = gguf.dequantize_torch(blocks, ggml_type, torch.bfloat16).reshape(shape)
        elif v.dim() == 2:
            want[name] = v.to(torch.float16)
            tensors.append((prefix + name, gguf.F16, shape, want[name]))
        else:
            want[name] = v.float()
            tensors.append((prefix + name, gguf.F32, shape, want[name]))
    gguf.write_gguf(path, tensors, {"general.architecture": "seedvr2", "general.alignment": 32})
    return want, {t[0][len(prefix):]: t[1] for t in tensors}
