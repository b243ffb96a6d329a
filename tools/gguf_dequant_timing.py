"""Time the GGUF expansion (HipOps.dequant_gguf, csrc/svr_gguf.hip) per type at the block count of the largest production matrix:
the 3B MLP input weight [6912, 2560] (--7b: the 7B one, [12288, 3072]), bf16 output.  Next to it gguf.dequantize_torch on the same
device: the reference's algorithm the way the reference runs it on a GPU (a chain of torch ops per tensor).  Bit equality of the two
is asserted first.  3 warm-ups, then the mean of --reps launches between HIP events; bytes = blocks read + bf16 written.

The working set of one matrix (3B: 10-15 MB of blocks + 35 MB of bf16) fits the 256 MiB last-level cache, so repeated launches on
the same buffers can run above the HBM rate; --rotate N gives every launch one of N buffer pairs (default: enough pairs to exceed
512 MiB), which is what a checkpoint load looks like: every byte is touched once.
python tools/gguf_dequant_timing.py [--7b] [--reps 2000] > profiles/gguf_dequant.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"


def timed(fn, warmup=3, reps=2000):
    for i in range(warmup):
        fn(i)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(reps):
        fn(i)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def finite_blocks(n, size, fields, seed):
    """random bytes on the device, every fp16 scale field finite"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    blocks = torch.randint(0, 256, (n, size), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    for at in fields:
        hi = blocks[:, at + 1]
        blocks[:, at + 1] = torch.where((hi & 0x7C) == 0x7C, hi & 0xBF, hi)
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--7b", dest="big", action="store_true", help="the 7B MLP input weight instead of the 3B one")
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rotate", type=int, default=0, help="buffer pairs to cycle through (0: enough to exceed 512 MiB)")
    args = ap.parse_args()
    ops_mod, gguf, config = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "gguf", "config"))
    ops = ops_mod.HipOps("cuda:0")
    cfg = config.DIT_7B if args.big else config.DIT_3B
    rows, cols = cfg.mlp_hidden, cfg.vid_dim
    fields = {gguf.Q8_0: (0,), gguf.Q4_K: (0, 2), gguf.Q5_K: (0, 2), gguf.Q6_K: (208,)}
    print(f"# {ops.device_info}")
    print(f"# GGUF expansion to bf16, the {'7B' if args.big else '3B'} MLP input weight [{rows}, {cols}] = {rows * cols} elements; "
          f"3 warm-ups, mean of {args.reps} launches (HIP events)")
    print("# bytes = blocks read + bf16 written; 'rotating': every launch on another buffer pair (working set > 512 MiB, the last-level")
    print("# cache holds 256 MiB); 'resident': every launch on the same pair (one matrix: served from the last-level cache)")
    print("# type   blocks   MB moved   kernel ms rotating   GB/s   kernel ms resident   GB/s   torch ms   torch / kernel   equal")
    for ggml_type in gguf.QUANTISED:
        name, per, size, _ = gguf.TYPES[ggml_type]
        n = rows * cols // per
        moved = n * (size + 2 * per)
        pairs = args.rotate or (512 << 20) // moved + 2
        src = [finite_blocks(n, size, fields[ggml_type], seed=ggml_type + 100 * k) for k in range(pairs)]
        dst = [torch.empty(n, per, dtype=torch.bfloat16, device="cuda") for _ in range(pairs)]
        same = torch.equal(ops.dequant_gguf(src[0], ggml_type, out=dst[0]).view(torch.int16),
                           gguf.dequantize_torch(src[0], ggml_type, torch.bfloat16).view(torch.int16))
        assert same, f"{name}: the kernel's result differs from gguf.dequantize_torch"
        rot = timed(lambda i: ops.dequant_gguf(src[i % pairs], ggml_type, out=dst[i % pairs]), reps=args.reps)
        res = timed(lambda i: ops.dequant_gguf(src[0], ggml_type, out=dst[0]), reps=args.reps)
        ref = timed(lambda i: gguf.dequantize_torch(src[i % pairs], ggml_type, torch.bfloat16), reps=max(args.reps // 5, 5))
        print(f"{name:6s} {n:8d} {moved / 1e6:9.1f} {rot:17.4f} {moved / (rot * 1e-3) / 1e9:10.1f} {res:17.4f} "
              f"{moved / (res * 1e-3) / 1e9:10.1f} {ref:10.3f} {ref / rot:13.1f}x   {'yes' if same else 'NO'}")
        del src, dst
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
