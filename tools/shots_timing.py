"""Time the frame-signature op (HipOps.frame_signatures, csrc/svr_shots.hip) on one chunk of the streaming workload -- 33 frames of
1280 x 720, fp32, C = 3 -- against its torch statement (shots.signatures_torch) on the same device tensor and against one plain
read of the chunk (a ``sum``): the floor any pass over the frames has.  Each of the three is taken twice, alternating (kernel,
torch, sum, kernel, torch, sum), 3 warm-ups and then enough launches between HIP events to fill about half a second; the bf16 chunk
and a flat (all-black) chunk, the kernel's contention case, follow.  The first run also checks the kernel against the statement.
No threshold is attached to any figure.

python tools/shots_timing.py [--frames 33] > profiles/shots.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"


def timed(fn, warmup=3, window_ms=500.0):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    reps = max(5, min(2000, int(window_ms / max(s.elapsed_time(e), 1e-3))))
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    args = ap.parse_args()
    ops_mod, shots = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "shots"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W = args.frames, args.height, args.width
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(T, H, W, 3, generator=g, device="cuda")
    out = torch.empty(T, 1024, dtype=torch.int32, device="cuda")
    same = torch.equal(ops.frame_signatures(x, out=out), shots.signatures_torch(x))
    print(f"# {ops.device_info}")
    print(f"# frame signatures of one chunk: {T} frames of {W} x {H}, C = 3; 3 warm-ups, mean over ~0.5 s of launches (HIP events)")
    print(f"# kernel equals the specification on this chunk: {'yes' if same else 'NO: RESULT DIFFERS FROM THE SPECIFICATION'}")
    print("# what                          dtype   pass   launches   ms/chunk   us/frame   GB/s of frames read")
    legs = (("kernel (svr_frame_signatures)", lambda t: ops.frame_signatures(t, out=out)),
            ("torch (signatures_torch)", shots.signatures_torch),
            ("plain read (sum)", lambda t: t.sum()))

    def table(t, label, legs_):
        nbytes = t.numel() * t.element_size()
        for rnd in (1, 2):
            for name, fn in legs_:
                ms, reps = timed(lambda: fn(t))
                print(f"{name:30s} {label:6s} {rnd:5d} {reps:10d} {ms:10.3f} {ms * 1e3 / T:10.2f} {nbytes / (ms * 1e-3) / 1e9:12.1f}")

    table(x, "fp32", legs)
    table(x.to(torch.bfloat16), "bf16", legs)
    flat = torch.zeros_like(x)
    print("# a flat (black) chunk: every lane of a wave on one counter")
    table(flat, "fp32", legs[:1] + legs[2:])
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
