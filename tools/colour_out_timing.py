"""Time the yuv420p10 pack (csrc/svr_frame_pack_colour.hip) through its two entry points and in its variants, in one process on
one production batch: 17 frames of 3840 x 2160 fp32 RGB, the same input and output buffers for every variant.  The first row,
"pack_frames yuv420p10 (today)", is HipOps.pack_frames' "yuv420p10": it reaches the same kernel through svr_pack_frames, with
BT.709, limited range and centre siting.  (It had a kernel pair of its own, constants baked in, when the tool was written: the
rows up to the removal in profiles/colour_out_pack.txt compare two kernels, the later ones one kernel through two entry points.)
The second row, "pack_yuv420p10 bt709 tv center", is therefore the same launch through svr_pack_yuv420p10, and its ratio says what
the measurement cannot tell apart.  5 warm-ups per variant, then 15 rounds that alternate the variants, each timed as 10 launches
between HIP events; the median over the rounds and the spread (min .. max) are printed, and each variant's ratio to the first row
(the column still headed "today's kernel").  Every variant is first checked against its specification on one frame.

Byte model per pixel: 12 B read (fp32 RGB; 6 B for bf16), 3 B written (2 B of Y + 2 x 0.5 B of chroma); left siting reads one
pixel more per 16 (12 B / 16 px), from a line the neighbouring lane streams anyway.
python tools/colour_out_timing.py [--frames 17] [--height 2160] [--width 3840] [--dtype fp32|bf16] > profiles/colour_out_pack.txt"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ops_mod, frameio = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "frameio"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W = args.frames, args.height, args.width
    dt = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand(T, H, W, 3, generator=g, device="cuda") * 1.2 - 0.1).to(dt)
    out = torch.empty(frameio.packed_shape(T, H, W, 3, "yuv420p10"), dtype=torch.uint16, device="cuda")
    variants = [("pack_frames yuv420p10 (today)", lambda: ops.pack_frames(x, "yuv420p10", out=out),
                 lambda f: frameio.pack_frames_torch(f, "yuv420p10"))]
    for combo in (("bt709", "tv", "center"), ("bt2020", "tv", "center"), ("bt2020", "tv", "left"), ("bt2020", "pc", "left")):
        variants.append(("pack_yuv420p10 " + " ".join(combo), lambda c=combo: ops.pack_yuv420p10(x, *c, out=out),
                         lambda f, c=combo: frameio.pack_yuv420p10_torch(f, *c)))
    model = H * W * (3 * x.element_size() + 3)
    print(f"# {ops.device_info}")
    print(f"# yuv420p10 planes, {T} frames of {W} x {H} {args.dtype} RGB, the same buffers; 5 warm-ups per variant, then {args.rounds} rounds "
          f"alternating the variants, {args.reps} launches per timing (HIP events); median (min .. max) over the rounds")
    print(f"# byte model: {model / 1e6:.1f} MB per frame ({3 * x.element_size()} B read and 3 B written per pixel)")
    same = []
    for name, run, spec in variants:
        got = run()[:1].cpu()
        same.append(torch.equal(got.view(torch.int16), spec(x[:1].cpu()).view(torch.int16)))
        for _ in range(5):
            run()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(args.rounds):
        for k, (name, run, spec) in enumerate(variants):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                run()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) / args.reps)
    base = statistics.median(times[0])
    print("# variant                            ms/batch median (min .. max)   ms/frame   GB/s (byte model)   ratio to today's kernel")
    for (name, run, spec), t, ok in zip(variants, times, same):
        med = statistics.median(t)
        print(f"{name:34s} {med:8.3f} ({min(t):.3f} .. {max(t):.3f}) {med / T:10.4f} {model * T / (med * 1e-3) / 1e9:14.1f} {med / base:18.3f}"
              f"{'' if ok else '    RESULT DIFFERS FROM THE SPECIFICATION'}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
