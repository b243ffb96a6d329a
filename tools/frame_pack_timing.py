"""Time the frame-pack op (HipOps.pack_frames: csrc/svr_frame_pack.hip for rgb8 / bgr8, csrc/svr_frame_pack_colour.hip with the
BT.709 limited-range constants for yuv420p10) on one production batch: 17 frames of 3840 x 2160 fp32 RGB.
3 warm-ups, then the mean of 20 launches between HIP events, per format, next to the torch expression for the same conversion on
the same device: for rgb8 the expression inference_cli.save_frames ran on the device before the formats had a kernel,
``(x.float().clamp(0, 1) * 255.0).round().to(torch.uint8)``; for bgr8 the same followed by the channel flip (done on the host
then); for yuv420p10, which had no predecessor, frameio.pack_frames_torch -- the specification itself.

Byte model per pixel: 12 B read (fp32 RGB; 6 B for bf16), 3 B written (8-bit formats and yuv420p10 alike: 2 B of Y + 2 x 0.5 B of
chroma).  python tools/frame_pack_timing.py [--frames 17] [--height 2160] [--width 3840] [--dtype fp32|bf16] > profiles/frame_pack_4k.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"


def timed(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    args = ap.parse_args()
    ops_mod, frameio = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "frameio"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W = args.frames, args.height, args.width
    dt = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand(T, H, W, 3, generator=g, device="cuda") * 1.2 - 0.1).to(dt)
    host8 = lambda: (x.float().clamp(0, 1) * 255.0).round().to(torch.uint8)
    torch_expr = {"rgb8": ("the writers' expression", host8), "bgr8": ("the writers' expression + flip", lambda: host8().flip(-1)),
                  "yuv420p10": ("frameio.pack_frames_torch", lambda: frameio.pack_frames_torch(x, "yuv420p10"))}
    model = H * W * (3 * x.element_size() + 3)
    print(f"# {ops.device_info}")
    print(f"# frame pack, {T} frames of {W} x {H} {args.dtype} RGB; 3 warm-ups, mean of 20 launches (HIP events)")
    print(f"# byte model: {model / 1e6:.1f} MB per frame ({3 * x.element_size()} B read and 3 B written per pixel)")
    print("# format      kernel ms/frame   ms/batch   GB/s (byte model)   torch ms/frame   torch / kernel   torch expression")
    for fmt in frameio.FORMATS:
        out = torch.empty(frameio.packed_shape(T, H, W, 3, fmt), dtype=frameio.packed_dtype(fmt), device="cuda")
        same = torch.equal(ops.pack_frames(x, fmt, out=out).view(torch.uint8), frameio.pack_frames_torch(x, fmt).view(torch.uint8))
        ms = timed(lambda: ops.pack_frames(x, fmt, out=out))
        name, fn = torch_expr[fmt]
        ref = timed(fn)
        print(f"{fmt:11s} {ms / T:14.4f} {ms:12.3f} {model * T / (ms * 1e-3) / 1e9:14.1f} {ref / T:18.4f} {ref / ms:14.1f}x    {name}"
              f"{'' if same else '    RESULT DIFFERS FROM THE SPECIFICATION'}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
