"""Time the frame-unpack op (HipOps.unpack_frames, csrc/svr_frame_unpack.hip) at 720p, 1080p and 4K: per format, 3 warm-ups, then the
mean of 20 launches between HIP events, as bytes computed from the shapes over that time.  No threshold is attached to any figure.

Byte model per pixel: the packed samples read once (rgb8 / bgr8 3 B, rgb16 6 B, yuv420p8 1.5 B, yuv420p10 3 B) plus 12 B of fp32
RGB written.  (The yuv kernels read each chroma row for the two or three luma row pairs that interpolate with it; those re-reads
come from cache and are not in the model.)  The first run of a format also checks the result against the specification.

python tools/frame_unpack_timing.py [--frames 8] > profiles/frame_unpack_timing.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
SIZES = (("720p", 720, 1280), ("1080p", 1080, 1920), ("4K", 2160, 3840))


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
    ap.add_argument("--frames", type=int, default=8)
    args = ap.parse_args()
    ops_mod, fin = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "frameio_in"))
    ops = ops_mod.HipOps("cuda:0")
    T = args.frames
    print(f"# {ops.device_info}")
    print(f"# frame unpack, {T} frames per launch, C = 3, bt709 tv; 3 warm-ups, mean of 20 launches (HIP events)")
    print("# size   format      B/px read   ms/frame   ms/launch   GB/s (packed read + 12 B/px written)   equals the specification")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, H, W in SIZES:
        for fmt in fin.FORMATS:
            shape, dtype = fin.packed_shape(T, H, W, 3, fmt), fin.packed_dtype(fmt)
            top = 1024 if fmt == "yuv420p10" else 65536 if dtype == torch.uint16 else 256
            packed = torch.randint(0, top, shape, generator=g, device="cuda", dtype=torch.int32).to(dtype)
            out = torch.empty(T, H, W, 3, dtype=torch.float32, device="cuda")
            run = lambda: ops.unpack_frames(packed, fmt, T, H, W, 3, "bt709", "tv", out=out)
            same = torch.equal(run()[:1], fin.unpack_frames_torch(packed[:1], fmt, 1, H, W, 3, "bt709", "tv"))
            ms = timed(run)
            read = packed.numel() * packed.element_size()
            print(f"{name:6s} {fmt:11s} {read / (T * H * W):9.2f} {ms / T:10.4f} {ms:11.3f} {(read + out.numel() * 4) / (ms * 1e-3) / 1e9:14.1f}"
                  f"{'':28s}{'yes' if same else 'NO: RESULT DIFFERS FROM THE SPECIFICATION'}")
            del packed, out
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
