"""Time the deinterlacing op (HipOps.deinterlace, csrc/svr_deinterlace.hip) next to the unpack it precedes, on one chunk of the
streaming workload: 17 woven frames of 1920 x 1080 in field rate -> 34 progressive frames, then HipOps.unpack_frames of those 34,
for yuv420p8 and for rgb16, and one plain device copy of the 34 packed frames as the floor.  Random samples over the whole code
range: every edge search takes its own way, the worst case for a wave's branches.  10 warm-ups, then five windows of about half a
second of back-to-back launches each between HIP events: the windows show the spread.  The first two frames of each chunk are
checked against the specification first (the whole chunk through the torch statement on the CPU would take minutes).  No threshold
is attached to any figure.

Bytes: "unique" counts every input byte once and every output byte once; "issued" counts the loads and stores the kernel makes (a
kept row 1 load + 1 store per sample, a computed row 8 loads + 1 store; the search's neighbours come from lines already loaded).

python tools/deinterlace_timing.py [--frames 17] > profiles/deinterlace.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
WARMUP, WINDOWS, WINDOW_MS = 10, 5, 500.0


def timed(fn):
    for _ in range(WARMUP):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    reps = max(10, min(5000, int(WINDOW_MS / max(s.elapsed_time(e), 1e-3))))
    out = []
    for _ in range(WINDOWS):
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        out.append((reps, s.elapsed_time(e) / reps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    ops_mod, de, fin = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "deinterlace", "frameio_in"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W, C = args.frames, args.height, args.width, 3
    print(f"# {ops.device_info}")
    print(f"# one chunk: {T} woven frames of {W} x {H} -> {2 * T} progressive frames (order tff, rate field, no context frames), then "
          f"unpack_frames of those {2 * T}; {WARMUP} warm-ups, {WINDOWS} windows of ~{WINDOW_MS / 1000:g} s of launches each (HIP events)")
    print("# what                           fmt        window   launches   ms/launch   unique MB   GB/s unique   issued MB   GB/s issued")
    g = torch.Generator(device="cuda").manual_seed(0)
    for fmt in ("yuv420p8", "rgb16"):
        dtype = fin.packed_dtype(fmt)
        shape = fin.packed_shape(T, H, W, C, fmt)
        if dtype == torch.uint8:
            packed = torch.randint(0, 256, shape, generator=g, device="cuda", dtype=torch.uint8)
        else:                                                                   # (every 16-bit pattern, drawn as int16)
            packed = torch.randint(-32768, 32768, shape, generator=g, device="cuda", dtype=torch.int16).view(torch.uint16)
        frame = packed.numel() // T * packed.element_size()                     # bytes
        out = torch.empty((2 * T,) + tuple(packed.shape[1:]), dtype=dtype, device="cuda")
        fp32 = torch.empty((2 * T, H, W, C), dtype=torch.float32, device="cuda")
        small = packed[:2].contiguous()
        same = torch.equal(ops.deinterlace(small, fmt, 2, H, W, C, "tff", "field").cpu(),
                           de.deinterlace_torch(small.cpu(), fmt, 2, H, W, C, "tff", "field"))
        print(f"# {fmt}: kernel equals the specification on the chunk's first two frames: "
              f"{'yes' if same else 'NO: RESULT DIFFERS FROM THE SPECIFICATION'}")
        flat_in, flat_out = out.view(torch.uint8).reshape(-1), fp32.view(torch.uint8).reshape(-1)[:2 * T * frame]
        legs = (("deinterlace (svr_deinterlace)", lambda: ops.deinterlace(packed, fmt, T, H, W, C, "tff", "field", out=out),
                 3 * T * frame, 2 * T * frame * 5.5),
                (f"unpack_frames ({2 * T} frames)", lambda: ops.unpack_frames(out, fmt, 2 * T, H, W, C, out=fp32),
                 2 * T * frame + fp32.numel() * 4, None),
                (f"plain copy ({2 * T} packed frames)", lambda: flat_out.copy_(flat_in), 2 * 2 * T * frame, None))
        for name, fn, unique, issued in legs:
            for w, (reps, ms) in enumerate(timed(fn)):
                tail = f"{issued / 1e6:11.1f} {issued / ms / 1e6:13.1f}" if issued else f"{'-':>11} {'-':>13}"
                print(f"{name:32s} {fmt:10s} {w + 1:6d} {reps:10d} {ms:11.4f} {unique / 1e6:11.1f} {unique / ms / 1e6:13.1f} {tail}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
