"""Time the planar route (HipOps.planar_codes, csrc/svr_planar.hip) next to the route the same source takes today, ALL IN THE SAME RUN,
on one chunk of the streaming workload: 17 frames of 1920 x 1080, for yuv422p10 BT.709 and for yuv420p10 BT.2020 "topleft".

  new route      h2d (planes)        the pinned planar bytes copied to the device: 4 bytes a pixel for 4:2:2, 3 for 4:2:0
                 planar_codes        planes -> rgb16 codes
                 unpack_frames       HipOps.unpack_frames("rgb16") of the codes
  today's route  h2d (rgb48le)       the same chunk as the rgb48le bytes ffmpeg's swscale would have made: 6 bytes a pixel
                 unpack_frames       HipOps.unpack_frames("rgb16") of them (the same launch as above: timed once more, on these bytes)

What swscale costs the host on today's route -- the conversion this route moves to the device -- is NOT measured here: the tool
starts no decoder.  10 warm-ups, then five windows of about half a second of back-to-back operations each between HIP events: the
windows show the spread.  The kernel is checked against the specification first.  No threshold is attached to any figure.
Bytes: "moved" counts every input byte once and every output byte once; "issued" counts the loads and stores the kernel makes
(planar_codes 4:2:0 "topleft": each chroma row is loaded by the unit of its own two luma rows and by the unit above; the seam
neighbours are not counted).

python tools/planar_timing.py > profiles/planar.txt"""
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
    sub = lambda m: importlib.import_module(f"{PKG}.{m}")
    planar = sub("planar")
    ops = sub("ops").HipOps("cuda:0")
    T, H, W = args.frames, args.height, args.width
    px = T * H * W
    print(f"# {ops.device_info}")
    print(f"# one chunk: {T} frames of {W} x {H}; pinned host buffers, copies and launches on the current stream; {WARMUP} warm-ups, "
          f"{WINDOWS} windows of ~{WINDOW_MS / 1000:g} s of operations each (HIP events), every leg in this one run")
    print("# swscale's host-side cost on today's route: not measured (no decoder runs here)")
    print("# source                    leg                            window   launches   ms/launch    moved MB   GB/s moved   issued MB   GB/s issued")
    g = torch.Generator().manual_seed(0)
    for name, sub_, bits, matrix, siting in (("yuv422p10 bt709", "422", 10, "bt709", "left"), ("yuv420p10 bt2020 topleft", "420", 10, "bt2020", "topleft")):
        shape = planar.planar_shape(T, H, W, sub_)
        host = torch.randint(0, 1 << bits, shape, generator=g).to(torch.int32).to(torch.uint16).pin_memory()
        dev = torch.empty_like(host, device="cuda")
        codes = torch.empty((T, H, W, 3), dtype=torch.uint16, device="cuda")
        fp32 = torch.empty((T, H, W, 3), dtype=torch.float32, device="cuda")
        dev.copy_(host, non_blocking=True)
        ops.planar_codes(dev, sub_, bits, T, H, W, matrix, "tv", siting, out=codes)
        same = torch.equal(codes[:2].cpu(), planar.planar_codes_torch(host[:2], sub_, bits, 2, H, W, matrix, "tv", siting))
        print(f"# {name}: the kernel equals the specification on the chunk's first two frames: "
              f"{'yes' if same else 'NO: RESULT DIFFERS FROM THE SPECIFICATION'}")
        host48 = codes.cpu().pin_memory()                                        # today's bytes across the pipe: rgb48le
        dev48 = torch.empty_like(codes)
        n_in = host.numel() * 2
        hc, wc = planar.chroma_dims(sub_, H, W)
        issued = T * (H * W + (4 if sub_ == "420" else 2) * hc * wc) * 2 + px * 6
        legs = (("new: h2d (planes)", lambda: dev.copy_(host, non_blocking=True), n_in, None),
                ("new: planar_codes", lambda: ops.planar_codes(dev, sub_, bits, T, H, W, matrix, "tv", siting, out=codes), n_in + px * 6, issued),
                ("new: unpack_frames (rgb16)", lambda: ops.unpack_frames(codes, "rgb16", T, H, W, 3, out=fp32), px * 6 + px * 12, None),
                ("today: h2d (rgb48le)", lambda: dev48.copy_(host48, non_blocking=True), px * 6, None),
                ("today: unpack_frames (rgb16)", lambda: ops.unpack_frames(dev48, "rgb16", T, H, W, 3, out=fp32), px * 6 + px * 12, None))
        means = {}
        for leg, fn, moved, iss in legs:
            windows = timed(fn)
            means[leg] = sum(ms for _, ms in windows) / len(windows)
            for w, (reps, ms) in enumerate(windows):
                tail = f"{iss / 1e6:11.1f} {iss / ms / 1e6:13.1f}" if iss else f"{'-':>11} {'-':>13}"
                print(f"{name:25s} {leg:30s} {w + 1:6d} {reps:10d} {ms:11.4f} {moved / 1e6:11.1f} {moved / ms / 1e6:12.1f} {tail}")
        new = sum(v for k, v in means.items() if k.startswith("new"))
        today = sum(v for k, v in means.items() if k.startswith("today"))
        print(f"# {name}: mean ms per chunk, new route (copy + planar_codes + unpack) {new:.3f}, today's route (copy + unpack) {today:.3f}; "
              f"bytes across PCIe {n_in / 1e6:.1f} MB against {px * 6 / 1e6:.1f} MB ({n_in / px:.2f} against 6 bytes a pixel)")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
