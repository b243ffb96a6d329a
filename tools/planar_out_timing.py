"""Time the planar output pack (HipOps.pack_planar: csrc/svr_planar_out.hip) and the device -> pinned-host copy of its result, in one
process on one production chunk: 17 frames of 3840 x 2160 fp32 RGB, the same input for every variant.  One row per (sub, bits) with
siting "left", plus 4:2:0 "topleft" at each depth (the third row of loads), all BT.709 tv (matrix, range and depth are integers to the
kernels, not instances).  The yardsticks run in the same rounds: HipOps.pack_frames "bgr8" (what the 8-bit ffmpeg route hands over
today) and HipOps.pack_yuv420p10 bt709 tv "left" (the kernel the 4:2:0 10-bit "left" instance restates), each with its copy.

5 warm-ups per variant, then --rounds rounds that alternate the variants; in a round a variant's pack is timed as --reps launches
between HIP events and its copy as --reps copies into the same pinned buffer.  Printed: the median over the rounds and the spread
(min .. max) of both, the bytes that cross PCIe per frame, the pack's GB/s against its byte model (input read once + result written)
and its ratio to each yardstick.  Every variant is first checked against its specification on a crop of two frames.  The last lines put the
4:2:0 10-bit "left" instance next to pack_yuv420p10 "left" with the run-to-run spread of the yardstick.
python tools/planar_out_timing.py [--frames 17] [--height 2160] [--width 3840] [--dtype fp32|bf16] > profiles/planar_out.txt"""
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ops_mod, frameio, planar, planar_out = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "frameio", "planar", "planar_out"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W = args.frames, args.height, args.width
    dt = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand(T, H, W, 3, generator=g, device="cuda") * 1.2 - 0.1).to(dt)

    # one device buffer and one pinned host buffer, as large as the largest result (4:4:4 in uint16): every variant packs into a view
    # of the first and is copied into a view of the second
    most = T * H * W * 3 * 2
    device_bytes, host_bytes = torch.empty(most, dtype=torch.uint8, device="cuda"), torch.empty(most, dtype=torch.uint8, pin_memory=True)

    def variant(name, shape, dtype, run, spec):
        n = torch.Size(shape).numel() * torch.empty(0, dtype=dtype).element_size()
        out, host = device_bytes[:n].view(dtype).view(shape), host_bytes[:n].view(dtype).view(shape)
        return dict(name=name, out=out, host=host, run=lambda: run(x, out), small=lambda f: run(f, None), spec=spec, pack=[], copy=[])

    variants = [variant("pack_frames bgr8 (today, 8 bits)", (T, H, W, 3), torch.uint8, lambda f, o: ops.pack_frames(f, "bgr8", out=o),
                        lambda f: frameio.pack_frames_torch(f, "bgr8")),
                variant("pack_yuv420p10 bt709 tv left", frameio.packed_shape(T, H, W, 3, "yuv420p10"), torch.uint16,
                        lambda f, o: ops.pack_yuv420p10(f, "bt709", "tv", "left", out=o), lambda f: frameio.pack_yuv420p10_torch(f, "bt709", "tv", "left"))]
    for sub, bits, siting in [(s, b, "left") for s in planar.SUBS for b in planar.BITS] + [("420", b, "topleft") for b in planar.BITS]:
        variants.append(variant(f"pack_planar {sub} {bits:2d} {siting}", planar.planar_shape(T, H, W, sub), planar.planar_dtype(bits),
                                lambda f, o, a=(sub, bits, "bt709", "tv", siting): ops.pack_planar(f, *a, out=o),
                                lambda f, a=(sub, bits, "bt709", "tv", siting): planar_out.pack_planar_torch(f, *a)))
    print(f"# {ops.device_info}")
    print(f"# {T} frames of {W} x {H} {args.dtype} RGB, one input; 5 warm-ups per variant, then {args.rounds} rounds alternating the variants, "
          f"{args.reps} launches and {args.reps} device -> pinned-host copies per timing (HIP events); median (min .. max) over the rounds")
    for v in variants:
        crop = x[:2, :66, :160].contiguous()                         # (the specification on the host: a crop, its own launch)
        got, want = v["small"](crop).cpu(), v["spec"](crop.cpu())
        as_int = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t
        v["ok"] = torch.equal(as_int(got), as_int(want))
        for _ in range(5):
            v["run"]()
            v["host"].copy_(v["out"])
    torch.cuda.synchronize()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.reps):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / args.reps

    for _ in range(args.rounds):
        for v in variants:
            v["pack"].append(timed(v["run"]))
            v["copy"].append(timed(lambda: v["host"].copy_(v["out"], non_blocking=True)))
    med = lambda t: statistics.median(t)
    bgr, yuv = med(variants[0]["pack"]), med(variants[1]["pack"])
    print("# variant                            pack ms/chunk median (min .. max)   copy ms/chunk median (min .. max)   MB/frame out"
          "   pack GB/s   pack+copy ms   pack / bgr8   pack / yuv420p10")
    for v in variants:
        p, c = v["pack"], v["copy"]
        nbytes = v["out"].numel() * v["out"].element_size()
        model = x.numel() * x.element_size() + nbytes
        print(f"{v['name']:34s} {med(p):8.3f} ({min(p):.3f} .. {max(p):.3f})   {med(c):16.3f} ({min(c):.3f} .. {max(c):.3f}) {nbytes / T / 1e6:14.2f}"
              f" {model / (med(p) * 1e-3) / 1e9:11.1f} {med(p) + med(c):14.3f} {med(p) / bgr:13.3f} {med(p) / yuv:18.3f}"
              f"{'' if v['ok'] else '    RESULT DIFFERS FROM THE SPECIFICATION'}")
    mine = next(v for v in variants if v["name"] == "pack_planar 420 10 left")["pack"]
    ref = variants[1]["pack"]
    spread = (max(ref) - min(ref)) / med(ref)
    print(f"# pack_planar 420 10 left against pack_yuv420p10 left: {med(mine):.3f} ms against {med(ref):.3f} ms, ratio {med(mine) / med(ref):.3f}; "
          f"the yardstick's run-to-run spread (max - min over the rounds) is {100 * spread:.1f} % of its median")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
