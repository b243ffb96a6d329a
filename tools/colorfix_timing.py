"""Time colour correction (phase 4 of pipeline.upscale) on a 17-frame 4K span: per method, colorfix.correct on the kernels
(csrc/svr_colorfix.hip through HipOps) and with impl="torch" -- colorfix.METHODS, the code of before -- in the same process, on the
pipeline's own layouts: the decoded frames channels-last ([T, H, W, 3] fp32, as ``final[w0:w1]``), the reference a [:, :, :H, :W]
slice of a [C, T, H', W'] buffer.  HIP events around each call after a warm-up; peak allocated memory above the operands for both
routes, and how far the two routes' results lie apart at that size (wavelet: 0, the same bits; the rank-matching methods exchange
the matched values of near-tied pixels).  No threshold is attached to any figure.

Byte model, printed next to the times: one pass over a span is T * H * W * 3 * 4 bytes (1.69 GB at 17 x 2160 x 3840).  The wavelet
launch ideally reads content and style and writes the result once: 3 passes.  The torch route makes on the order of sixty (two
operands x five levels x about six elementwise / index kernels, each reading and writing a span).  lab_planes reads 2 and writes 2
passes, lab_merge reads 4/3 and writes 1, AdaIN reads content twice and style once and writes once; the sorts of the rank matching
are torch's on both routes.

python tools/colorfix_timing.py [--frames 17] [--height 2160] [--width 3840] [--reps 5] > profiles/colorfix.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
METHODS = ("wavelet", "adain", "lab", "wavelet_adaptive")


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--methods", default=",".join(METHODS))
    args = ap.parse_args()
    ops_mod, cf = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "colorfix"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W = args.frames, args.height, args.width
    g = torch.Generator(device="cuda").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(float(H), device="cuda"), torch.arange(float(W), device="cuda"), indexing="ij")
    smooth = (0.4 * torch.sin(xx / 37) + 0.3 * torch.cos(yy / 23))[None, ..., None]
    tint = torch.tensor([0.10, -0.05, 0.02], device="cuda")
    frames = (smooth + tint + torch.randn(T, H, W, 3, generator=g, device="cuda") * 0.05).clamp_(-1, 1).contiguous()
    big = torch.empty(3, T, H + 8, W + 8, device="cuda")
    big[:, :, :H, :W] = (smooth * 0.8 - tint + torch.randn(T, H, W, 3, generator=g, device="cuda") * 0.02).clamp_(-1, 1).permute(3, 0, 1, 2)
    content, style = frames.permute(0, 3, 1, 2), big.permute(1, 0, 2, 3)[:, :, :H, :W]
    del smooth, yy, xx
    span = T * H * W * 3 * 4
    print(f"# {ops.device_info}")
    print(f"# span {T} x {H} x {W} x 3 fp32 = {span / 1e9:.2f} GB per pass; {args.warmup} warm-up, mean of {args.reps} calls between HIP events")
    print(f"# byte model: wavelet launch 3 passes = {3 * span / 1e9:.2f} GB (ideal); torch wavelet about 60 passes = {60 * span / 1e9:.0f} GB")
    print(f"{'method':18s} {'kernels ms':>11s} {'torch ms':>10s} {'ratio':>7s} {'kernels peak GB':>16s} {'torch peak GB':>14s}"
          f" {'max |k - t|':>12s} {'share > 2e-5':>13s}")
    for m in args.methods.split(","):
        assert cf.routes_to_device(content, style, m, ops), m
        dev = lambda: cf.correct(content, style, m, ops=ops)
        ref = lambda: cf.correct(content, style, m, ops=ops, impl="torch")
        t_dev, t_ref = timed(dev, args.warmup, args.reps), timed(ref, args.warmup, args.reps)
        p_dev, p_ref = peak_above(dev), peak_above(ref)
        d = (dev() - ref()).abs_()                                 # the two routes' results at the size timed
        print(f"{m:18s} {t_dev:11.2f} {t_ref:10.2f} {t_ref / t_dev:7.2f} {p_dev / 1e9:16.2f} {p_ref / 1e9:14.2f}"
              f" {float(d.max()):12.3e} {float((d > 2e-5).float().mean()):13.3e}")
        del d
    # the launches on their own
    base = ops.wavelet_reconstruct(content, style)
    t_w = timed(lambda: ops.wavelet_reconstruct(content, style, out=base), args.warmup, args.reps)
    planes = ops.lab_planes(base, style)
    t_p = timed(lambda: ops.lab_planes(base, style, c_lab=planes[0], s_lab=planes[1]), args.warmup, args.reps)
    c_lab = planes[0]
    t_m = timed(lambda: ops.lab_merge(c_lab[0], c_lab[0], c_lab[1], c_lab[2], 0.8, (T, H, W), out=base), args.warmup, args.reps)
    t_s = timed(lambda: ops.chan_stats(content, style), args.warmup, args.reps)
    t_a = timed(lambda: ops.adain(content, style, out=base), args.warmup, args.reps)
    for name, ms, passes in (("svr_wavelet_reconstruct", t_w, 3), ("svr_lab_planes", t_p, 4), ("svr_lab_merge", t_m, 4 / 3 + 1),
                             ("svr_chan_stats", t_s, 2), ("svr_chan_stats + svr_adain_apply", t_a, 4)):
        print(f"# {name:34s} {ms:8.2f} ms  model {passes * span / 1e9:5.2f} GB -> {passes * span / ms / 1e9:7.2f} TB/s of the model's bytes")


if __name__ == "__main__":
    main()
