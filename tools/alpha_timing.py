"""Time the alpha op (HipOps.alpha_upscale, csrc/svr_alpha.hip) on one production batch: 17 frames of 3840 x 2160 fp32 RGB, the
alpha of a 1280 x 720 input.  3 warm-ups, then 20 launches between HIP events, for the whole op and for each of its parts (the
bicubic base -- torch glue --, svr_alpha_stats, svr_alpha_edges, svr_alpha_refine), for a binary and for a soft matte.

Byte model per frame (fp32 RGB, 8.3 Mpixel): RGB read twice (edges, refine: 2 x 99.5 MB), the n map written and read (2 x 33.2 MB),
the base read and the alpha written (2 x 33.2 MB) = 331.8 MB; the statistics pass reads the RGB a third time and is reported on its
own.  python tools/alpha_timing.py [--frames 17] [--height 2160] [--width 3840] [--dtype fp32|bf16] > profiles/alpha_4k.txt"""
import argparse
import ctypes as C
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
    ops_mod, hip_lib, alpha = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "hip_lib", "alpha"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W = args.frames, args.height, args.width
    h, w = H // 3, W // 3
    dt = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    x = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    rgb = torch.empty(T, H, W, 3, dtype=dt, device="cuda")
    for t in range(T):
        for c in range(3):
            rgb[t, :, :, c] = (0.6 * torch.sin(0.011 * x + 0.4 * c + 0.1 * t) * torch.cos(0.013 * y - 0.3 * c)
                               + 0.05 * torch.randn(H, W, generator=g, device="cuda")).to(dt)
    yl = (torch.arange(h, device="cuda", dtype=torch.float32)[:, None] + 0.5) / h
    xl = (torch.arange(w, device="cuda", dtype=torch.float32)[None, :] + 0.5) / w
    d = ((yl - 0.5) ** 2 + ((xl - 0.5) * w / h) ** 2).sqrt()
    mattes = {"binary": (d < 0.3).float().expand(T, h, w).contiguous(), "soft": torch.exp(-(d / 0.35) ** 2).expand(T, h, w).contiguous()}
    px_bytes = rgb.element_size() * 3
    model = H * W * (2 * px_bytes + 4 * 4)                             # per frame: RGB twice, n map twice, base, alpha
    print(f"# {ops.device_info}")
    print(f"# alpha op, {T} frames of {W} x {H} {args.dtype} RGB, alpha from {w} x {h}; 3 warm-ups, mean of 20 launches (HIP events)")
    print(f"# byte model: {model / 1e6:.1f} MB per frame (RGB read twice, n map written and read, base read, alpha written)")
    lib, stream = ops.lib, ops._stream()
    nbytes = int(lib.svr_alpha_workspace_bytes(T, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(T, H, W, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    kind = 1 if dt == torch.float32 else 0
    for name, a in mattes.items():
        base = alpha.bicubic_base(a, H, W)
        n_alpha = a.numel()
        stats = lambda: hip_lib.check(lib.svr_alpha_stats(p(a), n_alpha, p(rgb), T, H, W, 3, kind, p(ws), nbytes, stream), "svr_alpha_stats")
        edges = lambda: hip_lib.check(lib.svr_alpha_edges(p(rgb), T, H, W, 3, kind, p(ws), nbytes, stream), "svr_alpha_edges")
        refine = lambda: hip_lib.check(lib.svr_alpha_refine(p(rgb), p(base), p(out), None, T, H, W, 3, kind, n_alpha, p(ws), nbytes,
                                                            stream), "svr_alpha_refine")
        whole = timed(lambda: ops.alpha_upscale(rgb, a, out=out))
        kernels = timed(lambda: ops.alpha_upscale(rgb, a, out=out, base=base))
        parts = {"bicubic base (torch)": timed(lambda: alpha.bicubic_base(a, H, W)), "svr_alpha_stats": timed(stats),
                 "svr_alpha_edges": timed(edges), "svr_alpha_refine": timed(refine)}
        print(f"{name} matte")
        print(f"  whole op (base + 3 kernels)   {whole / T:8.3f} ms/frame   {whole:8.2f} ms/batch")
        print(f"  3 kernels (base given)        {kernels / T:8.3f} ms/frame   {model * T / (kernels * 1e-3) / 1e9:8.1f} GB/s against the byte model")
        traffic = {"bicubic base (torch)": H * W * 4, "svr_alpha_stats": H * W * px_bytes, "svr_alpha_edges": H * W * (px_bytes + 4),
                   "svr_alpha_refine": H * W * (px_bytes + 12)}
        for k, ms in parts.items():
            print(f"    {k:27s} {ms / T:8.3f} ms/frame   {traffic[k] * T / (ms * 1e-3) / 1e9:8.1f} GB/s of its own minimum traffic")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
