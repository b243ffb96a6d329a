"""Time the active-picture-area feature (active.py, csrc/svr_active.hip, pipeline.upscale(area=...)); three legs, one per call:

  --leg op        the profile op (HipOps.active_profile) on one chunk of the streaming workload -- 33 frames of 1280 x 720, C = 3,
                  fp32 and bf16, a random field between black bars (picture 1280 x 536) -- against its torch statement
                  (active.profile_torch) on the same device tensor and against one plain read of the chunk (a ``sum``); each of
                  the three twice, alternating, 3 warm-ups and then enough launches between HIP events to fill about half a
                  second; then a chunk without bars (every pixel counts: the most LDS traffic) and a black one (none).  The first
                  run also checks the kernel against the statement.
  --leg baseline  end to end WITHOUT the feature: a synthetic 17-frame 1280 x 720 clip whose picture is 1280 x 536 between black
                  bars, ``pipeline.upscale`` to 2160 (3840 x 2160) in one batch with synthetic 3B weights and the VAE tiled
                  1024/128; per-phase times (the three runner calls between device synchronisations; "other" is the rest: input
                  transform, trims, colour correction, and with the feature the profile, its read-back and the canvas).  This leg
                  uses nothing the feature added, so ``--root <a checkout of the parent commit>`` times the parent on the same box.
  --leg area      the same clip through ``pipeline.upscale(area=active.Rule(...))`` at this commit.

One warm-up call and then ``--calls`` timed ones per leg; no threshold is attached to any figure.

python tools/active_timing.py --leg op > profiles/active_area.txt
python tools/active_timing.py --leg baseline --root <parent checkout> >> profiles/active_area.txt
python tools/active_timing.py --leg area >> profiles/active_area.txt"""
import argparse
import importlib
import os
import sys
import time

import torch

PKG = "comfyui-seedvr2_videoupscaler_amd"
RULE = dict(dark=8, specks=0, skew=4, margin=2, gain=6)     # stated here: the tool does not depend on active.DEFAULTS


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


def letterboxed(T, H, W, picture_rows, seed=0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.zeros(T, H, W, 3, device=device)
    top = (H - picture_rows) // 2
    x[:, top:top + picture_rows] = torch.rand(T, picture_rows, W, 3, generator=g, device=device) * 0.9 + 0.1
    return x


def leg_op(sub, args):
    ops, active = sub("ops").HipOps("cuda:0"), sub("active")
    T, H, W = args.chunk_frames, args.height, args.width
    x = letterboxed(T, H, W, args.picture_rows)
    out = torch.empty(H + W, dtype=torch.int32, device="cuda")
    same = torch.equal(ops.active_profile(x, RULE["dark"], out=out), active.profile_torch(x, RULE["dark"]))
    print(f"# {ops.device_info}")
    print(f"# active-area profile of one chunk: {T} frames of {W} x {H}, C = 3, picture {W} x {args.picture_rows} between black bars, "
          f"dark = {RULE['dark']}; 3 warm-ups, mean over ~0.5 s of launches (HIP events)")
    print(f"# kernel equals the specification on this chunk: {'yes' if same else 'NO: RESULT DIFFERS FROM THE SPECIFICATION'}")
    print("# what                          dtype   pass   launches   ms/chunk   us/frame   GB/s of frames read")
    legs = (("kernel (svr_active_profile)", lambda t: ops.active_profile(t, RULE["dark"], out=out)),
            ("torch (profile_torch)", lambda t: active.profile_torch(t, RULE["dark"])),
            ("plain read (sum)", lambda t: t.sum()))

    def table(t, label, legs_):
        nbytes = t.numel() * t.element_size()
        for rnd in (1, 2):
            for name, fn in legs_:
                ms, reps = timed(lambda: fn(t))
                print(f"{name:30s} {label:6s} {rnd:5d} {reps:10d} {ms:10.3f} {ms * 1e3 / T:10.2f} {nbytes / (ms * 1e-3) / 1e9:12.1f}")

    table(x, "fp32", legs)
    table(x.to(torch.bfloat16), "bf16", legs)
    print("# a chunk without bars: every pixel counts")
    table(letterboxed(T, H, W, H, seed=1), "fp32", legs[:1] + legs[2:])
    print("# a black chunk: nothing counts")
    table(torch.zeros_like(x), "fp32", legs[:1] + legs[2:])
    torch.cuda.synchronize()


def leg_e2e(sub, args, with_area):
    config, weights, runner_mod, pipeline = sub("config"), sub("weights"), sub("runner"), sub("pipeline")
    device = torch.device("cuda:0")
    ops = sub("ops").HipOps(device)
    dcfg, vcfg = config.DIT_3B, config.VAE_V3
    runner = runner_mod.VideoDiffusionInfer(
        runner_mod.default_config(dcfg, vcfg), encode_tiled=True, encode_tile_size=(1024, 1024), encode_tile_overlap=(128, 128),
        decode_tiled=True, decode_tile_size=(1024, 1024), decode_tile_overlap=(128, 128))
    runner.dit = sub("dit").NaDiTEngine(dcfg, weights.synth_dit_state_dict(dcfg, device=device), ops)
    runner.vae = sub("vae").VideoVAEEngine(vcfg, weights.synth_vae_state_dict(vcfg, device=device), ops)
    runner.configure_diffusion(device=device, dtype=torch.bfloat16)
    text = weights.synth_text_embedding(device=device)
    T, H, W = args.clip_frames, args.height, args.width
    clip = letterboxed(T, H, W, args.picture_rows, seed=2)
    kw = dict(resolution=args.resolution, batch_size=T)
    if with_area:
        kw["area"] = sub("active").Rule(**RULE)
    phase = {}

    def wrap(name, attr):
        real = getattr(runner, attr)

        def call(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real(*a, **k)
            torch.cuda.synchronize()
            phase[name] = phase.get(name, 0.0) + time.perf_counter() - t0
            return out

        setattr(runner, attr, call)

    for name, attr in (("encode", "vae_encode"), ("dit", "inference"), ("decode", "vae_decode")):
        wrap(name, attr)
    what = "upscale(area=Rule)" if with_area else "upscale"
    print(f"# {ops.device_info}")
    print(f"# end to end, {what}: {T} frames of {W} x {H}, picture {W} x {args.picture_rows} between black bars, resolution "
          f"{args.resolution}, one batch, synthetic 3B weights, VAE tiled 1024/128, colour correction lab; package from {args.root_label}")
    print("# call          encode s      dit s   decode s    other s    total s   output")
    rows = []
    for n in range(args.calls + 1):
        phase.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipeline.upscale(clip, runner, text, **kw)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        row = [phase.get("encode", 0.0), phase.get("dit", 0.0), phase.get("decode", 0.0)]
        row = row + [total - sum(row), total]
        label = "warm-up" if n == 0 else f"call {n}"
        print(f"{label:10s} " + " ".join(f"{v:10.3f}" for v in row) + f"   {tuple(out.shape)}", flush=True)
        if n:
            rows.append(row)
        del out
    mean = [sum(r[i] for r in rows) / len(rows) for i in range(5)]
    print(f"{'mean':10s} " + " ".join(f"{v:10.3f}" for v in mean))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("op", "baseline", "area"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose package is timed (default: this one)")
    ap.add_argument("--chunk-frames", type=int, default=33)
    ap.add_argument("--clip-frames", type=int, default=17)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--picture-rows", type=int, default=536)
    ap.add_argument("--resolution", type=int, default=2160)
    ap.add_argument("--calls", type=int, default=2)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    args.root_label = "this checkout" if root == os.path.dirname(os.path.dirname(os.path.abspath(__file__))) else "the --root checkout"
    sys.path.insert(0, root)
    sub = lambda m: importlib.import_module(f"{PKG}.{m}")
    if args.leg == "op":
        leg_op(sub, args)
    else:
        leg_e2e(sub, args, with_area=args.leg == "area")


if __name__ == "__main__":
    main()
