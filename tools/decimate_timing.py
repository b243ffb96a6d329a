"""Time decimation (HipOps.frame_diffs / HipOps.decimate_select / decimate.decimate, csrc/svr_decimate.hip); two legs, one per call:

  --leg op    the stage next to the stages around it, on one chunk of the streaming workload, ALL IN THE SAME RUN: 17 frames of
              1920 x 1080, for yuv420p8 and for rgb16;
                frame_diffs                      the diffs launch (and the memset of its 4 T bytes)
                decimate_select                  the copy launch, diffs given: 14 frames out
                decimate                         the whole stage: frame_diffs, decimate_select
                field_match                      the stage it follows: deinterlace at rate "frame", comb_counts, field_select
                unpack_frames                    HipOps.unpack_frames of the 14 frames it leaves, and of all 17
              The chunk is synthetic 3:2 telecined film: a smooth random picture panned six columns a picture with +-3 codes of
              noise, woven tff, so field matching finds two mixed frames in five and decimation one repeat.  10 warm-ups, then five
              windows of about half a second of back-to-back launches each between HIP events: the windows show the spread.  The
              kernels are checked against the specification first.  No threshold is attached to any figure.
              Bytes: "unique" counts every input byte once and every output byte once; "issued" counts the loads and stores the
              kernels make (frame_diffs: plane 0 of every frame twice, as F[t] and as F[t-1]; decimate_select: one load and one
              store per byte of the 4/5 of the frames it copies).
  --leg job   the wall time of one ``pipeline.upscale_stream`` job fed by FrameSource from a telecined 1280 x 720 yuv420p source of
              85 frames (68 film pictures) behind a stand-in decoder (a script that writes the raw planes), upscaled to 2160 with
              synthetic 3B weights and the VAE tiled 1024/128, in ONE buffer and batches of 17: with fields=("tff", "match") --
              the parent commit's path: 85 frames, five batches -- and with fields=("tff", "decimate"): 68 frames, four batches.
              The sizes are chosen so that both legs fill their batches; a chunk that decimates to a frame count just above a
              batch boundary saves less, one just below saves more.  One warm-up job and then ``--calls`` timed ones per rate.

python tools/decimate_timing.py --leg op > profiles/decimate.txt
python tools/decimate_timing.py --leg job >> profiles/decimate.txt"""
import argparse
import importlib
import importlib.util
import os
import stat
import sys
import tempfile
import time
from fractions import Fraction

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
WARMUP, WINDOWS, WINDOW_MS = 10, 5, 500.0
THR, MI, DUP = 10, 24, 1024                           # stated here: the tool does not depend on the modules' DEFAULTS


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


def telecined_chunk(fmt, T, H, W, g, device="cuda"):
    """T frames (tff) of 3:2 telecined film -- per four pictures A B C D the frames A, B, B|C, C|D, D; a smooth picture panned 6
    columns a picture, +-3 codes of noise per picture -- in fmt's packed layout (C = 3)"""
    coarse = torch.rand((1, 1, H // 16 + 2, W // 16 + 2), generator=g, device=device)
    base = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[0, 0] * 180 + 30
    n_pictures = (T + 4) // 5 * 4
    pictures = []
    for k in range(n_pictures):
        noise = torch.randint(-3, 4, (H, W), generator=g, device=device)
        pictures.append((torch.roll(base, 6 * k, dims=1).round().to(torch.int64) + noise).clamp(0, 255))
    first = [4 * (t // 5) + (0, 1, 1, 2, 3)[t % 5] for t in range(T)]          # the picture of the first (even-row) field
    second = [4 * (t // 5) + (0, 1, 2, 3, 3)[t % 5] for t in range(T)]

    def plane(rows, cols):
        frames = []
        for t in range(T):
            frame = pictures[second[t]][::rows, ::cols].clone()
            frame[0::2] = pictures[first[t]][::rows, ::cols][0::2]
            frames.append(frame)
        return torch.stack(frames)

    if fmt == "yuv420p8":
        y, c = plane(1, 1), plane(2, 2)
        return torch.cat([y.reshape(T, -1), c.reshape(T, -1), (255 - c).reshape(T, -1)], dim=1).to(torch.uint8)
    y = plane(1, 1) << 8                                                      # rgb16: the picture in all three channels
    return y[..., None].expand(T, H, W, 3).to(torch.int32).to(torch.uint16).contiguous()


def leg_op(sub, args):
    ops_mod, de, fm, dec, fin = (sub(m) for m in ("ops", "deinterlace", "fieldmatch", "decimate", "frameio_in"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W, C = args.frames, args.height, args.width, 3
    n_out = T - T // dec.CYCLE
    print(f"# {ops.device_info}")
    print(f"# one chunk: {T} telecined frames of {W} x {H} -> field matching (order tff, thr {THR}, mi {MI}) -> decimation (dup {DUP}) -> "
          f"{n_out} frames, no context frames; {WARMUP} warm-ups, {WINDOWS} windows of ~{WINDOW_MS / 1000:g} s of launches each (HIP events), "
          f"every leg in this one run")
    print("# what                           fmt        window   launches   ms/launch   unique MB   GB/s unique   issued MB   GB/s issued")
    g = torch.Generator(device="cuda").manual_seed(0)
    for fmt in ("yuv420p8", "rgb16"):
        woven = telecined_chunk(fmt, T, H, W, g)
        assert woven.dtype == fin.packed_dtype(fmt) and tuple(woven.shape) == tuple(fin.packed_shape(T, H, W, C, fmt))
        size = woven.element_size()
        frame = woven.numel() // T * size                                        # bytes
        plane0 = de.planes(fmt, H, W, C)[0][1] * de.planes(fmt, H, W, C)[0][2] * size
        fstats, dstats = fm.Stats("cuda:0"), dec.Stats("cuda:0")
        matched = fm.field_match(woven, fmt, T, H, W, C, "tff", THR, MI, ops=ops, stats=fstats)
        want, want_drops, want_diff = dec.decimate_torch(matched.cpu(), fmt, T, H, W, C)
        diff = ops.frame_diffs(matched, fmt, T, H, W, C)
        drops = torch.empty(T // dec.CYCLE, dtype=torch.int32, device="cuda")
        out = ops.decimate_select(matched, diff, fmt, T, H, W, C, DUP, drops=drops, stats=dstats.counts)
        same = torch.equal(diff.cpu(), want_diff) and torch.equal(drops.cpu(), want_drops) and torch.equal(out.cpu(), want)
        print(f"# {fmt}: kernels equal the specification on the chunk (diffs {want_diff.tolist()}, drops {want_drops.tolist()}): "
              f"{'yes' if same else 'NO: RESULT DIFFERS FROM THE SPECIFICATION'}")
        print(f"# {fmt}: the chunk: field matching {fstats.report()}; decimation {dstats.report()}")
        fp32 = torch.empty((T, H, W, C), dtype=torch.float32, device="cuda")
        matched_out = torch.empty_like(woven)
        legs = (("frame_diffs", lambda: ops.frame_diffs(matched, fmt, T, H, W, C, out=diff), T * plane0, 2 * (T - 1) * plane0),
                ("decimate_select", lambda: ops.decimate_select(matched, diff, fmt, T, H, W, C, DUP, out=out), (T + n_out) * frame, 2 * n_out * frame),
                ("decimate (the whole stage)", lambda: dec.decimate(matched, fmt, T, H, W, C, DUP, ops=ops, out=out), (T + n_out) * frame,
                 2 * (T - 1) * plane0 + 2 * n_out * frame),
                ("field_match (the stage before)", lambda: fm.field_match(woven, fmt, T, H, W, C, "tff", THR, MI, ops=ops, out=matched_out),
                 2 * T * frame, None),
                (f"unpack_frames ({n_out} frames)", lambda: ops.unpack_frames(out, fmt, n_out, H, W, C, out=fp32[:n_out]),
                 n_out * frame + n_out * H * W * C * 4, None),
                (f"unpack_frames ({T} frames)", lambda: ops.unpack_frames(matched, fmt, T, H, W, C, out=fp32), T * frame + fp32.numel() * 4, None))
        for name, fn, unique, issued in legs:
            for w, (reps, ms) in enumerate(timed(fn)):
                tail = f"{issued / 1e6:11.1f} {issued / ms / 1e6:13.1f}" if issued else f"{'-':>11} {'-':>13}"
                print(f"{name:32s} {fmt:10s} {w + 1:6d} {reps:10d} {ms:11.4f} {unique / 1e6:11.1f} {unique / ms / 1e6:13.1f} {tail}")
    torch.cuda.synchronize()


def stand_in_decoder(directory):
    """an executable that answers FrameSource's ffmpeg command line: the raw planes stored at the -i path, to stdout"""
    path = os.path.join(directory, "decoder")
    with open(path, "w") as f:
        f.write(f"#!{sys.executable}\nimport shutil, sys\n"
                "with open(sys.argv[sys.argv.index('-i') + 1], 'rb') as src:\n    shutil.copyfileobj(src, sys.stdout.buffer, 1 << 22)\n")
    os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)
    return path


def leg_job(sub, args):
    config, weights, runner_mod, pipeline = sub("config"), sub("weights"), sub("runner"), sub("pipeline")
    spec = importlib.util.spec_from_file_location("svr_cli_decimate_timing", os.path.join(ROOT, "inference_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
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
    T, H, W = args.clip_frames, args.job_height, args.job_width
    info = dict(width=W, height=H, fps=Fraction(30000, 1001), pix_fmt="yuv420p", color_space="bt709", color_range="tv", has_audio=False)
    print(f"# {ops.device_info}")
    print(f"# one job: FrameSource (stand-in decoder, one buffer of {T} frames) -> pipeline.upscale_stream: {T} telecined yuv420p frames of "
          f"{W} x {H}, resolution {args.resolution}, batches of {args.batch}, synthetic 3B weights, VAE tiled 1024/128; order tff, thr {THR}, "
          f"mi {MI}, dup {DUP}; wall time from opening the source to the last output frame on the device")
    print("# rate         call        frames out      wall s   reports")
    with tempfile.TemporaryDirectory() as tmp:
        exe, clip = stand_in_decoder(tmp), os.path.join(tmp, "clip.raw")
        with open(clip, "wb") as f:
            f.write(telecined_chunk("yuv420p8", T, H, W, torch.Generator().manual_seed(1), device="cpu").numpy().tobytes())
        means = {}
        for rate in ("match", "decimate"):
            walls = []
            for n in range(args.calls + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                src = cli.FrameSource(exe, clip, info, T, ops=ops, device=device, fields=("tff", rate), match=dict(thr=THR, mi=MI),
                                      decimate=dict(dup=DUP))
                frames = 0
                for out in pipeline.upscale_stream(src.chunks(), runner, text, resolution=args.resolution, batch_size=args.batch):
                    frames += out.shape[0]
                    del out
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                reports = f"{src.field_stats.report()}" + (f" {src.decimate_stats.report()}" if src.decimate_stats is not None else "")
                print(f"{rate:12s} {'warm-up' if n == 0 else f'call {n}':10s} {frames:11d} {wall:11.3f}   {reports}", flush=True)
                if n:
                    walls.append(wall)
            means[rate] = sum(walls) / len(walls)
        print(f"# mean wall time, decimate / match: {means['decimate']:.3f} / {means['match']:.3f} = {means['decimate'] / means['match']:.3f} "
              f"(frames out: {T - T // 5} / {T} = {(T - T // 5) / T:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("op", "job"), required=True)
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--clip-frames", type=int, default=85)
    ap.add_argument("--job-height", type=int, default=720)
    ap.add_argument("--job-width", type=int, default=1280)
    ap.add_argument("--resolution", type=int, default=2160)
    ap.add_argument("--batch", type=int, default=17)
    ap.add_argument("--calls", type=int, default=2)
    args = ap.parse_args()
    sub = lambda m: importlib.import_module(f"{PKG}.{m}")
    if args.leg == "op":
        leg_op(sub, args)
    else:
        leg_job(sub, args)


if __name__ == "__main__":
    main()
