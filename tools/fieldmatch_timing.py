"""Time field matching (HipOps.comb_counts / HipOps.field_select / fieldmatch.field_match, csrc/svr_fieldmatch.hip) next to the pair
it is measured against, on one chunk of the streaming workload, ALL IN THE SAME RUN: 17 woven frames of 1920 x 1080 -> 17
progressive frames, for yuv420p8 and for rgb16;
  comb_counts                      the counts launch (and the memset of its 24 T bytes)
  field_select                     the copy launches (one per plane), counts and deinterlaced clip given
  field_match                      the whole front: deinterlace at rate "frame", comb_counts, field_select
  deinterlace (rate frame)         HipOps.deinterlace of the same chunk
  unpack_frames                    HipOps.unpack_frames of its 17 frames
The chunk is synthetic interlaced video: a smooth random picture panned three columns a field with +-3 codes of noise, woven tff.
10 warm-ups, then five windows of about half a second of back-to-back launches each between HIP events: the windows show the
spread.  The first two frames of each chunk are checked against the specification first.  No threshold is attached to any figure.

Bytes: "unique" counts every input byte once and every output byte once; "issued" counts the loads and stores the kernels make
(comb_counts: every row of plane 0 of F[t] once, the tested rows -- half the rows -- of F[t-1] and F[t+1]: 2 bytes per plane-0
byte; field_select: one load and one store per byte).

python tools/fieldmatch_timing.py [--frames 17] > profiles/fieldmatch.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
WARMUP, WINDOWS, WINDOW_MS = 10, 5, 500.0
THR, MI = 10, 24


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


def woven_chunk(fmt, T, H, W, g):
    """T woven frames (tff) of a smooth picture panned 3 columns a field, +-3 codes of noise, in fmt's packed layout (C = 3)"""
    coarse = torch.rand((1, 1, H // 16 + 2, W // 16 + 2), generator=g, device="cuda")
    base = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[0, 0] * 180 + 30

    def field(k, rows, cols):                                                # the picture at field time k, subsampled
        pic = torch.roll(base, 3 * k, dims=1)[::rows, ::cols]
        noise = torch.randint(-3, 4, pic.shape, generator=g, device="cuda")
        return (pic.round().to(torch.int64) + noise).clamp(0, 255)

    def plane(rows, cols):
        frames = []
        for t in range(T):
            first, second = field(2 * t, rows, cols), field(2 * t + 1, rows, cols)
            second[0::2] = first[0::2]
            frames.append(second)
        return torch.stack(frames)

    if fmt == "yuv420p8":
        y, c = plane(1, 1), plane(2, 2)
        return torch.cat([y.reshape(T, -1), c.reshape(T, -1), (255 - c).reshape(T, -1)], dim=1).to(torch.uint8)
    y = plane(1, 1) << 8                                                      # rgb16: the picture in all three channels
    return y[..., None].expand(T, H, W, 3).to(torch.int32).to(torch.uint16).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    ops_mod, de, fm, fin = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "deinterlace", "fieldmatch", "frameio_in"))
    ops = ops_mod.HipOps("cuda:0")
    T, H, W, C = args.frames, args.height, args.width, 3
    print(f"# {ops.device_info}")
    print(f"# one chunk: {T} woven frames of {W} x {H} -> {T} progressive frames (order tff, thr {THR}, mi {MI}, no context frames); "
          f"{WARMUP} warm-ups, {WINDOWS} windows of ~{WINDOW_MS / 1000:g} s of launches each (HIP events), every leg in this one run")
    print("# what                           fmt        window   launches   ms/launch   unique MB   GB/s unique   issued MB   GB/s issued")
    g = torch.Generator(device="cuda").manual_seed(0)
    for fmt in ("yuv420p8", "rgb16"):
        packed = woven_chunk(fmt, T, H, W, g)
        assert packed.dtype == fin.packed_dtype(fmt) and tuple(packed.shape) == tuple(fin.packed_shape(T, H, W, C, fmt))
        size = packed.element_size()
        frame = packed.numel() // T * size                                       # bytes
        plane0 = de.planes(fmt, H, W, C)[0][1] * de.planes(fmt, H, W, C)[0][2] * size
        small = packed[:2].contiguous()
        want, want_modes, want_cnt = fm.field_match_torch(small.cpu(), fmt, 2, H, W, C, "tff", THR, MI)
        stats = fm.Stats("cuda:0")
        got = fm.field_match(small, fmt, 2, H, W, C, "tff", THR, MI, ops=ops, stats=stats)
        same = (torch.equal(got.cpu(), want) and torch.equal(ops.comb_counts(small, fmt, 2, H, W, C, "tff", THR).cpu(), want_cnt)
                and stats.counts[:4].tolist() == [want_modes.tolist().count(v) for v in range(4)])
        print(f"# {fmt}: kernels equal the specification on the chunk's first two frames (modes {want_modes.tolist()}): "
              f"{'yes' if same else 'NO: RESULT DIFFERS FROM THE SPECIFICATION'}")
        deint = ops.deinterlace(packed, fmt, T, H, W, C, "tff", "frame")
        cnt = ops.comb_counts(packed, fmt, T, H, W, C, "tff", THR)
        out = torch.empty_like(packed)
        fp32 = torch.empty((T, H, W, C), dtype=torch.float32, device="cuda")
        whole = fm.Stats("cuda:0")
        fm.field_match(packed, fmt, T, H, W, C, "tff", THR, MI, ops=ops, stats=whole)
        print(f"# {fmt}: the chunk: {whole.report()}")
        legs = (("comb_counts", lambda: ops.comb_counts(packed, fmt, T, H, W, C, "tff", THR, out=cnt), T * plane0, 2 * T * plane0),
                ("field_select", lambda: ops.field_select(packed, deint, cnt, fmt, T, H, W, C, "tff", MI, out=out), 3 * T * frame, 2 * T * frame),
                ("field_match (the whole front)", lambda: fm.field_match(packed, fmt, T, H, W, C, "tff", THR, MI, ops=ops, out=out),
                 2 * T * frame, None),
                ("deinterlace (rate frame)", lambda: ops.deinterlace(packed, fmt, T, H, W, C, "tff", "frame", out=deint), 2 * T * frame,
                 T * frame * 5.5),
                (f"unpack_frames ({T} frames)", lambda: ops.unpack_frames(out, fmt, T, H, W, C, out=fp32), T * frame + fp32.numel() * 4, None))
        for name, fn, unique, issued in legs:
            for w, (reps, ms) in enumerate(timed(fn)):
                tail = f"{issued / 1e6:11.1f} {issued / ms / 1e6:13.1f}" if issued else f"{'-':>11} {'-':>13}"
                print(f"{name:32s} {fmt:10s} {w + 1:6d} {reps:10d} {ms:11.4f} {unique / 1e6:11.1f} {unique / ms / 1e6:13.1f} {tail}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
