"""Time colour correction (phase 4 of pipeline.upscale) on a 17-frame 4K span: per method, colorfix.correct on the kernels
(csrc/svr_colorfix.hip through HipOps) and with impl="torch" -- colorfix.METHODS, the code of before -- in the same process, on the
pipeline's own layouts: the decoded frames channels-last ([T, H, W, 3] fp32, as ``final[w0:w1]``), the reference a [:, :, :H, :W]
slice of a [C, T, H', W'] buffer.  HIP events around each call after a warm-up; peak allocated memory above the operands for both
routes, and how far the two routes' results lie apart at that size (wavelet: 0, the same bits; the rank-matching methods exchange
the matched values of near-tied pixels).  No threshold is attached to any figure.

Byte model, printed next to the times: one pass over a span is T * H * W * 3 * 4 bytes (1.69 GB at 17 x 2160 x 3840).  The wavelet
launch ideally reads content and style and writes the result once: 3 passes.  The torch route makes on the order of sixty (two
operands x five levels x about six elementwise / index kernels, each reading and writing a span).  lab_planes reads 2 and writes 2
passes, lab_merge reads 4/3 and writes 1, AdaIN reads content twice and style once and writes once.

Rank matching (csrc/svr_rank.hip, the last section): per plane HipOps.rank_match against colorfix.histogram_match (torch's sorts) on
the same device planes; a sort's three launches per pass by difference; the whole lab route with colorfix.RANK_MATCH on and off
(mean, min and max of the repetitions) and both routes' peak memory.  The per-method table above runs with RANK_MATCH as it stands.

The HSV half (csrc/svr_hsv.hip, the section after it): the four calls on their own, svr_hue_match taken apart by the bins that
qualify, and the hsv and wavelet_adaptive routes with colorfix.HSV_MATCH on and off in turn (mean, min and max), with both routes' peak
memory.  HSV_MATCH = False is the torch chain of before.

python tools/colorfix_timing.py [--frames 17] [--height 2160] [--width 3840] [--reps 5] >> profiles/colorfix.txt"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
METHODS = ("wavelet", "adain", "lab", "wavelet_adaptive", "hsv")


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


def timed_each(fn, warmup, reps):
    """-> the ``reps`` single-call times in ms (an event pair per call), after the warm-up"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in pairs:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return [s.elapsed_time(e) for s, e in pairs]


def spread(ms):
    return f"{sum(ms) / len(ms):8.2f} ms (min {min(ms):.2f}, max {max(ms):.2f})"


def rank_section(ops, cf, content, style, args):
    """Rank matching (csrc/svr_rank.hip) against colorfix.histogram_match (torch's sorts) on the same device planes, in this
    process: per plane, the launches' shares of a pass, the whole lab route with colorfix.RANK_MATCH on and off, peak memory."""
    T, H, W = args.frames, args.height, args.width
    n = T * H * W
    c_lab, s_lab = ops.lab_planes(ops.wavelet_reconstruct(content, style), style)
    print(f"# ---- rank matching: {n} values per plane; byte model per element: source pairs 4 x (4 + 8 + 8) = 80 B (the last pass stores no "
          f"keys: 76 B), reference keys 4 x (4 + 4 + 4) = 48 B, final scatter 8 B read + 4 B stored at random = {n * 136 / 1e9:.1f} GB per plane "
          f"(+ the digit x tile table: 4 KiB per 4096-key tile and pass, {8 * 4096 * -(-n // 4096) / 1e9:.2f} GB)")
    for i, name in enumerate(("L", "a", "b")):
        src, ref = c_lab[i], s_lab[i]
        out = torch.empty_like(src)
        t_k = timed_each(lambda: ops.rank_match(src, ref, out=out), args.warmup, args.reps)
        t_t = timed_each(lambda: cf.histogram_match(src, ref), args.warmup, args.reps)
        mean_k = sum(t_k) / len(t_k)
        print(f"# plane {name}: ops.rank_match {spread(t_k)}  -> {n * 136 / mean_k / 1e9:6.2f} TB/s of the model's bytes;  "
              f"colorfix.histogram_match {spread(t_t)};  ratio {sum(t_t) / sum(t_k):.2f}")
        del out
    # one plane taken apart: the two sorts, the final scatter by difference, and the launches of a pass by difference
    # (svr_set_option("rank_launches", 1 | 2 | 3): the histogram, + the table scan, + the scatter of every pass)
    src, ref = c_lab[1], s_lab[1]
    out = torch.empty_like(src)
    sorted_, index = torch.empty_like(src), torch.empty(n, dtype=torch.int32, device=src.device)
    t_match = timed(lambda: ops.rank_match(src, ref, out=out), args.warmup, args.reps)
    t_keys = timed(lambda: ops.sort_f32(ref, index=False, sorted_out=sorted_), args.warmup, args.reps)
    t_pairs = timed(lambda: ops.sort_f32(src, index=True, sorted_out=sorted_, index_out=index), args.warmup, args.reps)
    print(f"# plane a: sort of the reference keys {t_keys:8.2f} ms ({n * 48 / t_keys / 1e9:5.2f} TB/s of 48 B),  sort of the source pairs "
          f"{t_pairs:8.2f} ms ({n * 80 / t_pairs / 1e9:5.2f} TB/s of 80 B),  rank_match {t_match:8.2f} ms,  final scatter by difference "
          f"{t_match - t_keys - t_pairs:8.2f} ms ({n * 12 / max(t_match - t_keys - t_pairs, 1e-3) / 1e9:5.2f} TB/s of 12 B; the pair sort "
          f"timed alone also stores 4 B of keys in its last pass)")
    # (one workspace for all of it, filled by a whole sort first: a pass cut short reads what that sort left there)
    need = int(ops.lib.svr_rank_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=src.device)

    def sort_with(with_index):
        rc = ops.lib.svr_sort_f32(src.data_ptr(), n, sorted_.data_ptr(), index.data_ptr() if with_index else None, ws.data_ptr(), need,
                                  ops._stream())
        assert rc == 0, ops.lib.svr_last_error()

    for label, with_index, bytes_ in (("keys", False, (4, 0, 8)), ("pairs", True, (4, 0, 16))):
        t = {}
        try:
            for stages in (3, 1, 2):
                ops.set_option("rank_launches", stages)
                t[stages] = timed(lambda: sort_with(with_index), args.warmup, args.reps)
        finally:
            ops.set_option("rank_launches", 3)                     # whatever happens: below 3 a sort stores nothing
        h, sc, st = t[1], t[2] - t[1], t[3] - t[2]
        print(f"# a pass of the {label:5s} sort (four passes, by difference): histogram {h / 4:6.2f} ms ({100 * h / t[3]:4.1f} %, "
              f"{n * bytes_[0] * 4 / h / 1e9:5.2f} TB/s),  table scan {sc / 4:6.2f} ms ({100 * sc / t[3]:4.1f} %),  scatter {st / 4:6.2f} ms "
              f"({100 * st / t[3]:4.1f} %, {n * bytes_[2] * 4 / max(st, 1e-3) / 1e9:5.2f} TB/s)")
    del out, sorted_, index, c_lab, s_lab
    # the whole lab route, both ways
    fn = lambda: cf.correct(content, style, "lab", ops=ops)
    shipped = cf.RANK_MATCH
    res = {True: ([], 0), False: ([], 0)}
    for flag in (True, False):
        cf.RANK_MATCH = flag
        res[flag] = ([], peak_above(fn))                           # (also the warm-up of that route)
    for _ in range(args.reps):                                     # the two routes in turn: a drift of the box meets both alike
        for flag in (True, False):
            cf.RANK_MATCH = flag
            res[flag][0].extend(timed_each(fn, 0, 1))
    cf.RANK_MATCH = True
    a, b = cf.correct(content, style, "lab", ops=ops), None
    same = torch.equal(a, cf.correct(content, style, "lab", ops=ops))
    cf.RANK_MATCH = False
    b = cf.correct(content, style, "lab", ops=ops)
    cf.RANK_MATCH = shipped
    d = (a - b).abs_()
    print(f"# lab route, colorfix.RANK_MATCH = True : {spread(res[True][0])}   peak above the operands {res[True][1] / 1e9:6.2f} GB   (two runs bit-equal: {same})")
    print(f"# lab route, colorfix.RANK_MATCH = False: {spread(res[False][0])}   peak above the operands {res[False][1] / 1e9:6.2f} GB")
    print(f"# the two routes apart: max {float(d.max()):.3e}, share > 2e-5 {float((d > 2e-5).float().mean()):.3e} (tied pixels exchange matched values)")
    slower = sum(res[True][0]) > sum(res[False][0])
    print(f"# -> RANK_MATCH default by the rule of DESIGN.md 7.3e: {'False (the radix route is slower)' if slower else 'True (not slower)'}"
          f"; as shipped: {shipped}")


def hsv_section(ops, cf, content, style, args):
    """The HSV kernels (csrc/svr_hsv.hip) on their own, and the hsv and wavelet_adaptive routes with colorfix.HSV_MATCH on and off in
    turn in this process (off: the torch chain of before), with both routes' peak memory."""
    T, H, W = args.frames, args.height, args.width
    n = T * H * W
    span = n * 3 * 4
    c_hsv, s_hs = ops.hsv_planes(content, style)
    counts = lambda h: [int(cf.hue_bin_mask(h, k).sum()) for k in range(12)]
    n_c, n_s = counts(c_hsv[0]), counts(s_hs[0])
    bins = [k for k in range(12) if n_c[k] > 100 and n_s[k] > 100]
    sorted_src, sorted_ref = sum(n_c[k] for k in bins), sum(n_s[k] for k in bins)
    # bytes: two class partitions (source 4 + 8 + 8, reference 4 + 8 + 4 per pixel), bin 0's own partition (20), out = c_s when not
    # in place (8); per sorted source element 76 + 8 (apply: index and value read) + 4 stored at random, per reference element 48
    model = n * (20 + 16 + 8 + (20 if 0 in bins else 0)) + sorted_src * 88 + sorted_ref * 48
    print(f"# ---- the HSV half: {n} pixels; bins that qualify {bins}; {sorted_src} source and {sorted_ref} reference elements sorted; "
          f"svr_hue_match byte model {model / 1e9:.1f} GB, workspace {int(ops.lib.svr_hue_match_workspace_bytes(n)) / 1e9:.2f} GB")
    t_p = timed(lambda: ops.hsv_planes(content, style, c_hsv=c_hsv, s_hs=s_hs), args.warmup, args.reps)
    sat = torch.empty_like(c_hsv[1])
    t_h = timed_each(lambda: ops.hue_match(c_hsv[0], c_hsv[1], s_hs[0], s_hs[1], out=sat), args.warmup, args.reps)
    same = torch.equal(sat, ops.hue_match(c_hsv[0], c_hsv[1], s_hs[0], s_hs[1]))
    # a style without hues qualifies no bin: the two class partitions, the host's read of the counts and out = c_s alone
    no_hue = torch.full_like(s_hs[0], float("nan"))
    t_0 = timed_each(lambda: ops.hue_match(c_hsv[0], c_hsv[1], no_hue, s_hs[1], out=sat), args.warmup, args.reps)
    del no_hue
    ops.hue_match(c_hsv[0], c_hsv[1], s_hs[0], s_hs[1], out=sat)
    base = ops.wavelet_reconstruct(content, style)
    out = torch.empty_like(base)
    t_m = timed(lambda: ops.hsv_merge(c_hsv[0], sat, c_hsv[2], (T, H, W), out=out), args.warmup, args.reps)
    t_b = timed(lambda: ops.adaptive_blend(base, content, style, c_hsv[0], sat, c_hsv[2], out=out), args.warmup, args.reps)
    mean_h = sum(t_h) / len(t_h)
    for name, ms, nbytes in (("svr_hsv_planes", t_p, 2 * span + 5 * n * 4), ("svr_hsv_merge", t_m, 3 * n * 4 + span),
                             ("svr_adaptive_blend", t_b, 3 * n * 4 + 4 * span)):
        print(f"# {name:34s} {ms:8.2f} ms  model {nbytes / 1e9:5.2f} GB -> {nbytes / ms / 1e9:7.2f} TB/s of the model's bytes")
    print(f"# {'svr_hue_match':34s} {spread(t_h)}  model {model / 1e9:5.2f} GB -> {model / mean_h / 1e9:7.2f} TB/s of the model's bytes "
          f"(one host read of the class counts inside; two runs bit-equal: {same})")
    print(f"# {'  of it, no bin qualifying':34s} {spread(t_0)}  the two class partitions ({n * 36 / 1e9:.2f} GB), the read of the counts and "
          f"out = c_s ({n * 8 / 1e9:.2f} GB); the sorts and scatters of the bins by difference {mean_h - sum(t_0) / len(t_0):.2f} ms")
    del sat, base, out, c_hsv, s_hs
    shipped = cf.HSV_MATCH
    verdict = {}
    for m in ("hsv", "wavelet_adaptive"):
        fn = lambda: cf.correct(content, style, m, ops=ops)
        res = {}
        for flag in (True, False):
            cf.HSV_MATCH = flag
            res[flag] = ([], peak_above(fn))                       # (also the warm-up of that route)
        for _ in range(args.reps):                                 # the two routes in turn: a drift of the box meets both alike
            for flag in (True, False):
                cf.HSV_MATCH = flag
                res[flag][0].extend(timed_each(fn, 0, 1))
        cf.HSV_MATCH = True
        a = cf.correct(content, style, m, ops=ops)
        cf.HSV_MATCH = False
        d = (a - cf.correct(content, style, m, ops=ops)).abs_()
        cf.HSV_MATCH = shipped
        print(f"# {m:16s} route, colorfix.HSV_MATCH = True : {spread(res[True][0])}   peak above the operands {res[True][1] / 1e9:6.2f} GB")
        print(f"# {m:16s} route, colorfix.HSV_MATCH = False: {spread(res[False][0])}   peak above the operands {res[False][1] / 1e9:6.2f} GB"
              f"   ratio {sum(res[False][0]) / sum(res[True][0]):.2f}")
        print(f"# {m:16s} the two routes apart: max {float(d.max()):.3e}, share > 2e-5 {float((d > 2e-5).float().mean()):.3e}")
        verdict[m] = sum(res[True][0]) <= sum(res[False][0])
        del a, d
    print(f"# -> HSV_MATCH default by the rule of DESIGN.md 7.3e: {'True (not slower on both methods)' if all(verdict.values()) else 'False (slower on ' + ', '.join(k for k, v in verdict.items() if not v) + ')'}"
          f"; as shipped: {shipped}")


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
    ap.add_argument("--methods", default=",".join(METHODS), help="comma-separated; empty: none of the per-method lines")
    ap.add_argument("--no-rank", action="store_true", help="leave the rank-matching section out")
    ap.add_argument("--no-hsv", action="store_true", help="leave the section of the HSV half out")
    ap.add_argument("--random-colours", action="store_true", help="uniformly random pixels instead of noise over a gradient: every "
                    "hue bin holds a twelfth of both operands, so the HSV matching sorts every pixel")
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
    if args.random_colours:
        frames.copy_(torch.rand(T, H, W, 3, generator=g, device="cuda") * 1.8 - 0.9)
        big[:, :, :H, :W] = (torch.rand(T, H, W, 3, generator=g, device="cuda") * 1.2 - 0.5).permute(3, 0, 1, 2)
    content, style = frames.permute(0, 3, 1, 2), big.permute(1, 0, 2, 3)[:, :, :H, :W]
    del smooth, yy, xx
    span = T * H * W * 3 * 4
    print(f"# {ops.device_info}")
    print(f"# span {T} x {H} x {W} x 3 fp32 = {span / 1e9:.2f} GB per pass; {args.warmup} warm-up, mean of {args.reps} calls between HIP events")
    print(f"# byte model: wavelet launch 3 passes = {3 * span / 1e9:.2f} GB (ideal); torch wavelet about 60 passes = {60 * span / 1e9:.0f} GB")
    print(f"{'method':18s} {'kernels ms':>11s} {'torch ms':>10s} {'ratio':>7s} {'kernels peak GB':>16s} {'torch peak GB':>14s}"
          f" {'max |k - t|':>12s} {'share > 2e-5':>13s}")
    for m in filter(None, args.methods.split(",")):
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
    del base, planes, c_lab
    if not args.no_rank and hasattr(ops, "rank_match"):
        rank_section(ops, cf, content, style, args)
    if not args.no_hsv and all(hasattr(ops, k) for k in cf._HSV_OPS):
        hsv_section(ops, cf, content, style, args)


if __name__ == "__main__":
    main()
