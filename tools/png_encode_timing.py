"""Time the PNG encoder (HipOps.encode_png, csrc/svr_png.hip) on 4K frames, the literal stream and the stream with run-length matches
(``runs``) side by side, and, next to them, what the command line did before: 17 frames of 3840 x 2160 x 3 fp32, depths 8 and 16; 3
warm-ups, then the mean of 20 calls between HIP events.  No threshold is attached to any figure.

Content, two sets: 0.5 + 0.3 sin(x / 9) + 0.2 cos(y / 7) plus N(0, 0.01) per sample and frame -- smooth with noise, what a decoded
frame looks like to a filter and a Huffman code (pure noise would say nothing about either) --, and the same frames with a quarter of
the rows zeroed as letterbox bars (the top and the bottom eighth).

Every (set, depth) is measured --repeats times (default 2), the modes alternating (--modes literal,runs), so that the spread between
two runs of the SAME mode stands next to the difference between the modes.

Device time: the whole call, and per pass by difference (svr_set_option("png_passes", 1 | 2 | 3) stops after the filter + code pass,
after the scan -- with runs the token + second-code pass is launched with the scan and counted there --, or runs every launch).  Byte
model per frame: 12 B per pixel sample triple read (4 B per fp32 sample), the filtered bytes written once and read once (twice more
with runs: the token pass, and the packer's look-ahead hits the cache), the stream written.  Host time per frame: the device ->
pinned host copy of the bytes produced, the chunk CRCs and the file write to a directory of this machine's memory file system (--dir,
default /dev/shm).  Beside them, on the same host and frames: PIL.Image.save of the rgb8 pack (zlib level 6, what PngWriter.write does)
per frame, and its file size.

--reference-lib PATH: a libseedvr2_hip.so of ANOTHER build (the parent commit's, say), loaded beside this tree's; its svr_png_encode
is measured as a third mode, "reference", in the same process, on the same frames and in the same alternation -- a comparison of two
builds taken in two processes mixes in what differs between processes on a shared host.

python tools/png_encode_timing.py [--frames 17] [--pil-frames 3] [--repeats 2] [--modes literal,runs] [--reference-lib PATH]
    > profiles/png_encode.txt"""
import argparse
import importlib
import io
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
H, W, C = 2160, 3840, 3


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


def frames_on_device(T):
    g = torch.Generator(device="cuda").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(float(H), device="cuda"), torch.arange(float(W), device="cuda"), indexing="ij")
    base = (0.5 + 0.3 * torch.sin(xx / 9) + 0.2 * torch.cos(yy / 7))[None, ..., None]
    return (base + torch.randn(T, H, W, C, generator=g, device="cuda") * 0.01).contiguous()


def letterboxed(x):
    bar = H // 8
    y = x.clone()
    y[:, :bar] = 0.0
    y[:, H - bar:] = 0.0
    return y


class ReferenceEncoder:
    """svr_png_encode of another build's library, with HipOps' calling convention (literal streams only)."""

    def __init__(self, path, hip_lib):
        import ctypes
        self.ctypes, self.lib = ctypes, ctypes.CDLL(path)
        for name in ("svr_png_encode_bytes", "svr_png_encode", "svr_set_option", "svr_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = hip_lib.SYMBOLS[name]

    def set_option(self, key, value):
        if self.lib.svr_set_option(key.encode(), int(value)) != 0:
            raise RuntimeError(self.lib.svr_last_error().decode())

    def encode_png_bytes(self, T, H_, W_, Cn, depth):
        scratch, cap = self.ctypes.c_int64(0), self.ctypes.c_int64(0)
        if self.lib.svr_png_encode_bytes(T, H_, W_, Cn, depth, self.ctypes.byref(scratch), self.ctypes.byref(cap)) != 0:
            raise RuntimeError(self.lib.svr_last_error().decode())
        return scratch.value, cap.value

    def encode_png(self, x, depth, out, sizes):
        T, H_, W_, Cn = x.shape
        nscratch, _ = self.encode_png_bytes(T, H_, W_, Cn, depth)
        scratch = torch.empty(nscratch, dtype=torch.uint8, device=x.device)
        p = lambda t: self.ctypes.c_void_p(t.data_ptr())
        stream = self.ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        if self.lib.svr_png_encode(p(x), 1, T, H_, W_, Cn, depth, p(scratch), nscratch, p(out), out.shape[1], p(sizes), stream) != 0:
            raise RuntimeError(self.lib.svr_last_error().decode())
        return out, sizes


def measure(ops, pngenc, frameio, x, depth, mode, where, reference=None):
    """One (frames, depth, mode): the device passes, the stream, the host's share -> the printed lines"""
    T = x.shape[0]
    raw8 = H * W * C
    runs = mode == "runs"
    _, cap = ops.encode_png_bytes(T, H, W, C, depth, runs=runs)
    out = torch.empty(T, cap, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(T, dtype=torch.int64, device="cuda")
    enc = reference if mode == "reference" else ops
    run = (lambda: reference.encode_png(x, depth, out, sizes)) if mode == "reference" else \
        (lambda: ops.encode_png(x, depth, out=out, sizes=sizes, runs=runs))
    ms = {}
    for passes in (1, 2, 3):
        enc.set_option("png_passes", passes)
        ms[passes] = timed(run)
    run()
    n = [int(v) for v in sizes.cpu().tolist()]
    first = pngenc.png_file(out[0, :n[0]].cpu().numpy(), W, H, C, depth)
    from PIL import Image
    img = Image.open(io.BytesIO(first))
    img.load()
    ok = img.size == (W, H)
    if depth == 8:
        import numpy as np
        ok = ok and np.array_equal(np.asarray(img), frameio.pack_frames(x[:1], "rgb8", ops)[0].cpu().numpy())
    filtered = H * (1 + W * C * depth // 8)
    stream = sum(n) / T
    moved = 12 * H * W + (3 if runs else 2) * filtered + stream
    mode = f"{mode:9s}"
    middle = "tokens + second code + scan" if runs else "scan"
    lines = [f"depth {depth:2d} {mode}  device ms/frame: whole call {ms[3] / T:7.3f} = filter + code {ms[1] / T:7.3f} + {middle} {(ms[2] - ms[1]) / T:7.3f}"
             f" + bit packing {(ms[3] - ms[2]) / T:7.3f}   ({ms[3]:.2f} ms per call)",
             f"          stream {stream / 1e6:7.3f} MB/frame = {stream / filtered:.4f} of the filtered bytes, {stream / (raw8 * depth // 8):.4f} of raw;"
             f" byte model {moved / 1e6:.1f} MB/frame -> {moved * T / (ms[3] * 1e-3) / 1e9:.1f} GB/s; PIL decodes frame 0{' to the rgb8 pack' if depth == 8 else ''}: {'yes' if ok else 'NO'}"]
    # the host's share: copy of the bytes produced, CRC, file write
    with tempfile.TemporaryDirectory(dir=where) as d:
        host = torch.empty(sum(n), dtype=torch.uint8, pin_memory=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        at = 0
        for t in range(T):
            host[at:at + n[t]].copy_(out[t, :n[t]])
            at += n[t]
        t1 = time.perf_counter()
        at = 0
        for t in range(T):                                  # (what PngWriter.write_streams does)
            s = host[at:at + n[t]].numpy()
            head, tail = pngenc.png_parts(s, W, H, C, depth)
            with open(os.path.join(d, f"frame_{t:06d}.png"), "wb") as f:
                f.write(head)
                f.write(s)
                f.write(tail)
            at += n[t]
        t2 = time.perf_counter()
    host_ms = (t2 - t0) * 1e3 / T
    lines.append(f"          host ms/frame: copy {(t1 - t0) * 1e3 / T:7.3f} + crc and write {(t2 - t1) * 1e3 / T:7.3f} = {host_ms:7.3f}"
                 f"   -> encode + host, one after the other: {1e3 / (ms[3] / T + host_ms):.1f} frames/s")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--pil-frames", type=int, default=3, help="frames the PIL comparison saves (seconds each)")
    ap.add_argument("--repeats", type=int, default=2, help="measurements of every (set, depth, mode), the modes alternating")
    ap.add_argument("--modes", default="literal,runs")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--reference-lib", default=None, help="another build's libseedvr2_hip.so: its svr_png_encode as a third mode")
    args = ap.parse_args()
    modes = [m.strip() for m in args.modes.split(",")]
    if not modes or any(m not in ("literal", "runs") for m in modes):
        ap.error(f"--modes takes literal and runs, got {args.modes!r}")
    ops_mod, pngenc, frameio, hip_lib = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "pngenc", "frameio", "hip_lib"))
    ops = ops_mod.HipOps("cuda:0")
    reference = None
    if args.reference_lib:
        reference = ReferenceEncoder(args.reference_lib, hip_lib)
        modes = ["reference"] + modes
    T = args.frames
    print(f"# {ops.device_info}")
    print(f"# png encode, {T} frames of {W} x {H} x {C} fp32 per call; 3 warm-ups, mean of 20 calls (HIP events); every line {args.repeats} times, modes alternating")
    if reference is not None:
        print("# reference: svr_png_encode of the library given with --reference-lib (the parent commit's build), same process and frames")
    raw8 = H * W * C
    from PIL import Image
    for name in ("smooth + noise", "smooth + noise, a quarter of the rows zeroed as letterbox bars"):
        x = frames_on_device(T)
        if name != "smooth + noise":
            x = letterboxed(x)
        print(f"## content: {name}")
        for depth in (8, 16):
            for rep in range(args.repeats):
                for mode in modes:
                    for line in measure(ops, pngenc, frameio, x, depth, mode, args.dir, reference):
                        print(line)
        # what PngWriter.write did (and does for host frames): PIL at zlib level 6 on one thread
        packed = frameio.pack_frames(x[:args.pil_frames], "rgb8", ops).cpu().numpy()
        with tempfile.TemporaryDirectory(dir=args.dir) as d:
            t0 = time.perf_counter()
            for t in range(packed.shape[0]):
                Image.fromarray(packed[t]).save(os.path.join(d, f"frame_{t:06d}.png"))
            dt = (time.perf_counter() - t0) / packed.shape[0]
            size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) / packed.shape[0]
        print(f"PIL.Image.save, depth 8, same frames ({packed.shape[0]} of them): {dt * 1e3:8.1f} ms/frame = {1 / dt:.2f} frames/s, {size / 1e6:.3f} MB/frame"
              f" = {size / raw8:.4f} of raw")
        del x
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
