"""Time the PNG encoder (HipOps.encode_png, csrc/svr_png.hip) on 4K frames and, next to it, what the command line did before: 17 frames
of 3840 x 2160 x 3 fp32, depths 8 and 16; 3 warm-ups, then the mean of 20 calls between HIP events.  No threshold is attached to any
figure.

Content: 0.5 + 0.3 sin(x / 9) + 0.2 cos(y / 7) plus N(0, 0.01) per sample and frame -- smooth with noise, what a decoded frame looks
like to a filter and a Huffman code (pure noise would say nothing about either).

Device time: the whole call, and per pass by difference (svr_set_option("png_passes", 1 | 2 | 3) stops after the filter + code pass,
after the scan, or runs all three).  Byte model per frame: 12 B per pixel sample triple read (4 B per fp32 sample), the filtered bytes
written once and read once, the stream written.  Host time per frame: the device -> pinned host copy of the bytes produced, the chunk
CRCs and the file write to a directory of this machine's memory file system (--dir, default /dev/shm).  Beside them, on the same
host and frames: PIL.Image.save of the rgb8 pack (zlib level 6, what PngWriter.write does) per frame, and its file size.

python tools/png_encode_timing.py [--frames 17] [--pil-frames 3] > profiles/png_encode.txt"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--pil-frames", type=int, default=3, help="frames the PIL comparison saves (seconds each)")
    ap.add_argument("--dir", default="/dev/shm")
    args = ap.parse_args()
    ops_mod, pngenc, frameio = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "pngenc", "frameio"))
    ops = ops_mod.HipOps("cuda:0")
    T = args.frames
    x = frames_on_device(T)
    print(f"# {ops.device_info}")
    print(f"# png encode, {T} frames of {W} x {H} x {C} fp32 per call, smooth + noise content; 3 warm-ups, mean of 20 calls (HIP events)")
    raw8 = H * W * C
    for depth in (8, 16):
        _, cap = ops.encode_png_bytes(T, H, W, C, depth)
        out = torch.empty(T, cap, dtype=torch.uint8, device="cuda")
        sizes = torch.empty(T, dtype=torch.int64, device="cuda")
        run = lambda: ops.encode_png(x, depth, out=out, sizes=sizes)
        ms = {}
        for passes in (1, 2, 3):
            ops.set_option("png_passes", passes)
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
        moved = 12 * H * W + 2 * filtered + stream
        print(f"depth {depth:2d}  device ms/frame: whole call {ms[3] / T:7.3f} = filter + code {ms[1] / T:7.3f} + scan {(ms[2] - ms[1]) / T:7.3f}"
              f" + bit packing {(ms[3] - ms[2]) / T:7.3f}   ({ms[3]:.2f} ms per call)")
        print(f"          stream {stream / 1e6:7.3f} MB/frame = {stream / filtered:.4f} of the filtered bytes, {stream / (raw8 * depth // 8):.4f} of raw;"
              f" byte model {moved / 1e6:.1f} MB/frame -> {moved * T / (ms[3] * 1e-3) / 1e9:.1f} GB/s; PIL decodes frame 0{' to the rgb8 pack' if depth == 8 else ''}: {'yes' if ok else 'NO'}")
        # the host's share: copy of the bytes produced, CRC, file write
        with tempfile.TemporaryDirectory(dir=args.dir) as d:
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
        print(f"          host ms/frame: copy {(t1 - t0) * 1e3 / T:7.3f} + crc and write {(t2 - t1) * 1e3 / T:7.3f} = {host_ms:7.3f}"
              f"   -> encode + host, one after the other: {1e3 / (ms[3] / T + host_ms):.1f} frames/s")
        del out, sizes
    # what PngWriter.write did (and does for host frames): PIL at zlib level 6 on one thread
    from PIL import Image
    packed = frameio.pack_frames(x[:args.pil_frames], "rgb8", ops).cpu().numpy()
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        t0 = time.perf_counter()
        for t in range(packed.shape[0]):
            Image.fromarray(packed[t]).save(os.path.join(d, f"frame_{t:06d}.png"))
        dt = (time.perf_counter() - t0) / packed.shape[0]
        size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) / packed.shape[0]
    print(f"PIL.Image.save, depth 8, same frames ({packed.shape[0]} of them): {dt * 1e3:8.1f} ms/frame = {1 / dt:.2f} frames/s, {size / 1e6:.3f} MB/frame"
          f" = {size / raw8:.4f} of raw")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
