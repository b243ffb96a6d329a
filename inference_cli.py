#!/usr/bin/env python
"""Command-line surface of the reference (inference_cli.py:1346-1481, 45 flags) in front of the MI355X hot path.

    python inference_cli.py clip.mp4 --resolution 2160 --batch_size 33 --uniform_batch_size --temporal_overlap 3 \\
           --vae_encode_tiled --vae_decode_tiled --cuda_device 0,1,2,3,4,5,6,7

Every flag of the reference parses with the same name, type, default and choices (tests/test_api_surface.py compares the
two parsers by ``ast``), so existing scripts keep working.  What the flags DO is deliberately thin:
  * frames -> ``pipeline.upscale`` (one GPU) or ``dist.upscale_sharded`` (--cuda_device a,b,...: one process per GPU over
    RCCL, temporal batches dealt round-robin; replaces the reference's mp.Process + mp.Queue workers,
    inference_cli.py:1127-1288);
  * flags that select a small-VRAM policy (--blocks_to_swap, --swap_io_components, --*_offload_device, --cache_dit/_vae),
    another attention backend or torch.compile are accepted and have no effect: one attention kernel, no tracing compiler,
    288 GB of HBM;
  * --chunk_size N streams a long clip: the input is read N frames at a time, each chunk goes through
    ``pipeline.upscale_stream`` (the previous chunk's last --temporal_overlap raw frames as context), its result is narrowed
    on the device (frameio.py / csrc/svr_frame_pack.hip) and handed to ONE writer thread through two pinned host buffers,
    so the encoder works while the next chunk computes and neither device nor host memory grows with the clip;
  * media I/O is plumbing, not the hot path: images through PIL, tensors as .pt / .npy, video in through OpenCV when it is
    installed (the reference's own dependency), video out through OpenCV or (--video_backend ffmpeg, with --10bit a real
    10-bit BT.709 plane) an ffmpeg subprocess fed through stdin.  An HDR / wide-gamut source (BT.2020 primaries or matrix, a PQ
    or HLG transfer) read through ffmpeg leaves --10bit as BT.2020 planes with left-sited chroma, tagged with the source's
    primaries and transfer (output_colour); every other source is written as it always was;
  * --video_backend ffmpeg also READS video through ffmpeg (FrameSource): ffprobe names the source's pixel format, an ffmpeg child
    emits the planes at their native depth, ONE reader thread fills two pinned host buffers while the previous chunk computes, and
    the packed bytes are widened to fp32 on the device (frameio_in.py / csrc/svr_frame_unpack.hip).  The source's audio stream is
    copied into an mp4 the ffmpeg writer produces;
  * png output of frames on the device is encoded there (pngenc.py / csrc/svr_png.hip; the writer thread does CRCs and file I/O),
    as 16-bit files where the source is deeper than 8 bits (output_depth: a video read through ffmpeg as rgb16 / yuv420p10, a
    16-bit RGB / RGBA png still, which load_frames reads with its 16 bits), as 8-bit files otherwise;
  * shot-aware batching has no flag -- the flag set equals the reference's: where shots.ENABLED is set (it ships
    off) and one GPU does the work, hard cuts are found on the device (shots.py / csrc/svr_shots.hip) and no batch, and no
    --chunk_size context, spans one (``pipeline.upscale_shots`` / ``upscale_stream(cuts=...)``);
  * the active picture area has no flag either: where active.ENABLED is set (it ships off) and one GPU does the
    work, the black bars of a letterboxed or pillarboxed clip are found on the device (active.py / csrc/svr_active.hip), only the
    picture goes through the model and the bars are a plain resize (``pipeline.upscale(area=...)``), per clip, per shot and per
    --chunk_size chunk;
  * interlaced sources have no flag either: where deinterlace.ENABLED is set (it ships off) and ffprobe's
    field_order tag names an order, FrameSource makes the woven frames progressive on the device, on the packed planes, between the
    upload and the unpack (deinterlace.py / csrc/svr_deinterlace.hip), at deinterlace.RATE: "field" gives two frames per source
    frame and the writer twice the source's frame rate.  --skip_first_frames, --load_cap and --chunk_size count SOURCE frames;
    --batch_size and --temporal_overlap count the frames the model sees.  With the switch off a source tagged interlaced is
    upscaled as stored, which is said once per job.  ffmpeg backend only;
  * field matching has no flag either: where fieldmatch.ENABLED is set (it ships off) and the tag names an order,
    FrameSource counts, per stored frame, the combing of the three weaves its kept field can make, copies the first clean weave
    (a progressive or telecined picture comes back bit for bit) and deinterlaces only the frames without one (fieldmatch.py /
    csrc/svr_fieldmatch.hip), with fieldmatch.DEFAULTS.  One frame out per frame in, the source's frame rate.  The job ends with
    one line: the frames per decision, and whether the comb counts agree with the tag's order.  It takes precedence over
    deinterlace.ENABLED;
  * decimation has no flag either: where decimate.ENABLED is set (it ships off) and the tag names an order,
    FrameSource matches the fields as above and then drops, of every five matched frames, the one that differs least from its
    predecessor -- a 3:2 telecined clip's repeated picture -- on the packed planes (decimate.py / csrc/svr_decimate.hip), with
    decimate.DEFAULTS.  Four frames out per five in, the writer gets 4/5 of the source's frame rate; a trailing partial cycle is
    kept whole.  The job ends with one more line: the cycles, where in the cycle the drops fell and how many dropped frames were
    no duplicates.  It takes precedence over fieldmatch.ENABLED.
"""
import argparse
import json
import os
import platform
import queue
import re
import shutil
import subprocess
import sys
import threading
import time
from fractions import Fraction
from typing import List, Optional

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
VIDEO_EXT = {".mp4", ".avi", ".mov", ".mkv", ".webm", ".m4v"}
IMAGE_EXT = {".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp"}
TENSOR_EXT = {".pt", ".npy"}
WHOLE_CLIP_READ_FRAMES = 8         # without --chunk_size, FrameSource's two host buffers hold this many frames each


def _itf():
    import importlib
    return importlib.import_module(f"{PKG}.interfaces")


def _pngenc():
    import importlib
    return importlib.import_module(f"{PKG}.pngenc")


def _shots():
    import importlib
    return importlib.import_module(f"{PKG}.shots")


_shots_warned = False


def shot_detector(rank: int, world: int):
    """A shots.Detector(**shots.DEFAULTS) where shots.ENABLED is set and one rank does the work, else None: with the switch off
    (the shipped state) nothing changes; with several ranks a shot cannot be sharded yet, which is said once on rank 0."""
    global _shots_warned
    shots = _shots()
    if not shots.ENABLED:
        return None
    if world > 1:
        if rank == 0 and not _shots_warned:
            print(f"Warning: shot-aware batching serves one GPU; {world} ranks batch by arithmetic alone", file=sys.stderr)
        _shots_warned = True
        return None
    return shots.Detector(**shots.DEFAULTS)


def _active():
    import importlib
    return importlib.import_module(f"{PKG}.active")


_active_warned = False


def active_rule(rank: int, world: int) -> dict:
    """{"area": active.Rule(**active.DEFAULTS)} where active.ENABLED is set and one rank does the work, else {}: with the switch off
    (the shipped state) no call changes; with several ranks the crop is not served yet, which is said once on rank 0."""
    global _active_warned
    active = _active()
    if not active.ENABLED:
        return {}
    if world > 1:
        if rank == 0 and not _active_warned:
            print(f"Warning: the active picture area serves one GPU; {world} ranks upscale the whole frame", file=sys.stderr)
        _active_warned = True
        return {}
    return {"area": active.Rule(**active.DEFAULTS)}


def _deinterlace():
    import importlib
    return importlib.import_module(f"{PKG}.deinterlace")


def _fieldmatch():
    import importlib
    return importlib.import_module(f"{PKG}.fieldmatch")


def _decimate():
    import importlib
    return importlib.import_module(f"{PKG}.decimate")


def source_fields(tag, rank: int):
    """ffprobe's field_order tag -> FrameSource's ``fields``: (order, decimate.RATE) where the tag names an order and
    decimate.ENABLED is set (it ships off); else (order, fieldmatch.RATE) where the tag names an order and
    fieldmatch.ENABLED is set (it ships off); else (order, deinterlace.RATE) where the tag names an order and
    deinterlace.ENABLED is set, else None -- with one warning line on rank 0 where the tag says interlaced and all switches are off
    (the shipped state): the frames are then upscaled as stored."""
    deinterlace = _deinterlace()
    order = deinterlace.field_order(tag)
    if order is None:
        return None
    decimate = _decimate()
    if decimate.ENABLED:
        return order, decimate.RATE
    fieldmatch = _fieldmatch()
    if fieldmatch.ENABLED:
        return order, fieldmatch.RATE
    if not deinterlace.ENABLED:
        if rank == 0:
            print(f"Warning: the source is tagged interlaced (field_order {tag}); deinterlacing is off, the frames are upscaled as stored",
                  file=sys.stderr)
        return None
    return order, deinterlace.RATE


def field_summary(stats, order: str) -> str:
    """The one line a field-matched job ends with (fieldmatch.Stats.report(): the feature's only read-back)."""
    r = stats.report()
    return (f"Field matching ({order}): {r['stored']} frames as stored, {r['prev']} matched to the previous frame, {r['next']} matched to "
            f"the next, {r['deinterlaced']} deinterlaced; combed samples against the previous : next frame over the deinterlaced ones "
            f"{r['sum_prev']} : {r['sum_next']}, which {r['verdict']} the field_order tag")


def decimate_summary(stats) -> str:
    """The one line a decimated job ends with (decimate.Stats.report(): the feature's only read-back)."""
    r = stats.report()
    line = (f"Decimation: {r['cycles']} cycles of five frames, the dropped frame at positions 0..4 in "
            f"{' / '.join(str(n) for n in r['positions'])} of them; {r['not_duplicates']} of the dropped frames were not duplicates")
    if 2 * r["not_duplicates"] > r["cycles"]:
        line += ", so the source does not look telecined"
    return line


def output_depth(inp: str, info: Optional[dict] = None, colour: Optional[dict] = None, fields=None) -> int:
    """Bits per sample of the png files written for this input: 16 where the source is deeper than 8 bits -- a video read through
    ffmpeg whose route is rgb16 / yuv420p10, a 16-bit RGB / RGBA png still --, 8 for everything else (.pt / .npy tensors, the
    OpenCV reader, 8-bit stills).  A source route_planar() routes (``colour``, ``fields``: FrameSource's) follows its own bits."""
    if info is not None:
        routed = route_planar(info, colour, fields)
        if routed is not None:
            return 8 if routed[2] == 8 else 16
        return 16 if route_input(info)[1] in ("rgb16", "yuv420p10") else 8
    if os.path.splitext(inp)[1].lower() == ".png":
        head = _pngenc().png_header(inp)
        return 16 if head is not None and head[2] == 16 and head[3] in (2, 6) and head[4] == 0 else 8
    return 8


def build_parser() -> argparse.ArgumentParser:
    itf = _itf()
    parser = argparse.ArgumentParser(
        description="SeedVR2 Video Upscaler - CLI for high-quality image/video upscaling and batch processing (MI355X backend)",
        formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    g = parser.add_argument_group("Input/Output options")
    g.add_argument("input", type=str, help="Input: video file, image file, tensor file (.pt / .npy, [T, H, W, 3] in [0, 1]) or directory")
    g.add_argument("--output", type=str, default=None, help="Output path (default: auto-generated in 'output/' directory)")
    g.add_argument("--output_format", type=str, default=None, choices=["mp4", "png", None],
                   help="Output format: 'mp4' (video) or 'png' (image sequence). Default: auto-detect from input type")
    g.add_argument("--video_backend", type=str, default="opencv", choices=["opencv", "ffmpeg"], help="Video encoder backend")
    g.add_argument("--10bit", dest="use_10bit", action="store_true", help="Save 10-bit video with x265 (requires --video_backend ffmpeg)")
    g.add_argument("--model_dir", type=str, default=None, help="Model directory (default: ./models/SEEDVR2)")
    g = parser.add_argument_group("Model selection")
    g.add_argument("--dit_model", type=str, default=itf.DEFAULT_DIT, choices=list(itf.DIT_MODELS), help="DiT model to use (3B / 7B, fp16 / fp8)")
    g = parser.add_argument_group("Processing parameters")
    g.add_argument("--resolution", type=int, default=1080, help="Target short-side resolution in pixels (default: 1080)")
    g.add_argument("--max_resolution", type=int, default=0, help="Maximum resolution for any edge. 0 = no limit (default: 0)")
    g.add_argument("--batch_size", type=int, default=5, help="Frames per batch (4n+1: 1, 5, 9, 13, 17, 21, ...). Default: 5")
    g.add_argument("--uniform_batch_size", action="store_true", help="Pad final batch to match batch_size")
    g.add_argument("--seed", type=int, default=42, help="Random seed for reproducibility (default: 42)")
    g.add_argument("--skip_first_frames", type=int, default=0, help="Skip N initial frames (default: 0)")
    g.add_argument("--load_cap", type=int, default=0, help="Load maximum N frames from video. 0 = load all (default: 0)")
    g.add_argument("--chunk_size", type=int, default=0, help="Frames per chunk for streaming mode: read, upscale, pack and write N frames at a time. 0 = whole clip resident in HBM (default: 0)")
    g.add_argument("--prepend_frames", type=int, default=0, help="Prepend N reversed frames to reduce start artifacts (auto-removed). Default: 0")
    g.add_argument("--temporal_overlap", type=int, default=0, help="Frames to overlap between batches/GPUs for smooth blending (default: 0)")
    g = parser.add_argument_group("Quality control")
    g.add_argument("--color_correction", type=str, default="lab", choices=list(itf.COLOR_CORRECTIONS), help="Color correction method (default: lab)")
    g.add_argument("--input_noise_scale", type=float, default=0.0, help="Input noise injection scale (0.0-1.0) (default: 0.0)")
    g.add_argument("--latent_noise_scale", type=float, default=0.0, help="Latent noise injection scale (0.0-1.0) (default: 0.0)")
    g = parser.add_argument_group("Device management")
    if platform.system() != "Darwin":
        g.add_argument("--cuda_device", type=str, default=None, help="GPU(s): single '0' or multi-GPU '0,1,2'. Default: device 0")
    g.add_argument("--dit_offload_device", type=str, default="none", help="accepted, no effect (models stay resident in HBM)")
    g.add_argument("--vae_offload_device", type=str, default="none", help="accepted, no effect")
    g.add_argument("--tensor_offload_device", type=str, default="cpu", help="accepted, no effect (intermediates stay in HBM)")
    g = parser.add_argument_group("Memory optimization (BlockSwap)")
    g.add_argument("--blocks_to_swap", type=int, default=0, help="accepted, no effect")
    g.add_argument("--swap_io_components", action="store_true", help="accepted, no effect")
    g = parser.add_argument_group("VAE tiling (for high resolution upscale)")
    g.add_argument("--vae_encode_tiled", action="store_true", help="Enable VAE encode tiling")
    g.add_argument("--vae_encode_tile_size", type=int, default=1024, help="VAE encode tile size in pixels (default: 1024)")
    g.add_argument("--vae_encode_tile_overlap", type=int, default=128, help="VAE encode tile overlap in pixels (default: 128)")
    g.add_argument("--vae_decode_tiled", action="store_true", help="Enable VAE decode tiling")
    g.add_argument("--vae_decode_tile_size", type=int, default=1024, help="VAE decode tile size in pixels (default: 1024)")
    g.add_argument("--vae_decode_tile_overlap", type=int, default=128, help="VAE decode tile overlap in pixels (default: 128)")
    g.add_argument("--tile_debug", type=str, default="false", choices=["false", "encode", "decode"], help="accepted, no effect")
    g = parser.add_argument_group("Performance optimization")
    g.add_argument("--attention_mode", type=str, default="sdpa", choices=list(itf.ATTENTION_MODES),
                   help="accepted; every mode runs the hand-written HIP window-attention kernel (results of the SDPA path)")
    g.add_argument("--compile_dit", action="store_true", help="accepted, no effect (no tracing compiler on the HIP path)")
    g.add_argument("--compile_vae", action="store_true", help="accepted, no effect")
    g.add_argument("--compile_backend", type=str, default="inductor", choices=["inductor", "cudagraphs"], help="accepted, no effect")
    g.add_argument("--compile_mode", type=str, default="default",
                   choices=["default", "reduce-overhead", "max-autotune", "max-autotune-no-cudagraphs"], help="accepted, no effect")
    g.add_argument("--compile_fullgraph", action="store_true", help="accepted, no effect")
    g.add_argument("--compile_dynamic", action="store_true", help="accepted, no effect")
    g.add_argument("--compile_dynamo_cache_size_limit", type=int, default=64, help="accepted, no effect")
    g.add_argument("--compile_dynamo_recompile_limit", type=int, default=128, help="accepted, no effect")
    g = parser.add_argument_group("Model caching (batch processing)")
    g.add_argument("--cache_dit", action="store_true", help="accepted (engines always stay resident within a process)")
    g.add_argument("--cache_vae", action="store_true", help="accepted")
    g = parser.add_argument_group("Debugging")
    g.add_argument("--debug", action="store_true", help="Enable verbose logging")
    return parser


# ---------------------------------------------------------------------------------------------------------
def load_frames(path: str, skip: int = 0, cap: int = 0):
    """-> (frames [T, H, W, 3] float32 in [0, 1], fps); [T, H, W, 4] where the input carries an alpha channel (an image with
    transparency, a four-channel tensor): pipeline.upscale upscales it edge-guided next to the RGB."""
    import numpy as np
    import torch
    ext = os.path.splitext(path)[1].lower()
    fps = 30.0
    if os.path.isdir(path):
        raise ValueError(f"{path} is a directory: main() runs each media file in it as its own job (list_inputs)")
    elif ext in TENSOR_EXT:
        t = torch.load(path, weights_only=True) if ext == ".pt" else torch.from_numpy(np.load(path))
        frames = t.float()
        if frames.dim() == 3:
            frames = frames[None]
    elif ext in IMAGE_EXT:
        from PIL import Image
        deep = _pngenc().read_png16(path) if ext == ".png" else None
        if deep is not None:                           # a 16-bit RGB / RGBA png keeps its 16 bits (PIL would reduce it to 8) and its alpha
            import importlib
            frames = importlib.import_module(f"{PKG}.frameio_in").unit(torch.from_numpy(deep.astype(np.int64)), 65535)[None]
        else:
            img = Image.open(path)
            has_alpha = img.mode in ("RGBA", "LA", "PA") or "transparency" in img.info
            frames = torch.from_numpy(np.asarray(img.convert("RGBA" if has_alpha else "RGB"), dtype=np.float32) / 255.0)[None]
    elif ext in VIDEO_EXT:
        try:
            import cv2  # type: ignore
        except ImportError as e:
            raise RuntimeError("reading video files needs OpenCV (the reference's own dependency); pass an image folder or a .pt tensor") from e
        cap_ = cv2.VideoCapture(path)
        fps = cap_.get(cv2.CAP_PROP_FPS) or 30.0
        out = []
        while True:
            ok, f = cap_.read()
            if not ok:
                break
            out.append(torch.from_numpy(cv2.cvtColor(f, cv2.COLOR_BGR2RGB)).float() / 255.0)
        cap_.release()
        frames = torch.stack(out)
    else:
        raise ValueError(f"unsupported input: {path}")
    if skip > 0:
        frames = frames[skip:]
    if cap > 0:
        frames = frames[:cap]
    if frames.shape[0] == 0:
        raise ValueError("No frames to process")
    return frames[..., :4 if frames.shape[-1] == 4 else 3].contiguous(), fps


def _keep_channels(frames):
    return frames[..., :4 if frames.shape[-1] == 4 else 3]


def open_chunks(path: str, chunk_size: int, skip: int = 0, cap: int = 0):
    """-> (generator of [t <= chunk_size, H, W, 3 | 4] float32 tensors in [0, 1], fps): the input read ``chunk_size`` frames at a
    time -- a video through cv2.VideoCapture, a .npy memory-mapped, a .pt loaded and sliced.  ``skip`` / ``cap`` as load_frames."""
    import numpy as np
    import torch
    ext = os.path.splitext(path)[1].lower()
    if chunk_size <= 0:
        raise ValueError("chunk_size must be positive")
    if ext in TENSOR_EXT:
        src = torch.load(path, weights_only=True) if ext == ".pt" else np.load(path, mmap_mode="r")
        if src.ndim == 3:
            src = src[None]
        stop = src.shape[0] if cap <= 0 else min(src.shape[0], skip + cap)
        if stop - skip <= 0:
            raise ValueError("No frames to process")

        def tensor_chunks():
            for i in range(skip, stop, chunk_size):
                part = src[i:min(i + chunk_size, stop)]
                part = part if ext == ".pt" else torch.from_numpy(np.array(part))          # (np.array: out of the mapping)
                yield _keep_channels(part.float()).contiguous()
        return tensor_chunks(), 30.0
    if ext not in VIDEO_EXT:
        raise ValueError(f"cannot stream {path}: a video or a .pt / .npy tensor is read in chunks (an image is one frame)")
    try:
        import cv2  # type: ignore
    except ImportError as e:
        raise RuntimeError("reading video files needs OpenCV (the reference's own dependency); pass an image folder or a .pt tensor") from e
    cap_ = cv2.VideoCapture(path)
    fps = cap_.get(cv2.CAP_PROP_FPS) or 30.0

    def video_chunks():
        try:
            for _ in range(skip):
                if not cap_.grab():
                    break
            left, first = (cap if cap > 0 else None), True
            while left is None or left > 0:
                out, want = [], chunk_size if left is None else min(chunk_size, left)
                while len(out) < want:
                    ok, f = cap_.read()
                    if not ok:
                        break
                    out.append(torch.from_numpy(cv2.cvtColor(f, cv2.COLOR_BGR2RGB)).float() / 255.0)
                if not out:
                    if first:
                        raise ValueError("No frames to process")
                    return
                first = False
                if left is not None:
                    left -= len(out)
                short = len(out) < want
                yield torch.stack(out)
                if short:
                    return
        finally:
            cap_.release()
    return video_chunks(), fps


# ---------------------------------------------------------------------------------------------------------
# Video in through ffmpeg (--video_backend ffmpeg): ffprobe says what the file holds, an ffmpeg child emits raw planes at the
# source's depth, frameio_in.py / csrc/svr_frame_unpack.hip widens them to fp32 where the engines live.
def find_ffprobe() -> str:
    exe = shutil.which("ffprobe")
    if exe is None:
        raise RuntimeError("--video_backend ffmpeg needs the ffprobe executable on PATH to read a video and there is none "
                           "(install ffmpeg, or use --video_backend opencv)")
    return exe


def _tail(errlog) -> str:
    errlog.seek(0)
    return errlog.read()[-2000:].decode(errors="replace").strip()


COLOUR_FIELDS = ("color_space", "color_primaries", "color_transfer", "color_range", "chroma_location")


def probe_stream(ffprobe: str, path: str):
    """One ffprobe run (JSON) -> (the FIRST video stream's dictionary as ffprobe wrote it -- the stream FrameSource maps --, the
    list of all streams)."""
    r = subprocess.run([ffprobe, "-v", "error", "-print_format", "json", "-show_streams", path], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise RuntimeError(f"ffprobe exited with status {r.returncode}: {r.stderr[-2000:].decode(errors='replace').strip()}")
    streams = json.loads(r.stdout.decode() or "{}").get("streams", [])
    video = [st for st in streams if st.get("codec_type") == "video"]
    if not video:
        raise ValueError(f"{path}: ffprobe found no video stream")
    return video[0], streams


def source_tags(v: dict, streams: list):
    """probe_stream's answer -> (probe_video's dictionary, probe_colour's dictionary)"""
    fps = Fraction(30)
    for key in ("r_frame_rate", "avg_frame_rate"):
        try:
            rate = Fraction(v.get(key, "0/0"))
        except (ValueError, ZeroDivisionError):
            continue
        if rate > 0:
            fps = rate
            break
    named = lambda key: v.get(key) if v.get(key) not in (None, "", "unknown", "unspecified") else None
    info = dict(width=int(v["width"]), height=int(v["height"]), fps=fps, pix_fmt=v.get("pix_fmt"), color_space=named("color_space"),
                color_range=named("color_range"), has_audio=any(st.get("codec_type") == "audio" for st in streams))
    return info, {key: named(key) for key in COLOUR_FIELDS}


def probe_source(ffprobe: str, path: str):
    """One ffprobe run -> (probe_video's dictionary, probe_colour's dictionary) of the first video stream."""
    return source_tags(*probe_stream(ffprobe, path))


def probe_video(ffprobe: str, path: str) -> dict:
    """-> width, height, fps (a Fraction, from r_frame_rate), pix_fmt, color_space, color_range (None where the file does not say)
    and has_audio."""
    return probe_source(ffprobe, path)[0]


def probe_colour(ffprobe: str, path: str) -> dict:
    """-> color_space, color_primaries, color_transfer, color_range, chroma_location as ffprobe names them; None where the field is
    absent, ``unknown`` or ``unspecified``."""
    return probe_source(ffprobe, path)[1]


HDR_TRANSFERS = ("smpte2084", "arib-std-b67")                # PQ, HLG


def output_colour(colour: Optional[dict], video_backend: str = "ffmpeg", ten_bit: bool = True):
    """What an mp4 written from a source with these colour tags (probe_colour's dictionary; None: not read through ffprobe) is
    written as -> (colour for FFmpegWriter or None = BT.709 as always, one warning line or None).  HDR / wide gamut: a PQ or HLG
    transfer, BT.2020 primaries or the bt2020nc matrix.  Such a source leaves --video_backend ffmpeg --10bit as BT.2020
    non-constant-luminance planes, tv range, chroma co-sited with even luma columns ("left": what a decoder assumes and
    frameio_in.upsample_chroma inverts), tagged with the source's own primaries and transfer; anything else -- and bt2020c, which
    no kernel here writes -- gets the BT.709 output with a warning."""
    if colour is None:
        return None, None
    if colour.get("color_space") == "bt2020c":
        return None, "Warning: the source is BT.2020 constant-luminance (bt2020c), which is not written; writing BT.709 video"
    hdr = (colour.get("color_transfer") in HDR_TRANSFERS or colour.get("color_primaries") == "bt2020"
           or colour.get("color_space") == "bt2020nc")
    if not hdr:
        return None, None
    if video_backend != "ffmpeg":
        return None, "Warning: the source is HDR / BT.2020 and the OpenCV writer has no colour tags; writing 8-bit BT.709 video (use --video_backend ffmpeg --10bit)"
    if not ten_bit:
        return None, "Warning: the source is HDR / BT.2020 and is written as 8-bit BT.709 video without --10bit (use --10bit to keep BT.2020)"
    return dict(matrix="bt2020", range_="tv", siting="left", primaries=colour.get("color_primaries") or "bt2020",
                trc=colour.get("color_transfer") or "bt709"), None


# source pix_fmt -> (what ffmpeg is asked for: the planes as they are, packed format, range or None = from color_range)
PLANAR_420 = {"yuv420p": ("yuv420p", "yuv420p8", None), "yuvj420p": ("yuvj420p", "yuv420p8", "pc"),
              "yuv420p10le": ("yuv420p10le", "yuv420p10", None)}
# every other format with at most 8 bits per component is converted by ffmpeg to rgb24 / rgba; everything else -- deeper formats
# and names this set does not know -- to rgb48le / rgba64le
EIGHT_BIT = {"yuv410p", "yuv411p", "yuv422p", "yuv440p", "yuv444p", "yuvj411p", "yuvj422p", "yuvj440p", "yuvj444p", "nv12", "nv21",
             "nv16", "nv24", "nv42", "yuyv422", "uyvy422", "yvyu422", "uyyvyy411", "gray", "monow", "monob", "pal8", "rgb24", "bgr24", "rgb0",
             "bgr0", "0rgb", "0bgr", "rgb8", "bgr8", "rgb4", "bgr4", "rgb4_byte", "bgr4_byte", "gbrp", "rgba", "bgra", "argb", "abgr",
             "ya8", "gbrap", "yuva420p", "yuva422p", "yuva444p"}
HAS_ALPHA = re.compile(r"^(yuva|gbrap|ya\d|rgba|bgra|argb|abgr|ayuv|vuya)")
MATRIX_OF = {"bt709": "bt709", "smpte170m": "bt601", "bt470bg": "bt601"}


def route_input(info: dict):
    """-> (ffmpeg's -pix_fmt, packed format, C, matrix, range_): planar 4:2:0 of 8 / 10 bits crosses the pipe as it is stored and is
    converted on the device with the stream's own matrix and range; anything else is converted by ffmpeg to RGB of enough depth."""
    pix = info.get("pix_fmt") or ""
    alpha = bool(HAS_ALPHA.match(pix))
    space = info.get("color_space")
    matrix = MATRIX_OF.get(space) if space is not None else ("bt709" if info["height"] >= 720 else "bt601")
    if pix in PLANAR_420 and matrix is not None:
        raw, fmt, range_ = PLANAR_420[pix]
        if range_ is None:
            range_ = "pc" if info.get("color_range") in ("pc", "jpeg") else "tv"
        return raw, fmt, 3, matrix, range_
    if pix in EIGHT_BIT:
        return ("rgba" if alpha else "rgb24"), "rgb8", (4 if alpha else 3), "bt709", "tv"
    return ("rgba64le" if alpha else "rgb48le"), "rgb16", (4 if alpha else 3), "bt709", "tv"


# source pix_fmt -> (subsampling, bits, range or None = from color_range): what planar.py turns into rgb16 codes on the device
PLANAR_SOURCES = {"yuv422p": ("422", 8, None), "yuvj422p": ("422", 8, "pc"), "yuv444p": ("444", 8, None), "yuvj444p": ("444", 8, "pc"),
                  "yuv422p10le": ("422", 10, None), "yuv444p10le": ("444", 10, None), "yuv420p12le": ("420", 12, None),
                  "yuv422p12le": ("422", 12, None), "yuv444p12le": ("444", 12, None),
                  # route_input's own two, only where it cannot say what the stream is: a BT.2020 matrix or top-left chroma
                  "yuv420p": ("420", 8, None), "yuv420p10le": ("420", 10, None)}
PLANAR_MATRIX_OF = dict(MATRIX_OF, bt2020nc="bt2020")


def _planar():
    import importlib
    return importlib.import_module(f"{PKG}.planar")


def route_planar(info: dict, colour: Optional[dict] = None, fields=None):
    """-> (ffmpeg's -pix_fmt: the planes as they are, sub, bits, matrix, range_, siting) for a source whose planes planar.py turns into
    rgb16 codes on the device, or None: route_input decides, as it always did.  None while planar.ENABLED is off (it ships off;
    DESIGN.md 7.3k), for a name outside PLANAR_SOURCES (alpha, semi-planar, 4:1:1 ...), for bt2020c or a matrix outside
    PLANAR_MATRIX_OF, for 4:2:0 of an interlaced source (``fields``: its vertical chroma filter would mix the fields), and for
    yuv420p / yuv420p10le that route_input already reads as they are stored (anything but a bt2020nc matrix or top-left chroma)."""
    pix = info.get("pix_fmt") or ""
    if not _planar().ENABLED or pix not in PLANAR_SOURCES:
        return None
    sub, bits, range_ = PLANAR_SOURCES[pix]
    space = info.get("color_space")
    matrix = PLANAR_MATRIX_OF.get(space) if space is not None else ("bt709" if info["height"] >= 720 else "bt601")
    if matrix is None:
        return None
    topleft = sub == "420" and (colour or {}).get("chroma_location") == "topleft"
    if sub == "420" and (fields is not None or (pix in PLANAR_420 and matrix != "bt2020" and not topleft)):
        return None
    if range_ is None:
        range_ = "pc" if info.get("color_range") in ("pc", "jpeg") else "tv"
    return pix, sub, bits, matrix, range_, ("topleft" if topleft else "left")


def _planar_out():
    import importlib
    return importlib.import_module(f"{PKG}.planar_out")


# source pix_fmt -> (subsampling, bits): PLANAR_420's and PLANAR_SOURCES' names
SOURCE_PLANES = {**{pix: ("420", 10 if "10" in fmt else 8) for pix, (_, fmt, _r) in PLANAR_420.items()},
                 **{pix: (sub, bits) for pix, (sub, bits, _r) in PLANAR_SOURCES.items()}}


def route_output(info: Optional[dict], colour: Optional[dict], video_backend: str = "ffmpeg", ten_bit: bool = False):
    """-> the (sub, bits, matrix, range_, siting) an mp4 is written as through planar_out.pack_planar (FFmpegWriter's ``planes``), or
    None: the writer packs as it always did.  None while planar_out.ENABLED is off (it ships off), for a backend
    other than ffmpeg and for a bt2020c source (output_colour's warning stands; today's route).  sub: the source's own subsampling
    (SOURCE_PLANES; any other name, and a source not read through ffprobe, "420").  bits: 8 without --10bit; with it 12 for a 12-bit
    source, else 10.  matrix / range: output_colour's decision -- bt2020 tv for an HDR / BT.2020 source with --10bit, bt709 tv
    otherwise.  siting: "topleft" for 4:2:0 from a source whose chroma_location says so, else "left" (what an untold decoder
    assumes and planar.py inverts)."""
    if not _planar_out().ENABLED or video_backend != "ffmpeg" or (colour or {}).get("color_space") == "bt2020c":
        return None
    sub, source_bits = SOURCE_PLANES.get((info or {}).get("pix_fmt") or "", ("420", 8))
    bits = 8 if not ten_bit else 12 if source_bits == 12 else 10
    hdr = output_colour(colour, video_backend, ten_bit)[0]
    matrix, range_ = (hdr["matrix"], hdr["range_"]) if hdr else ("bt709", "tv")
    topleft = sub == "420" and (colour or {}).get("chroma_location") == "topleft"
    return sub, bits, matrix, range_, ("topleft" if topleft else "left")


class FrameSource:
    """Video -> fp32 chunks on ``device``, the counterpart of FrameSink.  One ffmpeg child decodes every frame exactly once, in
    order (``-f rawvideo`` carries no timestamps, so ffmpeg neither drops nor duplicates frames), at the depth route_input()
    chose.  ONE reader thread fills one of TWO host buffers (pinned when ``device`` is a GPU) with up to ``chunk_size`` frames while
    the previous chunk computes; the thread makes no GPU call.  ``chunks()`` -- the caller's thread -- uploads the packed bytes and
    widens them with frameio_in.unpack_frames(..., ops): [t <= chunk_size, H, W, 3 | 4] fp32 tensors already on the device, which
    pipeline.upscale_stream takes as they are.  ``skip`` frames are read and dropped, after ``cap`` frames the child is
    terminated; a short last chunk and an empty stream behave as in open_chunks; a child that exits non-zero raises with the tail
    of its stderr.  ``exe``: the executable (find_ffmpeg(), resolved before any GPU work; a test passes its own).

    ``fields`` = (order, rate) (source_fields): an interlaced source.  The decoder's command is the same; ``chunks()`` makes the woven
    frames progressive on the packed bytes, between the upload and the unpack (deinterlace.py / csrc/svr_deinterlace.hip), with
    the previous buffer's last frame and the NEXT buffer's first frame as context -- so it stays one buffer ahead: buffer k + 1 is
    uploaded and its host slot handed back to the reader thread before buffer k is deinterlaced, at the cost of one more packed
    chunk on the device.  The chunks, concatenated, are deinterlace_torch of the whole clip followed by unpack_frames_torch, for
    any chunk size; a chunk has as many frames as were read, twice that at rate "field", where ``fps`` doubles too.
    ``fields`` = (order, "match") (fieldmatch.RATE): field matching instead, with the same context and the same one-buffer lead: the
    chunks, concatenated, are fieldmatch.field_match_torch of the whole clip followed by unpack_frames_torch; as many frames as were
    read, ``fps`` unchanged.  ``match``: dict(thr=, mi=), fieldmatch.DEFAULTS where None.  ``field_stats``: the fieldmatch.Stats the
    chunks add to on the device (None for every other source).
    ``fields`` = (order, "decimate") (decimate.RATE): field matching exactly as above -- the context, the one-buffer lead, ``match``
    and ``field_stats`` are the same -- and then decimation of the matched packed frames.  The source carries, on the device, the
    matched frames that do not yet fill a cycle of five (at most 4) and the matched frame ahead of them; from each buffer it emits
    whole cycles only, a buffer that completes no cycle yields nothing, and the end of the stream emits the partial cycle as it is.
    For any chunk size the chunks, concatenated, are decimate.decimate_torch of fieldmatch.field_match_torch of the whole clip
    followed by unpack_frames_torch; ``fps`` is 4/5 of the source's.  ``decimate``: dict(dup=), decimate.DEFAULTS where None.
    ``decimate_stats``: the decimate.Stats the chunks add to on the device (None for every other source).

    ``colour`` (probe_colour's dictionary): with planar.ENABLED, a source route_planar() routes -- planar 4:2:2 / 4:4:4, 12 bits,
    BT.2020 or top-left 4:2:0 -- is asked for in its own -pix_fmt, and every uploaded buffer becomes rgb16 codes at once
    (planar.planar_codes / csrc/svr_planar.hip; ``planar``: its (sub, bits, matrix, range_, siting)).  From there on the source IS an
    rgb16 source: the chunks, concatenated, are the chains above applied to planar_codes_torch of the whole clip as "rgb16"."""

    def __init__(self, exe: str, path: str, info: dict, chunk_size: int, skip: int = 0, cap: int = 0, ops=None, device="cpu",
                 fields=None, match=None, decimate=None, colour=None):
        import importlib
        import tempfile
        import torch
        if chunk_size <= 0:
            raise ValueError("chunk_size must be positive")
        self.frameio_in = importlib.import_module(f"{PKG}.frameio_in")
        self.raw, self.fmt, self.C, self.matrix, self.range_ = route_input(info)
        routed, self.planar = route_planar(info, colour, fields), None
        if routed is not None:                                   # the planes as stored; rgb16 codes from the upload on
            self.planes = _planar()
            self.raw, self.planar = routed[0], routed[1:]
            self.fmt, self.C, self.matrix, self.range_ = "rgb16", 3, "bt709", "tv"
        self.H, self.W, self.fps = info["height"], info["width"], info["fps"]
        self.fields, self.match, self.field_stats = fields, None, None
        self.decimate, self.decimate_stats = None, None
        if fields is not None:
            self.deinterlace = _deinterlace()
            self.fieldmatch = _fieldmatch()
            self.decimation = _decimate()
            order, rate = fields
            rates = self.deinterlace.RATES + (self.fieldmatch.RATE, self.decimation.RATE)
            if order not in self.deinterlace.ORDERS or rate not in rates:
                raise ValueError(f"fields must be (one of {self.deinterlace.ORDERS}, one of {rates}), got {fields!r}")
            if rate == "field":
                self.fps = 2 * Fraction(info["fps"])
            if rate in (self.fieldmatch.RATE, self.decimation.RATE):     # field matching: its two parameters, and what it did on the device
                self.match = dict(self.fieldmatch.DEFAULTS if match is None else match)
                self.field_stats = self.fieldmatch.Stats(torch.device(device))
            if rate == self.decimation.RATE:                     # ... then decimation: four frames out per five in
                self.fps = Fraction(info["fps"]) * 4 / 5
                self.decimate = dict(self.decimation.DEFAULTS if decimate is None else decimate)
                self.decimate_stats = self.decimation.Stats(torch.device(device))
                self.pending, self.pending_before = None, None   # matched frames short of a cycle; the matched frame ahead of them
        self.chunk_size, self.skip, self.cap, self.ops, self.device = chunk_size, skip, cap, ops, torch.device(device)
        self.frame_bytes = self.frameio_in.frame_bytes(self.H, self.W, self.C, self.fmt)
        if self.planar is not None:                              # (what the reader fills: the planes, not the codes)
            self.frame_bytes = self.planes.frame_bytes(self.H, self.W, self.planar[0], self.planar[1])
        pinned = self.device.type == "cuda"
        self.buffers = [torch.empty(chunk_size * self.frame_bytes, dtype=torch.uint8, pin_memory=pinned) for _ in range(2)]
        self.free, self.work = queue.Queue(), queue.Queue()
        for slot in range(2):
            self.free.put(slot)
        self.stopped = False
        self.errlog = tempfile.TemporaryFile()                   # (a file, not a pipe: nobody drains stderr while frames flow)
        self.proc = subprocess.Popen(self.command(exe, path), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=self.errlog)
        self.thread = threading.Thread(target=self._fill, name="frame-reader", daemon=True)
        self.thread.start()

    def command(self, exe, path):
        return [exe, "-loglevel", "error", "-noautorotate", "-i", path, "-map", "0:v:0", "-f", "rawvideo", "-pix_fmt", self.raw, "-"]

    def _read(self, view) -> int:
        """fill ``view`` from the child's stdout; -> bytes read (less than asked for: the stream ended)"""
        got = 0
        while got < len(view):
            n = self.proc.stdout.readinto(view[got:])
            if not n:
                break
            got += n
        return got

    def _fill(self):
        try:
            fb, left = self.frame_bytes, (self.cap if self.cap > 0 else None)
            ended = False
            if self.skip > 0:                                    # read and dropped, a chunk's worth at a time
                scratch = memoryview(bytearray(min(self.skip, self.chunk_size) * fb))
                todo = self.skip * fb
                while todo > 0 and not ended:
                    want = min(todo, len(scratch))
                    ended = self._read(scratch[:want]) < want
                    todo -= want
            while not ended and not self.stopped and (left is None or left > 0):
                slot = self.free.get()
                if slot is None:
                    break
                want = self.chunk_size if left is None else min(self.chunk_size, left)
                got = self._read(memoryview(self.buffers[slot].numpy())[:want * fb])
                ended = got < want * fb
                if got % fb:
                    raise RuntimeError(f"the decoder's output ended inside a frame ({got % fb} of {fb} bytes)")
                if left is not None:
                    left -= got // fb
                if got:
                    self.work.put((slot, got // fb))
            if not ended:                                        # --load_cap reached (or close() early): the rest is not decoded
                self.stopped = True
                self.proc.terminate()
            rc = self.proc.wait()
            if rc != 0 and not self.stopped:
                raise RuntimeError(f"ffmpeg exited with status {rc}: {_tail(self.errlog)}")
            self.work.put(None)
        except BaseException as e:                               # noqa: BLE001 (handed to the caller's thread)
            self.work.put(e)

    def _uploads(self):
        """the buffers the reader filled, in order: (packed samples where the frames are wanted, frames); the host slot is free
        again when one is yielded"""
        first = True
        while True:
            item = self.work.get()
            if isinstance(item, RuntimeError):                   # (the decoder's own failure: its message as it is)
                raise item
            if isinstance(item, BaseException):
                raise RuntimeError(f"reading frames failed: {type(item).__name__}: {item}") from item
            if item is None:
                if first:
                    raise ValueError("No frames to process")
                return
            slot, t = item
            first = False
            host = self.buffers[slot][:t * self.frame_bytes]
            packed = host.to(self.device) if self.device.type == "cuda" else host.clone()         # (returns when the bytes are there)
            self.free.put(slot)
            if self.planar is not None:                          # planar YUV -> rgb16 codes: the source is an rgb16 source from here on
                sub, bits, matrix, range_, siting = self.planar
                ready = [self.planes.planar_codes(packed.view(self.planes.planar_dtype(bits)), sub, bits, t, self.H, self.W, matrix, range_,
                                                  siting, ops=self.ops).reshape(-1)]
            else:
                ready = [packed.view(self.frameio_in.packed_dtype(self.fmt))]
            del packed, host                                     # (the caller's reference is the only one while this waits for the next)
            yield ready.pop(), t

    def _unpack(self, packed, t):
        return self.frameio_in.unpack_frames(packed, self.fmt, t, self.H, self.W, self.C, self.matrix, self.range_, ops=self.ops)

    def _decimated(self, matched, last):
        """``matched`` [t, frame]: the next matched frames -> the fp32 frames of the whole cycles they complete (``last``: and of the
        partial cycle the stream ends with), or None where they complete none"""
        import torch
        clip = matched if self.pending is None else torch.cat([self.pending, matched])
        n = clip.shape[0]
        whole = n if last else n - n % self.decimation.CYCLE
        if whole == 0:
            self.pending = clip
            return None
        frames = self.decimation.decimate(clip[:whole], self.fmt, whole, self.H, self.W, self.C, self.decimate["dup"],
                                          before=self.pending_before, ops=self.ops, stats=self.decimate_stats)
        self.pending_before = clip[whole - 1].clone()            # (copies of at most five frames: the buffer itself goes)
        self.pending = clip[whole:].clone() if whole < n else None
        return self._unpack(frames.reshape(-1), whole - whole // self.decimation.CYCLE)

    def _progressive(self, packed, t, before, after):
        """buffer ``packed`` of t woven frames between its neighbours' frames -> the fp32 frames of its T or 2 T outputs (decimation:
        of the cycles it completes, or None)"""
        order, rate = self.fields
        last = after is None
        if t == 1:                                               # nothing of its own to mirror at an end of the clip: the clip's mirror
            before, after = (after if before is None else before), (before if after is None else after)
        if rate in (self.fieldmatch.RATE, self.decimation.RATE):                 # t woven frames -> t progressive ones
            frames = self.fieldmatch.field_match(packed, self.fmt, t, self.H, self.W, self.C, order, self.match["thr"], self.match["mi"],
                                                 before=before, after=after, ops=self.ops, stats=self.field_stats)
            if rate == self.decimation.RATE:
                return self._decimated(frames.reshape(t, -1), last)
            return self._unpack(frames.reshape(-1), t)
        frames = self.deinterlace.deinterlace(packed, self.fmt, t, self.H, self.W, self.C, order, rate, before=before, after=after,
                                              ops=self.ops)
        return self._unpack(frames.reshape(-1), t * (2 if rate == "field" else 1))

    def chunks(self):
        try:
            if self.fields is None:
                for packed, t in self._uploads():
                    yield self._unpack(packed, t)
                    del packed
                return
            held, before = None, None                            # the buffer waiting for its successor; the last frame ahead of it
            for packed, t in self._uploads():
                packed = packed.reshape(t, -1)
                if held is not None:
                    ready = [self._progressive(held, held.shape[0], before, packed[0])]
                    if ready[0] is not None:                     # (decimation: a buffer that completes no cycle yields nothing)
                        yield ready.pop()                        # (the caller's reference is the only one, as in _uploads)
                    before = held[-1].clone()                    # (a copy of one frame: the buffer itself goes)
                held = packed
                del packed
            yield self._progressive(held, held.shape[0], before, None)
        finally:
            self.close()

    def close(self):
        """Stop the child if it still runs, let the thread end, drop the log (idempotent)."""
        if not self.stopped:
            self.stopped = True
            if self.proc.poll() is None:
                self.proc.terminate()
        self.free.put(None)
        self.thread.join()
        self.proc.wait()
        self.proc.stdout.close()
        self.errlog.close()


# ---------------------------------------------------------------------------------------------------------
# Writers: host code only (no GPU call), fed packed frames (frameio.py) as numpy arrays by FrameSink's thread.  ``fmt`` names the
# packed format a writer takes (None: the fp32 frames themselves), ``alpha`` whether it keeps a fourth channel.
class EncodedFrames:
    """What FrameSink hands a writer that takes streams: per frame the bytes of its zlib stream (views of a host buffer)."""

    def __init__(self, streams, channels: int):
        self.streams, self.channels = streams, channels


class PngWriter:
    """rgb8 (RGBA for four channels): one file per frame, frame_%06d.png, the index continuing across chunks; ``single``: the one
    frame of an image job goes to ``path`` itself.  ``depth`` 8 or 16 bits per sample.  ``streams`` tells FrameSink that the writer
    also takes frames already encoded where they live (pngenc.py / csrc/svr_png.hip): write_streams() frames each zlib stream as a
    file -- chunk CRCs and file I/O, no deflate on this thread.  write() takes uint8 frames (through PIL, as always) or uint16
    frames (16-bit files through pngenc.write_png).  ``runs``: FrameSink asks the backend for streams with run-length matches
    (pngenc.py "Runs": smaller files of the same samples)."""
    fmt, alpha, streams = "rgb8", True, True

    def __init__(self, path: str, single: bool = False, depth: int = 8, runs: bool = False):
        if depth not in (8, 16):
            raise ValueError(f"depth must be 8 or 16, got {depth}")
        self.path, self.single, self.index, self.depth, self.runs = path, single, 0, depth, bool(runs)

    def write(self, arr, height, width):
        from PIL import Image
        if self.single:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        else:
            os.makedirs(self.path, exist_ok=True)
        for a in arr:
            target = self.path if self.single else os.path.join(self.path, f"frame_{self.index:06d}.png")
            if a.dtype.itemsize == 2:
                _pngenc().write_png(target, a)
            else:
                Image.fromarray(a).save(target)
            self.index += 1

    def write_streams(self, streams, height, width, channels):
        pngenc = _pngenc()
        if self.single:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        else:
            os.makedirs(self.path, exist_ok=True)
        for s in streams:
            head, tail = pngenc.png_parts(s, width, height, channels, self.depth)
            with open(self.path if self.single else os.path.join(self.path, f"frame_{self.index:06d}.png"), "wb") as f:
                f.write(head)
                f.write(s)
                f.write(tail)
            self.index += 1

    def close(self):
        pass


class OpenCVWriter:
    """bgr8 into cv2.VideoWriter (mp4v), which stays open across chunks."""
    fmt, alpha = "bgr8", False

    def __init__(self, path: str, fps: float):
        self.path, self.fps, self.writer = path, fps, None

    def write(self, arr, height, width):
        import cv2  # type: ignore
        if self.writer is None:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            self.writer = cv2.VideoWriter(self.path, cv2.VideoWriter_fourcc(*"mp4v"), self.fps, (width, height))
        for a in arr:
            self.writer.write(a)

    def close(self):
        if self.writer is not None:
            self.writer.release()
            self.writer = None


def find_ffmpeg() -> str:
    exe = shutil.which("ffmpeg")
    if exe is None:
        raise RuntimeError("--video_backend ffmpeg needs the ffmpeg executable on PATH and there is none "
                           "(install ffmpeg, or use --video_backend opencv)")
    return exe


class FFmpegWriter:
    """An ffmpeg subprocess fed raw frames through stdin: bgr24 -> libx264 / yuv420p, or (``ten_bit``) yuv420p10le -> libx265 /
    yuv420p10le -- the planes frameio.py computes from the fp32 frames, not 8-bit frames widened.  The stream is tagged BT.709,
    tv range; with ``colour`` (output_colour's dictionary, ``ten_bit`` only) the planes are BT.2020 tv with left-sited chroma --
    ``pack`` tells FrameSink so: the (matrix, range_, siting) of frameio.pack_yuv420p10, None: ``fmt`` as always -- and the stream is
    tagged bt2020nc, the dictionary's primaries and transfer, tv range and that chroma location.  ``exe``: the executable (find_ffmpeg(), resolved before any GPU work; a test passes its own).  ``fps``: a float or a
    Fraction (passed on as num/den).  ``audio``: (source path, offset in seconds) -- the source as a second input whose audio
    stream, where it has one, is copied (no re-encoding: a codec the container refuses is ffmpeg's own message); None: the command
    without it, as it always was.  ``planes`` (route_output's (sub, bits, matrix, range_, siting); None: everything above, byte for
    byte): FrameSink hands over planar_out.pack_planar's planes, the raw input and the output are both planar_out.pix_fmt(sub, bits)
    (libx264 at 8 bits, libx265 at 10 and 12), nothing is left to a scale filter, and the matrix, range, the primaries and transfer
    (``colour``'s, else bt709) and, for 4:2:0 and 4:2:2, the chroma location are tagged on both sides of the raw input."""
    alpha = False
    MATRIX_TAGS = {"bt709": "bt709", "bt601": "smpte170m", "bt2020": "bt2020nc"}

    def __init__(self, exe: str, path: str, fps, ten_bit: bool = False, audio=None, colour=None, planes=None):
        self.exe, self.path, self.fps, self.ten_bit, self.audio = exe, path, fps, ten_bit, audio
        self.fmt = "yuv420p10" if ten_bit else "bgr8"
        self.colour = colour if ten_bit else None
        self.pack = (self.colour["matrix"], self.colour["range_"], self.colour["siting"]) if self.colour else None
        self.planes = tuple(planes) if planes is not None else None
        self.proc, self.errlog = None, None

    def planes_command(self, height, width, rate, second, mux):
        sub, bits, matrix, range_, siting = self.planes
        pix = _planar_out().pix_fmt(sub, bits)
        primaries, trc = (self.colour["primaries"], self.colour["trc"]) if self.colour else ("bt709", "bt709")
        tags = ["-colorspace", self.MATRIX_TAGS[matrix], "-color_primaries", primaries, "-color_trc", trc, "-color_range", range_]
        if sub != "444":
            tags += ["-chroma_sample_location", siting]
        return ([self.exe, "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", pix, "-s", f"{width}x{height}", "-r", rate]
                + tags + ["-i", "-"] + second + mux
                + ["-c:v", "libx264" if bits == 8 else "libx265", "-pix_fmt", pix, "-preset", "medium", "-crf", "12"] + tags + [self.path])

    def command(self, height, width):
        raw, codec, pix = ("yuv420p10le", "libx265", "yuv420p10le") if self.ten_bit else ("bgr24", "libx264", "yuv420p")
        tags = ["-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv"]
        if self.colour:
            tags = ["-colorspace", "bt2020nc", "-color_primaries", self.colour["primaries"], "-color_trc", self.colour["trc"],
                    "-color_range", self.colour["range_"], "-chroma_sample_location", self.colour["siting"]]
        # 8 bits: ffmpeg converts bgr24 itself, and its default RGB -> YUV matrix is BT.601 whatever the output is tagged with:
        # the scale filter is told the matrix and range the tags then state
        convert = [] if self.ten_bit else ["-vf", "scale=out_color_matrix=bt709:out_range=tv"]
        rate = f"{self.fps.numerator}/{self.fps.denominator}" if isinstance(self.fps, Fraction) and self.fps.denominator != 1 else f"{float(self.fps):g}"
        second, mux = [], []
        if self.audio is not None:
            src, offset = self.audio
            second = (["-ss", f"{float(offset):.6f}"] if offset > 0 else []) + ["-i", src]
            mux = ["-map", "0:v:0", "-map", "1:a?", "-c:a", "copy", "-shortest"]
        if self.planes is not None:
            return self.planes_command(height, width, rate, second, mux)
        return ([self.exe, "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", raw, "-s", f"{width}x{height}", "-r", rate]
                + (tags if self.ten_bit else []) + ["-i", "-"] + second + convert + mux
                + ["-c:v", codec, "-pix_fmt", pix, "-preset", "medium", "-crf", "12"] + tags + [self.path])

    def write(self, arr, height, width):
        if self.proc is None:
            import tempfile
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            self.errlog = tempfile.TemporaryFile()              # (a file, not a pipe: nobody drains stderr while frames flow)
            self.proc = subprocess.Popen(self.command(height, width), stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=self.errlog)
        try:
            self.proc.stdin.write(memoryview(arr).cast("B"))
        except (BrokenPipeError, OSError):
            self._finish()                                       # ffmpeg went away: report ITS message
            raise

    def _finish(self):
        proc, self.proc = self.proc, None
        if proc is None:
            return
        try:
            proc.stdin.close()
        except OSError:
            pass
        rc = proc.wait()
        self.errlog.seek(0)
        tail = self.errlog.read()[-2000:].decode(errors="replace")
        self.errlog.close()
        if rc != 0:
            raise RuntimeError(f"ffmpeg exited with status {rc}: {tail.strip()}")

    def close(self):
        self._finish()


class TensorWriter:
    """.pt output: the fp32 chunks collected on the host, saved once at close (streaming bounds DEVICE memory only here)."""
    fmt, alpha = None, True

    def __init__(self, path: str):
        self.path, self.parts = path, []

    def write(self, frames, height, width):
        self.parts.append(frames)

    def close(self):
        import torch
        if self.parts:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            torch.save(self.parts[0] if len(self.parts) == 1 else torch.cat(self.parts), self.path)
            self.parts = []


class FrameSink:
    """Frames -> writer.  ``put(frames)`` narrows a chunk to the writer's format -- or, for a writer whose ``pack`` attribute names
    a (matrix, range_, siting), to those yuv420p10 planes (frameio.pack_yuv420p10), or, for one whose ``planes`` attribute names a
    (sub, bits, matrix, range_, siting), to those planar YUV planes (planar_out.pack_planar) -- where the frames live (``ops.pack_frames`` on the
    device, ``ops`` being the resident runner's backend; frameio's torch statement for a backend without one and for host frames),
    copies the result into one of TWO host buffers (pinned for device frames) and hands it to ONE writer thread through a queue of depth 2, so the encoder works while the next chunk computes.  The thread makes no GPU
    call.  An exception of the writer is raised in the caller's thread at the next put() or at close().
    A writer whose ``streams`` attribute is true (PngWriter) and a backend with ``encode_png`` on the frames' device: the frames are
    ENCODED there (pngenc.py / csrc/svr_png.hip, at the writer's ``depth``, with run-length matches if its ``runs`` is true), only the bytes produced are copied to the host buffer
    and the thread frames and writes them (EncodedFrames -> write_streams).  A writer of ``depth`` 16 without such a backend is
    handed uint16 samples (frameio.codes(., 65535)); every other case is as above, byte for byte."""

    def __init__(self, writer, ops=None):
        self.writer, self.ops = writer, ops
        self.frames = 0
        self.error = None
        self.work = queue.Queue(maxsize=2)
        self.free = queue.Queue()
        self.buffers = [None, None]
        for slot in range(2):
            self.free.put(slot)
        self.warned_alpha = False
        self.thread = threading.Thread(target=self._drain, name="frame-writer", daemon=True)
        self.thread.start()

    def _drain(self):
        while True:
            item = self.work.get()
            if item is None:
                return
            slot, arr, height, width = item
            try:
                if self.error is None:                           # (after a failure: keep returning buffers, write nothing)
                    if isinstance(arr, EncodedFrames):
                        self.writer.write_streams(arr.streams, height, width, arr.channels)
                    else:
                        self.writer.write(arr, height, width)
            except BaseException as e:                           # noqa: BLE001 (handed to the caller's thread)
                self.error = e
            finally:
                del arr, item
                if slot is not None:
                    self.free.put(slot)

    def _raise_pending(self):
        if self.error is not None:
            raise RuntimeError(f"writing frames failed: {type(self.error).__name__}: {self.error}") from self.error

    def put(self, frames):
        import importlib
        import torch
        frameio = importlib.import_module(f"{PKG}.frameio")
        self._raise_pending()
        if frames.shape[-1] == 4 and not self.writer.alpha:
            if not self.warned_alpha:
                print("Warning: this output has no alpha channel; writing RGB only (use --output_format png to keep it)", file=sys.stderr)
                self.warned_alpha = True
            frames = frames[..., :3]
        height, width = frames.shape[1], frames.shape[2]
        self.frames += frames.shape[0]
        if self.writer.fmt is None:
            self.work.put((None, frames.cpu(), height, width))
            return
        if frames.dtype not in (torch.float32, torch.bfloat16):
            frames = frames.float()
        if frames.is_cuda and self.ops is None:
            raise ValueError("FrameSink: frames on a GPU need the backend that narrows them there (ops=runner.dit.ops)")
        depth = getattr(self.writer, "depth", 8)
        if getattr(self.writer, "streams", False) and hasattr(self.ops, "encode_png") and \
                frames.device.type == torch.device(getattr(self.ops, "device", "cuda")).type:
            # encoded where the frames live: only the bytes produced cross to the host, the writer thread frames and writes them
            if getattr(self.writer, "runs", False):
                out, sizes = self.ops.encode_png(frames.contiguous(), depth, runs=True)
            else:
                out, sizes = self.ops.encode_png(frames.contiguous(), depth)
            sizes = [int(n) for n in sizes.cpu().tolist()]       # (returns when the streams are there)
            nbytes = sum(sizes)
            slot = self.free.get()
            self._raise_pending()
            if self.buffers[slot] is None or self.buffers[slot].numel() < nbytes:
                self.buffers[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=out.is_cuda)
            host, at, streams = self.buffers[slot], 0, []
            for t, n in enumerate(sizes):
                host[at:at + n].copy_(out[t, :n])
                streams.append(host[at:at + n].numpy())
                at += n
            self.work.put((slot, EncodedFrames(streams, frames.shape[-1]), height, width))
            return
        if depth == 16:                                          # no encoder where the frames live: 16-bit samples to the host writer
            q = frameio.codes(frames, 65535.0).to(torch.int32).cpu().numpy().astype("uint16")
            self.work.put((None, q, height, width))
            return
        how, ops = getattr(self.writer, "pack", None), self.ops if frames.is_cuda else None
        planes = getattr(self.writer, "planes", None)
        if planes is not None:                                   # planar_out's planes: (sub, bits, matrix, range_, siting)
            packed = _planar_out().pack_planar(frames.contiguous(), *planes, ops=ops)
        elif how is None:
            packed = frameio.pack_frames(frames.contiguous(), self.writer.fmt, ops)
        else:
            packed = frameio.pack_yuv420p10(frames.contiguous(), *how, ops=ops)
        nbytes = packed.numel() * packed.element_size()
        slot = self.free.get()                                   # waits until the writer is done with one of the two buffers
        self._raise_pending()
        if self.buffers[slot] is None or self.buffers[slot].numel() < nbytes:
            self.buffers[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=packed.is_cuda)
        host = self.buffers[slot][:nbytes].view(packed.dtype).view(packed.shape)
        host.copy_(packed)                                       # (device -> pinned host: returns when the bytes are there)
        self.work.put((slot, host.numpy(), height, width))

    def close(self, quiet: bool = False):
        """Let the writer finish what it was handed, close it, raise what it raised (``quiet``: on the way out of another error)."""
        self.work.put(None)
        self.thread.join()
        try:
            self.writer.close()
        except BaseException as e:                               # noqa: BLE001
            if self.error is None:
                self.error = e
        if not quiet:
            self._raise_pending()


def open_writer(fmt: str, path: str, fps: float, single: bool = False, video_backend: str = "opencv", ten_bit: bool = False,
                ffmpeg: Optional[str] = None, audio=None, colour=None, depth: int = 8, planes=None):
    if fmt == "pt":
        return TensorWriter(path)
    if fmt == "png":
        return PngWriter(path, single, depth, runs=_pngenc().RUNS)
    if video_backend == "ffmpeg":
        return FFmpegWriter(ffmpeg or find_ffmpeg(), path, fps, ten_bit, audio, colour, planes)
    return OpenCVWriter(path, fps)


def save_frames(frames, path: str, fmt: str, fps: float = 30.0, ops=None, **writer_kw):
    """pt: the tensor as it is; png: RGB or, for four-channel frames, RGBA files; mp4 has no alpha: it is dropped with a warning.
    One hand-over to the writer the streaming path uses chunk by chunk."""
    single = fmt == "png" and frames.shape[0] == 1 and path.lower().endswith(".png")
    sink = FrameSink(open_writer(fmt, path, fps, single, **writer_kw), ops)
    try:
        sink.put(frames)
    except BaseException:
        sink.close(quiet=True)
        raise
    sink.close()


def list_inputs(path: str) -> List[str]:
    """A directory input = one job per media file in it (images AND videos, sorted by name), as the reference's CLI processes
    a folder (inference_cli.py: get_media_files / process_single_file): files of different sizes never meet in one clip and
    unrelated images are not blended through the temporal overlap.  A file input = that one job."""
    if not os.path.isdir(path):
        return [path]
    files = sorted(os.path.join(path, f) for f in os.listdir(path)
                   if os.path.splitext(f)[1].lower() in IMAGE_EXT | VIDEO_EXT | TENSOR_EXT)
    if not files:
        raise ValueError(f"no images, videos or tensors in {path}")
    return files


def free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def default_output(inp: str, fmt: str) -> str:
    stem = os.path.splitext(os.path.basename(os.path.normpath(inp)))[0]
    return os.path.join("output", f"{stem}_upscaled" + ("" if fmt == "png_dir" else f".{fmt}"))


def engines(args):
    """-> (runner, text embedding, pipeline keyword arguments, rank, world): the engines resident on cuda:LOCAL_RANK."""
    import importlib
    itf = _itf()
    dist_mod = importlib.import_module(f"{PKG}.dist")
    rank, world, local = dist_mod.init_from_env()
    device = f"cuda:{local}"
    vae_cfg = dict(model=itf.DEFAULT_VAE, device=device, encode_tiled=args.vae_encode_tiled,
                   encode_tile_size=args.vae_encode_tile_size, encode_tile_overlap=args.vae_encode_tile_overlap,
                   decode_tiled=args.vae_decode_tiled, decode_tile_size=args.vae_decode_tile_size,
                   decode_tile_overlap=args.vae_decode_tile_overlap)
    runner = itf.get_runner(dict(model=args.dit_model, device=device), vae_cfg, args.model_dir)
    text = itf.load_text_embedding(runner.dit.device, args.model_dir)
    kw = dict(resolution=args.resolution, max_resolution=args.max_resolution, batch_size=args.batch_size,
              uniform_batch_size=args.uniform_batch_size, temporal_overlap=args.temporal_overlap,
              prepend_frames=args.prepend_frames, color_correction=args.color_correction,
              input_noise_scale=args.input_noise_scale, latent_noise_scale=args.latent_noise_scale, seed=args.seed)
    return runner, text, kw, rank, world


def _sync(runner):
    import torch
    if runner.dit.device.type == "cuda":
        torch.cuda.synchronize()


def run(args, frames, eng=None, **override):
    """One rank's work: engines resident on cuda:LOCAL_RANK, single-GPU or sharded pipeline; returns (the full clip, rank) -- with
    several GPUs the clip on rank 0 and None on every other rank.  ``eng``: engines(args) where the caller already has it;
    ``override``: pipeline keyword arguments that differ from the flags (run_stream: prepend_frames after the first chunk)."""
    import importlib
    dist_mod = importlib.import_module(f"{PKG}.dist")
    pipeline = importlib.import_module(f"{PKG}.pipeline")
    runner, text, kw, rank, world = eng if eng is not None else engines(args)
    kw = {**kw, **override}
    t0 = time.time()
    detector = shot_detector(rank, world)              # (None unless shots.ENABLED: no batch across a cut)
    kw = {**kw, **active_rule(rank, world)}            # ({} unless active.ENABLED: only the picture is upscaled)
    if world > 1:                                      # only rank 0 writes the result: gather the frames there, not everywhere
        out = dist_mod.upscale_sharded(frames.to(runner.dit.device), runner, text, gather="root", **kw)
    elif detector is not None:
        out = pipeline.upscale_shots(frames.to(runner.dit.device), runner, text, cuts=detector, **kw)
    else:
        out = pipeline.upscale(frames.to(runner.dit.device), runner, text, **kw)
    _sync(runner)
    if rank == 0:
        dt = time.time() - t0
        print(f"Upscaled {out.shape[0]} frames to {out.shape[2]}x{out.shape[1]} in {dt:.2f}s ({out.shape[0] / dt:.2f} FPS, {world} GPU(s))")
    return out, rank


def run_stream(args, chunks, eng=None):
    """--chunk_size: a generator of upscaled chunks.  One GPU: pipeline.upscale_stream.  Several: every rank reads the same chunks
    and each (context + chunk) goes through run() -- batches sharded over the ranks, frames gathered on rank 0 -- with the same
    context rule (the previous chunk's last --temporal_overlap raw frames prepended, their output dropped, --prepend_frames on
    the first chunk only).  Rank 0 is yielded the chunks; every other rank is yielded None per chunk (it has nothing to write, but
    takes part in every chunk's collectives to the end of the clip)."""
    import importlib
    import torch
    pipeline = importlib.import_module(f"{PKG}.pipeline")
    eng = eng if eng is not None else engines(args)
    runner, text, kw, rank, world = eng
    detector = shot_detector(rank, world)              # one detector down the whole stream; None unless shots.ENABLED
    kw = {**kw, **active_rule(rank, world)}            # ({} unless active.ENABLED)
    if world == 1:
        yield from pipeline.upscale_stream((c.to(runner.dit.device) for c in chunks), runner, text, cuts=detector, **kw)
        return
    tail, overlap = None, args.temporal_overlap
    for k, chunk in enumerate(chunks):
        context = min(overlap, tail.shape[0]) if (tail is not None and overlap > 0) else 0
        frames = torch.cat([tail[-context:], chunk]) if context else chunk
        out, _ = run(args, frames, eng, prepend_frames=args.prepend_frames if k == 0 else 0)
        tail = chunk[-overlap:].clone() if overlap > 0 else None
        del frames, chunk
        yield None if out is None else out[context:]             # (gather="root": only rank 0 holds the frames)
        del out


def output_path(args, inp: str, fmt: str, n_jobs: int, single: bool) -> str:
    path = default_output(inp, fmt if not (fmt == "png" and not single) else "png_dir")
    if args.output:                                    # one job: the path as given; a folder of jobs: a directory to fill
        path = args.output if n_jobs == 1 else os.path.join(args.output, os.path.basename(path))
    return path


def main(argv: Optional[List[str]] = None) -> int:
    if argv is None and len(sys.argv) == 1:
        sys.argv.append("--help")
    args = build_parser().parse_args(argv)
    devices = [d for d in (getattr(args, "cuda_device", None) or "0").split(",") if d != ""]
    if len(devices) > 1 and "WORLD_SIZE" not in os.environ:
        # multi-GPU: one process per GPU over RCCL (torch.distributed), this script re-run under the launcher
        env = dict(os.environ, HIP_VISIBLE_DEVICES=",".join(devices))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={len(devices)}", "--master-addr",
               "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + (argv if argv is not None else sys.argv[1:])
        return subprocess.call(cmd, env=env)
    if len(devices) == 1 and "WORLD_SIZE" not in os.environ and devices[0] != "0":
        os.environ.setdefault("HIP_VISIBLE_DEVICES", devices[0])
    jobs = list_inputs(args.input)
    ext_of = lambda inp: os.path.splitext(inp)[1].lower()
    fmt_of = lambda inp: args.output_format or ("mp4" if ext_of(inp) in VIDEO_EXT else "pt" if ext_of(inp) in TENSOR_EXT else "png")
    # the encoder is looked for ONCE, before any GPU work: a missing executable must not cost a model load or a clip
    # ... and so is the decoder: with --video_backend ffmpeg a video input is read through ffmpeg too (FrameSource)
    via_ffmpeg = lambda inp: args.video_backend == "ffmpeg" and ext_of(inp) in VIDEO_EXT
    ffmpeg = ffprobe = None
    if args.video_backend == "ffmpeg" and any(fmt_of(inp) == "mp4" or via_ffmpeg(inp) for inp in jobs):
        ffmpeg = find_ffmpeg()
    if any(via_ffmpeg(inp) for inp in jobs):
        ffprobe = find_ffprobe()
    if args.use_10bit and args.video_backend != "ffmpeg":
        print("Warning: --10bit needs --video_backend ffmpeg; writing 8-bit video", file=sys.stderr)
    writer_kw = dict(video_backend=args.video_backend, ten_bit=args.use_10bit and args.video_backend == "ffmpeg", ffmpeg=ffmpeg)
    for inp in jobs:                                   # the engines stay resident between jobs (interfaces.get_runner)
        fmt = fmt_of(inp)
        probed = probe_stream(ffprobe, inp) if via_ffmpeg(inp) else None      # (before the engines: a file ffprobe refuses costs no model load)
        info, colour = source_tags(*probed) if probed else (None, None)
        eng = engines(args)
        rank, ops = eng[3], getattr(eng[0].dit, "ops", None)    # (the runner's backend also narrows the frames for the writers)
        fields = source_fields(probed[0].get("field_order"), rank) if probed else None         # an interlaced source
        job_kw = dict(writer_kw)
        if fmt == "png":                               # a source deeper than 8 bits leaves as 16-bit files
            job_kw["depth"] = output_depth(inp, info, colour, fields)
        if info is not None and info["has_audio"] and fmt == "mp4":            # (via_ffmpeg: the writer is FFmpegWriter)
            job_kw["audio"] = (inp, args.skip_first_frames / float(info["fps"]))
        if fmt == "mp4":                               # an HDR source keeps its colour through --10bit; anything else: BT.709 as always
            out_colour, warning = output_colour(colour, args.video_backend, writer_kw["ten_bit"])
            if warning and rank == 0:
                print(warning, file=sys.stderr)
            if out_colour is not None:
                job_kw["colour"] = out_colour
            planes = route_output(info, colour, args.video_backend, writer_kw["ten_bit"])      # (None as shipped: DESIGN.md 7.3l)
            if planes is not None:
                job_kw["planes"] = planes
        source = lambda n: FrameSource(ffmpeg, inp, info, n, args.skip_first_frames, args.load_cap, ops, eng[0].dit.device, fields,
                                       colour=colour)
        if args.chunk_size > 0 and ext_of(inp) not in IMAGE_EXT:
            # streaming: read, upscale, pack and write --chunk_size frames at a time
            if info is not None:
                src = source(args.chunk_size)
                chunks, fps = src.chunks(), src.fps              # (info["fps"]; twice that where fields come out as frames)
            else:
                chunks, fps = open_chunks(inp, args.chunk_size, args.skip_first_frames, args.load_cap)
            path = output_path(args, inp, fmt, len(jobs), single=False)
            sink, t0 = None, time.time()
            try:
                for out in run_stream(args, chunks, eng):
                    if rank == 0:
                        if sink is None:
                            sink = FrameSink(open_writer(fmt, path, fps, False, **job_kw), ops)
                        sink.put(out)
                    del out
            except BaseException:
                if sink is not None:
                    sink.close(quiet=True)
                raise
            if sink is not None:
                sink.close()
                dt = time.time() - t0
                print(f"Streamed {sink.frames} frames in chunks of {args.chunk_size} in {dt:.2f}s ({sink.frames / dt:.2f} FPS)")
                print(f"Saved: {path}")
            if rank == 0 and info is not None and src.field_stats is not None:
                print(field_summary(src.field_stats, fields[0]))
            if rank == 0 and info is not None and src.decimate_stats is not None:
                print(decimate_summary(src.decimate_stats))
            continue
        src = None
        if info is not None:                           # the whole clip, read in chunks and concatenated on the device
            import torch
            src = source(WHOLE_CLIP_READ_FRAMES)
            frames, fps = torch.cat(list(src.chunks())), src.fps
        else:
            frames, fps = load_frames(inp, args.skip_first_frames, args.load_cap)
        out, rank = run(args, frames, eng)
        if rank == 0:
            path = output_path(args, inp, fmt, len(jobs), single=out.shape[0] == 1)
            save_frames(out, path, fmt, fps, ops=ops, **job_kw)
            print(f"Saved: {path}")
            if src is not None and src.field_stats is not None:                 # what field matching did
                print(field_summary(src.field_stats, fields[0]))
            if src is not None and src.decimate_stats is not None:              # what decimation did
                print(decimate_summary(src.decimate_stats))
    return 0


if __name__ == "__main__":
    sys.exit(main())
