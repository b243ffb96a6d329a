"""TEST INFRASTRUCTURE shared by tests/test_frame_unpack.py and tests/test_gpu_frame_unpack.py: the shapes, random packed clips over
the whole code range, and stand-ins for the ``ffprobe`` and ``ffmpeg`` executables (no machine that runs the suite has the real ones).

The stand-ins are Python scripts in a directory of the test's own:
  ffprobe   prints ``<input>.json`` (the canned answer the test wrote next to its "video") and exits 0;
  ffmpeg    as a DECODER (last argument ``-``): writes ``<input>.raw`` to stdout -- the planes a real decoder would emit -- or, when
            ``<input>.fail`` exists, its text to stderr and exits 3; with ``<input>.endless`` it goes on repeating the raw bytes until
            it is terminated or its pipe closes (a clip longer than anybody reads).  As an ENCODER (anything else): keeps its
            arguments in ``<output>.args`` and its stdin in ``<output>``, like tests/test_stream.py's KEEP_STDIN.
Both append their argument list to ``calls.log`` in their own directory: a test can assert that neither was started."""
import json
import os
import stat
import sys

import torch

from conftest import sub

# [T, H, W]: fewer samples than one vector (1,1,1; 1,1,5), chroma rows and columns that clamp on both sides (1,2,2; 1,3,3; 2,3,5;
# 1,5,4), one and several 16-pixel units per row = the neighbour column across the unit seam and across the row end (1,1,16;
# 2,5,32; 1,4,32; 2,5,48; 1,16,64), odd H in the vector kernel (2,5,32; 2,5,48), W off a multiple of 16 (3,17,33; 1,64,66),
# frame starts off 16 bytes (2,3,5; 2,31,8; 3,17,33)
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 2, 2), (1, 3, 3), (2, 3, 5), (1, 5, 4), (3, 17, 33), (1, 1, 16), (2, 5, 32), (1, 4, 32), (2, 5, 48),
          (1, 16, 64), (1, 64, 66), (2, 31, 8)]
YUV = ("yuv420p8", "yuv420p10")


def channel_counts(fmt):
    return (3,) if fmt in YUV else (3, 4)


def random_packed(fmt, T, H, W, C, seed):
    """Random codes over the WHOLE code range of the container's meaningful bits: 0..255, 0..65535, and for the 10-bit planes 0..1023
    -- far outside the nominal 64..940 / 64..960, so the matrix meets negative numerators and both clamps."""
    fin = sub("frameio_in")
    g = torch.Generator().manual_seed(seed)
    top = {"rgb8": 256, "bgr8": 256, "yuv420p8": 256, "rgb16": 65536, "yuv420p10": 1024}[fmt]
    return torch.randint(0, top, fin.packed_shape(T, H, W, C, fmt), generator=g).to(fin.packed_dtype(fmt))


def raw_bytes(packed):
    """the little-endian byte stream a decoder emits for the packed clip"""
    return packed.contiguous().view(torch.uint8).numpy().tobytes()


_SCRIPT = r'''
import os, sys
here = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(here, "calls.log"), "a") as log:
    log.write(NAME + " " + " ".join(sys.argv[1:]) + "\n")
argv = sys.argv[1:]
if NAME == "ffprobe":
    sys.stdout.write(open(argv[-1] + ".json").read())
    sys.exit(0)
if argv[-1] == "-":                                        # decoder
    src = argv[argv.index("-i") + 1]
    open(src + ".args", "w").write("\n".join(argv))
    if os.path.exists(src + ".fail"):
        sys.stderr.write(open(src + ".fail").read())
        sys.exit(3)
    data = open(src + ".raw", "rb").read()
    out = sys.stdout.buffer
    try:
        out.write(data)
        while os.path.exists(src + ".endless"):
            out.write(data)
        out.flush()
    except BrokenPipeError:
        pass
    sys.exit(0)
open(argv[-1] + ".args", "w").write("\n".join(argv))       # encoder
open(argv[-1], "wb").write(sys.stdin.buffer.read())
'''


def stand_ins(directory):
    """-> (ffprobe, ffmpeg): executables of those names in ``directory``"""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name in ("ffprobe", "ffmpeg"):
        path = os.path.join(directory, name)
        with open(path, "w") as f:
            f.write(f"#!{sys.executable}\nNAME = {name!r}\n{_SCRIPT}")
        os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)
        paths.append(path)
    return tuple(paths)


def calls(directory):
    log = os.path.join(directory, "calls.log")
    return open(log).read().splitlines() if os.path.exists(log) else []


def fake_video(path, packed, pix_fmt, width, height, rate="24/1", audio=False, color_space=None, color_range=None, fail=None,
               endless=False):
    """A "video" at ``path`` as the stand-ins see it: the canned ffprobe answer, the raw planes the decoder emits -> the ffprobe
    dictionary the answer stands for."""
    open(path, "wb").close()
    video = dict(index=0, codec_type="video", codec_name="hevc", width=width, height=height, pix_fmt=pix_fmt, r_frame_rate=rate,
                 avg_frame_rate=rate)
    if color_space:
        video["color_space"] = color_space
    if color_range:
        video["color_range"] = color_range
    streams = [video] + ([dict(index=1, codec_type="audio", codec_name="aac", sample_rate="48000")] if audio else [])
    with open(str(path) + ".json", "w") as f:
        json.dump(dict(streams=streams), f)
    with open(str(path) + ".raw", "wb") as f:
        f.write(raw_bytes(packed) if packed is not None else b"")
    if fail is not None:
        open(str(path) + ".fail", "w").write(fail)
    if endless:
        open(str(path) + ".endless", "w").close()
