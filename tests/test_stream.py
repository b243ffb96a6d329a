"""-m "not gpu": streaming a long clip -- pipeline.upscale_stream against the per-chunk pipeline.upscale calls it stands for (bit for
bit, on the fp32 torch double of the C ABI), and the command line's --chunk_size path end to end: chunked readers, the frame sink
with its writer thread, the png / ffmpeg writers (the ffmpeg executable replaced by a script that keeps what it is fed)."""
import importlib.util
import os
import stat
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from ops_reference import TorchOps


def tiny_runner(ops, vae_channels=None):
    """After the model of tests/test_alpha.py::_tiny_runner.  ``vae_channels``: the device kernels serve GroupNorm widths of 128 and
    up, so the GPU tests take the reduced VAE of the pipeline goldens, (128, 128, 128, 128), instead of VAE_TINY's stages."""
    config, weights, dit, vae, runner = (sub(n) for n in ("config", "weights", "dit", "vae", "runner"))
    dcfg = config.DIT_TINY
    vcfg = config.VAE_TINY if vae_channels is None else config.VAEConfig(block_out_channels=tuple(vae_channels))
    r = runner.VideoDiffusionInfer(runner.default_config(dcfg, vcfg))
    r.dit = dit.NaDiTEngine(dcfg, weights.synth_dit_state_dict(dcfg), ops)
    r.vae = vae.VideoVAEEngine(vcfg, weights.synth_vae_state_dict(vcfg), ops)
    return r


KW = dict(resolution=16, batch_size=5, color_correction="lab")


@pytest.fixture(scope="module")
def rig():
    """(runner, text, 13 RGBA frames of 8 x 10)"""
    from test_alpha import rgba_clip
    return tiny_runner(TorchOps("cpu", act_dtype=torch.float32)), sub("weights").synth_text_embedding().float(), rgba_clip(frames=13, h=8, w=10)


def split(frames, n):
    return [frames[i:i + n] for i in range(0, frames.shape[0], n)]


@pytest.fixture(scope="module")
def streamed(rig):
    """the RGB stream of the 13 frames in chunks of 5, overlap 2, prepend 1: shared by the stream and the CLI tests, never changed"""
    runner, text, clip = rig
    rgb = clip[..., :3].contiguous()
    return list(sub("pipeline").upscale_stream(iter(split(rgb, 5)), runner, text, temporal_overlap=2, prepend_frames=1, **KW))


@pytest.mark.parametrize("overlap", [2, 0])
def test_stream_equals_upscale_of_each_context_plus_chunk(rig, streamed, overlap):
    pipeline = sub("pipeline")
    runner, text, clip = rig
    rgb = clip[..., :3].contiguous()
    chunks = split(rgb, 5)
    got = streamed if overlap == 2 else list(pipeline.upscale_stream(iter(chunks), runner, text, temporal_overlap=0, prepend_frames=1, **KW))
    assert [o.shape[0] for o in got] == [5, 5, 3]
    for k, o in enumerate(got):
        ctx = min(overlap, 5) if k > 0 else 0
        frames = torch.cat([chunks[k - 1][-ctx:], chunks[k]]) if ctx else chunks[k]
        want = pipeline.upscale(frames, runner, text, temporal_overlap=overlap, prepend_frames=1 if k == 0 else 0, **KW)
        assert want.shape[0] == ctx + chunks[k].shape[0]
        assert o.dtype == want.dtype and torch.equal(o, want[ctx:]), k
    assert got[0].shape[1:] == (16, 20, 3)


def test_one_chunk_covering_the_clip_is_upscale_of_the_clip(rig):
    pipeline = sub("pipeline")
    runner, text, clip = rig
    rgb = clip[:7, ..., :3].contiguous()
    kw = dict(temporal_overlap=1, prepend_frames=1, **KW)
    got = list(pipeline.upscale_stream([rgb], runner, text, **kw))
    assert len(got) == 1 and torch.equal(got[0], pipeline.upscale(rgb, runner, text, **kw))


def test_rgba_chunks_keep_four_channels_and_short_context(rig):
    """RGBA in, RGBA out; a first chunk shorter than the overlap lends only the frames it has (min(temporal_overlap, t_prev))."""
    pipeline = sub("pipeline")
    runner, text, clip = rig
    chunks = [clip[:1], clip[1:6]]
    got = list(pipeline.upscale_stream(iter(chunks), runner, text, temporal_overlap=2, **KW))
    assert [tuple(o.shape) for o in got] == [(1, 16, 20, 4), (5, 16, 20, 4)]
    want = pipeline.upscale(clip[:6], runner, text, temporal_overlap=2, **KW)[1:]
    assert torch.equal(got[1], want)
    assert float(got[1][..., 3].std()) > 0.1
    with pytest.raises(ValueError, match="chunk 0"):
        list(pipeline.upscale_stream([clip[:0]], runner, text, **KW))


def test_generator_keeps_only_the_raw_tail_between_chunks(rig):
    """Once chunk k + 1 is asked for, nothing of chunk k is referenced by the generator but its raw input tail: the yielded tensor
    and the chunk itself die with the caller's references."""
    import gc
    import weakref
    pipeline = sub("pipeline")
    runner, text, clip = rig
    rgb = clip[:4, ..., :3].contiguous()
    inputs = []

    def chunks():
        for i in range(2):
            c = rgb[2 * i:2 * i + 2].clone()
            inputs.append(weakref.ref(c))
            yield c
            del c

    stream = pipeline.upscale_stream(chunks(), runner, text, temporal_overlap=1, **{**KW, "batch_size": 1})
    first = next(stream)
    out_ref = weakref.ref(first)
    del first
    second = next(stream)
    gc.collect()
    assert out_ref() is None and inputs[0]() is None           # (inputs[1] is still the chunk source's own variable)
    assert second.shape[0] == 2
    stream.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
@pytest.fixture()
def cli(rig, monkeypatch):
    """inference_cli with the engines replaced by the tiny runner; .calls counts get_runner"""
    runner, text, _ = rig
    spec = importlib.util.spec_from_file_location("svr_cli_stream", os.path.join(ROOT, "inference_cli.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    itf = sub("interfaces")
    mod.calls = []
    monkeypatch.setattr(itf, "get_runner", lambda *a, **k: mod.calls.append(a) or runner)
    monkeypatch.setattr(itf, "load_text_embedding", lambda device, model_dir=None: text)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    return mod


ARGS = ["--resolution", "16", "--batch_size", "5", "--temporal_overlap", "2", "--prepend_frames", "1", "--chunk_size", "5"]


def fake_ffmpeg(directory, body):
    """an executable named ffmpeg in ``directory``: a Python script with ``body``"""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, "ffmpeg")
    with open(path, "w") as f:
        f.write(f"#!{sys.executable}\nimport sys\n{body}\n")
    os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)
    return path


KEEP_STDIN = ("open(sys.argv[-1] + '.args', 'w').write('\\n'.join(sys.argv[1:]))\n"
              "open(sys.argv[-1], 'wb').write(sys.stdin.buffer.read())")


def test_cli_streams_a_npy_into_a_png_folder(cli, rig, streamed, tmp_path, capsys):
    from PIL import Image
    frameio = sub("frameio")
    _, _, clip = rig
    np.save(tmp_path / "clip.npy", clip[..., :3].numpy())
    assert cli.main([str(tmp_path / "clip.npy"), "--output_format", "png", "--output", str(tmp_path / "out")] + ARGS) == 0
    want = torch.cat([frameio.pack_frames_torch(o, "rgb8") for o in streamed]).numpy()
    assert sorted(os.listdir(tmp_path / "out")) == [f"frame_{i:06d}.png" for i in range(13)]
    for i in range(13):
        img = Image.open(tmp_path / "out" / f"frame_{i:06d}.png")
        assert img.mode == "RGB" and np.array_equal(np.asarray(img), want[i]), i
    assert len(cli.calls) == 1 and "Streamed 13 frames" in capsys.readouterr().out
    # --skip_first_frames / --load_cap keep their meaning: frames 5..9 are the second chunk, now without context and with the prepend
    assert cli.main([str(tmp_path / "clip.npy"), "--output_format", "png", "--output", str(tmp_path / "part"),
                     "--skip_first_frames", "5", "--load_cap", "5"] + ARGS) == 0
    assert sorted(os.listdir(tmp_path / "part")) == [f"frame_{i:06d}.png" for i in range(5)]
    # the same clip as .pt, read and sliced; four channels stay RGBA files
    torch.save(clip[:6].clone(), tmp_path / "rgba.pt")
    assert cli.main([str(tmp_path / "rgba.pt"), "--output_format", "png", "--output", str(tmp_path / "rgba")] + ARGS) == 0
    assert Image.open(tmp_path / "rgba" / "frame_000005.png").mode == "RGBA" and len(os.listdir(tmp_path / "rgba")) == 6


@pytest.mark.parametrize("rank", [0, 1])
def test_cli_streams_over_several_ranks(cli, rig, streamed, tmp_path, monkeypatch, rank):
    """WORLD_SIZE 2 as one rank sees it: every (context + chunk) goes through run() and dist.upscale_sharded(gather="root"), which
    hands the frames to rank 0 and None to every other rank (replaced here by the single-rank pipeline resp. None: no process
    group in this test).  Rank 0 is yielded -- and writes -- the single-GPU stream; rank 1 goes through every chunk, is yielded
    None each time and writes nothing."""
    from PIL import Image
    frameio, pipeline, dist_mod = sub("frameio"), sub("pipeline"), sub("dist")
    runner, text, clip = rig
    real, seen = cli.engines, []

    def engines(args):
        r, t, kw, _, _ = real(args)
        return r, t, kw, rank, 2

    def sharded(frames, r, t, gather="all", **kw):
        assert gather == "root"
        seen.append((frames.shape[0], kw["prepend_frames"], kw["temporal_overlap"]))
        return pipeline.upscale(frames, r, t, **kw) if rank == 0 else None

    monkeypatch.setattr(cli, "engines", engines)
    monkeypatch.setattr(dist_mod, "upscale_sharded", sharded)
    rgb = clip[..., :3].contiguous()
    got = list(cli.run_stream(cli.build_parser().parse_args(["x.npy"] + ARGS), iter(split(rgb, 5))))
    assert seen == [(5, 1, 2), (7, 0, 2), (5, 0, 2)]                              # context 0, 2, 2; the prepend on chunk 0 only
    if rank == 0:
        assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, streamed))
    else:
        assert got == [None, None, None]
    np.save(tmp_path / "clip.npy", rgb.numpy())
    assert cli.main([str(tmp_path / "clip.npy"), "--output_format", "png", "--output", str(tmp_path / "out")] + ARGS) == 0
    if rank == 0:
        want = torch.cat([frameio.pack_frames_torch(o, "rgb8") for o in streamed]).numpy()
        assert sorted(os.listdir(tmp_path / "out")) == [f"frame_{i:06d}.png" for i in range(13)]
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "frame_000012.png")), want[12])
    else:
        assert not os.path.exists(tmp_path / "out")
    # the whole-clip path on a rank that receives nothing: nothing written, no error
    seen.clear()
    assert cli.main([str(tmp_path / "clip.npy"), "--output_format", "png", "--output", str(tmp_path / "whole"), "--load_cap", "3"] + ARGS[:-2]) == 0
    assert seen == [(3, 1, 2)] and os.path.exists(tmp_path / "whole") == (rank == 0)


def test_cli_feeds_ffmpeg_ten_bit_planes(cli, rig, streamed, tmp_path, monkeypatch):
    frameio = sub("frameio")
    _, _, clip = rig
    fake_ffmpeg(str(tmp_path / "bin"), KEEP_STDIN)
    monkeypatch.setenv("PATH", str(tmp_path / "bin") + os.pathsep + os.environ.get("PATH", ""))
    np.save(tmp_path / "clip.npy", clip[..., :3].numpy())
    out = tmp_path / "out.mp4"
    assert cli.main([str(tmp_path / "clip.npy"), "--output_format", "mp4", "--video_backend", "ffmpeg", "--10bit", "--output", str(out)] + ARGS) == 0
    want = torch.cat([frameio.pack_frames_torch(o, "yuv420p10") for o in streamed])
    assert tuple(want.shape) == (13, 16 * 20 + 2 * 8 * 10)
    assert out.read_bytes() == want.numpy().astype("<u2").tobytes()
    argv = open(str(out) + ".args").read().split("\n")
    pair = lambda flag: [argv[i + 1] for i, a in enumerate(argv) if a == flag]
    assert pair("-s") == ["20x16"] and pair("-r") == ["30"] and pair("-f") == ["rawvideo"] and pair("-i") == ["-"]
    assert pair("-pix_fmt") == ["yuv420p10le", "yuv420p10le"] and pair("-c:v") == ["libx265"]
    assert set(pair("-colorspace")) == {"bt709"} and set(pair("-color_range")) == {"tv"} and argv[-1] == str(out)
    # 8 bits through the same pipe: bgr24 into libx264
    out8 = tmp_path / "out8.mp4"
    assert cli.main([str(tmp_path / "clip.npy"), "--output_format", "mp4", "--video_backend", "ffmpeg", "--output", str(out8)] + ARGS) == 0
    assert out8.read_bytes() == torch.cat([frameio.pack_frames_torch(o, "bgr8") for o in streamed]).numpy().tobytes()
    argv = open(str(out8) + ".args").read().split("\n")
    assert [argv[i + 1] for i, a in enumerate(argv) if a == "-pix_fmt"] == ["bgr24", "yuv420p"] and "libx264" in argv
    # ffmpeg converts bgr24 itself on this route: it is told the matrix and range that the tags state
    assert [argv[i + 1] for i, a in enumerate(argv) if a == "-vf"] == ["scale=out_color_matrix=bt709:out_range=tv"]
    assert "-vf" not in open(str(out) + ".args").read().split("\n")            # (the 10-bit planes arrive converted)


def test_cli_looks_for_ffmpeg_before_the_engines(cli, rig, tmp_path, monkeypatch, capsys):
    _, _, clip = rig
    os.makedirs(tmp_path / "empty")
    monkeypatch.setenv("PATH", str(tmp_path / "empty"))
    np.save(tmp_path / "clip.npy", clip[:2, ..., :3].numpy())
    with pytest.raises(RuntimeError, match="ffmpeg"):
        cli.main([str(tmp_path / "clip.npy"), "--output_format", "mp4", "--video_backend", "ffmpeg", "--10bit"] + ARGS)
    assert cli.calls == []
    # --10bit without the ffmpeg backend: a warning, and the 8-bit route (here: the png writer never asks for an encoder)
    assert cli.main([str(tmp_path / "clip.npy"), "--output_format", "png", "--10bit", "--output", str(tmp_path / "o")] + ARGS) == 0
    assert "--10bit needs --video_backend ffmpeg" in capsys.readouterr().err


def test_a_failing_writer_is_reported_by_main(cli, rig, tmp_path, monkeypatch):
    _, _, clip = rig
    np.save(tmp_path / "clip.npy", clip[..., :3].numpy())

    def full(self, arr, height, width):
        raise OSError("no space left on device")
    monkeypatch.setattr(cli.PngWriter, "write", full)
    with pytest.raises(RuntimeError, match="no space left on device"):
        cli.main([str(tmp_path / "clip.npy"), "--output_format", "png", "--output", str(tmp_path / "out")] + ARGS)


def test_ffmpeg_writer_reports_a_failed_encoder_with_its_message(cli, tmp_path):
    exe = fake_ffmpeg(str(tmp_path / "bin"), "sys.stdin.buffer.read()\nsys.stderr.write('Unknown encoder libx265\\n')\nsys.exit(3)")
    sink = cli.FrameSink(cli.FFmpegWriter(exe, str(tmp_path / "o.mp4"), 24.0, ten_bit=True))
    sink.put(torch.rand(2, 4, 6, 3))
    with pytest.raises(RuntimeError, match="status 3.*Unknown encoder libx265"):
        sink.close()
    assert not sink.thread.is_alive()


def test_sink_hands_over_through_two_buffers_in_order(cli, tmp_path):
    """Five hand-overs through the two host buffers: the writer sees every chunk once, in order, with the bytes of its own chunk
    (a buffer is not reused before the writer is done with it); the whole-clip path writes the same files as the chunked one."""
    frameio = sub("frameio")
    seen = []

    class Slow:
        fmt, alpha = "rgb8", True

        def write(self, arr, height, width):
            seen.append((arr.copy(), height, width))

        def close(self):
            seen.append("closed")

    g = torch.Generator().manual_seed(0)
    chunks = [torch.rand(t, 4, 6, 3, generator=g) for t in (3, 3, 1, 3, 2)]
    sink = cli.FrameSink(Slow())
    for c in chunks:
        sink.put(c)
    sink.close()
    assert seen[-1] == "closed" and len(seen) == 6 and sink.frames == 12
    for c, (arr, h, w) in zip(chunks, seen):
        assert (h, w) == (4, 6) and np.array_equal(arr, frameio.pack_frames_torch(c, "rgb8").numpy())
    whole = torch.cat(chunks)
    cli.save_frames(whole, str(tmp_path / "a"), "png")
    sink = cli.FrameSink(cli.PngWriter(str(tmp_path / "b")))
    for c in chunks:
        sink.put(c)
    sink.close()
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == [f"frame_{i:06d}.png" for i in range(12)]
    for name in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    cli.save_frames(whole, str(tmp_path / "c.pt"), "pt")
    assert torch.equal(torch.load(tmp_path / "c.pt", weights_only=True), whole)
