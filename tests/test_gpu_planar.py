"""-m gpu: csrc/svr_planar.hip through HipOps.planar_codes against its specification planar.planar_codes_torch -- EQUAL, every
subsampling, depth, range and siting, BT.2020 and one of the other matrices (every result is an integer code: a mismatch is a finding,
not a tolerance) --, every 10-bit luma code against the extreme chroma codes, unaligned views, its refusals, and the command line's
FrameSource on the planar route on the device.

Outputs live in tests/guarded_out.py buffers and the guards must stay intact.  The output is uint16 and every bit pattern is a code a
kernel may store, so "no poison left" says nothing here: an element never written holds the guard pattern 0xA5A5 and fails the
comparison with the specification instead (a case whose specification has that very code at that very place aside)."""
import ctypes

import pytest
import torch

from conftest import sub
from guarded_out import guarded
from planar_cases import (BITS, RANGES, SHAPES, SOURCE_H, SOURCE_T, SOURCE_W, SUBS, chain_of_the_whole, load_cli, planar_source,
                          random_planes, shape_id, sitings, source_planes)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


def run_kernel(hip, planes, sub_, bits, T, H, W, matrix, range_, siting):
    g = guarded((T, H, W, 3), torch.uint16)
    out = hip.planar_codes(planes.cuda(), sub_, bits, T, H, W, matrix, range_, siting, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t
    g.assert_guards(f"planar_codes {sub_} {bits} {(T, H, W)} {matrix} {range_} {siting}")
    return out.cpu()


@pytest.mark.parametrize("sub_", SUBS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_kernel_equals_the_specification(hip, shape, sub_):
    planar = sub("planar")
    T, H, W = shape
    for bits in BITS:
        for k, (range_, siting) in enumerate((r, s) for r in RANGES for s in sitings(sub_)):
            planes = random_planes(sub_, bits, T, H, W, seed=sum(shape) + bits + k, whole_container=(k == 0))
            for matrix in ("bt2020", ("bt709", "bt601")[k % 2]):
                want = planar.planar_codes_torch(planes, sub_, bits, T, H, W, matrix, range_, siting)
                got = run_kernel(hip, planes, sub_, bits, T, H, W, matrix, range_, siting)
                assert got.shape == want.shape and torch.equal(got, want), (bits, matrix, range_, siting, int((got != want).sum()))


def test_every_ten_bit_luma_code_against_the_extreme_chroma_codes(hip):
    """All 1024 Y codes in flat-chroma 16 x 64 frames, one frame per pair of Cb, Cr in 0, 512, 1023, 0xFFFF (which counts as 1023):
    negative numerators, both clamps of the code and the clamp of the sample, in the vector kernel."""
    planar = sub("planar")
    H, W = 16, 64
    values = (0, 512, 1023, 0xFFFF)
    luma = torch.arange(1024)
    for sub_ in SUBS:
        hc, wc = planar.chroma_dims(sub_, H, W)
        frames = [torch.cat([luma, torch.full((hc * wc,), cb), torch.full((hc * wc,), cr)]) for cb in values for cr in values]
        planes = torch.stack(frames).to(torch.int32).to(torch.uint16)
        for range_ in RANGES:
            for siting in sitings(sub_):
                want = planar.planar_codes_torch(planes, sub_, 10, 16, H, W, "bt2020", range_, siting)
                assert torch.equal(run_kernel(hip, planes, sub_, 10, 16, H, W, "bt2020", range_, siting), want), (sub_, range_, siting)
        assert int(want.to(torch.int64).min()) == 0 and int(want.to(torch.int64).max()) == 65535


def test_output_allocated_by_the_op_and_unaligned_views(hip):
    """Without ``out`` the op allocates; planes that start 2 or 4 bytes into an allocation, and an ``out`` one element into its buffer,
    take the element kernel and give the same codes (the vector kernel needs both ends on 16 bytes)."""
    planar = sub("planar")
    T, H, W = 2, 6, 32
    for sub_ in SUBS:
        for bits in BITS:
            siting = sitings(sub_)[-1]
            planes = random_planes(sub_, bits, T, H, W, seed=4)
            want = planar.planar_codes_torch(planes, sub_, bits, T, H, W, "bt2020", "tv", siting)
            got = hip.planar_codes(planes.cuda(), sub_, bits, T, H, W, "bt2020", "tv", siting)
            assert got.dtype == torch.uint16 and got.is_cuda and torch.equal(got.cpu(), want), (sub_, bits)
            size = planes.element_size()
            for off in (2, 4):
                store = torch.empty(planes.numel() + off // size, dtype=planes.dtype, device="cuda")
                shifted = store[off // size:].view(planes.shape)
                shifted.copy_(planes)
                assert shifted.is_contiguous() and shifted.data_ptr() % 16 == off
                g = guarded((T, H, W, 3), torch.uint16)
                hip.planar_codes(shifted, sub_, bits, T, H, W, "bt2020", "tv", siting, out=g.t)
                torch.cuda.synchronize()
                g.assert_guards(f"{sub_} {bits} planes off {off}")
                assert torch.equal(g.t.cpu(), want), (sub_, bits, off)
            g = guarded((T * H * W * 3 + 1,), torch.uint16)
            out = g.t[1:].view(T, H, W, 3)
            hip.planar_codes(planes.cuda(), sub_, bits, T, H, W, "bt2020", "tv", siting, out=out)
            torch.cuda.synchronize()
            g.assert_guards(f"{sub_} {bits} out off 2")
            assert torch.equal(out.cpu(), want) and bool(g.poisoned()[0]), (sub_, bits)


def test_refusals_name_the_argument_and_launch_nothing(hip):
    hip_lib = sub("hip_lib")
    T, H, W = 2, 6, 8
    p8, p10 = random_planes("422", 8, T, H, W, 0).cuda(), random_planes("422", 10, T, H, W, 0).cuda()
    out = guarded((T, H, W, 3), torch.uint16)
    for kw, word in ((dict(sub="411"), "sub must be"), (dict(bits=9), "bits must be"), (dict(matrix="bt2020c"), "matrix must be"),
                     (dict(range_="full"), "range_ must be"), (dict(siting="topleft"), "siting must be"), (dict(T=0), "T, H, W must be positive"),
                     (dict(planes=p8), "planes must be torch.uint16"), (dict(W=9), "planes must hold"),
                     (dict(planes=p10.cpu()), "planes must live on"),
                     (dict(planes=torch.empty((T, 2 * p10.shape[1]), dtype=torch.uint16, device="cuda")[:, ::2]), "planes must be contiguous"),
                     (dict(out=torch.empty((T, H, W, 3), dtype=torch.int16, device="cuda")), "out must be"),
                     (dict(out=guarded((T, H, W, 4), torch.uint16).t), "out must be")):
        args = {**dict(planes=p10, sub="422", bits=10, T=T, H=H, W=W, matrix="bt709", range_="tv", siting="left", out=out.t), **kw}
        with pytest.raises(ValueError, match="planar_codes: " + word):
            hip.planar_codes(**args)
    # the C entry point itself, device pointers: wrong byte counts, a siting the subsampling does not take, out inside planes
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = hip.lib
    n_in, n_out = p10.numel() * 2, T * H * W * 6
    for nin, nout, word in ((n_in - 2, n_out, b"planes_bytes"), (n_in + 16, n_out, b"planes_bytes"), (n_in, n_out - 2, b"out_bytes"), (n_in, n_in, b"out_bytes")):
        assert L.svr_planar_codes(p(p10), nin, 1, 10, T, H, W, 0, 0, 1, p(out.t), nout, None) != 0
        assert word in L.svr_last_error()
    assert L.svr_planar_codes(p(p10), n_in, 1, 10, T, H, W, 0, 0, 2, p(out.t), n_out, None) != 0
    assert b"SVR_PLANAR_420 only" in L.svr_last_error()
    big = torch.empty(n_out // 2 + n_in // 2, dtype=torch.uint16, device="cuda")
    assert L.svr_planar_codes(p(big), n_in, 1, 10, T, H, W, 0, 0, 1, p(big[8:]), n_out, None) != 0
    assert b"out overlaps planes" in L.svr_last_error()
    with pytest.raises(hip_lib.HipLibraryError, match="matrix"):
        hip_lib.check(L.svr_planar_codes(p(p10), n_in, 1, 10, T, H, W, 7, 0, 1, p(out.t), n_out, None), "svr_planar_codes")
    torch.cuda.synchronize()
    out.assert_guards("refused calls")
    assert bool(out.poisoned().all())                                          # nothing was launched: the payload is untouched


def test_frame_source_on_the_planar_route_on_the_device(hip, tmp_path, monkeypatch):
    """yuv422p10le behind the stand-in ffmpeg, field matching, chunks of 5: the chunks on the device equal the CPU chain of
    tests/test_planar.py applied to the codes of the whole clip."""
    monkeypatch.setattr(sub("planar"), "ENABLED", True)
    cli = load_cli("svr_cli_gpu_planar")
    planes = source_planes("422", 10)
    want = chain_of_the_whole(planes, "422", 10, "bt709", "tv", "left", ("tff", "match"))
    src, _ = planar_source(cli, tmp_path, planes, "yuv422p10le", 5, fields=("tff", "match"), ops=hip, device="cuda:0")
    assert src.planar == ("422", 10, "bt709", "tv", "left") and all(b.is_pinned() for b in src.buffers)
    got = list(src.chunks())
    assert [c.shape[0] for c in got] == [5, 5, 3] and all(c.is_cuda and c.dtype == torch.float32 for c in got)
    assert torch.equal(torch.cat(got).cpu(), want) and want.shape == (SOURCE_T, SOURCE_H, SOURCE_W, 3)
    assert not src.thread.is_alive()
