"""-m "not gpu": colorfix.correct -- which calls go to the colour-correction kernels (csrc/svr_colorfix.hip) and which stay on
colorfix.METHODS -- and the host side of the five entry points: header, ctypes table, build list, and the refusals every one of
them makes before any launch.  No device is needed: a stand-in records what ``correct`` hands to the ops, and a refused call
launches nothing."""
import os
import re
import shutil

import pytest
import torch

from conftest import ROOT, sub
from ops_reference import TorchOps

ALL = ("lab", "wavelet_adaptive", "hsv", "wavelet", "adain")


def _pair(seed=11, shape=(2, 3, 24, 40)):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * 0.9, (torch.rand(shape, generator=g) * 2 - 1) * 0.6 + 0.1


class _AsCuda(torch.Tensor):
    """A CPU tensor that says it lives on the device: ``correct`` decides its route from is_cuda / dtype / shape alone."""

    @staticmethod
    def of(t):
        return t.as_subclass(_AsCuda)

    @property
    def is_cuda(self):
        return True


class _Recorder:
    """Stands in for HipOps: records every call (name, shapes, strides) and answers with colorfix's own torch functions."""

    def __init__(self, cf, fail=None):
        self.cf, self.calls, self.fail = cf, [], fail

    def _note(self, name, *tensors):
        self.calls.append((name, [(tuple(t.shape), tuple(t.stride())) for t in tensors if t is not None]))
        if self.fail == name:
            raise RuntimeError(f"{name} failed (rc=-1): refused")

    @staticmethod
    def _plain(t):
        return t.as_subclass(torch.Tensor)

    def wavelet_reconstruct(self, content, style, out=None):
        self._note("wavelet_reconstruct", content, style)
        out = self.cf.wavelet_reconstruction(self._plain(content), self._plain(style))
        return _AsCuda.of(out.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))       # a dense [T, H, W, 3] buffer, as HipOps answers

    def lab_planes(self, base, style, c_lab=None, s_lab=None):
        self._note("lab_planes", base, style)
        to01 = lambda x: ((self._plain(x) + 1.0) * 0.5).clamp(0.0, 1.0)
        planes = lambda x: self.cf.rgb_to_lab(to01(x)).permute(1, 0, 2, 3).reshape(3, -1).contiguous()
        return planes(base), planes(style)

    def lab_merge(self, c_L, m_L, m_a, m_b, luminance_weight, shape, out=None):
        self._note("lab_merge", c_L, m_L, m_a, m_b)
        T, H, W = shape
        L = c_L if m_L is None else c_L * luminance_weight + m_L * (1.0 - luminance_weight)
        lab = torch.stack([L.reshape(T, H, W), m_a.reshape(T, H, W), m_b.reshape(T, H, W)], dim=1)
        return self.cf.lab_to_rgb(lab) * 2.0 - 1.0

    def adain(self, content, style, eps=1e-5, out=None):
        self._note("adain", content, style)
        return self.cf.adaptive_instance_normalization(self._plain(content), self._plain(style), eps)


@pytest.mark.parametrize("method", ALL)
def test_correct_is_the_methods_table_wherever_no_kernel_serves(method):
    """CPU tensors, no ops, the torch double of the ops, impl="torch": METHODS[method], bit for bit."""
    cf = sub("colorfix")
    content, style = _pair()
    want = cf.METHODS[method](content.clone(), style.clone())
    rec = _Recorder(cf)
    for kw in (dict(), dict(ops=None), dict(ops=TorchOps("cpu")), dict(ops=rec), dict(ops=rec, impl="torch"),
               dict(ops=TorchOps("cpu"), impl="torch")):
        got = cf.correct(content.clone(), style.clone(), method, **kw)
        assert got.dtype == want.dtype and torch.equal(got, want), (method, kw)
    assert rec.calls == []                                        # CPU tensors never reach the ops
    got = cf.correct(_AsCuda.of(content.clone()), _AsCuda.of(style.clone()), method, ops=rec, impl="torch")
    assert torch.equal(got, want) and rec.calls == []
    with pytest.raises(ValueError, match="impl"):
        cf.correct(content, style, method, impl="hip")


def test_which_methods_route_to_the_device_and_with_what_layouts():
    """The pipeline's two views -- channels-last frames and a slice of a [C, T, H + 3, W + 5] buffer -- arrive at the ops as they
    lie: same shapes, their own strides, no copy."""
    cf = sub("colorfix")
    T, H, W = 2, 24, 40
    content, style = _pair(shape=(T, 3, H, W))
    frames = content.permute(0, 2, 3, 1).contiguous()                                   # [T, H, W, 3], as ``final[w0:w1]``
    big = torch.full((3, T, H + 3, W + 5), float("nan"))
    big[:, :, :H, :W] = style.permute(1, 0, 2, 3)
    c_view, s_view = frames.permute(0, 3, 1, 2), big.permute(1, 0, 2, 3)[:, :, :H, :W]
    shape, c_st, s_st = (T, 3, H, W), (H * W * 3, 1, W * 3, 3), ((H + 3) * (W + 5), T * (H + 3) * (W + 5), W + 5, 1)
    assert c_view.stride() == c_st and s_view.stride() == s_st
    n = T * H * W
    expect = {
        "wavelet": [("wavelet_reconstruct", [(shape, c_st), (shape, s_st)])],
        "adain": [("adain", [(shape, c_st), (shape, s_st)])],
        "wavelet_adaptive": [("wavelet_reconstruct", [(shape, c_st), (shape, s_st)])],
        "lab": [("wavelet_reconstruct", [(shape, c_st), (shape, s_st)]), ("lab_planes", [(shape, c_st), (shape, s_st)]),
                ("lab_merge", [((n,), (1,))] * 4)],
        "hsv": [],
    }
    for method in ALL:
        rec = _Recorder(cf)
        got = cf.correct(_AsCuda.of(c_view), _AsCuda.of(s_view), method, ops=rec)
        assert rec.calls == expect[method], (method, rec.calls)
        assert cf.routes_to_device(_AsCuda.of(c_view), _AsCuda.of(s_view), method, rec) == (method != "hsv")
        # (the stand-in answers with colorfix's own functions, so the composition around the ops is the specification's too)
        want = cf.METHODS[method](c_view, s_view)
        assert got.shape == want.shape and torch.equal(got.as_subclass(torch.Tensor), want), method


def test_what_does_not_route():
    """bf16 frames (output_dtype=None), unequal shapes, one operand on the CPU, ops without the methods: METHODS, no call."""
    cf = sub("colorfix")
    content, style = _pair()
    rec = _Recorder(cf)
    cuda = _AsCuda.of
    small = torch.nn.functional.interpolate(style, size=(12, 20), mode="bilinear", align_corners=False)
    for method in ALL:
        for c, s in ((cuda(content.bfloat16()), cuda(style.bfloat16())), (cuda(content), cuda(style.bfloat16())),
                     (cuda(content), cuda(small)), (cuda(content), style), (content, cuda(style)),
                     (cuda(content[:, :1]), cuda(style[:, :1]))):
            assert not cf.routes_to_device(c, s, method, rec)
        for c, s in ((content.bfloat16(), style.bfloat16()), (content, small)):
            got = cf.correct(cuda(c.clone()), cuda(s.clone()), method, ops=rec)
            want = cf.METHODS[method](c.clone(), s.clone())
            assert got.dtype == want.dtype and torch.equal(got.as_subclass(torch.Tensor), want), method
        assert not cf.routes_to_device(cuda(content), cuda(style), method, TorchOps("cpu"))
        assert not cf.routes_to_device(cuda(content), cuda(style), method, None)
    assert rec.calls == []


@pytest.mark.parametrize("method,call", [("wavelet", "wavelet_reconstruct"), ("adain", "adain"), ("lab", "wavelet_reconstruct"),
                                         ("lab", "lab_planes"), ("lab", "lab_merge"), ("wavelet_adaptive", "wavelet_reconstruct")])
def test_a_failing_library_call_raises_and_nothing_falls_back(method, call):
    cf = sub("colorfix")
    content, style = _pair()
    rec = _Recorder(cf, fail=call)
    with pytest.raises(RuntimeError, match=call):
        cf.correct(_AsCuda.of(content), _AsCuda.of(style), method, ops=rec)
    assert rec.calls[-1][0] == call


def test_pipeline_phase_four_goes_through_correct():
    src = open(os.path.join(ROOT, "comfyui-seedvr2_videoupscaler_amd", "pipeline.py")).read()
    assert 'colorfix.correct(sample, ref, color_correction, ops=getattr(runner.dit, "ops", None))' in src
    assert "colorfix.METHODS[color_correction](" not in src


# ---------------------------------------------------------------------------------------------------------------- C ABI
ENTRY_POINTS = {"svr_wavelet_reconstruct": 11, "svr_lab_planes": 11, "svr_lab_merge": 12, "svr_chan_stats": 12, "svr_adain_apply": 11}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_entry_points_are_declared_and_refuse_before_any_launch():
    """Header, ctypes table and build list know the five entry points and the workspace query; the ABI stays 9; each entry point
    refuses a null pointer, T < 1, H or W < 1, a short workspace and a non-fp32 kind on the host, naming the argument.  No device
    is needed: nothing is launched."""
    import ctypes
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    for name, n_args in ENTRY_POINTS.items():
        decl = re.search(rf"int {name}\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == n_args == len(hip_lib.SYMBOLS[name][1]), name
    assert re.search(r"int64_t svr_colorfix_workspace_bytes\(int32_t T\);", src) and len(hip_lib.SYMBOLS["svr_colorfix_workspace_bytes"][1]) == 1
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9 and L.svr_abi_version() == 9
    assert re.search(r"v9, additive: \+ svr_wavelet_reconstruct\(\)", src)
    assert '#include "svr_colorfix.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert os.path.join(hip_lib.CSRC, "svr_colorfix.hip") in hip_lib.sources()

    T, H, W = 2, 5, 7
    need = L.svr_colorfix_workspace_bytes(T)
    assert need >= 2 * T * 3 * 2 * 8 and L.svr_colorfix_workspace_bytes(0) == 0 and L.svr_colorfix_workspace_bytes(-3) == 0
    buf = (ctypes.c_char * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)                      # never dereferenced: every call below is refused on the host
    st = lambda *v: (ctypes.c_int64 * 4)(*v)
    dense = st(3 * H * W, H * W, W, 1)
    orders = {
        "svr_wavelet_reconstruct": ("content", "content_strides", "style", "style_strides", "out", "out_strides", "T", "H", "W", "kind", "stream"),
        "svr_lab_planes": ("base", "base_strides", "style", "style_strides", "c_lab", "s_lab", "T", "H", "W", "kind", "stream"),
        "svr_lab_merge": ("c_L", "m_L", "m_a", "m_b", "luminance_weight", "out", "out_strides", "T", "H", "W", "kind", "stream"),
        "svr_chan_stats": ("content", "content_strides", "style", "style_strides", "stats", "T", "H", "W", "kind", "workspace",
                           "workspace_bytes", "stream"),
        "svr_adain_apply": ("content", "content_strides", "stats", "eps", "out", "out_strides", "T", "H", "W", "kind", "stream"),
    }
    for name, order in orders.items():
        assert len(order) == ENTRY_POINTS[name]
        good = {k: p for k in order}
        good.update({k: dense for k in order if k.endswith("_strides")})
        good.update(T=T, H=H, W=W, kind=1, stream=None, luminance_weight=0.8, eps=1e-5, workspace_bytes=need)

        def refused(word, **kw):
            a = dict(good)
            a.update(kw)
            assert getattr(L, name)(*[a[k] for k in order]) != 0, (name, kw)
            msg = L.svr_last_error()
            assert name.encode() + b":" in msg and word in msg, (name, kw, msg)

        for k in order:
            if good[k] is p or k.endswith("_strides"):
                refused(k.encode(), **{k: None})                 # a null pointer, named
        refused(b"1 <= T", T=0)
        refused(b"1 <= T", T=-1)
        refused(b"H >= 1", H=0)
        refused(b"W >= 1", W=0)
        refused(b"W >= 1", W=-4)
        refused(b"1 <= T", T=21846)                               # T * 3 planes index a 16-bit grid dimension
        refused(b"below 2^24", T=4096, H=4096, W=7)               # one workgroup per 256 pixels of a row: 32-bit thread count
        for kind in (0, 2, 7):                                    # SVR_STORE_BF16, SVR_STORE_H16, nonsense
            refused(b"kind", kind=kind)
        for k in order:
            if k.endswith("_strides"):
                refused(k.encode(), **{k: st(3 * H * W, H * W, -W, 1)})
                if k == "out_strides":
                    refused(k.encode(), **{k: st(3 * H * W, 0, W, 1)})
        if "workspace_bytes" in order:
            refused(b"workspace_bytes", workspace_bytes=need - 1)
            refused(b"workspace_bytes", workspace_bytes=0)
            refused(b"workspace", workspace=ctypes.c_void_p(p.value + 4))
    # luminance_weight >= 1: m_L is not read, so a null m_L is not what gets refused (the next bad argument is)
    a = dict(c_L=p, m_L=None, m_a=p, m_b=p, luminance_weight=1.0, out=p, out_strides=dense, T=0, H=H, W=W, kind=1, stream=None)
    assert L.svr_lab_merge(*[a[k] for k in orders["svr_lab_merge"]]) != 0 and b"m_L" not in L.svr_last_error() and b"1 <= T" in L.svr_last_error()
