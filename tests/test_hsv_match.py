"""-m "not gpu": the HSV half of the colour correction (colorfix.hsv_spec / wavelet_adaptive_spec / hue_match_spec, csrc/svr_hsv.hip)
without a device.

  HUE_EDGES          bin membership by fp32 comparisons = the masks torch evaluates, at every edge and its fp32 neighbours
  remainder          q < 0 ? q + 6 : q  =  torch.remainder(q, 6) on [-1, 1], both zeros included
  spec vs torch      equal bin sizes: hsv_spec = METHODS["hsv"] bit for bit; unequal sizes: bit-equal at every pixel whose nearest-rank
                     index agrees with torch's linspace route (a condition, not a tolerance; the disagreements are printed)
  min_pixels         100 / 101 on either side, bin 11 over bin 0 and the reverse, h >= 1, a NaN hue
  route              colorfix.correct hands hsv and the HSV half of wavelet_adaptive to the four calls only where the ops have them,
                     HSV_MATCH is set and the plane fits; a failing call raises
  host               the five entry points: header, ctypes table, workspace size, refusals before any launch"""
import os
import re
import shutil

import pytest
import torch

from conftest import ROOT, sub
from test_colorfix_device import _AsCuda, _Recorder

F32 = torch.float32


def _next(x, up):
    return torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(float("inf") if up else float("-inf"), dtype=F32)).item()


# ---------------------------------------------------------------------------------------------------------------- edges
def test_hue_edges_are_the_values_torch_compares_with():
    cf = sub("colorfix")
    assert len(cf.HUE_EDGES) == 13 and cf.HUE_EDGES[0] == 0.0 and cf.HUE_EDGES[12] == 1.0
    assert cf.HUE_WRAP_EDGE == cf.HUE_EDGES[11]                   # float32(1 - 1/12) == float32(11 * (1/12)): bin 0 holds all of bin 11
    assert list(cf.HUE_EDGES) == sorted(set(cf.HUE_EDGES))
    for k in range(13):
        assert cf.HUE_EDGES[k] == torch.tensor(k * (1.0 / 12), dtype=F32).item()
    below = [k for k in range(13) if cf.HUE_EDGES[k] < k * (1.0 / 12)]
    assert below == [5, 7, 10], below                             # there the fp32 edge lies below the double; x >= edge still holds at x = edge
    probes = [-1.0, -0.0, 0.0, 1e-45, 0.5, 1.0, 1.5, float("inf"), float("-inf"), float("nan")]
    for e in list(cf.HUE_EDGES) + [cf.HUE_WRAP_EDGE]:
        probes += [_next(e, False), e, _next(e, True)]
    h = torch.tensor(probes, dtype=F32)
    width = 1.0 / 12
    seen = torch.zeros(h.numel(), dtype=torch.int64)
    for k in range(12):
        lo, hi = k * width, (k + 1) * width                       # hue_conditional_saturation_match's own expressions
        want = (((h >= 0) & (h < hi)) | (h >= 1.0 - width)) if k == 0 else ((h >= lo) & (h < hi))
        got = cf.hue_bin_mask(h, k)
        assert torch.equal(got, want), (k, h[got != want])
        seen += got.long()
        if k > 0:                                                 # the edge itself belongs to the bin it opens
            assert bool(cf.hue_bin_mask(torch.tensor([cf.HUE_EDGES[k]]), k)[0])
            assert not bool(cf.hue_bin_mask(torch.tensor([_next(cf.HUE_EDGES[k], False)]), k)[0])
    in11 = cf.hue_bin_mask(h, 11)
    assert bool((cf.hue_bin_mask(h, 0) | ~in11).all())            # bin 11 is inside bin 0
    assert bool((seen[in11] == 2).all()) and bool((seen[~in11] <= 1).all())
    assert bool(cf.hue_bin_mask(torch.tensor([1.0, 1.5, float("inf")]), 0).all()) and int(seen[torch.isnan(h)].sum()) == 0
    assert int(seen[h < 0].sum()) == 0 and bool(cf.hue_bin_mask(torch.tensor([-0.0]), 0)[0])


def test_remainder_restated_for_the_kernel():
    g = torch.Generator().manual_seed(1)
    q = torch.cat([torch.rand(200_000, generator=g) * 2 - 1, torch.tensor([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, -2.0 ** -24, 2.0 ** -24, -1e-8])])
    want = torch.remainder(q, 6.0)
    got = torch.where(q < 0, q + 6.0, q)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_nearest_rank_index():
    cf = sub("colorfix")
    for n in (2, 3, 101, 4097):
        assert torch.equal(cf.nearest_rank_index(n, n), torch.arange(n))
    for n_s, n_r in ((2, 1), (2, 7), (101, 1000), (1000, 101), (7, 2), (3, 2 ** 30)):
        idx = cf.nearest_rank_index(n_s, n_r)
        assert idx.dtype == torch.int64 and idx[0] == 0 and idx[-1] == n_r - 1 and bool((idx[1:] >= idx[:-1]).all())
        assert idx.tolist() == [(k * (n_r - 1)) // (n_s - 1) for k in range(n_s)]
    with pytest.raises(ValueError):
        cf.nearest_rank_index(1, 5)


# ---------------------------------------------------------------------------------------------------------------- spec vs torch
def _pair(T, H, W, seed=11):
    """the fixture of tests/test_gpu_colorfix.py"""
    g = torch.Generator().manual_seed(seed)
    content = (torch.rand(T, 3, H, W, generator=g) * 2 - 1) * 0.9
    style = (torch.rand(T, 3, H, W, generator=g) * 2 - 1) * 0.6 + 0.1
    return content, style


def test_spec_equals_torch_where_the_bins_have_equal_sizes():
    """content = the style's pixels in another order: every bin has n_s == n_r, so histogram_match takes no linspace and the CPU's
    sort (stable in practice) leaves nothing to differ."""
    cf = sub("colorfix")
    _, style = _pair(2, 48, 80)
    T, _, H, W = style.shape
    perm = torch.randperm(T * H * W, generator=torch.Generator().manual_seed(2))
    content = style.permute(1, 0, 2, 3).reshape(3, -1)[:, perm].reshape(3, T, H, W).permute(1, 0, 2, 3).contiguous()
    want = cf.METHODS["hsv"](content, style)
    assert torch.equal(cf.hsv_spec(content, style), want)
    assert not torch.equal(want, content)                         # (the matching moved something)
    assert torch.equal(cf.wavelet_adaptive_spec(content, style), cf.METHODS["wavelet_adaptive"](content, style))


def test_spec_equals_torch_wherever_the_nearest_rank_agrees():
    cf = sub("colorfix")
    content, style = _pair(3, 96, 160)
    to01 = lambda x: ((x + 1.0) * 0.5).clamp(0.0, 1.0)
    c, s = cf.rgb_to_hsv(to01(content)), cf.rgb_to_hsv(to01(style))
    ch, cs, sh = c[:, 0].flatten(), c[:, 1].flatten(), s[:, 0].flatten()
    ss = s[:, 1].flatten()
    agree = torch.ones(ch.numel(), dtype=torch.bool)
    tied = torch.zeros(ch.numel(), dtype=torch.bool)              # shares its saturation with another pixel of its bin
    stable = cs.clone()                                           # torch's route with its sort made stable: only the index differs
    positions = 0
    for k in range(12):
        where = cf.hue_bin_mask(ch, k).nonzero().flatten()
        ref = ss[cf.hue_bin_mask(sh, k)]
        n_s, n_r = where.numel(), ref.numel()
        assert n_s > 100 and n_r > 100 and n_s != n_r             # every bin is matched, between unequal sizes
        torch_idx = (torch.linspace(0, 1, n_s) * (n_r - 1)).long().clamp_(0, n_r - 1)
        same = torch_idx == cf.nearest_rank_index(n_s, n_r)
        positions += int((~same).sum())
        order = torch.sort(cf.sort_key(cs[where]), stable=True).indices
        agree[where[order]] = same                                # (a later bin overwrites, as its values do)
        stable[where[order]] = torch.sort(ref).values[torch_idx]
        _, inverse, counts = torch.unique(cs[where], return_inverse=True, return_counts=True)
        tied[where] = counts[inverse] > 1
    want_sat = cf.hue_conditional_saturation_match(c[:, 0], c[:, 1], s[:, 0], s[:, 1]).flatten()
    got_sat = cf.hue_match_spec(c[:, 0], c[:, 1], s[:, 0], s[:, 1]).flatten()
    diff = got_sat != want_sat
    print(f"nearest rank: {positions} positions differ from torch's linspace route in {int((~agree).sum())} of {agree.numel()} pixels; "
          f"{int(diff.sum())} saturations differ, max {float((got_sat - want_sat).abs().max()):.3e}; {int(tied.sum())} pixels tie within "
          f"their bin, {int((diff & agree & tied).sum())} of them in the other order of torch.sort")
    # the same sort on both sides: bit-equal wherever the two index vectors agree, every pixel counted
    assert torch.equal(got_sat[agree].view(torch.int32), stable[agree].view(torch.int32))
    # against torch's own function the order of tied saturations is torch.sort's choice (not stable: two tied pixels of this
    # fixture come out exchanged), so there the condition holds at every pixel that does not tie, and a tied pixel holds a value
    # torch gave to a pixel it ties with
    assert not bool((diff & agree & ~tied).any())
    for i in (diff & agree & tied).nonzero().flatten().tolist():
        mates = (cs == cs[i]) & tied
        assert bool((want_sat[mates] == got_sat[i]).any()), i
    agree = agree & ~(diff & tied)
    px = agree.reshape(3, 1, 96, 160).expand(3, 3, 96, 160)
    for method, spec in (("hsv", cf.hsv_spec), ("wavelet_adaptive", cf.wavelet_adaptive_spec)):
        want, got = cf.METHODS[method](content, style), spec(content, style)
        d = (got - want).abs()
        print(f"{method}: {int((got != want).sum())} values differ, share off by more than 2e-5: {float((d > 2e-5).float().mean()):.3e}, "
              f"max {float(d.max()):.3e}")
        assert torch.equal(got[px].view(torch.int32), want[px].view(torch.int32)), method


# ---------------------------------------------------------------------------------------------------------------- min_pixels
def _planes(cf, counts, seed):
    """hue and saturation planes holding ``counts[name]`` pixels of each named hue range, in random order, distinct saturations"""
    e = cf.HUE_EDGES
    ranges = {"bin0": (0.0, e[1]), "bin3": (e[3], e[4]), "bin4": (e[4], e[5]), "bin5": (e[5], e[6]), "bin11": (e[11], 1.0),
              "over": (1.0, 2.0), "nan": None}
    g = torch.Generator().manual_seed(seed)
    hs = []
    for name, n in counts.items():
        if ranges[name] is None:
            hs.append(torch.full((n,), float("nan")))
        else:
            lo, hi = ranges[name]
            h = lo + torch.rand(n, generator=g) * (hi - lo)
            hs.append(torch.where(h < hi, h, torch.full_like(h, lo)))           # (a product that rounded up to the open end)
    h = torch.cat(hs)
    n = h.numel()
    sat = (torch.randperm(4 * n, generator=g)[:n].float() + 0.5) / (4 * n)     # distinct: nothing ties
    perm = torch.randperm(n, generator=g)
    return h[perm].contiguous(), sat[perm].contiguous()


MIN_PIXEL_CASES = {
    # bins of equal sizes on both sides wherever they qualify, so torch's own function (no linspace, no ties) is the oracle
    "101_and_100": (dict(bin3=101, bin4=100, bin5=101, nan=7), dict(bin3=101, bin4=101, bin5=100, nan=3), {3}),
    "bin11_over_bin0": (dict(bin0=30, bin11=150, over=5), dict(bin0=25, bin11=150, over=10), {0, 11}),
    "bin0_over_bin11": (dict(bin0=60, bin11=50, over=20, bin3=100), dict(bin0=70, bin11=50, over=10, bin3=500), {0}),
    "wrap_only_through_h_above_one": (dict(over=101, bin11=100), dict(over=101, bin11=100), {0}),
    "nothing_qualifies": (dict(bin0=100, bin3=100, bin11=0, nan=50), dict(bin0=500, bin3=500), set()),
}


@pytest.mark.parametrize("name", sorted(MIN_PIXEL_CASES))
def test_min_pixels_and_the_wrap(name):
    cf = sub("colorfix")
    c_counts, s_counts, qualifying = MIN_PIXEL_CASES[name]
    c_h, c_s = _planes(cf, c_counts, 1)
    s_h, s_s = _planes(cf, s_counts, 2)
    assert {k for k in range(12) if int(cf.hue_bin_mask(c_h, k).sum()) > 100 and int(cf.hue_bin_mask(s_h, k).sum()) > 100} == qualifying
    for k in qualifying:
        assert int(cf.hue_bin_mask(c_h, k).sum()) == int(cf.hue_bin_mask(s_h, k).sum())
    got = cf.hue_match_spec(c_h, c_s, s_h, s_s)
    want = cf.hue_conditional_saturation_match(c_h, c_s, s_h, s_s)
    assert torch.equal(got, want)
    touched = torch.zeros_like(c_h, dtype=torch.bool)
    for k in qualifying:
        touched |= cf.hue_bin_mask(c_h, k)
    assert torch.equal(got[~touched], c_s[~touched]) and bool((got[touched] != c_s[touched]).any() or not qualifying)
    assert torch.equal(got[torch.isnan(c_h)], c_s[torch.isnan(c_h)])
    if name == "bin11_over_bin0":                                 # the pixels of [e_11, 1) hold bin 11's values, the others bin 0's
        in11 = cf.hue_bin_mask(c_h, 11)
        assert torch.equal(got[in11].sort().values, s_s[cf.hue_bin_mask(s_h, 11)].sort().values)
    if name == "bin0_over_bin11":
        in0 = cf.hue_bin_mask(c_h, 0)
        assert torch.equal(got[in0].sort().values, s_s[cf.hue_bin_mask(s_h, 0)].sort().values)
    # shapes pass through
    assert cf.hue_match_spec(c_h.reshape(1, -1), c_s.reshape(1, -1), s_h, s_s).shape == (1, c_h.numel())


def test_ties_go_to_the_lower_flat_index_of_the_whole_plane():
    cf = sub("colorfix")
    e = cf.HUE_EDGES
    # bin 0 from three classes interleaved in the plane, all saturations tied: the matched values must ascend with the flat index
    c_h = torch.tensor([e[11], 0.01, 1.0, 0.02, e[11] + 0.01, 1.5] * 40)
    c_s = torch.full_like(c_h, 0.5)
    s_h = torch.full((150,), 0.03)
    s_s = torch.rand(150, generator=torch.Generator().manual_seed(3))
    got = cf.hue_match_spec(c_h, c_s, s_h, s_s)
    assert bool((got[1:] >= got[:-1]).all()) and got[0] == s_s.min() and got[-1] == s_s.max()


# ---------------------------------------------------------------------------------------------------------------- route
class _HsvRecorder(_Recorder):
    """the recorder of test_colorfix_device with the four HSV calls, answering with the specification's own functions"""

    def hsv_planes(self, content, style, c_hsv=None, s_hs=None):
        self._note("hsv_planes", content, style)
        to01 = lambda x: ((self._plain(x) + 1.0) * 0.5).clamp(0.0, 1.0)
        planes = lambda x: self.cf.rgb_to_hsv(to01(x)).permute(1, 0, 2, 3).reshape(3, -1).contiguous()
        return planes(content), planes(style)[:2].contiguous()

    def hue_match(self, c_h, c_s, s_h, s_s, out=None):
        self._note("hue_match", c_h, c_s, s_h, s_s)
        res = self.cf.hue_match_spec(c_h, c_s, s_h, s_s)
        assert out is not None and out.data_ptr() == c_s.data_ptr()          # the saturation plane is matched in place
        out.copy_(res)
        return out

    def _hsv(self, h, sat, v, shape):
        T, H, W = shape
        hsv = torch.stack([h.reshape(T, H, W), sat.reshape(T, H, W), v.reshape(T, H, W)], dim=1)
        return self.cf.hsv_to_rgb(hsv).clamp(0.0, 1.0) * 2.0 - 1.0

    def hsv_merge(self, h, sat, v, shape, out=None):
        self._note("hsv_merge", h, sat, v)
        return self._hsv(h, sat, v, shape)

    def adaptive_blend(self, base, content, style, h, sat, v, threshold=0.15, sharpness=5.0, out=None):
        self._note("adaptive_blend", base, content, style, h, sat, v)
        base, content, style = (self._plain(x) for x in (base, content, style))
        T, _, H, W = base.shape
        w, _ = self.cf.adaptive_weight(base, content, style, threshold, sharpness)
        return base * (1.0 - w) + self._hsv(h, sat, v, (T, H, W)) * w


def _views():
    T, H, W = 2, 24, 40
    content, style = _pair(T, H, W)
    frames = content.permute(0, 2, 3, 1).contiguous()
    big = torch.full((3, T, H + 3, W + 5), float("nan"))
    big[:, :, :H, :W] = style.permute(1, 0, 2, 3)
    return frames.permute(0, 3, 1, 2), big.permute(1, 0, 2, 3)[:, :, :H, :W], (T, H, W)


def test_hsv_and_wavelet_adaptive_route_to_the_four_calls(monkeypatch):
    cf = sub("colorfix")
    assert isinstance(cf.HSV_MATCH, bool) and cf.HSV_MATCH_MAX == 2 ** 30
    c_view, s_view, (T, H, W) = _views()
    c, s = _AsCuda.of(c_view), _AsCuda.of(s_view)
    n = T * H * W
    shape, c_st, s_st = (T, 3, H, W), (H * W * 3, 1, W * 3, 3), ((H + 3) * (W + 5), T * (H + 3) * (W + 5), W + 5, 1)
    plane = ((n,), (1,))
    pixels = [(shape, c_st), (shape, s_st)]
    expect = {
        "hsv": [("hsv_planes", pixels), ("hue_match", [plane] * 4), ("hsv_merge", [plane] * 3)],
        "wavelet_adaptive": [("wavelet_reconstruct", pixels), ("hsv_planes", pixels), ("hue_match", [plane] * 4),
                             ("adaptive_blend", [(shape, c_st)] + pixels + [plane] * 3)],       # (the base is a dense [T, H, W, 3] buffer)
    }
    spec = {"hsv": cf.hsv_spec, "wavelet_adaptive": cf.wavelet_adaptive_spec}
    today = {"hsv": [], "wavelet_adaptive": ["wavelet_reconstruct"]}
    monkeypatch.setattr(cf, "HSV_MATCH", True)
    for method in ("hsv", "wavelet_adaptive"):
        rec = _HsvRecorder(cf)
        assert cf.routes_to_device(c, s, method, rec)
        got = cf.correct(c, s, method, ops=rec)
        assert rec.calls == expect[method], (method, rec.calls)
        assert torch.equal(got.as_subclass(torch.Tensor), spec[method](c_view, s_view)), method
        want_old = cf.METHODS[method](c_view, s_view)
        # ops without the four calls; the switch off; a plane one value above the limit: today's calls and bits
        plain = _Recorder(cf)
        got = cf.correct(c, s, method, ops=plain)
        assert [k for k, _ in plain.calls] == today[method] and torch.equal(got.as_subclass(torch.Tensor), want_old)
        assert cf.routes_to_device(c, s, method, plain) == (method != "hsv")
        for attr, value in (("HSV_MATCH", False), ("HSV_MATCH_MAX", n - 1)):
            monkeypatch.setattr(cf, attr, value)
            rec = _HsvRecorder(cf)
            got = cf.correct(c, s, method, ops=rec)
            assert [k for k, _ in rec.calls] == today[method], (method, attr, rec.calls)
            assert torch.equal(got.as_subclass(torch.Tensor), want_old), (method, attr)
            assert cf.routes_to_device(c, s, method, rec) == (method != "hsv")
            monkeypatch.undo()
            monkeypatch.setattr(cf, "HSV_MATCH", True)
        monkeypatch.setattr(cf, "HSV_MATCH_MAX", n)               # exactly at the limit: still the kernels
        rec = _HsvRecorder(cf)
        cf.correct(c, s, method, ops=rec)
        assert [k for k, _ in rec.calls] == [k for k, _ in expect[method]]
        monkeypatch.setattr(cf, "HSV_MATCH_MAX", 2 ** 30)
        # an op set with only some of the four calls does not route
        half =type("Half", (_Recorder,), {"hsv_planes": _HsvRecorder.hsv_planes, "hsv_merge": _HsvRecorder.hsv_merge})(cf)
        got = cf.correct(c, s, method, ops=half)
        assert [k for k, _ in half.calls] == today[method] and torch.equal(got.as_subclass(torch.Tensor), want_old)
        # CPU tensors and impl="torch" never reach the ops
        rec = _HsvRecorder(cf)
        assert torch.equal(cf.correct(c_view, s_view, method, ops=rec), want_old) and rec.calls == []
        assert torch.equal(cf.correct(c, s, method, ops=rec, impl="torch").as_subclass(torch.Tensor), want_old) and rec.calls == []
    # nothing else of the routing moved
    assert cf.DEVICE_METHODS == ("wavelet", "lab", "adain", "wavelet_adaptive")
    assert cf._DEVICE_OPS == ("wavelet_reconstruct", "lab_planes", "lab_merge", "adain")
    for method in ("lab", "wavelet", "adain"):
        rec = _HsvRecorder(cf)
        cf.correct(c, s, method, ops=rec)
        assert not {k for k, _ in rec.calls} & set(cf._HSV_OPS), method


@pytest.mark.parametrize("method,call", [("hsv", "hsv_planes"), ("hsv", "hue_match"), ("hsv", "hsv_merge"),
                                         ("wavelet_adaptive", "wavelet_reconstruct"), ("wavelet_adaptive", "hsv_planes"),
                                         ("wavelet_adaptive", "hue_match"), ("wavelet_adaptive", "adaptive_blend")])
def test_a_failing_hsv_call_raises_and_nothing_falls_back(monkeypatch, method, call):
    cf = sub("colorfix")
    monkeypatch.setattr(cf, "HSV_MATCH", True)
    c_view, s_view, _ = _views()
    rec = _HsvRecorder(cf, fail=call)
    with pytest.raises(RuntimeError, match=call):
        cf.correct(_AsCuda.of(c_view), _AsCuda.of(s_view), method, ops=rec)
    assert rec.calls[-1][0] == call


def test_hipops_offers_the_four_calls_and_torchops_none():
    from ops_reference import TorchOps
    cf, ops = sub("colorfix"), sub("ops")
    for name in cf._HSV_OPS:
        assert callable(getattr(ops.HipOps, name)) and not hasattr(TorchOps, name), name


# ---------------------------------------------------------------------------------------------------------------- C ABI
ENTRY_POINTS = {"svr_hsv_planes": 11, "svr_hue_match_workspace_bytes": 1, "svr_hue_match": 9, "svr_hsv_merge": 10, "svr_adaptive_blend": 18}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_entry_points_are_declared_and_refuse_before_any_launch():
    """Header, ctypes table and build list know the five entry points; the ABI stays 9; each refuses a null pointer, bad sizes, a
    short workspace, misalignment and overlap on the host, naming the argument.  No device is needed: nothing is launched."""
    import ctypes
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    for name, n_args in ENTRY_POINTS.items():
        decl = re.search(rf"(?:int|int64_t) {name}\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == n_args == len(hip_lib.SYMBOLS[name][1]), name
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9 and L.svr_abi_version() == 9
    assert re.search(r"v9, additive: \+ svr_hsv_planes\(\)", src)
    assert '#include "svr_hsv.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert os.path.join(hip_lib.CSRC, "svr_hsv.hip") in hip_lib.sources()

    # ---- the pixel calls: the refusals of the colour-correction family
    T, H, W = 2, 5, 7
    buf = (ctypes.c_char * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)                      # never dereferenced: every call below is refused on the host
    st = lambda *v: (ctypes.c_int64 * 4)(*v)
    dense = st(3 * H * W, H * W, W, 1)
    orders = {
        "svr_hsv_planes": ("content", "content_strides", "style", "style_strides", "c_hsv", "s_hs", "T", "H", "W", "kind", "stream"),
        "svr_hsv_merge": ("h", "sat", "v", "out", "out_strides", "T", "H", "W", "kind", "stream"),
        "svr_adaptive_blend": ("base", "base_strides", "content", "content_strides", "style", "style_strides", "h", "sat", "v",
                               "threshold", "sharpness", "out", "out_strides", "T", "H", "W", "kind", "stream"),
    }
    for name, order in orders.items():
        assert len(order) == ENTRY_POINTS[name]
        good = {k: p for k in order}
        good.update({k: dense for k in order if k.endswith("_strides")})
        good.update(T=T, H=H, W=W, kind=1, stream=None, threshold=0.15, sharpness=5.0)

        def refused(word, **kw):
            a = dict(good)
            a.update(kw)
            assert getattr(L, name)(*[a[k] for k in order]) != 0, (name, kw)
            msg = L.svr_last_error()
            assert name.encode() + b":" in msg and word in msg, (name, kw, msg)

        for k in order:
            if good[k] is p or k.endswith("_strides"):
                refused(k.encode() + b" is a null pointer", **{k: None})
        refused(b"1 <= T", T=0)
        refused(b"1 <= T", T=21846)
        refused(b"H >= 1", H=0)
        refused(b"W >= 1", W=-4)
        refused(b"below 2^24", T=4096, H=4096, W=7)
        for kind in (0, 2, 7):
            refused(b"kind", kind=kind)
        for k in order:
            if k.endswith("_strides"):
                refused(k.encode(), **{k: st(3 * H * W, H * W, -W, 1)})
                if k == "out_strides":
                    refused(k.encode(), **{k: st(3 * H * W, 0, W, 1)})
        if name == "svr_adaptive_blend":
            refused(b"threshold is not a number", threshold=float("nan"))
            refused(b"sharpness is not a number", sharpness=float("nan"))

    # ---- the matching: the refusals of the rank family
    for n in (0, -5, 2 ** 30 + 1, 2 ** 40):
        assert L.svr_hue_match_workspace_bytes(n) <= 0, n
    for n in (1, 2, 4096, 12345, 141_004_800, 2 ** 30):
        need = L.svr_hue_match_workspace_bytes(n)
        n4 = (4 * n + 255) // 256 * 256
        assert need == 5 * n4 + 3072 + L.svr_rank_workspace_bytes(n) and need % 16 == 0 and need < 48 * n + 131072, n
    n = 1000
    need = L.svr_hue_match_workspace_bytes(n)
    at = lambda k: ctypes.c_void_p((1 << 40) + k * (1 << 24))
    order = ("c_h", "c_s", "s_h", "s_s", "n", "out", "workspace", "workspace_bytes", "stream")
    pointers = [k for k in order if k not in ("n", "workspace_bytes", "stream")]
    good = {k: at(i) for i, k in enumerate(pointers)}
    good.update(n=n, workspace_bytes=need, stream=None)

    def refused(word, **kw):
        a = dict(good)
        a.update(kw)
        assert L.svr_hue_match(*[a[k] for k in order]) != 0, kw
        msg = L.svr_last_error()
        assert b"svr_hue_match:" in msg and word in msg, (kw, msg)

    for k in pointers:
        refused(k.encode() + b" is a null pointer", **{k: None})
    refused(b"n must", n=0)
    refused(b"n must", n=-1)
    refused(b"n must", n=2 ** 30 + 1, workspace_bytes=2 ** 40)
    refused(b"workspace_bytes", workspace_bytes=need - 1)
    refused(b"workspace_bytes", workspace_bytes=0)
    refused(b"workspace is not aligned", workspace=ctypes.c_void_p(good["workspace"].value + 8))
    for k in pointers:
        if k != "workspace":
            refused(k.encode() + b" is not aligned", **{k: ctypes.c_void_p(good[k].value + 2)})
            refused(k.encode() + b" overlaps workspace", **{k: ctypes.c_void_p(good["workspace"].value + need - 4)})
            refused(k.encode() + b" overlaps workspace", **{k: ctypes.c_void_p(good["workspace"].value - 4 * n + 4)})
    for k in ("c_h", "s_h", "s_s"):
        refused(b"out overlaps " + k.encode(), out=good[k])
        refused(b"out overlaps " + k.encode(), out=ctypes.c_void_p(good[k].value + 4 * n - 4))
    refused(b"out overlaps c_s", out=ctypes.c_void_p(good["c_s"].value + 4))   # only out == c_s is the in-place form
