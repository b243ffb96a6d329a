"""-m "not gpu": rank matching (colorfix.sort_key / rank_match_spec, csrc/svr_rank.hip) without a device.

  sort_key           a stable argsort of the key = the indices of torch.sort(stable=True) on the CPU, bit for bit
  rank_match_spec    a permutation of the canonical reference, monotone, ties in index order, = histogram_match where nothing ties
  rank_emulation     the launches as built (tile, digits, table, scan steps, in-tile ranks) restated in numpy = the stable argsort
  host               the four entry points: header, ctypes table, workspace sizes, refusals before any launch
  route              colorfix._lab_on_device hands the planes to ops.rank_match only where the ops have it and RANK_MATCH is set"""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import rank_emulation as emu
from conftest import ROOT, sub
from test_colorfix_device import _AsCuda, _Recorder

NAN_NEG = torch.tensor([-1], dtype=torch.int32).view(torch.float32)[0].item()           # 0xFFFFFFFF: a NaN with the sign bit set
SPECIALS = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, float("inf"), float("-inf"), float("nan"), NAN_NEG, 1.0, -1.0, 1.17549435e-38]


def _vectors():
    g = torch.Generator().manual_seed(5)
    normals = torch.randn(100_000, generator=g)
    normals[torch.randint(0, 100_000, (20_000,), generator=g)] = normals[:20_000].clone()      # planted ties
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    return {
        "specials": sp[torch.randint(0, len(SPECIALS), (4000,), generator=g)],
        "all_equal": torch.full((777,), 0.25),
        "three_values": torch.tensor([-0.0, 0.0, 2.5])[torch.randint(0, 3, (5000,), generator=g)],
        "normals_with_ties": normals,
        "one": torch.tensor([3.0]),
    }


VECTORS = _vectors()


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_sort_key_orders_as_the_stable_cpu_sort(name):
    cf = sub("colorfix")
    x = VECTORS[name]
    want = torch.sort(x, stable=True)
    key = cf.sort_key(x)
    assert key.dtype == torch.int64 and int(key.min()) >= 0 and int(key.max()) < 2 ** 32
    got = torch.sort(key, stable=True)
    assert torch.equal(got.indices, want.indices)
    vals = cf.key_value(got.values)
    n_nan = int(torch.isnan(want.values).sum())
    assert int(torch.isnan(vals).sum()) == n_nan and (n_nan == 0 or bool(torch.isnan(vals[-n_nan:]).all()))   # NaN exactly at the tail
    m = x.numel() - n_nan
    assert bool((vals[:m] == want.values[:m]).all())
    # canonical: no -0.0 and one NaN pattern among the values a key stands for
    bits = vals.view(torch.int32)
    assert not bool((bits == -2 ** 31).any()) and bool((bits[torch.isnan(vals)] == 0x7FC00000).all())


def test_sort_key_words():
    cf = sub("colorfix")
    x = torch.tensor([0.0, -0.0, float("nan"), NAN_NEG, 1.0, -1.0, float("inf"), float("-inf")])
    assert cf.sort_key(x).tolist() == [0x80000000, 0x80000000, 0xFFC00000, 0xFFC00000, 0xBF800000, 0x407FFFFF, 0xFF800000, 0x007FFFFF]


def _canonical_sorted(cf, ref):
    return cf.key_value(torch.sort(cf.sort_key(ref.flatten())).values)


@pytest.mark.parametrize("name", ["specials", "three_values", "normals_with_ties", "all_equal"])
def test_rank_match_spec_properties(name):
    cf = sub("colorfix")
    src = VECTORS[name]
    g = torch.Generator().manual_seed(9)
    ref = VECTORS[name][torch.randperm(src.numel(), generator=g)] if name != "all_equal" else torch.randn(src.numel(), generator=g).round(decimals=1)
    out = cf.rank_match_spec(src.reshape(1, -1), ref)
    assert out.shape == (1, src.numel())
    out = out.flatten()
    ref_sorted = _canonical_sorted(cf, ref)
    # a permutation of the canonical reference multiset (compared as bits: NaN included)
    assert torch.equal(torch.sort(cf.sort_key(out)).values, cf.sort_key(ref_sorted))
    assert torch.equal(out.view(torch.int32).sort().values, ref_sorted.view(torch.int32).sort().values)
    # monotone in the key order, and tied sources receive consecutive sorted reference values in index order
    order = torch.sort(cf.sort_key(src), stable=True).indices
    assert torch.equal(out[order].view(torch.int32), ref_sorted.view(torch.int32))
    ks, ko = cf.sort_key(src)[order], cf.sort_key(out)[order]
    assert bool((ko[1:] >= ko[:-1]).all())
    same = ks[1:] == ks[:-1]
    assert bool((order[1:][same] > order[:-1][same]).all())
    finite = ~(torch.isnan(src) | torch.isnan(out))
    s, o = src[finite][:600], out[finite][:600]
    assert not bool(((s[:, None] < s[None, :]) & (o[:, None] > o[None, :])).any())       # source_i < source_j => out_i <= out_j


def test_rank_match_spec_equals_histogram_match_without_ties():
    cf = sub("colorfix")
    g = torch.Generator().manual_seed(3)
    def distinct(shape, scale, shift):
        """torch.rand's values (24 bits: a few of 1e4 draws collide) with the duplicates taken out, in random order"""
        n = int(np.prod(shape))
        pool = (torch.rand(2 * n + 8, generator=g) * scale + shift).unique()
        return pool[torch.randperm(pool.numel(), generator=g)[:n]].reshape(shape)

    for shape in ((1,), (3, 41, 67), (50_000,)):
        src, ref = distinct(shape, 1.0, 0.0), distinct(shape, 3.0, -1.0)
        assert src.unique().numel() == src.numel() and ref.unique().numel() == ref.numel()
        assert torch.equal(cf.rank_match_spec(src, ref), cf.histogram_match(src, ref))
    with pytest.raises(ValueError, match="one size"):
        cf.rank_match_spec(torch.rand(5), torch.rand(6))


# ---------------------------------------------------------------------------------------------------------------- emulation
@pytest.mark.parametrize("n", [1, emu.TILE - 1, emu.TILE, emu.TILE + 1, 3 * emu.TILE + 17])
def test_the_launches_as_built_give_the_stable_argsort(n):
    cf = sub("colorfix")
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 4).round(decimals=1)                              # heavy ties
    x[torch.randint(0, n, (max(1, n // 50),), generator=g)] = float("nan")
    x[torch.randint(0, n, (max(1, n // 50),), generator=g)] = -0.0
    key = cf.sort_key(x)
    want = torch.sort(key, stable=True)
    k, i = emu.sort(key.numpy().astype(np.uint32))
    assert np.array_equal(i.astype(np.int64), want.indices.numpy()) and np.array_equal(k.astype(np.int64), want.values.numpy())
    assert torch.equal(torch.from_numpy(i.astype(np.int64)), torch.sort(x, stable=True).indices)


def test_emulation_constants_are_the_kernels():
    """the geometry rank_emulation restates, and tests/test_gpu_rank_match.py sizes its cases by, is the one in csrc/svr_rank.hip"""
    src = open(os.path.join(ROOT, "comfyui-seedvr2_videoupscaler_amd", "csrc", "svr_rank.hip")).read()
    for line in ("constexpr int RANK_BITS = 8;", "constexpr int RANK_THREADS = 256;", "constexpr int RANK_KPT = 16;",
                 "constexpr int RANK_TILE = RANK_THREADS * RANK_KPT;", "constexpr int RANK_GROUP = 16;",
                 "constexpr int RANK_SCAN_STEP = RANK_THREADS * 8;"):
        assert line in src, line
    assert (emu.BITS, emu.THREADS, emu.KPT, emu.TILE, emu.GROUP, emu.SCAN_STEP) == (8, 256, 16, 256 * 16, 16, 256 * 8)


def test_emulation_scan_crosses_its_step():
    """A self-check of the HELPER only (numpy against numpy, no product code): rank_emulation.scan's carry between steps.  The
    kernel's own carry is exercised on the device, by the sizes above 2048 tiles of tests/test_gpu_rank_match.py."""
    tiles_p = emu.SCAN_STEP + emu.GROUP
    g = np.random.default_rng(0)
    table = g.integers(0, emu.TILE, size=(emu.RADIX, tiles_p)).astype(np.uint32)
    scanned, totals = emu.scan(table)
    wide = table.astype(np.int64)
    assert np.array_equal(scanned.astype(np.int64), np.cumsum(wide, axis=1) - wide) and np.array_equal(totals.astype(np.int64), wide.sum(axis=1))


# ---------------------------------------------------------------------------------------------------------------- C ABI
ENTRY_POINTS = {"svr_rank_workspace_bytes": 1, "svr_rank_geometry": 1, "svr_sort_f32": 7, "svr_rank_match": 7}
WORKSPACE_CONSTANT = 65536           # include/seedvr2_hip.h: svr_rank_workspace_bytes(n) < 24 n + 65536


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_entry_points_are_declared_and_refuse_before_any_launch():
    import ctypes
    hip_lib = sub("hip_lib")
    hip_lib.build()
    L = hip_lib.lib()
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    for name, n_args in ENTRY_POINTS.items():
        decl = re.search(rf"(?:int|int64_t) {name}\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == n_args == len(hip_lib.SYMBOLS[name][1]), name
    assert "#define SVR_ABI_VERSION 9" in src and hip_lib.ABI_VERSION == 9 and L.svr_abi_version() == 9
    assert re.search(r"v9, additive: \+ svr_sort_f32\(\)", src) and "24 n + 65536" in src
    assert '#include "svr_rank.hip"' in open(os.path.join(hip_lib.CSRC, "svr_api.hip")).read()
    assert os.path.join(hip_lib.CSRC, "svr_rank.hip") in hip_lib.sources()

    geo = (ctypes.c_int32 * 2)(-1, -1)
    assert L.svr_rank_geometry(geo) == 0 and (geo[0], geo[1]) == (emu.TILE, 0)
    assert L.svr_rank_geometry(None) != 0 and b"out2" in L.svr_last_error()
    for n in (0, -5, 2 ** 30 + 1, 2 ** 40):
        assert L.svr_rank_workspace_bytes(n) <= 0, n
    for n in (1, 2, emu.TILE, 12345, 141_004_800, 2 ** 30):
        need = L.svr_rank_workspace_bytes(n)
        tiles_p = emu.geometry(n)[2]
        assert 0 < need <= 24 * n + WORKSPACE_CONSTANT, n
        assert need >= 20 * n + 4 * emu.RADIX * tiles_p + 4 * emu.RADIX, n           # five n-element arrays, the table, the totals

    n = 1000
    need = L.svr_rank_workspace_bytes(n)
    base = 1 << 40                                                 # never dereferenced: every call below is refused on the host
    at = lambda k: ctypes.c_void_p(base + k * (1 << 24))
    orders = {
        "svr_sort_f32": ("keys", "n", "sorted", "index", "workspace", "workspace_bytes", "stream"),
        "svr_rank_match": ("source", "reference", "n", "out", "workspace", "workspace_bytes", "stream"),
    }
    for name, order in orders.items():
        pointers = [k for k in order if k not in ("n", "workspace_bytes", "stream")]
        good = {k: at(i) for i, k in enumerate(pointers)}
        good.update(n=n, workspace_bytes=need, stream=None)

        def refused(word, **kw):
            a = dict(good)
            a.update(kw)
            assert getattr(L, name)(*[a[k] for k in order]) != 0, (name, kw)
            msg = L.svr_last_error()
            assert name.encode() + b":" in msg and word in msg, (name, kw, msg)

        for k in pointers:
            if k != "index":                                      # (a null index asks for keys only)
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
    a = dict(source=at(0), reference=at(1), n=n, out=at(3), workspace=at(4), workspace_bytes=need, stream=None)
    order = orders["svr_rank_match"]

    def refused_match(word, **kw):
        b = dict(a)
        b.update(kw)
        assert L.svr_rank_match(*[b[k] for k in order]) != 0 and word in L.svr_last_error(), (kw, L.svr_last_error())

    refused_match(b"out overlaps reference", out=at(1))
    refused_match(b"out overlaps reference", out=ctypes.c_void_p(at(1).value + 4 * n - 4))
    refused_match(b"out overlaps source", out=ctypes.c_void_p(at(0).value + 4))      # only out == source is the in-place form
    refused_match(b"source overlaps reference", reference=at(0))
    s = dict(keys=at(0), n=n, sorted=at(1), index=at(2), workspace=at(4), workspace_bytes=need, stream=None)
    for word, kw in ((b"sorted overlaps keys", dict(sorted=at(0))), (b"index overlaps keys", dict(index=at(0))),
                     (b"index overlaps sorted", dict(index=ctypes.c_void_p(at(1).value + 4 * n - 4)))):
        b = dict(s)
        b.update(kw)
        assert L.svr_sort_f32(*[b[k] for k in orders["svr_sort_f32"]]) != 0 and word in L.svr_last_error(), (kw, L.svr_last_error())


# ---------------------------------------------------------------------------------------------------------------- route
class _RankRecorder(_Recorder):
    """the recorder of test_colorfix_device with a rank_match that answers with the specification"""

    def rank_match(self, source, reference, out=None):
        self._note("rank_match", source, reference)
        res = self.cf.rank_match_spec(self._plain(source), self._plain(reference))
        if out is not None:
            assert out.data_ptr() == source.data_ptr()
            out.copy_(res)
            return out
        return res


def _quantised_pair():
    g = torch.Generator().manual_seed(21)
    q = lambda x: (x * 127.5).round() / 127.5
    return q((torch.rand(2, 3, 24, 40, generator=g) * 2 - 1) * 0.9), q((torch.rand(2, 3, 24, 40, generator=g) * 2 - 1) * 0.6 + 0.1)


def test_lab_route_uses_rank_match_only_where_the_ops_have_it_and_the_flag_is_set(monkeypatch):
    cf = sub("colorfix")
    assert isinstance(cf.RANK_MATCH, bool)
    content, style = _quantised_pair()
    c, s = _AsCuda.of(content), _AsCuda.of(style)
    old = ["wavelet_reconstruct", "lab_planes", "lab_merge"]
    want_old = cf.METHODS["lab"](content, style)

    def planes_matched():
        to01 = lambda x: ((x + 1.0) * 0.5).clamp(0.0, 1.0)
        pl = lambda x: cf.rgb_to_lab(to01(x)).permute(1, 0, 2, 3).reshape(3, -1).contiguous()
        c_lab, s_lab = pl(cf.wavelet_reconstruction(content, style)), pl(style)
        m = [cf.rank_match_spec(c_lab[i], s_lab[i]) for i in range(3)]
        lab = torch.stack([(c_lab[0] * 0.8 + m[0] * (1.0 - 0.8)).reshape(2, 24, 40), m[1].reshape(2, 24, 40), m[2].reshape(2, 24, 40)], dim=1)
        return cf.lab_to_rgb(lab) * 2.0 - 1.0

    monkeypatch.setattr(cf, "RANK_MATCH", True)
    rec = _RankRecorder(cf)
    got = cf.correct(c, s, "lab", ops=rec)
    assert [n for n, _ in rec.calls] == ["wavelet_reconstruct", "lab_planes", "rank_match", "rank_match", "rank_match", "lab_merge"]
    assert torch.equal(got.as_subclass(torch.Tensor), planes_matched())
    plain = _Recorder(cf)                                          # ops without rank_match: today's call list and result
    got = cf.correct(c, s, "lab", ops=plain)
    assert [n for n, _ in plain.calls] == old and torch.equal(got.as_subclass(torch.Tensor), want_old)
    monkeypatch.setattr(cf, "RANK_MATCH", False)
    rec = _RankRecorder(cf)
    got = cf.correct(c, s, "lab", ops=rec)
    assert [n for n, _ in rec.calls] == old and torch.equal(got.as_subclass(torch.Tensor), want_old)
    # a plane above svr_rank_match's limit keeps the route that has none: today's calls and result, nothing raises
    monkeypatch.setattr(cf, "RANK_MATCH", True)
    assert cf.RANK_MATCH_MAX == 2 ** 30                            # (svr_rank_workspace_bytes refuses 2^30 + 1: the test above)
    n = content.shape[0] * content.shape[2] * content.shape[3]
    for limit, wants_rank in ((n, True), (n - 1, False)):
        monkeypatch.setattr(cf, "RANK_MATCH_MAX", limit)
        rec = _RankRecorder(cf)
        got = cf.correct(c, s, "lab", ops=rec)
        assert ("rank_match" in [name for name, _ in rec.calls]) == wants_rank, limit
        if not wants_rank:
            assert [name for name, _ in rec.calls] == old and torch.equal(got.as_subclass(torch.Tensor), want_old)
    monkeypatch.setattr(cf, "RANK_MATCH_MAX", 2 ** 30)
    # nothing else of the routing moved
    assert cf.DEVICE_METHODS == ("wavelet", "lab", "adain", "wavelet_adaptive")
    assert cf._DEVICE_OPS == ("wavelet_reconstruct", "lab_planes", "lab_merge", "adain")
    for method in ("wavelet_adaptive", "hsv", "wavelet", "adain"):
        rec = _RankRecorder(cf)
        cf.correct(c, s, method, ops=rec)
        assert "rank_match" not in [n for n, _ in rec.calls], method
