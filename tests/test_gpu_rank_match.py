"""-m gpu: the radix sort and the rank matching of csrc/svr_rank.hip against their specification on the CPU (colorfix.sort_key,
colorfix.rank_match_spec; torch.sort(stable=True)), bit for bit.

Sizes come from svr_rank_geometry (tile K, scan width S): every n in 1..130 (the wave-64 boundaries and the ragged tail), K - 1, K,
K + 1, 3 K + 17, the boundary of a workgroup's 16 tiles (16 K - 1, 16 K + 1) and, S being 0 (one launch of the table scan covers any
number of tiles), the issue's 2^22 + 17: 1025 tiles, which rank_scan_kernel still walks in ONE step of 2048 table entries.  The
scan's carry from step to step -- what every 4K span runs, 17 steps -- is reached by two larger sizes on three families
(ACROSS_THE_SCAN_STEP): 2048 K + 17 (2049 tiles, a second step of one 16-tile piece) and (2048 + 16) K + 1 (2065 tiles, two
pieces), about 8.4 M keys each.  Every output and the workspace lie in guarded canvases, the outputs poisoned: a store outside
[0, n) or a missed element is seen.  The CPU sorts are computed once per (family, size), shared, and let go with the module."""
import ctypes
import functools

import pytest
import torch

import rank_emulation as emu
from conftest import sub
from guarded_out import Pool
from test_gpu_colorfix import _close_share, _cpu, _pair

pytestmark = pytest.mark.gpu

FAMILIES = ("normals", "all_equal", "three_values", "sorted", "reversed", "top_byte", "low_byte", "quantised", "specials")
SCAN_FAMILIES = ("normals", "quantised", "specials")


@pytest.fixture(scope="module")
def hip():
    yield sub("ops").HipOps("cuda:0")
    _cpu_sort.cache_clear()                                       # (hundreds of MB of shared CPU sorts)
    _keys.cache_clear()


def _across_the_scan_step():
    """sizes whose table has more entries per row than one step of rank_scan_kernel takes (tests/test_rank_match.py holds
    rank_emulation's constants to the kernel's)"""
    K, _ = _geometry()
    assert K == emu.TILE
    sizes = (emu.SCAN_STEP * K + 17, (emu.SCAN_STEP + emu.GROUP) * K + 1)
    assert all(emu.geometry(n)[2] > emu.SCAN_STEP for n in sizes)
    return sizes


@functools.lru_cache(maxsize=None)
def _geometry():
    L = sub("hip_lib").lib()
    geo = (ctypes.c_int32 * 2)()
    assert L.svr_rank_geometry(geo) == 0
    return int(geo[0]), int(geo[1])


@functools.lru_cache(maxsize=None)
def _sizes():
    K, S = _geometry()
    sizes = list(range(1, 131)) + [K - 1, K, K + 1, 3 * K + 17, 16 * K - 1, 16 * K + 1]
    if S > 0 and (S + 1) * K + 17 <= 2 ** 25:
        sizes.append((S + 1) * K + 17)
    elif S > 0:
        sizes += [min(S * K, 2 ** 25), min(S * K + 1, 2 ** 25)]
    else:
        sizes.append(2 ** 22 + 17)
    return tuple(sorted(set(sizes)))


def _from_bits(bits):
    return bits.to(torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=None)
def _keys(family, n):
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + n % 997)
    if family == "normals":
        return torch.randn(n, generator=g) * 30
    if family == "all_equal":
        return torch.full((n,), -7.25)
    if family == "three_values":
        return torch.tensor([-0.0, 0.0, 1.5])[torch.randint(0, 3, (n,), generator=g)]
    if family == "sorted":
        return torch.sort(torch.randn(n, generator=g)).values
    if family == "reversed":
        return torch.sort(torch.randn(n, generator=g), descending=True).values
    if family == "top_byte":                                      # the three low digits constant: only the last pass moves a key
        tops = torch.tensor([b for b in range(256) if b not in (0x7F, 0xFF)])                         # (those two would be NaNs)
        bits = tops[torch.randint(0, tops.numel(), (n,), generator=g)] * 2 ** 24 + 0x123456
        return _from_bits(torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits))
    if family == "low_byte":                                      # the three high digits constant: only the first pass moves a key
        return _from_bits(torch.randint(0, 256, (n,), generator=g) + 0x3F800000)
    if family == "quantised":                                     # the tie structure of real frames
        return (torch.rand(n, generator=g) * 255).round() / 255
    sp = torch.tensor([float("inf"), float("-inf"), 1e-45, -1e-45, 1e-39, -1e-39, 0.0, -0.0, 1.0, -2.0, float("nan")])
    x = sp[torch.randint(0, sp.numel(), (n,), generator=g)]
    neg_nan = torch.rand(n, generator=g) < 0.05                   # NaNs of the other sign and with payload bits
    return torch.where(neg_nan, _from_bits(torch.full((n,), -12345)), x)


@functools.lru_cache(maxsize=None)
def _cpu_sort(family, n):
    """(keys, indices of torch.sort(stable=True) on the CPU, its values): computed once, never modified"""
    x = _keys(family, n)
    s = torch.sort(x, stable=True)
    return x, s.indices, s.values


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch_sort(hip, x_dev, n, with_index, name):
    out_pool, ws_pool = Pool(), Pool()
    sorted_ = out_pool(n, dtype=torch.float32)
    index = out_pool(n, dtype=torch.int32) if with_index else None
    need = int(hip.lib.svr_rank_workspace_bytes(n))
    ws = ws_pool(need, dtype=torch.uint8)
    rc = hip.lib.svr_sort_f32(x_dev.data_ptr(), n, sorted_.data_ptr(), index.data_ptr() if with_index else None, ws.data_ptr(), need,
                              hip._stream())
    assert rc == 0, hip.lib.svr_last_error()
    torch.cuda.synchronize()
    out_pool.check(name)
    ws_pool.check(name + " workspace", written=False)
    return sorted_.cpu(), (index.cpu() if with_index else None)


@pytest.mark.parametrize("family", FAMILIES)
def test_sort_f32_equals_the_stable_cpu_sort(hip, family):
    _sort_cases(hip, family, _sizes())


@pytest.mark.parametrize("n", [0, 1], ids=["one_piece_past_the_step", "two_pieces_past_the_step"])
@pytest.mark.parametrize("family", SCAN_FAMILIES)
def test_sort_f32_where_the_table_scan_carries_from_step_to_step(hip, family, n):
    _sort_cases(hip, family, (_across_the_scan_step()[n],))


def _sort_cases(hip, family, sizes):
    for n in sizes:
        x, want_idx, want_val = _cpu_sort(family, n)
        x_dev = x.cuda()
        n_nan = int(torch.isnan(want_val).sum())
        for with_index in (True, False):
            name = f"sort_f32 {family} n={n} index={with_index}"
            got_val, got_idx = _launch_sort(hip, x_dev, n, with_index, name)
            if with_index:
                assert torch.equal(got_idx.to(torch.int64), want_idx), (name, int((got_idx != want_idx).sum()))
                if family == "all_equal":
                    assert torch.equal(got_idx, torch.arange(n, dtype=torch.int32)), name
            assert bool((got_val[:n - n_nan] == want_val[:n - n_nan]).all()), name
            assert int(torch.isnan(got_val).sum()) == n_nan and bool(torch.isnan(got_val[n - n_nan:]).all()), name
        assert torch.equal(_bits(x_dev.cpu()), _bits(x)), f"{family} n={n}: the keys were modified"


def test_sort_f32_through_the_ops(hip):
    cf = sub("colorfix")
    K, _ = _geometry()
    n = 3 * K + 17
    for family in ("quantised", "specials"):
        x, want_idx, _ = _cpu_sort(family, n)
        val, idx = hip.sort_f32(x.cuda())
        assert idx.dtype == torch.int32 and torch.equal(idx.cpu().to(torch.int64), want_idx)
        want = cf.key_value(torch.sort(cf.sort_key(x)).values)                # canonical: +0.0 for -0.0, one NaN pattern
        assert torch.equal(_bits(val.cpu()), _bits(want))
        val2, none = hip.sort_f32(x.cuda().reshape(1, -1), index=False)
        assert none is None and torch.equal(_bits(val2.cpu()), _bits(want))
    # keys only: the workspace and the sorted values are all that is allocated (no index of another 4 n bytes)
    x_dev = x.cuda()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    val2, none = hip.sort_f32(x_dev, index=False)
    torch.cuda.synchronize()
    above = torch.cuda.max_memory_allocated() - base
    assert none is None and above < int(hip.lib.svr_rank_workspace_bytes(n)) + 6 * n, (above, n)
    # the measurement setting under which svr_sort_f32 stores nothing is refused by both methods, and leaves no trace once reset
    hip.set_option("rank_launches", 2)
    try:
        with pytest.raises(sub("hip_lib").HipLibraryError, match="rank_launches"):
            hip.sort_f32(x_dev)
        with pytest.raises(sub("hip_lib").HipLibraryError, match="rank_launches"):
            hip.rank_match(x_dev, x_dev.clone())
    finally:
        hip.set_option("rank_launches", 3)
    assert torch.equal(_bits(hip.sort_f32(x_dev, index=False)[0].cpu()), _bits(want))
    with pytest.raises(ValueError, match="sort_f32"):
        hip.sort_f32(torch.empty(0, device="cuda"))
    with pytest.raises(ValueError, match="keys"):
        hip.sort_f32(torch.zeros(8, device="cuda", dtype=torch.float64))


def _spec(cf, family, ref_family, n):
    """colorfix.rank_match_spec from the shared CPU sorts: out[order] = the reference's sorted canonical values"""
    _, order, _ = _cpu_sort(family, n)
    _, _, ref_sorted = _cpu_sort(ref_family, n)
    want = torch.empty(n)
    want[order] = cf.key_value(cf.sort_key(ref_sorted))
    return want


@pytest.mark.parametrize("family", FAMILIES)
def test_rank_match_equals_the_specification(hip, family):
    _rank_match_cases(hip, family, FAMILIES[(FAMILIES.index(family) + 4) % len(FAMILIES)], _sizes())


@pytest.mark.parametrize("n", [0, 1], ids=["one_piece_past_the_step", "two_pieces_past_the_step"])
@pytest.mark.parametrize("family", SCAN_FAMILIES)
def test_rank_match_where_the_table_scan_carries_from_step_to_step(hip, family, n):
    ref_family = SCAN_FAMILIES[(SCAN_FAMILIES.index(family) + 1) % len(SCAN_FAMILIES)]      # (its CPU sort is shared with the sort test)
    _rank_match_cases(hip, family, ref_family, (_across_the_scan_step()[n],))


def _rank_match_cases(hip, family, ref_family, sizes):
    cf = sub("colorfix")
    K, _ = _geometry()
    for n in sizes:
        src, ref = _keys(family, n), _keys(ref_family, n)
        want = _spec(cf, family, ref_family, n)
        if n in (1, 7, 130, K + 1):                               # the shared sorts restate the specification: checked against it
            assert torch.equal(_bits(want), _bits(cf.rank_match_spec(src, ref)))
        src_dev, ref_dev = src.cuda(), ref.cuda()
        out_pool, ws_pool = Pool(), Pool()
        out = out_pool(n, dtype=torch.float32)
        need = int(hip.lib.svr_rank_workspace_bytes(n))
        ws = ws_pool(need, dtype=torch.uint8)
        rc = hip.lib.svr_rank_match(src_dev.data_ptr(), ref_dev.data_ptr(), n, out.data_ptr(), ws.data_ptr(), need, hip._stream())
        assert rc == 0, hip.lib.svr_last_error()
        torch.cuda.synchronize()
        name = f"rank_match {family} <- {ref_family} n={n}"
        out_pool.check(name)
        ws_pool.check(name + " workspace", written=False)
        assert torch.equal(_bits(out.cpu()), _bits(want)), (name, int((_bits(out.cpu()) != _bits(want)).sum()))
        assert torch.equal(_bits(src_dev.cpu()), _bits(src)) and torch.equal(_bits(ref_dev.cpu()), _bits(ref)), name + ": inputs modified"
        if n in (1, 65, 3 * K + 17):                              # through the ops, and matched in place
            got = hip.rank_match(src_dev.reshape(1, n), ref_dev)
            assert got.shape == (1, n) and torch.equal(_bits(got.cpu().flatten()), _bits(want)), name
            same = hip.rank_match(src_dev, ref_dev, out=src_dev)
            assert same.data_ptr() == src_dev.data_ptr() and torch.equal(_bits(src_dev.cpu()), _bits(want)), name + " in place"
            assert torch.equal(_bits(ref_dev.cpu()), _bits(ref))


def test_rank_match_refuses_what_it_does_not_serve(hip):
    a, b = torch.rand(100, device="cuda"), torch.rand(101, device="cuda")
    with pytest.raises(ValueError, match="same number"):
        hip.rank_match(a, b)
    with pytest.raises(sub("hip_lib").HipLibraryError, match="out overlaps reference"):
        hip.rank_match(a, b[:100], out=b[:100])
    with pytest.raises(ValueError, match="contiguous"):
        hip.rank_match(b[::2], b[:51])


# ---------------------------------------------------------------------------------------------------------------- lab
class _Spy:
    """HipOps with every method call noted by name"""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        attr = getattr(self._ops, name)
        if not callable(attr):
            return attr

        def call(*a, **kw):
            self.calls.append(name)
            return attr(*a, **kw)
        return call


def _lab_pairs():
    content, style = _pair(3, 96, 160)
    q = lambda x: (x * 127.5).round() / 127.5                    # 8 bits over [-1, 1]: ties abound
    return {"continuous": (content, style), "quantised": (q(content), q(style))}


@pytest.mark.parametrize("which", ["continuous", "quantised"])
def test_lab_is_defined_by_bits(hip, which, monkeypatch):
    cf = sub("colorfix")
    content, style = _lab_pairs()[which]
    c, s = content.cuda(), style.cuda()
    T, _, H, W = c.shape
    c_lab, s_lab = hip.lab_planes(hip.wavelet_reconstruct(c, s), s)
    c_cpu, s_cpu = c_lab.cpu(), s_lab.cpu()
    m = [cf.rank_match_spec(c_cpu[i], s_cpu[i]).cuda() for i in range(3)]
    want = hip.lab_merge(c_lab[0], m[0], m[1], m[2], 0.8, (T, H, W)).cpu()
    monkeypatch.setattr(cf, "RANK_MATCH", True)
    spy = _Spy(hip)
    got = cf.correct(c, s, "lab", ops=spy)
    assert spy.calls == ["wavelet_reconstruct", "lab_planes", "rank_match", "rank_match", "rank_match", "lab_merge"]
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    if which == "quantised":                                      # determinism where ties abound
        assert torch.equal(cf.correct(c, s, "lab", ops=hip).cpu(), got.cpu())
    # the flag off: today's calls (torch's sorts between the kernels) and today's result, held to test_gpu_colorfix's bounds
    monkeypatch.setattr(cf, "RANK_MATCH", False)
    sorts = []
    real = cf.histogram_match
    monkeypatch.setattr(cf, "histogram_match", lambda a, b: (sorts.append(1), real(a, b))[1])
    spy = _Spy(hip)
    old = cf.correct(c, s, "lab", ops=spy)
    assert spy.calls == ["wavelet_reconstruct", "lab_planes", "lab_merge"] and len(sorts) == 3
    if which == "continuous":
        share, worst = _close_share(old, _cpu("lab", 3, 96, 160))
        assert share < 5e-3 and worst < 5e-3, (share, worst)
        share, worst = _close_share(got, _cpu("lab", 3, 96, 160))
        print(f"lab with rank_match vs the CPU run: share off by more than 2e-5: {share:.3e}, max {worst:.3e}")
        assert share < 5e-3 and worst < 5e-3, (share, worst)
