"""-m "not gpu": the guarded, poisoned output buffers of tests/guarded_out.py, proven on the CPU (as tests/test_local_error.py
proves the per-element checker): faults are injected into a correct result and the instrument must see them -- and the exact-size
``torch.empty`` buffer the kernel tests used so far must be shown NOT to."""
import math

import pytest
import torch

import guarded_out as go
import local_error as le
from conftest import rel_err
from ops_reference import TorchOps, H16

BF16, F32 = torch.bfloat16, torch.float32
TOL_BF16 = 2.5e-3
ref = TorchOps("cpu", act_dtype=F32)
DTYPES = [BF16, H16, F32, torch.float64, torch.uint8, torch.int32]


def rnd(*shape, scale=1.0, seed=0, dtype=BF16):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def lazy_kernel(out, correct):
    """A "kernel" that computes the right values but skips one 16-byte store (8 bf16 of row 3) and the whole ragged last row."""
    keep = torch.ones(correct.shape, dtype=torch.bool)
    keep[3, 16:24] = False
    keep[-1] = False
    out[keep] = correct[keep]
    return ~keep


def test_stale_correct_data_hides_skipped_stores_and_poison_shows_them():
    M, N, K = 301, 128, 192
    A, W, bias = rnd(M, K), rnd(N, K, scale=1.0 / math.sqrt(K), seed=1), rnd(N, dtype=F32, seed=3)
    correct = ref.gemm(A, W, torch.empty(M, N, dtype=BF16), N=N, K=K, bias=bias)
    want32 = ref.gemm(A, W, torch.empty(M, N), N=N, K=K, bias=bias)
    # the exact-size buffer as the caching allocator hands it out again: the block of the previous run of the same case (another
    # kernel variant, same seeded inputs) -- its correct result
    stale = correct.clone()
    skipped = lazy_kernel(stale, correct)
    assert int(skipped.sum()) == 8 + N
    assert rel_err(stale.float(), want32) < TOL_BF16                     # the global metric passes,
    assert le.check_gemm(stale, A, W, N=N, K=K, bias=bias, name="stale block") <= 1.0    # and so does every per-element bound
    # the same kernel into a guarded, poisoned buffer
    g = go.guarded((M, N), BF16, device="cpu")
    lazy_kernel(g.t, correct)
    g.assert_guards("lazy kernel")                                       # (it wrote nothing outside)
    with pytest.raises(AssertionError) as e:
        g.assert_written("lazy kernel")
    assert f"{8 + N} of {M * N} elements" in str(e.value) and "(3, 16)" in str(e.value), str(e.value)
    with pytest.raises(AssertionError) as e:
        le.check_gemm(g.t, A, W, N=N, K=K, bias=bias, name="poisoned block")
    assert f"{8 + N} of {M * N} elements in 2 rows" in str(e.value) and "inf" in str(e.value), str(e.value)
    assert torch.equal(g.poisoned(), skipped)
    # restricted to a mask that leaves the skipped elements out, the payload counts as written; a complete kernel passes everything
    g.assert_written("lazy kernel, elsewhere", mask=~skipped)
    full = go.guarded((M, N), BF16, device="cpu")
    full.t.copy_(correct)
    full.assert_written("complete kernel")
    full.assert_guards("complete kernel")
    assert le.check_gemm(full.t, A, W, N=N, K=K, bias=bias) <= 1.0
    # a NaN the arithmetic itself produced is not poison: assert_written compares bits
    full.t[0, 0] = float("nan")
    full.assert_written("computed NaN")


@pytest.mark.parametrize("dtype", [BF16, F32, torch.uint8], ids=["bf16", "fp32", "uint8"])
def test_stray_writes_outside_the_payload_fail_the_guards(dtype):
    shape = (7, 33)                                                      # (an odd byte count: the rear guard starts mid-word)
    n = 7 * 33
    esize = torch.empty(0, dtype=dtype).element_size()

    def flat_with_margins(g):
        """the payload and its surroundings as one flat tensor of the payload's dtype, and the payload's first index in it"""
        lo = (g.off // esize) * esize - 64 * esize
        return g.buf[lo:lo + (64 + n + 64) * esize].view(dtype), (g.off - lo) // esize

    g = go.guarded(shape, dtype, device="cpu")
    g.t.fill_(1)
    g.assert_guards("all of the payload")
    flat, p0 = flat_with_margins(g)
    assert flat[p0 + n - 1] == 1
    flat[p0 + n - 1] = 2                                                 # the last payload element: inside
    g.assert_guards("last element")
    flat[p0 + n + 7] = 3                                                 # 8 elements past the end
    with pytest.raises(AssertionError) as e:
        g.assert_guards("past the end")
    assert f"the first at byte {(n + 7) * esize} " in str(e.value) and "0 in front" in str(e.value), str(e.value)

    g = go.guarded(shape, dtype, device="cpu")
    g.t.fill_(1)
    flat, p0 = flat_with_margins(g)
    flat[p0 - 8] = 3                                                     # 8 elements before the start
    with pytest.raises(AssertionError) as e:
        g.assert_guards("before the start")
    assert f"the first at byte {-8 * esize} " in str(e.value) and "0 behind" in str(e.value), str(e.value)
    # a value equal to the guard byte pattern cannot be told from the guard: the stray store of a real kernel is a computed value
    pool = go.Pool("cpu")
    out = pool(*shape, dtype=dtype)
    out.fill_(1)
    flat, p0 = flat_with_margins(pool.live[0])
    flat[p0 + n] = 3
    with pytest.raises(AssertionError):
        pool.check("pool")
    assert pool.live == []


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
@pytest.mark.parametrize("shape", [(1,), (3, 5, 7), (257, 12), (2, 3, 4, 8)])
def test_payload_alignment_and_layout(dtype, shape):
    """The payload sits where a fresh allocation would as far as the route predicates can tell: 256-byte aligned (they test 16),
    contiguous, of the requested shape and dtype, with GUARD_BYTES untouched guard bytes directly in front of and behind it."""
    held = [go.guarded(shape, dtype, device="cpu") for _ in range(3)]   # (several live blocks: different base addresses)
    for g in held:
        assert g.t.shape == shape and g.t.dtype == dtype and g.t.is_contiguous()
        assert g.t.data_ptr() % 256 == 0
        assert g.t.data_ptr() == g.buf.data_ptr() + g.off and g.off >= go.GUARD_BYTES
        assert g.nbytes == g.t.numel() * g.t.element_size()
        front, rear = g._guards()
        assert front.numel() == rear.numel() == go.GUARD_BYTES == 4096
        assert rear.data_ptr() == g.t.data_ptr() + g.nbytes and front.data_ptr() + 4096 == g.t.data_ptr()
        assert bool((front == 0xA5).all()) and bool((rear == 0xA5).all())
        g.assert_guards()


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_poison_patterns_round_trip(dtype):
    g = go.guarded((5, 9), dtype, device="cpu")
    assert bool(g.poisoned().all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(g.t).all())                              # NaN in every floating-point format ...
        assert bool(torch.isnan(le.values(g.t)).all())                   # ... also as local_error reads the stored values
        canonical = torch.full((1,), float("nan"), dtype=dtype)
        assert not bool((go._bits(g.t) == go._bits(canonical)).any())    # ... and none of them the NaN arithmetic produces
        # copies, clones and device transfers keep the bits (the pattern is a quiet NaN: nothing has to quieten it)
        assert torch.equal(go._bits(g.t.clone()), go._bits(g.t))
    else:
        assert bool((g.t.view(torch.uint8) == 0xA5).all())
    with pytest.raises(AssertionError) as e:
        g.assert_written("untouched")
    assert "45 of 45" in str(e.value)
    g.t[2, 3] = 1
    assert int(g.poisoned().sum()) == 44 and not bool(g.poisoned()[2, 3])
    # init=: the payload is that tensor's bits, no poison anywhere, guards intact
    src = (torch.arange(45).reshape(5, 9) % 7).to(dtype)
    h = go.guarded((5, 9), dtype, device="cpu", init=src)
    assert torch.equal(go._bits(h.t), go._bits(src)) and not bool(h.poisoned().any())
    h.assert_written("init")
    h.assert_guards("init")
    with pytest.raises(ValueError):
        go.guarded((5, 9), dtype, device="cpu", init=src.reshape(9, 5))
