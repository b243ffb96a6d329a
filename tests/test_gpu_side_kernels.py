"""-m gpu: the side kernels (csrc/svr_elementwise.hip, launchers in csrc/svr_api.hip) and the first-generation window attention at
sizes chosen FROM THEIR LAUNCHERS, so that the control flow the small kernel tests never enter runs: the second in-flight row slot
and the refill of rmsnorm_mod_kernel, the grid-stride loop and the ragged head walk of qknorm_rope_kernel, several / more than 256 /
ragged row blocks in the GroupNorm statistics, the capped grid and the per-chunk channel path of groupnorm_apply_kernel, the
smallest row and the first 1024-thread row of softmax_rows.  Each case states the launcher arithmetic that takes it there.

Every result is checked element by element against the fp64 reference and the derived bound of tests/local_error.py (index
kernels and untouched memory: bit-exact).

Every tensor a svr_* entry point writes comes from tests/guarded_out.py (``gout = Pool()``); where a launch gets a view that leaves
the last row / frame of the buffer out, the buffer starts as NaN (``init=``) and the test asserts that the row stayed NaN."""
import math

import pytest
import torch

import local_error as le
from conftest import sub
from guarded_out import Pool
from ops_reference import TorchOps, H16, H16_SCALE, _ld

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
KINDS = [BF16, F32, H16]
KIND_IDS = ["bf16", "fp32", "h16"]


@pytest.fixture(scope="module")
def hip():
    return sub("ops").HipOps("cuda:0")


@pytest.fixture(scope="module")
def ref():
    return TorchOps("cuda:0", act_dtype=torch.float32)


def nans(*shape, dtype=BF16):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def rnd(*shape, scale=1.0, seed=0, dtype=BF16, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    v = torch.randn(*shape, generator=g, device="cuda") * scale + shift
    return (v * H16_SCALE).to(H16) if dtype == H16 else v.to(dtype)


# ------------------------------------------------------------------ rmsnorm_mod
# svr_rmsnorm_mod: grid = ceil(rows / 4) blocks of 4 waves while rows < 8192, then 2048 blocks = 8192 waves, rows strided over the
# waves; a wave of the 2-byte kinds keeps D = 2 rows in flight (raw[0], raw[1]), of fp32 D = 1.
#   8191  last size of the one-row-per-wave grid            8192  2048 blocks, still one row per wave
#   8193  wave 0 owns rows 0 and 8192: raw[1] is used (fp32: refill of raw[0] and second loop trip)
#   16384 every wave uses both slots, nothing is refilled   16385 wave 0 refills raw[0] with row 16384 = row + D * nwaves: second trip
#   24579 waves 0..2 own four rows: both slots refilled, second trip through both (fp32: three refills)
# dim: 8 = one chunk, lanes 1..63 idle; 520 = 65 chunks, only lane 0 has a second one; 2560 / 3072 = NC 5 / 6; 4096 = RMS_MAXC.
RMS_ROWS = [8191, 8192, 8193, 16384, 16385, 24579]


@pytest.mark.parametrize("dim", [8, 520, 2560, 3072, 4096])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_rmsnorm_mod_rows_in_flight(hip, kind, dim):
    # per-row magnitude ramp 2^-5 .. 2^5: a row normalised with another row's 1 / rms is off by a factor of two at least
    ramp = torch.exp2(((torch.arange(RMS_ROWS[-1], device="cuda") * 7) % 11 - 5).float())[:, None]
    xall = rnd(RMS_ROWS[-1], dim, scale=2.0, dtype=F32) * ramp
    xall = (xall * H16_SCALE).to(H16) if kind == H16 else xall.to(kind)
    w, sc, sh = (rnd(dim, dtype=F32, seed=s) for s in (1, 2, 3))
    gout = Pool()
    for rows in RMS_ROWS:
        x = xall[:rows]
        for kw in (dict(), dict(scale=sc, shift=sh), dict(w=w, scale=sc, shift=sh)):
            out = gout(rows + 1, dim, dtype=BF16, init=nans(rows + 1, dim))
            hip.rmsnorm_mod(x, out[:rows], 1e-5, **kw)
            assert bool(torch.isnan(out[rows]).all())                               # nothing behind the last row
            le.check_rmsnorm_mod(out[:rows], x, 1e-5, name=f"rmsnorm_mod rows {rows} {sorted(kw)}", **kw)
            gout.check(f"rmsnorm_mod rows {rows}")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_rmsnorm_mod_every_chunk_count(hip, kind):
    """rmsnorm_mod_kernel<NC, kind> for every NC = ceil(dim / 512) in 1..8 the entry point can select, at the last dim of an NC
    (512 k: every lane holds k chunks) and the one before (512 k - 8: lane 63 holds one fewer).  9 rows: three workgroups of four
    waves, the last with one row."""
    rows = 9
    ramp = torch.exp2(((torch.arange(rows, device="cuda") * 7) % 11 - 5).float())[:, None]
    gout = Pool()
    for dim in [512 * k - d for k in range(1, 9) for d in (8, 0)]:
        x = rnd(rows, dim, scale=2.0, dtype=F32) * ramp
        x = (x * H16_SCALE).to(H16) if kind == H16 else x.to(kind)
        w, sc, sh = (rnd(dim, dtype=F32, seed=s) for s in (1, 2, 3))
        for kw in (dict(), dict(scale=sc, shift=sh), dict(w=w, scale=sc, shift=sh)):
            out = gout(rows + 1, dim, dtype=BF16, init=nans(rows + 1, dim))
            hip.rmsnorm_mod(x, out[:rows], 1e-5, **kw)
            assert bool(torch.isnan(out[rows]).all())                               # nothing behind the last row
            le.check_rmsnorm_mod(out[:rows], x, 1e-5, name=f"rmsnorm_mod dim {dim} {sorted(kw)}", **kw)
            gout.check(f"rmsnorm_mod dim {dim}")


# ------------------------------------------------------------------ qknorm_rope
def _rope_tables(n_pos, n_freq):
    ang = torch.arange(n_pos, dtype=F32)[:, None] * (10000.0 ** (-torch.arange(n_freq, dtype=F32) / max(n_freq, 1)))[None, :]
    return ang.cos().cuda().contiguous(), ang.sin().cuda().contiguous()


def _qknorm_case(hip, rows, heads, n_freq):
    n_pos, t_offset = 64, 2
    qkv = rnd(rows, 3 * heads * 128, scale=3.0, seed=heads)
    r = torch.arange(rows)
    # every row its own position triple; axis 0 with t_offset runs from -1 to 68 (clamped to 0 and to n_pos - 1 = 63 by the kernel),
    # axis 2 up to n_pos + 3
    pos = torch.stack([r % 70 - 3, (r * 7) % n_pos, (r * 13 + 5) % (n_pos + 4)], -1).to(torch.int16).cuda()
    cos, sin = _rope_tables(n_pos, n_freq)
    wq, wk = rnd(128, dtype=F32, seed=1) + 1, rnd(128, dtype=F32, seed=2) + 1
    gout = Pool()
    got = gout.like(qkv, init=qkv)                                                 # (in place: q and k rewritten, V left alone)
    hip.qknorm_rope(got, heads, pos, t_offset, cos, sin, wq, wk, 1e-5)
    le.check_qknorm_rope(got, qkv, heads, pos, t_offset, cos, sin, wq, wk, 1e-5, name=f"qknorm_rope rows {rows} heads {heads} n_freq {n_freq}")
    gout.check("qknorm_rope")


@pytest.mark.parametrize("n_freq", [21, 10, 1])
def test_qknorm_rope_grid_stride(hip, n_freq):
    """svr_qknorm_rope: 8 rows per block, grid = min(ceil(rows / 8), 16 * CUs).  rows = 128 * CUs + 11 -> 16 * CUs + 2 row blocks:
    blocks 0 and 1 take a second trip through the grid-stride loop, the last trip has 3 rows of 8 (row < rows trims whole 32-lane
    groups).  heads = 3: the four-heads-at-a-time walk has one trimmed slot (h0 + u < heads on load and store).
    n_freq 21: pairs 0..62 rotate, pair 63 passes through; 10: pairs 30..63 pass through (axis >= 3 for whole lanes); 1: pairs 3..63."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _qknorm_case(hip, 128 * cus + 11, 3, n_freq)


@pytest.mark.parametrize("n_freq", [21, 10, 1])
@pytest.mark.parametrize("heads", [1, 3, 5, 20, 24])
def test_qknorm_rope_ragged_heads(hip, heads, n_freq):
    """heads 1, 3, 5: the last group of four head vectors is trimmed to 1, 3, 1; 20 and 24 (the 3B / 7B models): never trimmed.
    203 rows = 26 blocks, the last with 3 rows."""
    _qknorm_case(hip, 203, heads, n_freq)


# ------------------------------------------------------------------ GroupNorm
# svr_groupnorm_stats: nblk = ceil(HW / 2048) blocks per frame write partials, groupnorm_reduce_kernel adds them: thread i takes
# partials i, i + 256, ...
#   2047  one ragged block (r1 = min(r0 + 2048, HW))    2048  one full block     2049  two blocks, the second with ONE row
#   4097  three blocks, ragged last                      257 * 2048  nblk = 257: thread 0 of the reduce adds two partials (b += 256)
#   1024 * 1024  nblk = 512: every reduce thread adds two
# svr_groupnorm_apply: gx = min(ceil(HW * C / 8 / 1024), 65535) workgroups per frame, each a contiguous span of ceil(nchunks / gx)
# chunks: HW 2047 / 2049 / 4097 give spans that are not multiples of 256 (ragged tails behind the 4-in-flight loop).
GN_HW = [(23, 89), (32, 64), (3, 683), (17, 241), (514, 1024), (1024, 1024)]


def _gn_case(hip, H, W, C, kind, groups, silus=(True,)):
    T = 2
    x = rnd(T, H, W, C, scale=1.5, shift=0.7, dtype=kind, seed=C)
    gamma, beta = rnd(C, dtype=F32, seed=1) + 1, rnd(C, dtype=F32, seed=2)
    gout = Pool()
    stats = gout(T, groups, 2, dtype=torch.float64)
    hip.groupnorm_stats(x, stats, groups)
    slab = 64 if H * W * C > (1 << 26) else None                                  # fp64 temporaries of a slab: <= 0.5 GB each
    tag = f"HW {H * W} C {C} groups {groups}"
    for t in range(T):
        le.check_groupnorm_stats(stats[t:t + 1], x[t:t + 1], groups, name=f"groupnorm_stats {tag}", slab_rows=slab)
    again = gout.like(stats)
    hip.groupnorm_stats(x, again, groups)
    assert torch.equal(stats, again)                                              # fixed-order reduction: bit-reproducible
    one = gout(1, groups, 2, dtype=torch.float64)
    hip.groupnorm_stats(x[1:2].contiguous(), one, groups)
    assert torch.equal(one[0], stats[1])                                          # independent of the frame's position, at nblk > 1 too
    for silu in silus:
        out = gout(T + 1, H, W, C, dtype=BF16, init=nans(T + 1, H, W, C))
        hip.groupnorm_apply(x, out[:T], stats, gamma, beta, groups, 1e-6, silu)
        assert bool(torch.isnan(out[T, 0, 0]).all())                              # nothing behind the last frame
        le.check_groupnorm_apply(out[:T], x, stats, gamma, beta, groups, 1e-6, silu, name=f"groupnorm_apply {tag} silu {silu}",
                                 slab_rows=slab)
        gout.check(f"groupnorm {tag} silu {silu}")


@pytest.mark.parametrize("C", [128, 256, 512])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("H,W", GN_HW, ids=[f"HW{h * w}" for h, w in GN_HW])
def test_groupnorm_block_structure(hip, H, W, kind, C):
    _gn_case(hip, H, W, C, kind, 32, silus=(True, False) if H * W < 5000 else (True,))


@pytest.mark.parametrize("H,W,C,groups", [(3, 683, 128, 16), (17, 241, 256, 8)])
def test_groupnorm_fewer_groups(hip, H, W, C, groups):
    """16 groups of 8 channels (two quads per group in the block's last stage), 8 groups of 32 (eight quads), over several blocks."""
    _gn_case(hip, H, W, C, BF16, groups, silus=(True, False))


@pytest.mark.parametrize("kind", [BF16, H16], ids=["bf16", "h16"])
def test_groupnorm_apply_capped_grid_on_an_untiled_4k_frame(hip, kind):
    """One 2160 x 3840 x 128 frame: 132.7 M chunks of 8 channels -> ceil(/ 1024) = 129 600 workgroups, CAPPED at 65 535, each with a
    span of ceil(132 710 400 / 65 535) = 2026 chunks = 7 full sweeps of 256 and a ragged one (production reaches this on untiled
    4K decodes).  The statistics come from 4050 row blocks (16 partials per reduce thread).  Reference in 64-row slabs."""
    H, W, C = 2160, 3840, 128
    x = rnd(1, H, W, C, scale=1.5, shift=0.7, dtype=kind)
    gamma, beta = rnd(C, dtype=F32, seed=1) + 1, rnd(C, dtype=F32, seed=2)
    gout = Pool()
    stats = gout(1, 32, 2, dtype=torch.float64)
    hip.groupnorm_stats(x, stats, 32)
    le.check_groupnorm_stats(stats, x, 32, name="groupnorm_stats 4K frame", slab_rows=64)
    out = gout(1, H, W, C, dtype=BF16)
    hip.groupnorm_apply(x, out, stats, gamma, beta, 32, 1e-6, True)
    le.check_groupnorm_apply(out, x, stats, gamma, beta, 32, 1e-6, True, name="groupnorm_apply 4K frame", slab_rows=64)
    gout.check("groupnorm 4K frame")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("C,groups", [(192, 32), (320, 32), (24, 3)])
def test_groupnorm_apply_channel_counts_that_do_not_divide_a_sweep(hip, ref, C, groups, kind):
    """256 % (C / 8) != 0 (24, 40 and 3 chunks per row): a thread's chunks start at a different channel on every sweep, so the
    kernel takes its per-chunk path (scale / offset read from LDS at i % cchunks).  svr_groupnorm_stats does not serve these C
    (its threads own one channel chunk each), so the statistics are the fp64 reference's.  1517 rows: 36 / 60 / 5 spans that are
    not multiples of C / 8, two frames."""
    T, H, W = 2, 37, 41
    x = rnd(T, H, W, C, scale=1.5, shift=0.7, dtype=kind, seed=C)
    gamma, beta = rnd(C, dtype=F32, seed=1) + 1, rnd(C, dtype=F32, seed=2)
    stats = ref.groupnorm_stats(x, torch.empty(T, groups, 2, device="cuda", dtype=torch.float64), groups)    # reference buffer
    gout = Pool()
    for silu in (True, False):
        out = gout(T + 1, H, W, C, dtype=BF16, init=nans(T + 1, H, W, C))
        hip.groupnorm_apply(x, out[:T], stats, gamma, beta, groups, 1e-6, silu)
        assert bool(torch.isnan(out[T]).all())
        le.check_groupnorm_apply(out[:T], x, stats, gamma, beta, groups, 1e-6, silu, name=f"groupnorm_apply C {C} silu {silu}")
        gout.check(f"groupnorm_apply C {C} silu {silu}")


# ------------------------------------------------------------------ softmax_rows
@pytest.mark.parametrize("cols", [4, 16384, 16388, 65532, 65536])
def test_softmax_rows_edges(hip, cols):
    """svr_softmax_rows: the 256-thread kernel up to 16384 columns (16 float4 per thread), the 1024-thread kernel above.
    4 columns: one float4, thread 0 alone holds data (every other lane contributes -inf / 0 to the reductions); 16384: the last
    row of the 256-thread kernel, every register slot full; 16388: the first row of the 1024-thread kernel (4097 float4: thread 0
    alone has a fifth); 65532 / 65536: its last sweep ragged / full."""
    g = torch.Generator(device="cuda").manual_seed(cols)
    S = torch.randn(7, cols, device="cuda", generator=g) * 30.0
    S[1, -1] = 400.0                                                               # the maximum is the row's last element
    S[2] = 3.25                                                                    # a row of equal values
    S[3, 0] = -1e4                                                                 # exp2 underflows to zero
    gout = Pool()
    P = gout(8, cols, dtype=BF16, init=nans(8, cols))
    hip.softmax_rows(S, P[:7], 0.044)
    assert bool(torch.isnan(P[7]).all())
    le.check_softmax_rows(P[:7], S, 0.044, name=f"softmax_rows cols {cols}")
    gout.check(f"softmax_rows cols {cols}")


# ------------------------------------------------------------------ rows_mean, unpatchify_euler
def test_rows_mean_one_group_and_ragged_dim(hip):
    """n_groups = 1 (a copy through fp32: bit-exact); dim 520 = 65 chunks: the second 64-thread block has one live thread."""
    src = rnd(58, 2560)
    gout = Pool()
    dst = gout(58, 2560, dtype=BF16)
    hip.rows_mean(src, dst, 1, 58)
    assert torch.equal(dst, src)
    for n_groups, rows, dim in ((7, 58, 520), (3, 5, 8)):
        src = rnd(n_groups * rows, dim)
        dst = gout(rows + 1, dim, dtype=BF16, init=nans(rows + 1, dim))
        hip.rows_mean(src, dst[:rows], n_groups, rows)
        assert bool(torch.isnan(dst[rows]).all())
        le.check(f"rows_mean {n_groups} x {rows} x {dim}", dst[:rows], *le.rows_mean_reference(src, n_groups, rows))
    gout.check("rows_mean")


def test_unpatchify_euler_padded_prediction(hip):
    """pred.stride(0) = 96 > 4 C = 64: production hands over the padded output of the last GEMM; the pad columns hold NaN."""
    T, H, W, C = 3, 8, 12, 16
    pred = rnd(T * (H // 2) * (W // 2), 96)
    pred[:, 4 * C:] = float("nan")
    x_t = rnd(T, H, W, C, seed=4)
    gout = Pool()
    for xt in (x_t, None):
        o = gout(T, H, W, C, dtype=BF16)
        hip.unpatchify_euler(pred, xt, o)
        le.check("unpatchify_euler ldp 96", o, *le.unpatchify_euler_reference(pred, xt, o.shape))
    o = gout(T, H, W, C, dtype=BF16)
    hip.unpatchify_euler(pred, None, o)                                            # without x_t it is an index map: bit-exact
    want = pred[:, :4 * C].reshape(T, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(T, H, W, C)
    assert torch.equal(o, want)
    gout.check("unpatchify_euler")


# ------------------------------------------------------------------ window attention, first-generation kernel
@pytest.mark.parametrize("lens,heads", [([2083, 2083, 641], 24), ([2083, 1, 2083, 2, 641], 3)], ids=["cfg5_24_heads", "3_heads_tiny_windows"])
def test_attn_varlen_windows_beyond_the_row_table(hip, lens, heads):
    """max_len 2083 > 2048 rows (the second kernel's LDS row table): the whole launch goes to the first-generation kernel, as the
    2083-row windows of BASELINE config 5 do with 24 heads.  2083 = 16 query tiles of 128 + 35 rows, 32 key tiles of 64 + 35 keys."""
    D, n_rows = 128, 5000
    qkv = rnd(n_rows, 3 * heads * D)
    g = torch.Generator().manual_seed(1)
    total = sum(lens)
    seq_rows = torch.cat([torch.randint(0, n_rows, (L,), generator=g) for L in lens]).to(torch.int32).cuda()
    out_rows = torch.randperm(total + 16, generator=g)[:total].to(torch.int32).cuda()
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32).cuda()
    gout = Pool()
    out = gout(total + 16, heads * D, dtype=BF16, init=torch.full((total + 16, heads * D), 7.0, device="cuda", dtype=BF16))
    before = out.clone()
    hip.attn_varlen(qkv, out, seq_rows, out_rows, cu, max(lens), heads, D, 1.0 / math.sqrt(D))
    le.check_attn(out, qkv, seq_rows, out_rows, cu, heads, D, 1.0 / math.sqrt(D), before=before, name=f"attn_varlen {lens} x {heads}")
    gout.check("attn_varlen beyond the row table")
