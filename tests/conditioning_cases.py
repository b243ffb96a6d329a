"""TEST INFRASTRUCTURE: inputs OUTSIDE the zero-mean, unit-scale Gaussians every other kernel test draws -- shared by the CPU proof
(tests/test_local_error.py) and the GPU tests (tests/test_gpu_conditioning.py), so that both see the same data.

  * offset_groups: GroupNorm inputs whose groups sit at mean / std = rho (the variance E[x^2] - mean^2 loses rho^2 of its digits);
  * scaled_rows: rows of a row-normalising kernel at the magnitudes the wide residual stream allows;
  * bias_sweep / act_sweep: fp32 values at which a store or a fast activation can go wrong (rounding ties, overflow, the
    subnormal range of a format, exp2 saturating);
  * attn_score_cases: (q, k, v) of one attention window whose SCORES are steered tile by tile -- growth of the running maximum
    just under and just over the deferral threshold of the window kernel's online softmax, rows of one query block that disagree
    about rescaling, weight on the keys the ragged last tile duplicates, exponents far from 0."""
import math

import torch

from ops_reference import H16, H16_SCALE, EPI_BIAS_GELU, EPI_BIAS_SILU, _st

F32 = torch.float32


def offset_groups(T, H, W, C, groups, rho, std, kind, device="cpu", seed=0):
    """std (rho_tg + N(0, 1)) in storage ``kind``: group g of frame t sits at rho_tg = +-rho (1 - ((g + 3 t) % 8) / 16) -- between
    9/16 rho and rho, another value in every neighbouring group and in the other frame (a statistic read from the wrong group or
    frame is off by 1/16 of the mean at least), the sign alternating with the frame."""
    gen = torch.Generator(device=device).manual_seed(seed + H * W + C)
    g, t = torch.arange(groups, device=device), torch.arange(T, device=device)[:, None]
    r = rho * (1.0 - ((g[None, :] + 3 * t) % 8).double() / 16.0) * (1.0 - 2.0 * (t % 2))                     # [T, groups]
    x = (torch.randn(T, H, W, C, generator=gen, device=device, dtype=torch.float64)
         + r.repeat_interleave(C // groups, dim=1)[:, None, None, :]) * std
    return _st(x.float(), torch.empty(0, dtype=kind, device=device))


ROW_KINDS = ("2^-20", "1", "2^21", "one channel x300", "zero")


def scaled_rows(dim, kind, device="cpu", seed=0):
    """[43, dim] in storage ``kind``.  Rows 0..19: five 4-row blocks (the row-normalising kernels take 4 rows per workgroup), one
    per ROW_KINDS entry -- N(0, 1) clamped to +-1.9 times 2^-20 / 1 / 2^21 (1.9 * 2^21 < 65504 * 64: the top of h16's range),
    N(0, 1) with channel 5 times 300 (the heavy-tail checkpoint statistic), all zero.  Rows 20..42: the five kinds in turn, so
    every 4-row block mixes four of them (and the last block is ragged).  -> (x, kind index of every row)."""
    gen = torch.Generator(device=device).manual_seed(seed + dim)
    which = torch.tensor([k for k in range(5) for _ in range(4)] + [i % 5 for i in range(23)], device=device)
    v = torch.randn(43, dim, generator=gen, device=device).clamp(-1.9, 1.9)
    scale = torch.tensor([2.0 ** -20, 1.0, 2.0 ** 21, 1.0, 0.0], device=device)[which][:, None]
    v = v * scale
    v[which == 3, 5 % dim] *= 300.0
    return _st(v, torch.empty(0, dtype=kind, device=device)), which


def _f32(bits, device):
    """fp32 values from their bit patterns"""
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32, device=device).view(F32)


def bias_sweep(device="cpu"):
    """fp32 values (a multiple of 8 of them) at which a bf16 / h16 / fp32 store can go wrong, both signs of each:
      * 0; the powers of two 2^-126 .. 2^127 in steps of 11 (the whole normal exponent range);
      * bf16 rounding ties: fp32 patterns ...8000 with bit 16 clear (even lower neighbour: rounds down) and set (odd: rounds up),
        at three exponents, and their neighbours ...7fff / ...8001 (just below / above the tie);
      * the last tie below bf16's maximum, 0x7f7f8000 (rounds to inf), and its two neighbours;
      * the h16 analogues (the stored half is x 2^-6, so x = 64 h): ties at 11 bits -- h = 1 + (2 k + 1) 2^-11 with the lower
        neighbour even and odd, +- one fp32 ulp; x around 65504 * 64 (65519.99 * 64 -> 65504, >= 65520 * 64 -> inf); x in and below
        half's subnormal range: 3.8e-6 {0.49, 0.5, 0.51, 1, 1.5} (2^-24 * 64 = 3.8e-6 is the smallest h16 value, half of it a tie
        to even = 0)."""
    bits = [0x00000000]
    bits += [(e << 23) for e in range(1, 255, 11)] + [0x7f000000]
    for e in (0x3f800000, 0x42000000, 0x2f800000):                         # 1.0, 32.0, 2^-32: mantissa ties
        for m in (0x00008000, 0x00018000, 0x007e8000, 0x007f8000):          # bit 16 clear / set / clear / set (carry into the exponent)
            bits += [e + m - 1, e + m, e + m + 1]
    bits += [0x7f7f7fff, 0x7f7f8000, 0x7f7f8001, 0x7f7f0000]
    v = _f32(bits, device)
    h = []
    for k in (0, 1, 511, 1022, 1023):                                      # ties of the 11-bit significand at h in [1, 2)
        tie = 1.0 + (2 * k + 1) * 2.0 ** -11
        h += [tie * (1 - 2.0 ** -23), tie, tie * (1 + 2.0 ** -23)]
    h += [65503.0, 65504.0, 65519.0, 65519.99, 65520.0, 65521.0, 70000.0, 2.0 ** 17]
    h += [2.0 ** -24 * f for f in (0.49, 0.5, 0.51, 1.0, 1.5, 2.5, 1023.5, 1024.0)]
    v = torch.cat([v, torch.tensor(h, dtype=torch.float64, device=device).mul(64.0).to(F32)])
    v = torch.cat([v, -v])
    return torch.cat([v, v[: -v.numel() % 8]])


ACT_ARGS = (0.0, 2.0 ** -130, 1e-30, 1e-3, 1.0, 10.0, 20.0, 80.0, 87.0, 88.7, 89.0, 100.0, 1e4, 1e19, 3e38)


def act_sweep(device="cpu"):
    """The arguments at which x sigmoid(x) / tanh-GELU through v_exp_f32 and v_rcp_f32 can go wrong, both signs (32 values, two of
    them the zeros): exp2 saturating to inf (x < -88.7) and to 0, rcp(inf), x^3 overflowing fp32 (|x| > 7e12), arguments in fp32's
    denormal range."""
    v = torch.tensor(ACT_ARGS, dtype=torch.float64, device=device).to(F32)
    return torch.cat([v, -v, v[:1], -v[:1]])


# ------------------------------------------------------------------------------------------------ attention: steered score ranges
LOG2E = 1.4426950408889634
TEXT_ROWS = 58                          # the text rows that close every production window
ATTN_SCORE_CASES = ("step_below", "step_above", "stairs", "rows_disagree", "one_row_votes", "ramp_down", "tail_pair", "flat_high",
                    "flat_low", "hot_gauss", "text_tail")


def attn_log2_scores(q, k, scale):
    """fp64 scores of the stored values in log2 units: [L, L]"""
    return (q.double() @ k.double().t()) * (scale * LOG2E)


def attn_score_cases(L, D, kt, device="cpu", seed=0):
    """name -> (q, k, v), bf16 [L, D], for one attention window with scale = 1 / sqrt(D) over ``kt``-key tiles (tile = key // kt).

    The steered cases put the score into coordinate 0: q[:, 0] = a_i and k[:, 0] = g_j sqrt(D) / log2(e), so that pair (i, j) scores
    a_i g_j in LOG2 units (the unit of the kernels' exponent and of the window kernel's deferral threshold); every other coordinate
    of q and k is N(0, 0.05^2) (0.004 log2 units of score), v is N(0, 1): every key has a value row of its own.

      step_below     a 1, g 5.75 [tile >= 1]      the maximum grows by just under 2^6 at tile 1 and stays: a deferred rescale, P up
                                                  to 2^5.75 for the rest of the window
      step_above     a 1, g 6.25 [tile >= 1]      just over 2^6: a rescale at tile 1
      stairs         a 1, g 5.75 tile             deferred and forced tiles in turn (growth counts from the kept maximum, not from
                                                  the previous tile)
      rows_disagree  a +1 even / -1 odd rows, g 9 tile     half of a query block's rows force every rescale, the other half get
                                                  alpha = 1 and vanishing P
      one_row_votes  a 1 on rows 13 mod 32 else 0, g 30 [tile >= 2]     one row (one lane pair) decides the block's vote
      ramp_down      a 1, g -20 tile              no rescale after tile 0, exponents down to -20 (tiles - 1)
      tail_pair      a 1, g 12 at key L - 2, 10 at key L - 1, else 0    the weight sits on the key a ragged tile duplicates (and
                                                  on its neighbour: duplicates of a ONE-hot key would change nothing)
      flat_high / flat_low   a 1, g +-115         s c - m c cancels at a large magnitude; uniform softmax
      hot_gauss      q, k ~ N(0, 4^2) in every coordinate     scores about +-100 log2 units, near one-hot, rescales at random rows
      text_tail      q, k, v ~ N(0, 1), the last 58 rows of q and k times 6     the production pattern (L >= 64 only)

    The premises the cases exist for are asserted here, on the fp64 scores of the STORED bf16 values (the rounding of k[:, 0]
    included): step_below / step_above -- every row's (tile-1 maximum - tile-0 maximum) lies in (5.0, 5.9) / (6.1, 7.0); tail_pair
    -- the last two keys hold more than 0.9 of every row's softmax mass (windows of more than 512 keys: the other L - 2 keys, at
    weight 1 each, outweigh that by count -- there more than 0.9 of (2^12 + 2^10) / (2^12 + 2^10 + L - 2), the share the stated g
    gives)."""
    gen = torch.Generator().manual_seed(seed + 131 * L + D + kt)         # (drawn on the host: the same data on every device)
    randn = lambda *s: torch.randn(*s, generator=gen)
    scale = 1.0 / math.sqrt(D)
    key = torch.arange(L)
    tile = (key // kt).float()
    one = torch.ones(L)
    row = torch.arange(L)
    tail = torch.zeros(L)
    tail[L - 1] = 10.0
    if L >= 2:
        tail[L - 2] = 12.0
    steered = {
        "step_below": (one, 5.75 * (tile >= 1)),
        "step_above": (one, 6.25 * (tile >= 1)),
        "stairs": (one, 5.75 * tile),
        "rows_disagree": (1.0 - 2.0 * (row % 2), 9.0 * tile),
        "one_row_votes": ((row % 32 == 13).float(), 30.0 * (tile >= 2)),
        "ramp_down": (one, -20.0 * tile),
        "tail_pair": (one, tail),
        "flat_high": (one, 115.0 * one),
        "flat_low": (one, -115.0 * one),
    }
    cases = {}
    for name, (a, g) in steered.items():
        q, k = randn(L, D) * 0.05, randn(L, D) * 0.05
        q[:, 0] = a
        k[:, 0] = g * (math.sqrt(D) / LOG2E)
        cases[name] = (q.to(torch.bfloat16), k.to(torch.bfloat16), randn(L, D).to(torch.bfloat16))
    cases["hot_gauss"] = ((randn(L, D) * 4.0).to(torch.bfloat16), (randn(L, D) * 4.0).to(torch.bfloat16), randn(L, D).to(torch.bfloat16))
    if L >= 64:
        q, k = randn(L, D), randn(L, D)
        q[L - TEXT_ROWS:] *= 6.0
        k[L - TEXT_ROWS:] *= 6.0
        cases["text_tail"] = (q.to(torch.bfloat16), k.to(torch.bfloat16), randn(L, D).to(torch.bfloat16))

    if L > kt:
        for name, lo, hi in (("step_below", 5.0, 5.9), ("step_above", 6.1, 7.0)):
            s = attn_log2_scores(*cases[name][:2], scale)
            growth = s[:, kt:min(2 * kt, L)].amax(dim=1) - s[:, :kt].amax(dim=1)
            assert bool(((growth > lo) & (growth < hi)).all()), (name, float(growth.min()), float(growth.max()))
    if L >= 2:
        mass = torch.softmax(attn_log2_scores(*cases["tail_pair"][:2], scale) * math.log(2.0), dim=1)[:, L - 2:].sum(dim=1)
        floor = 0.9 if L <= 512 else 0.9 * 5120.0 / (5120.0 + L - 2)
        assert bool((mass > floor).all()), ("tail_pair", float(mass.min()), floor)
    return {name: tuple(t.to(device) for t in qkv) for name, qkv in cases.items()}


# ------------------------------------------------------------------------------------------------ zero-operand launches, one per kernel class
# name -> the kernel class the launch must be served by (svr_gemm_kernel_class), its geometry -- the smallest that routes there --
# and the library options it needs.  mnk: a plain GEMM; conv: (Cin, Cout, taps, stride, spatial pads (lo, hi), T, H, W).
# frag: which fragment-ordered weight copy goes with it.  pairs: the (output, residual) storage kinds of EPI_RESID_GATE the class
# has a form for (None: all nine; ()): no residual at all).  acts: epilogue -> the class that serves it on this geometry
# ("error": the library refuses the launch), for the storage kinds in act_kinds.
OPTION_DEFAULTS = {"gemm_epi": 0, "conv_rows": 8, "conv_impl": 0}
_ALL_ACTS = lambda cls: {EPI_BIAS_SILU: cls, EPI_BIAS_GELU: cls}
ZERO_OPERAND_CASES = {
    "gemm_epi_direct": dict(cls="gemm", mnk=(257, 256, 64), options={"gemm_epi": 1}, acts=_ALL_ACTS("gemm")),
    "gemm_epi_lds": dict(cls="gemm", mnk=(257, 256, 64), options={"gemm_epi": 2}, acts=_ALL_ACTS("gemm")),
    # (h16 in the persistent kernel: bias -> h16 and h16 residual -> h16 only -- the two forms of the NaDiT's residual stream)
    "gemm_persistent": dict(cls="gemm_persistent", mnk=(4096, 4096, 128), acts=_ALL_ACTS("gemm_persistent"), act_kinds=("bf16", "fp32"),
                            pairs=(("bf16", "bf16"), ("bf16", "fp32"), ("fp32", "fp32"), ("fp32", "bf16"), ("h16", "h16"))),
    # (the LDS-halo kernel's epilogue has SiLU but no tanh-GELU: the generic kernel serves that launch; the thin-input geometry has
    # no other kernel, the library refuses it)
    "conv_halo_lds_weights": dict(cls="conv_halo", conv=(128, 128, (3, 3, 3), (1, 1, 1), (1, 1), 3, 10, 12),
                                  acts={EPI_BIAS_SILU: "conv_halo", EPI_BIAS_GELU: "conv_generic"}),
    "conv_halo_wreg_4rows": dict(cls="conv_halo", conv=(128, 128, (3, 3, 3), (1, 1, 1), (1, 1), 3, 10, 12), frag="conv33",
                                 options={"conv_rows": 4}, acts={EPI_BIAS_SILU: "conv_halo", EPI_BIAS_GELU: "conv_generic"}),
    "conv_halo_wreg_8rows": dict(cls="conv_halo", conv=(128, 128, (3, 3, 3), (1, 1, 1), (1, 1), 3, 10, 12), frag="conv33",
                                 options={"conv_rows": 8}, acts={EPI_BIAS_SILU: "conv_halo", EPI_BIAS_GELU: "conv_generic"}),
    "conv_subpixel": dict(cls="conv_subpixel", conv=(128, 128, (3, 2, 2), (1, 1, 1), (1, 0), 3, 9, 11), frag="conv22", pairs=(), acts={}),
    "conv_thin_in": dict(cls="conv_thin_in", conv=(4, 128, (1, 3, 3), (1, 1, 1), (1, 1), 2, 8, 32),
                         acts={EPI_BIAS_SILU: "conv_thin_in", EPI_BIAS_GELU: "error"}),
    "conv_thinout_3_cout": dict(cls="conv_thinout", conv=(128, 3, (1, 3, 3), (1, 1, 1), (1, 1), 2, 9, 33), acts=_ALL_ACTS("conv_thinout")),
    "conv_thinout_32_cout": dict(cls="conv_thinout", conv=(128, 32, (1, 3, 3), (1, 1, 1), (1, 1), 2, 9, 33), acts=_ALL_ACTS("conv_thinout")),
    "conv_generic_stride_2": dict(cls="conv_generic", conv=(256, 256, (3, 3, 3), (2, 2, 2), (0, 1), 5, 12, 10), acts=_ALL_ACTS("conv_generic")),
}
STORE_KINDS = {"bf16": torch.bfloat16, "h16": H16, "fp32": F32}


def zero_operand_problem(spec, opsmod, device="cpu", frag=None, operand="zero"):
    """The launch of a ZERO_OPERAND_CASES entry: -> (A, W, gemm keywords, output shape).  A (the conv input) is all zero, so the
    accumulator is exactly 0 whatever the weights are: W holds N(0, 1) bf16 values in the packed [ceil128(N), K] layout.
    ``frag(kind, W, spec) -> tensor``: builds the fragment-ordered copy ("conv33" / "conv22" / "gemm").  device "meta": shapes only
    (routing questions to svr_gemm_kernel_class)."""
    def weights(n, k):
        if device == "meta":
            return torch.empty(-(-n // 128) * 128, k, dtype=torch.bfloat16, device="meta")
        gen = torch.Generator().manual_seed(n + k)
        return torch.randn(-(-n // 128) * 128, k, generator=gen).to(torch.bfloat16).to(device)
    zeros = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device="meta") if device == "meta" else \
        torch.zeros(*s, dtype=torch.bfloat16, device=device)
    if "mnk" in spec:
        M, N, K = spec["mnk"]
        A, W, kw, shape = zeros(M, K), weights(N, K), dict(N=N, K=K), (M, N)
    else:
        Cin, Cout, k, stride, (plo, phi), T, H, W_ = spec["conv"]
        pt = k[0] - 1
        To = (T + pt - k[0]) // stride[0] + 1
        Ho, Wo = (H + plo + phi - k[1]) // stride[1] + 1, (W_ + plo + phi - k[2]) // stride[2] + 1
        K = 128 if Cin == 4 else k[0] * k[1] * k[2] * Cin                     # (thin input: taps * 4 zero-padded to 128)
        A, W = zeros(T, H, W_, Cin), weights(Cout, K)
        if Cin == 4 and device != "meta":
            W[:, k[0] * k[1] * k[2] * 4:] = 0
        kw = dict(N=Cout, K=K, conv=opsmod.Conv3dGeom(T, H, W_, Cin, To, Ho, Wo, k, stride, (pt, plo, plo), None), ldc=Cout)
        shape = (To, Ho, Wo, Cout)
    if spec.get("frag"):
        kw["W_frag"] = frag(spec["frag"], W, spec)
    return A, W, kw, shape
