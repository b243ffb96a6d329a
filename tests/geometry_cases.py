"""TEST INFRASTRUCTURE: launch geometries at the tile edges of the conv family, the plain GEMM and the window attention -- one
table, shared by the CPU tests (tests/test_geometry_cases.py: every row routes to the kernel class it names, the table covers
every class, kernel instance and axis value, the fp64 reference agrees with F.conv3d on every row) and the GPU sweep
(tests/test_gpu_geometry_sweep.py: every row against its per-element bounds on a guarded, poisoned output).

Why these rows.  The halo kernels work in patches -- conv_halo2_kernel 16 x 32 voxels (8 x 32 with conv_rows 4 and on a thin
input), conv_thinout_kernel 8 x 32, conv_thinout4_kernel and conv_sub_kernel 16 x 32 -- over 32-channel slices, one output frame at
a time.  The hand-picked cases of tests/test_gpu_kernels.py leave their edges unrun: frames smaller than one halo ring (H or W of
1 or 2), exactly one patch, one voxel more than a patch, a single input frame (the engine's branch for slices shorter than the
carry), the two-tap causal-head weight, the tail launch behind it (T = 2, kt = 3, pt = 1), the smallest Cin (two slices per
tap) and Cin 320 / 384.  Not a cross product: every value of every axis meets every kernel INSTANCE at least once (INSTANCES
says which values an instance can meet at all), test_geometry_cases.py asserts it.

A row:  R(instance, H, W, temporal case, Cin, N, output kind, residual kind, gn_groups, epilogue, sub=...)
  temporal case   key of TK: input frames T, temporal taps kt, causal pad pt, carried halo frames (0: the first frame repeated)
  kinds           "bf16" | "fp32" | "h16" (ops.H16: an IEEE half holding x * 2^-6); residual None: no residual
  gn_groups       32: the launch also produces the fused GroupNorm statistics (N / 32 in {4, 8, 16} channels per group)
  epilogue        "bias" | "resid" (EPI_RESID_GATE with the residual) | "silu"
  sub             conv_sub rows: ("phase" four single-phase launches | "quad" one launch, t_stride, border bias vectors or not)
"""
import collections
import math

import torch

from ops_reference import H16, H16_SCALE, EPI_BIAS, EPI_BIAS_SILU, EPI_BIAS_GELU, EPI_RESID_GATE

BF16, F32 = torch.bfloat16, torch.float32
STORE_KINDS = {"bf16": BF16, "h16": H16, "fp32": F32}
EPILOGUES = {"bias": EPI_BIAS, "resid": EPI_RESID_GATE, "silu": EPI_BIAS_SILU, "gelu": EPI_BIAS_GELU}

HW = [(1, 1), (1, 33), (2, 2), (2, 31), (7, 32), (8, 33), (15, 64), (16, 32), (17, 65), (33, 31), (48, 70)]
TK = {  # T, kt, pt, halo frames
    "T1_kt3": (1, 3, 2, 0),                 # one input frame, all three taps on it
    "T1_kt3_halo2": (1, 3, 2, 2),           # one input frame behind two carried ones
    "T1_kt2_head": (1, 2, 1, 0),            # the causal-head weight (two taps folded from three), one input frame
    "T2_kt3_pt1": (2, 3, 1, 0),             # the tail launch behind a causal-head launch: To = 1
    "T3_kt1": (3, 1, 0, 0),
    "T4_kt3_halo2": (4, 3, 2, 2),
}
TK_OTHER = {"T3_kt3": (3, 3, 2, 0)}          # temporal cases outside the coverage axes (the conv_band cases)


def temporal(tk):
    """(T, kt, pt, halo frames) of a row's temporal case"""
    return TK[tk] if tk in TK else TK_OTHER[tk]


CINS, NS = (64, 128, 320, 384, 512), (128, 256, 384, 512)
OUT_KINDS, RESID_KINDS = ("bf16", "fp32", "h16"), (None, "bf16", "fp32", "h16")
PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))

# kernel instance -> the class svr_gemm_kernel_class must report, the fragment-ordered weight copy and the options that select it,
# and the axis values it can meet (Cin / N / residual kinds; every instance meets all of HW, TK and OUT_KINDS).
# The library reports the CLASS of a launch only.  Which instance of a class serves a row is the launcher's reading of the row's
# W_frag / conv_rows / N (launch_conv_halo2, launch_conv_thinout): of that, the tests can observe the patch height through the
# block count of the fused statistics (patch_rows; asserted on the rows with gn_groups) and restate the 4-cout kernel's LDS rule
# (thinout4_serves) -- a launcher that ignored W_frag on a 16-row patch, or picked the other GEMM tile, would go unnoticed here.
INSTANCES = {
    "halo16_lds": dict(cls="conv_halo", frag=None, options={}, cins=CINS, ns=NS, resids=RESID_KINDS, patch_rows=16),   # conv_halo2_kernel<16, 0>
    "halo16_wreg8": dict(cls="conv_halo", frag="conv33", options={"conv_rows": 8}, cins=CINS, ns=NS, resids=RESID_KINDS, patch_rows=16),   # <16, 3>
    "halo8_wreg4": dict(cls="conv_halo", frag="conv33", options={"conv_rows": 4}, cins=CINS, ns=NS, resids=RESID_KINDS, patch_rows=8),    # <8, 1>
    "thin_in": dict(cls="conv_thin_in", frag=None, options={}, cins=(4,), ns=NS, resids=RESID_KINDS, patch_rows=8),    # <8, 2>
    "thinout32": dict(cls="conv_thinout", frag=None, options={}, cins=CINS, ns=(16, 32), resids=RESID_KINDS),       # conv_thinout_kernel
    "thinout4": dict(cls="conv_thinout", frag=None, options={}, cins=(64, 128, 320, 384), ns=(3, 4), resids=RESID_KINDS),
    "conv_sub": dict(cls="conv_subpixel", frag="conv22", options={}, cins=CINS, ns=NS, resids=(None,), patch_rows=16),
}
OPTION_DEFAULTS = {"conv_rows": 8, "conv_impl": 0, "conv_band": 1, "conv_sub": 1, "conv_thinout4": 1, "gemm_epi": 0, "gemm_w4": 1,
                   "gemm_w4r": 1, "attn_impl": 0}


def thinout4_serves(Cin, kt, N):
    """conv_thinout4_kernel takes a thin-output launch when its resident weights fit next to the halo ring (launch_conv_thinout in
    csrc/svr_conv_thinout.hip: 3 * 40960 B ring + ceil4096(Cin / 32 * kt * 9 * 256) + 8192 B <= 160 KiB); else conv_thinout_kernel."""
    return N <= 4 and Cin % 32 == 0 and 122880 + -(-(Cin // 32 * kt * 9 * 256) // 4096) * 4096 + 8192 <= 160 * 1024


ConvRow = collections.namedtuple("ConvRow", "inst H W tk Cin N out resid gn epi sub")


def R(inst, H, W, tk, Cin, N, out, resid, gn, epi, sub=None):
    return ConvRow(inst, H, W, tk, Cin, N, out, resid, gn, epi, sub)


def row_id(r):
    s = f"{r.inst}-{r.H}x{r.W}-{r.tk}-c{r.Cin}-n{r.N}-{r.out}-{r.epi}{'_' + r.resid if r.resid else ''}{'-gn' if r.gn else ''}"
    return s + (f"-{r.sub[0]}-ts{r.sub[1]}{'-bb' if r.sub[2] else ''}" if r.sub else "")


CONV_ROWS = [
    # conv_halo2_kernel: halo16_lds
    R("halo16_lds", 1, 1, "T4_kt3_halo2", 512, 512, "bf16", None, 32, "silu"),
    R("halo16_lds", 1, 33, "T2_kt3_pt1", 384, 384, "bf16", "bf16", 0, "resid"),
    R("halo16_lds", 2, 2, "T1_kt3_halo2", 320, 512, "fp32", None, 32, "bias"),
    R("halo16_lds", 2, 31, "T3_kt1", 512, 256, "h16", "h16", 0, "resid"),
    R("halo16_lds", 7, 32, "T1_kt2_head", 384, 128, "bf16", "fp32", 32, "resid"),
    R("halo16_lds", 8, 33, "T1_kt3", 320, 256, "fp32", "fp32", 0, "resid"),
    R("halo16_lds", 15, 64, "T3_kt1", 128, 384, "h16", None, 0, "silu"),
    R("halo16_lds", 16, 32, "T4_kt3_halo2", 64, 128, "bf16", "h16", 0, "resid"),
    R("halo16_lds", 17, 65, "T1_kt2_head", 128, 256, "fp32", "bf16", 32, "resid"),
    R("halo16_lds", 33, 31, "T2_kt3_pt1", 64, 512, "h16", "bf16", 0, "resid"),
    R("halo16_lds", 48, 70, "T1_kt3", 64, 128, "h16", "fp32", 32, "resid"),
    R("halo16_lds", 17, 65, "T1_kt3_halo2", 128, 128, "fp32", "h16", 0, "resid"),
    # conv_halo2_kernel: halo16_wreg8
    R("halo16_wreg8", 1, 1, "T4_kt3_halo2", 512, 512, "bf16", "fp32", 0, "resid"),
    R("halo16_wreg8", 1, 33, "T2_kt3_pt1", 384, 384, "fp32", "fp32", 0, "resid"),
    R("halo16_wreg8", 2, 2, "T1_kt3_halo2", 320, 512, "h16", None, 0, "bias"),
    R("halo16_wreg8", 2, 31, "T3_kt1", 512, 256, "bf16", "h16", 32, "resid"),
    R("halo16_wreg8", 7, 32, "T1_kt2_head", 384, 128, "fp32", "bf16", 0, "resid"),
    R("halo16_wreg8", 8, 33, "T1_kt3", 320, 256, "h16", "bf16", 32, "resid"),
    R("halo16_wreg8", 15, 64, "T3_kt1", 128, 384, "h16", "fp32", 0, "resid"),
    R("halo16_wreg8", 16, 32, "T4_kt3_halo2", 64, 128, "fp32", "h16", 32, "resid"),
    R("halo16_wreg8", 17, 65, "T1_kt2_head", 128, 256, "bf16", None, 0, "bias"),
    R("halo16_wreg8", 33, 31, "T2_kt3_pt1", 64, 512, "bf16", "bf16", 32, "resid"),
    R("halo16_wreg8", 48, 70, "T1_kt3", 64, 128, "fp32", None, 0, "silu"),
    R("halo16_wreg8", 17, 65, "T1_kt3_halo2", 128, 128, "h16", "h16", 32, "resid"),
    # conv_halo2_kernel: halo8_wreg4
    R("halo8_wreg4", 1, 1, "T4_kt3_halo2", 512, 512, "fp32", "bf16", 32, "resid"),
    R("halo8_wreg4", 1, 33, "T2_kt3_pt1", 384, 384, "h16", "bf16", 0, "resid"),
    R("halo8_wreg4", 2, 2, "T1_kt3_halo2", 320, 512, "h16", "fp32", 32, "resid"),
    R("halo8_wreg4", 2, 31, "T3_kt1", 512, 256, "fp32", "h16", 0, "resid"),
    R("halo8_wreg4", 7, 32, "T1_kt2_head", 384, 128, "bf16", None, 32, "bias"),
    R("halo8_wreg4", 8, 33, "T1_kt3", 320, 256, "bf16", "bf16", 0, "resid"),
    R("halo8_wreg4", 15, 64, "T3_kt1", 128, 384, "fp32", None, 0, "bias"),
    R("halo8_wreg4", 16, 32, "T4_kt3_halo2", 64, 128, "h16", "h16", 0, "resid"),
    R("halo8_wreg4", 17, 65, "T1_kt2_head", 128, 256, "bf16", "fp32", 32, "resid"),
    R("halo8_wreg4", 33, 31, "T2_kt3_pt1", 64, 512, "fp32", "fp32", 0, "resid"),
    R("halo8_wreg4", 48, 70, "T1_kt3", 64, 128, "h16", None, 32, "bias"),
    R("halo8_wreg4", 17, 65, "T1_kt3_halo2", 128, 128, "bf16", "h16", 0, "resid"),
    # conv_halo2_kernel<8, 2>: thin input (Cin 3 padded to 4, K = taps * 4 zero-padded to 128)
    R("thin_in", 1, 1, "T1_kt3_halo2", 4, 128, "bf16", "bf16", 0, "resid"),
    R("thin_in", 1, 33, "T1_kt2_head", 4, 256, "h16", None, 32, "bias"),
    R("thin_in", 2, 2, "T2_kt3_pt1", 4, 384, "fp32", "h16", 0, "resid"),
    R("thin_in", 2, 31, "T3_kt1", 4, 512, "bf16", "fp32", 32, "resid"),
    R("thin_in", 7, 32, "T4_kt3_halo2", 4, 128, "h16", "bf16", 0, "resid"),
    R("thin_in", 8, 33, "T1_kt3", 4, 256, "fp32", None, 32, "bias"),
    R("thin_in", 15, 64, "T1_kt3_halo2", 4, 384, "bf16", "h16", 0, "resid"),
    R("thin_in", 16, 32, "T1_kt2_head", 4, 512, "bf16", None, 32, "bias"),
    R("thin_in", 17, 65, "T2_kt3_pt1", 4, 128, "fp32", "fp32", 0, "resid"),
    R("thin_in", 33, 31, "T3_kt1", 4, 256, "h16", "fp32", 32, "resid"),
    R("thin_in", 48, 70, "T4_kt3_halo2", 4, 128, "h16", "h16", 0, "resid"),
    # conv_thinout_kernel: N in {16, 32} (and N <= 4 whose resident weights do not fit conv_thinout4_kernel's LDS)
    R("thinout32", 1, 1, "T2_kt3_pt1", 320, 16, "fp32", None, 0, "bias"),
    R("thinout32", 1, 33, "T3_kt1", 384, 32, "h16", "bf16", 0, "resid"),
    R("thinout32", 2, 2, "T4_kt3_halo2", 512, 16, "bf16", "fp32", 0, "resid"),
    R("thinout32", 2, 31, "T1_kt3", 64, 32, "fp32", "h16", 0, "resid"),
    R("thinout32", 7, 32, "T1_kt3_halo2", 128, 16, "h16", None, 0, "bias"),
    R("thinout32", 8, 33, "T1_kt2_head", 320, 32, "bf16", "bf16", 0, "resid"),
    R("thinout32", 15, 64, "T2_kt3_pt1", 384, 16, "fp32", "bf16", 0, "resid"),
    R("thinout32", 16, 32, "T3_kt1", 512, 32, "h16", "h16", 0, "resid"),
    R("thinout32", 17, 65, "T4_kt3_halo2", 64, 16, "h16", "fp32", 0, "resid"),
    R("thinout32", 33, 31, "T1_kt3", 128, 32, "fp32", "fp32", 0, "resid"),
    R("thinout32", 48, 70, "T1_kt3_halo2", 64, 16, "bf16", None, 0, "bias"),
    R("thinout32", 8, 33, "T4_kt3_halo2", 512, 3, "bf16", None, 0, "bias"),
    # conv_thinout4_kernel: N in {3, 4}; Cin 320 / 384 fit its resident weights with kt = 1 only
    R("thinout4", 1, 1, "T1_kt3", 128, 3, "h16", "h16", 0, "resid"),
    R("thinout4", 1, 33, "T3_kt1", 320, 4, "fp32", "bf16", 0, "resid"),
    R("thinout4", 2, 2, "T1_kt3_halo2", 64, 3, "bf16", "bf16", 0, "resid"),
    R("thinout4", 2, 31, "T3_kt1", 384, 4, "h16", None, 0, "bias"),
    R("thinout4", 7, 32, "T1_kt2_head", 128, 3, "fp32", "h16", 0, "resid"),
    R("thinout4", 8, 33, "T2_kt3_pt1", 64, 4, "bf16", "fp32", 0, "resid"),
    R("thinout4", 15, 64, "T3_kt1", 320, 3, "h16", "bf16", 0, "resid"),
    R("thinout4", 16, 32, "T4_kt3_halo2", 128, 4, "fp32", None, 0, "bias"),
    R("thinout4", 17, 65, "T3_kt1", 384, 3, "bf16", "h16", 0, "resid"),
    R("thinout4", 33, 31, "T1_kt2_head", 64, 4, "bf16", None, 0, "bias"),
    R("thinout4", 48, 70, "T4_kt3_halo2", 64, 3, "fp32", "fp32", 0, "resid"),
    # conv_sub_kernel: (kt, 2, 2) taps; sub = (single-phase launches | one quad launch, t_stride, with bias_border)
    R("conv_sub", 1, 1, "T1_kt3", 64, 128, "bf16", None, 32, "bias", sub=("phase", 1, True)),
    R("conv_sub", 1, 33, "T2_kt3_pt1", 512, 256, "fp32", None, 32, "bias", sub=("quad", 1, True)),
    R("conv_sub", 2, 2, "T1_kt2_head", 384, 512, "h16", None, 32, "bias", sub=("phase", 2, True)),
    R("conv_sub", 2, 31, "T3_kt1", 320, 384, "bf16", None, 0, "bias", sub=("quad", 2, False)),
    R("conv_sub", 7, 32, "T4_kt3_halo2", 128, 128, "fp32", None, 32, "bias", sub=("phase", 1, False)),
    R("conv_sub", 8, 33, "T1_kt3_halo2", 512, 128, "h16", None, 0, "bias", sub=("quad", 1, False)),
    R("conv_sub", 15, 64, "T1_kt2_head", 128, 256, "bf16", None, 32, "bias", sub=("phase", 2, True)),
    R("conv_sub", 16, 32, "T3_kt1", 64, 512, "fp32", None, 32, "bias", sub=("quad", 2, True)),
    R("conv_sub", 17, 65, "T2_kt3_pt1", 128, 384, "h16", None, 0, "bias", sub=("phase", 1, True)),
    R("conv_sub", 33, 31, "T1_kt3_halo2", 64, 256, "bf16", None, 32, "bias", sub=("quad", 1, False)),
    R("conv_sub", 48, 70, "T1_kt3", 64, 128, "fp32", None, 32, "bias", sub=("phase", 2, False)),
]

# conv_band (svr_set_option: tile rows per band of the frame-inner tile order of conv_halo2_kernel and conv_sub_kernel, "no effect on
# results"): H = 48 is three 16-row tile rows -- band 2 leaves a shorter last band, band 3 = tiles_y takes the frame-outermost
# branch like band 0; H = 17 is two tile rows.  (instance, H, W, temporal case, Cin, N, sub): W = 33 two tile columns, N = 256 two
# cout tiles, so that the order is a permutation of 3 x 3 x 2 x 2 tiles.
BAND_CASES = [
    ("halo16_wreg8", 48, 33, (0, 1, 2, 3)), ("halo16_wreg8", 17, 33, (1, 2)),
    ("conv_sub", 48, 33, (0, 1, 2, 3)), ("conv_sub", 17, 33, (1, 2)),
]


def band_row(inst, H, W):
    return R(inst, H, W, "T3_kt3", 128, 256, "bf16", None, 0, "bias", sub=("phase", 1, True) if inst == "conv_sub" else None)


# Plain GEMM: (M, N, K, output kind, epilogue, W_frag, kernel class).  The class of the 240- / 256-tile rows depends on the device
# (the persistent kernel wants >= 8 CUs; 256 are reported without a device, as on the MI355X).
GemmCase = collections.namedtuple("GemmCase", "M N K out epi frag cls")
GEMM_CASES = [
    GemmCase(4100, 4096, 64, "bf16", "bias", False, "gemm"),            # 17 x 16 tiles of 256 x 256 with ONE K tile (K < 128: never persistent)
    GemmCase(4100, 4096, 64, "fp32", "resid", False, "gemm"),
    GemmCase(3840, 4096, 128, "bf16", "bias", False, "gemm"),           # 240 tiles: below the routing boundary, 256 x 128 tiles
    GemmCase(3841, 4096, 128, "bf16", "bias", False, "gemm_persistent"),  # 256 tiles (ragged last row panel): gemm_w4q_kernel
    GemmCase(3841, 4096, 128, "bf16", "bias", True, "gemm_persistent"),   # ... gemm_w4r_kernel
    GemmCase(3841, 4096, 128, "fp32", "resid", True, "gemm_persistent"),
    # N % 8 != 0: not gemm_epi_lds_aligned, the direct epilogue whatever gemm_epi says (W is padded to 128 rows)
    GemmCase(257, 12, 64, "bf16", "bias", False, "gemm"), GemmCase(257, 12, 64, "fp32", "bias", False, "gemm"),
    GemmCase(257, 12, 64, "bf16", "resid", False, "gemm"), GemmCase(257, 12, 64, "fp32", "resid", False, "gemm"),
    GemmCase(300, 100, 128, "bf16", "bias", False, "gemm"), GemmCase(300, 100, 128, "fp32", "bias", False, "gemm"),
    GemmCase(300, 100, 128, "bf16", "resid", False, "gemm"), GemmCase(300, 100, 128, "fp32", "resid", False, "gemm"),
]
# rows that complete the classes of svr_gemm_kernel_class: an empty problem, and what the halo kernels do not take
EMPTY_GEMM = GemmCase(0, 256, 64, "bf16", "bias", False, "none")
GENERIC_CONV_ROWS = [
    R("generic", 8, 33, "T1_kt3", 64, 128, "bf16", None, 0, "gelu"),     # the halo geometry with tanh-GELU: the halo epilogue has none
]

# Window attention: (name, window lengths, heads, max_len passed to the launch).  (window, head) pairs 9 and 15 = 1 and 7 modulo
# the 8 XCDs; max_len overstated (512 for a longest window of 130 rows): query tiles past a window's end must write nothing.
ATTN_CASES = [
    ("pairs_9", [130, 64, 7], 3, None),
    ("pairs_15", [65, 1, 128, 33, 129], 3, None),
    ("max_len_overstated", [130, 64, 7], 3, 512),
    ("max_len_overstated_one_window", [130], 1, 512),
]


def gemm_id(c):
    return f"{c.M}x{c.N}x{c.K}-{c.out}-{c.epi}{'-wfrag' if c.frag else ''}"


# ------------------------------------------------------------------------------------------------ builders
def _rnd(shape, device, seed, scale=1.0, dtype=BF16):
    """N(0, scale^2) in storage ``dtype``, drawn on the CPU from a seed of the shape (the CPU and the GPU tests see the same data);
    device "meta": the shape only."""
    if device == "meta":
        return torch.empty(shape, dtype=dtype, device="meta")
    g = torch.Generator().manual_seed(seed + sum(shape))
    v = torch.randn(*shape, generator=g) * scale
    return ((v * H16_SCALE).to(H16) if dtype == H16 else v.to(dtype)).to(device)


def _packed(w5, packing, device, cin_pad=None, k_pad=None):
    """[ceil128(N), taps * Cin] in the packed K order (packing.pack_conv3d), optionally zero-padded to k_pad columns"""
    N, Cin, kt, kh, kw = w5.shape
    if device == "meta":
        return torch.empty(-(-N // 128) * 128, k_pad or kt * kh * kw * (cin_pad or Cin), dtype=BF16, device="meta")
    Wp = packing.pack_conv3d(w5, device, cin_pad)
    if k_pad is not None and Wp.shape[1] != k_pad:
        Wp = torch.nn.functional.pad(Wp, (0, k_pad - Wp.shape[1]))
    return Wp.contiguous()


Launch = collections.namedtuple("Launch", "w5 W kw frame0 phases")      # phases: [(py, px, w5, bias, bias_border)] the launch writes
Problem = collections.namedtuple("Problem", "x halo out_shape out_dtype launches geom")


def conv_problem(row, opsmod, packing, device="cpu", frag=None):
    """The launches of a table row: -> Problem.  A 3 x 3 row is one launch into [To, H, W, N]; a conv_sub row is four single-phase
    launches (or one quad launch) per temporal phase into the dense [To * t_stride, 2 H, 2 W, N] tensor, Launch.frame0 = the
    launch's first output frame.  Launch.kw: the keywords of HipOps.gemm / local_error.gemm_reference (without gn_groups).
    ``frag(kind, W, kt, Cin, N)``: the fragment-ordered copy ("conv33" / "conv22") for the instances that want one."""
    T, kt, pt, hf = temporal(row.tk)
    inst = INSTANCES.get(row.inst, dict(frag=None))
    H, W, Cin, N = row.H, row.W, row.Cin, row.N
    To = T + pt - kt + 1
    x = _rnd((T, H, W, Cin), device, 0)
    if Cin == 4 and device != "meta":
        x[..., 3] = 0                                                              # (RGB padded to four channels)
    halo = _rnd((hf, H, W, Cin), device, 9) if hf else None
    if halo is not None and Cin == 4 and device != "meta":
        halo[..., 3] = 0
    out_dt = STORE_KINDS[row.out]
    wide = dict(out_f32=True) if row.out != "bf16" else {}
    if row.sub is None:
        cw = 3 if Cin == 4 else Cin
        w5 = _rnd((N, cw, kt, 3, 3), device, 2, scale=1.0 / math.sqrt(cw * kt * 9))
        Wp = _packed(w5, packing, device, 4 if Cin == 4 else None, 128 if Cin == 4 else None)
        bias = _rnd((N,), device, 3, dtype=F32)
        geom = opsmod.Conv3dGeom(T, H, W, Cin, To, H, W, (kt, 3, 3), (1, 1, 1), (pt, 1, 1), halo)
        kw = dict(N=N, K=Wp.shape[1], bias=bias, conv=geom, epilogue=EPILOGUES[row.epi], ldc=N, **wide)
        if row.resid:
            kw.update(resid=_rnd((To, H, W, N), device, 11, dtype=STORE_KINDS[row.resid]), ldr=N)
        if inst["frag"]:
            kw["W_frag"] = frag(inst["frag"], Wp, kt, Cin, N)
        return Problem(x, halo, (To, H, W, N), out_dt, [Launch(w5, Wp, kw, 0, [(None, None, w5, bias, None)])], geom)
    mode, ts, with_bb = row.sub
    launches = []
    for tz in range(ts):
        quad, phases = [], []
        for ph, (py, px) in enumerate(PHASES):
            w5 = _rnd((N, Cin, kt, 2, 2), device, 20 + ph + 7 * tz, scale=1.0 / math.sqrt(Cin * 4 * kt))
            Wp = _packed(w5, packing, device)
            bias = _rnd((N,), device, 30 + ph, dtype=F32)
            bb = _rnd((3, N), device, 40 + ph, dtype=F32) if with_bb else None
            Wf = frag("conv22", Wp, kt, Cin, N)
            phases.append((py, px, w5, bias, bb))
            quad.append((py, px, Wp, bias, bb, Wf))
            if mode == "phase":
                geom = opsmod.Conv3dGeom(T, H, W, Cin, To, H, W, (kt, 2, 2), (1, 1, 1), (pt, 1 - py, 1 - px), halo)
                kw = dict(N=N, K=Wp.shape[1], bias=bias, conv=geom, phase=opsmod.PhaseScatter(py, px, bb, ts), W_frag=Wf, **wide)
                launches.append(Launch(w5, Wp, kw, tz, [phases[-1]]))
        if mode == "quad":
            q0 = quad[0]
            geom = opsmod.Conv3dGeom(T, H, W, Cin, To, H, W, (kt, 2, 2), (1, 1, 1), (pt, 1, 1), halo)
            kw = dict(N=N, K=q0[2].shape[1], bias=q0[3], conv=geom, W_frag=q0[5], phase=opsmod.PhaseScatter(0, 0, q0[4], ts, quad=quad),
                      **wide)
            launches.append(Launch(None, q0[2], kw, tz, phases))
    geom = opsmod.Conv3dGeom(T, H, W, Cin, To, H, W, (kt, 2, 2), (1, 1, 1), (pt, 1, 1), halo)
    return Problem(x, halo, (To * ts, 2 * H, 2 * W, N), out_dt, launches, geom)


def gemm_problem(case, packing, device="cpu", frag=None):
    """-> (A, W, keywords of HipOps.gemm, output shape, output dtype) of a GEMM_CASES row; "resid": gate * (acc + bias) + residual of
    the output's kind.  ``frag(W)``: the fragment-ordered copy for the persistent kernel."""
    M, N, K = case.M, case.N, case.K
    A = _rnd((max(M, 1), K), device, 0)
    if device == "meta":
        W = torch.empty(-(-N // 128) * 128, K, dtype=BF16, device="meta")
    else:
        W = packing.pack_matrix(_rnd((N, K), "cpu", 1, scale=1.0 / math.sqrt(K)), device)
    out_dt = STORE_KINDS[case.out]
    kw = dict(N=N, K=K, M=M, bias=_rnd((N,), device, 3, dtype=F32), epilogue=EPILOGUES[case.epi])
    if case.out != "bf16":
        kw["out_f32"] = True
    if case.epi == "resid":
        kw.update(gate=_rnd((N,), device, 4, dtype=F32), resid=_rnd((max(M, 1), N), device, 5, dtype=out_dt))
    if case.frag:
        kw["W_frag"] = frag(W)
    return A, W, kw, (max(M, 1), N), out_dt
