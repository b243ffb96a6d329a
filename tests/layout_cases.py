"""TEST INFRASTRUCTURE: strided and offset operands -- the layout contract of include/seedvr2_hip.h ("Operand layouts") as one
table, shared by the CPU test (tests/test_layout_cases.py: every row, filled into the C ABI with fake pointers at the row's
alignment, is served by the kernel class it names or refused with a message that names the operand) and the GPU sweep
(tests/test_gpu_layouts.py: every accepted row launched on canvases that can tell a stray access).

An operand is a column window ``canvas[:, c0:c0 + n]`` of a wider 2-D canvas whose first element sits ``off`` bytes behind a
256-byte aligned address:

    Place(c0, extra, off)      pitch = n + extra elements (c0 <= extra), base = aligned + off + c0 * element size

A row enters an accepted table only once reading the kernel that serves it shows every vector access naturally aligned and in
range (the header's table says which widths each kernel uses); everything else is a refused row and is never launched.

Why these rows.  The library picks kernels by pointer alignment and pitch: gemm_epi_lds_aligned() (C % 16, resid % 16, ldc % 8,
ldr % 8) chooses between the row-contiguous epilogue (16-byte stores) and the direct one (8-byte), gemm_w4_eligible() wants the
former, conv_halo_eligible() / conv_thin_eligible() want 16-byte output rows, conv_thinout4_kernel has a dense (ldc == N) and a
strided store path, conv_sub_eligible() wants ldc == N, attn_dispatch() wants 16-byte output rows for the window kernel.  Every
other kernel test passes dense operands at an allocator's alignment, so only one side of each of these decisions ever ran.

  (a) aligned strided: 16-byte aligned windows with a gap -- same class, same bits as the dense launch
  (b) 8-byte aligned only: the direct epilogue, the persistent kernel ineligible -- same bits as the dense launch under gemm_w4 = 0
      (tests/test_gpu_kernels.py::test_gemm_epilogue_paths_bit_identical holds the two epilogues to bit identity)
  (c) every epilogue and store kind under (a) and (b) placements
"""
import collections
import math

import torch

import geometry_cases as gc
from geometry_cases import BF16, F32, STORE_KINDS, _rnd
from ops_reference import H16, EPI_BIAS, EPI_BIAS_SILU, EPI_BIAS_GELU, EPI_RESID_GATE, EPI_SWIGLU

Place = collections.namedtuple("Place", "c0 extra off")
DENSE = Place(0, 0, 0)
ALIGN = 256
ELEM = {BF16: 2, H16: 2, F32: 4, torch.float64: 8, torch.uint8: 1}
EPILOGUES = {"bias": EPI_BIAS, "silu": EPI_BIAS_SILU, "gelu": EPI_BIAS_GELU, "resid": EPI_RESID_GATE, "swiglu": EPI_SWIGLU}


def P(c0=0, extra=0, off=0):
    assert 0 <= c0 <= extra or (c0 == 0 and extra < 0), (c0, extra)      # (extra < 0: a pitch short of its extent -- refused rows only)
    return Place(c0, extra, off)


def flat_elems(rows, n, place, dtype):
    """elements of the flat buffer that holds ``rows`` rows of the canvas behind ``off`` bytes"""
    assert place.off % ELEM[dtype] == 0
    return place.off // ELEM[dtype] + max(rows, 1) * max(n + place.extra, n if place.extra < 0 else 1)


def window(flat, rows, n, place):
    """(canvas [rows, pitch], window [rows, n]) inside the 1-D buffer ``flat`` (flat_elems elements, its first element 256-byte
    aligned); a pitch short of its extent (refused rows) is described by as_strided."""
    e0 = place.off // ELEM[flat.dtype]
    ld = n + place.extra
    if place.extra < 0:
        return None, flat.as_strided((rows, n), (ld, 1), e0)
    canvas = flat[e0:e0 + rows * ld].view(rows, ld)
    return canvas, canvas[:, place.c0:place.c0 + n]


def fake_ptr(t):
    """CPU routing: a 256-byte aligned fake allocation + the window's own offset"""
    return 0x10000000 + t.storage_offset() * t.element_size()


# ------------------------------------------------------------------------------------------------ plain GEMM
# resid: None | "bf16" | "fp32" | "h16" (a separate tensor of that kind) | "inplace" (aliases C: same window, ldr == ldc)
GemmLayout = collections.namedtuple("GemmLayout", "tag M N K out epi resid frag A C R cls")
S_NARROW, S_WIDE, S_PERS, S_ODD = (300, 384, 128), (4100, 4096, 64), (3841, 4096, 128), (257, 12, 64)


def G(tag, shape, out, epi, resid, frag, A, C, R, cls):
    return GemmLayout(tag, *shape, out, epi, resid, frag, A, C, R, cls)


def gemm_id(r):
    return f"{r.tag}-{r.M}x{r.N}x{r.K}-{r.out}-{r.epi}{'_' + r.resid if r.resid else ''}{'-wfrag' if r.frag else ''}"


def out_cols(r):
    return r.N // 2 if r.epi == "swiglu" else r.N


A_STR, C_STR8, C_STR72, R_STR = P(8, 64), P(8, 8), P(8, 72), P(16, 24)        # (a): 16-byte aligned windows, ldr != ldc
C_P4, C_OFF8, R_OFF8 = P(0, 4), P(0, 0, 8), P(0, 4, 8)                        # (b): 8-byte aligned only
GEMM_ROWS = []
for _shape, _frag, _cls in ((S_NARROW, False, "gemm"), (S_WIDE, False, "gemm"), (S_PERS, False, "gemm_persistent"),
                            (S_PERS, True, "gemm_persistent")):
    GEMM_ROWS += [
        G("a-ldc8", _shape, "bf16", "bias", None, _frag, A_STR, C_STR8, None, _cls),
        G("a-ldc72-resid", _shape, "bf16", "resid", "bf16", _frag, A_STR, C_STR72, R_STR, _cls),
        G("a-inplace", _shape, "bf16", "resid", "inplace", _frag, A_STR, C_STR8, C_STR8, _cls),
        G("b-ldc4", _shape, "bf16", "bias", None, _frag, DENSE, C_P4, None, "gemm"),
    ]
    if not _frag:
        GEMM_ROWS += [
            G("b-c-off8", _shape, "bf16", "bias", None, _frag, DENSE, C_OFF8, None, "gemm"),
            G("b-resid-off8", _shape, "bf16", "resid", "bf16", _frag, DENSE, DENSE, R_OFF8, "gemm"),
        ]
GEMM_ROWS += [
    # (c) epilogues and store kinds: the 256 x 128 tile's compact epilogue instances, (a) placement ...
    G("c-a", S_NARROW, "fp32", "bias", None, False, A_STR, C_STR72, None, "gemm"),
    G("c-a", S_NARROW, "h16", "bias", None, False, A_STR, C_STR72, None, "gemm"),
    G("c-a", S_NARROW, "bf16", "gelu", None, False, A_STR, C_STR72, None, "gemm"),
    G("c-a", S_NARROW, "bf16", "silu", None, False, A_STR, C_STR72, None, "gemm"),
    G("c-a", S_NARROW, "bf16", "swiglu", None, False, A_STR, C_STR8, None, "gemm"),
    G("c-a", S_NARROW, "fp32", "swiglu", None, False, A_STR, C_STR72, None, "gemm"),
    G("c-a", S_NARROW, "fp32", "resid", "fp32", False, A_STR, C_STR72, R_STR, "gemm"),
    G("c-a", S_NARROW, "h16", "resid", "h16", False, A_STR, C_STR72, R_STR, "gemm"),
    G("c-a", S_NARROW, "bf16", "resid", "fp32", False, A_STR, C_STR72, R_STR, "gemm"),
    G("c-a", S_NARROW, "h16", "resid", "bf16", False, A_STR, C_STR72, R_STR, "gemm"),
    G("c-a", S_NARROW, "bf16", "resid", "h16", False, A_STR, C_STR72, R_STR, "gemm"),
    # ... and (b) placement: the direct epilogue's quads (fp32 output: 16-byte quads, so C % 16 with ldc % 8 != 0)
    G("c-b", S_NARROW, "fp32", "bias", None, False, DENSE, P(4, 4), None, "gemm"),
    G("c-b", S_NARROW, "h16", "bias", None, False, DENSE, P(4, 4), None, "gemm"),
    G("c-b", S_NARROW, "bf16", "gelu", None, False, DENSE, P(4, 4), None, "gemm"),
    G("c-b", S_NARROW, "bf16", "swiglu", None, False, DENSE, P(4, 4), None, "gemm"),
    G("c-b", S_NARROW, "fp32", "swiglu", None, False, DENSE, P(4, 4), None, "gemm"),
    G("c-b", S_NARROW, "bf16", "resid", "bf16", False, DENSE, P(4, 4), P(4, 12), "gemm"),
    G("c-b", S_NARROW, "fp32", "resid", "fp32", False, DENSE, P(4, 4), P(1, 3), "gemm"),      # (fp32 / h16 residuals: element loads)
    G("c-b", S_NARROW, "h16", "resid", "h16", False, DENSE, P(4, 4), P(1, 3), "gemm"),
    G("c-b", S_NARROW, "bf16", "resid", "inplace", False, DENSE, P(4, 4), P(4, 4), "gemm"),
    # the 256 x 256 tile: h16 tensors take the run-time epilogue there
    G("c-a", S_WIDE, "h16", "bias", None, False, A_STR, C_STR72, None, "gemm"),
    G("c-a", S_WIDE, "h16", "resid", "h16", False, A_STR, C_STR72, R_STR, "gemm"),
    G("c-a", S_WIDE, "fp32", "resid", "fp32", False, A_STR, C_STR8, R_STR, "gemm"),
    # the persistent kernel: its compact instances, the two h16 forms of the NaDiT's residual stream included
    G("c-a", S_PERS, "fp32", "resid", "fp32", True, A_STR, C_STR72, R_STR, "gemm_persistent"),
    G("c-a", S_PERS, "h16", "bias", None, True, A_STR, C_STR72, None, "gemm_persistent"),
    G("c-a", S_PERS, "h16", "resid", "h16", True, A_STR, C_STR72, R_STR, "gemm_persistent"),
    G("c-a", S_PERS, "h16", "resid", "inplace", False, A_STR, C_STR8, C_STR8, "gemm_persistent"),
    G("c-a", S_PERS, "bf16", "gelu", None, False, A_STR, C_STR8, None, "gemm_persistent"),
    G("c-a", S_PERS, "bf16", "swiglu", None, True, A_STR, C_STR72, None, "gemm_persistent"),
    G("c-a", S_PERS, "h16", "resid", "bf16", False, A_STR, C_STR8, R_STR, "gemm"),            # (an h16 form the persistent kernel has no instance for)
    # N % 8 != 0 (W padded to 128 rows): the direct epilogue's whole quads and its element tail, ldc = 16 and 20
    G("c-n12-ldc16", S_ODD, "bf16", "bias", None, False, A_STR, P(4, 4), None, "gemm"),
    G("c-n12-ldc20", S_ODD, "bf16", "bias", None, False, A_STR, P(4, 8), None, "gemm"),
    G("c-n12-ldc16", S_ODD, "fp32", "resid", "fp32", False, A_STR, P(4, 4), P(1, 5), "gemm"),
    G("c-n12-ldc20", S_ODD, "fp32", "resid", "fp32", False, A_STR, P(4, 8), P(0, 4), "gemm"),
    G("c-n12-ldc20", S_ODD, "bf16", "resid", "bf16", False, A_STR, P(8, 8), P(4, 4), "gemm"),
]

# Refused: (row, the operand the message must name).  CPU only, never launched.
W_OFF = "W_off8"      # marker: the weight pointer 8 bytes off
GEMM_REFUSED = [
    (G("lda<K", S_NARROW, "bf16", "bias", None, False, P(0, -8), DENSE, None, "refused"), "lda"),
    (G("lda=0", S_NARROW, "bf16", "bias", None, False, P(0, -128), DENSE, None, "refused"), "lda"),
    (G("ldc<N", S_NARROW, "bf16", "bias", None, False, DENSE, P(0, -8), None, "refused"), "ldc"),
    (G("ldc<N/2", S_NARROW, "bf16", "swiglu", None, False, DENSE, P(0, -8), None, "refused"), "ldc"),
    (G("ldr<N", S_NARROW, "bf16", "resid", "bf16", False, DENSE, DENSE, P(0, -8), "refused"), "ldr"),
    (G("lda%8", S_NARROW, "bf16", "bias", None, False, P(0, 4), DENSE, None, "refused"), "lda"),
    (G("A-off8", S_NARROW, "bf16", "bias", None, False, P(0, 0, 8), DENSE, None, "refused"), " A "),
    (G("A-c0-4", S_PERS, "bf16", "bias", None, True, P(4, 8), DENSE, None, "refused"), " A "),
    (G(W_OFF, S_NARROW, "bf16", "bias", None, False, DENSE, DENSE, None, "refused"), " W "),
    (G("C-off4", S_NARROW, "bf16", "bias", None, False, DENSE, P(0, 0, 4), None, "refused"), " C "),
    (G("C-off2", S_PERS, "bf16", "bias", None, False, DENSE, P(1, 1), None, "refused"), " C "),
    (G("C-fp32-off8", S_NARROW, "fp32", "bias", None, False, DENSE, P(0, 0, 8), None, "refused"), " C "),
    (G("ldc%4", S_NARROW, "bf16", "bias", None, False, DENSE, P(0, 2), None, "refused"), "ldc"),
    (G("ldc%4-odd", S_ODD, "bf16", "bias", None, False, DENSE, P(0, 1), None, "refused"), "ldc"),
    (G("resid-off4", S_NARROW, "bf16", "resid", "bf16", False, DENSE, DENSE, P(0, 0, 4), "refused"), "resid"),
    (G("ldr%4", S_NARROW, "bf16", "resid", "bf16", False, DENSE, DENSE, P(0, 2), "refused"), "ldr"),
]


def gemm_operands(r, packing, device="cpu", frag=None):
    """The DENSE operands of a row -> dict(A, W, W_frag, bias, gate, resid, kw): kw = the keywords of HipOps.gemm /
    local_error.gemm_reference for the dense launch (resid = the residual as it is BEFORE the launch, in-place rows included)."""
    M, N, K = r.M, r.N, r.K
    A = _rnd((M, K), device, 0)
    if device == "meta":
        W = torch.empty(-(-N // 128) * 128, K, dtype=BF16, device="meta")
    elif r.epi == "swiglu":
        W = packing.pack_swiglu(_rnd((N // 2, K), "cpu", 7, scale=1.0 / math.sqrt(K)), _rnd((N // 2, K), "cpu", 8, scale=1.0 / math.sqrt(K)), device)
    else:
        W = packing.pack_matrix(_rnd((N, K), "cpu", 1, scale=1.0 / math.sqrt(K)), device)
    kw = dict(N=N, K=K, M=M, epilogue=EPILOGUES[r.epi])
    if r.epi != "swiglu":
        kw["bias"] = _rnd((N,), device, 3, dtype=F32)
    if r.out != "bf16":
        kw["out_f32"] = True
    if r.epi == "resid":
        rk = r.out if r.resid == "inplace" else r.resid
        kw.update(gate=_rnd((N,), device, 4, dtype=F32), resid=_rnd((M, N), device, 5, dtype=STORE_KINDS[rk]))
    if r.frag:
        kw["W_frag"] = frag(W)
    return A, W, kw


# ------------------------------------------------------------------------------------------------ conv family
# row: a geometry_cases.ConvRow (H, W, temporal case, Cin, N, kinds, gn, epilogue) + where C and the residual sit, the class
# expected, the options of the launch, and ``taps``: 3 (3 x 3 spatial) | 2 ((kt, 2, 2) taps without phase scatter).
ConvLayout = collections.namedtuple("ConvLayout", "tag row C R cls options taps twin_options")
FRAME = (21, 70)          # (tests/test_gpu_wide_trunk.py's small frame: two patch rows, three patch columns, both ragged)


def CR(inst, Cin, N, out, resid, gn, epi, tk="T3_kt3"):
    return gc.R(inst, FRAME[0], FRAME[1], tk, Cin, N, out, resid, gn, epi)


def CL(tag, row, C, R, cls, options=None, taps=3, twin_options=None):
    inst = gc.INSTANCES.get(row.inst, dict(options={}))
    opts = {**inst["options"], **(options or {})}
    return ConvLayout(tag, row, C, R, cls, opts, taps, {**opts, **(twin_options or {})})


def conv_id(c):
    return f"{c.tag}-{gc.row_id(c.row)}"


CONV_ROWS = [
    # the halo kernel, register-streamed and LDS-staged weights: ldc = N + 128, a separate residual with ldr = N + 64, fused statistics
    CL("halo-ldc128", CR("halo16_wreg8", 128, 128, "bf16", "bf16", 32, "resid"), P(64, 128), P(8, 64), "conv_halo"),
    CL("halo-ldc128", CR("halo16_lds", 128, 128, "bf16", "bf16", 32, "resid"), P(64, 128), P(8, 64), "conv_halo"),
    CL("halo-ldc128", CR("halo8_wreg4", 64, 256, "h16", "h16", 32, "resid"), P(8, 128), P(8, 64), "conv_halo"),
    CL("halo-ldc128", CR("halo16_lds", 64, 128, "fp32", "fp32", 32, "resid"), P(8, 128), P(8, 64), "conv_halo"),
    CL("halo-ldc8", CR("halo16_wreg8", 64, 128, "bf16", None, 0, "bias", tk="T1_kt3_halo2"), P(8, 8), None, "conv_halo"),
    # an 8-byte aligned output leaves the halo kernel (16-byte stores) for the generic one's direct epilogue; twin: conv_impl 1
    CL("halo-to-generic-ldc4", CR("halo16_lds", 64, 128, "bf16", None, 0, "bias"), P(4, 4), None, "conv_generic", twin_options={"conv_impl": 1}),
    CL("halo-to-generic-resid-off8", CR("halo16_wreg8", 64, 128, "bf16", "bf16", 0, "resid"), DENSE, P(0, 4, 8), "conv_generic",
       twin_options={"conv_impl": 1}),
    # the thin-input kernel
    CL("thin-in-ldc8", CR("thin_in", 4, 128, "bf16", None, 32, "bias"), P(8, 8), None, "conv_thin_in"),
    CL("thin-in-ldc72", CR("thin_in", 4, 256, "h16", "bf16", 0, "resid", tk="T1_kt3_halo2"), P(8, 72), P(16, 24), "conv_thin_in"),
    # thin output, N = 3 with ldc = 8: conv_thinout4_kernel's strided path, and the 32-cout kernel under conv_thinout4 = 0
    CL("thinout4-ldc8", CR("thinout4", 128, 3, "bf16", None, 0, "bias"), P(0, 5), None, "conv_thinout"),
    CL("thinout4-ldc8-c0", CR("thinout4", 64, 3, "fp32", None, 0, "bias", tk="T1_kt3_halo2"), P(5, 5), None, "conv_thinout"),
    CL("thinout32-ldc8", CR("thinout4", 128, 3, "bf16", None, 0, "bias"), P(0, 5), None, "conv_thinout", options={"conv_thinout4": 0}),
    CL("thinout32-ldc8-c0", CR("thinout4", 64, 3, "h16", "h16", 0, "resid", tk="T1_kt3_halo2"), P(5, 5), P(1, 5), "conv_thinout",
       options={"conv_thinout4": 0}),
    CL("thinout32-ldc20", CR("thinout32", 64, 16, "bf16", "bf16", 0, "resid"), P(4, 4), P(4, 8), "conv_thinout"),
    # the generic kernel: the halo geometry with tanh-GELU, row-contiguous (ldc % 8 == 0) and direct (ldc % 4 == 0) epilogues
    CL("generic-ldc8", CR("generic", 64, 128, "bf16", None, 0, "gelu", tk="T1_kt3"), P(8, 8), None, "conv_generic"),
    CL("generic-ldc4", CR("generic", 64, 128, "bf16", None, 0, "gelu", tk="T1_kt3"), P(4, 4), None, "conv_generic"),
    # a sub-pixel geometry ((kt, 2, 2) taps, fragment-ordered weights) without phase scatter: ldc != N leaves conv_sub_kernel (dense
    # stores at m * N + n) for the generic class; twin: conv_sub 0
    CL("sub-to-generic-ldc8", CR("conv_sub", 64, 128, "bf16", None, 0, "bias"), P(8, 8), None, "conv_generic", taps=2, twin_options={"conv_sub": 0}),
]

CONV_REFUSED = [
    (CL("thin-in-C-off8", CR("thin_in", 4, 128, "bf16", None, 0, "bias"), P(0, 0, 8), None, "refused"), " C"),
    (CL("thin-in-ldc4", CR("thin_in", 4, 128, "bf16", None, 0, "bias"), P(0, 4), None, "refused"), "ldc"),
    (CL("halo-C-off4", CR("halo16_lds", 64, 128, "bf16", None, 0, "bias"), P(0, 0, 4), None, "refused"), " C "),
    (CL("halo-ldc<N", CR("halo16_lds", 64, 128, "bf16", None, 0, "bias"), P(0, -8), None, "refused"), "ldc"),
    (CL("halo-ldr<N", CR("halo16_lds", 64, 128, "bf16", "bf16", 0, "resid"), DENSE, P(0, -8), "refused"), "ldr"),
    (CL("thinout-ldc18", CR("thinout32", 64, 16, "bf16", None, 0, "bias"), P(0, 2), None, "refused"), "ldc"),
    (CL("thinout-ldc<N", CR("thinout4", 64, 3, "bf16", None, 0, "bias"), P(0, -1), None, "refused"), "ldc"),
    (CL("A-off8", CR("halo16_lds", 64, 128, "bf16", None, 0, "bias"), DENSE, None, "refused", options={"A_off": 8}), " A "),
    (CL("halo-off8", CR("halo16_lds", 64, 128, "bf16", None, 0, "bias", tk="T1_kt3_halo2"), DENSE, None, "refused", options={"halo_off": 8}), "halo"),
    (CL("zeros-off8", CR("halo16_lds", 64, 128, "bf16", None, 0, "bias"), DENSE, None, "refused", options={"zeros_off": 8}), "zeros"),
]
POINTER_KNOBS = ("A_off", "halo_off", "zeros_off")      # (refused rows only: not library options)


def conv_launch(c, opsmod, packing, device="cpu", frag=None):
    """-> (Problem, Launch) of a conv row: the DENSE problem of geometry_cases (one launch; kw carries ldc = N, the dense
    residual and ldr = N).  taps 2: the (kt, 2, 2)-tap conv of a sub-pixel upsampler's phase (1, 1) as a plain same-size conv."""
    row = c.row
    if c.taps == 3:
        p = gc.conv_problem(row, opsmod, packing, device, frag=frag)
        return p, p.launches[0]
    T, kt, pt, hf = gc.temporal(row.tk)
    H, W, Cin, N = row.H, row.W, row.Cin, row.N
    To = T + pt - kt + 1
    x = _rnd((T, H, W, Cin), device, 0)
    w5 = _rnd((N, Cin, kt, 2, 2), device, 20, scale=1.0 / math.sqrt(Cin * 4 * kt))
    Wp = gc._packed(w5, packing, device)
    bias = _rnd((N,), device, 30, dtype=F32)
    geom = opsmod.Conv3dGeom(T, H, W, Cin, To, H, W, (kt, 2, 2), (1, 1, 1), (pt, 1, 1), None)
    kw = dict(N=N, K=Wp.shape[1], bias=bias, conv=geom, epilogue=EPILOGUES[row.epi], ldc=N, W_frag=frag("conv22", Wp, kt, Cin, N))
    if row.out != "bf16":
        kw["out_f32"] = True
    ln = gc.Launch(w5, Wp, kw, 0, [(None, None, w5, bias, None)])
    return gc.Problem(x, None, (To, H, W, N), STORE_KINDS[row.out], [ln], geom), ln


# ------------------------------------------------------------------------------------------------ window attention
# (name, window lengths, heads, head_dim, max_len, qkv placement, out placement, attn_impl of the dense twin or None = the row's own)
AttnLayout = collections.namedtuple("AttnLayout", "name lens heads D max_len Q O twin_impl")
ATTN_ROWS = [AttnLayout(f"{n}-ldq8", lens, heads, 128, ml, P(8, 8), P(8, 8), None) for n, lens, heads, ml in gc.ATTN_CASES]
ATTN_ROWS += [
    AttnLayout("pairs_9-ldq264", [130, 64, 7], 3, 128, None, P(128, 264), P(0, 8), None),
    AttnLayout("pairs_15-ldq264", [65, 1, 128, 33, 129], 3, 128, None, P(264, 264), P(8, 8), None),
    # output rows that are only 8-byte aligned: the window kernel's 16-byte stores do not apply, the first kernel (8-byte stores)
    # takes the launch whatever attn_impl says; twin: attn_impl 1
    AttnLayout("pairs_9-out8", [130, 64, 7], 3, 128, None, P(8, 8), P(4, 4), 1),
    AttnLayout("d512-ldq8", [130, 64, 7], 1, 512, None, P(8, 8), P(8, 8), None),
    AttnLayout("d512-ldq264-out4", [65, 1, 128, 33], 1, 512, None, P(64, 264), P(4, 4), None),
]
# (name, heads, D, ld_qkv, qkv byte offset, ld_out, out byte offset, the operand named)
ATTN_REFUSED = [
    ("ld_qkv%8", 3, 128, 3 * 3 * 128 + 4, 0, 3 * 128, 0, "ld_qkv"),
    ("qkv-off8", 3, 128, 3 * 3 * 128 + 8, 8, 3 * 128, 0, "qkv"),
    ("ld_qkv<extent", 3, 128, 3 * 3 * 128 - 8, 0, 3 * 128, 0, "ld_qkv"),
    ("ld_out<extent", 3, 128, 3 * 3 * 128, 0, 3 * 128 - 8, 0, "ld_out"),
    ("out-off4", 3, 128, 3 * 3 * 128, 0, 3 * 128, 4, "out"),
    ("ld_out%4", 3, 128, 3 * 3 * 128, 0, 3 * 128 + 2, 0, "ld_out"),
    ("d512-qkv-off8", 1, 512, 3 * 512, 8, 512, 0, "qkv"),
    ("d512-ld_out%4", 1, 512, 3 * 512, 0, 512 + 2, 0, "ld_out"),
]

# ------------------------------------------------------------------------------------------------ side kernels
# svr_softmax_rows: (cols, rows); 256-thread form up to 16384 columns, 1024-thread form above.  ld_s = cols + 4, ld_p = cols + 12.
SOFTMAX_ROWS = [(260, 7), (16384, 3), (16388, 3), (65536, 2)]
SOFTMAX_S, SOFTMAX_P = P(4, 4), P(4, 12)
# (name, cols, ld_s, S byte offset, ld_p, P byte offset, operand named)
SOFTMAX_REFUSED = [
    ("S-off8", 260, 264, 8, 264, 0, " S "), ("P-off4", 260, 264, 0, 264, 4, " P "),
    ("ld_s<cols", 260, 256, 0, 264, 0, "ld_s"), ("ld_p<cols", 260, 264, 0, 256, 0, "ld_p"),
    ("ld_s%4", 260, 262, 0, 264, 0, "leading dimensions"),
]
RMSNORM_REFUSED = [("x-off8", 8, 0, " x "), ("y-off8", 0, 8, " y ")]
# svr_unpatchify_euler: element accesses only -- ldp wider than 4 * C behind a base offset of an odd number of elements
UNPATCHIFY = dict(T=2, H=6, W=10, C=16, pred=P(3, 13))
# svr_alpha_*: an RGBA view (ld_px = 4) against the contiguous RGB copy (ld_px = 3)
ALPHA = dict(T=2, H=24, W=40, scale=2)
