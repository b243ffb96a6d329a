"""The exact refusal message of the engine's own entry points, svr_mfma_calibrate to svr_affine_slice (csrc/svr_api.hip), checked
without a GPU: the sibling of tests/test_refusal_messages.py, whose helpers it shares.

One row per refusing branch, rows with two faults that fix which one is reported first (several functions check their layout before
emptiness on purpose), and the empty calls: those return 0 and leave svr_last_error() as it was (``None`` in the table).  No row
reaches a launch -- every argument is validated on the host first, so a host buffer stands in for device memory.  svr_gemm_bf16
takes its svr_gemm_args from ops.fill_gemm_args on shape-only tensors with fake pointers; a row is a base launch plus the fields it
overwrites, and svr_gemm_kernel_class has to leave the same words for the same arguments.  The expected strings were recorded from
the library as it stood before these entry points were moved onto the refusal path of the rest of the file; the comparison is exact.
svr_device_info is not here: its result depends on the machine.
"""
import torch

from conftest import sub
from test_refusal_messages import Ptr, call, p  # noqa: F401 (Ptr: the type ``call`` recognises)

PLANTED = "svr_set_option: unknown key"


def G(**fields):
    """svr_conv_geom of a 1x1x1 conv over [1, 4, 4, 64] with ``fields`` overwritten (svr_im2col_causal reads it on the host)"""
    g = sub("hip_lib").ConvGeom()
    base = dict(enabled=1, T=1, H=4, W=4, Cin=64, To=1, Ho=4, Wo=4, kt=1, kh=1, kw=1, st=1, sh=1, sw=1)
    for k, v in {**base, **fields}.items():
        setattr(g, k, v)
    return g


# (function, arguments, message left in svr_last_error(); None: an empty call -> 0, the message before it still standing)

ROWS = [
    ('svr_mfma_calibrate', (None, 1, None, None), 'svr_mfma_calibrate: workspace of svr_mfma_calibrate_workspace_bytes() and iters > 0'),
    ('svr_mfma_calibrate', (p, 0, None, None), 'svr_mfma_calibrate: workspace of svr_mfma_calibrate_workspace_bytes() and iters > 0'),
    ('svr_mfma_calibrate', (p, -1, p, None), 'svr_mfma_calibrate: workspace of svr_mfma_calibrate_workspace_bytes() and iters > 0'),
    ('svr_mfma_calibrate', (None, 0, None, None), 'svr_mfma_calibrate: workspace of svr_mfma_calibrate_workspace_bytes() and iters > 0'),
    ('svr_set_option', (None, 0), 'svr_set_option: null key'),
    ('svr_set_option', (b'no_such_key', 0), 'svr_set_option: unknown key'),
    ('svr_set_option', (b'', 1), 'svr_set_option: unknown key'),
    ('svr_set_option', (b'gemm_w4r', 2), 'svr_set_option: gemm_w4r is 0 or 1'),
    ('svr_set_option', (b'gemm_w4r', -1), 'svr_set_option: gemm_w4r is 0 or 1'),
    ('svr_set_option', (b'png_passes', 0), 'svr_set_option: png_passes is 1, 2 or 3'),
    ('svr_set_option', (b'png_passes', 4), 'svr_set_option: png_passes is 1, 2 or 3'),
    ('svr_set_option', (b'rank_launches', 0), 'svr_set_option: rank_launches is 1, 2 or 3'),
    ('svr_set_option', (b'rank_launches', 4), 'svr_set_option: rank_launches is 1, 2 or 3'),
    ('svr_gemm_bf16', (None, None), 'svr_gemm_bf16: null args'),
    ('svr_gemm_kernel_class', (None,), 'svr_gemm_kernel_class: null args'),
    ('svr_groupnorm_reduce', (p, p, 1, 1, 0, None), 'svr_groupnorm_reduce: 1..65535 groups'),
    ('svr_groupnorm_reduce', (p, p, 1, 1, 65536, None), 'svr_groupnorm_reduce: 1..65535 groups'),
    ('svr_groupnorm_reduce', (None, p, 1, 1, 1, None), 'svr_groupnorm_reduce: null pointer'),
    ('svr_groupnorm_reduce', (p, None, 1, 1, 1, None), 'svr_groupnorm_reduce: null pointer'),
    ('svr_groupnorm_reduce', (None, p, 1, 1, 0, None), 'svr_groupnorm_reduce: 1..65535 groups'),
    ('svr_groupnorm_reduce', (p, p, 0, 1, 1, None), None),
    ('svr_groupnorm_reduce', (p, p, 1, 0, 1, None), None),
    ('svr_groupnorm_reduce', (None, None, 0, 1, 0, None), None),
    ('svr_rmsnorm_mod', (p + 8, p, 4, 64, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: x and y must be 16-byte aligned (rows are read and written in 16-byte units)'),
    ('svr_rmsnorm_mod', (p, p + 8, 4, 64, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: x and y must be 16-byte aligned (rows are read and written in 16-byte units)'),
    ('svr_rmsnorm_mod', (p + 8, p, 0, 64, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: x and y must be 16-byte aligned (rows are read and written in 16-byte units)'),
    ('svr_rmsnorm_mod', (p, p + 2, -1, 64, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: x and y must be 16-byte aligned (rows are read and written in 16-byte units)'),
    ('svr_rmsnorm_mod', (p, p, 4, 0, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: dim must be a multiple of 8 and <= 4096'),
    ('svr_rmsnorm_mod', (p, p, 4, 12, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: dim must be a multiple of 8 and <= 4096'),
    ('svr_rmsnorm_mod', (p, p, 4, 4104, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: dim must be a multiple of 8 and <= 4096'),
    ('svr_rmsnorm_mod', (None, p, 4, 64, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: null pointer'),
    ('svr_rmsnorm_mod', (p, None, 4, 64, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: null pointer'),
    ('svr_rmsnorm_mod', (p, p, 4, 64, 1e-6, None, None, None, 3, None), 'svr_rmsnorm_mod: x_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('svr_rmsnorm_mod', (p, p, 4, 64, 1e-6, None, None, None, -1, None), 'svr_rmsnorm_mod: x_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('svr_rmsnorm_mod', (p + 8, p, 4, 12, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: x and y must be 16-byte aligned (rows are read and written in 16-byte units)'),
    ('svr_rmsnorm_mod', (None, p, 4, 12, 1e-6, None, None, None, 0, None), 'svr_rmsnorm_mod: dim must be a multiple of 8 and <= 4096'),
    ('svr_rmsnorm_mod', (None, p, 4, 64, 1e-6, None, None, None, 3, None), 'svr_rmsnorm_mod: null pointer'),
    ('svr_rmsnorm_mod', (p, p, 0, 12, 1e-6, None, None, None, 3, None), None),
    ('svr_rmsnorm_mod', (None, None, 0, 64, 1e-6, None, None, None, 0, None), None),
    ('svr_rmsnorm_mod', (p, p, -1, 64, 1e-6, None, None, None, 0, None), None),
    ('svr_ada_combine', (p, p, p, p, 65536, 4, None), 'svr_ada_combine: at most 65535 vectors per call'),
    ('svr_ada_combine', (None, p, p, p, 2, 4, None), 'svr_ada_combine: null pointer'),
    ('svr_ada_combine', (p, None, p, p, 2, 4, None), 'svr_ada_combine: null pointer'),
    ('svr_ada_combine', (p, p, None, p, 2, 4, None), 'svr_ada_combine: null pointer'),
    ('svr_ada_combine', (p, p, p, None, 2, 4, None), 'svr_ada_combine: null pointer'),
    ('svr_ada_combine', (None, p, p, p, 65536, 4, None), 'svr_ada_combine: at most 65535 vectors per call'),
    ('svr_ada_combine', (p, p, p, p, 0, 4, None), None),
    ('svr_ada_combine', (p, p, p, p, 2, 0, None), None),
    ('svr_ada_combine', (None, None, None, None, 65536, 0, None), None),
    ('svr_qknorm_rope', (p, 4, 2, p, 0, p, p, 8, 0, p, p, 1e-6, None), 'svr_qknorm_rope: 1..21 frequencies per axis (head_dim 128)'),
    ('svr_qknorm_rope', (p, 4, 2, p, 0, p, p, 8, 22, p, p, 1e-6, None), 'svr_qknorm_rope: 1..21 frequencies per axis (head_dim 128)'),
    ('svr_qknorm_rope', (p, 4, 0, p, 0, p, p, 8, 21, p, p, 1e-6, None), 'svr_qknorm_rope: heads and n_pos must be positive'),
    ('svr_qknorm_rope', (p, 4, 2, p, 0, p, p, 0, 21, p, p, 1e-6, None), 'svr_qknorm_rope: heads and n_pos must be positive'),
    ('svr_qknorm_rope', (None, 4, 2, p, 0, p, p, 8, 21, p, p, 1e-6, None), 'svr_qknorm_rope: null pointer (wq / wk are required)'),
    ('svr_qknorm_rope', (p, 4, 2, None, 0, p, p, 8, 21, p, p, 1e-6, None), 'svr_qknorm_rope: null pointer (wq / wk are required)'),
    ('svr_qknorm_rope', (p, 4, 2, p, 0, None, p, 8, 21, p, p, 1e-6, None), 'svr_qknorm_rope: null pointer (wq / wk are required)'),
    ('svr_qknorm_rope', (p, 4, 2, p, 0, p, None, 8, 21, p, p, 1e-6, None), 'svr_qknorm_rope: null pointer (wq / wk are required)'),
    ('svr_qknorm_rope', (p, 4, 2, p, 0, p, p, 8, 21, None, p, 1e-6, None), 'svr_qknorm_rope: null pointer (wq / wk are required)'),
    ('svr_qknorm_rope', (p, 4, 2, p, 0, p, p, 8, 21, p, None, 1e-6, None), 'svr_qknorm_rope: null pointer (wq / wk are required)'),
    ('svr_qknorm_rope', (p, 4, 0, p, 0, p, p, 8, 0, p, p, 1e-6, None), 'svr_qknorm_rope: 1..21 frequencies per axis (head_dim 128)'),
    ('svr_qknorm_rope', (None, 4, 0, p, 0, p, p, 8, 21, p, p, 1e-6, None), 'svr_qknorm_rope: heads and n_pos must be positive'),
    ('svr_qknorm_rope', (p, 0, 2, p, 0, p, p, 8, 21, p, p, 1e-6, None), None),
    ('svr_qknorm_rope', (None, 0, 0, p, 0, p, p, 0, 0, p, p, 1e-6, None), None),
    ('svr_attn_varlen', (p, 760, p, 256, p, p, p, 3, 130, 2, 128, 0.1, None), 'svr_attn_varlen: ld_qkv must cover the 3 * heads * head_dim columns of a qkv row'),
    ('svr_attn_varlen', (p, 768, p, 248, p, p, p, 3, 130, 2, 128, 0.1, None), 'svr_attn_varlen: ld_out must cover the heads * head_dim columns of an out row'),
    ('svr_attn_varlen', (p + 8, 768, p, 256, p, p, p, 3, 130, 2, 128, 0.1, None), 'svr_attn_varlen: qkv must be 16-byte aligned and ld_qkv a multiple of 8 (rows are read in 16-byte units)'),
    ('svr_attn_varlen', (p, 772, p, 256, p, p, p, 3, 130, 2, 128, 0.1, None), 'svr_attn_varlen: qkv must be 16-byte aligned and ld_qkv a multiple of 8 (rows are read in 16-byte units)'),
    ('svr_attn_varlen', (p, 768, p + 4, 256, p, p, p, 3, 130, 2, 128, 0.1, None), "svr_attn_varlen: out must be 8-byte aligned and ld_out a multiple of 4 (the first kernel's 8-byte stores; the window kernel takes 16-byte aligned rows only)"),
    ('svr_attn_varlen', (p, 768, p, 258, p, p, p, 3, 130, 2, 128, 0.1, None), "svr_attn_varlen: out must be 8-byte aligned and ld_out a multiple of 4 (the first kernel's 8-byte stores; the window kernel takes 16-byte aligned rows only)"),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 65536, 130, 2, 128, 0.1, None), 'svr_attn_varlen: grid too large'),
    ('svr_attn_varlen', (p, 3 * 65536 * 128, p, 65536 * 128, p, p, p, 3, 130, 65536, 128, 0.1, None), 'svr_attn_varlen: grid too large'),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 3, 130, 2, 64, 0.1, None), 'svr_attn_varlen: head_dim must be 128 or 512'),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 3, 130, 0, 128, 0.1, None), 'svr_attn_varlen: heads must be positive'),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 3, 130, -1, 512, 0.1, None), 'svr_attn_varlen: heads must be positive'),
    ('svr_attn_varlen', (p + 8, 760, p, 256, p, p, p, 3, 130, 2, 128, 0.1, None), 'svr_attn_varlen: ld_qkv must cover the 3 * heads * head_dim columns of a qkv row'),
    ('svr_attn_varlen', (p, 768, p + 4, 248, p, p, p, 3, 130, 2, 128, 0.1, None), 'svr_attn_varlen: ld_out must cover the heads * head_dim columns of an out row'),
    ('svr_attn_varlen', (p + 8, 768, p + 4, 256, p, p, p, 3, 130, 2, 128, 0.1, None), 'svr_attn_varlen: qkv must be 16-byte aligned and ld_qkv a multiple of 8 (rows are read in 16-byte units)'),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 65536, 130, 2, 64, 0.1, None), 'svr_attn_varlen: grid too large'),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 3, 130, 0, 64, 0.1, None), 'svr_attn_varlen: head_dim must be 128 or 512'),
    ('svr_attn_varlen', (p + 8, 768, p, 256, p, p, p, 0, 130, 2, 128, 0.1, None), 'svr_attn_varlen: qkv must be 16-byte aligned and ld_qkv a multiple of 8 (rows are read in 16-byte units)'),
    ('svr_attn_varlen', (p, 768, p + 4, 256, p, p, p, 3, 0, 2, 128, 0.1, None), "svr_attn_varlen: out must be 8-byte aligned and ld_out a multiple of 4 (the first kernel's 8-byte stores; the window kernel takes 16-byte aligned rows only)"),
    ('svr_attn_varlen', (p, 768, p, 256, None, None, None, 0, 130, 2, 128, 0.1, None), None),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 3, 0, 2, 128, 0.1, None), None),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 0, 130, 2, 64, 0.1, None), None),
    ('svr_attn_varlen', (p, 768, p, 256, p, p, p, 65536, 0, 0, 64, 0.1, None), None),
    ('svr_conv_pack_frag_taps', (p, p, 0, 128, 1, 2, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 48, 128, 1, 2, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 0, 1, 2, 2, 0, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 192, 1, 2, 2, 48, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 0, 0, 2, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 512, 4, 2, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 0, 1, 0, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 256, 1, 4, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 0, 1, 2, 0, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 256, 1, 2, 4, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (p, p, 32, 127, 1, 2, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_conv_pack_frag_taps', (None, None, 32, 129, 1, 2, 2, 32, None), 'svr_conv_pack_frag_taps: need N % 32 == 0, Cin % 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin'),
    ('svr_gemm_pack_frag', (p, p, 0, 64, None), 'svr_gemm_pack_frag: need N % 128 == 0, K % 64 == 0'),
    ('svr_gemm_pack_frag', (p, p, 64, 64, None), 'svr_gemm_pack_frag: need N % 128 == 0, K % 64 == 0'),
    ('svr_gemm_pack_frag', (p, p, 128, 0, None), 'svr_gemm_pack_frag: need N % 128 == 0, K % 64 == 0'),
    ('svr_gemm_pack_frag', (p, p, 128, 32, None), 'svr_gemm_pack_frag: need N % 128 == 0, K % 64 == 0'),
    ('svr_gemm_pack_frag', (None, None, -128, -64, None), 'svr_gemm_pack_frag: need N % 128 == 0, K % 64 == 0'),
    ('svr_conv_pack_frag', (p, p, 0, 288, 1, 32, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_conv_pack_frag', (p, p, 48, 288, 1, 32, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_conv_pack_frag', (p, p, 32, 0, 1, 0, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_conv_pack_frag', (p, p, 32, 432, 1, 48, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_conv_pack_frag', (p, p, 32, 0, 0, 32, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_conv_pack_frag', (p, p, 32, 1152, 4, 32, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_conv_pack_frag', (p, p, 32, 287, 1, 32, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_conv_pack_frag', (None, None, 32, 128, 1, 32, None), 'svr_conv_pack_frag: need N % 32 == 0, Cin % 32 == 0, kt in 1..3, K == kt * 9 * Cin'),
    ('svr_softmax_rows', (p, p, 4, 64, 60, 64, 1.0, None), 'svr_softmax_rows: ld_s and ld_p must cover the cols columns of a row'),
    ('svr_softmax_rows', (p, p, 4, 64, 64, 60, 1.0, None), 'svr_softmax_rows: ld_s and ld_p must cover the cols columns of a row'),
    ('svr_softmax_rows', (p + 8, p, 4, 64, 64, 64, 1.0, None), 'svr_softmax_rows: S must be 16-byte aligned (rows are read as float4)'),
    ('svr_softmax_rows', (p, p + 4, 4, 64, 64, 64, 1.0, None), 'svr_softmax_rows: P must be 8-byte aligned (rows are written in 8-byte units)'),
    ('svr_softmax_rows', (None, p, 4, 64, 64, 64, 1.0, None), 'svr_softmax_rows: null pointer'),
    ('svr_softmax_rows', (p, None, 4, 64, 64, 64, 1.0, None), 'svr_softmax_rows: null pointer'),
    ('svr_softmax_rows', (p, p, 1 << 31, 64, 64, 64, 1.0, None), 'svr_softmax_rows: at most 2^31 - 1 rows per call'),
    ('svr_softmax_rows', (p, p, 4, 6, 8, 8, 1.0, None), 'svr_softmax_rows: cols must be a multiple of 4 and <= 65536, leading dimensions multiples of 4'),
    ('svr_softmax_rows', (p, p, 4, 65540, 65540, 65540, 1.0, None), 'svr_softmax_rows: cols must be a multiple of 4 and <= 65536, leading dimensions multiples of 4'),
    ('svr_softmax_rows', (p, p, 4, 64, 66, 64, 1.0, None), 'svr_softmax_rows: cols must be a multiple of 4 and <= 65536, leading dimensions multiples of 4'),
    ('svr_softmax_rows', (p, p, 4, 64, 64, 66, 1.0, None), 'svr_softmax_rows: cols must be a multiple of 4 and <= 65536, leading dimensions multiples of 4'),
    ('svr_softmax_rows', (p + 8, p, 4, 64, 60, 64, 1.0, None), 'svr_softmax_rows: ld_s and ld_p must cover the cols columns of a row'),
    ('svr_softmax_rows', (p + 8, p + 4, 4, 64, 64, 64, 1.0, None), 'svr_softmax_rows: S must be 16-byte aligned (rows are read as float4)'),
    ('svr_softmax_rows', (p, p, 0, 64, 60, 64, 1.0, None), 'svr_softmax_rows: ld_s and ld_p must cover the cols columns of a row'),
    ('svr_softmax_rows', (p + 8, p, 0, 64, 64, 64, 1.0, None), 'svr_softmax_rows: S must be 16-byte aligned (rows are read as float4)'),
    ('svr_softmax_rows', (p, p + 4, 0, 64, 64, 64, 1.0, None), 'svr_softmax_rows: P must be 8-byte aligned (rows are written in 8-byte units)'),
    ('svr_softmax_rows', (None, p, 1 << 31, 64, 64, 64, 1.0, None), 'svr_softmax_rows: null pointer'),
    ('svr_softmax_rows', (p, p, 1 << 31, 6, 8, 8, 1.0, None), 'svr_softmax_rows: at most 2^31 - 1 rows per call'),
    ('svr_softmax_rows', (p, p, 0, 64, 64, 64, 1.0, None), None),
    ('svr_softmax_rows', (p, p, 4, 0, 0, 0, 1.0, None), None),
    ('svr_softmax_rows', (p, p, 0, 6, 8, 8, 1.0, None), None),
    ('svr_softmax_rows', (None, None, -1, 64, 66, 66, 1.0, None), None),
    ('svr_rows_mean', (p, p, 2, 3, 12, None), 'svr_rows_mean: dim must be a multiple of 8'),
    ('svr_rows_mean', (p, p, 2, 65536, 64, None), 'svr_rows_mean: at most 65535 rows per group'),
    ('svr_rows_mean', (None, p, 2, 3, 64, None), 'svr_rows_mean: null pointer'),
    ('svr_rows_mean', (p, None, 2, 3, 64, None), 'svr_rows_mean: null pointer'),
    ('svr_rows_mean', (p, p, 2, 65536, 12, None), 'svr_rows_mean: dim must be a multiple of 8'),
    ('svr_rows_mean', (None, p, 2, 65536, 64, None), 'svr_rows_mean: at most 65535 rows per group'),
    ('svr_rows_mean', (p, p, 0, 3, 64, None), None),
    ('svr_rows_mean', (p, p, 2, 0, 64, None), None),
    ('svr_rows_mean', (p, p, 2, 3, 0, None), None),
    ('svr_rows_mean', (None, None, 0, 65536, 12, None), None),
    ('svr_patchify', (p, p, 1, 3, 4, 16, 64, None), 'svr_patchify: H, W must be even, C positive and kpad >= 4*C'),
    ('svr_patchify', (p, p, 1, 4, 3, 16, 64, None), 'svr_patchify: H, W must be even, C positive and kpad >= 4*C'),
    ('svr_patchify', (p, p, 1, 4, 4, 0, 64, None), 'svr_patchify: H, W must be even, C positive and kpad >= 4*C'),
    ('svr_patchify', (p, p, 1, 4, 4, 16, 63, None), 'svr_patchify: H, W must be even, C positive and kpad >= 4*C'),
    ('svr_patchify', (None, p, 1, 4, 4, 16, 64, None), 'svr_patchify: null pointer'),
    ('svr_patchify', (p, None, 1, 4, 4, 16, 64, None), 'svr_patchify: null pointer'),
    ('svr_patchify', (None, p, 1, 3, 4, 16, 64, None), 'svr_patchify: H, W must be even, C positive and kpad >= 4*C'),
    ('svr_patchify', (p, p, 0, 3, 4, 16, 64, None), 'svr_patchify: H, W must be even, C positive and kpad >= 4*C'),
    ('svr_patchify', (None, p, 0, 4, 4, 16, 64, None), 'svr_patchify: null pointer'),
    ('svr_patchify', (p, p, 0, 4, 4, 16, 64, None), None),
    ('svr_patchify', (p, p, 1, 0, 4, 16, 64, None), None),
    ('svr_patchify', (p, p, -1, 4, 4, 16, 64, None), None),
    ('svr_unpatchify_euler', (p, 64, None, p, 1, 3, 4, 16, None), 'svr_unpatchify_euler: H, W must be even'),
    ('svr_unpatchify_euler', (p, 64, None, p, 1, 4, 3, 16, None), 'svr_unpatchify_euler: H, W must be even'),
    ('svr_unpatchify_euler', (None, 64, None, p, 1, 4, 4, 16, None), 'svr_unpatchify_euler: null pointer'),
    ('svr_unpatchify_euler', (p, 64, None, None, 1, 4, 4, 16, None), 'svr_unpatchify_euler: null pointer'),
    ('svr_unpatchify_euler', (p, 63, p, p, 1, 4, 4, 16, None), 'svr_unpatchify_euler: ldp must cover the 4*C prediction columns'),
    ('svr_unpatchify_euler', (None, 64, None, p, 1, 3, 4, 16, None), 'svr_unpatchify_euler: H, W must be even'),
    ('svr_unpatchify_euler', (None, 63, None, p, 1, 4, 4, 16, None), 'svr_unpatchify_euler: null pointer'),
    ('svr_unpatchify_euler', (p, 63, None, p, 0, 4, 4, 16, None), 'svr_unpatchify_euler: ldp must cover the 4*C prediction columns'),
    ('svr_unpatchify_euler', (p, 64, None, p, 0, 4, 4, 16, None), None),
    ('svr_unpatchify_euler', (p, 0, None, p, 1, 4, 4, 0, None), None),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 0, 32, 0, None), 'svr_groupnorm_stats: need C > 0, 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 128, 0, 0, None), 'svr_groupnorm_stats: need C > 0, 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 130, 32, 0, None), 'svr_groupnorm_stats: need C > 0, 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_stats', (p, p, p, 65536, 16, 128, 32, 0, None), 'svr_groupnorm_stats: need C > 0, 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_stats', (None, p, p, 1, 16, 128, 32, 0, None), 'svr_groupnorm_stats: null pointer'),
    ('svr_groupnorm_stats', (p, None, p, 1, 16, 128, 32, 0, None), 'svr_groupnorm_stats: null pointer'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 132, 33, 0, None), 'svr_groupnorm_stats: need C in {128,256,512}-like (C%8==0, C<=512, groups<=32, (C/groups)%4==0)'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 1024, 32, 0, None), 'svr_groupnorm_stats: need C in {128,256,512}-like (C%8==0, C<=512, groups<=32, (C/groups)%4==0)'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 256, 64, 0, None), 'svr_groupnorm_stats: need C in {128,256,512}-like (C%8==0, C<=512, groups<=32, (C/groups)%4==0)'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 64, 32, 0, None), 'svr_groupnorm_stats: need C in {128,256,512}-like (C%8==0, C<=512, groups<=32, (C/groups)%4==0)'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 96, 8, 0, None), 'svr_groupnorm_stats: need C in {128,256,512}-like (C%8==0, C<=512, groups<=32, (C/groups)%4==0)'),
    ('svr_groupnorm_stats', (p, p, None, 1, 16, 128, 32, 0, None), 'svr_groupnorm_stats: workspace missing (svr_groupnorm_workspace_bytes)'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 128, 32, 3, None), 'svr_groupnorm_stats: x_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('svr_groupnorm_stats', (p, p, p, 1, 16, 128, 32, -1, None), 'svr_groupnorm_stats: x_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('svr_groupnorm_stats', (None, p, p, 1, 16, 0, 32, 0, None), 'svr_groupnorm_stats: need C > 0, 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_stats', (None, p, p, 1, 16, 1024, 32, 0, None), 'svr_groupnorm_stats: null pointer'),
    ('svr_groupnorm_stats', (p, p, None, 1, 16, 1024, 32, 0, None), 'svr_groupnorm_stats: need C in {128,256,512}-like (C%8==0, C<=512, groups<=32, (C/groups)%4==0)'),
    ('svr_groupnorm_stats', (p, p, None, 1, 16, 128, 32, 3, None), 'svr_groupnorm_stats: workspace missing (svr_groupnorm_workspace_bytes)'),
    ('svr_groupnorm_stats', (p, p, p, 0, 16, 128, 32, 0, None), None),
    ('svr_groupnorm_stats', (p, p, p, 1, 0, 128, 32, 0, None), None),
    ('svr_groupnorm_stats', (None, None, None, 0, 16, 0, 0, 3, None), None),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 0, 32, 1e-6, 0, 0, None), 'svr_groupnorm_apply: C must be a multiple of 8 and <= 512'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 12, 4, 1e-6, 0, 0, None), 'svr_groupnorm_apply: C must be a multiple of 8 and <= 512'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 520, 8, 1e-6, 0, 0, None), 'svr_groupnorm_apply: C must be a multiple of 8 and <= 512'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 128, 0, 1e-6, 0, 0, None), 'svr_groupnorm_apply: need 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 128, 3, 1e-6, 0, 0, None), 'svr_groupnorm_apply: need 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 65536, 16, 128, 32, 1e-6, 0, 0, None), 'svr_groupnorm_apply: need 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_apply', (None, p, p, p, p, 1, 16, 128, 32, 1e-6, 0, 0, None), 'svr_groupnorm_apply: null pointer'),
    ('svr_groupnorm_apply', (p, None, p, p, p, 1, 16, 128, 32, 1e-6, 0, 0, None), 'svr_groupnorm_apply: null pointer'),
    ('svr_groupnorm_apply', (p, p, None, p, p, 1, 16, 128, 32, 1e-6, 0, 0, None), 'svr_groupnorm_apply: null pointer'),
    ('svr_groupnorm_apply', (p, p, p, None, p, 1, 16, 128, 32, 1e-6, 0, 0, None), 'svr_groupnorm_apply: null pointer'),
    ('svr_groupnorm_apply', (p, p, p, p, None, 1, 16, 128, 32, 1e-6, 0, 0, None), 'svr_groupnorm_apply: null pointer'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 128, 32, 1e-6, 1, 3, None), 'svr_groupnorm_apply: x_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 128, 32, 1e-6, 0, -1, None), 'svr_groupnorm_apply: x_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 16, 12, 0, 1e-6, 0, 0, None), 'svr_groupnorm_apply: C must be a multiple of 8 and <= 512'),
    ('svr_groupnorm_apply', (None, p, p, p, p, 1, 16, 128, 0, 1e-6, 0, 0, None), 'svr_groupnorm_apply: need 1 <= groups dividing C, T <= 65535'),
    ('svr_groupnorm_apply', (None, p, p, p, p, 1, 16, 128, 32, 1e-6, 0, 3, None), 'svr_groupnorm_apply: null pointer'),
    ('svr_groupnorm_apply', (p, p, p, p, p, 0, 16, 128, 32, 1e-6, 0, 0, None), None),
    ('svr_groupnorm_apply', (p, p, p, p, p, 1, 0, 128, 32, 1e-6, 0, 0, None), None),
    ('svr_groupnorm_apply', (None, None, None, None, None, 0, 16, 0, 0, 1e-6, 0, 3, None), None),
    ('svr_im2col_causal', (p, p, None, 64, None), 'svr_im2col_causal: null geometry / pointer'),
    ('svr_im2col_causal', (None, p, G(), 64, None), 'svr_im2col_causal: null geometry / pointer'),
    ('svr_im2col_causal', (p, None, G(), 64, None), 'svr_im2col_causal: null geometry / pointer'),
    ('svr_im2col_causal', (p, p, G(Cin=0), 64, None), 'svr_im2col_causal: Cin % 4 == 0 and kpad a multiple of Cin covering all taps required'),
    ('svr_im2col_causal', (p, p, G(Cin=6), 66, None), 'svr_im2col_causal: Cin % 4 == 0 and kpad a multiple of Cin covering all taps required'),
    ('svr_im2col_causal', (p, p, G(), 96, None), 'svr_im2col_causal: Cin % 4 == 0 and kpad a multiple of Cin covering all taps required'),
    ('svr_im2col_causal', (p, p, G(kt=3, kh=3, kw=3), 64, None), 'svr_im2col_causal: Cin % 4 == 0 and kpad a multiple of Cin covering all taps required'),
    ('svr_im2col_causal', (None, p, G(Cin=0), 64, None), 'svr_im2col_causal: null geometry / pointer'),
    ('svr_im2col_causal', (p, p, G(Cin=0, To=0), 64, None), 'svr_im2col_causal: Cin % 4 == 0 and kpad a multiple of Cin covering all taps required'),
    ('svr_im2col_causal', (p, p, G(To=0), 64, None), None),
    ('svr_im2col_causal', (p, p, G(Ho=0), 128, None), None),
    ('svr_blend_accumulate', (p, p, p, p, p, 1, 2, 2, 4, 8, 8, -1, 0, None), 'svr_blend_accumulate: tile outside the canvas'),
    ('svr_blend_accumulate', (p, p, p, p, p, 1, 2, 2, 4, 8, 8, 0, -1, None), 'svr_blend_accumulate: tile outside the canvas'),
    ('svr_blend_accumulate', (p, p, p, p, p, 1, 2, 2, 4, 8, 8, 7, 0, None), 'svr_blend_accumulate: tile outside the canvas'),
    ('svr_blend_accumulate', (p, p, p, p, p, 1, 2, 2, 4, 8, 8, 0, 7, None), 'svr_blend_accumulate: tile outside the canvas'),
    ('svr_blend_accumulate', (None, p, p, p, p, 1, 2, 2, 4, 8, 8, 0, 0, None), 'svr_blend_accumulate: null pointer'),
    ('svr_blend_accumulate', (p, None, p, p, p, 1, 2, 2, 4, 8, 8, 0, 0, None), 'svr_blend_accumulate: null pointer'),
    ('svr_blend_accumulate', (p, p, None, p, p, 1, 2, 2, 4, 8, 8, 0, 0, None), 'svr_blend_accumulate: null pointer'),
    ('svr_blend_accumulate', (p, p, p, None, p, 1, 2, 2, 4, 8, 8, 0, 0, None), 'svr_blend_accumulate: null pointer'),
    ('svr_blend_accumulate', (p, p, p, p, None, 1, 2, 2, 4, 8, 8, 0, 0, None), 'svr_blend_accumulate: null pointer'),
    ('svr_blend_accumulate', (None, p, p, p, p, 1, 2, 2, 4, 8, 8, -1, 0, None), 'svr_blend_accumulate: tile outside the canvas'),
    ('svr_blend_accumulate', (p, p, p, p, p, 0, 2, 2, 4, 8, 8, 0, 0, None), None),
    ('svr_blend_accumulate', (p, p, p, p, p, 1, 2, 2, 0, 8, 8, 0, 0, None), None),
    ('svr_blend_accumulate', (None, None, None, None, None, 0, 2, 2, 4, 8, 8, -1, 7, None), None),
    ('svr_blend_finalize', (p, p, p, 1, 16, 4, 5, 1.0, 0.0, None), 'svr_blend_finalize: c_take > C'),
    ('svr_blend_finalize', (None, p, p, 1, 16, 4, 3, 1.0, 0.0, None), 'svr_blend_finalize: null pointer'),
    ('svr_blend_finalize', (p, None, p, 1, 16, 4, 3, 1.0, 0.0, None), 'svr_blend_finalize: null pointer'),
    ('svr_blend_finalize', (p, p, None, 1, 16, 4, 3, 1.0, 0.0, None), 'svr_blend_finalize: null pointer'),
    ('svr_blend_finalize', (None, p, p, 1, 16, 4, 5, 1.0, 0.0, None), 'svr_blend_finalize: c_take > C'),
    ('svr_blend_finalize', (p, p, p, 0, 16, 4, 3, 1.0, 0.0, None), None),
    ('svr_blend_finalize', (p, p, p, 1, 0, 4, 3, 1.0, 0.0, None), None),
    ('svr_blend_finalize', (p, p, p, 1, 16, 4, 0, 1.0, 0.0, None), None),
    ('svr_blend_finalize', (None, None, None, 0, 16, 4, 5, 1.0, 0.0, None), None),
    ('svr_affine_slice', (p, p, 4, 8, 0, 1.0, 0.0, None), 'svr_affine_slice: need 0 < c_out <= c_in'),
    ('svr_affine_slice', (p, p, 4, 8, 9, 1.0, 0.0, None), 'svr_affine_slice: need 0 < c_out <= c_in'),
    ('svr_affine_slice', (None, p, 4, 8, 4, 1.0, 0.0, None), 'svr_affine_slice: null pointer'),
    ('svr_affine_slice', (p, None, 4, 8, 4, 1.0, 0.0, None), 'svr_affine_slice: null pointer'),
    ('svr_affine_slice', (None, p, 4, 8, 0, 1.0, 0.0, None), 'svr_affine_slice: need 0 < c_out <= c_in'),
    ('svr_affine_slice', (p, p, 0, 8, 4, 1.0, 0.0, None), None),
    ('svr_affine_slice', (None, None, -1, 8, 9, 1.0, 0.0, None), None),
]


# ---- svr_gemm_bf16 / svr_gemm_kernel_class: (base launch, the svr_gemm_args fields overwritten, message)
FAKE = 0x10000000            # a 256-byte aligned fake device address: every operand of a base launch sits there


def _bases():
    """name -> svr_gemm_args of a launch the library accepts, filled by ops.fill_gemm_args from shape-only tensors"""
    ops = sub("ops")
    bf16, f32 = torch.bfloat16, torch.float32

    def t(*shape, dtype=bf16):
        return torch.empty(*shape, dtype=dtype, device="meta")

    def fill(A, W, out, **kw):
        return lambda: ops.fill_gemm_args(A, W, out, ptr=lambda _: FAKE, zeros_ptr=FAKE, **kw)[0]

    def conv(Cin, k):
        return ops.Conv3dGeom(T=2, H=8, W=8, Cin=Cin, To=2, Ho=8, Wo=8, k=k, stride=(1, 1, 1), pad=(0, 1, 1))

    return {
        # 256 x 256 x 128, bias epilogue, bf16 out
        "plain": fill(t(256, 128), t(256, 128), t(256, 256), N=256, K=128, bias=t(256, dtype=f32)),
        "fp32": fill(t(256, 128), t(256, 128), t(256, 256, dtype=f32), N=256, K=128, out_f32=True),
        "resid": fill(t(256, 128), t(256, 128), t(256, 256), N=256, K=128, epilogue=ops.EPI_RESID_GATE, gate=t(256, dtype=f32),
                      resid=t(256, 256)),
        "swiglu": fill(t(256, 128), t(256, 128), t(256, 128), N=256, K=128, epilogue=ops.EPI_SWIGLU),
        # [2, 8, 8, 64] -> 128 channels through 1x3x3 taps: the LDS-halo kernel's geometry
        "conv": fill(t(2, 8, 8, 64), t(128, 576), t(128, 128), N=128, K=576, conv=conv(64, (1, 3, 3))),
        # Cin = 4 with K padded to 128: the thin-input kernel's
        "thin": fill(t(2, 8, 8, 4), t(128, 128), t(128, 128), N=128, K=128, conv=conv(4, (1, 3, 3))),
        # one phase of a sub-pixel upsampler (1x2x2 taps) without fragment-ordered weights: the generic conv kernel's
        "phase": fill(t(2, 8, 8, 64), t(128, 256), t(2, 16, 16, 128), N=128, K=256, conv=conv(64, (1, 2, 2)),
                      phase=ops.PhaseScatter(0, 0)),
    }


GEMM_ROWS = [
    # gemm_route
    ('plain', {'K': 0}, 'svr_gemm_bf16: K must be a positive multiple of 64'),
    ('plain', {'K': 65, 'lda': 72}, 'svr_gemm_bf16: K must be a positive multiple of 64'),
    ('plain', {'epilogue': 5}, 'svr_gemm_bf16: unknown epilogue code'),
    ('plain', {'epilogue': -1}, 'svr_gemm_bf16: unknown epilogue code'),
    ('plain', {'resid': FAKE, 'ldr': 256}, 'svr_gemm_bf16: resid needs SVR_EPI_RESID_GATE'),
    ('plain', {'resid_f32': 1}, 'svr_gemm_bf16: resid_f32 without resid'),
    ('plain', {'out_f32': 3}, 'svr_gemm_bf16: out_f32 / resid_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('plain', {'out_f32': -1}, 'svr_gemm_bf16: out_f32 / resid_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('resid', {'resid_f32': 3}, 'svr_gemm_bf16: out_f32 / resid_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('swiglu', {'out_f32': 2}, 'svr_gemm_bf16: h16 output with SwiGLU / pixel shuffle'),
    ('plain', {'out_f32': 2, 'ps.enabled': 1}, 'svr_gemm_bf16: h16 output with SwiGLU / pixel shuffle'),
    ('thin', {'ldc': 132}, "svr_gemm_bf16(conv, thin Cin = 4 input): C, resid and bias must be 16-byte aligned, ldc and ldr multiples of 8 (the LDS-halo kernel's 16-byte accesses; no other kernel serves this geometry)"),
    ('thin', {'C': FAKE + 8}, "svr_gemm_bf16(conv, thin Cin = 4 input): C, resid and bias must be 16-byte aligned, ldc and ldr multiples of 8 (the LDS-halo kernel's 16-byte accesses; no other kernel serves this geometry)"),
    ('thin', {'bias': FAKE + 8}, "svr_gemm_bf16(conv, thin Cin = 4 input): C, resid and bias must be 16-byte aligned, ldc and ldr multiples of 8 (the LDS-halo kernel's 16-byte accesses; no other kernel serves this geometry)"),
    ('conv', {'conv.Cin': 32}, 'svr_gemm_bf16(conv): Cin must be a multiple of 64 (or the thin Cin = 4, 3x3, stride-1 geometry)'),
    ('conv', {'K': 640}, 'svr_gemm_bf16(conv): K != taps*Cin'),
    ('conv', {'M': 127}, 'svr_gemm_bf16(conv): M != To*Ho*Wo'),
    ('conv', {'conv.zeros': None}, 'svr_gemm_bf16(conv): zero page missing'),
    ('conv', {'conv.halo': FAKE, 'conv.halo_frames': 1, 'conv.pt': 2, 'conv.kt': 3, 'K': 1728}, 'svr_gemm_bf16(conv): halo shorter than causal pad'),
    ('swiglu', {'N': 48, 'ldc': 24}, 'svr_gemm_bf16: SWIGLU needs N % 32 == 0'),
    ('plain', {'ps.enabled': 1, 'ps.F': 1, 'ps.H': 16, 'ps.W': 16, 'ps.rz': 1, 'ps.C': 32}, 'svr_gemm_bf16: bad pixel-shuffle geometry'),
    ('plain', {'ps.enabled': 1, 'ps.F': 1, 'ps.H': 16, 'ps.W': 15, 'ps.rz': 1, 'ps.C': 64}, 'svr_gemm_bf16: bad pixel-shuffle geometry'),
    ('plain', {'N': 24, 'ldc': 24, 'ps.enabled': 1, 'ps.F': 1, 'ps.H': 16, 'ps.W': 16, 'ps.rz': 1, 'ps.C': 6}, 'svr_gemm_bf16: bad pixel-shuffle geometry'),
    ('plain', {'phase.enabled': 1}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'conv.sh': 2}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'conv.Ho': 4, 'M': 64}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'epilogue': 3}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'phase.py': 2}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'phase.px': -1}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'phase.t_stride': 3}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'gn_partial': FAKE, 'gn_groups': 32}, 'svr_gemm_bf16: phase scatter needs a stride-1 same-size conv without ps / residual / SwiGLU (fused statistics: sub-pixel conv kernel only)'),
    ('phase', {'phase.quad': 1}, 'svr_gemm_bf16: a quad phase launch is served by the sub-pixel conv kernel only ((kt, 2, 2) taps, four fragment-ordered weight copies, bias epilogue)'),
    ('plain', {'gn_partial': FAKE, 'gn_groups': 32}, 'svr_gemm_bf16: gn_partial set but this launch cannot produce fused GroupNorm statistics'),
    ('conv', {'gn_partial': FAKE, 'gn_groups': 0}, 'svr_gemm_bf16: gn_partial set but this launch cannot produce fused GroupNorm statistics'),
    # gemm_extent_refusal
    ('plain', {'lda': 120}, 'svr_gemm_bf16: lda must cover the K columns of a row of A (lda >= K)'),
    ('plain', {'ldc': 248}, 'svr_gemm_bf16: ldc must cover the columns of a row of C (ldc >= N, N / 2 for SwiGLU)'),
    ('swiglu', {'ldc': 120}, 'svr_gemm_bf16: ldc must cover the columns of a row of C (ldc >= N, N / 2 for SwiGLU)'),
    ('conv', {'ldc': 120}, 'svr_gemm_bf16: ldc must cover the columns of a row of C (ldc >= N, N / 2 for SwiGLU)'),
    ('resid', {'ldr': 248}, 'svr_gemm_bf16: ldr must cover the N columns of a row of resid (ldr >= N)'),
    # gemm_layout_refusal
    ('plain', {'W': FAKE + 8}, 'svr_gemm_bf16: W must be 16-byte aligned (staged in 16-byte units)'),
    ('conv', {'W': FAKE + 8}, 'svr_gemm_bf16: W must be 16-byte aligned (staged in 16-byte units)'),
    ('conv', {'A': FAKE + 8}, 'svr_gemm_bf16(conv): A must be 16-byte aligned (8-byte for the thin Cin = 4 input)'),
    ('thin', {'A': FAKE + 4}, 'svr_gemm_bf16(conv): A must be 16-byte aligned (8-byte for the thin Cin = 4 input)'),
    ('conv', {'conv.halo': FAKE + 8, 'conv.halo_frames': 0}, 'svr_gemm_bf16(conv): halo must be 16-byte aligned (8-byte for the thin Cin = 4 input)'),
    ('thin', {'conv.halo': FAKE + 4, 'conv.halo_frames': 0}, 'svr_gemm_bf16(conv): halo must be 16-byte aligned (8-byte for the thin Cin = 4 input)'),
    ('conv', {'conv.zeros': FAKE + 8}, 'svr_gemm_bf16(conv): zeros (the zero page) must be 16-byte aligned'),
    ('conv', {'W_frag': FAKE + 8}, 'svr_gemm_bf16(conv): W_frag must be 16-byte aligned'),
    ('conv', {'gn_partial': FAKE + 8, 'gn_groups': 32}, 'svr_gemm_bf16(conv): gn_partial must be 16-byte aligned (fp64 pairs)'),
    ('plain', {'A': FAKE + 8}, 'svr_gemm_bf16: A must be 16-byte aligned (rows are staged in 16-byte units)'),
    ('plain', {'lda': 132}, 'svr_gemm_bf16: lda must be a multiple of 8 (rows of A are staged in 16-byte units)'),
    # gemm_epi_direct_refusal (gemm_kernel, the generic conv kernel and the thin-output kernel)
    ('plain', {'C': FAKE + 4}, 'svr_gemm_bf16: C must be 8-byte aligned (16-byte for fp32 output): the direct epilogue stores whole quads of columns'),
    ('fp32', {'C': FAKE + 8}, 'svr_gemm_bf16: C must be 8-byte aligned (16-byte for fp32 output): the direct epilogue stores whole quads of columns'),
    ('plain', {'ldc': 258}, 'svr_gemm_bf16: ldc must be a multiple of 4 (phase scatter: N): the direct epilogue stores whole quads of columns'),
    ('conv', {'conv.st': 2, 'C': FAKE + 4}, 'svr_gemm_bf16: C must be 8-byte aligned (16-byte for fp32 output): the direct epilogue stores whole quads of columns'),
    ('conv', {'N': 32, 'ldc': 34}, 'svr_gemm_bf16: ldc must be a multiple of 4 (phase scatter: N): the direct epilogue stores whole quads of columns'),
    ('phase', {'N': 130}, 'svr_gemm_bf16: ldc must be a multiple of 4 (phase scatter: N): the direct epilogue stores whole quads of columns'),
    ('resid', {'resid': FAKE + 4}, 'svr_gemm_bf16: a bf16 resid must be 8-byte aligned with ldr a multiple of 4: the direct epilogue loads whole quads of columns'),
    ('resid', {'ldr': 258}, 'svr_gemm_bf16: a bf16 resid must be 8-byte aligned with ldr a multiple of 4: the direct epilogue loads whole quads of columns'),
    ('swiglu', {'N': 32, 'ldc': 16, 'C': FAKE + 4}, 'svr_gemm_bf16: C must be 8-byte aligned (16-byte for fp32 output): the direct epilogue stores whole quads of columns'),
    # two faults: which one is reported
    ('plain', {'K': 65, 'epilogue': 5}, 'svr_gemm_bf16: K must be a positive multiple of 64'),
    ('plain', {'epilogue': 5, 'resid': FAKE}, 'svr_gemm_bf16: unknown epilogue code'),
    ('plain', {'resid': FAKE, 'resid_f32': 3}, 'svr_gemm_bf16: resid needs SVR_EPI_RESID_GATE'),
    ('plain', {'out_f32': 3, 'lda': 120}, 'svr_gemm_bf16: out_f32 / resid_f32 must be SVR_STORE_BF16 / _FP32 / _H16'),
    ('plain', {'lda': 120, 'ldc': 248}, 'svr_gemm_bf16: lda must cover the K columns of a row of A (lda >= K)'),
    ('resid', {'ldc': 248, 'ldr': 248}, 'svr_gemm_bf16: ldc must cover the columns of a row of C (ldc >= N, N / 2 for SwiGLU)'),
    ('conv', {'conv.Cin': 32, 'M': 127}, 'svr_gemm_bf16(conv): Cin must be a multiple of 64 (or the thin Cin = 4, 3x3, stride-1 geometry)'),
    ('conv', {'M': 127, 'conv.zeros': None}, 'svr_gemm_bf16(conv): M != To*Ho*Wo'),
    ('conv', {'conv.zeros': None, 'W': FAKE + 8}, 'svr_gemm_bf16(conv): zero page missing'),
    ('plain', {'W': FAKE + 8, 'A': FAKE + 8}, 'svr_gemm_bf16: W must be 16-byte aligned (staged in 16-byte units)'),
    ('plain', {'A': FAKE + 8, 'lda': 132}, 'svr_gemm_bf16: A must be 16-byte aligned (rows are staged in 16-byte units)'),
    ('plain', {'lda': 132, 'C': FAKE + 4}, 'svr_gemm_bf16: lda must be a multiple of 8 (rows of A are staged in 16-byte units)'),
    ('plain', {'C': FAKE + 4, 'ldc': 258}, 'svr_gemm_bf16: C must be 8-byte aligned (16-byte for fp32 output): the direct epilogue stores whole quads of columns'),
    ('resid', {'ldc': 258, 'resid': FAKE + 4}, 'svr_gemm_bf16: ldc must be a multiple of 4 (phase scatter: N): the direct epilogue stores whole quads of columns'),
    ('conv', {'A': FAKE + 8, 'conv.zeros': FAKE + 8}, 'svr_gemm_bf16(conv): A must be 16-byte aligned (8-byte for the thin Cin = 4 input)'),
    ('swiglu', {'N': 48, 'ldc': 24, 'W': FAKE + 8}, 'svr_gemm_bf16: SWIGLU needs N % 32 == 0'),
    # empty problems: nothing else is looked at
    ('plain', {'M': 0}, None),
    ('plain', {'N': 0}, None),
    ('plain', {'M': 0, 'K': 65, 'W': FAKE + 8}, None),
    ('conv', {'M': -1, 'conv.zeros': None}, None),
]


def _planted(L):
    assert L.svr_set_option(b"no_such_key", 0) != 0             # (a known message first: an empty call leaves it standing)
    assert L.svr_last_error().decode() == PLANTED


def test_every_refusal_message_is_exact():
    L = sub("hip_lib").lib()
    for fn, args, message in ROWS:
        _planted(L)
        assert call(L, fn, args) == (0 if message is None else -1), (fn, args)
        assert L.svr_last_error().decode() == (PLANTED if message is None else message), (fn, args)


def gemm_args(bases, base, fields):
    a = bases[base]()
    for path, value in fields.items():
        *outer, leaf = path.split(".")
        target = a
        for name in outer:
            target = getattr(target, name)
        setattr(target, leaf, value)
    return a


def test_gemm_refusal_messages_are_exact_and_the_router_leaves_the_same_words():
    L = sub("hip_lib").lib()
    bases = _bases()
    for base, fields, message in GEMM_ROWS:
        a = gemm_args(bases, base, fields)
        _planted(L)
        assert call(L, "svr_gemm_bf16", (a, None)) == (0 if message is None else -1), (base, fields)
        assert L.svr_last_error().decode() == (PLANTED if message is None else message), (base, fields)
        _planted(L)
        assert call(L, "svr_gemm_kernel_class", (a,)) == (0 if message is None else -1), (base, fields)      # (0: SVR_KERNEL_NONE)
        assert L.svr_last_error().decode() == (PLANTED if message is None else message), (base, fields)


def test_the_base_launches_are_accepted():
    """... so that a row's message is the doing of the fields it overwrites: the router names a kernel class for every base"""
    hip_lib = sub("hip_lib")
    L = hip_lib.lib()
    classes = {}
    for name, base in _bases().items():
        _planted(L)
        classes[name] = hip_lib.KERNEL_CLASSES[call(L, "svr_gemm_kernel_class", (base(),))]
        assert L.svr_last_error().decode() == PLANTED, name
    assert classes == {"plain": "gemm", "fp32": "gemm", "resid": "gemm", "swiglu": "gemm", "conv": "conv_halo", "thin": "conv_thin_in",
                       "phase": "conv_generic"}


def test_the_table_covers_every_entry_point_in_the_range():
    covered = {fn for fn, _, _ in ROWS}
    assert covered == {
        "svr_mfma_calibrate", "svr_set_option", "svr_gemm_bf16", "svr_gemm_kernel_class", "svr_groupnorm_reduce", "svr_rmsnorm_mod",
        "svr_ada_combine", "svr_qknorm_rope", "svr_attn_varlen", "svr_conv_pack_frag_taps", "svr_gemm_pack_frag", "svr_conv_pack_frag",
        "svr_softmax_rows", "svr_rows_mean", "svr_patchify", "svr_unpatchify_euler", "svr_groupnorm_stats", "svr_groupnorm_apply",
        "svr_im2col_causal", "svr_blend_accumulate", "svr_blend_finalize", "svr_affine_slice"}
    empty = {fn for fn, _, message in ROWS if message is None}
    assert empty == {
        "svr_groupnorm_reduce", "svr_rmsnorm_mod", "svr_ada_combine", "svr_qknorm_rope", "svr_attn_varlen", "svr_softmax_rows",
        "svr_rows_mean", "svr_patchify", "svr_unpatchify_euler", "svr_groupnorm_stats", "svr_groupnorm_apply", "svr_im2col_causal",
        "svr_blend_accumulate", "svr_blend_finalize", "svr_affine_slice"}
    assert any(message is None for _, _, message in GEMM_ROWS)
    assert len(ROWS) + len(GEMM_ROWS) == 323
