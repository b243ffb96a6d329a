/*
 * libseedvr2_hip.so -- C ABI of the MI355X (gfx950) SeedVR2 hot path.
 *
 * The reference (numz/ComfyUI-SeedVR2_VideoUpscaler) is pure Python/PyTorch and has no FFI
 * layer; its hot path runs as torch ops below three call sites of the runner
 * (src/core/infer.py:164-184 vae.encode, :249-266 vae.decode, :361-367 dit forward).  Each entry
 * point below replaces the torch op sequence cited next to it.  All pointers are raw DEVICE
 * pointers (tensor.data_ptr()), all tensors are row-major (dense, or with the leading dimension the
 * entry point takes: "Operand layouts" below), activations bf16 unless noted,
 * `stream` is a hipStream_t.  Functions return 0 on success, non-zero on failure
 * (svr_last_error() gives the message).  The library never allocates caller-visible memory.
 *
 * Layouts: DiT activations  [tokens, channels]; VAE activations NDHWC = [T, H, W, C].
 *
 * Operand layouts (the contract of every pointer + leading-dimension pair; tests/layout_cases.py is its table, swept on the CPU by
 * tests/test_layout_cases.py and on the device by tests/test_gpu_layouts.py).  An operand may be a column window of a wider
 * row-major tensor -- base = tensor + c0, pitch = the tensor's row length, in ELEMENTS -- under two rules:
 *   1. a pitch covers its extent (lda >= K, ldc >= N, ldr >= N, ld_qkv >= 3 * heads * head_dim, ...): rows never overlap, and the
 *      columns between the extent and the pitch are neither read nor written;
 *   2. every vector access of the kernel that serves the call is naturally aligned: 16 bytes where a kernel moves uint4 / float4 /
 *      LDS-DMA units, 8 bytes where it moves uint2.  With base % B == 0 bytes and (pitch * element size) % B == 0 every row starts
 *      on a B-byte boundary; the tables below give B per operand as "base bytes / pitch multiple (elements)".
 * Where the kernel a call prefers would break rule 2, the call is routed to a kernel of the same family whose accesses are aligned
 * (a different class from svr_gemm_kernel_class(), same results within the same bounds); where there is none the call FAILS
 * BEFORE ANY LAUNCH (-1, svr_last_error() names the operand; svr_gemm_kernel_class() returns -1).  Dense tensors from an allocator
 * that aligns to 16 bytes or more meet every rule below whenever the extents themselves do (K % 64, N % 8, ...).
 *
 *   svr_gemm_bf16, plain GEMM                  A 16 / lda % 8     W 16 (dense [Npad, K])     W_frag 16
 *     SVR_KERNEL_GEMM_PERSISTENT, and the      C 16 / ldc % 8     resid 16 / ldr % 8     bias 16     gate 16      (any storage kind)
 *       row-contiguous epilogue of SVR_KERNEL_GEMM  (N % 8 == 0; a launch that misses any of these takes the next line)
 *     SVR_KERNEL_GEMM, direct epilogue         C 8 (fp32: 16) / ldc % 4     bf16 resid 8 / ldr % 4     fp32 | h16 resid, bias, gate: element
 *                                              (N < 4: no whole quad of columns, C / resid element-aligned too)
 *   svr_gemm_bf16, conv mode                   A 16, halo 16, zeros 16 (thin Cin = 4 input: A 8, halo 8), W 16, W_frag 16, gn_partial 16
 *     SVR_KERNEL_CONV_HALO / _THIN_IN          C 16 / ldc % 8     resid 16 / ldr % 8     bias 16     gate element
 *                                              (HALO: a launch that misses these takes SVR_KERNEL_CONV_GENERIC; THIN_IN: refused)
 *     SVR_KERNEL_CONV_SUBPIXEL                 C 16, ldc == N (phase scatter: dense output)     bias / bias_border 16
 *                                              (without phase scatter a launch that misses these takes SVR_KERNEL_CONV_GENERIC)
 *     SVR_KERNEL_CONV_THIN_OUT                 the direct epilogue's line above (ldc == N with a plain bias epilogue and N <= 4: the
 *                                              dense store path; any other ldc >= N: quad / element stores)
 *     SVR_KERNEL_CONV_GENERIC                  the two epilogue lines of the plain GEMM; pixel shuffle / phase scatter outputs are
 *                                              dense (ldc ignored): C 16 and ps.C % 8 for the row-contiguous epilogue, else C 8, ps.C % 4
 *   svr_attn_varlen                            qkv 16 / ld_qkv % 8 (both kernels read rows in 16-byte units)
 *                                              out 16 / ld_out % 8: window kernel (head_dim 128);  out 8 / ld_out % 4: first kernel
 *                                              (head_dim 128 output rows that are only 8-byte aligned are routed to it; head_dim 512)
 *   svr_softmax_rows                           S 16 / ld_s % 4 (float4)     P 8 / ld_p % 4 (uint2)     ld_s, ld_p >= cols
 *   svr_rmsnorm_mod                            x 16, y 16 (dense rows, dim % 8 == 0); w / scale / shift element
 *   svr_unpatchify_euler                       element accesses only: pred, x_t, out 2-byte aligned, any ldp >= 4 * C
 *   svr_alpha_*                                element accesses only: any ld_px >= 3
 *   svr_pack_frames                            element alignment is enough (frames 4 / 2 bytes for fp32 / bf16, out 2 bytes for
 *                                              yuv420p10); 16-byte loads and stores where frames and out are 16-byte aligned (and,
 *                                              for yuv420p10, W % 16 == 0), element accesses otherwise
 *   svr_pack_yuv420p10                         as svr_pack_frames' yuv420p10: element alignment is enough; 16-byte loads and stores where
 *                                              frames and out are 16-byte aligned and W % 16 == 0, element accesses otherwise
 *   svr_pack_planar                            element alignment is enough (frames 4 / 2 bytes, out 2 bytes at 10 / 12 bits, 1 at 8);
 *                                              16-byte loads and 16- / 8-byte stores where frames and out are 16-byte aligned and
 *                                              W % 16 == 0, element accesses otherwise
 *   svr_unpack_frames                          element alignment is enough (packed 2 bytes for the 16-bit formats, out 4 bytes);
 *                                              16-byte loads and stores where packed and out are 16-byte aligned (and, for the
 *                                              yuv420p formats, W % 16 == 0), element accesses otherwise
 *   svr_dequant_gguf                           blocks 32 (GGUF's own alignment), out 16; anything else is refused
 *   svr_png_encode, svr_png_encode_runs        frames element alignment, scratch 16, sizes 8, out any (byte stores)
 *   svr_wavelet_reconstruct, svr_lab_*,        element accesses only: pixel operands by four element strides (input >= 0, output
 *     svr_chan_stats, svr_adain_apply          >= 1), planes and stats dense fp32; svr_chan_stats' workspace 8
 *   svr_sort_f32, svr_rank_match               operands 4 (dense [n]), workspace 16
 *   svr_hsv_planes, svr_hsv_merge,             as svr_lab_*: pixel operands by four element strides, planes dense fp32, element
 *     svr_adaptive_blend                       accesses only
 *   svr_hue_match                              planes 4 (dense [n]), workspace 16
 *   svr_frame_signatures                       element alignment is enough (frames 4 / 2 bytes for fp32 / bf16, sig 4); 16-byte loads
 *                                              where frames is 16-byte aligned, element accesses otherwise
 *   svr_active_profile                         as svr_frame_signatures (frames 4 / 2 bytes, out 4; 16-byte loads where frames is
 *                                              16-byte aligned, element accesses otherwise)
 *   svr_deinterlace                            element alignment is enough (2 bytes for the 16-bit formats); per plane, 16-byte loads and
 *                                              stores where packed, before, after and out are 16-byte aligned and the frame, the
 *                                              plane's offset and its rows are multiples of 16 bytes, element accesses otherwise
 *   svr_comb_counts                            element alignment is enough (2 bytes for the 16-bit formats, cnt 4); 16-byte loads where
 *                                              packed, before and after are 16-byte aligned and the frame and plane 0's rows are
 *                                              multiples of 16 bytes, element accesses otherwise
 *   svr_field_select                           as svr_deinterlace, deint counting as an input (cnt and modes 4, stats 8); per plane,
 *                                              16-byte loads and stores or element accesses by svr_deinterlace's rule
 *   svr_frame_diffs                            element alignment is enough (2 bytes for the 16-bit formats, diff 4); 16-byte loads where
 *                                              packed and before are 16-byte aligned and the frame and plane 0's rows are
 *                                              multiples of 16 bytes, element accesses otherwise
 *   svr_decimate_select                        element alignment is enough (2 bytes for the 16-bit formats, diff and drops 4, stats 8);
 *                                              16-byte loads and stores where packed and out are 16-byte aligned and the frame is a
 *                                              multiple of 16 bytes, element accesses otherwise
 *   svr_planar_codes                           element alignment is enough (2 bytes for the 10 / 12-bit planes and for out); 16-byte
 *                                              loads and stores where planes and out are 16-byte aligned and W % 16 == 0, element
 *                                              accesses otherwise
 */
#ifndef SEEDVR2_HIP_H
#define SEEDVR2_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v8 (round 5): svr_rmsnorm_mod takes SVR_STORE_H16 inputs; svr_gemm_bf16's persistent kernel serves the two h16 forms of the NaDiT's
 * residual stream (bias -> h16; gate * (acc + bias) + h16 residual -> h16); svr_qknorm_rope / svr_groupnorm_apply refuse NULL weights;
 * svr_set_option keys "gemm_asym", "gn_grid_cap", attn_variant 5..10 and gemm_w4r = 2 are gone (measured, deleted); "conv_thinout16" became "conv_thinout4" (1 default: N <= 4 thin-output
 * convs on conv_thinout4_kernel, 0: on the 32-cout kernel).  No signature changed.
 * v9 (round 6): + svr_mfma_calibrate() / svr_mfma_calibrate_workspace_bytes() (measurement aid, not on the data path); a thin-output
 * conv with N <= 4 couts accepts an exact [N, K] weight (the 4-row units take rows >= N from the zero page).  No signature changed.
 * v9, additive: + svr_alpha_workspace_bytes() / svr_alpha_stats() / svr_alpha_edges() / svr_alpha_refine() (edge-guided alpha
 * upscaling).  New symbols only -- nothing that existed changed, so the version number stays 9.
 * v9, additive: + svr_pack_frames() (output frames narrowed to rgb8 / bgr8 / yuv420p10 on the device).  A new symbol only.
 * v9, additive: + svr_dequant_gguf() (GGUF Q8_0 / Q4_K / Q5_K / Q6_K blocks expanded to bf16 / fp32 on the device).  A new symbol only.
 * v9, additive: + svr_unpack_frames() (packed input frames -- rgb8 / bgr8 / rgb16 / yuv420p8 / yuv420p10 as a decoder emits them --
 * widened to fp32 [T, H, W, C] on the device).  A new symbol only.
 * v9, additive: + svr_pack_yuv420p10() (yuv420p10 planes with a chosen matrix -- BT.709 / BT.601 / BT.2020 --, range and chroma
 * siting: what an HDR source is written with).  A new symbol only; svr_pack_frames and its bytes are untouched.
 * v9, additive: + svr_png_encode() / svr_png_encode_bytes() (output frames encoded as PNG zlib streams, 8 or 16 bits, on the
 * device).  New symbols only.
 * v9, additive: + svr_wavelet_reconstruct() / svr_lab_planes() / svr_lab_merge() / svr_chan_stats() / svr_adain_apply() and
 * svr_colorfix_workspace_bytes() (colour correction after the decode: wavelet, LAB and AdaIN on the device).  New symbols only.
 * v9, additive: + svr_sort_f32() / svr_rank_match() / svr_rank_workspace_bytes() / svr_rank_geometry() (a stable radix sort of fp32
 * keys and the rank matching of the LAB colour transfer on top of it).  New symbols only.
 * v9, additive: + svr_hsv_planes() / svr_hue_match() / svr_hue_match_workspace_bytes() / svr_hsv_merge() / svr_adaptive_blend() (the
 * HSV half of the colour correction: the `hsv` method and the HSV half and blend of `wavelet_adaptive`).  New symbols only.
 * v9, additive: + svr_png_encode_runs() / svr_png_encode_runs_bytes() (the PNG streams with run-length matches at distance 1; never
 * longer than svr_png_encode()'s).  New symbols only; svr_png_encode and its bytes are untouched.
 * v9, additive: + svr_frame_signatures() (per frame a 4 x 4 grid of 64-bin luma histograms: what cut detection compares).  A new
 * symbol only.
 * v9, additive: + svr_active_profile() (per row and per column the number of pixels brighter than a threshold: what finds the bars
 * of a letterboxed clip).  A new symbol only.
 * v9, additive: + svr_deinterlace() (the woven frames of an interlaced source made progressive on the packed planes, before
 * svr_unpack_frames widens them).  A new symbol only.
 * v9, additive: + svr_comb_counts() / svr_field_select() (field matching: per frame the combing of the three weaves its kept field
 * can make, and the frames copied from the first clean weave or from the deinterlaced clip).  New symbols only.
 * v9, additive: + svr_frame_diffs() / svr_decimate_select() (decimation: per frame the largest block sum of its difference from
 * the frame before it, and of every cycle of five frames the four that are not the smallest).  New symbols only.
 * v9, additive: + svr_planar_codes() (planar 4:2:0 / 4:2:2 / 4:4:4 sources of 8 / 10 / 12 bits, BT.709 / BT.601 / BT.2020, turned
 * into the 16-bit RGB codes svr_unpack_frames takes as SVR_UNPACK_RGB16).  A new symbol only; svr_unpack_frames is untouched.
 * v9, additive: + svr_pack_planar() (output frames as planar 4:2:0 / 4:2:2 / 4:4:4 of 8 / 10 / 12 bits, BT.709 / BT.601 / BT.2020, chroma
 * sited center, left or, for 4:2:0, topleft: what svr_planar_codes reads, written).  A new symbol only; svr_pack_frames and
 * svr_pack_yuv420p10 are untouched.
 * v9, clarification: the operand-layout contract above (alignment and pitch of every pointer + leading-dimension pair) is written
 * down and enforced on the host: a layout whose serving kernel would make a misaligned vector access, or whose pitch does not cover
 * its extent, is routed to a kernel with aligned accesses or refused before any launch instead of being launched as it was.  Dense,
 * allocator-aligned calls route exactly as before; a thin-output conv's exact [N, K] weight is honoured by the 32-cout kernel too
 * (couts >= N are staged from the zero page).  No signature changed. */
#define SVR_ABI_VERSION 9

/* ---- GEMM / implicit-GEMM convolution epilogues ------------------------------------------ */
/* Storage kinds of activation tensors that are NOT MFMA operands (svr_gemm_args.out_f32 / .resid_f32, the x_f32 arguments).
 * SVR_STORE_H16 (ABI v6): an IEEE half holding x * 2^-6 -- 11 significant bits for bf16's bytes, range +-4.2e6, absolute floor
 * 3.8e-6: the residual trunk of the VAE (ResnetBlock3D / attention outputs, attn_video_vae.py:311-362, 615-665), a block's conv1
 * output and (v8) the NaDiT's residual stream (mmsr_block.py:108-126): tensors read only by GroupNorm / RMSNorm and residual adds.
 * Every MFMA operand is bf16. */
#define SVR_STORE_BF16 0
#define SVR_STORE_FP32 1
#define SVR_STORE_H16  2

#define SVR_EPI_BIAS        0   /* C = acc + bias                                              */
#define SVR_EPI_BIAS_SILU   1   /* C = silu(acc + bias)                 embedding.py:56-61     */
#define SVR_EPI_RESID_GATE  2   /* C = resid + gate * (acc + bias)      mmsr_block.py:108-109,
                                   125-126 (AdaSingle "out" + residual); attn_video_vae.py:360 */
#define SVR_EPI_BIAS_GELU   4   /* C = gelu_tanh(acc + bias)            dit_7b/mlp.py:36-41    */
#define SVR_EPI_SWIGLU      3   /* C[:, h] = silu(acc[:, gate h]) * acc[:, in h]; W rows are
                                   interleaved in blocks of 16 (gate16 | in16)  mlp.py:60-61   */

typedef struct svr_conv_geom {
    int32_t enabled;            /* 0: plain GEMM, A is [M, K]                                  */
    int32_t T, H, W, Cin;       /* input  [T, H, W, Cin]                                       */
    int32_t To, Ho, Wo;         /* output [To, Ho, Wo, N];  M = To*Ho*Wo                       */
    int32_t kt, kh, kw;         /* kernel taps; W is [Npad, kt*kh*kw*Cin], tap-major, Cin minor */
    int32_t st, sh, sw;         /* strides                                                     */
    int32_t pt, ph, pw;         /* front pads: pt causal head frames, ph/pw zero pad (low side;
                                   reads past H/W on the high side are zero too)               */
    int32_t halo_frames;        /* frames in `halo` (previous temporal slice tail), 0 = none   */
    const void* halo;           /* bf16 [halo_frames, H, W, Cin] or NULL: replicate frame 0
                                   (causal_inflation_lib.py:422-437 extend_head / :260-278)    */
    const void* zeros;          /* >= 16 zero bytes on the device (spatial padding source)     */
} svr_conv_geom;

typedef struct svr_pixel_shuffle {
    int32_t enabled;            /* scatter-store epilogue of Upsample3D.upscale_conv:
                                   "b (x y z c) f h w -> b c (f z) (h x) (w y)"
                                   attn_video_vae.py:137-143, + remove_head :152-153           */
    int32_t F, H, W;            /* input grid (M = F*H*W)                                      */
    int32_t rz;                 /* temporal ratio 1 | 2 (spatial ratio is always 2)            */
    int32_t C;                  /* output channels (N = 4*rz*C)                                */
    int32_t drop_first;         /* 1: drop the duplicated 2nd output frame (first slice only)  */
} svr_pixel_shuffle;

typedef struct svr_phase_scatter {
    int32_t enabled;            /* conv mode, stride 1: this launch computes ONE output phase of a 2x spatially upsampled
                                   grid ("sub-pixel convolution"): output voxel (to, yo, xo) of the conv is stored at
                                   C[to * t_stride][2*yo + py][2*xo + px][n], C dense [*, 2*Ho, 2*Wo, N] (the caller offsets C to
                                   the first frame of the launch).  Used to run Upsample3D's 1x1x1 upscale_conv + pixel
                                   shuffle + 3x3x3 conv (attn_video_vae.py:110-174) as (kt', 2, 2)-tap convs over the
                                   LOW-resolution input with merged weights: four spatial phases, and for a temporal
                                   upsampler two temporal phases (t_stride 2) interleaving their frames.              */
    int32_t py, px;             /* 0 | 1                                                                              */
    int32_t t_stride;           /* 1 | 2: output frames between consecutive conv output frames                        */
    const float* bias_border;   /* fp32 [3][N] or NULL: bias used INSTEAD of `bias` on the voxels whose window loses its
                                   border tap to the zero padding of the upsampled grid -- row yo == (py ? Ho-1 : 0):
                                   [0]; column xo == (px ? Wo-1 : 0): [1]; both: [2]                                  */
    int32_t quad;               /* 1 (ABI v6): ONE launch computes all four spatial phases -- phase p = py * 2 + px takes its
                                   fragment-ordered weights, bias and border bias from the arrays below and its spatial pads
                                   (1 - py, 1 - px); py / px / bias_border above, conv.ph / conv.pw, W_frag and bias of the
                                   launch are ignored.  The phase is the FASTEST index of the tile order, so the four
                                   workgroups that stage the same low-resolution halo run next to each other on one XCD
                                   (three of the four stagings come from L2 instead of HBM).  Served by the sub-pixel conv
                                   kernel only (svr_gemm_kernel_class() == SVR_KERNEL_CONV_SUBPIXEL), refused otherwise.   */
    int32_t reserved_;
    const void* W_frag4[4];
    const float* bias4[4];
    const float* bias_border4[4];
} svr_phase_scatter;

typedef struct svr_gemm_args {
    const void* A;  int64_t lda;        /* bf16 [M, K] (ignored rows/K layout when conv.enabled: A = input tensor); lda >= K.
                                           Alignment of every operand below: "Operand layouts" at the top of this file     */
    const void* W;                      /* bf16 [Npad, K] row-major (nn.Linear layout), K % 64 == 0,
                                           Npad = N rounded up to the tile width (128)                       */
    void* C;        int64_t ldc;        /* bf16 (or fp32 if out_f32) [M, N(/2 for SWIGLU)]; ldc >= N (N / 2); ignored
                                           (dense output) with ps / phase                                      */
    int32_t M, N, K;
    const float* bias;                  /* fp32 [N] or NULL                                                    */
    const float* gate;                  /* fp32 [N] or NULL (=1)            SVR_EPI_RESID_GATE                 */
    const void* resid; int64_t ldr;     /* bf16 [M, N] or NULL (may alias C, then with ldr == ldc) SVR_EPI_RESID_GATE;
                                           ldr >= N                                                            */
    int32_t epilogue;
    int32_t out_f32;
    svr_conv_geom conv;
    svr_pixel_shuffle ps;
    /* Optional fused GroupNorm statistics of the STORED output (conv mode, N = channel count): when the
     * launch is served by the LDS-halo conv kernel (svr_gemm_gn_blocks(args) > 0) every workgroup writes
     * the (sum, sum of squares) of its patch per group to gn_partial[frame][block][group] (fp64 pairs,
     * svr_gemm_gn_blocks() blocks per frame); svr_groupnorm_reduce() turns them into `stats`.  Fixed
     * reduction order and fp64 accumulation from the first add on, like svr_groupnorm_stats (same accuracy
     * guarantee).  NULL / 0: off.                                                                         */
    void* gn_partial;
    int32_t gn_groups;
    /* Optional (conv mode, 3x3 spatial taps, stride 1, Cin % 32 == 0, N % 128 == 0): the same weights in
     * MFMA-fragment order as written by svr_conv_pack_frag().  When set, the LDS-halo conv kernel streams the
     * weights from this copy straight into registers instead of staging W through LDS.  NULL: off.
     * Plain GEMMs (ABI v7): the copy written by svr_gemm_pack_frag().  When set and the problem is served by the persistent
     * GEMM kernel (svr_gemm_kernel_class() == SVR_KERNEL_GEMM_PERSISTENT), that kernel streams the weights from it into
     * registers and only the activations pass through LDS (by LDS-DMA); same results, bit for bit.  Ignored by every other
     * plain-GEMM kernel. */
    const void* W_frag;
    svr_phase_scatter phase;            /* conv mode only; not together with ps / SWIGLU / resid                        */
    int32_t resid_f32;                  /* 1: `resid` is fp32 [M, N] (ldr in elements).  Wide residual trunk (ABI v5): with out_f32
                                           the skip path of ResnetBlock3D (attn_video_vae.py:311-362) / the NaDiT residual stream
                                           (mmsr_block.py:108-126) is carried in fp32 and only MFMA operands are rounded to bf16 */
} svr_gemm_args;

/* W [N, K = kt * 9 * Cin] (conv weight rows, K order (dt, dy, dx, c)) -> out (same byte size, N * K bf16) in the
 * fragment order svr_gemm_args.W_frag expects.  N % 32 == 0, Cin % 32 == 0.  Done once per checkpoint.     */
int svr_conv_pack_frag(const void* W, void* out, int32_t N, int32_t K, int32_t kt, int32_t Cin, void* stream);

/* W [N, K] (plain GEMM weight rows, N % 128 == 0 -- rows past the problem's N zero-filled --, K % 64 == 0) -> out (same byte
 * size) in the fragment order a plain GEMM's svr_gemm_args.W_frag expects: 16-byte unit
 * (((n / 128) * (K / 32) + k / 32) * 8 + (n % 128) / 16) * 64 + lane holds W[(n & ~15) + (lane & 15)][(k & ~31) + (lane >> 4) * 8 .. + 7],
 * the first operand of v_mfma_f32_16x16x32_bf16.  Done once per checkpoint (replaces nothing in the reference: its nn.Linear weights,
 * src/models/dit_3b/nablocks/attention/mmattn.py:173,207-208,269 and mlp.py:60-61, have no kernel-side layout).  ABI v7.          */
int svr_gemm_pack_frag(const void* W, void* out, int32_t N, int32_t K, void* stream);

/* Same for any spatial tap grid (K = kt * kh * kw * Cin, K order (dt, dy, dx, c)): kh = kw = 3 is svr_conv_pack_frag; kh = kw = 2
 * feeds the sub-pixel upsampler conv kernel (stride 1, pads 0 | 1, same-size output, N % 128 == 0, plain bias epilogue,
 * with or without svr_gemm_args.phase).                                                                        */
int svr_conv_pack_frag_taps(const void* W, void* out, int32_t N, int32_t K, int32_t kt, int32_t kh, int32_t kw, int32_t Cin,
                            void* stream);

/* Number of per-frame partial blocks the launch described by `args` will write to args->gn_partial
 * (0: the kernel that serves this problem does not produce fused statistics -- use svr_groupnorm_stats). */
int32_t svr_gemm_gn_blocks(const svr_gemm_args* args);

/* Which kernel svr_gemm_bf16 would launch for `args` (no launch): one of SVR_KERNEL_*, or -1 with svr_last_error() set when
 * svr_gemm_bf16 would refuse the arguments.  ABI v6.  bench.py attributes launch times to kernels with it (the `roofline`
 * object is the SVR_KERNEL_CONV_HALO launches only), tests pin it on the shapes a VAE tile issues.
 * One class depends on the DEVICE: SVR_KERNEL_GEMM_PERSISTENT needs at least 8 compute units (one workgroup per CU in multiples of
 * the 8 XCDs; a smaller partition gets SVR_KERNEL_GEMM), and this function reads the CU count of the calling thread's CURRENT
 * device (256 when there is no GPU), whereas svr_gemm_bf16 launches on the device of its stream.  Callers that attribute by it
 * (bench.py) make the stream's device current first, as torch.cuda.set_device does; every other class is a function of `args` alone. */
#define SVR_KERNEL_NONE            0   /* empty problem: nothing is launched                                           */
#define SVR_KERNEL_GEMM            1   /* gemm_kernel (eight waves, 256x256 / 256x128 tiles)                           */
#define SVR_KERNEL_GEMM_PERSISTENT 2   /* gemm_w4r_kernel / gemm_w4q_kernel (persistent four-wave workgroups, the NaDiT's big GEMMs; with / without W_frag) */
#define SVR_KERNEL_CONV_HALO       3   /* conv_halo2_kernel: stride-1 3x3 spatial taps, LDS halo (the dominant kernel) */
#define SVR_KERNEL_CONV_SUBPIXEL   4   /* conv_sub_kernel: (kt, 2, 2)-tap phases of the sub-pixel upsamplers           */
#define SVR_KERNEL_CONV_THIN_IN    5   /* conv_halo2_kernel<8, thin>: Cin = 4 (encoder.conv_in)                        */
#define SVR_KERNEL_CONV_THIN_OUT   6   /* conv_thinout4_kernel (Cout <= 4) / conv_thinout_kernel (Cout <= 32): conv_out */
#define SVR_KERNEL_CONV_GENERIC    7   /* gemm_kernel in conv mode: strided / 1x1x1 / everything else                  */
int32_t svr_gemm_kernel_class(const svr_gemm_args* args);
const char* svr_gemm_kernel_name(int32_t kernel_class);

/* nn.Linear / F.conv3d replacement (MFMA bf16, fp32 accumulate).
 * Replaces: every nn.Linear in src/models/dit_3b (mmattn.py:173,269; mlp.py:60-61; patch_v1.py:96,113;
 * embedding.py:56-61; nadit.py:211) and InflatedCausalConv3d.forward (causal_inflation_lib.py:213-305). */
int svr_gemm_bf16(const svr_gemm_args* args, void* stream);

/* ---- DiT elementwise / normalisation ------------------------------------------------------- */
/* y = rms_norm(x) [* w] * scale + shift, per row.  normalization.py:88-109 + modulation.py:110.
 * x [rows, dim] of storage kind x_f32 (SVR_STORE_BF16 | _FP32 | _H16: the NaDiT's residual stream is wide), y bf16; w (affine
 * weight) / scale / shift fp32 [dim] or NULL. */
int svr_rmsnorm_mod(const void* x, void* y, int64_t rows, int32_t dim, float eps,
                    const float* w, const float* scale, const float* shift, int32_t x_f32, void* stream);

/* mod[l][i] = emb[i*stride + off(l)] + param[l][i]: builds the fused AdaSingle vectors
 * (scaleA+scaleB, shiftA+shiftB, gateA+gateB).  modulation.py:76,88-113.
 * emb bf16 [dim*6] viewed "(d l g)"; params bf16 [n_vec, dim]; slot[n_vec] = l*3+g; out fp32.    */
int svr_ada_combine(const void* emb, const void* params, const int32_t* slot, float* out,
                    int32_t n_vec, int32_t dim, void* stream);

/* In-place q/k RMSNorm(head_dim, affine) + 3-axis interleaved-pair RoPE on a packed qkv buffer.
 * mmattn.py:207-208 + rope.py:118-126,172-173.  qkv bf16 [rows, 3*heads*128]; pos int16 [rows,3];
 * cs fp32 [n_pos, 2, 63] = cos|sin(pos * freq) table per axis is folded on the host into one
 * table indexed by position; wq,wk fp32 [128]; t_offset is added to pos[:,0] (text length).
 * Every table row index -- pos[:,0] + t_offset, pos[:,1], pos[:,2] -- is CLAMPED to [0, n_pos - 1]: a position outside
 * the table takes the first / last row's cos | sin, it is never read out of bounds and never an error.
 * Pairs 3 * n_freq .. 63 of a head vector are normalised and pass through unrotated.                 */
int svr_qknorm_rope(void* qkv, int64_t rows, int32_t heads, const int16_t* pos, int32_t t_offset,
                    const float* cos_tab, const float* sin_tab, int32_t n_pos, int32_t n_freq,
                    const float* wq, const float* wk, float eps, void* stream);

/* Variable-length window attention, softmax(q k^T / sqrt(d)) v per window.  attention.py:27-64,
 * mmattn.py:245-264 (gather by window, text rows appended to every window, scatter back).
 * qkv bf16 [*, 3*heads*D] (q|k|v); seq_rows int32 [total] = source row of each window position;
 * out_rows int32 [total] = destination row in `out` (bf16 [*, heads*D]); cu int32 [n_seq+1].
 * ld_qkv >= 3*heads*D, ld_out >= heads*D; alignment: "Operand layouts" above.
 * Size limit: the window kernel (head_dim 128, max_len <= 2048) keeps each window row's byte offset
 * seq_rows[i] * ld_qkv * 2 in 16-byte units in 32 bits, so every row that seq_rows names must start below
 * byte 2^36 (64 GiB) of qkv.  A row beyond that would wrap silently: the row indices are device data, the
 * launcher cannot see them.  (The largest qkv of the 7B model, 65 frames at 4K, is 10.2 GB.)          */
int svr_attn_varlen(const void* qkv, int64_t ld_qkv, void* out, int64_t ld_out,
                    const int32_t* seq_rows, const int32_t* out_rows, const int32_t* cu,
                    int32_t n_seq, int32_t max_len, int32_t heads, int32_t head_dim, float scale,
                    void* stream);

/* dst[j] = mean_w src[w*n_txt + j] (text outputs coalesced over windows, na.py:396-417).          */
int svr_rows_mean(const void* src, void* dst, int32_t n_groups, int32_t rows_per_group, int32_t dim,
                  void* stream);

/* patchify "(T t)(H h)(W w) c -> T H W (t h w c)" (t,h,w = 1,2,2), zero-padded to kpad columns.
 * patch_v1.py:91.  in bf16 [T,H,W,C] -> out bf16 [T*(H/2)*(W/2), kpad]                             */
int svr_patchify(const void* in, void* out, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kpad,
                 void* stream);

/* un-patchify + one-step Euler endpoint x0 = x_t - pred  (patch_v1.py:119-123, euler.py:60-63,
 * schedules/base.py:108-110 with A=0,B=1).  pred bf16 [T*(H/2)*(W/2), ldp] (first 4*C cols),
 * x_t bf16 [T,H,W,C] -> out bf16 [T,H,W,C]; x_t NULL -> out = pred.                                */
int svr_unpatchify_euler(const void* pred, int64_t ldp, const void* x_t, void* out,
                         int32_t T, int32_t H, int32_t W, int32_t C, void* stream);

/* ---- VAE elementwise ------------------------------------------------------------------------- */
/* Per-frame GroupNorm statistics over NDHWC.  causal_inflation_lib.py:366-408.
 * x bf16 (fp32 if x_f32) [T, HW, C]; stats fp64 [T, groups, 2] (sum, sumsq), fully overwritten.  Reductions run in a
 * fixed order (no atomics): bit-reproducible, independent of temporal slicing.  `workspace` is a
 * caller-provided scratch of svr_groupnorm_workspace_bytes(T, HW, groups) bytes.
 * Accuracy: svr_groupnorm_apply forms var = sumsq / n - (sum / n)^2, which cancels rho^2 = (mean / std)^2 of the
 * sums' digits.  The sums are therefore accumulated in fp64 from the first add on (a stored value and its square are
 * exact in fp64; here and in the statistics fused into the conv epilogues, svr_gemm_args.gn_partial), so that
 *     |var - var_exact| <= 2^-9 (var_exact + eps)   -- rstd to 2^-10, a quarter of one bf16 store roundoff --
 * holds for every group with |mean| / std <= 1024 (and far beyond: the error is ~ n_chain 2^-53 rho^2), var_exact the
 * two-pass variance of the stored values; a constant group gives var = 0, never a negative value.
 * tests/test_gpu_conditioning.py holds both paths to it.                                            */
int64_t svr_groupnorm_workspace_bytes(int32_t T, int64_t HW, int32_t groups);
int svr_groupnorm_stats(const void* x, double* stats, void* workspace, int32_t T, int64_t HW, int32_t C,
                        int32_t groups, int32_t x_f32, void* stream);
/* stats[t][g] = fixed-order sum over the `nblk` block partials [T][nblk][groups] (fp64 pairs) written by
 * svr_groupnorm_stats' first stage or by a conv launch with gn_partial set.                           */
int svr_groupnorm_reduce(const void* partial, double* stats, int32_t T, int32_t nblk, int32_t groups, void* stream);
/* y = [silu](gamma * (x - mean) * rstd + beta); x bf16 (fp32 if x_f32), y bf16.  attn_video_vae.py:316-323,343-350.
 * Any C % 8 == 0, C <= 512 with groups dividing C -- a superset of what svr_groupnorm_stats serves (C / 8 dividing 256):
 * for the other C (24, 192, 320, ...) the caller brings statistics of its own.                                          */
int svr_groupnorm_apply(const void* x, void* y, const double* stats, const float* gamma, const float* beta,
                        int32_t T, int64_t HW, int32_t C, int32_t groups, float eps, int32_t apply_silu,
                        int32_t x_f32, void* stream);
/* P[r, :] = softmax(scale * S[r, :]): fp32 scores [rows, cols] (ld_s) -> bf16 probabilities (ld_p); cols <= 65536.
 * The softmax of the VAE mid-block attention (diffusers Attention, 1 head x 512; attn_video_vae.py:659-665) when it is
 * run as two MFMA GEMMs around a materialised score matrix.                                            */
int svr_softmax_rows(const float* S, void* P, int64_t rows, int32_t cols, int64_t ld_s, int64_t ld_p, float scale,
                     void* stream);
/* im2col for thin-input causal convs (Cin = 3 / 16): out bf16 [To*Ho*Wo, kpad].                    */
int svr_im2col_causal(const void* in, void* out, const svr_conv_geom* g, int32_t kpad, void* stream);
/* acc[T, y0:y0+h, x0:x0+w, C] += tile * wy[h] * wx[w]  (fp32 accumulator; tiled_encode/decode
 * blending, attn_video_vae.py:1445-1457, 1606-1619) and cnt[y, x] += wy*wx.                       */
int svr_blend_accumulate(const void* tile, float* acc, float* cnt, const float* wy, const float* wx,
                         int32_t T, int32_t h, int32_t w, int32_t C, int32_t H, int32_t W,
                         int32_t y0, int32_t x0, void* stream);
/* out[..., :c_take] = (acc / max(cnt, 1e-6) - shift) * scale -> bf16.  attn_video_vae.py:1463 + infer.py:188. */
int svr_blend_finalize(const float* acc, const float* cnt, void* out, int32_t T, int64_t HW, int32_t C,
                       int32_t c_take, float scale, float shift, void* stream);
/* out[r, :c_out] = (in[r, :c_out] - shift) * scale   (latent (de)scaling + mean slice, infer.py:188, 236). */
int svr_affine_slice(const void* in, void* out, int64_t rows, int32_t c_in, int32_t c_out,
                     float scale, float shift, void* stream);

/* ---- edge-guided alpha upscaling ----------------------------------------------------------- */
/* alpha_upscaling.py:289-438 edge_guided_alpha_upscale(method='guided') for one batch of frames, after the bicubic base
 * (F.interpolate, torch glue): rgb [T, H, W, >= 3] (fp32 or bf16: rgb_kind SVR_STORE_FP32 / SVR_STORE_BF16; ld_px elements from
 * one pixel to the next, frames dense) is the UPSCALED clip in [-1, 1] or [0, 1], alpha_lo the n_alpha input-resolution alpha
 * values (fp32), base the bicubic upsample [T, H, W] fp32, out [T, H, W] fp32.  Call the three in this order on one stream; no call
 * synchronises with the host: what the data decides (binary matte or not = radius 2 + snapping or radius 3, whether the rgb is
 * normalised (x + 1) / 2 once (min < 0) and, for the edge detector only, twice (min < -1), each frame's Sobel maximum) is left in
 * `workspace` by one kernel and read there by the next.  Integer atomics only: same bits on every run.
 * workspace: svr_alpha_workspace_bytes(T, H, W) bytes of device memory, [flags: int32 x 4 | maxima: int32 x T (padded to 4) |
 * n map: int32 x T*H*W]; every call checks workspace_bytes against it.  1 <= T <= 65535, H >= 2, W >= 2 (BORDER_REFLECT_101).  */
int64_t svr_alpha_workspace_bytes(int32_t T, int32_t H, int32_t W);
/* flags = {count(alpha_lo < 0.1), count(alpha_lo > 0.9), min(rgb) < 0, min(rgb) < -1}; clears the maxima. */
int svr_alpha_stats(const float* alpha_lo, int64_t n_alpha, const void* rgb, int32_t T, int32_t H, int32_t W, int64_t ld_px,
                    int32_t rgb_kind, void* workspace, int64_t workspace_bytes, void* stream);
/* detect_edges_batch (:125-188) up to the division: u8 = trunc(clip(x * 255, 0, 255)), OpenCV's 8-bit RGB2GRAY, 3x3 Sobel with
 * BORDER_REFLECT_101, n = sx^2 + sy^2 -> n map; per-frame max(n) -> maxima. */
int svr_alpha_edges(const void* rgb, int32_t T, int32_t H, int32_t W, int64_t ld_px, int32_t rgb_kind, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* guided filter (:191-286; zero-padded box means, radius 2 / eps 0.002 for a binary matte, else radius 3) of `base` guided by the
 * channel mean of the once-normalised rgb, then steps 3-8 (:370-408) for a binary matte, clamp(0, 1) -> out.  The edge byte
 * trunc(sqrt(n) / sqrt(max n) * 255) (fp64; 0 on a constant frame) goes to edge_out [T, H, W] uint8 unless that is NULL. */
int svr_alpha_refine(const void* rgb, const float* base, float* out, uint8_t* edge_out, int32_t T, int32_t H, int32_t W,
                     int64_t ld_px, int32_t rgb_kind, int64_t n_alpha, const void* workspace, int64_t workspace_bytes, void* stream);

/* ---- packed output frames ------------------------------------------------------------------- */
/* frameio.py (the specification, bit for bit): frames [T, H, W, C] dense, fp32 or bf16 (x_kind SVR_STORE_FP32 / SVR_STORE_BF16),
 * nominally in [0, 1], C = 3 or 4 -> out:
 *   SVR_PACK_RGB8 / SVR_PACK_BGR8   uint8 [T, H, W, C]: rint(clamp(x, 0, 1) * 255) (ties to even); BGR8 swaps channels 0 and 2, a
 *                                   fourth channel stays in place.  out_bytes = T*H*W*C.
 *   SVR_PACK_YUV420P10              C = 3 only.  uint16 [T, H*W + 2*h2*w2], h2 = ceil(H/2), w2 = ceil(W/2): per frame the Y plane,
 *                                   then Cb, then Cr (ffmpeg's yuv420p10le), BT.709 limited range in exact integers from
 *                                   q = rint(clamp(x, 0, 1) * 65535); chroma from the sums over 2 x 2 blocks, rows / columns beyond
 *                                   the frame repeating the last one.  out_bytes = 2 * T * (H*W + 2*h2*w2).
 * NaN -> code 0, +inf -> full scale, -inf -> 0.  Every argument is checked before the launch (T * H * W <= 2^40 pixels); out_bytes
 * must be EXACTLY the size above.  One launch on `stream`, no host synchronisation, no workspace. */
#define SVR_PACK_RGB8      0
#define SVR_PACK_BGR8      1
#define SVR_PACK_YUV420P10 2
int svr_pack_frames(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t fmt, void* out,
                    int64_t out_bytes, void* stream);

/* ---- yuv420p10 planes with a chosen matrix, range and chroma siting ----------------------------- */
/* frameio.pack_yuv420p10_torch (the specification, bit for bit): frames [T, H, W, 3] dense, fp32 or bf16 (x_kind SVR_STORE_FP32 /
 * SVR_STORE_BF16), nominally in [0, 1] -> out uint16 [T, H*W + 2*h2*w2] in SVR_PACK_YUV420P10's plane layout (Y, Cb, Cr per frame;
 * h2 = ceil(H/2), w2 = ceil(W/2)).  Exact integers from q = rint(clamp(x, 0, 1) * 65535), D = 65535 * 65536:
 *   range   SVR_COLOUR_RANGE_TV: y0 = 64, ys = 876, cs = 896;  SVR_COLOUR_RANGE_PC: y0 = 0, ys = cs = 1023.
 *   matrix  Kr / Kb 0.2126 / 0.0722 (BT709), 0.299 / 0.114 (BT601), 0.2627 / 0.0593 (BT2020), every weight rounded to nearest at 2^16,
 *           the luma deficit to green; as wr, wg, wb | cb_r, cb_g | cr_g, cr_b:
 *             BT709   13933, 46871, 4732 |  -7509, -25259 | -29763, -3005
 *             BT601   19595, 38470, 7471 | -11058, -21710 | -27439, -5329
 *             BT2020  17216, 44434, 3886 |  -9151, -23617 | -30133, -2635
 *   luma    Y = y0 + (ys * (wr r + wg g + wb b) + D/2) / D.
 *   siting  sr, sg, sb = weighted sums of q, total weight S, indices clamped to the frame.  SVR_COLOUR_SITING_CENTER: the 2 x 2
 *           block, weights 1, S = 4.  SVR_COLOUR_SITING_LEFT: rows 2j, 2j+1, columns 2k-1, 2k, 2k+1 with weights 1, 2, 1, S = 8
 *           (chroma co-sited with even luma columns: the H.264 / HEVC default, what svr_unpack_frames assumes).
 *   chroma  Cb = min((S * 512 * D + cs * (cb_r sr + cb_g sg + 32768 sb) + S * D/2) / (S * D), 1023), Cr with (32768, cr_g, cr_b).
 * (BT709, TV, CENTER) gives the bytes of svr_pack_frames' SVR_PACK_YUV420P10.  NaN -> code 0, +inf -> full scale, -inf -> 0.
 * Every argument is checked before the launch (T * H * W <= 2^40 pixels); out_bytes must be EXACTLY 2 * T * (H*W + 2*h2*w2).  One
 * launch on `stream`, no host synchronisation, no workspace. */
#define SVR_COLOUR_MATRIX_BT709  0
#define SVR_COLOUR_MATRIX_BT601  1
#define SVR_COLOUR_MATRIX_BT2020 2
#define SVR_COLOUR_RANGE_TV 0
#define SVR_COLOUR_RANGE_PC 1
#define SVR_COLOUR_SITING_CENTER 0
#define SVR_COLOUR_SITING_LEFT   1
int svr_pack_yuv420p10(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t matrix, int32_t range,
                       int32_t siting, void* out, int64_t out_bytes, void* stream);

/* ---- frame signatures for cut detection ---------------------------------------------------------- */
/* shots.py (the specification, bit for bit): frames [T, H, W, C] dense, fp32 or bf16 (kind SVR_STORE_FP32 / SVR_STORE_BF16), C = 3 or
 * 4 (a fourth channel is ignored), H >= 4, W >= 4, H * W < 2^31 -> sig int32 [T, 1024], indexed [cell_row * 4 + cell_col][bin]: the
 * number of pixels of frame t with cell_row = (y * 4) / H, cell_col = (x * 4) / W and bin = Y8 >> 2, where
 *   q  = rint(clamp(x, 0, 1) * 255) per channel (ties to even; NaN -> 0, +inf -> 255, -inf -> 0)
 *   Y8 = (13933 r + 46871 g + 4732 b + 32768) >> 16          (the BT.709 luma weights of SVR_PACK_YUV420P10; 0..255).
 * Every row of sig sums to H * W.  The call itself zeroes sig on `stream` (what the buffer held does not matter), then one launch
 * adds the counts with integer atomics: two calls give the same bits.  Every argument is checked before anything is enqueued;
 * sig_bytes must be EXACTLY T * 4096.  No host synchronisation, no workspace. */
int svr_frame_signatures(const void* frames, int32_t kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t* sig,
                         int64_t sig_bytes, void* stream);

/* ---- active-area profile of a letterboxed clip -------------------------------------------------- */
/* active.py (the specification, bit for bit): frames [T, H, W, C] dense, fp32 or bf16 (kind SVR_STORE_FP32 / SVR_STORE_BF16), C = 3 or
 * 4 (a fourth channel is ignored), T, H, W >= 1, T * max(H, W) < 2^31, dark in 0..255 -> out int32 [H + W]: out[y] for y < H is the
 * number of pixels (t, x) of row y, over all T frames, with Y8 > dark, out[H + x] the same for column x; Y8 as for
 * svr_frame_signatures.  Both halves have the same sum.  The call itself zeroes out on `stream` (what the buffer held does not
 * matter), then one launch adds the counts with integer atomics: two calls give the same bits.  Every argument is checked before
 * anything is enqueued; out_bytes must be EXACTLY (H + W) * 4.  No host synchronisation, no workspace. */
int svr_active_profile(const void* frames, int32_t kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t dark, int32_t* out,
                       int64_t out_bytes, void* stream);

/* ---- PNG streams encoded on the device ------------------------------------------------------- */
/* pngenc.py (the specification, byte for byte): frames [T, H, W, C] dense, fp32 or bf16 (x_kind SVR_STORE_FP32 / SVR_STORE_BF16),
 * C = 3 or 4, depth 8 or 16 -> per frame ONE zlib stream, out + t * out_capacity, of sizes[t] bytes (int64 [T], on the device):
 * samples q = rint(clamp(x, 0, 1) * 255 | 65535) (NaN -> 0; 16-bit samples big-endian), each row filtered with the PNG filter type
 * 0..4 of least sum of (f < 128 ? f : 256 - f), a tie to the lowest type; segments of R = max(1, 65536 / stride) rows, stride =
 * 1 + W * C * depth / 8, each ONE dynamic-Huffman deflate block of literals only (lengths by the two-queue construction, counts
 * halved -- (c + 1) >> 1 -- while the tree is deeper than 15; 1106 header bits) followed by an empty stored block; 78 01 in front,
 * 03 00 and the big-endian Adler-32 behind.  pngenc.png_file() frames a stream as a file on the host.
 * svr_png_encode_bytes(): the scratch bytes a call needs and the capacity every frame's slot of `out` must have: 2 + 6 + the sum
 * over the frame's segments of n filtered bytes each of 139 + ceil(15 (n + 1) / 8) + 5 (pngenc.frame_bound).
 * svr_png_encode(): every argument is checked before the first launch (C, depth, T / H / W >= 1, H <= 2^24, W * bytes per pixel
 * < 2^24, T * H < 2^31, scratch 16-byte and sizes 8-byte aligned, scratch_bytes and out_capacity at least what
 * svr_png_encode_bytes() says).  Three launches on `stream`, no host synchronisation.  Bytes of a frame's slot past sizes[t] are
 * not written.  Vector stores and LDS integer atomics only; the result does not depend on scheduling. */
int svr_png_encode_bytes(int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, int64_t* scratch_bytes, int64_t* capacity);
int svr_png_encode(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, void* scratch,
                   int64_t scratch_bytes, void* out, int64_t out_capacity, int64_t* sizes, void* stream);
/* The same with run-length matches (pngenc.py "Runs", encode_frames_spec(..., runs=True), byte for byte): a segment's bytes split
 * into maximal runs of one byte; a run longer than 3 is a literal, matches of up to 258 bytes at DISTANCE 1 and at most two more
 * literals; a second code over 286 symbols (the same construction; one distance code of length 1; 1222 header bits); per segment
 * the run block is written iff it has a match and is strictly smaller in bits than the literal block, else the literal block of
 * svr_png_encode().  So no stream is longer than svr_png_encode()'s, a frame without a useful run gives the same bytes, and the
 * capacity is the same; the scratch is larger (svr_png_encode_runs_bytes()).  Same arguments, same checks, same guarantees; four
 * launches on `stream`. */
int svr_png_encode_runs_bytes(int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, int64_t* scratch_bytes, int64_t* capacity);
int svr_png_encode_runs(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, void* scratch,
                        int64_t scratch_bytes, void* out, int64_t out_capacity, int64_t* sizes, void* stream);

/* ---- colour correction ------------------------------------------------------------------------ */
/* colorfix.py (the specification; src/utils/color_fix.py).  Pixel operands are fp32 (kind = SVR_STORE_FP32, the only kind served)
 * and indexed [T, 3, H, W]: element (t, c, y, x) lies at strides[0] * t + strides[1] * c + strides[2] * y + strides[3] * x ELEMENTS
 * from the pointer (`*_strides`: int64 [4] on the host), so channels-last frames ({H*W*3, 1, W*3, 3}) and a slice of a [C, T, H, W]
 * buffer are read where they lie.  Input strides are >= 0, output strides >= 1; an output's elements must not overlap and only
 * its T * 3 * H * W addressed elements are written.  Every argument is checked before the first launch (a null pointer or stride
 * array, a bad stride, kind, 1 <= T <= 21845, H >= 1, W >= 1, T * H * ceil(W / 256) < 2^24, a short workspace) and
 * svr_last_error() names it.  All launches go to `stream`, none synchronises with the host; plain vector stores, no atomics: the
 * same bits on every run.
 * svr_wavelet_reconstruct(): out = clamp(high5(content) + low5(style), -1, 1), colorfix.wavelet_reconstruction BIT FOR BIT: five
 *   levels, level i with radius min(2^i, max(1, min(H, W) / 8)), each blur (x[y - r] + x[y + r]) * 0.25 + 0.5 * x[y] down the
 *   rows, then the same along them, indices clamped to the image; high = (high + image) - low from zero.  One launch.
 * svr_lab_planes(): base, style in [-1, 1] -> ((x + 1) * 0.5) clamped to [0, 1] -> CIELAB (D65) as colorfix.rgb_to_lab orders it
 *   -> c_lab, s_lab: dense planar fp32 [3, T*H*W] (L, a, b).  One launch.
 * svr_lab_merge(): c_L, m_L, m_a, m_b dense fp32 [T*H*W]; L = c_L * w + m_L * (1 - w) with w = luminance_weight (both factors
 *   rounded to fp32 from fp64); for w >= 1, L = c_L and m_L is not read (may be NULL); colorfix.lab_to_rgb, clamped to [0, 1],
 *   * 2 - 1 -> out.  One launch.
 * svr_chan_stats(): stats fp32 [T, 3, 4] = {mean, unbiased variance} of content, then of style, per frame and channel; fp64 sums in
 *   a fixed order.  workspace: svr_colorfix_workspace_bytes(T) bytes of device memory, 8-byte aligned.  Two launches.
 * svr_adain_apply(): out = (content - mean_c) / sqrt(var_c + eps) * sqrt(var_s + eps) + mean_s with svr_chan_stats()'s stats.
 *   One launch. */
int64_t svr_colorfix_workspace_bytes(int32_t T);
int svr_wavelet_reconstruct(const void* content, const int64_t* content_strides, const void* style, const int64_t* style_strides,
                            void* out, const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream);
int svr_lab_planes(const void* base, const int64_t* base_strides, const void* style, const int64_t* style_strides, void* c_lab,
                   void* s_lab, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream);
int svr_lab_merge(const void* c_L, const void* m_L, const void* m_a, const void* m_b, double luminance_weight, void* out,
                  const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream);
int svr_chan_stats(const void* content, const int64_t* content_strides, const void* style, const int64_t* style_strides, void* stats,
                   int32_t T, int32_t H, int32_t W, int32_t kind, void* workspace, int64_t workspace_bytes, void* stream);
int svr_adain_apply(const void* content, const int64_t* content_strides, const void* stats, float eps, void* out,
                    const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream);

/* Rank matching (colorfix.sort_key / colorfix.rank_match_spec are the specification, BIT FOR BIT; csrc/svr_rank.hip): a stable
 * least-significant-digit radix sort of fp32 keys, 8-bit digits, four passes of three launches (per-tile digit counts, a scan of the
 * digit x tile table, a stable scatter).  No workgroup waits on another, no atomic decides a position: the same bits on every run.
 * All operands are dense fp32 / uint32 [n], 4-byte aligned, 1 <= n <= 2^30; inputs are not modified.  The order is that of
 * torch.sort(stable=True) on the CPU: -inf ... -0.0 = +0.0 ... +inf, NaN last, equal keys in the order of their indices; a sorted
 * value is canonical (-0.0 reads back as +0.0, any NaN as the quiet NaN 0x7FC00000).
 * svr_rank_workspace_bytes(n): bytes of device memory either call needs, 16-byte aligned: 5 * roundup(4 n, 256) + 1024 *
 *   roundup(ceil(n / 4096), 16) + 1024, which is at most 20.25 n + 20 KiB (below 24 n + 65536); <= 0: n is refused.
 * svr_rank_geometry(out2): out2[0] = 4096, the keys of one tile (one column of the table; a workgroup walks 16 consecutive tiles, so
 *   n = 65536 is a boundary as well); out2[1] = 0: one launch of the table scan covers any number of tiles.
 * svr_sort_f32(): sorted[k] = the k-th smallest key's canonical value; index (may be NULL: keys only, 4 bytes per element and pass
 *   less) [k] = where that key stood in `keys`.  12 launches.
 * svr_rank_match(): out[i] = sorted_reference[r(i)], r(i) = the number of j with key(source_j) < key(source_i), plus the number of
 *   j < i with an equal key.  The reference is sorted first (keys only) and its 4 n bytes kept, then the source's key + index pairs
 *   are sorted and out[index[k]] = sorted_reference[k] is stored.  25 launches.
 * No two of the operands, outputs and the workspace may overlap, with one exception: out may be `source` itself (the same pointer).
 * Every argument is checked before the first launch (a null pointer, n, alignment, a workspace below svr_rank_workspace_bytes(n),
 * overlap) and svr_last_error() names it; nothing is allocated, all launches go to `stream`, none synchronises with the host. */
int64_t svr_rank_workspace_bytes(int64_t n);
int svr_rank_geometry(int32_t* out2);
int svr_sort_f32(const void* keys, int64_t n, void* sorted, void* index, void* workspace, int64_t workspace_bytes, void* stream);
int svr_rank_match(const void* source, const void* reference, int64_t n, void* out, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* The HSV half (colorfix.hsv_spec / wavelet_adaptive_spec / hue_match_spec are the specification; csrc/svr_hsv.hip).  Pixel operands,
 * T, H, W, kind and their checks are those of the colour-correction calls above; planes are dense fp32 [T*H*W].
 * svr_hsv_planes(): content, style in [-1, 1] -> ((x + 1) * 0.5) clamped to [0, 1] -> colorfix.rgb_to_hsv in its operation order
 *   (IEEE divisions, no contraction) -> c_hsv: dense planar fp32 [3, T*H*W] (h, s, v), s_hs: [2, T*H*W] (h, s).  BIT FOR BIT the
 *   CPU run for finite and infinite inputs (a NaN input is not pinned).  One launch.
 * svr_hue_match(): colorfix.hue_match_spec BIT FOR BIT with bins = 12, min_pixels = 100: for every hue bin k (fp32 comparisons
 *   against colorfix.HUE_EDGES; bin 0 also holds every h >= e_11) with more than 100 pixels in c_h and in s_h, the content
 *   saturations of the bin are rank-matched to the style saturations of the bin: the j-th smallest (stable: ties to the lower flat
 *   index of the whole plane) of n_s receives the sorted reference value of rank (j * (n_r - 1)) / (n_s - 1), an exact integer
 *   quotient.  Bins are applied in the order 0..11 and all read the original c_s; a pixel of no qualifying bin keeps its value.
 *   out may be c_s itself (the same pointer); otherwise no two of out, the inputs and the workspace may overlap.  1 <= n <= 2^30.
 *   Launches: two partitions by hue class (one radix pass each: 3 launches), then per qualifying bin two four-pass sorts and one
 *   scatter (25 launches; bin 0 three more for a partition of its own): at most 6 + 3 + 12 * 25 launches and one device-to-device
 *   copy.  The class counts that decide which bins qualify are READ BY THE HOST: one 2 KiB device-to-host copy and one
 *   synchronisation of `stream` per call, so the call cannot be captured into a graph.
 * svr_hue_match_workspace_bytes(n): 5 * roundup(4 n, 256) + 3072 + svr_rank_workspace_bytes(n) (below 48 n + 131072); <= 0: n is
 *   refused.  16-byte aligned.
 * svr_hsv_merge(): colorfix.hsv_to_rgb(h, sat, v) in its operation order, clamped to [0, 1], * 2 - 1 -> out.  BIT FOR BIT.  One launch.
 * svr_adaptive_blend(): the blend of colorfix.wavelet_adaptive_color_correction: with hsv = svr_hsv_merge's pixel, s = the
 *   saturation map of ((x + 1) * 0.5) clamped, w = sigmoid(sharpness * (s(content) - s(style) - threshold)) where s(base) - s(style) >
 *   threshold * 0.5 and 0 elsewhere, out = base * (1 - w) + hsv * w.  threshold, threshold * 0.5 and sharpness are rounded to fp32
 *   from fp64 once.  The saturation maps and the mask are exact; the sigmoid is 1 / (1 + expf(-x)).  One launch. */
int svr_hsv_planes(const void* content, const int64_t* content_strides, const void* style, const int64_t* style_strides, void* c_hsv,
                   void* s_hs, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream);
int64_t svr_hue_match_workspace_bytes(int64_t n);
int svr_hue_match(const void* c_h, const void* c_s, const void* s_h, const void* s_s, int64_t n, void* out, void* workspace,
                  int64_t workspace_bytes, void* stream);
int svr_hsv_merge(const void* h, const void* sat, const void* v, void* out, const int64_t* out_strides, int32_t T, int32_t H, int32_t W,
                  int32_t kind, void* stream);
int svr_adaptive_blend(const void* base, const int64_t* base_strides, const void* content, const int64_t* content_strides,
                       const void* style, const int64_t* style_strides, const void* h, const void* sat, const void* v, double threshold,
                       double sharpness, void* out, const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind,
                       void* stream);

/* ---- packed input frames -------------------------------------------------------------------- */
/* frameio_in.py (the specification, bit for bit), the inverse of svr_pack_frames: packed samples as a decoder emits them -> out
 * fp32 [T, H, W, C] dense, nominally in [0, 1].  Every value is an integer code q over a full scale D, computed in exact integers,
 * and ONE fp32 operation: the fp32 value nearest to q / D.
 *   SVR_UNPACK_RGB8 / _BGR8    uint8 [T, H, W, C], C = 3 or 4, D = 255; BGR8 swaps channels 0 and 2 back, a fourth stays in place.
 *   SVR_UNPACK_RGB16           uint16 [T, H, W, C], C = 3 or 4, D = 65535 (rgb48le / rgba64le).
 *   SVR_UNPACK_YUV420P8 / _P10 C = 3 only.  uint8 / uint16 [T, H*W + 2*h2*w2], h2 = ceil(H/2), w2 = ceil(W/2): per frame the Y
 *                              plane, then Cb, then Cr (svr_pack_frames' layout; a 10-bit sample above 1023 counts as 1023).
 *                              D = 65535.  `matrix` SVR_MATRIX_BT709 / _BT601, `range` SVR_RANGE_TV / _PC; chroma upsampled
 *                              bilinearly in integers, co-sited with even luma columns and midway between luma rows, indices
 *                              clamped to the plane; numerators may be negative: floor division, then clamp to 0..65535.
 * The RGB formats ignore nothing: `matrix` and `range` must be valid codes there too.  Every argument is checked before the launch
 * (T * H * W <= 2^40 pixels); packed_bytes and out_bytes (= 4 * T*H*W*C) must be EXACTLY the sizes above.  One launch on `stream`,
 * no host synchronisation, no workspace. */
#define SVR_UNPACK_RGB8      0    /* (the three formats svr_pack_frames writes keep its ids) */
#define SVR_UNPACK_BGR8      1
#define SVR_UNPACK_YUV420P10 2
#define SVR_UNPACK_RGB16     3
#define SVR_UNPACK_YUV420P8  4
#define SVR_MATRIX_BT709 0
#define SVR_MATRIX_BT601 1
#define SVR_RANGE_TV 0
#define SVR_RANGE_PC 1
int svr_unpack_frames(const void* packed, int64_t packed_bytes, int32_t fmt, int32_t T, int32_t H, int32_t W, int32_t C,
                      int32_t matrix, int32_t range, float* out, int64_t out_bytes, void* stream);

/* ---- planar YUV sources ------------------------------------------------------------------------ */
/* planar.py (the specification, bit for bit): `planes` T frames of planar YUV as a decoder emits them -> `out` uint16 [T, H, W, 3]
 * dense: the 16-bit RGB codes svr_unpack_frames, svr_deinterlace, svr_comb_counts and svr_frame_diffs take as SVR_UNPACK_RGB16.
 *   sub     SVR_PLANAR_420 / _422 / _444.  Per frame the Y plane [H, W], then Cb, then Cr, each [hc, wc] row-major: 420 hc = ceil(H/2),
 *           wc = ceil(W/2); 422 hc = H, wc = ceil(W/2); 444 hc = H, wc = W.
 *   bits    8 (uint8 samples), 10 or 12 (uint16; a sample above 2^bits - 1 counts as 2^bits - 1).
 *   matrix  SVR_COLOUR_MATRIX_BT709 / _BT601 / _BT2020 (non-constant luminance); range SVR_COLOUR_RANGE_TV / _PC (y0 = 16, ys = 219,
 *           cs = 224, each << (bits - 8); or y0 = 0, ys = cs = 2^bits - 1).
 *   siting  SVR_PLANAR_SITING_LEFT: chroma co-sited with even luma columns and (420) midway between luma rows -- what
 *           svr_unpack_frames assumes; SVR_PLANAR_SITING_TOPLEFT (420 only): co-sited with even luma columns AND even luma rows.
 * Chroma is upsampled bilinearly in integers (weights over 8, indices clamped to the plane), the matrix is svr_unpack_frames' in
 * exact 64-bit integers: floor division, then clamp to 0..65535.  For 422 and 444 an output row depends on its input row alone.
 * Every argument is checked before the launch: null pointers, sizes below 1 (T * H * W <= 2^40 pixels), an unknown sub, bits, matrix,
 * range or siting (TOPLEFT with 422 / 444 included), planes_bytes and out_bytes (= 6 * T*H*W) other than EXACTLY the sizes above, a
 * 16-bit operand or out not aligned to 2 bytes, out overlapping planes.  One launch on `stream`, no host synchronisation, no
 * workspace. */
#define SVR_PLANAR_420 0
#define SVR_PLANAR_422 1
#define SVR_PLANAR_444 2
#define SVR_PLANAR_SITING_LEFT    1    /* (SVR_COLOUR_SITING_LEFT's value) */
#define SVR_PLANAR_SITING_TOPLEFT 2
int svr_planar_codes(const void* planes, int64_t planes_bytes, int32_t sub, int32_t bits, int32_t T, int32_t H, int32_t W,
                     int32_t matrix, int32_t range, int32_t siting, void* out, int64_t out_bytes, void* stream);

/* ---- planar YUV output ------------------------------------------------------------------------- */
/* planar_out.py (the specification, bit for bit): `frames` [T, H, W, 3] dense, fp32 or bf16 (x_kind SVR_STORE_FP32 / SVR_STORE_BF16)
 * -> `out`: per frame the Y plane [H, W], then Cb, then Cr, each [hc, wc] row-major, svr_planar_codes' layout: uint8 samples at 8
 * bits, uint16 at 10 and 12 -- ffmpeg's yuv4??p / yuv4??p10le / yuv4??p12le rawvideo.
 *   sub     SVR_PLANAR_420 / _422 / _444;  bits 8, 10 or 12 (n);  matrix SVR_COLOUR_MATRIX_*, the weights of svr_pack_yuv420p10;
 *           range SVR_COLOUR_RANGE_TV (y0 = 16, ys = 219, cs = 224, each << (n - 8)) / _PC (y0 = 0, ys = cs = 2^n - 1).
 *   siting  the taps of one chroma sample, indices clamped to the frame, total weight S = Sv * Sh:
 *           vertical    422 / 444 the row itself; 420 SVR_COLOUR_SITING_CENTER / _LEFT rows 2j, 2j+1, weights 1, 1;
 *                       420 SVR_PLANAR_SITING_TOPLEFT rows 2j-1, 2j, 2j+1, weights 1, 2, 1
 *           horizontal  444 the column itself; CENTER columns 2k, 2k+1, weights 1, 1; LEFT / TOPLEFT columns 2k-1, 2k, 2k+1,
 *                       weights 1, 2, 1
 *           TOPLEFT is for 420 only; 444 takes LEFT only.
 * q = rint(clamp(x, 0, 1) * 65535) (NaN -> 0), D = 65535 * 65536, half = 2^(n-1), top = 2^n - 1:
 *   Y  = y0 + (ys * (wr r + wg g + wb b) + D/2) / D
 *   Cb = min((S half D + cs * (cb_r sr + cb_g sg + 32768 sb) + S D/2) / (S D), top), Cr likewise: every numerator is positive and
 *   below 2^62.  (420, 10 bits, CENTER / LEFT) is svr_pack_yuv420p10, bit for bit.
 * Every argument is checked before the launch, in svr_pack_yuv420p10's order: null pointers, x_kind, sizes below 1 (T * H * W <=
 * 2^40 pixels), an unknown sub, bits, matrix, range or siting and a siting its sub does not take, misaligned frames (and out at 10 /
 * 12 bits: 2 bytes), out_bytes other than EXACTLY the planes' size.  One launch on `stream`, no host synchronisation, no workspace. */
int svr_pack_planar(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t sub, int32_t bits, int32_t matrix,
                    int32_t range, int32_t siting, void* out, int64_t out_bytes, void* stream);

/* ---- interlaced sources ------------------------------------------------------------------------ */
/* deinterlace.py (the specification, bit for bit): `packed` T woven frames in one of the SVR_UNPACK_* formats (same layouts and
 * element types as svr_unpack_frames takes) -> `out` T (SVR_DEINT_FRAME) or 2 T (SVR_DEINT_FIELD) progressive frames in the same
 * format.  Per plane -- the one plane of the RGB formats, whose channels lie C elements apart, or Y, Cb and Cr each with its own
 * rows -- the rows of the kept field are copied and the others are computed by a motion-adaptive, edge-directed rule in exact
 * integers (temporal average of the neighbouring fields of the missing parity, clamped around it by the largest of three temporal
 * differences; the spatial prediction searches five directions).  `order`: SVR_FIELD_TFF the first field in time is the even rows,
 * SVR_FIELD_BFF the odd ones.  SVR_DEINT_FRAME keeps the first field of every frame; SVR_DEINT_FIELD gives output 2 t the first and
 * output 2 t + 1 the second field of frame t.  `before` / `after`: one packed frame each, the frame ahead of the clip and the one
 * behind it, or NULL: the clip is then mirrored at that end (F[-1] = F[min(1, T-1)], F[T] = F[max(T-2, 0)]).
 * Every argument is checked before the first launch: null packed / out, an unknown fmt, order or rate, a C the format does not
 * take, sizes below 1 (T * H * W <= 2^40 pixels), packed_bytes and out_bytes other than EXACTLY the format's sizes, a pointer not
 * aligned to its element, out overlapping packed, before or after.  One launch per plane on `stream`, no host synchronisation, no
 * workspace. */
#define SVR_FIELD_TFF 0
#define SVR_FIELD_BFF 1
#define SVR_DEINT_FRAME 0
#define SVR_DEINT_FIELD 1
int svr_deinterlace(const void* packed, int64_t packed_bytes, const void* before, const void* after, int32_t fmt, int32_t T, int32_t H,
                    int32_t W, int32_t C, int32_t order, int32_t rate, void* out, int64_t out_bytes, void* stream);

/* ---- field matching ---------------------------------------------------------------------------- */
/* fieldmatch.py (the specification, bit for bit).  `packed`, `before`, `after`, fmt, T, H, W, C and `order` are svr_deinterlace's: T
 * woven frames in one of the SVR_UNPACK_* formats, one context frame ahead and one behind or NULL (the mirror).  p = order is the
 * parity of the kept (first) field.
 * svr_comb_counts: `cnt` int32 [T, 3, 2].  Only plane 0 is read (Y, or the interleaved RGB plane: R = H rows of N samples, channels s
 *   apart).  thr' = thr << shift, shift 0 for the 8-bit formats, 2 for SVR_UNPACK_YUV420P10, 8 for SVR_UNPACK_RGB16; thr in 0..255.
 *   Tested rows: r % 2 == 1 - p, 1 <= r <= R - 2.  Candidate k takes row r from X_0 = F[t], X_1 = F[t-1], X_2 = F[t+1]; with
 *   u = F[t][r-1][i], l = F[t][r+1][i], m = X_k[r][i], sample i is combed iff m < min(u, l) - thr' or m > max(u, l) + thr'.  Blocks are
 *   16 plane rows by 16 pixel columns (block row r / 16, block column (i / s) / 16).  cnt[t][k] = (total, peak): the combed samples
 *   of the frame, and the largest count of any one block.  R < 3: all zero.  The call zeroes `cnt` on `stream`; ONE launch follows
 *   (block counters in LDS, integer atomic add / max to `cnt`: two runs give the same bits).
 * svr_field_select: `deint` the T frames of svr_deinterlace(..., SVR_DEINT_FRAME) of the same clip, `cnt` as above, both read from
 *   device memory in stream order -> `out` T frames.  With pc, pa, pb the peaks of candidates 0, 1, 2 and bound = mi * s (s of plane
 *   0, mi >= 0): mode 0 if pc <= bound; else (q, m) = (pa, 1) if pa <= pb else (pb, 2), mode m if q <= bound, else 3.  In every
 *   plane rows of parity p (and the only row of a one-row plane) are F[t]'s, the other rows F[t]'s, F[t-1]'s, F[t+1]'s for modes 0,
 *   1, 2; in mode 3 the whole frame is deint[t].  `modes` int32 [T] and `stats` int64 [6] may be NULL: modes[t] is the mode; stats
 *   is ADDED to: entries 0..3 the frames per mode, 4 and 5 the sums of cnt[t][1][0] and cnt[t][2][0] over the mode-3 frames (one
 *   lane per frame, 64-bit integer atomic adds).  One launch per plane.
 * Every argument is checked before anything is enqueued: null pointers, an unknown fmt or order, a C the format does not take,
 * sizes below 1 (T * H * W <= 2^40 pixels; svr_comb_counts: H * W * C <= 2^31, the counters are int32), thr outside 0..255, mi < 0,
 * byte counts other than EXACTLY the format's and 24 T for cnt, a pointer not aligned to its element, an output (cnt; out, modes,
 * stats) overlapping an input or another output.  No host synchronisation, no workspace. */
int svr_comb_counts(const void* packed, int64_t packed_bytes, const void* before, const void* after, int32_t fmt, int32_t T, int32_t H,
                    int32_t W, int32_t C, int32_t order, int32_t thr, void* cnt, int64_t cnt_bytes, void* stream);
int svr_field_select(const void* packed, int64_t packed_bytes, const void* before, const void* after, const void* deint,
                     int64_t deint_bytes, const void* cnt, int64_t cnt_bytes, int32_t fmt, int32_t T, int32_t H, int32_t W, int32_t C,
                     int32_t order, int32_t mi, void* out, int64_t out_bytes, void* modes, void* stats, void* stream);

/* ---- decimation -------------------------------------------------------------------------------- */
/* decimate.py (the specification, bit for bit).  `packed`, fmt, T, H, W, C are svr_deinterlace's: T frames in one of the SVR_UNPACK_*
 * formats -- normally svr_field_select's output --; `before` one frame, the frame ahead of the clip, or NULL at the clip's start.
 * There is no order, no `after` and no mirror.
 * svr_frame_diffs: `diff` int32 [T].  Only plane 0 is read (Y, or the interleaved RGB plane: R = H rows of N samples, channels s
 *   apart), samples as stored.  Blocks are 32 plane rows by 32 pixel columns (block row r / 32, block column (i / s) / 32, partial
 *   at the edges).  diff[t] = the largest block sum of |F[t][r][i] - F[t-1][r][i]| (at most 32 * 32 * 4 * 65535 < 2^31); diff[0]
 *   compares with `before`, and is 2^31 - 1 where `before` is NULL.  The call zeroes `diff` on `stream`; ONE launch follows (block
 *   sums in LDS, integer atomic max to `diff`: two runs give the same bits).
 * svr_decimate_select: `diff` as above, read from device memory in stream order -> `out` T - T / 5 frames.  Per whole cycle c of five
 *   frames the drop is the position 0..4 of the smallest of diff[5c .. 5c + 4], the FIRST of a tie; the cycle's other four frames
 *   are copied in their order, and so are the T % 5 frames of a trailing partial cycle (T < 5: a copy).  `drops` int32 [T / 5] and
 *   `stats` int64 [6] may be NULL (and `drops` is not looked at where T < 5): drops[c] is the drop; stats is ADDED to: entries 0..4
 *   the cycles per drop position, entry 5 the dropped frames with diff > dup * s << shift (s of plane 0; shift 0 for the 8-bit
 *   formats, 2 for SVR_UNPACK_YUV420P10, 8 for SVR_UNPACK_RGB16; dup in 0..2^18), which decides nothing (one lane per cycle, 64-bit
 *   integer atomic adds).  ONE launch.
 * Every argument is checked before anything is enqueued: null pointers, an unknown fmt, a C the format does not take, sizes below 1
 * (T * H * W <= 2^40 pixels), dup outside 0..2^18, byte counts other than EXACTLY the format's (T - T / 5 frames for out) and 4 T for
 * diff, a pointer not aligned to its element, an output (diff; out, drops, stats) overlapping an input or another output.  No
 * host synchronisation, no workspace. */
int svr_frame_diffs(const void* packed, int64_t packed_bytes, const void* before, int32_t fmt, int32_t T, int32_t H, int32_t W, int32_t C,
                    void* diff, int64_t diff_bytes, void* stream);
int svr_decimate_select(const void* packed, int64_t packed_bytes, const void* diff, int64_t diff_bytes, int32_t fmt, int32_t T, int32_t H,
                        int32_t W, int32_t C, int32_t dup, void* out, int64_t out_bytes, void* drops, void* stats, void* stream);

/* ---- GGUF block-quantised weights, expanded at load ------------------------------------------- */
/* gguf.py (the specification, bit for bit): `n_blocks` consecutive blocks of one ggml type -> n_blocks * block size values, each
 * the format's fp32 dequantisation, stored as fp32 (out_kind SVR_STORE_FP32) or rounded once to bf16, nearest even (SVR_STORE_BF16).
 * d / dmin are IEEE fp16, everything little-endian:
 *   SVR_GGML_Q8_0  34 B / 32    d | int8 q[32]                              x = d * q
 *   SVR_GGML_Q4_K  144 B / 256  d | dmin | scales[12] | qs[128]             x = (d * sc) * q - dmin * m
 *   SVR_GGML_Q5_K  176 B / 256  d | dmin | scales[12] | qh[32] | qs[128]    the same, q in 0..31
 *   SVR_GGML_Q6_K  210 B / 256  ql[128] | qh[64] | int8 scales[16] | d      x = (d * scales[e / 16]) * (q - 32)
 * (the ggml type ids of the file format).  Every argument is checked before the launch: null pointers, a type outside the four, a
 * bad out_kind, n_blocks < 1 or more than 2^40 elements, out_bytes other than EXACTLY n_blocks * block size * element size, blocks
 * not 32-byte aligned or out not 16-byte aligned.  One launch on `stream`, no host synchronisation, no workspace. */
#define SVR_GGML_Q8_0 8
#define SVR_GGML_Q4_K 12
#define SVR_GGML_Q5_K 13
#define SVR_GGML_Q6_K 14
int svr_dequant_gguf(const void* blocks, int32_t ggml_type, int64_t n_blocks, void* out, int32_t out_kind, int64_t out_bytes,
                     void* stream);

/* ---- misc ------------------------------------------------------------------------------------ */
/* Tuning / measurement knobs (no effect on results):
 * "conv_impl" 0 auto (LDS-halo kernels for stride-1 3x3 convs; register-streamed weights when W_frag is given)
 * | 1 generic implicit GEMM everywhere | 3 LDS-halo kernel ignoring W_frag (weights through LDS),
 * "conv_rows" patch rows per wave of the register-streamed conv kernel: 8 (default: 256 accumulators, one wave per SIMD) | 4
 * (two workgroups per CU),
 * "conv_band" tile rows per band of the conv kernel's frame-inner tile order (default 1; 0: frame outermost),
 * "conv_sub" 1 (default) (kt, 2, 2)-tap convs with W_frag run on the sub-pixel conv kernel | 0 on the generic kernel,
 * "conv_lds" dynamic LDS bytes to request for the halo kernel (> 80 KiB forces one workgroup per CU),
 * "conv_thinout4" 1 (default) stride-1 3x3 convs with Cout <= 4 (decoder conv_out) on the resident-weight frame-streaming kernel | 0 on
 * the 32-cout thin-output kernel,
 * "gemm_w4" 1 (default) plain GEMMs with N % 256 == 0 and >= 256 tiles on the persistent four-wave kernel (256 accumulators per
 * wave, the vendor library's tile shape and MFMA) | 0 on the eight-wave kernel like everything else,
 * "gemm_w4r" 1 (default) the persistent kernel streams the weights of a launch that carries W_frag from that copy into registers and
 * brings the activations into LDS by LDS-DMA | 0 it stages both operands through LDS whether W_frag is given or not,
 * "gemm_epi" epilogue of the GEMM kernel: 0 auto | 1 stores straight from the accumulators | 2 through LDS wherever possible,
 * "attn_impl" 0 auto (second-generation window kernel for head_dim 128 / windows <= 2048 rows) | 1 first kernel everywhere,
 * "attn_variant" build variant of the second-generation window kernel (0 default = 8 waves x 32 queries; 1 / 3 / 4: 4-wave and
 * s_setprio builds -- see svr_attn_win.hip),
 * "rank_launches" 3 (default) | 1 | 2: measurement only -- svr_sort_f32 issues only the histogram, or the histogram and the table scan,
 * of every pass (nothing is stored to its outputs; svr_rank_match refuses), so that the launches can be timed by difference,
 * "pipe_abl" measurement-only ablations in -DSVR_ABLATIONS builds (non-zero values give garbage). */
int svr_set_option(const char* key, int32_t value);
/* Calibration aid, NOT on the data path (ABI v9; the reference has no counterpart -- its timing report is src/utils/debug.py): launches
 * a bare v_mfma_f32_32x32x16_bf16 loop on pseudo-random operands, four 512-thread workgroups per CU, `iters` x 16 MFMAs per wave, no
 * memory traffic, on `stream`; `*flops` (if not NULL) receives the FLOPs the launch executes.  The caller times it with events on the
 * same stream: FLOPs / time is the matrix-pipe rate this device sustains under its power limit at that moment (bench.py reports it
 * as roofline.power_limited_peak next to the nominal 2.5 PFLOP/s).  `workspace`: svr_mfma_calibrate_workspace_bytes() of device memory. */
int64_t svr_mfma_calibrate_workspace_bytes(void);
int svr_mfma_calibrate(void* workspace, int32_t iters, double* flops, void* stream);
const char* svr_last_error(void);
int svr_abi_version(void);
/* hex SHA-256 of the sources (every .hip and .h file under csrc/ and this header; sorted by name) AND the compile configuration (hipcc flags
 * and -D defines: a measurement build is not the product build) this binary was compiled from, as passed by the
 * build (-DSVR_BUILD_ID=...); "unknown" if the build did not pass one.  The Python loader refuses a library whose id differs
 * from the sources next to it (a stale binary shipped with newer sources). */
const char* svr_build_id(void);
/* prints device name / CU count into buf; returns 0 if a gfx950 device is current. */
int svr_device_info(char* buf, int32_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* SEEDVR2_HIP_H */
