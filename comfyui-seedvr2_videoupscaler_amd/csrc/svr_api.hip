// extern "C" entry points of libseedvr2_hip.so (see include/seedvr2_hip.h for the contract).
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"
#include <cstdio>
#include <cstdarg>
#include <vector>
#include <algorithm>
#include <cstring>
#include <type_traits>

// single translation unit: the kernel sources are included here so one hipcc call builds the library
#include "svr_gemm.hip"
#include "svr_conv_halo2.hip"
#include "svr_conv_sub.hip"
#include "svr_conv_thinout.hip"
#include "svr_attn_win.hip"
#include "svr_attn.hip"
#include "svr_elementwise.hip"
#include "svr_calibrate.hip"
#include "svr_alpha.hip"
#include "svr_frame_pack.hip"
#include "svr_frame_pack_colour.hip"
#include "svr_planar_out.hip"
#include "svr_frame_unpack.hip"
#include "svr_planar.hip"
#include "svr_png.hip"
#include "svr_colorfix.hip"
#include "svr_rank.hip"
#include "svr_hsv.hip"
#include "svr_gguf.hip"
#include "svr_shots.hip"
#include "svr_active.hip"
#include "svr_deinterlace.hip"
#include "svr_fieldmatch.hip"
#include "svr_decimate.hip"

using namespace svr;

static thread_local char g_err[512] = "";

static inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- what the entry points share: one way to refuse a call, one step from a run-time code to a template constant, one capped
// grid.  An entry point states its name once, in its Entry.
struct Entry {
    const char* fn;
    // "<fn>: <message>" left in g_err -> -1
    __attribute__((format(printf, 2, 3))) int refuse(const char* fmt, ...) const {
        char msg[sizeof(g_err)];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
        return -1;
    }
    // a router's message (gemm_route, attn_dispatch: worded in the kernel files, prefix included) left in g_err as it is -> -1
    int relay(const char* message) const {
        snprintf(g_err, sizeof(g_err), "%s", message);
        return -1;
    }
    // a byte count that has to be exact: "<arg> is N, <words> exactly M"
    int wrong_size(const char* arg, int64_t is, const char* words, int64_t exactly) const {
        return refuse("%s is %lld, %s exactly %lld", arg, (long long)is, words, (long long)exactly);
    }
    // a HIP call's status: 0, or the status with "<fn>[: <doing>]: <HIP's words>" left in g_err
    int hip(int status, const char* doing = "") const {
        if (status) refuse("%s%s%s", doing, *doing ? ": " : "", hipGetErrorString((hipError_t)status));
        return status;
    }
    int launched() const { return hip(hipGetLastError()); }
};
// an entry point that launches: on its stream's device until it returns
struct Launch : Entry {
    StreamDeviceGuard on_stream_device;
    Launch(const char* fn, void* stream) : Entry{fn}, on_stream_device(stream) {}
};

// f(std::integral_constant<int, V>{}) for the V of the list that equals v -> whether there was one.  Every caller has checked v.
// At run time the order of a list means nothing; the compiler, though, emits the kernels one call instantiates last value first,
// and the lists below are written so that the code object keeps the order of its kernels.
template <int... Vs, class F>
static bool with_const(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <class F>
static bool with_kind(int kind, F&& f) { return with_const<SVR_STORE_BF16, SVR_STORE_FP32>(kind, f); }
// ... and of the operands that may be h16 as well
template <class F>
static bool with_store(int kind, F&& f) { return with_const<SVR_STORE_BF16, SVR_STORE_H16, SVR_STORE_FP32>(kind, f); }

// one workgroup of 256 per 256 items of work, at most eight per CU (the kernels stride over the rest).  Capped in 64 bits: under the
// 2^40-pixel limit the block count of the element-wise routes does not fit 32
static unsigned capped_grid(int64_t work) { return (unsigned)std::min<int64_t>((work + 255) / 256, (int64_t)device_cu_count() * 8); }

extern "C" {

const char* svr_last_error(void) { return g_err; }
int svr_abi_version(void) { return SVR_ABI_VERSION; }
#ifndef SVR_BUILD_ID
#define SVR_BUILD_ID "unknown"
#endif
// (stored behind a marker so that the loader can read it from the file without dlopen()ing a possibly stale binary)
static const char g_build_id[] = "SVR_BUILD_ID=" SVR_BUILD_ID;
const char* svr_build_id(void) { return g_build_id + 13; }


int64_t svr_mfma_calibrate_workspace_bytes(void) { return (int64_t)device_cu_count() * 4 * 512 * (int64_t)sizeof(float); }

int svr_mfma_calibrate(void* workspace, int32_t iters, double* flops, void* stream) {
    const Launch e{"svr_mfma_calibrate", stream};
    if (!workspace || iters <= 0) return e.refuse("workspace of svr_mfma_calibrate_workspace_bytes() and iters > 0");
    const unsigned grid = (unsigned)device_cu_count() * 4;
    hipLaunchKernelGGL(mfma_calibrate_kernel, dim3(grid), dim3(512), 0, (hipStream_t)stream, (float*)workspace, iters);
    // 8 waves per workgroup, 16 MFMAs of 2 * 32 * 32 * 16 FLOP per wave and iteration
    if (flops) *flops = (double)grid * 8.0 * 16.0 * (2.0 * 32 * 32 * 16) * (double)iters;
    return e.launched();
}

int svr_set_option(const char* key, int32_t value) {
    const Entry e{"svr_set_option"};
    if (!key) return e.refuse("null key");
    if (!strcmp(key, "pipe_abl")) { g_pipe_abl = value; return 0; }
    if (!strcmp(key, "conv_impl")) { g_conv_impl = value; return 0; }
    if (!strcmp(key, "gemm_epi")) { g_gemm_epi = value; return 0; }
    if (!strcmp(key, "gemm_w4")) { g_gemm_w4 = value; return 0; }
    if (!strcmp(key, "gemm_w4r")) { if ((unsigned)value > 1u) return e.refuse("gemm_w4r is 0 or 1"); g_gemm_w4r = value; return 0; }
    if (!strcmp(key, "conv_rows")) { g_conv_rows = value; return 0; }
    if (!strcmp(key, "conv_band")) { g_conv_band = value; return 0; }
    if (!strcmp(key, "conv_sub")) { g_conv_sub = value; return 0; }
    if (!strcmp(key, "conv_lds")) { g_conv_lds_dbg = value; return 0; }
    if (!strcmp(key, "conv_thinout4")) { g_conv_thinout4 = value; return 0; }
    if (!strcmp(key, "attn_impl")) { g_attn_impl = value; return 0; }
    if (!strcmp(key, "attn_variant")) { g_attn_variant = value; return 0; }
    if (!strcmp(key, "png_passes")) { if (value < 1 || value > 3) return e.refuse("png_passes is 1, 2 or 3"); g_png_passes = value; return 0; }
    if (!strcmp(key, "rank_launches")) { if (value < 1 || value > 3) return e.refuse("rank_launches is 1, 2 or 3"); g_rank_launches = value; return 0; }
    return e.refuse("unknown key");
}

int svr_device_info(char* buf, int32_t buflen) {
    const Entry e{"svr_device_info"};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return e.refuse("no HIP device");
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return e.refuse("hipGetDeviceProperties failed");
    if (buf && buflen > 0)
        snprintf(buf, buflen, "%s arch=%s CUs=%d LDS/block=%zu mem=%.1fGB", p.name, p.gcnArchName,
                 p.multiProcessorCount, (size_t)p.maxSharedMemoryPerMultiProcessor, p.totalGlobalMem / 1e9);
    return strstr(p.gcnArchName, "gfx950") ? 0 : e.refuse("current device is not gfx950");
}

// (gemm_route and attn_dispatch word their refusals themselves, prefix included: relayed as they are)
int svr_gemm_bf16(const svr_gemm_args* args, void* stream) {
    const Launch e{"svr_gemm_bf16", stream};
    if (!args) return e.refuse("null args");
    const char* why = nullptr;
    const int rc = gemm_dispatch(*args, (hipStream_t)stream, &why);
    return why ? e.relay(why) : e.hip(rc);
}

int32_t svr_gemm_kernel_class(const svr_gemm_args* args) {
    const Entry e{"svr_gemm_kernel_class"};
    if (!args) return e.refuse("null args");
    const char* why = nullptr;
    const int cls = gemm_route(*args, &why);
    if (why) e.relay(why);
    return cls;
}

const char* svr_gemm_kernel_name(int32_t cls) {
    switch (cls) {
        case SVR_KERNEL_NONE: return "none";
        case SVR_KERNEL_GEMM: return "svr::gemm_kernel";
        case SVR_KERNEL_GEMM_PERSISTENT: return "svr::gemm_w4r_kernel";      // (gemm_w4q_kernel when the launch carries no W_frag)
        case SVR_KERNEL_CONV_HALO: return "svr::conv_halo2_kernel";
        case SVR_KERNEL_CONV_SUBPIXEL: return "svr::conv_sub_kernel";
        case SVR_KERNEL_CONV_THIN_IN: return "svr::conv_halo2_kernel<8, 2> (thin input)";
        case SVR_KERNEL_CONV_THIN_OUT: return "svr::conv_thinout_kernel";
        case SVR_KERNEL_CONV_GENERIC: return "svr::gemm_kernel<..., CONV>";
        default: return "invalid";
    }
}

int32_t svr_gemm_gn_blocks(const svr_gemm_args* args) {
    if (!args || !args->conv.enabled || args->gn_groups <= 0) return 0;
    return conv_gn_blocks(*args);
}

int svr_groupnorm_reduce(const void* partial, double* stats, int32_t T, int32_t nblk, int32_t groups, void* stream) {
    const Launch e{"svr_groupnorm_reduce", stream};
    if (T <= 0 || nblk <= 0) return 0;
    if (groups <= 0 || groups > 65535) return e.refuse("1..65535 groups");
    if (!partial || !stats) return e.refuse("null pointer");
    hipLaunchKernelGGL(groupnorm_reduce_kernel, dim3(T, groups), dim3(256), 0, (hipStream_t)stream,
                       (const double2*)partial, stats, (int)nblk, groups);
    return e.launched();
}

int svr_rmsnorm_mod(const void* x, void* y, int64_t rows, int32_t dim, float eps, const float* w, const float* scale,
                    const float* shift, int32_t x_f32, void* stream) {
    const Launch e{"svr_rmsnorm_mod", stream};
    // layout contract (checked on an empty call too): rows are dense and dim % 8 == 0, so a 16-byte aligned base makes every uint4
    // load of x and store of y naturally aligned
    if ((uintptr_t)x % 16 || (uintptr_t)y % 16) return e.refuse("x and y must be 16-byte aligned (rows are read and written in 16-byte units)");
    if (rows <= 0) return 0;
    if (dim <= 0 || dim % 8 || dim > 64 * 8 * 8) return e.refuse("dim must be a multiple of 8 and <= 4096");
    if (!x || !y) return e.refuse("null pointer");
    if ((unsigned)x_f32 > (unsigned)SVR_STORE_H16) return e.refuse("x_f32 must be SVR_STORE_BF16 / _FP32 / _H16");
    const unsigned grid = (unsigned)(rows < 4 * 2048 ? blocks_for(rows, 4) : 2048);      // 8 blocks per CU, rows strided
    // 512-element chunks of a row held in registers: 1..8, as dim was checked
    with_const<8, 7, 6, 5, 4, 3, 2, 1>((dim + 511) / 512, [&](auto NC) { with_store(x_f32, [&](auto K) {
        hipLaunchKernelGGL((rmsnorm_mod_kernel<NC(), K()>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, rows, dim, eps, w, scale, shift);
    }); });
    return e.launched();
}

int svr_ada_combine(const void* emb, const void* params, const int32_t* slot, float* out, int32_t n_vec, int32_t dim,
                    void* stream) {
    const Launch e{"svr_ada_combine", stream};
    if (n_vec <= 0 || dim <= 0) return 0;
    if (n_vec > 65535) return e.refuse("at most 65535 vectors per call");
    if (!emb || !params || !slot || !out) return e.refuse("null pointer");
    hipLaunchKernelGGL(ada_combine_kernel, dim3(blocks_for(dim, 256), n_vec), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)emb, (const bf16_t*)params, slot, out, n_vec, dim);
    return e.launched();
}

int svr_qknorm_rope(void* qkv, int64_t rows, int32_t heads, const int16_t* pos, int32_t t_offset, const float* cos_tab,
                    const float* sin_tab, int32_t n_pos, int32_t n_freq, const float* wq, const float* wk, float eps,
                    void* stream) {
    const Launch e{"svr_qknorm_rope", stream};
    if (rows <= 0) return 0;
    if (n_freq <= 0 || n_freq * 3 > 64) return e.refuse("1..21 frequencies per axis (head_dim 128)");
    if (heads <= 0 || n_pos <= 0) return e.refuse("heads and n_pos must be positive");
    if (!qkv || !pos || !cos_tab || !sin_tab || !wq || !wk) return e.refuse("null pointer (wq / wk are required)");
    // 8 rows (q and k of each: 16 groups of 16 lanes) per block and step; 16 blocks per CU, the rest in the grid-stride loop
    const int64_t nblk = (rows + 7) / 8;
    const unsigned grid = (unsigned)std::min<int64_t>(nblk, (int64_t)device_cu_count() * 16);
    hipLaunchKernelGGL(qknorm_rope_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       (bf16_t*)qkv, rows, heads, pos, t_offset, cos_tab, sin_tab, n_pos, n_freq, wq, wk, eps);
    return e.launched();
}

int svr_attn_varlen(const void* qkv, int64_t ld_qkv, void* out, int64_t ld_out, const int32_t* seq_rows,
                    const int32_t* out_rows, const int32_t* cu, int32_t n_seq, int32_t max_len, int32_t heads,
                    int32_t head_dim, float scale, void* stream) {
    const Launch e{"svr_attn_varlen", stream};
    const char* why = nullptr;
    const int rc = attn_dispatch(qkv, ld_qkv, out, ld_out, seq_rows, out_rows, cu, n_seq, max_len, heads, head_dim,
                                 scale, (hipStream_t)stream, &why);
    return why ? e.relay(why) : e.hip(rc);
}

#ifdef SVR_ABLATIONS
#include "measure/svr_api_measure_1.inc"
#endif

int svr_conv_pack_frag_taps(const void* W, void* out, int32_t N, int32_t K, int32_t kt, int32_t kh, int32_t kw, int32_t Cin, void* stream) {
    const Launch e{"svr_conv_pack_frag_taps", stream};
    if (N <= 0 || N % 32 || Cin <= 0 || Cin % 32 || kt < 1 || kt > 3 || kh < 1 || kh > 3 || kw < 1 || kw > 3 || K != kt * kh * kw * Cin)
        return e.refuse("need N %% 32 == 0, Cin %% 32 == 0, kt, kh, kw in 1..3, K == kt * kh * kw * Cin");
    // one thread per 16-byte chunk of eight weights (here and in the two packers below)
    hipLaunchKernelGGL(conv_pack_frag_taps_kernel, dim3(blocks_for((int64_t)N * K / 8, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)W, (uint4*)out, N, K, kt, kh, kw, Cin);
    return e.launched();
}

int svr_gemm_pack_frag(const void* W, void* out, int32_t N, int32_t K, void* stream) {
    const Launch e{"svr_gemm_pack_frag", stream};
    if (N <= 0 || N % 128 || K <= 0 || K % 64) return e.refuse("need N %% 128 == 0, K %% 64 == 0");
    hipLaunchKernelGGL(gemm_pack_frag_kernel, dim3(blocks_for((int64_t)N * K / 8, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)W, (uint4*)out, N, K);
    return e.launched();
}

int svr_conv_pack_frag(const void* W, void* out, int32_t N, int32_t K, int32_t kt, int32_t Cin, void* stream) {
    const Launch e{"svr_conv_pack_frag", stream};
    if (N <= 0 || N % 32 || Cin <= 0 || Cin % 32 || kt < 1 || kt > 3 || K != kt * 9 * Cin)
        return e.refuse("need N %% 32 == 0, Cin %% 32 == 0, kt in 1..3, K == kt * 9 * Cin");
    hipLaunchKernelGGL(conv_pack_frag_kernel, dim3(blocks_for((int64_t)N * K / 8, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)W, (uint4*)out, N, K, kt, Cin);
    return e.launched();
}

int svr_softmax_rows(const float* S, void* P, int64_t rows, int32_t cols, int64_t ld_s, int64_t ld_p, float scale,
                     void* stream) {
    const Launch e{"svr_softmax_rows", stream};
    // layout contract (checked on an empty call too, so that a caller's layout can be validated without a launch): float4 loads at
    // S + r * ld_s + 4 j, uint2 stores at P + r * ld_p + 4 j
    if (ld_s < cols || ld_p < cols) return e.refuse("ld_s and ld_p must cover the cols columns of a row");
    if ((uintptr_t)S % 16) return e.refuse("S must be 16-byte aligned (rows are read as float4)");
    if ((uintptr_t)P % 8) return e.refuse("P must be 8-byte aligned (rows are written in 8-byte units)");
    if (rows <= 0 || cols <= 0) return 0;
    if (!S || !P) return e.refuse("null pointer");
    if (rows > 0x7fffffff) return e.refuse("at most 2^31 - 1 rows per call");
    if (cols % 4 || cols > 1024 * SM_MAXV * 4 || ld_s % 4 || ld_p % 4)
        return e.refuse("cols must be a multiple of 4 and <= 65536, leading dimensions multiples of 4");
    with_const<1024, 256>(cols <= 256 * SM_MAXV * 4 ? 256 : 1024, [&](auto NT) {
        hipLaunchKernelGGL(softmax_rows_kernel<NT()>, dim3((unsigned)rows), dim3(NT()), 0, (hipStream_t)stream, S, (bf16_t*)P, cols,
                           ld_s, ld_p, scale * 1.4426950408889634f);
    });
    return e.launched();
}

int svr_rows_mean(const void* src, void* dst, int32_t n_groups, int32_t rows_per_group, int32_t dim, void* stream) {
    const Launch e{"svr_rows_mean", stream};
    if (n_groups <= 0 || rows_per_group <= 0 || dim <= 0) return 0;
    if (dim % 8) return e.refuse("dim must be a multiple of 8");
    if (rows_per_group > 65535) return e.refuse("at most 65535 rows per group");
    if (!src || !dst) return e.refuse("null pointer");
    hipLaunchKernelGGL(rows_mean_kernel, dim3(blocks_for(dim / 8, 64), rows_per_group), dim3(64), 0,
                       (hipStream_t)stream, (const bf16_t*)src, (bf16_t*)dst, n_groups, rows_per_group, dim);
    return e.launched();
}

int svr_patchify(const void* in, void* out, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kpad, void* stream) {
    const Launch e{"svr_patchify", stream};
    if ((H & 1) || (W & 1) || C <= 0 || kpad < 4 * C) return e.refuse("H, W must be even, C positive and kpad >= 4*C");
    if (!in || !out) return e.refuse("null pointer");
    const int64_t total = (int64_t)T * (H / 2) * (W / 2) * kpad;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(patchify_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)in, (bf16_t*)out, T, H, W, C, kpad);
    return e.launched();
}

int svr_unpatchify_euler(const void* pred, int64_t ldp, const void* x_t, void* out, int32_t T, int32_t H, int32_t W,
                         int32_t C, void* stream) {
    const Launch e{"svr_unpatchify_euler", stream};
    if ((H & 1) || (W & 1)) return e.refuse("H, W must be even");
    if (!pred || !out) return e.refuse("null pointer");
    if (ldp < 4 * (int64_t)C) return e.refuse("ldp must cover the 4*C prediction columns");
    const int64_t total = (int64_t)T * H * W * C;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(unpatchify_euler_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)pred, ldp, (const bf16_t*)x_t, (bf16_t*)out, T, H, W, C);
    return e.launched();
}

int64_t svr_groupnorm_workspace_bytes(int32_t T, int64_t HW, int32_t groups) {
    return (int64_t)T * blocks_for(HW, GN_ROWS_PER_BLOCK) * groups * 16;
}

int svr_groupnorm_stats(const void* x, double* stats, void* workspace, int32_t T, int64_t HW, int32_t C, int32_t groups,
                        int32_t x_f32, void* stream) {
    const Launch e{"svr_groupnorm_stats", stream};
    if (T <= 0 || HW <= 0) return 0;
    if (C <= 0 || groups <= 0 || C % groups || T > 65535) return e.refuse("need C > 0, 1 <= groups dividing C, T <= 65535");
    if (!x || !stats) return e.refuse("null pointer");
    if (C % 8 || C > 512 || groups > 32 || (C / groups) % 4 || (256 % (C / 8)))
        return e.refuse("need C in {128,256,512}-like (C%%8==0, C<=512, groups<=32, (C/groups)%%4==0)");
    if (!workspace) return e.refuse("workspace missing (svr_groupnorm_workspace_bytes)");
    const unsigned nblk = blocks_for(HW, GN_ROWS_PER_BLOCK);
    if ((unsigned)x_f32 > (unsigned)SVR_STORE_H16) return e.refuse("x_f32 must be SVR_STORE_BF16 / _FP32 / _H16");
    with_store(x_f32, [&](auto K) {
        hipLaunchKernelGGL(groupnorm_stats_kernel<K()>, dim3(nblk, T), dim3(256), 0, (hipStream_t)stream, x, (double2*)workspace, HW, C, groups);
    });
    hipLaunchKernelGGL(groupnorm_reduce_kernel, dim3(T, groups), dim3(256), 0, (hipStream_t)stream,
                       (const double2*)workspace, stats, (int)nblk, groups);
    return e.launched();
}

int svr_groupnorm_apply(const void* x, void* y, const double* stats, const float* gamma, const float* beta, int32_t T,
                        int64_t HW, int32_t C, int32_t groups, float eps, int32_t apply_silu, int32_t x_f32, void* stream) {
    const Launch e{"svr_groupnorm_apply", stream};
    if (T <= 0 || HW <= 0) return 0;
    if (C <= 0 || C % 8 || C > 512) return e.refuse("C must be a multiple of 8 and <= 512");
    if (groups <= 0 || C % groups || T > 65535) return e.refuse("need 1 <= groups dividing C, T <= 65535");
    if (!x || !y || !stats || !gamma || !beta) return e.refuse("null pointer");
    const int64_t nchunks = HW * (C / 8);
    // workgroups per frame, each streaming one contiguous span of >= 4 x 4 KiB (measured: spans of 16 KiB 6.4 TB/s, 32 KiB 6.25,
    // 64 KiB 5.65, 128 KiB 5.2 on 5 x 1024^2 x 128: profiles/r5_gn_apply_ab.txt)
    unsigned gx = blocks_for(nchunks, 256 * 4);
    if (gx > 65535u) gx = 65535u;
    if ((unsigned)x_f32 > (unsigned)SVR_STORE_H16) return e.refuse("x_f32 must be SVR_STORE_BF16 / _FP32 / _H16");
    with_store(x_f32, [&](auto K) { with_const<0, 1>(apply_silu != 0, [&](auto SILU) {
        hipLaunchKernelGGL((groupnorm_apply_kernel<K(), SILU() != 0>), dim3(gx, T), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, stats, gamma, beta, HW, C, groups, eps);
    }); });
    return e.launched();
}

int svr_im2col_causal(const void* in, void* out, const svr_conv_geom* g, int32_t kpad, void* stream) {
    const Launch e{"svr_im2col_causal", stream};
    if (!g || !in || !out) return e.refuse("null geometry / pointer");
    if (g->Cin <= 0 || g->Cin % 4 || kpad % g->Cin || kpad < g->kt * g->kh * g->kw * g->Cin)
        return e.refuse("Cin %% 4 == 0 and kpad a multiple of Cin covering all taps required");
    const int64_t total = (int64_t)g->To * g->Ho * g->Wo * (kpad / g->Cin);
    if (total <= 0) return 0;
    hipLaunchKernelGGL(im2col_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)in, (bf16_t*)out, *g, kpad);
    return e.launched();
}

int svr_blend_accumulate(const void* tile, float* acc, float* cnt, const float* wy, const float* wx, int32_t T,
                         int32_t h, int32_t w, int32_t C, int32_t H, int32_t W, int32_t y0, int32_t x0, void* stream) {
    const Launch e{"svr_blend_accumulate", stream};
    const int64_t total = (int64_t)T * h * w * C;
    if (total <= 0) return 0;
    if (y0 < 0 || x0 < 0 || y0 + h > H || x0 + w > W) return e.refuse("tile outside the canvas");
    if (!tile || !acc || !cnt || !wy || !wx) return e.refuse("null pointer");
    hipLaunchKernelGGL(blend_accumulate_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)tile, acc, cnt, wy, wx, T, h, w, C, H, W, y0, x0);
    return e.launched();
}

int svr_blend_finalize(const float* acc, const float* cnt, void* out, int32_t T, int64_t HW, int32_t C, int32_t c_take,
                       float scale, float shift, void* stream) {
    const Launch e{"svr_blend_finalize", stream};
    const int64_t total = (int64_t)T * HW * c_take;
    if (total <= 0) return 0;
    if (c_take > C) return e.refuse("c_take > C");
    if (!acc || !cnt || !out) return e.refuse("null pointer");
    hipLaunchKernelGGL(blend_finalize_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream, acc, cnt,
                       (bf16_t*)out, T, HW, C, c_take, scale, shift);
    return e.launched();
}

int svr_affine_slice(const void* in, void* out, int64_t rows, int32_t c_in, int32_t c_out, float scale, float shift,
                     void* stream) {
    const Launch e{"svr_affine_slice", stream};
    if (rows <= 0) return 0;
    if (c_out <= 0 || c_out > c_in) return e.refuse("need 0 < c_out <= c_in");
    if (!in || !out) return e.refuse("null pointer");
    hipLaunchKernelGGL(affine_slice_kernel, dim3(blocks_for(rows * c_out, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)in, (bf16_t*)out, rows, c_in, c_out, scale, shift);
    return e.launched();
}

// ---- edge-guided alpha upscaling (svr_alpha.hip).  Workspace: [flags 4 | maxima T, padded to 4 | n map T*H*W] int32.
static inline int64_t alpha_header_ints(int32_t T) { return 4 + ((int64_t)T + 3) / 4 * 4; }

int64_t svr_alpha_workspace_bytes(int32_t T, int32_t H, int32_t W) {
    if (T < 1 || H < 2 || W < 2) return 0;
    return (alpha_header_ints(T) + (int64_t)T * H * W) * 4;
}

static const char* alpha_args_error(const void* rgb, int32_t T, int32_t H, int32_t W, int64_t ld_px, int32_t rgb_kind,
                                    const void* workspace, int64_t workspace_bytes) {
    if (!rgb || !workspace) return "null pointer";
    if (T < 1 || T > 65535 || H < 2 || W < 2) return "need 1 <= T <= 65535, H >= 2, W >= 2";
    if (ld_px < 3) return "ld_px (elements between pixels) must be >= 3";
    if (rgb_kind != SVR_STORE_BF16 && rgb_kind != SVR_STORE_FP32) return "rgb_kind must be SVR_STORE_BF16 or SVR_STORE_FP32";
    if (workspace_bytes < svr_alpha_workspace_bytes(T, H, W)) return "workspace shorter than svr_alpha_workspace_bytes()";
    return nullptr;
}

int svr_alpha_stats(const float* alpha_lo, int64_t n_alpha, const void* rgb, int32_t T, int32_t H, int32_t W, int64_t ld_px,
                    int32_t rgb_kind, void* workspace, int64_t workspace_bytes, void* stream) {
    const Launch e{"svr_alpha_stats", stream};
    const char* why = alpha_args_error(rgb, T, H, W, ld_px, rgb_kind, workspace, workspace_bytes);
    if (!why && !alpha_lo) why = "null pointer";
    if (!why && (n_alpha < 1 || n_alpha > 0x7fffffff)) why = "need 1 <= n_alpha < 2^31 (the counts are int32)";
    if (why) return e.refuse("%s", why);
    int* flags = (int*)workspace;
    if (int rc = e.hip(hipMemsetAsync(flags, 0, (size_t)alpha_header_ints(T) * 4, (hipStream_t)stream))) return rc;
    const int64_t n_px = (int64_t)T * H * W;
    const unsigned grid = std::min<unsigned>(blocks_for(std::max(n_px, n_alpha), 256 * 8), (unsigned)device_cu_count() * 8);
    with_kind(rgb_kind, [&](auto K) { hipLaunchKernelGGL(alpha_stats_kernel<K()>, dim3(grid), dim3(256), 0, (hipStream_t)stream, alpha_lo, n_alpha, rgb, n_px, ld_px, flags); });
    return e.launched();
}

int svr_alpha_edges(const void* rgb, int32_t T, int32_t H, int32_t W, int64_t ld_px, int32_t rgb_kind, void* workspace,
                    int64_t workspace_bytes, void* stream) {
    const Launch e{"svr_alpha_edges", stream};
    if (const char* why = alpha_args_error(rgb, T, H, W, ld_px, rgb_kind, workspace, workspace_bytes)) return e.refuse("%s", why);
    int* flags = (int*)workspace;
    int* maxima = flags + 4;
    int* nmap = flags + alpha_header_ints(T);
    const dim3 grid(blocks_for(W, ALPHA_TILE), blocks_for(H, ALPHA_TILE), T);
    if (grid.y > 65535u) return e.refuse("H beyond 65535 tiles");
    with_kind(rgb_kind, [&](auto K) { hipLaunchKernelGGL(alpha_edges_kernel<K()>, grid, dim3(256), 0, (hipStream_t)stream, rgb, ld_px, H, W, flags, nmap, maxima); });
    return e.launched();
}

int svr_alpha_refine(const void* rgb, const float* base, float* out, uint8_t* edge_out, int32_t T, int32_t H, int32_t W,
                     int64_t ld_px, int32_t rgb_kind, int64_t n_alpha, const void* workspace, int64_t workspace_bytes, void* stream) {
    const Launch e{"svr_alpha_refine", stream};
    const char* why = alpha_args_error(rgb, T, H, W, ld_px, rgb_kind, workspace, workspace_bytes);
    if (!why && (!base || !out)) why = "null pointer";
    if (!why && (n_alpha < 1 || n_alpha > 0x7fffffff)) why = "need 1 <= n_alpha < 2^31 (the counts are int32)";
    if (why) return e.refuse("%s", why);
    const int* flags = (const int*)workspace;
    const int* maxima = flags + 4;
    const int* nmap = flags + alpha_header_ints(T);
    const dim3 grid(blocks_for(W, ALPHA_TILE), blocks_for(H, ALPHA_TILE), T);
    if (grid.y > 65535u) return e.refuse("H beyond 65535 tiles");
    with_kind(rgb_kind, [&](auto K) { hipLaunchKernelGGL(alpha_refine_kernel<K()>, grid, dim3(256), 0, (hipStream_t)stream, rgb, ld_px, base, H, W, (float)n_alpha, flags, nmap, maxima, out, edge_out); });
    return e.launched();
}

// ---- packed output frames (svr_frame_pack.hip: rgb8 / bgr8; svr_frame_pack_colour.hip: yuv420p10, whichever entry point asks)
// The refusals svr_pack_frames and svr_pack_yuv420p10 share, in the order both report them -> 0, or -1 with the message in g_err.
// ``own``: the caller's refusal of its own format / colour codes (nullptr: none), which ranks between the geometry and the
// alignment.  ``C8``: bytes per pixel of an 8-bit format, 0 for planes: those of ``sub`` in samples of ``sample`` bytes (yuv420p10
// where nothing is said; svr_pack_planar says).  ``needs``: the caller's words.
static int pack_refusal(const Entry& e, const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C8,
                        const char* own, const void* out, int64_t out_bytes, const char* needs, int32_t sub = SVR_PLANAR_420,
                        int32_t sample = 2) {
    const char* why = nullptr;
    if (!frames) why = "frames is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if (x_kind != SVR_STORE_BF16 && x_kind != SVR_STORE_FP32) why = "x_kind must be SVR_STORE_BF16 or SVR_STORE_FP32";
    else if (T < 1 || H < 1 || W < 1) why = "need T >= 1, H >= 1, W >= 1";
    else if ((int64_t)H * W > ((int64_t)1 << 40) / T) why = "T * H * W must not exceed 2^40 pixels";
    else if (own) why = own;
    else if ((uintptr_t)frames % (x_kind == SVR_STORE_FP32 ? 4 : 2)) why = "frames is not aligned to its element size";
    else if (!C8 && sample == 2 && (uintptr_t)out % 2) why = "out is not aligned to 2 bytes";
    if (why) return e.refuse("%s", why);
    const int64_t h2 = sub == SVR_PLANAR_420 ? ((int64_t)H + 1) / 2 : H, w2 = sub == SVR_PLANAR_444 ? W : ((int64_t)W + 1) / 2;
    const int64_t need = C8 ? (int64_t)T * H * W * C8 : sample * (int64_t)T * ((int64_t)H * W + 2 * h2 * w2);
    return out_bytes == need ? 0 : e.wrong_size("out_bytes", out_bytes, needs, need);
}

// Kr, Kb exact decimals, every weight rounded at 2^16, luma deficit to green (frameio.yuv_matrix): wr, wg, wb | cb_r, cb_g | cr_g, cr_b
static PackCoef pack_coef(int32_t matrix, int32_t range) {
    PackCoef k = matrix == SVR_COLOUR_MATRIX_BT709 ? PackCoef{0, 0, 0, 13933, 46871, 4732, -7509, -25259, -29763, -3005}
               : matrix == SVR_COLOUR_MATRIX_BT601 ? PackCoef{0, 0, 0, 19595, 38470, 7471, -11058, -21710, -27439, -5329}
                                                   : PackCoef{0, 0, 0, 17216, 44434, 3886, -9151, -23617, -30133, -2635};
    if (range == SVR_COLOUR_RANGE_TV) { k.y0 = 64; k.ys = 876; k.cs = 896; } else { k.y0 = 0; k.ys = 1023; k.cs = 1023; }
    return k;
}

// the one yuv420p10 launch: 16 x 2 pixels per lane where every row, plane and frame starts on 16 bytes, else one chroma sample
static void launch_pack_yuv420p10(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, const PackCoef& k, bool left,
                                  unsigned short* o, hipStream_t s) {
    const bool vec = (uintptr_t)frames % 16 == 0 && (uintptr_t)o % 16 == 0 && W % 16 == 0;
    const int64_t h2 = ((int64_t)H + 1) / 2, w2 = ((int64_t)W + 1) / 2;
    const unsigned grid = capped_grid((int64_t)T * h2 * (vec ? W / 16 : w2));
    with_kind(x_kind, [&](auto K) { with_const<0, 1>(left, [&](auto LEFT) {
        if (vec) hipLaunchKernelGGL((pack_colour_vec_kernel<K(), LEFT() != 0>), dim3(grid), dim3(256), 0, s, frames, o, T, H, W, k);
        else hipLaunchKernelGGL((pack_colour_kernel<K(), LEFT() != 0>), dim3(grid), dim3(256), 0, s, frames, o, T, H, W, k);
    }); });
}

int svr_pack_frames(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t fmt, void* out,
                    int64_t out_bytes, void* stream) {
    const Launch e{"svr_pack_frames", stream};
    const bool yuv = fmt == SVR_PACK_YUV420P10;
    const char* own = nullptr;
    if (fmt != SVR_PACK_RGB8 && fmt != SVR_PACK_BGR8 && !yuv) own = "fmt must be SVR_PACK_RGB8, SVR_PACK_BGR8 or SVR_PACK_YUV420P10";
    else if (yuv ? C != 3 : (C != 3 && C != 4)) own = yuv ? "C must be 3 for SVR_PACK_YUV420P10" : "C must be 3 or 4";
    if (pack_refusal(e, frames, x_kind, T, H, W, yuv ? 0 : C, own, out, out_bytes, "the format needs")) return -1;
    const hipStream_t s = (hipStream_t)stream;
    if (yuv) {                                                     // BT.709, limited range, centre-sited chroma
        launch_pack_yuv420p10(frames, x_kind, T, H, W, pack_coef(SVR_COLOUR_MATRIX_BT709, SVR_COLOUR_RANGE_TV), false, (unsigned short*)out, s);
        return e.launched();
    }
    const int64_t n = (int64_t)T * H * W * C;
    const int swap = fmt == SVR_PACK_BGR8 ? C : 0;                 // pack8_kernel's C: 0 = samples in place
    const int unit = swap == 3 ? 48 : 16;
    const int64_t n_units = (uintptr_t)frames % 16 == 0 && (uintptr_t)out % 16 == 0 ? n / unit : 0;
    const unsigned grid = capped_grid(std::max<int64_t>(n_units, n - n_units * unit));
    unsigned char* o = (unsigned char*)out;
    with_kind(x_kind, [&](auto K) { with_const<4, 3, 0>(swap, [&](auto CH) {
        hipLaunchKernelGGL((pack8_kernel<K(), CH()>), dim3(grid), dim3(256), 0, s, frames, o, n_units, n);
    }); });
    return e.launched();
}

// ---- yuv420p10 planes with a chosen matrix, range and chroma siting
int svr_pack_yuv420p10(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t matrix, int32_t range,
                       int32_t siting, void* out, int64_t out_bytes, void* stream) {
    const Launch e{"svr_pack_yuv420p10", stream};
    const char* own = nullptr;
    if (matrix != SVR_COLOUR_MATRIX_BT709 && matrix != SVR_COLOUR_MATRIX_BT601 && matrix != SVR_COLOUR_MATRIX_BT2020)
        own = "matrix must be SVR_COLOUR_MATRIX_BT709, SVR_COLOUR_MATRIX_BT601 or SVR_COLOUR_MATRIX_BT2020";
    else if (range != SVR_COLOUR_RANGE_TV && range != SVR_COLOUR_RANGE_PC) own = "range must be SVR_COLOUR_RANGE_TV or SVR_COLOUR_RANGE_PC";
    else if (siting != SVR_COLOUR_SITING_CENTER && siting != SVR_COLOUR_SITING_LEFT) own = "siting must be SVR_COLOUR_SITING_CENTER or SVR_COLOUR_SITING_LEFT";
    if (pack_refusal(e, frames, x_kind, T, H, W, 0, own, out, out_bytes, "the planes need")) return -1;
    launch_pack_yuv420p10(frames, x_kind, T, H, W, pack_coef(matrix, range), siting == SVR_COLOUR_SITING_LEFT, (unsigned short*)out,
                          (hipStream_t)stream);
    return e.launched();
}

// ---- planar YUV planes of a chosen subsampling, depth, matrix, range and chroma siting (svr_planar_out.hip)
int svr_pack_planar(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t sub, int32_t bits, int32_t matrix,
                    int32_t range, int32_t siting, void* out, int64_t out_bytes, void* stream) {
    const Launch e{"svr_pack_planar", stream};
    const char* own = nullptr;
    if (sub != SVR_PLANAR_420 && sub != SVR_PLANAR_422 && sub != SVR_PLANAR_444)
        own = "sub must be SVR_PLANAR_420, SVR_PLANAR_422 or SVR_PLANAR_444";
    else if (bits != 8 && bits != 10 && bits != 12) own = "bits must be 8, 10 or 12";
    else if (matrix != SVR_COLOUR_MATRIX_BT709 && matrix != SVR_COLOUR_MATRIX_BT601 && matrix != SVR_COLOUR_MATRIX_BT2020)
        own = "matrix must be SVR_COLOUR_MATRIX_BT709, SVR_COLOUR_MATRIX_BT601 or SVR_COLOUR_MATRIX_BT2020";
    else if (range != SVR_COLOUR_RANGE_TV && range != SVR_COLOUR_RANGE_PC) own = "range must be SVR_COLOUR_RANGE_TV or SVR_COLOUR_RANGE_PC";
    else if (siting != SVR_COLOUR_SITING_CENTER && siting != SVR_COLOUR_SITING_LEFT && siting != SVR_PLANAR_SITING_TOPLEFT)
        own = "siting must be SVR_COLOUR_SITING_CENTER, SVR_COLOUR_SITING_LEFT or SVR_PLANAR_SITING_TOPLEFT";
    else if (siting == SVR_PLANAR_SITING_TOPLEFT && sub != SVR_PLANAR_420) own = "siting SVR_PLANAR_SITING_TOPLEFT is for SVR_PLANAR_420 only";
    else if (siting == SVR_COLOUR_SITING_CENTER && sub == SVR_PLANAR_444) own = "siting must be SVR_COLOUR_SITING_LEFT for SVR_PLANAR_444";
    const bool wide = bits != 8;                                                       // 16-bit samples
    if (pack_refusal(e, frames, x_kind, T, H, W, 0, own, out, out_bytes, "the planes need", sub, wide ? 2 : 1)) return -1;
    PlanarOutCoef c{pack_coef(matrix, range), 1 << (bits - 1), (1 << bits) - 1};       // (planar.yuv_constants at this depth)
    if (range == SVR_COLOUR_RANGE_TV) { c.k.y0 = 16 << (bits - 8); c.k.ys = 219 << (bits - 8); c.k.cs = 224 << (bits - 8); }
    else { c.k.y0 = 0; c.k.ys = c.k.cs = c.top; }
    const bool vec = (uintptr_t)frames % 16 == 0 && (uintptr_t)out % 16 == 0 && W % 16 == 0;
    const int64_t hc = sub == SVR_PLANAR_420 ? ((int64_t)H + 1) / 2 : H, wc = sub == SVR_PLANAR_444 ? W : ((int64_t)W + 1) / 2;
    const unsigned grid = capped_grid((int64_t)T * hc * (vec ? W / 16 : wc));
    const hipStream_t s = (hipStream_t)stream;
    with_kind(x_kind, [&](auto K) { with_const<SVR_PLANAR_444, SVR_PLANAR_422, SVR_PLANAR_420>(sub, [&](auto SUB) {
        with_const<2, 1, 0>(siting, [&](auto SIT) { with_const<1, 0>(wide, [&](auto WIDE) {
            if constexpr ((SIT() == 2 && SUB() != SVR_PLANAR_420) || (SIT() == 0 && SUB() == SVR_PLANAR_444)) return;   // (refused above)
            else if (vec) hipLaunchKernelGGL((planar_out_vec_kernel<K(), SUB(), SIT(), WIDE() != 0>), dim3(grid), dim3(256), 0, s, frames, out,
                                             T, H, W, c);
            else hipLaunchKernelGGL((planar_out_kernel<K(), SUB(), SIT(), WIDE() != 0>), dim3(grid), dim3(256), 0, s, frames, out, T, H, W, c);
        }); });
    }); });
    return e.launched();
}

// ---- frame signatures for cut detection (svr_shots.hip)
int svr_frame_signatures(const void* frames, int32_t kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t* sig,
                         int64_t sig_bytes, void* stream) {
    const Launch e{"svr_frame_signatures", stream};
    const char* why = nullptr;
    if (!frames) why = "frames is a null pointer";
    else if (!sig) why = "sig is a null pointer";
    else if (kind != SVR_STORE_BF16 && kind != SVR_STORE_FP32) why = "kind must be SVR_STORE_BF16 or SVR_STORE_FP32";
    else if (T < 1) why = "need T >= 1";
    else if (H < 4) why = "H must be at least 4 (one pixel row per cell row)";
    else if (W < 4) why = "W must be at least 4 (one pixel column per cell column)";
    else if (C != 3 && C != 4) why = "C must be 3 or 4";
    else if ((int64_t)H * W >= ((int64_t)1 << 31)) why = "H * W must stay below 2^31 pixels (the counters are int32)";
    else if ((uintptr_t)frames % (kind == SVR_STORE_FP32 ? 4 : 2)) why = "frames is not aligned to its element size";
    else if ((uintptr_t)sig % 4) why = "sig is not aligned to 4 bytes";
    if (why) return e.refuse("%s", why);
    if (sig_bytes != (int64_t)T * 4096) return e.wrong_size("sig_bytes", sig_bytes, "int32 [T, 1024] is", (int64_t)T * 4096);
    const int bands = (int)((((int64_t)H + 3) / 4 + SIG_BAND_ROWS - 1) / SIG_BAND_ROWS);      // of the tallest cell row
    const int64_t grid = (int64_t)T * 4 * bands;
    if (grid > 0x7fffffffll) return e.refuse("T * H needs more than 2^31 - 1 workgroups");
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = e.hip(hipMemsetAsync(sig, 0, (size_t)sig_bytes, s))) return rc;
    const int vec = (uintptr_t)frames % 16 == 0;
    with_kind(kind, [&](auto K) { with_const<4, 3>(C, [&](auto CH) {
        hipLaunchKernelGGL((signature_kernel<K(), CH()>), dim3((unsigned)grid), dim3(256), 0, s, frames, (int*)sig, H, W, bands, vec);
    }); });
    return e.launched();
}

// ---- active-area profile of a letterboxed clip (svr_active.hip)
int svr_active_profile(const void* frames, int32_t kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t dark, int32_t* out,
                       int64_t out_bytes, void* stream) {
    const Launch e{"svr_active_profile", stream};
    const char* why = nullptr;
    if (!frames) why = "frames is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if (kind != SVR_STORE_BF16 && kind != SVR_STORE_FP32) why = "kind must be SVR_STORE_BF16 or SVR_STORE_FP32";
    else if (T < 1) why = "need T >= 1";
    else if (H < 1) why = "H must be at least 1";
    else if (W < 1) why = "W must be at least 1";
    else if (C != 3 && C != 4) why = "C must be 3 or 4";
    else if (dark < 0 || dark > 255) why = "dark must lie in 0..255";
    else if ((int64_t)T * (H > W ? H : W) >= ((int64_t)1 << 31)) why = "T * max(H, W) must stay below 2^31 (the counters are int32)";
    else if ((uintptr_t)frames % (kind == SVR_STORE_FP32 ? 4 : 2)) why = "frames is not aligned to its element size";
    else if ((uintptr_t)out % 4) why = "out is not aligned to 4 bytes";
    if (why) return e.refuse("%s", why);
    if (out_bytes != ((int64_t)H + W) * 4) return e.wrong_size("out_bytes", out_bytes, "int32 [H + W] is", ((int64_t)H + W) * 4);
    const int bands = (int)(((int64_t)H + ACT_BAND_ROWS - 1) / ACT_BAND_ROWS);
    const int64_t grid = (int64_t)T * bands;                                                  // <= T * H < 2^31
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = e.hip(hipMemsetAsync(out, 0, (size_t)out_bytes, s))) return rc;
    const int vec = (uintptr_t)frames % 16 == 0;
    with_kind(kind, [&](auto K) { with_const<4, 3>(C, [&](auto CH) {
        hipLaunchKernelGGL((active_profile_kernel<K(), CH()>), dim3((unsigned)grid), dim3(256), 0, s, frames, (int*)out, H, W, bands, (uint32_t)dark, vec);
    }); });
    return e.launched();
}

// ---- PNG streams encoded on the device (svr_png.hip)
static const char* png_geometry_refusal(int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth) {
    if (C != 3 && C != 4) return "C must be 3 or 4";
    if (depth != 8 && depth != 16) return "depth must be 8 or 16";
    if (T < 1 || H < 1 || W < 1) return "need T >= 1, H >= 1, W >= 1";
    if (H > (1 << 24)) return "H must not exceed 2^24 rows";
    if ((int64_t)W * (C * depth / 8) >= (1 << 24)) return "W must stay below 2^24 bytes per row";
    if ((int64_t)T * H > 0x7FFFFFFFll) return "T * H must stay below 2^31 rows";
    return nullptr;
}

static int png_encode_bytes(const Entry& e, bool runs, int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, int64_t* scratch_bytes,
                            int64_t* capacity) {
    if (const char* why = png_geometry_refusal(T, H, W, C, depth)) return e.refuse("%s", why);
    const PngLayout L = png_layout(T, H, W, C, depth, runs);
    if (scratch_bytes) *scratch_bytes = L.scratch_bytes;
    if (capacity) *capacity = L.capacity;
    return 0;
}

static int png_encode(const Entry& e, bool runs, const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C,
                      int32_t depth, void* scratch, int64_t scratch_bytes, void* out, int64_t out_capacity, int64_t* sizes, void* stream) {
    const char* why = nullptr;
    if (!frames) why = "frames is a null pointer";
    else if (!scratch) why = "scratch is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if (!sizes) why = "sizes is a null pointer";
    else if (x_kind != SVR_STORE_BF16 && x_kind != SVR_STORE_FP32) why = "x_kind must be SVR_STORE_BF16 or SVR_STORE_FP32";
    else if ((why = png_geometry_refusal(T, H, W, C, depth))) {}
    else if ((uintptr_t)frames % (x_kind == SVR_STORE_FP32 ? 4 : 2)) why = "frames is not aligned to its element size";
    else if ((uintptr_t)scratch % 16) why = "scratch is not aligned to 16 bytes";
    else if ((uintptr_t)sizes % 8) why = "sizes is not aligned to 8 bytes";
    if (why) return e.refuse("%s", why);
    const PngLayout L = png_layout(T, H, W, C, depth, runs);
    if (scratch_bytes < L.scratch_bytes)
        return e.refuse("scratch_bytes is %lld, the geometry needs at least %lld", (long long)scratch_bytes, (long long)L.scratch_bytes);
    if (out_capacity < L.capacity)
        return e.refuse("out_capacity is %lld per frame, the geometry needs at least %lld", (long long)out_capacity, (long long)L.capacity);
    const hipStream_t s = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)scratch;
    unsigned char* filt = base + L.filt_off;
    uint32_t* table = (uint32_t*)(base + L.table_off);
    uint32_t* meta = (uint32_t*)(base + L.meta_off);
    int64_t* segoff = (int64_t*)(base + L.segoff_off);
    uint32_t* table2 = (uint32_t*)(base + L.table2_off);         // (inside the scratch with runs only, and only then used)
    const dim3 grid((unsigned)((int64_t)T * L.nseg)), block(256);
    with_kind(x_kind, [&](auto K) { with_const<16, 8>(depth, [&](auto DEPTH) { with_const<4, 3>(C, [&](auto CH) {
        hipLaunchKernelGGL((png_filter_kernel<K(), DEPTH(), CH()>), grid, block, 0, s, frames, filt, table, meta, H, W, L.R, L.nseg);
    }); }); });
    // (g_png_passes < 3, tools/png_encode_timing.py only: the launches up to that pass, to time them by difference; with runs the
    // token + second code pass counts with the scan, so that the first figure is the same work in both modes)
    if (runs && g_png_passes >= 2) hipLaunchKernelGGL(png_runs_kernel, grid, block, 0, s, filt, table2, meta, H, L.stride, L.R, L.nseg);
    if (g_png_passes >= 2) hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)T), block, 0, s, meta, segoff, (unsigned char*)out, out_capacity, sizes, H, L.stride, L.R, L.nseg);
    if (g_png_passes >= 3) {
        if (runs) hipLaunchKernelGGL(png_pack_kernel<true>, grid, block, 0, s, filt, table, table2, meta, segoff, (unsigned char*)out, out_capacity, H, L.stride, L.R, L.nseg);
        else hipLaunchKernelGGL(png_pack_kernel<false>, grid, block, 0, s, filt, table, table2, meta, segoff, (unsigned char*)out, out_capacity, H, L.stride, L.R, L.nseg);
    }
    return e.launched();
}

int svr_png_encode_bytes(int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, int64_t* scratch_bytes, int64_t* capacity) {
    return png_encode_bytes(Entry{"svr_png_encode_bytes"}, false, T, H, W, C, depth, scratch_bytes, capacity);
}

int svr_png_encode(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, void* scratch,
                   int64_t scratch_bytes, void* out, int64_t out_capacity, int64_t* sizes, void* stream) {
    return png_encode(Launch{"svr_png_encode", stream}, false, frames, x_kind, T, H, W, C, depth, scratch, scratch_bytes, out, out_capacity, sizes, stream);
}

int svr_png_encode_runs_bytes(int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, int64_t* scratch_bytes, int64_t* capacity) {
    return png_encode_bytes(Entry{"svr_png_encode_runs_bytes"}, true, T, H, W, C, depth, scratch_bytes, capacity);
}

int svr_png_encode_runs(const void* frames, int32_t x_kind, int32_t T, int32_t H, int32_t W, int32_t C, int32_t depth, void* scratch,
                        int64_t scratch_bytes, void* out, int64_t out_capacity, int64_t* sizes, void* stream) {
    return png_encode(Launch{"svr_png_encode_runs", stream}, true, frames, x_kind, T, H, W, C, depth, scratch, scratch_bytes, out, out_capacity, sizes, stream);
}

// ---- colour correction (svr_colorfix.hip).  Every argument is checked here, before any launch.
static const char* colorfix_strides(const int64_t* st, bool is_output, PixStrides& s) {
    if (!st) return "is a null pointer";
    for (int i = 0; i < 4; ++i)
        if (st[i] < (is_output ? 1 : 0)) return is_output ? "holds a stride below 1" : "holds a negative stride";
    s = PixStrides{st[0], st[1], st[2], st[3]};
    return nullptr;
}
static const char* colorfix_geometry(int32_t T, int32_t H, int32_t W, int32_t kind) {
    if (kind != SVR_STORE_FP32) return "kind must be SVR_STORE_FP32";
    if (T < 1 || T > 21845) return "need 1 <= T <= 21845";
    if (H < 1 || W < 1) return "need H >= 1 and W >= 1";
    // (a launch's threads per grid dimension are a 32-bit count: 2^24 workgroups of 256)
    if ((int64_t)T * H * (((int64_t)W + COLORFIX_ROW_PIXELS - 1) / COLORFIX_ROW_PIXELS) >= (1ll << 24)) return "T * H * ceil(W / 256) must stay below 2^24";
    if (((int64_t)H + WAVELET_TILE - 1) / WAVELET_TILE > 65535) return "H beyond 65535 tiles";
    return nullptr;
}
// thin over the Entry ``e`` of the entry point that uses them: they name the argument they refuse by its spelling
#define SVR_COLORFIX_PTR(p) do { if (!(p)) return e.refuse(#p " is a null pointer"); } while (0)
#define SVR_COLORFIX_STRIDES(st, is_output, dst) do { if (const char* w_ = colorfix_strides(st, is_output, dst)) return e.refuse(#st " %s", w_); } while (0)
#define SVR_COLORFIX_GEOMETRY() do { if (const char* w_ = colorfix_geometry(T, H, W, kind)) return e.refuse("%s", w_); } while (0)

int64_t svr_colorfix_workspace_bytes(int32_t T) {
    if (T < 1 || T > 21845) return 0;
    return (int64_t)2 * T * 3 * CHAN_STATS_PARTS * 2 * (int64_t)sizeof(double);
}

int svr_wavelet_reconstruct(const void* content, const int64_t* content_strides, const void* style, const int64_t* style_strides,
                            void* out, const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream) {
    const Launch e{"svr_wavelet_reconstruct", stream};
    PixStrides cs, ss, os;
    SVR_COLORFIX_PTR(content);
    SVR_COLORFIX_PTR(style);
    SVR_COLORFIX_PTR(out);
    SVR_COLORFIX_STRIDES(content_strides, false, cs);
    SVR_COLORFIX_STRIDES(style_strides, false, ss);
    SVR_COLORFIX_STRIDES(out_strides, true, os);
    SVR_COLORFIX_GEOMETRY();
    WaveletRadii radii;
    int halo = 0;
    for (int i = 0; i < WAVELET_LEVELS; ++i) halo += radii.r[i] = std::min(1 << i, std::max(1, std::min(H, W) / 8));
    static uint64_t lds_attr_done = 0;               // per device (svr_common.h)
    if (int rc = set_max_dynamic_lds((const void*)wavelet_kernel, WAVELET_LDS_BYTES, lds_attr_done)) return e.hip(rc);
    const dim3 grid(blocks_for(W, WAVELET_TILE), blocks_for(H, WAVELET_TILE), (unsigned)T * 3);
    hipLaunchKernelGGL(wavelet_kernel, grid, dim3(WAVELET_THREADS), WAVELET_LDS_BYTES, (hipStream_t)stream, (const float*)content, cs,
                       (const float*)style, ss, (float*)out, os, H, W, radii, halo);
    return e.launched();
}

int svr_lab_planes(const void* base, const int64_t* base_strides, const void* style, const int64_t* style_strides, void* c_lab,
                   void* s_lab, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream) {
    const Launch e{"svr_lab_planes", stream};
    PixStrides bs, ss;
    SVR_COLORFIX_PTR(base);
    SVR_COLORFIX_PTR(style);
    SVR_COLORFIX_PTR(c_lab);
    SVR_COLORFIX_PTR(s_lab);
    SVR_COLORFIX_STRIDES(base_strides, false, bs);
    SVR_COLORFIX_STRIDES(style_strides, false, ss);
    SVR_COLORFIX_GEOMETRY();
    const int chunks = (int)blocks_for(W, COLORFIX_ROW_PIXELS);
    const dim3 grid((unsigned)((int64_t)T * H * chunks), 2);
    hipLaunchKernelGGL(lab_planes_kernel, grid, dim3(COLORFIX_ROW_PIXELS), 0, (hipStream_t)stream, (const float*)base, bs,
                       (const float*)style, ss, (float*)c_lab, (float*)s_lab, H, W, chunks, (int64_t)T * H * W);
    return e.launched();
}

int svr_lab_merge(const void* c_L, const void* m_L, const void* m_a, const void* m_b, double luminance_weight, void* out,
                  const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream) {
    const Launch e{"svr_lab_merge", stream};
    PixStrides os;
    const bool blend = luminance_weight < 1.0;
    SVR_COLORFIX_PTR(c_L);
    if (blend) SVR_COLORFIX_PTR(m_L);
    SVR_COLORFIX_PTR(m_a);
    SVR_COLORFIX_PTR(m_b);
    SVR_COLORFIX_PTR(out);
    SVR_COLORFIX_STRIDES(out_strides, true, os);
    if (!(luminance_weight == luminance_weight)) return e.refuse("luminance_weight is not a number");
    SVR_COLORFIX_GEOMETRY();
    const int chunks = (int)blocks_for(W, COLORFIX_ROW_PIXELS);
    // (both factors rounded from fp64 once, as torch rounds the Python scalars luminance_weight and 1.0 - luminance_weight)
    hipLaunchKernelGGL(lab_merge_kernel, dim3((unsigned)((int64_t)T * H * chunks)), dim3(COLORFIX_ROW_PIXELS), 0, (hipStream_t)stream,
                       (const float*)c_L, blend ? (const float*)m_L : nullptr, (const float*)m_a, (const float*)m_b,
                       (float)luminance_weight, (float)(1.0 - luminance_weight), (float*)out, os, H, W, chunks);
    return e.launched();
}

int svr_chan_stats(const void* content, const int64_t* content_strides, const void* style, const int64_t* style_strides, void* stats,
                   int32_t T, int32_t H, int32_t W, int32_t kind, void* workspace, int64_t workspace_bytes, void* stream) {
    const Launch e{"svr_chan_stats", stream};
    PixStrides cs, ss;
    SVR_COLORFIX_PTR(content);
    SVR_COLORFIX_PTR(style);
    SVR_COLORFIX_PTR(stats);
    SVR_COLORFIX_PTR(workspace);
    SVR_COLORFIX_STRIDES(content_strides, false, cs);
    SVR_COLORFIX_STRIDES(style_strides, false, ss);
    SVR_COLORFIX_GEOMETRY();
    if ((uintptr_t)workspace % 8) return e.refuse("workspace is not aligned to 8 bytes");
    if (workspace_bytes < svr_colorfix_workspace_bytes(T)) return e.refuse("workspace_bytes is below svr_colorfix_workspace_bytes(T)");
    hipLaunchKernelGGL(chan_stats_kernel, dim3(CHAN_STATS_PARTS, (unsigned)T * 3, 2), dim3(256), 0, (hipStream_t)stream,
                       (const float*)content, cs, (const float*)style, ss, H, W, (double*)workspace);
    hipLaunchKernelGGL(chan_stats_finish_kernel, dim3(blocks_for((int64_t)2 * T * 3, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double*)workspace, T * 3, (double)H * (double)W, (float*)stats);
    return e.launched();
}

int svr_adain_apply(const void* content, const int64_t* content_strides, const void* stats, float eps, void* out,
                    const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream) {
    const Launch e{"svr_adain_apply", stream};
    PixStrides cs, os;
    SVR_COLORFIX_PTR(content);
    SVR_COLORFIX_PTR(stats);
    SVR_COLORFIX_PTR(out);
    SVR_COLORFIX_STRIDES(content_strides, false, cs);
    SVR_COLORFIX_STRIDES(out_strides, true, os);
    SVR_COLORFIX_GEOMETRY();
    const int chunks = (int)blocks_for(W, COLORFIX_ROW_PIXELS);
    hipLaunchKernelGGL(adain_apply_kernel, dim3((unsigned)((int64_t)T * H * chunks)), dim3(COLORFIX_ROW_PIXELS), 0, (hipStream_t)stream,
                       (const float*)content, cs, (const float*)stats, eps, (float*)out, os, H, W, chunks);
    return e.launched();
}

// ---- rank matching (svr_rank.hip): a stable radix sort of fp32 keys and the scatter that hands out the sorted reference.
// Workspace (bytes; n4 = 4 * n rounded up to 256): [sorted reference values n4][keys A n4][indices A n4][keys B n4][indices B n4]
// [table 256 * tiles_p * 4][totals 1024], tiles_p = ceil(n / 4096) rounded up to 16.
struct RankPlan {
    uint32_t n, tiles_p, groups;
    char *ref, *keys[2], *idx[2];
    uint32_t *table, *totals;
    int64_t bytes;
};
static RankPlan rank_plan(int64_t n, void* workspace) {
    RankPlan p;
    const int64_t tiles = (n + RANK_TILE - 1) / RANK_TILE, n4 = (4 * n + 255) / 256 * 256;
    p.n = (uint32_t)n;
    p.groups = (uint32_t)((tiles + RANK_GROUP - 1) / RANK_GROUP);
    p.tiles_p = p.groups * RANK_GROUP;
    char* w = (char*)workspace;
    p.ref = w;
    p.keys[0] = w + n4; p.idx[0] = w + 2 * n4; p.keys[1] = w + 3 * n4; p.idx[1] = w + 4 * n4;
    p.table = (uint32_t*)(w + 5 * n4);
    p.totals = p.table + (int64_t)RANK_RADIX * p.tiles_p;
    p.bytes = 5 * n4 + (int64_t)RANK_RADIX * p.tiles_p * 4 + RANK_RADIX * 4;
    return p;
}
// The four passes of one sort: in -> A -> B -> A -> (out_keys, out_idx).  pairs: indices travel with the keys (the first pass
// makes them: a key's place in ``in``).  out_mode: what the last pass stores (svr_rank.hip, rank_scatter_kernel).  keyed: ``in``
// holds keys already, not fp32 values, and (pairs) ``in_idx`` their indices: a run of a partition (svr_hue_match); no pass is a
// first pass then.
static void rank_sort_launch(const RankPlan& p, const void* in, bool pairs, int out_mode, void* out_keys, void* out_idx, hipStream_t s,
                             bool keyed = false, const void* in_idx = nullptr) {
    const void* src_k = in;
    const void* src_i = keyed ? in_idx : nullptr;
    for (int pass = 0; pass < 32 / RANK_BITS; ++pass) {
        const bool last = pass == 32 / RANK_BITS - 1;
        const int shift = pass * RANK_BITS, first = pass == 0 && !keyed, mode = last ? out_mode : 0;
        void* dst_k = last ? out_keys : p.keys[pass & 1];
        void* dst_i = last ? out_idx : p.idx[pass & 1];
        hipLaunchKernelGGL(rank_hist_kernel<0>, dim3(p.groups), dim3(RANK_THREADS), 0, s, (const uint32_t*)src_k, (const float*)nullptr, p.n, shift, first, p.table, p.tiles_p);
        // (g_rank_launches < 3, tools/colorfix_timing.py only: every pass's launches up to that one, to time them by difference; the
        // passes then read what an earlier whole sort left in the workspace and the outputs are not written)
        if (g_rank_launches >= 2) hipLaunchKernelGGL(rank_scan_kernel, dim3(RANK_RADIX), dim3(RANK_THREADS), 0, s, p.table, p.tiles_p, p.totals);
        if (g_rank_launches < 3) { src_k = p.keys[pass & 1]; src_i = p.idx[pass & 1]; continue; }
        if (pairs)
            hipLaunchKernelGGL((rank_scatter_kernel<true, 0>), dim3(p.groups), dim3(RANK_THREADS), 0, s, (const uint32_t*)src_k, (const uint32_t*)src_i,
                               (const float*)nullptr, p.n, shift, first, mode, (const uint32_t*)p.table, p.tiles_p, (const uint32_t*)p.totals, (uint32_t*)dst_k, (uint32_t*)dst_i);
        else
            hipLaunchKernelGGL((rank_scatter_kernel<false, 0>), dim3(p.groups), dim3(RANK_THREADS), 0, s, (const uint32_t*)src_k, (const uint32_t*)nullptr,
                               (const float*)nullptr, p.n, shift, first, mode, (const uint32_t*)p.table, p.tiles_p, (const uint32_t*)p.totals, (uint32_t*)dst_k, (uint32_t*)nullptr);
        src_k = dst_k; src_i = dst_i;
    }
}
static bool rank_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}
// (``bytes_fn``: svr_rank_workspace_bytes or svr_hue_match_workspace_bytes, named in the refusal)
#define SVR_RANK_N_AND_WORKSPACE(bytes_fn) do { \
        if (n < 1 || n > RANK_MAX_N) return e.refuse("n must be in [1, 2^30]"); \
        if ((uintptr_t)workspace % 16) return e.refuse("workspace is not aligned to 16 bytes"); \
        if (workspace_bytes < bytes_fn(n)) return e.refuse("workspace_bytes is below " #bytes_fn "(n)"); \
    } while (0)
#define SVR_RANK_ALIGNED(p) do { if ((uintptr_t)(p) % 4) return e.refuse(#p " is not aligned to 4 bytes"); } while (0)
#define SVR_RANK_APART(a, b) do { if (rank_overlap(a, 4 * n, b, 4 * n)) return e.refuse(#a " overlaps " #b); } while (0)
#define SVR_RANK_OFF_WORKSPACE(a, bytes) do { if (rank_overlap(a, 4 * n, workspace, bytes)) return e.refuse(#a " overlaps workspace"); } while (0)

int64_t svr_rank_workspace_bytes(int64_t n) {
    if (n < 1 || n > RANK_MAX_N) return 0;
    return rank_plan(n, nullptr).bytes;
}

int svr_rank_geometry(int32_t* out2) {
    const Entry e{"svr_rank_geometry"};
    SVR_COLORFIX_PTR(out2);
    out2[0] = RANK_TILE;
    out2[1] = 0;                                     // rank_scan_kernel walks a row of any length with a carry
    return 0;
}

int svr_sort_f32(const void* keys, int64_t n, void* sorted, void* index, void* workspace, int64_t workspace_bytes, void* stream) {
    const Launch e{"svr_sort_f32", stream};
    SVR_COLORFIX_PTR(keys);
    SVR_COLORFIX_PTR(sorted);
    SVR_COLORFIX_PTR(workspace);
    SVR_RANK_N_AND_WORKSPACE(svr_rank_workspace_bytes);
    const int64_t need = svr_rank_workspace_bytes(n);
    SVR_RANK_ALIGNED(keys);
    SVR_RANK_ALIGNED(sorted);
    SVR_RANK_ALIGNED(index);
    SVR_RANK_APART(sorted, keys);
    if (index) {
        SVR_RANK_APART(index, keys);
        SVR_RANK_APART(index, sorted);
        SVR_RANK_OFF_WORKSPACE(index, need);
    }
    SVR_RANK_OFF_WORKSPACE(keys, need);
    SVR_RANK_OFF_WORKSPACE(sorted, need);
    const RankPlan p = rank_plan(n, workspace);
    rank_sort_launch(p, keys, index != nullptr, 1, sorted, index, (hipStream_t)stream);
    return e.launched();
}

int svr_rank_match(const void* source, const void* reference, int64_t n, void* out, void* workspace, int64_t workspace_bytes, void* stream) {
    const Launch e{"svr_rank_match", stream};
    SVR_COLORFIX_PTR(source);
    SVR_COLORFIX_PTR(reference);
    SVR_COLORFIX_PTR(out);
    SVR_COLORFIX_PTR(workspace);
    if (g_rank_launches != 3) return e.refuse("svr_set_option(\"rank_launches\") below 3 serves svr_sort_f32 only");
    SVR_RANK_N_AND_WORKSPACE(svr_rank_workspace_bytes);
    const int64_t need = svr_rank_workspace_bytes(n);
    SVR_RANK_ALIGNED(source);
    SVR_RANK_ALIGNED(reference);
    SVR_RANK_ALIGNED(out);
    SVR_RANK_APART(out, reference);
    if (out != source) SVR_RANK_APART(out, source);          // out == source: the plane is matched in place
    SVR_RANK_APART(source, reference);
    SVR_RANK_OFF_WORKSPACE(source, need);
    SVR_RANK_OFF_WORKSPACE(reference, need);
    SVR_RANK_OFF_WORKSPACE(out, need);
    const RankPlan p = rank_plan(n, workspace);
    const hipStream_t s = (hipStream_t)stream;
    rank_sort_launch(p, reference, false, 1, p.ref, nullptr, s);               // the reference's sorted values stay in the workspace
    rank_sort_launch(p, source, true, 2, nullptr, p.idx[1], s);                // source: only where each rank came from is kept
    hipLaunchKernelGGL(rank_apply_kernel, dim3(blocks_for(n, 1024)), dim3(256), 0, s, (const uint32_t*)p.idx[1], (const uint32_t*)p.ref,
                       p.n, (uint32_t*)out);
    return e.launched();
}

// ---- the HSV half (svr_hsv.hip)
int svr_hsv_planes(const void* content, const int64_t* content_strides, const void* style, const int64_t* style_strides, void* c_hsv,
                   void* s_hs, int32_t T, int32_t H, int32_t W, int32_t kind, void* stream) {
    const Launch e{"svr_hsv_planes", stream};
    PixStrides cs, ss;
    SVR_COLORFIX_PTR(content);
    SVR_COLORFIX_PTR(style);
    SVR_COLORFIX_PTR(c_hsv);
    SVR_COLORFIX_PTR(s_hs);
    SVR_COLORFIX_STRIDES(content_strides, false, cs);
    SVR_COLORFIX_STRIDES(style_strides, false, ss);
    SVR_COLORFIX_GEOMETRY();
    const int chunks = (int)blocks_for(W, COLORFIX_ROW_PIXELS);
    const dim3 grid((unsigned)((int64_t)T * H * chunks), 2);
    hipLaunchKernelGGL(hsv_planes_kernel, grid, dim3(COLORFIX_ROW_PIXELS), 0, (hipStream_t)stream, (const float*)content, cs,
                       (const float*)style, ss, (float*)c_hsv, (float*)s_hs, H, W, chunks, (int64_t)T * H * W);
    return e.launched();
}

int svr_hsv_merge(const void* h, const void* sat, const void* v, void* out, const int64_t* out_strides, int32_t T, int32_t H, int32_t W,
                  int32_t kind, void* stream) {
    const Launch e{"svr_hsv_merge", stream};
    PixStrides os;
    SVR_COLORFIX_PTR(h);
    SVR_COLORFIX_PTR(sat);
    SVR_COLORFIX_PTR(v);
    SVR_COLORFIX_PTR(out);
    SVR_COLORFIX_STRIDES(out_strides, true, os);
    SVR_COLORFIX_GEOMETRY();
    const int chunks = (int)blocks_for(W, COLORFIX_ROW_PIXELS);
    hipLaunchKernelGGL(hsv_merge_kernel, dim3((unsigned)((int64_t)T * H * chunks)), dim3(COLORFIX_ROW_PIXELS), 0, (hipStream_t)stream,
                       (const float*)h, (const float*)sat, (const float*)v, (float*)out, os, H, W, chunks);
    return e.launched();
}

int svr_adaptive_blend(const void* base, const int64_t* base_strides, const void* content, const int64_t* content_strides,
                       const void* style, const int64_t* style_strides, const void* h, const void* sat, const void* v, double threshold,
                       double sharpness, void* out, const int64_t* out_strides, int32_t T, int32_t H, int32_t W, int32_t kind,
                       void* stream) {
    const Launch e{"svr_adaptive_blend", stream};
    PixStrides bs, cs, ss, os;
    SVR_COLORFIX_PTR(base);
    SVR_COLORFIX_PTR(content);
    SVR_COLORFIX_PTR(style);
    SVR_COLORFIX_PTR(h);
    SVR_COLORFIX_PTR(sat);
    SVR_COLORFIX_PTR(v);
    SVR_COLORFIX_PTR(out);
    SVR_COLORFIX_STRIDES(base_strides, false, bs);
    SVR_COLORFIX_STRIDES(content_strides, false, cs);
    SVR_COLORFIX_STRIDES(style_strides, false, ss);
    SVR_COLORFIX_STRIDES(out_strides, true, os);
    if (!(threshold == threshold)) return e.refuse("threshold is not a number");
    if (!(sharpness == sharpness)) return e.refuse("sharpness is not a number");
    SVR_COLORFIX_GEOMETRY();
    const int chunks = (int)blocks_for(W, COLORFIX_ROW_PIXELS);
    hipLaunchKernelGGL(adaptive_blend_kernel, dim3((unsigned)((int64_t)T * H * chunks)), dim3(COLORFIX_ROW_PIXELS), 0, (hipStream_t)stream,
                       (const float*)base, bs, (const float*)content, cs, (const float*)style, ss, (const float*)h, (const float*)sat,
                       (const float*)v, (float)threshold, (float)(threshold * 0.5), (float)sharpness, (float*)out, os, H, W, chunks);
    return e.launched();
}

// Hue-conditional rank matching.  Workspace (bytes; n4 = 4 * n rounded up to 256): [source keys by class n4][source indices by class
// n4][source keys, bin 0 first n4][source indices, bin 0 first n4][reference keys by class n4][class counts: source 1024, reference
// 1024, bin-0 partition 1024][the workspace of one sort of n keys: svr_rank_workspace_bytes(n)].
constexpr int HUE_MIN_PIXELS = 100;                 // a bin is matched when both sides hold MORE pixels than this
struct HuePlan {
    RankPlan sort;                                  // buffers, table and geometry of a sort of all n keys
    char *cls_k, *cls_i, *bin0_k, *bin0_i, *ref_k;
    uint32_t *tot_src, *tot_ref, *tot_bin0;
    int64_t bytes;
};
static HuePlan hue_plan(int64_t n, void* workspace) {
    HuePlan p;
    const int64_t n4 = (4 * n + 255) / 256 * 256;
    char* w = (char*)workspace;
    p.cls_k = w; p.cls_i = w + n4; p.bin0_k = w + 2 * n4; p.bin0_i = w + 3 * n4; p.ref_k = w + 4 * n4;
    p.tot_src = (uint32_t*)(w + 5 * n4);
    p.tot_ref = p.tot_src + RANK_RADIX;
    p.tot_bin0 = p.tot_ref + RANK_RADIX;
    p.sort = rank_plan(n, w + 5 * n4 + 3 * RANK_RADIX * 4);
    p.bytes = 5 * n4 + 3 * RANK_RADIX * 4 + p.sort.bytes;
    return p;
}
// the sort of a run of m <= n keys in the buffers of the sort of n: the same addresses whatever m is (a run's sorted reference stays
// where the next sort does not write), its own tile counts
static RankPlan hue_run_plan(const RankPlan& whole, uint32_t m) {
    RankPlan p = whole;
    p.n = m;
    p.groups = (uint32_t)(((int64_t)m + (int64_t)RANK_GROUP * RANK_TILE - 1) / ((int64_t)RANK_GROUP * RANK_TILE));
    p.tiles_p = p.groups * RANK_GROUP;
    return p;
}
// one pass whose digit is the hue's (svr_rank.hip, DIGIT 1: the class, or 2: outside bin 0): keys (and flat indices) of ``sat`` in the
// stable order of the digit.  ``out_idx`` is nullptr where ``pairs`` is false
static void hue_partition_launch(const RankPlan& p, bool by_class, const void* sat, const void* hue, bool pairs, uint32_t* totals,
                                 void* out_keys, void* out_idx, hipStream_t s) {
    with_const<2, 1>(by_class ? 1 : 2, [&](auto DIGIT) {
        hipLaunchKernelGGL(rank_hist_kernel<DIGIT()>, dim3(p.groups), dim3(RANK_THREADS), 0, s, (const uint32_t*)sat, (const float*)hue, p.n, 0, 1,
                           p.table, p.tiles_p);
    });
    hipLaunchKernelGGL(rank_scan_kernel, dim3(RANK_RADIX), dim3(RANK_THREADS), 0, s, p.table, p.tiles_p, totals);
    auto scatter = [&](auto PAIRS, auto DIGIT) {
        hipLaunchKernelGGL((rank_scatter_kernel<PAIRS(), DIGIT()>), dim3(p.groups), dim3(RANK_THREADS), 0, s, (const uint32_t*)sat,
                           (const uint32_t*)nullptr, (const float*)hue, p.n, 0, 1, 0, (const uint32_t*)p.table, p.tiles_p,
                           (const uint32_t*)totals, (uint32_t*)out_keys, (uint32_t*)out_idx);
    };
    if (!by_class) scatter(std::true_type{}, std::integral_constant<int, 2>{});      // (the partition of bin 0 serves the source side only)
    else if (pairs) scatter(std::true_type{}, std::integral_constant<int, 1>{});
    else scatter(std::false_type{}, std::integral_constant<int, 1>{});
}

int64_t svr_hue_match_workspace_bytes(int64_t n) {
    if (n < 1 || n > RANK_MAX_N) return 0;
    return hue_plan(n, nullptr).bytes;
}

int svr_hue_match(const void* c_h, const void* c_s, const void* s_h, const void* s_s, int64_t n, void* out, void* workspace,
                  int64_t workspace_bytes, void* stream) {
    const Launch e{"svr_hue_match", stream};
    SVR_COLORFIX_PTR(c_h);
    SVR_COLORFIX_PTR(c_s);
    SVR_COLORFIX_PTR(s_h);
    SVR_COLORFIX_PTR(s_s);
    SVR_COLORFIX_PTR(out);
    SVR_COLORFIX_PTR(workspace);
    if (g_rank_launches != 3) return e.refuse("svr_set_option(\"rank_launches\") below 3 serves svr_sort_f32 only");
    SVR_RANK_N_AND_WORKSPACE(svr_hue_match_workspace_bytes);
    const int64_t need = svr_hue_match_workspace_bytes(n);
    SVR_RANK_ALIGNED(c_h);
    SVR_RANK_ALIGNED(c_s);
    SVR_RANK_ALIGNED(s_h);
    SVR_RANK_ALIGNED(s_s);
    SVR_RANK_ALIGNED(out);
    SVR_RANK_APART(out, c_h);
    if (out != c_s) SVR_RANK_APART(out, c_s);                 // out == c_s: the saturation plane is matched in place
    SVR_RANK_APART(out, s_h);
    SVR_RANK_APART(out, s_s);
    SVR_RANK_OFF_WORKSPACE(c_h, need);
    SVR_RANK_OFF_WORKSPACE(c_s, need);
    SVR_RANK_OFF_WORKSPACE(s_h, need);
    SVR_RANK_OFF_WORKSPACE(s_s, need);
    SVR_RANK_OFF_WORKSPACE(out, need);
    const HuePlan p = hue_plan(n, workspace);
    const hipStream_t s = (hipStream_t)stream;
    hue_partition_launch(p.sort, true, c_s, c_h, true, p.tot_src, p.cls_k, p.cls_i, s);
    hue_partition_launch(p.sort, true, s_s, s_h, false, p.tot_ref, p.ref_k, nullptr, s);
    if (int rc = e.launched()) return rc;
    // the one read of the call: 2 x 256 class counts (source, reference), which decide the bins that are sorted and their runs
    uint32_t counts[2 * RANK_RADIX];
    if (int rc = e.hip(hipMemcpyAsync(counts, p.tot_src, sizeof(counts), hipMemcpyDeviceToHost, s), "class counts")) return rc;
    if (int rc = e.hip(hipStreamSynchronize(s), "class counts")) return rc;
    const uint32_t *n_src = counts, *n_ref = counts + RANK_RADIX;
    uint32_t at_src[HUE_CLASSES + 1] = {0}, at_ref[HUE_CLASSES + 1] = {0};
    for (int d = 0; d < HUE_CLASSES; ++d) { at_src[d + 1] = at_src[d] + n_src[d]; at_ref[d + 1] = at_ref[d] + n_ref[d]; }
    if (at_src[HUE_CLASSES] != (uint32_t)n || at_ref[HUE_CLASSES] != (uint32_t)n)
        return e.refuse("the class counts read back do not add up to n");
    if (out != c_s)
        if (int rc = e.hip(hipMemcpyAsync(out, c_s, (size_t)(4 * n), hipMemcpyDeviceToDevice, s), "out = c_s")) return rc;
    for (int bin = 0; bin < HUE_BINS; ++bin) {
        // digits of the bin's classes (svr_rank.hip, rank_hue_class): bin 0 = digits 0..2, bin 11 = digit 2, bin k = digit k + 2
        const int d0 = bin == 0 ? 0 : (bin == HUE_BINS - 1 ? 2 : bin + 2), d1 = bin == 0 ? 3 : d0 + 1;
        const uint32_t m_src = at_src[d1] - at_src[d0], m_ref = at_ref[d1] - at_ref[d0];
        if (m_src <= (uint32_t)HUE_MIN_PIXELS || m_ref <= (uint32_t)HUE_MIN_PIXELS) continue;
        const char *run_k = p.cls_k + 4 * (int64_t)at_src[d0], *run_i = p.cls_i + 4 * (int64_t)at_src[d0];
        if (bin == 0) {                            // its three classes in the order of the plane: the head of a partition of its own
            hue_partition_launch(p.sort, false, c_s, c_h, true, p.tot_bin0, p.bin0_k, p.bin0_i, s);
            run_k = p.bin0_k; run_i = p.bin0_i;
        }
        rank_sort_launch(hue_run_plan(p.sort, m_ref), p.ref_k + 4 * (int64_t)at_ref[d0], false, 1, p.sort.ref, nullptr, s, true);
        rank_sort_launch(hue_run_plan(p.sort, m_src), run_k, true, 2, nullptr, p.sort.idx[1], s, true, run_i);
        hipLaunchKernelGGL(hue_apply_kernel, dim3(blocks_for(m_src, 256)), dim3(256), 0, s, (const uint32_t*)p.sort.idx[1],
                           (const uint32_t*)p.sort.ref, m_src, m_ref, (uint32_t*)out);
    }
    return e.launched();
}
#undef SVR_RANK_OFF_WORKSPACE
#undef SVR_RANK_APART
#undef SVR_RANK_ALIGNED
#undef SVR_RANK_N_AND_WORKSPACE
#undef SVR_COLORFIX_GEOMETRY
#undef SVR_COLORFIX_STRIDES
#undef SVR_COLORFIX_PTR

// ---- packed input frames (svr_frame_unpack.hip)
int svr_unpack_frames(const void* packed, int64_t packed_bytes, int32_t fmt, int32_t T, int32_t H, int32_t W, int32_t C,
                      int32_t matrix, int32_t range, float* out, int64_t out_bytes, void* stream) {
    const Launch e{"svr_unpack_frames", stream};
    const bool yuv = fmt == SVR_UNPACK_YUV420P8 || fmt == SVR_UNPACK_YUV420P10;
    const bool wide = fmt == SVR_UNPACK_RGB16 || fmt == SVR_UNPACK_YUV420P10;          // 16-bit samples
    const char* why = nullptr;
    if (!packed) why = "packed is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if (T < 1 || H < 1 || W < 1) why = "need T >= 1, H >= 1, W >= 1";
    else if ((int64_t)H * W > ((int64_t)1 << 40) / T) why = "T * H * W must not exceed 2^40 pixels";
    else if (fmt != SVR_UNPACK_RGB8 && fmt != SVR_UNPACK_BGR8 && fmt != SVR_UNPACK_RGB16 && !yuv)
        why = "fmt must be SVR_UNPACK_RGB8, SVR_UNPACK_BGR8, SVR_UNPACK_RGB16, SVR_UNPACK_YUV420P8 or SVR_UNPACK_YUV420P10";
    else if (yuv ? C != 3 : (C != 3 && C != 4)) why = yuv ? "C must be 3 for the yuv420p formats" : "C must be 3 or 4";
    else if (matrix != SVR_MATRIX_BT709 && matrix != SVR_MATRIX_BT601) why = "matrix must be SVR_MATRIX_BT709 or SVR_MATRIX_BT601";
    else if (range != SVR_RANGE_TV && range != SVR_RANGE_PC) why = "range must be SVR_RANGE_TV or SVR_RANGE_PC";
    else if (wide && (uintptr_t)packed % 2) why = "packed is not aligned to 2 bytes";
    else if ((uintptr_t)out % 4) why = "out is not aligned to 4 bytes";
    if (why) return e.refuse("%s", why);
    const int64_t px = (int64_t)T * H * W, h2 = ((int64_t)H + 1) / 2, w2 = ((int64_t)W + 1) / 2;
    const int64_t n = yuv ? (int64_t)T * ((int64_t)H * W + 2 * h2 * w2) : px * C;       // samples
    const int64_t need_in = n * (wide ? 2 : 1), need_out = px * C * 4;
    if (packed_bytes != need_in) return e.wrong_size("packed_bytes", packed_bytes, "the format needs", need_in);
    if (out_bytes != need_out) return e.wrong_size("out_bytes", out_bytes, "fp32 [T, H, W, C] needs", need_out);
    const bool aligned = (uintptr_t)packed % 16 == 0 && (uintptr_t)out % 16 == 0;
    const hipStream_t s = (hipStream_t)stream;
    if (yuv) {
        // Kr, Kb exact decimals, the four products rounded at 2^16: 2 (1 - Kr), 2 (1 - Kb) Kb / Kg, 2 (1 - Kr) Kr / Kg, 2 (1 - Kb)
        const YuvCoef k = matrix == SVR_MATRIX_BT709 ? YuvCoef{103206, 12276, 30679, 121609} : YuvCoef{91881, 22553, 46802, 116130};
        const bool vec = aligned && W % 16 == 0;
        const unsigned grid = capped_grid(vec ? (int64_t)T * h2 * (W / 16) : px);
        with_const<10, 8>(fmt == SVR_UNPACK_YUV420P8 ? 8 : 10, [&](auto BITS) { with_const<SVR_RANGE_PC, SVR_RANGE_TV>(range, [&](auto PC) {
            if (vec) hipLaunchKernelGGL((unpack_yuv_vec_kernel<BITS(), PC()>), dim3(grid), dim3(256), 0, s, packed, out, T, H, W, k);
            else hipLaunchKernelGGL((unpack_yuv_kernel<BITS(), PC()>), dim3(grid), dim3(256), 0, s, packed, out, T, H, W, k);
        }); });
        return e.launched();
    }
    const int swap = fmt == SVR_UNPACK_BGR8 ? C : 0;               // unpack_rgb_kernel's C: 0 = samples in place
    const int unit = wide ? 8 : swap == 3 ? 48 : 16;
    const int64_t n_units = aligned ? n / unit : 0;
    const unsigned grid = capped_grid(std::max<int64_t>(n_units, n - n_units * unit));
    if (wide) hipLaunchKernelGGL((unpack_rgb_kernel<2, 0>), dim3(grid), dim3(256), 0, s, packed, out, n_units, n);
    else with_const<4, 3, 0>(swap, [&](auto CH) {
        hipLaunchKernelGGL((unpack_rgb_kernel<1, CH()>), dim3(grid), dim3(256), 0, s, packed, out, n_units, n);
    });
    return e.launched();
}

// ---- planar YUV sources turned into rgb16 codes (svr_planar.hip)
int svr_planar_codes(const void* planes, int64_t planes_bytes, int32_t sub, int32_t bits, int32_t T, int32_t H, int32_t W,
                     int32_t matrix, int32_t range, int32_t siting, void* out, int64_t out_bytes, void* stream) {
    const Launch e{"svr_planar_codes", stream};
    const bool wide = bits != 8;                                                       // 16-bit samples
    const char* why = nullptr;
    if (!planes) why = "planes is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if (T < 1 || H < 1 || W < 1) why = "need T >= 1, H >= 1, W >= 1";
    else if ((int64_t)H * W > ((int64_t)1 << 40) / T) why = "T * H * W must not exceed 2^40 pixels";
    else if (sub != SVR_PLANAR_420 && sub != SVR_PLANAR_422 && sub != SVR_PLANAR_444)
        why = "sub must be SVR_PLANAR_420, SVR_PLANAR_422 or SVR_PLANAR_444";
    else if (bits != 8 && bits != 10 && bits != 12) why = "bits must be 8, 10 or 12";
    else if (matrix != SVR_COLOUR_MATRIX_BT709 && matrix != SVR_COLOUR_MATRIX_BT601 && matrix != SVR_COLOUR_MATRIX_BT2020)
        why = "matrix must be SVR_COLOUR_MATRIX_BT709, SVR_COLOUR_MATRIX_BT601 or SVR_COLOUR_MATRIX_BT2020";
    else if (range != SVR_COLOUR_RANGE_TV && range != SVR_COLOUR_RANGE_PC) why = "range must be SVR_COLOUR_RANGE_TV or SVR_COLOUR_RANGE_PC";
    else if (siting != SVR_PLANAR_SITING_LEFT && siting != SVR_PLANAR_SITING_TOPLEFT)
        why = "siting must be SVR_PLANAR_SITING_LEFT or SVR_PLANAR_SITING_TOPLEFT";
    else if (siting == SVR_PLANAR_SITING_TOPLEFT && sub != SVR_PLANAR_420)
        why = "siting SVR_PLANAR_SITING_TOPLEFT is for SVR_PLANAR_420 only";
    else if (wide && (uintptr_t)planes % 2) why = "planes is not aligned to 2 bytes";
    else if ((uintptr_t)out % 2) why = "out is not aligned to 2 bytes";
    if (why) return e.refuse("%s", why);
    const int64_t px = (int64_t)T * H * W;
    const int64_t hc = sub == SVR_PLANAR_420 ? ((int64_t)H + 1) / 2 : H, wc = sub == SVR_PLANAR_444 ? W : ((int64_t)W + 1) / 2;
    const int64_t need_in = (int64_t)T * ((int64_t)H * W + 2 * hc * wc) * (wide ? 2 : 1), need_out = px * 6;
    if (planes_bytes != need_in) return e.wrong_size("planes_bytes", planes_bytes, "the format needs", need_in);
    if (out_bytes != need_out) return e.wrong_size("out_bytes", out_bytes, "uint16 [T, H, W, 3] needs", need_out);
    if (rank_overlap(out, need_out, planes, need_in)) return e.refuse("out overlaps planes");
    // Kr, Kb exact decimals, the four products rounded at 2^16 (planar.MATRICES)
    const YuvCoef k = matrix == SVR_COLOUR_MATRIX_BT709 ? YuvCoef{103206, 12276, 30679, 121609}
                    : matrix == SVR_COLOUR_MATRIX_BT601 ? YuvCoef{91881, 22553, 46802, 116130} : YuvCoef{96639, 10784, 37444, 123299};
    const bool vec = (uintptr_t)planes % 16 == 0 && (uintptr_t)out % 16 == 0 && W % 16 == 0;
    const unsigned grid = capped_grid(vec ? (int64_t)T * hc * (W / 16) : px);
    const hipStream_t s = (hipStream_t)stream;
    with_const<SVR_PLANAR_444, SVR_PLANAR_422, SVR_PLANAR_420>(sub, [&](auto SUB) { with_const<12, 10, 8>(bits, [&](auto BITS) {
        with_const<SVR_COLOUR_RANGE_PC, SVR_COLOUR_RANGE_TV>(range, [&](auto PC) { with_const<1, 0>(siting == SVR_PLANAR_SITING_TOPLEFT, [&](auto TOPLEFT) {
            if constexpr (TOPLEFT() && SUB() != SVR_PLANAR_420) return;                // (refused above)
            else if (vec) hipLaunchKernelGGL((planar_vec_kernel<SUB(), BITS(), PC(), TOPLEFT()>), dim3(grid), dim3(256), 0, s, planes,
                                             (unsigned short*)out, T, H, W, k);
            else hipLaunchKernelGGL((planar_kernel<SUB(), BITS(), PC(), TOPLEFT()>), dim3(grid), dim3(256), 0, s, planes,
                                    (unsigned short*)out, T, H, W, k);
        }); });
    }); });
    return e.launched();
}

// ---- interlaced sources made progressive on the packed planes (svr_deinterlace.hip): one launch per plane
int svr_deinterlace(const void* packed, int64_t packed_bytes, const void* before, const void* after, int32_t fmt, int32_t T, int32_t H,
                    int32_t W, int32_t C, int32_t order, int32_t rate, void* out, int64_t out_bytes, void* stream) {
    const Launch e{"svr_deinterlace", stream};
    const bool yuv = fmt == SVR_UNPACK_YUV420P8 || fmt == SVR_UNPACK_YUV420P10;
    const bool wide = fmt == SVR_UNPACK_RGB16 || fmt == SVR_UNPACK_YUV420P10;          // 16-bit samples
    const char* why = nullptr;
    if (!packed) why = "packed is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if (T < 1 || H < 1 || W < 1) why = "need T >= 1, H >= 1, W >= 1";
    else if ((int64_t)H * W > ((int64_t)1 << 40) / T) why = "T * H * W must not exceed 2^40 pixels";
    else if (fmt != SVR_UNPACK_RGB8 && fmt != SVR_UNPACK_BGR8 && fmt != SVR_UNPACK_RGB16 && !yuv)
        why = "fmt must be SVR_UNPACK_RGB8, SVR_UNPACK_BGR8, SVR_UNPACK_RGB16, SVR_UNPACK_YUV420P8 or SVR_UNPACK_YUV420P10";
    else if (yuv ? C != 3 : (C != 3 && C != 4)) why = yuv ? "C must be 3 for the yuv420p formats" : "C must be 3 or 4";
    else if (order != SVR_FIELD_TFF && order != SVR_FIELD_BFF) why = "order must be SVR_FIELD_TFF or SVR_FIELD_BFF";
    else if (rate != SVR_DEINT_FRAME && rate != SVR_DEINT_FIELD) why = "rate must be SVR_DEINT_FRAME or SVR_DEINT_FIELD";
    else if (wide && (uintptr_t)packed % 2) why = "packed is not aligned to 2 bytes";
    else if (wide && (uintptr_t)before % 2) why = "before is not aligned to 2 bytes";
    else if (wide && (uintptr_t)after % 2) why = "after is not aligned to 2 bytes";
    else if (wide && (uintptr_t)out % 2) why = "out is not aligned to 2 bytes";
    if (why) return e.refuse("%s", why);
    const int size = wide ? 2 : 1;
    const int64_t h2 = ((int64_t)H + 1) / 2, w2 = ((int64_t)W + 1) / 2;
    const int64_t frame = yuv ? (int64_t)H * W + 2 * h2 * w2 : (int64_t)H * W * C;      // samples
    const int64_t need_in = (int64_t)T * frame * size, need_out = need_in * (rate == SVR_DEINT_FIELD ? 2 : 1);
    if (packed_bytes != need_in) return e.wrong_size("packed_bytes", packed_bytes, "the format needs", need_in);
    if (out_bytes != need_out) return e.wrong_size("out_bytes", out_bytes, "the format and rate need", need_out);
    if (rank_overlap(out, need_out, packed, need_in)) return e.refuse("out overlaps packed");
    if (before && rank_overlap(out, need_out, before, frame * size)) return e.refuse("out overlaps before");
    if (after && rank_overlap(out, need_out, after, frame * size)) return e.refuse("out overlaps after");
    const bool aligned = (uintptr_t)packed % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)before % 16 == 0 &&
                         (uintptr_t)after % 16 == 0 && frame * size % 16 == 0;
    // the planes of a frame: offset, rows, samples per row, column step (deinterlace.planes)
    struct Plane { int64_t off; int R, N, s; };
    const Plane planes[3] = {{0, H, yuv ? W : W * C, yuv ? 1 : C}, {(int64_t)H * W, (int)h2, (int)w2, 1}, {(int64_t)H * W + h2 * w2, (int)h2, (int)w2, 1}};
    const hipStream_t s = (hipStream_t)stream;
    const int64_t n_out = (int64_t)T * (rate == SVR_DEINT_FIELD ? 2 : 1);
    for (int pl = 0; pl < (yuv ? 3 : 1); ++pl) {
        const Plane& p = planes[pl];
        const bool vec = aligned && p.off * size % 16 == 0 && (int64_t)p.N * size % 16 == 0;       // every row starts on 16 bytes
        const unsigned grid = capped_grid(n_out * p.R * (vec ? p.N / (16 / size) : p.N));
        with_const<2, 1>(size, [&](auto BYTES) { with_const<SVR_DEINT_FIELD, SVR_DEINT_FRAME>(rate, [&](auto FIELD) {
            typedef typename std::conditional<BYTES() == 2, unsigned short, unsigned char>::type S;
            const DeintClip<S> clip{(const S*)packed, (const S*)before, (const S*)after, T, frame};
            if (vec) with_const<4, 3, 1>(p.s, [&](auto STEP) {
                hipLaunchKernelGGL((deint_vec_kernel<S, STEP(), FIELD()>), dim3(grid), dim3(256), 0, s, clip, (S*)out, p.off, p.R, p.N, order);
            });
            else hipLaunchKernelGGL((deint_elem_kernel<S, FIELD()>), dim3(grid), dim3(256), 0, s, clip, (S*)out, p.off, p.R, p.N, p.s, order);
        }); });
        if (int rc = e.launched()) return rc;
    }
    return 0;
}

// ---- field matching on the packed planes (svr_fieldmatch.hip).  What its two entry points share with svr_deinterlace: the formats,
// the frame's size and planes, the refusals of the clip's own arguments
struct FieldClip {
    bool yuv, wide;
    int size;                                           // bytes per sample
    int64_t h2, w2, frame;                              // chroma rows and columns; samples per frame
    struct Plane { int64_t off; int R; int64_t N; int s; } planes[3];
    int n_planes;
};
// (in two steps, so that an entry point with an argument of its own between them -- field matching's order -- keeps its place in the
// order of the refusals, and one without it -- decimation -- takes the two as they are)
static const char* clip_shape_error(int32_t fmt, int32_t T, int32_t H, int32_t W, int32_t C) {
    const bool yuv = fmt == SVR_UNPACK_YUV420P8 || fmt == SVR_UNPACK_YUV420P10;
    if (T < 1 || H < 1 || W < 1) return "need T >= 1, H >= 1, W >= 1";
    if ((int64_t)H * W > ((int64_t)1 << 40) / T) return "T * H * W must not exceed 2^40 pixels";
    if (fmt != SVR_UNPACK_RGB8 && fmt != SVR_UNPACK_BGR8 && fmt != SVR_UNPACK_RGB16 && !yuv)
        return "fmt must be SVR_UNPACK_RGB8, SVR_UNPACK_BGR8, SVR_UNPACK_RGB16, SVR_UNPACK_YUV420P8 or SVR_UNPACK_YUV420P10";
    if (yuv ? C != 3 : (C != 3 && C != 4)) return yuv ? "C must be 3 for the yuv420p formats" : "C must be 3 or 4";
    return nullptr;
}
static const char* clip_alignment_error(const void* packed, const void* before, const void* after, int32_t fmt) {
    const bool wide = fmt == SVR_UNPACK_RGB16 || fmt == SVR_UNPACK_YUV420P10;
    if (wide && (uintptr_t)packed % 2) return "packed is not aligned to 2 bytes";
    if (wide && (uintptr_t)before % 2) return "before is not aligned to 2 bytes";
    if (wide && (uintptr_t)after % 2) return "after is not aligned to 2 bytes";
    return nullptr;
}
static const char* field_clip_error(const void* packed, const void* before, const void* after, int32_t fmt, int32_t T, int32_t H,
                                    int32_t W, int32_t C, int32_t order) {
    if (const char* why = clip_shape_error(fmt, T, H, W, C)) return why;
    if (order != SVR_FIELD_TFF && order != SVR_FIELD_BFF) return "order must be SVR_FIELD_TFF or SVR_FIELD_BFF";
    return clip_alignment_error(packed, before, after, fmt);
}
static FieldClip field_clip(int32_t fmt, int32_t H, int32_t W, int32_t C) {
    FieldClip c;
    c.yuv = fmt == SVR_UNPACK_YUV420P8 || fmt == SVR_UNPACK_YUV420P10;
    c.wide = fmt == SVR_UNPACK_RGB16 || fmt == SVR_UNPACK_YUV420P10;
    c.size = c.wide ? 2 : 1;
    c.h2 = ((int64_t)H + 1) / 2, c.w2 = ((int64_t)W + 1) / 2;
    c.frame = c.yuv ? (int64_t)H * W + 2 * c.h2 * c.w2 : (int64_t)H * W * C;
    c.planes[0] = {0, H, c.yuv ? (int64_t)W : (int64_t)W * C, c.yuv ? 1 : C};
    c.planes[1] = {(int64_t)H * W, (int)c.h2, c.w2, 1};
    c.planes[2] = {(int64_t)H * W + c.h2 * c.w2, (int)c.h2, c.w2, 1};
    c.n_planes = c.yuv ? 3 : 1;
    return c;
}

int svr_comb_counts(const void* packed, int64_t packed_bytes, const void* before, const void* after, int32_t fmt, int32_t T, int32_t H,
                    int32_t W, int32_t C, int32_t order, int32_t thr, void* cnt, int64_t cnt_bytes, void* stream) {
    const Launch e{"svr_comb_counts", stream};
    const char* why = nullptr;
    if (!packed) why = "packed is a null pointer";
    else if (!cnt) why = "cnt is a null pointer";
    else if ((why = field_clip_error(packed, before, after, fmt, T, H, W, C, order))) {}
    else if ((int64_t)H * W * C > ((int64_t)1 << 31)) why = "H * W * C must not exceed 2^31 samples (the counters are int32)";
    else if (thr < 0 || thr > 255) why = "thr must lie in 0..255";
    else if ((uintptr_t)cnt % 4) why = "cnt is not aligned to 4 bytes";
    if (why) return e.refuse("%s", why);
    const FieldClip c = field_clip(fmt, H, W, C);
    const int64_t need_in = (int64_t)T * c.frame * c.size, need_cnt = (int64_t)T * 24;
    if (packed_bytes != need_in) return e.wrong_size("packed_bytes", packed_bytes, "the format needs", need_in);
    if (cnt_bytes != need_cnt) return e.wrong_size("cnt_bytes", cnt_bytes, "int32 [T, 3, 2] needs", need_cnt);
    if (rank_overlap(cnt, need_cnt, packed, need_in)) return e.refuse("cnt overlaps packed");
    if (before && rank_overlap(cnt, need_cnt, before, c.frame * c.size)) return e.refuse("cnt overlaps before");
    if (after && rank_overlap(cnt, need_cnt, after, c.frame * c.size)) return e.refuse("cnt overlaps after");
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = e.hip(hipMemsetAsync(cnt, 0, (size_t)need_cnt, s), "zeroing cnt")) return rc;
    const FieldClip::Plane& p = c.planes[0];
    if (p.R < 3) return 0;                                                   // no tested row: the counts are zero
    const bool vec = (uintptr_t)packed % 16 == 0 && (uintptr_t)before % 16 == 0 && (uintptr_t)after % 16 == 0 &&
                     c.frame * c.size % 16 == 0 && p.N * c.size % 16 == 0;
    const int unit = vec ? 16 / c.size : 1;                                  // samples per lane column
    const int per = FM_BLOCK * p.s / unit, cb = FM_LANES / per;              // lanes per block column, block columns per workgroup
    const int64_t block_cols = (p.N / p.s + FM_BLOCK - 1) / FM_BLOCK;
    const int chunks = (int)((block_cols + cb - 1) / cb);
    const int thr_code = thr << (fmt == SVR_UNPACK_RGB16 ? 8 : fmt == SVR_UNPACK_YUV420P10 ? 2 : 0);
    const unsigned grid = capped_grid((int64_t)T * ((p.R + FM_BLOCK - 1) / FM_BLOCK) * chunks * 256);
    with_const<2, 1>(c.size, [&](auto BYTES) { with_const<1, 0>(vec ? 1 : 0, [&](auto VEC) {
        typedef typename std::conditional<BYTES() == 2, unsigned short, unsigned char>::type S;
        const DeintClip<S> clip{(const S*)packed, (const S*)before, (const S*)after, T, c.frame};
        hipLaunchKernelGGL((comb_kernel<S, VEC()>), dim3(grid), dim3(FM_LANES), 0, s, clip, p.R, p.N, per, cb, chunks, p.N / unit, order,
                           thr_code, (int*)cnt);
    }); });
    return e.launched();
}

int svr_field_select(const void* packed, int64_t packed_bytes, const void* before, const void* after, const void* deint,
                     int64_t deint_bytes, const void* cnt, int64_t cnt_bytes, int32_t fmt, int32_t T, int32_t H, int32_t W, int32_t C,
                     int32_t order, int32_t mi, void* out, int64_t out_bytes, void* modes, void* stats, void* stream) {
    const Launch e{"svr_field_select", stream};
    const bool wide = fmt == SVR_UNPACK_RGB16 || fmt == SVR_UNPACK_YUV420P10;
    const char* why = nullptr;
    if (!packed) why = "packed is a null pointer";
    else if (!deint) why = "deint is a null pointer";
    else if (!cnt) why = "cnt is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if ((why = field_clip_error(packed, before, after, fmt, T, H, W, C, order))) {}
    else if (mi < 0) why = "mi must not be negative";
    else if (wide && (uintptr_t)deint % 2) why = "deint is not aligned to 2 bytes";
    else if (wide && (uintptr_t)out % 2) why = "out is not aligned to 2 bytes";
    else if ((uintptr_t)cnt % 4) why = "cnt is not aligned to 4 bytes";
    else if ((uintptr_t)modes % 4) why = "modes is not aligned to 4 bytes";
    else if ((uintptr_t)stats % 8) why = "stats is not aligned to 8 bytes";
    if (why) return e.refuse("%s", why);
    const FieldClip c = field_clip(fmt, H, W, C);
    const int64_t need = (int64_t)T * c.frame * c.size, need_cnt = (int64_t)T * 24, one = c.frame * c.size;
    if (packed_bytes != need) return e.wrong_size("packed_bytes", packed_bytes, "the format needs", need);
    if (deint_bytes != need) return e.wrong_size("deint_bytes", deint_bytes, "the format needs", need);
    if (cnt_bytes != need_cnt) return e.wrong_size("cnt_bytes", cnt_bytes, "int32 [T, 3, 2] needs", need_cnt);
    if (out_bytes != need) return e.wrong_size("out_bytes", out_bytes, "the format needs", need);
    // no output may overlap an input, or another output
    struct Span { const char* name; const void* at; int64_t bytes; };
    const Span inputs[] = {{"packed", packed, need}, {"before", before, one}, {"after", after, one}, {"deint", deint, need}, {"cnt", cnt, need_cnt}};
    const Span outputs[] = {{"out", out, need}, {"modes", modes, (int64_t)T * 4}, {"stats", stats, 48}};
    for (int o = 0; o < 3; ++o) {
        if (!outputs[o].at) continue;
        for (const Span& in : inputs)
            if (in.at && rank_overlap(outputs[o].at, outputs[o].bytes, in.at, in.bytes)) return e.refuse("%s overlaps %s", outputs[o].name, in.name);
        for (int q = 0; q < o; ++q)
            if (outputs[q].at && rank_overlap(outputs[o].at, outputs[o].bytes, outputs[q].at, outputs[q].bytes))
                return e.refuse("%s overlaps %s", outputs[o].name, outputs[q].name);
    }
    const bool aligned = (uintptr_t)packed % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)before % 16 == 0 &&
                         (uintptr_t)after % 16 == 0 && (uintptr_t)deint % 16 == 0 && one % 16 == 0;
    const int64_t bound = (int64_t)mi * c.planes[0].s;
    const hipStream_t s = (hipStream_t)stream;
    for (int pl = 0; pl < c.n_planes; ++pl) {
        const FieldClip::Plane& p = c.planes[pl];
        const bool vec = aligned && p.off * c.size % 16 == 0 && p.N * c.size % 16 == 0;            // every row starts on 16 bytes
        const int64_t cols = vec ? p.N / (16 / c.size) : p.N;
        const unsigned grid = capped_grid((int64_t)T * p.R * cols);
        with_const<2, 1>(c.size, [&](auto BYTES) { with_const<1, 0>(vec ? 1 : 0, [&](auto VEC) {
            typedef typename std::conditional<BYTES() == 2, unsigned short, unsigned char>::type S;
            const DeintClip<S> clip{(const S*)packed, (const S*)before, (const S*)after, T, c.frame};
            hipLaunchKernelGGL((select_kernel<S, VEC()>), dim3(grid), dim3(FM_LANES), 0, s, clip, (const S*)deint, (const int*)cnt, bound,
                               (S*)out, p.off, p.R, p.N, cols, order, pl == 0 ? 1 : 0, pl == 0 ? (int*)modes : nullptr,
                               pl == 0 ? (unsigned long long*)stats : nullptr);
        }); });
        if (int rc = e.launched()) return rc;
    }
    return 0;
}

// ---- decimation on the packed planes (svr_decimate.hip), after field matching: the clip's own arguments are refused in field
// matching's words (a clip here has no order and no ``after``)
int svr_frame_diffs(const void* packed, int64_t packed_bytes, const void* before, int32_t fmt, int32_t T, int32_t H, int32_t W, int32_t C,
                    void* diff, int64_t diff_bytes, void* stream) {
    const Launch e{"svr_frame_diffs", stream};
    const char* why = nullptr;
    if (!packed) why = "packed is a null pointer";
    else if (!diff) why = "diff is a null pointer";
    else if ((why = clip_shape_error(fmt, T, H, W, C))) {}
    else if ((why = clip_alignment_error(packed, before, nullptr, fmt))) {}
    else if ((uintptr_t)diff % 4) why = "diff is not aligned to 4 bytes";
    if (why) return e.refuse("%s", why);
    const FieldClip c = field_clip(fmt, H, W, C);
    const int64_t need_in = (int64_t)T * c.frame * c.size, need_diff = (int64_t)T * 4;
    if (packed_bytes != need_in) return e.wrong_size("packed_bytes", packed_bytes, "the format needs", need_in);
    if (diff_bytes != need_diff) return e.wrong_size("diff_bytes", diff_bytes, "int32 [T] needs", need_diff);
    if (rank_overlap(diff, need_diff, packed, need_in)) return e.refuse("diff overlaps packed");
    if (before && rank_overlap(diff, need_diff, before, c.frame * c.size)) return e.refuse("diff overlaps before");
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = e.hip(hipMemsetAsync(diff, 0, (size_t)need_diff, s), "zeroing diff")) return rc;
    const FieldClip::Plane& p = c.planes[0];
    const bool vec = (uintptr_t)packed % 16 == 0 && (uintptr_t)before % 16 == 0 && c.frame * c.size % 16 == 0 && p.N * c.size % 16 == 0;
    const int unit = vec ? 16 / c.size : 1;                                  // samples per lane column
    const int per = DEC_BLOCK * p.s / unit, cb = DEC_LANES / per;            // lanes per block column, block columns per workgroup
    const int64_t block_cols = (p.N / p.s + DEC_BLOCK - 1) / DEC_BLOCK;
    const int chunks = (int)((block_cols + cb - 1) / cb);
    const unsigned grid = capped_grid((int64_t)T * ((p.R + DEC_BLOCK - 1) / DEC_BLOCK) * chunks * 256);
    with_const<2, 1>(c.size, [&](auto BYTES) { with_const<1, 0>(vec ? 1 : 0, [&](auto VEC) {
        typedef typename std::conditional<BYTES() == 2, unsigned short, unsigned char>::type S;
        hipLaunchKernelGGL((diff_kernel<S, VEC()>), dim3(grid), dim3(DEC_LANES), 0, s, (const S*)packed, (const S*)before, T, c.frame, p.R,
                           p.N, per, cb, chunks, p.N / unit, (int*)diff);
    }); });
    return e.launched();
}

int svr_decimate_select(const void* packed, int64_t packed_bytes, const void* diff, int64_t diff_bytes, int32_t fmt, int32_t T, int32_t H,
                        int32_t W, int32_t C, int32_t dup, void* out, int64_t out_bytes, void* drops, void* stats, void* stream) {
    const Launch e{"svr_decimate_select", stream};
    const bool wide = fmt == SVR_UNPACK_RGB16 || fmt == SVR_UNPACK_YUV420P10;
    const char* why = nullptr;
    if (!packed) why = "packed is a null pointer";
    else if (!diff) why = "diff is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if ((why = clip_shape_error(fmt, T, H, W, C))) {}
    else if ((why = clip_alignment_error(packed, nullptr, nullptr, fmt))) {}
    else if (dup < 0 || dup > (1 << 18)) why = "dup must lie in 0..262144";
    else if (wide && (uintptr_t)out % 2) why = "out is not aligned to 2 bytes";
    else if ((uintptr_t)diff % 4) why = "diff is not aligned to 4 bytes";
    else if ((uintptr_t)drops % 4) why = "drops is not aligned to 4 bytes";
    else if ((uintptr_t)stats % 8) why = "stats is not aligned to 8 bytes";
    if (why) return e.refuse("%s", why);
    const FieldClip c = field_clip(fmt, H, W, C);
    const int cycles = T / DEC_CYCLE;
    const int64_t one = c.frame * c.size, need = (int64_t)T * one, need_diff = (int64_t)T * 4, need_out = (int64_t)(T - cycles) * one;
    if (packed_bytes != need) return e.wrong_size("packed_bytes", packed_bytes, "the format needs", need);
    if (diff_bytes != need_diff) return e.wrong_size("diff_bytes", diff_bytes, "int32 [T] needs", need_diff);
    if (out_bytes != need_out) return e.wrong_size("out_bytes", out_bytes, "the T - T / 5 frames need", need_out);
    // no output may overlap an input, or another output (a clip without a whole cycle has no drops)
    struct Span { const char* name; const void* at; int64_t bytes; };
    const Span inputs[] = {{"packed", packed, need}, {"diff", diff, need_diff}};
    const Span outputs[] = {{"out", out, need_out}, {"drops", cycles ? drops : nullptr, (int64_t)cycles * 4}, {"stats", stats, 48}};
    for (int o = 0; o < 3; ++o) {
        if (!outputs[o].at) continue;
        for (const Span& in : inputs)
            if (rank_overlap(outputs[o].at, outputs[o].bytes, in.at, in.bytes)) return e.refuse("%s overlaps %s", outputs[o].name, in.name);
        for (int q = 0; q < o; ++q)
            if (outputs[q].at && rank_overlap(outputs[o].at, outputs[o].bytes, outputs[q].at, outputs[q].bytes))
                return e.refuse("%s overlaps %s", outputs[o].name, outputs[q].name);
    }
    const bool vec = (uintptr_t)packed % 16 == 0 && (uintptr_t)out % 16 == 0 && one % 16 == 0;
    const int64_t units = vec ? one / 16 : c.frame;
    const int64_t bound = ((int64_t)dup * c.planes[0].s) << (fmt == SVR_UNPACK_RGB16 ? 8 : fmt == SVR_UNPACK_YUV420P10 ? 2 : 0);
    const unsigned grid = capped_grid((int64_t)(T - cycles) * units);
    with_const<2, 1>(c.size, [&](auto BYTES) { with_const<1, 0>(vec ? 1 : 0, [&](auto VEC) {
        typedef typename std::conditional<BYTES() == 2, unsigned short, unsigned char>::type S;
        hipLaunchKernelGGL((decimate_select_kernel<S, VEC()>), dim3(grid), dim3(DEC_LANES), 0, (hipStream_t)stream, (const S*)packed,
                           (const int*)diff, T, c.frame, units, bound, (S*)out, cycles ? (int*)drops : nullptr,
                           (unsigned long long*)stats);
    }); });
    return e.launched();
}

// ---- GGUF blocks expanded at load (svr_gguf.hip)
int svr_dequant_gguf(const void* blocks, int32_t ggml_type, int64_t n_blocks, void* out, int32_t out_kind, int64_t out_bytes,
                     void* stream) {
    const Launch e{"svr_dequant_gguf", stream};
    const bool known = ggml_type == SVR_GGML_Q8_0 || ggml_type == SVR_GGML_Q4_K || ggml_type == SVR_GGML_Q5_K || ggml_type == SVR_GGML_Q6_K;
    const int64_t per = ggml_type == SVR_GGML_Q8_0 ? 32 : 256;            // elements per block
    const char* why = nullptr;
    if (!blocks) why = "blocks is a null pointer";
    else if (!out) why = "out is a null pointer";
    else if (!known) why = "ggml_type must be SVR_GGML_Q8_0, SVR_GGML_Q4_K, SVR_GGML_Q5_K or SVR_GGML_Q6_K";
    else if (out_kind != SVR_STORE_BF16 && out_kind != SVR_STORE_FP32) why = "out_kind must be SVR_STORE_BF16 or SVR_STORE_FP32";
    else if (n_blocks < 1) why = "need n_blocks >= 1";
    else if (n_blocks > ((int64_t)1 << 40) / per) why = "n_blocks times the block size must not exceed 2^40 elements";
    else if ((uintptr_t)blocks % 32) why = "blocks is not aligned to 32 bytes";
    else if ((uintptr_t)out % 16) why = "out is not aligned to 16 bytes";
    if (why) return e.refuse("%s", why);
    const int64_t need = n_blocks * per * (out_kind == SVR_STORE_FP32 ? 4 : 2);
    if (out_bytes != need) return e.wrong_size("out_bytes", out_bytes, "the type and block count need", need);
    const int64_t n_units = n_blocks * (per / 8);                          // eight outputs per lane
    const unsigned grid = capped_grid(n_units);
    const unsigned char* b = (const unsigned char*)blocks;
    const hipStream_t s = (hipStream_t)stream;
    with_const<SVR_GGML_Q6_K, SVR_GGML_Q5_K, SVR_GGML_Q4_K, SVR_GGML_Q8_0>(ggml_type, [&](auto TYPE) { with_kind(out_kind, [&](auto K) {
        hipLaunchKernelGGL((dequant_gguf_kernel<TYPE(), K()>), dim3(grid), dim3(256), 0, s, b, out, n_units);
    }); });
    return e.launched();
}

}  // extern "C"
