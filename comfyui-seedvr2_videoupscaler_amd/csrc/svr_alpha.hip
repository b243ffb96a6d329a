// Edge-guided alpha upscaling (alpha.py is the specification; reference: src/core/alpha_upscaling.py:125-438).
// Three HBM-bound passes on one stream, no host round trip: every data-dependent decision (binary matte or not, how often the
// RGB is normalised, the per-frame edge maximum) is written to device memory by one kernel and read by the next.
//   alpha_stats_kernel   counts of the input alpha below 0.1 / above 0.9, min(rgb) < 0, min(rgb) < -1      -> flags
//   alpha_edges_kernel   8-bit gray, 3x3 Sobel (BORDER_REFLECT_101), n = sx^2 + sy^2 as int32, per-frame max -> n map, maxima
//   alpha_refine_kernel  guided filter (r = 2 binary / 3 soft) over LDS tiles + the binary tail             -> alpha
// Integer atomics only, so the result is the same bits on every run.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

constexpr int ALPHA_TILE = 32;                      // output tile edge of the edge and refine kernels
constexpr int ALPHA_RMAX = 3;                       // largest guided-filter radius
constexpr int ALPHA_FLAGS = 4;                      // int32 {count(a < 0.1), count(a > 0.9), min(rgb) < 0, min(rgb) < -1}

template <int KIND>                                  // SVR_STORE_FP32 / SVR_STORE_BF16 (widened on load)
SVR_DEVICE float alpha_load(const void* p, int64_t i) {
    if constexpr (KIND == SVR_STORE_FP32) return ((const float*)p)[i];
    else return bf2f(((const bf16_t*)p)[i]);
}

template <int KIND>
__global__ __launch_bounds__(256) void alpha_stats_kernel(const float* __restrict__ alpha_lo, int64_t n_alpha,
                                                          const void* __restrict__ rgb, int64_t n_px, int64_t ld_px,
                                                          int* __restrict__ flags) {
    __shared__ int part[ALPHA_FLAGS];
    if (threadIdx.x < ALPHA_FLAGS) part[threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    int lt = 0, gt = 0, neg0 = 0, neg1 = 0;
    for (int64_t i = first; i < n_alpha; i += step) {
        const float a = alpha_lo[i];
        lt += a < 0.1f;
        gt += a > 0.9f;
    }
    for (int64_t i = first; i < n_px; i += step) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = alpha_load<KIND>(rgb, i * ld_px + c);
            neg0 |= v < 0.f;
            neg1 |= v < -1.f;
        }
    }
    if (lt) atomicAdd(&part[0], lt);
    if (gt) atomicAdd(&part[1], gt);
    if (neg0) atomicOr(&part[2], 1);
    if (neg1) atomicOr(&part[3], 1);
    __syncthreads();
    if (threadIdx.x < 2) { if (part[threadIdx.x]) atomicAdd(&flags[threadIdx.x], part[threadIdx.x]); }
    else if (threadIdx.x < ALPHA_FLAGS) { if (part[threadIdx.x]) atomicOr(&flags[threadIdx.x], 1); }
}

// OpenCV's 8-bit RGB2GRAY of the pixel as detect_edges_batch sees it: normalised once more than the guide when min(rgb) < -1.
template <int KIND>
SVR_DEVICE int alpha_gray(const void* rgb, int64_t px, int64_t ld_px, bool neg0, bool neg1) {
    int u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = alpha_load<KIND>(rgb, px * ld_px + c);
        if (neg0) v = (v + 1.f) / 2.f;
        if (neg1) v = (v + 1.f) / 2.f;
        u[c] = (int)fminf(fmaxf(v * 255.f, 0.f), 255.f);
    }
    return (4899 * u[0] + 9617 * u[1] + 1868 * u[2] + 8192) >> 14;
}

template <int KIND>
__global__ __launch_bounds__(256) void alpha_edges_kernel(const void* __restrict__ rgb, int64_t ld_px, int H, int W,
                                                          const int* __restrict__ flags, int* __restrict__ nmap,
                                                          int* __restrict__ maxima) {
    constexpr int SW = ALPHA_TILE + 2;
    __shared__ int gray[SW * SW];
    __shared__ int tile_max;
    const int x0 = blockIdx.x * ALPHA_TILE, y0 = blockIdx.y * ALPHA_TILE, t = blockIdx.z;
    const bool neg0 = flags[2] != 0, neg1 = flags[3] != 0;
    if (threadIdx.x == 0) tile_max = 0;
    for (int i = threadIdx.x; i < SW * SW; i += 256) {
        int gy = y0 - 1 + i / SW, gx = x0 - 1 + i % SW;
        // BORDER_REFLECT_101 (H, W >= 2); positions further out belong to no output pixel of this tile
        gy = gy < 0 ? -gy : gy; gx = gx < 0 ? -gx : gx;
        gy = gy >= H ? 2 * H - 2 - gy : gy; gx = gx >= W ? 2 * W - 2 - gx : gx;
        gray[i] = (gy >= 0 && gx >= 0) ? alpha_gray<KIND>(rgb, ((int64_t)t * H + gy) * W + gx, ld_px, neg0, neg1) : 0;
    }
    __syncthreads();
    int best = 0;
    for (int i = threadIdx.x; i < ALPHA_TILE * ALPHA_TILE; i += 256) {
        const int ly = i / ALPHA_TILE, lx = i % ALPHA_TILE;
        if (y0 + ly >= H || x0 + lx >= W) continue;
        const int* g = gray + ly * SW + lx;                       // top-left of the pixel's 3x3 window
        const int sx = (g[2] + 2 * g[SW + 2] + g[2 * SW + 2]) - (g[0] + 2 * g[SW] + g[2 * SW]);
        const int sy = (g[2 * SW] + 2 * g[2 * SW + 1] + g[2 * SW + 2]) - (g[0] + 2 * g[1] + g[2]);
        const int n = sx * sx + sy * sy;
        nmap[((int64_t)t * H + y0 + ly) * W + x0 + lx] = n;
        best = max(best, n);
    }
    if (best) atomicMax(&tile_max, best);
    __syncthreads();
    if (threadIdx.x == 0 && tile_max) atomicMax(&maxima[t], tile_max);
}

// (edge / edge.max() * 255).astype(uint8) with the reference's fp64 operation order; a constant frame (0 / 0 there) gives 0
SVR_DEVICE int alpha_edge_byte(int n, int nmax) {
    return nmax > 0 ? (int)(sqrt((double)n) / sqrt((double)nmax) * 255.0) : 0;
}

template <int KIND, int R>
SVR_DEVICE void alpha_refine_tile(double* __restrict__ I_s, float* __restrict__ P_s, double* __restrict__ A_s, double* __restrict__ B_s,
                                  const void* __restrict__ rgb, int64_t ld_px, const float* __restrict__ base, int H, int W,
                                  bool neg0, const int* __restrict__ nmap, int nmax, float* __restrict__ out,
                                  unsigned char* __restrict__ edge_out) {
    constexpr int SW = ALPHA_TILE + 4 * R, AW = ALPHA_TILE + 2 * R, K = 2 * R + 1;
    constexpr double k2 = (double)(K * K), eps = 0.002;
    const int x0 = blockIdx.x * ALPHA_TILE, y0 = blockIdx.y * ALPHA_TILE, t = blockIdx.z;
    const int64_t frame = (int64_t)t * H * W;
    // guide (mean of the once-normalised channels) and base over the tile + 2R, zero outside the image (avg_pool2d's padding)
    for (int i = threadIdx.x; i < SW * SW; i += 256) {
        const int gy = y0 - 2 * R + i / SW, gx = x0 - 2 * R + i % SW;
        double g = 0.0;
        float p = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int64_t px = frame + (int64_t)gy * W + gx;
            double c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c[k] = (double)alpha_load<KIND>(rgb, px * ld_px + k);
                if (neg0) c[k] = (c[k] + 1.0) / 2.0;
            }
            g = (c[0] + c[1] + c[2]) / 3.0;
            p = base[px];
        }
        I_s[i] = g; P_s[i] = p;
    }
    __syncthreads();
    // a, b over the tile + R; zero outside the image (the second pooling pads them with zeros).  Guide, window sums, a and b are
    // fp64: var = E[I^2] - E[I]^2 cancels against eps = 0.002, and the tests bound the result against the fp64 run of alpha.py
    // by a small multiple of what fp32 loses there
    for (int i = threadIdx.x; i < AW * AW; i += 256) {
        const int ly = i / AW, lx = i % AW;
        const int gy = y0 - R + ly, gx = x0 - R + lx;
        double a = 0.0, b = 0.0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            double sI = 0, sP = 0, sII = 0, sIP = 0;
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int dx = 0; dx < K; ++dx) {
                    const double g = I_s[(ly + dy) * SW + lx + dx], p = (double)P_s[(ly + dy) * SW + lx + dx];
                    sI += g; sP += p; sII += g * g; sIP += g * p;
                }
            const double mI = sI / k2, mP = sP / k2;
            const double var = sII / k2 - mI * mI, cov = sIP / k2 - mI * mP;
            a = cov / (var + eps);
            b = mP - a * mI;
        }
        A_s[i] = a; B_s[i] = b;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ALPHA_TILE * ALPHA_TILE; i += 256) {
        const int ly = i / ALPHA_TILE, lx = i % ALPHA_TILE;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        double sA = 0, sB = 0;
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dx = 0; dx < K; ++dx) { sA += A_s[(ly + dy) * AW + lx + dx]; sB += B_s[(ly + dy) * AW + lx + dx]; }
        float q = (float)(sA / k2 * I_s[(ly + 2 * R) * SW + lx + 2 * R] + sB / k2);
        const int64_t px = frame + (int64_t)gy * W + gx;
        const int n = nmap[px];
        const int e8 = alpha_edge_byte(n, nmax);
        if (edge_out) edge_out[px] = (unsigned char)e8;
        if constexpr (R == 2) {                                   // binary matte: steps 3-8 of edge_guided_alpha_upscale
            int zone_n = n;                                       // 3x3 max-pool of the edge map = edge byte of the pooled n
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = gy + dy, xx = gx + dx;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) zone_n = max(zone_n, nmap[frame + (int64_t)yy * W + xx]);
                }
            const float edge = (float)e8 / 255.f, zone = (float)alpha_edge_byte(zone_n, nmax) / 255.f;
            const float contrast = 1.f / (1.f + expf(-((q - 0.5f) * 12.f)));
            const float strength = fminf(fmaxf(edge / 0.25f, 0.f), 1.f);
            const float in_edges = q * (1.f - strength) + contrast * strength;
            float v = zone < 0.05f ? (q > 0.5f ? 1.f : 0.f) : in_edges;
            if (zone < 0.03f) v = v > 0.5f ? 1.f : 0.f;
            if (v > 0.3f && v < 0.7f && !(edge > 0.15f)) v = v > 0.5f ? 1.f : 0.f;
            q = v;
        }
        out[px] = fminf(fmaxf(q, 0.f), 1.f);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void alpha_refine_kernel(const void* __restrict__ rgb, int64_t ld_px, const float* __restrict__ base,
                                                           int H, int W, float n_alpha, const int* __restrict__ flags,
                                                           const int* __restrict__ nmap, const int* __restrict__ maxima,
                                                           float* __restrict__ out, unsigned char* __restrict__ edge_out) {
    // guide fp64 15.1 KiB + base fp32 7.6 KiB + a, b fp64 2 x 11.3 KiB = 45.3 KiB: three workgroups per CU
    __shared__ double I_s[(ALPHA_TILE + 4 * ALPHA_RMAX) * (ALPHA_TILE + 4 * ALPHA_RMAX)];
    __shared__ float P_s[(ALPHA_TILE + 4 * ALPHA_RMAX) * (ALPHA_TILE + 4 * ALPHA_RMAX)];
    __shared__ double A_s[(ALPHA_TILE + 2 * ALPHA_RMAX) * (ALPHA_TILE + 2 * ALPHA_RMAX)];
    __shared__ double B_s[(ALPHA_TILE + 2 * ALPHA_RMAX) * (ALPHA_TILE + 2 * ALPHA_RMAX)];
    // (count(a < 0.1) + count(a > 0.9)) / numel > 0.95 in fp32, counts converted before the addition; uniform over the grid
    const bool binary = ((float)flags[0] + (float)flags[1]) / n_alpha > 0.95f;
    const bool neg0 = flags[2] != 0;
    const int nmax = maxima[blockIdx.z];
    if (binary) alpha_refine_tile<KIND, 2>(I_s, P_s, A_s, B_s, rgb, ld_px, base, H, W, neg0, nmap, nmax, out, edge_out);
    else alpha_refine_tile<KIND, 3>(I_s, P_s, A_s, B_s, rgb, ld_px, base, H, W, neg0, nmap, nmax, out, edge_out);
}

}  // namespace svr
