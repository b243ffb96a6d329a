// GGUF block-quantised weights expanded to bf16 (or fp32) on the device at load (gguf.py is the specification, bit for bit).
// Streaming kernels: no LDS, no atomics, a capped grid with a grid-stride loop over UNITS of eight consecutive outputs.  A lane
// owns one unit: 16 bytes of bf16 (one store) or 32 bytes of fp32 (two stores); unit u of the tensor is outputs 8u .. 8u + 7, so
// a 256-element block is 32 units and a Q8_0 block four, and every unit lies inside one sub-block: one scale (and min) per lane,
// decoded once.
//   Q8_0  34 B   d | int8 q[32]                                x = d * q
//   Q4_K  144 B  d | dmin | scales[12] | qs[128]               x = (d * sc) * q - dmin * m     q: a nibble of qs[32 (e / 64) + e % 32]
//   Q5_K  176 B  d | dmin | scales[12] | qh[32] | qs[128]      the same with bit e / 32 of qh[e % 32] as the fifth bit
//   Q6_K  210 B  ql[128] | qh[64] | int8 scales[16] | d        x = (d * scales[e / 16]) * (q - 32)
// d, dmin: IEEE fp16.  d * sc * q is exact in fp32 (11 + 7 + 5 significant bits), the subtraction is the one rounding: contracted to
// an FMA or not, the bits are the same.
// Alignment: the base is 32-byte aligned (checked by the entry point).  Q4_K / Q5_K blocks are multiples of 16 bytes: a lane's
// eight quant bytes are one 8-byte load, the header words 4-byte loads.  Q8_0 and Q6_K blocks are only 2-byte aligned (their phase
// against 16 bytes has period 8): they are read with 2-byte loads (the int8 sub-scale of Q6_K with a byte load), never with a wide
// load off its natural alignment.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

SVR_DEVICE float gguf_half(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }

// eight bytes from a 2-byte aligned address, as two little-endian words
SVR_DEVICE uint2 gguf_load8_a2(const unsigned char* p) {
    const unsigned short* h = (const unsigned short*)p;
    return make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
}
SVR_DEVICE uint32_t gguf_byte(const uint2& v, int k) { return ((k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 0xffu; }

// six-bit scale and min of sub-block j (0..7) from the 12 scale bytes (three little-endian words)
SVR_DEVICE void gguf_k_scale_min(uint32_t s0, uint32_t s1, uint32_t s2, int j, float& sc, float& mn) {
    auto byte = [&](int i) { return ((i < 4 ? s0 : i < 8 ? s1 : s2) >> (8 * (i & 3))) & 0xffu; };   // (selects: no indexed array)
    uint32_t a, b;
    if (j < 4) { a = byte(j) & 63u; b = byte(j + 4) & 63u; }
    else { a = (byte(j + 4) & 15u) | ((byte(j - 4) >> 6) << 4); b = (byte(j + 4) >> 4) | ((byte(j) >> 6) << 4); }
    sc = (float)a; mn = (float)b;
}

template <int KIND>                                  // SVR_STORE_BF16 / SVR_STORE_FP32
SVR_DEVICE void gguf_store8(void* out, int64_t u, const float* x) {
    if constexpr (KIND == SVR_STORE_BF16) {
        *(uint4*)((unsigned short*)out + 8 * u) = pack8(x);
    } else {
        float4* o = (float4*)((float*)out + 8 * u);
        o[0] = make_float4(x[0], x[1], x[2], x[3]);
        o[1] = make_float4(x[4], x[5], x[6], x[7]);
    }
}

template <int TYPE, int KIND>
__global__ __launch_bounds__(256) void dequant_gguf_kernel(const unsigned char* __restrict__ blocks, void* __restrict__ out,
                                                           int64_t n_units) {
    constexpr int BYTES = TYPE == SVR_GGML_Q8_0 ? 34 : TYPE == SVR_GGML_Q4_K ? 144 : TYPE == SVR_GGML_Q5_K ? 176 : 210;
    constexpr int UNITS = TYPE == SVR_GGML_Q8_0 ? 4 : 32;                  // per block
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n_units; u += step) {
        const unsigned char* blk = blocks + (u / UNITS) * BYTES;
        const int p = (int)(u % UNITS);                                    // the unit inside its block: elements 8p .. 8p + 7
        float x[8];
        if constexpr (TYPE == SVR_GGML_Q8_0) {
            const float d = gguf_half(*(const unsigned short*)blk);
            const uint2 q = gguf_load8_a2(blk + 2 + 8 * p);
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = d * (float)(int)(signed char)gguf_byte(q, k);
        } else if constexpr (TYPE == SVR_GGML_Q4_K || TYPE == SVR_GGML_Q5_K) {
            const uint4 head = *(const uint4*)blk;                         // d | dmin, scales[12]
            const int j = p >> 2, l0 = 8 * (p & 3);                        // sub-block, first position in it
            float sc, mn;
            gguf_k_scale_min(head.y, head.z, head.w, j, sc, mn);
            const float dl = gguf_half(head.x & 0xffffu) * sc, dm = gguf_half(head.x >> 16) * mn;
            constexpr int QS = TYPE == SVR_GGML_Q4_K ? 16 : 48;
            const uint2 qs = *(const uint2*)(blk + QS + 32 * (j >> 1) + l0);
            uint2 qh = make_uint2(0u, 0u);
            if constexpr (TYPE == SVR_GGML_Q5_K) qh = *(const uint2*)(blk + 16 + l0);
            const int shift = 4 * (j & 1);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                uint32_t q = (gguf_byte(qs, k) >> shift) & 15u;
                if constexpr (TYPE == SVR_GGML_Q5_K) q |= ((gguf_byte(qh, k) >> j) & 1u) << 4;
                x[k] = dl * (float)q - dm;
            }
        } else {
            const int h = p >> 4, r = (p >> 2) & 3, l0 = 8 * (p & 3);      // half, row of 32 in it, first position in the row
            const uint2 ql = gguf_load8_a2(blk + 64 * h + 32 * (r & 1) + l0);
            const uint2 qh = gguf_load8_a2(blk + 128 + 32 * h + l0);
            const float dl = gguf_half(*(const unsigned short*)(blk + 208)) * (float)(int)((const signed char*)blk)[192 + (p >> 1)];
            const int lo_shift = 4 * (r >> 1), hi_shift = 2 * r;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q = (int)(((gguf_byte(ql, k) >> lo_shift) & 15u) | (((gguf_byte(qh, k) >> hi_shift) & 3u) << 4)) - 32;
                x[k] = dl * (float)q;
            }
        }
        gguf_store8<KIND>(out, u, x);
    }
}

}  // namespace svr
