// Interlaced sources made progressive on the packed planes, before svr_frame_unpack.hip widens them (deinterlace.py is the
// specification, bit for bit: integers in, integers out).  Streaming kernels: no LDS, no atomics, capped grids with a grid-stride
// loop, 64-bit offsets (T * frame elements passes 2^31 for long 1080-line clips).
// Launch rule: ONE LAUNCH PER PLANE -- one for rgb8 / bgr8 / rgb16, three (Y, Cb, Cr) for yuv420p8 / yuv420p10: each plane has its own
// rows R, samples per row N and column step s (the samples of one channel lie s elements apart), and each is routed on its own:
//   deint_vec_kernel    the plane's every row starts on 16 bytes in every operand (all four pointers, the plane's offset, N and the
//                       frame size are multiples of 16 bytes).  A lane owns one 16-byte unit of one output row: 16 samples of 8
//                       bits, 8 of 16 bits.  A kept row is ONE 16-byte load and ONE 16-byte store.  A computed row reads the eight
//                       operands that sit at the output's own columns -- B[r], A[r], P[up], P[dn], Nx[up], Nx[dn] and c = cur[up],
//                       e = cur[dn] -- as 16-byte loads, the 3 s samples of cur[up] and cur[dn] on either side of the unit (the
//                       edge search's reach) one by one, and stores 16 bytes.
//   deint_elem_kernel   any other geometry: a lane owns one sample, element accesses.
// The frame outside the clip is ``before`` / ``after`` where given, else the mirror F[min(1, T-1)] / F[max(T-2, 0)].
// A sample the edge search would read outside its row is never used (the search runs only where i - 3 s >= 0 and i + 3 s <= N - 1);
// the vector kernel fills those window slots with zero instead of loading them.  All arithmetic in int32: samples are below 2^16, a
// score is a sum of three differences.
#include "svr_common.h"
#include "../../include/seedvr2_hip.h"

namespace svr {

// the clip with its two context frames: frame j in -1 .. T
template <class S>
struct DeintClip {
    const S* packed;
    const S* before;                                  // may be null: the mirror
    const S* after;
    int T;
    int64_t frame;                                    // elements per frame
    SVR_DEVICE const S* at(int j) const {
        if (j < 0) return before ? before : packed + (int64_t)(T > 1 ? 1 : 0) * frame;
        if (j >= T) return after ? after : packed + (int64_t)(T > 1 ? T - 2 : 0) * frame;
        return packed + (int64_t)j * frame;
    }
};

SVR_DEVICE int deint_abs(int v) { return v < 0 ? -v : v; }

// the temporal half and the clamp: sp the spatial prediction, b / a the missing-parity samples before / after, c / e the kept rows
// above / below, (pu, pd) / (nu, nd) those rows in the previous / next frame
SVR_DEVICE int deint_blend(int sp, int b, int a, int c, int e, int pu, int pd, int nu, int nd) {
    const int d = (b + a) >> 1;
    const int t0 = deint_abs(b - a) >> 1;
    const int t1 = (deint_abs(pu - c) + deint_abs(pd - e)) >> 1;
    const int t2 = (deint_abs(nu - c) + deint_abs(nd - e)) >> 1;
    const int diff = max(t0, max(t1, t2));
    return min(max(sp, d - diff), d + diff);
}

// the edge search at window position w of cu / ce (the rows above / below; w - 3 s .. w + 3 s are valid slots): deinterlace.py's
// two passes
template <class U, class D>
SVR_DEVICE int deint_search(U&& cu, D&& ce, int s, int sp) {
    auto score = [&](int j) {
        return deint_abs(cu((j - 1) * s) - ce((-1 - j) * s)) + deint_abs(cu(j * s) - ce(-j * s)) + deint_abs(cu((j + 1) * s) - ce((1 - j) * s));
    };
    auto pred = [&](int j) { return (cu(j * s) + ce(-j * s)) >> 1; };
    int best = score(0) - 1;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int j1 = pass ? 1 : -1, j2 = 2 * j1;
        const int s1 = score(j1);
        if (s1 < best) {
            best = s1, sp = pred(j1);
            const int s2 = score(j2);
            if (s2 < best) best = s2, sp = pred(j2);
        }
    }
    return sp;
}

// output frame o -> its source frame t, whether it keeps the second field (k), and the kept parity p
template <int FIELD>
SVR_DEVICE void deint_output(int64_t o, int first, int& t, int& k, int& p) {
    t = FIELD ? (int)(o >> 1) : (int)o;
    k = FIELD ? (int)(o & 1) : 0;
    p = k ? 1 - first : first;
}

// the samples of one 16-byte unit as ints
template <class S>
SVR_DEVICE void deint_load_unit(const S* p, int* v) {
    constexpr int U = 16 / (int)sizeof(S);
    const uint4 a = *(const uint4*)p;
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int j = 0; j < U; ++j)
        v[j] = sizeof(S) == 1 ? (int)((w[j / 4] >> (8 * (j % 4))) & 0xffu) : (int)((w[j / 2] >> (16 * (j % 2))) & 0xffffu);
}

// S: unsigned char / unsigned short; STEP: the plane's column step (1, 3 or 4); FIELD: 1 = two outputs per frame.
// off / R / N: the plane inside a frame (elements).  first: the parity of the first field in time (0 tff, 1 bff).
template <class S, int STEP, int FIELD>
__global__ __launch_bounds__(256) void deint_vec_kernel(DeintClip<S> clip, S* __restrict__ out, int64_t off, int R, int N, int first) {
    constexpr int U = 16 / (int)sizeof(S), HALO = 3 * STEP;
    const int units = N / U;
    const int64_t total = (int64_t)clip.T * (FIELD ? 2 : 1) * R * units;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int x0 = (int)(idx % units) * U, r = (int)(idx / units % R);
        const int64_t o = idx / units / R;
        int t, k, p;
        deint_output<FIELD>(o, first, t, k, p);
        const S* cur = clip.at(t) + off;
        S* dst = out + o * clip.frame + off + (int64_t)r * N + x0;
        if ((r & 1) == p || R == 1) {
            *(uint4*)dst = *(const uint4*)(cur + (int64_t)r * N + x0);
            continue;
        }
        const int up = r >= 1 ? r - 1 : r + 1, dn = r + 1 < R ? r + 1 : r - 1;
        const S* P = clip.at(t - 1) + off;
        const S* Nx = clip.at(t + 1) + off;
        const S* B = k ? cur : P;
        const S* A = k ? Nx : cur;
        const S* cu_row = cur + (int64_t)up * N;
        const S* ce_row = cur + (int64_t)dn * N;
        // the window of the two kept rows: slots [0, HALO) left of the unit, [HALO, HALO + U) the unit, then HALO to its right
        int cu[U + 2 * HALO], ce[U + 2 * HALO];
        deint_load_unit<S>(cu_row + x0, cu + HALO);
        deint_load_unit<S>(ce_row + x0, ce + HALO);
#pragma unroll
        for (int m = 0; m < HALO; ++m) {
            const int lo = x0 - HALO + m, hi = x0 + U + m;
            cu[m] = lo >= 0 ? (int)cu_row[lo] : 0;
            ce[m] = lo >= 0 ? (int)ce_row[lo] : 0;
            cu[HALO + U + m] = hi < N ? (int)cu_row[hi] : 0;
            ce[HALO + U + m] = hi < N ? (int)ce_row[hi] : 0;
        }
        int b[U], a[U], pu[U], pd[U], nu[U], nd[U];
        deint_load_unit<S>(B + (int64_t)r * N + x0, b);
        deint_load_unit<S>(A + (int64_t)r * N + x0, a);
        deint_load_unit<S>(P + (int64_t)up * N + x0, pu);
        deint_load_unit<S>(P + (int64_t)dn * N + x0, pd);
        deint_load_unit<S>(Nx + (int64_t)up * N + x0, nu);
        deint_load_unit<S>(Nx + (int64_t)dn * N + x0, nd);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int i = x0 + j, c = cu[HALO + j], e = ce[HALO + j];
            int sp = (c + e) >> 1;
            if (i - HALO >= 0 && i + HALO <= N - 1)
                sp = deint_search([&](int d) { return cu[HALO + j + d]; }, [&](int d) { return ce[HALO + j + d]; }, STEP, sp);
            const uint32_t v = (uint32_t)deint_blend(sp, b[j], a[j], c, e, pu[j], pd[j], nu[j], nd[j]);
            if (sizeof(S) == 1) w[j / 4] |= v << (8 * (j % 4));
            else w[j / 2] |= v << (16 * (j % 2));
        }
        *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

template <class S, int FIELD>
__global__ __launch_bounds__(256) void deint_elem_kernel(DeintClip<S> clip, S* __restrict__ out, int64_t off, int R, int N, int s,
                                                         int first) {
    const int64_t total = (int64_t)clip.T * (FIELD ? 2 : 1) * R * N;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int i = (int)(idx % N), r = (int)(idx / N % R);
        const int64_t o = idx / N / R;
        int t, k, p;
        deint_output<FIELD>(o, first, t, k, p);
        const S* cur = clip.at(t) + off;
        S* dst = out + o * clip.frame + off + (int64_t)r * N + i;
        if ((r & 1) == p || R == 1) {
            *dst = cur[(int64_t)r * N + i];
            continue;
        }
        const int up = r >= 1 ? r - 1 : r + 1, dn = r + 1 < R ? r + 1 : r - 1;
        const S* P = clip.at(t - 1) + off;
        const S* Nx = clip.at(t + 1) + off;
        const S* B = k ? cur : P;
        const S* A = k ? Nx : cur;
        const S* cu_row = cur + (int64_t)up * N;
        const S* ce_row = cur + (int64_t)dn * N;
        const int c = cu_row[i], e = ce_row[i];
        int sp = (c + e) >> 1;
        if (i - 3 * s >= 0 && i + 3 * s <= N - 1)                              // (every index below then lies in [0, N))
            sp = deint_search([&](int d) { return (int)cu_row[i + d]; }, [&](int d) { return (int)ce_row[i + d]; }, s, sp);
        *dst = (S)deint_blend(sp, B[(int64_t)r * N + i], A[(int64_t)r * N + i], c, e, P[(int64_t)up * N + i], P[(int64_t)dn * N + i],
                              Nx[(int64_t)up * N + i], Nx[(int64_t)dn * N + i]);
    }
}

}  // namespace svr
