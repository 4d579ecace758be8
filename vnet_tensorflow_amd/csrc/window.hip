// window.hip -- libvnet_window.so (csrc/vnet_window.h), gfx950: the glue of a mirrored or weighted sliding-window evaluation.
//   vnet_window_crop_flip  : gather of a window with zero fill past the extent, mirrored along the axes of `mask`.
//   vnet_window_accumulate : vol += w * patch (read mirrored), cnt += w, w the product of three per-axis weights or 1.
// Both are HBM-bound and walk the window ROW by row (a row is the window's last axis): a wave owns one row, or 64 / L rows side by
// side when a row has L <= 32 voxels (L a power of two), forms the row's offsets, its inside-the-volume test and the row's weight
// w0[i] * w1[j] once (one 32-bit division per row), and its lanes walk the row in steps of L voxels.  A thread owns all channels of
// its voxel: K <= 5 values sit in registers, K = 2 / K = 4 move as one float2 / float4 where the bases are aligned for it.  A
// mirrored last axis turns the lane order around inside a row: a wave still reads one contiguous span, whole cache lines.
// No LDS, no atomics: every element belongs to one thread of one launch.  Voxel counts fit an int32 (checked on the host), element
// offsets are 64-bit.  Every float operation is rounded once: contraction is off for this translation unit (the `==` tiers of the
// tests rest on it).
#include <limits.h>
#include "common.h"
#include "vnet_window.h"

#pragma clang fp contract(off)

namespace {

constexpr int WB = 256, WW = WB / 64, W_CAP = 2048, MAX_K = 65535;

// rows of the window -> the grid: lzs = log2(L), L the power of two >= min(P2, 64)
inline int lane_shift(int P2) {
    int s = 0;
    while (s < 6 && (1 << s) < P2) ++s;
    return s;
}
inline int blocks_for_rows(size_t rows, int lzs) {
    const size_t per_wave = (size_t)64 >> lzs, groups = (rows + per_wave - 1) / per_wave, b = (groups + WW - 1) / WW;
    return (int)(b < 1 ? 1 : b > (size_t)W_CAP ? (size_t)W_CAP : b);
}

// the row (i, j) of this lane in trip `grp` of its wave; false past the last row
struct Row {
    unsigned i, j;
    int lk, L;
};
__device__ __forceinline__ bool row_of(size_t grp, int lzs, unsigned P1, size_t nrows, Row& r) {
    const int lane = threadIdx.x & 63;
    r.L = 1 << lzs;
    r.lk = lane & (r.L - 1);
    const size_t row = (grp << (6 - lzs)) + (size_t)(lane >> lzs);
    if (row >= nrows) return false;
    const unsigned q = (unsigned)row;                 // (rows <= voxels <= 2^31 - 1)
    r.i = q / P1;
    r.j = q - r.i * P1;
    return true;
}

// ---- mirrored window of words with zero fill ------------------------------------------------------------------------------------------
struct CropP {
    const unsigned* src;
    unsigned* dst;
    int X, Y, Z, C, sx, sy, sz, P0, P1, P2, mask, lzs;
};

template <bool VEC>
__global__ void __launch_bounds__(WB) window_crop_flip_kernel(CropP p) {
    const size_t nrows = (size_t)p.P0 * p.P1, ngrp = (nrows + (64u >> p.lzs) - 1) >> (6 - p.lzs);
    const unsigned* __restrict__ src = p.src;
    unsigned* __restrict__ dst = p.dst;
    const int C = p.C;
    for (size_t grp = (size_t)blockIdx.x * WW + (threadIdx.x >> 6); grp < ngrp; grp += (size_t)gridDim.x * WW) {
        Row r;
        if (!row_of(grp, p.lzs, (unsigned)p.P1, nrows, r)) continue;
        // (s < extent <= 2^31 - 1 and f < P <= 2^31 - 1: the sums fit an unsigned)
        const unsigned ix = (unsigned)p.sx + ((p.mask & 1) ? (unsigned)p.P0 - 1u - r.i : r.i);
        const unsigned iy = (unsigned)p.sy + ((p.mask & 2) ? (unsigned)p.P1 - 1u - r.j : r.j);
        const bool row_in = ix < (unsigned)p.X && iy < (unsigned)p.Y;
        const unsigned* srow = src + ((size_t)ix * p.Y + iy) * p.Z * C;            // (only read when row_in)
        unsigned* drow = dst + ((size_t)r.i * p.P1 + r.j) * p.P2 * C;
        for (int k = r.lk; k < p.P2; k += r.L) {
            const unsigned iz = (unsigned)p.sz + (unsigned)((p.mask & 4) ? p.P2 - 1 - k : k);
            const bool inside = row_in && iz < (unsigned)p.Z;
            const unsigned* s = srow + (size_t)iz * C;
            unsigned* d = drow + (size_t)k * C;
            if constexpr (VEC) {
                for (int c = 0; c < C; c += 4) {
                    uint4 w = make_uint4(0u, 0u, 0u, 0u);
                    if (inside) w = *reinterpret_cast<const uint4*>(s + c);
                    *reinterpret_cast<uint4*>(d + c) = w;
                }
            } else {
                for (int c = 0; c < C; ++c) d[c] = inside ? s[c] : 0u;
            }
        }
    }
}

// ---- mirrored, weighted accumulation --------------------------------------------------------------------------------------------------
struct AccP {
    const float* patch;
    float* vol;
    float* cnt;
    const float* w0;
    const float* w1;
    const float* w2;
    int K, P0, P1, P2, o0, o1, o2, D0, D1, D2, mask, lzs;
};

// vol[0 .. KT) = vol + w * patch for one voxel; KT values in registers, one access per array where V says so
template <int KT, bool V, bool WGT>
__device__ __forceinline__ void add_voxel(const float* __restrict__ ps, float* __restrict__ vs, float w) {
    if constexpr (V && KT == 2) {
        const float2 a = *reinterpret_cast<const float2*>(ps);
        float2 b = *reinterpret_cast<float2*>(vs);
        if constexpr (WGT) { b.x = b.x + w * a.x; b.y = b.y + w * a.y; }
        else { b.x = b.x + a.x; b.y = b.y + a.y; }
        *reinterpret_cast<float2*>(vs) = b;
    } else if constexpr (V && KT == 4) {
        const float4 a = *reinterpret_cast<const float4*>(ps);
        float4 b = *reinterpret_cast<float4*>(vs);
        if constexpr (WGT) { b.x = b.x + w * a.x; b.y = b.y + w * a.y; b.z = b.z + w * a.z; b.w = b.w + w * a.w; }
        else { b.x = b.x + a.x; b.y = b.y + a.y; b.z = b.z + a.z; b.w = b.w + a.w; }
        *reinterpret_cast<float4*>(vs) = b;
    } else {
        float a[KT], b[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c) { a[c] = ps[c]; b[c] = vs[c]; }
#pragma unroll
        for (int c = 0; c < KT; ++c) vs[c] = WGT ? b[c] + w * a[c] : b[c] + a[c];
    }
}

// KT: the class count as a constant (1 .. 5), 0 = read p.K
template <int KT, bool V, bool WGT>
__global__ void __launch_bounds__(WB) window_accumulate_kernel(AccP p) {
    const size_t nrows = (size_t)p.P0 * p.P1, ngrp = (nrows + (64u >> p.lzs) - 1) >> (6 - p.lzs);
    const int K = KT ? KT : p.K;
    const float* __restrict__ w2 = p.w2;
    // the part of a row that lies inside the volume: k < min(P2, D2 - o2)
    const int kend = p.o2 >= p.D2 ? 0 : (p.D2 - p.o2 < p.P2 ? p.D2 - p.o2 : p.P2);
    for (size_t grp = (size_t)blockIdx.x * WW + (threadIdx.x >> 6); grp < ngrp; grp += (size_t)gridDim.x * WW) {
        Row r;
        if (!row_of(grp, p.lzs, (unsigned)p.P1, nrows, r)) continue;
        const unsigned gx = (unsigned)p.o0 + r.i, gy = (unsigned)p.o1 + r.j;          // (o, i <= 2^31 - 1: no wrap)
        if (gx >= (unsigned)p.D0 || gy >= (unsigned)p.D1) continue;
        const unsigned si = (p.mask & 1) ? (unsigned)p.P0 - 1u - r.i : r.i, sj = (p.mask & 2) ? (unsigned)p.P1 - 1u - r.j : r.j;
        const float* prow = p.patch + ((size_t)si * p.P1 + sj) * p.P2 * K;
        const size_t g0 = ((size_t)gx * p.D1 + gy) * p.D2 + (size_t)p.o2;
        float* vrow = p.vol + g0 * K;
        float* crow = p.cnt ? p.cnt + g0 : nullptr;
        float wr = 1.0f;
        if constexpr (WGT) wr = p.w0[r.i] * p.w1[r.j];
        for (int k = r.lk; k < kend; k += r.L) {
            const int sk = (p.mask & 4) ? p.P2 - 1 - k : k;
            float w = 1.0f;
            if constexpr (WGT) w = wr * w2[k];
            const float* ps = prow + (size_t)sk * K;
            float* vs = vrow + (size_t)k * K;
            if constexpr (KT != 0) {
                add_voxel<KT, V, WGT>(ps, vs, w);
            } else {
                for (int c = 0; c < K; ++c) vs[c] = WGT ? vs[c] + w * ps[c] : vs[c] + ps[c];
            }
            if (crow) crow[k] = crow[k] + w;
        }
    }
}

// the host checks: sizes >= 1 (else VNET_E_BADARG), a voxel count an int32 indexes (else VNET_E_UNSUPPORTED)
inline bool sizes_ok(int A, int B, int C) { return A >= 1 && B >= 1 && C >= 1; }
inline bool fits(int A, int B, int C) { return (size_t)A * (size_t)B * (size_t)C <= (size_t)INT_MAX; }
inline bool aligned(const void* a, const void* b, uintptr_t n) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & (n - 1)) == 0;
}

template <int KT, bool V>
int launch_accumulate(const AccP& p, int blocks, hipStream_t st) {
    return with_bool(p.w0 != nullptr, [&](auto WGT) {
        return launch<window_accumulate_kernel<KT, V, decltype(WGT)::value>>(dim3(blocks), dim3(WB), 0, st, p);
    });
}

}  // namespace

extern "C" {

int vnet_window_crop_flip(const void* src, void* dst, int X, int Y, int Z, int C, int sx, int sy, int sz, int P0, int P1, int P2,
                          int mask, void* stream) {
    if (!src || !dst || src == dst || C < 1 || !sizes_ok(X, Y, Z) || !sizes_ok(P0, P1, P2) || sx < 0 || sy < 0 || sz < 0 ||
        sx >= X || sy >= Y || sz >= Z || mask < 0 || mask > 7)
        return VNET_E_BADARG;
    if (!fits(X, Y, Z) || !fits(P0, P1, P2)) return VNET_E_UNSUPPORTED;
    CropP p{};
    p.src = static_cast<const unsigned*>(src); p.dst = static_cast<unsigned*>(dst);
    p.X = X; p.Y = Y; p.Z = Z; p.C = C; p.sx = sx; p.sy = sy; p.sz = sz; p.P0 = P0; p.P1 = P1; p.P2 = P2; p.mask = mask;
    p.lzs = lane_shift(P2);
    const bool vec = C % 4 == 0 && aligned(src, dst, 16);
    const int blocks = blocks_for_rows((size_t)P0 * P1, p.lzs);
    return with_bool(vec, [&](auto V) { return launch<window_crop_flip_kernel<decltype(V)::value>>(dim3(blocks), dim3(WB), 0, (hipStream_t)stream, p); });
}

int vnet_window_accumulate(const float* patch, float* vol, float* cnt, int K, int P0, int P1, int P2, int o0, int o1, int o2,
                           int D0, int D1, int D2, int mask, const float* w0, const float* w1, const float* w2, void* stream) {
    const int given = (w0 != nullptr) + (w1 != nullptr) + (w2 != nullptr);
    if (!patch || !vol || K < 1 || K > MAX_K || !sizes_ok(P0, P1, P2) || !sizes_ok(D0, D1, D2) || o0 < 0 || o1 < 0 || o2 < 0 ||
        mask < 0 || mask > 7 || (given != 0 && given != 3))
        return VNET_E_BADARG;
    if (!fits(D0, D1, D2) || !fits(P0, P1, P2)) return VNET_E_UNSUPPORTED;
    AccP p{};
    p.patch = patch; p.vol = vol; p.cnt = cnt; p.w0 = w0; p.w1 = w1; p.w2 = w2;
    p.K = K; p.P0 = P0; p.P1 = P1; p.P2 = P2; p.o0 = o0; p.o1 = o1; p.o2 = o2; p.D0 = D0; p.D1 = D1; p.D2 = D2; p.mask = mask;
    p.lzs = lane_shift(P2);
    const int blocks = blocks_for_rows((size_t)P0 * P1, p.lzs);
    hipStream_t st = (hipStream_t)stream;
    switch (K) {
        case 1: return launch_accumulate<1, false>(p, blocks, st);
        case 2: return aligned(patch, vol, 8) ? launch_accumulate<2, true>(p, blocks, st) : launch_accumulate<2, false>(p, blocks, st);
        case 3: return launch_accumulate<3, false>(p, blocks, st);
        case 4: return aligned(patch, vol, 16) ? launch_accumulate<4, true>(p, blocks, st) : launch_accumulate<4, false>(p, blocks, st);
        case 5: return launch_accumulate<5, false>(p, blocks, st);
        default: return launch_accumulate<0, false>(p, blocks, st);
    }
}

}  // extern "C"
