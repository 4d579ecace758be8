// prepare.hip -- a case of evaluate on the device, in front of the network and behind it (include/vnet_hip_prepare.h), gfx950.
//   vnet_channel_stats    : {sum, css, min, max} per channel in fp64.  grid = (blocks over the voxels, channel units): a block's threads
//                           all work on the same channel (or channel quad), so the pre-map and the mean are wave-uniform and a thread
//                           keeps its accumulators in registers.  pass 1 (sum, min, max) -> finalize (fixed order; mean = sum / n)
//                           -> pass 2 (css about that mean) -> finalize.  Per thread, per wave (shuffles), per block (LDS), one partial
//                           per block in ws: no atomics, the same bits every run.
//   vnet_window_intensity : transforms._window operation for operation, the same grid shape (the five parameters are wave-uniform).
//   vnet_crop_words       : gather of a window with zero fill past the extent, flat grid-stride (sample.hip's crop without the label).
//   vnet_argmax_label     : one row per thread, rows read as float4 / float2 / float as K and the base's alignment allow.
// All four are HBM-bound; no LDS beyond the block reductions.  Voxel counts fit an int32 (checked on the host), element offsets are 64-bit.
// Every fp64 operation is rounded once: contraction is off for this translation unit (the `==` tiers of the tests rest on it).
#include <math.h>
#include <limits.h>
#include "common.h"
#include "../../include/vnet_hip_prepare.h"

#pragma clang fp contract(off)

namespace {

constexpr int PB = 256, PW = PB / 64, ST_CAP = VNET_STATS_MAX_BLOCKS, EW_CAP = 4096, MAX_CU = 65535;

typedef long long i64;

inline int blocks_for(size_t units, int cap) {
    size_t b = (units + PB - 1) / PB;
    return (int)(b < 1 ? 1 : b > (size_t)cap ? (size_t)cap : b);
}

// np.min / np.max: a NaN on either side wins
__device__ __forceinline__ double min_nan(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min_nan(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- channel statistics -----------------------------------------------------------------------------------------------------------
// ws: part [C][ST_CAP][4] = {sum, css, min, max} of block b of channel c, then mean [C]
struct StatsP {
    const float* x;
    const double* pre;
    double* part;
    double* mean;
    double* out;
    i64 n;
    int C, nblk;
};

template <int W>
__device__ __forceinline__ void load_unit(const float* x, i64 v, int C, int c0, float f[W]) {
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4*>(x + (size_t)v * C + c0);
        f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
    } else {
        f[0] = x[(size_t)v * C + c0];
    }
}

// PASS 0: sum, min, max.  PASS 1: css about mean[c].  VEC: a unit is 4 consecutive channels of a voxel, else one channel.
template <bool VEC, int PASS>
__global__ void __launch_bounds__(PB) stats_pass_kernel(StatsP p) {
    constexpr int W = VEC ? 4 : 1, NV = PASS == 0 ? 3 : 1;
    __shared__ double red[PW][W][NV];
    const int c0 = blockIdx.y * W;
    const bool mapped = p.pre != nullptr;
    double a[W], b[W], mean[W], acc[W], mn[W], mx[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        a[j] = mapped ? p.pre[2 * (c0 + j)] : 0.0;
        b[j] = mapped ? p.pre[2 * (c0 + j) + 1] : 1.0;
        mean[j] = PASS == 1 ? p.mean[c0 + j] : 0.0;
        acc[j] = 0.0; mn[j] = INFINITY; mx[j] = -INFINITY;
    }
    for (i64 v = (i64)blockIdx.x * PB + threadIdx.x; v < p.n; v += (i64)gridDim.x * PB) {
        float f[W];
        load_unit<W>(p.x, v, p.C, c0, f);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const double val = mapped ? ((double)f[j] - a[j]) / b[j] : (double)f[j];
            if constexpr (PASS == 0) {
                acc[j] = acc[j] + val;
                mn[j] = min_nan(mn[j], val);
                mx[j] = max_nan(mx[j], val);
            } else {
                const double d = val - mean[j];
                const double q = d * d;
                acc[j] = acc[j] + q;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const double s = wave_sum_d(acc[j]);
        double lo = 0.0, hi = 0.0;
        if constexpr (PASS == 0) { lo = wave_min_d(mn[j]); hi = wave_max_d(mx[j]); }
        if (lane == 0) {
            red[wave][j][0] = s;
            if constexpr (PASS == 0) { red[wave][j][1] = lo; red[wave][j][2] = hi; }
        }
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int j = threadIdx.x;
        double s = red[0][j][0];
#pragma unroll
        for (int w = 1; w < PW; ++w) s = s + red[w][j][0];
        double* row = p.part + ((size_t)(c0 + j) * ST_CAP + blockIdx.x) * 4;
        if constexpr (PASS == 0) {
            double lo = red[0][j][1], hi = red[0][j][2];
#pragma unroll
            for (int w = 1; w < PW; ++w) { lo = min_nan(lo, red[w][j][1]); hi = max_nan(hi, red[w][j][2]); }
            row[0] = s; row[2] = lo; row[3] = hi;
        } else {
            row[1] = s;
        }
    }
}

// one block per channel: the partials of blocks t, t + PB, ... per thread in ascending order, then wave and block as above.
// PASS 0 writes sum, min, max and the mean; PASS 1 writes css.
template <int PASS>
__global__ void __launch_bounds__(PB) stats_finalize_kernel(StatsP p) {
    constexpr int NV = PASS == 0 ? 3 : 1;
    __shared__ double red[PW][NV];
    const int c = blockIdx.x;
    const double* part = p.part + (size_t)c * ST_CAP * 4;
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int b = threadIdx.x; b < p.nblk; b += PB) {
        s = s + part[4 * b + (PASS == 0 ? 0 : 1)];
        if constexpr (PASS == 0) { lo = min_nan(lo, part[4 * b + 2]); hi = max_nan(hi, part[4 * b + 3]); }
    }
    s = wave_sum_d(s);
    if constexpr (PASS == 0) { lo = wave_min_d(lo); hi = wave_max_d(hi); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = s;
        if constexpr (PASS == 0) { red[wave][1] = lo; red[wave][2] = hi; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0][0];
#pragma unroll
        for (int w = 1; w < PW; ++w) t = t + red[w][0];
        if constexpr (PASS == 0) {
            double l = red[0][1], h = red[0][2];
#pragma unroll
            for (int w = 1; w < PW; ++w) { l = min_nan(l, red[w][1]); h = max_nan(h, red[w][2]); }
            p.out[4 * c + 0] = t; p.out[4 * c + 2] = l; p.out[4 * c + 3] = h;
            p.mean[c] = t / (double)p.n;
        } else {
            p.out[4 * c + 1] = t;
        }
    }
}

// ---- intensity window -------------------------------------------------------------------------------------------------------------
// (in and out may be the same array: no __restrict__)
template <bool VEC>
__global__ void __launch_bounds__(PB) window_kernel(const float* in, float* out, const double* __restrict__ prm, i64 n, int C) {
    constexpr int W = VEC ? 4 : 1;
    const int c0 = blockIdx.y * W;
    double a[W], b[W], wmin[W], scale[W];
    bool flat[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const double* r = prm + 5 * (c0 + j);
        a[j] = r[0]; b[j] = r[1]; wmin[j] = r[2]; scale[j] = r[3]; flat[j] = r[4] != 0.0;
    }
    for (i64 v = (i64)blockIdx.x * PB + threadIdx.x; v < n; v += (i64)gridDim.x * PB) {
        float f[W], g[W];
        load_unit<W>(in, v, C, c0, f);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const double val = ((double)f[j] - a[j]) / b[j];
            if (flat[j]) {
                g[j] = val < wmin[j] ? 0.0f : 255.0f;
            } else {
                const double t = val - wmin[j];
                const double u = t * scale[j];
                const double y = u + 0.0;
                g[j] = (float)(y < 0.0 ? 0.0 : (y > 255.0 ? 255.0 : y));
            }
        }
        if constexpr (VEC) *reinterpret_cast<float4*>(out + (size_t)v * C + c0) = make_float4(g[0], g[1], g[2], g[3]);
        else out[(size_t)v * C + c0] = g[0];
    }
}

// ---- window of words with zero fill -----------------------------------------------------------------------------------------------
struct CropP {
    const unsigned* src;
    unsigned* dst;
    int X, Y, Z, C, sx, sy, sz, P0, P1, P2;
};

template <bool VEC>
__global__ void __launch_bounds__(PB) crop_words_kernel(CropP p) {
    const int CU = VEC ? p.C >> 2 : p.C;
    const size_t n = (size_t)p.P0 * p.P1 * p.P2 * CU;
    const unsigned* __restrict__ src = p.src;
    unsigned* __restrict__ dst = p.dst;
    for (size_t idx = (size_t)blockIdx.x * PB + threadIdx.x; idx < n; idx += (size_t)gridDim.x * PB) {
        size_t v = idx / CU;
        const int cu = (int)(idx - v * CU);
        const int oz = (int)(v % p.P2); v /= p.P2;
        const int oy = (int)(v % p.P1), ox = (int)(v / p.P1);
        // (s < extent <= 2^31 - 1 and o < P <= 2^31 - 1: the sums fit an unsigned)
        const unsigned ix = (unsigned)p.sx + (unsigned)ox, iy = (unsigned)p.sy + (unsigned)oy, iz = (unsigned)p.sz + (unsigned)oz;
        const bool inside = ix < (unsigned)p.X && iy < (unsigned)p.Y && iz < (unsigned)p.Z;
        const size_t iv = ((size_t)ix * p.Y + iy) * p.Z + iz;
        if constexpr (VEC) {
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (inside) w = *reinterpret_cast<const uint4*>(src + iv * p.C + (size_t)cu * 4);
            reinterpret_cast<uint4*>(dst)[idx] = w;
        } else {
            dst[idx] = inside ? src[iv * p.C + cu] : 0u;
        }
    }
}

// ---- argmax -----------------------------------------------------------------------------------------------------------------------
// the running best is replaced by a larger value or by the first NaN, and by nothing once it is a NaN
__device__ __forceinline__ void argmax_step(float v, int k, float& best, int& at) {
    if (best == best && (v > best || v != v)) { best = v; at = k; }
}

template <int V>
__global__ void __launch_bounds__(PB) argmax_kernel(const float* __restrict__ vol, int* __restrict__ label, i64 n, int K) {
    for (i64 r = (i64)blockIdx.x * PB + threadIdx.x; r < n; r += (i64)gridDim.x * PB) {
        const float* row = vol + (size_t)r * K;
        float best;
        int at = 0;
        if constexpr (V == 4) {
            const float4 f = *reinterpret_cast<const float4*>(row);
            best = f.x;
            argmax_step(f.y, 1, best, at); argmax_step(f.z, 2, best, at); argmax_step(f.w, 3, best, at);
            for (int k = 4; k < K; k += 4) {
                const float4 g = *reinterpret_cast<const float4*>(row + k);
                argmax_step(g.x, k, best, at); argmax_step(g.y, k + 1, best, at);
                argmax_step(g.z, k + 2, best, at); argmax_step(g.w, k + 3, best, at);
            }
        } else if constexpr (V == 2) {
            const float2 f = *reinterpret_cast<const float2*>(row);
            best = f.x;
            argmax_step(f.y, 1, best, at);
            for (int k = 2; k < K; k += 2) {
                const float2 g = *reinterpret_cast<const float2*>(row + k);
                argmax_step(g.x, k, best, at); argmax_step(g.y, k + 1, best, at);
            }
        } else {
            best = row[0];
            for (int k = 1; k < K; ++k) argmax_step(row[k], k, best, at);
        }
        label[r] = at;
    }
}

inline size_t stats_ws(int C) { return sizeof(double) * (size_t)C * (4 * (size_t)ST_CAP + 1); }

// 0, VNET_E_BADARG on a size < 1, VNET_E_UNSUPPORTED when an int32 cannot index the volume
inline int volume_count(int X, int Y, int Z, size_t& n) {
    if (X < 1 || Y < 1 || Z < 1) return VNET_E_BADARG;
    n = (size_t)X * (size_t)Y * (size_t)Z;
    return n > (size_t)INT_MAX ? VNET_E_UNSUPPORTED : 0;
}

inline bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

}  // namespace

extern "C" {

size_t vnet_channel_stats_ws_bytes(int C) { return C < 1 || C > MAX_CU ? 0 : stats_ws(C); }

int vnet_channel_stats(const float* image, const double* pre, double* out, long long n, int C, void* ws, size_t ws_bytes, void* stream) {
    if (!image || !out || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || n < 1 || C < 1) return VNET_E_BADARG;
    if (n > (long long)INT_MAX || C > MAX_CU) return VNET_E_UNSUPPORTED;
    if (ws_bytes < stats_ws(C)) return VNET_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    StatsP p{};
    p.x = image; p.pre = pre; p.out = out; p.n = n; p.C = C;
    p.part = static_cast<double*>(ws);
    p.mean = p.part + (size_t)C * ST_CAP * 4;
    p.nblk = blocks_for((size_t)n, ST_CAP);
    const bool vec = C % 4 == 0 && aligned16(image, nullptr);
    const dim3 grid(p.nblk, vec ? C / 4 : C), fin(C);
    return with_bool(vec, [&](auto V) {
        if (int e = launch<stats_pass_kernel<V, 0>>(grid, dim3(PB), 0, st, p)) return e;
        if (int e = launch<stats_finalize_kernel<0>>(fin, dim3(PB), 0, st, p)) return e;
        if (int e = launch<stats_pass_kernel<V, 1>>(grid, dim3(PB), 0, st, p)) return e;
        return launch<stats_finalize_kernel<1>>(fin, dim3(PB), 0, st, p);
    });
}

int vnet_window_intensity(const float* in, float* out, const double* prm, long long n, int C, void* stream) {
    if (!in || !out || !prm || n < 1 || C < 1) return VNET_E_BADARG;
    if (n > (long long)INT_MAX || C > MAX_CU) return VNET_E_UNSUPPORTED;
    const bool vec = C % 4 == 0 && aligned16(in, out);
    const dim3 grid(blocks_for((size_t)n, EW_CAP), vec ? C / 4 : C);
    return with_bool(vec, [&](auto V) { return launch<window_kernel<V>>(grid, dim3(PB), 0, (hipStream_t)stream, in, out, prm, (i64)n, C); });
}

int vnet_crop_words(const void* src, void* dst, int X, int Y, int Z, int C, int sx, int sy, int sz, int P0, int P1, int P2, void* stream) {
    size_t n = 0, m = 0;
    if (!src || !dst || C < 1 || X < 1 || Y < 1 || Z < 1 || P0 < 1 || P1 < 1 || P2 < 1 || sx < 0 || sy < 0 || sz < 0 ||
        sx >= X || sy >= Y || sz >= Z)
        return VNET_E_BADARG;
    if (int e = volume_count(X, Y, Z, n)) return e;
    if (int e = volume_count(P0, P1, P2, m)) return e;
    CropP p{};
    p.src = static_cast<const unsigned*>(src); p.dst = static_cast<unsigned*>(dst);
    p.X = X; p.Y = Y; p.Z = Z; p.C = C; p.sx = sx; p.sy = sy; p.sz = sz; p.P0 = P0; p.P1 = P1; p.P2 = P2;
    const bool vec = C % 4 == 0 && aligned16(src, dst);
    const size_t units = m * (size_t)(vec ? C / 4 : C);
    return with_bool(vec, [&](auto V) { return launch<crop_words_kernel<V>>(dim3(blocks_for(units, EW_CAP)), dim3(PB), 0, (hipStream_t)stream, p); });
}

int vnet_argmax_label(const float* vol, int* label, long long n, int K, void* stream) {
    if (!vol || !label || n < 1 || K < 1) return VNET_E_BADARG;
    if (n > (long long)INT_MAX) return VNET_E_UNSUPPORTED;
    const uintptr_t a = reinterpret_cast<uintptr_t>(vol);
    const int v = (K % 4 == 0 && (a & 15) == 0) ? 4 : (K % 2 == 0 && (a & 7) == 0) ? 2 : 1;
    const dim3 grid(blocks_for((size_t)n, EW_CAP));
    return with_int<1, 2, 4>(v, [&](auto V) {
        return launch<argmax_kernel<decltype(V)::value>>(grid, dim3(PB), 0, (hipStream_t)stream, vol, label, (i64)n, K);
    });
}

}  // extern "C"
