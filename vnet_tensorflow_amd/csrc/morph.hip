// morph.hip -- the data-preparation tools on the device (csrc/vnet_tools.h), gfx950.
//   vnet_select_bits : one wave per word: lane k reads voxel c = 64 w + k of a row in the label's own dtype, the wave's ballot is the
//                      word (lanes at c >= C vote 0, which keeps the unused high bits zero).  Reads the label once.
//   vnet_dilate_bits : a block takes a tile of 8 x 32 rows of ONE word column w.  It stages the (8 + 2r) x (32 + 2r) source words of
//                      the tile and its halo in LDS, each already SPREAD along c for the r + 1 distinct half-widths h = 0 .. r
//                      (OR of the word shifted by -h .. h bits, the carries from words w - 1 and w + 1), formed once per source word.
//                      An output word is then the OR, over the in-plane offsets (da, db) of the ball, of the neighbour row's spread
//                      of half-width h(da, db): one ds_read_b64 per offset (97 at r = 5) for 64 voxels.  A half-wave reads 32
//                      consecutive words, so the reads are conflict-free.  LDS: (r + 1)(8 + 2r)(32 + 2r) * 8 bytes, 82944 at r = 8.
//                      The offsets and h are folded at compile time (one instance per r).
//   vnet_bits_bbox   : a thread per word (popcount, first / last set bit), 64-lane butterfly, one set of integer atomics per wave
//                      that saw a set bit.
//   vnet_masked_crop : a thread per destination element of 1 / 2 / 4 / 8 bytes; vnet_unpack_bits: a thread per voxel.
// Voxel counts fit an int32 (checked on the host); word, element and byte offsets are size_t.
#include <limits.h>
#include "common.h"
#include "vnet_tools.h"

namespace {

constexpr int PB = 256, CAP = 4096, BBOX_CAP = 256, TA = 8, TB = 32;

typedef unsigned long long u64;
typedef long long i64;

inline int blocks_for(size_t units, int cap) {
    size_t b = (units + PB - 1) / PB;
    return (int)(b < 1 ? 1 : b > (size_t)cap ? (size_t)cap : b);
}

// A * B * C as n; VNET_E_BADARG / VNET_E_UNSUPPORTED
inline int volume_count(int A, int B, int C, size_t& n) {
    if (A < 1 || B < 1 || C < 1) return VNET_E_BADARG;
    n = (size_t)A * (size_t)B * (size_t)C;
    return n > (size_t)INT_MAX ? VNET_E_UNSUPPORTED : 0;
}

// ---- select ---------------------------------------------------------------------------------------------------------------------------
struct Values {
    i64 v[VNET_TOOLS_MAX_VALUES];
    int n;
};

template <typename T>
__global__ __launch_bounds__(PB) void select_bits_kernel(const T* __restrict__ label, u64* __restrict__ bits, Values vals,
                                                         size_t rows, int C, int W) {
    const int lane = threadIdx.x & 63;
    const size_t words = rows * (size_t)W, step = (size_t)gridDim.x * (PB / 64);
    for (size_t idx = (size_t)blockIdx.x * (PB / 64) + (threadIdx.x >> 6); idx < words; idx += step) {
        const size_t row = idx / (size_t)W;
        const int c = (int)(idx - row * (size_t)W) * 64 + lane;
        bool hit = false;
        if (c < C) {
            const i64 x = (i64)label[row * (size_t)C + (size_t)c];
            for (int k = 0; k < vals.n; ++k) hit |= (x == vals.v[k]);
        }
        const u64 word = __ballot(hit);
        if (lane == 0) bits[idx] = word;
    }
}

// ---- dilate ---------------------------------------------------------------------------------------------------------------------------
// the largest dc >= 0 with 4 (s + dc^2) <= (2R + 1)^2, or -1 when the in-plane offset itself lies outside the ball
constexpr int half_width(int R, int s) {
    int h = -1;
    for (int dc = 0; dc <= R; ++dc)
        if (4 * (s + dc * dc) <= (2 * R + 1) * (2 * R + 1)) h = dc;
    return h;
}

constexpr size_t dilate_lds_bytes(int R) { return (size_t)(R + 1) * (TA + 2 * R) * (TB + 2 * R) * sizeof(u64); }

template <int R>
__global__ __launch_bounds__(PB) void dilate_bits_kernel(const u64* __restrict__ in, u64* __restrict__ out, int A, int B, int W,
                                                         u64 last_mask, int tiles_b, size_t ntiles) {
    constexpr int SA = TA + 2 * R, SB = TB + 2 * R, PLANE = SA * SB;
    extern __shared__ u64 spread[];          // [R + 1][SA][SB]
    const int tid = threadIdx.x, la = tid / TB, lb = tid % TB;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int w = (int)(tile % (size_t)W);
        const size_t t2 = tile / (size_t)W;
        const int a0 = (int)(t2 / (size_t)tiles_b) * TA, b0 = (int)(t2 % (size_t)tiles_b) * TB;
        for (int s = tid; s < PLANE; s += PB) {
            const int a = a0 + s / SB - R, b = b0 + s % SB - R;
            u64 x = 0, prev = 0, next = 0;
            if (a >= 0 && a < A && b >= 0 && b < B) {
                const u64* row = in + ((size_t)a * (size_t)B + (size_t)b) * (size_t)W;
                x = row[w];
                if (w > 0) prev = row[w - 1];
                if (w + 1 < W) next = row[w + 1];
            }
            u64 acc = x;
            spread[s] = acc;
#pragma unroll
            for (int h = 1; h <= R; ++h) {
                acc |= (x << h) | (prev >> (64 - h)) | (x >> h) | (next << (64 - h));
                spread[h * PLANE + s] = acc;
            }
        }
        __syncthreads();
        u64 acc = 0;
#pragma unroll
        for (int da = -R; da <= R; ++da) {
#pragma unroll
            for (int db = -R; db <= R; ++db) {
                constexpr int none = -1;
                const int h = half_width(R, da * da + db * db);
                if (h != none) acc |= spread[h * PLANE + (la + da + R) * SB + (lb + db + R)];
            }
        }
        const int a = a0 + la, b = b0 + lb;
        if (a < A && b < B) out[((size_t)a * (size_t)B + (size_t)b) * (size_t)W + (size_t)w] = (w == W - 1) ? (acc & last_mask) : acc;
        __syncthreads();                     // the next tile's staging overwrites what this one read
    }
}

// ---- bounding box ---------------------------------------------------------------------------------------------------------------------
__global__ void bbox_init_kernel(i64* out7, int A, int B, int C) {
    const int t = threadIdx.x;
    if (t < 7) out7[t] = t == 0 ? 0 : t == 1 ? A : t == 2 ? B : t == 3 ? C : -1;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(PB) void bits_bbox_kernel(const u64* __restrict__ bits, i64* out7, int B, int W, size_t words) {
    int count = 0, lo_a = INT_MAX, lo_b = INT_MAX, lo_c = INT_MAX, hi_a = -1, hi_b = -1, hi_c = -1;     // (a thread sees < 2^31 voxels)
    const size_t step = (size_t)gridDim.x * PB;
    for (size_t idx = (size_t)blockIdx.x * PB + threadIdx.x; idx < words; idx += step) {
        const u64 word = bits[idx];
        if (word) {
            const size_t row = idx / (size_t)W;
            const int w = (int)(idx - row * (size_t)W), a = (int)(row / (size_t)B), b = (int)(row - (size_t)a * (size_t)B);
            count += __popcll(word);
            lo_a = min(lo_a, a); hi_a = max(hi_a, a);
            lo_b = min(lo_b, b); hi_b = max(hi_b, b);
            lo_c = min(lo_c, w * 64 + (__ffsll((i64)word) - 1));
            hi_c = max(hi_c, w * 64 + 63 - __clzll((i64)word));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    lo_a = wave_min_i(lo_a); lo_b = wave_min_i(lo_b); lo_c = wave_min_i(lo_c);
    hi_a = wave_max_i(hi_a); hi_b = wave_max_i(hi_b); hi_c = wave_max_i(hi_c);
    if ((threadIdx.x & 63) == 0 && count > 0) {
        atomicAdd(reinterpret_cast<u64*>(out7), (u64)count);
        atomicMin(out7 + 1, (i64)lo_a); atomicMin(out7 + 2, (i64)lo_b); atomicMin(out7 + 3, (i64)lo_c);
        atomicMax(out7 + 4, (i64)hi_a); atomicMax(out7 + 5, (i64)hi_b); atomicMax(out7 + 6, (i64)hi_c);
    }
}

// ---- masked crop, unpack --------------------------------------------------------------------------------------------------------------
struct CropP {
    const void* src;
    const u64* bits;
    void* dst;
    int B, C, W, s0, s1, s2, n1, n2;
    size_t n;
};

template <typename T>
__global__ __launch_bounds__(PB) void masked_crop_kernel(CropP p) {
    const T* __restrict__ src = static_cast<const T*>(p.src);
    T* __restrict__ dst = static_cast<T*>(p.dst);
    const size_t step = (size_t)gridDim.x * PB;
    for (size_t i = (size_t)blockIdx.x * PB + threadIdx.x; i < p.n; i += step) {
        const size_t q = i / (size_t)p.n2;
        const int c = p.s2 + (int)(i - q * (size_t)p.n2);
        const size_t q1 = q / (size_t)p.n1;
        const size_t row = (q1 + (size_t)p.s0) * (size_t)p.B + (q - q1 * (size_t)p.n1) + (size_t)p.s1;
        T v = src[row * (size_t)p.C + (size_t)c];
        if (p.bits && !((p.bits[row * (size_t)p.W + (size_t)(c >> 6)] >> (c & 63)) & 1)) v = 0;
        dst[i] = v;
    }
}

__global__ __launch_bounds__(PB) void unpack_bits_kernel(const u64* __restrict__ bits, unsigned char* __restrict__ dst, int C, int W, size_t n) {
    const size_t step = (size_t)gridDim.x * PB;
    for (size_t i = (size_t)blockIdx.x * PB + threadIdx.x; i < n; i += step) {
        const size_t row = i / (size_t)C;
        const int c = (int)(i - row * (size_t)C);
        dst[i] = (unsigned char)((bits[row * (size_t)W + (size_t)(c >> 6)] >> (c & 63)) & 1);
    }
}

template <typename T>
int select_launch(const void* label, u64* bits, const Values& vals, size_t rows, int C, int W, hipStream_t st) {
    const size_t words = rows * (size_t)W;
    return launch<select_bits_kernel<T>>(dim3(blocks_for(words * 64, CAP)), dim3(PB), 0, st, static_cast<const T*>(label), bits, vals, rows, C, W);
}

}  // namespace

extern "C" {

int vnet_select_bits(const void* label, int dtype_code, const long long* values, int nvalues, long long* bits,
                     int A, int B, int C, void* stream) {
    size_t n = 0;
    if (!label || !values || !bits || nvalues < 1 || nvalues > VNET_TOOLS_MAX_VALUES || dtype_code < 0 || dtype_code > 4) return VNET_E_BADARG;
    if (int e = volume_count(A, B, C, n)) return e;
    Values vals{};
    for (int k = 0; k < nvalues; ++k) vals.v[k] = values[k];
    vals.n = nvalues;
    const size_t rows = (size_t)A * (size_t)B;
    const int W = (C + 63) / 64;
    u64* out = reinterpret_cast<u64*>(bits);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype_code) {
        case 0: return select_launch<unsigned char>(label, out, vals, rows, C, W, st);
        case 1: return select_launch<signed char>(label, out, vals, rows, C, W, st);
        case 2: return select_launch<short>(label, out, vals, rows, C, W, st);
        case 3: return select_launch<unsigned short>(label, out, vals, rows, C, W, st);
        default: return select_launch<int>(label, out, vals, rows, C, W, st);
    }
}

int vnet_dilate_bits(const long long* bits, long long* out, int A, int B, int C, int r, void* stream) {
    size_t n = 0;
    if (!bits || !out || bits == out || r < 1 || r > VNET_TOOLS_MAX_RADIUS) return VNET_E_BADARG;
    if (int e = volume_count(A, B, C, n)) return e;
    const int W = (C + 63) / 64, tiles_a = ceil_div(A, TA), tiles_b = ceil_div(B, TB);
    const size_t ntiles = (size_t)tiles_a * (size_t)tiles_b * (size_t)W;
    const u64 last_mask = (C & 63) ? ((1ull << (C & 63)) - 1ull) : ~0ull;
    const dim3 grid((unsigned)(ntiles < (size_t)CAP ? ntiles : (size_t)CAP));
    return with_int<1, 2, 3, 4, 5, 6, 7, 8>(r, [&](auto Rc) {
        constexpr int R = decltype(Rc)::value;
        return launch<dilate_bits_kernel<R>>(grid, dim3(PB), dilate_lds_bytes(R), (hipStream_t)stream, reinterpret_cast<const u64*>(bits),
                                             reinterpret_cast<u64*>(out), A, B, W, last_mask, tiles_b, ntiles);
    });
}

int vnet_bits_bbox(const long long* bits, long long* out7, int A, int B, int C, void* stream) {
    size_t n = 0;
    if (!bits || !out7) return VNET_E_BADARG;
    if (int e = volume_count(A, B, C, n)) return e;
    const int W = (C + 63) / 64;
    const size_t words = (size_t)A * (size_t)B * (size_t)W;
    hipStream_t st = (hipStream_t)stream;
    if (int e = launch<bbox_init_kernel>(dim3(1), dim3(64), 0, st, out7, A, B, C)) return e;
    return launch<bits_bbox_kernel>(dim3(blocks_for(words, BBOX_CAP)), dim3(PB), 0, st, reinterpret_cast<const u64*>(bits), out7, B, W, words);
}

int vnet_masked_crop(const void* src, const long long* bits, void* dst, int A, int B, int C, int elem_bytes,
                     int s0, int s1, int s2, int n0, int n1, int n2, void* stream) {
    size_t n = 0, m = 0;
    if (!src || !dst || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) || A < 1 || B < 1 || C < 1 ||
        s0 < 0 || s1 < 0 || s2 < 0 || n0 < 1 || n1 < 1 || n2 < 1 || s0 >= A || s1 >= B || s2 >= C || n0 > A - s0 || n1 > B - s1 || n2 > C - s2)
        return VNET_E_BADARG;
    if (int e = volume_count(A, B, C, n)) return e;
    if (int e = volume_count(n0, n1, n2, m)) return e;
    CropP p{};
    p.src = src; p.bits = reinterpret_cast<const u64*>(bits); p.dst = dst;
    p.B = B; p.C = C; p.W = (C + 63) / 64; p.s0 = s0; p.s1 = s1; p.s2 = s2; p.n1 = n1; p.n2 = n2; p.n = m;
    const dim3 grid(blocks_for(m, CAP));
    hipStream_t st = (hipStream_t)stream;
    switch (elem_bytes) {
        case 1: return launch<masked_crop_kernel<uint8_t>>(grid, dim3(PB), 0, st, p);
        case 2: return launch<masked_crop_kernel<uint16_t>>(grid, dim3(PB), 0, st, p);
        case 4: return launch<masked_crop_kernel<uint32_t>>(grid, dim3(PB), 0, st, p);
        default: return launch<masked_crop_kernel<uint64_t>>(grid, dim3(PB), 0, st, p);
    }
}

int vnet_unpack_bits(const long long* bits, unsigned char* dst_u8, int A, int B, int C, void* stream) {
    size_t n = 0;
    if (!bits || !dst_u8) return VNET_E_BADARG;
    if (int e = volume_count(A, B, C, n)) return e;
    return launch<unpack_bits_kernel>(dim3(blocks_for(n, CAP)), dim3(PB), 0, (hipStream_t)stream, reinterpret_cast<const u64*>(bits), dst_u8,
                                      C, (C + 63) / 64, n);
}

}  // extern "C"
