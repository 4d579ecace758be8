// summary.hip -- the image summaries of a step as uint8 slices (include/vnet_hip_summary.h; reference model.py:326-334, 459-463,
// 579-585: tf.cast / grayscale_to_rainbow, then tf.transpose(t[b:b+1, :, :, :, c], [3,1,2,0])), gfx950.
//   One kernel template, four element rules.  For a fixed (b, x) the source is a matrix [y][z * C + c] with (z, c) fastest and the
//   output a matrix [(c, z)][y] with y fastest: a transpose.  A workgroup stages a 64 (y) x 64 (z, c) tile through LDS: it reads rows
//   contiguous in (z, c) -- 64 lanes on 64 consecutive elements --, converts each element to its output word on the way in (a byte, or
//   R | G << 8 | B << 16), and writes rows contiguous in y.  The LDS row pitch is 65 words: the lanes of a half-wave, which hold 32
//   consecutive columns on the way in and 32 consecutive rows on the way out, fall on 32 different banks both times.
//   Tiles are numbered (b * X + x, y tile, zc tile) and dealt to at most VNET_SUMMARY_MAX_BLOCKS workgroups in a loop over the grid.
// HBM-bound; element counts fit an int32 (checked on the host), tile numbers and element offsets are 64-bit.  No scratch, no atomics.
// Every fp32 operation of the rainbow rule is rounded once: contraction is off for this translation unit (a fused 6 * H - 3 changes
// output bytes; the `==` tier of tests/test_hip_summary.py rests on it).
#include <limits.h>
#include "common.h"
#include "../../include/vnet_hip_summary.h"

#pragma clang fp contract(off)

namespace {

constexpr int SB = 256, TY = 64, TZ = 64, PITCH = TZ + 1, ROWS = SB / 64, TRIPS = TY / ROWS;

typedef long long i64;

enum { RULE_F32 = 0, RULE_I32 = 1, RULE_I64 = 2, RULE_RAINBOW = 3 };

struct SliceP {
    const void* src;
    unsigned char* dst;
    i64 tiles;      // B * X * ty_n * tz_n
    i64 ZC;         // Z * C
    int ty_n, tz_n;
    int X, Y, Z, C;
    unsigned factor;
};

// tf.cast(float -> uint8) on its defined range, saturating outside of it, NaN -> 0
__device__ __forceinline__ unsigned byte_of(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    return (unsigned)v;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// grayscale_to_rainbow + tf.image.hsv_to_rgb (S = V = 1) + tf.cast(. * 255, uint8), operation by operation
__device__ __forceinline__ unsigned rainbow_of(float p) {
    const float one_minus = 1.0f - p;
    const float twice = one_minus * 2.0f;
    const float H = twice / 3.0f;
    const float dh = H * 6.0f;
    const float r = clamp01(fabsf(dh - 3.0f) - 1.0f);
    const float g = clamp01(2.0f - fabsf(dh - 2.0f));
    const float b = clamp01(2.0f - fabsf(dh - 4.0f));
    return byte_of(r * 255.0f) | (byte_of(g * 255.0f) << 8) | (byte_of(b * 255.0f) << 16);
}

template <int RULE>
__device__ __forceinline__ unsigned word_of(const void* src, size_t i, unsigned factor) {
    if constexpr (RULE == RULE_F32) return byte_of(static_cast<const float*>(src)[i]);
    else if constexpr (RULE == RULE_I32) return ((unsigned)static_cast<const int*>(src)[i] * factor) & 255u;
    else if constexpr (RULE == RULE_I64) return ((unsigned)(unsigned long long)static_cast<const i64*>(src)[i] * factor) & 255u;
    else return rainbow_of(static_cast<const float*>(src)[i]);
}

template <int RULE>
__global__ void __launch_bounds__(SB) slices_kernel(SliceP p) {
    __shared__ unsigned tile[TY * PITCH];
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    for (i64 t = blockIdx.x; t < p.tiles; t += gridDim.x) {
        const int tz = (int)(t % p.tz_n);
        const i64 rest = t / p.tz_n;
        const int ty = (int)(rest % p.ty_n);
        const i64 bx = rest / p.ty_n;                      // b * X + x
        const int y0 = ty * TY;
        const i64 zc0 = (i64)tz * TZ;
        // in: lane lo reads column zc0 + lo of rows y0 + hi, + ROWS, ...
        {
            const i64 zc = zc0 + lo;
            const bool col = zc < p.ZC;
#pragma unroll
            for (int k = 0; k < TRIPS; ++k) {
                const int yl = hi + ROWS * k, y = y0 + yl;
                if (col && y < p.Y)
                    tile[yl * PITCH + lo] = word_of<RULE>(p.src, (size_t)((bx * p.Y + y) * p.ZC + zc), p.factor);
            }
        }
        __syncthreads();
        // out: lane lo writes pixel y0 + lo of the planes zc0 + hi, + ROWS, ...
        {
            const int y = y0 + lo;
            const i64 b = bx / p.X;
            const int x = (int)(bx % p.X);
            if (y < p.Y) {
#pragma unroll
                for (int k = 0; k < TRIPS; ++k) {
                    const int zl = hi + ROWS * k;
                    const i64 zc = zc0 + zl;
                    if (zc < p.ZC) {
                        const int z = (int)(zc / p.C), c = (int)(zc % p.C);
                        const unsigned w = tile[lo * PITCH + zl];
                        const size_t o = (size_t)((((b * p.C + c) * p.Z + z) * p.X + x) * p.Y + y);
                        if constexpr (RULE == RULE_RAINBOW) {
                            p.dst[3 * o] = (unsigned char)w;
                            p.dst[3 * o + 1] = (unsigned char)(w >> 8);
                            p.dst[3 * o + 2] = (unsigned char)(w >> 16);
                        } else {
                            p.dst[o] = (unsigned char)w;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <int RULE>
int run(const void* src, unsigned char* dst, int factor, int B, int X, int Y, int Z, int C, void* stream) {
    if (!src || !dst || B < 1 || X < 1 || Y < 1 || Z < 1 || C < 1) return VNET_E_BADARG;
    i64 n = 1;
    for (int e : {B, X, Y, Z, C}) {
        if (n > (i64)INT_MAX / e) return VNET_E_UNSUPPORTED;
        n *= e;
    }
    SliceP p;
    p.src = src; p.dst = dst;
    p.ZC = (i64)Z * C;
    p.ty_n = (Y + TY - 1) / TY;
    p.tz_n = (int)((p.ZC + TZ - 1) / TZ);
    p.tiles = (i64)B * X * p.ty_n * p.tz_n;
    p.X = X; p.Y = Y; p.Z = Z; p.C = C;
    p.factor = (unsigned)factor;
    const int grid = (int)(p.tiles < VNET_SUMMARY_MAX_BLOCKS ? p.tiles : VNET_SUMMARY_MAX_BLOCKS);
    return launch<slices_kernel<RULE>>(dim3(grid), dim3(SB), 0, (hipStream_t)stream, p);
}

}  // namespace

extern "C" {

int vnet_summary_slices_f32(const float* src, unsigned char* dst, int B, int X, int Y, int Z, int C, void* stream) {
    return run<RULE_F32>(src, dst, 0, B, X, Y, Z, C, stream);
}

int vnet_summary_slices_i32(const int* src, unsigned char* dst, int factor, int B, int X, int Y, int Z, int C, void* stream) {
    return run<RULE_I32>(src, dst, factor, B, X, Y, Z, C, stream);
}

int vnet_summary_slices_i64(const long long* src, unsigned char* dst, int factor, int B, int X, int Y, int Z, int C, void* stream) {
    return run<RULE_I64>(src, dst, factor, B, X, Y, Z, C, stream);
}

int vnet_summary_rainbow_f32(const float* src, unsigned char* dst, int B, int X, int Y, int Z, int K, void* stream) {
    return run<RULE_RAINBOW>(src, dst, 0, B, X, Y, Z, K, stream);
}

}  // extern "C"
