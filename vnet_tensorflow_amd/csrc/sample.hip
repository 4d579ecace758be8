// sample.hip -- the random tail of the training pipeline on device-resident prepared cases (include/vnet_hip_sample.h; reference
// NiftiDataset3D.py: ConfidenceCrop2 661-793, RandomCrop 458-551, RandomFlip 187-208, RandomNoise 553-572), gfx950.
//   vnet_cc_table     : the representative map of components.hip -> dense rows {representative, count, lo[3], hi[3]} in ascending
//                       representative order: the count / scan / rank / box launches of cc_table.h (shared with score.hip, which adds
//                       the index sums to the box pass), here without the sums.
//   vnet_window_count : grid-stride over a window, wave reduction, one 64-bit atomicAdd pair per wave.
//   vnet_sample_patch : one kernel writes image and label of one sample: gather with per-axis reversal, Philox4x32-10 + Box-Muller noise
//                       keyed by (seed, output element).  Channel quads with 16-byte accesses or one channel (resample.hip's rule),
//                       grid-stride under the same fixed cap, no LDS.
// Voxel indices are int32 (n <= 2^31 - 1, checked on the host); element offsets are 64-bit.
#include <math.h>
#include <limits.h>
#include "common.h"
#include "cc_table.h"
#include "philox_noise.h"          // philox4x32_10, box_muller, sp_noise_quad / sp_noise_one, sp_bad_window (shared with deform_sample.hip)
#include "../../include/vnet_hip_components.h"
#include "../../include/vnet_hip_sample.h"

namespace {

// ---- window count ---------------------------------------------------------------------------------------------------------------
__global__ void window_zero_kernel(u64* out) {
    if (threadIdx.x < 2) out[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(SP_BLOCK) window_count_kernel(const int* __restrict__ label, u64* out, int Y, int Z, int sx, int sy, int sz,
                                                                int wx, int wy, int wz, int lo, int hi) {
    const size_t n = (size_t)wx * wy * wz;
    long long cnt = 0, sum = 0;
    for (size_t idx = (size_t)blockIdx.x * SP_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * SP_BLOCK) {
        size_t v = idx / wz;
        const int z = (int)(idx - v * wz), y = (int)(v % wy), x = (int)(v / wy);
        const int l = label[((size_t)(sx + x) * Y + (sy + y)) * Z + (sz + z)];
        cnt += l >= lo && l <= hi;
        sum += l;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); sum += __shfl_xor(sum, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (cnt) atomicAdd(out, (u64)cnt);
        if (sum) atomicAdd(out + 1, (u64)sum);       // (two's complement: a negative sum adds up all the same)
    }
}

// ---- sample ---------------------------------------------------------------------------------------------------------------------
struct SampleP {
    const float* x; const int* l; float* y; int* yl;
    int Y, Z, C, sx, sy, sz, P0, P1, P2, flip;
    float sigma;
    unsigned k0, k1;
};

// VEC: a unit is 4 consecutive channels of one output voxel, else one channel.  NOISE false: the crop bit for bit.
template <bool VEC, bool NOISE>
__global__ void __launch_bounds__(SP_BLOCK) sample_patch_kernel(SampleP p) {
    const int CU = VEC ? p.C >> 2 : p.C;
    const size_t n = (size_t)p.P0 * p.P1 * p.P2 * CU;
    const float* __restrict__ x = p.x;
    const int* __restrict__ l = p.l;
    float* __restrict__ y = p.y;
    int* __restrict__ yl = p.yl;
    for (size_t idx = (size_t)blockIdx.x * SP_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * SP_BLOCK) {
        size_t v = idx / CU;
        const int cu = (int)(idx - v * CU);
        const size_t ov = v;                                             // output voxel
        const int oz = (int)(v % p.P2); v /= p.P2;
        const int oy = (int)(v % p.P1), ox = (int)(v / p.P1);
        const int ix = p.sx + ((p.flip & 1) ? p.P0 - 1 - ox : ox), iy = p.sy + ((p.flip & 2) ? p.P1 - 1 - oy : oy),
                  iz = p.sz + ((p.flip & 4) ? p.P2 - 1 - oz : oz);
        const size_t iv = ((size_t)ix * p.Y + iy) * p.Z + iz;
        if (cu == 0) yl[ov] = l[iv];
        if constexpr (VEC) {
            float4 f = *reinterpret_cast<const float4*>(x + iv * p.C + (size_t)cu * 4);
            if constexpr (NOISE) f = sp_noise_quad(f, idx, p.sigma, p.k0, p.k1);               // (idx IS the group index q here)
            reinterpret_cast<float4*>(y)[idx] = f;
        } else {
            float f = x[iv * p.C + cu];
            if constexpr (NOISE) f = sp_noise_one(f, idx, p.sigma, p.k0, p.k1);
            y[idx] = f;
        }
    }
}

}  // namespace

extern "C" {

size_t vnet_cc_table_ws_bytes(int X, int Y, int Z) {
    size_t n = 0;
    return sp_count(X, Y, Z, n) ? 0 : cc_table_bytes(n);
}

int vnet_cc_table(const int* label, int* n_out, int* table, int max_components, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream) {
    return cc_table_run<false>(label, n_out, table, nullptr, max_components, X, Y, Z, ws, ws_bytes, stream);
}

int vnet_window_count(const int* label, long long* out, int X, int Y, int Z, int sx, int sy, int sz, int wx, int wy, int wz,
                      int lo, int hi, void* stream) {
    size_t n = 0;
    if (!label || !out || X < 1 || Y < 1 || Z < 1 || sp_bad_window(X, sx, wx) || sp_bad_window(Y, sy, wy) || sp_bad_window(Z, sz, wz))
        return VNET_E_BADARG;
    if (int e = sp_count(X, Y, Z, n)) return e;
    hipStream_t st = (hipStream_t)stream;
    u64* o = reinterpret_cast<u64*>(out);
    if (int e = launch<window_zero_kernel>(dim3(1), dim3(64), 0, st, o)) return e;
    return launch<window_count_kernel>(dim3(sp_blocks((size_t)wx * wy * wz)), dim3(SP_BLOCK), 0, st, label, o, Y, Z, sx, sy, sz, wx, wy, wz, lo, hi);
}

int vnet_sample_patch(const float* image, const int* label, float* out_image, int* out_label, int X, int Y, int Z, int C,
                      int sx, int sy, int sz, int P0, int P1, int P2, int flip, float sigma, unsigned long long seed, void* stream) {
    size_t n = 0;
    if (!image || !label || !out_image || !out_label || C < 1 || X < 1 || Y < 1 || Z < 1 || sp_bad_window(X, sx, P0) ||
        sp_bad_window(Y, sy, P1) || sp_bad_window(Z, sz, P2) || flip < 0 || flip > 7 || !isfinite(sigma) || sigma < 0.f)
        return VNET_E_BADARG;
    if (int e = sp_count(X, Y, Z, n)) return e;
    SampleP p{};
    p.x = image; p.l = label; p.y = out_image; p.yl = out_label;
    p.Y = Y; p.Z = Z; p.C = C; p.sx = sx; p.sy = sy; p.sz = sz; p.P0 = P0; p.P1 = P1; p.P2 = P2; p.flip = flip;
    p.sigma = sigma; p.k0 = (unsigned)(seed & 0xFFFFFFFFull); p.k1 = (unsigned)(seed >> 32);
    const bool vec = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(out_image)) & 15) == 0;
    const size_t units = (size_t)P0 * P1 * P2 * (vec ? C / 4 : C);
    return with_bool(vec, [&](auto V) {
        return with_bool(sigma != 0.f, [&](auto N) {
            return launch<sample_patch_kernel<V, N>>(dim3(sp_blocks(units)), dim3(SP_BLOCK), 0, (hipStream_t)stream, p);
        });
    });
}

}  // extern "C"
