// deform_sample.hip -- one training sample cut from a device-resident case through the free-form deformation
// (include/vnet_hip_deform_sample.h), fp32 [X,Y,Z,C] -> [P0,P1,P2,C] on gfx950: bspline_deform_kernel (deform.hip) restricted to the voxels
// of the window, with the flip and the noise of sample_patch_kernel (sample.hip) on the way out.  Deforming the whole image to keep one
// patch of it costs a store and a re-read of X*Y*Z*C floats per sample; here the deformed image is never formed.
// The structure is that of deform.hip: a workgroup takes a chunk of whole z-rows OF THE PATCH and works in two phases,
//   1. per row and displacement component the 13 partial sums over the x and y control indices (39 doubles per row) into LDS;
//   2. one thread per voxel: the contraction along z (12 LDS reads), the 8-tap gather from the resident image for every channel of the
//      voxel (the displacement is shared by its channels), the noise of the OUTPUT element, the store at the flipped index.
// The control grid, the valid region and the inside test are those of the volume; the window only chooses which voxels are evaluated.
// The arithmetic is that of the two units, by inclusion: bspline_field.h (no FMA contraction) and philox_noise.h.
// Grid-stride over the chunks under the fixed grid cap, int32 voxel indices (checked on the host), 64-bit element offsets.
#include <math.h>
#include "common.h"
#include "philox_noise.h"
#include "bspline_field.h"
#include "../../include/vnet_hip_deform_sample.h"

#pragma clang fp contract(off)

namespace {

constexpr int DS_BLOCK = 256, DS_MAXBLK = 4096;      // (the block and the grid cap of deform.hip)
constexpr int DS_ROWS = 8, DS_CHUNK = 1024;          // a chunk: clamp(DS_CHUNK / P2, 1, DS_ROWS) z-rows of the patch

struct DeformSampleP {
    const float* x; const int* l; const double* coef; float* y; int* yl;
    int X, Y, Z, C, rows;
    int sx, sy, sz, P0, P1, P2, flip;
    double s0, s1, s2;
    float sigma;
    unsigned k0, k1;
};

// The noise of philox_noise.h behind a call.  Inlined into phase 2 its scalar constants (the argument reduction of sinf / cosf) are hoisted
// over the three loops on top of the kernel's own scalars, and 16 SGPRs end up parked in VGPR lanes; called, they live in the callee
// alone: no SGPR spill, and 126 VGPRs for quads with noise where inlining took 147.  The arithmetic is the same code either way.
__device__ __attribute__((noinline)) float4 ds_noise_quad(float4 f, unsigned long long q, float sigma, unsigned k0, unsigned k1) {
    return sp_noise_quad(f, q, sigma, k0, k1);
}
__device__ __attribute__((noinline)) float ds_noise_one(float f, unsigned long long e, float sigma, unsigned k0, unsigned k1) {
    return sp_noise_one(f, e, sigma, k0, k1);
}

// VEC: the channels of a voxel go in quads, else one by one.  NOISE false: the deformed window bit for bit.
template <bool VEC, bool NOISE>
__global__ void __launch_bounds__(DS_BLOCK) deform_sample_kernel(DeformSampleP p) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ double S[DS_ROWS][3][G];
    const float* __restrict__ x = p.x;
    const int* __restrict__ l = p.l;
    float* __restrict__ y = p.y;
    int* __restrict__ yl = p.yl;
    const double* __restrict__ coef = p.coef;
    const int CU = VEC ? p.C >> 2 : p.C;
    const int NR = p.P0 * p.P1, nchunks = NR / p.rows + (NR % p.rows != 0);
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {          // (the trip count is the same for every thread of the block)
        const int row0 = ch * p.rows, nrows = min(p.rows, NR - row0);
        for (int it = threadIdx.x; it < nrows * 3 * G; it += DS_BLOCK) {
            const int r = it / (3 * G), q = it - r * (3 * G), a = q / G, k = q - a * G;
            const int row = row0 + r, px = row / p.P1, py = row - px * p.P1;
            const BsAxis ax = bs_axis(p.sx + px, p.s0, p.X), ay = bs_axis(p.sy + py, p.s1, p.Y);
            S[r][a][k] = bs_row_sum(coef, a, k, ax, ay);
        }
        __syncthreads();
        for (int v = threadIdx.x; v < nrows * p.P2; v += DS_BLOCK) {
            const int r = v / p.P2, pz = v - r * p.P2;
            const int row = row0 + r, px = row / p.P1, py = row - px * p.P1;
            const int ix = p.sx + px, iy = p.sy + py, iz = p.sz + pz;   // the voxel of the volume this thread deforms
            const BsAxis az = bs_axis(iz, p.s2, p.Z);
            double d[3];
            bs_displacement(S[r], az, d);
            const DfAxis sx = df_axis((double)ix + d[0] / p.s0, p.X), sy = df_axis((double)iy + d[1] / p.s1, p.Y),
                         sz = df_axis((double)iz + d[2] / p.s2, p.Z);
            const bool in = sx.in && sy.in && sz.in;
            // where it goes: axis a reversed within the patch
            const int ox = (p.flip & 1) ? p.P0 - 1 - px : px, oy = (p.flip & 2) ? p.P1 - 1 - py : py, oz = (p.flip & 4) ? p.P2 - 1 - pz : pz;
            const size_t ov = ((size_t)ox * p.P1 + oy) * p.P2 + oz;
            yl[ov] = l[((size_t)ix * p.Y + iy) * p.Z + iz];
            size_t tap[8];                                               // tap k = (upper x) * 4 + (upper y) * 2 + (upper z)
#pragma unroll
            for (int k = 0; k < 8; ++k)
                tap[k] = in ? (((size_t)((k & 4) ? sx.hi : sx.lo) * p.Y + ((k & 2) ? sy.hi : sy.lo)) * p.Z + ((k & 1) ? sz.hi : sz.lo)) * p.C : 0;
            for (int cu = 0; cu < CU; ++cu) {
                float res[W];
#pragma unroll
                for (int w = 0; w < W; ++w) res[w] = 0.f;
                if (in) {
                    double t[8][W];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const size_t e = tap[k] + (size_t)cu * W;
                        if constexpr (VEC) {
                            const float4 f = *reinterpret_cast<const float4*>(x + e);
                            t[k][0] = f.x; t[k][1] = f.y; t[k][2] = f.z; t[k][3] = f.w;
                        } else {
                            t[k][0] = (double)x[e];
                        }
                    }
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        res[w] = df_out(df_blend(t[0][w], t[1][w], t[2][w], t[3][w], t[4][w], t[5][w], t[6][w], t[7][w], sx.d, sy.d, sz.d), float());
                }
                const size_t unit = ov * CU + cu;                        // VEC: the noise group q of the output; else its element
                if constexpr (VEC) {
                    float4 f = make_float4(res[0], res[1], res[2], res[3]);
                    if constexpr (NOISE) f = ds_noise_quad(f, unit, p.sigma, p.k0, p.k1);
                    reinterpret_cast<float4*>(y)[unit] = f;
                } else {
                    float f = res[0];
                    if constexpr (NOISE) f = ds_noise_one(f, unit, p.sigma, p.k0, p.k1);
                    y[unit] = f;
                }
            }
        }
        __syncthreads();                                                 // S is rewritten by the next chunk
    }
}

}  // namespace

extern "C" {

int vnet_deform_sample_patch(const float* image, const int* deformed_label, const double* coef, float* out_image, int* out_label,
                             int X, int Y, int Z, int C, double s0, double s1, double s2, int sx, int sy, int sz, int P0, int P1, int P2,
                             int flip, float sigma, unsigned long long seed, void* stream) {
    if (!image || !deformed_label || !coef || !out_image || !out_label || X < 1 || Y < 1 || Z < 1 || sp_bad_window(X, sx, P0) ||
        sp_bad_window(Y, sy, P1) || sp_bad_window(Z, sz, P2) || flip < 0 || flip > 7 || !isfinite(sigma) || sigma < 0.f)
        return VNET_E_BADARG;
    if (int e = df_check_grid(X, Y, Z, C, s0, s1, s2)) return e;         // (C, the spacing: BADARG; then the int32 voxel index)
    DeformSampleP p{};
    p.x = image; p.l = deformed_label; p.coef = coef; p.y = out_image; p.yl = out_label;
    p.X = X; p.Y = Y; p.Z = Z; p.C = C; p.sx = sx; p.sy = sy; p.sz = sz; p.P0 = P0; p.P1 = P1; p.P2 = P2; p.flip = flip;
    p.s0 = s0; p.s1 = s1; p.s2 = s2;
    p.sigma = sigma; p.k0 = (unsigned)(seed & 0xFFFFFFFFull); p.k1 = (unsigned)(seed >> 32);
    p.rows = DS_CHUNK / P2 < 1 ? 1 : DS_CHUNK / P2 > DS_ROWS ? DS_ROWS : DS_CHUNK / P2;
    const int NR = P0 * P1, nchunks = NR / p.rows + (NR % p.rows != 0);  // (P0 * P1 <= X * Y: an int32)
    const dim3 grid(nchunks > DS_MAXBLK ? DS_MAXBLK : nchunks);
    const bool vec = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(out_image)) & 15) == 0;
    return with_bool(vec, [&](auto V) {
        return with_bool(sigma != 0.f, [&](auto N) {
            return launch<deform_sample_kernel<V, N>>(grid, dim3(DS_BLOCK), 0, (hipStream_t)stream, p);
        });
    });
}

}  // extern "C"
