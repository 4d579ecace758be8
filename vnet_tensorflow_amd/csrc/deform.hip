// deform.hip -- free-form deformation of a volume by a cubic B-spline displacement field (include/vnet_hip_deform.h): the reference's
// `BSplineDeformation` augmentation (NiftiDataset3D.py:795-832), fp32 [X,Y,Z,C] / int32 [X,Y,Z] on gfx950.  A streaming gather on the
// pattern of resample.hip (grid-stride under the same fixed grid cap, 64-bit element offsets, fp64 coordinates and blend, the same tap
// rules, a channel quad with 16-byte accesses when C % 4 == 0 and both bases are 16-byte aligned, else one channel at a time), with the
// displacement field in front of it.  Evaluated naively the field is 64 control points x 3 components per voxel, 192 fp64 loads that
// dwarf the 8 taps; it is separable, so a workgroup takes a chunk of whole z-rows and works in two phases:
//   1. per row (x, y fixed) and component, the 13 partial sums over the x and y control indices, S[a][k] = sum_j wy_j sum_i wx_i coef_a[k][j][i]
//      (39 doubles per row, 16 coefficient reads each), into LDS;
//   2. one thread per voxel: d_a = sum_k wz_k S[a][m_z + k] (12 LDS reads), then the 8-tap gather for every channel of the voxel -- the
//      displacement is computed once per voxel and shared by its channels.
// The 52 KB coefficient table is read through L2 (a chunk touches 16 * 39 entries of it per row, neighbouring rows the same ones); what
// is staged in LDS is the 312-byte row state, not the table: a full copy per workgroup would cost 52 KB of LDS and of L2 traffic for
// every 1024 voxels and cap the occupancy at three workgroups per CU.
#include <math.h>
#include "common.h"
#include "bspline_field.h"        // bs_axis, bs_row_sum, bs_displacement, df_axis, df_blend, df_out (shared with deform_sample.hip)
#include "../../include/vnet_hip_deform.h"

// equal neighbours must give exactly their value, and the weights must be those of the NumPy restatement bit for bit: no FMA contraction
#pragma clang fp contract(off)

namespace {

constexpr int DF_BLOCK = 256, DF_MAXBLK = 4096;      // (the block and the grid cap of resample.hip and pool.hip)
constexpr int DF_ROWS = 8, DF_CHUNK = 1024;          // a chunk: clamp(DF_CHUNK / Z, 1, DF_ROWS) z-rows

struct DeformP {
    const void* x; void* y; const double* coef;
    int X, Y, Z, C, rows;
    double sx, sy, sz;
};

// T: float (image) or int (label map, C = 1).  VEC: the channels of a voxel go in quads, else one by one.
template <typename T, bool VEC>
__global__ void __launch_bounds__(DF_BLOCK) bspline_deform_kernel(DeformP p) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ double S[DF_ROWS][3][G];
    const T* __restrict__ x = static_cast<const T*>(p.x);
    T* __restrict__ y = static_cast<T*>(p.y);
    const double* __restrict__ coef = p.coef;
    const int CU = VEC ? p.C >> 2 : p.C;
    const int NR = p.X * p.Y, nchunks = NR / p.rows + (NR % p.rows != 0);
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {          // (the trip count is the same for every thread of the block)
        const int row0 = ch * p.rows, nrows = min(p.rows, NR - row0);
        for (int it = threadIdx.x; it < nrows * 3 * G; it += DF_BLOCK) {
            const int r = it / (3 * G), q = it - r * (3 * G), a = q / G, k = q - a * G;
            const int row = row0 + r, ix = row / p.Y, iy = row - ix * p.Y;
            const BsAxis ax = bs_axis(ix, p.sx, p.X), ay = bs_axis(iy, p.sy, p.Y);
            S[r][a][k] = bs_row_sum(coef, a, k, ax, ay);
        }
        __syncthreads();
        for (int v = threadIdx.x; v < nrows * p.Z; v += DF_BLOCK) {
            const int r = v / p.Z, iz = v - r * p.Z;
            const int row = row0 + r, ix = row / p.Y, iy = row - ix * p.Y;
            const BsAxis az = bs_axis(iz, p.sz, p.Z);
            double d[3];
            bs_displacement(S[r], az, d);
            const DfAxis sx = df_axis((double)ix + d[0] / p.sx, p.X), sy = df_axis((double)iy + d[1] / p.sy, p.Y),
                         sz = df_axis((double)iz + d[2] / p.sz, p.Z);
            const bool in = sx.in && sy.in && sz.in;
            const size_t out = ((size_t)row * p.Z + iz) * p.C;
            size_t tap[8];                                               // tap k = (upper x) * 4 + (upper y) * 2 + (upper z)
#pragma unroll
            for (int k = 0; k < 8; ++k)
                tap[k] = in ? (((size_t)((k & 4) ? sx.hi : sx.lo) * p.Y + ((k & 2) ? sy.hi : sy.lo)) * p.Z + ((k & 1) ? sz.hi : sz.lo)) * p.C : 0;
            for (int cu = 0; cu < CU; ++cu) {
                T res[W];
#pragma unroll
                for (int w = 0; w < W; ++w) res[w] = T(0);
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
                    for (int w = 0; w < W; ++w) {
                        res[w] = df_out(df_blend(t[0][w], t[1][w], t[2][w], t[3][w], t[4][w], t[5][w], t[6][w], t[7][w], sx.d, sy.d, sz.d), T());
                    }
                }
                if constexpr (VEC) *reinterpret_cast<float4*>(y + out + (size_t)cu * 4) = make_float4(res[0], res[1], res[2], res[3]);
                else y[out + cu] = res[0];
            }
        }
        __syncthreads();                                                 // S is rewritten by the next chunk
    }
}

inline int df_check(const void* x, const void* y, const double* coef, int X, int Y, int Z, int C, double sx, double sy, double sz) {
    if (!x || !y || !coef) return VNET_E_BADARG;
    return df_check_grid(X, Y, Z, C, sx, sy, sz);
}

template <typename T>
int df_launch(const T* x, T* y, int X, int Y, int Z, int C, const double* coef, double sx, double sy, double sz, bool vec, void* stream) {
    DeformP p{};
    p.x = x; p.y = y; p.coef = coef; p.X = X; p.Y = Y; p.Z = Z; p.C = C; p.sx = sx; p.sy = sy; p.sz = sz;
    p.rows = DF_CHUNK / Z < 1 ? 1 : DF_CHUNK / Z > DF_ROWS ? DF_ROWS : DF_CHUNK / Z;
    const int nchunks = X * Y / p.rows + (X * Y % p.rows != 0);
    const dim3 grid(nchunks > DF_MAXBLK ? DF_MAXBLK : nchunks);
    if constexpr (std::is_same<T, float>::value) {
        return with_bool(vec, [&](auto V) {
            return launch<bspline_deform_kernel<float, V>>(grid, dim3(DF_BLOCK), 0, (hipStream_t)stream, p);
        });
    } else {
        return launch<bspline_deform_kernel<int, false>>(grid, dim3(DF_BLOCK), 0, (hipStream_t)stream, p);
    }
}

}  // namespace

extern "C" {

int vnet_bspline_deform_f32(const float* x, float* y, int X, int Y, int Z, int C, const double* coef, double sx, double sy, double sz,
                            void* stream) {
    if (int e = df_check(x, y, coef, X, Y, Z, C, sx, sy, sz)) return e;
    const bool vec = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    return df_launch<float>(x, y, X, Y, Z, C, coef, sx, sy, sz, vec, stream);
}

int vnet_bspline_deform_i32(const int* x, int* y, int X, int Y, int Z, int C, const double* coef, double sx, double sy, double sz,
                            void* stream) {
    if (int e = df_check(x, y, coef, X, Y, Z, C, sx, sy, sz)) return e;
    if (C != 1) return VNET_E_BADARG;
    return df_launch<int>(x, y, X, Y, Z, 1, coef, sx, sy, sz, false, stream);
}

}  // extern "C"
