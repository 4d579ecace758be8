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
#include "../../include/vnet_hip_deform.h"

// equal neighbours must give exactly their value, and the weights must be those of the NumPy restatement bit for bit: no FMA contraction
#pragma clang fp contract(off)

namespace {

constexpr int DF_BLOCK = 256, DF_MAXBLK = 4096;      // (the block and the grid cap of resample.hip and pool.hip)
constexpr int DF_ROWS = 8, DF_CHUNK = 1024;          // a chunk: clamp(DF_CHUNK / Z, 1, DF_ROWS) z-rows
constexpr int G = VNET_BSPLINE_GRID, G3 = G * G * G;

struct DeformP {
    const void* x; void* y; const double* coef;
    int X, Y, Z, C, rows;
    double sx, sy, sz;
};

// one axis of a voxel on the control grid: first control index of the cubic support, the four weights, the valid-region test
struct BsAxis { int m; double w[4]; bool ok; };

__device__ __forceinline__ BsAxis bs_axis(int i, double s, int n) {
    const double D = (double)n * s / 10.0, u = ((double)i * s) / D, f = floor(u);
    BsAxis a;
    a.ok = u >= 0.0 && u < 10.0;                     // ITK: 1 <= u + 1 < 11 (true for every voxel centre)
    a.m = a.ok ? min((int)f, 9) : 0;                 // taps m .. m + 3 stay inside 0 .. 12
    const double t = u - f, t2 = t * t, t3 = t2 * t, o = 1.0 - t;
    a.w[0] = o * o * o / 6.0;
    a.w[1] = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
    a.w[2] = (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0;
    a.w[3] = t3 / 6.0;
    return a;
}

// one axis of the source position: the two neighbours, the weight of the upper one, the inside test -0.5 <= c < n - 0.5
struct DfAxis { int lo, hi; double d; bool in; };

__device__ __forceinline__ DfAxis df_axis(double c, int n) {
    const double f = floor(c);
    DfAxis a;
    a.in = c >= -0.5 && c < (double)n - 0.5;         // (false for a NaN)
    const int b = a.in ? (int)f : 0;                 // inside: -1 <= f <= n - 1; outside c may exceed the int range
    a.lo = b > 0 ? b : 0;
    a.hi = b + 1 < n ? b + 1 : n - 1;
    a.d = c - f;
    return a;
}

__device__ __forceinline__ double df_lerp(double lo, double hi, double d) { return lo + d * (hi - lo); }

__device__ __forceinline__ float df_out(double v, float) { return (float)v; }
__device__ __forceinline__ int df_out(double v, int) {          // static_cast<int> after clamping: truncation toward zero
    return v <= -2147483648.0 ? (int)0x80000000 : v >= 2147483647.0 ? 0x7fffffff : (int)v;
}

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
            double acc = 0.0;
            if (ax.ok && ay.ok) {
                const double* c = coef + a * G3 + (k * G + ay.m) * G + ax.m;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) s += ax.w[i] * c[j * G + i];
                    acc += ay.w[j] * s;
                }
            }
            S[r][a][k] = acc;
        }
        __syncthreads();
        for (int v = threadIdx.x; v < nrows * p.Z; v += DF_BLOCK) {
            const int r = v / p.Z, iz = v - r * p.Z;
            const int row = row0 + r, ix = row / p.Y, iy = row - ix * p.Y;
            const BsAxis az = bs_axis(iz, p.sz, p.Z);
            double d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += az.w[k] * S[r][a][az.m + k];
                d[a] = az.ok ? s : 0.0;
            }
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
                        const double z00 = df_lerp(t[0][w], t[1][w], sz.d), z01 = df_lerp(t[2][w], t[3][w], sz.d);
                        const double z10 = df_lerp(t[4][w], t[5][w], sz.d), z11 = df_lerp(t[6][w], t[7][w], sz.d);
                        res[w] = df_out(df_lerp(df_lerp(z00, z01, sy.d), df_lerp(z10, z11, sy.d), sx.d), T());
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
    if (!x || !y || !coef || X < 1 || Y < 1 || Z < 1 || C < 1 || !isfinite(sx) || !isfinite(sy) || !isfinite(sz) ||
        !(sx > 0.0) || !(sy > 0.0) || !(sz > 0.0)) return VNET_E_BADARG;
    const unsigned long long xy = (unsigned long long)X * (unsigned long long)Y;
    if (xy > 0x7fffffffull || xy * (unsigned long long)Z > 0x7fffffffull) return VNET_E_UNSUPPORTED;      // int32 voxel index
    return 0;
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
