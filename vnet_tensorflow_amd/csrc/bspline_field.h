// bspline_field.h -- the device arithmetic of the free-form deformation (include/vnet_hip_deform.h), shared by deform.hip (a whole volume)
// and deform_sample.hip (the window of one training sample): one axis of a voxel on the control grid, the two phases of the separable
// displacement (the 13 partial sums of a z-row over the x and y control indices; their contraction along z at a voxel), one axis of the
// source position, and the 8-tap blend.  Both units produce the same bits for the same voxel because they run these functions, in this
// order, without FMA contraction: the pragma below holds for everything after this header in the including unit as well.
#pragma once
#include <math.h>
#include "common.h"
#include "../../include/vnet_hip_deform.h"

// equal neighbours must give exactly their value, and the weights must be those of the NumPy restatement bit for bit: no FMA contraction
#pragma clang fp contract(off)

namespace {

constexpr int G = VNET_BSPLINE_GRID, G3 = G * G * G;

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

// phase 1: S[a][k] of the z-row at (ax, ay) = sum_j wy_j sum_i wx_i coef_a[k][j][i]; 0 off the valid region
__device__ __forceinline__ double bs_row_sum(const double* __restrict__ coef, int a, int k, const BsAxis& ax, const BsAxis& ay) {
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
    return acc;
}

// phase 2: d_a = sum_k wz_k S[a][m_z + k] from the row's partial sums S[3][G]; 0 off the valid region
__device__ __forceinline__ void bs_displacement(const double (*S)[G], const BsAxis& az, double d[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += az.w[k] * S[a][az.m + k];
        d[a] = az.ok ? s : 0.0;
    }
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

// the 8 taps of one channel, tap k = (upper x) * 4 + (upper y) * 2 + (upper z): along z, then y, then x
__device__ __forceinline__ double df_blend(double t0, double t1, double t2, double t3, double t4, double t5, double t6, double t7,
                                           double dx, double dy, double dz) {
    const double z00 = df_lerp(t0, t1, dz), z01 = df_lerp(t2, t3, dz);
    const double z10 = df_lerp(t4, t5, dz), z11 = df_lerp(t6, t7, dz);
    return df_lerp(df_lerp(z00, z01, dy), df_lerp(z10, z11, dy), dx);
}

__device__ __forceinline__ float df_out(double v, float) { return (float)v; }
__device__ __forceinline__ int df_out(double v, int) {          // static_cast<int> after clamping: truncation toward zero
    return v <= -2147483648.0 ? (int)0x80000000 : v >= 2147483647.0 ? 0x7fffffff : (int)v;
}

// 0, VNET_E_BADARG (a size or C < 1, a spacing that is not finite or not > 0) or VNET_E_UNSUPPORTED (an int32 cannot index the voxels)
inline int df_check_grid(int X, int Y, int Z, int C, double sx, double sy, double sz) {
    if (X < 1 || Y < 1 || Z < 1 || C < 1 || !isfinite(sx) || !isfinite(sy) || !isfinite(sz) || !(sx > 0.0) || !(sy > 0.0) || !(sz > 0.0))
        return VNET_E_BADARG;
    const unsigned long long xy = (unsigned long long)X * (unsigned long long)Y;
    if (xy > 0x7fffffffull || xy * (unsigned long long)Z > 0x7fffffffull) return VNET_E_UNSUPPORTED;      // int32 voxel index
    return 0;
}

}  // namespace
