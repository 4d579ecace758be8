// resample.hip -- resampling a volume onto a grid of another voxel spacing (include/vnet_hip_resample.h): the reference's `Resample`
// transform (NiftiDataset3D.py:345-398) and the way back of its evaluate_single_3D (model.py:817-977), fp32 [X,Y,Z,C] / int32 [X,Y,Z]
// on gfx950.  Both are streaming gathers on the pattern of pool.hip: grid-stride under a fixed grid cap, one thread per OUTPUT unit --
// a channel quad with 16-byte accesses (C % 4 == 0, 16-byte aligned bases) or one channel (anything else, misaligned views included) --
// no LDS, 64-bit element offsets.  Coordinates and the 8-tap blend are double (ITK blends a float image in double and rounds once);
// the kernel stays HBM-bound: 3 double multiplies and 7 double lerps per channel against 8 taps of mostly L2-resident reads.
#include <math.h>
#include "common.h"
#include "../../include/vnet_hip_resample.h"

namespace {

constexpr int RS_BLOCK = 256, RS_MAXBLK = 4096;

struct ResampleP {
    const float* x; const float* div; float* y;      // linear
    const int* xi; int* yi;                          // nearest
    int C, X, Y, Z, Xo, Yo, Zo;
    double rx, ry, rz;
};

// one axis of an output index: the two source indices, the weight of the upper one, and the inside test c < n - 0.5
struct RsAxis { int lo, hi; double d; bool in; };

__device__ __forceinline__ RsAxis rs_axis(int i, double r, int n) {
    const double c = (double)i * r, f = floor(c);
    RsAxis a;
    a.in = c < (double)n - 0.5;
    a.lo = a.in ? (int)f : 0;                        // (inside: 0 <= f <= n - 1; outside c may exceed the int range)
    a.hi = a.lo + 1 < n ? a.lo + 1 : n - 1;          // in (n - 1, n - 0.5) the last voxel alone
    a.d = c - f;
    return a;
}

__device__ __forceinline__ double rs_lerp(double lo, double hi, double d) { return lo + d * (hi - lo); }

// output index -> (ox, oy, oz, unit within the voxel); z fastest among the voxels, the unit fastest of all
__device__ __forceinline__ void rs_split(size_t idx, int CU, int Yo, int Zo, int& ox, int& oy, int& oz, int& cu) {
    size_t v = idx / CU; cu = (int)(idx - v * CU);
    oz = (int)(v % Zo); v /= Zo;
    oy = (int)(v % Yo); ox = (int)(v / Yo);
}

// VEC: a unit is 4 consecutive channels of one voxel, else one channel.  DIV: every tap is x / div (0 where div is 0).
template <bool VEC, bool DIV>
__global__ void __launch_bounds__(RS_BLOCK) resample_linear_kernel(ResampleP p) {
    constexpr int W = VEC ? 4 : 1;
    const int CU = VEC ? p.C >> 2 : p.C;
    const size_t n = (size_t)p.Xo * p.Yo * p.Zo * CU;
    const float* __restrict__ x = p.x;
    const float* __restrict__ dv = p.div;
    float* __restrict__ y = p.y;
    for (size_t idx = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * RS_BLOCK) {
        int ox, oy, oz, cu;
        rs_split(idx, CU, p.Yo, p.Zo, ox, oy, oz, cu);
        const RsAxis ax = rs_axis(ox, p.rx, p.X), ay = rs_axis(oy, p.ry, p.Y), az = rs_axis(oz, p.rz, p.Z);
        float r[W];
#pragma unroll
        for (int w = 0; w < W; ++w) r[w] = 0.f;
        if (ax.in && ay.in && az.in) {
            double t[8][W];                                        // tap k = (upper x) * 4 + (upper y) * 2 + (upper z)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const size_t v = ((size_t)((k & 4) ? ax.hi : ax.lo) * p.Y + ((k & 2) ? ay.hi : ay.lo)) * p.Z + ((k & 1) ? az.hi : az.lo);
                const size_t e = v * p.C + (size_t)cu * W;
                float q[W];
                if constexpr (VEC) {
                    const float4 f = *reinterpret_cast<const float4*>(x + e);
                    q[0] = f.x; q[1] = f.y; q[2] = f.z; q[3] = f.w;
                } else {
                    q[0] = x[e];
                }
                if constexpr (DIV) {
                    const double c = (double)dv[v];
#pragma unroll
                    for (int w = 0; w < W; ++w) t[k][w] = c == 0.0 ? 0.0 : (double)q[w] / c;
                } else {
#pragma unroll
                    for (int w = 0; w < W; ++w) t[k][w] = (double)q[w];
                }
            }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const double z00 = rs_lerp(t[0][w], t[1][w], az.d), z01 = rs_lerp(t[2][w], t[3][w], az.d);
                const double z10 = rs_lerp(t[4][w], t[5][w], az.d), z11 = rs_lerp(t[6][w], t[7][w], az.d);
                r[w] = (float)rs_lerp(rs_lerp(z00, z01, ay.d), rs_lerp(z10, z11, ay.d), ax.d);
            }
        }
        if constexpr (VEC) reinterpret_cast<float4*>(y)[idx] = make_float4(r[0], r[1], r[2], r[3]);
        else y[idx] = r[0];
    }
}

__global__ void __launch_bounds__(RS_BLOCK) resample_nearest_i32_kernel(ResampleP p) {
    const size_t n = (size_t)p.Xo * p.Yo * p.Zo;
    const int* __restrict__ x = p.xi;
    int* __restrict__ y = p.yi;
    for (size_t idx = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * RS_BLOCK) {
        int ox, oy, oz, cu;
        rs_split(idx, 1, p.Yo, p.Zo, ox, oy, oz, cu);
        const double cx = (double)ox * p.rx, cy = (double)oy * p.ry, cz = (double)oz * p.rz;
        int r = 0;
        if (cx < (double)p.X - 0.5 && cy < (double)p.Y - 0.5 && cz < (double)p.Z - 0.5) {
            // floor(c + 0.5) <= n - 1 inside; the clamp only covers c + 0.5 rounding up to n in double at the very edge
            const int sx = min((int)floor(cx + 0.5), p.X - 1), sy = min((int)floor(cy + 0.5), p.Y - 1), sz = min((int)floor(cz + 0.5), p.Z - 1);
            r = x[((size_t)sx * p.Y + sy) * p.Z + sz];
        }
        y[idx] = r;
    }
}

inline int rs_blocks(size_t units) {
    size_t b = (units + RS_BLOCK - 1) / RS_BLOCK;
    return (int)(b < 1 ? 1 : b > RS_MAXBLK ? RS_MAXBLK : b);
}

inline bool rs_bad(int X, int Y, int Z, int Xo, int Yo, int Zo, double rx, double ry, double rz) {
    return X < 1 || Y < 1 || Z < 1 || Xo < 1 || Yo < 1 || Zo < 1 || !isfinite(rx) || !isfinite(ry) || !isfinite(rz) ||
           !(rx > 0.0) || !(ry > 0.0) || !(rz > 0.0);
}

}  // namespace

extern "C" {

int vnet_resample_linear(const float* x, const float* div, float* y, int C, int X, int Y, int Z, int Xo, int Yo, int Zo,
                         double rx, double ry, double rz, void* stream) {
    if (!x || !y || C < 1 || rs_bad(X, Y, Z, Xo, Yo, Zo, rx, ry, rz)) return VNET_E_BADARG;
    ResampleP p{};
    p.x = x; p.div = div; p.y = y; p.C = C; p.X = X; p.Y = Y; p.Z = Z; p.Xo = Xo; p.Yo = Yo; p.Zo = Zo; p.rx = rx; p.ry = ry; p.rz = rz;
    const bool vec = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    const size_t units = (size_t)Xo * Yo * Zo * (vec ? C / 4 : C);
    return with_bool(vec, [&](auto V) {
        return with_bool(div != nullptr, [&](auto D) {
            return launch<resample_linear_kernel<V, D>>(dim3(rs_blocks(units)), dim3(RS_BLOCK), 0, (hipStream_t)stream, p);
        });
    });
}

int vnet_resample_nearest_i32(const int* x, int* y, int X, int Y, int Z, int Xo, int Yo, int Zo, double rx, double ry, double rz,
                              void* stream) {
    if (!x || !y || rs_bad(X, Y, Z, Xo, Yo, Zo, rx, ry, rz)) return VNET_E_BADARG;
    ResampleP p{};
    p.xi = x; p.yi = y; p.C = 1; p.X = X; p.Y = Y; p.Z = Z; p.Xo = Xo; p.Yo = Yo; p.Zo = Zo; p.rx = rx; p.ry = ry; p.rz = rz;
    return launch<resample_nearest_i32_kernel>(dim3(rs_blocks((size_t)Xo * Yo * Zo)), dim3(RS_BLOCK), 0, (hipStream_t)stream, p);
}

}  // extern "C"
