// pool.hip -- 2x2x2 stride-2 VALID max-pooling of the reference's U-Net (tf.nn.max_pool3d, networks.py:120) and its gradient, fp32 NDHWC
// on gfx950.  Both are HBM-bound streams on the pattern of bn_act_fwd_kernel (elementwise.hip): grid-stride, one thread per channel
// quad with 16-byte accesses (C % 4 == 0) or per channel (any C), no LDS.
//   forward : one thread per OUTPUT unit reads its 8 fine units (1.125 floats moved per fine element);
//   backward: one thread per FINE unit -- so every element of dx is written exactly once, the zeros of the losers and of the trailing
//             plane / row / column VALID drops included -- re-reads its window's 8 fine units (L2 hits: the 8 threads of a window run
//             in neighbouring waves) and takes the gradient when it is the FIRST voxel equal to the maximum in (dz, dy, dx) order.
#include "common.h"
#include "../../include/vnet_hip_unet.h"

namespace {

constexpr int POOL_BLOCK = 256, POOL_MAXBLK = 4096;

struct PoolP {
    const float* x; const float* y; const float* dy; float* out;
    int C, B, Df, Hf, Wf, Dc, Hc, Wc, accum;
};

template <bool VEC> struct PoolUnit { using T = float; };
template <> struct PoolUnit<true> { using T = float4; };

__device__ __forceinline__ float pmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float4 pmax(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }

// VEC: a unit is 4 consecutive channels of one voxel (C % 4 == 0, 16-byte aligned tensors), else one channel
template <bool VEC>
__global__ void __launch_bounds__(POOL_BLOCK) maxpool2_fwd_kernel(PoolP p) {
    using U = typename PoolUnit<VEC>::T;
    const int CU = VEC ? p.C >> 2 : p.C;
    const size_t n = (size_t)p.B * p.Dc * p.Hc * p.Wc * CU;
    const U* __restrict__ x = reinterpret_cast<const U*>(p.x);
    U* __restrict__ y = reinterpret_cast<U*>(p.out);
    const size_t sx = CU, sy = (size_t)p.Wf * CU, sz = (size_t)p.Hf * sy;
    for (size_t idx = (size_t)blockIdx.x * POOL_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * POOL_BLOCK) {
        size_t v = idx / CU; const int c = (int)(idx - v * CU);
        const int ox = (int)(v % p.Wc); v /= p.Wc;
        const int oy = (int)(v % p.Hc); v /= p.Hc;
        const int oz = (int)(v % p.Dc); const int b = (int)(v / p.Dc);
        const U* s = x + (((size_t)b * p.Df + 2 * oz) * p.Hf + 2 * oy) * sy + (size_t)(2 * ox) * sx + c;   // (2o + 1 < fine size: VALID)
        const U a0 = s[0], a1 = s[sx], a2 = s[sy], a3 = s[sy + sx], a4 = s[sz], a5 = s[sz + sx], a6 = s[sz + sy], a7 = s[sz + sy + sx];
        y[idx] = pmax(pmax(pmax(a0, a1), pmax(a2, a3)), pmax(pmax(a4, a5), pmax(a6, a7)));
    }
}

// one channel of one fine voxel: e[k] = the window's values in scan order, k = this voxel's place in it, m = the window's maximum
__device__ __forceinline__ float pool_take(const float (&e)[8], int k, float m, float g) {
    bool first = e[k] == m;
#pragma unroll
    for (int j = 0; j < 7; ++j) first = first && !(j < k && e[j] == m);
    return first ? g : 0.f;
}

template <bool VEC>
__global__ void __launch_bounds__(POOL_BLOCK) maxpool2_bwd_kernel(PoolP p) {
    using U = typename PoolUnit<VEC>::T;
    const int CU = VEC ? p.C >> 2 : p.C;
    const size_t n = (size_t)p.B * p.Df * p.Hf * p.Wf * CU;
    const U* __restrict__ x = reinterpret_cast<const U*>(p.x);
    const U* __restrict__ y = reinterpret_cast<const U*>(p.y);
    const U* __restrict__ dy = reinterpret_cast<const U*>(p.dy);
    U* dx = reinterpret_cast<U*>(p.out);
    const size_t sx = CU, sy = (size_t)p.Wf * CU, sz = (size_t)p.Hf * sy;
    for (size_t idx = (size_t)blockIdx.x * POOL_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * POOL_BLOCK) {
        size_t v = idx / CU; const int c = (int)(idx - v * CU);
        const int fx = (int)(v % p.Wf); v /= p.Wf;
        const int fy = (int)(v % p.Hf); v /= p.Hf;
        const int fz = (int)(v % p.Df); const int b = (int)(v / p.Df);
        const int oz = fz >> 1, oy = fy >> 1, ox = fx >> 1;
        U r;
        if constexpr (VEC) r = make_float4(0.f, 0.f, 0.f, 0.f); else r = 0.f;
        if (oz < p.Dc && oy < p.Hc && ox < p.Wc) {         // (else: a voxel VALID dropped, gradient 0)
            const size_t o = ((((size_t)b * p.Dc + oz) * p.Hc + oy) * p.Wc + ox) * CU + c;
            const U* s = x + (((size_t)b * p.Df + 2 * oz) * p.Hf + 2 * oy) * sy + (size_t)(2 * ox) * sx + c;
            const U w[8] = {s[0], s[sx], s[sy], s[sy + sx], s[sz], s[sz + sx], s[sz + sy], s[sz + sy + sx]};
            const U m = y[o], g = dy[o];
            const int k = (fz & 1) * 4 + (fy & 1) * 2 + (fx & 1);
            if constexpr (VEC) {
                float e0[8], e1[8], e2[8], e3[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { e0[j] = w[j].x; e1[j] = w[j].y; e2[j] = w[j].z; e3[j] = w[j].w; }
                r = make_float4(pool_take(e0, k, m.x, g.x), pool_take(e1, k, m.y, g.y), pool_take(e2, k, m.z, g.z), pool_take(e3, k, m.w, g.w));
            } else {
                r = pool_take(w, k, m, g);
            }
        }
        if (p.accum) {
            const U old = dx[idx];
            if constexpr (VEC) { r.x += old.x; r.y += old.y; r.z += old.z; r.w += old.w; } else r += old;
        }
        dx[idx] = r;
    }
}

inline int pool_blocks(size_t units) {
    size_t b = (units + POOL_BLOCK - 1) / POOL_BLOCK;
    return (int)(b < 1 ? 1 : b > POOL_MAXBLK ? POOL_MAXBLK : b);
}

inline bool pool_vec(int C, const void* a, const void* b, const void* c, const void* d) {
    return C % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace

extern "C" {

int vnet_maxpool2_fwd(const float* x, float* y, int C, int B, int Df, int Hf, int Wf, void* stream) {
    if (!x || !y || C <= 0 || B <= 0 || Df < 2 || Hf < 2 || Wf < 2) return VNET_E_BADARG;
    PoolP p{};
    p.x = x; p.out = y; p.C = C; p.B = B; p.Df = Df; p.Hf = Hf; p.Wf = Wf; p.Dc = Df / 2; p.Hc = Hf / 2; p.Wc = Wf / 2;
    const bool vec = pool_vec(C, x, y, nullptr, nullptr);
    const size_t units = (size_t)B * p.Dc * p.Hc * p.Wc * (vec ? C / 4 : C);
    return with_bool(vec, [&](auto V) {
        return launch<maxpool2_fwd_kernel<V>>(dim3(pool_blocks(units)), dim3(POOL_BLOCK), 0, (hipStream_t)stream, p);
    });
}

int vnet_maxpool2_bwd(const float* dy, const float* x, const float* y, float* dx, int C, int B, int Df, int Hf, int Wf, int accum,
                      void* stream) {
    if (!dy || !x || !y || !dx || C <= 0 || B <= 0 || Df < 2 || Hf < 2 || Wf < 2) return VNET_E_BADARG;
    PoolP p{};
    p.x = x; p.y = y; p.dy = dy; p.out = dx; p.accum = accum ? 1 : 0;
    p.C = C; p.B = B; p.Df = Df; p.Hf = Hf; p.Wf = Wf; p.Dc = Df / 2; p.Hc = Hf / 2; p.Wc = Wf / 2;
    const bool vec = pool_vec(C, dy, x, y, dx);
    const size_t units = (size_t)B * Df * Hf * Wf * (vec ? C / 4 : C);
    return with_bool(vec, [&](auto V) {
        return launch<maxpool2_bwd_kernel<V>>(dim3(pool_blocks(units)), dim3(POOL_BLOCK), 0, (hipStream_t)stream, p);
    });
}

}  // extern "C"
