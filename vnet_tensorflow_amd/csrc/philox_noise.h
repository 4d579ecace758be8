// philox_noise.h -- the noise of a training sample (include/vnet_hip_sample.h), shared by sample.hip and deform_sample.hip: the normal deviate
// of output element e is a function of (seed, e) alone -- Philox4x32-10 keyed by the seed on the counter q = e >> 2, two Box-Muller pairs
// per group of four elements -- and the element becomes fmaf(sigma, z, x).  sp_noise_quad serves a thread that owns the four elements
// of a group, sp_noise_one a thread that owns one element; the values do not depend on which.
#pragma once
#include <math.h>
#include "common.h"

namespace {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one Box-Muller pair from two words (precise logf / sqrtf / cosf / sinf)
__device__ __forceinline__ void box_muller(unsigned ka, unsigned kb, float& zc, float& zs) {
    const float u1 = ((float)(ka >> 9) + 0.5f) * 1.1920928955078125e-07f;       // 2^-23
    const float u2 = (float)(kb >> 8) * 5.9604644775390625e-08f;                // 2^-24
    const float r = sqrtf(-2.0f * logf(u1));
    const float th = 6.2831855f * u2;
    zc = r * cosf(th);
    zs = r * sinf(th);
}

// the four elements 4q .. 4q + 3 of group q
__device__ __forceinline__ float4 sp_noise_quad(float4 f, unsigned long long q, float sigma, unsigned k0, unsigned k1) {
    unsigned k[4];
    philox4x32_10((unsigned)q, (unsigned)(q >> 32), 0u, 0u, k0, k1, k);
    float z0, z1, z2, z3;
    box_muller(k[0], k[1], z0, z1);
    box_muller(k[2], k[3], z2, z3);
    f.x = fmaf(sigma, z0, f.x); f.y = fmaf(sigma, z1, f.y); f.z = fmaf(sigma, z2, f.z); f.w = fmaf(sigma, z3, f.w);
    return f;
}

// element e alone
__device__ __forceinline__ float sp_noise_one(float f, unsigned long long e, float sigma, unsigned k0, unsigned k1) {
    const unsigned long long q = e >> 2;
    const int j = (int)(e & 3);
    unsigned k[4];
    philox4x32_10((unsigned)q, (unsigned)(q >> 32), 0u, 0u, k0, k1, k);
    float zc, zs;
    box_muller((j & 2) ? k[2] : k[0], (j & 2) ? k[3] : k[1], zc, zs);
    return fmaf(sigma, (j & 1) ? zs : zc, f);
}

inline bool sp_bad_window(int n, int s, int w) { return s < 0 || w < 1 || s > n - w; }

}  // namespace
