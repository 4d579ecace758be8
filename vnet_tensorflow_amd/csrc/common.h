// common.h -- shared helpers for the gfx950 kernels of libvnet_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>
#include "../../include/vnet_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// two fp32 -> packed bf16 pair, round-to-nearest-even (the rounding of every bf16 operand in this library)
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// ---- the one launch path of the library ----
// Dynamic-LDS bytes configured for kernel K, per device (the attribute is per (kernel, device)).
template <auto K>
inline std::atomic<size_t> vnet_lds_set[64];

// Launches K<<<grid, block, lds, st>>>(args...) and returns 0 or the hipError_t (as an int).  A non-zero `lds` first raises
// K's dynamic-LDS limit on the current device when it is below `lds`: once per (kernel, device), again only for a larger
// size.  Launches may come from several host threads (vnet_infer's workers, torch's autograd thread): the check that finds
// the limit already set is one atomic load; the rare setting is serialised.
template <auto K, typename... A>
int launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... args) {
    if (lds) {
        int dev = 0;
        if (hipError_t e = hipGetDevice(&dev)) return (int)e;
        std::atomic<size_t>& set = vnet_lds_set<K>[dev & 63];
        if (set.load(std::memory_order_acquire) < lds) {
            static std::mutex mu;
            std::lock_guard<std::mutex> lk(mu);
            if (set.load(std::memory_order_relaxed) < lds) {
                if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
                    return (int)e;
                set.store(lds, std::memory_order_release);
            }
        }
    }
    hipLaunchKernelGGL(K, grid, block, lds, st, std::forward<A>(args)...);
    return (int)hipGetLastError();
}

// Runtime value -> template argument: f(std::integral_constant<bool, b>{}) ...
template <typename F>
decltype(auto) with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// ... and f(std::integral_constant<int, V>{}) for the V of Vs equal to v; VNET_E_UNSUPPORTED when none is.
template <int... Vs, typename F>
int with_int(int v, F&& f) {
    int r = VNET_E_UNSUPPORTED;
    (void)((v == Vs && ((r = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return r;
}

// compute units of the current device (cached per device; 256 on MI355X)
inline int device_cus() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int c = cached[dev & 63].load(std::memory_order_relaxed);
    if (c == 0) {
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 8) c = 256;
        cached[dev & 63].store(c, std::memory_order_relaxed);
    }
    return c;
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// 64-lane butterfly sum (wave = 64 on gfx950)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// XCD-aware bijective remap of a linear workgroup id (8 XCDs, block b runs on XCD b%8):
// consecutive remapped ids share an XCD/L2, so neighbouring bricks (which share halo voxels and
// all weights) hit the same L2.  Speed only; any placement is correct.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7, k = orig >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}
