// components.hip -- face-connected components of a label map and the two label filters that close the reference's evaluate
// (include/vnet_hip_components.h; reference model.py:117-140 `volume_threshold`, model.py:142-167 `ExtractLargestConnectedComponents`),
// int32 [X,Y,Z] on gfx950.  A lock-free union-find over the voxel array, `parent[v] <= v` throughout:
//   init    : parent[v] = first voxel of v's z-run inside this wave (or the voxel in front of the wave when the run started earlier), -1 on
//             the background; sizes and the selection key are zeroed here, by the kernel
//   link    : every foreground voxel unites itself with its y and x predecessors (the z predecessor is the init pass's link); a link that
//             the previous voxel of the row makes already is skipped
//   flatten : every voxel's parent becomes its root, in place; the same pass counts the voxels per root, aggregated per wave
//   select  : one 64-bit atomicMax per wave on (count << 32 | ~representative)
//   write   : the 0/1 map
// Streaming passes on the pattern of pool.hip and resample.hip: grid-stride under a fixed grid cap, one thread per voxel, no LDS, no
// scratch.  Voxel indices are int32 (n <= 2^31 - 1, checked on the host); element offsets are 64-bit.  No thread ever waits for another:
// every loop below strictly decreases an index.  Why the link pass is correct across the XCDs' L2s: DESIGN.md section 6c.
#include <math.h>
#include <limits.h>
#include "common.h"
#include "cc_union.h"
#include "../../include/vnet_hip_components.h"

namespace {

constexpr int CC_BLOCK = 256, CC_MAXBLK = 4096;
constexpr size_t CC_HEAD = 16;                       // the selection key, padded so that the int arrays behind it stay 16-byte aligned

typedef unsigned long long u64;

// cc_find_agent / cc_unite (link pass) and cc_find_plain / cc_flatten_body (flatten pass): cc_union.h, shared with bbox.hip

// In the three kernels with wave-wide votes the loop runs on the block's base index, so that all 64 lanes of a wave make every trip
// together and lane l of a wave holds voxel (wave's first voxel) + l.
__global__ void __launch_bounds__(CC_BLOCK) cc_init_kernel(const int* __restrict__ label, int* __restrict__ parent, int* __restrict__ sizes,
                                                           u64* __restrict__ key, size_t n, int Z) {
    const int lane = threadIdx.x & 63;
    if (key && blockIdx.x == 0 && threadIdx.x == 0) *key = 0;
    for (size_t base = (size_t)blockIdx.x * CC_BLOCK; base < n; base += (size_t)gridDim.x * CC_BLOCK) {
        const size_t idx = base + threadIdx.x;
        const bool valid = idx < n;
        const int z = valid ? (int)((unsigned)idx % (unsigned)Z) : 0;
        const bool fg = valid && label[idx] != 0;
        const u64 mfg = __ballot(fg);
        // the voxel in front of this one in its row: the lane below, or for lane 0 a load (z > 0: idx - 1 is in the same row)
        const bool prev = lane ? ((mfg >> (lane - 1)) & 1) != 0 : (valid && z > 0 && label[idx - 1] != 0);
        const bool start = fg && (z == 0 || !prev);
        const u64 mst = __ballot(start);
        if (valid) {
            int p = -1;
            if (fg) {
                const u64 below = mst & ((2ull << lane) - 1ull);                       // run starts at lanes <= this one
                p = below ? (int)idx - (lane - (63 - __clzll((long long)below)))       // the nearest one starts this voxel's run
                          : (int)idx - lane - 1;                                       // the run began in front of the wave: chain on
            }
            parent[idx] = p;
            if (sizes) sizes[idx] = 0;
        }
    }
}

__global__ void __launch_bounds__(CC_BLOCK) cc_link_kernel(const int* __restrict__ label, int* parent, size_t n, int Y, int Z) {
    const int YZ = Y * Z;
    for (size_t idx = (size_t)blockIdx.x * CC_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * CC_BLOCK) {
        if (label[idx] == 0) continue;
        const unsigned row = (unsigned)idx / (unsigned)Z;
        const int v = (int)idx, z = (int)((unsigned)idx - row * (unsigned)Z), y = (int)(row % (unsigned)Y), x = (int)(row / (unsigned)Y);
        // neighbours come from the coordinates: at z == 0 the voxel idx - 1 is the end of another row, at y == 0 idx - Z another plane
        const bool zp = z > 0 && label[idx - 1] != 0;
        // (v - 1, u - 1 both foreground: v ~ v - 1 and u ~ u - 1 are run links of the init pass and v - 1 ~ u - 1 is made at v - 1)
        if (y > 0 && label[idx - Z] != 0 && !(zp && label[idx - Z - 1] != 0)) cc_unite(parent, v - Z, v);
        if (x > 0 && label[idx - YZ] != 0 && !(zp && label[idx - YZ - 1] != 0)) cc_unite(parent, v - YZ, v);
    }
}

__global__ void __launch_bounds__(CC_BLOCK) cc_flatten_kernel(int* parent, int* sizes, size_t n) {
    cc_flatten_body<CC_BLOCK>(parent, sizes, n);
}

// sizes[v] > 0 only at a representative.  More voxels win; of equal counts the smaller representative (the larger ~v).
__global__ void __launch_bounds__(CC_BLOCK) cc_select_kernel(const int* __restrict__ sizes, u64* key, size_t n) {
    u64 k = 0;
    for (size_t idx = (size_t)blockIdx.x * CC_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * CC_BLOCK) {
        const int c = sizes[idx];
        if (c > 0) {
            const u64 mine = ((u64)(unsigned)c << 32) | (u64)(0xFFFFFFFFu - (unsigned)idx);
            k = mine > k ? mine : k;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(k, o, 64);
        k = other > k ? other : k;
    }
    if ((threadIdx.x & 63) == 0 && k) atomicMax(key, k);
}

__global__ void __launch_bounds__(CC_BLOCK) cc_write_largest_kernel(const int* __restrict__ roots, const u64* __restrict__ key,
                                                                    unsigned char* __restrict__ out, size_t n, int thresholded, double volume,
                                                                    double voxel_volume) {
    const u64 k = *key;
    const unsigned count = (unsigned)(k >> 32);
    const int rep = (int)(0xFFFFFFFFu - (unsigned)k);
    const bool keep = count > 0 && (!thresholded || (double)count * voxel_volume > volume);      // no foreground: key 0, nothing kept
    for (size_t idx = (size_t)blockIdx.x * CC_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * CC_BLOCK)
        out[idx] = keep && roots[idx] == rep ? 1 : 0;
}

__global__ void __launch_bounds__(CC_BLOCK) cc_write_threshold_kernel(const int* __restrict__ roots, const int* __restrict__ sizes,
                                                                      unsigned char* __restrict__ out, size_t n, double volume,
                                                                      double voxel_volume) {
    for (size_t idx = (size_t)blockIdx.x * CC_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * CC_BLOCK) {
        const int r = roots[idx];
        out[idx] = r >= 0 && (double)sizes[r] * voxel_volume > volume ? 1 : 0;
    }
}

inline int cc_blocks(size_t n) {
    size_t b = (n + CC_BLOCK - 1) / CC_BLOCK;
    return (int)(b < 1 ? 1 : b > CC_MAXBLK ? CC_MAXBLK : b);
}

// 0 and the voxel count, VNET_E_BADARG on a size < 1, VNET_E_UNSUPPORTED when an int32 cannot index the volume
inline int cc_count(int X, int Y, int Z, size_t& n) {
    if (X < 1 || Y < 1 || Z < 1) return VNET_E_BADARG;
    n = (size_t)X * (size_t)Y * (size_t)Z;
    return n > (size_t)INT_MAX ? VNET_E_UNSUPPORTED : 0;
}

// init, link, flatten (+ count when sizes is given) on `roots`
inline int cc_label(const int* label, int* roots, int* sizes, u64* key, size_t n, int Y, int Z, hipStream_t st) {
    const dim3 grid(cc_blocks(n)), block(CC_BLOCK);
    if (int e = launch<cc_init_kernel>(grid, block, 0, st, label, roots, sizes, key, n, Z)) return e;
    if (int e = launch<cc_link_kernel>(grid, block, 0, st, label, roots, n, Y, Z)) return e;
    return launch<cc_flatten_kernel>(grid, block, 0, st, roots, sizes, n);
}

struct CcWs { u64* key; int* roots; int* sizes; };

inline bool cc_bad_ws(const void* ws) { return !ws || (reinterpret_cast<uintptr_t>(ws) & 7); }

inline int cc_carve(void* ws, size_t ws_bytes, size_t n, CcWs& w) {
    if (ws_bytes < CC_HEAD + 8 * n) return VNET_E_WORKSPACE;
    char* b = static_cast<char*>(ws);
    w.key = reinterpret_cast<u64*>(b);
    w.roots = reinterpret_cast<int*>(b + CC_HEAD);
    w.sizes = w.roots + n;
    return 0;
}

}  // namespace

extern "C" {

size_t vnet_cc_ws_bytes(int X, int Y, int Z) {
    size_t n = 0;
    return cc_count(X, Y, Z, n) ? 0 : CC_HEAD + 8 * n;
}

int vnet_cc_roots(const int* label, int* roots, int* sizes, int X, int Y, int Z, void* stream) {
    size_t n = 0;
    if (!label || !roots) return VNET_E_BADARG;
    if (int e = cc_count(X, Y, Z, n)) return e;
    return cc_label(label, roots, sizes, nullptr, n, Y, Z, (hipStream_t)stream);
}

int vnet_cc_largest(const int* label, unsigned char* out, int X, int Y, int Z, int thresholded, double volume, double voxel_volume,
                    void* ws, size_t ws_bytes, void* stream) {
    size_t n = 0;
    CcWs w{};
    if (!label || !out || cc_bad_ws(ws) || !isfinite(volume) || !isfinite(voxel_volume)) return VNET_E_BADARG;
    if (int e = cc_count(X, Y, Z, n)) return e;
    if (int e = cc_carve(ws, ws_bytes, n, w)) return e;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cc_blocks(n)), block(CC_BLOCK);
    if (int e = cc_label(label, w.roots, w.sizes, w.key, n, Y, Z, st)) return e;
    if (int e = launch<cc_select_kernel>(grid, block, 0, st, (const int*)w.sizes, w.key, n)) return e;
    return launch<cc_write_largest_kernel>(grid, block, 0, st, (const int*)w.roots, (const u64*)w.key, out, n, thresholded ? 1 : 0, volume,
                                           voxel_volume);
}

int vnet_cc_volume_threshold(const int* label, unsigned char* out, int X, int Y, int Z, double volume, double voxel_volume,
                             void* ws, size_t ws_bytes, void* stream) {
    size_t n = 0;
    CcWs w{};
    if (!label || !out || cc_bad_ws(ws) || !isfinite(volume) || !isfinite(voxel_volume)) return VNET_E_BADARG;
    if (int e = cc_count(X, Y, Z, n)) return e;
    if (int e = cc_carve(ws, ws_bytes, n, w)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int e = cc_label(label, w.roots, w.sizes, w.key, n, Y, Z, st)) return e;
    return launch<cc_write_threshold_kernel>(dim3(cc_blocks(n)), dim3(CC_BLOCK), 0, st, (const int*)w.roots, (const int*)w.sizes, out, n,
                                             volume, voxel_volume);
}

}  // extern "C"
