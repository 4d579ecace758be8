// cc_table.h -- the dense component table, shared by sample.hip (vnet_cc_table), score.hip (vnet_cc_shape) and bbox.hip: the representative map of
// components.hip -> rows {representative, count, lo[3], hi[3]} in ascending representative order, and with SUMS the int64 index sums
// {sum x, sum y, sum z} of every row.  The rank of a root (the number of roots with a smaller index) is a device-wide prefix sum,
// written as three launches so that NO thread waits for another (no look-back, no flags, no spin):
//   count : every block counts the roots of its own contiguous chunk of voxels
//   scan  : one block turns the block counts into exclusive offsets, writes n and zeroes the rows past it
//   rank  : every block walks its chunk in order and ranks its roots with ballots; a root writes its row's head
//           and leaves its rank where its count stood (the count array becomes the root -> row map)
// and a fourth pass folds every voxel's coordinates into its row with atomicMin / atomicMax (SUMS: and 64-bit atomicAdd), combined per
// wave first (components.hip's counting scheme: a solid organ issues one set of atomics per wave-trip run, not per voxel).
// SUMS is a template argument: the kernels of vnet_cc_table are the ones they were before this header existed.
// Voxel indices are int32 (n <= 2^31 - 1, checked on the host); element offsets are 64-bit.
#pragma once
#include <limits.h>
#include "common.h"
#include "../../include/vnet_hip_components.h"
#include "../../include/vnet_hip_sample.h"

namespace {

constexpr int SP_BLOCK = 256, SP_MAXBLK = 4096, SP_WAVES = SP_BLOCK / 64;

typedef unsigned long long u64;

inline int sp_blocks(size_t units) {
    size_t b = (units + SP_BLOCK - 1) / SP_BLOCK;
    return (int)(b < 1 ? 1 : b > SP_MAXBLK ? SP_MAXBLK : b);
}

// 0 and the voxel count, VNET_E_BADARG on a size < 1, VNET_E_UNSUPPORTED when an int32 cannot index the volume
inline int sp_count(int X, int Y, int Z, size_t& n) {
    if (X < 1 || Y < 1 || Z < 1) return VNET_E_BADARG;
    n = (size_t)X * (size_t)Y * (size_t)Z;
    return n > (size_t)INT_MAX ? VNET_E_UNSUPPORTED : 0;
}

// Chunks: block b owns voxels [b * chunk, min(n, (b + 1) * chunk)), chunk a multiple of SP_BLOCK, at most SP_MAXBLK blocks.
struct TableP {
    const int* roots;      // representative map (vnet_cc_roots)
    int* sizes;            // count at the representative; after the rank pass: the representative's row, -1 past the capacity
    int* blk;              // [SP_MAXBLK] root count of each block, then its exclusive offset
    int* n;
    int* table;
    long long* sums;       // SUMS: [cap, 3]
    int cap, nblk;
    size_t nvox, chunk;
    int Y, Z;
};

__global__ void __launch_bounds__(SP_BLOCK) table_count_kernel(TableP p) {
    __shared__ int wsum[SP_WAVES];
    const size_t lo = (size_t)blockIdx.x * p.chunk, hi = lo + p.chunk < p.nvox ? lo + p.chunk : p.nvox;
    int c = 0;
    for (size_t idx = lo + threadIdx.x; idx < hi; idx += SP_BLOCK) c += p.roots[idx] == (int)idx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < SP_WAVES; ++w) s += wsum[w];
        p.blk[blockIdx.x] = s;
    }
}

// one block: blk[b] <- sum of blk[0 .. b), *n <- the total, rows [min(n, cap), cap) <- 0
template <bool SUMS>
__global__ void __launch_bounds__(SP_BLOCK) table_scan_kernel(TableP p) {
    constexpr int PER = SP_MAXBLK / SP_BLOCK;
    __shared__ int part[SP_BLOCK];
    __shared__ int total;
    int v[PER], s = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int b = threadIdx.x * PER + i;
        v[i] = b < p.nblk ? p.blk[b] : 0;
        s += v[i];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {                          // 256 adds by one thread, once per case
        int run = 0;
        for (int t = 0; t < SP_BLOCK; ++t) { const int c = part[t]; part[t] = run; run += c; }
        total = run;
        *p.n = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int b = threadIdx.x * PER + i;
        if (b < p.nblk) p.blk[b] = run;
        run += v[i];
    }
    const int first = total < p.cap ? total : p.cap;
    for (int w = first * VNET_CC_ROW + threadIdx.x; w < p.cap * VNET_CC_ROW; w += SP_BLOCK) p.table[w] = 0;
    if constexpr (SUMS)
        for (size_t w = (size_t)first * 3 + threadIdx.x; w < (size_t)p.cap * 3; w += SP_BLOCK) p.sums[w] = 0;
}

// The loop runs on the block's base index so that all lanes of a wave make every trip together (wave-wide votes).
template <bool SUMS>
__global__ void __launch_bounds__(SP_BLOCK) table_rank_kernel(TableP p) {
    __shared__ int wcnt[2][SP_WAVES];                // double-buffered by trip parity: one barrier per trip
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t lo = (size_t)blockIdx.x * p.chunk, hi = lo + p.chunk < p.nvox ? lo + p.chunk : p.nvox;
    int run = p.blk[blockIdx.x];                     // roots in front of this trip
    int trip = 0;
    for (size_t base = lo; base < hi; base += SP_BLOCK, trip ^= 1) {
        const size_t idx = base + threadIdx.x;
        const bool root = idx < hi && p.roots[idx] == (int)idx;
        const u64 m = __ballot(root);
        if (lane == 0) wcnt[trip][wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SP_WAVES; ++w) {
            const int c = wcnt[trip][w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (root) {
            const int k = run + before + __popcll(m & ((1ull << lane) - 1ull));
            const int count = p.sizes[idx];
            p.sizes[idx] = k < p.cap ? k : -1;
            if (k < p.cap) {
                int* row = p.table + (size_t)k * VNET_CC_ROW;
                row[0] = (int)idx; row[1] = count;
                row[2] = INT_MAX; row[3] = INT_MAX; row[4] = INT_MAX;
                row[5] = 0; row[6] = 0; row[7] = 0;
                if constexpr (SUMS) {
                    long long* s = p.sums + (size_t)k * 3;
                    s[0] = 0; s[1] = 0; s[2] = 0;
                }
            }
        }
        run += all;
    }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}
// (a coordinate is below 2^31 and a wave holds 64 of them: below 2^37)
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void box_fold(int* row, const int lo[3], const int hi[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(row + 2 + a, lo[a]); atomicMax(row + 5 + a, hi[a]); }
}

// integer adds commute: the sums are the same whatever order the waves arrive in
__device__ __forceinline__ void sum_fold(long long* s, const long long v[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(reinterpret_cast<u64*>(s) + a, (u64)v[a]);
}

// The lanes that share the first foreground lane's root fold their extremes once per run of trips with that root; the others one each.
template <bool SUMS>
__global__ void __launch_bounds__(SP_BLOCK) table_box_kernel(TableP p) {
    const int lane = threadIdx.x & 63;
    int acc_row = -1, alo[3] = {INT_MAX, INT_MAX, INT_MAX}, ahi[3] = {0, 0, 0};      // wave-uniform
    long long asum[3] = {0, 0, 0};
    int acc_root = -1;
    for (size_t base = (size_t)blockIdx.x * SP_BLOCK; base < p.nvox; base += (size_t)gridDim.x * SP_BLOCK) {
        const size_t idx = base + threadIdx.x;
        const int r = idx < p.nvox ? p.roots[idx] : -1;
        const bool fg = r >= 0;
        const u64 m = __ballot(fg);
        if (m == 0) continue;
        const unsigned row_i = (unsigned)idx / (unsigned)p.Z;
        int c[3];
        c[2] = (int)((unsigned)idx - row_i * (unsigned)p.Z); c[1] = (int)(row_i % (unsigned)p.Y); c[0] = (int)(row_i / (unsigned)p.Y);
        const int r0 = __shfl(r, __ffsll(m) - 1, 64);
        const bool same = fg && r == r0;
        if (r0 != acc_root) {
            if (acc_row >= 0 && lane == 0) {
                box_fold(p.table + (size_t)acc_row * VNET_CC_ROW, alo, ahi);
                if constexpr (SUMS) sum_fold(p.sums + (size_t)acc_row * 3, asum);
            }
            acc_root = r0;
            acc_row = p.sizes[r0];                   // (-1: a component past the capacity has no row)
#pragma unroll
            for (int a = 0; a < 3; ++a) { alo[a] = INT_MAX; ahi[a] = 0; asum[a] = 0; }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int l = wave_min_i(same ? c[a] : INT_MAX), h = wave_max_i(same ? c[a] : 0);
            alo[a] = l < alo[a] ? l : alo[a];
            ahi[a] = h > ahi[a] ? h : ahi[a];
            if constexpr (SUMS) asum[a] += wave_sum_ll(same ? (long long)c[a] : 0ll);
        }
        if (fg && !same) {
            const int k = p.sizes[r];
            if (k >= 0) {
                box_fold(p.table + (size_t)k * VNET_CC_ROW, c, c);
                if constexpr (SUMS) {
                    const long long cl[3] = {c[0], c[1], c[2]};
                    sum_fold(p.sums + (size_t)k * 3, cl);
                }
            }
        }
    }
    if (acc_row >= 0 && lane == 0) {
        box_fold(p.table + (size_t)acc_row * VNET_CC_ROW, alo, ahi);
        if constexpr (SUMS) sum_fold(p.sums + (size_t)acc_row * 3, asum);
    }
}

inline size_t cc_table_bytes(size_t n) { return 8 * n + sizeof(int) * SP_MAXBLK; }

// Carves `ws` (cc_table_bytes(n), 8-byte aligned) into the block counts, the representative map and the counts, and sets the chunking
// of p for a volume [., Y, Z] of n voxels.  Returns the representative map for the labelling passes to fill (with p.sizes).
inline int* cc_table_carve(TableP& p, void* ws, size_t n, int* n_out, int* table, long long* sums, int max_components, int Y, int Z) {
    p.blk = static_cast<int*>(ws);                   // (in front: the voxel arrays behind it stay 8-byte aligned whatever n is)
    int* roots = p.blk + SP_MAXBLK;
    p.roots = roots; p.sizes = roots + n; p.n = n_out; p.table = table; p.sums = sums; p.cap = max_components;
    p.nvox = n; p.Y = Y; p.Z = Z;
    p.chunk = align_up((n + SP_MAXBLK - 1) / SP_MAXBLK, (size_t)SP_BLOCK);
    p.nblk = (int)((n + p.chunk - 1) / p.chunk);
    return roots;
}

// count, scan, rank, box on a representative map with its counts (p.roots, p.sizes): shared with bbox.hip, whose map stays inside slices
template <bool SUMS>
inline int cc_table_passes(const TableP& p, hipStream_t st) {
    if (int e = launch<table_count_kernel>(dim3(p.nblk), dim3(SP_BLOCK), 0, st, p)) return e;
    if (int e = launch<table_scan_kernel<SUMS>>(dim3(1), dim3(SP_BLOCK), 0, st, p)) return e;
    if (int e = launch<table_rank_kernel<SUMS>>(dim3(p.nblk), dim3(SP_BLOCK), 0, st, p)) return e;
    return launch<table_box_kernel<SUMS>>(dim3(sp_blocks(p.nvox)), dim3(SP_BLOCK), 0, st, p);
}

// The checks of vnet_cc_table / vnet_cc_shape (VNET_E_BADARG, VNET_E_UNSUPPORTED, VNET_E_WORKSPACE, in that order), then the launches.
template <bool SUMS>
inline int cc_table_run(const int* label, int* n_out, int* table, long long* sums, int max_components, int X, int Y, int Z, void* ws,
                        size_t ws_bytes, void* stream) {
    size_t n = 0;
    if (!label || !n_out || !table || (SUMS && !sums) || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || max_components < 1)
        return VNET_E_BADARG;
    if (int e = sp_count(X, Y, Z, n)) return e;
    if ((size_t)max_components > (size_t)INT_MAX / VNET_CC_ROW) return VNET_E_UNSUPPORTED;
    if (ws_bytes < cc_table_bytes(n)) return VNET_E_WORKSPACE;
    TableP p{};
    int* roots = cc_table_carve(p, ws, n, n_out, table, sums, max_components, Y, Z);
    if (int e = vnet_cc_roots(label, roots, p.sizes, X, Y, Z, stream)) return e;
    return cc_table_passes<SUMS>(p, (hipStream_t)stream);
}

}  // namespace
