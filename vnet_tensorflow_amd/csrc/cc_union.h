// cc_union.h -- the lock-free union-find over a voxel array, shared by components.hip (face-connected components of a volume) and
// bbox.hip (components inside a slice, one class each): the two finds, the unite, and the body of the flatten-and-count pass.
// `parent[v] <= v` throughout, -1 on the background.  No thread ever waits for another: every loop below strictly decreases an index
// or ends.  Why a link pass built on these is correct across the XCDs' L2s: DESIGN.md section 6c.
// The functions are the ones components.hip held before this header existed: its kernels are what they were.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;

// ---- link pass: every access to parent[] is an agent-scope atomic (another workgroup may be writing the word) ----
__device__ __forceinline__ int cc_find_agent(int* parent, int a) {
    // bounded: a is replaced by parent[a] < a, or the loop ends (parent[a] == a: a root; anything else cannot be followed)
    for (;;) {
        const int p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)p >= (unsigned)a) return a;
        a = p;
    }
}

__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
    a = cc_find_agent(parent, a);
    b = cc_find_agent(parent, b);
    // bounded: every trip replaces max(a, b) by a strictly smaller index (old < a, and a root is never above its voxel) or ends
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);    // agent-scope RMW: a, a root when read, now hangs under the smaller root b
        if (old == a) break;                         // a still was a root: linked
        // a had been linked under `old` meanwhile and now points at min(old, b): the sets of old and b are still to be united
        a = cc_find_agent(parent, old);
        b = cc_find_agent(parent, b);
    }
}

// ---- flatten pass: no union runs in this launch, so the forest is fixed and a word holds either its parent of the launch's start or its
// root -- both are ancestors, whichever a load sees.  Relaxed single-word atomics at wavefront scope: plain loads and stores, never torn.
__device__ __forceinline__ int cc_find_plain(const int* parent, int a) {
    // bounded: a is replaced by parent[a] < a, or the loop ends
    for (;;) {
        const int p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if ((unsigned)p >= (unsigned)a) return a;
        a = p;
    }
}

// The body of a flatten kernel of BLOCK threads: every voxel's parent becomes its root, in place; with `sizes` the same pass counts the
// voxels per root, aggregated per wave.  The loop runs on the block's base index, so that all 64 lanes of a wave make every trip
// together (wave-wide votes) and lane l of a wave holds voxel (wave's first voxel) + l.
template <int BLOCK>
__device__ __forceinline__ void cc_flatten_body(int* parent, int* sizes, size_t n) {
    const int lane = threadIdx.x & 63;
    int acc_root = -1, acc_n = 0;                    // wave-uniform: voxels of one root seen in consecutive trips, added once
    // bounded: a grid-stride loop over n voxels; cc_find_plain inside it is bounded on its own
    for (size_t base = (size_t)blockIdx.x * BLOCK; base < n; base += (size_t)gridDim.x * BLOCK) {
        const size_t idx = base + threadIdx.x;
        int r = -1;
        if (idx < n) {
            const int p = __hip_atomic_load(parent + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (p >= 0) {
                r = cc_find_plain(parent, (int)idx);
                if (r != p) __hip_atomic_store(parent + idx, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        if (!sizes) continue;
        // integer adds only; the lanes that share the first foreground lane's root add their number once, the others one each
        const bool fg = r >= 0;
        const u64 m = __ballot(fg);
        if (m == 0) continue;
        const int r0 = __shfl(r, __ffsll(m) - 1, 64);
        const bool same = fg && r == r0;
        const u64 ms = __ballot(same);
        if (r0 != acc_root) {
            if (acc_n && lane == 0) atomicAdd(sizes + acc_root, acc_n);
            acc_root = r0;
            acc_n = 0;
        }
        acc_n += __popcll(ms);
        if (fg && !same) atomicAdd(sizes + r, 1);
    }
    if (sizes && acc_n && lane == 0) atomicAdd(sizes + acc_root, acc_n);
}

}  // namespace
