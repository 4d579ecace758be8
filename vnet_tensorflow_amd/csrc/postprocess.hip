// postprocess.hip -- the post-processing pipeline of evaluate on the device label (vnet_post.h; rules: vnet_tensorflow_amd/postprocess.py,
// DESIGN.md section 6k), int32 [X,Y,Z] on gfx950, built into libvnet_post.so.  The lock-free union-find of cc_union.h (unchanged)
// under two linking rules:
//   classes    : two face neighbours are linked iff they hold the same label and that label is one of <= 16 values -- every class is
//                labelled by ONE init / link / flatten sequence (vnet_post_class_roots, vnet_post_filter_components)
//   complement : the foreground is label != klass, one mask (vnet_post_fill_holes: its components that touch no face are the cavities)
//   init    : parent[v] = first voxel of v's z-run inside this wave (or the voxel in front of the wave when the run started earlier), -1
//             where the voxel is not foreground; a run starts where the LABEL changes, not only where foreground begins; sizes and
//             the face flags are zeroed here, by the kernel
//   link    : every foreground voxel unites itself with its y and x predecessors of its own kind; a link that the previous voxel of the
//             row makes already is skipped
//   flatten : cc_flatten_body: every parent becomes its root, in place; with sizes the same pass counts the voxels per root
//   select  : mode 0: one 64-bit key per class slot, the maximum of (count << 32 | ~representative) over the representatives, by a
//             fixed two-launch reduction (per block into scratch, then one block over the blocks) -- no atomic
//   faces   : a byte per representative is set to 1 from the voxels on the six faces (equal-value stores)
//   write   : the int32 label, class values kept
// Streaming passes on the pattern of components.hip: grid-stride under a fixed grid cap, one thread per voxel (one per word in
// vnet_post_not_bits), no scratch, LDS only in the two selection kernels (512 B and 2 KiB).  The unit itself calls no atomic
// function: the union-find's are inside cc_union.h.  Voxel indices are int32 (n <= 2^31 - 1, checked on the host); element offsets are 64-bit.
// No thread ever waits for another: every loop below strictly decreases an index or walks a fixed range.  Why the link pass stays
// correct across the XCDs' L2s under the class rule: DESIGN.md section 6k (the argument of 6c, which never looks at the rule).
#include <math.h>
#include <limits.h>
#include "common.h"
#include "cc_union.h"
#include "vnet_post.h"

namespace {

constexpr int PP_BLOCK = 256, PP_MAXBLK = 4096;
constexpr int PP_SLOTS = VNET_POST_MAX_VALUES;
constexpr size_t PP_HEAD = PP_SLOTS * sizeof(u64);                   // the selection keys, one per class slot

// What counts as foreground and which neighbours belong together.  n == 0: the complement rule on v[0] (foreground is label != v[0]).
struct Rule {
    int v[VNET_POST_MAX_VALUES];
    int n;
};

// the class slot of a label under the class rule, -1 when it is none of the values
__device__ __forceinline__ int pp_slot(const Rule& r, int lab) {
    int s = -1;
    for (int k = 0; k < r.n; ++k) s = (lab == r.v[k]) ? k : s;
    return s;
}

__device__ __forceinline__ bool pp_foreground(const Rule& r, int lab) { return r.n ? pp_slot(r, lab) >= 0 : lab != r.v[0]; }

// whether a neighbour holding `other` belongs with a FOREGROUND voxel holding `lab`
__device__ __forceinline__ bool pp_same(const Rule& r, int lab, int other) { return r.n ? other == lab : other != r.v[0]; }

// In the kernels with wave-wide votes the loop runs on the block's base index, so that all 64 lanes of a wave make every trip together
// and lane l of a wave holds voxel (wave's first voxel) + l.
__global__ void __launch_bounds__(PP_BLOCK) pp_init_kernel(const int* __restrict__ label, int* __restrict__ parent, int* __restrict__ sizes,
                                                           unsigned char* __restrict__ flags, Rule rule, size_t n, int Z) {
    const int lane = threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * PP_BLOCK; base < n; base += (size_t)gridDim.x * PP_BLOCK) {
        const size_t idx = base + threadIdx.x;
        const bool valid = idx < n;
        const int z = valid ? (int)((unsigned)idx % (unsigned)Z) : 0;
        const int lab = valid ? label[idx] : 0;
        const bool fg = valid && pp_foreground(rule, lab);
        // the label in front of this voxel in its row: the lane below, or for lane 0 a load (z > 0: idx - 1 is in the same row)
        const int below_lab = __shfl_up(lab, 1, 64);
        const bool has_prev = valid && z > 0;
        const int prev_lab = has_prev ? (lane ? below_lab : label[idx - 1]) : 0;
        const bool start = fg && !(has_prev && pp_same(rule, lab, prev_lab));          // the row begins, or the voxel in front is of another kind
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
            if (flags) flags[idx] = 0;
        }
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_link_kernel(const int* __restrict__ label, int* parent, Rule rule, size_t n, int Y, int Z) {
    const int YZ = Y * Z;
    for (size_t idx = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * PP_BLOCK) {
        const int lab = label[idx];
        if (!pp_foreground(rule, lab)) continue;
        const unsigned row = (unsigned)idx / (unsigned)Z;
        const int v = (int)idx, z = (int)((unsigned)idx - row * (unsigned)Z), y = (int)(row % (unsigned)Y), x = (int)(row / (unsigned)Y);
        // neighbours come from the coordinates: at z == 0 the voxel idx - 1 is the end of another row, at y == 0 idx - Z another plane
        const bool zp = z > 0 && pp_same(rule, lab, label[idx - 1]);
        // (v - 1, u - 1 both of v's kind: v ~ v - 1 and u ~ u - 1 are run links of the init pass and v - 1 ~ u - 1 is made at v - 1)
        if (y > 0 && pp_same(rule, lab, label[idx - Z]) && !(zp && pp_same(rule, lab, label[idx - Z - 1]))) cc_unite(parent, v - Z, v);
        if (x > 0 && pp_same(rule, lab, label[idx - YZ]) && !(zp && pp_same(rule, lab, label[idx - YZ - 1]))) cc_unite(parent, v - YZ, v);
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_flatten_kernel(int* parent, int* sizes, size_t n) {
    cc_flatten_body<PP_BLOCK>(parent, sizes, n);
}

// sizes[v] > 0 only at a representative.  Per class slot: more voxels win; of equal counts the smaller representative (the larger ~v).
// A maximum of integers in a fixed tree: thread, wave (shuffles), block (LDS), then pp_select_final_kernel over the blocks' rows.
// best[] is only ever indexed by unrolled constants, so it stays in registers.
__global__ void __launch_bounds__(PP_BLOCK) pp_select_partial_kernel(const int* __restrict__ label, const int* __restrict__ sizes,
                                                                     u64* __restrict__ partial, Rule rule, size_t n) {
    __shared__ u64 wbest[PP_BLOCK / 64][PP_SLOTS];
    u64 best[PP_SLOTS];
#pragma unroll
    for (int k = 0; k < PP_SLOTS; ++k) best[k] = 0;
    for (size_t idx = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * PP_BLOCK) {
        const int c = sizes[idx];
        if (c <= 0) continue;
        const int s = pp_slot(rule, label[idx]);                                           // (a representative is a selected voxel)
        const u64 mine = ((u64)(unsigned)c << 32) | (u64)(0xFFFFFFFFu - (unsigned)idx);
#pragma unroll
        for (int k = 0; k < PP_SLOTS; ++k) best[k] = (k == s && mine > best[k]) ? mine : best[k];
    }
#pragma unroll
    for (int k = 0; k < PP_SLOTS; ++k) {
        u64 b = best[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(b, o, 64);
            b = other > b ? other : b;
        }
        if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6][k] = b;
    }
    __syncthreads();
    if (threadIdx.x < PP_SLOTS) {
        u64 b = wbest[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < PP_BLOCK / 64; ++w) b = wbest[w][threadIdx.x] > b ? wbest[w][threadIdx.x] : b;
        partial[(size_t)blockIdx.x * PP_SLOTS + threadIdx.x] = b;
    }
}

// One block: thread t takes slot t % 16 of the rows t / 16, t / 16 + 16, ...; LDS joins the 16 threads of a slot.  Writes all 16 keys.
__global__ void __launch_bounds__(PP_BLOCK) pp_select_final_kernel(const u64* __restrict__ partial, u64* __restrict__ keys, int rows) {
    __shared__ u64 col[PP_BLOCK / PP_SLOTS][PP_SLOTS];
    const int k = threadIdx.x % PP_SLOTS, g = threadIdx.x / PP_SLOTS;
    u64 b = 0;
    for (int r = g; r < rows; r += PP_BLOCK / PP_SLOTS) {
        const u64 v = partial[(size_t)r * PP_SLOTS + k];
        b = v > b ? v : b;
    }
    col[g][k] = b;
    __syncthreads();
    if (threadIdx.x < PP_SLOTS) {
        u64 m = col[0][threadIdx.x];
        for (int j = 1; j < PP_BLOCK / PP_SLOTS; ++j) m = col[j][threadIdx.x] > m ? col[j][threadIdx.x] : m;
        keys[threadIdx.x] = m;
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_write_largest_kernel(const int* __restrict__ label, const int* __restrict__ roots,
                                                                    const u64* __restrict__ keys, int* __restrict__ out, int nkeys,
                                                                    size_t n) {
    for (size_t idx = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * PP_BLOCK) {
        const int r = roots[idx];
        bool keep = r < 0;                                                                  // not one of the classes: copied
        // representatives are voxel indices, so a voxel can only equal the winner of its own class (a slot without voxels: key 0, -1)
        for (int k = 0; k < nkeys; ++k) keep |= (r == (int)(0xFFFFFFFFu - (unsigned)keys[k]) && (keys[k] >> 32) != 0);
        out[idx] = keep ? label[idx] : 0;
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_write_threshold_kernel(const int* __restrict__ label, const int* __restrict__ roots,
                                                                      const int* __restrict__ sizes, int* __restrict__ out, size_t n,
                                                                      double volume, double voxel_volume) {
    for (size_t idx = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * PP_BLOCK) {
        const int r = roots[idx];
        out[idx] = (r < 0 || (double)sizes[r] * voxel_volume > volume) ? label[idx] : 0;
    }
}

// One thread per voxel of the six faces (edges and corners come up more than once: the stores are of equal value).
__global__ void __launch_bounds__(PP_BLOCK) pp_faces_kernel(const int* __restrict__ roots, unsigned char* flags, int X, int Y, int Z) {
    const size_t fx = (size_t)Y * Z, fy = (size_t)X * Z, fz = (size_t)X * Y, total = 2 * (fx + fy + fz);
    for (size_t i = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * PP_BLOCK) {
        size_t j = i;
        int x, y, z;
        if (j < 2 * fx) {
            x = j < fx ? 0 : X - 1;
            j -= j < fx ? 0 : fx;
            y = (int)(j / (size_t)Z); z = (int)(j % (size_t)Z);
        } else if ((j -= 2 * fx) < 2 * fy) {
            y = j < fy ? 0 : Y - 1;
            j -= j < fy ? 0 : fy;
            x = (int)(j / (size_t)Z); z = (int)(j % (size_t)Z);
        } else {
            j -= 2 * fy;
            z = j < fz ? 0 : Z - 1;
            j -= j < fz ? 0 : fz;
            x = (int)(j / (size_t)Y); y = (int)(j % (size_t)Y);
        }
        const int r = roots[((size_t)x * Y + y) * Z + z];
        if (r >= 0) flags[r] = 1;
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_write_fill_kernel(const int* __restrict__ label, const int* __restrict__ roots,
                                                                 const unsigned char* __restrict__ flags, int* __restrict__ out, int klass,
                                                                 size_t n) {
    for (size_t idx = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * PP_BLOCK) {
        const int lab = label[idx];
        int o = lab;
        if (lab == 0) {                                       // (klass != 0: a background voxel is in the complement and has a root)
            const int r = roots[idx];
            if (r >= 0 && !flags[r]) o = klass;
        }
        out[idx] = o;
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_not_bits_kernel(const u64* __restrict__ bits, u64* __restrict__ out, int W, u64 last_mask,
                                                               size_t words) {
    for (size_t i = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; i < words; i += (size_t)gridDim.x * PP_BLOCK) {
        const bool last = (int)(i % (size_t)W) == W - 1;
        out[i] = ~bits[i] & (last ? last_mask : ~0ull);
    }
}

__global__ void __launch_bounds__(PP_BLOCK) pp_apply_bits_kernel(const int* __restrict__ label, const u64* __restrict__ bits,
                                                                 int* __restrict__ out, int klass, int C, int W, size_t n) {
    for (size_t i = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * PP_BLOCK) {
        const size_t row = i / (size_t)C;
        const int c = (int)(i - row * (size_t)C);
        const bool m = ((bits[row * (size_t)W + (size_t)(c >> 6)] >> (c & 63)) & 1) != 0;
        const int lab = label[i];
        out[i] = (m && lab == 0) ? klass : (lab == klass && !m) ? 0 : lab;
    }
}

inline int pp_blocks(size_t units) {
    size_t b = (units + PP_BLOCK - 1) / PP_BLOCK;
    return (int)(b < 1 ? 1 : b > PP_MAXBLK ? PP_MAXBLK : b);
}

// 0 and the voxel count, VNET_E_BADARG on a size < 1, VNET_E_UNSUPPORTED when an int32 cannot index the volume
inline int pp_count(int X, int Y, int Z, size_t& n) {
    if (X < 1 || Y < 1 || Z < 1) return VNET_E_BADARG;
    n = (size_t)X * (size_t)Y * (size_t)Z;
    return n > (size_t)INT_MAX ? VNET_E_UNSUPPORTED : 0;
}

// the class rule of a host array: 1 .. 16 distinct non-zero values
inline int pp_rule(const int* values, int nvalues, Rule& r) {
    if (!values || nvalues < 1 || nvalues > VNET_POST_MAX_VALUES) return VNET_E_BADARG;
    r = Rule{};
    for (int k = 0; k < nvalues; ++k) {
        if (values[k] == 0) return VNET_E_BADARG;
        for (int j = 0; j < k; ++j)
            if (values[j] == values[k]) return VNET_E_BADARG;
        r.v[k] = values[k];
    }
    r.n = nvalues;
    return 0;
}

// init, link, flatten (+ count when sizes is given) on `roots`
inline int pp_label(const int* label, int* roots, int* sizes, unsigned char* flags, const Rule& rule, size_t n, int Y, int Z,
                    hipStream_t st) {
    const dim3 grid(pp_blocks(n)), block(PP_BLOCK);
    if (int e = launch<pp_init_kernel>(grid, block, 0, st, label, roots, sizes, flags, rule, n, Z)) return e;
    if (int e = launch<pp_link_kernel>(grid, block, 0, st, label, roots, rule, n, Y, Z)) return e;
    return launch<pp_flatten_kernel>(grid, block, 0, st, roots, sizes, n);
}

inline bool pp_bad_ws(const void* ws) { return !ws || (reinterpret_cast<uintptr_t>(ws) & 7); }

// scratch of vnet_post_filter_components: the keys, a row of keys per block of the selection, roots and sizes
inline size_t pp_filter_ws(size_t n) { return PP_HEAD + (size_t)pp_blocks(n) * PP_HEAD + 8 * n; }

}  // namespace

extern "C" {

int vnet_post_class_roots(const int* label, const int* values, int nvalues, int* roots, int* sizes, int X, int Y, int Z, void* stream) {
    size_t n = 0;
    Rule rule{};
    if (!label || !roots) return VNET_E_BADARG;
    if (int e = pp_rule(values, nvalues, rule)) return e;
    if (int e = pp_count(X, Y, Z, n)) return e;
    return pp_label(label, roots, sizes, nullptr, rule, n, Y, Z, (hipStream_t)stream);
}

size_t vnet_post_filter_components_ws_bytes(int X, int Y, int Z) {
    size_t n = 0;
    return pp_count(X, Y, Z, n) ? 0 : pp_filter_ws(n);
}

int vnet_post_filter_components(const int* label, int* out, const int* values, int nvalues, int mode, double volume, double voxel_volume,
                                int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream) {
    size_t n = 0;
    Rule rule{};
    if (!label || !out || pp_bad_ws(ws) || (mode != 0 && mode != 1)) return VNET_E_BADARG;
    if (mode == 1 && (!isfinite(volume) || !isfinite(voxel_volume))) return VNET_E_BADARG;
    if (int e = pp_rule(values, nvalues, rule)) return e;
    if (int e = pp_count(X, Y, Z, n)) return e;
    if (ws_bytes < pp_filter_ws(n)) return VNET_E_WORKSPACE;
    const dim3 grid(pp_blocks(n)), block(PP_BLOCK);
    u64* keys = static_cast<u64*>(ws);
    u64* partial = keys + PP_SLOTS;
    int* roots = reinterpret_cast<int*>(partial + (size_t)grid.x * PP_SLOTS);
    int* sizes = roots + n;
    hipStream_t st = (hipStream_t)stream;
    if (int e = pp_label(label, roots, sizes, nullptr, rule, n, Y, Z, st)) return e;
    if (mode == 1)
        return launch<pp_write_threshold_kernel>(grid, block, 0, st, label, (const int*)roots, (const int*)sizes, out, n, volume, voxel_volume);
    if (int e = launch<pp_select_partial_kernel>(grid, block, 0, st, label, (const int*)sizes, partial, rule, n)) return e;
    if (int e = launch<pp_select_final_kernel>(dim3(1), block, 0, st, (const u64*)partial, keys, (int)grid.x)) return e;
    return launch<pp_write_largest_kernel>(grid, block, 0, st, label, (const int*)roots, (const u64*)keys, out, nvalues, n);
}

size_t vnet_post_fill_holes_ws_bytes(int X, int Y, int Z) {
    size_t n = 0;
    return pp_count(X, Y, Z, n) ? 0 : 5 * n;
}

int vnet_post_fill_holes(const int* label, int* out, int klass, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream) {
    size_t n = 0;
    if (!label || !out || pp_bad_ws(ws) || klass == 0) return VNET_E_BADARG;
    if (int e = pp_count(X, Y, Z, n)) return e;
    if (ws_bytes < 5 * n) return VNET_E_WORKSPACE;
    Rule rule{};
    rule.v[0] = klass;                                        // n == 0: the complement rule
    int* roots = static_cast<int*>(ws);
    unsigned char* flags = reinterpret_cast<unsigned char*>(roots + n);
    hipStream_t st = (hipStream_t)stream;
    if (int e = pp_label(label, roots, nullptr, flags, rule, n, Y, Z, st)) return e;
    const size_t faces = 2 * ((size_t)Y * Z + (size_t)X * Z + (size_t)X * Y);
    if (int e = launch<pp_faces_kernel>(dim3(pp_blocks(faces)), dim3(PP_BLOCK), 0, st, (const int*)roots, flags, X, Y, Z)) return e;
    return launch<pp_write_fill_kernel>(dim3(pp_blocks(n)), dim3(PP_BLOCK), 0, st, label, (const int*)roots, (const unsigned char*)flags, out,
                                        klass, n);
}

int vnet_post_not_bits(const long long* bits, long long* out, int A, int B, int C, void* stream) {
    size_t n = 0;
    if (!bits || !out || bits == out) return VNET_E_BADARG;
    if (int e = pp_count(A, B, C, n)) return e;
    const int W = (C + 63) / 64;
    const size_t words = (size_t)A * (size_t)B * (size_t)W;
    const u64 last_mask = (C & 63) ? ((1ull << (C & 63)) - 1ull) : ~0ull;
    return launch<pp_not_bits_kernel>(dim3(pp_blocks(words)), dim3(PP_BLOCK), 0, (hipStream_t)stream, reinterpret_cast<const u64*>(bits),
                                      reinterpret_cast<u64*>(out), W, last_mask, words);
}

int vnet_post_apply_bits(const int* label, const long long* bits, int klass, int* out, int A, int B, int C, void* stream) {
    size_t n = 0;
    if (!label || !bits || !out || klass == 0) return VNET_E_BADARG;
    if (int e = pp_count(A, B, C, n)) return e;
    return launch<pp_apply_bits_kernel>(dim3(pp_blocks(n)), dim3(PP_BLOCK), 0, (hipStream_t)stream, label, reinterpret_cast<const u64*>(bits),
                                        out, klass, C, (C + 63) / 64, n);
}

}  // extern "C"
