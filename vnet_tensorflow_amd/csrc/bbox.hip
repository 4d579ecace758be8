// bbox.hip -- the device side of the bounding-box tool (csrc/vnet_bbox.h; reference utils/bounding_box/bbox.py: ExtractImageFilter per
// slice, ConnectedComponentImageFilter + LabelShapeStatisticsImageFilter per slice and class, a matplotlib picture per slice), gfx950.
//   vnet_slice_stack_* : [X,Y,Z] -> [S,V,U], a permutation that moves the fastest axis.  For a fixed third index it is a matrix
//                        transpose: a workgroup stages a 64 x 64 tile of 4-byte words through LDS, reads rows contiguous in z -- 64
//                        lanes on 64 consecutive words -- and writes rows contiguous in u.  The LDS row pitch is 65 words: a write
//                        or a 4-byte read takes bank (word index) mod 32 per 32-lane half; the lanes of a half hold 32 consecutive
//                        columns on the way in (banks c .. c + 31) and 32 consecutive rows on the way out (pitch 65 = 1 mod 32: banks
//                        r .. r + 31): no conflict either way.  Tiles are dealt to at most BB_MAXBLK workgroups in a loop.
//   vnet_plane_cc_table: the union-find of components.hip (cc_union.h) with a rule that stays inside a slice and separates classes:
//                        init links runs of one positive value along u inside one row, link unites a voxel with its v - 1 neighbour
//                        of equal value, nothing links across s; flatten-and-count is cc_union.h's, the count / scan / rank / box
//                        launches are cc_table.h's on the stack as a volume (S, V, U).
//   vnet_bbox_render   : one thread per pixel, a workgroup inside one slice; the slice's boxes pass through LDS in chunks of BB_CHUNK.
// No thread ever waits for another: every loop below is a counted loop or strictly decreases an index (the argument stands at each).
// The cross-XCD argument of DESIGN.md section 6c carries over unchanged: the parent words, the atomics and their scopes are the same.
// Voxel indices are int32 (n <= 2^31 - 1, checked on the host); element offsets are 64-bit.
#include <limits.h>
#include "common.h"
#include "cc_union.h"
#include "cc_table.h"
#include "vnet_bbox.h"

namespace {

constexpr int BB_BLOCK = 256, BB_MAXBLK = 4096;
constexpr int BT = 64, BPITCH = BT + 1, BROWS = BB_BLOCK / 64, BTRIPS = BT / BROWS;
constexpr int BB_CHUNK = 256;                        // boxes of a slice held in LDS at a time (5 words each)

typedef long long i64;

// 0 and the voxel count, VNET_E_BADARG on a size < 1, VNET_E_UNSUPPORTED when an int32 cannot index the volume
inline int bb_count(int A, int B, int C, size_t& n) {
    if (A < 1 || B < 1 || C < 1) return VNET_E_BADARG;
    n = (size_t)A * (size_t)B * (size_t)C;
    return n > (size_t)INT_MAX ? VNET_E_UNSUPPORTED : 0;
}

inline int bb_blocks(size_t units) {
    size_t b = (units + BB_BLOCK - 1) / BB_BLOCK;
    return (int)(b < 1 ? 1 : b > BB_MAXBLK ? BB_MAXBLK : b);
}

// ---- slice stack ----------------------------------------------------------------------------------------------------------------
// A tile transposes (a, z) for a fixed b: word a * sa + b * sb + z of the source goes to word z * dz + b * db + a of the destination.
struct StackP {
    const unsigned* src;
    unsigned* dst;
    i64 tiles;          // NB * ta_n * tz_n
    i64 sa, sb, dz, db;
    int ta_n, tz_n;
    int NA, Z;
};

__global__ void __launch_bounds__(BB_BLOCK) slice_stack_kernel(StackP p) {
    __shared__ unsigned tile[BT * BPITCH];
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    // bounded: a counted loop over the tiles, the same trips for every thread of a workgroup (the barriers inside are uniform)
    for (i64 t = blockIdx.x; t < p.tiles; t += gridDim.x) {
        const int tz = (int)(t % p.tz_n);
        const i64 rest = t / p.tz_n;
        const int ta = (int)(rest % p.ta_n);
        const i64 b = rest / p.ta_n;
        const int a0 = ta * BT, z0 = tz * BT;
        // in: lane lo reads column z0 + lo of rows a0 + hi, + BROWS, ...
        {
            const int z = z0 + lo;
            if (z < p.Z) {
#pragma unroll
                for (int k = 0; k < BTRIPS; ++k) {
                    const int al = hi + BROWS * k, a = a0 + al;
                    if (a < p.NA) tile[al * BPITCH + lo] = p.src[(size_t)(a * p.sa + b * p.sb + z)];
                }
            }
        }
        __syncthreads();
        // out: lane lo writes element a0 + lo of the rows z0 + hi, + BROWS, ...
        {
            const int a = a0 + lo;
            if (a < p.NA) {
#pragma unroll
                for (int k = 0; k < BTRIPS; ++k) {
                    const int zl = hi + BROWS * k, z = z0 + zl;
                    if (z < p.Z) p.dst[(size_t)(z * p.dz + b * p.db + a)] = tile[lo * BPITCH + zl];
                }
            }
        }
        __syncthreads();
    }
}

int stack_run(const void* src, void* dst, int X, int Y, int Z, int axis, void* stream) {
    size_t n = 0;
    if (!src || !dst || axis < 0 || axis > 2) return VNET_E_BADARG;
    if (int e = bb_count(X, Y, Z, n)) return e;
    StackP p;
    p.src = static_cast<const unsigned*>(src); p.dst = static_cast<unsigned*>(dst);
    p.Z = Z;
    i64 NB;
    if (axis == 0) {            // a = y, b = x: dst[(x * Z + z) * Y + y]
        p.NA = Y; NB = X; p.sa = Z; p.sb = (i64)Y * Z; p.dz = Y; p.db = (i64)Z * Y;
    } else {                    // a = x, b = y
        p.NA = X; NB = Y; p.sa = (i64)Y * Z; p.sb = Z;
        if (axis == 2) { p.dz = (i64)Y * X; p.db = X; }         // dst[(z * Y + y) * X + x]
        else           { p.dz = X; p.db = (i64)Z * X; }         // dst[(y * Z + z) * X + x]
    }
    p.ta_n = (p.NA + BT - 1) / BT;
    p.tz_n = (Z + BT - 1) / BT;
    p.tiles = NB * p.ta_n * p.tz_n;
    const int grid = (int)(p.tiles < BB_MAXBLK ? p.tiles : BB_MAXBLK);
    return launch<slice_stack_kernel>(dim3(grid), dim3(BB_BLOCK), 0, (hipStream_t)stream, p);
}

// ---- components inside a slice, one class each --------------------------------------------------------------------------------------
// In the kernels with wave-wide votes the loop runs on the block's base index, so that all 64 lanes of a wave make every trip together
// and lane l of a wave holds voxel (wave's first voxel) + l.
// init: parent[v] = first voxel of v's run of equal positive values along u inside this wave (or the voxel in front of the wave when
// the run started earlier, in the same row by construction), -1 on the background; the counts are zeroed here, by the kernel.
__global__ void __launch_bounds__(BB_BLOCK) plane_init_kernel(const int* __restrict__ stack, int* __restrict__ parent, int* __restrict__ sizes,
                                                              size_t n, int U) {
    const int lane = threadIdx.x & 63;
    // bounded: a counted grid-stride loop; nothing inside it loops
    for (size_t base = (size_t)blockIdx.x * BB_BLOCK; base < n; base += (size_t)gridDim.x * BB_BLOCK) {
        const size_t idx = base + threadIdx.x;
        const bool valid = idx < n;
        const int u = valid ? (int)((unsigned)idx % (unsigned)U) : 0;
        const int l = valid ? stack[idx] : 0;
        const bool fg = l > 0;
        // the value in front of this voxel in its row: the lane below, or for lane 0 a load (u > 0: idx - 1 is in the same row)
        const int below_l = __shfl_up(l, 1, 64);
        const int prev = lane ? below_l : (valid && u > 0 ? stack[idx - 1] : 0);
        const bool start = fg && (u == 0 || prev != l);
        const u64 mst = __ballot(start);
        if (valid) {
            int p = -1;
            if (fg) {
                // a foreground lane that starts no run continues the lane below it (same row, same value): with no run start at or
                // below this lane every lane from 0 up to it continues, and the run began in front of the wave
                const u64 below = mst & ((2ull << lane) - 1ull);                       // run starts at lanes <= this one
                p = below ? (int)idx - (lane - (63 - __clzll((long long)below)))       // the nearest one starts this voxel's run
                          : (int)idx - lane - 1;                                       // chain on to the voxel in front of the wave
            }
            parent[idx] = p;
            sizes[idx] = 0;
        }
    }
}

// link: a voxel and its v - 1 neighbour of equal value.  Nothing links across s: at v == 0 the voxel idx - U is another slice's.
__global__ void __launch_bounds__(BB_BLOCK) plane_link_kernel(const int* __restrict__ stack, int* parent, size_t n, int V, int U) {
    // bounded: a counted grid-stride loop; cc_unite inside it is bounded on its own (cc_union.h)
    for (size_t idx = (size_t)blockIdx.x * BB_BLOCK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * BB_BLOCK) {
        const int l = stack[idx];
        if (l <= 0) continue;
        const unsigned row = (unsigned)idx / (unsigned)U;
        const int u = (int)((unsigned)idx - row * (unsigned)U), v = (int)(row % (unsigned)V);
        if (v == 0 || stack[idx - U] != l) continue;
        // (u - 1 and the voxel above it both of this value: the two run links are the init pass's and the link above is made at u - 1)
        if (u > 0 && stack[idx - 1] == l && stack[idx - U - 1] == l) continue;
        cc_unite(parent, (int)idx - U, (int)idx);
    }
}

__global__ void __launch_bounds__(BB_BLOCK) plane_flatten_kernel(int* parent, int* sizes, size_t n) {
    cc_flatten_body<BB_BLOCK>(parent, sizes, n);
}

// ---- render ---------------------------------------------------------------------------------------------------------------------
__constant__ unsigned char BB_PALETTE[8][3] = {{255, 0, 0}, {0, 255, 255}, {0, 255, 0}, {255, 255, 0},
                                               {255, 0, 255}, {255, 128, 0}, {0, 128, 255}, {255, 255, 255}};

struct RenderP {
    const float* image;
    const int* label;
    const int* boxes;
    const int* first;
    unsigned char* rgb;
    i64 units;          // S * per
    int per;            // workgroups' worth of pixels in a slice
    int VU, U;
    float wmin, wmax, scale;
    int alpha;
};

// No multiply-add pair: a subtraction, then a product, each rounded once whatever the contraction setting is.
__device__ __forceinline__ unsigned grey_of(float v, float wmin, float wmax, float scale) {
    if (v != v) return 0u;
    if (wmax == wmin) return v < wmin ? 0u : 255u;
    const float t = (v - wmin) * scale;
    if (!(t > 0.0f)) return 0u;
    if (t >= 255.0f) return 255u;
    return (unsigned)t;
}

__global__ void __launch_bounds__(BB_BLOCK) render_kernel(RenderP p) {
    __shared__ int box[BB_CHUNK * 5];
    // bounded: a counted loop over (slice, pixel chunk) units, the same trips for every thread of a workgroup
    for (i64 t = blockIdx.x; t < p.units; t += gridDim.x) {
        const int s = (int)(t / p.per);
        const i64 pix = (t % p.per) * BB_BLOCK + threadIdx.x;                      // (64-bit: the last chunk may reach past 2^31 - 1)
        const bool valid = pix < p.VU;
        const int v = valid ? (int)pix / p.U : 0, u = valid ? (int)pix - v * p.U : 0;
        const int b0 = p.first[s], b1 = p.boxes ? p.first[s + 1] : b0;
        int hit = 0;
        bool on = false;
        // bounded: c grows by BB_CHUNK up to b1, a value every thread of the workgroup read from the same word
        for (int c = b0; c < b1; c += BB_CHUNK) {
            const int cnt = b1 - c < BB_CHUNK ? b1 - c : BB_CHUNK;
            for (int i = threadIdx.x; i < cnt * 5; i += BB_BLOCK) box[i] = p.boxes[(size_t)c * 5 + i];
            __syncthreads();
            if (valid) {
                for (int j = 0; j < cnt; ++j) {                                       // (every lane reads the same word: a broadcast)
                    const int x = box[5 * j], y = box[5 * j + 1], w = box[5 * j + 2], h = box[5 * j + 3];
                    const bool edge = ((u == x || u == x + w) && y <= v && v <= y + h) || ((v == y || v == y + h) && x <= u && u <= x + w);
                    if (edge) { on = true; hit = box[5 * j + 4]; }                     // later boxes win
                }
            }
            __syncthreads();
        }
        if (valid) {
            const size_t o = (size_t)s * p.VU + (size_t)pix;
            unsigned r, g, b;
            if (on) {
                const unsigned char* c = BB_PALETTE[(hit - 1) & 7];
                r = c[0]; g = c[1]; b = c[2];
            } else {
                const unsigned grey = grey_of(p.image[o], p.wmin, p.wmax, p.scale);
                const int l = p.label[o];
                r = g = b = grey;
                if (l > 0) {
                    const unsigned char* c = BB_PALETTE[(l - 1) & 7];
                    const unsigned a = (unsigned)p.alpha, base = grey * (256u - a) + 128u;
                    r = (base + c[0] * a) >> 8; g = (base + c[1] * a) >> 8; b = (base + c[2] * a) >> 8;
                }
            }
            p.rgb[3 * o] = (unsigned char)r;
            p.rgb[3 * o + 1] = (unsigned char)g;
            p.rgb[3 * o + 2] = (unsigned char)b;
        }
    }
}

}  // namespace

extern "C" {

int vnet_slice_stack_f32(const float* src, float* dst, int X, int Y, int Z, int axis, void* stream) {
    return stack_run(src, dst, X, Y, Z, axis, stream);
}

int vnet_slice_stack_i32(const int* src, int* dst, int X, int Y, int Z, int axis, void* stream) {
    return stack_run(src, dst, X, Y, Z, axis, stream);
}

size_t vnet_plane_cc_table_ws_bytes(int S, int V, int U) {
    size_t n = 0;
    return bb_count(S, V, U, n) ? 0 : cc_table_bytes(n);
}

int vnet_plane_cc_table(const int* stack, int* n_out, int* table, int max_components, int S, int V, int U,
                        void* ws, size_t ws_bytes, void* stream) {
    size_t n = 0;
    if (!stack || !n_out || !table || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || max_components < 1) return VNET_E_BADARG;
    if (int e = bb_count(S, V, U, n)) return e;
    if ((size_t)max_components > (size_t)INT_MAX / VNET_CC_ROW) return VNET_E_UNSUPPORTED;
    if (ws_bytes < cc_table_bytes(n)) return VNET_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    TableP p{};
    int* roots = cc_table_carve(p, ws, n, n_out, table, nullptr, max_components, V, U);
    const dim3 grid(bb_blocks(n)), block(BB_BLOCK);
    if (int e = launch<plane_init_kernel>(grid, block, 0, st, stack, roots, p.sizes, n, U)) return e;
    if (int e = launch<plane_link_kernel>(grid, block, 0, st, stack, roots, n, V, U)) return e;
    if (int e = launch<plane_flatten_kernel>(grid, block, 0, st, roots, p.sizes, n)) return e;
    return cc_table_passes<false>(p, st);
}

int vnet_bbox_render(const float* image, const int* label, const int* boxes, const int* first, unsigned char* rgb,
                     int S, int V, int U, float wmin, float wmax, float scale, int alpha256, void* stream) {
    size_t n = 0;
    if (!image || !label || !first || !rgb || alpha256 < 0 || alpha256 > 256) return VNET_E_BADARG;
    if (int e = bb_count(S, V, U, n)) return e;
    RenderP p;
    p.image = image; p.label = label; p.boxes = boxes; p.first = first; p.rgb = rgb;
    p.VU = V * U; p.U = U;
    p.per = (p.VU + BB_BLOCK - 1) / BB_BLOCK;
    p.units = (i64)S * p.per;
    p.wmin = wmin; p.wmax = wmax; p.scale = scale; p.alpha = alpha256;
    const int grid = (int)(p.units < BB_MAXBLK ? p.units : BB_MAXBLK);
    return launch<render_kernel>(dim3(grid), dim3(BB_BLOCK), 0, (hipStream_t)stream, p);
}

}  // extern "C"
