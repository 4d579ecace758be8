// surface.hip -- the surface-distance scores of Batch_Evaluate on the device (csrc/vnet_surface.h, part of libvnet_hip.so), gfx950.
//   vnet_surface_bits   : one wave per word: lane k reads voxel z = 64 w + k of row (x, y) and its four in-plane neighbours, five ballots
//                         are the class mask's word and its neighbour rows' words; the two z neighbours come from the word itself
//                         shifted by one bit, the bits carried in from words w - 1 and w + 1 read by lanes 0 and 1 (a sixth ballot).
//                         Lanes at z >= Z vote 0, which keeps the unused high bits zero and makes the volume's edge "outside".
//   vnet_edt2           : z pass, one wave per word: the nearest set bit at or below and at or above every voxel by clz / ctz on the
//                         row's words, |dz| as int32 (NONE when the row has no bit).  y and x passes, one thread per voxel in flat
//                         order, so the lanes of a wave run along z and every load of a candidate is one contiguous segment: a voxel
//                         walks outward from its own index, d = 1, 2, ..., and stops once fl(s2 d^2) >= best -- the term added to it
//                         is >= 0 and fl(a + t) is monotone, so nothing further out can win; a wave leaves when all its lanes have
//                         stopped.  With best = +inf the walk spans the whole axis.  The candidates are read through the caches, not
//                         staged in LDS: a (row, 64 z) slab of fp64 candidates is 512 bytes per index, 1 MiB at the axis cap, and
//                         the slab a block walks (Y * 512 bytes) stays in L2 as it is.
//   vnet_surface_gather : stream compaction over the mask's words in flat order (= voxel order): popcounts per chunk of words -> one
//                         wave scans the chunk sums -> a block per chunk scans its words tile by tile and every thread writes the
//                         values of its word's bits; a last kernel zeroes list[min(n, cap):].
//   vnet_list_select    : the rank-k element on the uint64 patterns, bit by bit from bit 62 down: a pass counts, per rank, the elements
//                         that share the prefix found so far and have the bit clear (ballot + popcount per wave, one fixed slot per
//                         block), a one-block kernel adds the slots and moves prefix and rank.  63 passes, no host round trip.
//   vnet_list_root_sum  : per-thread strided sums of sqrt, butterfly per wave, fixed-slot partials per block, one workgroup adds them.
// No read-modify-write on memory anywhere: every result is the same from launch to launch.
// Voxel counts fit an int32 (checked on the host); word, element and byte offsets are size_t.
// Every fp64 operation is rounded once: contraction is off for this translation unit (the `==` tiers of the tests rest on it).
#include <math.h>
#include <limits.h>
#include "common.h"
#include "vnet_surface.h"

#pragma clang fp contract(off)

namespace {

constexpr int PB = 256, PW = PB / 64, MAXK = VNET_SURFACE_MAX_RANKS, MAX_AXIS = VNET_SURFACE_MAX_AXIS, NONE = INT_MAX, TOP_BIT = 62;
constexpr int BITS_CAP = 4096;          // blocks of the wave-per-word kernels (vnet_surface_bits, the z pass)
constexpr int EDT_CAP = 2048;           // blocks of the y and x passes
constexpr int GATHER_CAP = 1024;        // chunks of the compaction, one block each
constexpr int LIST_CAP = 1024;          // blocks of the list kernels: the fixed slots of their partial sums

typedef unsigned long long u64;
typedef long long i64;

inline int blocks_for(size_t units, int cap) {
    size_t b = (units + PB - 1) / PB;
    return (int)(b < 1 ? 1 : b > (size_t)cap ? (size_t)cap : b);
}

// X * Y * Z as n; VNET_E_BADARG / VNET_E_UNSUPPORTED
inline int volume_count(int X, int Y, int Z, size_t& n) {
    if (X < 1 || Y < 1 || Z < 1) return VNET_E_BADARG;
    n = (size_t)X * (size_t)Y * (size_t)Z;
    return (n > (size_t)INT_MAX || X > MAX_AXIS || Y > MAX_AXIS || Z > MAX_AXIS) ? VNET_E_UNSUPPORTED : 0;
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 7) != 0; }

__device__ __forceinline__ i64 wave_sum_i(i64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- surface ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void surface_bits_kernel(const int* __restrict__ label, u64* __restrict__ bits, int klass,
                                                          int X, int Y, int Z, int W, size_t words) {
    const int lane = threadIdx.x & 63;
    const size_t step = (size_t)gridDim.x * PW, plane = (size_t)Y * (size_t)Z;
    auto member = [klass](int v) { return klass == 0 ? v != 0 : v == klass; };
    for (size_t idx = (size_t)blockIdx.x * PW + (threadIdx.x >> 6); idx < words; idx += step) {      // (wave-uniform)
        const size_t row = idx / (size_t)W;
        const int w = (int)(idx - row * (size_t)W), x = (int)(row / (size_t)Y), y = (int)(row - (size_t)x * (size_t)Y), z = w * 64 + lane;
        const int* r = label + row * (size_t)Z;
        bool m = false, xm = false, xp = false, ym = false, yp = false, e = false;
        if (z < Z) {
            m = member(r[z]);
            xm = x > 0 && member(*(r + z - plane));
            xp = x + 1 < X && member(*(r + z + plane));
            ym = y > 0 && member(*(r + z - (size_t)Z));
            yp = y + 1 < Y && member(*(r + z + (size_t)Z));
        }
        if (lane == 0 && w > 0) e = member(r[w * 64 - 1]);
        if (lane == 1 && w * 64 + 64 < Z) e = member(r[w * 64 + 64]);
        const u64 M = __ballot(m), XM = __ballot(xm), XP = __ballot(xp), YM = __ballot(ym), YP = __ballot(yp), E = __ballot(e);
        const u64 below = (M << 1) | (E & 1ull), above = (M >> 1) | ((E >> 1) << 63);
        if (lane == 0) bits[idx] = M & ~(XM & XP & YM & YP & below & above);
    }
}

// ---- distance field ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void edt_z_kernel(const u64* __restrict__ bits, int* __restrict__ dz, int Z, int W, size_t words) {
    const int lane = threadIdx.x & 63;
    const size_t step = (size_t)gridDim.x * PW;
    for (size_t idx = (size_t)blockIdx.x * PW + (threadIdx.x >> 6); idx < words; idx += step) {
        const size_t row = idx / (size_t)W;
        const int w = (int)(idx - row * (size_t)W), z = w * 64 + lane;
        const u64* r = bits + row * (size_t)W;
        const u64 word = r[w], lo = word & ((2ull << lane) - 1ull), hi = word & (~0ull << lane);      // the bits at or below / above z
        int zl = -1, zr = -1;
        if (lo) zl = w * 64 + 63 - __clzll((i64)lo);
        else
            for (int v = w - 1; v >= 0; --v) {
                const u64 t = r[v];
                if (t) { zl = v * 64 + 63 - __clzll((i64)t); break; }
            }
        if (hi) zr = w * 64 + __ffsll((i64)hi) - 1;
        else
            for (int v = w + 1; v < W; ++v) {
                const u64 t = r[v];
                if (t) { zr = v * 64 + __ffsll((i64)t) - 1; break; }
            }
        if (z < Z) {
            int d = NONE;
            if (zl >= 0) d = z - zl;
            if (zr >= 0) d = min(d, zr - z);
            dz[row * (size_t)Z + (size_t)z] = d;
        }
    }
}

// a candidate of the y pass: fl(s2z dz^2) from the z pass's int32, +inf for a row without a bit; of the x pass: the y pass's fp64
__device__ __forceinline__ double candidate(const int* src, size_t i, double s2z) {
    const int d = src[i];
    return d == NONE ? (double)INFINITY : s2z * (double)(d * d);
}
__device__ __forceinline__ double candidate(const double* src, size_t i, double) { return src[i]; }

// dst[o, a, j] = min over a' of fl(fl(s2 (a - a')^2) + candidate[o, a', j]) on a volume seen as [outer, A, inner]
template <typename S>
__global__ __launch_bounds__(PB) void edt_axis_kernel(const S* __restrict__ src, double* __restrict__ dst, double s2z, double s2,
                                                      int A, size_t inner, size_t n) {
    const size_t step = (size_t)gridDim.x * PB;
    for (size_t base = (size_t)blockIdx.x * PB; base < n; base += step) {                             // (block-uniform)
        const size_t i = base + threadIdx.x;
        const bool live = i < n;
        int a = 0, reach = 0;
        double best = 0.0;
        if (live) {
            a = (int)((i / inner) % (size_t)A);
            reach = max(a, A - 1 - a);
            best = candidate(src, i, s2z);
        }
        for (int d = 1;; ++d) {
            double t = 0.0;
            bool go = false;
            if (d <= reach) {
                t = s2 * (double)(d * d);
                go = t < best;
            }
            if (!__any(go)) break;
            if (go) {
                if (a - d >= 0) {
                    const double c = t + candidate(src, i - (size_t)d * inner, s2z);
                    best = c < best ? c : best;
                }
                if (a + d < A) {
                    const double c = t + candidate(src, i + (size_t)d * inner, s2z);
                    best = c < best ? c : best;
                }
            }
        }
        if (live) dst[i] = best;
    }
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------------
// chunk c of the mask's words: [c * per, min((c + 1) * per, NW))
__global__ __launch_bounds__(PB) void gather_count_kernel(const u64* __restrict__ bits, i64* __restrict__ chunk_sum, size_t NW, size_t per) {
    __shared__ i64 part[PW];
    const size_t lo = (size_t)blockIdx.x * per, hi = lo + per < NW ? lo + per : NW;
    i64 c = 0;
    for (size_t q = lo + threadIdx.x; q < hi; q += PB) c += __popcll(bits[q]);
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 s = 0;
        for (int k = 0; k < PW; ++k) s += part[k];
        chunk_sum[blockIdx.x] = s;
    }
}

// one wave: lane l owns chunks [l * each, (l + 1) * each)
__global__ __launch_bounds__(64) void gather_scan_kernel(const i64* __restrict__ chunk_sum, i64* __restrict__ chunk_off, int nchunks,
                                                         i64* __restrict__ n_out) {
    const int lane = threadIdx.x, each = (nchunks + 63) / 64, lo = lane * each, hi = min(lo + each, nchunks);
    i64 mine = 0;
    for (int c = lo; c < hi; ++c) mine += chunk_sum[c];
    i64 inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const i64 v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    i64 acc = inc - mine;
    for (int c = lo; c < hi; ++c) {
        chunk_off[c] = acc;
        acc += chunk_sum[c];
    }
    if (lane == 63) n_out[0] = inc;
}

__global__ __launch_bounds__(PB) void gather_scatter_kernel(const double* __restrict__ d2, const u64* __restrict__ bits,
                                                            double* __restrict__ list, const i64* __restrict__ chunk_off, i64 cap,
                                                            size_t NW, size_t per, int W, int Z) {
    __shared__ int wave_total[PW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t lo = (size_t)blockIdx.x * per, hi = lo + per < NW ? lo + per : NW;
    i64 base = chunk_off[blockIdx.x];
    for (size_t t0 = lo; t0 < hi; t0 += PB) {                                                        // (block-uniform)
        const size_t q = t0 + threadIdx.x;
        u64 word = q < hi ? bits[q] : 0ull;
        const int c = __popcll(word);
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (lane >= o) inc += v;
        }
        if (lane == 63) wave_total[wv] = inc;
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < PW; ++k) {
            const int t = wave_total[k];
            if (k < wv) before += t;
            total += t;
        }
        if (word) {
            const size_t row = q / (size_t)W;
            const double* src = d2 + row * (size_t)Z + (q - row * (size_t)W) * 64;
            i64 pos = base + before + inc - c;
            while (word) {
                const int k = __ffsll((i64)word) - 1;
                word &= word - 1ull;
                if (pos < cap) list[pos] = src[k];
                ++pos;
            }
        }
        base += total;
        __syncthreads();                     // the next tile overwrites wave_total
    }
}

__global__ __launch_bounds__(PB) void zero_tail_kernel(double* __restrict__ list, const i64* __restrict__ n, i64 cap) {
    const i64 from = n[0] < cap ? n[0] : cap, step = (i64)gridDim.x * PB;
    for (i64 i = from + (i64)blockIdx.x * PB + threadIdx.x; i < cap; i += step) list[i] = 0.0;
}

// ---- select -----------------------------------------------------------------------------------------------------------------------------
struct SelState {
    u64 prefix[MAXK];        // the bits above the current one, found so far
    i64 k[MAXK];             // the rank among the elements that share the prefix
};

struct Ranks {
    i64 v[MAXK];
};

__global__ void select_init_kernel(SelState* st, Ranks ranks) {
    const int r = threadIdx.x;
    if (r < MAXK) {
        st->prefix[r] = 0ull;
        st->k[r] = ranks.v[r];
    }
}

__global__ __launch_bounds__(PB) void select_count_kernel(const u64* __restrict__ list, i64 n, const SelState* __restrict__ st,
                                                          i64* __restrict__ partial, int bit, int nk) {
    __shared__ i64 part[PW][MAXK];
    u64 prefix[MAXK];
    i64 cnt[MAXK];
#pragma unroll
    for (int r = 0; r < MAXK; ++r) {
        prefix[r] = st->prefix[r];
        cnt[r] = 0;
    }
    const i64 step = (i64)gridDim.x * PB;
    for (i64 base = (i64)blockIdx.x * PB; base < n; base += step) {                                   // (block-uniform)
        const i64 i = base + threadIdx.x;
        const bool live = i < n;
        const u64 v = live ? list[i] : 0ull;
        const bool clear = live && !((v >> bit) & 1ull);
#pragma unroll
        for (int r = 0; r < MAXK; ++r)
            if (r < nk) cnt[r] += __popcll(__ballot(clear && ((v ^ prefix[r]) >> (bit + 1)) == 0ull));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int r = 0; r < MAXK; ++r) part[threadIdx.x >> 6][r] = cnt[r];
    }
    __syncthreads();
    if (threadIdx.x < MAXK) {
        i64 s = 0;
        for (int k = 0; k < PW; ++k) s += part[k][threadIdx.x];
        partial[(size_t)blockIdx.x * MAXK + threadIdx.x] = s;
    }
}

// one block of MAXK waves: wave r adds rank r's slots, then moves its prefix and rank; after bit 0 the prefix is the element
__global__ __launch_bounds__(64 * MAXK) void select_step_kernel(const i64* __restrict__ partial, int nblocks, SelState* st, int bit,
                                                                int nk, double* __restrict__ out) {
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (r >= nk) return;
    i64 c0 = 0;
    for (int b = lane; b < nblocks; b += 64) c0 += partial[(size_t)b * MAXK + r];
    c0 = wave_sum_i(c0);
    if (lane == 0) {
        u64 prefix = st->prefix[r];
        i64 k = st->k[r];
        if (k >= c0) {
            prefix |= 1ull << bit;
            k -= c0;
        }
        st->prefix[r] = prefix;
        st->k[r] = k;
        if (bit == 0) out[r] = __longlong_as_double((i64)prefix);
    }
}

// ---- sum of roots -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_d(double v, double* part) {      // the result is thread 0's
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < PW; ++k) s += part[k];
    return s;
}

__global__ __launch_bounds__(PB) void root_partial_kernel(const double* __restrict__ list, i64 n, double* __restrict__ partial) {
    __shared__ double part[PW];
    const i64 step = (i64)gridDim.x * PB;
    double acc = 0.0;
    for (i64 i = (i64)blockIdx.x * PB + threadIdx.x; i < n; i += step) acc += sqrt(list[i]);
    const double s = block_sum_d(acc, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(PB) void root_final_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out) {
    __shared__ double part[PW];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += PB) acc += partial[b];
    const double s = block_sum_d(acc, part);
    if (threadIdx.x == 0) out[0] = s;
}

inline size_t gather_chunks(size_t NW) { return (size_t)blocks_for(NW, GATHER_CAP); }
inline bool spacing_ok(double s) { return s > 0.0 && s < (double)INFINITY; }

}  // namespace

extern "C" {

int vnet_surface_bits(const int* label, int klass, long long* bits, int X, int Y, int Z, void* stream) {
    size_t n = 0;
    if (!label || !bits || klass < 0 || misaligned(bits)) return VNET_E_BADARG;
    if (int e = volume_count(X, Y, Z, n)) return e;
    const int W = (Z + 63) / 64;
    const size_t words = (size_t)X * (size_t)Y * (size_t)W;
    return launch<surface_bits_kernel>(dim3(blocks_for(words * 64, BITS_CAP)), dim3(PB), 0, (hipStream_t)stream, label,
                                       reinterpret_cast<u64*>(bits), klass, X, Y, Z, W, words);
}

size_t vnet_edt2_ws_bytes(int X, int Y, int Z) {
    size_t n = 0;
    if (volume_count(X, Y, Z, n)) return 0;
    return align_up(n * sizeof(int), 8) + n * sizeof(double);
}

int vnet_edt2(const long long* bits, double* d2, double sx, double sy, double sz, int X, int Y, int Z,
              void* ws, size_t ws_bytes, void* stream) {
    size_t n = 0;
    if (!bits || !d2 || !ws || misaligned(bits) || misaligned(d2) || misaligned(ws) || !spacing_ok(sx) || !spacing_ok(sy) || !spacing_ok(sz))
        return VNET_E_BADARG;
    if (int e = volume_count(X, Y, Z, n)) return e;
    if (ws_bytes < vnet_edt2_ws_bytes(X, Y, Z)) return VNET_E_WORKSPACE;
    int* dz = static_cast<int*>(ws);
    double* g2 = reinterpret_cast<double*>(static_cast<char*>(ws) + align_up(n * sizeof(int), 8));
    const int W = (Z + 63) / 64;
    const size_t words = (size_t)X * (size_t)Y * (size_t)W;
    const double s2x = sx * sx, s2y = sy * sy, s2z = sz * sz;
    hipStream_t st = (hipStream_t)stream;
    if (int e = launch<edt_z_kernel>(dim3(blocks_for(words * 64, BITS_CAP)), dim3(PB), 0, st, reinterpret_cast<const u64*>(bits), dz, Z, W, words))
        return e;
    const dim3 grid(blocks_for(n, EDT_CAP));
    if (int e = launch<edt_axis_kernel<int>>(grid, dim3(PB), 0, st, (const int*)dz, g2, s2z, s2y, Y, (size_t)Z, n)) return e;
    return launch<edt_axis_kernel<double>>(grid, dim3(PB), 0, st, (const double*)g2, d2, 0.0, s2x, X, (size_t)Y * (size_t)Z, n);
}

size_t vnet_surface_gather_ws_bytes(int X, int Y, int Z) {
    size_t n = 0;
    if (volume_count(X, Y, Z, n)) return 0;
    return 2 * (size_t)GATHER_CAP * sizeof(i64);
}

int vnet_surface_gather(const double* d2, const long long* at_bits, double* list, long long* n_out, long long cap, int X, int Y, int Z,
                        void* ws, size_t ws_bytes, void* stream) {
    size_t n = 0;
    if (!at_bits || !n_out || !ws || cap < 0 || (cap > 0 && (!d2 || !list)) || misaligned(d2) || misaligned(at_bits) || misaligned(list) ||
        misaligned(n_out) || misaligned(ws))
        return VNET_E_BADARG;
    if (int e = volume_count(X, Y, Z, n)) return e;
    if (cap > (long long)INT_MAX) return VNET_E_UNSUPPORTED;
    if (ws_bytes < vnet_surface_gather_ws_bytes(X, Y, Z)) return VNET_E_WORKSPACE;
    const int W = (Z + 63) / 64;
    const size_t NW = (size_t)X * (size_t)Y * (size_t)W, chunks = gather_chunks(NW), per = (NW + chunks - 1) / chunks;
    i64* chunk_sum = static_cast<i64*>(ws);
    i64* chunk_off = chunk_sum + GATHER_CAP;
    const u64* bits = reinterpret_cast<const u64*>(at_bits);
    hipStream_t st = (hipStream_t)stream;
    if (int e = launch<gather_count_kernel>(dim3((unsigned)chunks), dim3(PB), 0, st, bits, chunk_sum, NW, per)) return e;
    if (int e = launch<gather_scan_kernel>(dim3(1), dim3(64), 0, st, (const i64*)chunk_sum, chunk_off, (int)chunks, (i64*)n_out)) return e;
    if (cap == 0) return 0;
    if (int e = launch<gather_scatter_kernel>(dim3((unsigned)chunks), dim3(PB), 0, st, d2, bits, list, (const i64*)chunk_off, (i64)cap, NW, per, W, Z))
        return e;
    return launch<zero_tail_kernel>(dim3(blocks_for((size_t)cap, LIST_CAP)), dim3(PB), 0, st, list, (const i64*)n_out, (i64)cap);
}

size_t vnet_list_select_ws_bytes(long long n, int nk) {
    if (n < 1 || n > (long long)INT_MAX || nk < 1 || nk > MAXK) return 0;
    return sizeof(SelState) + (size_t)blocks_for((size_t)n, LIST_CAP) * MAXK * sizeof(i64);
}

int vnet_list_select(const double* list, long long n, const long long* ranks, int nk, double* out,
                     void* ws, size_t ws_bytes, void* stream) {
    if (!list || !ranks || !out || !ws || n < 1 || nk < 1 || nk > MAXK || misaligned(list) || misaligned(out) || misaligned(ws)) return VNET_E_BADARG;
    Ranks rk{};
    for (int r = 0; r < nk; ++r) {
        if (ranks[r] < 0 || ranks[r] >= n) return VNET_E_BADARG;
        rk.v[r] = ranks[r];
    }
    if (n > (long long)INT_MAX) return VNET_E_UNSUPPORTED;
    if (ws_bytes < vnet_list_select_ws_bytes(n, nk)) return VNET_E_WORKSPACE;
    SelState* state = static_cast<SelState*>(ws);
    i64* partial = reinterpret_cast<i64*>(state + 1);
    const int nblocks = blocks_for((size_t)n, LIST_CAP);
    hipStream_t st = (hipStream_t)stream;
    if (int e = launch<select_init_kernel>(dim3(1), dim3(64), 0, st, state, rk)) return e;
    for (int bit = TOP_BIT; bit >= 0; --bit) {
        if (int e = launch<select_count_kernel>(dim3(nblocks), dim3(PB), 0, st, reinterpret_cast<const u64*>(list), (i64)n,
                                                (const SelState*)state, partial, bit, nk))
            return e;
        if (int e = launch<select_step_kernel>(dim3(1), dim3(64 * MAXK), 0, st, (const i64*)partial, nblocks, state, bit, nk, out)) return e;
    }
    return 0;
}

size_t vnet_list_root_sum_ws_bytes(long long n) {
    if (n < 1 || n > (long long)INT_MAX) return 0;
    return (size_t)blocks_for((size_t)n, LIST_CAP) * sizeof(double);
}

int vnet_list_root_sum(const double* list, long long n, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (!list || !out || !ws || n < 1 || misaligned(list) || misaligned(out) || misaligned(ws)) return VNET_E_BADARG;
    if (n > (long long)INT_MAX) return VNET_E_UNSUPPORTED;
    if (ws_bytes < vnet_list_root_sum_ws_bytes(n)) return VNET_E_WORKSPACE;
    double* partial = static_cast<double*>(ws);
    const int nblocks = blocks_for((size_t)n, LIST_CAP);
    hipStream_t st = (hipStream_t)stream;
    if (int e = launch<root_partial_kernel>(dim3(nblocks), dim3(PB), 0, st, list, (i64)n, partial)) return e;
    return launch<root_final_kernel>(dim3(1), dim3(PB), 0, st, (const double*)partial, nblocks, out);
}

}  // extern "C"
