// score.hip -- the two measures that score a label map against its ground truth (include/vnet_hip_score.h; reference
// utils/batch_evaluate: LabelOverlapMeasuresImageFilter, ConnectedComponentImageFilter + LabelShapeStatisticsImageFilter), gfx950.
//   vnet_label_overlap : one streaming pass over both maps.  Every workgroup keeps the 3 * (L + 1) counters in LDS; a wave first
//                        combines the lanes that hold the label of its first lane, and keeps that count in registers for as long as
//                        the following trips start with the same label (components.hip's counting scheme: a solid organ costs one
//                        LDS atomic per run, not one per voxel); the other lanes add one each, in LDS.  One flush per workgroup: a
//                        64-bit atomicAdd per non-zero counter.  Integer adds only.
//   vnet_cc_shape      : the launches of cc_table.h with the index sums folded in the box pass.
// Streaming passes: grid-stride under the fixed grid cap of the sibling files, one thread per voxel, no scratch.
#include <limits.h>
#include "common.h"
#include "cc_table.h"
#include "../../include/vnet_hip_score.h"

namespace {

__global__ void __launch_bounds__(SP_BLOCK) overlap_zero_kernel(u64* out, int words) {
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i < words) out[i] = 0;
}

// One column of the counters.  v: the lane's label (0 .. L), -1 for a lane that counts nothing.  (acc_v, acc_n) is wave-uniform: the
// lanes that shared the first counting lane's label in the trips since acc_v last changed.  Called by all 64 lanes together.
__device__ __forceinline__ void run_count(unsigned* cnt, int col, int v, int& acc_v, unsigned& acc_n, int lane) {
    const u64 m = __ballot(v >= 0);
    if (m == 0) return;
    const int v0 = __shfl(v, __ffsll(m) - 1, 64);
    const bool same = v == v0;
    const u64 ms = __ballot(same);
    if (v0 != acc_v) {
        if (acc_n && lane == 0) atomicAdd(cnt + acc_v * 3 + col, acc_n);
        acc_v = v0;
        acc_n = 0;
    }
    acc_n += (unsigned)__popcll(ms);
    if (v >= 0 && !same) atomicAdd(cnt + v * 3 + col, 1u);
}

// The loop runs on the block's base index so that all lanes of a wave make every trip together (wave-wide votes).  A workgroup sees
// fewer than 2^32 voxels (n <= 2^31 - 1), so 32-bit LDS counters cannot wrap.
__global__ void __launch_bounds__(SP_BLOCK) overlap_count_kernel(const int* __restrict__ a, const int* __restrict__ b, u64* out, size_t n,
                                                                 int L) {
    __shared__ unsigned cnt[3 * (VNET_OVERLAP_MAX_LABELS + 1)];
    const int lane = threadIdx.x & 63, words = 3 * (L + 1);
    for (int i = threadIdx.x; i < words; i += SP_BLOCK) cnt[i] = 0;
    __syncthreads();
    int va = -1, vb = -1, vi = -1;
    unsigned na = 0, nb = 0, ni = 0;
    for (size_t base = (size_t)blockIdx.x * SP_BLOCK; base < n; base += (size_t)gridDim.x * SP_BLOCK) {
        const size_t idx = base + threadIdx.x;
        int la = -1, lb = -1;
        if (idx < n) {
            la = a[idx]; lb = b[idx];
            la = (unsigned)la < (unsigned)L ? la : L;
            lb = (unsigned)lb < (unsigned)L ? lb : L;
        }
        run_count(cnt, 1, la, va, na, lane);
        run_count(cnt, 2, lb, vb, nb, lane);
        run_count(cnt, 0, (la == lb && la < L) ? la : -1, vi, ni, lane);
    }
    if (lane == 0) {
        if (na) atomicAdd(cnt + va * 3 + 1, na);
        if (nb) atomicAdd(cnt + vb * 3 + 2, nb);
        if (ni) atomicAdd(cnt + vi * 3 + 0, ni);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += SP_BLOCK) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(out + i, (u64)c);
    }
}

}  // namespace

extern "C" {

int vnet_label_overlap(const int* a, const int* b, long long* out, long long n, int L, void* stream) {
    if (!a || !b || !out || n < 1 || L < 1) return VNET_E_BADARG;
    if (n > (long long)INT_MAX || L > VNET_OVERLAP_MAX_LABELS) return VNET_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    u64* o = reinterpret_cast<u64*>(out);
    const int words = 3 * (L + 1);
    if (int e = launch<overlap_zero_kernel>(dim3(sp_blocks((size_t)words)), dim3(SP_BLOCK), 0, st, o, words)) return e;
    return launch<overlap_count_kernel>(dim3(sp_blocks((size_t)n)), dim3(SP_BLOCK), 0, st, a, b, o, (size_t)n, L);
}

size_t vnet_cc_shape_ws_bytes(int X, int Y, int Z) {
    size_t n = 0;
    return sp_count(X, Y, Z, n) ? 0 : cc_table_bytes(n);
}

int vnet_cc_shape(const int* label, int* n_out, int* table, long long* sums, int max_components, int X, int Y, int Z,
                  void* ws, size_t ws_bytes, void* stream) {
    return cc_table_run<true>(label, n_out, table, sums, max_components, X, Y, Z, ws, ws_bytes, stream);
}

}  // extern "C"
