/* vnet_hip_sample.h -- seventh public header of libvnet_hip.so: the random tail of the reference's training pipeline on prepared cases
 * that live in device memory (NiftiDataset3D.py: ConfidenceCrop2 661-793, RandomCrop 458-551, RandomFlip 187-208, RandomNoise 553-572).
 * The index decisions stay on the host (a few integers per sample); the device supplies what they read -- the table of a case's
 * connected components and foreground counts of candidate windows -- and writes the sample straight into its slot of the batch.
 * Same conventions as vnet_hip_components.h: contiguous volumes with the last axis fastest, every pointer a DEVICE pointer owned by the
 * caller, the library allocates nothing and keeps no state, scratch is the caller's `ws` / `ws_bytes` (size: the `*_ws_bytes` query;
 * 8-byte aligned), all work is enqueued on `stream` (hipStream_t, last argument), return value 0, a negative VNET_E_* code or a positive
 * hipError_t.  EVERY element of every output is written by a kernel; no result depends on what an output or `ws` held before.  Only
 * integer atomics: results are identical from run to run.
 * Sizes: X * Y * Z <= 2^31 - 1 voxels (voxel indices are int32, element offsets 64-bit); a larger volume is VNET_E_UNSUPPORTED.
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, a ws that is not 8-byte aligned, a size / capacity / channel
 * count < 1, a window that does not lie inside the volume, a flip mask outside 0..7, a sigma that is negative or not finite),
 * VNET_E_UNSUPPORTED, VNET_E_WORKSPACE (ws_bytes below the query). */
#ifndef VNET_HIP_SAMPLE_H
#define VNET_HIP_SAMPLE_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int32 words of one row of the component table: {representative, count, lo[3], hi[3]} */
#define VNET_CC_ROW 8

/* scratch of vnet_cc_table: 8 bytes per voxel + 16 KiB; 0 for sizes it would refuse */
size_t vnet_cc_table_ws_bytes(int X, int Y, int Z);

/* ---- the dense component table of a label map (int32 [X,Y,Z]; components as vnet_cc_roots defines them: label != 0, 6 neighbours).
 *   n     : int32 [1], the TRUE number of components, also when it exceeds max_components.
 *   table : int32 [max_components, VNET_CC_ROW].  Row k < min(n, max_components) is the component with the (k+1)-th smallest
 *           representative -- scipy.ndimage.label's component k + 1 -- as {representative (smallest linear index (x * Y + y) * Z + z),
 *           voxel count, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z}, the bounding box with hi INCLUSIVE.  Rows from min(n, max_components) up
 *           are 0. */
int vnet_cc_table(const int* label, int* n, int* table, int max_components, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream);

/* ---- two sums over the window [sx, sx + wx) x [sy, sy + wy) x [sz, sz + wz) of a label map (int32 [X,Y,Z]):
 *   out : int64 [2] = {number of voxels with lo <= label <= hi, sum of the labels}. */
int vnet_window_count(const int* label, long long* out, int X, int Y, int Z, int sx, int sy, int sz, int wx, int wy, int wz,
    int lo, int hi, void* stream);

/* ---- one sample of a batch: the window of P0 x P1 x P2 voxels at (sx, sy, sz), flipped, plus Gaussian noise on the image.
 *   image float32 [X,Y,Z,C], label int32 [X,Y,Z]  ->  out_image float32 [P0,P1,P2,C], out_label int32 [P0,P1,P2(,1)].
 *   flip  : bit a set = axis a is reversed WITHIN the patch (crop, then flip): output index i_a reads source index s_a + P_a - 1 - i_a.
 *   sigma : 0 = the crop bit for bit (no noise arithmetic at all).  sigma > 0: out = fmaf(sigma, z, x), z = the element's normal deviate.
 *   The deviate of output element e (flat index in [P0,P1,P2,C]) is a function of (seed, e) alone:
 *     Philox4x32-10, key = (seed & 0xFFFFFFFF, seed >> 32), counter = (q & 0xFFFFFFFF, q >> 32, 0, 0) with q = e >> 2  ->  k0..k3;
 *     two Box-Muller pairs, (k0, k1) for elements 4q, 4q + 1 and (k2, k3) for 4q + 2, 4q + 3:
 *       u1 = ((k >> 9) + 0.5) * 2^-23 (in (0, 1)), u2 = (k' >> 8) * 2^-24 (in [0, 1)) -- both exact in float --
 *       r = sqrtf(-2 * logf(u1)), theta = 6.2831855f * u2, z = r * cosf(theta) for the even element and r * sinf(theta) for the odd one.
 *   A thread handles four consecutive channels with 16-byte accesses when C % 4 == 0 and image and out_image are 16-byte aligned, one
 *   channel otherwise; the values do not depend on which. */
int vnet_sample_patch(const float* image, const int* label, float* out_image, int* out_label, int X, int Y, int Z, int C,
    int sx, int sy, int sz, int P0, int P1, int P2, int flip, float sigma, unsigned long long seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_SAMPLE_H */
