/* vnet_hip_components.h -- fifth public header of libvnet_hip.so: face-connected components of a label map and the two label filters
 * that close the reference's evaluate (model.py:1218-1223): `ExtractLargestConnectedComponents` (model.py:142-167) and
 * `volume_threshold` (model.py:117-140).
 * Same conventions as vnet_hip.h: contiguous [X,Y,Z] volumes with the last axis fastest, every pointer a DEVICE pointer owned by the
 * caller, the library allocates nothing and keeps no state, scratch is the caller's `ws` / `ws_bytes` (size: vnet_cc_ws_bytes; 8-byte
 * aligned), all work is enqueued on `stream` (hipStream_t, last argument), return value 0, a negative VNET_E_* code or a positive
 * hipError_t.
 *
 * Rules.  Foreground is label != 0 and ALL non-zero classes form one mask (neighbouring voxels of classes 2 and 5 are connected; a
 * negative label is foreground).  Connectivity is face connectivity, 6 neighbours (sitk.ConnectedComponentImageFilter's and
 * scipy.ndimage.label's default).  A component's representative is its smallest linear index ((x * Y + y) * Z + z).
 * EVERY element of every output is written by a kernel; no result depends on what an output or `ws` held before.  Counts are exact
 * integers (integer atomics only): results are identical from run to run.
 * Sizes: X * Y * Z <= 2^31 - 1 voxels (indices are int32, element offsets 64-bit); a larger volume is VNET_E_UNSUPPORTED.
 * Checked before any launch, in this order: VNET_E_BADARG (a null label / output / ws, a ws that is not 8-byte aligned, a size < 1, a
 * `volume` or `voxel_volume` that is not finite), VNET_E_UNSUPPORTED, VNET_E_WORKSPACE (ws_bytes below the query). */
#ifndef VNET_HIP_COMPONENTS_H
#define VNET_HIP_COMPONENTS_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scratch of vnet_cc_largest and vnet_cc_volume_threshold: 16 + 8 bytes per voxel; 0 for sizes the two would refuse */
size_t vnet_cc_ws_bytes(int X, int Y, int Z);

/* ---- the representative map: roots[v] = representative of v's component, -1 on the background.
 *   sizes (may be null): int32 [X,Y,Z], the component's voxel count AT its representative and 0 at every other voxel.
 *   `roots` is the union-find's parent array while the call runs; no scratch. */
int vnet_cc_roots(const int* label, int* roots, int* sizes, int X, int Y, int Z, void* stream);

/* ---- ExtractLargestConnectedComponents: out (uint8 [X,Y,Z]) = 1 on the component with the most voxels, 0 elsewhere; of components
 *   of equal count the one with the smaller representative (whose first voxel comes first in C order); no foreground: all 0.
 *   thresholded != 0: volume_threshold applied to that 0/1 result as well -- it is ONE component, so it stays iff
 *   (double)count * voxel_volume > volume and the output is all 0 otherwise.  thresholded == 0: volume, voxel_volume are only checked. */
int vnet_cc_largest(const int* label, unsigned char* out, int X, int Y, int Z, int thresholded, double volume, double voxel_volume,
    void* ws, size_t ws_bytes, void* stream);

/* ---- volume_threshold: out (uint8 [X,Y,Z]) = 1 on every component with (double)count * voxel_volume > volume (compared in double,
 *   strictly), 0 elsewhere.  voxel_volume: the product of the voxel spacing, formed once in double by the caller. */
int vnet_cc_volume_threshold(const int* label, unsigned char* out, int X, int Y, int Z, double volume, double voxel_volume,
    void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_COMPONENTS_H */
