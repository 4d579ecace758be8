/* vnet_surface.h -- the package's OWN entry points for the surface-distance scores: part of libvnet_hip.so, not part of the
 * published C ABI under include/.  What the SURFACE scores of Batch_Evaluate (Hausdorff distance, its 95th percentile, average symmetric
 * surface distance) run on the device.  A label map becomes the packed surface of a class mask, the surface becomes an exact squared
 * Euclidean distance field in fp64, the field is read at the voxels of the other map's surface into a list, and the list gives up an
 * order statistic and the sum of its roots.  The rules: vnet_tensorflow_amd/score.py and DESIGN.md section 6j.
 * Conventions of include/vnet_hip_score.h: contiguous volumes [X,Y,Z] with Z fastest, every pointer but `ranks` a DEVICE pointer owned
 * by the caller (8-byte aligned but for `label`), the library allocates nothing and keeps no state, scratch is the caller's `ws` /
 * `ws_bytes` (size: the `*_ws_bytes` query; 8-byte aligned), all work is enqueued on `stream` (hipStream_t, last argument), return
 * value 0, a negative VNET_E_* code (include/vnet_hip.h) or a positive hipError_t.  EVERY element of every output is written by a
 * kernel; no result depends on what an output or `ws` held before.  No atomics at all and every sum in a fixed order: results are
 * identical from run to run.  Every fp64 operation is rounded once (no contraction).
 * A PACKED MASK is an int64 array [X,Y,W], W = ceil(Z / 64): bit k of word w of row (x, y) is voxel z = 64 w + k; the bits of a row's
 * last word at z >= Z are zero (vnet_surface_bits writes them as zero, the others rely on it) -- the convention of csrc/vnet_tools.h.
 * Sizes: X * Y * Z <= 2^31 - 1 voxels and X, Y, Z <= VNET_SURFACE_MAX_AXIS each (index differences are squared in int32 and walked
 * one by one), lists of at most 2^31 - 1 elements; more is VNET_E_UNSUPPORTED.  Grids are capped and the kernels loop.
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, a ws that is not 8-byte aligned, a size / count < 1, a
 * negative klass or cap, a spacing that is not positive and finite, a rank outside [0, n)), VNET_E_UNSUPPORTED, VNET_E_WORKSPACE
 * (ws_bytes below the query). */
#ifndef VNET_SURFACE_H
#define VNET_SURFACE_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VNET_SURFACE_MAX_AXIS 2048
#define VNET_SURFACE_MAX_RANKS 4

/* ---- bits = the packed SURFACE of the class mask of label (int32 [X,Y,Z]).
 *   mask    : label != 0 for klass == 0, label == klass for klass > 0.
 *   surface : the voxels of the mask with at least one of their 6 neighbours outside it; outside the volume counts as outside. */
int vnet_surface_bits(const int* label, int klass, long long* bits, int X, int Y, int Z, void* stream);

/* scratch of vnet_edt2: 12 bytes per voxel (an int32 |dz| and the fp64 field of the z and y passes); 0 for sizes it would refuse */
size_t vnet_edt2_ws_bytes(int X, int Y, int Z);

/* ---- d2 (fp64 [X,Y,Z]) = the squared distance from every voxel to the nearest set bit of `bits`, voxels sx, sy, sz apart:
 *   s2_a = fl(s_a * s_a);  d2(v) = min over set s of fl(fl(s2_x dx^2) + fl(fl(s2_y dy^2) + fl(s2_z dz^2))), the integer squares exact;
 *   +inf everywhere when no bit is set.  Formed axis by axis (z, then y, then x), which gives the same bits as the minimum over all
 *   set voxels because fl(a + t) is monotone in t. */
int vnet_edt2(const long long* bits, double* d2, double sx, double sy, double sz, int X, int Y, int Z,
    void* ws, size_t ws_bytes, void* stream);

/* scratch of vnet_surface_gather (a few KiB, whatever the size); 0 for sizes it would refuse */
size_t vnet_surface_gather_ws_bytes(int X, int Y, int Z);

/* ---- list = the values of d2 at the set bits of at_bits, in voxel (C) order.
 *   n    : int64 [1], the TRUE number of set bits, also when it exceeds cap.
 *   list : fp64 [cap]; elements from min(n, cap) up are 0.  cap == 0 only counts: list and d2 may then be null. */
int vnet_surface_gather(const double* d2, const long long* at_bits, double* list, long long* n, long long cap, int X, int Y, int Z,
    void* ws, size_t ws_bytes, void* stream);

/* scratch of vnet_list_select; 0 for arguments it would refuse */
size_t vnet_list_select_ws_bytes(long long n, int nk);

/* ---- out[j] (fp64 [nk]) = the element of rank ranks[j] (0-based: the ranks[j]-th smallest) of list (fp64 [n]), exactly.
 *   list  : non-negative numbers (sign bit clear; +inf allowed, no NaN): their order is the order of their bit patterns.
 *   ranks : HOST array of 1 .. VNET_SURFACE_MAX_RANKS numbers in [0, n), copied into the kernel's arguments. */
int vnet_list_select(const double* list, long long n, const long long* ranks, int nk, double* out,
    void* ws, size_t ws_bytes, void* stream);

/* scratch of vnet_list_root_sum; 0 for an n it would refuse */
size_t vnet_list_root_sum_ws_bytes(long long n);

/* ---- out[0] (fp64) = the sum of sqrt(list[i]) over list (fp64 [n], non-negative), each root correctly rounded, added in an order that
 *   depends on n alone. */
int vnet_list_root_sum(const double* list, long long n, double* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_SURFACE_H */
