/* vnet_bbox.h -- the package's OWN entry points of libvnet_hip.so, not part of the published C ABI under include/: what the
 * bounding-box tool (vnet_tensorflow_amd/bounding_box.py; the reference's utils/bounding_box) runs on the device.  A volume becomes a
 * stack of slices, the components of every class are labelled inside each slice and tabled with their boxes, and every slice is
 * rendered as an RGB picture: windowed grey, label overlay, box outlines.  The rules: bounding_box.py and DESIGN.md section 6h.
 * Same conventions as vnet_hip_components.h, vnet_hip_sample.h and vnet_hip_score.h: contiguous arrays with the last axis fastest, every
 * pointer a DEVICE pointer owned by the caller, the library allocates nothing and keeps no state, scratch is the caller's `ws` /
 * `ws_bytes` (size: the `*_ws_bytes` query; 8-byte aligned), all work is enqueued on `stream` (hipStream_t, last argument), return
 * value 0, a negative VNET_E_* code or a positive hipError_t.  EVERY element of every output is written by a kernel; no result depends
 * on what an output or `ws` held before.  Only integer atomics: results are identical from run to run.
 * Sizes: at most 2^31 - 1 voxels (voxel indices are int32, element offsets 64-bit); more is VNET_E_UNSUPPORTED.
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, a ws that is not 8-byte aligned, a size / capacity < 1, an
 * axis outside 0 .. 2, an alpha outside 0 .. 256), VNET_E_UNSUPPORTED, VNET_E_WORKSPACE (ws_bytes below the query). */
#ifndef VNET_BBOX_H
#define VNET_BBOX_H
#include "../../include/vnet_hip.h"
#include "../../include/vnet_hip_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a volume [X,Y,Z] (Z fastest) as a stack of slices [S,V,U] (U fastest), 4-byte elements copied bit for bit.
 *   axis : the slicing axis.  u is the lower-numbered in-plane axis, v the higher:
 *          2 (axial): (S,V,U) = (Z,Y,X);  1 (coronal): (S,V,U) = (Y,Z,X);  0 (sagittal): (S,V,U) = (X,Z,Y). */
int vnet_slice_stack_f32(const float* src, float* dst, int X, int Y, int Z, int axis, void* stream);
int vnet_slice_stack_i32(const int* src, int* dst, int X, int Y, int Z, int axis, void* stream);

/* scratch of vnet_plane_cc_table: 8 bytes per voxel + 16 KiB; 0 for sizes it would refuse */
size_t vnet_plane_cc_table_ws_bytes(int S, int V, int U);

/* ---- the component table of a stack (int32 [S,V,U]).  A component is a maximal set of voxels of one value > 0 inside one slice,
 *   joined through u +- 1 / v +- 1 neighbours; values <= 0 are background.
 *   n, table : as vnet_cc_table defines them (include/vnet_hip_sample.h) on the stack as a volume (S, V, U): the TRUE number of
 *              components, and int32 [max_components, VNET_CC_ROW] rows {representative, count, lo_s, lo_v, lo_u, hi_s, hi_v, hi_u}
 *              (hi inclusive, lo_s == hi_s) in ascending representative order, the representative the smallest linear index
 *              (s * V + v) * U + u of the component; rows from min(n, max_components) up 0. */
int vnet_plane_cc_table(const int* stack, int* n, int* table, int max_components, int S, int V, int U,
    void* ws, size_t ws_bytes, void* stream);

/* ---- one RGB picture per slice: uint8 [S,V,U,3].
 *   image, label : float32 / int32 [S,V,U].
 *   boxes        : int32 [nb, 5] rows {x, y, w, h, label} grouped by slice; may be null when nb == 0.
 *   first        : int32 [S + 1], slice s owns the rows first[s] .. first[s + 1] - 1; nb = first[S].  0 <= first[s] <= first[s + 1].
 *   grey byte    : wmax != wmin: trunc(clamp((v - wmin) * scale, 0, 255)), every operation rounded in float32, NaN -> 0 (the caller
 *                  passes scale = float(255) / (wmax - wmin)); wmax == wmin: NaN -> 0, v < wmin -> 0, else 255.
 *   overlay      : where label l > 0 every channel is (g * (256 - alpha256) + c * alpha256 + 128) >> 8, c the channel of palette entry
 *                  (l - 1) mod 8; elsewhere the three channels are g.
 *   outlines     : the boxes of the slice in row order, later rows win: pixel (u, v) is on the outline of a row when
 *                  (u == x or u == x + w) and y <= v <= y + h, or (v == y or v == y + h) and x <= u <= x + w; it takes palette entry
 *                  (label - 1) mod 8 at full opacity.  Any number of boxes per slice.
 *   0 <= alpha256 <= 256. */
int vnet_bbox_render(const float* image, const int* label, const int* boxes, const int* first, unsigned char* rgb,
    int S, int V, int U, float wmin, float wmax, float scale, int alpha256, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_BBOX_H */
