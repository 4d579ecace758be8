/* vnet_post.h -- the package's OWN entry points of libvnet_post.so, not part of the published C ABI under include/: what the
 * post-processing pipeline of evaluate (vnet_tensorflow_amd/postprocess.py) runs on the device label.  Components are labelled class
 * by class in one pass, the largest of a class is kept or the small ones dropped, cavities of a class are filled, and a packed mask is
 * complemented or written back into the label.  The rules: postprocess.py and DESIGN.md section 6k.
 * A label map is a dense int32 array [X,Y,Z] with Z fastest.  Connectivity is face connectivity (6 neighbours).  A PACKED MASK is an
 * int64 array [A,B,W], W = ceil(C / 64), in the convention of vnet_tools.h: bit k of word w of row (a, b) is voxel c = 64 w + k, the
 * bits of a row's last word at c >= C are zero; every entry point that writes a packed mask writes them as zero.
 * Conventions of the training library: every pointer but `values` is a DEVICE pointer owned by the caller (8-byte aligned for a
 * packed mask and for `ws`), the library allocates nothing and keeps no state, scratch comes through `ws` / `ws_bytes` with a
 * `*_ws_bytes` query (0 for sizes the entry point refuses), all work is enqueued on `stream` (hipStream_t, last argument), return
 * value 0, a negative VNET_E_* code (include/vnet_hip.h) or a positive hipError_t.  EVERY element of every output is written by a
 * kernel; no result depends on what an output or the scratch held before.  Only integer atomics: results are identical from run to
 * run.  An output must not overlap an input.
 * Sizes: X * Y * Z <= 2^31 - 1 voxels, more is VNET_E_UNSUPPORTED; element and byte offsets are size_t inside the kernels.
 * Grids are capped and the kernels loop: 4096 blocks of 256 threads, one thread per voxel (vnet_post_not_bits: per word).
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, a misaligned `ws`, a size < 1, a count or mode outside what
 * is stated below, a class value 0, a value given twice, a volume that is not finite), VNET_E_UNSUPPORTED, VNET_E_WORKSPACE. */
#ifndef VNET_POST_H
#define VNET_POST_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VNET_POST_MAX_VALUES 16

/* ---- the components of every class in values[0 .. nvalues - 1] at once: two face neighbours are linked iff they hold the same label
 *   and that label is one of the values.
 *   values : HOST array of 1 .. VNET_POST_MAX_VALUES distinct non-zero class values, copied into the kernels' arguments.
 *   roots  : [X,Y,Z], the smallest linear index of the voxel's component, -1 where the voxel's class is not one of the values.
 *   sizes  : [X,Y,Z] or null: the component's voxel count at its representative, 0 elsewhere. */
int vnet_post_class_roots(const int* label, const int* values, int nvalues, int* roots, int* sizes,
    int X, int Y, int Z, void* stream);

/* ---- out = label with components of the classes in `values` removed (set to 0); every other voxel is copied.
 *   mode 0 : of each class the component with the most voxels stays, of equal counts the one with the smaller representative
 *            (volume and voxel_volume are not read).
 *   mode 1 : a component stays iff (double)count * voxel_volume > volume. */
size_t vnet_post_filter_components_ws_bytes(int X, int Y, int Z);
int vnet_post_filter_components(const int* label, int* out, const int* values, int nvalues, int mode, double volume,
    double voxel_volume, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream);

/* ---- out = klass where label == 0 and the voxel lies in a cavity of class klass (a face-connected component of label != klass that
 *   touches no face of the volume), label elsewhere.  klass != 0. */
size_t vnet_post_fill_holes_ws_bytes(int X, int Y, int Z);
int vnet_post_fill_holes(const int* label, int* out, int klass, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream);

/* ---- out = the complement of the packed mask bits inside the volume [A,B,C]. */
int vnet_post_not_bits(const long long* bits, long long* out, int A, int B, int C, void* stream);

/* ---- the mask of class klass (!= 0) written back: out = klass where the bit is set and label == 0, 0 where label == klass and the
 *   bit is clear, label elsewhere.  A class grows into the background only. */
int vnet_post_apply_bits(const int* label, const long long* bits, int klass, int* out, int A, int B, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_POST_H */
