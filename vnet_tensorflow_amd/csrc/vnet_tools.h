/* vnet_tools.h -- the package's OWN entry points of libvnet_hip.so, not part of the published C ABI under include/: what the offline
 * data-preparation tools (vnet_tensorflow_amd/prepare_data.py; the reference's utils/prepare_data) run on the device.  A label map becomes a bit-packed mask, the mask is dilated by ITK's ball, its bounding box is found, and a
 * window of a volume is cut out with the voxels outside the mask zeroed.  The rules: prepare_data.py and DESIGN.md section 6i.
 * Every volume is a dense array [A,B,C] with C fastest; the axes carry no meaning (the ball is isotropic).
 * A PACKED MASK is an int64 array [A,B,W], W = ceil(C / 64): bit k of word w of row (a, b) is voxel c = 64 w + k.  The bits of a row's
 * last word at c >= C are zero; every entry point that writes a packed mask writes them as zero, every one that reads one relies on it.
 * Conventions of the training library: every pointer but `values` is a DEVICE pointer owned by the caller (8-byte aligned for a
 * packed mask and for out7), the library allocates nothing, keeps no state and needs no scratch, all work is enqueued on `stream`
 * (hipStream_t, last argument), return value 0, a negative VNET_E_* code (include/vnet_hip.h) or a positive hipError_t.  EVERY element
 * of every output is written by a kernel; no result depends on what an output held before.  Only integer atomics: results are
 * identical from run to run.
 * Sizes: A * B * C <= 2^31 - 1 voxels, more is VNET_E_UNSUPPORTED; element and byte offsets are size_t inside the kernels.
 * Grids are capped and the kernels loop: 4096 blocks of 256 threads (vnet_dilate_bits: 4096 tiles of 8 x 32 rows of one word;
 * vnet_bits_bbox: 256 blocks).
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, a size < 1, a count, code, radius, element size or window
 * outside what is stated below), VNET_E_UNSUPPORTED. */
#ifndef VNET_TOOLS_H
#define VNET_TOOLS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VNET_TOOLS_MAX_VALUES 16
#define VNET_TOOLS_MAX_RADIUS 8

/* ---- bits = (label is one of values[0 .. nvalues - 1]), packed.
 *   label      : [A,B,C] of dtype_code 0 uint8, 1 int8, 2 int16, 3 uint16, 4 int32.
 *   values     : HOST array of 1 .. VNET_TOOLS_MAX_VALUES numbers, copied into the kernel's arguments; a value outside the dtype's
 *                range matches nothing. */
int vnet_select_bits(const void* label, int dtype_code, const long long* values, int nvalues, long long* bits,
    int A, int B, int C, void* stream);

/* ---- out = bits dilated by the ball of radius r, 1 <= r <= VNET_TOOLS_MAX_RADIUS, out of place (out must not overlap bits).
 *   offset (da, db, dc) is in the ball iff 4 (da^2 + db^2 + dc^2) <= (2 r + 1)^2; voxels outside the volume are 0. */
int vnet_dilate_bits(const long long* bits, long long* out, int A, int B, int C, int r, void* stream);

/* ---- out7 = {count, lo_a, lo_b, lo_c, hi_a, hi_b, hi_c} of the set voxels (hi inclusive); an empty mask gives
 *   {0, A, B, C, -1, -1, -1}.  out7 is initialised by the entry point. */
int vnet_bits_bbox(const long long* bits, long long* out7, int A, int B, int C, void* stream);

/* ---- dst[n0,n1,n2] = the window of src[A,B,C] starting at (s0, s1, s2), elements of elem_bytes = 1, 2, 4 or 8 copied bit for bit
 *   (src and dst aligned to elem_bytes); where bits is not null, an element whose mask bit is 0 becomes all-zero bytes.
 *   The window lies inside the volume: 0 <= s, 1 <= n, s + n <= extent on every axis. */
int vnet_masked_crop(const void* src, const long long* bits, void* dst, int A, int B, int C, int elem_bytes,
    int s0, int s1, int s2, int n0, int n1, int n2, void* stream);

/* ---- dst_u8[A,B,C] = the mask as bytes 0 / 1. */
int vnet_unpack_bits(const long long* bits, unsigned char* dst_u8, int A, int B, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_TOOLS_H */
