/* vnet_hip_summary.h -- tenth public header of libvnet_hip.so: the image summaries of a training / test step rendered on the device (the
 * reference's tf.summary.image calls of its 3-D branch, model.py:326-334, 459-463, 579-585).  A channels-last batch [B,X,Y,Z,C] becomes
 * uint8 slices: output plane [b][c][z] holds the image of height X and width Y that tf.transpose(t[b:b+1, :, :, :, c], [3,1,2,0]) makes
 * of slice z, so the host PNG-encodes rows it never has to transpose and only bytes cross PCIe (vnet_tensorflow_amd/summary.py holds the
 * NumPy restatements of the three rules and the event-file writer).
 * Same conventions as vnet_hip_score.h and vnet_hip_prepare.h: dense tensors with the last axis fastest, every pointer a DEVICE pointer
 * owned by the caller, the library allocates nothing and keeps no state, no scratch, all work is enqueued on `stream` (hipStream_t, last
 * argument), return value 0, a negative VNET_E_* code or a positive hipError_t.  EVERY byte of every output is written by the kernel; no
 * result depends on what the output held before.  No atomics: results are identical from run to run.
 * Sizes: B * X * Y * Z * C <= 2^31 - 1 elements (element offsets are 64-bit, tile counts int64); more is VNET_E_UNSUPPORTED.
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, an extent < 1), VNET_E_UNSUPPORTED. */
#ifndef VNET_HIP_SUMMARY_H
#define VNET_HIP_SUMMARY_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most workgroups of a launch; a larger tensor is covered by a loop over the grid */
#define VNET_SUMMARY_MAX_BLOCKS 4096

/* ---- intensity slices: src float32 [B,X,Y,Z,C] -> dst uint8 [B,C,Z,X,Y], every channel in one launch.
 *   tf.cast(float32 -> uint8) where TensorFlow defines it: 0 <= v < 256 truncates toward zero (and so does -1 < v < 0, to 0).
 *   Where it does not (this library's choice): v <= -1 gives 0, v >= 256 gives 255, NaN gives 0. */
int vnet_summary_slices_f32(const float* src, unsigned char* dst, int B, int X, int Y, int Z, int C, void* stream);

/* ---- index-map slices (label: int32, prediction: int64): src [B,X,Y,Z,C] -> dst uint8 [B,C,Z,X,Y] = (src * factor) mod 256
 *   (tf.cast of the integer product to uint8 wraps).  factor: any int; the caller computes floor(255 / (K - 1)) or floor(255 / K). */
int vnet_summary_slices_i32(const int* src, unsigned char* dst, int factor, int B, int X, int Y, int Z, int C, void* stream);
int vnet_summary_slices_i64(const long long* src, unsigned char* dst, int factor, int B, int X, int Y, int Z, int C, void* stream);

/* ---- rainbow slices of a softmax: src float32 [B,X,Y,Z,K] -> dst uint8 [B,K,Z,X,Y,3] (RGB), every class in one launch.
 *   The reference's grayscale_to_rainbow (model.py:16-24) with tf.image.hsv_to_rgb at S = V = 1, then tf.cast(. * 255, uint8), every
 *   operation rounded separately in float32:  H = ((1 - p) * 2) / 3,  dh = 6 * H,  r = clamp(|dh - 3| - 1, 0, 1),
 *   g = clamp(2 - |dh - 2|, 0, 1),  b = clamp(2 - |dh - 4|, 0, 1),  byte = trunc(channel * 255).  A NaN channel gives 0. */
int vnet_summary_rainbow_f32(const float* src, unsigned char* dst, int B, int X, int Y, int Z, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_SUMMARY_H */
