/* vnet_hip_prepare.h -- eighth public header of libvnet_hip.so: what evaluate does to a case in front of the network and behind it, on
 * a volume that lives in device memory (the intensity windows of NiftiDataset3D.py: Normalization 167-185, StatisticalNormalization
 * 210-254, ExtremumNormalization 256-283, ManualNormalization 285-308; Padding 400-456; the window crop of model.py:94-115; the argmax of
 * model.py:934).  Same conventions as vnet_hip_sample.h: dense volumes with the last axis fastest, every pointer a DEVICE pointer owned by
 * the caller, the library allocates nothing and keeps no state, scratch is the caller's `ws` / `ws_bytes` (size: the `*_ws_bytes` query;
 * 8-byte aligned), all work is enqueued on `stream` (hipStream_t, last argument), return value 0, a negative VNET_E_* code or a positive
 * hipError_t.  EVERY element of every output is written by a kernel; no result depends on what an output or `ws` held before.  No
 * floating-point atomics: results are identical from run to run.
 * Sizes: a volume holds at most 2^31 - 1 voxels (n, X * Y * Z and P0 * P1 * P2); a larger one is VNET_E_UNSUPPORTED, and so is a channel
 * count above 65535 in vnet_channel_stats / vnet_window_intensity.  Element offsets are 64-bit.
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer other than `pre`, a ws that is not 8-byte aligned, a size, n, C
 * or K < 1, a start < 0 or at or past the extent), VNET_E_UNSUPPORTED, VNET_E_WORKSPACE (ws_bytes below the query).
 * Every fp64 operation below is ONE IEEE operation, rounded once (no contraction into fused multiply-adds). */
#ifndef VNET_HIP_PREPARE_H
#define VNET_HIP_PREPARE_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most blocks vnet_channel_stats spreads the voxels of one channel (or channel quad) over: each handles 256 voxels per trip */
#define VNET_STATS_MAX_BLOCKS 1024

/* scratch of vnet_channel_stats: 8 * C * (4 * VNET_STATS_MAX_BLOCKS + 1) bytes; 0 for a C it would refuse */
size_t vnet_channel_stats_ws_bytes(int C);

/* ---- per-channel statistics of image float32 [n, C] (n voxels).
 *   pre : double [C][2] = {a, b}, the value of an element is v = ((double)x - a) / b; a null pointer: v = (double)x.
 *   out : double [C][4] = {sum, css, min, max} of v, css = sum of (v - mean)^2 with mean = sum / n (one division, formed on the device
 *         between the two passes over the volume).  A NaN among the values makes all four NaN.
 *   Per-thread fp64 accumulators, wave reduction, block reduction, one partial per block in ws, added in a fixed order by a last kernel
 *   of each pass.  The grid follows n alone.  Channel quads with 16-byte loads when C % 4 == 0 and image is 16-byte aligned, one channel
 *   otherwise; on data whose sums are exact in fp64 the results do not depend on which. */
int vnet_channel_stats(const float* image, const double* pre, double* out, long long n, int C, void* ws, size_t ws_bytes, void* stream);

/* ---- the intensity window (sitk.IntensityWindowingImageFilter onto [0, 255]) of in float32 [n, C] -> out float32 [n, C]; out == in is
 * allowed (any other overlap is not).
 *   prm : double [C][5] = {a, b, wmin, scale, flag}.  v = ((double)x - a) / b, then
 *     flag == 0 : y = (v - wmin) * scale + 0.0;  y < 0 ? 0 : (y > 255 ? 255 : y);  one rounding to float.  NaN stays NaN.
 *     flag != 0 : v < wmin ? 0 : 255  (the degenerate window wmax == wmin; NaN gives 255).
 *   Quads / one channel as above; the values do not depend on which. */
int vnet_window_intensity(const float* in, float* out, const double* prm, long long n, int C, void* stream);

/* ---- a window of 32-bit words with zero fill: src [X,Y,Z,C] -> dst [P0,P1,P2,C], dst[i,j,k,:] = src[sx + i, sy + j, sz + k, :] where
 * that voxel exists and the word 0 where an index is at or past the extent.  float32 images and int32 labels (C = 1) alike.  dst must
 * not overlap src.  0 <= s_a < the extent of axis a.  Four words with 16-byte accesses when C % 4 == 0 and src and dst are 16-byte
 * aligned, one word otherwise. */
int vnet_crop_words(const void* src, void* dst, int X, int Y, int Z, int C, int sx, int sy, int sz, int P0, int P1, int P2, void* stream);

/* ---- vol float32 [n, K] -> label int32 [n]: the first index of the largest value of a row; a NaN counts as larger than every number
 * and the first NaN wins (np.argmax, torch.argmax). */
int vnet_argmax_label(const float* vol, int* label, long long n, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_PREPARE_H */
