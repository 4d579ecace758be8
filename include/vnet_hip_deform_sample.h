/* vnet_hip_deform_sample.h -- eleventh public header of libvnet_hip.so: one training sample cut from a device-resident case THROUGH the
 * free-form deformation, the `BSplineDeformation` in front of the crop of the reference's training pipeline (NiftiDataset3D.py:795-832,
 * then ConfidenceCrop2 661-793 | RandomCrop 458-551, RandomFlip 187-208, RandomNoise 553-572) without a deformed copy of the image:
 * only the voxels of the window are deformed, straight into their slot of the batch.
 * Same conventions as vnet_hip_deform.h and vnet_hip_sample.h: contiguous tensors with the last axis fastest, every pointer a DEVICE
 * pointer owned by the caller, the library allocates nothing and keeps no state, all work is enqueued on `stream` (hipStream_t, last
 * argument), return value 0, a negative VNET_E_* code or a positive hipError_t.
 *
 * The rule.  With D = vnet_bspline_deform_f32(image, coef, s0, s1, s2) -- the whole deformed image, which is never formed --
 *   out_image is, bit for bit, what vnet_sample_patch(D, ., window, flip, sigma, seed) writes: the window of D, axis a reversed within
 *             the patch where bit a of `flip` is set, plus the noise of vnet_hip_sample.h keyed by (seed, output element); sigma 0 = no
 *             noise arithmetic at all;
 *   out_label is the window of deformed_label, flipped the same way.  deformed_label is the caller's vnet_bspline_deform_i32 of the case's
 *             label map under the same coef: the crop's index decisions need it whole, so it exists already.
 * The control grid, the valid region and the inside test are those of the VOLUME [X,Y,Z], not of the patch: a voxel of the window reads
 * the resident image wherever its source position falls, also outside the window, and is 0 where that falls outside the volume.  The
 * displacement and the blend run in the arithmetic of vnet_bspline_deform_f32 (double, no FMA contraction, the same summation order).
 * A thread handles the channels of a voxel in quads with 16-byte accesses when C % 4 == 0 and image and out_image are 16-byte aligned,
 * one channel at a time otherwise; the values do not depend on which.  EVERY element of both outputs is written.
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, a size or C < 1, a spacing that is not finite or not > 0, a
 * window that does not lie inside the volume, a flip mask outside 0..7, a sigma that is negative or not finite), VNET_E_UNSUPPORTED
 * (X * Y * Z beyond int32: voxel indices are int32, element offsets 64-bit). */
#ifndef VNET_HIP_DEFORM_SAMPLE_H
#define VNET_HIP_DEFORM_SAMPLE_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* image float32 [X,Y,Z,C] (undeformed), deformed_label int32 [X,Y,Z], coef double [VNET_BSPLINE_PARAMS] (vnet_hip_deform.h)
 *   ->  out_image float32 [P0,P1,P2,C], out_label int32 [P0,P1,P2(,1)]: the window of P0 x P1 x P2 voxels at (sx, sy, sz).
 *   s0, s1, s2 : the voxel spacing of the case along x, y, z. */
int vnet_deform_sample_patch(const float* image, const int* deformed_label, const double* coef,
    float* out_image, int* out_label, int X, int Y, int Z, int C, double s0, double s1, double s2,
    int sx, int sy, int sz, int P0, int P1, int P2, int flip, float sigma, unsigned long long seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_DEFORM_SAMPLE_H */
