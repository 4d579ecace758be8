/* vnet_hip_resample.h -- fourth public header of libvnet_hip.so: resampling a volume onto a grid of another voxel spacing, the
 * `Resample` transform of the reference's pipeline (pipeline/NiftiDataset3D.py:345-398: sitk.ResampleImageFilter, identity transform,
 * output origin and direction of the input, default pixel value 0) and the way back of its evaluate_single_3D (model.py:817-977).
 * Same conventions as vnet_hip.h: contiguous tensors, every pointer a DEVICE pointer owned by the caller, the library allocates nothing
 * and keeps no state, all work is enqueued on `stream` (hipStream_t, last argument), return value 0, a negative VNET_E_* code or a
 * positive hipError_t.
 *
 * Geometry (stated from knowledge of ITK, unpinned by the reference: DESIGN.md section 6b).  Origin and direction are shared and the
 * transform is the identity, so the axes decouple: output index i_a reads the source at the continuous index c_a = i_a * r_a with
 * r_a = (output spacing) / (source spacing), formed ONCE in double by the caller; c_a is computed in double.  A sample is inside iff
 * c_a < n_a - 0.5 on every axis (n_a the source size; c_a >= 0 always); an outside sample is 0.  EVERY element of y is written.
 * Volumes are [X,Y,Z,(C)] with the last axis fastest; element offsets are 64-bit (X*Y*Z*C may pass 2^31).
 * VNET_E_BADARG: a null x or y, a size < 1, C < 1, a ratio that is not finite or not > 0. */
#ifndef VNET_HIP_RESAMPLE_H
#define VNET_HIP_RESAMPLE_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- tri-linear (sitk.sitkLinear), float32 x [X,Y,Z,C] -> y [Xo,Yo,Zo,C]
 *   b_a = floor(c_a), d_a = c_a - b_a, upper neighbour min(b_a + 1, n_a - 1) (in (n_a - 1, n_a - 0.5) the last voxel alone); the
 *   8-tap blend runs in double (lerp along z, then y, then x, each as lo + d * (hi - lo)) and is rounded to float once.
 *   div (may be null): float32 [X,Y,Z]; every tap is then (double)x[v,c] / (double)div[v] -- the count map of the sliding window, so
 *   that the probability maps go back without vol / cnt ever being stored.  A tap whose div[v] is 0 has the value 0. */
int vnet_resample_linear(const float* x, const float* div, float* y, int C, int X, int Y, int Z, int Xo, int Yo, int Zo,
    double rx, double ry, double rz, void* stream);

/* ---- nearest neighbour (sitk.sitkNearestNeighbor) of a label map, int32 x [X,Y,Z] -> y [Xo,Yo,Zo], same grid and inside test:
 *   source index floor(c_a + 0.5) per axis (half-integers round up). */
int vnet_resample_nearest_i32(const int* x, int* y, int X, int Y, int Z, int Xo, int Yo, int Zo, double rx, double ry, double rz,
    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_RESAMPLE_H */
