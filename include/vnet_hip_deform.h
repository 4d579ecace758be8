/* vnet_hip_deform.h -- sixth public header of libvnet_hip.so: free-form deformation of a volume by a cubic B-spline displacement field,
 * the `BSplineDeformation` augmentation of the reference's pipeline (pipeline/NiftiDataset3D.py:795-832: sitk.BSplineTransform(3, 3) with
 * the image's origin and direction, physical size n_a * s_a, mesh size (10, 10, 10); sitk.Resample(image, bspline) onto the image's own
 * grid with the default interpolator -- linear, for the label too -- and default pixel value 0).
 * Same conventions as vnet_hip.h: contiguous tensors, every pointer a DEVICE pointer owned by the caller, the library allocates nothing
 * and keeps no state, all work is enqueued on `stream` (hipStream_t, last argument), return value 0, a negative VNET_E_* code or a
 * positive hipError_t.
 *
 * Rules (stated from knowledge of ITK, unpinned by the reference: DESIGN.md section 6b; executable form: vnet_tensorflow_amd/deform.py).
 * Volumes are [X,Y,Z,(C)] with the last axis fastest; array axis 0 is ITK's x.  Origin 0, direction identity (shared, so they cancel).
 *   control grid : G = 13 points per axis, 3 * 13^3 = 6591 doubles, coef[a * 2197 + (k * 13 + j) * 13 + i] with a the displaced
 *                  component (x, y, z), k, j, i the z, y, x control indices.
 *   displacement : voxel i_a sits at p_a = i_a * s_a; control spacing D_a = n_a * s_a / 10; u_a = p_a / D_a, m_a = floor(u_a),
 *                  t = u_a - m_a, weights ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 on the control indices m_a .. m_a + 3;
 *                  d_a = sum_k sum_j sum_i wz_k wy_j wx_i coef_a[k][j][i] in double; 0 (all components) unless 0 <= u_a < 10 on every axis.
 *   sampling     : c_a = i_a + d_a / s_a; inside iff -0.5 <= c_a < n_a - 0.5 on every axis, an outside sample is 0; b = floor(c),
 *                  d = c - b, neighbours max(b, 0) and min(b + 1, n - 1); the 8-tap blend runs in double, lo + d * (hi - lo) along z,
 *                  then y, then x, without FMA contraction.
 * EVERY element of y is written.  Element offsets are 64-bit; the voxel count X*Y*Z must fit an int32 (VNET_E_UNSUPPORTED otherwise,
 * before any launch).  VNET_E_BADARG: a null x, y or coef, a size < 1, C < 1, a spacing that is not finite or not > 0. */
#ifndef VNET_HIP_DEFORM_H
#define VNET_HIP_DEFORM_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VNET_BSPLINE_GRID 13                    /* control points per axis: mesh size 10 + spline order 3 */
#define VNET_BSPLINE_PARAMS (3 * 13 * 13 * 13)  /* doubles in coef */

/* ---- image: float32 x [X,Y,Z,C] -> y [X,Y,Z,C]; the blend is rounded to float once.  The displacement of a voxel is computed once
 *   and shared by its C channels. */
int vnet_bspline_deform_f32(const float* x, float* y, int X, int Y, int Z, int C, const double* coef, double sx, double sy, double sz,
    void* stream);

/* ---- label map: int32 x [X,Y,Z] -> y [X,Y,Z] (C must be 1), the same linear blend, TRUNCATED toward zero to int32 after clamping to
 *   its range (ITK's static_cast of the interpolator's double: deformed label borders erode -- a reference quirk, kept). */
int vnet_bspline_deform_i32(const int* x, int* y, int X, int Y, int Z, int C, const double* coef, double sx, double sy, double sz,
    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_DEFORM_H */
