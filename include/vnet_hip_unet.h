/* vnet_hip_unet.h -- second public header of libvnet_hip.so: the entry points only the reference's U-Net needs
 * (reference networks.py:4-150, selected by TrainingSetting.Networks.Name == "UNet", model.py:414-427).
 * Same conventions as vnet_hip.h: float32 NDHWC contiguous tensors, every pointer a DEVICE pointer owned by the caller, the library
 * allocates nothing and keeps no state, all work is enqueued on `stream` (hipStream_t, last argument), return value 0, a negative
 * VNET_E_* code or a positive hipError_t.
 * The U-Net's 3x3x3 stride-1 SAME convolutions (networks.py:52,57,78,83) need no entry point of their own: vnet_pack_weights,
 * vnet_conv_fwd / _acc / _stats, vnet_conv_wgrad and their size queries in vnet_hip.h take ks = 3, stride = 1, kx = 0 or 3. */
#ifndef VNET_HIP_UNET_H
#define VNET_HIP_UNET_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- tf.nn.max_pool3d(x, ksize=[1,2,2,2,1], strides=[1,2,2,2,1], padding='VALID') (networks.py:120)
 *   x [B,Df,Hf,Wf,C] -> y [B,Df/2,Hf/2,Wf/2,C] (integer division: VALID drops the trailing plane / row / column of an odd axis;
 *   every axis >= 2).  y[b,z,y,x,c] = max over the 8 fine voxels (2z+dz, 2y+dy, 2x+dx).  A max has no rounding: bit-exact. */
int vnet_maxpool2_fwd(const float* x, float* y, int C, int B, int Df, int Hf, int Wf, void* stream);

/* its gradient (the MaxPool3DGrad autodiff builds at model.py:660): the winner is recomputed from x and y, no index tensor.
 *   dy, y [B,Df/2,Hf/2,Wf/2,C]; x, dx [B,Df,Hf,Wf,C].  The gradient of a window goes to its FIRST voxel equal to the maximum in
 *   (dz, dy, dx) scan order; every other voxel -- the dropped trailing planes included -- gets 0.  EVERY element of dx is written.
 *   accum = 1: dx += that gradient instead (dx holds the gradient of x's other consumer, the decoder's skip connection). */
int vnet_maxpool2_bwd(const float* dy, const float* x, const float* y, float* dx, int C, int B, int Df, int Hf, int Wf, int accum,
    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_UNET_H */
