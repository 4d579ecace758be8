/* vnet_hip_head.h -- third public header of libvnet_hip.so: the V-Net decoder's last batch-norm (+ residual, + activation) with the
 * 1x1x1 output convolution behind it (reference networks.py:298-302) folded into its passes.  float32 tensors only (ComputeDtype
 * fp32 and fp32_split3); the bf16-storage mode keeps vnet_bn_act_*_b16 + vnet_head_*_b16.
 * Same conventions as vnet_hip.h: NDHWC contiguous tensors flattened to [M][C], every pointer a 16-byte aligned DEVICE pointer owned
 * by the caller, the library allocates nothing and keeps no state, all work is enqueued on `stream` (hipStream_t, last argument),
 * return value 0, a negative VNET_E_* code or a positive hipError_t.  Reductions are partial rows per workgroup summed in float64 by
 * a finalize kernel: deterministic, no float atomics.
 *
 * The three passes replace these sequences of vnet_hip.h, with s = x (+ r), xhat = (s - mean) * invstd, z = gamma * xhat + beta,
 * y = act(z) ([M][C]), W [C][K], logits = y W + bias ([M][K]):
 *   forward:          vnet_bn_act_fwd, vnet_head_fwd and the statistics pass of vnet_bn_stats over the logits
 *   backward, sums:   the dw / db half of vnet_head_bwd and vnet_bn_act_bwd_reduce with dy = dlogits W^T
 *   backward, apply:  vnet_bn_act_bwd_apply with that dy
 * dy is formed per voxel from dlogits and W and never stored.  C is 8 or 16, K is 1..8 (vnet_bn_head_ok); gamma / beta are the
 * layer's own or the closed-form coefficients of a batch-norm chain (vnet_bn_chain_coef_fwd), as for vnet_bn_act_fwd. */
#ifndef VNET_HIP_HEAD_H
#define VNET_HIP_HEAD_H
#include "vnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when the three passes are built for C channels and K classes, else 0 (the caller then runs the unfused sequence). */
int vnet_bn_head_ok(int C, int K);
/* rows of [sum(K) | sum of squares(K)] vnet_bn_act_head_fwd writes into `stats` for M voxels of C channels (at most 1024). */
int vnet_bn_head_stats_rows(int64_t M, int C);
/* scratch of vnet_bn_act_bwd_reduce_head. */
size_t vnet_bn_head_ws_bytes(int C, int K);

/* y = act(gamma * xhat + beta) (y null: not stored), logits = y W + bias (bias null: 0), and (stats null: not computed) the partial
 * sums of the logits for the batch-norm behind the head: stats [vnet_bn_head_stats_rows(M, C)][2K], every row written, the layout
 * vnet_bn_finalize_partial(stats, rows, K, M, ...) takes.  y and logits have the bits of vnet_bn_act_fwd + vnet_head_fwd: a voxel's
 * logit is the bias plus its channel quads' shares, added in quad order.  The rows group the voxels by workgroup, not as
 * vnet_bn_stats does: mean / invstd finalized from them agree with vnet_bn_stats to rounding, not to the bit. */
int vnet_bn_act_head_fwd(const float* x, const float* r, int64_t M, int C,
    const float* mean, const float* invstd, const float* gamma, const float* beta, int act, const float* alpha,
    const float* w, const float* bias, int K, float* y, float* logits, float* stats, void* stream);

/* dgamma = sum dz xhat, dbeta = sum dz, dalpha = sum dy min(0, z) (act = PRELU) with dy = dlogits W^T, dz = dy act'(z); and the
 * head's dw [C][K] = sum_voxels y^T dlogits (y rebuilt as the forward computes it), db [K] = sum_voxels dlogits.  Every sum is taken
 * in the order of vnet_head_bwd + vnet_bn_act_bwd_reduce (same rows per thread, same tree per workgroup, same finalize). */
int vnet_bn_act_bwd_reduce_head(const float* dlogits, const float* w, int K, const float* x, const float* r, int64_t M, int C,
    const float* mean, const float* invstd, const float* gamma, const float* beta, int act, const float* alpha,
    float* dgamma, float* dbeta, float* dalpha, float* dw, float* db, void* ws, size_t ws_bytes, void* stream);

/* ds = gamma invstd (dz - sum_dz / M_total - xhat sum_dz_xhat / M_total) + xhat xhat_coef (xhat_coef null: 0), the gradient of
 * s = x (+ r), as vnet_bn_act_bwd_apply computes it from a stored dy. */
int vnet_bn_act_bwd_apply_head(const float* dlogits, const float* w, int K, const float* x, const float* r, int64_t M, int C,
    const float* mean, const float* invstd, const float* gamma, const float* beta, int act, const float* alpha,
    const float* sum_dz, const float* sum_dz_xhat, double M_total, const float* xhat_coef, float* ds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_HIP_HEAD_H */
