/* vnet_window.h -- the package's OWN entry points of libvnet_window.so, not part of the published C ABI under include/: the
 * device-side glue of a mirrored or weighted sliding-window evaluation (vnet_tensorflow_amd/window.py).  A window is cut from the
 * case mirrored along any subset of its axes, and a window's softmax is mirrored back, weighted and added to the running sums.
 * The rules: window.py and DESIGN.md section 6l.
 * Arrays are dense, last axis fastest: a volume [X,Y,Z,C] of 32-bit words, a window [P0,P1,P2,C] or [P0,P1,P2,K].
 * MIRRORS: bit a of `mask` (0 .. 7) mirrors axis a of the window: f_a(i) = P_a - 1 - i when the bit is set, else i.
 * Conventions of the training library: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing and keeps
 * no state, all work is enqueued on `stream` (hipStream_t, last argument), return value 0, a negative VNET_E_* code
 * (include/vnet_hip.h) or a positive hipError_t.  No atomic of any kind: every element is read and written by one thread of one
 * launch, launches are ordered on the stream, and the results are identical from run to run.
 * ARITHMETIC: every floating-point operation stated below is ONE IEEE float32 operation, rounded once, in the order the parentheses
 * give; nothing is contracted into a fused multiply-add (the unit is built with -ffp-contract=off and states it with a pragma).
 * Sizes: a volume and a window hold at most 2^31 - 1 voxels each, more is VNET_E_UNSUPPORTED; element offsets are size_t inside the
 * kernels.  Grids are capped and the kernels loop: at most 2048 blocks of 256 threads.  A wave owns whole rows (the last axis) of the
 * window: one row of more than 32 voxels, else 64 / L rows side by side, L the power of two >= P2; the row's offsets are formed once,
 * a lane walks the row in steps of L voxels.  One trip of the capped grid is therefore 2048 * 4 * (64 / L) rows.
 * Checked before any launch, in this order: VNET_E_BADARG (a null pointer, a size < 1, a start outside the volume, a negative offset,
 * a mask outside 0 .. 7, K outside 1 .. 65535, some but not all weight vectors, dst == src), then VNET_E_UNSUPPORTED. */
#ifndef VNET_WINDOW_H
#define VNET_WINDOW_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dst[i,j,k,:] = src[sx + f0(i), sy + f1(j), sz + f2(k), :], the word 0 where a source index is at or past the extent.
 *   src : [X,Y,Z,C] words (a float32 image, or an int32 label with C = 1);  dst : [P0,P1,P2,C], must not overlap src.
 *   0 <= sx < X, 0 <= sy < Y, 0 <= sz < Z.  mask = 0 gives the bytes of vnet_crop_words.
 *   C % 4 == 0 and both pointers 16-byte aligned: 16-byte accesses; otherwise one word at a time, with the same values. */
int vnet_window_crop_flip(const void* src, void* dst, int X, int Y, int Z, int C,
    int sx, int sy, int sz, int P0, int P1, int P2, int mask, void* stream);

/* ---- for every window voxel (i,j,k) whose volume voxel g = (o0 + i, o1 + j, o2 + k) lies inside [D0,D1,D2]:
 *          w        = (w0[i] * w1[j]) * w2[k]
 *          vol[g,c] = vol[g,c] + w * patch[f0(i), f1(j), f2(k), c]      for every c < K
 *          cnt[g]   = cnt[g] + w
 *   The weights index the window in the VOLUME's frame; the patch is read mirrored.
 *   patch : [P0,P1,P2,K];  vol : [D0,D1,D2,K];  cnt : [D0,D1,D2] or null;  w0, w1, w2 : P0, P1, P2 floats, all null or all given.
 *   Null weights: w = 1 and w * p is not formed (vol = vol + p, cnt = cnt + 1); with mask = 0 that is vnet_accumulate_patch bit for
 *   bit.  Offsets o_a >= 0; 1 <= K <= 65535.  K = 2 (K = 4) with patch and vol 8-byte (16-byte) aligned: one float2 (float4) access
 *   per voxel and array; K <= 5 keeps a voxel's values in registers; the values are the same on every path. */
int vnet_window_accumulate(const float* patch, float* vol, float* cnt, int K,
    int P0, int P1, int P2, int o0, int o1, int o2, int D0, int D1, int D2,
    int mask, const float* w0, const float* w1, const float* w2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNET_WINDOW_H */
