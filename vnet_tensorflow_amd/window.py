"""Mirrored passes and window weights of the sliding-window evaluation (evaluate(), Batch_Evaluate).  Not in the
reference, whose windows all count 1 everywhere and go through the network once.

This module STATES the rules (the functions of the first half): which mirrors a `Mirror` setting asks for and in which order, the
weight vectors of a window, and the two device operations as NumPy float32 restatements, operation for operation -- the yardstick the
kernels are held `==` to, and the route of a CPU tensor (a CPU model's).  The second half is the ctypes binding of libvnet_window.so
(csrc/vnet_window.h, csrc/window.hip) and its ops.  A library of its own beside libvnet_hip.so: the header is the package's own, not
part of the published C ABI, and none of this is in _lib.HEADERS.

The rules.  A MASK is an integer 0 .. 7: bit a mirrors axis a of a window, f_a(i) = P_a - 1 - i.
  flip_sets(mirror)      the masks of the passes of one batch, identity (0) first.
  weight_vectors(kind)   "uniform": None, every voxel of a window counts 1.  "gaussian": three float32 vectors, the weight of window
                         voxel (i,j,k) is (w0[i] * w1[j]) * w2[k] in float32.  Separable, so a kernel reads P0 + P1 + P2 floats and
                         not a P0*P1*P2 array; computed on the host in float64, so no kernel evaluates an exponential.  Not
                         normalised: a common factor cancels in vol / cnt and in the argmax.
  crop_flip              dst[i,j,k,:] = src[s0 + f0(i), s1 + f1(j), s2 + f2(k), :], 0 where the source index is past the extent.
  accumulate             vol[g,:] += w * patch[f0(i), f1(j), f2(k), :], cnt[g] += w at g = origin + (i,j,k) inside the volume: the
                         patch is the softmax of a MIRRORED window and is read mirrored back; the weights index the window in the
                         volume's frame.

Same conventions as _lib / ops on the device side: there is NO fallback -- a missing library or a kernel that reports an error raises
VnetHipError; ops launch on torch's current stream of the calling thread; outputs are allocated through this module's `torch` name."""
import ctypes
import os

import numpy as np
import torch

from . import ops
from ._lib import VnetHipError, check
from .ops import _thread_stream as _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VNET_WINDOW_LIB") or os.path.join(_HERE, "libvnet_window.so")
HEADER = "vnet_tensorflow_amd/csrc/vnet_window.h"

KINDS = ("uniform", "gaussian")
MIN_WEIGHT = 2.0 ** -100         # the smallest window weight taken: 2^-26 of headroom above the smallest normal float for w * p
MAX_K, MAX_VOXELS = 65535, 2 ** 31 - 1


# ---- the rules ----------------------------------------------------------------------------------------------------------------------------
def _axis(a, mirror):
    if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 0 <= int(a) <= 2:
        raise ValueError("window: Mirror %r names axis %r; the axes of a window are 0, 1 and 2" % (mirror, a))
    return int(a)


def _set_mask(axes, mirror):
    axes = [_axis(a, mirror) for a in axes]
    if len(set(axes)) != len(axes):
        raise ValueError("window: Mirror %r names axis %d twice" % (mirror, [a for a in axes if axes.count(a) > 1][0]))
    return sum(1 << a for a in axes)


def flip_sets(mirror):
    """The masks of the passes of a batch, identity first.
    A flat list of distinct axes: every subset of them, in binary counting order of the listed axes ([0, 2] -> 0, 1, 4, 5).
    A list of lists: identity, then each listed set in the given order ([[0, 1]] -> 0, 3: the one joint flip).
    [] or None: [0]."""
    if mirror is None:
        return [0]
    if isinstance(mirror, (str, bytes)) or not isinstance(mirror, (list, tuple)):
        raise ValueError("window: Mirror %r is not a list of axes or a list of axis sets" % (mirror,))
    mirror = list(mirror)
    if not mirror:
        return [0]
    nested = [isinstance(m, (list, tuple)) for m in mirror]
    if any(nested):
        if not all(nested):
            raise ValueError("window: Mirror %r mixes axes and axis sets" % (mirror,))
        out = [0]
        for s in mirror:
            if len(s) == 0:
                raise ValueError("window: Mirror %r holds an empty set; the identity pass is always run, first" % (mirror,))
            m = _set_mask(s, mirror)
            if m in out:
                raise ValueError("window: Mirror %r names the set %r twice" % (mirror, list(s)))
            out.append(m)
        return out
    _set_mask(mirror, mirror)                        # (the axes are valid and distinct)
    axes = [int(a) for a in mirror]
    return [sum(1 << axes[b] for b in range(len(axes)) if n >> b & 1) for n in range(1 << len(axes))]


def _three_shape(patch_shape):
    ps = tuple(int(v) for v in patch_shape)
    if len(ps) != 3 or any(p < 1 for p in ps):
        raise ValueError("window: a window shape is three sizes >= 1, got %r" % (patch_shape,))
    return ps


def weight_vectors(kind, patch_shape, sigma=0.125):
    """None for "uniform"; for "gaussian" three float32 vectors w_a[i] = float32(exp(-0.5 * ((i - (P_a - 1) / 2) / (sigma_a * P_a))^2)),
    evaluated in float64.  sigma: a number or three, in units of the window's size.  Refused: a window whose corner weight
    (w0[0] * w1[0]) * w2[0], formed in float32, is below 2^-100."""
    if kind not in KINDS:
        raise ValueError("window: WindowWeights %r (known: %s)" % (kind, ", ".join(KINDS)))
    ps = _three_shape(patch_shape)
    if kind == "uniform":
        return None
    sig = [sigma] * 3 if isinstance(sigma, (int, float, np.integer, np.floating)) and not isinstance(sigma, bool) else list(sigma)
    if len(sig) != 3 or any(isinstance(s, bool) or not np.isfinite(float(s)) or float(s) <= 0 for s in sig):
        raise ValueError("window: WindowSigma %r is not a positive number or three of them" % (sigma,))
    out = []
    for P, s in zip(ps, sig):
        i = np.arange(P, dtype=np.float64)
        out.append(np.exp(-0.5 * ((i - (P - 1) / 2.0) / (float(s) * P)) ** 2).astype(np.float32))
    corner = np.float32(np.float32(out[0][0] * out[1][0]) * out[2][0])
    if not corner >= np.float32(MIN_WEIGHT):
        raise ValueError("window: with WindowSigma %r the corner of a %dx%dx%d window weighs %.3g, below 2^-100: a product w * p could "
                         "become subnormal" % ((sigma,) + ps + (float(corner),)))
    return tuple(out)


def _mask(mask):
    if isinstance(mask, bool) or int(mask) != mask or not 0 <= int(mask) <= 7:
        raise ValueError("window: mask %r (an integer 0 .. 7)" % (mask,))
    return int(mask)


def _mirrored(n, flip):
    i = np.arange(n, dtype=np.int64)
    return n - 1 - i if flip else i


def crop_flip_np(src, start, size, mask):
    """vnet_window_crop_flip as a rule: src [X,Y,Z,C] or [X,Y,Z] -> the window of `size` at `start`, mirrored along the axes of `mask`,
    zero where the source index is at or past the extent."""
    src = np.asarray(src)
    start, size, mask = ops._three(start, "crop_flip: start"), _three_shape(size), _mask(mask)
    if src.ndim not in (3, 4) or any(not 0 <= s < n for s, n in zip(start, src.shape[:3])):
        raise ValueError("crop_flip: window %s + %s on a volume %s" % (start, size, src.shape))
    out = np.zeros(size + src.shape[3:], dtype=src.dtype)
    at = [start[a] + _mirrored(size[a], mask >> a & 1) for a in range(3)]
    ok = [np.flatnonzero(at[a] < src.shape[a]) for a in range(3)]
    if all(o.size for o in ok):
        out[np.ix_(*ok)] = src[np.ix_(*[at[a][ok[a]] for a in range(3)])]
    return out


def accumulate_np(patch, vol, cnt, origin, mask, weights):
    """vnet_window_accumulate as a rule, IN PLACE on the float32 arrays vol [D0,D1,D2,K] and cnt [D0,D1,D2] (or None), every operation
    one float32 operation: w = (w0[i] * w1[j]) * w2[k]; vol += w * patch (read mirrored); cnt += w.  weights None: vol += patch,
    cnt += 1."""
    origin, mask = ops._three(origin, "accumulate: origin"), _mask(mask)
    if patch.dtype != np.float32 or vol.dtype != np.float32 or (cnt is not None and cnt.dtype != np.float32):
        raise ValueError("accumulate: float32 arrays")
    if patch.ndim != 4 or vol.ndim != 4 or patch.shape[3] != vol.shape[3] or any(o < 0 for o in origin):
        raise ValueError("accumulate: patch %s at %s on a volume %s" % (patch.shape, origin, vol.shape))
    n = [max(0, min(patch.shape[a], vol.shape[a] - origin[a])) for a in range(3)]
    if not all(n):
        return
    for a in range(3):
        if mask >> a & 1:
            patch = np.flip(patch, axis=a)
    src = patch[:n[0], :n[1], :n[2]]
    sl = tuple(slice(o, o + m) for o, m in zip(origin, n))
    if weights is None:
        vol[sl] = vol[sl] + src
        if cnt is not None:
            cnt[sl] = cnt[sl] + np.float32(1)
        return
    w0, w1, w2 = (np.asarray(w, dtype=np.float32) for w in weights)
    w = (w0[:n[0], None, None] * w1[None, :n[1], None]) * w2[None, None, :n[2]]
    assert w.dtype == np.float32
    vol[sl] = vol[sl] + w[..., None] * src
    if cnt is not None:
        cnt[sl] = cnt[sl] + w


# ---- libvnet_window.so --------------------------------------------------------------------------------------------------------------------
_vp, _i = ctypes.c_void_p, ctypes.c_int

# name -> (restype, argtypes) : every symbol csrc/vnet_window.h declares (tests/test_window_host.py holds the table to the header)
SIGNATURES_WINDOW = {
    "vnet_window_crop_flip": (_i, [_vp, _vp] + [_i] * 11 + [_vp]),
    "vnet_window_accumulate": (_i, [_vp, _vp, _vp] + [_i] * 11 + [_vp, _vp, _vp, _vp]),
}

_window = None


def lib():
    """The loaded libvnet_window.so (raises if it has not been built: there is no fallback path)."""
    global _window
    if _window is None:
        if not os.path.exists(LIB_PATH):
            raise VnetHipError("libvnet_window.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc, gfx950).  The HIP library is the only compute path." % LIB_PATH)
        # torch (imported above) has loaded its own libamdhip64 by now: both libraries and torch's streams live in ONE HIP runtime
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES_WINDOW.items():
            fn = getattr(L, name)              # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        _window = L
    return _window


def _dense(t, what):
    if not isinstance(t, torch.Tensor):
        raise VnetHipError("%s: takes a tensor, got %s" % (what, type(t).__name__))
    if t.numel() == 0 or not t.is_contiguous():
        raise VnetHipError("%s: the tensor is dense and not empty, got %s" % (what, tuple(t.shape)))
    return t


def crop_flip(src, start, size, mask, out=None):
    """ops.crop_window with mirrors: the window of `size` voxels at `start` of a dense tensor, mirrored along the axes of `mask`, zero
    where it reaches past the extent.  float32 [X,Y,Z,C] -> [P0,P1,P2,C] or int32 [X,Y,Z] -> [P0,P1,P2]; 0 <= start < extent.
    A device tensor takes the kernel, a CPU tensor the rule (crop_flip_np).  out: the caller's slot (dense, same dtype and device, any
    4-byte offset), or None = a new tensor."""
    start, size, mask = ops._three(start, "crop_flip: start"), ops._three(size, "crop_flip: size"), _mask(mask)
    src = _dense(src, "crop_flip")
    if not ((src.dim() == 4 and src.dtype == torch.float32) or (src.dim() == 3 and src.dtype == torch.int32)):
        raise VnetHipError("crop_flip: takes float32 [X,Y,Z,C] or int32 [X,Y,Z], got %s %s" % (src.dtype, tuple(src.shape)))
    X, Y, Z = (int(v) for v in src.shape[:3])
    C = int(src.shape[3]) if src.dim() == 4 else 1
    if any(s < 0 or s >= n or p < 1 for s, p, n in zip(start, size, (X, Y, Z))):
        raise ValueError("crop_flip: window %s + %s on a volume %s" % (start, size, (X, Y, Z)))
    shape = size + tuple(src.shape[3:])
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != src.dtype or
                            out.device != src.device or not out.is_contiguous()):
        raise VnetHipError("crop_flip: out is a dense %s tensor %s on the source's device (%s)" % (src.dtype, shape, src.device))
    if src.device.type != "cuda":
        res = torch.from_numpy(crop_flip_np(src.numpy(), start, size, mask))
        return res if out is None else out.copy_(res)
    if X * Y * Z > MAX_VOXELS or size[0] * size[1] * size[2] > MAX_VOXELS:
        raise VnetHipError("crop_flip: a volume %s or a window %s has more voxels than an int32 indexes" % ((X, Y, Z), size))
    if out is None:
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
    with torch.cuda.device(src.device):
        check(lib().vnet_window_crop_flip(src.data_ptr(), out.data_ptr(), X, Y, Z, C, *start, *size, mask, _stream(src.device)),
              "vnet_window_crop_flip")
    return out


def device_weights(weights, device):
    """weight_vectors' result as three float32 tensors on `device` (None stays None): uploaded once per case, not once per window."""
    if weights is None:
        return None
    return tuple(torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(device) for w in weights)


def accumulate(patch, vol, cnt, origin, mask, weights):
    """vol[origin + (i,j,k), :] += w * patch[f(i,j,k), :]; cnt += w -- IN PLACE, for the window voxels inside the volume (accumulate_np).
    patch float32 [P0,P1,P2,K], vol float32 [D0,D1,D2,K], cnt float32 [D0,D1,D2] or None, weights None (w = 1) or three float32
    vectors of P0, P1, P2 values, all on one device.  Device tensors take the kernel, CPU tensors the rule."""
    origin, mask = ops._three(origin, "accumulate: origin"), _mask(mask)
    if isinstance(patch, torch.Tensor):
        patch = patch.contiguous()
    patch, vol = _dense(patch, "accumulate: patch"), _dense(vol, "accumulate: vol")
    tensors = [("patch", patch), ("vol", vol)]
    if cnt is not None:
        tensors.append(("cnt", _dense(cnt, "accumulate: cnt")))
    if weights is not None:
        weights = tuple(weights)
        if len(weights) != 3:
            raise VnetHipError("accumulate: weights are three vectors or None, got %d" % len(weights))
        tensors += [("w%d" % a, _dense(w, "accumulate: w%d" % a)) for a, w in enumerate(weights)]
    for name, t in tensors:
        if t.dtype != torch.float32:
            raise VnetHipError("accumulate: %s is %s; every tensor is float32" % (name, t.dtype))
        if t.device != vol.device:
            raise VnetHipError("accumulate: %s is on %s, vol on %s" % (name, t.device, vol.device))
    if patch.dim() != 4 or vol.dim() != 4 or patch.shape[3] != vol.shape[3]:
        raise VnetHipError("accumulate: patch [P0,P1,P2,K] and vol [D0,D1,D2,K], got %s and %s" % (tuple(patch.shape), tuple(vol.shape)))
    P, D, K = tuple(int(v) for v in patch.shape[:3]), tuple(int(v) for v in vol.shape[:3]), int(patch.shape[3])
    if cnt is not None and tuple(cnt.shape) != D:
        raise VnetHipError("accumulate: cnt %s for a volume %s" % (tuple(cnt.shape), D))
    if weights is not None and any(w.dim() != 1 or int(w.numel()) != p for w, p in zip(weights, P)):
        raise VnetHipError("accumulate: weight vectors of %s values for a window %s" % ([tuple(w.shape) for w in weights], P))
    if any(o < 0 for o in origin):
        raise ValueError("accumulate: origin %s" % (origin,))
    if not 1 <= K <= MAX_K:
        raise VnetHipError("accumulate: %d classes (1 .. %d)" % (K, MAX_K))
    if vol.device.type != "cuda":
        accumulate_np(patch.numpy(), vol.numpy(), None if cnt is None else cnt.numpy(), origin, mask,
                      None if weights is None else tuple(w.numpy() for w in weights))
        return
    if P[0] * P[1] * P[2] > MAX_VOXELS or D[0] * D[1] * D[2] > MAX_VOXELS:
        raise VnetHipError("accumulate: a volume %s or a window %s has more voxels than an int32 indexes" % (D, P))
    w = (None, None, None) if weights is None else tuple(t.data_ptr() for t in weights)
    with torch.cuda.device(vol.device):
        check(lib().vnet_window_accumulate(patch.data_ptr(), vol.data_ptr(), None if cnt is None else cnt.data_ptr(), K, *P, *origin, *D,
                                           mask, w[0], w[1], w[2], _stream(vol.device)), "vnet_window_accumulate")
