"""The device ops over csrc/vnet_surface.h (csrc/surface.hip): what the SURFACE scores of Batch_Evaluate run on the device
(vnet_tensorflow_amd/score.py states the rules).  The header is the package's own, not part of the published C
ABI; its entry points live in libvnet_hip.so and are bound by _lib.lib() like every other row of _lib.HEADERS.

Same conventions as _lib / ops: there is NO fallback -- a missing library or a kernel that reports an error raises VnetHipError,
nothing routes to PyTorch or the CPU; ops launch on torch's current stream of the calling thread; outputs are allocated through this
module's `torch` name, scratch comes from ops.workspace.

A label map is an int32 device tensor [X,Y,Z].  A PACKED MASK is an int64 tensor [X,Y,ceil(Z/64)] in morph.py's convention: bit k of
word w is voxel z = 64 w + k, the unused high bits of a row's last word are zero.  The word count loses Z, so the ops that take a mask
take Z beside it.  A list is a 1-D float64 device tensor of non-negative numbers."""
import ctypes

import torch

from . import ops
from ._lib import VnetHipError, check, lib
from .morph import words
from .ops import _thread_stream as _stream

HEADER = "vnet_tensorflow_amd/csrc/vnet_surface.h"        # its row of _lib.HEADERS

MAX_AXIS, MAX_RANKS, MAX_VOXELS = 2048, 4, 2 ** 31 - 1        # VNET_SURFACE_MAX_AXIS, VNET_SURFACE_MAX_RANKS


def _device(x, what):
    if not isinstance(x, torch.Tensor):
        raise VnetHipError("%s: takes a device tensor, got %s" % (what, type(x).__name__))
    if x.device.type != "cuda":
        raise VnetHipError("%s: the tensor is on %s; the kernels run on the device only (no CPU path)" % (what, x.device))


def _volume(x, dtype, what):
    """(X, Y, Z) of a dense 3-D device tensor of `dtype` the kernels take."""
    _device(x, what)
    if x.dim() != 3 or x.numel() == 0 or x.dtype != dtype:
        raise VnetHipError("%s: takes a non-empty %s [X,Y,Z] tensor, got %s %s" % (what, dtype, x.dtype, tuple(x.shape)))
    shape = tuple(int(v) for v in x.shape)
    _sizes(shape, what)
    return shape


def _sizes(shape, what):
    if shape[0] * shape[1] * shape[2] > MAX_VOXELS or max(shape) > MAX_AXIS:
        raise VnetHipError("%s: %dx%dx%d has more voxels than an int32 indexes or an axis above %d" % ((what,) + tuple(shape) + (MAX_AXIS,)))


def _mask(bits, Z, what):
    """(X, Y, Z) of a packed mask with Z voxels per row."""
    _device(bits, what)
    if bits.dim() != 3 or bits.numel() == 0 or bits.dtype != torch.int64:
        raise VnetHipError("%s: a packed mask is a non-empty int64 [X,Y,W] tensor, got %s %s" % (what, bits.dtype, tuple(bits.shape)))
    Z = int(Z)
    if Z < 1 or int(bits.shape[2]) != words(Z):
        raise ValueError("%s: a mask of %d words per row does not hold rows of Z = %d voxels" % (what, int(bits.shape[2]), Z))
    shape = (int(bits.shape[0]), int(bits.shape[1]), Z)
    _sizes(shape, what)
    return shape


def _list(x, what):
    _device(x, what)
    if x.dim() != 1 or x.dtype != torch.float64 or not x.is_contiguous():
        raise VnetHipError("%s: a list is a contiguous 1-D float64 tensor, got %s %s" % (what, x.dtype, tuple(x.shape)))
    return int(x.numel())


def _slot(out, k, device, what):
    """A float64 result of k numbers: `out` (a contiguous float64 device tensor of k elements, e.g. a slice of the caller's) or new."""
    if out is None:
        return torch.empty(k, dtype=torch.float64, device=device)
    if _list(out, what) != k or out.device != device:
        raise ValueError("%s: out holds %d numbers on %s, the result %d on %s" % (what, out.numel(), out.device, k, device))
    return out


def empty_list(n, device):
    """An uninitialised list of n numbers on `device`."""
    return torch.empty(int(n), dtype=torch.float64, device=device)


def surface_bits(label, klass=0):
    """int32 device label map [X,Y,Z] -> the packed surface of the class mask (score.surface_mask): label != 0 for klass 0, label ==
    klass above; the voxels of the mask with one of their 6 neighbours outside it, the volume's edge counting as outside."""
    X, Y, Z = _volume(label, torch.int32, "surface_bits")
    klass = int(klass)
    if klass < 0:
        raise ValueError("surface_bits: klass %d" % klass)
    label = label.contiguous()
    bits = torch.empty((X, Y, words(Z)), dtype=torch.int64, device=label.device)
    with torch.cuda.device(label.device):
        check(lib().vnet_surface_bits(label.data_ptr(), klass, bits.data_ptr(), X, Y, Z, _stream(label.device)), "vnet_surface_bits")
    return bits


def _spacing(spacing, what):
    sp = tuple(float(v) for v in spacing)
    if len(sp) != 3 or not all(0.0 < v < float("inf") for v in sp):
        raise ValueError("%s: spacing %r is not three positive numbers" % (what, spacing))
    return sp


def edt2(bits, Z, spacing=(1.0, 1.0, 1.0)):
    """Packed mask [X,Y,W] of rows of Z voxels -> float64 [X,Y,Z]: the squared Euclidean distance from every voxel to the nearest set
    voxel, voxels `spacing` apart (score.edt2, bit for bit); +inf everywhere for an empty mask.  12 bytes of scratch per voxel."""
    X, Y, Z = _mask(bits, Z, "edt2")
    sp = _spacing(spacing, "edt2")
    bits = bits.contiguous()
    L = lib()
    need = L.vnet_edt2_ws_bytes(X, Y, Z)
    ws = ops.workspace(need, bits.device)
    d2 = torch.empty((X, Y, Z), dtype=torch.float64, device=bits.device)
    with torch.cuda.device(bits.device):
        check(L.vnet_edt2(bits.data_ptr(), d2.data_ptr(), sp[0], sp[1], sp[2], X, Y, Z, ws.data_ptr(), need, _stream(bits.device)), "vnet_edt2")
    return d2


def _gather(d2, at_bits, shape, dst, n, cap):
    X, Y, Z = shape
    L = lib()
    need = L.vnet_surface_gather_ws_bytes(X, Y, Z)
    ws = ops.workspace(need, at_bits.device)
    with torch.cuda.device(at_bits.device):
        check(L.vnet_surface_gather(None if d2 is None else d2.data_ptr(), at_bits.data_ptr(), dst, n.data_ptr(), cap, X, Y, Z,
                                    ws.data_ptr(), need, _stream(at_bits.device)), "vnet_surface_gather")


def popcounts(masks, Z):
    """[number of set voxels] of packed masks of one device with rows of Z voxels: one launch each, ONE read-back of len(masks)
    numbers."""
    masks = list(masks)
    if not masks:
        return []
    shapes = [_mask(m, Z, "popcounts") for m in masks]
    n = torch.empty(len(masks), dtype=torch.int64, device=masks[0].device)
    for k, (m, shape) in enumerate(zip(masks, shapes)):
        if m.device != n.device:
            raise ValueError("popcounts: masks on %s and %s" % (n.device, m.device))
        _gather(None, m.contiguous(), shape, None, n[k:k + 1], 0)
    return [int(v) for v in n.cpu().tolist()]


def gather(d2, at_bits, Z, out=None, offset=0):
    """(list, n): the values of the float64 field d2 [X,Y,Z] at the set voxels of the packed mask at_bits, in voxel (C) order
    (score.gather).  n is a one-element int64 DEVICE tensor with the TRUE number of set voxels -- nothing is read back here.
    out None: a new list of exactly that length (one read-back of the count to size it).  out: a contiguous 1-D float64 device tensor;
    the values go to out[offset:], whose length is the capacity -- values past it are dropped, elements past n are zeroed -- and
    `out` itself is returned (a second gather behind the first fills one buffer)."""
    X, Y, Z = _volume(d2, torch.float64, "gather")
    if _mask(at_bits, Z, "gather")[:2] != (X, Y) or at_bits.device != d2.device:
        raise ValueError("gather: the mask %s does not cover the field %s" % (tuple(at_bits.shape), (X, Y, Z)))
    d2, at_bits = d2.contiguous(), at_bits.contiguous()
    if out is None:
        out, offset = torch.empty(popcounts([at_bits], Z)[0], dtype=torch.float64, device=d2.device), 0
    offset = int(offset)
    if not 0 <= offset <= _list(out, "gather") or out.device != d2.device:
        raise ValueError("gather: offset %d into a list of %d on %s" % (offset, out.numel(), out.device))
    cap = out.numel() - offset
    n = torch.empty(1, dtype=torch.int64, device=d2.device)
    _gather(d2, at_bits, (X, Y, Z), out.data_ptr() + 8 * offset if cap else None, n, cap)
    return out, n


def _ranks(ranks, n, what):
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= MAX_RANKS:
        raise ValueError("%s: takes 1 .. %d ranks, got %d" % (what, MAX_RANKS, len(ranks)))
    if any(r < 0 or r >= n for r in ranks):
        raise ValueError("%s: ranks %r outside a list of %d" % (what, ranks, n))
    return ranks


def kth(values, ranks, out=None):
    """float64 device tensor [len(ranks)]: the elements of 0-based rank ranks[j] (the ranks[j]-th smallest; 1 .. 4 ranks) of a list of
    non-negative numbers, +inf allowed -- exactly np.sort(values)[ranks] (score.kth).  Nothing is read back."""
    n = _list(values, "kth")
    ranks = _ranks(ranks, n, "kth")
    out = _slot(out, len(ranks), values.device, "kth")
    L = lib()
    need = L.vnet_list_select_ws_bytes(n, len(ranks))
    ws = ops.workspace(need, values.device)
    host = (ctypes.c_longlong * len(ranks))(*ranks)
    with torch.cuda.device(values.device):
        check(L.vnet_list_select(values.data_ptr(), n, host, len(ranks), out.data_ptr(), ws.data_ptr(), need, _stream(values.device)),
              "vnet_list_select")
    return out


def root_sum(values, out=None):
    """float64 device tensor [1]: the sum of the square roots of a non-empty list, added in an order that depends on its length alone
    (the same bits from launch to launch; within (n + 2) 2^-52 relative of np.sqrt(values).sum()).  Nothing is read back."""
    n = _list(values, "root_sum")
    if n < 1:
        raise ValueError("root_sum: an empty list")
    out = _slot(out, 1, values.device, "root_sum")
    L = lib()
    need = L.vnet_list_root_sum_ws_bytes(n)
    ws = ops.workspace(need, values.device)
    with torch.cuda.device(values.device):
        check(L.vnet_list_root_sum(values.data_ptr(), n, out.data_ptr(), ws.data_ptr(), need, _stream(values.device)), "vnet_list_root_sum")
    return out
