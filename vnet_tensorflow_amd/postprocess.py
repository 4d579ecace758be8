"""The post-processing pipeline of evaluate() and Batch_Evaluate: steps that clean the label class by class, read from YAML and run on
the int32 device label before it is copied out and before `on_label` hands it to the scorer.  Not in the
reference, whose feature list ends with it unchecked.

This module STATES every rule as a NumPy / scipy restatement (the functions of the first half): they are the yardstick the kernels are
held `==` to, and the route of an ndarray label and of a CPU model.  The second half is the ctypes binding of libvnet_post.so
(csrc/vnet_post.h, csrc/postprocess.hip) and its device ops.  A library of its own beside libvnet_hip.so: the header is the package's
own, not part of the published C ABI, and none of this is in _lib.HEADERS.

The rules.  L is the running label [X,Y,Z]; `classes` is a list of 1 .. 16 distinct class values, by default every non-zero class
1 .. K-1 in ascending order; class 0 is refused.  Connectivity is face connectivity (6 neighbours), as in csrc/components.hip.
  KeepLargestComponent(classes)       each class c on its own: of the components of L == c the one with the most voxels stays, of equal
                                      counts the one whose first voxel comes first in C order; every other voxel of class c becomes 0.
                                      Voxels of other classes are untouched: classes 2 and 5 side by side are not connected.
  RemoveSmallComponents(volume, ...)  a component of L == c stays iff (double)count * prod(spacing) > volume: strict, in double, as
                                      model.volume_threshold; spacing is that of the grid the label is returned on.
  FillHoles(classes)                  for each c in order, on the running label: H = binary_fill_holes(L == c) & (L == 0); L[H] = c.
                                      The 6-connected components of the complement of the class mask that touch no face of the volume
                                      are cavities; only their background voxels are filled -- a tumour inside a liver stays.
  Dilate / Erode / Open / Close(radius, classes)   1 <= radius <= 8 with prepare_data.ball(radius); for each c in order on the running
                                      label: M = (L == c), M' = op(M), L = where(M' & (L == 0), c, where((L == c) & ~M', 0, L)): a
                                      class grows into the background only.  Dilation takes the outside of the volume as 0
                                      (prepare_data.dilate), erosion as 1 (~dilate(~M)); Open = dilate(erode), Close = erode(dilate).

Same conventions as _lib / ops on the device side: there is NO fallback -- a missing library or a kernel that reports an error raises
VnetHipError; ops launch on torch's current stream of the calling thread; outputs are allocated through this module's `torch` name,
scratch comes from ops.workspace."""
import ctypes
import os

import numpy as np
import torch

from . import morph, ops, prepare_data
from ._lib import VnetHipError, check
from .ops import _thread_stream as _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VNET_POST_LIB") or os.path.join(_HERE, "libvnet_post.so")
HEADER = "vnet_tensorflow_amd/csrc/vnet_post.h"

MAX_CLASSES, MAX_RADIUS, MAX_VOXELS = 16, 8, 2 ** 31 - 1            # VNET_POST_MAX_VALUES, VNET_TOOLS_MAX_RADIUS


# ---- the rules ----------------------------------------------------------------------------------------------------------------------------
def check_classes(classes):
    """The class list of a step as the rules take it: 1 .. 16 distinct integers, none of them 0."""
    if isinstance(classes, (int, np.integer)) and not isinstance(classes, bool):
        classes = [classes]
    out = []
    for c in classes:
        if isinstance(c, bool) or int(c) != c:
            raise ValueError("postprocess: class %r is not an integer" % (c,))
        out.append(int(c))
    if not 1 <= len(out) <= MAX_CLASSES:
        raise ValueError("postprocess: a step takes 1 .. %d classes, got %d" % (MAX_CLASSES, len(out)))
    if 0 in out:
        raise ValueError("postprocess: class 0 is the background and cannot be post-processed (classes %r)" % (out,))
    if len(set(out)) != len(out):
        raise ValueError("postprocess: classes %r are not distinct" % (out,))
    if any(c < -2 ** 31 or c > 2 ** 31 - 1 for c in out):
        raise ValueError("postprocess: classes %r outside int32" % (out,))
    return out


def default_classes(K):
    """Every non-zero class of a K-class label, ascending."""
    K = int(K)
    if K - 1 > MAX_CLASSES:
        raise ValueError("postprocess: %d classes; a step takes at most %d, name them with `classes:`" % (K - 1, MAX_CLASSES))
    return list(range(1, K))


def _label3(label):
    label = np.asarray(label)
    if label.ndim != 3 or label.size == 0:
        raise ValueError("postprocess: takes a non-empty [X,Y,Z] label, got %s" % (label.shape,))
    return label


def _components(mask):
    """(component map 1 .. n in the C order of the first voxels, counts[0 .. n]) of a mask under face connectivity."""
    from scipy import ndimage
    cc, n = ndimage.label(mask)                      # (default structure: the 6 face neighbours)
    return cc, np.bincount(cc.ravel(), minlength=n + 1)


def class_roots(label, values):
    """vnet_post_class_roots as a rule: (roots, sizes) int32 -- the smallest linear index of the voxel's component of its own class, -1
    where the class is not one of `values`; the component's count at its representative, 0 elsewhere."""
    label = _label3(label)
    roots = np.full(label.size, -1, dtype=np.int32)
    sizes = np.zeros(label.size, dtype=np.int32)
    for c in check_classes(values):
        cc, counts = _components(label == c)
        flat = cc.ravel()
        idx = np.flatnonzero(flat)
        first = np.full(counts.size, -1, dtype=np.int64)
        first[flat[idx][::-1]] = idx[::-1]
        roots[idx] = first[flat[idx]]
        sizes[first[1:]] = counts[1:]
    return roots.reshape(label.shape), sizes.reshape(label.shape)


def keep_largest(label, classes):
    label = _label3(label)
    out = label.copy()
    for c in check_classes(classes):
        cc, counts = _components(label == c)
        if counts.size > 1:
            best = int(np.argmax(counts[1:])) + 1            # (the first maximum: components are numbered by their first voxel)
            out[(cc != 0) & (cc != best)] = 0
    return out


def voxel_volume(spacing):
    return float(np.prod(spacing))                   # the double model.volume_threshold forms


def remove_small(label, volume, spacing, classes):
    label = _label3(label)
    out = label.copy()
    vv = voxel_volume(spacing)
    for c in check_classes(classes):
        cc, counts = _components(label == c)
        keep = counts.astype(np.float64) * vv > float(volume)
        keep[0] = True
        out[~keep[cc]] = 0
    return out


def fill_holes(label, classes):
    from scipy import ndimage
    out = _label3(label).copy()
    for c in check_classes(classes):
        out[ndimage.binary_fill_holes(out == c) & (out == 0)] = c        # (default structure: face connectivity)
    return out


def _radius(r):
    if isinstance(r, bool) or int(r) != r or not 1 <= int(r) <= MAX_RADIUS:
        raise ValueError("postprocess: radius %r (an integer 1 .. %d)" % (r, MAX_RADIUS))
    return int(r)


def dilate_mask(mask, r):
    return prepare_data.dilate(np.asarray(mask, dtype=np.uint8), _radius(r)).astype(bool)            # outside the volume: 0


def erode_mask(mask, r):
    return ~dilate_mask(~np.asarray(mask, dtype=bool), r)                                            # outside the volume: 1


def open_mask(mask, r):
    return dilate_mask(erode_mask(mask, r), r)


def close_mask(mask, r):
    return erode_mask(dilate_mask(mask, r), r)


MASK_OPS = {"Dilate": dilate_mask, "Erode": erode_mask, "Open": open_mask, "Close": close_mask}


def apply_mask(label, mask, c):
    """The write-back of a class mask: the class grows into the background only and never overwrites another class."""
    return np.where(mask & (label == 0), np.asarray(c, dtype=label.dtype), np.where((label == c) & ~mask, np.asarray(0, dtype=label.dtype), label))


def morphology(label, op, radius, classes):
    out = _label3(label).copy()
    for c in check_classes(classes):
        out = apply_mask(out, MASK_OPS[op](out == c, radius), c)
    return out


# ---- the steps ----------------------------------------------------------------------------------------------------------------------------
class Step(object):
    """One step of the pipeline.  classes None: every non-zero class of the label it is run on."""
    VARIABLES = ("classes",)

    def __init__(self, classes=None):
        self.classes = None if classes is None else check_classes(classes)

    def _of(self, default):
        return self.classes if self.classes is not None else list(default)

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.VARIABLES))


class KeepLargestComponent(Step):
    def host(self, label, spacing, default):
        return keep_largest(label, self._of(default))

    def device(self, label, spacing, default):
        return filter_components(label, self._of(default), 0)


class RemoveSmallComponents(Step):
    VARIABLES = ("volume", "classes")

    def __init__(self, volume, classes=None):
        Step.__init__(self, classes)
        self.volume = float(volume)
        if not np.isfinite(self.volume):
            raise ValueError("postprocess: RemoveSmallComponents volume %r is not finite" % (volume,))

    def host(self, label, spacing, default):
        return remove_small(label, self.volume, spacing, self._of(default))

    def device(self, label, spacing, default):
        return filter_components(label, self._of(default), 1, self.volume, voxel_volume(spacing))


class FillHoles(Step):
    def host(self, label, spacing, default):
        return fill_holes(label, self._of(default))

    def device(self, label, spacing, default):
        for c in self._of(default):
            label = fill_holes_class(label, c)
        return label


class _Morphology(Step):
    VARIABLES = ("radius", "classes")

    def __init__(self, radius, classes=None):
        Step.__init__(self, classes)
        self.radius = _radius(radius)

    def host(self, label, spacing, default):
        return morphology(label, type(self).__name__, self.radius, self._of(default))

    def device(self, label, spacing, default):
        Z, r = int(label.shape[2]), self.radius
        for c in self._of(default):
            label = apply_bits(label, self.bits(morph.select_bits(label, [c]), Z, r), c)
        return label


def _erode_bits(bits, Z, r):
    return not_bits(morph.dilate_bits(not_bits(bits, Z), Z, r), Z)


class Dilate(_Morphology):
    @staticmethod
    def bits(bits, Z, r):
        return morph.dilate_bits(bits, Z, r)


class Erode(_Morphology):
    bits = staticmethod(_erode_bits)


class Open(_Morphology):
    @staticmethod
    def bits(bits, Z, r):
        return morph.dilate_bits(_erode_bits(bits, Z, r), Z, r)


class Close(_Morphology):
    @staticmethod
    def bits(bits, Z, r):
        return _erode_bits(morph.dilate_bits(bits, Z, r), Z, r)


REGISTRY = {c.__name__: c for c in (KeepLargestComponent, RemoveSmallComponents, FillHoles, Dilate, Erode, Open, Close)}


def build_steps(entries):
    """[step] of a list of {name:, variables:} entries (the dialect of the `preprocess:` section)."""
    out = []
    for t in entries or []:
        if not isinstance(t, dict) or "name" not in t:
            raise ValueError("postprocess: a step is a mapping with `name:` (and `variables:`), got %r" % (t,))
        name = t["name"]
        if name not in REGISTRY:
            raise ValueError("postprocess: unknown step %r (known: %s)" % (name, ", ".join(sorted(REGISTRY))))
        extra = sorted(set(t) - {"name", "variables"})
        if extra:
            raise ValueError("postprocess: step %r has unknown key %r" % (name, extra[0]))
        kw = dict(t.get("variables") or {})
        cls = REGISTRY[name]
        for k in kw:
            if k not in cls.VARIABLES:
                raise ValueError("postprocess: step %r has no variable %r (it takes: %s)" % (name, k, ", ".join(cls.VARIABLES)))
        missing = [k for k in cls.VARIABLES if k != "classes" and k not in kw]
        if missing:
            raise ValueError("postprocess: step %r needs the variable %r" % (name, missing[0]))
        out.append(cls(**kw))
    return out


def build(path):
    """[step] of postprocess -> evaluate -> 3D of a YAML file (which may be the one EvaluationSetting.Pipeline names)."""
    import yaml
    with open(path) as f:
        spec = yaml.load(f, Loader=yaml.SafeLoader) or {}
    return build_steps(((spec.get("postprocess") or {}).get("evaluate") or {}).get("3D") or [])


def run(steps, label, spacing=(1.0, 1.0, 1.0), classes=None):
    """The steps in order on `label`: an int32 device tensor goes to the kernels and gives an int32 device tensor; an ndarray (or a CPU
    tensor: a CPU model's label) goes to the restatements and comes back in its own type.  classes: K, the number of classes of the
    label (a step without `classes:` takes 1 .. K-1), or the default class list itself; None reads the label's largest value."""
    spacing = tuple(float(v) for v in spacing)
    if len(spacing) != 3:
        raise ValueError("postprocess: spacing %r is not three numbers" % (spacing,))
    steps = list(steps or [])
    tensor = isinstance(label, torch.Tensor)
    on_device = tensor and label.device.type == "cuda"
    if on_device and (label.dtype != torch.int32 or label.dim() != 3 or label.numel() == 0):
        raise VnetHipError("postprocess.run: a device label is a non-empty int32 [X,Y,Z] tensor, got %s %s" % (label.dtype, tuple(label.shape)))
    if classes is None and any(s.classes is None for s in steps):
        classes = int(label.max()) + 1
    default = [] if classes is None else (default_classes(classes) if isinstance(classes, (int, np.integer)) else check_classes(classes))
    if on_device:
        out = label.contiguous()
        for s in steps:
            if s._of(default):
                out = s.device(out, spacing, default)
        return out
    host = label.numpy() if tensor else _label3(label)
    for s in steps:
        if s._of(default):
            host = s.host(host, spacing, default)
    return torch.from_numpy(np.ascontiguousarray(host)) if tensor else host


# ---- libvnet_post.so ----------------------------------------------------------------------------------------------------------------------
_vp, _i, _sz, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes) : every symbol csrc/vnet_post.h declares (tests/test_postprocess_host.py holds the table to the header)
SIGNATURES_POST = {
    "vnet_post_class_roots": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "vnet_post_filter_components_ws_bytes": (_sz, [_i, _i, _i]),
    "vnet_post_filter_components": (_i, [_vp, _vp, _vp, _i, _i, _d, _d, _i, _i, _i, _vp, _sz, _vp]),
    "vnet_post_fill_holes_ws_bytes": (_sz, [_i, _i, _i]),
    "vnet_post_fill_holes": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "vnet_post_not_bits": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "vnet_post_apply_bits": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp]),
}

_post = None


def lib():
    """The loaded libvnet_post.so (raises if it has not been built: there is no fallback path)."""
    global _post
    if _post is None:
        if not os.path.exists(LIB_PATH):
            raise VnetHipError("libvnet_post.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc, gfx950).  The HIP library is the only compute path." % LIB_PATH)
        # torch (imported above) has loaded its own libamdhip64 by now: both libraries and torch's streams live in ONE HIP runtime
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES_POST.items():
            fn = getattr(L, name)              # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        _post = L
    return _post


def _device_label(label, what):
    """(X, Y, Z) of an int32 device label the kernels take."""
    if not isinstance(label, torch.Tensor):
        raise VnetHipError("%s: takes a device tensor, got %s" % (what, type(label).__name__))
    if label.device.type != "cuda":
        raise VnetHipError("%s: the tensor is on %s; the kernels run on the device only (postprocess.run takes the rules)" % (what, label.device))
    if label.dim() != 3 or label.numel() == 0 or label.dtype != torch.int32:
        raise VnetHipError("%s: takes a non-empty int32 [X,Y,Z] label, got %s %s" % (what, label.dtype, tuple(label.shape)))
    if label.numel() > MAX_VOXELS:
        raise VnetHipError("%s: %dx%dx%d has more voxels than an int32 indexes" % ((what,) + tuple(label.shape)))
    return tuple(int(v) for v in label.shape)


def _values(values):
    values = check_classes(values)
    return (ctypes.c_int * len(values))(*values), len(values)


def class_roots_device(label, values, sizes=False):
    """int32 device label -> int32 [X,Y,Z]: the smallest linear index of the voxel's component of its own class, -1 where the class is
    not one of `values` (class_roots).  sizes=True: also the count at each representative, 0 elsewhere.  One labelling for all classes."""
    X, Y, Z = _device_label(label, "class_roots")
    host, n = _values(values)
    label = label.contiguous()
    roots = torch.empty((X, Y, Z), dtype=torch.int32, device=label.device)
    cnt = torch.empty((X, Y, Z), dtype=torch.int32, device=label.device) if sizes else None
    with torch.cuda.device(label.device):
        check(lib().vnet_post_class_roots(label.data_ptr(), host, n, roots.data_ptr(), None if cnt is None else cnt.data_ptr(), X, Y, Z,
                                          _stream(label.device)), "vnet_post_class_roots")
    return (roots, cnt) if sizes else roots


def filter_components(label, values, mode, volume=0.0, voxel_volume=1.0):
    """int32 device label -> the label without the components of the classes in `values` that mode 0 (keep_largest) or mode 1
    (remove_small: `(double)count * voxel_volume > volume` stays) drops; class values kept."""
    X, Y, Z = _device_label(label, "filter_components")
    host, n = _values(values)
    label = label.contiguous()
    L = lib()
    need = L.vnet_post_filter_components_ws_bytes(X, Y, Z)
    out = torch.empty((X, Y, Z), dtype=torch.int32, device=label.device)
    ws = ops.workspace(need, label.device)
    with torch.cuda.device(label.device):
        check(L.vnet_post_filter_components(label.data_ptr(), out.data_ptr(), host, n, int(mode), float(volume), float(voxel_volume), X, Y, Z,
                                            ws.data_ptr(), need, _stream(label.device)), "vnet_post_filter_components")
    return out


def fill_holes_class(label, klass):
    """int32 device label -> the label with the background voxels inside the cavities of class `klass` set to it (fill_holes, one class)."""
    X, Y, Z = _device_label(label, "fill_holes_class")
    klass = check_classes([klass])[0]
    label = label.contiguous()
    L = lib()
    need = L.vnet_post_fill_holes_ws_bytes(X, Y, Z)
    out = torch.empty((X, Y, Z), dtype=torch.int32, device=label.device)
    ws = ops.workspace(need, label.device)
    with torch.cuda.device(label.device):
        check(L.vnet_post_fill_holes(label.data_ptr(), out.data_ptr(), klass, X, Y, Z, ws.data_ptr(), need, _stream(label.device)),
              "vnet_post_fill_holes")
    return out


def not_bits(bits, C):
    """Packed mask [A,B,W] of rows of C voxels (morph.py's layout) -> its complement inside the volume; the bits at c >= C stay zero."""
    A, B, C = morph._mask(bits, C, "not_bits")
    bits = bits.contiguous()
    out = torch.empty((A, B, morph.words(C)), dtype=torch.int64, device=bits.device)
    with torch.cuda.device(bits.device):
        check(lib().vnet_post_not_bits(bits.data_ptr(), out.data_ptr(), A, B, C, _stream(bits.device)), "vnet_post_not_bits")
    return out


def apply_bits(label, bits, klass):
    """int32 device label, packed mask of class `klass` -> the label with the mask written back (apply_mask)."""
    A, B, C = _device_label(label, "apply_bits")
    klass = check_classes([klass])[0]
    if morph._mask(bits, C, "apply_bits")[:2] != (A, B) or bits.device != label.device:
        raise ValueError("apply_bits: the mask %s does not cover the label %s" % (tuple(bits.shape), (A, B, C)))
    label, bits = label.contiguous(), bits.contiguous()
    out = torch.empty((A, B, C), dtype=torch.int32, device=label.device)
    with torch.cuda.device(label.device):
        check(lib().vnet_post_apply_bits(label.data_ptr(), bits.data_ptr(), klass, out.data_ptr(), A, B, C, _stream(label.device)),
              "vnet_post_apply_bits")
    return out
