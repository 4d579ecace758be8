"""NumPy fp64 restatement of the reference's `Resample` geometry (pipeline/NiftiDataset3D.py:345-398: sitk.ResampleImageFilter with the
identity transform, the input's origin and direction, default pixel value 0) -- the oracle of the kernels in csrc/resample.hip
(include/vnet_hip_resample.h) and the backend of CPU worker threads, which must never launch on the device.

Stated from knowledge of ITK, unpinned by the reference (SimpleITK is not installed here).  Origin and direction
are shared, so the axes decouple: output index i reads the source at the continuous index c = i * r, r = (output spacing) / (source
spacing) formed once in double.  Inside iff c < n - 0.5 on every axis (c >= 0 always); outside samples are 0.
    linear : b = floor(c), d = c - b, upper neighbour min(b + 1, n - 1); per axis lo + d * (hi - lo) in double, z then y then x,
             rounded to float once.
    nearest: floor(c + 0.5) (ITK's Math::RoundHalfIntegerUp).
ITK's own index -> point -> index chain is not bit-identical to i * r at exact ties; that is part of the unpinned statement."""
import math

import numpy as np


def output_size(size, spacing, new_spacing):
    """NiftiDataset3D.py:376-380: int(ceil(s * n / s')) per axis."""
    return tuple(int(math.ceil(float(s) * int(n) / float(t))) for n, s, t in zip(size, spacing, new_spacing))


def ratios(spacing, new_spacing):
    """r_a = s'_a / s_a, one double division per axis."""
    return tuple(float(t) / float(s) for s, t in zip(spacing, new_spacing))


def _axis(n_out, r, n):
    c = np.arange(n_out, dtype=np.float64) * float(r)
    inside = c < n - 0.5
    b = np.floor(c)
    d = c - b
    lo = np.where(inside, b, 0).astype(np.int64)
    return inside, lo, np.minimum(lo + 1, n - 1), d, c


def _check(shape3, out_size, ratio):
    out_size, ratio = tuple(int(v) for v in out_size), tuple(float(v) for v in ratio)
    if len(out_size) != 3 or len(ratio) != 3 or min(out_size) < 1 or min(shape3) < 1:
        raise ValueError("resample: sizes must be three positive integers, got %s -> %s" % (tuple(shape3), out_size))
    if not all(math.isfinite(r) and r > 0 for r in ratio):
        raise ValueError("resample: ratios must be finite and positive, got %s" % (ratio,))
    return out_size, ratio


def linear64(x, out_size, ratio, divisor=None):
    """x [X,Y,Z] or [X,Y,Z,C] -> float64 of the output size: the blend before its one rounding to float.
    divisor [X,Y,Z]: every tap is x / divisor in double, 0 where the divisor is 0."""
    x = np.asarray(x)
    out_size, ratio = _check(x.shape[:3], out_size, ratio)
    v = x.astype(np.float64)
    if divisor is not None:
        dv = np.asarray(divisor, dtype=np.float64)
        dv = dv.reshape(dv.shape + (1,) * (v.ndim - 3))
        v = np.divide(v, dv, out=np.zeros_like(v), where=dv != 0)
    inside = []
    for a in (2, 1, 0):                                            # z, then y, then x: the order of the kernel's lerps
        ok, lo, hi, d, _ = _axis(out_size[a], ratio[a], x.shape[a])
        inside.insert(0, ok)
        d = d.reshape((-1,) + (1,) * (v.ndim - 1 - a))
        vl, vh = np.take(v, lo, axis=a), np.take(v, hi, axis=a)
        v = vl + d * (vh - vl)
    mask = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
    return np.where(mask.reshape(mask.shape + (1,) * (v.ndim - 3)), v, 0.0)


def linear(x, out_size, ratio, divisor=None):
    """float32 result of linear64."""
    return linear64(x, out_size, ratio, divisor).astype(np.float32)


def nearest(x, out_size, ratio):
    """x [X,Y,Z] (any dtype) -> the same dtype on the output grid."""
    x = np.asarray(x)
    out_size, ratio = _check(x.shape[:3], out_size, ratio)
    idx, inside = [], []
    for a in range(3):
        ok, _, _, _, c = _axis(out_size[a], ratio[a], x.shape[a])
        inside.append(ok)
        idx.append(np.where(ok, np.minimum(np.floor(c + 0.5), x.shape[a] - 1), 0).astype(np.int64))
    out = x[np.ix_(idx[0], idx[1], idx[2])]
    mask = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
    return np.where(mask, out, np.zeros((), dtype=x.dtype))
