"""NumPy fp64 restatement of the reference's `BSplineDeformation` (pipeline/NiftiDataset3D.py:795-832: sitk.BSplineTransform(3, 3) on the
image's own domain with mesh size (10, 10, 10), then sitk.Resample(image, bspline) and sitk.Resample(label, bspline) onto the image's grid,
default interpolator and default pixel value) -- the oracle of the kernels in csrc/deform.hip (include/vnet_hip_deform.h) and the backend
of loader threads when the transform runs without a device.

Stated from knowledge of ITK, unpinned by the reference (SimpleITK is not installed here).  A sample is [X,Y,Z,(C)],
array axis 0 is ITK's x; origin and direction are shared by image and transform domain, so they cancel: origin 0, direction identity.
    control grid : GRID = 10 + 3 = 13 points per axis, PARAMS = 3 * 13^3 = 6591 doubles in ITK's layout: the displaced component a
                   (x, y, z) slowest, then the z, y, x control indices, x fastest: coef[a * 13^3 + (k * 13 + j) * 13 + i].
    displacement : voxel i_a sits at p_a = i_a * s_a; the control spacing is D_a = n_a * s_a / 10 and the grid's origin -D_a; u = p_a / D_a,
                   m = floor(u), t = u - m, weights ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 on control indices m .. m + 3;
                   d_a = sum_k sum_j sum_i wz_k wy_j wx_i coef_a[k][j][i].  ITK's valid region is 0 <= u < 10 on every axis (true for
                   every voxel centre); outside it the displacement is 0.
    sampling     : c_a = i_a + d_a / s_a; inside iff -0.5 <= c_a < n_a - 0.5 on every axis, outside samples are 0.  Linear exactly as
                   resample.py: b = floor(c), d = c - b, neighbours max(b, 0) and min(b + 1, n - 1), lo + d * (hi - lo) in double along z,
                   then y, then x.  The image is rounded to float once; the LABEL takes the same linear blend, truncated toward zero to
                   its integer type after clamping to the type's range (ITK's static_cast): deformed label borders erode (kept).
Unpinned: ITK's parameter layout, that truncation, and the behaviour at exact ties c = k and c = n - 0.5."""
import numpy as np

MESH = 10
GRID = MESH + 3
PARAMS = 3 * GRID ** 3


def _coef(coef):
    coef = np.asarray(coef, dtype=np.float64)
    if coef.size != PARAMS:
        raise ValueError("bspline_deform: the control grid has %d parameters, got %d" % (PARAMS, coef.size))
    return coef.reshape(3, GRID, GRID, GRID)                         # [a, k (z), j (y), i (x)]


def _spacing(spacing):
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3 or not all(np.isfinite(s) and s > 0 for s in spacing):
        raise ValueError("bspline_deform: spacing must be three finite positive values, got %s" % (spacing,))
    return spacing


def weights(n, spacing):
    """One axis of n voxels of size `spacing`: (m int64 [n], w float64 [n, 4], valid bool [n]) -- voxel i blends the control indices
    m[i] .. m[i] + 3 with the weights w[i]; valid is ITK's region test."""
    n, s = int(n), float(spacing)
    D = n * s / 10.0
    u = (np.arange(n, dtype=np.float64) * s) / D
    f = np.floor(u)
    valid = (u >= 0.0) & (u < 10.0)
    m = np.minimum(np.where(valid, f, 0).astype(np.int64), MESH - 1)
    t = u - f
    t2 = t * t
    t3 = t2 * t
    o = 1.0 - t
    w = np.stack([o * o * o / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0, (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0, t3 / 6.0], axis=1)
    return m, w, valid


def _dense(n, spacing):
    """The weights of one axis as a matrix [n, GRID] (zero off the support)."""
    m, w, valid = weights(n, spacing)
    A = np.zeros((n, GRID), dtype=np.float64)
    rows = np.arange(n)
    for q in range(4):
        A[rows, m + q] = w[:, q]
    return A, valid


def _window(shape, window):
    """The slices of `window` = (start, size) inside a volume of `shape`; None is the whole volume."""
    if window is None:
        return tuple(slice(0, int(n)) for n in shape)
    start, size = (tuple(int(v) for v in w) for w in window)
    if len(start) != 3 or len(size) != 3 or any(s < 0 or w < 1 or s + w > int(n) for s, w, n in zip(start, size, shape)):
        raise ValueError("bspline_deform: window %s + %s does not lie inside the volume %s" % (start, size, tuple(shape)))
    return tuple(slice(s, s + w) for s, w in zip(start, size))


def displacement(shape, spacing, coef, window=None):
    """float64 [X,Y,Z,3]: the displacement (physical units, components x, y, z) at every voxel centre, evaluated separably: one contraction
    per axis, x first, then y, then z.  window = (start, size): only the voxels of that window of the volume, [*size, 3] -- the control
    grid and the valid region stay those of `shape`; only the rows of the three weight matrices are restricted."""
    coef, spacing = _coef(coef), _spacing(spacing)
    (Ax, vx), (Ay, vy), (Az, vz) = ((A[w], v[w]) for (A, v), w in zip((_dense(int(n), s) for n, s in zip(shape, spacing)), _window(shape, window)))
    # each contraction adds its 13 terms in ascending control index, one array operation per term: the order of a voxel's sum does not
    # depend on how many voxels are evaluated with it (np.einsum picks its loop order by the operands' shapes: a window one voxel wide
    # came out an ulp away from the same voxels of the whole volume).  Off the support the weights are exact zeros, so this is also the
    # order of the kernels: ((w0 c0 + w1 c1) + w2 c2) + w3 c3 over the four taps, x first, then y, then z
    t1 = np.zeros(coef.shape[:3] + (Ax.shape[0],), dtype=np.float64)                   # [a, k, j, x]
    for i in range(GRID):
        t1 += Ax[None, None, None, :, i] * coef[..., i, None]
    t2 = np.zeros(coef.shape[:2] + (Ax.shape[0], Ay.shape[0]), dtype=np.float64)      # [a, k, x, y]
    for j in range(GRID):
        t2 += Ay[None, None, None, :, j] * t1[:, :, j, :, None]
    d = np.zeros((Ax.shape[0], Ay.shape[0], Az.shape[0], 3), dtype=np.float64)
    for k in range(GRID):
        d += Az[None, None, :, k, None] * np.moveaxis(t2[:, k], 0, -1)[:, :, None, :]
    ok = vx[:, None, None] & vy[None, :, None] & vz[None, None, :]
    return np.where(ok[..., None], d, 0.0)


def displacement_direct(shape, spacing, coef):
    """The same field as the plain 64-term sum per voxel (a check of `displacement`; small shapes only)."""
    coef, spacing = _coef(coef), _spacing(spacing)
    (mx, wx, vx), (my, wy, vy), (mz, wz, vz) = (weights(int(n), s) for n, s in zip(shape, spacing))
    X, Y, Z = (int(n) for n in shape)
    d = np.zeros((X, Y, Z, 3), dtype=np.float64)
    for k in range(4):
        for j in range(4):
            for i in range(4):
                w = wz[None, None, :, k] * wy[None, :, None, j] * wx[:, None, None, i]
                c = coef[:, (mz + k)[None, None, :], (my + j)[None, :, None], (mx + i)[:, None, None]]
                d += w[..., None] * np.moveaxis(c, 0, -1)
    ok = vx[:, None, None] & vy[None, :, None] & vz[None, None, :]
    return np.where(ok[..., None], d, 0.0)


def source_index(shape, spacing, coef, window=None):
    """float64 [X,Y,Z,3]: the continuous source index c_a = i_a + d_a / s_a of every voxel (window: of the window's voxels alone; the
    indices are those of the volume)."""
    spacing = _spacing(spacing)
    d = displacement(shape, spacing, coef, window)
    grid = np.meshgrid(*(np.arange(w.start, w.stop, dtype=np.float64) for w in _window(shape, window)), indexing="ij")
    return np.stack([g + d[..., a] / spacing[a] for a, g in enumerate(grid)], axis=-1)


def undecidable(shape, spacing, coef, eps=1e-9):
    """bool [X,Y,Z]: voxels whose source index lies within eps of an integer or of n - 0.5 (or -0.5) on some axis: floor(c), the inside
    test and the label's truncation there may differ between two summation orders of the displacement."""
    c = source_index(shape, spacing, coef)
    bad = np.zeros(c.shape[:3], dtype=bool)
    for a, n in enumerate(shape):
        ca = c[..., a]
        bad |= (np.abs(ca - np.rint(ca)) < eps) | (np.abs(ca - (int(n) - 0.5)) < eps) | (np.abs(ca + 0.5) < eps)
    return bad


def linear64(x, coef, spacing, window=None):
    """x [X,Y,Z] or [X,Y,Z,C] (any dtype) -> float64 of the same shape: the 8-tap blend at the deformed position, before its one
    conversion to the output type; 0 outside.  window = (start, size): only the voxels of that window are evaluated, [*size(, C)]; their
    taps are gathered from the whole of x and the inside test is that of the volume."""
    x = np.asarray(x)
    if x.ndim not in (3, 4) or min(x.shape[:3]) < 1:
        raise ValueError("bspline_deform: takes a non-empty [X,Y,Z] or [X,Y,Z,C] volume, got %s" % (x.shape,))
    shape = x.shape[:3]
    c = source_index(shape, spacing, coef, window)
    v = x.astype(np.float64).reshape(shape + (-1,))
    inside = np.ones(c.shape[:3], dtype=bool)
    lo, hi, d = [], [], []
    for a, n in enumerate(shape):
        ca = c[..., a]
        ok = (ca >= -0.5) & (ca < n - 0.5)
        inside &= ok
        f = np.floor(ca)
        b = np.where(ok, f, 0).astype(np.int64)
        lo.append(np.maximum(b, 0))
        hi.append(np.minimum(b + 1, n - 1))
        d.append((ca - f)[..., None])

    def tap(ux, uy, uz):
        return v[hi[0] if ux else lo[0], hi[1] if uy else lo[1], hi[2] if uz else lo[2]]

    def lerp(a, b, w):
        return a + w * (b - a)
    z00, z01 = lerp(tap(0, 0, 0), tap(0, 0, 1), d[2]), lerp(tap(0, 1, 0), tap(0, 1, 1), d[2])
    z10, z11 = lerp(tap(1, 0, 0), tap(1, 0, 1), d[2]), lerp(tap(1, 1, 0), tap(1, 1, 1), d[2])
    out = lerp(lerp(z00, z01, d[1]), lerp(z10, z11, d[1]), d[0])
    return np.where(inside[..., None], out, 0.0).reshape(c.shape[:3] + x.shape[3:])


def linear(image, coef, spacing):
    """float32 result of linear64: the deformed image."""
    return linear64(image, coef, spacing).astype(np.float32)


def label(label, coef, spacing):
    """The deformed label map, in the label's integer dtype: the linear blend truncated toward zero after clamping to the dtype's range."""
    label = np.asarray(label)
    if label.ndim != 3 or not np.issubdtype(label.dtype, np.integer):
        raise ValueError("bspline_deform: a label map is an integer [X,Y,Z] array, got %s %s" % (label.dtype, label.shape))
    info = np.iinfo(label.dtype)
    return np.clip(np.trunc(linear64(label, coef, spacing)), info.min, info.max).astype(label.dtype)
