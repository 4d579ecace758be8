"""NumPy restatements of include/vnet_hip_sample.h -- the yardsticks of its tests and the statement of its rules.

Noise.  The normal deviate of output element e (flat index of the [P0,P1,P2,C] patch) is a function of (seed, e) alone:
Philox4x32-10 with key (seed & 0xFFFFFFFF, seed >> 32) and counter (q & 0xFFFFFFFF, q >> 32, 0, 0), q = e >> 2, gives four words
k0..k3; (k0, k1) is the Box-Muller pair of elements 4q and 4q + 1, (k2, k3) the pair of 4q + 2 and 4q + 3:
    u1 = ((k >> 9) + 0.5) * 2^-23   in (0, 1)       u2 = (k' >> 8) * 2^-24   in [0, 1)        (both exact in float32)
    r = sqrt(-2 ln u1), theta = 2 pi u2, z = r cos(theta) for the even element, r sin(theta) for the odd one.
The device evaluates r, theta and z in float32 with the precise logf / sqrtf / cosf / sinf and forms fmaf(sigma, z, x); here
Philox is written out in uint32 / uint64 arithmetic and Box-Muller runs in float64.  The two differ by less than 5e-6 in z:
r <= sqrt(2 * 24 * ln 2) = 5.77, the float32 angle is within 2^-22 of 2 pi u2, and logf, sinf, cosf are within 2 ulp.

Table.  Row k of the component table is scipy.ndimage.label's component k + 1 (face connectivity, numbered in C order of first
voxels -- tests/test_components_host.py pins that): {representative, count, lo[3], hi[3]}, the bounding box of find_objects with hi
inclusive."""
import numpy as np

ROW = 8                       # VNET_CC_ROW
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or scalars) of one shape, key: 2 uint32 scalars or arrays -> 4 uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint32)) for c in counter)
    k0, k1 = (np.atleast_1d(np.asarray(k, dtype=np.uint32)) for k in key)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0, p1 = c0.astype(np.uint64) * _M0, c2.astype(np.uint64) * _M1
            h0, l0 = (p0 >> _S32).astype(np.uint32), (p0 & _LO).astype(np.uint32)
            h1, l1 = (p1 >> _S32).astype(np.uint32), (p1 & _LO).astype(np.uint32)
            c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
            k0, k1 = k0 + _W0, k1 + _W1
    return c0, c1, c2, c3


def normal(seed, count, first=0):
    """float64 [count]: the deviates of output elements first .. first + count - 1 under `seed` (a 64-bit integer)."""
    seed = int(seed) & (2 ** 64 - 1)
    first, count = int(first), int(count)
    q0, q1 = first >> 2, (first + count + 3) >> 2
    q = np.arange(q0, q1, dtype=np.uint64)
    k = philox4x32_10(((q & _LO).astype(np.uint32), (q >> _S32).astype(np.uint32), np.zeros(q.shape, np.uint32), np.zeros(q.shape, np.uint32)),
                      (np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)))
    z = np.empty((q.size, 4), dtype=np.float64)
    for pair in range(2):
        u1 = ((k[2 * pair] >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        u2 = (k[2 * pair + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        z[:, 2 * pair], z[:, 2 * pair + 1] = r * np.cos(th), r * np.sin(th)
    off = first - 4 * q0
    return z.reshape(-1)[off:off + count]


def flip_axes(mask):
    return tuple(a for a in range(3) if (int(mask) >> a) & 1)


def patch(image, label, start, size, flip=0, sigma=0.0, seed=0):
    """The sample vnet_sample_patch writes: (float64 [P0,P1,P2,C] -- exactly the float32 crop when sigma is 0 --, label [P0,P1,P2])."""
    sl = tuple(slice(int(s), int(s) + int(n)) for s, n in zip(start, size))
    img, lab = np.flip(image[sl], flip_axes(flip)), np.flip(label[sl], flip_axes(flip))
    img = np.ascontiguousarray(img)
    if sigma:
        img = img.astype(np.float64) + float(sigma) * normal(seed, img.size).reshape(img.shape)
    return img, np.ascontiguousarray(lab)


def deform_patch(image, label, coef, spacing, start, size, flip=0, sigma=0.0, seed=0):
    """The sample vnet_deform_sample_patch writes (include/vnet_hip_deform_sample.h) from the UNDEFORMED case: what
    patch(deform.linear(image, coef, spacing), deform.label(label, coef, spacing), start, size, flip, sigma, seed) returns, evaluated
    for the voxels of the window alone -- deform.linear64 restricted to the window: the displacement from the rows of the volume's
    weight matrices that belong to it, the taps gathered from the whole volume, the inside test against the volume."""
    from . import deform as D
    image, label = np.asarray(image), np.asarray(label)
    if image.ndim != 4 or label.ndim != 3 or image.shape[:3] != label.shape or not np.issubdtype(label.dtype, np.integer):
        raise ValueError("deform_patch: image [X,Y,Z,C] and an integer label [X,Y,Z] of one grid, got %s / %s %s" % (image.shape, label.dtype, label.shape))
    window = (tuple(int(s) for s in start), tuple(int(n) for n in size))
    img = D.linear64(image, coef, spacing, window).astype(np.float32)
    info = np.iinfo(label.dtype)
    lab = np.clip(np.trunc(D.linear64(label, coef, spacing, window)), info.min, info.max).astype(label.dtype)
    img, lab = np.ascontiguousarray(np.flip(img, flip_axes(flip))), np.ascontiguousarray(np.flip(lab, flip_axes(flip)))
    if sigma:
        img = img.astype(np.float64) + float(sigma) * normal(seed, img.size).reshape(img.shape)
    return img, lab


def component_table(label):
    """(n, int32 [n, ROW]) of label != 0 from ndimage.label + find_objects."""
    from scipy import ndimage
    label = np.asarray(label)
    cc, n = ndimage.label(label != 0)
    rows = np.zeros((n, ROW), dtype=np.int32)
    if n:
        flat = cc.reshape(-1)
        vals, first = np.unique(flat, return_index=True)               # (first occurrence of every value, values ascending)
        rows[:, 0] = first[vals > 0]
        rows[:, 1] = np.bincount(flat, minlength=n + 1)[1:]
        for k, box in enumerate(ndimage.find_objects(cc)):
            rows[k, 2:5] = [s.start for s in box]
            rows[k, 5:8] = [s.stop - 1 for s in box]
    return n, rows


def window_count(label, start, size, lo, hi):
    sl = tuple(slice(int(s), int(s) + int(n)) for s, n in zip(start, size))
    w = np.asarray(label)[sl].astype(np.int64)
    return int(((w >= lo) & (w <= hi)).sum()), int(w.sum())
