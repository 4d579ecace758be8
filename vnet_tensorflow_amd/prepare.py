"""A case of evaluate prepared on the device (include/vnet_hip_prepare.h): the host side of the intensity windows, the NumPy
restatements of the four kernels -- the yardsticks of their tests and the statement of their rules -- and prepare_on_device, which
applies a deterministic pipeline to device tensors.

The four normalisations of transforms.py are one intensity window per channel, [wmin, wmax] -> [0, 255], whose ends follow from four
numbers of the channel: sum, css = sum (v - mean)^2, min, max.  The device forms those (ops.channel_stats), the host turns them into the
window with the arithmetic of transforms.py, operation for operation (window_params), and the device applies it (ops.window_intensity):
per normalisation a [C, 4] read-back and a [C, 5] upload cross the bus, the volume never does.
    row of the window table: {a, b, wmin, scale, flag};  v = ((double)x - a) / b  (a, b = 0, 1 unless StatisticalNormalization's
    pre_norm put sitk.NormalizeImageFilter in front);  flag 0: clip((v - wmin) * scale + 0.0, 0, 255), scale = 255.0 / (wmax - wmin);
    flag 1 (wmax == wmin): v < wmin ? 0 : 255.  One rounding to float.  That is transforms._window."""
import numpy as np

from . import transforms as T

SUM, CSS, MIN, MAX = range(4)
NORMALISATIONS = (T.Normalization, T.StatisticalNormalization, T.ExtremumNormalization, T.ManualNormalization)
ON_DEVICE = NORMALISATIONS + (T.Resample, T.Padding)


# ---- NumPy restatements of the kernels ----------------------------------------------------------------------------------------------
def channel_stats(image, pre=None):
    """image [..., C] -> float64 [C, 4] = {sum, css, min, max} of v = (x - a) / b in double (pre [C, 2] = {a, b}; None: v = x), summed
    the way NumPy's mean() and std() sum (pairwise): css = sum (v - sum / n)^2."""
    image = np.asarray(image)
    C = image.shape[-1]
    out = np.empty((C, 4), np.float64)
    with np.errstate(all="ignore"):
        for c in range(C):
            v = image[..., c].astype(np.float64)
            if pre is not None:
                v = (v - pre[c][0]) / pre[c][1]
            s = v.sum()
            out[c] = s, ((v - s / v.size) ** 2).sum(), v.min(), v.max()
    return out


def window_intensity(image, prm):
    """image [..., C], prm [C, 5] -> float32: the rule of vnet_window_intensity."""
    image = np.asarray(image)
    out = np.empty(image.shape, np.float32)
    with np.errstate(all="ignore"):
        for c in range(image.shape[-1]):
            a, b, wmin, scale, flag = (np.float64(p) for p in prm[c])
            v = (image[..., c].astype(np.float64) - a) / b
            if flag != 0:
                out[..., c] = np.where(v < wmin, 0.0, 255.0)
            else:
                out[..., c] = np.clip((v - wmin) * scale + 0.0, 0.0, 255.0)
    return out


def crop_window(src, start, size):
    """The window of `size` voxels at `start` over the three leading axes, 0 past the extent: np.pad, then slice."""
    src = np.asarray(src)
    pads = [(0, max(s + p - n, 0)) for s, p, n in zip(start, size, src.shape[:3])] + [(0, 0)] * (src.ndim - 3)
    return np.ascontiguousarray(np.pad(src, pads)[tuple(slice(s, s + p) for s, p in zip(start, size))])


def argmax_label(vol):
    return np.argmax(np.asarray(vol), axis=-1).astype(np.int32)


# ---- statistics -> window -----------------------------------------------------------------------------------------------------------
def stats_passes(transform):
    """How many ops.channel_stats passes window_params needs for `transform`: 0 (ManualNormalization), 1, or 2 (pre_norm)."""
    if type(transform) is T.ManualNormalization:
        return 0
    return 2 if type(transform) is T.StatisticalNormalization and transform.pre_norm else 1


def _moments(stats, n):
    """(mean, std with ddof = 1) per channel as ndarray.mean() and ndarray.std(ddof=1) form them from the sum and the css."""
    with np.errstate(all="ignore"):
        s, css = np.asarray(stats, np.float64)[:, SUM], np.asarray(stats, np.float64)[:, CSS]
        return s / n, np.sqrt(css / max(n - 1, 0))


def pre_map(stats, n):
    """[C, 2] = {mean, std} of a first statistics pass: sitk.NormalizeImageFilter as the pre-map of the second
    (StatisticalNormalization(pre_norm=True))."""
    return np.stack(_moments(stats, n), axis=1)


def window_params(transform, stats, n, pre=None, channels=None):
    """float64 [C, 5] rows {a, b, wmin, scale, flag} of the window that `transform` (one of the four normalisations) applies to a
    volume of n voxels whose channels have the statistics `stats` ([C, 4] = {sum, css, min, max} of (x - a) / b, pre = [C, 2] = {a, b}
    or None for 0, 1) -- the arithmetic of transforms.py, operation for operation.  ManualNormalization needs no statistics:
    stats None and `channels` given."""
    kind = type(transform)
    if kind not in NORMALISATIONS:
        raise TypeError("window_params: %r is not an intensity normalisation" % (transform,))
    if stats is not None:
        stats = np.asarray(stats, np.float64)
        C = stats.shape[0]
    elif kind is T.ManualNormalization and channels is not None:
        C = int(channels)
    else:
        raise ValueError("window_params: %s needs the channel statistics" % kind.__name__)
    out = np.empty((C, 5), np.float64)
    out[:, 0], out[:, 1] = 0.0, 1.0
    if pre is not None:
        out[:, :2] = np.asarray(pre, np.float64)
    with np.errstate(all="ignore"):
        if kind is T.StatisticalNormalization:
            mean, std = _moments(stats, n)
        for c in range(C):
            if kind is T.ManualNormalization:
                wmin, wmax = transform.windowMin, transform.windowMax
            elif kind is T.Normalization:
                wmin, wmax = stats[c, MIN], stats[c, MAX]
            elif kind is T.ExtremumNormalization:
                lo, hi = stats[c, MIN], stats[c, MAX]
                wmin, wmax = (hi - lo) * transform.percent + lo, (hi - lo) * (1 - transform.percent) + lo
            else:
                mu, sd = mean[c], std[c]
                fi = np.finfo(np.float32)
                wmax = min(mu + transform.sigma * sd, float(fi.max))
                wmin = max(mu - transform.sigma * sd, float(fi.min))
            flat = bool(wmax == wmin)
            out[c, 2] = wmin
            out[c, 3] = 0.0 if flat else 255.0 / (wmax - wmin)
            out[c, 4] = 1.0 if flat else 0.0
    return out


# ---- the pipeline on device tensors -------------------------------------------------------------------------------------------------
def prepare_on_device(transforms, image, spacing, label=None):
    """A pipeline made only of the four normalisations, Resample and Padding applied to device tensors: image float32 [X,Y,Z,C],
    label int32 [X,Y,Z] or None, spacing the voxel size -> (image, label, spacing), image and label on the device (the caller's tensors
    are not written).  None when the list holds anything else: the caller keeps the host path."""
    if any(type(t) not in ON_DEVICE for t in transforms):
        return None
    from . import ops
    from . import resample as R
    spacing = tuple(float(v) for v in spacing)
    owned = False                                    # `image` is a tensor made here: the next window may be applied in place
    for t in transforms:
        if type(t) in NORMALISATIONS:
            n, C = image.numel() // int(image.shape[-1]), int(image.shape[-1])
            pre, stats = None, None
            if stats_passes(t) == 2:
                pre = pre_map(ops.channel_stats(image).cpu().numpy(), n)
            if stats_passes(t) >= 1:
                stats = ops.channel_stats(image, pre).cpu().numpy()
            image = ops.window_intensity(image, window_params(t, stats, n, pre, channels=C), out=image if owned else None)
            owned = True
        elif type(t) is T.Resample:
            size, ratio = R.output_size(image.shape[:3], spacing, t.voxel_size), R.ratios(spacing, t.voxel_size)
            image = ops.resample(image, size, ratio, "linear")
            if label is not None:
                label = ops.resample(label, size, ratio, "nearest")
            spacing, owned = t.voxel_size, True
        else:
            old = tuple(int(v) for v in image.shape[:3])
            if all(o >= m for o, m in zip(old, t.output_size)):
                continue
            size = tuple(max(o, m) for o, m in zip(old, t.output_size))
            image = ops.crop_window(image, (0, 0, 0), size)
            if label is not None:
                label = ops.crop_window(label, (0, 0, 0), size)
            owned = True
    return image, label, spacing
