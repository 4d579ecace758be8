"""Array restatements of the reference's 3-D sample transforms that are pure index / intensity arithmetic
(pipeline/NiftiDataset3D.py) -- the input side of the hot path without SimpleITK (absent in this image):

    StatisticalNormalization  NiftiDataset3D.py:210-254      ManualNormalization  NiftiDataset3D.py:285-308
    ExtremumNormalization     NiftiDataset3D.py:256-283      Normalization        NiftiDataset3D.py:167-185
    RandomFlip                NiftiDataset3D.py:187-208      Padding              NiftiDataset3D.py:400-456
    RandomCrop                NiftiDataset3D.py:458-551      RandomNoise          NiftiDataset3D.py:553-572
    ConfidenceCrop2           NiftiDataset3D.py:661-793      Resample             NiftiDataset3D.py:345-398
    BSplineDeformation        NiftiDataset3D.py:795-832

A sample is {'image': float32 [X,Y,Z,C] (the reference keeps a list of C SimpleITK images), 'label': int [X,Y,Z]}; every
transform is `t(sample, rng)` with an explicit numpy Generator (the reference draws from the global `random` / `np.random`
state).  `build_pipeline` reads the reference's YAML schema (pipeline/pipeline3D.yaml: preprocess -> train|test|evaluate ->
3D -> [{name, variables}], model.py:340-372) and instantiates by class name exactly like model.py:350.  `Resample` changes the
grid: the sample then carries its voxel spacing under 'spacing' (apply_pipeline / run_pipeline keep it alongside the sample through
the transforms that know nothing of it), and build_pipeline instantiates it only when asked to (geometry=True).
`BSplineDeformation` keeps the grid and resamples on it (vnet_tensorflow_amd/deform.py states the rules); build_pipeline instantiates
it only when asked to (deformation=True).  The other transforms that need SimpleITK's geometry (Reorient, Invert, ConfidenceCrop) are
out of scope: naming one raises."""
import numpy as np

_SITK_ONLY = ("Reorient", "Invert", "BSplineDeformation", "ConfidenceCrop")
_GEOMETRY = ("Resample",)
_DEFORMATION = ("BSplineDeformation",)       # (listed in _SITK_ONLY: refused unless build_pipeline is asked for it)


def _size3(v, what):
    if isinstance(v, int):
        return (v, v, v)
    assert isinstance(v, (tuple, list)) and len(v) == 3, "%s: int or 3 values" % what
    return tuple(int(x) for x in v)


def _window(img, wmin, wmax, omin=0.0, omax=255.0):
    """sitk.IntensityWindowingImageFilter: linear map of [wmin, wmax] onto [omin, omax], values outside clamp."""
    x = np.asarray(img, dtype=np.float64)
    if wmax == wmin:
        return np.where(x < wmin, omin, omax).astype(np.float32)
    y = (x - wmin) * ((omax - omin) / (wmax - wmin)) + omin
    return np.clip(y, omin, omax).astype(np.float32)


class Normalization(object):
    """sitk.RescaleIntensityImageFilter to [0, 255] (per channel)."""
    name = 'Normalization'

    def __call__(self, sample, rng=None):
        img = sample['image']
        out = np.empty(img.shape, dtype=np.float32)
        for c in range(img.shape[-1]):
            ch = img[..., c].astype(np.float64)
            out[..., c] = _window(ch, ch.min(), ch.max())
        return {'image': out, 'label': sample['label']}


class StatisticalNormalization(object):
    """Window [mean - sigma*std, mean + sigma*std] -> [0, 255] per channel; std is ITK's (unbiased, N-1)."""

    def __init__(self, sigma, pre_norm=False):
        self.name = 'StatisticalNormalization'
        assert isinstance(sigma, float)
        self.sigma, self.pre_norm = sigma, pre_norm

    def __call__(self, sample, rng=None):
        img = sample['image']
        out = np.empty(img.shape, dtype=np.float32)
        for c in range(img.shape[-1]):
            ch = img[..., c].astype(np.float64)
            if self.pre_norm:                                   # sitk.NormalizeImageFilter: zero mean, unit variance
                ch = (ch - ch.mean()) / ch.std(ddof=1)
            mu, sd = ch.mean(), ch.std(ddof=1)
            fi = np.finfo(np.float32)
            wmax = min(mu + self.sigma * sd, float(fi.max))
            wmin = max(mu - self.sigma * sd, float(fi.min))
            out[..., c] = _window(ch, wmin, wmax)
        return {'image': out, 'label': sample['label']}


class ExtremumNormalization(object):
    def __init__(self, percent=0.05):
        self.name = 'ExtremumNormalization'
        assert isinstance(percent, float)
        self.percent = percent

    def __call__(self, sample, rng=None):
        img = sample['image']
        out = np.empty(img.shape, dtype=np.float32)
        for c in range(img.shape[-1]):
            ch = img[..., c].astype(np.float64)
            lo, hi = ch.min(), ch.max()
            out[..., c] = _window(ch, (hi - lo) * self.percent + lo, (hi - lo) * (1 - self.percent) + lo)
        return {'image': out, 'label': sample['label']}


class ManualNormalization(object):
    def __init__(self, windowMin, windowMax):
        self.name = 'ManualNormalization'
        assert isinstance(windowMax, (int, float)) and isinstance(windowMin, (int, float))
        self.windowMax, self.windowMin = float(windowMax), float(windowMin)

    def __call__(self, sample, rng=None):
        return {'image': _window(sample['image'], self.windowMin, self.windowMax), 'label': sample['label']}


class RandomFlip(object):
    """One coin flip per sample; heads flips image and label along every axis whose entry in `axes` is true."""

    def __init__(self, axes):
        self.name = 'Flip'
        assert len(axes) > 0 and len(axes) <= 3
        self.axes = axes

    def __call__(self, sample, rng):
        image, label = sample['image'], sample['label']
        if int(rng.integers(2)):
            ax = tuple(i for i, f in enumerate(self.axes) if f)
            image, label = np.flip(image, ax), np.flip(label, ax)
        return {'image': np.ascontiguousarray(image), 'label': np.ascontiguousarray(label)}


class Padding(object):
    """Grow the volume to at least output_size: the reference resamples onto a larger grid with the same origin, spacing
    and direction, i.e. the old voxels keep their indices and the new ones (high side of each axis) are 0."""

    def __init__(self, output_size):
        self.name = 'Padding'
        self.output_size = _size3(output_size, 'output_size')
        assert all(i > 0 for i in self.output_size)

    def __call__(self, sample, rng=None):
        image, label = sample['image'], sample['label']
        old = label.shape
        if all(o >= n for o, n in zip(old, self.output_size)):
            return sample
        pads = [(0, max(n - o, 0)) for o, n in zip(old, self.output_size)]
        return {'image': np.pad(image, pads + [(0, 0)]), 'label': np.pad(label, pads)}


class RandomCrop(object):
    """Random window of output_size; a window with fewer than min_pixel foreground voxels is kept only with probability
    drop_ratio, otherwise another one is drawn (NiftiDataset3D.py:518-541).  np.random.randint(0, n) of the reference
    excludes n, so the last admissible start index (old - new) is never drawn -- kept."""

    def __init__(self, output_size, drop_ratio=0.1, min_pixel=1):
        self.name = 'Random Crop'
        self.output_size = _size3(output_size, 'output_size')
        assert isinstance(drop_ratio, (int, float))
        if not 0 <= drop_ratio <= 1:
            raise RuntimeError('Drop ratio should be between 0 and 1')
        assert isinstance(min_pixel, int)
        if min_pixel < 0:
            raise RuntimeError('Min label pixel count should be integer larger than 0')
        self.drop_ratio, self.min_pixel = drop_ratio, min_pixel

    def __call__(self, sample, rng):
        image, label = sample['image'], sample['label']
        old, new = label.shape, self.output_size
        fg = (label >= 1) & (label <= 255)
        while True:
            start = [0 if o <= n else int(rng.integers(0, o - n)) for o, n in zip(old, new)]
            sl = tuple(slice(s, s + n) for s, n in zip(start, new))
            if int(fg[sl].sum()) >= self.min_pixel or rng.random() <= self.drop_ratio:
                break
        return {'image': np.ascontiguousarray(image[sl]), 'label': np.ascontiguousarray(label[sl])}

    def start_index(self, shape, rng, table, count):
        """The start index of the window __call__ would cut from a label map of `shape`, drawing from `rng` exactly as __call__ does
        (the short-circuited rng.random() included), without the voxels: count(start, size, lo, hi) -> (number of voxels of the window
        with lo <= label <= hi, sum of its labels).  `table` is not asked (ConfidenceCrop2.start_index reads it)."""
        old, new = tuple(shape), self.output_size
        size = tuple(min(o, n) for o, n in zip(old, new))
        while True:
            start = [0 if o <= n else int(rng.integers(0, o - n)) for o, n in zip(old, new)]
            if int(count(start, size, 1, 255)[0]) >= self.min_pixel or rng.random() <= self.drop_ratio:
                return start


class RandomNoise(object):
    """sitk.AdditiveGaussianNoiseImageFilter(mean 0, standard deviation sigma) on every channel."""

    def __init__(self, sigma=5):
        self.name = 'Random Noise'
        self.sigma = sigma

    def __call__(self, sample, rng):
        image = sample['image']
        noise = rng.standard_normal(image.shape, dtype=np.float32) * np.float32(self.sigma)
        return {'image': image + noise, 'label': sample['label']}


class ConfidenceCrop2(object):
    """With probability `probability` (in tenths, as the reference's choice list) crop around the bounding-box centre of a
    randomly chosen connected label component, offset by a uniform integer in [-rand_range, rand_range] per axis; otherwise
    (or when there is no label) a random region -- optionally one without any label (NiftiDataset3D.py:661-793)."""

    def __init__(self, output_size, rand_range=3, probability=0.5, random_empty_region=False):
        self.name = 'Confidence Crop 2'
        self.output_size = _size3(output_size, 'output_size')
        self.rand_range = _size3(rand_range, 'rand_range')
        assert isinstance(probability, float) and 0 <= probability <= 1
        self.probability = probability
        assert isinstance(random_empty_region, bool)
        self.random_empty_region = random_empty_region

    def _crop(self, image, label, index):
        sl = tuple(slice(i, i + n) for i, n in zip(index, self.output_size))
        return np.ascontiguousarray(image[sl]), np.ascontiguousarray(label[sl])

    def _random_index(self, size, rng):
        # random.choice(range(0, size - out - 1)): the last two admissible starts are never drawn (reference as written)
        idx = []
        for s, n in zip(size, self.output_size):
            if s - n == 0:
                idx.append(0)
            else:
                hi = s - n - 1
                if hi <= 0:
                    raise IndexError("Cannot choose from an empty sequence")          # what random.choice(range(0, 0)) raises
                idx.append(int(rng.integers(0, hi)))
        return idx

    def RandomRegion(self, image, label, rng):
        return self._crop(image, label, self._random_index(label.shape, rng))

    def RandomEmptyRegion(self, image, label, rng):
        while True:
            img, lab = self._crop(image, label, self._random_index(label.shape, rng))
            if lab.sum() < 1:
                return img, lab

    def __call__(self, sample, rng):
        from scipy import ndimage
        image, label = sample['image'], sample['label'].astype(np.int16)
        choices = [0] * int(10 * (1 - self.probability)) + [1] * int(10 * self.probability)
        label_type = choices[int(rng.integers(len(choices)))]
        pick_random = self.RandomEmptyRegion if self.random_empty_region else self.RandomRegion
        if label_type == 0:
            image, label = pick_random(image, label, rng)
            return {'image': image, 'label': label}
        cc, n = ndimage.label(label != 0)           # face connectivity = sitk.ConnectedComponentImageFilter default
        if n == 0:
            image, label = pick_random(image, label, rng)
            return {'image': image, 'label': label}
        sel = int(rng.integers(n)) + 1
        box = ndimage.find_objects((cc == sel).astype(np.uint8))[0]
        index = []
        for i in range(3):
            lo, ext = box[i].start, box[i].stop - box[i].start
            ix = lo + int(ext / 2) - int(self.output_size[i] / 2) + int(rng.integers(-self.rand_range[i], self.rand_range[i] + 1))
            if label.shape[i] - ix - 1 < self.output_size[i]:
                ix = label.shape[i] - self.output_size[i] - 1
            if ix < 0:
                ix = 0
            index.append(ix)
        image, label = self._crop(image, label, index)
        return {'image': image, 'label': label}

    def start_index(self, shape, rng, table, count):
        """The start index of the window __call__ would cut from a label map of `shape`, drawing from `rng` exactly as __call__ does
        (the RandomEmptyRegion loop included), without the voxels: table() -> (n, rows) with row k = {representative, count, lo[3],
        hi[3] inclusive} of ndimage.label's component k + 1 (asked only on the branch that labels), count(start, size, lo, hi) ->
        (number of voxels of the window with lo <= label <= hi, sum of its labels)."""
        shape = tuple(shape)
        choices = [0] * int(10 * (1 - self.probability)) + [1] * int(10 * self.probability)
        label_type = choices[int(rng.integers(len(choices)))]

        def pick_random():
            while True:
                index = self._random_index(shape, rng)
                if not self.random_empty_region or count(index, self.output_size, 1, 255)[1] < 1:
                    return index
        if label_type == 0:
            return pick_random()
        n, rows = table()
        if n == 0:
            return pick_random()
        row = rows[int(rng.integers(n))]
        index = []
        for i in range(3):
            lo, ext = int(row[2 + i]), int(row[5 + i]) + 1 - int(row[2 + i])
            ix = lo + int(ext / 2) - int(self.output_size[i] / 2) + int(rng.integers(-self.rand_range[i], self.rand_range[i] + 1))
            if shape[i] - ix - 1 < self.output_size[i]:
                ix = shape[i] - self.output_size[i] - 1
            if ix < 0:
                ix = 0
            index.append(ix)
        return index


class Resample(object):
    """Resample image (linear, every channel) and label (nearest neighbour) to `voxel_size` on a grid with the input's origin and
    direction: n' = int(ceil(s * n / s')) voxels per axis, samples past the input are 0 (vnet_tensorflow_amd/resample.py states the
    rules).  The sample's voxel spacing is sample['spacing'] ((1, 1, 1) when absent); the result carries the new one.
    device: None = NumPy (the only backend a loader thread may use: a launch from another thread can invalidate the training
    loop's stream capture); a torch device = upload, ops.resample, download."""

    def __init__(self, voxel_size, device=None):
        self.name = 'Resample'
        assert isinstance(voxel_size, (float, tuple, list))
        if isinstance(voxel_size, float):
            self.voxel_size = (voxel_size, voxel_size, voxel_size)
        else:
            assert len(voxel_size) == 3
            self.voxel_size = tuple(float(v) for v in voxel_size)
        self.device = device

    def __call__(self, sample, rng=None):
        from . import resample as R
        image, label = sample['image'], sample['label']
        spacing = tuple(float(v) for v in sample.get('spacing', (1.0, 1.0, 1.0)))
        size, ratio = R.output_size(label.shape, spacing, self.voxel_size), R.ratios(spacing, self.voxel_size)
        if self.device is None:
            image, label = R.linear(image, size, ratio), R.nearest(label, size, ratio)
        else:
            import torch
            from . import ops
            img = ops.resample(torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(self.device), size, ratio, "linear")
            lab = ops.resample(torch.from_numpy(np.ascontiguousarray(label, dtype=np.int32)).to(self.device), size, ratio, "nearest")
            image, label = img.cpu().numpy(), lab.cpu().numpy().astype(label.dtype, copy=False)
        return {'image': image, 'label': label, 'spacing': self.voxel_size}


class BSplineDeformation(object):
    """Free-form deformation: image and label are resampled on their own grid through a cubic B-spline displacement field whose
    3 * 13^3 control values are `rng.random(6591) * randomness` (the reference draws np.random.random); linear interpolation for the
    image AND the label (the reference passes no interpolator), the label truncated to its integer type, samples from outside are 0
    (vnet_tensorflow_amd/deform.py states the rules).  The grid is kept: the sample's 'spacing' ((1, 1, 1) when absent) is read and
    passed through.
    device: None = NumPy; a torch device = pinned staging, upload, ops.bspline_deform, download, all inside ops.side_work(device) --
    which is what makes this transform safe on a loader thread (loader_safe) while the training loop captures or replays its graph."""
    loader_safe = True

    def __init__(self, randomness=10, device=None):
        self.name = 'BSpline Deformation'
        if not isinstance(randomness, (int, float)) or not randomness > 0:
            raise RuntimeError('Randomness should be non zero values')
        self.randomness = randomness
        self.device = device

    def __call__(self, sample, rng):
        from . import deform as D
        image, label = sample['image'], sample['label']
        spacing = tuple(float(v) for v in sample.get('spacing', (1.0, 1.0, 1.0)))
        coef = rng.random(D.PARAMS) * self.randomness
        if self.device is None:
            image, label = D.linear(image, coef, spacing), D.label(label, coef, spacing)
        else:
            image, label = self._on_device(image, label, coef, spacing)
        return {'image': image, 'label': label, 'spacing': spacing}

    def _on_device(self, image, label, coef, spacing):
        import torch
        from . import ops
        if not np.issubdtype(label.dtype, np.integer) or label.dtype.itemsize > 4 or label.dtype == np.uint32:
            raise ValueError("BSplineDeformation(device=...): the label map goes through int32, got %s" % (label.dtype,))
        with ops.side_work(self.device) as stream:
            hi = ops.pinned_staging("deform.image", image.shape, torch.float32)
            hl = ops.pinned_staging("deform.label", label.shape, torch.int32)
            hc = ops.pinned_staging("deform.coef", coef.shape, torch.float64)
            np.copyto(hi.numpy(), image, casting="unsafe")
            np.copyto(hl.numpy(), label, casting="unsafe")
            np.copyto(hc.numpy(), coef)
            di, dl, dc = (h.to(self.device, non_blocking=True) for h in (hi, hl, hc))
            yi, yl = ops.bspline_deform(di, dc, spacing, "image"), ops.bspline_deform(dl, dc, spacing, "label")
            hi.copy_(yi, non_blocking=True)
            hl.copy_(yl, non_blocking=True)
            stream.synchronize()
            # (the staging buffers are this thread's and are reused by its next call: hand out copies)
            return hi.numpy().copy(), hl.numpy().astype(label.dtype)


_REGISTRY = {c.__name__: c for c in (Normalization, StatisticalNormalization, ExtremumNormalization, ManualNormalization,
                                     RandomFlip, Padding, RandomCrop, RandomNoise, ConfidenceCrop2, Resample,
                                     BSplineDeformation)}
# transforms that draw from `rng`: everything in front of the first one is a pure function of the case (deterministic_prefix)
_RANDOM = (RandomFlip, RandomCrop, RandomNoise, ConfidenceCrop2, BSplineDeformation)


def build_pipeline(yaml_path, phase, geometry=False, deformation=False, device=None):
    """[transform] of preprocess -> `phase` ('train' | 'test' | 'evaluate') -> 3D of a reference pipeline YAML.
    geometry: instantiate `Resample` (the caller then passes each volume's voxel spacing to apply_pipeline / run_pipeline);
    False keeps refusing it by name, like the transforms that stay out of scope.
    deformation: instantiate `BSplineDeformation` (False keeps refusing it by name), on `device` (None = NumPy)."""
    import yaml
    with open(yaml_path) as f:
        spec = yaml.load(f, Loader=yaml.SafeLoader)
    entries = (spec.get("preprocess", {}).get(phase, {}) or {}).get("3D") or []
    out = []
    for t in entries:
        name = t["name"]
        if (name in _SITK_ONLY and not (deformation and name in _DEFORMATION)) or (name in _GEOMETRY and not geometry):
            raise NotImplementedError("transform %r resamples on the physical grid and needs SimpleITK (out of scope here); "
                                      "resample the volumes offline and drop it from the pipeline" % name)
        if name not in _REGISTRY:
            raise AttributeError("module 'NiftiDataset3D' has no attribute %r" % name)
        kw = dict(t.get("variables") or {})
        if name in _DEFORMATION and device is not None:
            kw["device"] = device
        out.append(_REGISTRY[name](**kw))
    return out


def deterministic_prefix(transforms):
    """Number of leading transforms that never draw from `rng`: their result is the same for every visit of a case."""
    n = 0
    while n < len(transforms) and not isinstance(transforms[n], _RANDOM):
        n += 1
    return n


class TailPlan(object):
    """What plan_tail recognised: the crop (ConfidenceCrop2 | RandomCrop), then RandomFlip or None, then RandomNoise or None."""

    def __init__(self, crop, flip, noise):
        self.crop, self.flip, self.noise = crop, flip, noise

    def draw(self, shape, rng, table, count):
        """(start index, flip mask, sigma, noise seed) of one sample, drawn from `rng` in the order the transforms would: the crop's
        draws (start_index), RandomFlip's coin, and for RandomNoise ONE 64-bit seed (the NumPy transform draws the deviates
        themselves, so the noise of the two paths differs; everything in front of it does not)."""
        start = self.crop.start_index(shape, rng, table, count)
        mask = 0
        if self.flip is not None and int(rng.integers(2)):
            mask = sum(1 << i for i, f in enumerate(self.flip.axes) if f)
        sigma, seed = 0.0, 0
        if self.noise is not None:
            sigma, seed = float(self.noise.sigma), int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        return start, mask, sigma, seed


def plan_tail(transforms):
    """TailPlan of a random tail that a device-resident case can serve -- one of ConfidenceCrop2 | RandomCrop, then optionally
    RandomFlip, then optionally RandomNoise, in that order and nothing else -- or None (any other tail, a BSplineDeformation in front
    of the crop included: the dataset then keeps the loader path)."""
    tf = list(transforms)
    if not tf or type(tf[0]) not in (ConfidenceCrop2, RandomCrop):
        return None
    crop, rest = tf[0], tf[1:]
    flip = rest.pop(0) if rest and type(rest[0]) is RandomFlip else None
    noise = rest.pop(0) if rest and type(rest[0]) is RandomNoise else None
    if rest:
        return None
    return TailPlan(crop, flip, noise)


class DeformedTailPlan(TailPlan):
    """What plan_deformed_tail recognised: a BSplineDeformation, then the tail of a TailPlan."""

    def __init__(self, deform, crop, flip, noise):
        TailPlan.__init__(self, crop, flip, noise)
        self.deform = deform

    def draw(self, shape, rng, deformed):
        """(coefficients, start index, flip mask, sigma, noise seed) of one sample, drawn from `rng` in the order the transforms would:
        BSplineDeformation's rng.random(6591) * randomness, then TailPlan.draw -- the crop's draws, the flip's coin, the one noise seed.
        The crop decides on the DEFORMED label, which exists only once the coefficients do: deformed(coef) -> (table, count), the two
        callables of TailPlan.draw, answering for the label map deformed by `coef`."""
        from .deform import PARAMS
        coef = rng.random(PARAMS) * self.deform.randomness
        table, count = deformed(coef)
        return (coef,) + TailPlan.draw(self, shape, rng, table, count)


def plan_deformed_tail(transforms):
    """DeformedTailPlan of a random tail that a device-resident case can serve THROUGH the deformation -- one BSplineDeformation, then a
    tail plan_tail recognises (ConfidenceCrop2 | RandomCrop, then optionally RandomFlip, then optionally RandomNoise) and nothing else --
    or None.  (plan_tail keeps answering None for such a list: the dataset asks it first, then this planner.)"""
    tf = list(transforms)
    if not tf or type(tf[0]) is not BSplineDeformation:
        return None
    rest = plan_tail(tf[1:])
    if rest is None:
        return None
    return DeformedTailPlan(tf[0], rest.crop, rest.flip, rest.noise)


def run_pipeline(transforms, sample, rng):
    """The sample after every transform, its voxel spacing under 'spacing' ((1, 1, 1) when the sample came without): the spacing is
    carried past the transforms that return image and label alone (they keep the grid's spacing: crops and Padding keep origin-side
    voxels and their size)."""
    spacing = tuple(sample.get('spacing', (1.0, 1.0, 1.0)))
    sample = dict(sample, spacing=spacing)
    for t in transforms:
        out = t(sample, rng)
        spacing = tuple(out.get('spacing', spacing))
        sample = dict(out, spacing=spacing)
    return sample


def apply_pipeline(transforms, image, label, rng, spacing=(1, 1, 1)):
    sample = run_pipeline(transforms, {'image': image, 'label': label, 'spacing': spacing}, rng)
    return sample['image'], sample['label']
