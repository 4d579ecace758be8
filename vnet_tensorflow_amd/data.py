"""Input side of the hot path: the data contract of the reference's NiftiDataset3D
(pipeline/NiftiDataset3D.py:125-165) without SimpleITK (absent here): image float32
[X,Y,Z,Cin] (axis order after the (2,1,0) transpose, NiftiDataset3D.py:154), label int32
[X,Y,Z] remapped to class *indices* of SegmentationClasses (NiftiDataset3D.py:125-137).

Sources: a case directory tree holding `.npy` or single-file NIfTI-1 `.nii` / `.nii.gz` files, or the
synthetic generator of SURVEY.md 8(d) (the shipped sample volumes are Git-LFS stubs).  Without a
transform list the pure index-math RandomCrop to PatchShape is applied; with one (transforms.py),
the case's voxel spacing travels with the sample, which is what `Resample` reads."""
import os
import struct

import numpy as np


# ---- minimal NIfTI-1 (single-file; written uncompressed, read also gzip-compressed) ------------------------------------------------
_NIFTI_DTYPES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8,
                 512: np.uint16, 768: np.uint32}


def _open_nifti(path):
    """The file object of a single-file NIfTI-1: gzip-compressed for `.nii.gz` (standard library), plain otherwise."""
    if path.endswith(".gz"):
        import gzip
        return gzip.open(path, "rb")
    return open(path, "rb")


def _nifti_header(f, path):
    """The 348 header bytes of an open file.  A compressed file is decompressed only as far as they reach."""
    try:
        hdr = f.read(348)
    except (EOFError, OSError) as e:                 # a truncated or damaged gzip stream (gzip.BadGzipFile is an OSError)
        raise ValueError("%s: not a readable NIfTI-1 file (%s)" % (path, e))
    if len(hdr) < 348 or struct.unpack("<i", hdr[:4])[0] != 348:
        raise ValueError("%s: not a little-endian NIfTI-1 file (Git-LFS pointer?)" % path)
    return hdr


def read_nifti(path):
    """Returns (array [X,Y,Z], header dict).  NIfTI stores x fastest, i.e. Fortran order [X,Y,Z].  `.nii` or gzip-compressed
    `.nii.gz`."""
    with _open_nifti(path) as f:
        hdr = _nifti_header(f, path)
        dim = struct.unpack("<8h", hdr[40:56])
        datatype, bitpix = struct.unpack("<hh", hdr[70:74])
        pixdim = struct.unpack("<8f", hdr[76:108])
        vox_offset = struct.unpack("<f", hdr[108:112])[0]
        slope, inter = struct.unpack("<ff", hdr[112:120])
        shape = tuple(int(d) for d in dim[1:1 + dim[0]])
        dt = _NIFTI_DTYPES[datatype]
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        try:
            f.seek(int(vox_offset))
            raw = f.read(nbytes)
        except (EOFError, OSError) as e:
            raise ValueError("%s: the voxel array cannot be read (%s)" % (path, e))
        if len(raw) < nbytes:
            raise ValueError("%s: truncated, %d of %d bytes of the voxel array" % (path, len(raw), nbytes))
        data = np.frombuffer(raw, dtype=dt).reshape(shape, order="F")
    if slope not in (0.0, 1.0) or inter != 0.0:
        data = data.astype(np.float32) * (slope if slope != 0 else 1.0) + inter
    return data, {"pixdim": pixdim[1:4], "dim": shape, "datatype": datatype}


def write_nifti(path, arr, pixdim=(1.0, 1.0, 1.0)):
    arr = np.asarray(arr)
    code = {v: k for k, v in _NIFTI_DTYPES.items()}[arr.dtype.type]
    hdr = bytearray(348)
    struct.pack_into("<i", hdr, 0, 348)
    dim = [arr.ndim] + list(arr.shape) + [1] * (7 - arr.ndim)
    struct.pack_into("<8h", hdr, 40, *dim)
    struct.pack_into("<hh", hdr, 70, code, arr.dtype.itemsize * 8)
    struct.pack_into("<8f", hdr, 76, 1.0, *pixdim, 1.0, 1.0, 1.0, 1.0)
    struct.pack_into("<f", hdr, 108, 352.0)
    struct.pack_into("<ff", hdr, 112, 1.0, 0.0)
    hdr[344:348] = b"n+1\0"
    with open(path, "wb") as f:
        f.write(bytes(hdr) + b"\0\0\0\0")
        f.write(np.asfortranarray(arr).tobytes(order="F"))


def volume_spacing(path):
    """Voxel spacing (pixdim) of a volume file -- from the 348-byte NIfTI-1 header alone, the voxel array is not read (of a `.nii.gz`
    only the header's bytes are decompressed); (1, 1, 1) for .npy arrays, which carry none."""
    if path.endswith((".nii", ".nii.gz")):
        with _open_nifti(path) as f:
            hdr = _nifti_header(f, path)
        return tuple(float(v) for v in struct.unpack("<8f", hdr[76:108])[1:4])
    return (1.0, 1.0, 1.0)


def load_volume(path):
    if path.endswith(".npy"):
        return np.load(path)
    if path.endswith((".nii", ".nii.gz")):
        return read_nifti(path)[0]
    raise ValueError("unsupported volume format: %s (.npy, .nii or .nii.gz single-file NIfTI-1; SimpleITK is not available)" % path)


def remap_labels(label, classes):
    """NiftiDataset3D.py:125-137: label values -> index into SegmentationClasses (others -> 0)."""
    out = np.zeros(label.shape, dtype=np.int32)
    for idx, c in enumerate(classes):
        out[label == c] = idx
    return out


def synthetic_case(shape, cin, K, seed):
    """One synthetic volume per SURVEY.md 8(d): clamp(127.5 + 40 N(0,1), 0, 255) + 60 inside the
    label spheres; background 0 plus one sphere of radius P/6 per foreground class."""
    rng = np.random.default_rng(seed)
    shape = tuple(shape)
    img = 127.5 + 40.0 * rng.standard_normal(shape + (cin,), dtype=np.float32)
    lab = np.zeros(shape, dtype=np.int32)
    P = min(shape)
    grids = np.ogrid[tuple(slice(0, s) for s in shape)]
    for c in range(1, K):
        ctr = [rng.uniform(s / 4.0, 3.0 * s / 4.0) for s in shape]
        d2 = sum((g - c0) ** 2 for g, c0 in zip(grids, ctr))
        lab[d2 <= (P / 6.0) ** 2] = c
    img += 60.0 * (lab > 0)[..., None]
    return np.clip(img, 0.0, 255.0).astype(np.float32), lab


def random_crop(image, label, patch, rng):
    """Index-math RandomCrop (NiftiDataset3D.py:458-548 without the SimpleITK resampling): pad with
    zeros up to the patch size, then take a uniformly random window."""
    pads = [(0, max(p - s, 0)) for s, p in zip(label.shape, patch)]
    if any(hi for _, hi in pads):
        image = np.pad(image, pads + [(0, 0)])
        label = np.pad(label, pads)
    start = [int(rng.integers(0, s - p + 1)) for s, p in zip(label.shape, patch)]
    sl = tuple(slice(a, a + p) for a, p in zip(start, patch))
    return image[sl], label[sl]


class VolumeDataset(object):
    """Iterates batches (image float32 [B,*P,Cin], label int32 [B,*P,1]) like the reference's
    tf.data pipeline: shuffle, batch(drop_remainder=True) (model.py:289-295).

    Data parallel: every rank shuffles with the SAME generator (seed + epoch), the order is truncated to
    a multiple of world * batch and strided by rank, so the shards are disjoint and every rank yields the same number
    of batches (the gradient all-reduces of the ranks pair up one to one; a rank with fewer steps would leave the
    others blocked in RCCL).  Crop windows are drawn from a per-rank generator.  train=False (the test pass, which holds no
    collective) is not sharded: every rank iterates all cases.

    The epoch rule: the plan of epoch e -- order and crop seeds, from which every window, flip, noise draw and deformation of the
    epoch follows -- is a function of (seed, rank, world, e) alone.  A run restored at epoch e passes epoch=e (or calls
    skip_epochs) and trains on what the uninterrupted run would have seen, not on epoch 0's samples again."""

    def __init__(self, data_dir, image_filenames, label_filename, classes, patch_shape, batch_size,
                 train=True, seed=0, synthetic=None, rank=0, world=1, cache=None, transforms=None,
                 device_tail=None, device_cache_bytes=16 << 30, max_components=4096, epoch=0):
        self.image_filenames, self.label_filename = list(image_filenames), label_filename
        self.classes, self.patch, self.batch = list(classes), tuple(patch_shape), int(batch_size)
        self.train, self.seed, self.epoch = train, int(seed), 0
        self.rng = np.random.default_rng(seed + 7919 * rank)          # crop windows of this rank
        self.rank, self.world = rank, world
        self.synthetic = synthetic
        # the reference's per-sample transform list (vnet_tensorflow_amd.transforms.build_pipeline of TrainingSetting.Pipeline);
        # None = zero-pad + uniform RandomCrop to PatchShape
        self.transforms = transforms
        if any(getattr(t, "device", None) is not None and not getattr(t, "loader_safe", False) for t in (transforms or ())):
            # batches are made on loader threads while the main thread may be capturing or replaying the step's hipGraph: a launch
            # from another thread can invalidate the capture.  The exception is a transform that declares loader_safe: its device
            # work runs inside ops.side_work (a lock the capture holds, a stream of the thread's own, synchronised before release)
            raise ValueError("VolumeDataset runs its transforms on loader threads: they take the NumPy backend (device=None)")
        # volumes kept in host memory after the first load (synthetic cases are a pure function of their seed;
        # regenerating a 128^3 case costs ~0.3 s, 10x a training step)
        self.cache = {} if (cache if cache is not None else synthetic is not None) else None
        if synthetic is not None:
            self.cases = list(range(int(synthetic.get("Cases", 8))))
        else:
            if not os.path.isdir(data_dir):
                raise FileNotFoundError("data directory %s does not exist" % data_dir)
            self.cases = sorted(os.path.join(data_dir, d) for d in os.listdir(data_dir)
                                if os.path.isdir(os.path.join(data_dir, d)))
        # device_tail (a torch device; TrainingSetting.SampleOnDevice): prepared cases -- the case after the pipeline's deterministic
        # prefix -- live in device memory under an LRU byte budget, the random tail's index decisions stay on the host and one kernel
        # writes each sample into a device batch (vnet_tensorflow_amd/sample.py).  Only the tails
        # transforms.plan_tail recognises, and those with one BSplineDeformation in front (transforms.plan_deformed_tail: the label is
        # deformed and its components tabled per visit, the image is deformed by the kernel that writes the sample, for the window's
        # voxels alone); any other keeps the loader path below
        self.device_tail, self._tail, self._deformed = None, None, False
        if device_tail is not None:
            from .transforms import deterministic_prefix, plan_deformed_tail, plan_tail
            self._tail_at = deterministic_prefix(transforms) if transforms is not None else 0
            self._tail = plan_tail(transforms[self._tail_at:]) if transforms is not None else None
            if self._tail is None and transforms is not None:
                self._tail = plan_deformed_tail(transforms[self._tail_at:])
                self._deformed = self._tail is not None
            if self._tail is None:
                print("VolumeDataset: the pipeline's random tail is not one the device serves ([BSplineDeformation,] ConfidenceCrop2 | "
                      "RandomCrop, then RandomFlip, then RandomNoise); samples keep the loader path")
            elif tuple(self._tail.crop.output_size) != self.patch:
                raise ValueError("the pipeline's crop produces %s samples, PatchShape is %s" % (tuple(self._tail.crop.output_size), self.patch))
            else:
                import collections
                import torch
                self.device_tail = torch.device(device_tail)
                self.device_cache_bytes, self.max_components = int(device_cache_bytes), int(max_components)
                # case -> (image, label, (n, rows) | None, spacing) on the device, least recently used first.  No lock of its own: it is
                # touched only inside ops.side_work, whose lock is exclusive (one loader thread at a time, and never during a capture)
                self._dev_cache, self._dev_bytes, self._dev_host_only = collections.OrderedDict(), 0, set()
                # (its bookkeeping -- look-up, evictions, insertion -- is atomic all the same: under a side_work that excludes nobody, the
                # CPU stand-ins of the tests, two loader threads must not both evict and then both insert)
                import threading
                self._dev_lock = threading.Lock()
                self.device_stats = {"uploads": 0, "evictions": 0, "host_samples": 0}
        if self.train and self.steps_per_epoch() == 0:
            raise ValueError("%d cases give no full batch for %d rank(s) x batch %d: every rank needs at least one batch per "
                             "epoch (a rank without work would sit in no collective at all)" % (len(self.cases), world, self.batch))
        # epoch = e (a run restored at epoch e, model.image2label._train): the next plan is the e-th plan of a dataset that started at 0
        self.skip_epochs(epoch)

    def skip_epochs(self, n):
        """Stand where a dataset stands after n more epochs, without making a batch: the shuffle of an epoch is a function of
        (seed, epoch), its crop seeds are the next steps_per_epoch() x batch draws of this rank's generator -- the very draws
        epoch_plan() makes, consumed here in the same calls, so the plans that follow are those of the uninterrupted sequence."""
        for _ in range(int(n)):
            for _ in range(self.steps_per_epoch()):
                self.rng.integers(0, 2 ** 62, size=self.batch)
            self.epoch += 1

    def steps_per_epoch(self):
        # the TEST pass holds no collective (model.image2label.train: forward + metrics per rank), so it is not sharded: every
        # rank walks every test case, drop_remainder like the reference (model.py:293) -- a test set smaller than
        # world x batch must neither abort the job nor lose cases
        if not self.train:
            return len(self.cases) // self.batch
        return len(self.cases) // (self.world * self.batch)

    def _load(self, case, keep=True):
        if self.cache is not None and case in self.cache:
            return self.cache[case]
        if self.synthetic is not None:
            shape = self.synthetic.get("Shape", self.patch)
            out = synthetic_case(shape, len(self.image_filenames), len(self.classes),
                                 int(self.synthetic.get("Seed", 1000)) + case)
        else:
            chans = [np.asarray(load_volume(os.path.join(case, f)), dtype=np.float32) for f in self.image_filenames]
            out = np.stack(chans, axis=-1), remap_labels(load_volume(os.path.join(case, self.label_filename)), self.classes)
        if self.cache is not None and keep:
            self.cache[case] = out
        return out

    def _spacing(self, case):
        if self.synthetic is not None:
            return tuple(float(v) for v in self.synthetic.get("Spacing", (1.0, 1.0, 1.0)))
        return volume_spacing(os.path.join(case, self.image_filenames[0]))

    def _prepared(self, case):
        """(sample, n): the case after the first n transforms.  With the cache on, n is the pipeline's deterministic prefix -- every
        transform before the first one that draws from the generator (normalisation, Resample, Padding) -- and the result is what
        is cached, so the resampling of a case is paid once, not once per visit; without a cache n = 0."""
        from .transforms import deterministic_prefix, run_pipeline
        key = ("prepared", case)
        if self.cache is not None and key in self.cache:
            return self.cache[key]
        image, label = self._load(case, keep=False)
        sample = {'image': image, 'label': label, 'spacing': self._spacing(case)}
        n = deterministic_prefix(self.transforms) if self.cache is not None else 0
        out = run_pipeline(self.transforms[:n], sample, None), n
        if self.cache is not None:
            self.cache[key] = out
        return out

    def epoch_plan(self):
        """[(cases of the batch, crop seeds)] of this rank for the next epoch; advances the epoch counter."""
        order = list(self.cases)
        if self.train:
            np.random.default_rng(self.seed + 104729 * self.epoch).shuffle(order)     # identical on every rank
        self.epoch += 1
        if self.train:
            per = self.world * self.batch
            order = order[:len(order) // per * per][self.rank::self.world]
        else:
            order = order[:len(order) // self.batch * self.batch]
        plan = []
        for i in range(0, len(order), self.batch):
            plan.append((order[i:i + self.batch], [int(v) for v in self.rng.integers(0, 2 ** 62, size=self.batch)]))
        return plan

    def batch_shapes(self):
        """(image shape, label shape) of one batch: [B, *patch, Cin] float32 and [B, *patch, 1] int32."""
        return (self.batch,) + tuple(self.patch) + (len(self.image_filenames),), (self.batch,) + tuple(self.patch) + (1,)

    def _prepared_split(self, case):
        """The case after the deterministic prefix, whether or not the host cache is on (the device cache is what keeps it)."""
        from .transforms import run_pipeline
        if self.cache is not None:
            return self._prepared(case)[0]           # (kept on the host as well: a re-upload after an eviction prepares nothing again)
        image, label = self._load(case, keep=False)
        return run_pipeline(self.transforms[:self._tail_at], {'image': image, 'label': label, 'spacing': self._spacing(case)}, None)

    def _device_case(self, case):
        """(image float32 [X,Y,Z,C], label int32 [X,Y,Z], component table | None, spacing) on the device, or None when the case takes the
        NumPy path: larger than the budget, or more components than max_components.  Called inside ops.side_work.  The table belongs to
        the prepared case -- a pure function of the file and the deterministic prefix -- so it is computed once, at the upload, and
        leaves the cache with the case.  Behind a deformation there is no such table: the components are those of the deformed label,
        which differ from visit to visit (_deformed_sample)."""
        with self._dev_lock:
            return self._device_case_locked(case)

    def _device_case_locked(self, case):
        import torch
        from . import ops
        from .transforms import ConfidenceCrop2
        if case in self._dev_host_only:
            return None
        entry = self._dev_cache.get(case)
        if entry is not None:
            self._dev_cache.move_to_end(case)
            return entry
        sample = self._prepared_split(case)
        image = np.ascontiguousarray(sample['image'], dtype=np.float32)
        label = np.ascontiguousarray(sample['label'], dtype=np.int32)
        nbytes = image.nbytes + label.nbytes
        if nbytes > self.device_cache_bytes:
            self._dev_host_only.add(case)
            return None
        while self._dev_cache and self._dev_bytes + nbytes > self.device_cache_bytes:
            _, old = self._dev_cache.popitem(last=False)
            self._dev_bytes -= old[0].numel() * 4 + old[1].numel() * 4
            self.device_stats["evictions"] += 1
        di, dl = torch.from_numpy(image).to(self.device_tail), torch.from_numpy(label).to(self.device_tail)
        table = None
        if isinstance(self._tail.crop, ConfidenceCrop2) and not self._deformed:
            need = ops._lib.lib().vnet_cc_table_ws_bytes(*label.shape)
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device_tail)     # (this thread's, on its side stream)
            table = ops.component_table(dl, self.max_components, ws=ws)
            if table[0] > self.max_components:
                self._dev_host_only.add(case)
                return None
        entry = (di, dl, table, tuple(float(v) for v in sample.get('spacing', (1.0, 1.0, 1.0))))
        self._dev_cache[case] = entry
        self._dev_bytes += nbytes
        self.device_stats["uploads"] += 1
        return entry

    class _TooManyComponents(Exception):
        pass

    def _deformed_sample(self, entry, rng, out_image, out_label):
        """One sample through the deformation, inside ops.side_work: the coefficients go up (52 KB, pinned staging), the LABEL is deformed
        whole -- the crop decides on it -- into a volume of this thread, its components are tabled for ConfidenceCrop2, the draws are
        made, and one kernel deforms the window's voxels of the resident image into the slot.  Transient per loader thread: the deformed
        label (4 B/voxel) and the table's scratch (8 B/voxel).  Raises _TooManyComponents (after the coefficients were drawn) when the
        deformed label holds more than max_components components."""
        import torch
        from . import ops
        from .transforms import ConfidenceCrop2
        di, dl, _, spacing = entry
        shape = tuple(dl.shape)
        state = {}

        def deformed(coef):
            # (the staging buffer is this thread's and is written again by its next sample: every sample ends in a read-back -- the
            # table's or a window count's -- or in the synchronise of side_work, behind this copy on the same stream)
            hc = ops.pinned_staging("deform_sample.coef", coef.shape, torch.float64)
            np.copyto(hc.numpy(), coef)
            dc = state["coef"] = hc.to(self.device_tail, non_blocking=True)
            yl = state["label"] = ops.bspline_deform(dl, dc, spacing, "label")
            table = None
            if isinstance(self._tail.crop, ConfidenceCrop2):
                need = ops._lib.lib().vnet_cc_table_ws_bytes(*shape)
                ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device_tail)
                table = ops.component_table(yl, max(self.max_components, 1), ws=ws)
                if table[0] > self.max_components:
                    raise VolumeDataset._TooManyComponents()
            return (lambda: table), (lambda s, n, lo, hi: ops.window_count(yl, s, n, lo, hi))
        _, start, mask, sigma, seed = self._tail.draw(shape, rng, deformed)
        ops.deform_sample_patch(di, state["label"], state["coef"], spacing, start, self.patch, mask, sigma, seed, out_image, out_label)

    def _host_sample(self, case, rng, out_image, out_label):
        """The NumPy tail of one sample, copied into its slot of the device batch."""
        import torch
        from .transforms import run_pipeline
        self.device_stats["host_samples"] += 1
        sample = run_pipeline(self.transforms[self._tail_at:], self._prepared_split(case), rng)
        if tuple(sample['label'].shape) != self.patch:
            raise ValueError("the transform pipeline produced a %s sample, PatchShape is %s" % (tuple(sample['label'].shape), self.patch))
        out_image.copy_(torch.from_numpy(np.ascontiguousarray(sample['image'], dtype=np.float32)))
        out_label[..., 0].copy_(torch.from_numpy(np.ascontiguousarray(sample['label'], dtype=np.int32)))

    def _make_batch_device(self, cases, seeds):
        """Device tensors (image float32 [B,*P,Cin], label int32 [B,*P,1]); wholly inside ops.side_work: the loader thread's
        uploads, launches and read-backs run on its own stream and never while the step graph is being captured."""
        import torch
        from . import ops
        si, sl = (len(cases),) + self.batch_shapes()[0][1:], (len(cases),) + self.batch_shapes()[1][1:]
        with ops.side_work(self.device_tail):
            img = torch.empty(si, dtype=torch.float32, device=self.device_tail)
            lab = torch.empty(sl, dtype=torch.int32, device=self.device_tail)
            for i, (case, sd) in enumerate(zip(cases, seeds)):
                rng = np.random.default_rng(sd)
                entry = self._device_case(case)
                if entry is None:
                    self._host_sample(case, rng, img[i], lab[i])
                    continue
                di, dl, table, _ = entry
                shape = tuple(dl.shape)
                if any(s < p for s, p in zip(shape, self.patch)):
                    raise ValueError("the prepared case is %s, smaller than PatchShape %s (put a Padding in front of the crop, like "
                                     "the reference's pipeline3D.yaml)" % (shape, self.patch))
                if self._deformed:
                    try:
                        self._deformed_sample(entry, rng, img[i], lab[i])
                    except VolumeDataset._TooManyComponents:
                        # the coefficients were drawn from `rng` already: the NumPy tail starts over on a generator of its own
                        self._host_sample(case, np.random.default_rng(sd), img[i], lab[i])
                    continue
                start, mask, sigma, seed = self._tail.draw(shape, rng, lambda: table,
                                                           lambda s, n, lo, hi: ops.window_count(dl, s, n, lo, hi))
                ops.sample_patch(di, dl, start, self.patch, mask, sigma, seed, img[i], lab[i])
        return img, lab

    def make_batch(self, cases, seeds, out=None):
        """out = (image float32 [B,*P,Cin], label int32 [B,*P,1]) NumPy arrays to fill (e.g. views of pinned host tensors: the
        crop is then the ONLY copy between the cached volume and the DMA source); None: new arrays.
        With device_tail the batch is made on the device and returned as device tensors (`out` is not used)."""
        if self.device_tail is not None:
            return self._make_batch_device(cases, seeds)
        imgs, labs = [], []
        for i, (case, sd) in enumerate(zip(cases, seeds)):
            if self.transforms is not None:
                from .transforms import run_pipeline
                sample, n = self._prepared(case)
                sample = run_pipeline(self.transforms[n:], sample, np.random.default_rng(sd))
                image, label = sample['image'], sample['label']
                if tuple(label.shape) != self.patch:
                    raise ValueError("the transform pipeline produced a %s sample, PatchShape is %s (end it with a crop to "
                                     "PatchShape, like the reference's pipeline3D.yaml)" % (tuple(label.shape), self.patch))
            else:
                image, label = self._load(case)
                image, label = random_crop(image, label, self.patch, np.random.default_rng(sd))
            if out is not None:
                np.copyto(out[0][i], image, casting="unsafe")
                np.copyto(out[1][i, ..., 0], label, casting="unsafe")
                continue
            imgs.append(image)
            labs.append(label[..., None])
        if out is not None:
            return out
        return np.stack(imgs).astype(np.float32, copy=False), np.stack(labs).astype(np.int32, copy=False)

    def __iter__(self):
        for cases, seeds in self.epoch_plan():
            yield self.make_batch(cases, seeds)


class Prefetcher(object):
    """Runs `dataset.make_batch` on worker threads (NumPy releases the GIL in the copies that dominate it), `depth`
    batches ahead of the consumer and in order, and hands them over as PINNED host tensors, so that the training loop's
    host-to-device copy is asynchronous (`non_blocking=True`) and overlaps the previous step's kernels.
    The counterpart of the reference's tf.data `prefetch` (model.py:289-295)."""

    def __init__(self, dataset, depth=4, workers=3, pin=True):
        self.dataset, self.depth, self.workers, self.pin = dataset, int(depth), int(workers), pin

    def _job(self, cases, seeds):
        import torch
        if getattr(self.dataset, "device_tail", None) is not None:
            # the batch is made in device memory (VolumeDataset._make_batch_device): nothing to pin, no pinned allocation
            return self.dataset.make_batch(cases, seeds)
        if self.pin and torch.cuda.is_available() and len(cases) == self.dataset.batch and hasattr(self.dataset, "batch_shapes"):
            # crop straight into pinned memory (torch's caching host allocator hands a block out again only after the
            # asynchronous copies that read it have finished): one host copy per batch instead of three
            si, sl = self.dataset.batch_shapes()
            ti = torch.empty(si, dtype=torch.float32, pin_memory=True)
            tl = torch.empty(sl, dtype=torch.int32, pin_memory=True)
            self.dataset.make_batch(cases, seeds, out=(ti.numpy(), tl.numpy()))
            return ti, tl
        img, lab = self.dataset.make_batch(cases, seeds)
        ti, tl = torch.from_numpy(img), torch.from_numpy(lab)
        if self.pin and torch.cuda.is_available():
            ti, tl = ti.pin_memory(), tl.pin_memory()
        return ti, tl

    def __iter__(self):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        plan = self.dataset.epoch_plan()
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            pending, it = deque(), iter(plan)
            for cases, seeds in it:
                pending.append(pool.submit(self._job, cases, seeds))
                if len(pending) >= self.depth:
                    break
            while pending:
                out = pending.popleft().result()
                nxt = next(it, None)
                if nxt is not None:
                    pending.append(pool.submit(self._job, *nxt))
                yield out
