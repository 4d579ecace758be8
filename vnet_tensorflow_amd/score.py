"""Scoring a label map against its ground truth (reference utils/batch_evaluate: `Accuracy` of batch_evaluate.py and
batch_evaluate_stride.py) -- the rules, the NumPy restatements of include/vnet_hip_score.h (the yardsticks of its tests and the path of a
CPU model), and `Accuracy`, which takes arrays (host) or int32 tensors on a HIP device (kernels) and returns equal values either way.

The reference scores with SimpleITK, which this project does not have.  What its filters compute is restated here from integer counts:

Overlap (sitk.LabelOverlapMeasuresImageFilter, GetDiceCoefficient() / GetJaccardCoefficient() with no label argument): over all
labels l >= 1, with I_l = #(gt == l and out == l), A_l = #(gt == l), B_l = #(out == l):
    Dice = 2 sum I / (sum A + sum B)        Jaccard = sum I / (sum A + sum B - sum I)
formed in float64 from the integer counts.  With no foreground in either map ITK divides by zero; here both are 0.0.

Items (sitk.ConnectedComponentImageFilter + LabelShapeStatisticsImageFilter, `Accuracy` of batch_evaluate_stride.py:48-122): the
components are those of the whole foreground mask (label != 0) with 6 neighbours -- ITK's defaults, and the rules vnet_cc_roots
states.  A component's centroid is (sum of its voxel indices / count) * spacing in float64.  The reference copies the ground truth's
origin and direction onto the output: both maps share them, the direction is orthonormal, so neither enters a distance between two
centroids and neither is carried here."""
import numpy as np

MAX_LABELS = 1024             # VNET_OVERLAP_MAX_LABELS
DEFAULT_COMPONENTS = 4096


# ---- restatements of the two entry points -----------------------------------------------------------------------------------------
def label_overlap(a, b, L):
    """vnet_label_overlap: int64 [L + 1, 3].  Row l < L = {#(a == l and b == l), #(a == l), #(b == l)}; row L = {0, #(a outside
    [0, L)), #(b outside [0, L))}."""
    a, b, L = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64), int(L)
    if a.shape != b.shape or a.size == 0:
        raise ValueError("label_overlap: two non-empty maps of one shape, got %d and %d elements" % (a.size, b.size))
    if not 1 <= L <= MAX_LABELS:
        raise ValueError("label_overlap: 1 <= L <= %d, got %d" % (MAX_LABELS, L))
    a = np.where((a >= 0) & (a < L), a, L)
    b = np.where((b >= 0) & (b < L), b, L)
    out = np.zeros((L + 1, 3), dtype=np.int64)
    out[:, 1] = np.bincount(a, minlength=L + 1)
    out[:, 2] = np.bincount(b, minlength=L + 1)
    out[:L, 0] = np.bincount(a[(a == b) & (a < L)], minlength=L)[:L]
    return out


def component_shapes(label, max_components=DEFAULT_COMPONENTS):
    """vnet_cc_shape: (n, rows int32 [m, 8], sums int64 [m, 3]) with m = min(n, max_components); n is the true number of components
    of label != 0, row k = {representative, count, lo[3], hi[3]} of scipy.ndimage.label's component k + 1 (sample.component_table),
    sums[k] = {sum x, sum y, sum z} over its voxels."""
    from scipy import ndimage
    from .sample import component_table
    label = np.asarray(label)
    if label.ndim != 3 or label.size == 0:
        raise ValueError("component_shapes: takes a non-empty [X,Y,Z] label map, got %s" % (label.shape,))
    cap = int(max_components)
    if cap < 1:
        raise ValueError("component_shapes: max_components %d" % cap)
    n, rows = component_table(label)
    sums = np.zeros((n, 3), dtype=np.int64)
    if n:
        cc = ndimage.label(label != 0)[0].reshape(-1)
        fg = np.flatnonzero(cc)
        idx = np.stack(np.unravel_index(fg, label.shape), axis=1).astype(np.int64)
        for a in range(3):
            sums[:, a] = _int_bincount(cc[fg], idx[:, a], n + 1)[1:]
    m = min(n, cap)
    return n, rows[:m].copy(), sums[:m].copy()


def _int_bincount(keys, values, length):
    """Exact int64 sums per key (np.bincount's weights are float64: exact only below 2^53)."""
    out = np.zeros(length, dtype=np.int64)
    np.add.at(out, keys, values)
    return out


# ---- the rules -------------------------------------------------------------------------------------------------------------------
def overlap_measures(counts):
    """(Dice, Jaccard) over all labels l >= 1 of a label_overlap table (rows {I, A, B}; the last row, labels out of range, has I = 0
    and counts as foreground in A and B, as ITK counts a label only one map holds): Dice = 2 sum I / (sum A + sum B), Jaccard =
    sum I / (sum A + sum B - sum I), float64 from the integer counts.
    Rule for empty maps: with no foreground in either map (sum A + sum B == 0) both are 0.0 -- ITK divides by zero there."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 2:
        raise ValueError("overlap_measures: an int64 [L + 1, 3] table, got %s" % (c.shape,))
    i, a, b = (int(v) for v in c[1:].sum(axis=0))
    if a + b == 0:
        return 0.0, 0.0
    return 2.0 * float(i) / float(a + b), float(i) / float(a + b - i)


def centroids(shapes, spacing):
    """float64 [m, 3]: (sums / count) * spacing of the rows of a component_shapes result."""
    _, rows, sums = shapes
    if len(rows) == 0:
        return np.zeros((0, 3), dtype=np.float64)
    return sums.astype(np.float64) / rows[:, 1:2].astype(np.float64) * np.asarray(spacing, dtype=np.float64)[None, :]


def item_scores(gt_shapes, out_shapes, spacing, tolerance, thickness_threshold=6, min_inplane=2, min_physical_size=None):
    """`Accuracy` of batch_evaluate_stride.py:48-122 on two component_shapes results: {"TP", "FP", "FN", "Item Sensitivity",
    "Item IoU"}.
    An OUTPUT component is dropped when its box extent along z is < thickness_threshold or along x or y is < min_inplane (extent =
    hi - lo + 1, ITK's GetBoundingBox()[3:6]); with min_physical_size, components of EITHER side with count * voxel volume below it are
    dropped too (the reference's `GetPhysicalSize(i + 1) >= pi * 4 / 3`).  A ground-truth centroid is a TP when some kept output
    centroid lies at Euclidean distance < tolerance, else an FN.  FP = kept outputs - TP, as the reference has it: two ground-truth
    items that share one output item make it NEGATIVE -- kept, not clamped.  Sensitivity = TP / (TP + FN), IoU = TP / (kept outputs +
    FN).  With no ground-truth item: TP = 0, FP = kept outputs, FN = 0, sensitivity and IoU 0.0.
    Both tables must be complete (n <= the capacity they were made with)."""
    for name, s in (("ground truth", gt_shapes), ("output", out_shapes)):
        if s[0] != len(s[1]):
            raise ValueError("item_scores: the %s has %d components, its table holds %d (raise max_components)" % (name, s[0], len(s[1])))
    sp = np.asarray(spacing, dtype=np.float64)
    voxel = float(np.prod(sp))

    def large(rows):
        if min_physical_size is None:
            return np.ones(len(rows), dtype=bool)
        return rows[:, 1].astype(np.float64) * voxel >= float(min_physical_size)
    g = centroids(gt_shapes, sp)[large(gt_shapes[1])]
    rows = out_shapes[1]
    ext = rows[:, 5:8].astype(np.int64) - rows[:, 2:5].astype(np.int64) + 1
    keep = (ext[:, 2] >= thickness_threshold) & (ext[:, 0] >= min_inplane) & (ext[:, 1] >= min_inplane) & large(rows)
    o = centroids(out_shapes, sp)[keep]
    kept = int(len(o))
    if len(g) == 0:
        return {"TP": 0, "FP": kept, "FN": 0, "Item Sensitivity": 0.0, "Item IoU": 0.0}
    tp = 0
    for c in g:
        d = np.sqrt(((o - c[None, :]) ** 2).sum(axis=1)) if kept else np.zeros(0)
        tp += bool((d < float(tolerance)).any())
    fn = len(g) - tp
    return {"TP": tp, "FP": kept - tp, "FN": fn, "Item Sensitivity": tp / float(tp + fn), "Item IoU": tp / float(kept + fn)}


# ---- the reference's entry point ---------------------------------------------------------------------------------------------------
def _on_device(x):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(x, torch.Tensor) and x.is_cuda


def _overlap(a, b, L):
    if _on_device(a):
        from . import ops
        return ops.label_overlap(a, b, L)
    return label_overlap(_array(a), _array(b), L)


def _array(x):
    return x.numpy() if hasattr(x, "numpy") and not isinstance(x, np.ndarray) else np.asarray(x)


def shapes_of(label, max_components=DEFAULT_COMPONENTS):
    """The COMPLETE component_shapes of an array (host) or an int32 device tensor (kernel): asked again with room for every
    component when there are more than max_components."""
    if _on_device(label):
        from . import ops
        fn = ops.component_shapes
    else:
        label, fn = _array(label), component_shapes
    s = fn(label, max_components)
    return s if s[0] <= max_components else fn(label, s[0])


def num_labels(*maps):
    """L for label_overlap: one past the largest label of the maps, at least 2 and at most MAX_LABELS (labels above land in row L)."""
    hi = max(int(m.max()) for m in maps)
    return max(2, min(hi + 1, MAX_LABELS))


def Accuracy(groundTruth, output, spacing=(1, 1, 1), tolerence=3, mode=("DICE",), L=None, gt_shapes=None):
    """The reference's Accuracy(groundTruth, output, tolerence, mode) on two label maps of one shape: a dict with DICE and Jaccard for
    "DICE" in mode, TP, FP, FN, Item Sensitivity and Item IoU for "ITEM" in mode.  (The ITEM branch of the reference's
    batch_evaluate.py cannot run -- `math` is not imported, `dice` is undefined, it returns a tuple; the behaviour kept is that of its
    batch_evaluate_stride.py with the thresholds of batch_evaluate.py: thickness 6, in-plane 2, no physical-size rule.)
    Arrays take the NumPy restatements; int32 tensors on a HIP device take the kernels (ops.label_overlap, ops.component_shapes) and
    only the count table and the component rows come to the host.  The values are equal either way.
    L: labels 0 .. L - 1 are counted one by one (None: read from the maps' maxima); gt_shapes: the ground truth's shapes_of, when the
    caller has them already."""
    if tuple(groundTruth.shape) != tuple(output.shape):
        raise ValueError("Accuracy: ground truth %s and output %s differ in shape" % (tuple(groundTruth.shape), tuple(output.shape)))
    if _on_device(groundTruth) != _on_device(output):
        raise ValueError("Accuracy: both maps are arrays, or both are tensors on the device")
    result = {}
    if "DICE" in mode:
        if L is None:
            L = num_labels(groundTruth, output)
        result["DICE"], result["Jaccard"] = overlap_measures(_overlap(groundTruth, output, L))
    if "ITEM" in mode:
        if gt_shapes is None:
            gt_shapes = shapes_of(groundTruth)
        result.update(item_scores(gt_shapes, shapes_of(output), spacing, tolerence))
    return result
