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


# ---- surface distances: the rules and the restatements of csrc/vnet_surface.h ---------------------------------------------------------
# The reference has no surface score; these are the usual definitions, stated in full because there is no SimpleITK here to copy.
#   MASK of a label map [X,Y,Z] and a class: label != 0 for klass == 0, label == klass for klass > 0.
#   SURFACE S(M): the voxels of M with at least one of their 6 neighbours outside M; outside the volume counts as outside M.
#   SQUARED DISTANCE FIELD to a set S, fp64, every operation rounded once, nothing contracted: s2_a = fl(sp_a sp_a),
#       D2(v) = min over s in S of fl(fl(s2_x dx^2) + fl(fl(s2_y dy^2) + fl(s2_z dz^2))), the integer squares exact; +inf for empty S.
#     fl(a + t) is monotone in t, so the minimum may be taken axis by axis and gives the same bits, whatever search finds it:
#       G1 = min_z' fl(s2_z dz^2),  G2 = min_y' fl(fl(s2_y dy^2) + G1),  D2 = min_x' fl(fl(s2_x dx^2) + G2).
#   SCORES of ground truth g and output o: L1 = D2 to S(o) at the voxels of S(g), L2 = D2 to S(g) at the voxels of S(o), L their union,
#   n = n1 + n2:  HD = sqrt(max L);  HD95 = sqrt(sorted(L)[(95 n + 99) // 100 - 1]) -- nearest rank in integers, the smallest distance
#   that covers >= 95 % of all surface voxels;  ASSD = (sum sqrt L1 + sum sqrt L2) / n.  Both surfaces empty: everything 0.0.  Exactly
#   one empty: everything inf (the field to an empty set is +inf, so the formulas say so themselves; the mean over the empty side is
#   inf by rule).  The selected D2 values get their root on the host (np.sqrt, correctly rounded); sqrt is monotone, so selecting on
#   D2 is exact.
def class_mask(label, klass=0):
    label, klass = np.asarray(label), int(klass)
    if label.ndim != 3 or label.size == 0:
        raise ValueError("class_mask: takes a non-empty [X,Y,Z] label map, got %s" % (label.shape,))
    if klass < 0:
        raise ValueError("class_mask: klass %d" % klass)
    return label != 0 if klass == 0 else label == klass


def surface_mask(label, klass=0):
    """vnet_surface_bits before packing: bool [X,Y,Z], M & ~erosion(M) with the 6-neighbour cross and the border outside."""
    from scipy import ndimage
    m = class_mask(label, klass)
    return m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(3, 1), border_value=0)


def pack(mask):
    """bool / 0-1 [X,Y,Z] -> the packed mask int64 [X,Y,ceil(Z/64)] of morph.py (prepare_data.pack_bits)."""
    from .prepare_data import pack_bits
    return pack_bits(mask)


def _spacing2(spacing):
    sp = np.asarray(spacing, dtype=np.float64)
    if sp.shape != (3,) or not np.all((sp > 0) & np.isfinite(sp)):
        raise ValueError("spacing %r is not three positive numbers" % (spacing,))
    return sp * sp


def _axis_min(G, s2, axis, budget=1 << 22):
    """min over a' of fl(fl(s2 (a - a')^2) + G[.. a' ..]) along `axis`, a chunk of a at a time."""
    G = np.moveaxis(G, axis, 0)
    A, rest = G.shape[0], G.shape[1:]
    idx = np.arange(A, dtype=np.float64)
    out = np.empty_like(G)
    chunk = max(1, budget // max(1, A * int(np.prod(rest))))
    for a0 in range(0, A, chunk):
        t = s2 * (idx[a0:a0 + chunk, None] - idx[None, :]) ** 2                      # [chunk, A]: the squares exact, one rounding
        out[a0:a0 + chunk] = (t.reshape(t.shape + (1,) * len(rest)) + G[None]).min(axis=1)
    return np.moveaxis(out, 0, axis)


def edt2(mask, spacing=(1.0, 1.0, 1.0)):
    """vnet_edt2: float64 [X,Y,Z], the squared distance field to the set voxels of `mask` in its separable form."""
    mask = np.asarray(mask) != 0
    if mask.ndim != 3 or mask.size == 0:
        raise ValueError("edt2: takes a non-empty [X,Y,Z] mask, got %s" % (mask.shape,))
    s2 = _spacing2(spacing)
    G = np.where(mask, 0.0, np.inf)
    for axis in (2, 1, 0):
        G = _axis_min(G, s2[axis], axis)
    return G


def edt2_brute(mask, spacing=(1.0, 1.0, 1.0)):
    """The definition itself, the minimum over every set voxel (tiny shapes only)."""
    mask = np.asarray(mask) != 0
    s2 = _spacing2(spacing)
    out = np.full(mask.shape, np.inf)
    gx, gy, gz = (g.astype(np.float64) for g in np.meshgrid(*(np.arange(n) for n in mask.shape), indexing="ij"))
    for x, y, z in np.argwhere(mask):
        out = np.minimum(out, s2[0] * (gx - x) ** 2 + (s2[1] * (gy - y) ** 2 + s2[2] * (gz - z) ** 2))
    return out


def gather(d2, mask):
    """vnet_surface_gather with room for all: the values of d2 at the set voxels of mask, in voxel (C) order."""
    return np.asarray(d2, dtype=np.float64)[np.asarray(mask) != 0]


def kth(values, ranks):
    """vnet_list_select: the elements of 0-based rank `ranks` of a list of non-negative numbers."""
    return np.sort(np.asarray(values, dtype=np.float64))[np.asarray(ranks, dtype=np.int64)]


def hd95_rank(n):
    """The 0-based rank of the 95th percentile of n >= 1 numbers by nearest rank: ceil(0.95 n) - 1 in integers."""
    n = int(n)
    if n < 1:
        raise ValueError("hd95_rank: n %d" % n)
    return (95 * n + 99) // 100 - 1


SURFACE_KEYS = ("HD", "HD95", "ASSD", "n_gt", "n_out", "mean_gt_to_out", "mean_out_to_gt")


def _surface_result(n1, n2, hd2=0.0, hd95_2=0.0, s1=0.0, s2=0.0):
    """The rule from the two selected squared distances and the two sums of roots."""
    if n1 == 0 and n2 == 0:
        v = (0.0,) * 5
    elif n1 == 0 or n2 == 0:
        v = (float("inf"),) * 5
    else:
        v = (float(np.sqrt(np.float64(hd2))), float(np.sqrt(np.float64(hd95_2))), float((np.float64(s1) + np.float64(s2)) / (n1 + n2)),
             float(np.float64(s1) / n1), float(np.float64(s2) / n2))
    return {"HD": v[0], "HD95": v[1], "ASSD": v[2], "n_gt": int(n1), "n_out": int(n2), "mean_gt_to_out": v[3], "mean_out_to_gt": v[4]}


def surface_field(label, spacing, klass=0):
    """(surface, D2 to it) of a label map: what surface_distances needs of one side, for a caller that scores the same ground truth
    again and again.  An array gives (bool mask, float64 array); an int32 device tensor gives (packed mask, float64 tensor)."""
    if _on_device(label):
        from . import surface as S
        bits = S.surface_bits(label, klass)
        return bits, S.edt2(bits, label.shape[2], spacing)
    s = surface_mask(_array(label), klass)
    return s, edt2(s, spacing)


def surface_distances(gt, out, spacing=(1.0, 1.0, 1.0), klass=0, gt_field=None):
    """{"HD", "HD95", "ASSD", "n_gt", "n_out", "mean_gt_to_out", "mean_out_to_gt"} of two label maps of one shape by the rules above.
    Arrays take the NumPy restatements; int32 tensors on a HIP device take the kernels (vnet_tensorflow_amd/surface.py) and only the two
    counts and four numbers come to the host.  HD, HD95 and the counts are equal either way; ASSD and the two means rest on sums of
    roots, which agree within (n + 2) 2^-52 relative.  gt_field: the ground truth's surface_field, when the caller has it already."""
    if tuple(gt.shape) != tuple(out.shape):
        raise ValueError("surface_distances: ground truth %s and output %s differ in shape" % (tuple(gt.shape), tuple(out.shape)))
    if _on_device(gt) != _on_device(out):
        raise ValueError("surface_distances: both maps are arrays, or both are tensors on the device")
    if _on_device(gt):
        from . import surface as S
        Z = int(gt.shape[2])
        sg, fg = gt_field if gt_field is not None else (S.surface_bits(gt, klass), None)
        so = S.surface_bits(out, klass)
        n1, n2 = S.popcounts([sg, so], Z)
        if n1 == 0 or n2 == 0:
            return _surface_result(n1, n2)
        if fg is None:
            fg = S.edt2(sg, Z, spacing)
        fo = S.edt2(so, Z, spacing)
        both = S.empty_list(n1 + n2, gt.device)
        S.gather(fo, sg, Z, out=both, offset=0)
        S.gather(fg, so, Z, out=both, offset=n1)
        four = S.empty_list(4, gt.device)
        S.kth(both, [n1 + n2 - 1, hd95_rank(n1 + n2)], out=four[0:2])
        S.root_sum(both[:n1], out=four[2:3])
        S.root_sum(both[n1:], out=four[3:4])
        return _surface_result(n1, n2, *four.cpu().tolist())
    sg, fg = gt_field if gt_field is not None else surface_field(gt, spacing, klass)
    so = surface_mask(_array(out), klass)
    n1, n2 = int(np.count_nonzero(sg)), int(np.count_nonzero(so))
    if n1 == 0 or n2 == 0:
        return _surface_result(n1, n2)
    l1, l2 = gather(edt2(so, spacing), sg), gather(fg, so)
    hd2, hd95_2 = kth(np.concatenate([l1, l2]), [n1 + n2 - 1, hd95_rank(n1 + n2)])
    return _surface_result(n1, n2, hd2, hd95_2, np.sqrt(l1).sum(), np.sqrt(l2).sum())


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


def Accuracy(groundTruth, output, spacing=(1, 1, 1), tolerence=3, mode=("DICE",), L=None, gt_shapes=None, gt_field=None):
    """The reference's Accuracy(groundTruth, output, tolerence, mode) on two label maps of one shape: a dict with DICE and Jaccard for
    "DICE" in mode, TP, FP, FN, Item Sensitivity and Item IoU for "ITEM" in mode, HD, HD95 and ASSD of the foreground (surface_distances
    with klass 0; not in the reference) for "SURFACE" in mode.  (The ITEM branch of the reference's
    batch_evaluate.py cannot run -- `math` is not imported, `dice` is undefined, it returns a tuple; the behaviour kept is that of its
    batch_evaluate_stride.py with the thresholds of batch_evaluate.py: thickness 6, in-plane 2, no physical-size rule.)
    Arrays take the NumPy restatements; int32 tensors on a HIP device take the kernels (ops.label_overlap, ops.component_shapes) and
    only the count table and the component rows come to the host.  The values are equal either way.
    L: labels 0 .. L - 1 are counted one by one (None: read from the maps' maxima); gt_shapes: the ground truth's shapes_of, when the
    caller has them already; gt_field: the ground truth's surface_field(groundTruth, spacing), likewise."""
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
    if "SURFACE" in mode:
        d = surface_distances(groundTruth, output, spacing, 0, gt_field)
        result.update({k: d[k] for k in ("HD", "HD95", "ASSD")})
    return result
