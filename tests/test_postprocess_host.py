"""No GPU: the rules of the post-processing pipeline (vnet_tensorflow_amd/postprocess.py) against independent statements -- the
component steps against scipy.ndimage.label per class and a brute-force flood, FillHoles against binary_fill_holes, the four
morphology ops against scipy.ndimage.binary_* with ball(r) and the stated border values -- the YAML dialect, the ledger of
csrc/vnet_post.h against the ctypes table (needs the built library), and evaluate_case on a CPU model.  Every comparison is `==` on
integers.  planted() is the generated label of tests/test_hip_postprocess.py too."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import guard
from tests.test_abi_ledger import RULE, _result_types
from vnet_tensorflow_amd import _lib, postprocess as PP, prepare_data

ROOT = guard.ROOT
SHAPES = [(1, 1, 1), (3, 4, 64), (5, 7, 65), (13, 17, 131)]
SP = (0.7, 0.8, 2.5)


# ---- the generated label -------------------------------------------------------------------------------------------------------------------
def planted(shape, seed=0, p=0.04):
    """(label int32, {shell name: the slices of its 3^3 inside}): sparse noise of classes 1 .. 3 and, where the volume has room
    (X, Y >= 9, Z >= 131), four hollow one-voxel shells of class 1 around 3^3 insides, each in a cleared 7^3 neighbourhood:
    `closed` (background inside), `tumour` (closed, a voxel of class 2 in the middle), `channel` (one shell voxel missing: the inside
    reaches the outside) and `cut` (cut by the face x = 0, so its inside lies on that face)."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    lab = (rng.integers(1, 4, size=shape) * (rng.random(shape) < p)).astype(np.int32)
    inside = {}
    if X < 9 or Y < 9 or Z < 131:
        return lab, inside

    def clip(lo, hi, n):
        return slice(max(lo, 0), min(hi, n))

    def shell(name, x0, y0, z0):
        lab[clip(x0 - 1, x0 + 6, X), clip(y0 - 1, y0 + 6, Y), clip(z0 - 1, z0 + 6, Z)] = 0
        lab[clip(x0, x0 + 5, X), clip(y0, y0 + 5, Y), clip(z0, z0 + 5, Z)] = 1
        inside[name] = (clip(x0 + 1, x0 + 4, X), clip(y0 + 1, y0 + 4, Y), clip(z0 + 1, z0 + 4, Z))
        lab[inside[name]] = 0

    shell("closed", 2, 2, 10)
    shell("tumour", 2, 2, 40)
    lab[4, 4, 42] = 2
    shell("channel", 2, 2, 70)
    lab[4, 4, 70] = 0
    shell("cut", -2, 2, 100)
    return lab, inside


def assert_not_vacuous(lab, inside, volume, spacing):
    """From the rules alone: the planted label exercises what the steps are for."""
    classes = [1, 2, 3]
    filled = PP.fill_holes(lab, classes)
    assert int(((filled != lab) & (lab == 0)).sum()) > 0 and not ((filled != lab) & (lab != 0)).any()
    assert (filled[inside["closed"]] == 1).all()
    t = filled[inside["tumour"]]
    assert t[1, 1, 1] == 2 and int((t == 1).sum()) == 26                   # the enclosed voxel of another class stays
    assert (filled[inside["channel"]] == 0).all() and (filled[inside["cut"]] == 0).all()
    for c in classes:
        assert ndimage.label(lab == c)[1] >= 2, c
    small = PP.remove_small(lab, volume, spacing, classes)
    assert int((small != 0).sum()) > 0 and int(((small == 0) & (lab != 0)).sum()) > 0
    return filled


# ---- independent statements ----------------------------------------------------------------------------------------------------------------
def flood_components(lab, c):
    """[(first voxel, sorted voxel list)] of the face-connected components of lab == c, by a brute-force flood in C order."""
    X, Y, Z = lab.shape
    seen, out = np.zeros(lab.shape, bool), []
    for v in range(lab.size):
        x, y, z = np.unravel_index(v, lab.shape)
        if lab[x, y, z] != c or seen[x, y, z]:
            continue
        stack, comp = [(x, y, z)], []
        seen[x, y, z] = True
        while stack:
            a = stack.pop()
            comp.append(int(np.ravel_multi_index(a, lab.shape)))
            for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                b = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
                if 0 <= b[0] < X and 0 <= b[1] < Y and 0 <= b[2] < Z and lab[b] == c and not seen[b]:
                    seen[b] = True
                    stack.append(b)
        out.append((v, sorted(comp)))
    return out


def flood_keep_largest(lab, classes):
    out = lab.copy().ravel()
    for c in classes:
        comps = flood_components(lab, c)
        if comps:
            best = max(comps, key=lambda fc: (len(fc[1]), -fc[0]))
            for f, comp in comps:
                if f != best[0]:
                    out[comp] = 0
    return out.reshape(lab.shape)


def flood_remove_small(lab, volume, spacing, classes):
    out = lab.copy().ravel()
    vv = float(np.prod(spacing))
    for c in classes:
        for _, comp in flood_components(lab, c):
            if not float(len(comp)) * vv > volume:
                out[comp] = 0
    return out.reshape(lab.shape)


def scipy_keep_largest(lab, classes):
    out = lab.copy()
    for c in classes:
        cc, n = ndimage.label(lab == c)
        if n:
            counts = ndimage.sum(np.ones(lab.shape, np.int64), cc, index=np.arange(1, n + 1)).astype(np.int64)
            out[(lab == c) & (cc != 1 + int(np.flatnonzero(counts == counts.max())[0]))] = 0
    return out


def small_labels():
    rng = np.random.default_rng(11)
    for shape in ((1, 1, 1), (2, 3, 4), (4, 4, 5), (3, 5, 6)):
        for p in (0.3, 0.6, 0.95):
            yield (rng.integers(1, 4, size=shape) * (rng.random(shape) < p)).astype(np.int32)


# ---- component steps -------------------------------------------------------------------------------------------------------------------------
def test_component_rules_against_a_flood():
    for lab in small_labels():
        for classes in ([1, 2, 3], [3, 1], [2]):
            assert np.array_equal(PP.keep_largest(lab, classes), flood_keep_largest(lab, classes))
            for volume in (0.0, 1.0, 2.5):
                assert np.array_equal(PP.remove_small(lab, volume, (1.0, 1.0, 1.0), classes), flood_remove_small(lab, volume, (1.0, 1.0, 1.0), classes))
        roots, sizes = PP.class_roots(lab, [1, 3])
        want_r, want_s = np.full(lab.size, -1, np.int32), np.zeros(lab.size, np.int32)
        for c in (1, 3):
            for f, comp in flood_components(lab, c):
                want_r[comp], want_s[f] = f, len(comp)
        assert np.array_equal(roots.ravel(), want_r) and np.array_equal(sizes.ravel(), want_s)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_component_rules_against_scipy_per_class(shape):
    lab, _ = planted(shape, seed=3)
    got = PP.keep_largest(lab, [1, 2, 3])
    assert np.array_equal(got, scipy_keep_largest(lab, [1, 2, 3]))
    only2 = PP.keep_largest(lab, [2])
    assert np.array_equal(only2[lab != 2], lab[lab != 2])                    # other classes untouched
    assert set(np.unique(got)) <= set(np.unique(lab))                         # class values preserved
    for c in (1, 2, 3):
        assert ndimage.label(got == c)[1] == min(1, int((lab == c).sum()))
    vv = float(np.prod(SP))
    small = PP.remove_small(lab, 1.5 * vv, SP, [1, 3])
    for c in (1, 3):
        cc, n = ndimage.label(lab == c)
        counts = np.bincount(cc.ravel(), minlength=n + 1)
        assert np.array_equal(small == c, (cc != 0) & (counts[cc] >= 2))
    assert np.array_equal(small == 2, lab == 2)


def test_two_classes_side_by_side_are_not_connected():
    lab = np.zeros((3, 3, 6), np.int32)
    lab[1, 1, 0:2], lab[1, 1, 2:5] = 2, 5                                    # touching runs of classes 2 and 5
    lab[0, 0, 0], lab[2, 2, 5] = 5, 2
    out = PP.keep_largest(lab, [2, 5])
    assert (out[1, 1, 0:2] == 2).all() and (out[1, 1, 2:5] == 5).all() and out[0, 0, 0] == 0 and out[2, 2, 5] == 0
    roots, sizes = PP.class_roots(lab, [2, 5])
    assert roots[1, 1, 1] == 24 and roots[1, 1, 4] == 26 and sizes[1, 1, 0] == 2 and sizes[1, 1, 2] == 3     # (1, 1, 0) is voxel 24
    assert (PP.class_roots(lab, [5])[0][lab == 2] == -1).all()


def test_ties_go_to_the_first_voxel_in_c_order():
    lab = np.zeros((5, 6, 7), np.int32)
    lab[0, 0, 1:5] = 3                                                        # 4 voxels, first voxel 1
    lab[3:5, 3:5, 3] = 3                                                      # 4 voxels, first voxel later
    lab[2, 0, 0:3] = 3                                                        # 3 voxels
    out = PP.keep_largest(lab, [3])
    assert (out[0, 0, 1:5] == 3).all() and int((out != 0).sum()) == 4
    rev = np.ascontiguousarray(lab[::-1, ::-1, ::-1])
    out = PP.keep_largest(rev, [3])
    assert (out[0:2, 1:3, 3] == 3).all() and int((out != 0).sum()) == 4
    assert np.array_equal(out, flood_keep_largest(rev, [3]))


def test_the_threshold_is_strict_and_in_double():
    lab = np.zeros((6, 6, 6), np.int32)
    lab[0:2, 0:2, 0:2] = 1                                                    # 8 voxels: 8 * 0.125 == 1.0 exactly in double -> dropped
    lab[3:6, 3:6, 5] = 2                                                      # 9 voxels: kept
    sp = (0.5, 0.5, 0.5)
    assert 8.0 * float(np.prod(sp)) == 1.0
    out = PP.remove_small(lab, 1.0, sp, [1, 2])
    assert not (out == 1).any() and np.array_equal(out == 2, lab == 2)
    assert np.array_equal(PP.remove_small(lab, np.nextafter(1.0, 0.0), sp, [1, 2]), lab)
    odd = (0.3, 0.7, 1.1)                                                     # a product that rounds: count * prod decides, as the host forms it
    v = 8.0 * float(np.prod(odd))
    assert not (PP.remove_small(lab, v, odd, [1]) == 1).any() and (PP.remove_small(lab, np.nextafter(v, 0.0), odd, [1]) == 1).sum() == 8


# ---- FillHoles -------------------------------------------------------------------------------------------------------------------------------
def test_fill_holes_against_scipy_and_the_planted_shells():
    lab, inside = planted((13, 17, 131), seed=0)
    filled = assert_not_vacuous(lab, inside, 1.5 * float(np.prod(SP)), SP)
    run = lab.copy()
    for c in (1, 2, 3):
        run[ndimage.binary_fill_holes(run == c) & (run == 0)] = c
    assert np.array_equal(filled, run)
    # in words: the complement's components that touch no face are the cavities
    cc, n = ndimage.label(lab != 1)
    on_face = set(np.unique(np.concatenate([cc[0].ravel(), cc[-1].ravel(), cc[:, 0].ravel(), cc[:, -1].ravel(), cc[:, :, 0].ravel(),
                                            cc[:, :, -1].ravel()])))
    cavity = ~np.isin(cc, sorted(on_face)) & (cc != 0)
    assert np.array_equal(PP.fill_holes(lab, [1]), np.where(cavity & (lab == 0), 1, lab))
    for shape in SHAPES[:3]:
        small, _ = planted(shape, seed=1, p=0.5)
        assert np.array_equal(PP.fill_holes(small, [2]), np.where(ndimage.binary_fill_holes(small == 2) & (small == 0), 2, small))


def test_fill_holes_runs_in_the_given_order_on_the_running_label():
    lab = np.zeros((7, 7, 7), np.int32)
    lab[1:6, 1:6, 1:6] = 1
    lab[2:5, 2:5, 2:5] = 2
    lab[3, 3, 3] = 0                                                          # a hole inside 2, which lies inside 1
    assert PP.fill_holes(lab, [1, 2])[3, 3, 3] == 1 and PP.fill_holes(lab, [2, 1])[3, 3, 3] == 2


# ---- morphology ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 3])
def test_mask_ops_against_scipy(r):
    ball = prepare_data.ball(r)
    for shape in ((1, 1, 1), (3, 4, 64), (5, 7, 65), (9, 6, 11)):
        m = np.random.default_rng(r).random(shape) < 0.6
        d = ndimage.binary_dilation(m, ball, border_value=0)
        e = ndimage.binary_erosion(m, ball, border_value=1)
        assert np.array_equal(PP.dilate_mask(m, r), d) and np.array_equal(PP.erode_mask(m, r), e)
        o, c = PP.open_mask(m, r), PP.close_mask(m, r)
        assert np.array_equal(o, ndimage.binary_dilation(e, ball, border_value=0))
        assert np.array_equal(c, ndimage.binary_erosion(d, ball, border_value=1))
        assert (c >= m).all() and np.array_equal(PP.close_mask(c, r), c)            # extensive, idempotent
        assert (o <= m).all() and np.array_equal(PP.open_mask(o, r), o)             # anti-extensive (and idempotent)
        assert (d >= m).all() and (e <= m).all()


def test_morphology_grows_into_the_background_only():
    lab, _ = planted((5, 7, 65), seed=2, p=0.3)
    for op in ("Dilate", "Erode", "Open", "Close"):
        run = lab.copy()
        for c in (2, 1):
            m2 = PP.MASK_OPS[op](run == c, 1)
            run = np.where(m2 & (run == 0), c, np.where((run == c) & ~m2, 0, run))
        got = PP.morphology(lab, op, 1, [2, 1])
        assert got.dtype == lab.dtype and np.array_equal(got, run)
    grown = PP.morphology(lab, "Dilate", 2, [1])
    assert np.array_equal(grown[(lab != 0) & (lab != 1)], lab[(lab != 0) & (lab != 1)])   # never overwrites another class
    assert np.array_equal(grown == 1, (lab == 1) | (PP.dilate_mask(lab == 1, 2) & (lab == 0)))
    shrunk = PP.morphology(lab, "Erode", 1, [3])
    assert np.array_equal(shrunk[lab != 3], lab[lab != 3]) and set(np.unique(shrunk)) <= {0, 1, 2, 3}


# ---- YAML ------------------------------------------------------------------------------------------------------------------------------------
PIPELINE = """
preprocess:
  evaluate:
    3D:
      - name: "StatisticalNormalization"
        variables:
          sigma: 2.5
postprocess:
  evaluate:
    3D:
      - name: "KeepLargestComponent"
      - name: "RemoveSmallComponents"
        variables:
          volume: 12.5
          classes: [1, 3]
      - name: "FillHoles"
        variables:
          classes: [2]
      - name: "Close"
        variables:
          radius: 2
"""


def _yaml(tmp_path, text, name="pipeline.yaml"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def _one(tmp_path, step):
    return _yaml(tmp_path, "postprocess:\n  evaluate:\n    3D:\n      - %s\n" % step)


def test_build_reads_the_file_shared_with_preprocess(tmp_path):
    from vnet_tensorflow_amd import transforms
    path = _yaml(tmp_path, PIPELINE)
    steps = PP.build(path)
    assert [type(s).__name__ for s in steps] == ["KeepLargestComponent", "RemoveSmallComponents", "FillHoles", "Close"]
    assert steps[0].classes is None and steps[1].volume == 12.5 and steps[1].classes == [1, 3] and steps[2].classes == [2]
    assert steps[3].radius == 2 and steps[3].classes is None
    assert len(transforms.build_pipeline(path, "evaluate")) == 1            # the other section is read as before
    assert PP.build(_yaml(tmp_path, "preprocess:\n  evaluate:\n    3D: []\n", "none.yaml")) == []
    lab, _ = planted((5, 7, 65), seed=4, p=0.3)
    want = PP.morphology(PP.fill_holes(PP.remove_small(PP.keep_largest(lab, [1, 2, 3]), 12.5, SP, [1, 3]), [2]), "Close", 2, [1, 2, 3])
    got = PP.run(steps, lab, SP, classes=4)
    assert got.dtype == lab.dtype and np.array_equal(got, want)
    assert np.array_equal(PP.run(steps, lab, SP), want)                      # K read from the label
    assert np.array_equal(PP.run([], lab, SP, classes=4), lab)
    cpu = PP.run(steps, torch.from_numpy(lab), SP, classes=4)               # a CPU model's label
    assert cpu.dtype == torch.int32 and np.array_equal(cpu.numpy(), want)


@pytest.mark.parametrize("step, word", [
    ('{name: "TopComponents"}', "TopComponents"),
    ('{name: "FillHoles", variables: {connectivity: 26}}', "connectivity"),
    ('{name: "Close", variables: {radius: 1, volume: 2}}', "volume"),
    ('{name: "FillHoles", variables: {classes: [0, 1]}}', "class 0"),
    ('{name: "KeepLargestComponent", variables: {classes: [%s]}}' % ", ".join(str(c) for c in range(1, 18)), "17"),
    ('{name: "Dilate", variables: {radius: 0}}', "radius 0"),
    ('{name: "Open", variables: {radius: 9}}', "radius 9"),
    ('{name: "Erode"}', "radius"),
    ('{name: "KeepLargestComponent", variables: {classes: [2, 2]}}', "distinct"),
])
def test_build_refuses_what_it_does_not_know(tmp_path, step, word):
    with pytest.raises(ValueError, match=word):
        PP.build(_one(tmp_path, step))


def test_sixteen_classes_and_radius_eight_are_taken(tmp_path):
    steps = PP.build(_one(tmp_path, '{name: "Dilate", variables: {radius: 8, classes: [%s]}}' % ", ".join(str(c) for c in range(1, 17))))
    assert steps[0].radius == 8 and steps[0].classes == list(range(1, 17))
    with pytest.raises(ValueError, match="at most 16"):
        PP.run([PP.FillHoles()], np.zeros((2, 2, 2), np.int32), classes=18)


# ---- csrc/vnet_post.h: declared == bound == exported ------------------------------------------------------------------------------------------
def test_post_header_ledger():
    path = os.path.join(ROOT, PP.HEADER)
    fns = guard.header_functions(path)
    assert set(fns) == set(PP.SIGNATURES_POST) and len(fns) == 7
    exported = ctypes.CDLL(PP.LIB_PATH)
    assert not [n for n in fns if not hasattr(exported, n)]
    results = _result_types(path)
    for name, params in fns.items():
        res, args = PP.SIGNATURES_POST[name]
        want = [ctypes.c_void_p if (p[1] and p[3].replace(" ", "") != "constchar*") else RULE[p[3]] for p in params]
        assert args == want, (name, args, want)
        assert res is RULE[results[name]] and (res is ctypes.c_size_t) == name.endswith("_ws_bytes"), name
    pointer = guard.pointer_entry_points(path)
    assert set(pointer) == {n for n in fns if not n.endswith("_ws_bytes")} and len(pointer) == 5
    assert all(ps[-1][0] == "stream" for ps in pointer.values())
    # a library of its own: none of these names is in the training library's registry, the header is not published
    assert not set(fns) & set(_lib.all_signatures()) and PP.HEADER not in [h for h, _ in _lib.HEADERS]
    assert not os.path.exists(os.path.join(ROOT, "include", "vnet_post.h")) and os.path.basename(PP.LIB_PATH) == "libvnet_post.so"
    main = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in fns if hasattr(main, n)]
    mk = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "Makefile")).read()
    for word in ("POST_SRCS = postprocess.hip", "POST_OBJS", "POST_LIB  = ../libvnet_post.so", "$(POST_OBJS): vnet_post.h"):
        assert word in mk, word
    assert "#define VNET_POST_MAX_VALUES %d" % PP.MAX_CLASSES in open(path).read()
    assert PP.lib().vnet_post_fill_holes.argtypes == PP.SIGNATURES_POST["vnet_post_fill_holes"][1]


def test_error_codes_need_no_device():
    """Before any launch, in the documented order: VNET_E_BADARG (-1), VNET_E_UNSUPPORTED (-2), VNET_E_WORKSPACE (-3); the size queries
    answer 0 for what the entry points refuse."""
    L = PP.lib()
    one, dims, big = ctypes.c_void_p(16), (5, 4, 3), (2048, 2048, 512)
    vals = (ctypes.c_int * 3)(1, 2, 3)
    need_f, need_h = L.vnet_post_filter_components_ws_bytes(*dims), L.vnet_post_fill_holes_ws_bytes(*dims)
    assert need_f == 128 + 128 * 1 + 8 * 60 and need_h == 5 * 60          # the keys, a row of keys per block of 256 voxels, roots and sizes
    assert L.vnet_post_filter_components_ws_bytes(9, 251, 517) == 128 + 128 * 4096 + 8 * 9 * 251 * 517              # (the grid cap)
    assert L.vnet_post_filter_components_ws_bytes(*big) == 0 and L.vnet_post_fill_holes_ws_bytes(0, 4, 3) == 0
    roots = lambda label=one, values=vals, n=3, out=one, d=dims: L.vnet_post_class_roots(label, values, n, out, None, *d, None)
    filt = lambda label=one, out=one, values=vals, n=3, mode=0, vol=1.0, vv=1.0, d=dims, ws=one, nb=need_f: \
        L.vnet_post_filter_components(label, out, values, n, mode, vol, vv, *d, ws, nb, None)
    fill = lambda label=one, out=one, k=1, d=dims, ws=one, nb=need_h: L.vnet_post_fill_holes(label, out, k, *d, ws, nb, None)
    assert roots(label=None) == -1 and roots(values=None) == -1 and roots(out=None) == -1 and roots(n=0) == -1 and roots(n=17) == -1
    assert roots(values=(ctypes.c_int * 3)(1, 0, 3)) == -1 and roots(values=(ctypes.c_int * 3)(1, 2, 1)) == -1
    assert roots(d=(5, 0, 3)) == -1 and roots(d=big) == -2
    assert filt(label=None) == -1 and filt(out=None) == -1 and filt(ws=None) == -1 and filt(ws=ctypes.c_void_p(20)) == -1
    assert filt(mode=2) == -1 and filt(mode=-1) == -1 and filt(n=17) == -1 and filt(d=(5, 4, -1)) == -1
    assert filt(mode=1, vol=float("nan")) == -1 and filt(mode=1, vv=float("inf")) == -1
    assert filt(d=big, nb=1 << 40) == -2 and filt(nb=need_f - 1) == -3 and filt(d=big, nb=0) == -2       # UNSUPPORTED before WORKSPACE
    assert filt(n=17, d=big, nb=0) == -1                                                                    # BADARG before both
    assert fill(label=None) == -1 and fill(out=None) == -1 and fill(k=0) == -1 and fill(ws=None) == -1 and fill(d=(0, 4, 3)) == -1
    assert fill(d=big, nb=0) == -2 and fill(nb=need_h - 1) == -3 and fill(k=0, d=big, nb=0) == -1
    assert L.vnet_post_not_bits(None, one, *dims, None) == -1 and L.vnet_post_not_bits(one, one, *dims, None) == -1   # in place
    assert L.vnet_post_not_bits(one, ctypes.c_void_p(32), 5, 4, 0, None) == -1 and L.vnet_post_not_bits(one, ctypes.c_void_p(32), *big, None) == -2
    assert L.vnet_post_apply_bits(None, one, 1, one, *dims, None) == -1 and L.vnet_post_apply_bits(one, one, 0, one, *dims, None) == -1
    assert L.vnet_post_apply_bits(one, None, 1, one, *dims, None) == -1 and L.vnet_post_apply_bits(one, one, 1, one, *big, None) == -2


def test_ops_refuse_cpu_tensors():
    from vnet_tensorflow_amd._lib import VnetHipError
    lab = torch.ones(5, 4, 3, dtype=torch.int32)
    for fn in (lambda: PP.class_roots_device(lab, [1]), lambda: PP.filter_components(lab, [1], 0), lambda: PP.fill_holes_class(lab, 1),
               lambda: PP.apply_bits(lab, torch.zeros(5, 4, 1, dtype=torch.int64), 1)):
        with pytest.raises(VnetHipError, match="on cpu"):
            fn()


# ---- evaluate on a CPU model -----------------------------------------------------------------------------------------------------------------
VOLUME = (24, 20, 18)


@pytest.fixture()
def cpu_model(monkeypatch):
    """A model on the CPU whose network and accumulation are stood in for (the kernels have no CPU path): the softmax of a window is a
    fixed function of its intensities, so the label has several classes and components."""
    from vnet_tensorflow_amd import model, ops
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": ".", "TestingDataDirectory": ".", "ImageFilenames": ["image.nii"], "LabelFilename": "label.nii"},
        "BatchSize": 1, "PatchShape": [16, 16, 16], "SegmentationClasses": [0, 1, 2], "Epoches": 1,
        "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 1], "BottomConvolutions": 1},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}},
        "Loss": {"Name": "sorensen"}},
        "EvaluationSetting": {"Data": {"EvaluateDataDirectory": ".", "ImageFilenames": ["image.nii"], "LabelFilename": "label_tf.nii"},
                              "CheckpointPath": "ckpt", "Stride": [8, 8, 8], "BatchSize": 4}}
    m = model.image2label(None, cfg, device=torch.device("cpu"), verbose=False)
    m.read_config()
    m.build_model_graph()

    def infer(batch):
        x = batch[..., 0]
        return torch.stack([(x < 0.55).float(), ((x >= 0.55) & (x < 0.8)).float(), (x >= 0.8).float()], dim=-1)

    def accumulate(patch, vol, cnt, origin):
        sl = tuple(slice(o, o + n) for o, n in zip(origin, patch.shape[:3]))
        vol[sl] += patch
        cnt[sl] += 1
    monkeypatch.setattr(m, "_infer", infer)
    monkeypatch.setattr(ops, "accumulate_patch", accumulate)
    image = np.random.default_rng(5).random(VOLUME + (1,)).astype(np.float32)
    return m, image


def test_evaluate_case_on_a_cpu_model(cpu_model, tmp_path):
    m, image = cpu_model
    plain, _ = m.evaluate_case(image, SP, None, False)
    assert plain.shape == VOLUME and set(np.unique(plain)) == {0, 1, 2}
    seen = []
    m.evaluate_postprocess = _yaml(tmp_path, PIPELINE)
    got, _ = m.evaluate_case(image, SP, None, False, on_label=lambda t: seen.append(t.numpy().copy()))
    want = PP.run(PP.build(m.evaluate_postprocess), plain, SP, classes=3)
    assert (want != plain).any() and got.dtype == plain.dtype and np.array_equal(got, want)
    assert len(seen) == 1 and seen[0].dtype == np.int32 and np.array_equal(seen[0], want)      # the scorer gets the processed label
    # the key absent or empty: what it was, bit for bit, down the fast path
    for off in (None, ""):
        m.evaluate_postprocess = off
        again, _ = m.evaluate_case(image, SP, None, False)
        assert again.dtype == plain.dtype and again.tobytes() == plain.tobytes()
    direct, _ = m.evaluate_single_3D(image, postprocess=PP.build(_yaml(tmp_path, PIPELINE)), spacing=SP)
    assert np.array_equal(direct, want)
    assert m.evaluate_single_3D(image, postprocess=[])[0].tobytes() == plain.tobytes()


def test_the_config_key_and_the_command_line(tmp_path):
    import inspect
    from vnet_tensorflow_amd import batch_evaluate as BE, model
    p = inspect.signature(model.image2label.evaluate_single_3D).parameters
    assert p["postprocess"].default is None and list(p)[-2:] == ["postprocess", "on_label"]         # (on_label stays the last one)
    args = ["-cd", str(tmp_path), "-d", str(tmp_path), "-o", str(tmp_path)]
    assert BE.get_args(args).postprocess is None and BE.get_args(args + ["--postprocess", "p.yaml"]).postprocess == "p.yaml"
    cfg = {"TrainingSetting": {"PatchShape": [16, 16, 16]}, "EvaluationSetting": {"Postprocess": "config.yaml"}}
    assert BE.Batch_Evaluate(config_json=cfg, patch_size=None, patch_layer=None).config()["EvaluationSetting"]["Postprocess"] == "config.yaml"
    over = BE.Batch_Evaluate(config_json=cfg, patch_size=None, patch_layer=None, postprocess="cli.yaml").config()
    assert over["EvaluationSetting"]["Postprocess"] == "cli.yaml" and cfg["EvaluationSetting"]["Postprocess"] == "config.yaml"
