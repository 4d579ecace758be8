"""CPU tests of the surface-distance scores (vnet_tensorflow_amd/score.py: surface_mask, edt2, surface_distances, Accuracy's SURFACE mode;
batch_evaluate.py's --mode SURFACE) and what csrc/vnet_surface.h alone has to say beside its row of tests/test_abi_ledger.py (needs
the built library)."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import guard
from tests.test_score_host import CFG, StandIn, _sweep_folders
from vnet_tensorflow_amd import _lib, batch_evaluate as BE, data, score as SC, surface

ROOT = guard.ROOT
SPACINGS = [(1.0, 1.0, 1.0), (0.7, 0.7, 2.5), (3.0, 0.5, 1.0)]


def _masks(shape, seed=0):
    rng = np.random.default_rng(seed)
    yield "empty", np.zeros(shape, bool)
    yield "full", np.ones(shape, bool)
    m = np.zeros(shape, bool)
    m[0, 0, 0] = True
    yield "corner", m
    m = np.zeros(shape, bool)
    m[shape[0] // 2] = True
    yield "plane", m
    yield "noise", rng.random(shape) < 0.3


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 7), (3, 1, 1), (3, 4, 5), (5, 3, 9)])
def test_separable_field_is_the_brute_force_minimum_bit_for_bit(shape):
    for name, m in _masks(shape):
        for sp in SPACINGS:
            assert np.array_equal(SC.edt2(m, sp), SC.edt2_brute(m, sp)), (name, sp)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 4, 5), (9, 10, 17), (17, 9, 66)])
def test_field_against_scipy(shape):
    """sqrt(D2) against scipy.ndimage.distance_transform_edt: exact at unit spacing (integer squares, one correctly rounded root on
    both sides), rtol 1e-14 otherwise (at most 6 roundings here, scipy's own there: ~45 ulp is a derived bound)."""
    for name, m in _masks(shape):
        if not m.any():
            assert np.all(np.isposinf(SC.edt2(m)))                   # (scipy has no answer for an empty set)
            continue
        for sp in SPACINGS:
            got, want = np.sqrt(SC.edt2(m, sp)), ndimage.distance_transform_edt(~m, sampling=sp)
            if sp == (1.0, 1.0, 1.0):
                assert np.array_equal(got, want), name
            else:
                assert np.allclose(got, want, rtol=1e-14, atol=0.0), (name, sp)


def test_surface_mask_and_class_mask():
    lab = np.zeros((5, 6, 7), np.int32)
    lab[1:4, 1:5, 1:6] = 1
    lab[2, 2, 2] = 2
    s = SC.surface_mask(lab)
    assert s.dtype == bool and s.sum() == 3 * 4 * 5 - 1 * 2 * 3 and not s[2, 2, 3] and s[1, 1, 1]
    assert np.array_equal(SC.surface_mask(lab, 2), lab == 2) and SC.surface_mask(lab, 1)[2, 2, 3]         # a hole makes surface
    full = np.ones((3, 3, 3), np.int32)
    assert SC.surface_mask(full).sum() == 26                                                              # the border is outside
    with pytest.raises(ValueError):
        SC.class_mask(lab, -1)
    packed = SC.pack(np.ones((1, 1, 70), bool))
    assert packed.dtype == np.int64 and packed.shape == (1, 1, 2) and packed[0, 0, 0] == -1 and packed[0, 0, 1] == 63


def test_hd95_rank_on_hand_made_lists():
    assert [SC.hd95_rank(n) for n in (1, 2, 19, 20, 21, 100, 101)] == [0, 1, 18, 18, 19, 94, 95]
    for n in list(range(1, 60)) + [99, 100, 101, 200, 399]:
        v = np.random.default_rng(n).random(n)
        assert SC.kth(v, [SC.hd95_rank(n)])[0] == np.percentile(v, 95, method="inverted_cdf"), n
    with pytest.raises(ValueError):
        SC.hd95_rank(0)
    # two single voxels 3 apart along z, spacing 2: every list entry is 36
    g, o = np.zeros((1, 1, 9), np.int32), np.zeros((1, 1, 9), np.int32)
    g[0, 0, 1], o[0, 0, 4] = 1, 1
    r = SC.surface_distances(g, o, (1, 1, 2))
    assert r == {"HD": 6.0, "HD95": 6.0, "ASSD": 6.0, "n_gt": 1, "n_out": 1, "mean_gt_to_out": 6.0, "mean_out_to_gt": 6.0}
    # 19 voxels of the output on the ground truth's line, one 4 away: n = 20 + 20, rank 37 of 40 is still 0, the maximum 4
    g, o = np.zeros((3, 9, 22), np.int32), np.zeros((3, 9, 22), np.int32)
    g[1, 2, 1:21] = 1
    o[1, 2, 1:20] = 1
    o[1, 6, 20] = 1
    r = SC.surface_distances(g, o)
    assert (r["n_gt"], r["n_out"], r["HD"], r["HD95"]) == (20, 20, 4.0, 0.0)
    assert r["mean_gt_to_out"] == 1.0 / 20 and r["mean_out_to_gt"] == 4.0 / 20 and r["ASSD"] == 5.0 / 40
    assert list(r) == list(SC.SURFACE_KEYS)


def test_empty_rules():
    z, g = np.zeros((4, 5, 6), np.int32), np.zeros((4, 5, 6), np.int32)
    g[1:3, 1:3, 1:3] = 3
    both = SC.surface_distances(z, z)
    assert both == {"HD": 0.0, "HD95": 0.0, "ASSD": 0.0, "n_gt": 0, "n_out": 0, "mean_gt_to_out": 0.0, "mean_out_to_gt": 0.0}
    for a, b in ((g, z), (z, g)):
        r = SC.surface_distances(a, b)
        assert all(r[k] == np.inf for k in ("HD", "HD95", "ASSD", "mean_gt_to_out", "mean_out_to_gt")) and r["n_gt"] + r["n_out"] == 8
    assert SC.surface_distances(g, g, klass=2)["HD"] == 0.0 and SC.surface_distances(g, g, klass=2)["n_gt"] == 0      # no voxel of class 2
    # the formulas say inf themselves: the field to an empty set is +inf everywhere
    assert np.all(np.isposinf(SC.gather(SC.edt2(SC.surface_mask(z)), SC.surface_mask(g))))
    with pytest.raises(ValueError):
        SC.surface_distances(g, z[:3])
    with pytest.raises(ValueError):
        SC.edt2(g != 0, (1, 0, 1))


def test_accuracy_modes_on_arrays():
    rng = np.random.default_rng(4)
    g = (rng.random((9, 8, 12)) < 0.4).astype(np.int32) * 2
    o = (rng.random((9, 8, 12)) < 0.4).astype(np.int32)
    sp = (0.7, 0.7, 2.5)
    d = SC.surface_distances(g, o, sp)
    s = SC.Accuracy(g, o, spacing=sp, mode=["SURFACE"])
    assert list(s) == ["HD", "HD95", "ASSD"] and s == {k: d[k] for k in s} and 0 < s["HD95"] <= s["HD"] and s["ASSD"] <= s["HD"]
    a = SC.Accuracy(g, o, spacing=sp, mode=["DICE", "ITEM", "SURFACE"])
    assert list(a) == ["DICE", "Jaccard"] + BE.ITEM_COLUMNS + BE.SURFACE_COLUMNS
    assert {k: a[k] for k in s} == s and {k: v for k, v in a.items() if k not in s} == SC.Accuracy(g, o, spacing=sp, mode=["DICE", "ITEM"])
    assert SC.Accuracy(g, o, spacing=sp, mode=["DICE"]) == SC.Accuracy(g, o, spacing=sp)                   # the default is unchanged
    # the caller's half: the ground truth's surface and field
    field = SC.surface_field(g, sp)
    assert np.array_equal(field[0], SC.surface_mask(g)) and np.array_equal(field[1], SC.edt2(field[0], sp))
    assert SC.Accuracy(g, o, spacing=sp, mode=["SURFACE"], gt_field=field) == s
    # HD against scipy's transform, the long way round
    sg, so = SC.surface_mask(g), SC.surface_mask(o)
    far = max(ndimage.distance_transform_edt(~so, sampling=sp)[sg].max(), ndimage.distance_transform_edt(~sg, sampling=sp)[so].max())
    assert np.isclose(s["HD"], far, rtol=1e-14, atol=0.0)


# ---- Batch_Evaluate around the stand-in model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [["SURFACE"], ["DICE", "ITEM", "SURFACE"]])
@pytest.mark.parametrize("cache_fields", [True, False])
def test_batch_evaluate_surface_around_a_stand_in_model(tmp_path, monkeypatch, mode, cache_fields):
    ck, dat, out = _sweep_folders(tmp_path)
    np.save(str(dat / "case_b" / "label.npy"), np.zeros((10, 9, 12), np.int16))               # one empty truth: its rows are inf
    be = BE.Batch_Evaluate(config_json=CFG, model_folder=str(ck), output_folder=str(out), data_folder=str(dat),
                           ground_truth_filename="label.npy", stride_layer_min=4, stride_layer_max=4, stride_inplane_min=8,
                           stride_inplane_max=10, patch_size=None, patch_layer=None, step=2, checkpoint_min=10, checkpoint_max=20,
                           batch_size=3, mode=mode, tolerance=2, cache_fields=cache_fields)
    models, fields = [], []
    monkeypatch.setattr(BE.Batch_Evaluate, "build_model", lambda self, cfg: models.append(StandIn(cfg)) or models[-1])
    real = SC.surface_field
    monkeypatch.setattr(SC, "surface_field", lambda *a, **k: fields.append(1) or real(*a, **k))
    be.Execute()
    m, = models
    assert len(fields) == (2 if cache_fields else 2 * 4)                  # once per case, or once per case and combination
    cols = ["Case"] + (["DICE", "Jaccard"] + BE.ITEM_COLUMNS if "DICE" in mode else []) + ["HD", "HD95", "ASSD"]
    assert BE.columns(mode) == cols and BE.SURFACE_COLUMNS == ["HD", "HD95", "ASSD"]
    for s in (10, 20):
        for a in (8, 10):
            with open(str(out / ("result_checkpoint-%d_stride_inplane-%d_stride_layer-4.csv" % (s, a))), newline="") as f:
                rd = csv.DictReader(f, delimiter=",", quotechar="|", quoting=csv.QUOTE_MINIMAL)
                rows = list(rd)
            assert rd.fieldnames == cols and [r["Case"] for r in rows] == ["case_a", "case_b", "average"]
            want = []
            for c in ("case_a", "case_b"):
                img = np.load(str(dat / c / "image.npy"))[..., None]
                gt = data.remap_labels(np.load(str(dat / c / "label.npy")), [0, 2])
                want.append(SC.Accuracy(gt, m.label_of(img, s, [a, a, 4]).astype(np.int32), tolerence=2, mode=mode))
            for r, w in zip(rows, want):
                assert {k: float(v) for k, v in r.items() if k != "Case"} == {k: float(v) for k, v in w.items()}
            assert 0 <= float(rows[0]["HD95"]) <= float(rows[0]["HD"]) < np.inf and float(rows[0]["HD"]) > 0
            for k in ("HD", "HD95", "ASSD"):
                assert float(rows[1][k]) == np.inf and float(rows[2][k]) == np.inf             # np.mean, as for every column
            for k in cols[1:-3]:
                assert float(rows[2][k]) == float(np.mean([w[k] for w in want])), k


def test_get_args_and_the_constructor_take_surface(tmp_path):
    a = BE.get_args(["-cd", str(tmp_path), "-d", str(tmp_path), "-o", str(tmp_path), "--mode", "SURFACE"])
    assert a.mode == ["SURFACE"]
    a = BE.get_args(["-cd", str(tmp_path), "-d", str(tmp_path), "-o", str(tmp_path), "--mode", "DICE", "ITEM", "SURFACE"])
    assert a.mode == ["DICE", "ITEM", "SURFACE"]
    with pytest.raises(SystemExit):
        BE.get_args(["-cd", str(tmp_path), "-d", str(tmp_path), "-o", str(tmp_path), "--mode", "HAUSDORFF"])
    assert BE.Batch_Evaluate(mode=["SURFACE"]).cache_fields is True and BE.Batch_Evaluate(cache_fields=False).cache_fields is False
    with pytest.raises(AssertionError):
        BE.Batch_Evaluate(mode=["HAUSDORFF"])
    assert BE.columns(["DICE"]) == ["Case", "DICE", "Jaccard"] and BE.columns(["ITEM"]) == ["Case"] + BE.ITEM_COLUMNS


# ---- csrc/vnet_surface.h: what its row of tests/test_abi_ledger.py does not say --------------------------------------------------------
def test_surface_lives_in_the_one_library():
    assert surface.HEADER in [h for h, _ in _lib.HEADERS] and surface.lib is _lib.lib and not hasattr(surface, "LIB_PATH")
    names = set(guard.header_functions(os.path.join(ROOT, surface.HEADER)))
    assert len(names) == 9 and names <= set(_lib.all_signatures())
    main = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in names if not hasattr(main, n)]
    assert not surface.HEADER.startswith("include/") and not os.path.exists(os.path.join(ROOT, "include", "vnet_surface.h"))
    mk = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "Makefile")).read()
    assert "libvnet_surface" not in mk and "SURF_" not in mk
    head = open(os.path.join(ROOT, surface.HEADER)).read()
    assert "#define VNET_SURFACE_MAX_AXIS %d" % surface.MAX_AXIS in head and "#define VNET_SURFACE_MAX_RANKS %d" % surface.MAX_RANKS in head
    assert surface.MAX_AXIS >= 2048
    src = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "surface.hip")).read()
    assert "#pragma clang fp contract(off)" in src


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1), VNET_E_UNSUPPORTED (-2), VNET_E_WORKSPACE (-3) before any launch, in that order."""
    L = _lib.lib()
    one, odd, big = ctypes.c_void_p(16), ctypes.c_void_p(20), 1 << 40
    assert L.vnet_surface_bits(None, 0, one, 5, 4, 3, None) == -1 and L.vnet_surface_bits(one, -1, one, 5, 4, 3, None) == -1
    assert L.vnet_surface_bits(one, 0, odd, 5, 4, 3, None) == -1 and L.vnet_surface_bits(one, 0, one, 0, 4, 3, None) == -1
    assert L.vnet_surface_bits(one, 0, one, 2049, 1, 1, None) == -2 and L.vnet_surface_bits(one, 0, one, 2048, 2048, 512, None) == -2
    assert L.vnet_surface_bits(None, 0, one, 2049, 1, 1, None) == -1                                       # BADARG comes first
    assert L.vnet_edt2_ws_bytes(5, 4, 3) == 4 * 60 + 8 * 60 and L.vnet_edt2_ws_bytes(3, 3, 3) == 112 + 8 * 27
    assert L.vnet_edt2_ws_bytes(0, 4, 3) == 0 and L.vnet_edt2_ws_bytes(1, 2049, 1) == 0
    ok = [one, one, 1.0, 1.0, 1.0, 5, 4, 3, one, 720, None]
    for pos, v in ((0, None), (1, None), (8, None), (8, odd), (2, 0.0), (3, -1.0), (4, float("inf")), (4, float("nan")), (5, 0)):
        bad = list(ok)
        bad[pos] = v
        assert L.vnet_edt2(*bad) == -1, pos
    assert L.vnet_edt2(*(ok[:5] + [1, 1, 2049] + ok[8:])) == -2
    assert L.vnet_edt2(*(ok[:9] + [719, None])) == -3
    assert L.vnet_edt2(*(ok[:5] + [1, 1, 2049, one, 0, None])) == -2                                          # UNSUPPORTED before WORKSPACE
    need = L.vnet_surface_gather_ws_bytes(5, 4, 3)
    assert 0 < need <= 1 << 16 and L.vnet_surface_gather_ws_bytes(5, 4, 0) == 0
    ok = [one, one, one, one, 7, 5, 4, 3, one, need, None]
    for pos, v in ((0, None), (1, None), (2, None), (3, None), (4, -1), (8, None), (3, odd)):
        bad = list(ok)
        bad[pos] = v
        assert L.vnet_surface_gather(*bad) == -1, pos
    assert L.vnet_surface_gather(*(ok[:4] + [2 ** 31] + ok[5:])) == -2 and L.vnet_surface_gather(*(ok[:9] + [need - 1, None])) == -3
    assert L.vnet_list_select_ws_bytes(1000, 2) == 64 + 4 * 4 * 8 and L.vnet_list_select_ws_bytes(0, 1) == 0
    assert L.vnet_list_select_ws_bytes(10, 5) == 0 and L.vnet_list_select_ws_bytes(2 ** 31, 1) == 0
    ranks = (ctypes.c_longlong * 2)(0, 9)
    ok = [one, 10, ranks, 2, one, one, 1 << 20, None]
    for pos, v in ((0, None), (1, 0), (2, None), (3, 0), (3, 5), (4, None), (5, None), (1, 9)):                # (n = 9: rank 9 is outside)
        bad = list(ok)
        bad[pos] = v
        assert L.vnet_list_select(*bad) == -1, pos
    assert L.vnet_list_select(one, 2 ** 31, ranks, 2, one, one, big, None) == -2 and L.vnet_list_select(*(ok[:6] + [8, None])) == -3
    assert L.vnet_list_root_sum_ws_bytes(1000) == 4 * 8 and L.vnet_list_root_sum_ws_bytes(0) == 0
    assert L.vnet_list_root_sum(None, 10, one, one, 64, None) == -1 and L.vnet_list_root_sum(one, 0, one, one, 64, None) == -1
    assert L.vnet_list_root_sum(one, 2 ** 31, one, one, big, None) == -2 and L.vnet_list_root_sum(one, 10, one, one, 7, None) == -3


def test_ops_refuse_cpu_tensors():
    E = surface.VnetHipError
    lab, bits = torch.zeros((5, 4, 3), dtype=torch.int32), torch.zeros((5, 4, 1), dtype=torch.int64)
    d2, lst = torch.zeros((5, 4, 3), dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
    for what, call in (("surface_bits", lambda: surface.surface_bits(lab)), ("edt2", lambda: surface.edt2(bits, 3)),
                       ("gather", lambda: surface.gather(d2, bits, 3)), ("popcounts", lambda: surface.popcounts([bits], 3)),
                       ("kth", lambda: surface.kth(lst, [0])), ("root_sum", lambda: surface.root_sum(lst))):
        with pytest.raises(E, match=what + ".*no CPU path"):
            call()
    with pytest.raises(E):
        surface.surface_bits(lab.numpy())
    # a label map that is a CPU tensor takes the rules, like an array
    assert SC.surface_distances(lab, lab)["n_gt"] == 0
