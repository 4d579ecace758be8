"""-m gpu: the kernels of csrc/vnet_surface.h through the ops of vnet_tensorflow_amd/surface.py against the NumPy
rules of vnet_tensorflow_amd/score.py.  Every comparison is `==` (np.array_equal, +inf included) but the sums of roots, which are held
to the derived bound (n + 2) 2^-52 relative: at most 1 ulp (2^-52) per root on either side, (n - 1) 2^-53 per summation order."""
import csv
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import guard
from tests.test_score_host import CFG, StandIn, _sweep_folders
from vnet_tensorflow_amd import batch_evaluate as BE, data, score as SC, surface

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (1, 1, 70), (5, 1, 1), (3, 4, 65), (9, 10, 131), (17, 9, 130), (33, 40, 64)]
SPACINGS = [(1.0, 1.0, 1.0), (0.7, 0.7, 2.5), (3.0, 0.5, 1.0)]
CORNERS = ["corner%d%d%d" % (a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
KINDS = ["empty", "full"] + CORNERS + ["plane", "blobs", "noise"]
U = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _mask(shape, kind):
    m = np.zeros(shape, bool)
    if kind == "full":
        m[:] = True
    elif kind.startswith("corner"):
        m[tuple((n - 1) * int(c) for n, c in zip(shape, kind[-3:]))] = True
    elif kind == "plane":
        m[:, shape[1] // 2, :] = True
    elif kind == "blobs":
        m[:max(1, shape[0] // 4), :max(1, shape[1] // 4), :max(1, shape[2] // 8)] = True
        m[shape[0] - max(1, shape[0] // 5):, shape[1] - max(1, shape[1] // 3):, shape[2] - max(1, shape[2] // 6):] = True
    elif kind == "noise":
        m = np.random.default_rng(sum(shape)).random(shape) < 0.3
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _field(shape, kind, spacing):
    f = SC.edt2(_mask(shape, kind), spacing)
    f.setflags(write=False)
    return f


def _dev(a, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)


def _bits(mask, dev):
    return _dev(SC.pack(mask), dev, torch.int64)


def _cap(name):
    src = open(os.path.join(guard.ROOT, "vnet_tensorflow_amd", "csrc", "surface.hip")).read()
    pb = int(re.search(r"constexpr int PB = (\d+)", src).group(1))
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)), pb


# ---- surface ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_surface_bits(dev, shape):
    rng = np.random.default_rng(5)
    for kind in KINDS:
        m = _mask(shape, kind)
        label = np.where(m, 2, np.where(rng.random(shape) < 0.2, rng.integers(1, 4, shape), 0)).astype(np.int32)
        t = _dev(label, dev, torch.int32)
        for klass in (0, 2):
            got = surface.surface_bits(t, klass).cpu().numpy()
            assert got.dtype == np.int64 and np.array_equal(got, SC.pack(SC.surface_mask(label, klass))), (kind, klass)
    solid = np.zeros(shape, np.int32)                              # a solid block: an interior that is NOT surface, where the shape has one
    solid[:, :, :] = 3
    assert np.array_equal(surface.surface_bits(_dev(solid, dev, torch.int32), 3).cpu().numpy(), SC.pack(SC.surface_mask(solid, 3)))


# ---- distance field ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_edt2_every_voxel(dev, shape):
    for kind in KINDS:
        bits = _bits(_mask(shape, kind), dev)
        for sp in SPACINGS:
            got = surface.edt2(bits, shape[2], sp).cpu().numpy()
            want = _field(shape, kind, sp)
            assert got.dtype == np.float64 and got.shape == shape and np.array_equal(got, want), (kind, sp)
            if kind == "empty":
                assert np.all(np.isposinf(got))
            if kind.startswith("corner"):                          # the far corner found the one set voxel across every axis
                far = tuple((n - 1) * (1 - int(c)) for n, c in zip(shape, kind[-3:]))
                s2 = np.asarray(sp) ** 2
                assert got[far] == s2[0] * (shape[0] - 1) ** 2 + (s2[1] * (shape[1] - 1) ** 2 + s2[2] * (shape[2] - 1) ** 2)


def test_edt2_against_the_brute_force_definition(dev):
    shape = (5, 6, 70)
    m = np.random.default_rng(1).random(shape) < 0.01
    m[4, 5, 69] = True
    for sp in SPACINGS:
        assert np.array_equal(surface.edt2(_bits(m, dev), 70, sp).cpu().numpy(), SC.edt2_brute(m, sp))


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gather_order_count_and_capacity(dev, shape):
    d2 = np.random.default_rng(2).random(shape) + 1.0
    t = _dev(d2, dev, torch.float64)
    for kind in ("empty", "full", "corner111", "blobs", "noise"):
        m = _mask(shape, kind)
        bits, want = _bits(m, dev), SC.gather(d2, m)
        assert surface.popcounts([bits, bits], shape[2]) == [len(want)] * 2
        got, n = surface.gather(t, bits, shape[2])
        assert int(n) == len(want) and np.array_equal(got.cpu().numpy(), want), kind
        # a capacity below n drops the values past it and still reports the true count; one above n is zeroed from n up
        for cap in (max(0, len(want) - 3), len(want) + 5):
            out = torch.full((cap + 2,), -1.0, dtype=torch.float64, device=dev)
            back, n = surface.gather(t, bits, shape[2], out=out, offset=2)
            assert back is out and int(n) == len(want)
            assert np.array_equal(out.cpu().numpy(), np.concatenate([[-1.0, -1.0], want[:cap], np.zeros(max(0, cap - len(want)))])), (kind, cap)


# ---- the lists --------------------------------------------------------------------------------------------------------------------------
def _lists():
    rng = np.random.default_rng(3)
    yield "one", np.array([2.5])
    yield "zero", np.zeros(7)
    yield "ties", rng.integers(0, 6, 300).astype(np.float64)
    v = rng.random(1000) * 1e-300
    v[::7] = np.inf
    yield "inf and tiny", v
    yield "all inf", np.full(65, np.inf)
    yield "squares", (rng.integers(0, 2000, 70001).astype(np.float64) ** 2) * 0.49
    yield "subnormal", np.array([5e-324, 0.0, 1e-310, 5e-324, 2.0])


def test_kth(dev):
    for name, v in _lists():
        n = len(v)
        ranks = [0, n - 1, SC.hd95_rank(n)]
        got = surface.kth(_dev(v, dev, torch.float64), ranks).cpu().numpy()
        assert np.array_equal(got, SC.kth(v, ranks)), name
        mid = surface.kth(_dev(v, dev, torch.float64), [n // 2, n // 3, n // 5, 0]).cpu().numpy()
        assert np.array_equal(mid, SC.kth(v, [n // 2, n // 3, n // 5, 0])), name
    with pytest.raises(ValueError):
        surface.kth(_dev(np.ones(4), dev, torch.float64), [4])
    with pytest.raises(ValueError):
        surface.kth(_dev(np.ones(4), dev, torch.float64), [0] * 5)


def _root_sum_ok(v, dev):
    t = _dev(v, dev, torch.float64)
    runs = [surface.root_sum(t).cpu().numpy() for _ in range(3)]
    assert runs[0].shape == (1,) and runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()       # the same bits, launch after launch
    want = np.sqrt(v).sum()
    if np.isinf(want):
        assert runs[0][0] == np.inf
    else:
        assert abs(runs[0][0] - want) <= (len(v) + 2) * U * want, (runs[0][0], want)


def test_root_sum(dev):
    for name, v in _lists():
        _root_sum_ok(v, dev)
    with pytest.raises(ValueError):
        surface.root_sum(torch.zeros(0, dtype=torch.float64, device=dev))


# ---- past every grid cap ----------------------------------------------------------------------------------------------------------------
def test_word_kernels_past_their_grid_cap(dev):
    """vnet_surface_bits and the z pass of vnet_edt2 take one word per wave, BITS_CAP blocks of PB / 64 waves: more words than that."""
    cap, pb = _cap("BITS_CAP")
    shape = (129, 128, 1)
    assert shape[0] * shape[1] > cap * (pb // 64) >= 128 * 128
    label = (np.random.default_rng(7).random(shape) < 0.6).astype(np.int32)
    got = surface.surface_bits(_dev(label, dev, torch.int32))
    assert np.array_equal(got.cpu().numpy(), SC.pack(SC.surface_mask(label)))
    m = np.random.default_rng(8).random(shape) < 0.002
    assert np.array_equal(surface.edt2(_bits(m, dev), 1, (0.7, 0.7, 2.5)).cpu().numpy(), SC.edt2(m, (0.7, 0.7, 2.5)))


def test_axis_passes_past_their_grid_cap(dev):
    """The y and x passes take one voxel per thread, EDT_CAP blocks of PB threads."""
    cap, pb = _cap("EDT_CAP")
    shape = (129, 64, 64)
    assert shape[0] * shape[1] * shape[2] > cap * pb >= 128 * 64 * 64
    m = np.random.default_rng(9).random(shape) < 0.0005
    assert np.array_equal(surface.edt2(_bits(m, dev), 64, (3.0, 0.5, 1.0)).cpu().numpy(), SC.edt2(m, (3.0, 0.5, 1.0)))


def test_gather_past_its_grid_cap(dev):
    """The compaction takes GATHER_CAP chunks of words, one block each: more than PB words per chunk, so a block walks several tiles."""
    cap, pb = _cap("GATHER_CAP")
    shape = (513, 512, 1)
    assert shape[0] * shape[1] > cap * pb >= 512 * 512
    m = np.random.default_rng(10).random(shape) < 0.3
    d2 = np.arange(m.size, dtype=np.float64).reshape(shape)
    got, n = surface.gather(_dev(d2, dev, torch.float64), _bits(m, dev), 1)
    assert int(n) == int(m.sum()) and np.array_equal(got.cpu().numpy(), SC.gather(d2, m))


def test_list_kernels_past_their_grid_cap(dev):
    cap, pb = _cap("LIST_CAP")
    n = cap * pb + 77
    rng = np.random.default_rng(11)
    v = (rng.integers(0, 5000, n).astype(np.float64)) * 0.25
    v[rng.integers(0, n, 50)] = np.inf
    ranks = [0, n - 1, SC.hd95_rank(n), n // 2]
    assert np.array_equal(surface.kth(_dev(v, dev, torch.float64), ranks).cpu().numpy(), SC.kth(v, ranks))
    _root_sum_ok(np.where(np.isinf(v), 1.0, v), dev)
    # the zeroing of a gathered list's tail walks the same cap
    shape = (2, 2, 3)
    m = _mask(shape, "full")
    out = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    surface.gather(_dev(np.ones(shape), dev, torch.float64), _bits(m, dev), 3, out=out)
    assert np.array_equal(out.cpu().numpy(), np.concatenate([np.ones(12), np.zeros(n - 12)]))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _same_scores(got, want):
    assert list(got) == list(want) == list(SC.SURFACE_KEYS)
    for k in ("HD", "HD95", "n_gt", "n_out"):
        assert got[k] == want[k], (k, got, want)
    n = want["n_gt"] + want["n_out"]
    for k in ("ASSD", "mean_gt_to_out", "mean_out_to_gt"):
        assert got[k] == want[k] or abs(got[k] - want[k]) <= (n + 2) * U * want[k], (k, got, want)


@pytest.mark.parametrize("shape", [(3, 4, 65), (17, 9, 130), (33, 40, 64)], ids=str)
def test_surface_distances_on_the_device_are_those_of_the_arrays(dev, shape):
    rng = np.random.default_rng(12)
    g = np.where(_mask(shape, "blobs"), 2, 0).astype(np.int32)
    g[rng.random(shape) < 0.02] = 1
    o = np.roll(g, 1, axis=0)
    o[rng.random(shape) < 0.02] = 2
    zero = np.zeros(shape, np.int32)
    for sp in SPACINGS:
        for klass in (0, 2):
            tg, to = _dev(g, dev, torch.int32), _dev(o, dev, torch.int32)
            want = SC.surface_distances(g, o, sp, klass)
            assert want["n_gt"] > 0 and want["n_out"] > 0 and want["HD"] > 0
            _same_scores(SC.surface_distances(tg, to, sp, klass), want)
            field = SC.surface_field(tg, sp, klass)
            assert np.array_equal(field[0].cpu().numpy(), SC.pack(SC.surface_mask(g, klass)))
            _same_scores(SC.surface_distances(tg, to, sp, klass, gt_field=field), want)
    for a, b in ((g, zero), (zero, g), (zero, zero)):
        got = SC.surface_distances(_dev(a, dev, torch.int32), _dev(b, dev, torch.int32), SPACINGS[1])
        assert got == SC.surface_distances(a, b, SPACINGS[1])
    # the kernels need no special case for one empty side: the field to an empty set is +inf, and so is every score drawn from it
    inf = surface.edt2(surface.surface_bits(_dev(zero, dev, torch.int32)), shape[2], SPACINGS[1])
    lst, n = surface.gather(inf, surface.surface_bits(_dev(g, dev, torch.int32)), shape[2])
    assert int(n) == lst.numel() > 0 and surface.kth(lst, [0]).item() == np.inf and surface.root_sum(lst).item() == np.inf
    a = SC.Accuracy(_dev(g, dev, torch.int32), _dev(o, dev, torch.int32), spacing=SPACINGS[1], mode=["DICE", "SURFACE"])
    w = SC.Accuracy(g, o, spacing=SPACINGS[1], mode=["DICE", "SURFACE"])
    assert list(a) == list(w) == ["DICE", "Jaccard", "HD", "HD95", "ASSD"] and all(a[k] == w[k] for k in ("DICE", "Jaccard", "HD", "HD95"))


class DeviceStandIn(StandIn):
    """tests/test_score_host.py's stand-in model on the device: the hook gets an int32 device tensor, as from evaluate_single_3D."""

    def __init__(self, cfg, dev):
        StandIn.__init__(self, cfg)
        self.device = dev

    def evaluate_case(self, image, spacing, tf, regrid, on_label=None):
        self.calls.append((self.step, tuple(self.evaluate_stride), self.evaluate_batch))
        label = self.label_of(image, self.step, self.evaluate_stride)
        on_label(torch.from_numpy(label.astype(np.int32)).to(self.device))
        return label, None


@pytest.mark.parametrize("cache_fields", [True, False])
def test_batch_evaluate_mode_surface_end_to_end(dev, tmp_path, monkeypatch, cache_fields):
    """The command line with --mode SURFACE around the stand-in model on the device: every CSV holds what the rules give on arrays."""
    ck, dat, out = _sweep_folders(tmp_path)
    out.mkdir()
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(CFG))
    args = BE.get_args(["-cd", str(ck), "-d", str(dat), "-o", str(out), "-c", str(cfg), "-cmin", "10", "-cmax", "20", "-slmin", "4", "-slmax", "4",
                        "-spmin", "8", "-spmax", "10", "-gt", "label.npy", "--mode", "DICE", "SURFACE", "--gpu", str(dev.index or 0)])
    models = []
    monkeypatch.setattr(BE.Batch_Evaluate, "build_model", lambda self, cfg: models.append(DeviceStandIn(cfg, dev)) or models[-1])
    if not cache_fields:
        real = BE.Batch_Evaluate.__init__
        monkeypatch.setattr(BE.Batch_Evaluate, "__init__", lambda self, **kw: real(self, cache_fields=False, **kw))
    calls = []
    real_field = SC.surface_field
    monkeypatch.setattr(SC, "surface_field", lambda *a, **k: calls.append(1) or real_field(*a, **k))
    BE.main(args)
    m, = models
    assert len(calls) == (2 if cache_fields else 0)               # (without the cache the device path builds the two halves itself)
    for s in (10, 20):
        for a in (8, 10):
            with open(str(out / ("result_checkpoint-%d_stride_inplane-%d_stride_layer-4.csv" % (s, a))), newline="") as f:
                rd = csv.DictReader(f, delimiter=",", quotechar="|", quoting=csv.QUOTE_MINIMAL)
                rows = list(rd)
            assert rd.fieldnames == ["Case", "DICE", "Jaccard", "HD", "HD95", "ASSD"]
            assert [r["Case"] for r in rows] == ["case_a", "case_b", "average"]
            got = []
            for c, r in zip(("case_a", "case_b"), rows):
                img = np.load(str(dat / c / "image.npy"))[..., None]
                gt = data.remap_labels(np.load(str(dat / c / "label.npy")), [0, 2])
                label = m.label_of(img, s, [a, a, 4]).astype(np.int32)
                sp = data.volume_spacing(str(dat / c / "label.npy"))
                w = SC.Accuracy(gt, label, spacing=sp, mode=["DICE", "SURFACE"])
                d = SC.surface_distances(gt, label, sp)
                assert all(float(r[k]) == w[k] for k in ("DICE", "Jaccard", "HD", "HD95")) and w["HD"] > 0
                assert abs(float(r["ASSD"]) - w["ASSD"]) <= (d["n_gt"] + d["n_out"] + 2) * U * w["ASSD"]
                got.append({k: float(r[k]) for k in rd.fieldnames[1:]})
            for k in rd.fieldnames[1:]:
                assert float(rows[2][k]) == float(np.mean([g[k] for g in got])), k
