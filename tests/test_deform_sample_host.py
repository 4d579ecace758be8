"""A training sample cut from a resident case through BSplineDeformation, the parts that need no GPU: plan_deformed_tail and its draw
against the NumPy transforms on the same generator, the windowed restatement (sample.deform_patch) against deforming the whole volume
and cropping, VolumeDataset(device_tail=...) on such a tail through CPU stand-ins of the device entry points, the error codes of
vnet_deform_sample_patch before any launch, the op up to the first launch, and the ledger of include/vnet_hip_deform_sample.h."""
import contextlib
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

from tests import guard
from vnet_tensorflow_amd import deform as D
from vnet_tensorflow_amd import sample as S
from vnet_tensorflow_amd import transforms as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "vnet_hip_deform_sample.h")
SHAPE, SPACING = (21, 18, 23), (1.0, 0.8, 1.25)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def test_plan_deformed_tail():
    bs, crop2, crop, flip, noise = T.BSplineDeformation(4), T.ConfidenceCrop2(8, 3, 0.8), T.RandomCrop(8), T.RandomFlip([True]), T.RandomNoise()
    p = T.plan_deformed_tail([bs, crop2, noise])
    assert isinstance(p, T.DeformedTailPlan) and p.deform is bs and p.crop is crop2 and p.flip is None and p.noise is noise
    p = T.plan_deformed_tail([bs, crop2])
    assert p.deform is bs and p.crop is crop2 and p.flip is None and p.noise is None
    p = T.plan_deformed_tail([bs, crop, flip, noise])
    assert p.deform is bs and p.crop is crop and p.flip is flip and p.noise is noise
    p = T.plan_deformed_tail([bs, crop, flip])
    assert p.crop is crop and p.flip is flip and p.noise is None
    for bad in ([], [bs], [crop2, noise], [crop, flip], [crop2, bs], [crop2, bs, noise], [bs, bs, crop2], [bs, crop2, noise, T.Padding(8)],
                [bs, T.Padding(8), crop2], [bs, noise, crop2], [bs, crop2, noise, flip], [bs, crop2, crop]):
        assert T.plan_deformed_tail(bad) is None, bad
    # the first planner keeps refusing the deformation; behind the deterministic prefix the second one takes it
    full = [T.ManualNormalization(0, 255), T.Padding(8), bs, crop2, noise]
    n = T.deterministic_prefix(full)
    assert n == 2 and T.plan_tail(full[n:]) is None and T.plan_deformed_tail(full[n:]).deform is bs


def _blob(shape=SHAPE):
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    lab = (sum((a - 0.55 * s) ** 2 for a, s in zip(g, shape)) <= (min(shape) / 3.5) ** 2).astype(np.int32)
    lab[1:3, 1:3, 1:4] = 1
    return lab


@pytest.mark.parametrize("crop", ["confidence", "random"])
def test_draw_follows_the_transforms(crop):
    """40 seeds: BSplineDeformation, the crop and the flip as NumPy transforms on one generator against DeformedTailPlan.draw on another of
    the same seed, the crop's questions answered for the label deformed by the coefficients draw hands out: the same coefficients, the
    same window and flip (the samples are equal), and the same generator state afterwards (the noise seed is what the transforms' generator
    gives next)."""
    rng0 = np.random.default_rng(2)
    image = rng0.normal(100.0, 30.0, SHAPE + (2,)).astype(np.float32)
    label = _blob()
    bs = T.BSplineDeformation(4)
    first = T.ConfidenceCrop2([8, 6, 10], rand_range=3, probability=0.5) if crop == "confidence" else T.RandomCrop([8, 6, 10], 0.3, 20)
    flip = T.RandomFlip([True, False, True])
    plan = T.plan_deformed_tail([bs, first, flip, T.RandomNoise(3)])
    masks, starts = set(), set()
    for seed in range(40):
        a = np.random.default_rng(seed)
        ref = flip(first(bs({'image': image, 'label': label, 'spacing': SPACING}, a), a), a)
        seen = {}

        def deformed(coef):
            seen["coef"] = coef
            lab = seen["label"] = D.label(label, coef, SPACING)
            return (lambda: S.component_table(lab)), (lambda s, n, lo, hi: S.window_count(lab, s, n, lo, hi))
        b = np.random.default_rng(seed)
        coef, start, mask, sigma, nseed = plan.draw(SHAPE, b, deformed)
        assert coef is seen["coef"] and np.array_equal(coef, np.random.default_rng(seed).random(D.PARAMS) * 4)
        img, lab = S.patch(D.linear(image, coef, SPACING), seen["label"], start, first.output_size, mask)
        assert np.array_equal(ref['image'], img) and np.array_equal(ref['label'], lab), (seed, start, mask)
        assert mask in (0, 5) and sigma == 3.0 and nseed == int(a.integers(0, 2 ** 64, dtype=np.uint64))
        assert a.bit_generator.state == b.bit_generator.state
        masks.add(mask)
        starts.add(tuple(start))
    assert masks == {0, 5} and len(starts) > 10


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def _case(shape, spacing, C, seed):
    rng = np.random.default_rng(100 + seed)
    image = rng.normal(20.0, 30.0, shape + (C,)).astype(np.float32)
    label = (rng.random(shape) < 0.5).astype(np.int32)
    return image, label, np.random.default_rng(seed).random(D.PARAMS) * 6.0


def _windows(shape, patch=(8, 6, 10)):
    far = tuple(n - p for n, p in zip(shape, patch))
    return [((0, 0, 0), patch), (far, patch), ((far[0], 0, 5), patch), ((3, far[1], 0), patch), ((0, 0, 0), shape),
            ((4, 5, 6), (1, 6, 10)), ((4, 5, 6), (8, 1, 1)), ((shape[0] - 1, shape[1] - 1, shape[2] - 1), (1, 1, 1))]


@pytest.mark.parametrize("shape,spacing,C", [((21, 18, 23), (1.0, 0.8, 1.25), 3), ((24, 20, 28), (1.0, 1.0, 1.0), 1)])
def test_windowed_restatement_is_deform_then_crop(shape, spacing, C):
    """sample.deform_patch evaluates the window's voxels alone; what it returns is == the window of the whole deformed volume: all 8 flips,
    the corners, the whole volume, windows one voxel wide, with and without noise.  It is not that composition: source_index is asked for
    the window only (the spy), and some voxels of a window take taps outside it or sample outside the volume."""
    image, label, coef = _case(shape, spacing, C, seed=3)
    whole_i, whole_l = D.linear(image, coef, spacing), D.label(label, coef, spacing)
    assert whole_i.dtype == np.float32 and (whole_i == 0).any() and (whole_l != label).any()
    asked, real = [], D.source_index

    def spy(shp, sp, cf, window=None):
        asked.append(window)
        return real(shp, sp, cf, window)
    D.source_index = spy
    try:
        for start, size in _windows(shape):
            for flip in range(8):
                gi, gl = S.deform_patch(image, label, coef, spacing, start, size, flip)
                ri, rl = S.patch(whole_i, whole_l, start, size, flip)
                assert gi.dtype == np.float32 and gl.dtype == label.dtype and gi.shape == tuple(size) + (C,)
                assert gi.tobytes() == ri.tobytes() and np.array_equal(gl, rl), (start, size, flip)
            gi, gl = S.deform_patch(image, label, coef, spacing, start, size, 6, 5.0, 0xABCDEF0123)
            ri, rl = S.patch(whole_i, whole_l, start, size, 6, 5.0, 0xABCDEF0123)
            assert gi.dtype == np.float64 and gi.tobytes() == ri.tobytes() and np.array_equal(gl, rl)
            assert not np.array_equal(gi, S.deform_patch(image, label, coef, spacing, start, size, 6)[0])
    finally:
        D.source_index = real
    assert asked and all(w is not None for w in asked) and {tuple(w[1]) for w in asked} == {tuple(s) for _, s in _windows(shape)}
    start, size = _windows(shape)[1]
    c = D.source_index(shape, spacing, coef, (start, size))
    assert c.shape == tuple(size) + (3,)
    sl = tuple(slice(s, s + n) for s, n in zip(start, size))
    assert np.array_equal(c, D.source_index(shape, spacing, coef)[sl])
    outside = np.zeros(size, bool)
    leaves = np.zeros(size, bool)
    for a, n in enumerate(shape):
        outside |= ~((c[..., a] >= -0.5) & (c[..., a] < n - 0.5))
        leaves |= (np.floor(c[..., a]) < start[a]) | (np.floor(c[..., a]) + 1 > start[a] + size[a] - 1)
    assert outside.any() and (leaves & ~outside).any() and not outside.all()
    with pytest.raises(ValueError, match="window"):
        S.deform_patch(image, label, coef, spacing, (shape[0] - 7, 0, 0), (8, 6, 10))
    with pytest.raises(ValueError, match="deform_patch"):
        S.deform_patch(image[..., 0], label, coef, spacing, (0, 0, 0), (8, 6, 10))


def test_issue_inputs_are_decidable():
    """The inputs the GPU tests use (tests/test_hip_deform_sample.py): no undecidable voxel at eps 1e-9, shifts of 5 to 6 voxels, a good part
    of the voxels sampling outside the volume."""
    for shape, spacing in (((21, 18, 23), (1.0, 0.8, 1.25)), ((24, 20, 28), (1.0, 1.0, 1.0))):
        for seed in range(12):
            coef = np.random.default_rng(seed).random(D.PARAMS) * 6.0
            assert not D.undecidable(shape, spacing, coef).any(), (shape, seed)
            c = D.source_index(shape, spacing, coef)
            grid = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"), axis=-1)
            assert 4.0 < np.abs(c - grid).max() < 8.0
            out = np.zeros(shape, bool)
            for a, n in enumerate(shape):
                out |= ~((c[..., a] >= -0.5) & (c[..., a] < n - 0.5))
            assert 0.2 < out.mean() < 0.7, (shape, seed, out.mean())


# ---- the dataset through CPU stand-ins -----------------------------------------------------------------------------------------------------
def _stand_ins(monkeypatch):
    """The device entry points the deformed tail uses, on CPU tensors through the restatements: the dataset's own logic (plan, cache,
    evictions, per-visit table, fall-backs, slots) without a device."""
    from vnet_tensorflow_amd import ops
    calls = {"deform_sample_patch": 0, "bspline_deform": 0, "component_table": 0}

    lock = threading.RLock()

    @contextlib.contextmanager
    def side_work(device):
        with lock:                          # (exclusive, like the real one: one loader thread at a time)
            yield None

    def component_table(label, max_components=4096, ws=None):
        calls["component_table"] += 1
        n, rows = S.component_table(label.numpy())
        return n, rows[:max_components]

    def bspline_deform(x, coef, spacing, kind="image"):
        assert kind == "label" and x.dtype == torch.int32 and coef.dtype == torch.float64
        calls["bspline_deform"] += 1
        return torch.from_numpy(D.label(x.numpy(), coef.numpy(), spacing))

    def deform_sample_patch(image, deformed_label, coef, spacing, start, patch, flip, sigma, seed, out_image, out_label):
        calls["deform_sample_patch"] += 1
        img = D.linear64(image.numpy(), coef.numpy(), spacing, (start, patch)).astype(np.float32)
        lab = S.patch(image.numpy(), deformed_label.numpy(), start, patch, flip)[1]
        img = np.ascontiguousarray(np.flip(img, S.flip_axes(flip)))
        assert not sigma
        out_image.copy_(torch.from_numpy(img))
        out_label.copy_(torch.from_numpy(lab.reshape(tuple(out_label.shape)).copy()))
    monkeypatch.setattr(ops, "side_work", side_work)
    monkeypatch.setattr(ops, "pinned_staging", lambda name, shape, dtype: torch.empty(tuple(shape), dtype=dtype))
    monkeypatch.setattr(ops, "component_table", component_table)
    monkeypatch.setattr(ops, "bspline_deform", bspline_deform)
    monkeypatch.setattr(ops, "window_count", lambda label, s, n, lo, hi: S.window_count(label.numpy(), s, n, lo, hi))
    monkeypatch.setattr(ops, "deform_sample_patch", deform_sample_patch)
    monkeypatch.setattr(ops._lib, "lib", lambda: type("L", (), {"vnet_cc_table_ws_bytes": staticmethod(lambda X, Y, Z: 8 * X * Y * Z + 16384)})())
    return calls


@pytest.mark.parametrize("crop", ["confidence", "random"])
def test_dataset_deformed_tail_is_the_numpy_dataset_through_stand_ins(monkeypatch, crop, capsys):
    """VolumeDataset(device_tail=...) on [ManualNormalization, BSplineDeformation, crop, RandomFlip] with the device entry points replaced
    by their restatements: the batches equal the NumPy dataset's bit for bit, with room for every case and with a budget of one case; the
    component table is built per visit, of the deformed label; and a Prefetcher hands the batches on as they are."""
    from vnet_tensorflow_amd import data
    calls = _stand_ins(monkeypatch)

    def make(**kw):
        first = T.ConfidenceCrop2([8, 8, 8], rand_range=3, probability=0.5) if crop == "confidence" else T.RandomCrop([8, 8, 8], 0.2, 30)
        tf = [T.ManualNormalization(0, 255), T.BSplineDeformation(4), first, T.RandomFlip([True, False, True])]
        return data.VolumeDataset("synthetic", ["a.npy", "b.npy"], "l.npy", [0, 1], (8, 8, 8), 2, train=True, seed=5,
                                  synthetic={"Cases": 6, "Shape": [20, 18, 22], "Spacing": list(SPACING)}, transforms=tf, **kw)
    case_bytes = 20 * 18 * 22 * 4 * 3
    for budget in (16 << 30, case_bytes * 3 // 2):
        host, on_dev = make(), make(device_tail="cpu", device_cache_bytes=budget)
        assert on_dev.device_tail == torch.device("cpu") and on_dev._tail_at == 1 and on_dev._deformed
        assert "loader path" not in capsys.readouterr().out
        before = dict(calls)
        for epoch in range(2):
            ref = list(host)
            got = list(data.Prefetcher(on_dev, depth=2, workers=2)) if epoch else list(on_dev)
            assert len(ref) == len(got) == 3
            for (ri, rl), (gi, gl) in zip(ref, got):
                assert isinstance(gi, torch.Tensor) and gi.dtype == torch.float32 and gl.dtype == torch.int32 and not gi.is_pinned()
                assert gi.numpy().tobytes() == ri.tobytes() and np.array_equal(gl.numpy(), rl)
        st = on_dev.device_stats
        assert calls["deform_sample_patch"] - before["deform_sample_patch"] == 12 == calls["bspline_deform"] - before["bspline_deform"]
        assert calls["component_table"] - before["component_table"] == (12 if crop == "confidence" else 0)      # per visit, never per upload
        assert all(e[2] is None and e[3] == SPACING for e in on_dev._dev_cache.values())
        if budget < 16 << 30:
            assert st["evictions"] >= 6 and len(on_dev._dev_cache) == 1 and st["host_samples"] == 0
        else:
            assert st["uploads"] == 6 and st["evictions"] == 0 and st["host_samples"] == 0
    # a budget below one case, a table capacity below the deformed label's components: the NumPy tail on a fresh generator, same batch
    for kw in ({"device_cache_bytes": 100}, {"max_components": 0}):
        host, on_dev = make(), make(device_tail="cpu", **kw)
        before = calls["deform_sample_patch"]
        (ri, rl), (gi, gl) = next(iter(host)), next(iter(on_dev))
        if crop == "confidence" or "device_cache_bytes" in kw:
            assert on_dev.device_stats["host_samples"] == 2 and calls["deform_sample_patch"] == before
            assert on_dev.device_stats["uploads"] == (0 if "device_cache_bytes" in kw else 2)
        else:
            assert on_dev.device_stats["host_samples"] == 0 and calls["deform_sample_patch"] == before + 2     # RandomCrop asks no table
        assert gi.numpy().tobytes() == ri.tobytes() and np.array_equal(gl.numpy(), rl)


def test_dataset_still_refuses_other_deformed_tails(capsys):
    from vnet_tensorflow_amd import data
    args = ("synthetic", ["a.npy"], "l.npy", [0, 1], (8, 8, 8), 1)
    syn = {"Cases": 2, "Shape": [12, 10, 9]}
    ds = data.VolumeDataset(*args, synthetic=syn, transforms=[T.BSplineDeformation(2.0), T.Padding(8), T.RandomCrop(8)], device_tail="cuda")
    assert ds.device_tail is None and not ds._deformed and "loader path" in capsys.readouterr().out
    with pytest.raises(ValueError, match="PatchShape"):
        data.VolumeDataset(*args, synthetic=syn, transforms=[T.BSplineDeformation(2.0), T.RandomCrop(6)], device_tail="cuda")


# ---- the op up to the first launch, error codes ---------------------------------------------------------------------------------------
def _op_args(device, C=2, **over):
    kw = dict(image=torch.zeros(5, 4, 3, C, device=device), deformed_label=torch.zeros(5, 4, 3, dtype=torch.int32, device=device),
              coef=torch.zeros(D.PARAMS, dtype=torch.float64, device=device), spacing=SPACING, start=(1, 1, 0), patch=(2, 2, 2), flip=3,
              sigma=0.0, seed=1, out_image=torch.zeros(2, 2, 2, C, device=device), out_label=torch.zeros(2, 2, 2, 1, dtype=torch.int32, device=device))
    kw.update(over)
    return kw


def test_op_meta_and_refuses_cpu_tensors():
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    assert ops.deform_sample_patch(**_op_args("meta")) is None
    assert ops.deform_sample_patch(**_op_args("meta", out_label=torch.zeros(2, 2, 2, dtype=torch.int32, device="meta"))) is None
    with pytest.raises(VnetHipError, match="deform_sample_patch"):
        ops.deform_sample_patch(**_op_args("cpu"))
    with pytest.raises(VnetHipError, match="meta"):
        ops.deform_sample_patch(**_op_args("meta", coef=torch.zeros(D.PARAMS, dtype=torch.float64)))
    with pytest.raises(VnetHipError, match="control grid"):
        ops.deform_sample_patch(**_op_args("meta", coef=torch.zeros(12, dtype=torch.float64, device="meta")))
    with pytest.raises(VnetHipError, match="outputs"):
        ops.deform_sample_patch(**_op_args("meta", out_image=torch.zeros(2, 2, 2, 3, device="meta")))
    with pytest.raises(VnetHipError, match="int32"):
        ops.deform_sample_patch(**_op_args("meta", deformed_label=torch.zeros(5, 4, 3, device="meta")))
    with pytest.raises(VnetHipError, match="does not go with"):
        ops.deform_sample_patch(**_op_args("meta", image=torch.zeros(5, 4, 4, 2, device="meta")))
    with pytest.raises(ValueError, match="leaves the volume"):
        ops.deform_sample_patch(**_op_args("meta", start=(4, 1, 0)))
    with pytest.raises(ValueError, match="spacing"):
        ops.deform_sample_patch(**_op_args("meta", spacing=(1.0, 0.0, 1.0)))


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1) for every class the header names, then VNET_E_UNSUPPORTED (-2), before any launch."""
    from vnet_tensorflow_amd import _lib
    fn = _lib.lib().vnet_deform_sample_patch
    one = ctypes.c_void_p(16)
    #     image lab  coef out  outl X  Y  Z  C  s0   s1   s2    sx sy sz P0 P1 P2 flip sigma seed stream
    ok = (one, one, one, one, one, 5, 4, 3, 2, 1.0, 0.8, 1.25, 1, 1, 1, 4, 3, 2, 0, 1.0, 7, None)
    for pos in range(5):                                             # a null pointer
        bad = list(ok)
        bad[pos] = None
        assert fn(*bad) == -1, pos
    for pos in (5, 6, 7, 8):                                         # a size or C < 1
        for v in (0, -3):
            bad = list(ok)
            bad[pos] = v
            assert fn(*bad) == -1, (pos, v)
    for pos in (9, 10, 11):                                          # a spacing not finite or not > 0
        for v in (0.0, -1.0, float("nan"), float("inf")):
            bad = list(ok)
            bad[pos] = v
            assert fn(*bad) == -1, (pos, v)
    for pos, v in ((12, -1), (12, 2), (13, 2), (14, 2), (15, 0), (15, 5), (16, 4), (17, -1), (17, 3)):      # a window not inside the volume
        bad = list(ok)
        bad[pos] = v
        assert fn(*bad) == -1, (pos, v)
    for pos, v in ((18, 8), (18, -1), (19, -1.0), (19, float("nan")), (19, float("inf"))):                  # the flip mask, sigma
        bad = list(ok)
        bad[pos] = v
        assert fn(*bad) == -1, (pos, v)
    # more voxels than an int32 index holds -- and BADARG first where both apply
    big = (one, one, one, one, one, 2048, 1024, 1024, 1, 1.0, 1.0, 1.0, 0, 0, 0, 1, 1, 1, 0, 0.0, 0, None)
    assert fn(*big) == -2
    assert fn(one, one, one, one, one, 65536, 65536, 1, 1, 1.0, 1.0, 1.0, 0, 0, 0, 1, 1, 1, 0, 0.0, 0, None) == -2
    for pos, v in ((0, None), (8, 0), (9, 0.0), (12, -1), (18, 9), (19, -2.0)):
        bad = list(big)
        bad[pos] = v
        assert fn(*bad) == -1, (pos, v)


# ---- the ledger of include/vnet_hip_deform_sample.h ---------------------------------------------------------------------------------------
def test_deform_sample_header_ledger():
    """include/vnet_hip_deform_sample.h beyond tests/test_abi_ledger.py: the 22 parameters begin with three inputs and two outputs under
    these names; deform.hip and sample.hip include the two shared device headers instead of holding copies; the loaded library carries
    the table's argument types."""
    from vnet_tensorflow_amd import _lib
    (params,) = guard.header_functions(HEADER).values()
    assert len(params) == 22
    assert [p[0] for p in params][:5] == ["image", "deformed_label", "coef", "out_image", "out_label"]
    assert [p[2] for p in params][:5] == [True, True, True, False, False]
    csrc = os.path.join(ROOT, "vnet_tensorflow_amd", "csrc")
    # shared, not copied: each device function is defined once, in the header its two users include
    src = {n: open(os.path.join(csrc, n)).read() for n in ("deform.hip", "sample.hip", "deform_sample.hip", "bspline_field.h", "philox_noise.h")}
    for fn_name, home in (("bs_axis(int", "bspline_field.h"), ("df_axis(double", "bspline_field.h"), ("df_lerp(double", "bspline_field.h"),
                          ("philox4x32_10(unsigned", "philox_noise.h"), ("box_muller(unsigned", "philox_noise.h")):
        assert [n for n, text in src.items() if fn_name in text] == [home], fn_name
    assert '#include "bspline_field.h"' in src["deform.hip"] and '#include "bspline_field.h"' in src["deform_sample.hip"]
    assert '#include "philox_noise.h"' in src["sample.hip"] and '#include "philox_noise.h"' in src["deform_sample.hip"]
    assert "#pragma clang fp contract(off)" in src["bspline_field.h"] and "#pragma clang fp contract(off)" in src["deform_sample.hip"]
    bound = _lib.lib()
    assert bound.vnet_deform_sample_patch.argtypes == _lib.SIGNATURES_DEFORM_SAMPLE["vnet_deform_sample_patch"][1]
