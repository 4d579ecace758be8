"""A case of evaluate prepared on the device, the parts that need no GPU: window_params with the NumPy restatement of the window against
the four normalisation classes of transforms.py (==), the exactness of the tier-E inputs, prepare_on_device's refusal of other
pipelines, the configuration switch, the ledger of include/vnet_hip_prepare.h and its error codes before any launch."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import prepare_data as D
from vnet_tensorflow_amd import prepare as P
from vnet_tensorflow_amd import transforms as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "vnet_hip_prepare.h")
SHAPE = (13, 9, 11)


def _volume(C, seed, constant=None):
    x = np.random.default_rng([seed, C]).normal(80.0, 200.0, SHAPE + (C,)).astype(np.float32)
    if constant is not None:
        x[..., constant] = np.float32(-37.5)
    return x


def _through_restatements(t, x):
    """What prepare_on_device does with a normalisation, on the host: NumPy's own sums in, the restated window out."""
    n = x[..., 0].size
    pre, stats = None, None
    if P.stats_passes(t) == 2:
        pre = P.pre_map(P.channel_stats(x), n)
    if P.stats_passes(t) >= 1:
        stats = P.channel_stats(x, pre)
    prm = P.window_params(t, stats, n, pre, channels=x.shape[-1])
    assert prm.shape == (x.shape[-1], 5) and prm.dtype == np.float64
    return P.window_intensity(x, prm), prm


TRANSFORMS = {
    "normalization": lambda: T.Normalization(),
    "statistical": lambda: T.StatisticalNormalization(2.5),
    "statistical narrow": lambda: T.StatisticalNormalization(0.3),
    "statistical pre_norm": lambda: T.StatisticalNormalization(2.5, pre_norm=True),
    "extremum": lambda: T.ExtremumNormalization(0.05),
    "manual": lambda: T.ManualNormalization(-100, 300.5),
}


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", sorted(TRANSFORMS))
def test_window_params_is_the_transform(name, C):
    t = TRANSFORMS[name]()
    for seed, constant in ((0, None), (1, None), (2, C - 1)):
        x = _volume(C, seed, constant)
        with np.errstate(all="ignore"):
            want = t({'image': x, 'label': np.zeros(SHAPE, np.int32)})['image']
        got, prm = _through_restatements(t, x)
        assert got.dtype == want.dtype == np.float32
        assert np.array_equal(got, want, equal_nan=True), (name, C, seed)
        if constant is not None and name in ("normalization", "statistical", "extremum"):
            assert prm[constant, 4] == 1.0 and set(np.unique(got[..., constant])) == {np.float32(255.0)}      # the degenerate window
        if constant is None:
            assert not prm[:, 4].any() and len(np.unique(got)) > 50 and got.min() >= 0.0 and got.max() <= 255.0
    assert P.stats_passes(t) == {"manual": 0, "statistical pre_norm": 2}.get(name, 1)


def test_window_restatement_edges():
    """NaN stays NaN (flag 0) or becomes 255 (flag 1), infinities clamp, -0.0 comes out as +0.0: transforms._window on the same values."""
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 10.0, 20.0, 15.0, 3e38, -3e38], np.float32).reshape(-1, 1, 1, 1)
    for wmin, wmax in ((10.0, 20.0), (15.0, 15.0)):
        t = T.ManualNormalization(wmin, wmax)
        want = t({'image': x, 'label': None})['image']
        got = P.window_intensity(x, P.window_params(t, None, x.size, channels=1))
        assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))
    with pytest.raises(ValueError):
        P.window_params(T.Normalization(), None, 5, channels=1)
    with pytest.raises(TypeError):
        P.window_params(T.Padding(8), None, 5, channels=1)


@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 4099, 300001])
def test_tier_e_is_exact(n):
    """The tier-E inputs: NumPy's pairwise sums and math.fsum agree on sum and css, the mean is an integer."""
    for C in (1, 3):
        x = D.tier_e(n, C, 5)
        assert x.dtype == np.float32 and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 2048
        a, b = P.channel_stats(x), D.fsum_stats(x)
        assert np.array_equal(a, b)
        assert np.array_equal(a[:, 0] / n, np.round(a[:, 0] / n))
    b = D.tier_b(4099, 2, 1)
    assert b.dtype == np.float32 and np.abs(b).min() >= 1.0


def test_crop_and_argmax_restatements():
    x = np.arange(3 * 5 * 2 * 2, dtype=np.float32).reshape(3, 5, 2, 2) + 1
    got = P.crop_window(x, (1, 2, 0), (4, 4, 4))
    assert got.shape == (4, 4, 4, 2) and np.array_equal(got[:2, :3, :2], x[1:, 2:]) and not got[2:].any() and not got[:, 3:].any()
    assert not got[:, :, 2:].any()
    lab = np.arange(30, dtype=np.int32).reshape(3, 5, 2)
    assert P.crop_window(lab, (0, 0, 0), (3, 6, 2)).shape == (3, 6, 2)
    v = np.array([[0.0, -0.0, 0.0], [1.0, np.nan, np.nan], [-5.0, -2.0, -2.0]], np.float32)
    assert list(P.argmax_label(v)) == [0, 1, 1] and P.argmax_label(v).dtype == np.int32


def test_prepare_on_device_serves_deterministic_pipelines_only():
    import torch
    img = torch.zeros(4, 4, 4, 1)
    assert P.prepare_on_device([T.ManualNormalization(0, 1), T.RandomFlip([True])], img, (1, 1, 1)) is None
    assert P.prepare_on_device([T.RandomNoise(), T.Padding(8)], img, (1, 1, 1)) is None
    assert P.prepare_on_device([T.BSplineDeformation()], img, (1, 1, 1)) is None
    out = P.prepare_on_device([], img, (1, 2, 3))
    assert out[0] is img and out[1] is None and out[2] == (1.0, 2.0, 3.0)
    out = P.prepare_on_device([T.Padding(4)], img, (1, 1, 1))             # (nothing to grow: nothing launched)
    assert out[0] is img


def test_config_switch_is_off_by_default(tmp_path):
    from tests.test_host import _config
    from vnet_tensorflow_amd.model import image2label
    m = image2label(None, _config(tmp_path), device="cpu", verbose=False)
    m.read_config()
    assert m.prepare_on_device is False
    cfg = _config(tmp_path)
    cfg["EvaluationSetting"]["PrepareOnDevice"] = True
    m = image2label(None, cfg, device="cpu", verbose=False)
    m.read_config()
    assert m.prepare_on_device is True


# ---- the op up to the first launch, error codes ---------------------------------------------------------------------------------------
def test_ops_refuse_cpu_tensors():
    import torch
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    x = torch.zeros(5, 4, 3, 2)
    with pytest.raises(VnetHipError, match="channel_stats"):
        ops.channel_stats(x)
    with pytest.raises(VnetHipError, match="window_intensity"):
        ops.window_intensity(x, np.zeros((2, 5)))
    with pytest.raises(VnetHipError, match="crop_window"):
        ops.crop_window(x, (0, 0, 0), (2, 2, 2))
    with pytest.raises(VnetHipError, match="argmax_label"):
        ops.argmax_label(x)


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1), VNET_E_UNSUPPORTED (-2), VNET_E_WORKSPACE (-3) before any launch, in that order."""
    from vnet_tensorflow_amd import _lib, ops
    L = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    big = 2 ** 31
    need = 8 * 3 * (4 * ops.STATS_MAX_BLOCKS + 1)
    assert L.vnet_channel_stats_ws_bytes(3) == need and L.vnet_channel_stats_ws_bytes(0) == 0 and L.vnet_channel_stats_ws_bytes(65536) == 0
    s = (one, None, one, 100, 3, one, need, None)                       # (pre may be null)
    for pos in (0, 2, 5):
        bad = list(s)
        bad[pos] = None
        assert L.vnet_channel_stats(*bad) == -1, pos
    for pos, v in ((3, 0), (3, -1), (4, 0), (4, -2), (5, odd)):
        bad = list(s)
        bad[pos] = v
        assert L.vnet_channel_stats(*bad) == -1, (pos, v)
    assert L.vnet_channel_stats(one, None, one, big, 3, one, need, None) == -2
    assert L.vnet_channel_stats(one, None, one, 100, 65536, one, 1 << 40, None) == -2
    assert L.vnet_channel_stats(one, None, one, big, 3, one, 0, None) == -2          # UNSUPPORTED comes before WORKSPACE
    assert L.vnet_channel_stats(one, None, one, 0, 3, one, 0, None) == -1            # BADARG before both
    assert L.vnet_channel_stats(one, one, one, 100, 3, one, need - 1, None) == -3
    w = (one, one, one, 100, 3, None)
    for pos in (0, 1, 2):
        bad = list(w)
        bad[pos] = None
        assert L.vnet_window_intensity(*bad) == -1, pos
    for pos, v in ((3, 0), (4, 0), (4, -1)):
        bad = list(w)
        bad[pos] = v
        assert L.vnet_window_intensity(*bad) == -1, (pos, v)
    assert L.vnet_window_intensity(one, one, one, big, 3, None) == -2 and L.vnet_window_intensity(one, one, one, 100, 65536, None) == -2
    c = (one, one, 5, 4, 3, 2, 1, 1, 1, 4, 4, 4, None)
    for pos in (0, 1):
        bad = list(c)
        bad[pos] = None
        assert L.vnet_crop_words(*bad) == -1, pos
    for pos, v in ((2, 0), (3, -1), (4, 0), (5, 0), (6, -1), (6, 5), (7, 4), (8, 3), (8, 7), (9, 0), (10, -3), (11, 0)):
        bad = list(c)
        bad[pos] = v
        assert L.vnet_crop_words(*bad) == -1, (pos, v)
    assert L.vnet_crop_words(one, one, 2048, 1024, 1024, 1, 0, 0, 0, 4, 4, 4, None) == -2
    assert L.vnet_crop_words(one, one, 5, 4, 3, 1, 0, 0, 0, 2048, 1024, 1024, None) == -2
    assert L.vnet_crop_words(one, one, 2048, 1024, 1024, 1, 2048, 0, 0, 4, 4, 4, None) == -1   # BADARG before UNSUPPORTED
    a = (one, one, 100, 2, None)
    for pos in (0, 1):
        bad = list(a)
        bad[pos] = None
        assert L.vnet_argmax_label(*bad) == -1, pos
    for pos, v in ((2, 0), (2, -5), (3, 0), (3, -1)):
        bad = list(a)
        bad[pos] = v
        assert L.vnet_argmax_label(*bad) == -1, (pos, v)
    assert L.vnet_argmax_label(one, one, big, 2, None) == -2


# ---- the ledger of include/vnet_hip_prepare.h ---------------------------------------------------------------------------------------------
def test_prepare_header_ledger():
    """include/vnet_hip_prepare.h beyond tests/test_abi_ledger.py: the grid cap is one number in the header and in ops."""
    import re
    from vnet_tensorflow_amd import ops
    cap = int(re.search(r"#define VNET_STATS_MAX_BLOCKS (\d+)", open(HEADER).read()).group(1))
    assert cap == ops.STATS_MAX_BLOCKS and cap * 256 < 2 ** 21
