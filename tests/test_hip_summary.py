"""-m gpu: include/vnet_hip_summary.h on the device, every byte of every output `==` its NumPy restatement
(vnet_tensorflow_amd/summary.py), then the product: image2label.train() with TrainingSetting.SummaryInterval on the 16^3 synthetic
config of tests/test_hip_train_loop.py -- event files that read back CRC-clean with the tags of DESIGN.md section 6g, a trajectory that
does not depend on SummaryInterval, and no file at all without the key.

Shapes (B,X,Y,Z,C): extents all different and none a multiple of the 64 x 64 tile (a swapped axis or a tile-tail error cannot cancel),
one voxel, whole tiles, more than one tile along y and along (z, c), and more tiles than VNET_SUMMARY_MAX_BLOCKS workgroups."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_hip_train_loop import _cfg
from tests.test_summary_host import FMA_PROBES, decode_png
from tests.util import g
from vnet_tensorflow_amd import summary as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 5, 7, 3, 3), (1, 33, 17, 65, 1), (1, 1, 1, 1, 1), (1, 64, 64, 64, 2), (1, 3, 70, 5, 2), (1, 4099, 3, 2, 1)]
SPECIAL = np.float32([-0.0, -1.0, 0.999, 255.0, 255.999, 256.0, 1e9, np.inf, -np.inf, np.nan, -0.5, 254.999, 1e-40, -1e-40])


def _fill(shape, values):
    """`values` repeated over the tensor: the first ones are in every shape that has room for them."""
    return np.resize(values, int(np.prod(shape))).reshape(shape)


def test_shape_list_covers_the_paths():
    from vnet_tensorflow_amd import ops
    tiles = [B * X * -(-Y // 64) * -(-(Z * C) // 64) for B, X, Y, Z, C in SHAPES]
    assert max(tiles) > ops.SUMMARY_MAX_BLOCKS and min(tiles) == 1
    assert any(Y > 64 for _, _, Y, _, _ in SHAPES) and any(Z * C > 64 for _, _, _, Z, C in SHAPES)


@pytest.mark.parametrize("shape", SHAPES)
def test_intensity_slices(dev, shape):
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(sum(shape))
    vals = (rng.random(5000, dtype=np.float32) * np.float32(262) - np.float32(3)).astype(np.float32)
    vals[rng.integers(0, 5000, 600)] = SPECIAL[rng.integers(0, len(SPECIAL), 600)]
    x = _fill(shape, np.concatenate([SPECIAL, vals])).astype(np.float32)
    got = ops.summary_slices_intensity(g(x, dev))
    B, X, Y, Z, C = shape
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, C, Z, X, Y)
    assert np.array_equal(got.cpu().numpy(), S.slices_intensity(x))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shape", SHAPES)
def test_index_slices(dev, shape, dtype):
    from vnet_tensorflow_amd import ops
    npd = np.int32 if dtype == torch.int32 else np.int64
    rng = np.random.default_rng(sum(shape) + 1)
    info = np.iinfo(npd)
    for K, classes in ((2, [0, 1]), (5, [0, 1, 2, 3, 4]), (3, [1, 2, 3])):
        factor = S.index_factor(K, classes)
        vals = np.concatenate([np.arange(K), [K, 255, 256, 257, -1, -300, info.max, info.min, 2 ** 31 - 1, -2 ** 31],
                               rng.integers(0, K, 3000), rng.integers(-1000, 1000, 500)]).astype(npd)
        x = _fill(shape, vals).astype(npd)
        got = ops.summary_slices_index(g(x, dev, dtype), factor)
        assert np.array_equal(got.cpu().numpy(), S.slices_index(x, factor)), (K, factor)
    got = ops.summary_slices_index(g(x, dev, dtype), -7)
    assert np.array_equal(got.cpu().numpy(), S.slices_index(x, -7))


@pytest.mark.parametrize("shape", SHAPES)
def test_rainbow_slices(dev, shape):
    """The k/1024 grid, seeded draws, and in front of them the probes at which a contracted 6 * H - 3 / - 2 / - 4 changes a byte."""
    from vnet_tensorflow_amd import ops
    probes = np.array(FMA_PROBES, dtype=np.uint32).view(np.float32)
    grid = np.arange(1025, dtype=np.float32) / np.float32(1024)
    draws = np.random.default_rng(sum(shape) + 2).random(20000, dtype=np.float32)
    x = _fill(shape, np.concatenate([probes, grid, draws, np.float32([np.nan])])).astype(np.float32)
    got = ops.summary_slices_rainbow(g(x, dev))
    B, X, Y, Z, K = shape
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, K, Z, X, Y, 3)
    ref = S.slices_rainbow(x)
    bad = np.nonzero((got.cpu().numpy() != ref).any(-1))
    assert len(bad[0]) == 0, "first differing pixel %s: %s vs %s" % ([int(i[0]) for i in bad], got.cpu().numpy()[bad][0], ref[bad][0])


def test_fma_probes_reach_the_kernel(dev):
    """Every probe, alone: the kernel gives the separately rounded bytes (a fused multiply-add gives other ones, tests/test_summary_host.py)."""
    from vnet_tensorflow_amd import ops
    p = np.array(FMA_PROBES, dtype=np.uint32).view(np.float32).reshape(1, 1, 1, len(FMA_PROBES), 1)
    got = ops.summary_slices_rainbow(g(p, dev)).cpu().numpy()
    assert np.array_equal(got, S.slices_rainbow(p))


@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 3), (1, 64, 64, 64, 2)])
def test_softmax_rows_of_the_loss_head(dev, shape):
    """What the product feeds the kernels: the fp32 softmax and the int64 prediction of ops.softmax_argmax (the loss head's own)."""
    from vnet_tensorflow_amd import ops
    logits = g(np.random.default_rng(5).normal(0, 3, shape).astype(np.float32), dev)
    sm, pred = ops.softmax_argmax(logits)
    assert sm.dtype == torch.float32 and pred.dtype == torch.int64            # the head keeps logits and softmax fp32 in every ComputeDtype
    assert np.array_equal(ops.summary_slices_rainbow(sm).cpu().numpy(), S.slices_rainbow(sm.cpu().numpy()))
    f = S.index_factor(shape[-1], list(range(shape[-1])))
    p5 = pred.reshape(shape[:-1] + (1,))
    assert np.array_equal(ops.summary_slices_index(p5, f).cpu().numpy(), S.slices_index(p5.cpu().numpy(), f))


def test_arguments_are_checked(dev):
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    x = torch.zeros((1, 2, 3, 4, 1), device=dev)
    with pytest.raises(VnetHipError):
        ops.summary_slices_intensity(x.cpu())
    with pytest.raises(VnetHipError):
        ops.summary_slices_intensity(x.to(torch.bfloat16))
    with pytest.raises(VnetHipError):
        ops.summary_slices_rainbow(x[..., 0])
    with pytest.raises(VnetHipError):
        ops.summary_slices_index(x, 255)
    with pytest.raises(VnetHipError):
        ops.summary_slices_intensity(x, out=torch.empty(23, dtype=torch.uint8, device=dev))
    out = torch.empty(24, dtype=torch.uint8, device=dev)
    assert ops.summary_slices_intensity(x, out=out) is out and not out.any()


# ---- the product ---------------------------------------------------------------------------------------------------------------------
def _design_patterns():
    """The first column of the tag table of DESIGN.md section 6g: {pattern: 'mixed' | 'image' | ''}."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 6g."):]
    sec = sec[:sec.index("\n## ", 5)]
    rows = re.findall(r"^\| `([^`]+)` \| ([^|]*) \|", sec, re.M)
    assert rows
    return {tag: when.strip() for tag, when in rows}


def _pattern(tag, files):
    m = re.match(r"^(.*)_batch\d+/image(/\d+)?$", tag)
    if m:
        name = m.group(1)
        name = "<file>" if name in files else ("softmax_<class>" if name.startswith("softmax_") else name)
        return "%s_batch<b>/image/<z>" % name
    return re.sub(r"^metrics/(sensitivity|specificity|dice|auc)_.+$", r"metrics/\1_<class>", tag)


def _events(logdir, run):
    files = S.event_files(os.path.join(logdir, run))
    assert len(files) == 1 and S.file_version(files[0]) == "brain.Event:2"
    return list(S.read_events(files[0]))[1:]                                  # (both CRCs of every record verified)


@pytest.mark.parametrize("loss", ["sorensen", "mixed_sorensen"])
def test_train_writes_event_files(tmp_path, dev, loss):
    from vnet_tensorflow_amd.model import image2label
    np.random.seed(0)
    cfg = _cfg(tmp_path, SummaryInterval=1, ImageLog=True, Testing=True)
    cfg["TrainingSetting"]["Loss"]["Name"] = loss
    m = image2label(None, cfg, device=dev, verbose=False)
    m.train()
    assert m.global_step == 4 and m._summary_writers == (None, None) and not m._summary_on            # closed on the way out
    train, test = _events(str(tmp_path / "log"), "train"), _events(str(tmp_path / "log"), "test")
    assert [e[1] for e in train] == list(range(1, m.global_step + 1)) and [e[1] for e in test] == [2, 4]
    files, Z = ["image.npy"], 16
    want = S.step_tags(files, [0, 1], 2, Z, loss, True)
    table = _design_patterns()
    mixed = loss.startswith("mixed_")
    for _wall, _step, values in train + test:
        assert list(values) == want
        assert {_pattern(t, files) for t in values} == {p for p, when in table.items() if mixed or when != "mixed"}
        for name in ("image.npy", "label", "pred", "softmax_0", "softmax_1"):
            for b in range(2):
                entries = [values[t] for t in S.image_tags("%s_batch%d" % (name, b), Z)]
                assert len(entries) == Z and all(e[:3] == (16, 16, 3 if name.startswith("softmax") else 1) for e in entries)
        scalars = {t: v for t, v in values.items() if isinstance(v, float)}
        assert all(np.isfinite(v) for v in scalars.values()) and 0.0 <= scalars["metrics/accuracy"] <= 1.0
        if mixed:
            assert scalars["loss/1.dice"] + scalars["loss/2.regularized_xent"] == pytest.approx(scalars["loss/0.total_loss"], abs=1e-6)
    last = train[-1][2]
    assert last["loss/0.total_loss"] == m.last_loss
    from vnet_tensorflow_amd import optim
    assert last["learning_rate_1"] == float(np.float32(optim.exponential_decay(1e-2, 3, 100, 0.99)))       # the rate step 4 used
    for tag in S.image_tags("label_batch0", Z) + S.image_tags("pred_batch1", Z):
        pix = decode_png(last[tag][3])
        assert pix.shape == (16, 16) and set(np.unique(pix)) <= {0, 255}
    rgb = decode_png(last["softmax_1_batch0/image/7"][3])
    assert rgb.shape == (16, 16, 3) and (rgb.max(-1) == 255).all()                           # S = V = 1: one channel is saturated
    img = np.stack([decode_png(last[t][3]) for t in S.image_tags("label_batch0", Z)])
    assert img.any()                                                                           # the synthetic label is not empty


def _trajectory(tmp, dev, interval):
    from vnet_tensorflow_amd.model import image2label
    np.random.seed(7)
    over = {} if interval is None else {"SummaryInterval": interval}
    cfg = _cfg(tmp, Testing=False, Epoches=3, PrefetchDepth=0, ImageLog=True, **over)
    m = image2label(None, cfg, device=dev, verbose=False)
    m.train()
    torch.cuda.synchronize()
    assert m.global_step == 6 and m.dropout_rate == 0.05 and m.step_mode() == "whole" and m._graphs is not None
    return m


def test_trajectory_does_not_depend_on_summary_interval(tmp_path, dev):
    """Dropout 0.05, the step graph on, the same seeds, 6 steps: once without summaries (steps 1 and 2 eager warm-up, the capture at
    step 3, replays from there) and once with SummaryInterval 2 (steps 2, 4 and 6 enqueued eagerly with the loss head asked for softmax
    and prediction; steps 1 and 3 the warm-up, step 5 the capture and a replay).  Every parameter and every moving statistic is bit-identical."""
    a = _trajectory(tmp_path / "a", dev, 0)
    b = _trajectory(tmp_path / "b", dev, 2)
    assert [e[1] for e in _events(str(tmp_path / "b" / "log"), "train")] == [2, 4, 6]
    assert a.last_loss == b.last_loss
    assert torch.equal(a.flat.data, b.flat.data)
    sa, sb = dict(a.network.state_dict()), dict(b.network.state_dict())
    assert set(sa) == set(sb) and any("moving_mean" in k for k in sa)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert not os.path.exists(tmp_path / "a" / "log" / "train") and not os.path.exists(tmp_path / "b" / "log" / "test")


def test_no_key_no_files(tmp_path, dev):
    m = _trajectory(tmp_path, dev, None)
    assert m.summary_interval == 0
    log = tmp_path / "log"
    assert os.path.isdir(log) and [f for _r, _d, fs in os.walk(log) for f in fs] == []
    assert not os.path.exists(log / "train") and not os.path.exists(log / "test")
