"""U-Net, the parts that need no GPU: the fp64 restatement (tests/unet_oracle.py) against the fixtures made from the reference's own
graph code (tests/golden/make_ref_wiring_unet.py) and against an independent PyTorch-CPU restatement, max-pooling known answers, the
product's variable names, routing of the 3^3 convolutions, the ledger of include/vnet_hip_unet.h and the config surface.

The third fixture is NOT the (6, 10, 12) patch: a level of odd size does not build in the reference -- max_pool3d VALID floors 3 -> 1
and conv3d_transpose SAME back to 3 needs ceil(3 / 2) = 2 coarse voxels, which TF 1.15 rejects -- so the fixture is the non-cubic
(4, 8, 12) patch, and test_odd_level_is_refused_by_name pins that the product refuses the odd one by name.  Odd sizes of the pooling
kernels themselves are covered by the max-pool tests here and in tests/test_hip_unet.py."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import unet_oracle as U, unet_torch as UT

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("c1k2", "c3k3", "odd")


def load_fixture(case):
    z = np.load(os.path.join(HERE, "golden", "unet_ref_wiring_%s.npz" % case))
    cin, K, C, levels, convs, bottom = [int(v) for v in z["config"]]
    names = [str(n) for n in z["names"]]
    trainable = [bool(t) for t in z["trainable"]]
    shapes = [tuple(int(v) for v in str(s).split(",")) if str(s) else () for s in z["shapes"]]
    values = {n: z["v:" + n].astype(np.float64) for n in names}
    return z, (cin, K, C, levels, convs, bottom), names, trainable, shapes, values


def make_oracle(cfg, names, trainable, values):
    cin, K, C, levels, convs, bottom = cfg
    ps = O.ParamStore(rng=np.random.default_rng(0), values=values)
    for n, t in zip(names, trainable):
        if not t:
            ps.state[n] = values[n].copy()
    return U.UNetOracle(K, 0.0, C, levels, convs, bottom, "relu", ps), ps


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_reference_wiring(case):
    """Same variables in the same order, logits and moving statistics to 1e-10 (the bound of
    test_reference_wiring_matches_oracle_and_product_names).  Pins wiring and names, not TF numerics: parity stays unpinned."""
    z, cfg, names, trainable, shapes, values = load_fixture(case)
    net, ps = make_oracle(cfg, names, trainable, values)
    logits = net.GetNetwork(z["x"].astype(np.float64))
    assert [(n, tuple(ps.vars[n].v.shape)) for n in ps.order] == [(n, s) for n, s, t in zip(names, shapes, trainable) if t]
    assert set(ps.state) == {n for n, t in zip(names, trainable) if not t}
    for i, n in enumerate(names):
        if n.endswith("/gamma"):
            base = n[:-len("gamma")]
            assert names[i + 1:i + 4] == [base + "beta", base + "moving_mean", base + "moving_variance"]
    assert np.abs(logits.v - z["logits"]).max() < 1e-10 * max(1.0, np.abs(z["logits"]).max())
    for n in ps.state:
        assert np.abs(ps.state[n] - z["u:" + n]).max() < 1e-10, n
    # the decoder block's batch-norms sit outside its conv_i scopes (networks.py:65,84)
    assert "unet/decoder/level_1/batch_normalization/gamma" in names and "unet/decoder/level_1/batch_normalization_1/gamma" in names
    assert not any(re.search(r"decoder/level_\d+/conv_\d+/batch_normalization", n) for n in names)


@pytest.mark.parametrize("case", ("c1k2", "c3k3"))
def test_oracle_matches_torch_fp64(case):
    """Loss, logits and every gradient against PyTorch-CPU fp64 autograd (F.conv3d, F.max_pool3d, F.conv_transpose3d), to 1e-10."""
    z, cfg, names, trainable, shapes, values = load_fixture(case)
    cin, K, C, levels, convs, bottom = cfg
    net, ps = make_oracle(cfg, names, trainable, values)
    x, lab = z["x"].astype(np.float64), z["labels"].astype(np.int64)
    ref = O.run_step(x, lab[..., None], net, "sorensen")
    loss, logits, grads = UT.run(values, x, lab, K, C, levels, convs, bottom, torch.float64)
    assert abs(loss - ref["loss"]) < 1e-10
    assert np.abs(logits - ref["logits"]).max() < 1e-10
    assert set(grads) == set(ref["grads"])
    for k in grads:
        assert np.abs(grads[k] - ref["grads"][k]).max() < 1e-10, k


def _pool_grad(x, g):
    v = O.Var(np.asarray(x, dtype=np.float64))
    y = U.max_pool2(v)
    O.backward(y, seed=g)
    return y.v, v.g


def test_max_pool_known_answers():
    # a window with a unique maximum
    x = np.arange(8, dtype=np.float64).reshape(1, 2, 2, 2, 1)
    x[0, 0, 1, 0, 0] = 99.0
    y, dx = _pool_grad(x, np.full((1, 1, 1, 1, 1), 3.0))
    assert y.shape == (1, 1, 1, 1, 1) and y[0, 0, 0, 0, 0] == 99.0
    want = np.zeros_like(x); want[0, 0, 1, 0, 0] = 3.0
    assert np.array_equal(dx, want)
    # odd sizes floor (VALID): the trailing plane / row / column takes no part and gets zero gradient
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 3, 7, 3))
    y, dx = _pool_grad(x, np.ones((2, 2, 1, 3, 3)))
    assert y.shape == (2, 2, 1, 3, 3)
    ref = torch.nn.functional.max_pool3d(torch.from_numpy(x).permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1).numpy()
    assert np.array_equal(y, ref)
    assert not dx[:, 4].any() and not dx[:, :, 2].any() and not dx[:, :, :, 6].any()
    assert dx.sum() == y.size and set(np.unique(dx)) == {0.0, 1.0}
    # a tied window: the gradient goes to the FIRST maximum in (dz, dy, dx) scan order
    x = np.zeros((1, 2, 2, 2, 1)); x[0, 0, 1, 1, 0] = x[0, 1, 0, 0, 0] = x[0, 1, 1, 1, 0] = 5.0
    y, dx = _pool_grad(x, np.full((1, 1, 1, 1, 1), 2.0))
    want = np.zeros_like(x); want[0, 0, 1, 1, 0] = 2.0
    assert y[0, 0, 0, 0, 0] == 5.0 and np.array_equal(dx, want)
    x = np.zeros((1, 2, 2, 2, 1))                          # all eight tied (a ReLU window of zeros): the first voxel
    _, dx = _pool_grad(x, np.full((1, 1, 1, 1, 1), 1.0))
    assert dx[0, 0, 0, 0, 0] == 1.0 and dx.sum() == 1.0


@pytest.mark.parametrize("case", CASES)
def test_product_creates_the_fixture_variables(case):
    from vnet_tensorflow_amd import networks
    z, cfg, names, trainable, shapes, values = load_fixture(case)
    cin, K, C, levels, convs, bottom = cfg
    net = networks.UNet(K, 0.0, C, levels, convs, bottom, True, "relu", device="cpu").build(tuple(z["x"].shape))
    sd = net.state_dict()
    assert [n for n, _ in net.named_parameters()] == [n for n, t in zip(names, trainable) if t]
    assert [n for n in net.variables.buffers] == [n for n, t in zip(names, trainable) if not t]
    for n, s in zip(names, shapes):
        assert tuple(sd[n].shape) == s, n
    assert set(sd) == set(names)


def test_unet_signature_and_refusals():
    import inspect
    from vnet_tensorflow_amd import networks, layers2, ops
    from vnet_tensorflow_amd._lib import VnetHipError
    sig = inspect.signature(networks.UNet.__init__)
    assert list(sig.parameters)[1:] == ["num_output_channels", "dropout_rate", "num_channels", "num_levels", "num_convolutions",
                                        "bottom_convolutions", "is_training", "activation_fn", "device"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["dropout_rate"], d["num_channels"], d["num_levels"], d["num_convolutions"], d["bottom_convolutions"],
            d["is_training"], d["activation_fn"], d["device"]) == (0.01, 4, 4, 2, 2, True, "relu", None)
    with pytest.raises(ValueError, match="num_convolutions"):
        networks.UNet(2, num_convolutions=(1, 2))
    x = torch.zeros(1, 4, 4, 4, 2)
    with pytest.raises(VnetHipError, match="max_pool2"):
        ops.max_pool2(x)                                    # a CPU tensor: no fallback
    for kw, word in ((dict(ksize=[1, 3, 3, 3, 1]), "ksize"), (dict(strides=[1, 1, 1, 1, 1]), "strides"), (dict(padding="SAME"), "padding")):
        with pytest.raises(NotImplementedError, match=word):
            layers2.max_pool3d(x, **kw)


def test_odd_level_is_refused_by_name():
    from vnet_tensorflow_amd import networks
    from vnet_tensorflow_amd._lib import VnetHipError
    with pytest.raises(VnetHipError, match="odd size"):
        networks.UNet(2, 0.0, 8, 2, 2, 1, device="cpu").build((2, 6, 10, 12, 1))      # 6 -> 3 at level 2


def test_route_ks3():
    from vnet_tensorflow_amd import _lib, ops
    L = _lib.lib()
    for (C0, C1, Cout, B, dims) in ((1, 0, 4, 2, (8, 8, 8)), (4, 4, 4, 1, (8, 8, 8)), (32, 32, 32, 1, (16, 16, 16)), (16, 0, 16, 1, (128, 128, 128)),
                                 (256, 0, 256, 1, (8, 8, 8)), (8, 0, 8, 2, (4, 8, 12))):
        Cin, N = C0 + C1, B * dims[0] * dims[1] * dims[2]
        shape = "%d^3x%d %d->%d" % (dims[2], B, Cin, Cout)
        f = ops.route(ops.FWD, 3, 1, 0, False, False, C0, C1, Cout, B, dims, dims)
        assert (f.family, f.pack, f.tag, f.flops) == ("conv", (ops.PACK_FWD, 27, Cin, Cout), "conv k3 s1 " + shape, 2.0 * N * 27 * Cin * Cout)
        assert f.ws == L.vnet_conv_ws_bytes(3, 0, 1, 0, Cin, Cout, B, *dims)
        assert f.stats_rows == L.vnet_conv_stats_rows(3, 0, 1, 0, Cin, Cout, 0, B, *dims)
        b = ops.route(ops.BWD, 3, 1, 0, False, False, C0, C1, Cout, B, dims, dims)
        assert (b.family, b.pack, b.flops) == ("conv", (ops.PACK_BWD, 27, Cin, Cout), 2.0 * N * 27 * Cin * Cout)
        assert b.tag == "conv k3 s1 %d^3x%d %d->%d" % (dims[2], B, Cout, Cin)
        assert b.ws == L.vnet_conv_ws_bytes(3, 0, 1, 0, Cout, Cin, B, *dims) and b.stats_rows == 0
        w = ops.route(ops.WGRAD, 3, 1, 0, False, False, C0, C1, Cout, B, dims, dims)
        assert (w.family, w.pack, w.tag, w.flops) == ("wgrad", None, "wgrad k3 s1 " + shape, 2.0 * N * 27 * Cin * Cout)
        assert w.ws == L.vnet_wgrad_ws_bytes(3, 0, 1, Cin, Cout, B, *dims) and w.ws > 0
        # fp32_split3: the f32x3 kernels are 5^3 only, the 3^3 layers stay on the fp32 MFMA family
        assert ops.route(ops.FWD, 3, 1, 0, False, True, C0, C1, Cout, B, dims, dims).family == "conv"
        assert ops.route(ops.WGRAD, 3, 1, 0, False, True, C0, C1, Cout, B, dims, dims).family == "wgrad"
    assert L.vnet_conv_ws_bytes(3, 0, 1, 0, 256, 256, 1, 8, 8, 8) > 0          # split-K at the deep levels
    assert L.vnet_conv_ws_bytes(3, 0, 1, 0, 16, 16, 1, 128, 128, 128) == 0
    assert L.vnet_conv_ws_bytes(3, 3, 1, 0, 256, 256, 1, 8, 8, 8) == L.vnet_conv_ws_bytes(3, 0, 1, 0, 256, 256, 1, 8, 8, 8)
    # what stays refused: stride 2, the transposed form, another x extent
    assert L.vnet_conv_ws_bytes(3, 0, 2, 0, 256, 256, 1, 8, 8, 8) == 0 and L.vnet_conv_ws_bytes(3, 1, 1, 0, 256, 256, 1, 8, 8, 8) == 0
    assert L.vnet_conv_stats_rows(3, 0, 2, 0, 16, 16, 0, 1, 8, 8, 8) == 0 and L.vnet_wgrad_ws_bytes(3, 0, 2, 16, 16, 1, 8, 8, 8) == 0
    one = ctypes.c_void_p(16)
    assert L.vnet_conv_fwd(3, 0, 2, 0, one, 16, None, 0, one, None, one, 16, None, 0, 1, 8, 8, 8, 4, 4, 4, None, 0, None) == -2
    assert L.vnet_conv_wgrad(3, 1, 1, one, 16, None, 0, one, 16, one, 1, 8, 8, 8, 8, 8, 8, None, 0, None) == -2


def test_unet_header_ledger():
    """include/vnet_hip_unet.h beyond tests/test_abi_ledger.py: the guarded cases of tests/test_hip_unet_guard.py also run the
    ks = 3 launches of vnet_hip.h the U-Net opens."""
    from tests import test_hip_unet_guard as TG
    covered = set()
    for entries, _fn in TG.CASES.values():
        covered |= set(entries)
    assert {"vnet_conv_fwd", "vnet_conv_fwd_stats", "vnet_conv_fwd_acc", "vnet_conv_wgrad"} <= covered


def _config(name="UNet", dtype=None):
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": "./data/training", "TestingDataDirectory": "./data/testing", "ImageFilenames": ["image.nii.gz"],
                 "LabelFilename": "label.nii.gz"},
        "BatchSize": 1, "PatchShape": [16, 16, 16], "SegmentationClasses": [0, 1], "Epoches": 1,
        "Networks": {"Name": name, "Dropout": 0.01, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": 2, "BottomConvolutions": 2},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}},
        "Loss": {"Name": "sorensen"}}}
    if dtype:
        cfg["TrainingSetting"]["ComputeDtype"] = dtype
    return cfg


def test_unet_config_parses_and_bf16_is_refused_by_name():
    from vnet_tensorflow_amd import model
    from vnet_tensorflow_amd._lib import VnetHipError
    m = model.image2label(None, _config(), device="cpu", verbose=False)
    m.read_config()
    assert m.network_name == "UNet" and m.num_convolutions == 2 and m.bottom_convolutions == 2
    m.build_model_graph()
    assert type(m.network).__name__ == "UNet" and m.network.activation_fn == "relu"
    assert "unet/encoder/level_1/conv_1/weights" in m.network.state_dict() and "unet/output/batch_normalization/gamma" in m.network.state_dict()
    for dt in ("fp32", "fp32_split3"):
        model.image2label(None, _config(dtype=dt), device="cpu", verbose=False).read_config()
    with pytest.raises(VnetHipError, match="bf16.*UNet"):
        model.image2label(None, _config(dtype="bf16"), device="cpu", verbose=False).read_config()
    with pytest.raises(SystemExit):                                              # unknown names keep the reference's exit
        bad = model.image2label(None, _config(name="Dense"), device="cpu", verbose=False)
        bad.read_config()
        bad.build_model_graph()


# ---- the full-size fixtures (tests/golden/make_golden_full_unet.py) -------------------------------------------------------------------
def _full_fixtures():
    import glob
    gold = os.path.join(HERE, "golden")
    return sorted(glob.glob(os.path.join(gold, "unet_*cube*.npz")) + glob.glob(os.path.join(gold, "spread", "unet_*cube*.npz")))


def test_full_size_generator_recipe_at_16cube(tmp_path):
    """make() at a size the CPU suite can afford: the names in creation order, the stored sample positions and a loss equal to
    O.run_step on the same seeds."""
    from tests.golden import make_golden_full_unet as G
    from tests.golden.make_golden_full import SAMPLE, STRIDE, sample_indices
    case = "u64b2s2"
    z = np.load(G.make(case, root=str(tmp_path), P=16))
    fname, _, B, seed = G.CASES[case]
    net, ps = G.make_net(G.WEIGHT_SEED[case])
    x, lab = O.synthetic_batch(B, 16, 1, G.CONFIG[0], seed=seed)
    ref = O.run_step(x.astype(np.float64), lab, net, "sorensen")
    names = list(ps.vars.keys())
    assert [str(n) for n in z["names"]] == names == G.creation_order(G.WEIGHT_SEED[case])[0] and len(names) == 100
    assert float(z["loss"]) == ref["loss"] and z["logits_sample"].dtype == z["grad_sample"].dtype == np.float64
    assert np.array_equal(z["logits_sample"], ref["logits"][:, ::STRIDE, ::STRIDE, ::STRIDE])
    for i, n in enumerate(names):
        gr = ref["grads"][n].ravel()
        idx = sample_indices(i, gr.size)
        assert len(idx) == min(gr.size, SAMPLE) and np.array_equal(z["grad_sample"][i][:len(idx)], gr[idx]), n
        assert z["grad_norm"][i] == np.linalg.norm(gr)
    assert not os.path.exists(os.path.join(str(tmp_path), G.TF_DIR))          # crops belong to the 128^3 case alone
    for n, v in ps.state.items():
        assert np.array_equal(z["state:" + n], v.astype(np.float32))


def test_full_size_fixtures_are_well_formed():
    """Every committed unet_*cube*.npz: the oracle's creation order for the stated configuration, finite arrays, a zero gradient
    norm for the biases and for nothing else; the teacher-forcing crops of the 128^3 case are all there."""
    from tests.golden import make_golden_full_unet as G
    files = _full_fixtures()
    assert sorted(os.path.relpath(f, os.path.join(HERE, "golden")) for f in files) == sorted(c[0] for c in G.CASES.values())
    order = G.creation_order()[0]
    for f in files:
        z = np.load(f)
        assert [str(n) for n in z["names"]] == order, f
        for k in z.files:
            if k != "names":
                assert np.isfinite(z[k]).all(), (f, k)
        for n, gn in zip(order, z["grad_norm"]):
            assert (gn < 1e-7) == n.endswith("/biases"), (f, n, gn)
        case = [c for c, v in G.CASES.items() if f.endswith(os.sep + os.path.basename(v[0])) and ("spread" in f) == ("spread" in v[0])][0]
        assert [int(v) for v in z["config"]] == [G.CASES[case][1], G.CASES[case][2], G.WEIGHT_SEED[case], G.CASES[case][3]]
    for tag in [t for t, _ in G.TF_LAYERS.values()] + [G.TF_POOL[0]]:
        x, dy, lo = G.load_tf(tag)
        assert np.isfinite(x).all() and np.isfinite(dy).all() and np.abs(x).max() > 0 and np.abs(dy).max() > 0
        assert os.path.getsize(G.tf_path(tag, "x")) < 2 ** 20 and os.path.getsize(G.tf_path(tag, "dy")) < 2 ** 20


def test_torch_fp64_reproduces_the_64cube_fixture():
    """tests/unet_torch.py in float64 shares no code with the generator's oracle; against unet_64cube_b2.npz: logits max-abs 1e-9, loss
    1e-12, sampled gradient rel-L2 1e-7 per tensor -- about 100 x what the two fp64 implementations differ by on this case (1.8e-11,
    7.9e-15, 9.5e-10) and five orders below the fp32 figures.  The one place a mistake in the generator would otherwise go unseen."""
    from tests.golden import make_golden_full_unet as G
    from tests.golden.make_golden_full import STRIDE, sample_indices
    from tests.util import rel_l2
    fname, P, B, seed = G.CASES["u64b2"]
    z = np.load(os.path.join(HERE, "golden", fname))
    names, values = G.creation_order(G.WEIGHT_SEED["u64b2"])
    K, _, C, levels, convs, bottom, _ = G.CONFIG
    x, lab = O.synthetic_batch(B, P, 1, K, seed=seed)
    loss, logits, grads = UT.run(values, x.astype(np.float64), lab[..., 0], K, C, levels, convs, bottom, torch.float64)
    e_logits, e_loss, worst = np.abs(logits[:, ::STRIDE, ::STRIDE, ::STRIDE] - z["logits_sample"]).max(), abs(loss - float(z["loss"])), 0.0
    compared = 0
    for i, n in enumerate(names):
        if n.endswith("/biases"):
            continue
        got = grads[n].ravel()
        idx = sample_indices(i, got.size)
        worst = max(worst, rel_l2(got[idx], z["grad_sample"][i][:len(idx)]))
        compared += 1
    print("torch fp64 against unet_64cube_b2: logits %.2e loss %.2e gradients %.2e (%d tensors)" % (e_logits, e_loss, worst, compared))
    assert compared == 77
    assert e_logits < 1e-9 and e_loss < 1e-12 and worst < 1e-7
