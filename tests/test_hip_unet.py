"""-m gpu: the U-Net path on the HIP library -- the 3^3 convolution family, 2x2x2 max-pooling, networks.UNet as a whole, training
steps, hipGraph replay, sliding-window evaluation and checkpoints -- against the fp64 restatement tests/unet_oracle.py.

Whole-network bounds are those tests/test_hip_network.py holds the small V-Nets to (logits rel-L2 1e-4 or max-abs 1e-3, loss 1e-5,
per-tensor gradient rel-L2 1e-3 for filters and 5e-3 for per-channel vectors).  A case that misses one is not widened by eye: the
PyTorch-CPU fp32 restatement (tests/unet_torch.py) of the same net on the same inputs gives the error fp32 arithmetic through the
batch-norms costs against the fp64 oracle, and the bound becomes 2 x that (profiles/unet_parity.txt)."""
import os

import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import unet_oracle as U, unet_torch as UT
from tests.test_hip_ops import _conv_case
from tests.test_unet_host import load_fixture, make_oracle
from tests.util import g, check_close, rel_l2

pytestmark = pytest.mark.gpu


# ---- 1. the 3^3 convolution family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [
    # B, D, H, W, C0, C1, Cout
    (2, 8, 8, 8, 1, 0, 4),          # first layer, one modality: scalar gather, Cout < 16
    (1, 8, 8, 8, 3, 0, 4),          # three modalities
    (2, 4, 4, 4, 4, 0, 8),
    (1, 16, 16, 16, 8, 0, 8),
    (1, 32, 32, 32, 16, 0, 16),     # wide rows: 4x4x16 filter-gradient bricks
    (1, 16, 16, 16, 32, 32, 64),    # two sources (decoder concat), NS = 4
    (2, 5, 9, 13, 16, 0, 16),       # ragged
    (1, 5, 9, 13, 4, 4, 4),         # ragged, two narrow sources
    (1, 8, 8, 8, 64, 0, 64),        # split-K
    (1, 4, 4, 4, 256, 0, 256),      # 4x4x4 bricks, split-K + tap split
    (1, 8, 8, 8, 256, 0, 256),
    (1, 6, 6, 18, 3, 0, 5),         # neither channel count a multiple of 4
])
def test_conv3(dev, shape):
    _conv_case(dev, *shape, ks=3, stride=1, seed=sum(shape))


@pytest.mark.parametrize("shape", [(1, 16, 16, 16, 16, 0, 16), (1, 8, 8, 8, 64, 0, 64), (2, 5, 9, 13, 4, 4, 8), (1, 8, 8, 8, 32, 32, 32)])
def test_conv3_accumulate_is_a_separate_add(dev, shape):
    """y += conv(x) is bit-identical to the same kernel's plain output added to y."""
    from vnet_tensorflow_amd import ops
    B, D, H, W, C0, C1, Co = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x0 = torch.randn(B, D, H, W, C0, generator=gen).to(dev)
    x1 = torch.randn(B, D, H, W, C1, generator=gen).to(dev) if C1 else None
    w = (torch.randn(3, 3, 3, C0 + C1, Co, generator=gen) * 0.1).to(dev)
    prev = torch.randn(B, D, H, W, Co, generator=gen).to(dev)
    r = ops.route(ops.FWD, 3, 1, 0, False, False, C0, C1, Co, B, (D, H, W), (D, H, W))
    y = torch.empty_like(prev)
    ops._conv_launch(r, x0, x1, w, None, y)
    acc = prev.clone()
    ops._conv_launch(r, x0, x1, w, None, acc, accum=True)
    assert torch.equal(acc, prev + y)


@pytest.mark.parametrize("shape,Cin,Cout,residual", [
    ((1, 32, 32, 32), 16, 16, True),
    ((2, 24, 20, 28), 8, 24, False),      # ragged bricks: voxels outside the volume must not be counted
    ((1, 8, 8, 8), 64, 64, True),         # split-K: statistics come from the reduce kernel
    ((2, 8, 8, 8), 1, 4, False),          # the first layer
])
def test_conv3_epilogue_statistics(dev, shape, Cin, Cout, residual):
    epilogue_statistics_case(dev, shape, Cin, Cout, residual)


def epilogue_statistics_case(dev, shape, Cin, Cout, residual):
    """As test_batch_norm_statistics_from_the_conv_epilogue for the 5^3 kernels, same tolerances: the epilogue's partial sums
    finalize to the moments of the stored tensor, and the normalised output equals the stream-statistics path's.  (Also run at the
    sizes of the 128^3 step by tests/test_hip_unet_fullsize.py.)"""
    from vnet_tensorflow_amd import ops
    gen = torch.Generator().manual_seed(Cin * 7 + Cout)
    B, D, H, W = shape
    x = (torch.randn(B, D, H, W, Cin, generator=gen) * 1.5 + 0.3).to(dev)
    w = (torch.randn(3, 3, 3, Cin, Cout, generator=gen) * 0.05).to(dev)
    b = torch.randn(Cout, generator=gen).to(dev)
    r = (torch.randn(B, D, H, W, Cout, generator=gen) * 2.0).to(dev) if residual else None
    gamma, beta = (torch.rand(Cout, generator=gen) + 0.5).to(dev), torch.randn(Cout, generator=gen).to(dev)
    outs = {}
    try:
        for fused in (True, False):
            ops.set_epilogue_bn_stats(fused, fp32_direct=True)
            mm, mv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
            with torch.no_grad():
                y = ops.conv(x, w, b, 3, 1, bn_stats=True, bn_residual=r)
                assert (getattr(y, "_vnet_stats", None) is not None) == fused
                z, mean, invstd = ops.bn_act(y, gamma, beta, "relu", None, r, False, mm, mv, want_stats=True)
            outs[fused] = (y.clone(), z.clone(), mean.clone(), invstd.clone(), mm.clone(), mv.clone())
    finally:
        ops.set_epilogue_bn_stats(True, fp32_direct=True)
    yf, zf, mean, invstd, mm, mv = outs[True]
    assert torch.equal(yf, outs[False][0])
    s = yf.double() + (r.double() if residual else 0.0)
    mu, var = s.mean(dim=(0, 1, 2, 3)), s.var(dim=(0, 1, 2, 3), unbiased=False)
    check_close("mean", mean, mu.cpu().numpy(), 1e-6, atol=1e-6)
    check_close("invstd", invstd, (1.0 / torch.sqrt(var + 1e-3)).cpu().numpy(), 1e-6)
    check_close("normalised output", zf, outs[False][1].cpu().numpy(), 2e-6)
    check_close("moving mean", mm, (0.01 * mu).cpu().numpy(), 1e-5, atol=1e-7)
    check_close("moving variance", mv, (0.99 + 0.01 * var).cpu().numpy(), 1e-6)


# ---- 2. max-pooling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 8, 8, 8, 4), (2, 5, 7, 9, 3), (2, 6, 10, 12, 16), (1, 7, 4, 13, 20), (1, 32, 32, 32, 16), (2, 3, 2, 5, 4)])
def test_max_pool_is_bit_identical_to_torch(dev, shape):
    from vnet_tensorflow_amd import ops
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen)                              # tie-free
    xc = x.clone().requires_grad_(True)
    yc = torch.nn.functional.max_pool3d(xc.permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1)
    dy = torch.randn(*yc.shape, generator=gen)
    yc.backward(dy)
    xg = x.to(dev).requires_grad_(True)
    y = ops.max_pool2(xg)
    assert tuple(y.shape) == tuple(yc.shape)
    assert torch.equal(y.detach().cpu(), yc.detach())
    y.backward(dy.to(dev))
    assert torch.equal(xg.grad.cpu(), xc.grad)


def test_max_pool_ties_go_to_the_first_maximum(dev):
    from vnet_tensorflow_amd import ops
    for C in (1, 4):
        x = np.zeros((1, 2, 2, 2, C), np.float32)
        x[0, 0, 1, 1] = x[0, 1, 0, 0] = x[0, 1, 1, 1] = 5.0
        xg = g(x, dev).requires_grad_(True)
        y = ops.max_pool2(xg)
        y.backward(torch.full_like(y, 2.0))
        want = np.zeros_like(x); want[0, 0, 1, 1] = 2.0
        assert float(y.max()) == 5.0 and np.array_equal(xg.grad.cpu().numpy(), want)
        xg = g(np.zeros((1, 3, 2, 2, C), np.float32), dev).requires_grad_(True)      # all tied + a trailing plane
        y = ops.max_pool2(xg)
        y.backward(torch.ones_like(y))
        want = np.zeros((1, 3, 2, 2, C), np.float32); want[0, 0, 0, 0] = 1.0
        assert np.array_equal(xg.grad.cpu().numpy(), want)


def test_max_pool_accumulates_into_the_skip_gradient(dev):
    """vnet_maxpool2_bwd(accum = 1): dx += the pooling gradient, bit-identical to a separate add."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 5, 8, 8, generator=gen).to(dev)
    y = torch.empty(2, 3, 2, 4, 8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    assert L.vnet_maxpool2_fwd(x.data_ptr(), y.data_ptr(), 8, 2, 6, 5, 8, s) == 0
    dy, prev = torch.randn(2, 3, 2, 4, 8, generator=gen).to(dev), torch.randn(2, 6, 5, 8, 8, generator=gen).to(dev)
    dx, acc = torch.empty_like(x), prev.clone()
    assert L.vnet_maxpool2_bwd(dy.data_ptr(), x.data_ptr(), y.data_ptr(), dx.data_ptr(), 8, 2, 6, 5, 8, 0, s) == 0
    assert L.vnet_maxpool2_bwd(dy.data_ptr(), x.data_ptr(), y.data_ptr(), acc.data_ptr(), 8, 2, 6, 5, 8, 1, s) == 0
    assert torch.equal(acc, prev + dx)
    assert L.vnet_maxpool2_fwd(x.data_ptr(), y.data_ptr(), 8, 2, 1, 5, 8, s) == -1          # an axis shorter than the window


# ---- 3. the whole network ----------------------------------------------------------------------------------------------------------
def _gtol(name):
    return 1e-3 if name.endswith("weights") else 5e-3


def _unet(dev, cfg, values, shape):
    from vnet_tensorflow_amd import networks
    cin, K, C, levels, convs, bottom = cfg
    net = networks.UNet(K, 0.0, C, levels, convs, bottom, True, "relu", device=dev)
    net.variables.values = values
    return net.build(shape)


def _check_network(dev, tag, cfg, values, x, lab, ref):
    """Forward + loss + backward of the product against the oracle's `ref`, at the bounds of test_small_network_golden; prints every
    figure before it asserts."""
    from vnet_tensorflow_amd import ops
    net = _unet(dev, cfg, values, x.shape)
    logits = net.GetNetwork(g(x, dev))
    loss, _, _, _ = ops.softmax_loss(logits, g(lab, dev, torch.int32), "sorensen")
    loss.backward()
    worst = {}
    for n, p in net.named_parameters():
        r = ref["grads"][n]
        if np.linalg.norm(r) < 1e-7:          # conv biases in front of a batch-norm: analytically zero
            assert p.grad is None or np.abs(p.grad.cpu().numpy()).max() < 1e-4, n
            continue
        worst[n] = rel_l2(p.grad.cpu().numpy(), r)
    wn = max(worst, key=lambda n: worst[n] / _gtol(n))
    print("%s: logits rel-L2 %.3e max-abs %.3e | loss err %.3e | worst gradient %s rel-L2 %.3e (bound %.0e)" % (
        tag, rel_l2(logits.detach().cpu().numpy(), ref["logits"]), np.abs(logits.detach().cpu().numpy() - ref["logits"]).max(),
        abs(float(loss.detach()) - ref["loss"]), wn, worst[wn], _gtol(wn)))
    check_close(tag + " logits", logits, ref["logits"], 1e-4, atol=1e-3)
    assert abs(float(loss.detach()) - ref["loss"]) < 1e-5, (float(loss.detach()), ref["loss"])
    for n, e in worst.items():
        assert e < _gtol(n), (n, e)
    return net


@pytest.mark.parametrize("compute", ["fp32", "fp32_split3"])
@pytest.mark.parametrize("case", ["c1k2", "c3k3", "odd"])
def test_unet_fixture_configurations(dev, case, compute):
    from vnet_tensorflow_amd import ops
    z, cfg, names, trainable, shapes, values = load_fixture(case)
    onet, ps = make_oracle(cfg, names, trainable, values)
    x, lab = z["x"], z["labels"].astype(np.int32)[..., None]
    ref = O.run_step(x.astype(np.float64), lab, onet, "sorensen")
    assert np.abs(ref["logits"] - z["logits"]).max() < 1e-10
    ops.set_compute_dtype(compute)
    try:
        net = _check_network(dev, "unet %s %s" % (case, compute), cfg, values, x, lab, ref)
    finally:
        ops.set_compute_dtype("fp32")
    for n in ps.state:                         # moving statistics after the step's update ops
        check_close(n, net.variables.buffers[n], z["u:" + n], 1e-4, atol=1e-6)


@pytest.mark.parametrize("compute", ["fp32", "fp32_split3"])
def test_unet_32cube_c16_l3(dev, compute):
    from vnet_tensorflow_amd import ops
    cfg = (1, 2, 16, 3, 2, 2)
    x, lab = O.synthetic_batch(1, 32, 1, 2, seed=3100)
    ps = O.ParamStore(rng=np.random.default_rng(31), perturb=0.1)
    onet = U.UNetOracle(2, 0.0, 16, 3, 2, 2, "relu", ps)
    ref = O.run_step(x.astype(np.float64), lab, onet, "sorensen")
    ops.set_compute_dtype(compute)
    try:
        ops.profile_start()
        try:
            _check_network(dev, "unet 32^3 c16 l3 %s" % compute, cfg, {k: v.v for k, v in ps.vars.items()}, x, lab, ref)
        finally:
            recs = ops.profile_stop()
    finally:
        ops.set_compute_dtype("fp32")
    tags = set(r[0] for r in recs)
    assert any(t.startswith("conv k3 s1 ") for t in tags) and any(t.startswith("wgrad k3 s1 ") for t in tags), sorted(tags)
    assert any(t.startswith("maxpool2 fwd") for t in tags) and any(t.startswith("maxpool2 bwd") for t in tags), sorted(tags)
    assert not any(t.startswith(("conv-x3", "wgrad-x3", "conv k5", "wgrad k5")) for t in tags), sorted(tags)


# ---- 4. training ---------------------------------------------------------------------------------------------------------------------
def test_unet_training_steps_match_oracle_adam(dev):
    """Three TF-form Adam steps track the oracle at the loss bound of test_training_steps_match_oracle_adam (2e-5); then the loss
    decreases over 30 steps on the fixed batch."""
    from vnet_tensorflow_amd import ops, optim
    ps = O.ParamStore(rng=np.random.default_rng(9), perturb=0.1)
    onet = U.UNetOracle(2, 0.0, 4, 2, 2, 2, "relu", ps)
    x, lab = O.synthetic_batch(2, 16, 1, 2, seed=4000)
    onet.GetNetwork(x.astype(np.float64))
    net = _unet(dev, (1, 2, 4, 2, 2, 2), {k: v.v for k, v in ps.vars.items()}, x.shape)
    flat = optim.FlatParams(net.named_parameters())
    opt = optim.AdamOptimizer(flat)
    adam = O.TFAdam()
    tx, tl = g(x, dev), g(lab, dev, torch.int32)
    losses = []
    for step in range(30):
        lr = optim.exponential_decay(1e-3, step, 100, 0.99)
        flat.zero_grad()
        loss, _, _, _ = ops.softmax_loss(net.GetNetwork(tx), tl, "sorensen")
        loss.backward()
        opt.apply(lr)
        losses.append(float(loss))
        if step < 3:
            ref = O.run_step(x.astype(np.float64), lab, onet, "sorensen")
            params = adam.step({k: v.v for k, v in ps.vars.items()}, ref["grads"], lr)
            for k, v in params.items():
                ps.vars[k].v = v
            print("step %d: loss %.7f oracle %.7f" % (step, losses[-1], ref["loss"]))
            assert abs(losses[-1] - ref["loss"]) < 2e-5, (step, losses[-1], ref["loss"])
            if step == 2:
                for n, p in net.named_parameters():
                    check_close("after 3 steps " + n, p, ps.vars[n].v, 2e-3, atol=2e-4)
    assert losses[-1] < losses[0], losses


def _cfg(P=16, dropout=0.0, compute="fp32", cin=1, K=2, nch=4, levels=2):
    return {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": "synthetic", "TestingDataDirectory": "synthetic",
                 "ImageFilenames": ["image%d.npy" % i for i in range(cin)], "LabelFilename": "label.npy", "Synthetic": {"Cases": 4}},
        "SegmentationClasses": list(range(K)), "BatchSize": 2, "PatchShape": [P] * 3, "ComputeDtype": compute,
        "Networks": {"Name": "UNet", "Dropout": dropout, "NumChannel": nch, "NumLevels": levels, "NumConvolutions": 2, "BottomConvolutions": 2},
        "Loss": {"Name": "sorensen"},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.9, "Steps": 3}},
        "EvaluationSetting": {}}}


def _run_steps(dev, graph, steps, monkeypatch, **kw):
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd.model import image2label
    monkeypatch.setenv("VNET_STEP_GRAPH", "1" if graph else "0")
    cfg = _cfg(**kw)
    T = cfg["TrainingSetting"]
    cin, K, P = len(T["Data"]["ImageFilenames"]), len(T["SegmentationClasses"]), T["PatchShape"][0]
    np.random.seed(7)
    m = image2label(None, cfg, device=dev, verbose=False)
    try:
        m.read_config()
        m.build_model_graph()
        m._setup_training()
        batches = [O.synthetic_batch(2, P, cin, K, seed=40 + i) for i in range(2)]
        batches = [(torch.from_numpy(x).to(dev), torch.from_numpy(l).to(dev)) for x, l in batches]
        losses = [float(m.train_step(*batches[i % 2])) for i in range(steps)]
        torch.cuda.synchronize()
        assert (m._graph_mode() == "whole") == graph
        if graph:
            assert m._graphs is not None and len(m._graphs) == 1, "the step was never captured"
    finally:
        ops.set_compute_dtype("fp32")
    return losses, m.flat.data.clone(), {k: v.clone() for k, v in m.network.state_dict().items()}, m


@pytest.mark.parametrize("kw", [dict(), dict(dropout=0.05, cin=2, K=3, nch=8)], ids=["adam", "dropout-c2k3"])
def test_unet_graph_replay_is_bit_identical_to_eager(dev, monkeypatch, kw):
    """On the pattern of test_hip_step_graph.py: 2 eager warm-up steps + capture + 4 replays against 6 eager steps, bit for bit."""
    a = _run_steps(dev, True, 6, monkeypatch, **kw)
    b = _run_steps(dev, False, 6, monkeypatch, **kw)
    assert a[0] == b[0], (a[0], b[0])
    assert torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert a[0][-1] < a[0][0]


# ---- 6. sliding-window evaluation ---------------------------------------------------------------------------------------------------
def test_unet_sliding_window_evaluate(dev):
    """On the pattern of test_sliding_window_evaluate: model.evaluate_single_3D on a volume larger than the patch equals the oracle's
    forward stitched the same way (patch enumeration with stride, last patch clamped, duplicated last batch; model.py:866-937)."""
    import math
    from vnet_tensorflow_amd import model as M
    cfg = _cfg()
    cfg["TrainingSetting"]["BatchSize"] = 1
    cfg["EvaluationSetting"] = {"Stride": [8, 12, 16], "BatchSize": 2, "ProbabilityOutput": True}
    m = M.image2label(None, cfg, device=dev, verbose=False)
    m.read_config()
    m.build_model_graph()
    vol, _ = O.synthetic_batch(1, 24, 1, 2, seed=77)
    vol = vol[0][:, :22, :20]
    label, softmax = m.evaluate_single_3D(vol)
    ps, st, dims = [16, 16, 16], [8, 12, 16], vol.shape[:3]
    nums = [int(math.ceil((dims[a] - ps[a]) / float(st[a]))) + 1 for a in range(3)]
    idxs = [[min(n * st[a], dims[a] - ps[a]) for a, n in enumerate((i, j, k))]
            for i in range(nums[0]) for j in range(nums[1]) for k in range(nums[2])]
    groups = [idxs[i:i + 2] for i in range(0, len(idxs), 2)]
    groups.append(groups[-1])
    values = {n: p.detach().cpu().numpy().astype(np.float64) for n, p in m.network.named_parameters()}
    onet = U.UNetOracle(2, 0.0, 4, 2, 2, 2, "relu", O.ParamStore(values=values))
    acc, cnt = np.zeros(dims + (2,), np.float64), np.zeros(dims, np.float64)
    for grp in groups:
        batch = np.stack([vol[s[0]:s[0] + 16, s[1]:s[1] + 16, s[2]:s[2] + 16] for s in grp]).astype(np.float64)
        sm = O.softmax(onet.GetNetwork(batch)).v
        for s, p_ in zip(grp, sm):
            acc[s[0]:s[0] + 16, s[1]:s[1] + 16, s[2]:s[2] + 16] += p_
            cnt[s[0]:s[0] + 16, s[1]:s[1] + 16, s[2]:s[2] + 16] += 1
    prob = acc / cnt[..., None]
    err = np.abs(np.moveaxis(softmax, 0, -1) - prob).max()
    print("sliding window: max |softmax - oracle| = %.3e" % err)
    assert err < 1e-4, err
    srt = np.sort(prob, axis=-1)
    sure = (srt[..., -1] - srt[..., -2]) > 1e-4
    assert (label == acc.argmax(-1))[sure].all()


# ---- 7. checkpoints --------------------------------------------------------------------------------------------------------------------
def test_unet_checkpoint_round_trip(dev, monkeypatch, tmp_path):
    from vnet_tensorflow_amd import model as M
    _, _, state, m = _run_steps(dev, False, 2, monkeypatch)
    m.ckpt_dir = str(tmp_path / "ckpt")
    x = torch.from_numpy(O.synthetic_batch(2, 16, 1, 2, seed=90)[0]).to(dev)
    with torch.no_grad():
        before = m.forward(x)[0].clone()
    state = {k: v.clone() for k, v in m.network.state_dict().items()}      # (the forward moved the moving averages)
    m.save_checkpoint()
    prefix = m.save_tf_checkpoint()
    names = list(m.network.state_dict().keys())
    for loader in ("torch", "tf"):
        np.random.seed(11)
        m2 = M.image2label(None, _cfg(), device=dev, verbose=False)
        m2.read_config()
        m2.build_model_graph()
        m2._setup_training()
        m2.ckpt_dir = m.ckpt_dir
        if loader == "torch":
            m2.load_checkpoint()
        else:
            m2.load_tf_checkpoint(prefix)
        assert list(m2.network.state_dict().keys()) == names
        assert any(n == "unet/decoder/level_1/batch_normalization_2/moving_variance" for n in names)
        for k, v in m2.network.state_dict().items():
            assert torch.equal(v, state[k]), (loader, k)
        with torch.no_grad():
            # (batch statistics are always used, so the forward also moves the moving averages: compare the logits only)
            assert torch.equal(m2.forward(x)[0], before), loader
