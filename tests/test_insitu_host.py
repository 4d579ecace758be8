"""CPU: the oracle adapters of tests/insitu.py (what tests/test_hip_insitu_backward.py holds the HIP step to) against an independent
restatement -- oracle/torch_ref.py or plain torch-CPU float64 autograd -- on small random inputs, at the 1e-10 the two oracles hold
to each other in tests/test_oracle.py.  Also the recorder's bookkeeping that needs no device: the call-site scan and the bounds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as TR
from oracle import vnet_oracle as O
from tests import insitu as S

TOL = 1e-10


def _t(a, grad=True):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def _close(name, got, ref, floor=0.0):
    """floor: what the error is measured against where the reference is analytically zero (a beta in front of another batch-norm)."""
    got = np.asarray(got, dtype=np.float64)
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) / (max(float(np.abs(ref).max()), floor) + 1e-300)
    assert err <= TOL, "%s: %.3e" % (name, err)


def _against_torch(name, adapter, A, dy, torch_fn, tensors):
    """adapter(A, dy) against torch autograd of torch_fn(**tensors as float64 leaves) seeded with dy."""
    A = dict(A)
    A.setdefault("_b16", False)
    fwd, contrib = adapter(A, dy)
    leaves = {k: _t(A[k]) for k in tensors}
    y = torch_fn(**leaves)
    ys = y if isinstance(y, tuple) else (y,)
    fs = fwd if isinstance(fwd, tuple) else (fwd,)
    for i, (a, b) in enumerate(zip(fs, ys)):
        _close("%s forward[%d]" % (name, i), a, b)
    dys = dy if isinstance(dy, tuple) else (dy,)
    torch.autograd.backward(list(ys), [torch.tensor(np.asarray(d, np.float64)).reshape(v.shape) for d, v in zip(dys, ys)])
    assert set(contrib) - {"_abs"} == set(tensors), (name, sorted(contrib), sorted(tensors))
    for k, scale in contrib.get("_abs", {}).items():         # per channel, sum of magnitudes >= |sum|: the scale of a column sum's error
        if scale is not None:
            assert k in tensors and np.all(np.asarray(scale) * (1 + 1e-12) >= np.abs(contrib[k])), (name, k)
    floor = 1e-4 * sum(float(np.abs(d).sum()) for d in dys)          # (the inputs are O(1): a real gradient here is far above this)
    for k in tensors:
        _close("%s d%s" % (name, k), contrib[k], leaves[k].grad, floor)
    return contrib


def _bn(x, g, b):
    return TR.batch_norm(x, g, b)


def _act(z, kind, alpha):
    if kind == "prelu":
        return TR.prelu(z, alpha)
    if kind == "relu":
        return torch.relu(z)
    if kind == "lrelu":
        return F.leaky_relu(z, 0.2)
    return z


def _params(rng, C, n):
    out = {}
    for i in range(1, n + 1):
        out["g%d" % i], out["b%d" % i] = 1 + 0.3 * rng.standard_normal(C), 0.3 * rng.standard_normal(C)
    return out


@pytest.mark.parametrize("ks,stride,two", [(5, 1, False), (5, 1, True), (3, 1, True), (2, 2, False)])
def test_conv_adapter_and_the_two_source_split(ks, stride, two):
    rng = np.random.default_rng(ks + 10 * two)
    C0, C1, Co = 3, (2 if two else 0), 4
    A = dict(x0=rng.standard_normal((2, 5, 6, 7, C0)), x1=rng.standard_normal((2, 5, 6, 7, C1)) if two else None,
             w=rng.standard_normal((ks,) * 3 + (C0 + C1, Co)) * 0.2, b=rng.standard_normal(Co), stride=stride)
    y0, _ = S.a_conv(dict(A, _b16=False), None)
    dy = rng.standard_normal(y0.shape)

    def fn(x0, w, b, x1=None):
        return TR.convolution(x0 if x1 is None else torch.cat((x0, x1), -1), w, b, stride)
    c = _against_torch("conv", S.a_conv, A, dy, fn, ("x0", "x1", "w", "b") if two else ("x0", "w", "b"))
    if two:                                # the split hands each source its own channels of the one backward-data result
        assert c["x0"].shape[-1] == C0 and c["x1"].shape[-1] == C1


def test_conv_adapter_bf16_storage_rounds_the_filter_and_keeps_dw_straight_through():
    rng = np.random.default_rng(3)
    x = O.round_bf16(rng.standard_normal((1, 4, 5, 6, 8)))
    x[..., 3:] = 0.0                                            # the cast network input: 3 real channels, zero-padded to 8
    w, b = rng.standard_normal((5, 5, 5, 3, 4)) * 0.2, rng.standard_normal(4)
    dy = O.round_bf16(rng.standard_normal((1, 4, 5, 6, 4)))
    fwd, c = S.a_conv(dict(x0=x, x1=None, w=w, b=b, stride=1, _b16=True, _req={"x0": False}), dy)
    xt, wt, bt = _t(x[..., :3]), _t(w), _t(b)
    TR.STORAGE = "bf16"
    try:
        y = TR.convolution(xt, wt, bt, 1)
    finally:
        TR.STORAGE = None
    _close("fwd", fwd, y)
    y.backward(torch.tensor(dy))
    _close("dw", c["w"], wt.grad)
    _close("db", c["b"], bt.grad)
    assert "x0" not in c


@pytest.mark.parametrize("osp", [(6, 8, 10), (5, 7, 9)])
def test_transposed_conv_adapter_even_and_odd_extent(osp):
    rng = np.random.default_rng(sum(osp))
    coarse = tuple(-(-v // 2) for v in osp)
    A = dict(x=rng.standard_normal((2,) + coarse + (6,)), w=rng.standard_normal((2, 2, 2, 3, 6)) * 0.3, b=rng.standard_normal(3),
             out_spatial=osp)
    dy = rng.standard_normal((2,) + osp + (3,))
    _against_torch("up", S.a_conv_transpose2, A, dy, lambda x, w, b: TR.deconvolution(x, w, b, osp, 2), ("x", "w", "b"))


def test_input_conv_adapter():
    rng = np.random.default_rng(5)
    C, Co = 4, 4
    img = rng.standard_normal((2, 5, 6, 7, 1)) * 40 + 100
    mean = np.full(C, img.mean())
    invstd = np.full(C, 1.0 / np.sqrt(img.var() + 1e-3))
    A = dict(img=img, gamma=1 + 0.3 * rng.standard_normal(C), beta=0.3 * rng.standard_normal(C), mean=mean, invstd=invstd,
             w=rng.standard_normal((5, 5, 5, C, Co)) * 0.1, b=rng.standard_normal(Co))
    dy = rng.standard_normal((2, 5, 6, 7, Co))
    ti, tm, ts = torch.tensor(img), torch.tensor(mean), torch.tensor(invstd)

    def fn(gamma, beta, w, b):             # the statistics are constants here, exactly as the op receives them
        return TR.convolution((ti.expand(-1, -1, -1, -1, C) - tm) * ts * gamma + beta, w, b, 1)
    _against_torch("input block", S.a_input_conv, A, dy, fn, ("gamma", "beta", "w", "b"))


@pytest.mark.parametrize("act,res,tile", [("prelu", True, False), ("relu", False, False), (None, False, True), ("lrelu", True, False)])
def test_bn_act_adapter(act, res, tile):
    rng = np.random.default_rng(len(str(act)) + res)
    C = 6
    shp = (2, 4, 5, 3, 1 if tile else C)
    A = dict(x=rng.standard_normal(shp) * 2 + 0.5, residual=rng.standard_normal(shp) if res else None, gamma=1 + 0.3 * rng.standard_normal(C),
             beta=0.3 * rng.standard_normal(C), alpha=0.1 + 0.05 * rng.standard_normal(C) if act == "prelu" else None, act=act, tile=tile)
    dy = rng.standard_normal(shp[:-1] + (C,))

    def fn(x, gamma, beta, residual=None, alpha=None):
        s = x.expand(-1, -1, -1, -1, C) if tile else x
        return _act(_bn(s if residual is None else s + residual, gamma, beta), act, alpha)
    names = ["x", "gamma", "beta"] + (["residual"] if res else []) + (["alpha"] if act == "prelu" else [])
    _against_torch("bn_act", S.a_bn_act, A, dy, fn, tuple(names))


def _chain(kind, x, p, act, alpha):
    if kind == 0:
        y1 = _bn(x, p["g1"], p["b1"])
        z = _bn(y1 + _bn(y1, p["g2"], p["b2"]), p["g3"], p["b3"])
    elif kind == 1:
        z = _bn(x + _bn(x, p["g1"], p["b1"]), p["g2"], p["b2"])
    else:
        z = _bn(x, p["g1"], p["b1"])
    return _act(z, act, alpha)


@pytest.mark.parametrize("kind,act", [(0, "prelu"), (1, "prelu"), (0, "relu"), (1, None)])
def test_bn_chain_adapter(kind, act):
    rng = np.random.default_rng(kind + 7)
    C = 5
    P = _params(rng, C, 3 if kind == 0 else 2)
    A = dict(P, x=rng.standard_normal((2, 3, 4, 5, C)) * 1.5 + 0.3, kind=kind, act=act,
             alpha=0.1 + 0.05 * rng.standard_normal(C) if act == "prelu" else None)
    if kind == 1:
        A.update(g3=None, b3=None)
    dy = rng.standard_normal(A["x"].shape)

    def fn(x, alpha=None, **p):
        return _chain(kind, x, p, act, alpha)
    names = ["x"] + sorted(P) + (["alpha"] if act == "prelu" else [])
    _against_torch("bn_chain %d" % kind, S.a_bn_chain, A, dy, fn, tuple(names))


@pytest.mark.parametrize("kind,res", [(0, False), (1, False), (-1, True), (-1, False)])
def test_bn_head_adapter(kind, res):
    rng = np.random.default_rng(kind + 11 + res)
    C, K = 6, 3
    P = _params(rng, C, {0: 3, 1: 2, -1: 1}[kind])
    A = dict({"g2": None, "b2": None, "g3": None, "b3": None}, **P)
    A.update(x=rng.standard_normal((2, 3, 4, 5, C)), residual=rng.standard_normal((2, 3, 4, 5, C)) if res else None, kind=kind, act="prelu",
             alpha=0.1 + 0.05 * rng.standard_normal(C), w=rng.standard_normal((1, 1, 1, C, K)) * 0.3, b=rng.standard_normal(K))
    dy = rng.standard_normal((2, 3, 4, 5, K))

    def fn(x, w, b, alpha, residual=None, **p):
        y = _chain(kind, x if residual is None else x + residual, p, "prelu", alpha)
        return y @ w[0, 0, 0] + b
    names = ["x", "w", "b", "alpha"] + sorted(P) + (["residual"] if res else [])
    _against_torch("bn_head %d" % kind, S.a_bn_head, A, dy, fn, tuple(names))


def test_bn_concat_adapter():
    rng = np.random.default_rng(13)
    C0, C1 = 4, 3
    A = dict(x0=rng.standard_normal((2, 3, 4, 5, C0)), x1=rng.standard_normal((2, 3, 4, 5, C1)) * 2 + 1,
             gamma=1 + 0.3 * rng.standard_normal(C0 + C1), beta=0.3 * rng.standard_normal(C0 + C1))
    dy = (rng.standard_normal(A["x0"].shape), rng.standard_normal(A["x1"].shape))

    def fn(x0, x1, gamma, beta):
        y = _bn(torch.cat((x0, x1), -1), gamma, beta)
        return y[..., :C0], y[..., C0:]
    _against_torch("bn_concat", S.a_bn_concat, A, dy, fn, ("x0", "x1", "gamma", "beta"))


def test_head_conv_and_activation_adapters():
    rng = np.random.default_rng(17)
    A = dict(x=rng.standard_normal((2, 3, 4, 5, 6)), w=rng.standard_normal((1, 1, 1, 6, 3)), b=rng.standard_normal(3))
    _against_torch("head", S.a_head_conv, A, rng.standard_normal((2, 3, 4, 5, 3)), lambda x, w, b: x @ w[0, 0, 0] + b, ("x", "w", "b"))
    A = dict(x=rng.standard_normal((2, 3, 4, 5, 6)), alpha=0.1 + 0.05 * rng.standard_normal(6), act="prelu")
    _against_torch("prelu", S.a_activation, A, rng.standard_normal(A["x"].shape), lambda x, alpha: TR.prelu(x, alpha), ("x", "alpha"))
    A = dict(x=rng.standard_normal((2, 3, 4, 5, 6)), alpha=None, act="lrelu")
    _against_torch("lrelu", S.a_activation, A, rng.standard_normal(A["x"].shape), lambda x: F.leaky_relu(x, 0.2), ("x",))


def test_max_pool_adapter_first_maximum_on_ties_and_odd_extent():
    rng = np.random.default_rng(19)
    x = rng.standard_normal((2, 5, 6, 7, 3))                    # odd axes floor: the trailing plane / column gets no gradient
    A = dict(x=x)
    dy = rng.standard_normal((2, 2, 3, 3, 3))
    c = _against_torch("max pool", S.a_max_pool2, A, dy,
                       lambda x: F.max_pool3d(x.permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1), ("x",))
    assert not c["x"][:, 4].any() and not c["x"][:, :, :, 6].any()
    # ties: the whole gradient of a window goes to its first maximum in (z, y, x) scan order (test_max_pool_ties_go_to_the_first_maximum)
    x = np.zeros((1, 2, 2, 2, 1))
    x[0, 0, 1, 0, 0] = x[0, 1, 0, 1, 0] = 3.0
    _, c = S.a_max_pool2(dict(x=x), np.full((1, 1, 1, 1, 1), 2.5))
    want = np.zeros_like(x)
    want[0, 0, 1, 0, 0] = 2.5
    assert np.array_equal(c["x"], want)


def test_dropout_adapter_uses_the_mask_the_kernel_drew():
    rng = np.random.default_rng(23)
    x = rng.standard_normal((2, 3, 4, 5, 6))
    x[0, 0, 0, 0, :3] = 0.0                                     # a zero input is "kept" whatever the mask: its output is 0 either way
    keep = rng.random(x.shape) > 0.3
    out = x * keep / 0.7
    dy = rng.standard_normal(x.shape)
    fwd, c = S.a_dropout(dict(x=x, rate=0.3, _out=out), dy)
    _close("fwd", fwd, out)
    nz = x != 0
    _close("dx", c["x"][nz], (dy * keep / 0.7)[nz])


@pytest.mark.parametrize("loss", ["sorensen", "mixed_weighted_jaccard", "weighted_xent", "jaccard"])
def test_loss_adapter_with_labels_outside_the_classes(loss):
    rng = np.random.default_rng(29)
    K = 3
    z = rng.standard_normal((2, 3, 4, 5, K))
    lab = rng.integers(0, K, size=(2, 3, 4, 5, 1)).astype(np.int32)
    lab[0, 0, 0, :2, 0] = (K, -1)                               # tf.one_hot: all-zero rows
    wts = [0.3, 0.7, 1.0]
    for labels in (lab, lab[..., 0]):                            # [B,D,H,W,1] and [B,D,H,W]
        A = dict(logits=z, labels=labels, loss_name=loss, weights=wts, alpha=0.5)
        _against_torch(loss, S.a_softmax_loss, A, np.asarray(1.7),
                       lambda logits: TR.loss_head(logits, torch.from_numpy(lab), loss, wts, 0.5)[0], ("logits",))


def test_call_sites_are_read_from_the_code_and_every_op_has_an_adapter():
    net, model = S.op_call_sites()
    assert {"conv", "input_conv", "conv_transpose2", "bn_act", "bn_chain", "bn_head", "bn_concat", "bn_update_only", "head_conv",
            "max_pool2", "dropout", "activation", "fork", "cut", "cast_input"} <= net
    assert "softmax_loss" in model
    assert not [n for n in net if n not in S.ADAPTERS and n not in S.STRUCTURAL]
    assert set(S.TOL) == set(S.ADAPTERS)


def test_two_consumer_bf16_bound():
    """RNE(RNE(a) + b) passes, in either order; a dropped, a doubled or a twice-rounded-then-scaled contribution does not.  The
    relative form 2^-9 (max|c_i| + |total|) is NOT met by the exact double rounding (half an ulp is up to 2^-8 of the value): the
    ulp form is what the device test uses."""
    rng = np.random.default_rng(31)
    a, b = rng.standard_normal(4096), rng.standard_normal(4096) * 0.3
    for first, second in ((a, b), (b, a)):
        got = O.round_bf16(O.round_bf16(first) + second)
        assert S.bf16_two_consumer_excess(got, [a, b]) <= 1.0
        assert 1.0 < S.bf16_two_consumer_excess(got, [a, b], literal=True) <= 2.0
    assert S.bf16_two_consumer_excess(O.round_bf16(a), [a, b]) > 1.0
    assert S.bf16_two_consumer_excess(O.round_bf16(a + 2 * b), [a, b]) > 1.0
    assert S.bf16_two_consumer_excess(O.round_bf16((a + b) * (1 + 2.0 ** -6)), [a, b]) > 1.0
    h = S.half_ulp_bf16(np.array([1.0, 1.99, 2.0, 0.0, -3.0]))
    assert np.array_equal(h, [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0, 2.0 ** -7])
