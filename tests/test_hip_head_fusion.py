"""-m gpu: the decoder's last batch-norm with the 1x1x1 head folded in (include/vnet_hip_head.h, ops.bn_head) against the unfused
sequence it replaces and against the fp64 oracle (oracle/vnet_oracle.py).

Summation order: KEPT, forward and backward.
* Forward: a voxel's logit is the bias plus its channel quads' shares added in quad order, the expression of head_fwd_kernel, and y
  is bn_act_fwd_kernel's expression -- y and the logits must be BIT-IDENTICAL to vnet_bn_act_fwd + vnet_head_fwd, for every K.
* Backward: dy = dlogits W^T is head_bwd_kernel's fma chain, every thread sums the rows the unfused kernels give it in their order,
  the workgroup trees and the finalize are theirs.  For K = 2 (the arithmetic checked instruction by instruction against the
  unfused kernels' code) dgamma, dbeta, dalpha, dw, db and ds must be BIT-IDENTICAL to vnet_head_bwd + vnet_bn_act_bwd_reduce +
  vnet_bn_act_bwd_apply, and ops.bn_head in its default setting to bn_chain / bn_act + head_conv.  It matters: db is analytically 0
  in front of a batch-norm, its value is round-off, and Adam makes a full-size step of it.  For other K the compiler is free to
  contract the unfused kernels' products differently, so those are held to the bounds below.
* The optional statistics rows of the logits (set_head_fusion(stats=True)) group the voxels differently from vnet_bn_stats: bounds.
The bounds are those of the existing tests of the kernels replaced, each named where it is used:
  tests/test_hip_ops.py::_bn_act_case   y 5e-6; dx / dr 5e-5 (atol 1e-5); dgamma / dbeta / dalpha 2e-5
  tests/test_hip_ops.py::test_bn_chain  dx 5e-5 (atol 1e-5); dgamma 5e-5 (atol 1e-5); dbeta 2e-5 (atol 1e-6); dalpha 2e-5
  tests/test_hip_ops.py::test_head      logits, dw, db 2e-6 -- for the exact input, so the references here are fp64 products of the
                                        y the device computed
  tests/test_hip_ops.py::test_bn_stats_generic_path_is_deterministic   mean rtol 2e-6 + atol 2e-6, invstd rtol 5e-6"""
import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests.util import g, check_close

pytestmark = pytest.mark.gpu


def _act(y, act, A_):
    return O.prelu(y, A_) if act == "prelu" else O.relu(y) if act == "relu" else O.leaky_relu(y) if act == "lrelu" else y


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- the three entry points against the entry points they replace ---------------------------------------------------------------
NATIVE = [
    # (shape of the voxel grid, C, K, activation, residual)
    ((1, 128, 128, 128), 16, 2, "prelu", False),        # the 128^3 x 16 crop of the headline step
    ((1, 128, 128, 128), 16, 2, "prelu", True),
    ((1, 64, 128, 128), 8, 5, "relu", True),
    ((2, 5, 6, 7), 16, 2, "prelu", False),              # ragged: 420 voxels
    ((2, 5, 6, 7), 16, 5, "prelu", True),
    ((1, 3, 7, 11), 8, 2, "lrelu", False),              # 231 voxels
    ((1, 1, 1, 5), 8, 5, None, True),
    ((3, 9, 13, 17), 8, 2, "prelu", True),
    ((1, 31, 33, 67), 16, 5, "relu", False),            # more quads than one grid pass of 1024 workgroups, ragged tail
    ((1, 1, 2, 3), 16, 8, "prelu", False),
]


@pytest.mark.parametrize("shp,C,K,act,res", NATIVE)
def test_fused_passes_against_unfused_and_oracle(dev, shp, C, K, act, res):
    from vnet_tensorflow_amd import _lib, ops
    L = _lib.lib()
    P = ops._ptr
    rng = np.random.default_rng(sum(shp) + 10 * C + K)
    M = int(np.prod(shp))
    x = (rng.standard_normal(shp + (C,)) * 3.0 + 1.5).astype(np.float32)
    r = rng.standard_normal(shp + (C,)).astype(np.float32) if res else None
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    alpha = rng.uniform(0.05, 0.3, C).astype(np.float32)
    w = rng.standard_normal((C, K)).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    dl = rng.standard_normal(shp + (K,)).astype(np.float32)
    tx, tr, tg, tb, ta, tw, tbi, tdl = (g(a, dev) if a is not None else None for a in (x, r, gamma, beta, alpha, w, b, dl))
    a = ops.ACT[act]
    al = tb if a != 2 else ta                            # (a non-null pointer the kernels do not read without PRELU)
    s = ops._stream()
    E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    mean, invstd = E(C), E(C)
    nb = max(L.vnet_bn_ws_bytes(C), L.vnet_head_ws_bytes(C, K), L.vnet_bn_head_ws_bytes(C, K))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    assert L.vnet_bn_stats(P(tx), P(tr), 0, M, C, 1e-3, 0.99, P(mean), P(invstd), None, None, P(ws), nb, s) == 0
    bn = (P(mean), P(invstd), P(tg), P(tb), a, P(al))

    # the unfused sequence
    y0, lg0 = E(M, C), E(M, K)
    assert L.vnet_bn_act_fwd(P(tx), P(tr), 0, M, C, *bn, P(y0), s) == 0
    assert L.vnet_head_fwd(P(y0), P(tw), P(tbi), P(lg0), M, C, K, s) == 0
    dy0, dw0, db0 = E(M, C), E(C, K), E(K)
    assert L.vnet_head_bwd(P(y0), P(tw), P(tdl), P(dy0), P(dw0), P(db0), M, C, K, P(ws), nb, s) == 0
    dg0, dbt0, da0, ds0 = E(C), E(C), E(C), E(M, C)
    assert L.vnet_bn_act_bwd_reduce(P(dy0), P(tx), P(tr), 0, M, C, *bn, P(dg0), P(dbt0), P(da0), P(ws), nb, s) == 0
    assert L.vnet_bn_act_bwd_apply(P(dy0), P(tx), P(tr), 0, M, C, *bn, P(dbt0), P(dg0), float(M), None, P(ds0), s) == 0

    # the fused passes
    assert L.vnet_bn_head_ok(C, K) == 1
    rows = L.vnet_bn_head_stats_rows(M, C)
    assert 1 <= rows <= 1024
    y1, lg1, st = E(M, C), E(M, K), torch.full((rows, 2 * K), float("nan"), device=dev)
    assert L.vnet_bn_act_head_fwd(P(tx), P(tr), M, C, *bn, P(tw), P(tbi), K, P(y1), P(lg1), P(st), s) == 0
    lg2 = E(M, K)
    assert L.vnet_bn_act_head_fwd(P(tx), P(tr), M, C, *bn, P(tw), P(tbi), K, None, P(lg2), P(st), s) == 0      # y not stored
    dg1, dbt1, da1, dw1, db1, ds1 = E(C), E(C), E(C), E(C, K), E(K), E(M, C)
    assert L.vnet_bn_act_bwd_reduce_head(P(tdl), P(tw), K, P(tx), P(tr), M, C, *bn, P(dg1), P(dbt1), P(da1), P(dw1), P(db1),
                                         P(ws), nb, s) == 0
    assert L.vnet_bn_act_bwd_apply_head(P(tdl), P(tw), K, P(tx), P(tr), M, C, *bn, P(dbt1), P(dg1), float(M), None, P(ds1), s) == 0
    torch.cuda.synchronize()

    # forward: the bits of the unfused kernels (summation order kept)
    assert torch.equal(y1, y0), "y differs from vnet_bn_act_fwd"
    assert torch.equal(lg1, lg0) and torch.equal(lg2, lg0), "logits differ from vnet_bn_act_fwd + vnet_head_fwd"
    # the statistics rows, finalized by the unchanged vnet_bn_finalize_partial, against fp64 moments of the logits the device wrote
    m2, i2 = E(K), E(K)
    assert L.vnet_bn_finalize_partial(P(st), rows, K, float(M), 1e-3, 0.99, P(m2), P(i2), None, None, s) == 0
    l64 = _f64(lg1)
    np.testing.assert_allclose(_f64(m2), l64.mean(0), rtol=2e-6, atol=2e-6)          # test_bn_stats_generic_path_is_deterministic
    np.testing.assert_allclose(_f64(i2), 1.0 / np.sqrt(l64.var(0) + 1e-3), rtol=5e-6)

    # the fp64 oracle: batch-norm (+ residual) + activation + 1x1x1 convolution, seeded with dlogits
    X, G_, B_, A_ = O.Var(x.astype(np.float64)), O.Var(gamma.astype(np.float64)), O.Var(beta.astype(np.float64)), O.Var(alpha.astype(np.float64))
    R = O.Var(r.astype(np.float64)) if res else None
    yv = _act(O.batch_norm_train(O.add(X, R) if res else X, G_, B_), act, A_)
    W_, Bi = O.Var(w.astype(np.float64).reshape(1, 1, 1, C, K)), O.Var(b.astype(np.float64))
    O.backward(O.convolution(yv, W_, Bi, 1), dl.astype(np.float64))
    tag = "fused head %s C%d K%d %s res%d" % (shp, C, K, act, res)
    y64 = _f64(y1)
    check_close(tag + " y", y1.reshape(yv.v.shape), yv.v, 5e-6)                       # _bn_act_case
    check_close(tag + " logits", lg1, y64 @ w.astype(np.float64) + b, 2e-6)           # test_head
    check_close(tag + " dw", dw1, y64.T @ dl.reshape(-1, K).astype(np.float64), 2e-6)  # test_head
    check_close(tag + " db", db1, dl.reshape(-1, K).astype(np.float64).sum(0), 2e-6)   # test_head
    check_close(tag + " ds", ds1.reshape(X.g.shape), X.g, 5e-5, atol=1e-5)            # _bn_act_case
    check_close(tag + " dgamma", dg1, G_.g, 2e-5)
    check_close(tag + " dbeta", dbt1, B_.g, 2e-5)
    if act == "prelu":
        check_close(tag + " dalpha", da1, A_.g, 2e-5)
    if K == 2:                                           # the backward has the unfused kernels' bits (module docstring)
        for name, a1, a0 in (("dgamma", dg1, dg0), ("dbeta", dbt1, dbt0), ("dw", dw1, dw0), ("db", db1, db0), ("ds", ds1, ds0)):
            assert torch.equal(a1, a0), "%s %s: %d elements differ from the unfused kernels" % (tag, name, int((a1 != a0).sum()))
        if act == "prelu":
            assert torch.equal(da1, da0), tag + " dalpha differs from the unfused kernels"
    # and next to the unfused kernels' own results, at the same bounds
    check_close(tag + " ds vs unfused", ds1, _f64(ds0), 5e-5, atol=1e-5)
    check_close(tag + " dw vs unfused", dw1, _f64(dw0), 2e-6)
    check_close(tag + " db vs unfused", db1, _f64(db0), 2e-6)
    check_close(tag + " dgamma vs unfused", dg1, _f64(dg0), 2e-5)
    check_close(tag + " dbeta vs unfused", dbt1, _f64(dbt0), 2e-5)


def test_fused_passes_refuse_what_they_do_not_build(dev):
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    assert [L.vnet_bn_head_ok(C, K) for C, K in ((16, 2), (8, 8), (16, 1), (4, 2), (32, 2), (12, 2), (16, 9), (16, 0))] == [1, 1, 1, 0, 0, 0, 0, 0]
    one = torch.zeros(64, device=dev).data_ptr()
    assert L.vnet_bn_act_head_fwd(one, None, 4, 32, one, one, one, one, 0, None, one, None, 2, None, one, one, None) == -2
    assert L.vnet_bn_act_head_fwd(one, None, 4, 16, one, one, one, one, 2, None, one, None, 2, None, one, one, None) == -1      # PRELU, no alpha
    assert L.vnet_bn_act_bwd_reduce_head(one, one, 2, one, None, 4, 16, one, one, one, one, 0, None, one, one, None, one, one, one, 16, None) == -3
    assert L.vnet_bn_act_bwd_apply_head(one, one, 9, one, None, 4, 16, one, one, one, one, 0, None, one, one, 4.0, None, one, None) == -2


# ---- ops.bn_head: the forms the decoder output takes ----------------------------------------------------------------------------
FORMS = [
    # (kind, C, K, activation, residual, voxel grid)
    (0, 16, 2, "prelu", False, (2, 5, 6, 7)), (0, 8, 5, "relu", False, (1, 7, 9, 11)), (0, 16, 5, None, False, (1, 3, 5, 33)),
    (1, 16, 2, "prelu", False, (2, 5, 6, 7)), (1, 8, 2, "lrelu", False, (1, 4, 6, 19)), (1, 16, 5, "prelu", False, (1, 16, 16, 16)),
    (-1, 16, 2, "prelu", True, (2, 5, 6, 7)), (-1, 8, 5, "relu", True, (1, 7, 9, 11)), (-1, 16, 2, "prelu", False, (1, 9, 9, 9)),
    (0, 16, 2, "prelu", False, (1, 64, 64, 64)),
]


@pytest.mark.parametrize("kind,C,K,act,res,shp", FORMS)
def test_bn_head_op(dev, kind, C, K, act, res, shp):
    """ops.bn_head fused against the two ops it stands for (set_head_fusion(False)) and against the oracle's layer-by-layer graph:
    bn_chain kind 0 / 1 (test_bn_chain's inputs: gammas of both signs, variances spread over three decades) and bn_act with the
    residual of the unchained decoder block."""
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(100 * (kind + 1) + C + K)
    nl = 3 if kind == 0 else 2 if kind == 1 else 1
    if kind >= 0:
        scale = np.exp(rng.uniform(np.log(0.02), np.log(20.0), C))
        x = rng.standard_normal(shp + (C,)) * scale * (1.0 + rng.standard_normal(C) * 0.5)
        gam = [rng.uniform(0.3, 1.5, C) * rng.choice([-1.0, 1.0], C) for _ in range(nl)]
    else:
        x = rng.standard_normal(shp + (C,)) * 3.0 + 1.5
        gam = [rng.uniform(0.5, 1.5, C)]
    x = x.astype(np.float32).astype(np.float64)
    r = rng.standard_normal(shp + (C,)).astype(np.float32).astype(np.float64) if res else None
    bet = [rng.standard_normal(C) for _ in range(nl)]
    alpha = rng.uniform(0.05, 0.3, C)
    w, b = rng.standard_normal((1, 1, 1, C, K)), rng.standard_normal(K)
    dl = rng.standard_normal(shp + (K,))

    X, A_, W_, Bi = O.Var(x), O.Var(alpha), O.Var(w), O.Var(b)
    R = O.Var(r) if res else None
    G_, B_ = [O.Var(v) for v in gam], [O.Var(v) for v in bet]
    st = [[] for _ in range(nl)]
    if kind == 0:
        y1 = O.batch_norm_train(X, G_[0], B_[0], stats_out=st[0])
        y2 = O.batch_norm_train(y1, G_[1], B_[1], stats_out=st[1])
        y = O.batch_norm_train(O.add(y1, y2), G_[2], B_[2], stats_out=st[2])
    elif kind == 1:
        y = O.batch_norm_train(O.add(X, O.batch_norm_train(X, G_[0], B_[0], stats_out=st[0])), G_[1], B_[1], stats_out=st[1])
    else:
        y = O.batch_norm_train(O.add(X, R) if res else X, G_[0], B_[0], stats_out=st[0])
    O.backward(O.convolution(_act(y, act, A_), W_, Bi, 1), dl)

    def run(fused, stats=False):
        tx = g(x, dev).requires_grad_(True)
        tr = g(r, dev).requires_grad_(True) if res else None
        tg, tb = [g(v, dev).requires_grad_(True) for v in gam], [g(v, dev).requires_grad_(True) for v in bet]
        ta, tw, tbi = (g(v, dev).requires_grad_(True) for v in (alpha, w, b))
        mov = []
        for k in range(3):
            mov += [torch.zeros(C, device=dev), torch.ones(C, device=dev)] if k < nl else [None, None]
        gb = [v for k in range(nl) for v in (tg[k], tb[k])] + [None] * (6 - 2 * nl)
        prev = ops.set_head_fusion(fused, stats)
        try:
            lg = ops.bn_head(tx, tw, tbi, kind, act, ta if act == "prelu" else None, *gb, residual=tr, moving=tuple(mov))
            assert (getattr(lg, "_vnet_stats", None) is not None) == (fused and stats)
            lg.backward(g(dl, dev))
        finally:
            ops.set_head_fusion(*prev)
        return dict(lg=lg, dx=tx.grad, dr=tr.grad if res else None, dg=[t.grad for t in tg], db=[t.grad for t in tb],
                    da=ta.grad if act == "prelu" else None, dw=tw.grad, dbi=tbi.grad, mov=mov)

    f, fs, u = run(True), run(True, True), run(False)
    tag = "bn_head kind%d C%d K%d %s res%d" % (kind, C, K, act, res)
    for got in (f, fs):
        assert torch.equal(got["lg"], u["lg"]), tag + ": logits differ from the unfused ops (the summation order is kept)"
        for k in range(2 * nl):
            assert torch.equal(got["mov"][k], u["mov"][k]), tag + ": moving statistics differ"
    if K == 2:                                           # the default setting computes the unfused ops' bits (module docstring)
        flat = lambda d: [d["dx"], d["dr"], d["da"], d["dw"], d["dbi"]] + d["dg"] + d["db"]
        for i, (a1, a0) in enumerate(zip(flat(f), flat(u))):
            assert (a1 is None and a0 is None) or torch.equal(a1, a0), "%s: gradient %d differs from the unfused ops" % (tag, i)
    chain = kind >= 0
    for name, got in (("fused", f), ("fused + statistics rows", fs), ("unfused", u)):
        t = "%s %s" % (tag, name)
        check_close(t + " dx", got["dx"], X.g, 5e-5, atol=1e-5)
        if res:
            check_close(t + " dr", got["dr"], R.g, 5e-5, atol=1e-5)
        for k in range(nl):
            check_close(t + " dgamma%d" % k, got["dg"][k], G_[k].g, 5e-5 if chain else 2e-5, atol=1e-5 if chain else None)
            check_close(t + " dbeta%d" % k, got["db"][k], B_[k].g, 2e-5, atol=1e-6 if chain else None)
        if act == "prelu":
            check_close(t + " dalpha", got["da"], A_.g, 2e-5)
    # the head's own gradients: fp64 products of the y the device computed (what test_head's 2e-6 is a bound for)
    tx = g(x, dev)
    tg, tb = [g(v, dev) for v in gam], [g(v, dev) for v in bet]
    ta = g(alpha, dev) if act == "prelu" else None
    if chain:
        ty = ops.bn_chain(tx, kind, act, ta, tg[0], tb[0], tg[1], tb[1], tg[2] if kind == 0 else None, tb[2] if kind == 0 else None)
    else:
        ty = ops.bn_act(tx, tg[0], tb[0], act, ta, g(r, dev) if res else None)
    y64 = _f64(ty).reshape(-1, C)
    check_close(tag + " logits", f["lg"], (y64 @ w[0, 0, 0] + b).reshape(dl.shape), 2e-6)
    check_close(tag + " dw", f["dw"], (y64.T @ dl.reshape(-1, K)).reshape(w.shape), 2e-6)
    check_close(tag + " db", f["dbi"], dl.reshape(-1, K).sum(0), 2e-6)
    check_close(tag + " dw vs unfused", f["dw"], _f64(u["dw"]), 2e-6)


def test_bn_head_leaves_its_ds_in_the_fork_slot(dev):
    """bn_head over a forked residual (kind -1) leaves its ds in the residual's fork slot, fused or not, as bn_act does: the block
    input's other consumer then accumulates its gradient into that tensor and no add kernel runs."""
    from vnet_tensorflow_amd import ops
    C, K, shp = 16, 2, (1, 4, 5, 6)
    rng = np.random.default_rng(3)
    for fused in (True, False):
        x = g(rng.standard_normal(shp + (C,)), dev).requires_grad_(True)
        _, r = ops.fork(g(rng.standard_normal(shp + (C,)), dev).requires_grad_(True))
        slot, found = r._vnet_slot, []
        r.register_hook(lambda gr: found.append(slot.first is not None and slot.first.data_ptr() == gr.data_ptr()))
        par = [g(v, dev).requires_grad_(True) for v in (rng.standard_normal((1, 1, 1, C, K)), rng.standard_normal(K),
                                                        rng.uniform(0.05, 0.3, C), rng.uniform(0.5, 1.5, C), rng.standard_normal(C))]
        prev = ops.set_head_fusion(fused)
        try:
            lg = ops.bn_head(x, par[0], par[1], -1, "prelu", par[2], par[3], par[4], residual=r)
            lg.backward(g(rng.standard_normal(shp + (K,)), dev))
        finally:
            ops.set_head_fusion(*prev)
        assert found == [True], "fused %s: the residual's gradient is not in its fork slot" % fused
        assert slot.first is None                        # (the fork node has run and dropped it)


def test_network_takes_the_fused_head(dev):
    """networks.VNet with dropout 0 runs the fused passes and none of the head's own kernels; fuse_head = False or a dropout layer
    between the decoder and the head keeps the unfused ops.  With K = 2 the fused network computes the unfused network's bits:
    logits and every parameter gradient -- with the decoder's chains in closed form and, fuse_bn_chains = False, with the head folded
    into bn_act with the residual (kind -1).  No forked tensor's gradient needs an add kernel: its fork node finds the sum its second
    consumer wrote, or a single gradient."""
    from vnet_tensorflow_amd import _lib, networks, ops
    real_lib = _lib.lib
    real = real_lib()
    seen = []

    class Rec(object):
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)
    rec = Rec()
    fork_backward = ops._ForkFn.backward
    forks = []

    def watched(ctx, ga, gb):
        forks.append(ctx.slot.total is not None or ga is None or gb is None)
        return fork_backward(ctx, ga, gb)
    fused_names = {"vnet_bn_act_head_fwd", "vnet_bn_act_bwd_reduce_head", "vnet_bn_act_bwd_apply_head"}
    images, _ = O.synthetic_batch(1, 16, 1, 2, seed=7)
    out = {}
    for fuse, rate, chains in ((True, 0.0, True), (False, 0.0, True), (True, 0.25, True), (True, 0.0, False), (False, 0.0, False)):
        for nconv in ((1, 2), (2, 2)):                       # the level-1 decoder block ends in chain kind 0 / kind 1
            np.random.seed(5)                                # (the initialisers draw from NumPy's global generator)
            net = networks.VNet(2, rate, 8, 2, nconv, 2, True, "prelu", device=dev)
            net.fuse_head, net.fuse_bn_chains = fuse, chains
            net.build((1, 16, 16, 16, 1))
            del seen[:], forks[:]
            _lib.lib = lambda: rec
            ops._ForkFn.backward = staticmethod(watched)
            try:
                logits = net.GetNetwork(torch.from_numpy(images).to(dev))
                logits.square().sum().backward()
            finally:
                _lib.lib = real_lib
                ops._ForkFn.backward = staticmethod(fork_backward)
            names = set(seen)
            if fuse and rate == 0.0:
                assert fused_names <= names and not {"vnet_head_fwd", "vnet_head_bwd"} & names, sorted(names)
            else:
                assert {"vnet_head_fwd", "vnet_head_bwd"} <= names and not fused_names & names, sorted(names)
            assert ("vnet_bn_chain_coef_fwd" in names) == chains
            assert forks and all(forks), forks
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
            out[(fuse, rate, chains, nconv)] = (logits.detach().clone(), [(n, p.grad.clone()) for n, p in net.named_parameters()])
    for chains in (True, False):
        for nconv in ((1, 2), (2, 2)):
            (lf, gf), (lu, gu) = out[(True, 0.0, chains, nconv)], out[(False, 0.0, chains, nconv)]
            assert torch.equal(lf, lu), "logits of the fused network differ from the unfused one's"
            for (n, a1), (_, a0) in zip(gf, gu):
                assert torch.equal(a1, a0), "gradient of %s differs between the fused and the unfused network" % n
