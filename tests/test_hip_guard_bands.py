"""-m gpu: guard bands and poisoned scratch around the kernel launches (tests/guard.py).

Every case runs PRODUCT code (ops.route -> ops._conv_launch / _wgrad_launch, the batch-norm routes, the ctypes table of _lib.py)
with all its device buffers carved from one arena: inputs, every tensor ops allocates, packed filters of exactly
vnet_packed_weight_floats floats, and ops.workspace() replaced by arena scratch of EXACTLY the bytes route() reported.  A device
pointer outside the arena fails the case.  Checked: (a) no guard byte touched, no input changed; (b) no `out` element left
unwritten; (c) the result against the fp64 oracle -- the case functions and tolerances ARE the existing tests' (imported, not
restated); (d) the run on 0xFF-filled and the run on 0x00-filled outputs and scratch agree bit for bit -- for every case: ATOMIC_KERNELS,
the kernels that once added through LDS float atomics in an order the hardware picks, is empty (tests/test_hip_determinism.py).

COVERED, EXEMPT, FAMILIES and the case table are what tests/test_host.py's ledger reads.  The 5x5x1 convolution (kx = 1) runs in the
input-im2col cases, the bf16 conv2-direct `up` launch in b16-conv2-direct-odd-b2 (forward of the transposed layer and backward-data
of the down layer)."""
import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import guard
from tests import test_hip_b16 as T16
from tests import test_hip_ops as TO
from tests import test_hip_parity_holes as TP
from tests import util as TU
from tests.util import check_close

pytestmark = pytest.mark.gpu

# elementwise.hip kernels that add floats with atomicAdd (LDS) would be held to (a)-(c) only: there are none (tests/test_host.py holds
# this tuple against the source; the generic batch-norm reduce, column sum and head backward had such adds and keep their case ids)
ATOMIC_KERNELS = ()


def _split3(fn):
    def run(fx):
        with TU.split3(True):
            fn(fx)
    return run


def _direct(on, fn):
    def run(fx):
        from vnet_tensorflow_amd import ops
        fx.monkeypatch.setitem(ops._FUSE, "input_direct", on)
        fn(fx)
    return run


def _conv(ks, stride, *shape):
    return lambda fx: TO._conv_case(fx.dev, *shape, ks=ks, stride=stride, seed=sum(shape))



# ---- cases of this file's own: explicit arena tensors (fx.h.g: input; _out: poisoned output; _io: accumulate target) into the
# product's launch functions or the ctypes table; references in numpy float64, tolerances those of the existing test of the kernel
def _out(fx, name, shape, dtype=torch.float32):
    return fx.h.arena.tensor(name, shape, dtype, "out")


def _io(fx, name, a, dtype=torch.float32):
    a = np.ascontiguousarray(a)
    return fx.h.arena.tensor(name, a.shape, dtype, "inout", torch.as_tensor(a).to(dtype))


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64) if t.dtype == torch.bfloat16 else t.detach().cpu().numpy().astype(np.float64)


def _conv_stats_acc(mode, B, D, H, W, Ci, Co):
    """5^3 forward with bias, residual and epilogue statistics into stats[Route.stats_rows][2][Co] of exactly that size, the
    batch-norm finalize from those rows (BnRoute 'epilogue'), then y += conv in place (and, bf16, added out of place)."""
    def run(fx):
        from vnet_tensorflow_amd import ops
        b16, x3 = mode == "bf16", mode == "x3"
        rng = np.random.default_rng(B + D + H + W + Ci + Co)
        rnd = T16.rb if b16 else (lambda a: a)
        x, res, prev = (rnd(rng.standard_normal((B, D, H, W, c))) for c in (Ci, Co, Co))
        w, b = rng.standard_normal((5, 5, 5, Ci, Co)) * 0.1, rng.standard_normal(Co)
        dt = torch.bfloat16 if b16 else torch.float32
        tx, tres, tw, tb = fx.h.g(x, None, dt), fx.h.g(res, None, dt), fx.h.g(w), fx.h.g(b)
        dims = (D, H, W)
        r = ops.route(ops.FWD, 5, 1, 0, b16, x3, Ci, 0, Co, B, dims, dims, True, 0, True)
        assert r.stats_rows > 0, r
        y, stats = _out(fx, "y", (B, D, H, W, Co), dt), _out(fx, "stats", (r.stats_rows, 2 * Co))
        ops._conv_launch(r, tx, None, tw, tb, y, stats=stats, res=tres)
        conv = O.conv_nd_fwd(x, rnd(w), 1)
        if b16:
            T16.check_bf16("y", y, conv + b)
        else:
            check_close("y", y, conv + b, 2e-6)
        v = (_np(y) + res).reshape(-1, Co)                       # statistics of the stored output (+ residual)
        part = _np(stats).sum(0)
        np.testing.assert_allclose(part[:Co], v.sum(0), rtol=2e-5, atol=1e-6 * np.abs(v).sum(0).max())
        np.testing.assert_allclose(part[Co:], (v * v).sum(0), rtol=2e-5)
        M = v.shape[0]
        rt = ops.bn_route("act", M, Co, x16=b16, r16=b16 if b16 else None, epilogue=True, store16=b16, sync=False)
        assert rt.stats == "epilogue"
        mm, mv = _io(fx, "mm", np.zeros(Co)), _io(fx, "mv", np.ones(Co))
        mean, invstd, _ = ops._bn_stats(rt, y, tres, False, M, Co, mm, mv, ops._EpilogueStats(stats, r.stats_rows, tres))
        np.testing.assert_allclose(_np(mean), v.mean(0), rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(_np(invstd), 1.0 / np.sqrt(v.var(0) + 1e-3), rtol=5e-6)
        check_close("moving_mean", mm, 0.01 * v.mean(0), 1e-5, atol=1e-7)
        check_close("moving_var", mv, 0.99 + 0.01 * v.var(0), 1e-5)
        r2 = ops.route(ops.FWD, 5, 1, 0, b16, x3, Ci, 0, Co, B, dims, dims)
        acc = _io(fx, "acc", prev, dt)
        ops._conv_launch(r2, tx, None, tw, None, acc, accum=True)
        if b16:
            T16.check_bf16("y += conv", acc, conv + prev)
            oop = _out(fx, "oop", (B, D, H, W, Co), dt)
            ops._conv_launch(r2, tx, None, tw, None, oop, acc_src=fx.h.g(prev, None, dt))
            assert torch.equal(oop, acc)
        else:
            check_close("y += conv", acc, conv + prev, 2e-6)
    return run


def _padded_input(fx):
    """fp32 image of 4 modalities -> vnet_cast_bf16 (8 channels, the last 4 zero) -> vnet_conv_fwd_b16_padded with statistics."""
    from vnet_tensorflow_amd import ops
    D, H, W, cin, Co = 32, 64, 64, 3, 16
    rng = np.random.default_rng(cin + D)
    x = T16.rb(rng.standard_normal((1, D, H, W, cin)))
    w, b = rng.standard_normal((5, 5, 5, cin, Co)) * 0.2, rng.standard_normal(Co)
    tx = ops.cast_input(fx.h.g(x))
    assert tx.shape[-1] == 8 and np.array_equal(_np(tx)[..., :cin], x) and not _np(tx)[..., cin:].any()
    r = ops.route(ops.FWD, 5, 1, 0, True, False, 8, 0, Co, 1, (D, H, W), (D, H, W), True, cin)
    assert r.family == "conv-bf16-padded" and r.stats_rows > 0, r
    y, stats = _out(fx, "y", (1, D, H, W, Co), torch.bfloat16), _out(fx, "stats", (r.stats_rows, 2 * Co))
    ops._conv_launch(r, tx, None, fx.h.g(w), fx.h.g(b), y, stats=stats)
    T16.check_bf16("padded fwd", y, O.conv_nd_fwd(x, T16.rb(w), 1) + b)
    v, part = _np(y).reshape(-1, Co), _np(stats).sum(0)
    np.testing.assert_allclose(part[:Co], v.sum(0), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(part[Co:], (v * v).sum(0), rtol=1e-5)


def _wgrad16(shape, **opts):
    """vnet_conv_wgrad_b16 with the library option that selects the z-streaming / row-reuse kernel."""
    def run(fx):
        from vnet_tensorflow_amd import ops
        for k, v in opts.items():
            fx.lib_option(k, v)
        B, D, H, W, C0, C1, Co = shape
        x0, x1, w, b, dy = T16._conv5_inputs(shape, sum(shape) + 5)
        xcat = x0 if x1 is None else np.concatenate((x0, x1), -1)
        _, dw_ex = O.conv_nd_bwd(xcat, T16.rb(w), dy, 1, need_dx=False)
        bf = torch.bfloat16
        dw = _out(fx, "dw", w.shape)
        ops._wgrad5_b16_call(fx.h.g(x0, None, bf), fx.h.g(x1, None, bf) if C1 else None, fx.h.g(dy, None, bf), dw, (D, H, W), C0 + C1)
        check_close("dw %s %s" % (opts, shape,), dw, dw_ex, 2e-6)
    return run


def _sink(fx, ops, r, dw):
    s = ops.GradSink(dw)
    s.ws = fx.h.workspace(r.ws)                     # this layer's slabs: exactly Route.ws bytes, alive until the flush
    return s


def _deferred_group(fx):
    """A deferring pass on bf16 tensors: three 5^3 layers and a 2^3 layer leave their slabs side by side in the arena, one grouped
    launch (vnet_conv_wgrad_b16_group, mixed ks = 5 / 2 job list) and one flush reduce them."""
    from vnet_tensorflow_amd import ops
    bf = torch.bfloat16
    todo = []
    with ops.deferred_wgrad_reduce():
        for k, shape in enumerate([(1, 8, 16, 32, 32, 0, 32), (2, 5, 9, 16, 16, 0, 32), (1, 6, 7, 5, 32, 32, 32)]):
            B, D, H, W, C0, C1, Co = shape
            x0, x1, w, b, dy = T16._conv5_inputs(shape, 100 + 7 * k + sum(shape))
            r = ops.route(ops.WGRAD, 5, 1, 0, True, False, C0, C1, Co, B, (D, H, W), (D, H, W), True, C0 + C1)
            dw = _out(fx, "dw%d" % k, w.shape)
            ops._wgrad_launch(r, fx.h.g(x0, None, bf), fx.h.g(x1, None, bf) if C1 else None, fx.h.g(dy, None, bf), dw, _sink(fx, ops, r, dw))
            xcat = x0 if x1 is None else np.concatenate((x0, x1), -1)
            todo.append((dw, O.conv_nd_bwd(xcat, np.zeros(w.shape), dy, 1, need_dx=False)[1]))
        rng = np.random.default_rng(9)
        B, dims, C = 2, (9, 11, 17), 16
        dc = tuple(-(-v // 2) for v in dims)
        x, dy = T16.rb(rng.standard_normal((B,) + dims + (C,))), T16.rb(rng.standard_normal((B,) + dc + (2 * C,)))
        r = ops.route(ops.WGRAD, 2, 2, 0, True, False, C, 0, 2 * C, B, dims, dc)
        dw = _out(fx, "dw2", (2, 2, 2, C, 2 * C))
        ops._wgrad_launch(r, fx.h.g(x, None, bf), None, fx.h.g(dy, None, bf), dw, _sink(fx, ops, r, dw))
        todo.append((dw, O.conv_nd_bwd(x, np.zeros((2, 2, 2, C, 2 * C)), dy, 2, need_dx=False)[1]))
        assert len(ops._DEFER["jobs"]) == 4                    # nothing has been launched yet
    for k, (dw, ex) in enumerate(todo):
        check_close("deferred group member %d" % k, dw, ex, 2e-6)


def _deferred_fp32(fx):
    """vnet_wgrad_defer .. vnet_wgrad_flush on fp32 tensors: two layers' slabs live side by side until the one batched reduce."""
    from vnet_tensorflow_amd import ops
    todo = []
    with ops.deferred_wgrad_reduce():
        for k, (B, D, H, W, Ci, Co) in enumerate([(1, 8, 8, 8, 32, 32), (2, 5, 9, 17, 16, 16)]):
            rng = np.random.default_rng(k + 40)
            x, dy = rng.standard_normal((B, D, H, W, Ci)), rng.standard_normal((B, D, H, W, Co))
            r = ops.route(ops.WGRAD, 5, 1, 0, False, False, Ci, 0, Co, B, (D, H, W), (D, H, W))
            assert r.ws > 0
            dw = _out(fx, "dw%d" % k, (5, 5, 5, Ci, Co))
            ops._wgrad_launch(r, fx.h.g(x), None, fx.h.g(dy), dw, _sink(fx, ops, r, dw))
            todo.append((dw, O.conv_nd_bwd(x, np.zeros((5, 5, 5, Ci, Co)), dy, 1, need_dx=False)[1]))
    for k, (dw, ex) in enumerate(todo):
        check_close("deferred fp32 layer %d" % k, dw, ex, 2e-6)


def _sync(fn):
    """Cross-replica batch-norm with a world of one replica: the all-reduce is the identity, the kernels are the moments / finalize /
    all-reduced-apply ones."""
    def run(fx):
        from vnet_tensorflow_amd import ops
        fx.monkeypatch.setattr(ops, "_SYNC_BN", ((lambda t: None), 1))
        fn(fx)
    return run


def _bn_act_bwd_fused(fx):
    """vnet_bn_act_bwd (reduce + apply in one call) through the ctypes table."""
    from vnet_tensorflow_amd import _lib, ops
    L = _lib.lib()
    C, shp = 16, (2, 5, 6, 7)
    rng = np.random.default_rng(77)
    x, r = rng.standard_normal(shp + (C,)) * 3.0 + 1.5, rng.standard_normal(shp + (C,))
    gamma, beta, alpha = rng.uniform(0.5, 1.5, C), rng.standard_normal(C), rng.uniform(0.05, 0.3, C)
    X, R, G_, B_, A_ = (O.Var(a) for a in (x, r, gamma, beta, alpha))
    st = []
    y = O.prelu(O.batch_norm_train(O.add(X, R), G_, B_, stats_out=st), A_)
    dy = rng.standard_normal(y.v.shape)
    O.backward(y, dy)
    mu, var = st[0]
    M = x.size // C
    t = [fx.h.g(a) for a in (dy, x, r, mu, 1.0 / np.sqrt(var + 1e-3), gamma, beta, alpha)]
    dg, db, da, ds = _out(fx, "dgamma", (C,)), _out(fx, "dbeta", (C,)), _out(fx, "dalpha", (C,)), _out(fx, "ds", x.shape)
    nb = L.vnet_bn_ws_bytes(C)
    ws = fx.h.workspace(nb)
    p = ops._ptr
    _lib.check(L.vnet_bn_act_bwd(p(t[0]), p(t[1]), p(t[2]), 0, M, C, p(t[3]), p(t[4]), p(t[5]), p(t[6]), 2, p(t[7]), p(dg), p(db), p(da),
                                 p(ds), p(ws), nb, ops._stream()), "vnet_bn_act_bwd")
    check_close("ds", ds, X.g, 5e-5, atol=1e-5)
    check_close("dgamma", dg, G_.g, 2e-5)
    check_close("dbeta", db, B_.g, 2e-5)
    check_close("dalpha", da, A_.g, 2e-5)


def _seed_const(fx, ops, values):
    """ops._const_vector uploads a small constant once per process: hand it the arena's copy."""
    key = (tuple(float(v) for v in values), fx.dev)
    fx.monkeypatch.setitem(ops._CONST_VEC, key, fx.h.g(np.asarray(key[0])))


def _loss(loss_name, B, K, dims):
    def run(fx):
        from vnet_tensorflow_amd import ops
        rng = np.random.default_rng(B * 10 + K)
        z = rng.standard_normal((B,) + dims + (K,)) * 2.0
        lab = rng.integers(0, K, size=(B,) + dims + (1,)).astype(np.int32)
        wts = list(rng.uniform(0.1, 1.0, K))
        Z = O.Var(z)
        loss, sm = O.loss_head(Z, lab, loss_name, wts, 0.7)
        O.backward(loss, 1.7)
        _seed_const(fx, ops, wts)
        tz = fx.h.g(z).requires_grad_(True)
        tl, _, tsm, tpred = ops.softmax_loss(tz, fx.h.g(lab, None, torch.int32), loss_name, wts, 0.7, want_softmax=True, want_pred=True)
        check_close(loss_name + " loss", tl, loss.v, 2e-6)
        check_close(loss_name + " softmax", tsm, sm.v, 2e-6)
        assert (tpred.cpu().numpy() == O.argmax_pred(z)).all()
        tl.backward(fx.h.g(np.float64(1.7)).reshape(()))
        check_close(loss_name + " dlogits", tz.grad, Z.g, 1e-5)
    return run


def _dice(fx):
    from vnet_tensorflow_amd import model, ops
    rng = np.random.default_rng(0)
    B, dims, K = 3, (4, 5, 7), 3
    p = O.softmax(O.Var(rng.standard_normal((B,) + dims + (K,)))).v.astype(np.float32).astype(np.float64)
    t = O.one_hot(rng.integers(0, K, size=(B,) + dims), K)
    w = [0.2, 0.5, 1.0]
    P = O.Var(p)
    d = O.dice_coe(P, t, "jaccard", weights=w)
    O.backward(d)
    tp, tt, tw = fx.h.g(p).requires_grad_(True), fx.h.g(t), fx.h.g(w)
    td = model._DiceCoeFn.apply(tp, tt, True, tw, 1e-5)
    check_close("dice_coe", td, d.v, 2e-6)
    td.backward(fx.h.g(np.float64(1.0)).reshape(()))
    check_close("dice_coe grad", tp.grad, P.g, 1e-5)


def _dropout(fx):
    """fp32 (plain, and with the device step state), bf16, and their backward kernels; the reference uses the kernel's own mask."""
    from vnet_tensorflow_amd import _lib, ops
    L, p = _lib.lib(), ops._ptr
    n, rate = 8 * 1237, 0.25                      # not a multiple of the block
    rng = np.random.default_rng(4)
    x, dy = rng.standard_normal(n) + 3.0, rng.standard_normal(n)
    state = _io(fx, "state", np.zeros(32), torch.uint8)
    ops.set_step_state(state, 1e-2, 2e-3, 5)
    for kind in ("plain", "dev", "b16"):
        dt = torch.bfloat16 if kind == "b16" else torch.float32
        xs, dys = (T16.rb(x), T16.rb(dy)) if kind == "b16" else (x, dy)
        tx, tdy = fx.h.g(xs, None, dt), fx.h.g(dys, None, dt)
        y, mask, dx = _out(fx, "y_" + kind, (n,), dt), _out(fx, "mask_" + kind, (n,), torch.uint8), _out(fx, "dx_" + kind, (n,), dt)
        if kind == "plain":
            _lib.check(L.vnet_dropout_fwd(p(tx), p(y), p(mask), n, rate, 41, ops._stream()), "vnet_dropout_fwd")
        elif kind == "dev":
            _lib.check(L.vnet_dropout_fwd_dev(p(tx), p(y), p(mask), n, rate, 41, p(state), ops._stream()), "vnet_dropout_fwd_dev")
        else:
            _lib.check(L.vnet_dropout_fwd_b16(p(tx), p(y), p(mask), n, rate, 41, None, ops._stream()), "vnet_dropout_fwd_b16")
        fn = L.vnet_dropout_bwd_b16 if kind == "b16" else L.vnet_dropout_bwd
        _lib.check(fn(p(tdy), p(mask), p(dx), n, rate, ops._stream()), "vnet_dropout_bwd")
        m = mask.cpu().numpy().astype(np.float64)
        assert set(np.unique(m)) <= {0.0, 1.0} and abs(m.mean() - (1 - rate)) < 0.02
        if kind == "b16":
            T16.check_bf16("dropout fwd", y, xs * m / (1 - rate), noise=1e-7)
            T16.check_bf16("dropout bwd", dx, dys * m / (1 - rate), noise=1e-7)
        else:
            check_close("dropout fwd " + kind, y, xs * m / (1 - rate), 1e-6)
            check_close("dropout bwd " + kind, dx, dys * m / (1 - rate), 1e-6)


def _optimisers(fx):
    """Adam / SGD / Momentum (plain and Nesterov), with host scalars and with the device step state, n not a multiple of 4."""
    from vnet_tensorflow_amd import ops
    n, lr = 4099, 1e-2
    rng = np.random.default_rng(5)
    p0, g, m0, v0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n) * 0.1, rng.uniform(0.0, 0.2, n)
    b1, b2, eps, gs = 0.9, 0.999, 1e-8, 0.5
    lr_t = lr * np.sqrt(1 - b2 ** 3) / (1 - b1 ** 3)
    ge = g * gs
    m1, v1 = b1 * m0 + (1 - b1) * ge, b2 * v0 + (1 - b2) * ge * ge
    state = _io(fx, "state", np.zeros(32), torch.uint8)
    ops.set_step_state(state, lr, lr_t, 3)
    tg = fx.h.g(g)
    for st in (None, state):
        tag = "dev" if st is not None else "host"
        p, m, v = _io(fx, "p_adam_" + tag, p0), _io(fx, "m_" + tag, m0), _io(fx, "v_" + tag, v0)
        ops.adam_apply(p, tg, m, v, float(lr_t), b1, b2, eps, gs, state=st)
        check_close("adam p " + tag, p, p0 - lr_t * m1 / (np.sqrt(v1) + eps), 2e-6)
        check_close("adam m " + tag, m, m1, 2e-6)
        check_close("adam v " + tag, v, v1, 2e-6)
        p = _io(fx, "p_sgd_" + tag, p0)
        ops.sgd_apply(p, tg, lr, gs, state=st)
        check_close("sgd " + tag, p, p0 - lr * ge, 2e-6)
        for nesterov in (False, True):
            p, acc = _io(fx, "p_mom%d_%s" % (nesterov, tag), p0), _io(fx, "acc%d_%s" % (nesterov, tag), m0)
            ops.momentum_apply(p, tg, acc, lr, 0.9, nesterov, gs, state=st)
            a1 = 0.9 * m0 + ge
            check_close("momentum acc", acc, a1, 2e-6)
            check_close("momentum p", p, p0 - lr * ((ge + 0.9 * a1) if nesterov else a1), 2e-6)


def _repack_batched(fx):
    """vnet_pack_weights_batched (one single-image record, one both-images record) == vnet_pack_weights, bit for bit."""
    import ctypes
    from vnet_tensorflow_amd import _lib, ops
    L, p = _lib.lib(), ops._ptr
    rng = np.random.default_rng(6)
    rows, pairs = [], []
    for mode, taps, I, Oc in ((ops.PACK_FWD, 125, 6, 10), (ops.PACK_BOTH, 125, 32, 32), (ops.PACK_UP, 8, 32, 16)):
        w = fx.h.g(rng.standard_normal((taps, I, Oc)))
        modes = (ops.PACK_FWD, ops.PACK_BWD) if mode == ops.PACK_BOTH else (mode,)
        one, bat = [], []
        for md in modes:
            nfl = L.vnet_packed_weight_floats(md, taps, I, Oc)
            one.append(_out(fx, "single%d_%d" % (md, I), (nfl,)))
            bat.append(_out(fx, "batched%d_%d" % (md, I), (nfl,)))
            _lib.check(L.vnet_pack_weights(md, p(w), p(one[-1]), taps, I, Oc, ops._stream()), "vnet_pack_weights")
        if mode == ops.PACK_BOTH:
            rows.append([p(w), p(bat[0]), mode, taps, I, Oc, p(bat[1]), 0])
        else:
            cq, npad = ctypes.c_int(), ctypes.c_int()
            _lib.check(L.vnet_packed_dims(mode, taps, I, Oc, ctypes.byref(cq), ctypes.byref(npad)), "vnet_packed_dims")
            rows.append([p(w), p(bat[0]), mode, taps, I, Oc, cq.value, npad.value])
        pairs += list(zip(one, bat))
    descs = fx.h.g(np.asarray(rows, dtype=np.int64), None, torch.int64)
    _lib.check(L.vnet_pack_weights_batched(p(descs), len(rows), ops._stream()), "vnet_pack_weights_batched")
    for a, b in pairs:
        assert torch.equal(a, b)


def _auc(fx):
    from vnet_tensorflow_amd import ops
    K, N, T = 3, 20011, 200
    rng = np.random.default_rng(K)
    lab = rng.integers(0, K, size=N).astype(np.int32)
    sm = O.softmax(O.Var(rng.standard_normal((N, K)) + 1.5 * (lab[:, None] == np.arange(K)))).v.astype(np.float32)
    th = ops.tf_auc_thresholds(T)
    sm[:50, 1] = th[1:51]                                      # predictions ON thresholds: the strict `>`
    _seed_const(fx, ops, th)
    hist = ops.auc_histogram(fx.h.g(sm), fx.h.g(lab, None, torch.int32), K, 1, T)
    bins = (sm[:, 1][:, None] > th[None, :]).sum(1)
    ref = np.stack([np.bincount(bins[lab == 1], minlength=T + 1), np.bincount(bins[lab != 1], minlength=T + 1)])
    assert np.array_equal(hist.cpu().numpy(), ref.astype(np.float64))


def _accumulate_patch(fx):
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(8)
    D, H, W, K, (pz, py, px), origin = 7, 9, 11, 3, (4, 5, 6), (3, 4, 5)          # the patch ends on the volume's last voxel
    patch, vol0, cnt0 = rng.standard_normal((pz, py, px, K)), rng.standard_normal((D, H, W, K)), rng.integers(0, 3, (D, H, W)).astype(np.float64)
    vol, cnt = _io(fx, "vol", vol0), _io(fx, "count", cnt0)
    ops.accumulate_patch(fx.h.g(patch), vol, cnt, origin)
    sl = tuple(slice(o, o + n) for o, n in zip(origin, (pz, py, px)))
    vol0[sl] += patch
    cnt0[sl] += 1
    check_close("vol", vol, vol0, 1e-6)
    assert np.array_equal(cnt.cpu().numpy(), cnt0)


def _head16(K):
    def run(fx):
        from vnet_tensorflow_amd import ops
        rng = np.random.default_rng(K)
        x = T16.rb(rng.standard_normal((2, 5, 6, 7, 16)))
        w, b, dy = rng.standard_normal((1, 1, 1, 16, K)) * 0.3, rng.standard_normal(K), rng.standard_normal((2, 5, 6, 7, K))
        tx, tw, tb = fx.h.g(x, None, torch.bfloat16).requires_grad_(True), fx.h.g(w).requires_grad_(True), fx.h.g(b).requires_grad_(True)
        y = ops.head_conv(tx, tw, tb)
        check_close("head fwd", y, x @ w[0, 0, 0] + b, 2e-6)
        tdy = fx.h.g(dy)
        y.backward(tdy)
        dy32 = _np(tdy)
        T16.check_bf16("head dx", tx.grad, dy32 @ w[0, 0, 0].T, noise=2e-6)
        check_close("head dw", tw.grad, (x.reshape(-1, 16).T @ dy32.reshape(-1, K)).reshape(w.shape), 5e-6)
        check_close("head db", tb.grad, dy32.reshape(-1, K).sum(0), 5e-6, atol=1e-5)
    return run


PACK, COLSUM = "vnet_pack_weights", "vnet_colsum"
CONV5 = ("vnet_conv_fwd", "vnet_conv_wgrad", PACK, COLSUM)
X3 = ("vnet_conv_fwd_x3", "vnet_conv_wgrad_x3", PACK, COLSUM)
BN = ("vnet_bn_stats", "vnet_bn_act_fwd", "vnet_bn_act_bwd_reduce", "vnet_bn_act_bwd_apply")
BN16 = ("vnet_bn_stats_b16", "vnet_bn_act_fwd_b16", "vnet_bn_act_bwd_reduce_b16", "vnet_bn_act_bwd_apply_b16")
SMALL16 = ("vnet_bn_small_fwd_b16", "vnet_bn_small_bwd_b16")
CHAIN = ("vnet_bn_stats", "vnet_bn_chain_coef_fwd", "vnet_bn_act_fwd", "vnet_bn_act_bwd_reduce", "vnet_bn_chain_coef_bwd",
         "vnet_bn_act_bwd_apply")
IN_DIRECT = ("vnet_input_conv_fold", "vnet_input_conv_fold_border", "vnet_input_conv_direct_fwd", "vnet_input_wgrad_direct",
             "vnet_input_conv_grads", "vnet_bn_stats", "vnet_bn_act_fwd", "vnet_bn_act_bwd_reduce", COLSUM)
IN_IM2COL = ("vnet_input_conv_fold", "vnet_tile_im2col_x", "vnet_conv_fwd", "vnet_conv_wgrad", "vnet_input_conv_grads", PACK,
             "vnet_bn_stats", "vnet_bn_act_fwd", "vnet_bn_act_bwd_reduce", COLSUM)

# id -> (entry points the case must reach, families / batch-norm routes it must take, deterministic (d), the case)
CASES = {
    # ---- fp32 MFMA convolutions: forward, backward-data (two destinations with a second source), filter gradient, bias gradient
    "conv5-wide-brick": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 1, 8, 16, 32, 16, 0, 16)),
    "conv5-ragged-two-source-b2": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 2, 5, 9, 17, 16, 16, 16)),
    "conv5-cube-brick-split-k": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 1, 8, 8, 8, 32, 32, 32)),
    "conv5-split-k-two-cout-blocks": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 1, 4, 4, 4, 128, 0, 128)),
    "conv5-2cube": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 1, 2, 2, 2, 64, 0, 64)),
    "conv5-1x1x1-b3": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 3, 1, 1, 1, 16, 0, 16)),
    "conv5-narrow-channels": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 1, 6, 7, 9, 4, 4, 8)),
    "conv5-cin3-gather": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 1, 6, 6, 18, 3, 0, 16)),
    "conv5-cout5-scatter": (CONV5, ("conv", "wgrad"), True, _conv(5, 1, 1, 4, 6, 16, 16, 0, 5)),
    "down-direct-f32": (("vnet_conv2_direct_f32", "vnet_conv_wgrad", COLSUM), ("conv2-direct", "wgrad"), True,
                        _conv(2, 2, 1, 8, 16, 32, 16, 0, 32)),
    "down-direct-f32-odd-b2": (("vnet_conv2_direct_f32", "vnet_conv_wgrad", COLSUM), ("conv2-direct", "wgrad"), True,
                               _conv(2, 2, 2, 5, 7, 9, 32, 0, 64)),
    "down-generic-odd": (("vnet_conv_fwd", "vnet_conv_wgrad", PACK, COLSUM), ("conv", "wgrad"), True, _conv(2, 2, 1, 5, 7, 9, 4, 0, 8)),
    "down-generic-2cube": (("vnet_conv_fwd", "vnet_conv_wgrad", PACK, COLSUM), ("conv", "wgrad"), True,
                           _conv(2, 2, 1, 2, 2, 2, 128, 0, 256)),
    "up-direct-f32": (("vnet_conv2_direct_f32", "vnet_conv_wgrad", COLSUM), ("conv2-direct", "wgrad"), True,
                      lambda fx: TO._up_case(fx.dev, (2, 4, 4, 8, 64, 32, None), 7)),
    "up-generic-odd-output": (("vnet_conv_fwd", "vnet_conv_wgrad", PACK, COLSUM), ("conv", "wgrad"), True,
                              lambda fx: TO._up_case(fx.dev, (1, 3, 4, 5, 8, 4, (5, 7, 9)), 8)),
    "up-generic-1x1x1": (("vnet_conv_fwd", "vnet_conv_wgrad", PACK, COLSUM), ("conv", "wgrad"), True,
                         lambda fx: TO._up_case(fx.dev, (1, 1, 1, 1, 256, 128, None), 9)),
    # ---- f32x3: wide brick, 8-wide brick, K-split (ws > 0), two cout blocks, two sources / two destinations
    "x3-wide-ragged-two-source-b2": (X3, ("conv-x3", "wgrad-x3"), True, _split3(_conv(5, 1, 2, 5, 9, 17, 16, 16, 16))),
    "x3-two-cout-blocks": (X3, ("conv-x3", "wgrad-x3"), True, _split3(_conv(5, 1, 1, 8, 8, 16, 32, 0, 32))),
    "x3-k-split": (X3, ("conv-x3", "wgrad-x3"), True, _split3(_conv(5, 1, 1, 8, 8, 16, 128, 0, 32))),
    "x3-8-wide-ragged-b2": (X3, ("conv-x3", "wgrad-x3"), True, _split3(_conv(5, 1, 2, 6, 10, 8, 16, 16, 48))),
    "x3-8-wide-k-split": (X3, ("conv-x3", "wgrad-x3"), True, _split3(_conv(5, 1, 1, 8, 8, 8, 128, 0, 64))),
    "x3-smaller-than-a-brick": (X3, ("conv-x3", "wgrad-x3"), True, _split3(_conv(5, 1, 1, 3, 5, 7, 16, 0, 48))),
    # ---- bf16 storage
    "b16-conv5-ragged-two-source-b2": (("vnet_conv_fwd_b16", "vnet_conv_wgrad_b16", "vnet_colsum_b16", PACK), ("conv-bf16", "wgrad-bf16"),
                                       True, lambda fx: T16.test_conv5_b16_against_oracle_and_fp32_output_kernels(
                                           fx.dev, (2, 5, 9, 17, 16, 16, 16), fx.monkeypatch, fx.lib_option)),
    "b16-conv5-split-k": (("vnet_conv_fwd_b16", "vnet_conv_wgrad_b16", "vnet_colsum_b16", PACK), ("conv-bf16", "wgrad-bf16"), True,
                          lambda fx: T16.test_conv5_b16_against_oracle_and_fp32_output_kernels(
                              fx.dev, (1, 4, 4, 4, 128, 0, 128), fx.monkeypatch, fx.lib_option)),
    "b16-conv2-direct-odd-b2": (("vnet_conv2_direct_b16", "vnet_conv2_wgrad_b16", "vnet_colsum_b16"), ("conv2-direct", "wgrad2-b16"), True,
                                lambda fx: T16.test_conv2_down_and_up_b16(fx.dev, (2, 9, 11, 17, 16), True)),
    "b16-conv2-generic-odd-b2": (("vnet_conv2_fwd_b16", "vnet_conv2_wgrad_b16", "vnet_colsum_b16", PACK), ("conv2-b16", "wgrad2-b16"), True,
                                 lambda fx: T16.test_conv2_down_and_up_b16(fx.dev, (2, 9, 11, 17, 16), False)),
    "b16-conv2-generic-split-k": (("vnet_conv2_fwd_b16", "vnet_conv2_wgrad_b16", "vnet_colsum_b16", PACK), ("conv2-b16", "wgrad2-b16"), True,
                                  lambda fx: T16.test_conv2_down_and_up_b16(fx.dev, (1, 4, 4, 4, 128), False)),
    "b16-bn-stream": (BN16, ("stream",), True, lambda fx: T16.test_bn_act_b16(fx.dev, (1, 9, 11, 13), 32, "prelu", True, False, fx.monkeypatch)),
    "b16-bn-small": (SMALL16, ("small",), True, lambda fx: T16.test_bn_act_b16(fx.dev, (1, 5, 3, 7), 8, None, False, True, fx.monkeypatch)),
    "b16-bn-small-res": (SMALL16, ("small",), True, lambda fx: T16.test_bn_act_b16(fx.dev, (1, 4, 4, 4), 256, "prelu", True, True, fx.monkeypatch)),
    # ---- input block
    "input-direct-ragged-b2": (IN_DIRECT, ("input-direct", "input-wgrad-direct"), True,
                               _direct(True, lambda fx: TO._input_block_case(fx.dev, (2, 5, 9, 17, 16), True))),
    "input-direct-8-wide": (IN_DIRECT, ("input-direct", "input-wgrad-direct"), True,
                            _direct(True, lambda fx: TO._input_block_case(fx.dev, (1, 8, 8, 8, 8), True))),
    "input-im2col-ragged": (IN_IM2COL, ("conv", "wgrad"), True, _direct(False, lambda fx: TO._input_block_case(fx.dev, (2, 5, 9, 17, 16), False))),
    "input-im2col-4ch": (IN_IM2COL, ("conv", "wgrad"), True, _direct(True, lambda fx: TO._input_block_case(fx.dev, (1, 6, 7, 9, 4), True))),
    # ---- batch-norm (fp32): vector path, row path (C <= 8), generic path (fixed-order LDS meeting in both passes), tile
    "bn-vec-res": (BN, ("stream",), True, lambda fx: TO._bn_act_case(fx.dev, 16, "prelu", True, False, (2, 5, 6, 7), 23)),
    "bn-vec-256": (BN, ("stream",), True, lambda fx: TO._bn_act_case(fx.dev, 256, "prelu", True, False, (1, 3, 3, 7), 24)),
    "bn-row-c5": (BN, ("stream",), True, lambda fx: TO._bn_act_case(fx.dev, 5, "lrelu", True, False, (2, 5, 6, 7), 12)),
    "bn-generic-c12-atomic": (BN, ("stream",), True, lambda fx: TO._bn_act_case(fx.dev, 12, "prelu", False, False, (3, 5, 6, 7), 12)),
    "bn-tile": (BN, ("stream",), True, lambda fx: TO._bn_act_case(fx.dev, 16, None, False, True, (2, 5, 6, 7), 16)),
    "bn-chain-kind0": (CHAIN, ("stream",), True, lambda fx: TO.test_bn_chain(fx.dev, 0, 16, "prelu")),
    "bn-chain-kind1": (CHAIN, ("stream",), True, lambda fx: TO.test_bn_chain(fx.dev, 1, 64, "lrelu")),
    # ---- head, loss, activation, metrics, dropout
    "head-vec": (("vnet_head_fwd", "vnet_head_bwd"), (), True, lambda fx: TO.test_head(fx.dev, 16, 5)),
    "head-generic-atomic": (("vnet_head_fwd", "vnet_head_bwd"), (), True, lambda fx: TO.test_head(fx.dev, 6, 2)),
    "act-prelu": (("vnet_act_fwd", "vnet_act_bwd"), (), True, lambda fx: TO.test_activation_standalone(fx.dev)),
    "confusion-matrix": (("vnet_confusion_matrix",), (), True, lambda fx: TO.test_hard_metrics(fx.dev)),
    # ---- epilogue statistics into exactly Route.stats_rows rows, the finalize from them, y += conv (in and out of place)
    "conv5-stats-res-acc": (("vnet_conv_fwd_stats", "vnet_conv_fwd_acc", "vnet_bn_finalize_partial", PACK), ("conv", "epilogue"), True,
                            _conv_stats_acc("fp32", 2, 5, 9, 17, 16, 16)),
    "conv5-stats-split-k": (("vnet_conv_fwd_stats", "vnet_conv_fwd_acc", "vnet_bn_finalize_partial", PACK), ("conv", "epilogue"), True,
                            _conv_stats_acc("fp32", 1, 8, 8, 8, 64, 64)),
    "x3-stats-res-acc": (("vnet_conv_fwd_x3", "vnet_bn_finalize_partial", PACK), ("conv-x3", "epilogue"), True,
                         _split3(_conv_stats_acc("x3", 2, 6, 10, 20, 16, 32))),
    "x3-stats-8-wide-k-split": (("vnet_conv_fwd_x3", "vnet_bn_finalize_partial", PACK), ("conv-x3", "epilogue"), True,
                                _split3(_conv_stats_acc("x3", 1, 8, 8, 8, 128, 64))),
    "b16-stats-res-acc": (("vnet_conv_fwd_b16", "vnet_bn_finalize_partial", PACK), ("conv-bf16", "epilogue"), True,
                          _conv_stats_acc("bf16", 2, 5, 9, 17, 16, 32)),
    "b16-padded-input": (("vnet_cast_bf16", "vnet_conv_fwd_b16_padded", PACK), ("conv-bf16-padded",), True, _padded_input),
    # ---- filter gradients: kernels behind library options, the deferred form, the grouped launch
    "b16-wgrad-z-streaming": (("vnet_conv_wgrad_b16",), ("wgrad-bf16",), True, _wgrad16((2, 7, 9, 17, 16, 0, 32), WGRAD_ZS="1")),
    "b16-wgrad-z-streaming-8-wide": (("vnet_conv_wgrad_b16",), ("wgrad-bf16",), True, _wgrad16((1, 6, 7, 5, 32, 32, 96), WGRAD_ZS="1")),
    "b16-wgrad-row-reuse": (("vnet_conv_wgrad_b16",), ("wgrad-bf16",), True, _wgrad16((2, 5, 11, 40, 8, 0, 16), WGRAD_RR="2")),
    "b16-wgrad-generic": (("vnet_conv_wgrad_b16",), ("wgrad-bf16",), True, _wgrad16((1, 6, 9, 33, 64, 0, 32), WGRAD_RR="0")),
    "b16-wgrad-deferred-group": (("vnet_conv_wgrad_b16_group",), ("wgrad-bf16", "wgrad2-b16"), True, _deferred_group),
    "wgrad-deferred-fp32": (("vnet_conv_wgrad",), ("wgrad",), True, _deferred_fp32),
    # ---- cross-replica batch-norm pieces (BnRoute 'moments', all-reduced backward), the one-call backward
    "bn-sync": (("vnet_bn_moments", "vnet_bn_finalize", "vnet_bn_act_fwd", "vnet_bn_act_bwd_reduce", "vnet_bn_act_bwd_apply"), ("moments",),
                True, _sync(lambda fx: TO._bn_act_case(fx.dev, 16, "prelu", True, False, (2, 5, 6, 7), 23))),
    "b16-bn-sync": (("vnet_bn_moments_b16", "vnet_bn_finalize", "vnet_bn_act_fwd_b16", "vnet_bn_act_bwd_reduce_b16",
                     "vnet_bn_act_bwd_apply_b16"), ("moments",), True,
                    _sync(lambda fx: T16.test_bn_act_b16(fx.dev, (1, 9, 11, 13), 32, "prelu", True, False, fx.monkeypatch))),
    "bn-act-bwd-one-call": (("vnet_bn_act_bwd",), (), True, _bn_act_bwd_fused),
    # ---- loss, dropout, optimisers, repack, metrics, sliding window, bf16 head
    "loss-weighted-sorensen-b3": (("vnet_softmax_dice_fwd", "vnet_softmax_dice_bwd"), (), True, _loss("weighted_sorensen", 3, 5, (6, 7, 9))),
    "loss-mixed-jaccard-k2": (("vnet_softmax_dice_fwd", "vnet_softmax_dice_bwd"), (), True, _loss("mixed_jaccard", 1, 2, (1, 1, 1))),
    "loss-weighted-xent-k5": (("vnet_softmax_dice_fwd", "vnet_softmax_dice_bwd"), (), True, _loss("weighted_xent", 2, 5, (3, 5, 33))),
    "dice-coe": (("vnet_dice_coe_fwd", "vnet_dice_coe_bwd"), (), True, _dice),
    "dropout": (("vnet_dropout_fwd", "vnet_dropout_fwd_dev", "vnet_dropout_fwd_b16", "vnet_dropout_bwd", "vnet_dropout_bwd_b16",
                 "vnet_step_state_set"), (), True, _dropout),
    "optimisers": (("vnet_adam_apply", "vnet_adam_apply_dev", "vnet_sgd_apply", "vnet_sgd_apply_dev", "vnet_momentum_apply",
                    "vnet_momentum_apply_dev", "vnet_step_state_set"), (), True, _optimisers),
    "repack-batched": ((PACK, "vnet_pack_weights_batched", "vnet_packed_dims"), (), True, _repack_batched),
    "auc-histogram": (("vnet_auc_histogram",), (), True, _auc),
    "accumulate-patch": (("vnet_accumulate_patch",), (), True, _accumulate_patch),
    "b16-head-k5": (("vnet_head_fwd_b16", "vnet_head_bwd_b16"), (), True, _head16(5)),
    "b16-head-k2": (("vnet_head_fwd_b16", "vnet_head_bwd_b16"), (), True, _head16(2)),
}

COVERED = {}
for _cid, (_entries, _fams, _det, _fn) in CASES.items():
    for _e in _entries:
        COVERED.setdefault(_e, []).append(_cid)
FAMILIES = set(f for c in CASES.values() for f in c[1])

# Entry points with a pointer parameter that no case runs, with the reason.  No convolution, filter-gradient, input-block,
# batch-norm, head or loss entry point may appear here (tests/test_host.py).
EXEMPT = {}


class _Fx(object):
    def __init__(self, dev, monkeypatch, lib_option):
        self.dev, self.monkeypatch, self.lib_option = dev, monkeypatch, lib_option


def _run(cid, fx, poison):
    """One guarded run of a case: checks (a) and (c) always, (b) on the 0xFF pre-fill; returns (snapshot, calls, routes taken, names
    of the tensors vnet_colsum wrote)."""
    from vnet_tensorflow_amd import model, ops
    entries, fams, det, fn = CASES[cid]
    arena = guard.Arena(fx.dev, poison=poison)
    seen = set()
    real = {n: getattr(ops, n) for n in ("route", "bn_route", "_conv_launch", "_wgrad_launch")}

    def route(*a, **k):
        r = real["route"](*a, **k)
        seen.add(r.family)
        return r

    def bn_route(*a, **k):
        r = real["bn_route"](*a, **k)
        seen.add(r.stats)
        return r

    def launch(name):
        def run(r, *a, **k):                              # scratch asked for while route r is launched: never more than Route.ws
            n0 = len(fx.h.ws_requests)
            out = real[name](r, *a, **k)
            assert all(q <= r.ws for q in fx.h.ws_requests[n0:]), (r.tag, r.ws, fx.h.ws_requests[n0:])
            return out
        return run
    for n, f in (("route", route), ("bn_route", bn_route), ("_conv_launch", launch("_conv_launch")), ("_wgrad_launch", launch("_wgrad_launch"))):
        fx.monkeypatch.setattr(ops, n, f)
    try:
        with guard.guarded(arena, modules=(model, TO, T16), g_modules=(TO, T16)) as h:
            fx.h = h
            fn(fx)                                        # (c): the comparison with the fp64 oracle
            arena.check()                                 # (a)
            if poison == guard.GUARD:
                arena.check_written()                     # (b)
    finally:
        for n, f in real.items():
            fx.monkeypatch.setattr(ops, n, f)
    return arena.snapshot(), h.calls, seen


@pytest.mark.parametrize("cid", sorted(CASES))
def test_guard_bands(dev, cid, monkeypatch, lib_option):
    entries, fams, det, fn = CASES[cid]
    fx = _Fx(dev, monkeypatch, lib_option)
    snap_ff, calls, seen = _run(cid, fx, guard.GUARD)
    missing = set(entries) - set(calls)
    assert not missing, "%s never reached %s (called: %s)" % (cid, sorted(missing), sorted(set(calls)))
    table = guard.pointer_entry_points()
    undeclared = set(c for c in calls if c in table) - set(entries)
    assert not undeclared, "%s also runs %s: name them in its row" % (cid, sorted(undeclared))
    assert set(fams) <= seen, "%s: expected the routes %s, took %s" % (cid, fams, sorted(seen))
    if det:
        snap_00, _, _ = _run(cid, fx, 0x00)
        guard.assert_same_bits(snap_ff, snap_00)          # (d)
