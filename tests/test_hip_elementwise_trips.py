"""-m gpu: every kernel family of csrc/elementwise.hip past one trip of its grid-stride loop.

ew_blocks() caps a launch at VNET_EW_MAXBLK blocks of EW_BLOCK threads, so past TRIP = 262 144 work items a thread walks its loop more
than once, and several kernels are right across trips only because the stride is a multiple of the channel-quad count (the vector
statistics / reduce / head kernels), of the row group (the generic statistics kernel) or of a whole row (the row kernels).  The per-op
tests run a few hundred rows; here each case is the smallest shape that wraps, against the NumPy fp64 oracle on the same
float32-valued inputs, at the tolerance the per-op test of the same op holds (its case function is called where there is one).

Every case states the launch it means to wrap through _wraps(): the work-item expression its launcher hands to ew_blocks(), the items
the kernel's loop walks and how many of them a block takes per trip, all from the constants read out of elementwise.hip.  It asserts
that the grid is at its cap, that the loop makes at least two trips and (ragged) that the last trip is a partial one -- so a change
of the cap either keeps a case wrapping or fails it here, never turns it into a one-trip case silently."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import test_hip_b16 as T16
from tests import test_hip_head_fusion as THF
from tests import test_hip_ops as TO
from tests.util import g, check_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _consts():
    src = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "elementwise.hip")).read()
    m = (re.search(r"constexpr int EW_BLOCK = (\d+);", src), re.search(r"#define VNET_EW_MAXBLK (\d+)", src),
         re.search(r"#define VNET_BN_RED_U (\d+)", src),
         # voxels per thread and trip of the loss head's forward kernel
         re.search(r"softmax_dice_fwd_kernel\(LossP p\) \{.*?constexpr int U = (\d+);", src, re.S),
         # vnet_colsum_b16 has a cap and a block of its own: RB rows per block and trip
         re.search(r"colsum_b16_kernel\(.*?const int RB = (\d+) / CO, tid", src, re.S),
         re.search(r"const int nblk = \(int\)min\(\(int64_t\)(\d+), \(M \+ RB - 1\) / RB\);", src))
    assert all(m), "elementwise.hip no longer states its blocks, caps and unroll factors as it did"
    return tuple(int(v.group(1)) for v in m)


BLOCK, MAXBLK, RED_U, LOSS_U, CS16_BLOCK, CS16_MAXBLK = _consts()
TRIP = BLOCK * MAXBLK                # work items of one trip of a capped grid (262 144)


def _wraps(name, launch, items=None, per_block=None, ragged=True, capped=True, blocks=1):
    """A launch of ew_blocks(launch) * blocks workgroups whose loop walks `items` (default: launch), per_block of them per block and
    trip (default: one per thread): the grid is capped (capped=False: a kernel that rides along with the one the case is about, whose
    launcher divides its work by four), the loop makes >= 2 trips, the last one is partial.  Returns the trip count."""
    items = launch if items is None else items
    per_block = BLOCK if per_block is None else per_block
    grid = min(MAXBLK, max(1, -(-launch // BLOCK))) * blocks
    per_trip = grid * per_block
    trips = -(-items // per_trip)
    assert not capped or grid == MAXBLK * blocks, "%s: %d work items do not reach the grid cap of %d blocks" % (name, launch, MAXBLK)
    assert trips >= 2, "%s: %d items in one trip of %d" % (name, items, per_trip)
    assert not ragged or items % per_trip != 0, "%s: %d items are whole trips of %d" % (name, items, per_trip)
    return trips


def _red_mode(C):
    q = C // 4
    return 0 if C % 4 == 0 and q & (q - 1) == 0 and q <= BLOCK else 1 if C <= 8 else 2


def _bn_wraps(tag, M, C, tile=False, stats=True, reduce=True, apply=True):
    """The four launches of a float32 batch-norm (vnet_bn_stats, vnet_bn_act_fwd, vnet_bn_act_bwd_reduce, _apply) over M rows of C
    channels, each from its launcher's own expression; the statistics and reduce kernels are the ones the cases are sized for."""
    Cs = 1 if tile else C
    if stats:
        mode = _red_mode(Cs)
        if mode == 0:
            _wraps(tag + " stats vec", M * (Cs // 4))
        elif mode == 1:
            _wraps(tag + " stats row", M)
        elif Cs > BLOCK:
            _wraps(tag + " stats wide", M * Cs, items=M, per_block=1)
        else:
            _wraps(tag + " stats generic", M * Cs, items=M, per_block=BLOCK // Cs)
    if apply:
        vec = C % 4 == 0
        ew = M * C // 4 // (4 if vec else 1) + 1
        n = M * C // 4 if vec else M * C
        _wraps(tag + " fwd", ew, items=n, capped=False)
        _wraps(tag + " apply", ew, items=n, capped=False)
    if reduce:
        mode = _red_mode(C)
        if mode == 0:
            _wraps(tag + " reduce vec", M * C // 16 + 1, items=M * C // 4, per_block=BLOCK * RED_U)
        elif mode == 1:
            _wraps(tag + " reduce row", M)
        else:
            _wraps(tag + " reduce generic", M * C // 4 + 1, items=M, per_block=1 if C > BLOCK else BLOCK // C)     # (row groups)


# ---- batch-norm, float32 -----------------------------------------------------------------------------------------------------------
ROWS = TRIP + 1003                   # just above one trip of rows; odd, so never a power of two

BN_CASES = [
    # C, act, residual, tile, rows
    (2, "prelu", False, False, ROWS), (5, "lrelu", True, False, ROWS), (7, "relu", False, False, ROWS),       # row mode (C <= 8, no quads)
    (5, "prelu", False, True, ROWS),                                                                          # tile: statistics of one channel
    (8, None, True, False, 2 * TRIP + 1003),                                                                  # two quads: the narrowest vector case
    (12, "prelu", True, False, 4 * TRIP // 12 + 51), (37, "relu", False, False, 4 * TRIP // 37 + 11),         # generic, C <= 256
    (300, "lrelu", False, False, 4 * TRIP // 300 + 6), (1021, "prelu", True, False, MAXBLK + 77),             # generic, wide branch
    (64, "prelu", True, False, 16 * TRIP // 64 + 65), (128, None, False, False, 16 * TRIP // 128 + 33),       # vector, CQ = 16, 32, 64
    (256, "lrelu", True, False, 16 * TRIP // 256 + 27),
]


@pytest.mark.parametrize("C,act,res,tile,M", BN_CASES)
def test_bn_act(dev, C, act, res, tile, M):
    assert M & (M - 1) != 0
    _bn_wraps("bn_act C%d" % C, M, C, tile)
    if C > BLOCK:
        assert M > MAXBLK                                    # the wide branch steps gridDim rows
    TO._bn_act_case(dev, C, act, res, tile, (M,), 1000 + C + 7 * bool(res))


@pytest.mark.parametrize("C,res,tile,M", [(2, False, False, ROWS), (5, True, False, ROWS), (7, False, False, ROWS), (5, False, True, ROWS),
                                          (16, True, False, 4 * TRIP // 16 + 1003), (12, False, False, 4 * TRIP // 12 + 51),
                                          (300, True, False, MAXBLK + 77)])
def test_bn_moments_exact(dev, C, res, tile, M):
    """The statistics kernels alone (vnet_bn_moments: the raw sums of x and x^2 per channel, in float64) on small non-zero integers:
    every float32 partial sum is an integer far below 2^24 and so exact, and the sums equal NumPy's to the last bit -- unless a row
    is counted twice or not at all, which moves the sum of squares by at least 1.  test_bn_act alone would not tell: one row of
    263 147 counted twice moves its mean and variance by about as much as its bar allows."""
    from vnet_tensorflow_amd import _lib, ops
    L = _lib.lib()
    Cs = 1 if tile else C
    _bn_wraps("bn_moments C%d" % C, M, C, tile, reduce=False, apply=False)
    rng = np.random.default_rng(40 + C)
    x = rng.integers(1, 8, size=(M, Cs)).astype(np.float32)
    r = rng.integers(1, 5, size=(M, C)).astype(np.float32) if res else None
    tx, tr = torch.from_numpy(x).to(dev), torch.from_numpy(r).to(dev) if res else None
    nb = L.vnet_bn_ws_bytes(C)
    ws, sums = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(2 * C, dtype=torch.float64, device=dev)
    rc = L.vnet_bn_moments(ops._ptr(tx), ops._ptr(tr) if res else None, int(tile), M, C, ops._ptr(sums), ops._ptr(ws), nb, ops._stream())
    assert rc == 0
    s = (x + r if res else np.broadcast_to(x, (M, C))).astype(np.int64)
    ref = np.concatenate([s.sum(0), (s * s).sum(0)])
    assert np.array_equal(sums.cpu().numpy(), ref.astype(np.float64)), (sums.cpu().numpy() - ref)


@pytest.mark.parametrize("kind,C,act", [(0, 16, "prelu"), (1, 6, "lrelu")])
def test_bn_chain(dev, kind, C, act):
    M = 16 * TRIP // C + 1003 if _red_mode(C) == 0 else ROWS
    _bn_wraps("bn_chain C%d" % C, M, C)
    TO._bn_chain_case(dev, kind, C, act, (M,))


def test_bn_concat(dev):
    """BN(concat(x0, x1)) as its two halves (U-Net decoder): a vector half and a row half, each past the cap."""
    from vnet_tensorflow_amd import ops
    C0, C1, M = 16, 5, ROWS
    _bn_wraps("bn_concat C%d" % C0, M, C0)
    _bn_wraps("bn_concat C%d" % C1, M, C1)
    rng = np.random.default_rng(21)
    x0, x1 = rng.standard_normal((M, C0)) * 3.0 + 1.5, rng.standard_normal((M, C1)) * 2.0 - 0.5
    gamma, beta = rng.uniform(0.5, 1.5, C0 + C1), rng.standard_normal(C0 + C1)
    X0, X1, G_, B_ = O.Var(x0), O.Var(x1), O.Var(gamma), O.Var(beta)
    st = []
    y = O.batch_norm_train(O.concat_channels(X0, X1), G_, B_, stats_out=st)
    dy = rng.standard_normal(y.v.shape)
    O.backward(y, dy)
    t0, t1, tg, tb = (g(a, dev).requires_grad_(True) for a in (x0, x1, gamma, beta))
    mm, mv = torch.zeros(C0 + C1, device=dev), torch.ones(C0 + C1, device=dev)
    y0, y1 = ops.bn_concat(t0, t1, tg, tb, mm, mv)
    # the bars of _bn_act_case
    check_close("bn_concat fwd0", y0, y.v[:, :C0], 5e-6)
    check_close("bn_concat fwd1", y1, y.v[:, C0:], 5e-6)
    torch.autograd.backward([y0, y1], [g(dy[:, :C0], dev), g(dy[:, C0:], dev)])
    check_close("bn_concat dx0", t0.grad, X0.g, 5e-5, atol=1e-5)
    check_close("bn_concat dx1", t1.grad, X1.g, 5e-5, atol=1e-5)
    check_close("bn_concat dgamma", tg.grad, G_.g, 2e-5)
    check_close("bn_concat dbeta", tb.grad, B_.g, 2e-5)
    mu, var = st[0]
    check_close("bn_concat moving_mean", mm, 0.01 * mu, 1e-5, atol=1e-7)
    check_close("bn_concat moving_var", mv, 0.99 + 0.01 * var, 1e-5)


# ---- column sum, activations, head ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 5])
def test_colsum(dev, C):
    """vnet_colsum: the vector kernel (red_mode 0) and the generic one.  The bar of the convolutions' bias gradient (_conv_case)."""
    from vnet_tensorflow_amd import ops
    M = 4 * TRIP // C + 1003 if _red_mode(C) else ROWS
    if _red_mode(C) == 0:
        _wraps("colsum vec", M * (C // 4) // 4 + 1, items=M * (C // 4))
    else:
        _wraps("colsum generic", M * C // 4 + 1, items=M, per_block=BLOCK // C)              # (256 / C row groups per block)
    x = np.random.default_rng(C).standard_normal((M, C)).astype(np.float32)
    got = ops.colsum(torch.from_numpy(x).to(dev), C)
    x64 = x.astype(np.float64)
    check_close("colsum C%d" % C, got, x64.sum(0), 2e-6, atol=1e-7 * float(np.abs(x64).sum(0).max()))


@pytest.mark.parametrize("act,C", [("prelu", 16), ("prelu", 5), ("prelu", 12), ("lrelu", 6)])
def test_activation(dev, act, C):
    """ops.activation: act_fwd / act_bwd (the identity batch-norm of the apply kernels) and, for prelu, the reduce kernel of each mode
    for dalpha.  The bars of test_activation_standalone."""
    from vnet_tensorflow_amd import ops
    mode = _red_mode(C)
    M = (16 if mode == 0 else 4) * TRIP // C + 1003 if mode != 1 or act != "prelu" else ROWS
    _bn_wraps("activation %s C%d" % (act, C), M, C, stats=False, reduce=act == "prelu")
    rng = np.random.default_rng(3 + C)
    x = rng.standard_normal((M, C))
    x[::1001, : min(C, 4)] = 0.0      # exact zeros: TF tie rule gives gradient 0
    a = rng.uniform(0.05, 0.3, C)
    X, A_ = O.Var(x), O.Var(a)
    y = O.prelu(X, A_) if act == "prelu" else O.leaky_relu(X)
    dy = rng.standard_normal(x.shape)
    O.backward(y, dy)
    tx, ta = g(x, dev).requires_grad_(True), g(a, dev).requires_grad_(True)
    ty = ops.activation(tx, act, ta)
    check_close(act + " fwd", ty, y.v, 1e-6)
    ty.backward(g(dy, dev))
    check_close(act + " dx", tx.grad, X.g, 1e-6)
    if act == "prelu":
        check_close(act + " dalpha", ta.grad, A_.g, 2e-6)


@pytest.mark.parametrize("C,K", [(16, 2), (16, 5), (8, 8), (5, 3), (6, 2)])
def test_head(dev, C, K):
    """ops.head_conv: head_fwd_kernel (M / 2), head_bwd_kernel (M C / 16) or head_bwd_generic_kernel (M C / 4), each past its own trip.
    The bars of test_head."""
    from vnet_tensorflow_amd import ops
    vec = _red_mode(C) == 0
    M = (2 if vec else 4) * TRIP + 1003
    _wraps("head fwd", M // 2 + 1, items=M)
    if vec:
        _wraps("head bwd vec", M * (C // 4) // 4 + 1, items=M * (C // 4))
    else:
        _wraps("head bwd generic", M * C // 4 + 1, items=M, per_block=BLOCK // C)            # (256 / C row groups per block)
    rng = np.random.default_rng(C * K)
    x = rng.standard_normal((M, C)).astype(np.float32).astype(np.float64)
    w = rng.standard_normal((1, 1, 1, C, K)).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(K)
    y_ref = x @ w[0, 0, 0] + b
    dy = rng.standard_normal(y_ref.shape).astype(np.float32).astype(np.float64)
    tx, tw, tb = (g(a, dev).requires_grad_(True) for a in (x, w, b))
    y = ops.head_conv(tx, tw, tb)
    check_close("head fwd", y, y_ref, 2e-6)
    y.backward(g(dy, dev))
    check_close("head dx", tx.grad, dy @ w[0, 0, 0].T, 2e-6)
    check_close("head dw", tw.grad, (x.T @ dy).reshape(w.shape), 2e-6)
    check_close("head db", tb.grad, dy.sum(0), 2e-6)


@pytest.mark.parametrize("kind,C,K,act,res", [(-1, 16, 2, "prelu", True), (1, 8, 5, "lrelu", False)])
def test_bn_head(dev, kind, C, K, act, res):
    """The fused batch-norm + head passes at the smallest M that wraps bn_head_blocks(): everything test_bn_head_op holds them to."""
    M = 16 * TRIP // C + 1003
    _wraps("bn_head fwd / apply", M * C // 4 // 4 + 1, items=M * (C // 4))
    _wraps("bn_head reduce", M * C // 4 // 4 + 1, items=M * (C // 4), per_block=BLOCK * RED_U)
    THF.test_bn_head_op(dev, kind, C, K, act, res, (1, M, 1, 1))       # (the oracle's convolution wants [B, D, H, W, C])


# ---- loss head -----------------------------------------------------------------------------------------------------------------------
V_LOSS = 4 * TRIP + 1003
_LOSS_IN = {}
LOSS_CASES = [(n, B, K) for B, K in ((1, 2), (2, 5), (1, 8)) for n in TO.LOSSES]


def _loss_inputs(B, K):
    if (B, K) not in _LOSS_IN:
        rng = np.random.default_rng(B * 10 + K)
        z = (rng.standard_normal((B, V_LOSS, K)) * 2.0).astype(np.float32).astype(np.float64)
        lab = rng.integers(0, K, size=(B, V_LOSS, 1)).astype(np.int32)
        lab[:, ::100003] = -1         # a few stray labels: tf.one_hot gives an all-zero row
        lab[:, 7::250007] = K
        wts = list(rng.uniform(0.1, 1.0, K))
        _LOSS_IN[(B, K)] = (z, lab, wts)
    return _LOSS_IN[(B, K)]


@pytest.mark.parametrize("loss_name,B,K", LOSS_CASES)
def test_softmax_loss(dev, loss_name, B, K):
    """softmax_dice_fwd_kernel<K> (LOSS_U voxels per thread and trip) and softmax_dice_bwd_kernel<K>.  The bars of test_softmax_loss."""
    from vnet_tensorflow_amd import ops
    _wraps("loss fwd", V_LOSS // 4 + 1, items=V_LOSS, per_block=LOSS_U * BLOCK)
    _wraps("loss bwd", V_LOSS // 4 + 1, items=V_LOSS)
    z, lab, wts = _loss_inputs(B, K)
    Z = O.Var(z)
    loss, sm = O.loss_head(Z, lab, loss_name, wts, 0.7)
    O.backward(loss, 1.7)
    tz = g(z, dev).requires_grad_(True)
    tl, _, tsm, tpred = ops.softmax_loss(tz, g(lab, dev, torch.int32), loss_name, wts, 0.7, want_softmax=True, want_pred=True)
    check_close(loss_name + " loss", tl, loss.v, 2e-6)
    check_close(loss_name + " softmax", tsm, sm.v, 2e-6)
    assert (tpred.cpu().numpy() == O.argmax_pred(z)).all()
    (tl * 1.7).backward()
    check_close(loss_name + " dlogits", tz.grad, Z.g, 1e-5)


@pytest.mark.parametrize("kind", ["sorensen", "jaccard"])
@pytest.mark.parametrize("weights", [[], [0.2, 0.5, 1.0]])
def test_dice_coe(dev, kind, weights):
    """model.dice_coe on probability / one-hot tensors: dice_sums_kernel<3> and dice_grad_kernel.  The bars of test_dice_coe_known_answers."""
    from vnet_tensorflow_amd import model
    K, V = 3, V_LOSS
    _wraps("dice sums", V // 4 + 1, items=V)
    _wraps("dice grad", V * K // 4 + 1, items=V * K)
    rng = np.random.default_rng(17)
    e = np.exp(rng.standard_normal((1, V, 1, 1, K)))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32).astype(np.float64)
    t = O.one_hot(rng.integers(0, K, size=(1, V, 1, 1)), K)
    P = O.Var(p)
    d = O.dice_coe(P, t, kind, weights=weights)
    O.backward(d)
    tp = g(p, dev).requires_grad_(True)
    td = model.dice_coe(tp, g(t, dev), kind, weights=weights)
    check_close("dice_coe %s %s" % (kind, weights), td, d.v, 2e-6)
    td.backward()
    check_close("dice_coe grad %s %s" % (kind, weights), tp.grad, P.g, 1e-5)


# ---- dropout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
def test_dropout(dev, bf16):
    """The generator is counter-based: element i of a seed's mask does not depend on the size of the launch, so the mask of n elements
    (several trips) starts with the mask of n0 (one trip, an uncapped grid) -- a stride error breaks that.  Forward and backward against
    the oracle with the kernel's own mask (test_dropout_against_oracle_with_the_kernels_mask; bf16: test_head_and_dropout_b16)."""
    from vnet_tensorflow_amd import ops
    rate, seed = 0.3, 4711
    if bf16:
        n, n0 = 16 * TRIP + 8 * 1003, 200000
        _wraps("dropout b16", n // 8 // 2 + 1, items=n // 8)
    else:
        n, n0 = 4 * TRIP + 1003, 200003
        _wraps("dropout", n // 4 + 1, items=n)
    assert n0 < TRIP
    rng = np.random.default_rng(8)
    xs, gs = O.round_bf16(rng.standard_normal(n)), O.round_bf16(rng.standard_normal(n))
    put = (lambda a: T16.g16(a, dev)) if bf16 else (lambda a: g(a, dev))
    x = put(xs).requires_grad_(True)
    ops._DROP_SEED[0] = seed
    y = ops.dropout(x, rate)
    mask_t = y.grad_fn.saved_tensors[0]
    ops._DROP_SEED[0] = seed
    y0 = ops.dropout(put(xs[:n0]).requires_grad_(True), rate)
    assert torch.equal(mask_t[:n0], y0.grad_fn.saved_tensors[0])
    mask = mask_t.cpu().numpy().astype(np.float64)
    assert set(np.unique(mask)) <= {0.0, 1.0} and abs(mask.mean() - (1.0 - rate)) < 0.005
    y.backward(put(gs))
    xv = O.Var(xs)
    ref = O.dropout(xv, rate, mask)
    xv.g = None
    O.backward(ref, seed=gs)
    if bf16:
        T16.check_bf16("dropout fwd", y, ref.v, noise=1e-7)
        T16.check_bf16("dropout bwd", x.grad, xv.g, noise=1e-7)
    else:
        check_close("dropout fwd", y, ref.v, 2e-7)
        check_close("dropout bwd", x.grad, xv.g, 2e-7)
    assert np.array_equal(y.detach().float().cpu().numpy() != 0, (mask != 0) & (xs != 0))


# ---- optimisers ----------------------------------------------------------------------------------------------------------------------
N_OPT = 4 * TRIP + 1003               # n % 4 == 3


def _opt_wraps(name, n):
    return _wraps(name, n // 4 + 1, items=n, blocks=2)


@pytest.mark.parametrize("name", ["SGD", "Momentum", "NesterovMomentum"])
def test_sgd_and_momentum(dev, name):
    """Three steps against O.sgd_step / O.TFMomentum, the schedule and the bar of test_optimisers."""
    from vnet_tensorflow_amd import ops, optim
    n = N_OPT
    assert n % 4 != 0
    _opt_wraps(name, n)
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    p, acc = g(p0, dev), torch.zeros(n, device=dev)
    ref = {"p": p0}
    ro = O.TFMomentum(0.9, name == "NesterovMomentum") if "Momentum" in name else None
    for step in range(3):
        gr = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        lr = optim.exponential_decay(1e-2, step, 100, 0.99)
        if ro is None:
            ops.sgd_apply(p, g(gr, dev), lr)
        else:
            ops.momentum_apply(p, g(gr, dev), acc, lr, 0.9, name == "NesterovMomentum")
        ref = ro.step(ref, {"p": gr}, lr) if ro else O.sgd_step(ref, {"p": gr}, lr)
    check_close(name, p, ref["p"], 2e-6)


def _offset_view(a, off, dev):
    """float32 `a` on the device, `off` floats into a 16-byte aligned buffer."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _adam_reference(p, grad, m, v, lr_t, b1, b2, eps, gs):
    """TF's ApplyAdam form in float64 with the float32 scalars the kernel receives (test_adam_full_parameter_vector)."""
    omb1 = float(np.float32(1) - np.float32(b1)); omb2 = float(np.float32(1) - np.float32(b2))
    gd = (grad * np.float32(gs)).astype(np.float64)
    mr = m.astype(np.float64) + (gd - m) * omb1
    vr = v.astype(np.float64) + (gd * gd - v) * omb2
    step = float(np.float32(lr_t)) * mr / (np.sqrt(vr) + float(np.float32(eps)))
    return p.astype(np.float64) - step, mr, vr, step


def _adam_check(tag, tp, tm, tv, ref):
    pr, mr, vr, step = ref
    p, m, v = (t.cpu().numpy().astype(np.float64) for t in (tp, tm, tv))
    # the bars of test_adam_full_parameter_vector
    assert float((np.abs(p - pr) / (np.abs(pr) + np.abs(step) + 1e-3)).max()) < 5e-7, tag
    assert float(np.abs(m - mr).max()) < 1e-9 and float(np.abs(v - vr).max()) < 1e-11, tag


def _adam_inputs(n):
    rng = np.random.default_rng(3)
    return (rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 1e-2).astype(np.float32),
            (rng.standard_normal(n) * 1e-3).astype(np.float32), (rng.random(n) * 1e-4).astype(np.float32))


ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, t=7, gs=0.125)


@pytest.mark.parametrize("offsets", [(1, 1, 1, 1), (0, 1, 0, 0), (0, 0, 0, 0)])
def test_adam_branches(dev, offsets):
    """adam_kernel takes its scalar loop when any of p, g, m, v is not 16-byte aligned (all four offset by one float; only g), else the
    float4 loop and a tail of n % 4 elements.  n is sized for the float4 loop (n / 4 items) to wrap, the scalar loop then makes four
    times as many trips; the tail is at most three elements and cannot."""
    from vnet_tensorflow_amd import ops
    n = 2 * N_OPT + 1                   # n % 4 == 3
    assert n % 4 in (1, 2, 3)
    _opt_wraps("adam scalar", n)
    if not any(offsets):
        _wraps("adam float4", n // 4 + 1, items=n // 4, blocks=2)
    a = ADAM
    lr_t = a["lr"] * np.sqrt(1 - a["b2"] ** a["t"]) / (1 - a["b1"] ** a["t"])
    host = _adam_inputs(n)
    tp, tg, tm, tv = (_offset_view(h, off, dev) for h, off in zip(host, offsets))
    assert [t.data_ptr() % 16 for t in (tp, tg, tm, tv)] == [4 * o for o in offsets]
    ops.adam_apply(tp, tg, tm, tv, lr_t, a["b1"], a["b2"], a["eps"], a["gs"])
    _adam_check("adam offsets %s" % (offsets,), tp, tm, tv, _adam_reference(*host, lr_t, a["b1"], a["b2"], a["eps"], a["gs"]))


def test_optimisers_from_the_step_state(dev):
    """The `_dev` forms read lr / lr_t from the device step state (the graph-replayable form): the argument is ignored."""
    from vnet_tensorflow_amd import ops
    n, a = N_OPT, ADAM
    _opt_wraps("_dev forms", n)
    lr, lr_t = 3e-3, a["lr"] * np.sqrt(1 - a["b2"] ** a["t"]) / (1 - a["b1"] ** a["t"])
    st = ops.step_state(dev)
    ops.set_step_state(st, lr, lr_t, 5)
    host = _adam_inputs(n)
    tp, tg, tm, tv = (torch.from_numpy(h).to(dev) for h in host)
    ops.adam_apply(tp, tg, tm, tv, 123.0, a["b1"], a["b2"], a["eps"], a["gs"], state=st)
    _adam_check("adam_apply_dev", tp, tm, tv, _adam_reference(*host, lr_t, a["b1"], a["b2"], a["eps"], a["gs"]))
    p0, gr = host[0].astype(np.float64), host[1].astype(np.float64) * 100.0
    for nesterov in (None, False, True):
        p, acc = g(p0, dev), torch.zeros(n, device=dev)
        if nesterov is None:
            ops.sgd_apply(p, g(gr, dev), 123.0, state=st)
            ref = O.sgd_step({"p": p0}, {"p": gr}, lr)
        else:
            ro = O.TFMomentum(0.9, nesterov)
            ref = {"p": p0}
            for _ in range(2):
                ops.momentum_apply(p, g(gr, dev), acc, 123.0, 0.9, nesterov, state=st)
                ref = ro.step(ref, {"p": gr}, lr)
        check_close("_dev nesterov=%s" % nesterov, p, ref["p"], 2e-6)


# ---- evaluate helpers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_count", [True, False])
def test_accumulate_patch(dev, with_count):
    """A 65 x 64 x 64 patch of three classes that hangs over the high faces of the volume on all three axes, applied twice: exact for
    integer-valued data."""
    from vnet_tensorflow_amd import ops
    pz, py, px, K = 65, 64, 64, 3
    D, H, W = 70, 66, 65
    z0, y0, x0 = 10, 5, 3
    _wraps("accumulate_patch", pz * py * px)
    assert z0 + pz > D and y0 + py > H and x0 + px > W
    rng = np.random.default_rng(4)
    patch = rng.integers(-50, 50, size=(pz, py, px, K)).astype(np.float32)
    vol0 = rng.integers(-9, 9, size=(D, H, W, K)).astype(np.float32)
    vol, cnt = torch.from_numpy(vol0).to(dev), torch.zeros((D, H, W), device=dev) if with_count else None
    tpatch = torch.from_numpy(patch).to(dev)
    for _ in range(2):
        ops.accumulate_patch(tpatch, vol, cnt, (z0, y0, x0))
    ref, rcnt = vol0.astype(np.float64), np.zeros((D, H, W))
    ref[z0:, y0:, x0:] += 2.0 * patch[:D - z0, :H - y0, :W - x0]
    rcnt[z0:, y0:, x0:] += 2.0
    assert np.array_equal(vol.cpu().numpy().astype(np.float64), ref)
    if with_count:
        assert np.array_equal(cnt.cpu().numpy().astype(np.float64), rcnt)


def _cap(pattern, name):
    src = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "input_block.hip")).read()
    m = re.search(pattern, src)
    assert m, "input_block.hip no longer states the grid of %s as it did" % name
    return int(m.group(1)) * int(m.group(2)), int(m.group(3))


def test_confusion_matrix(dev):
    """vnet_confusion_matrix past its own cap (16 elements per thread up to 1024 blocks): exact counts, stray labels and predictions
    outside [0, K) are not counted."""
    from vnet_tensorflow_amd import ops
    per_block, cap = _cap(r"const int nblk = \(int\)\(\(n \+ (\d+) \* (\d+) - 1\) / \(256 \* 16\) > (\d+) \?", "vnet_confusion_matrix")
    n, K = per_block * cap + 5003, 5
    assert -(-n // per_block) > cap and n % (cap * 256) != 0
    rng = np.random.default_rng(2)
    lab = rng.integers(-1, K + 1, size=n).astype(np.int32)
    pred = np.where(rng.uniform(size=n) < 0.7, lab, rng.integers(0, K, size=n)).astype(np.int64)
    m = ops.hard_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev), K)
    ok = (lab >= 0) & (lab < K) & (pred >= 0) & (pred < K)
    ref = np.bincount(lab[ok].astype(np.int64) * K + pred[ok], minlength=K * K).reshape(K, K)
    assert np.array_equal(m["confusion"], ref.astype(np.float64))


def test_auc_histogram(dev):
    """vnet_auc_histogram past its cap of 256 blocks: bin = number of float32 thresholds strictly below the prediction, exact counts."""
    from vnet_tensorflow_amd import ops
    per_block, cap = _cap(r"const int64_t want = \(n \+ (\d+) \* (\d+) - 1\) / \(256 \* 16\);\s*const int nblk = \(int\)\(want > (\d+) \?",
                          "vnet_auc_histogram")
    n, K, cls, T = per_block * cap + 5003, 3, 1, 200
    assert -(-n // per_block) > cap and n % (cap * 256) != 0
    rng = np.random.default_rng(6)
    e = np.exp(rng.standard_normal((n, K)) * 2.0)
    sm = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    sm[::1013, cls] = ops.tf_auc_thresholds(T)[(np.arange(0, n, 1013) % (T - 2)) + 1]      # predictions ON a threshold are not above it
    lab = rng.integers(0, K, size=n).astype(np.int32)
    hist = ops.auc_histogram(torch.from_numpy(sm).to(dev), torch.from_numpy(lab).to(dev), K, cls, T).cpu().numpy()
    bins = np.searchsorted(ops.tf_auc_thresholds(T), sm[:, cls], side="left")
    ref = np.stack([np.bincount(bins[lab == cls], minlength=T + 1), np.bincount(bins[lab != cls], minlength=T + 1)])
    assert np.array_equal(hist, ref.astype(np.float64))


# ---- bf16 storage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4])
def test_cast_input(dev, C):
    """vnet_cast_bf16: RNE of every value, the pad channels exactly zero."""
    from vnet_tensorflow_amd import ops
    M = 2 * TRIP + 1003
    _wraps("cast_bf16", M * (8 // 8) // 2 + 1, items=M)
    x = (np.random.default_rng(C).standard_normal((M, C)) * 30.0).astype(np.float32)
    y = ops.cast_input(torch.from_numpy(x).to(dev))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (M, 8)
    yv = y.float().cpu().numpy()
    assert np.array_equal(yv[:, :C].astype(np.float64), O.round_bf16(x.astype(np.float64)))
    assert not yv[:, C:].any()


@pytest.mark.parametrize("C,act,res", [(16, "prelu", True), (16, "relu", False), (64, "prelu", False), (64, None, True),
                                       (256, "prelu", True), (256, "relu", False)])
def test_bn_act_b16(dev, C, act, res, monkeypatch):
    """The bf16 streaming kernels (statistics / normalise / reduce / apply: two 16-byte units per thread and trip) just past their cap,
    the small-tensor kernels switched off.  Everything test_bn_act_b16 holds them to."""
    from vnet_tensorflow_amd import ops
    monkeypatch.setitem(ops._SMALL_BN, "on", False)
    M = 16 * TRIP // C + 1003
    assert M & (M - 1) != 0
    _wraps("bn b16", M * (C // 8) // 2 + 1, items=M * (C // 8), per_block=2 * BLOCK)
    T16._bn_act_b16_case(dev, (M,), C, act, res)


def test_bn_tile_b16(dev, monkeypatch):
    """tf.tile of the fp32 one-channel image + batch-norm -> bf16 under ComputeDtype bf16: the bar of test_bn_tile_and_chain_b16."""
    from vnet_tensorflow_amd import ops
    monkeypatch.setitem(ops._SMALL_BN, "on", False)
    M, C = TRIP + 1003, 16
    _wraps("bn b16 tile", M * (C // 8) // 2 + 1, items=M * (C // 8), per_block=2 * BLOCK)
    rng = np.random.default_rng(3)
    img = (rng.standard_normal((M, 1)) * 40 + 100).astype(np.float32).astype(np.float64)
    gamma, beta = 1 + 0.3 * rng.standard_normal(C), 0.3 * rng.standard_normal(C)
    ref = O.batch_norm_train(O.tile_channels(O.Var(img), C), O.Var(gamma), O.Var(beta))
    ops.set_compute_dtype("bf16")
    try:
        y = ops.bn_act(g(img, dev), g(gamma, dev), g(beta, dev), None, None, tile=True)
    finally:
        ops.set_compute_dtype("fp32")
    T16.check_bf16("tile+bn", y, ref.v, noise=2e-6)


def test_colsum16(dev):
    """vnet_colsum_b16 (its own cap of CS16_MAXBLK blocks of CS16_BLOCK / (C / 8) rows): the bar of the bf16 convolutions' bias gradient."""
    from vnet_tensorflow_amd import ops
    C = 16
    rows_per_trip = CS16_MAXBLK * (CS16_BLOCK // (C // 8))
    M = rows_per_trip + 1003
    assert M > rows_per_trip and M % rows_per_trip != 0
    x = O.round_bf16(np.random.default_rng(9).standard_normal((M, C)))
    out = torch.empty(C, dtype=torch.float32, device=dev)
    ops.colsum16(T16.g16(x, dev), C, out)
    check_close("colsum16", out, x.sum(0), 2e-6, atol=1e-6 * float(np.abs(x).sum(0).max()))


@pytest.mark.parametrize("K", [2, 5])
def test_head_b16(dev, K):
    """head_fwd_b16_kernel (M / 2) and head_bwd_b16_kernel (M C / 16) past their caps: the bars of test_head_and_dropout_b16."""
    from vnet_tensorflow_amd import ops
    C, M = 16, 2 * TRIP + 1003
    _wraps("head fwd b16", M // 2 + 1, items=M)
    _wraps("head bwd b16", M * (C // 8) // 2 + 1, items=M * (C // 8))
    rng = np.random.default_rng(K)
    x = O.round_bf16(rng.standard_normal((M, C)))
    w = (rng.standard_normal((1, 1, 1, C, K)) * 0.3).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(K)
    dy = rng.standard_normal((M, K)).astype(np.float32).astype(np.float64)
    tx, tw, tb = T16.g16(x, dev).requires_grad_(True), g(w, dev).requires_grad_(True), g(b, dev).requires_grad_(True)
    y = ops.head_conv(tx, tw, tb)
    assert y.dtype == torch.float32
    check_close("head fwd", y, x @ w[0, 0, 0] + b, 2e-6)
    y.backward(g(dy, dev))
    T16.check_bf16("head dx", tx.grad, dy @ w[0, 0, 0].T, noise=2e-6)
    check_close("head dw", tw.grad, (x.T @ dy).reshape(w.shape), 5e-6)
    check_close("head db", tb.grad, dy.sum(0), 5e-6, atol=1e-5)
