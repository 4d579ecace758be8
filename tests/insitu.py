"""In-situ ("teacher-forced") parity of one training step, forward AND backward, op by op against the fp64 oracle.

A Recorder wraps every op function the networks and the model reach through `ops.<name>` and keeps, per call, the tensors the op
actually received and produced; a hook on every op output clones the gradient that arrives there.  After the step, for every
tensor T the step differentiates (each op output, each parameter)

    grad(T) as the HIP step produced it  ==  sum over the consumers c of T of  VJP_c(c's actual inputs, c's actual incoming gradient)

with every VJP evaluated by an ADAPTER below: a pure function over float64 arrays built from oracle/vnet_oracle.py.  Every term is
local to one op, so the whole-network comparison's chaotic amplification never enters, and the statement is per TENSOR, which is
what pins the accumulate-in-the-producer machinery of ops.py (fork / _GradSlot, acc_src, GradSink, the side stream).

Not a conftest: tests import it (tests/test_insitu_host.py pins the adapters on the CPU, tests/test_hip_insitu_backward.py uses them).
"""
import collections
import inspect
import os
import re

import numpy as np
import torch

from oracle import vnet_oracle as O
from tests import unet_oracle as UO

BF = torch.bfloat16
F64 = np.float64


# ---------------------------------------------------------------------------------------------------------------------------
# which functions to wrap: the call sites, read from the code
# ---------------------------------------------------------------------------------------------------------------------------
NETWORK_SOURCES = ("networks.py", "layers2.py", "VNet.py")     # every ops.<name>( here is an op (or listed in NOT_AN_OP)
MODEL_SOURCE = "model.py"                                      # ... here only the names that have an adapter are ops
NOT_AN_OP = {"storage_is_bf16", "zero_bias_gradients", "VnetHipError"}      # switches / errors the networks reach through ops.
STRUCTURAL = {"fork", "cut", "cast_input", "bn_update_only"}                # recorded, not differentiated through an adapter


def op_call_sites():
    """(names the network modules call through ops.<name>(...), names model.py calls) -- enumerated from the source text."""
    import vnet_tensorflow_amd
    root = os.path.dirname(os.path.abspath(vnet_tensorflow_amd.__file__))
    pat = re.compile(r"\bops\.([A-Za-z_][A-Za-z_0-9]*)\(")

    def names(fname):
        with open(os.path.join(root, fname)) as f:
            return set(pat.findall(f.read()))
    net = set()
    for fname in NETWORK_SOURCES:
        net |= names(fname)
    return net - NOT_AN_OP, names(MODEL_SOURCE)


# ---------------------------------------------------------------------------------------------------------------------------
# oracle adapters: (arguments as float64 arrays / plain values, dy) -> forward value and {argument name: contribution}
# ---------------------------------------------------------------------------------------------------------------------------
# Tolerances are the ones the per-op tests hold the same kernels to (tests/test_hip_ops.py: _conv_case, _bn_act_case,
# _bn_chain_case, _input_block_case, test_head, test_softmax_loss, test_activation_standalone; tests/test_hip_head_fusion.py).
# rel-L2 per contribution; "fwd" is the forward output's.  The per-op tests' ABSOLUTE atols (1e-5 on unit-scale Gaussian data) are
# not carried over: on a real step's gradients (1e-3 .. 1e-9) they would forgive anything.
TOL = {
    "conv": dict(fwd=2e-6, x0=2e-6, x1=2e-6, w=2e-6, b=2e-6),
    "conv_transpose2": dict(fwd=2e-6, x=2e-6, w=2e-6, b=2e-6),
    "input_conv": dict(fwd=5e-6, w=1e-5, b=1e-5, gamma=5e-5, beta=5e-5),
    "bn_act": dict(fwd=5e-6, x=5e-5, residual=5e-5, gamma=2e-5, beta=2e-5, alpha=2e-5),
    "bn_chain": dict(fwd=1e-5, x=5e-5, g1=5e-5, g2=5e-5, g3=5e-5, b1=2e-5, b2=2e-5, b3=2e-5, alpha=2e-5),
    "bn_head": dict(fwd=1e-5, x=5e-5, residual=5e-5, g1=5e-5, g2=5e-5, g3=5e-5, b1=2e-5, b2=2e-5, b3=2e-5, alpha=2e-5, w=2e-6, b=2e-6),
    "bn_concat": dict(fwd=5e-6, x0=5e-5, x1=5e-5, gamma=2e-5, beta=2e-5),
    "head_conv": dict(fwd=2e-6, x=2e-6, w=2e-6, b=2e-6),
    # selection / one multiplication: exact up to the fp32 rounding of the one product (2^-24 = 6e-8) or of an accumulating add
    "max_pool2": dict(fwd=0.0, x=1e-7),
    "dropout": dict(fwd=2e-7, x=2e-7),
    "activation": dict(fwd=1e-6, x=1e-6, alpha=2e-6),
    "softmax_loss": dict(fwd=2e-6, logits=1e-5),
}
# (bn_head's forward is the logits of a batch-norm chain: the chain's forward figure, the loosest of its parts)
# bf16 storage: the fp32 tensors (parameter gradients, logits) where tests/test_hip_b16.py holds another figure than the fp32 test
TOL_B16 = {
    "bn_act": dict(gamma=1e-5, beta=1e-5, alpha=1e-5),
    "bn_chain": dict(g1=1e-4, g2=1e-4, g3=1e-4, b1=1e-4, b2=1e-4, b3=1e-4, alpha=1e-4),
    "head_conv": dict(fwd=1e-5, w=5e-6, b=5e-6),
}
# check_bf16's `noise` (fp32 accumulation noise relative to the tensor's largest value) per op kind, as tests/test_hip_b16.py passes
# it for the same kernels (forward value, data gradient); min_equal stays at check_bf16's 0.995 for every gradient.
NOISE_B16 = {
    "conv": (4e-6, 4e-6), "conv_transpose2": (4e-6, 4e-6), "bn_act": (4e-6, 2e-5), "bn_chain": (5e-5, 2e-4),
    "head_conv": (None, 2e-6), "dropout": (1e-7, 1e-7),
}
# arguments that carry a gradient requirement but that the op does not differentiate (the producing conv's epilogue only READS
# the residual for the statistics; mean / invstd of the input block are functions of the image alone)
NOT_DIFFERENTIATED = {"conv": {"bn_residual"}, "input_conv": {"bn_residual", "mean", "invstd", "img"}}


def _act(z, kind, alpha):
    if kind == "prelu":
        return O.prelu(z, alpha)
    if kind == "relu":
        return O.relu(z)
    if kind == "lrelu":
        return O.leaky_relu(z)
    assert kind in (None, "none"), kind
    return z


def _var(a):
    return None if a is None else O.Var(a)


def _g(v, like=None):
    """A tape variable's gradient; zeros when nothing reached it."""
    if v is None:
        return None
    return v.g if v.g is not None else np.zeros_like(v.v)


def _colsum(dy):
    return dy.reshape(-1, dy.shape[-1]).sum(0)


def _colabs(g):
    """Per channel, the sum of magnitudes of what a per-channel gradient sums over the voxels -- the scale of its fp32 error."""
    return np.abs(g).reshape(-1, g.shape[-1]).sum(0)


def a_conv(A, dy):
    x = A["x0"] if A.get("x1") is None else np.concatenate((A["x0"], A["x1"]), -1)
    C0, I = A["x0"].shape[-1], A["w"].shape[-2]
    x = x[..., :I]                                             # (the cast network input carries zero channels behind the real ones)
    w = O.round_bf16(A["w"]).astype(x.dtype) if A["_b16"] else A["w"]      # bf16 storage: the kernels round every spatial filter
    y = O.conv_nd_fwd(x, w, A["stride"]) + A["b"]
    if dy is None:
        return y, {}
    need_dx = I >= C0 and any(A.get("_req", {}).get(k, True) for k in ("x0", "x1"))
    dx, dw = O.conv_nd_bwd(x, w, dy, A["stride"], need_dx=need_dx)
    out = {"w": dw, "b": _colsum(dy), "_abs": {"b": _colabs(dy)}}      # (straight-through: dw goes to the fp32 master filter)
    if need_dx:
        out["x0"] = dx[..., :C0]
        if A.get("x1") is not None:
            out["x1"] = dx[..., C0:]
    return y, out


def a_conv_transpose2(A, dy):
    w = O.round_bf16(A["w"]).astype(A["x"].dtype) if A["_b16"] else A["w"]
    y = O.conv_nd_transpose_fwd(A["x"], w, tuple(int(v) for v in A["out_spatial"]), 2) + A["b"]
    if dy is None:
        return y, {}
    _, dw = O.conv_nd_bwd(dy, A["w"], A["x"], 2, need_dx=False)
    return y, {"x": O.conv_nd_fwd(dy, w, 2), "w": dw, "b": _colsum(dy), "_abs": {"b": _colabs(dy)}}


def a_input_conv(A, dy):
    """conv5(BN(tile(img))) + b with the batch-norm's statistics AS GIVEN (they belong to the image, not to the tape)."""
    C = A["w"].shape[-2]
    xhat = (O.tile_channels(O.Var(A["img"]), C).v - A["mean"]) * A["invstd"]
    xn = xhat * A["gamma"] + A["beta"]
    y = O.conv_nd_fwd(xn, A["w"], 1) + A["b"]
    if dy is None:
        return y, {}
    dxn, dw = O.conv_nd_bwd(xn, A["w"], dy, 1)
    return y, {"w": dw, "b": _colsum(dy), "gamma": _colsum(dxn * xhat), "beta": _colsum(dxn),
               "_abs": {"b": _colabs(dy), "gamma": _colabs(dxn * xhat), "beta": _colabs(dxn)}}


def _bn_tape(A, kind, x, r):
    """The batch-norm (chain) of bn_act / bn_chain / bn_head on the tape: returns (y, {argument name: Var}, nodes); nodes = the
    batch-norm outputs as (gamma name, beta name, Var) and the activation as ("alpha", pre-activation Var, y) for _bn_abs."""
    v = {k: _var(A.get(k)) for k in ("g1", "b1", "g2", "b2", "g3", "b3", "alpha")}
    s = O.add(x, r) if r is not None else x
    nodes = []

    def bn(t, i):
        out = O.batch_norm_train(t, v["g%d" % i], v["b%d" % i])
        nodes.append(("g%d" % i, "b%d" % i, out))
        return out
    if kind < 0:
        z = bn(s, 1)
    elif kind == 0:                                            # act(BN3(BN1(x) + BN2(BN1(x))))
        y1 = bn(s, 1)
        z = bn(O.add(y1, bn(y1, 2)), 3)
    else:                                                      # act(BNb(x + BNa(x)))
        z = bn(O.add(s, bn(s, 1)), 2)
    y = _act(z, A.get("act"), v["alpha"])
    if v["alpha"] is not None:
        nodes.append(("alpha", z, y))
    return y, v, nodes


def _bn_abs(v, nodes):
    """After the backward sweep: per channel, the summed magnitudes behind every gamma / beta / alpha gradient of the tape."""
    out = {}
    for a, b, node in nodes:
        if a == "alpha":
            out["alpha"] = _colabs(node.g * np.minimum(b.v, 0.0)) if node.g is not None else None
            continue
        if node.g is None:
            continue
        gam = np.where(v[a].v == 0, 1.0, v[a].v)
        out[b] = _colabs(node.g)
        out[a] = _colabs(node.g * (node.v - v[b].v) / gam)
    return out


def _bn_grads(v, names=("g1", "b1", "g2", "b2", "g3", "b3", "alpha")):
    return {k: _g(v[k]) for k in names if v.get(k) is not None}


def a_bn_act(A, dy):
    x, r = O.Var(A["x"]), _var(A.get("residual"))
    xs = O.tile_channels(x, A["gamma"].size) if A.get("tile") else x
    y, v, nodes = _bn_tape(dict(g1=A["gamma"], b1=A["beta"], alpha=A.get("alpha") if A.get("act") == "prelu" else None, act=A.get("act")),
                           -1, xs, r)
    if dy is None:
        return y.v, {}
    O.backward(y, seed=dy)
    ab = _bn_abs(v, nodes)
    out = {"x": _g(x), "gamma": _g(v["g1"]), "beta": _g(v["b1"]), "_abs": {"gamma": ab.get("g1"), "beta": ab.get("b1"), "alpha": ab.get("alpha")}}
    if r is not None:
        out["residual"] = _g(r)
    if v["alpha"] is not None:
        out["alpha"] = _g(v["alpha"])
    return y.v, out


def a_bn_chain(A, dy):
    x = O.Var(A["x"])
    B = dict(A)
    if A.get("act") != "prelu":
        B["alpha"] = None
    y, v, nodes = _bn_tape(B, int(A["kind"]), x, None)
    if dy is None:
        return y.v, {}
    O.backward(y, seed=dy)
    return y.v, dict(_bn_grads(v), x=_g(x), _abs=_bn_abs(v, nodes))


def a_bn_head(A, dy):
    x, r = O.Var(A["x"]), _var(A.get("residual"))
    B = dict(A)
    if A.get("act") != "prelu":
        B["alpha"] = None
    y, v, nodes = _bn_tape(B, int(A["kind"]), x, r)
    w, b = O.Var(A["w"]), O.Var(A["b"])
    logits = O.convolution(y, w, b)                            # 1x1x1: no operand rounding in any mode
    if dy is None:
        return logits.v, {}
    O.backward(logits, seed=dy)
    out = dict(_bn_grads(v), x=_g(x), w=_g(w), b=_g(b), _abs=dict(_bn_abs(v, nodes), b=_colabs(np.asarray(dy))))
    if r is not None:
        out["residual"] = _g(r)
    return logits.v, out


def a_bn_concat(A, dy):
    x0, x1, g, b = O.Var(A["x0"]), O.Var(A["x1"]), O.Var(A["gamma"]), O.Var(A["beta"])
    y = O.batch_norm_train(O.concat_channels(x0, x1), g, b)
    C0 = A["x0"].shape[-1]
    fwd = (y.v[..., :C0], y.v[..., C0:])
    if dy is None:
        return fwd, {}
    seed = np.concatenate([d if d is not None else np.zeros_like(f) for d, f in zip(dy, fwd)], -1)
    O.backward(y, seed=seed)
    return fwd, {"x0": _g(x0), "x1": _g(x1), "gamma": _g(g), "beta": _g(b),
                 "_abs": {"beta": _colabs(seed), "gamma": _colabs(seed * (y.v - b.v) / np.where(g.v == 0, 1.0, g.v))}}


def a_head_conv(A, dy):
    x, w, b = O.Var(A["x"]), O.Var(A["w"]), O.Var(A["b"])
    y = O.convolution(x, w, b)
    if dy is None:
        return y.v, {}
    O.backward(y, seed=dy)
    return y.v, {"x": _g(x), "w": _g(w), "b": _g(b), "_abs": {"b": _colabs(np.asarray(dy))}}


def a_max_pool2(A, dy):
    x = O.Var(A["x"])
    y = UO.max_pool2(x)                                        # the gradient of a window goes to its FIRST maximum in scan order
    if dy is None:
        return y.v, {}
    O.backward(y, seed=dy)
    return y.v, {"x": _g(x)}


def a_dropout(A, dy):
    """With the mask the kernel drew: a kept value is nonzero unless the input was zero."""
    x = O.Var(A["x"])
    mask = ((A["_out"] != 0) | (A["x"] == 0)).astype(A["x"].dtype)
    y = O.dropout(x, float(A["rate"]), mask=mask)
    if dy is None:
        return y.v, {}
    O.backward(y, seed=dy)
    return y.v, {"x": _g(x)}


def a_activation(A, dy):
    x, alpha = O.Var(A["x"]), _var(A.get("alpha") if A["act"] == "prelu" else None)
    y = _act(x, A["act"], alpha)
    if dy is None:
        return y.v, {}
    O.backward(y, seed=dy)
    out = {"x": _g(x)}
    if alpha is not None:
        out["alpha"] = _g(alpha)
        out["_abs"] = {"alpha": _colabs(np.asarray(dy) * np.minimum(x.v, 0.0))}
    return y.v, out


def a_softmax_loss(A, dy):
    z = O.Var(A["logits"])
    lab = np.asarray(A["labels"])
    if lab.ndim == z.v.ndim - 1:
        lab = lab[..., None]
    w = A.get("weights")
    loss, _ = O.loss_head(z, lab, A["loss_name"], tuple(w) if w is not None else (), float(A["alpha"]))
    if dy is None:
        return loss.v, {}
    O.backward(loss, seed=np.asarray(dy, dtype=z.v.dtype).reshape(np.shape(loss.v)))
    return loss.v, {"logits": _g(z)}


ADAPTERS = {"conv": a_conv, "conv_transpose2": a_conv_transpose2, "input_conv": a_input_conv, "bn_act": a_bn_act, "bn_chain": a_bn_chain,
            "bn_head": a_bn_head, "bn_concat": a_bn_concat, "head_conv": a_head_conv, "max_pool2": a_max_pool2, "dropout": a_dropout,
            "activation": a_activation, "softmax_loss": a_softmax_loss}


# ---------------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------------
def tkey(t):
    """Identity of a forward tensor: its storage address, shape and dtype.  The record keeps every tensor it names alive, so no
    address is recycled; a fork's two views and a no-op's result (dropout at rate 0, cut on one rank) share the key of their base."""
    return (t.data_ptr(), tuple(t.shape), t.dtype)


Call = collections.namedtuple("Call", "index name args req outs out_req")
# one consumer's share of a tensor's gradient: the call, the argument, the oracle's contribution, the per-op rel-L2 tolerance and (a
# per-channel parameter gradient) what a correct fp32 column sum may be off by per channel, else None
Term = collections.namedtuple("Term", "call arg value tol colsum_atol")


def _tensors(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (tuple, list)):
        for e in v:
            for t in _tensors(e):
                yield t


class Recorder(object):
    """rec = Recorder(monkeypatch): from here on every op call of the networks / the model on real tensors is recorded (calls on
    meta tensors -- the shape pass that creates the variables -- are not).  monkeypatch restores ops when the test ends."""

    def __init__(self, monkeypatch):
        from vnet_tensorflow_amd import ops
        self.ops = ops
        self.calls, self.grads, self.forks = [], {}, []
        self.alias = {}                 # view / pass-through key -> base key
        self.families, self.side_launches, self.epilogue_stats = [], 0, 0
        self.store16 = False
        self._depth, self._inner = 0, [0]
        net_names, model_names = op_call_sites()
        unknown = sorted(n for n in net_names if n not in ADAPTERS and n not in STRUCTURAL)
        assert not unknown, "the networks call ops.%s, which tests/insitu.py has no adapter for" % ", ops.".join(unknown)
        self.wrapped = sorted(net_names | (model_names & set(ADAPTERS)))
        for name in self.wrapped:
            self._wrap(monkeypatch, name)
        for name in ("_conv_launch", "_wgrad_launch"):           # which kernel family every launch was routed to
            self._wrap_launch(monkeypatch, name)

    def _wrap_launch(self, monkeypatch, name):
        orig = getattr(self.ops, name)

        def f(r, *a, **k):
            self.families.append(r.family)
            self.side_launches += self.ops._LAUNCH_ON[0] is not None       # (redirected to the parameter-gradient stream)
            return orig(r, *a, **k)
        monkeypatch.setattr(self.ops, name, f)

    def _wrap(self, monkeypatch, name):
        orig = getattr(self.ops, name)
        sig = inspect.signature(orig)

        def f(*a, **k):
            self._depth += 1
            self._inner.append(0)
            try:
                out = orig(*a, **k)
            finally:
                self._depth -= 1
                inner = self._inner.pop()
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            if any(t.device.type == "meta" for v in bound.arguments.values() for t in _tensors(v)):
                return out
            if inner:                       # a composition of recorded ops (bn_head run as bn_act / bn_chain + head_conv): its parts are the record
                self._inner[-1] += inner
                return out
            self._inner[-1] += 1
            self._record(name, bound.arguments, out)
            return out
        monkeypatch.setattr(self.ops, name, f)

    def _record(self, name, arguments, out):
        args, req = {}, {}
        self.store16 = self.store16 or self.ops.storage_is_bf16()
        for k, v in arguments.items():
            if isinstance(v, torch.Tensor):
                args[k], req[k] = v.detach(), bool(v.requires_grad and v.is_floating_point())
            else:
                args[k] = v
        outs_live = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        outs = tuple(o.detach() if isinstance(o, torch.Tensor) else None for o in outs_live)
        out_req = tuple(bool(isinstance(o, torch.Tensor) and o.requires_grad and o.is_floating_point()) for o in outs_live)
        call = Call(len(self.calls), name, args, req, outs, out_req)
        self.calls.append(call)
        if name == "fork":
            base = tkey(args["x"])
            self.forks.append((base, tkey(outs[0]), tkey(outs[1])))
            for o in outs:
                self.alias[tkey(o)] = base
            return
        if name == "conv" and getattr(outs_live[0], "_vnet_stats", None) is not None:
            self.epilogue_stats += 1
        ins = {tkey(t) for t in args.values() if isinstance(t, torch.Tensor)}
        for o, live, rq in zip(outs, outs_live, out_req):
            if o is None:
                continue
            k = tkey(o)
            if k in ins:                    # handed through unchanged (cut on one rank, dropout at rate 0)
                continue
            if rq and name not in STRUCTURAL:
                live.register_hook(lambda g, k=k: self._grab(k, g))

    def _grab(self, k, g):
        # a CLONE, never the gradient tensor itself: autograd accumulates later gradients in place into a tensor it holds the last
        # reference to (see _ConvFn._backward) and the slot mechanism adds into these tensors -- a kept reference would change the
        # behaviour under test
        assert k not in self.grads, "two gradients arrived at one op output"
        self.grads[k] = g.detach().clone()

    def base(self, k):
        while k in self.alias and self.alias[k] != k:
            k = self.alias[k]
        return k

    def kinds(self):
        return sorted(set(c.name for c in self.calls))


# ---------------------------------------------------------------------------------------------------------------------------
# evaluating a record
# ---------------------------------------------------------------------------------------------------------------------------
def np64(t, dtype=F64):
    if t is None:
        return None
    if t.is_floating_point():
        return t.detach().float().cpu().numpy().astype(dtype)
    return t.detach().cpu().numpy()


def _is_identity(call):
    ins = {tkey(t) for t in call.args.values() if isinstance(t, torch.Tensor)}
    return all(o is None or tkey(o) in ins for o in call.outs)


def evaluate_call(rec, call, dtype=F64):
    """The adapter of one recorded call on its actual inputs and its actual incoming gradient(s), in `dtype` (float64: the oracle;
    float32: the yardstick of what a plain fp32 implementation of the same VJP achieves).  Returns (forward value, contributions)."""
    A = {k: (np64(v, dtype) if isinstance(v, torch.Tensor) else v) for k, v in call.args.items()}
    A["_b16"] = any(isinstance(v, torch.Tensor) and v.dtype == BF for v in call.args.values())
    A["_out"] = np64(call.outs[0], dtype)
    A["_req"] = call.req
    dys = [np64(rec.grads.get(tkey(o)), dtype) if o is not None and rq else None for o, rq in zip(call.outs, call.out_req)]
    if call.name == "softmax_loss" and dys[0] is None:
        dys[0] = np.ones((), dtype)                            # the step's seed
    if call.name == "bn_concat":
        dy = tuple(dys) if any(d is not None for d in dys) else None
    else:
        dy = dys[0]
    return ADAPTERS[call.name](A, dy)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, F64) - np.asarray(b, F64)) / (np.linalg.norm(np.asarray(b, F64)) + 1e-300))


def half_ulp_bf16(v):
    """Half a bf16 ulp at |v| (8 significant bits: 2^(floor(log2 |v|) - 8)); 0 at 0."""
    v = np.abs(np.asarray(v, F64))
    with np.errstate(divide="ignore"):
        return np.where(v > 0, 2.0 ** (np.floor(np.log2(np.where(v > 0, v, 1.0))) - 8), 0.0)


def bf16_two_consumer_excess(got, contribs, literal=False):
    """A bf16 tensor with two consumers holds RNE(RNE(a) + b), in either order: one half ulp at the first contribution plus one at
    the sum, |got - exact| <= (hu(c_first) + hu(|total| + hu(c_first))) (1 + 1e-3) + 4e-6 scale elementwise, taken for the order
    that allows more.  Returns the largest error / bound ratio (<= 1 passes).
    literal: the bound in the relative form 2^-9 (max|c_i| + |total|) instead.  Half an ulp is 2^-9 |v| only at the top of a binade
    and 2^-8 |v| at its bottom (check_bf16 writes the half ulp as 2^-8 |v| for that reason), so exact RNE(RNE(a) + b) exceeds the
    literal form by up to 2x (tests/test_insitu_host.py::test_two_consumer_bf16_bound shows it); the ulp form above is the tightest
    bound a correct double rounding meets, and is never looser than 2^-8 (max|c_i| + |total|)."""
    total = sum(contribs)
    scale = float(np.abs(total).max()) + 1e-30
    if literal:
        big = np.max(np.abs(np.stack(contribs)), axis=0)
        tol = 2.0 ** -9 * (big + np.abs(total)) * (1 + 1e-3) + 4e-6 * scale
    else:
        first = np.max(np.stack([half_ulp_bf16(c) for c in contribs]), axis=0)
        tol = (first + half_ulp_bf16(np.abs(total) + first)) * (1 + 1e-3) + 4e-6 * scale
    return float((np.abs(got - total) / tol).max())


class Tensor(object):
    """One differentiated tensor of the record: who produced it, the gradient the step left, and its consumers' contributions."""
    __slots__ = ("label", "got", "dtype", "terms", "param")

    def __init__(self, label, got, dtype, param=False):
        self.label, self.got, self.dtype, self.terms, self.param = label, got, dtype, [], param


def collect(rec, named_params, flat=None, dtype=F64, forward=True):
    """Walks the record once: per call the adapter's forward value and contributions.  Returns (tensors: key -> Tensor with .terms =
    [(call, argument, contribution, tolerance)], forward: [(call, output index, got, exact, tolerance)])."""
    params = {}
    for n, p in named_params:
        params[tkey(p)] = n
    tensors, fwd = collections.OrderedDict(), []
    producer = {}
    for c in rec.calls:
        if c.name in STRUCTURAL or _is_identity(c):
            continue
        for i, (o, rq) in enumerate(zip(c.outs, c.out_req)):
            if o is not None and rq:
                producer[tkey(o)] = "%s#%d%s" % (c.name, c.index, "[%d]" % i if len(c.outs) > 1 and c.name == "bn_concat" else "")
    for c in rec.calls:
        if c.name in STRUCTURAL or _is_identity(c):
            continue
        b16 = any(isinstance(v, torch.Tensor) and v.dtype == BF for v in c.args.values())
        tol = dict(TOL[c.name])
        if rec.store16 or b16:
            tol.update(TOL_B16.get(c.name, {}))
        exact, contrib = evaluate_call(rec, c, dtype)
        if forward:
            ex = exact if isinstance(exact, tuple) else (exact,)
            for i, e in enumerate(ex):
                fwd.append((c, i, c.outs[i], e, tol["fwd"]))
        skip = NOT_DIFFERENTIATED.get(c.name, set())
        for k, v in c.args.items():
            if not isinstance(v, torch.Tensor) or not c.req.get(k):
                continue
            if k in skip:
                continue
            assert k in contrib, "%s#%d: argument %s requires a gradient and the adapter has none for it" % (c.name, c.index, k)
            key = rec.base(tkey(v))
            if key in params:
                label, isp = params[key], True
            else:
                assert key in producer, "%s#%d: argument %s was produced by no recorded op" % (c.name, c.index, k)
                label, isp = producer[key], False
            t = tensors.get(key)
            if t is None:
                t = tensors[key] = Tensor(label, None, v.dtype, isp)
            scale = contrib.get("_abs", {}).get(k)
            if scale is not None:       # a per-channel gradient summed over n voxels: what its fp32 column sum may be off by
                n = max(int(np.prod(c.outs[0].shape[:-1])), 2)
                scale = np.log2(n) * 2.0 ** -24 * np.asarray(scale, F64).reshape(tuple(v.shape))
            t.terms.append(Term(c, k, np.asarray(contrib[k], dtype).reshape(tuple(v.shape)), tol[k], scale))
    # parameters nothing differentiates (dead batch-norms, conv biases of the closed form count through their conv)
    for n, p in named_params:
        if tkey(p) not in tensors:
            tensors[tkey(p)] = Tensor(n, None, p.dtype, True)
    for n, p in named_params:
        t = tensors[tkey(p)]
        t.got = np64(p.grad) if p.grad is not None else None
    for key, t in tensors.items():
        if not t.param:
            g = rec.grads.get(key)
            t.got = np64(g) if g is not None else None
    return tensors, fwd


def check_step(rec, named_params, zero_bias=True, log=None, yardstick=False, strict=True):
    """Every differentiated tensor and every forward output of the record against the oracle, by the rules of
    tests/test_hip_insitu_backward.py's docstring.  Returns (number of tensors checked, op kinds checked, per-kind worst figures);
    raises AssertionError naming the first failing tensor AFTER all figures were collected (log: a callable that gets a line per tensor)."""
    from tests.test_hip_b16 import check_bf16
    tensors, fwd = collect(rec, named_params)
    y32 = None
    if yardstick:                       # the same VJPs in plain float32 on the same inputs (reported, never a bound by itself)
        y32 = collect(rec, named_params, dtype=np.float32, forward=False)[0]
    say = log or (lambda s: None)
    failures, worst, kinds = [], {}, set()

    def note(kind, what, figure, bound, yard=None):
        w = worst.setdefault((kind, what), [0.0, bound, 0.0])
        w[0], w[1] = max(w[0], figure), bound
        if yard is not None:
            w[2] = max(w[2], yard)

    # ---- forward --------------------------------------------------------------------------------------------------------
    for c, i, got, exact, tol in fwd:
        tag = "forward %s#%d[%d]" % (c.name, c.index, i)
        if got.dtype == BF:
            noise = NOISE_B16.get(c.name, (4e-6, 4e-6))[0]
            try:
                eq = check_bf16(tag, got, exact, noise=noise, min_equal=0.97 if c.name == "bn_chain" else 0.995)
                note(c.name, "fwd(b16, 1-equal)", 1.0 - eq, 0.03 if c.name == "bn_chain" else 0.005)
            except AssertionError as e:
                failures.append(str(e))
        else:
            gv = np64(got)
            r = rel_l2(gv, exact) if np.linalg.norm(exact) > 0 else float(np.abs(gv).max())
            note(c.name, "fwd", r, tol)
            if c.name == "max_pool2":
                ok = np.array_equal(gv, exact)
            else:
                ok = r <= tol
            if not ok or not np.isfinite(gv).all():
                failures.append("%s: rel-L2 %.3e (tol %.1e)" % (tag, r, tol))
        say("%-40s ok" % tag)
    # ---- backward: per tensor ---------------------------------------------------------------------------------------------
    checked = 0
    for key, t in tensors.items():
        names = sorted(set(x.call.name for x in t.terms))
        kind = "+".join(names) if names else "none"
        what = "+".join(sorted(set(x.arg for x in t.terms))) or "-"
        tag = "grad(%s) <- %s" % (t.label, ", ".join("%s#%d.%s" % (x.call.name, x.call.index, x.arg) for x in t.terms) or "nothing")
        contribs = [x.value for x in t.terms]
        if not t.terms:
            # nobody differentiates it: its gradient is the empty sum
            ok = t.got is None or not np.any(t.got)
            if not ok:
                failures.append("%s: expected an all-zero gradient" % tag)
            checked += 1
            continue
        if t.got is None:
            failures.append("%s: no gradient arrived" % tag)
            continue
        total = sum(contribs)
        tol = max(x.tol for x in t.terms)
        bias_zero = (zero_bias and t.param and all(x.call.name in ("conv", "conv_transpose2", "input_conv") and x.arg == "b" for x in t.terms))
        if bias_zero:
            # closed form: a conv bias in front of a batch-norm has gradient 0 identically, and the step leaves EXACTLY 0.  What the
            # oracle sums from the ACTUAL dy is what is left of a sum that cancels (the batch-norm's data gradient has zero column
            # sums): fp32 round-off, or -- a dy stored as bf16 -- the sum of its roundings, at most half an ulp (2^-8 |dy|) each
            bound = 0.0
            for x in t.terms:
                dyt = rec.grads[tkey(x.call.outs[0])]
                n = max(dyt.numel() // dyt.shape[-1], 2)
                bound += float(_colabs(np64(dyt)).max()) * (2.0 ** -8 if dyt.dtype == BF else np.log2(n) * 2.0 ** -24)
            resid = float(np.abs(total).max())
            note("conv", "b (closed-form 0; |oracle column sum| / bound)", resid / bound, 1.0)
            if np.any(t.got) or resid > bound:
                failures.append("%s: conv bias in front of a batch-norm: got max %.3e (must be exactly 0), oracle column sum %.3e (bound %.3e)"
                                % (tag, float(np.abs(t.got).max()), resid, bound))
        elif t.dtype == BF and len(contribs) == 1:
            c0 = t.terms[0].call
            noise = NOISE_B16.get(c0.name, (4e-6, 4e-6))[1]
            try:
                eq = check_bf16(tag, torch.from_numpy(t.got).to(BF), total, noise=noise)
                note(kind, what + " (b16, 1-equal)", 1.0 - eq, 0.005)
            except AssertionError as e:
                failures.append(str(e))
        elif t.dtype == BF:
            ex = bf16_two_consumer_excess(t.got, contribs)
            note(kind, what + " (b16 two consumers, err/bound)", ex, 1.0)
            note(kind, what + " (b16 two consumers, err / the 2^-9 relative form: reported, not asserted)",
                 bf16_two_consumer_excess(t.got, contribs, literal=True), float("nan"))
            if not ex <= 1.0:
                failures.append("%s: two-consumer bf16 sum off by %.3f x its bound" % (tag, ex))
        else:
            r = rel_l2(t.got, total)
            # cancelling sums.  Two consumers: the sum's error is relative to what was added, not to what is left.  A per-channel
            # parameter gradient (bias, gamma, beta, alpha) is a column sum over N voxels: pairwise / blocked fp32 summation errs by up
            # to log2(N) 2^-24 of the column's sum of MAGNITUDES (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), which
            # is all there is where the true sum is analytically 0 (a bias or beta in front of another batch-norm).
            err = np.abs(t.got - total)
            m = float(err.max())
            atol, ok_abs = None, False
            if all(x.colsum_atol is not None for x in t.terms):
                lim = sum(x.colsum_atol for x in t.terms)
                atol, ok_abs = float(lim.max()), bool((err <= lim).all())
                note(kind, what + " (|err| / column-sum bound)", float((err / np.maximum(lim, 1e-300)).max()), 1.0)
            elif len(contribs) > 1:
                atol = tol * float(sum(np.abs(v).max() for v in contribs))
                ok_abs = m <= atol
            yard = rel_l2(sum(x.value for x in y32[key].terms), total) if y32 is not None else None
            note(kind, what, r, tol, yard)
            ok = np.isfinite(t.got).all() and (r <= tol or ok_abs)
            if not ok:
                failures.append("%s: rel-L2 %.3e (tol %.1e), max-abs %.3e (atol %s)%s" % (
                    tag, r, tol, m, atol, "" if yard is None else ", fp32-CPU yardstick %.3e" % yard))
            say("%-60s rel-L2 %.3e tol %.1e%s" % (tag[:60], r, tol, "" if yard is None else " yard %.3e" % yard))
        checked += 1
        kinds.update(names)
    if not strict:                      # (measurement scripts: every figure, the failures as text)
        return checked, kinds, worst, failures
    assert not failures, "%d in-situ checks failed:\n  %s" % (len(failures), "\n  ".join(failures[:40]))
    return checked, kinds, worst


def differentiated_count(rec, named_params):
    """Independent count of what check_step must have checked: the parameters, plus every recorded op output that requires a
    gradient and that some recorded op consumes (the loss, which nothing consumes, is the step's seed)."""
    consumed = set()
    for c in rec.calls:
        if c.name in STRUCTURAL or _is_identity(c):
            continue
        skip = NOT_DIFFERENTIATED.get(c.name, set())
        for k, v in c.args.items():
            if isinstance(v, torch.Tensor) and c.req.get(k) and k not in skip:
                consumed.add(rec.base(tkey(v)))
    pkeys = {tkey(p) for _, p in named_params}
    outs = set()
    for c in rec.calls:
        if c.name in STRUCTURAL or _is_identity(c):
            continue
        for o, rq in zip(c.outs, c.out_req):
            if o is not None and rq and rec.base(tkey(o)) in consumed:
                outs.add(rec.base(tkey(o)))
    return len(pkeys) + len(outs - pkeys)
