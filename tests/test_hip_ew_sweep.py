"""-m gpu: the exact per-element sweep of csrc/elementwise.hip (variant table, generator, oracle and tiers: tests/ew_sweep.py; the
design is proved exact on the host by tests/test_ew_sweep_host.py).

One test per case.  The row's entry points are called directly through _lib.lib(), as test_bn_moments_exact does, so that mean,
invstd, the backward sums, M_total, coef and gscale stay the dyadic operands the oracle was given.  Cases that fit run inside
tests.guard.guarded(): every tensor is carved from the arena, outputs and scratch hold 0xFF (NaN) before the launch, the workspace
is exactly the queried size; afterwards the guards are intact, no input has changed and no output element is left unwritten.  The
one case per row past the grid cap runs on plain tensors (poisoned the same way) after the trips test's _wraps() assertions.  Every
element of every output is then held to its tier: E and R with `==` on values, B within the bound the oracle derived.

A failure names the case, the output, how many elements are wrong, the first and the last wrong index, and how the wrong indices
fall relative to the row's units (a thread's vector, a block's slot, the grid's slot, the unrolled group): a tail bug reads as one.

THAT IT CAN FAIL.  Value-only mutations of elementwise.hip (no address, mask or trip count moved), each built into a library of
its own from a scratch copy of the tree and run once on the MI355X against this file's cases of the family and against the per-op
and trips tests the parent commit holds the same kernels with:
(six mutants; "parent" = tests/test_hip_ops.py, test_hip_b16.py, test_hip_elementwise_trips.py and test_hip_insitu_backward.py
on the kernels concerned, run against the same mutated library; the unmutated library passes all 483 cases of this file).
 1. An apply kernel's last vector.  bn_act_bwd_apply_kernel<true>: the `xh * k2` term times 1.0001f in the LAST quad only
    (idx + 1 == nq).  Parent: all 44 tests pass (test_bn_act 10 + random cases, test_bn_chain, test_activation_standalone, the trips
    file's test_bn_act 12 / test_bn_chain / test_bn_concat / test_activation, the in-situ backward file).  This file: 12 of the 21
    selected cases fail -- all 9 bn-apply-vec cases, the capped one included ("3 of 1028 elements wrong, first at 1024, last at 1027
    ... 3 of 3 wrong elements in the LAST slot, 3 in the last item") and the 3 bn-bwd-composite cases whose width takes the vector
    kernel; the C = 3 composite case and the 8 act-bwd-vec cases pass, as they must (scalar kernel; identity: k2 = 0).
 2. A clamped duplicate load not zeroed in one unrolled slot.  bn_act_bwd_reduce_kernel<0>: `if (!ok && u + 1 != U)` -- the
    duplicate's dy survives in the last slot of the group.  Parent: 26 of 44 fail (dx rel-L2 3e-2: at their sizes a quarter of the
    threads hold a duplicate).  This file: 10 of 20 fail -- 7 of the 8 bn-reduce-m0 cases, the capped one included (C = 8, M = 256
    fills its last group and passes), the two prelu act-bwd-vec cases (dalpha through the same kernel) and the M = 64 composite case;
    the other activations' act-bwd-vec cases launch no reduce and pass.
 3. A bf16 twin's second half-trip.  bn_act_bwd_reduce_b16_kernel: xhat times 1.0001f where u == 1.  Parent: 15 of 26 fail
    (dgamma rel-L2 6.2e-5 against a bar of 1e-5).  This file: 18 of 27 bn16-reduce cases fail -- exactly those whose second slot holds
    data (n8 = 129 x 2, 33 x 8, 9 x 32, 257, 511 and the capped one), in each (BCAST, HASR) instantiation.
 4. An optimiser's scalar tail.  adam_kernel: lr_t * 1.0001f in the tail loop behind the float4 loop.  Parent: all 6 pass
    (test_optimisers, test_adam_branches 3, the step-state forms, test_adam_full_parameter_vector: 5e-7 of |p| + |step| + 1e-3).
    This file: the 6 adam-aligned cases fail ("1 of 1029 elements wrong, first at 1028 ... 1 of 1 wrong elements in the TAIL, 0 in
    the last whole vector"), the 6 adam-offset cases (scalar loop) pass.
 5. The last 16-byte unit of a bf16 tensor.  bn_act_fwd_b16_kernel: 0.5f added to z of the second half-trip's unit when it is
    the last of the tensor (j1 + 1 == n8).  Parent: 10 of 26 fail (check_bf16 counts wrong roundings per element: "8 of 524288
    values are not a correct rounding").  This file: 15 of 27 bn16-fwd cases fail, the ones that end in the second slot ("8 of 4088
    elements wrong, first at 4080, last at 4087 ... slot of the unrolled group: [1]").
 6. One row unit counted twice.  bn_stats_b16_kernel: the clamped duplicate of the LAST unit is kept (ok1 || idx + 1 == n8).
    Parent: 5 of 26 fail (the smallest shape, and four trips cases through the normalised output; C = 16 passes).  This file: 4 of
    9 bn16-stats cases fail on `sums` -- those that end in the first slot of a group, the capped one included ("got 4.0, expected
    2.0" at M = 1); the cases of mutation 5 are the complement.
The parent's per-op tests miss 1 and 4 -- a relative-L2 bar over a tensor, or a bar relative to |p| + |step|, does not see one
vector -- and catch 2, 3, 5 and 6 at some of their shapes; this file fails on each, names the elements, and passes the kernels the
mutation does not touch."""
import contextlib

import numpy as np
import pytest
import torch

from tests import ew_sweep as S
from tests import guard

pytestmark = pytest.mark.gpu
CASES = S.generate()
F32, BF, F64, U8, I32, I64 = torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32, torch.int64


def P(t):
    return t.data_ptr() if t is not None else None


class Env(object):
    """Tensors of one case: arena tensors (h: what guarded() yields) or plain poisoned ones (the case past the cap)."""

    def __init__(self, dev, h=None):
        from vnet_tensorflow_amd import _lib, ops
        self.dev, self.h, self.L, self.called, self.n = dev, h, _lib.lib(), [], 0
        self.st = ops._stream() if torch.device(dev).type == "cuda" else None
        self.keep = []                        # (a plain tensor whose pointer alone was passed on must outlive the launch)

    def i(self, a, dtype=F32):
        if self.h is not None:
            return self.h.g(a, None, dtype)
        self.keep.append(torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(self.dev))
        return self.keep[-1]

    def o(self, shape, dtype=F32):
        self.n += 1
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        if self.h is not None:
            return self.h.arena.tensor("out#%d" % self.n, shape, dtype, "out")
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        t.view(-1).view(U8).fill_(0xFF)
        self.keep.append(t)
        return t

    def io(self, a, dtype=F32):
        self.n += 1
        a = np.ascontiguousarray(a)
        if self.h is not None:
            return self.h.arena.tensor("inout#%d" % self.n, a.shape, dtype, "inout", torch.as_tensor(a).to(dtype))
        self.keep.append(torch.as_tensor(a).to(dtype).to(self.dev))
        return self.keep[-1]

    def ws(self, nbytes):
        if self.h is not None:
            return self.h.workspace(nbytes)
        self.keep.append(torch.full((int(nbytes),), 0xFF, dtype=U8, device=self.dev))
        return self.keep[-1]

    def call(self, name, *args):
        rc = getattr(self.L, name)(*args)
        assert rc == 0, "%s returned %d" % (name, rc)
        self.called.append(name)

    def query(self, name, *args):
        self.called.append(name)
        return getattr(self.L, name)(*args)


def _np(t):
    return t.detach().to(F64).cpu().numpy() if t.dtype != U8 else t.cpu().numpy().astype(np.float64)


# ---- the families' launches ------------------------------------------------------------------------------------------------------
def run_bn(env, p, d):
    M, C, b16, bc, op = p["M"], p["C"], p.get("b16"), int(bool(p.get("bcast"))), p["op"]
    act = S.ACT[p.get("act", "none")]
    T, sfx = (BF, "_b16") if b16 else (F32, "")
    x = env.i(d["x"].reshape(-1) if (b16 and bc) else d["x"], F32 if bc else T)
    r = env.i(d["r"], T) if p.get("res") else None
    vec = lambda k: P(env.i(d[k]))
    alpha = vec("alpha") if p.get("act") == "prelu" else None
    st = env.st
    if op == "moments":
        nb = env.query("vnet_bn_ws_bytes", C)
        sums, mean, invstd = env.o(2 * C, F64), env.o(C), env.o(C)
        if b16:
            env.call("vnet_bn_moments_b16", P(x), P(r), M, C, P(sums), P(env.ws(nb)), nb, st)
            env.call("vnet_bn_stats_b16", P(x), P(r), M, C, S.EPS, 0.99, P(mean), P(invstd), None, None, P(env.ws(nb)), nb, st)
        else:
            env.call("vnet_bn_moments", P(x), P(r), bc, M, C, P(sums), P(env.ws(nb)), nb, st)
            env.call("vnet_bn_stats", P(x), P(r), bc, M, C, S.EPS, 0.99, P(mean), P(invstd), None, None, P(env.ws(nb)), nb, st)
        return {"sums": sums, "mean": mean, "invstd": invstd}
    if op == "fwd":
        y = env.o((M, C), T)
        if p.get("identity"):
            env.call("vnet_act_fwd", P(x), M, C, act, alpha, P(y), st)
        else:
            env.call("vnet_bn_act_fwd" + sfx, P(x), P(r), bc, M, C, vec("mean"), vec("invstd"), vec("gamma"), vec("beta"), act, alpha, P(y), st)
        return {"y": y}
    dy = env.i(d["dy"], T)
    if op == "act_bwd":
        nb = env.query("vnet_bn_ws_bytes", C)
        dalpha, dx = env.o(C) if alpha else None, env.o((M, C))
        env.call("vnet_act_bwd", P(dy), P(x), M, C, act, alpha, P(dalpha), P(dx), P(env.ws(nb)), nb, st)
        return dict({"dx": dx}, **({"dalpha": dalpha} if alpha else {}))
    coef = (vec("mean"), vec("invstd"), vec("gamma"), vec("beta"), act, alpha)
    if op == "bwd":                                        # vnet_bn_act_bwd: reduce, then apply with the sums it wrote and M_total = M
        nb = env.query("vnet_bn_ws_bytes", C)
        dgamma, dbeta, dalpha, ds = env.o(C), env.o(C), env.o(C) if alpha else None, env.o((M, C))
        env.call("vnet_bn_act_bwd", P(dy), P(x), P(r), bc, M, C, *coef, P(dgamma), P(dbeta), P(dalpha), P(ds), P(env.ws(nb)), nb, st)
        return dict({"dgamma": dgamma, "dbeta": dbeta, "ds": ds}, **({"dalpha": dalpha} if alpha else {}))
    if op == "reduce":
        nb = env.query("vnet_bn_ws_bytes", C)
        dgamma, dbeta, dalpha = env.o(C), env.o(C), env.o(C) if alpha else None
        env.call("vnet_bn_act_bwd_reduce" + sfx, P(dy), P(x), P(r), bc, M, C, *coef, P(dgamma), P(dbeta), P(dalpha), P(env.ws(nb)), nb, st)
        return dict({"dgamma": dgamma, "dbeta": dbeta}, **({"dalpha": dalpha} if alpha else {}))
    ds = env.o((M, C), T)
    env.call("vnet_bn_act_bwd_apply" + sfx, P(dy), P(x), P(r), bc, M, C, *coef, vec("sdz"), vec("sdzx"), S.M_TOTAL,
             vec("ex") if p.get("ex") else None, P(ds), st)
    return {"ds": ds}


def run_partial(env, p, d):
    rows, C = p["M"], p["C"]
    mean, invstd, mean2, invstd2 = (env.o(C) for _ in range(4))
    env.call("vnet_bn_finalize_partial", P(env.i(d["part"])), rows, C, S.M_TOTAL, S.EPS, 0.99, P(mean), P(invstd), None, None, env.st)
    sums = env.i(np.concatenate([d["part"][:, 0].sum(0), d["part"][:, 1].sum(0)]), F64)
    env.call("vnet_bn_finalize", P(sums), S.M_TOTAL, C, S.EPS, 0.99, P(mean2), P(invstd2), None, None, env.st)
    return {"mean": mean, "invstd": invstd, "mean2": mean2, "invstd2": invstd2}


def run_small(env, p, d):
    M, C, act = p["M"], p["C"], S.ACT[p["act"]]
    x, r = env.i(d["x"], BF), env.i(d["r"], BF) if p["res"] else None
    vec = lambda k: P(env.i(d[k]))
    alpha = vec("alpha") if p["act"] == "prelu" else None
    if p["_family"] == "small_fwd":
        assert env.query("vnet_bn_small_ok", M, C) == 1
        mean, invstd, y = env.o(C), env.o(C), env.o((M, C), BF)
        env.call("vnet_bn_small_fwd_b16", P(x), P(r), M, C, S.small_eps(p), 0.99, vec("gamma"), vec("beta"), act, alpha, P(mean), P(invstd), None, None,
                 P(y), env.st)
        return {"mean": mean, "invstd": invstd, "y": y}
    dgamma, dbeta, dalpha, ds = env.o(C), env.o(C), env.o(C) if alpha else None, env.o((M, C), BF)
    env.call("vnet_bn_small_bwd_b16", P(env.i(d["dy"], BF)), P(x), P(r), M, C, vec("mean"), vec("invstd"), vec("gamma"), vec("beta"), act, alpha,
             P(dgamma), P(dbeta), P(dalpha), P(ds), env.st)
    return dict({"dgamma": dgamma, "dbeta": dbeta, "ds": ds}, **({"dalpha": dalpha} if alpha else {}))


def run_bn_head(env, p, d):
    M, C, K, op, act = p["M"], p["C"], p["K"], p["op"], S.ACT[p["act"]]
    x, r = env.i(d["x"]), env.i(d["r"]) if p["res"] else None
    vec = lambda k: P(env.i(d[k]))
    alpha = vec("alpha") if p["act"] == "prelu" else None
    coef = (vec("mean"), vec("invstd"), vec("gamma"), vec("beta"), act, alpha)
    w = env.i(d["w"])
    if op == "fwd":
        assert env.query("vnet_bn_head_ok", C, K) == 1
        rows = env.query("vnet_bn_head_stats_rows", M, C)
        y, logits, stats = env.o((M, C)), env.o((M, K)), env.o((rows, 2 * K))
        env.call("vnet_bn_act_head_fwd", P(x), P(r), M, C, *coef, P(w), vec("bias"), K, P(y), P(logits), P(stats), env.st)
        return {"y": y, "logits": logits, "stats": stats}
    dl = env.i(d["dl"])
    if op == "reduce":
        nb = env.query("vnet_bn_head_ws_bytes", C, K)
        dgamma, dbeta, dalpha, dw, db = env.o(C), env.o(C), env.o(C) if alpha else None, env.o((C, K)), env.o(K)
        env.call("vnet_bn_act_bwd_reduce_head", P(dl), P(w), K, P(x), P(r), M, C, *coef, P(dgamma), P(dbeta), P(dalpha), P(dw), P(db),
                 P(env.ws(nb)), nb, env.st)
        return dict({"dgamma": dgamma, "dbeta": dbeta, "dw": dw, "db": db}, **({"dalpha": dalpha} if alpha else {}))
    ds = env.o((M, C))
    env.call("vnet_bn_act_bwd_apply_head", P(dl), P(w), K, P(x), P(r), M, C, *coef, vec("sdz"), vec("sdzx"), S.M_TOTAL,
             vec("ex") if p.get("ex") else None, P(ds), env.st)
    return {"ds": ds}


def run_head(env, p, d):
    M, C, K, b16 = p["M"], p["C"], p["K"], p.get("b16")
    T, sfx = (BF, "_b16") if b16 else (F32, "")
    x, w = env.i(d["x"], T), env.i(d["w"])
    if p["op"] == "fwd":
        y = env.o((M, K))
        env.call("vnet_head_fwd" + sfx, P(x), P(w), P(env.i(d["bias"])), P(y), M, C, K, env.st)
        return {"y": y}
    nb = env.query("vnet_head_ws_bytes", C, K)
    dx, dw, db = env.o((M, C), T), env.o((C, K)), env.o(K)
    env.call("vnet_head_bwd" + sfx, P(x), P(w), P(env.i(d["dy"])), P(dx), P(dw), P(db), M, C, K, P(env.ws(nb)), nb, env.st)
    return {"dx": dx, "dw": dw, "db": db}


def run_colsum(env, p, d):
    M, C, b16 = p["M"], p["C"], p.get("b16")
    nb = env.query("vnet_colsum_b16_ws_bytes" if b16 else "vnet_colsum_ws_bytes", C)
    out = env.o(C)
    env.call("vnet_colsum_b16" if b16 else "vnet_colsum", P(env.i(d["x"], BF if b16 else F32)), P(out), M, C, P(env.ws(nb)), nb, env.st)
    return {"out": out}


def run_loss(env, p, d):
    B, V, K, kind = p["B"], p["M"], p["K"], p["kind"]
    z, lab = env.i(d["z"]), env.i(d["lab"], I32)
    w = P(env.i(d["w"])) if kind & 16 else None
    if p["op"] == "fwd":
        nb = env.query("vnet_loss_ws_bytes", B, K)
        sm, pred, loss, dice, coef = env.o((B, V, K)), env.o((B, V), I64), env.o(1), env.o(1), env.o(2 * B * K + 1)
        env.call("vnet_softmax_dice_fwd", P(z), P(lab), B, V, K, kind, w, 0.5, 1e-5, P(sm), P(pred), P(loss), P(dice), P(coef), P(env.ws(nb)), nb, env.st)
        return {"softmax": sm, "pred": pred, "loss": loss, "dice": dice, "coef": coef}
    dl = env.o((B, V, K))
    env.call("vnet_softmax_dice_bwd", P(z), P(lab), B, V, K, kind, w, 0.5, P(env.i(d["coef"])), P(env.i(d["gs"])), P(dl), env.st)
    return {"dlogits": dl}


def run_dice(env, p, d):
    B, V, K, jac = p["B"], p["M"], p["K"], p["jac"]
    po, pt = env.i(d["p"]), env.i(d["t"])
    if p["op"] == "fwd":
        nb = env.query("vnet_loss_ws_bytes", B, K) + 4
        dice, coef = env.o(1), env.o(2 * B * K + 1)
        env.call("vnet_dice_coe_fwd", P(po), P(pt), B, V, K, jac, P(env.i(d["w"])) if p["wx"] else None, 1e-5, P(dice), P(coef), P(env.ws(nb)), nb, env.st)
        return {"dice": dice, "coef": coef}
    dout = env.o((B, V, K))
    env.call("vnet_dice_coe_bwd", P(po), P(pt), B, V, K, jac, P(env.i(d["coef"])), P(env.i(d["gs"])), P(dout), env.st)
    return {"dout": dout}


def _state(env, lr, lr_t, step):
    st = env.io(np.zeros(32, np.uint8), U8)
    env.call("vnet_step_state_set", P(st), lr, lr_t, step, env.st)
    return st


def run_dropout(env, p, d):
    b16, rate, seed = p.get("b16"), p["rate"], d["seed"]
    n = p["M"] * (8 if b16 else 1)
    T = BF if b16 else F32
    x, dy, y, dx, mask = env.i(d["x"], T), env.i(d["dy"], T), env.o(n, T), env.o(n, T), env.o(n, U8)
    state = _state(env, 0.0, 0.0, d["step"]) if p["dev"] else None
    if b16:
        env.call("vnet_dropout_fwd_b16", P(x), P(y), P(mask), n, rate, seed, P(state), env.st)
        env.call("vnet_dropout_bwd_b16", P(dy), P(mask), P(dx), n, rate, env.st)
    else:
        if state is not None:
            env.call("vnet_dropout_fwd_dev", P(x), P(y), P(mask), n, rate, seed, P(state), env.st)
        else:
            env.call("vnet_dropout_fwd", P(x), P(y), P(mask), n, rate, seed, env.st)
        env.call("vnet_dropout_bwd", P(dy), P(mask), P(dx), n, rate, env.st)
    return {"mask": mask, "y": y, "dx": dx}


PAD = -77.0                                # what the floats around a 4-byte-offset view hold before and after the launch


def run_opt(env, p, d):
    n, kind, off, o = p["M"], p["kind"], p["off"], S.OPT
    bufs = {}

    def view(k, inout):
        a = np.concatenate([[PAD], d[k], [PAD] * 3]) if off else d[k]
        bufs[k] = env.io(a) if inout else env.i(a)
        return bufs[k].data_ptr() + 4 * off
    pp, g = view("p", True), view("g", False)
    assert pp % 16 == 4 * off
    state = _state(env, o["lr"], o["lr_t"], 3) if p["dev"] else None
    sfx = "_dev" if state is not None else ""
    if kind == "sgd":
        env.call("vnet_sgd_apply" + sfx, pp, g, n, P(state) if state is not None else o["lr"], o["gs"], env.st)
        names = ("p",)
    elif kind in ("momentum", "nesterov"):
        env.call("vnet_momentum_apply" + sfx, pp, g, view("acc", True), n, P(state) if state is not None else o["lr"], o["mom"], int(kind == "nesterov"),
                 o["gs"], env.st)
        names = ("p", "acc")
    else:
        env.call("vnet_adam_apply" + sfx, pp, g, view("m", True), view("v", True), n, P(state) if state is not None else o["lr_t"], o["b1"], o["b2"],
                 o["eps"], o["gs"], env.st)
        names = ("p", "m", "v")
    out = {}
    for k in names:
        if off:
            pads = torch.cat([bufs[k][:1], bufs[k][n + 1:]])
            assert bool((pads == PAD).all()), "%s: the floats around the offset view of `%s` changed" % (kind, k)
        out[k] = bufs[k][off:off + n]
    return out


def run_cast(env, p, d):
    M, C, Cpad = p["M"], p["C"], p["Cpad"]
    y = env.o((M, Cpad), BF)
    env.call("vnet_cast_bf16", P(env.i(d["x"])), P(y), M, C, Cpad, env.st)
    return {"y": y}


def run_patch(env, p, d):
    vol, cnt = env.io(d["vol"]), env.io(d["cnt"]) if p["count"] else None
    env.call("vnet_accumulate_patch", P(env.i(d["patch"])), P(vol), P(cnt), p["K"], p["M"], p["py"], p["px"], p["z0"], p["y0"], p["x0"],
             p["D"], p["H"], p["W"], env.st)
    return dict({"vol": vol}, **({"cnt": cnt} if cnt is not None else {}))


RUN = {"bn": run_bn, "partial": run_partial, "small_fwd": run_small, "small_bwd": run_small, "bn_head": run_bn_head, "head": run_head,
       "colsum": run_colsum, "loss": run_loss, "dice": run_dice, "dropout": run_dropout, "opt": run_opt, "cast": run_cast, "patch": run_patch}


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
ELEMENTWISE = ("y", "ds", "dx", "logits", "softmax", "pred", "dlogits", "dout", "mask", "p", "m", "v", "acc", "vol", "cnt")


def _where(case, name, n_out, bad):
    """How the wrong flat indices of an output of n_out elements fall relative to the row's units."""
    g = S.geom_of(case)
    if name not in ELEMENTWISE:
        return "a reduction's output of %d elements: wrong indices modulo 4: %s, modulo 8: %s" % (
            n_out, sorted(set(int(b) % 4 for b in bad)), sorted(set(int(b) % 8 for b in bad)))
    if g.vec and n_out == g.vec[0]:                          # a vector body with a scalar tail
        whole = g.vec[0] // g.vec[1] * g.vec[1]
        return "%d elements = %d whole vectors of %d and a tail of %d: %d of %d wrong elements in the TAIL, %d in the last whole vector" % (
            n_out, whole // g.vec[1], g.vec[1], n_out - whole, int((np.asarray(bad) >= whole).sum()), len(bad),
            int(((np.asarray(bad) >= whole - g.vec[1]) & (np.asarray(bad) < whole)).sum()))
    if g.items <= 0 or n_out % g.items != 0:
        return "output of %d elements, not a whole number per work item" % n_out
    per = n_out // g.items                                   # elements of one work item (a thread's vector, a row, a voxel)
    it = np.asarray(bad) // per
    stride = g.grid * g.per_block
    last_slot, last_block = (g.items - 1) // stride, (g.items - 1) // g.per_block
    parts = ["%d elements per work item, %d items; %d per block, %d per slot of the grid, %d slots a trip" % (per, g.items, g.per_block, stride, g.U),
             "wrong items %d .. %d" % (int(it.min()), int(it.max())),
             "%d of %d wrong elements in the LAST slot (slot %d), %d in the LAST block's share, %d in the last item" % (
                 int((it // stride == last_slot).sum()), len(bad), last_slot, int((it // g.per_block == last_block).sum()),
                 int((it == g.items - 1).sum())),
             "slots hit: %s" % sorted(set(int(v) for v in it // stride))[:8],
             "position in the item: %s" % sorted(set(int(b) % per for b in bad))[:16]]
    if g.U > 1:
        parts.append("slot of the unrolled group: %s" % sorted(set(int(v) for v in (it // stride) % g.U)))
    return "; ".join(parts)


def _check(case, name, tier, got, want, tol=None):
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape or got.size == want.size, "%s %s: shape %s, expected %s" % (S.cid(case), name, got.shape, want.shape)
    got, want = got.reshape(-1), want.reshape(-1)
    if tol is None:
        wrong = ~(got == want)                               # (NaN != anything: poison that was read or left behind counts)
    else:
        wrong = ~(np.abs(got - want) <= np.asarray(tol, np.float64).reshape(-1))
    if not wrong.any():
        return
    bad = np.nonzero(wrong)[0]
    lines = ["  [%d] got %r, expected %r%s" % (i, float(got[i]), float(want[i]), "" if tol is None else " +- %.3e" % float(np.asarray(tol).reshape(-1)[i]))
             for i in sorted(set(list(bad[:4]) + list(bad[-2:])))]
    raise AssertionError("%s: output `%s` (tier %s): %d of %d elements wrong, first at %d, last at %d\n  %s\n%s" % (
        S.cid(case), name, tier, bad.size, got.size, int(bad[0]), int(bad[-1]), _where(case, name, got.size, bad), "\n".join(lines)))


@contextlib.contextmanager
def _guarded(dev):
    arena = guard.Arena(dev, capacity=128 << 20)
    with guard.guarded(arena) as h:
        yield h
        torch.cuda.synchronize()
        arena.check()
        arena.check_written()
    del arena


@pytest.mark.parametrize("case", CASES, ids=S.cid)
def test_ew_sweep(dev, case):
    row = S.ROWS[case.row]
    p = S._with_row(case)
    p["_family"] = row.family
    d = S.operands(case)
    with contextlib.ExitStack() as stack:
        if case.capped:
            S.wraps(case)
            env = Env(dev)
        else:
            env = Env(dev, stack.enter_context(_guarded(dev)))
        outs = RUN[row.family](env, p, d)
        torch.cuda.synchronize()
        got = {k: _np(v) for k, v in outs.items()}
    assert set(n for n in row.entries if not n.endswith(("_ws_bytes", "_ok", "_rows"))) & set(env.called), (row.entries, env.called)
    exp = S.exact(case, d, invstd=got["invstd"] if row.family == "small_fwd" else None)
    checked = 0
    for name, tier in row.tiers.items():
        if name not in got:
            assert name not in exp or name in ("dalpha", "cnt"), (S.cid(case), name)
            continue
        _check(case, name, tier, got[name], exp[name], exp.get(name + "~"))
        checked += 1
    assert checked == len(got) and checked > 0, (S.cid(case), sorted(got), sorted(row.tiers))


# ---- the wide-row branch (C > 256) of colsum_generic_kernel and head_bwd_generic_kernel ----------------------------------------------
# The table's rows rotate C = 1 .. 37 for these two kernels (bn-reduce-m2 has C = 300); their branch for rows wider than a block --
# a row per block and trip, a thread owns the columns tid + j * 256 -- runs here, on integer operands whose sums are exact: `==`.
@pytest.mark.parametrize("C,K,M", [(300, 3, 1531), (257, 2, 5), (1021, 1, 1100)])
def test_generic_kernels_wide_rows(dev, C, K, M):
    rng = np.random.default_rng(C * K + M)
    d = {"x": S._ints(rng, 3, (M, C)), "w": S._ints(rng, 3, (C, K)), "bias": S._ints(rng, 3, K), "dy": S._ints(rng, 3, (M, K))}
    assert np.abs(d["x"]).sum(0).max() * 9 < S.LIMIT                            # (every partial sum exact in float32)
    with _guarded(dev) as h:
        env = Env(dev, h)
        got = run_colsum(env, dict(M=M, C=C), d)
        got.update(run_head(env, dict(M=M, C=C, K=K, op="bwd"), d))
        torch.cuda.synchronize()
        got = {k: _np(v) for k, v in got.items()}
    want = {"out": d["x"].sum(0), "dx": d["dy"] @ d["w"].T, "dw": d["x"].T @ d["dy"], "db": d["dy"].sum(0)}
    for name in sorted(want):
        bad = np.nonzero(~(got[name].reshape(-1) == want[name].reshape(-1)))[0]
        assert bad.size == 0, "C = %d, K = %d, M = %d: output `%s`: %d of %d elements wrong, first at %d" % (
            C, K, M, name, bad.size, want[name].size, int(bad[0]))
