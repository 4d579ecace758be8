"""No GPU: the library calls the batch-norm ops make -- entry point, order and every argument -- against the recorded traces of
tests/golden/bn_call_trace.json (written by tests/golden/make_bn_call_trace.py from this file's cases).

The public wrappers (ops.bn_act, bn_chain, bn_head, bn_concat, bn_update_only) run forward and backward on CPU tensors with a
stand-in for _lib.lib(): size queries and the `_ok` predicates go to the real library, every launch is recorded and returns 0.
A recorded call is [entry point, arguments]: scalars by value, a pointer as the NAME of the test tensor it falls inside plus the byte
offset ("gamma+64": the second half of bn_concat's gamma), else "ws" (the workspace), "new" (a tensor the op allocated) or None.
Beside the launches a trace holds "all_reduce" (the cross-replica reduction: argument, element count), "deferred" (the thunk the fused
input convolution leaves on gamma) and "slot_target" (what the second consumer of a forked residual finds in the fork slot: "first"
when the batch-norm left its ds there for it to accumulate into), then the outputs and which inputs received a gradient.

One entry may differ from the recorded one: bn_head with kind -1 and a forked residual.  The traces were recorded when the fused head
did not leave ds in the fork slot (slot_target None); leaving it there, as bn_act does, is accepted."""
import contextlib
import ctypes
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_call_trace.json")
STREAM = "stream"
F32, B16 = torch.float32, torch.bfloat16


class Env(object):
    """The named tensors of one case and the calls recorded while it runs."""

    def __init__(self):
        self.named, self.calls = {}, []

    def t(self, name, *shape, **kw):
        t = torch.zeros(shape, dtype=kw.get("dtype", F32)).requires_grad_(kw.get("grad", False))
        self.named[name] = t
        return t

    def pointer(self, p, ops):
        if p is None or p == STREAM:
            return p
        for name, t in self.named.items():
            base = t.untyped_storage().data_ptr()
            if base <= p < base + max(t.untyped_storage().nbytes(), 1):
                return name if p == base else "%s+%d" % (name, p - base)
        for ws in ops._WS.values():
            if ws.data_ptr() <= p < ws.data_ptr() + ws.numel():
                return "ws"
        return "new"


@contextlib.contextmanager
def recording(env, sync=False):
    """ops with the recording stand-in for the library, no device check, a fresh workspace table and (sync) cross-replica statistics
    over a world of 2."""
    from vnet_tensorflow_amd import _lib, ops
    real_lib = _lib.lib
    real = real_lib()
    sigs = _lib.all_signatures()

    class Rec(object):
        def __getattr__(self, name):
            if name.endswith(("_bytes", "_rows", "_ok")):
                return getattr(real, name)
            types = sigs[name][1]

            def launch(*args):
                assert len(args) == len(types), name
                env.calls.append((name, [env.pointer(a, ops) if t is ctypes.c_void_p else a for a, t in zip(args, types)]))
                return 0
            return launch
    rec = Rec()

    def all_reduce(t):
        env.calls.append(("all_reduce", [env.pointer(t.data_ptr(), ops), t.numel()]))
    saved = (ops._raw_stream, ops._need_gpu, ops._SYNC_BN, ops._WS)
    _lib.lib = lambda: rec
    ops._raw_stream, ops._need_gpu, ops._WS = (lambda: STREAM), (lambda *a, **k: None), {}
    ops._SYNC_BN = (all_reduce, 2) if sync else None
    try:
        yield ops
    finally:
        _lib.lib = real_lib
        ops._raw_stream, ops._need_gpu, ops._SYNC_BN, ops._WS = saved


def _describe(t):
    return None if t is None else [str(t.dtype).replace("torch.", "")] + list(t.shape)


def _finish(env, outs, seeds, extra=None):
    """Backward from `outs` seeded with `seeds`; the trace of the case."""
    torch.autograd.backward(outs, seeds)
    grads = dict((n, _describe(t.grad)) for n, t in env.named.items() if t.requires_grad)
    trace = {"calls": env.calls, "out": [_describe(o) for o in outs], "grads": grads}
    trace.update(extra or {})
    return json.loads(json.dumps(trace))


class _SecondConsumer(torch.autograd.Function):
    """The other consumer of a forked tensor (conv_1 of a residual block), created BEFORE the batch-norm so that its backward runs
    after it: records whether ops._slot_target hands it the batch-norm's ds to accumulate into."""

    @staticmethod
    def forward(ctx, a, slot, env, ops):
        ctx.args = (slot, env, ops)
        return a.view_as(a)

    @staticmethod
    def backward(ctx, dy):
        slot, env, ops = ctx.args
        env.calls.append(("slot_target", ["first" if ops._slot_target(slot, dy, dy.shape) is not None else None]))
        return dy, None, None, None


def _forked_residual(env, ops, M, C, dtype=F32):
    """(residual handle, [output of the second consumer], [its gradient seed]) of a block input with two consumers."""
    a, r = ops.fork(env.t("inp", M, C, dtype=dtype, grad=True))
    return r, [_SecondConsumer.apply(a, a._vnet_slot, env, ops)], [env.t("dconv", M, C, dtype=dtype)]


def _sink(env, ops, p, name):
    p._vnet_sink = ops.GradSink(env.t("sink_" + name, *p.shape))


def bn_act_case(M=300, C=16, dtype=F32, act=None, residual=False, tile=False, xgrad=True, sinks=False, epilogue=None, sync=False,
                want_stats=False):
    env = Env()
    with recording(env, sync) as ops:
        x = env.t("x", M, 1 if tile else C, dtype=dtype, grad=xgrad)
        gamma, beta = env.t("gamma", C, grad=True), env.t("beta", C, grad=True)
        alpha = env.t("alpha", C, grad=True) if act == "prelu" else None
        r, outs, seeds = _forked_residual(env, ops, M, C, dtype) if residual else (None, [], [])
        if sinks:
            for p, n in ((gamma, "gamma"), (beta, "beta"), (alpha, "alpha")):
                if p is not None:
                    _sink(env, ops, p, n)
            gamma._vnet_deferred = lambda accumulate: env.calls.append(("deferred", [accumulate]))
        if epilogue is not None:          # "own": the producer's sums of exactly x (+ r); "other": sums of x alone beside a residual
            x._vnet_stats = ops._EpilogueStats(env.t("partial", 4, 2 * C), 4, r if epilogue == "own" else None)
        res = ops.bn_act(x, gamma, beta, act, alpha, r, tile, env.t("mm", C), env.t("mv", C), want_stats)
        extra = {}
        if want_stats:
            y, mean, invstd = res
            extra["stats"] = [_describe(mean), mean.requires_grad, _describe(invstd), invstd.requires_grad]
        else:
            y = res
        return _finish(env, [y] + outs, [env.t("dy", M, C, dtype=dtype)] + seeds, extra)


def bn_chain_case(kind, M=300, C=16, dtype=F32, act="prelu", sync=False, sinks=False):
    env = Env()
    with recording(env, sync) as ops:
        x = env.t("x", M, C, dtype=dtype, grad=True)
        nl = 3 if kind == 0 else 2
        g = []
        for k in range(3):
            g += [env.t("g%d" % (k + 1), C, grad=True), env.t("b%d" % (k + 1), C, grad=True)] if k < nl else [None, None]
        moving = [env.t("m%s%d" % (s, k + 1), C) if k < nl else None for k in range(3) for s in "mv"]
        alpha = env.t("alpha", C, grad=True) if act == "prelu" else None
        if sinks:
            for k, p in enumerate(g):
                if p is not None:
                    _sink(env, ops, p, "gb"[k % 2] + str(k // 2 + 1))
        y = ops.bn_chain(x, kind, act, alpha, *g, moving=tuple(moving))
        return _finish(env, [y], [env.t("dy", M, C, dtype=dtype)])


def bn_head_case(kind, C, K, M=300, act="prelu", fusion=(True, False), sync=False, sinks=False):
    env = Env()
    with recording(env, sync) as ops:
        x = env.t("x", M, C, grad=True)
        nl = 3 if kind == 0 else 2 if kind == 1 else 1
        g = []
        for k in range(3):
            g += [env.t("g%d" % (k + 1), C, grad=True), env.t("b%d" % (k + 1), C, grad=True)] if k < nl else [None, None]
        moving = [env.t("m%s%d" % (s, k + 1), C) if k < nl else None for k in range(3) for s in "mv"]
        alpha = env.t("alpha", C, grad=True) if act == "prelu" else None
        w, b = env.t("w", 1, 1, 1, C, K, grad=True), env.t("b", K, grad=True)
        if sinks:
            for p, n in ((w, "w"), (b, "b"), (g[0], "g1"), (g[1], "b1")):
                _sink(env, ops, p, n)
        r, outs, seeds = _forked_residual(env, ops, M, C) if kind < 0 else (None, [], [])
        prev = ops.set_head_fusion(*fusion)
        try:
            lg = ops.bn_head(x, w, b, kind, act, alpha, *g, residual=r, moving=tuple(moving))
        finally:
            ops.set_head_fusion(*prev)
        st = getattr(lg, "_vnet_stats", None)
        extra = {"logits_stats": None if st is None else [_describe(st.partial), st.rows, st.residual is None]}
        return _finish(env, [lg] + outs, [env.t("dl", M, K)] + seeds, extra)


def bn_concat_case(C0=16, C1=8, M=300, sync=False, sinks=False, forked=False):
    env = Env()
    with recording(env, sync) as ops:
        x0 = env.t("x0", M, C0, grad=True)
        gamma, beta = env.t("gamma", C0 + C1, grad=True), env.t("beta", C0 + C1, grad=True)
        if sinks:
            _sink(env, ops, gamma, "gamma")
            _sink(env, ops, beta, "beta")
        if forked:
            x1, outs, seeds = _forked_residual(env, ops, M, C1)
        else:
            x1, outs, seeds = env.t("x1", M, C1, grad=True), [], []
        y0, y1 = ops.bn_concat(x0, x1, gamma, beta, env.t("mm", C0 + C1), env.t("mv", C0 + C1))
        return _finish(env, [y0, y1] + outs, [env.t("dy0", M, C0), env.t("dy1", M, C1)] + seeds)


def bn_update_only_case(epilogue, M=300, C=16, dtype=F32, sync=False):
    env = Env()
    with recording(env, sync) as ops:
        x = env.t("x", M, C, dtype=dtype)
        if epilogue:
            x._vnet_stats = ops._EpilogueStats(env.t("partial", 4, 2 * C), 4, None)
        assert ops.bn_update_only(x, C, env.t("mm", C), env.t("mv", C)) is None
        return json.loads(json.dumps({"calls": env.calls}))


CASES = {
    "bn_act plain": lambda: bn_act_case(),
    "bn_act relu": lambda: bn_act_case(act="relu"),
    "bn_act forked residual prelu": lambda: bn_act_case(act="prelu", residual=True),
    "bn_act tile": lambda: bn_act_case(tile=True, act="prelu"),
    "bn_act x without grad": lambda: bn_act_case(act="prelu", xgrad=False),
    "bn_act x without grad forked residual": lambda: bn_act_case(residual=True, xgrad=False),
    "bn_act sinks": lambda: bn_act_case(act="prelu", sinks=True),
    "bn_act tile sinks deferred": lambda: bn_act_case(tile=True, sinks=True, xgrad=False, want_stats=True),
    "bn_act want_stats": lambda: bn_act_case(act="relu", want_stats=True),
    "bn_act epilogue": lambda: bn_act_case(act="prelu", epilogue="own"),
    "bn_act epilogue forked residual": lambda: bn_act_case(act="prelu", residual=True, epilogue="own"),
    "bn_act epilogue of another sum": lambda: bn_act_case(act="prelu", residual=True, epilogue="other"),
    "bn_act sync": lambda: bn_act_case(act="prelu", sync=True),
    "bn_act sync forked residual epilogue": lambda: bn_act_case(act="prelu", residual=True, epilogue="own", sync=True),
    "bn_act sync x without grad": lambda: bn_act_case(xgrad=False, sync=True),
    "bn_act bf16 small": lambda: bn_act_case(M=512, dtype=B16, act="prelu"),
    "bn_act bf16 small forked residual": lambda: bn_act_case(M=512, dtype=B16, act="prelu", residual=True),
    "bn_act bf16 stream": lambda: bn_act_case(M=4096, dtype=B16, act="prelu"),
    "bn_act bf16 stream forked residual epilogue": lambda: bn_act_case(M=4096, dtype=B16, act="relu", residual=True, epilogue="own"),
    "bn_act bf16 sync": lambda: bn_act_case(M=512, dtype=B16, act="prelu", sync=True),
    "bn_update_only": lambda: bn_update_only_case(False),
    "bn_update_only epilogue": lambda: bn_update_only_case(True),
    "bn_update_only bf16": lambda: bn_update_only_case(False, dtype=B16),
    "bn_update_only sync": lambda: bn_update_only_case(True, sync=True),
    "bn_concat": lambda: bn_concat_case(),
    "bn_concat sinks forked skip": lambda: bn_concat_case(sinks=True, forked=True),
    "bn_concat sync": lambda: bn_concat_case(sync=True),
    "bn_head stats rows": lambda: bn_head_case(0, 16, 2, fusion=(True, True)),
    "bn_head stats rows sync": lambda: bn_head_case(1, 16, 2, fusion=(True, True), sync=True),
    "bn_head fusion off kind 0": lambda: bn_head_case(0, 16, 2, fusion=(False, False)),
    "bn_head fusion off kind -1": lambda: bn_head_case(-1, 16, 2, fusion=(False, False)),
    "bn_head C32 kind 1": lambda: bn_head_case(1, 32, 2),
    "bn_head C32 kind -1": lambda: bn_head_case(-1, 32, 2),
    "bn_head kind 0 sinks relu": lambda: bn_head_case(0, 16, 2, act="relu", sinks=True),
    "bn_head kind 1 sync": lambda: bn_head_case(1, 8, 5, sync=True),
    "bn_head kind -1 sync": lambda: bn_head_case(-1, 16, 2, sync=True),
}
for _kind in (0, 1):
    for _dtype, _tag in ((F32, "fp32"), (B16, "bf16")):
        CASES["bn_chain kind %d %s" % (_kind, _tag)] = lambda k=_kind, d=_dtype: bn_chain_case(k, dtype=d)
    CASES["bn_chain kind %d sync" % _kind] = lambda k=_kind: bn_chain_case(k, sync=True)
    CASES["bn_chain kind %d sinks relu" % _kind] = lambda k=_kind: bn_chain_case(k, act="relu", sinks=True)
for _kind in (-1, 0, 1):
    for _C in (8, 16):
        for _K in (2, 5):
            CASES["bn_head kind %d C%d K%d" % (_kind, _C, _K)] = lambda k=_kind, c=_C, kk=_K: bn_head_case(k, c, kk)


@pytest.fixture(scope="module")
def golden():
    from vnet_tensorflow_amd import _lib
    try:
        _lib.lib()
    except (OSError, _lib.VnetHipError) as e:
        pytest.skip("libvnet_hip.so cannot be loaded here: %s" % e)
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bn_call_trace(golden, case):
    got, want = CASES[case](), golden[case]
    fused_head_residual = case.startswith("bn_head kind -1")
    assert len(got["calls"]) == len(want["calls"]), [c[0] for c in got["calls"]]
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        if fused_head_residual and w == ["slot_target", [None]] and g == ["slot_target", ["first"]]:
            continue                      # the fused head leaves its ds in the fork slot like bn_act (module docstring)
        assert g == w, "call %d of %r" % (k, case)
    for key in want:
        if key != "calls":
            assert got.get(key) == want[key], (case, key)
    assert sorted(got) == sorted(want)
