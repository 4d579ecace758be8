"""-m gpu: guard bands (tests/guard.py) around the entry points of include/vnet_hip_head.h, reached the way the network
reaches them (ops.bn_head through autograd, with and without the optional statistics rows) and directly with y stored.  Every tensor of a launch is carved from a guarded arena,
scratch has exactly the queried size; checked: (a) every guard byte intact and no input modified, (b) every output byte written on
the 0xFF pre-fill -- the statistics rows and the data gradient included -- (c) bit-identical results on a 0xFF and a 0x00 pre-fill.
(Results against the oracle: tests/test_hip_head_fusion.py.)  CASES (entry points a case must reach, function) is what the ledger
test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
FUSED = ("vnet_bn_act_head_fwd", "vnet_bn_act_bwd_reduce_head", "vnet_bn_act_bwd_apply_head")


def _op(kind, shp, C, K, act, res, stats=True):
    def run(h):
        from vnet_tensorflow_amd import ops
        prev = ops.set_head_fusion(True, stats)
        try:
            _op_body(h, kind, shp, C, K, act, res, stats)
        finally:
            ops.set_head_fusion(*prev)
    return run


def _op_body(h, kind, shp, C, K, act, res, stats):
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(sum(shp) + C + K + kind)
    nl = 3 if kind == 0 else 2 if kind == 1 else 1
    tx = h.g(rng.standard_normal(shp + (C,)) * 3.0 + 1.5).requires_grad_(True)
    tr = h.g(rng.standard_normal(shp + (C,))).requires_grad_(True) if res else None
    gb = []
    for _ in range(nl):
        gb += [h.g(rng.uniform(0.5, 1.5, C)).requires_grad_(True), h.g(rng.standard_normal(C)).requires_grad_(True)]
    gb += [None] * (6 - len(gb))
    ta = h.g(rng.uniform(0.05, 0.3, C)).requires_grad_(True) if act == "prelu" else None
    tw, tb = h.g(rng.standard_normal((1, 1, 1, C, K))).requires_grad_(True), h.g(rng.standard_normal(K)).requires_grad_(True)
    mov = []
    for k in range(3):
        mov += [h.arena.tensor("mm%d" % k, (C,), torch.float32, "inout", np.zeros(C)),
                h.arena.tensor("mv%d" % k, (C,), torch.float32, "inout", np.ones(C))] if k < nl else [None, None]
    lg = ops.bn_head(tx, tw, tb, kind, act, ta, *gb, residual=tr, moving=tuple(mov))
    assert (getattr(lg, "_vnet_stats", None) is not None) == stats
    # the batch-norm behind the head finalizes the rows the fused pass wrote
    gk, bk = h.g(rng.uniform(0.5, 1.5, K)).requires_grad_(True), h.g(rng.standard_normal(K)).requires_grad_(True)
    out = ops.bn_act(lg, gk, bk)
    assert ("vnet_bn_finalize_partial" if stats else "vnet_bn_stats") == h.calls[-2], h.calls[-3:]
    leaves = [t for t in [tx, tr] + gb + [ta, tw, tb, gk, bk] if t is not None]
    grads = torch.autograd.grad(out, leaves, h.g(rng.standard_normal(tuple(out.shape))))
    assert all(torch.isfinite(t).all() for t in grads) and torch.isfinite(out).all()
    assert not {"vnet_head_fwd", "vnet_head_bwd"} & set(h.calls), h.calls


def _native(M, C, K, res):
    """The three entry points with y stored and scratch of exactly vnet_bn_head_ws_bytes."""
    def run(h):
        from vnet_tensorflow_amd import _lib, ops
        L = _lib.lib()
        rng = np.random.default_rng(M + C + K)
        P = ops._ptr
        out = lambda name, *shape: h.arena.tensor(name, shape, torch.float32, "out")
        tx, tr = h.g(rng.standard_normal((M, C)) * 2 + 1), (h.g(rng.standard_normal((M, C))) if res else None)
        mean, invstd = h.g(rng.standard_normal(C)), h.g(rng.uniform(0.3, 0.6, C))
        tg, tb, ta = h.g(rng.uniform(0.5, 1.5, C)), h.g(rng.standard_normal(C)), h.g(rng.uniform(0.05, 0.3, C))
        tw, tbi, tdl = h.g(rng.standard_normal((C, K))), h.g(rng.standard_normal(K)), h.g(rng.standard_normal((M, K)))
        sdz, sdzx, ex = h.g(rng.standard_normal(C)), h.g(rng.standard_normal(C)), h.g(rng.standard_normal(C) * 1e-3)
        rows = L.vnet_bn_head_stats_rows(M, C)
        y, lg, st = out("y", M, C), out("logits", M, K), out("stats", rows, 2 * K)
        bn = (P(mean), P(invstd), P(tg), P(tb), 2, P(ta))
        s = ops._stream()
        assert L.vnet_bn_act_head_fwd(P(tx), P(tr), M, C, *bn, P(tw), P(tbi), K, P(y), P(lg), P(st), s) == 0
        nb = L.vnet_bn_head_ws_bytes(C, K)
        ws = ops.workspace(nb, tx.device)
        dg, dbt, da, dw, db, ds = out("dg", C), out("dbt", C), out("da", C), out("dw", C, K), out("db", K), out("ds", M, C)
        assert L.vnet_bn_act_bwd_reduce_head(P(tdl), P(tw), K, P(tx), P(tr), M, C, *bn, P(dg), P(dbt), P(da), P(dw), P(db), P(ws), nb, s) == 0
        assert L.vnet_bn_act_bwd_apply_head(P(tdl), P(tw), K, P(tx), P(tr), M, C, *bn, P(sdz), P(sdzx), float(M), P(ex), P(ds), s) == 0
    return run


CASES = {
    "chain kind 0, 16 -> 2, 2x5x6x7": (FUSED, _op(0, (2, 5, 6, 7), 16, 2, "prelu", False)),
    "chain kind 1, 8 -> 5, 1x7x9x11": (FUSED, _op(1, (1, 7, 9, 11), 8, 5, "relu", False)),
    "chain kind 0, 16 -> 2, 2x5x6x7, no statistics rows (the network's setting)": (FUSED, _op(0, (2, 5, 6, 7), 16, 2, "prelu", False, False)),
    "bn_act + residual, 16 -> 2, 1x9x9x9, no statistics rows": (FUSED, _op(-1, (1, 9, 9, 9), 16, 2, "relu", True, False)),
    "bn_act + residual, 16 -> 5, 1x3x5x33": (FUSED, _op(-1, (1, 3, 5, 33), 16, 5, "prelu", True)),
    "bn_act + residual, 8 -> 2, 32^3 (every workgroup busy)": (FUSED, _op(-1, (1, 32, 32, 32), 8, 2, "lrelu", True)),
    "chain kind 0, 16 -> 2, 48^3 (grid-stride tail)": (FUSED, _op(0, (1, 48, 48, 48), 16, 2, "prelu", False)),
    "entry points, y stored, 16 -> 8, 1001 rows": (FUSED, _native(1001, 16, 8, True)),
    "entry points, y stored, 8 -> 3, 7 rows": (FUSED, _native(7, 8, 3, False)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_head_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, need_output=False)
