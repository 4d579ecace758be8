"""Host-side checks of the exact elementwise sweep (tests/ew_sweep.py): the coverage conditions of the generated case set and the
rows' `absent` declarations, in both directions; bound(case) < 2^24 for every case; the restated launcher expressions against the
shape-only queries the library exports; THE PROOF that the design is exact on its own -- for every E and R output of every case below
the cap a NumPy float32 evaluation of the kernel's formula equals the float64 oracle in three summation orders, with every
multiply-add rounded twice and rounded once; the dropout hash pinned by hand-computed values; the ledger of the entry points
elementwise.hip implements; and the GPU test's launches against the ctypes binding (argument count and kind) on a stand-in library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ew_sweep as S
from tests import guard

CASES = S.generate()
BY_ROW = {name: [c for c in CASES if c.row == name] for name in S.ROWS}
ROOT = S.ROOT


def test_ids_are_unique_and_every_row_has_its_cases():
    ids = [S.cid(c) for c in CASES]
    assert len(ids) == len(set(ids))
    assert S.generate() == CASES                                               # deterministic
    for name, row in S.ROWS.items():
        cs = BY_ROW[name]
        assert [c for c in cs if not c.capped], name
        capped = [c for c in cs if c.capped]
        assert len(capped) == (0 if row.nocap else 1), (name, row.nocap)
        for c in capped:
            assert S.wraps(c) >= 2
        for c in cs:
            assert row.accept(S.case_params(c)), S.cid(c)
    assert len(S.table(CASES).splitlines()) == len(S.ROWS) + 1


@pytest.mark.parametrize("name", list(S.ROWS))
def test_coverage_conditions(name):
    row, cs = S.ROWS[name], [c for c in BY_ROW[name] if not c.capped]
    have = set()
    for c in cs:
        g = S.geom_of(c)
        assert not g.capped, S.cid(c)
        have |= set(S.classes(g).items())
    need = row.needed()
    assert need <= have, "%s: classes %s never occur" % (name, sorted(need - have))
    # every class of every axis is either needed or declared absent with a reason, and a declared-absent class really is not
    # realisable below the cap
    real = S.realisable(row)
    for axis, absent in row.absent.items():
        assert row.absent_why[axis], (name, axis)
        for cls in absent:
            assert cls in S.CLASSES and (axis, cls) not in real, "%s: %s / %s is declared absent but an extent realises it" % (name, axis, cls)
    axes = set(a for a, _ in need) - {"slot"}
    for axis in axes:
        assert set(c for a, c in need if a == axis) | set(row.absent.get(axis, ())) == set(S.CLASSES), (name, axis)
    if row.clamped:
        assert ("slot", "out") in have and S.geom_of(cs[0]).U > 1, name
    # every value of every rotated parameter (the channel classes of the mode, K = 1..8, B = 1..3, the activations, bcast, the patch
    # faces ...) occurs at a NON-DEGENERATE extent: more than one block's slot and at least five rows -- one row, one voxel or one
    # element proves nothing about a tail, a reduction or an index
    for k, vals in row.rot.items():
        seen = set(S.case_params(c)[k] for c in cs if row.sizes or S.nondegenerate(S.geom_of(c), c.size))
        assert set(vals) <= seen, "%s: %s = %s never occurs at a non-degenerate extent" % (name, k, sorted(set(vals) - seen))
    if not row.sizes:
        assert sum(1 for c in cs if S.nondegenerate(S.geom_of(c), c.size)) >= max(len(v) for v in row.rot.values()), name
        assert any(S.geom_of(c).items % S.geom_of(c).per_block for c in cs if S.nondegenerate(S.geom_of(c), c.size)) or \
            S.geom_of(cs[0]).per_block == 1, name                              # a ragged block tail past the first block


def test_patch_windows_overhang_partially():
    """Every case of a face hangs over it with part of the window inside the volume and part outside, `zyx` over all three at once."""
    for name in ("patch-count", "patch-nocount"):
        faces = set()
        for c in BY_ROW[name]:
            p = S.case_params(c)
            inside = {"z": (p["D"] - p["z0"], p["M"]), "y": (p["H"] - p["y0"], p["py"]), "x": (p["W"] - p["x0"], p["px"])}
            for ax, (room, ext) in inside.items():
                if ax in p["face"]:
                    assert 0 < room < ext, (S.cid(c), ax, room, ext)
                else:
                    assert room >= ext, (S.cid(c), ax)
            faces.add(p["face"])
        assert faces == {"z", "y", "x", "zyx", "none"}


def test_channel_classes_of_the_reduction_modes():
    def widths(name):
        return set(S.case_params(c)["C"] for c in BY_ROW[name])
    assert {4, 8, 64, 256} <= widths("bn-reduce-m0") and {4, 8, 64, 256} <= widths("bn-moments-vec")        # CQ = 1, 2, 16, 64
    assert {1, 3} <= widths("bn-reduce-m1") and {1, 3} <= widths("bn-moments-row")
    assert S._red_mode(8) == 0                                                # (two quads: the vector kernels take C = 8, not the row kernels)
    assert {12, 37, 255, 300} <= widths("bn-reduce-m2") and {12, 37, 255} <= widths("bn-moments-generic")
    assert {257, 300} <= widths("bn-moments-wide")
    for name, mode in (("bn-reduce-m0", 0), ("bn-reduce-m1", 1), ("bn-reduce-m2", 2)):
        assert all(S._red_mode(S.case_params(c)["C"]) == mode for c in BY_ROW[name]), name
    for name in ("bn-head-fwd", "bn-head-reduce", "bn-head-apply"):
        assert widths(name) == {8, 16} and set(S.case_params(c)["K"] for c in BY_ROW[name]) == set(range(1, 9))
    assert set((S.case_params(c)["K"], ) for c in BY_ROW["loss-fwd"]) == set((k,) for k in range(1, 9))
    assert set(S.case_params(c)["B"] for c in BY_ROW["loss-fwd"]) == {1, 2, 3}


@pytest.mark.parametrize("name", list(S.ROWS))
def test_every_case_passes_the_exactness_bound(name):
    for c in BY_ROW[name]:
        d = S.operands(c)
        b = S.bound(c, d)
        assert b < S.LIMIT, (S.cid(c), b)


def _proved(row, key):
    t = row.tiers.get(key, "")
    return key.startswith("_") or t.startswith("E") or t.startswith("R")


@pytest.mark.parametrize("name", list(S.ROWS))
def test_float32_evaluation_equals_the_oracle(name):
    """The proof.  Every E output (and the internal sums a B output is computed from, `_I` ...) in float32: three summation orders x
    {every multiply-add rounded twice, rounded once}; every R output likewise (its restatement has no multiply-add to contract).
    The one case per row past the grid cap is proved in one of the six ways; beyond that it rests on bound(case) < 2^24."""
    row = S.ROWS[name]
    n = 0
    for c in BY_ROW[name]:
        d = S.operands(c)
        kw = {}
        if row.family == "small_fwd":                                        # (the device's invstd stands in: any float32 near the reference)
            kw["invstd"] = np.asarray(S.formula(c, d, S.Arith())["invstd"], np.float32).astype(np.float64)
        want = S.exact(c, d, **kw)
        # (the case past the cap -- its own operand level, sums of 2^18 rows and more -- in one order: pairwise, contracted)
        for order, fused in ([("pair", True)] if c.capped else S.PROOFS):
            got = S.formula(c, d, S.Arith(f32=True, fused=fused, order=order), **kw)
            for k, v in got.items():
                if k.endswith("~") or not _proved(row, k):
                    continue
                v, w = S.stored(c, got)[k], want[k]
                assert v.shape == w.shape and np.array_equal(v, w), "%s: `%s` differs in float32 (order %s, contraction %s): %d elements" % (
                    S.cid(c), k, order, fused, int((v != w).sum()))
                n += 1
    assert n > 0, name


def test_softmax_of_the_voxel_kinds_is_exact_in_float32():
    """expf(0) = 1, expf(-128) = 0 with or without denormals (e^-128 = 2.6e-56, below the smallest denormal 1.4e-45), 1.f / m exact."""
    assert np.exp(np.float32(0)) == 1 and np.exp(np.float32(-128)) == 0 and float(np.exp(-128.0)) < 2.0 ** -149 / 2
    c = max((c for c in BY_ROW["loss-fwd"] if S.case_params(c)["K"] == 8 and not c.capped), key=lambda c: c.size)
    d = S.operands(c)
    z = d["z"].astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    se = np.cumsum(e, axis=-1, dtype=np.float32)[..., -1:]
    p, pred = S._softmax(d)
    assert np.array_equal((e * (np.float32(1) / se)).astype(np.float64), p)
    assert (d["lab"] < 0).any() and (d["lab"] >= 8).any()
    ties = set()
    for cc in BY_ROW["loss-fwd"]:
        ties |= set(int(m) for m in np.unique(S.operands(cc)["m"])) if not cc.capped else set()
    assert ties == {1, 2, 4, 8}
    first = np.asarray([[int(np.nonzero(row == row.max())[0][0]) for row in b] for b in d["z"]])
    assert np.array_equal(pred, first) and (p.max(-1) < 1).any()              # a tie goes to the first index
    assert not (d["lab"] == 7).any()                                          # a class absent from the patch


def test_dropout_hash_is_pinned():
    """mix32(seed * 0x9E3779B97F4A7C15 + i) >> 8 worked by hand (python integers, modulo 2^64) for three (seed, i)."""
    def by_hand(seed, i):
        x = (seed * 0x9E3779B97F4A7C15 + i) % (1 << 64)
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd % (1 << 64)
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 % (1 << 64)
        x ^= x >> 33
        return (x & 0xffffffff) >> 8
    pinned = {(1, 0): 10791726, (4711, 5): 6393964, (0x5EED, 1000003): 8778385}
    for (seed, i), v in pinned.items():
        assert by_hand(seed, i) == v, (seed, i, by_hand(seed, i))
        for rate in (0.5, 0.75):
            keep = S.dropout_mask(seed, i + 1, rate)
            assert bool(keep[i]) == (np.float32(v) * np.float32(2.0 ** -24) >= np.float32(rate)), (seed, i, rate)
    # with a step state the seed moves by step * 0xD1342543DE82EF95
    assert np.array_equal(S.dropout_mask(7, 100, 0.5, step=3), S.dropout_mask((7 + 3 * S.STEP_MUL) % (1 << 64), 100, 0.5))
    m = S.dropout_mask(4711, 1 << 16, 0.75)
    assert abs(m.mean() - 0.25) < 0.01


def test_queries():
    """The launcher expressions ew_sweep.py restates against the shape-only queries of the library."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    MB = S.MAXBLK
    for C in (1, 3, 8, 12, 64, 300, 1024):
        assert L.vnet_bn_ws_bytes(C) == MB * 3 * max(C, 8) * 4
        assert L.vnet_colsum_ws_bytes(C) == MB * max(C, 8) * 4
        assert L.vnet_colsum_b16_ws_bytes(C) == S.CS16_MAXBLK * C * 4
    for C in (4, 5, 16, 64):
        for K in range(1, 9):
            assert L.vnet_head_ws_bytes(C, K) == MB * (C * K + K) * 4
            assert L.vnet_bn_head_ok(C, K) == int(C in (8, 16))
            assert L.vnet_bn_head_ws_bytes(C, K) == MB * (3 * C + C * K + K) * 4
    assert L.vnet_bn_head_ok(8, 9) == 0 and L.vnet_bn_head_ok(16, 0) == 0
    for B in (1, 2, 3):
        for K in range(1, 9):
            assert L.vnet_loss_ws_bytes(B, K) == B * MB * (3 * K + 1) * 4 + B * (3 * K + 1) * 8 + 16
    for c in BY_ROW["bn-head-fwd"]:
        p = S.case_params(c)
        rows, blk = S._head_rows(p["M"], p["C"])
        assert L.vnet_bn_head_stats_rows(p["M"], p["C"]) == rows == S.geom_of(c).grid and blk.max() < rows
    assert L.vnet_bn_head_stats_rows(100, 12) == 0
    for M, C, ok in ((1, 8, 1), (8192, 24, 1), (8193, 8, 0), (100, 12, 0), (100, 1032, 0), (0, 8, 0)):
        assert L.vnet_bn_small_ok(M, C) == ok
    for name in ("bn16-small-fwd-r0", "bn16-small-bwd-r1"):
        assert all(L.vnet_bn_small_ok(S.case_params(c)["M"], S.case_params(c)["C"]) == 1 for c in BY_ROW[name])


# ---- the ledger -------------------------------------------------------------------------------------------------------------------
def _implemented():
    src = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "elementwise.hip")).read()
    return set(re.findall(r"^(?:int|size_t) (vnet_[a-z0-9_]+)\(", src, re.M))


def test_entry_point_ledger():
    """Every entry point include/vnet_hip.h and include/vnet_hip_head.h declare and elementwise.hip implements is named by a row of
    the table or excluded with a reason; a new one fails here until it has a row."""
    declared = set(guard.header_functions()) | set(guard.header_functions(os.path.join(ROOT, "include", "vnet_hip_head.h")))
    ours = declared & _implemented()
    assert len(ours) >= 50, sorted(ours)
    named = set()
    for row in S.ROWS.values():
        named |= set(row.entries)
    assert named <= ours, sorted(named - ours)
    assert not named & set(S.EXCLUDED), sorted(named & set(S.EXCLUDED))
    assert set(S.EXCLUDED) <= ours and all(S.EXCLUDED.values())
    assert ours == named | set(S.EXCLUDED), "entry points of elementwise.hip without a row: %s" % sorted(ours - named - set(S.EXCLUDED))
    assert _implemented() <= declared, sorted(_implemented() - declared)


# ---- the GPU test's launches against the binding -------------------------------------------------------------------------------------
class _StandIn(object):
    """_lib.lib() without a device: a launch converts its arguments as ctypes would and returns 0; a query is answered by the library."""

    def __init__(self, real, sigs):
        self.real, self.sigs, self.calls = real, sigs, []

    def __getattr__(self, name):
        res, argtypes = self.sigs[name]
        if name.endswith(("_ws_bytes", "_ok", "_rows")):
            return getattr(self.real, name)

        def fn(*args):
            assert len(args) == len(argtypes), "%s: %d arguments, the binding has %d" % (name, len(args), len(argtypes))
            for j, (a, t) in enumerate(zip(args, argtypes)):
                if t is ctypes.c_void_p:
                    assert a is None or isinstance(a, int), "%s: argument %d is %r, not a pointer" % (name, j, type(a))
                else:
                    assert a is not None and not isinstance(a, torch.Tensor), "%s: argument %d" % (name, j)
                    t(a)                                                      # TypeError where ctypes would refuse the value
                    if t in (ctypes.c_int, ctypes.c_int64):
                        assert isinstance(a, (int, np.integer)), "%s: argument %d is %r, an integer is declared" % (name, j, a)
            self.calls.append(name)
            return 0
        return fn


def test_launches_match_the_binding(monkeypatch):
    """Every case below the cap through the GPU test's own launch code on CPU tensors: each call has the binding's argument count,
    pointers where it declares pointers and numbers where it declares numbers; across a row's cases every entry point it names is
    called; the outputs have the oracle's names and sizes."""
    from vnet_tensorflow_amd import _lib
    from tests import test_hip_ew_sweep as T
    stand = _StandIn(_lib.lib(), _lib.all_signatures())
    monkeypatch.setattr(_lib, "lib", lambda: stand)
    for name, row in S.ROWS.items():
        called = set()
        for c in BY_ROW[name]:
            if c.capped:
                continue
            p = S._with_row(c)
            p["_family"] = row.family
            d = S.operands(c)
            env = T.Env(torch.device("cpu"))
            outs = T.RUN[row.family](env, p, d)
            called |= set(env.called)
            exp = S.exact(c, d)
            for k, t in outs.items():
                assert k in row.tiers and k in exp and t.numel() == exp[k].size, (S.cid(c), k)
        assert set(row.entries) <= called, (name, sorted(set(row.entries) - called))
