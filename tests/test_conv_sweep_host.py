"""Host-side checks of the exact-integer convolution sweep (tests/conv_sweep.py): the coverage conditions of the generated case
set, stated as code; the identity of the float64 torch oracle and oracle/vnet_oracle.py on integer operands, which the GPU
comparison rests on; the 2^20 exactness guard of every case; the restated C planners against the library's shape-only queries; and
ops.route()'s family for every launch of every case, so that a routing change fails here and does not silently empty the sweep."""
import collections

import numpy as np
import pytest

from oracle import vnet_oracle as O
from tests import conv_sweep as S
from tests import util as TU

CASES = S.generate()
BY_VARIANT = collections.OrderedDict((name, [c for c in CASES if c.variant == name]) for name in S.VARIANTS)


@pytest.fixture
def forced(lib_option, monkeypatch):
    """forced(case): the case's library options and ops switches for the duration of the test (shared with the GPU test)."""
    import contextlib
    stack = contextlib.ExitStack()

    def go(case):
        S.force(case, lib_option, monkeypatch, stack)
    yield go
    stack.close()


def test_no_duplicates_and_every_variant_has_cases():
    ids = [c.cid for c in CASES]
    assert len(ids) == len(set(ids))
    shapes = [(c.variant, c.B, c.D, c.H, c.W, c.C0, c.C1, c.O) for c in CASES]
    assert len(shapes) == len(set(shapes))
    for name, cs in BY_VARIANT.items():
        assert cs, name
        for c in cs:
            assert c.v.accept(c), "%s: the variant's planner does not take this shape" % c.cid


@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_coverage_conditions(name):
    v, cs = S.VARIANTS[name], BY_VARIANT[name]
    cls = [S.case_classes(c) for c in cs]
    # every (variant, axis, class) triple the variant's shape rule admits
    for axis in range(3):
        want = set(S.classes_of(v, axis))
        assert want, (name, axis)
        have = set(k[axis] for k in cls)
        assert want <= have, "%s axis %d: classes %s never occur" % (name, axis, sorted(want - have))
    # all three axes ragged at once (where every axis has a ragged class)
    if all(set(S.RAGGED) & set(S.classes_of(v, a)) for a in range(3)):
        assert any(all(k in S.RAGGED for k in kk) for kk in cls), name
    assert any(c.B == 3 for c in cs) and any(c.B == 2 for c in cs), name
    if v.two_src:
        assert any(c.C1 > 0 for c in cs), name
    if v.persistent:
        items = [v.items(c) for c in cs]
        more = [n for n in items if n > v.persistent and n % v.persistent]
        assert more, "%s: no case with more items than the %d workgroups and a remainder: %s" % (name, v.persistent, items)
        if v.mode == "x3":
            assert any(n % 8 for n in more), (name, more)           # items are partitioned by blockIdx % 8
        if name not in MIN_ITEMS:
            assert any(n < v.persistent for n in items), "%s: no case with fewer items than workgroups: %s" % (name, items)
        else:
            assert MIN_ITEMS[name] <= min(items) <= MIN_ITEMS[name] + 8, (name, items)
    if v.split(cs[0]) is not None:
        splits = [v.split(c) for c in cs]
        assert any(s > 1 for s in splits) and any(s == 1 for s in splits), (name, splits)


# persistent forms whose own planner demands at least one item per workgroup: "fewer items than workgroups" cannot exist; the
# boundary (exactly that many items) is in the set instead
MIN_ITEMS = {"b16-c16": 256, "b16-r32": 256, "b16-padded": 256, "x3-conv-nb2": 256, "x3-conv-nb1": 512}


def test_special_widths_and_shapes():
    w = lambda name: set(c.W for c in BY_VARIANT[name])
    for name in ("x3-conv", "x3-wgrad"):
        assert {7, 9} <= w(name), name                               # the narrow brick is chosen on equality: its neighbours take the normal one
    assert w("x3-conv-narrow") == {8} and w("x3-wgrad-narrow") == {8}
    for name, cs in BY_VARIANT.items():
        if S.VARIANTS[name].op == "pair":
            assert any(min(c.dims) >= 3 and c.D % 2 and c.H % 2 and c.W % 2 for c in cs), name      # an odd extent of 1 proves nothing
    inp = [c for c in CASES if c.v.op == "input"]
    assert {16, 8} <= set(c.O for c in inp)
    assert any(1 in c.dims for c in inp if c.variant.startswith("input-direct")) and any(1 in c.dims for c in inp if c.variant == "input-im2col")
    assert set(c.C0 for c in BY_VARIANT["b16-padded"]) == {1, 3, 4}


def _twin_queries(c, lib_option):
    from vnet_tensorflow_amd import ops
    out = []
    for name in (c.variant, c.v.twin):
        t = S.VARIANTS[name]
        for k, val in t.opts:
            lib_option(k, val)
        r = ops.route(*S.launches(c._replace(variant=name))[0][2])
        out.append((r.stats_rows, r.ws))
    return out


@pytest.mark.parametrize("name", [n for n, v in S.VARIANTS.items() if v.twin])
def test_option_twins_are_told_apart_where_a_query_can(name, lib_option):
    """A variant Python cannot observe runs under both option values (its twin row has the other one).  That the option took effect is
    shown by the shape-only queries where they differ -- statistics rows or workspace bytes; where none does the row says so."""
    v = S.VARIANTS[name]
    assert v.observe
    differ = any(a != b for a, b in (_twin_queries(c, lib_option) for c in BY_VARIANT[name]))
    assert differ == (not v.observe.startswith("no shape-only query")), (name, v.observe)


SMALLEST = {}
for _c in CASES:
    _k = (_c.v.op, _c.v.mode == "bf16") if _c.v.op != "conv5" else ("conv5", _c.variant.split("-")[0])
    _n = _c.B * _c.D * _c.H * _c.W * (_c.C0 + _c.C1) * _c.O
    if _c.v.op != "input" and (_k not in SMALLEST or _n < SMALLEST[_k][0]):
        SMALLEST[_k] = (_n, _c)
PAIR_PARITY = [min((c for c in CASES if c.v.op == "pair" and (c.D % 2, c.H % 2, c.W % 2) == p), key=lambda c: c.D * c.H * c.W * c.B * c.C0, default=None)
               for p in ((0, 0, 0), (1, 1, 1))]
IDENTITY = [c for _, c in SMALLEST.values()] + [c for c in PAIR_PARITY if c is not None]


@pytest.mark.parametrize("case", IDENTITY, ids=lambda c: c.cid)
def test_torch_oracle_equals_numpy_oracle_bit_for_bit(case):
    """5^3, 3^3, 2^3 stride 2 and the transposed 2^3 onto even and odd shapes: two independent float64 implementations agree exactly
    on the integer operands -- the claim the GPU `==` rests on."""
    d = S.operands(case)
    e = S.exact(case, d)
    if case.v.op == "pair":
        assert np.array_equal(e["y"], O.conv_nd_fwd(d["x"], d["w"], 2) + d["b"])
        dx, dw = O.conv_nd_bwd(d["x"], d["w"], d["dy"], 2)
        assert np.array_equal(e["dx0"], dx) and np.array_equal(e["dw"], dw)
        assert np.array_equal(e["yu"], O.conv_nd_transpose_fwd(d["xu"], d["wu"], case.dims, 2) + d["bu"])
        assert np.array_equal(e["dxu"], O.conv_nd_fwd(d["dyu"], d["wu"], 2))
        assert np.array_equal(e["dwu"], O.conv_nd_bwd(d["dyu"], d["wu"], d["xu"], 2, need_dx=False)[1])
        assert np.array_equal(e["dbu"], d["dyu"].reshape(-1, case.C0).sum(0))
    else:
        assert np.array_equal(e["y"], O.conv_nd_fwd(d["x"], d["w"], 1) + d["b"])
        dx, dw = O.conv_nd_bwd(d["x"], d["w"], d["dy"], 1)
        assert np.array_equal(np.concatenate((e["dx0"], e["dx1"]), -1), dx) and np.array_equal(e["dw"], dw)
        assert np.array_equal(e["db"], d["dy"].reshape(-1, case.O).sum(0))
    for a in e.values():
        assert np.array_equal(a, np.round(a))


@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_every_case_passes_the_exactness_guard(name):
    """bound(case) -- the oracle on |x|, |w|, |dy|, |bias| -- is at most 2^20, and the cheap bound operands() narrows the value range
    with really is an upper bound of it."""
    for c in BY_VARIANT[name]:
        d = S.operands(c)
        b = S.bound(c, d)
        assert b <= S.LIMIT, (c.cid, b)
        assert b <= S._cheap_bound(c, d) * (1 + 1e-12), (c.cid, b, S._cheap_bound(c, d))
        assert d["ranges"][0] >= 1 and d["ranges"][1] >= 1 and d["ranges"][2] >= 1


@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_route_and_plans(name, forced):
    """ops.route() answers the family the table claims for the forward, backward-data and filter-gradient launch of every case, under
    the case's mode and flags; and the library's shape-only queries agree with the restated planners (statistics rows = the form's
    brick count, workspace = the form's split), which is what ties a table row to the kernel that runs."""
    from vnet_tensorflow_amd import ops
    v = S.VARIANTS[name]
    for c in BY_VARIANT[name]:
        forced(c)
        for label, fam, args in S.launches(c):
            r = ops.route(*args)
            assert r.family == fam, "%s %s: routed to %s, the table says %s" % (c.cid, label, r.family, fam)
        exp = S.expected_queries(c)
        if exp is not None:
            r = ops.route(*S.launches(c)[0][2])
            assert (r.stats_rows, r.ws) == exp, "%s: library says rows, ws = %s, the restated plan %s" % (c.cid, (r.stats_rows, r.ws), exp)


def test_table_prints_every_case():
    assert len(S.table(CASES).splitlines()) == len(CASES) + 1


def test_class_pairs_the_each_choice_design_covers():
    """The generator is each-choice with rotated offsets, not pairwise: per variant and pair of axes it covers at least as many
    distinct class pairs as the longer of the two axes has classes (each class of an axis meets a different class of the other in
    every row), not all of them.  The counts go into profiles/conv_sweep.txt."""
    for name, d in S.pair_coverage(CASES).items():
        for (a, b), (have, total) in d.items():
            n = max(len(S.classes_of(S.VARIANTS[name], a)), len(S.classes_of(S.VARIANTS[name], b)))
            assert min(n, total) <= have <= total, (name, a, b, have, total)
