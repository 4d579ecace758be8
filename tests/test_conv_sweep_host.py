"""Host-side checks of the exact-integer convolution sweep (tests/conv_sweep.py): the coverage conditions of the generated case
set, stated as code; the identity of the float64 torch oracle and oracle/vnet_oracle.py on integer operands, which the GPU
comparison rests on; the 2^20 exactness guard of every case; the restated C planners against the library's shape-only queries; and
ops.route()'s family for every launch of every case, so that a routing change fails here and does not silently empty the sweep.
For the operand profiles of the f32x3 rows (S.PROFILES): the split identity, the two exactness conditions, the piece shares, the
coverage of sparse filters and of the filter gradient's bricks, and a float32 restatement of the six product streams."""
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


# ---- the operand profiles of the f32x3 rows (S.PROFILES): operands that fill the m and l pieces, still compared with `==` ------------
X3_CASES = S.x3_cases()
X3_RUNS = S.x3_runs()
# the sparse operand(s) of the filter-gradient launch (x, dy), per profile
WGRAD_SPARSE = {"x-deep": ("dy",), "w-deep": ("x", "dy"), "dy-deep": ("x",), "mid-dense-x": ("dy",), "mid-dense-w": ("x", "dy"), "mid-mid": ("dy",)}
COVER_FILTER = ("x-deep", "dy-deep", "mid-mid")                  # profiles whose filter is the sparse side of both convolution launches
EMPTY_CAP = 0.25


def x3_conditions(c, profile):
    """Every host condition of one (case, profile); returns the figures of its row in profiles/conv_sweep.txt."""
    d = S.operands_x3(c, profile)
    pieces = S.check_e1(d, profile)                               # the split identity and (E1)
    b = d["bound"]                                                # (E2): bound_x3 of these very operands, the oracle on magnitudes
    assert max(b.values()) < S.X3_LIMIT, (c.cid, profile, b)
    assert ("db" in b) == (profile != "dy-deep")
    assert np.array_equal(d["b"], np.round(d["b"]))
    row = dict(thin=d["thin"], bound=max(b.values()), m=0.0, l=0.0, empty=0.0)
    deep = S.DEEP.get(profile)
    if deep:
        a, (h, m, l) = d[deep], pieces[deep]
        row["m"], row["l"] = float((m != 0).mean()), float((l != 0).mean())
        assert row["m"] >= S.M_FLOOR, (c.cid, profile, row)
        assert row["l"] >= S.l_floor(c, profile), (c.cid, profile, row, S.l_floor(c, profile))
        for piece in (a, h, m) + ((l,) if S.DEPTHS[profile][("x", "w", "dy").index(deep)] == 3 else ()):
            assert (piece > 0).any() and (piece < 0).any(), (c.cid, profile)
        assert a.all(), "the deep operand of %s is dense" % profile
    else:                                                         # mid-mid: every operand carries second pieces of both signs
        for name in ("x", "w", "dy"):
            m = pieces[name][1]
            assert (m > 0).any() and (m < 0).any(), (c.cid, name)
        row["m"] = float((pieces["x"][1] != 0).mean())
    if profile in COVER_FILTER:
        nz = d["w"].reshape(125, c.C0 + c.C1, c.O) != 0
        assert nz.any(2).all(), "%s %s: a (tap, input channel) without a weight" % (c.cid, profile)
        assert nz.any(1).all(), "%s %s: a (tap, output channel) without a weight" % (c.cid, profile)
    else:
        assert (np.abs(d["w"]).reshape(125, -1).max(1) > 0).all()
    p = S.x3_wgrad_plan(c.C0 + c.C1, c.O, c.B, c.D, c.H, c.W)
    assert p.brick == c.v.brick(c.W) and p.nb == S._bricks_of((c.B,) + c.dims, p.brick)
    row["empty"] = max(S.empty_bricks(d[name], p.brick) for name in WGRAD_SPARSE[profile])
    if row["empty"] > 0:
        print("%s %s: %.1f %% of the %d bricks hold no non-zero of the sparse operand" % (c.cid, profile, 100 * row["empty"], p.nb))
    assert row["empty"] <= EMPTY_CAP, (c.cid, profile, row)
    if c.v.launch == "wgrad":                                     # (the filter-gradient rows are small: (E2) leaves room for every brick)
        assert row["empty"] == 0.0, (c.cid, profile, row)
    return row


@pytest.mark.parametrize("case", X3_CASES, ids=lambda c: c.cid)
def test_x3_profiles_hold_their_conditions(case):
    """Per (case, profile): the restated split reproduces every operand, (E1) and (E2) hold, the deep operand has m != 0 in >= 90 % and
    l != 0 in >= l_floor (20 %, or what (E2) leaves at that channel ratio) of its elements with both signs in every piece, a sparse
    filter uses every (tap, input channel) and every (tap, output channel), and the sparse operand of the filter gradient reaches
    every brick of x3_wgrad_plan's tiling (at most 25 % empty, none on the filter-gradient rows)."""
    profiles = [p for c, p in X3_RUNS if c == case]
    assert set(("x-deep", "w-deep", "dy-deep")) <= set(profiles)
    for profile in profiles:
        x3_conditions(case, profile)


def test_x3_runs_keep_every_profile_on_every_row():
    """The deep profiles run on every f32x3 case; the mid-dense and mid-mid profiles on the most ragged case of each of the seven rows."""
    assert set(X3_RUNS) <= set((c, p) for c in X3_CASES for p in S.PROFILES)
    for name in set(c.variant for c in X3_CASES):
        for p in S.PROFILES:
            cs = [c for c, q in X3_RUNS if q == p and c.variant == name]
            assert cs, (name, p)
            if p.startswith("mid"):
                n = sum(k in S.RAGGED for k in S.case_classes(cs[0]))
                assert len(cs) == 1 and n == (2 if name.endswith("narrow") else 3), (name, p, cs)
            else:
                assert len(cs) == len(BY_VARIANT[name])


def test_x3_profiles_reach_every_stream():
    """Over the profiles, each of the three launches multiplies non-zero pieces in each of the six streams."""
    for ia, ib in ((0, 1), (2, 1), (0, 2)):                      # (x, w), (dy, w), (x, dy)
        reached = set()
        for dep in S.DEPTHS.values():
            reached |= set((pa, pb) for pa in range(dep[ia]) for pb in range(dep[ib]))
        assert reached >= {(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)}, (ia, ib, reached)


def _smallest_x3(n=3):
    best = {}
    for c in X3_CASES:
        k = c.B * c.D * c.H * c.W * (c.C0 + c.C1) * c.O
        if c.variant not in best or k < best[c.variant][0]:
            best[c.variant] = (k, c)
    return [c for _, c in sorted(best.values(), key=lambda t: t[0])[:n]]


def _patches(a):
    """[voxels, 125 * C] SAME-padded 5^3 patches of a [B, D, H, W, C] tensor (tap-major, as a [5, 5, 5, C, .] filter reshapes)."""
    B, D, H, W, C = a.shape
    p = np.pad(a, ((0, 0), (2, 2), (2, 2), (2, 2), (0, 0)))
    v = np.lib.stride_tricks.sliding_window_view(p, (5, 5, 5), axis=(1, 2, 3))          # [B, D, H, W, C, 5, 5, 5]
    return np.ascontiguousarray(np.moveaxis(v, 4, 7)).reshape(B * D * H * W, 125 * C)


STREAMS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))


def _emulate(A, Bm, drop=None):
    """sum_k A[n, k] B[k, o] from the six streams of the pieces, every product and every partial sum in float32, in three orders:
    sequential, sequential over a random permutation of the (stream, k) terms, numpy's pairwise reduction (with a stream dropped:
    the pairwise one only).  A, Bm: piece triples; streams whose pieces are all zero add exact zeros and are left out."""
    live = [(pa, pb) for s, (pa, pb) in enumerate(STREAMS) if s != drop and A[pa].any() and Bm[pb].any()]
    if not live:
        return [np.zeros((A[0].shape[0], Bm[0].shape[1]), np.float32)]
    terms = np.concatenate([A[pa].astype(np.float32)[:, :, None] * Bm[pb].astype(np.float32)[None, :, :] for pa, pb in live], axis=1)
    assert terms.dtype == np.float32
    if drop is not None:
        return [terms.sum(axis=1, dtype=np.float32)]
    seq = lambda t: np.add.accumulate(t, axis=1, dtype=np.float32)[:, -1]
    return [seq(terms), seq(terms[:, np.random.default_rng(7).permutation(terms.shape[1])]), terms.sum(axis=1, dtype=np.float32)]


@pytest.mark.parametrize("profile", S.PROFILES)
@pytest.mark.parametrize("case", _smallest_x3(), ids=lambda c: c.cid)
def test_x3_six_stream_emulation_equals_the_oracle(case, profile):
    """The kernels' arithmetic restated in float32 -- six streams of piece products, summed in three orders -- equals the float64
    oracle bit for bit on the profile's operands (what the GPU `==` rests on), for y, dx and one tap plane of dw; and leaving out any
    one stream the profile's depths reach changes the result, so no reachable stream is multiplying zeros."""
    d = S.operands_x3(case, profile)
    pc = S.check_e1(d, profile)
    e = S.exact(case, d)
    Cin, Co = case.C0 + case.C1, case.O
    dx = np.concatenate((e["dx0"], e["dx1"]), -1)
    wf = lambda a: a.reshape(125 * Cin, Co)
    wb = lambda a: np.ascontiguousarray(a[::-1, ::-1, ::-1].transpose(0, 1, 2, 4, 3)).reshape(125 * Co, Cin)
    dx_, dw_ = ("dy", "w"), ("x", "dy")
    jobs = [("y", tuple(_patches(p) for p in pc["x"]), tuple(wf(p) for p in pc["w"]), e["y"].reshape(-1, Co) - d["b"], (0, 1)),
            ("dx", tuple(_patches(p) for p in pc["dy"]), tuple(wb(p) for p in pc["w"]), dx.reshape(-1, Cin), (2, 1)),
            # dw[tap 62 (the centre), ci, co] = sum_v x[v, ci] dy[v, co]
            ("dw", tuple(p.reshape(-1, Cin).T for p in pc["x"]), tuple(p.reshape(-1, Co) for p in pc["dy"]), e["dw"].reshape(125, Cin, Co)[62], (0, 2))]
    dep = S.DEPTHS[profile]
    for name, A, Bm, want, (ia, ib) in jobs:
        for got in _emulate(A, Bm):
            assert np.array_equal(got.astype(np.float64), want), (case.cid, profile, name)
        for s, (pa, pb) in enumerate(STREAMS):
            if pa < dep[ia] and pb < dep[ib]:
                assert not np.array_equal(_emulate(A, Bm, drop=s)[0].astype(np.float64), want), (case.cid, profile, name, "stream", s)
            else:
                assert not A[pa].any() or not Bm[pb].any(), (case.cid, profile, name, s)


def test_colsum_roundings_counts_the_vector_and_the_generic_kernel():
    """The counted bound of the dy-deep bias gradient: trips - 1 + log2(256 / (C / 4)) + 1 roundings in the vector kernel; a thread's
    trips - 1, the 256 / C - 1 additions of the group sums in their fixed order and + 1 in the generic one (C / 4 no power of two: the
    48-channel cases)."""
    assert S.colsum_roundings(1024, 16) == 3 + 6 + 1                      # 4096 float4 on 5 blocks (a block per 1024): 4 trips
    assert S.colsum_roundings(1024 * 256 * 3, 16) == 11 + 6 + 1           # the grid cap, 1024 blocks: 12 trips
    assert S.colsum_roundings(1024, 32) == 3 + 5 + 1
    assert S.colsum_roundings(64, 48) == 3 + 4 + 1                        # 64 rows on 4 blocks of 5 row groups: 4 trips, 5 groups meet
    assert S.colsum_roundings(7, 300) == 2 + 0 + 1                        # 7 rows on 3 blocks, a row per block and trip: 3 trips, nothing meets
    assert any(c.O == 48 for c in X3_CASES) and any(c.O in (16, 32) for c in X3_CASES)
