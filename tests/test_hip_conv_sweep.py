"""-m gpu: exact-integer ragged-shape sweep of every convolution kernel form (case table, generator and oracle: tests/conv_sweep.py;
the coverage conditions, the oracle identity and the 2^20 guard are proved on the host by tests/test_conv_sweep_host.py).

One test per case.  The case's kernel form is forced (library options, ops switches, compute mode), the layer runs forward and
backward through ops.conv / ops.conv_transpose2 / ops.input_conv INSIDE tests.guard.guarded() -- every tensor carved from an arena
whose surroundings are 0xFF, NaN in fp32 and in bf16, so an unmasked halo read becomes a NaN and a missed write leaves poison -- and
every result is compared with `torch.equal` against the float64 oracle: y, dx0, dx1 (bf16 tensors against round_bf16(exact)), dw and
db in fp32.  No tolerance: with integer operands whose partial sums stay below 2^20 every kernel's result is exact whatever its
summation order.  Then the arena's check() (guards intact, inputs unchanged) and check_written() (no output element left unwritten).
A mismatch is reported with its count, the first coordinates (b, z, y, x, c), and the brick and edge class of each axis they fall in.

Not exact, and not claimed to be: the epilogue statistics (sums of y^2 exceed 2^24) -- requested on the cases whose forward writes
them and held to the comparison and tolerance of test_hip_parity_holes.py::test_batch_norm_statistics_from_the_conv_epilogue
(mean: rel-L2 1e-6 or 1e-6 absolute, inverse standard deviation: rel-L2 1e-6); and the input block's dgamma / dbeta, sums over all
voxels, taps and channels -- held to test_hip_ops.py::test_input_block's 5e-5.

Variants Python cannot observe (c16 vs c16pp, deep vs generic, row-reuse / z-streaming filter gradients, X3_NB2) are separate rows
of the table with the other option value: both run against the oracle; the host test asserts the shape-only query that tells them
apart where one exists.  The grouped bf16 filter gradient runs through tests/test_hip_wgrad_group.py's own helper on sweep operands.

Measured on one MI355X in one session, this file inside the whole -m gpu suite (profiles/conv_sweep.txt has the case table with the
seconds of every case): the suite 282.3 s wall; this file's 354 tests 46.1 s; all other tests, i.e. the parent's suite, 228.1 s.  The
sweep costs 20 % of the parent's suite (a quarter would be 57 s), so nothing was thinned; the slowest case takes 1.9 s.  A pairwise
design (25 cases per variant in place of 5-8) would cost about four times as much, which is why the generator is each-choice.

THAT IT CAN FAIL.  Three value-only mutations of the library (no address or mask moved or widened), each one build and one run of this
file on the MI355X (354 tests: 353 cases + the grouped filter gradient; the unmutated library passes all 354), then the existing tests
of the mutated family against the same mutated library:
 1. conv_kernels.h XTile::issue_part, the tile staging of the fp32-tensor MFMA kernels: the first row past the high y edge reads 1.0, not 0.
    Sweep: 131 cases failed, every one a row whose kernels stage through XTile -- f32-k5-*, f32-wgrad-*, f32-k3-*, every f32-conv2-* row
    (direct rows: their filter gradient), input-im2col, and the f32x3 rows of the normal brick (x3-conv, -ksplit, -nb1, -nb2, x3-wgrad:
    conv_x3.h stages the wide brick through the same XTile).  No bf16 row, no input-direct row, no x3-*-narrow row failed.
    Existing tests: caught (test_hip_ops.py: test_conv5 10 cases, test_down_conv, test_up_conv, test_conv_family_random_shapes;
    test_hip_unet.py: test_conv3 11 cases).
 2. conv_kernels.h pack_bf16_elem, forward image of the bf16 5^3 filter: taps (0,1,2) and (0,2,1) swapped.
    Sweep: 97 cases failed, every one a bf16 5^3 row (b16-generic-*, -c16, -c16pp, -r32, -deep*, -padded, and the b16-wgrad-* rows, whose
    cases run the forward too); no fp32, f32x3, 2^3 or input-block row failed.
    Existing tests: caught (test_hip_b16.py 20 cases, test_hip_deep.py 22 cases).
 3. conv_c16pp.h epilogue: `ox < Wo` one column narrower where W is no multiple of 16.
    Sweep: 9 cases failed: the six b16-c16pp cases with ragged W, in y (768 of 1 584 384 elements in 2x3x8x2063: 0.05 %), and dx0 of
    b16-generic-4x8x16-1x516x8x31 and of two b16-r32 cases -- their backward-data launch has 16 output channels and >= 256 bricks, i.e. it
    IS the c16pp kernel.  No b16-c16 case (BF16_C16PP = 0) and no case with W = 16k failed.
    Existing tests: caught as well (test_hip_b16.py, 4 failed: the 30x50x70 and 33x40x49 shapes of CONV5_SHAPES, one statistics case, the
    c16 / c16pp bit-identity test).  The expectation that the hand-picked lists miss a one-column mask error did not hold for this kernel:
    check_bf16 forgives 0.5 % of unlucky roundings, but no wrong value.

ALL THREE PIECES OF THE f32x3 SPLIT (test_conv_sweep_x3_pieces).  Integer operands are bf16-exact: m = l = 0, so the tests above hold the
index math of the h plane only.  The seven f32x3 rows run again under the operand profiles of tests/conv_sweep.py (x-deep, w-deep,
dy-deep on every case; mid-dense-x, mid-dense-w, mid-mid on the most ragged case of each row): 18-bit and 9-10-bit operands that put
non-zero values into the m and l tile images, the m / l filter pieces and all six product streams, sized per case so that every
partial sum stays below 2^24 units -- y, dx0, dx1, dw (and db, except under dy-deep: a counted rounding bound) are still `==` the
float64 oracle.  Measured on one MI355X in one session, inside the whole -m gpu suite: the suite 350.8 s wall; these 174 tests 82.5 s;
all other tests, i.e. the parent's suite, 256.2 s (a quarter: 64 s).  All 306 (case, profile) pairs took 145 s and passed; being over
a quarter, the three mid profiles were thinned to one case per row as the sweep's rule says, the deep profiles were not (3 x 51
tests, 77 s).  The time is the host's float64 oracle, twice per test; the slowest test takes 4.3 s.
Mutations (value only; each one build, one run of the new tests and of test_hip_x3.py, the integer f32x3 rows, test_hip_insitu_backward.py,
test_hip_golden_full.py; details in profiles/conv_sweep.txt):
 1. conv_x3.h tile_commit writes 0 for the l piece of the last tile row: 18 new tests failed (x-deep and dy-deep of the nine cases
    whose last halo row lies inside the volume).  Parent: missed, all 103 tests passed.
 2. x3_pack.h / the batched repack write 0 for the l piece of pair 62, tap (4, 4, 4): 36 new tests failed, all w-deep.  Parent: every
    test that runs a kernel passed; test_hip_x3.py::test_x3_split_is_exact, which adds up the packed image itself, failed.
 3. conv_x3.h wgrad commit leaves the m piece of -dy un-negated in the negated bricks: 17 new tests failed (dy-deep and mid-mid of the
    cases with more bricks than filter-gradient workgroups).  Parent: caught, test_hip_x3.py 9 failed."""
import contextlib

import numpy as np
import pytest
import torch

from tests import conv_sweep as S
from tests import guard
from tests.util import check_close

pytestmark = pytest.mark.gpu
CASES = S.generate()
BF = torch.bfloat16


def _where(idx, shape, brick):
    """'(b, z, y, x, c) brick (bz, by, bx) z:interior|last(class) ...' of one element of a [B, D, H, W, C] tensor."""
    b, z, y, x, c = (int(v) for v in idx)
    parts = []
    for name, p, e, t in zip("zyx", (z, y, x), shape[1:4], brick):
        last = p // t == (e - 1) // t
        parts.append("%s: brick %d%s, offset %d of %d (%s)" % (name, p // t, " = last" if last else "", p % t, t, S.classify(e, t)))
    return "(b %d, z %d, y %d, x %d, c %d) %s" % (b, z, y, x, c, "; ".join(parts))


def _equal(case, name, got, exact, brick=None):
    """torch.equal(got, what the device must store for `exact`), with the location of the first mismatches in the message: the exact
    value itself in an fp32 tensor (dw and db in every mode), round_bf16 of it in a bf16 tensor."""
    assert got.dtype == (BF if (case.v.mode == "bf16" and brick is not None) else torch.float32), (case.cid, name, got.dtype)
    want = torch.from_numpy(np.ascontiguousarray(S.stored(case, exact) if got.dtype == BF else exact))
    have = got.detach().to(torch.float32).cpu().double()
    assert tuple(have.shape) == tuple(want.shape), "%s %s: shape %s vs %s" % (case.cid, name, tuple(have.shape), tuple(want.shape))
    if torch.equal(have, want):
        return
    bad = torch.nonzero(~(have == want))                     # (NaN != anything: poison that was read or left behind counts)
    lines = []
    for idx in bad[:6]:
        t = tuple(int(v) for v in idx)
        loc = _where(t, have.shape, brick) if (brick is not None and have.dim() == 5) else str(t)
        lines.append("  got %r, exact %r at %s" % (float(have[t]), float(want[t]), loc))
    raise AssertionError("%s %s: %d of %d elements differ from the exact result (brick %s)\n%s" % (
        case.cid, name, bad.shape[0], have.numel(), brick, "\n".join(lines)))


def _moments(case, y, mean, invstd):
    """The comparison of test_batch_norm_statistics_from_the_conv_epilogue, unchanged: float64 moments of the STORED tensor."""
    s = y.detach().to(torch.float32).double()
    mu = s.mean(dim=(0, 1, 2, 3))
    var = s.var(dim=(0, 1, 2, 3), unbiased=False)
    check_close(case.cid + " mean", mean, mu.cpu().numpy(), 1e-6, atol=1e-6)
    check_close(case.cid + " invstd", invstd, (1.0 / torch.sqrt(var + 1e-3)).cpu().numpy(), 1e-6)


@contextlib.contextmanager
def _arena(dev):
    arena = guard.Arena(dev)
    with guard.guarded(arena) as h:
        yield h
        torch.cuda.synchronize()
        arena.check()
        arena.check_written()
    del arena


def _stats_of(case, ops, y, C, h):
    st = getattr(y, "_vnet_stats", None)
    assert st is not None, "%s: the forward route has statistics rows but the launch wrote none" % case.cid
    _, mean, invstd = ops.bn_act(y, h.g(np.ones(C)), h.g(np.zeros(C)), "relu", None, None, False, None, None, want_stats=True)
    _moments(case, y, mean, invstd)


def _run_conv(case, dev, d, e):
    from vnet_tensorflow_amd import ops
    v = case.v
    ks = 3 if v.op == "conv3" else 5
    dt = BF if v.mode == "bf16" else torch.float32
    padded = v.families[0] == "conv-bf16-padded"
    brick = v.brick(case.W)
    fwd = ops.route(*S.launches(case)[0][2])
    with _arena(dev) as h:
        if padded:
            tx0, tx1 = ops.cast_input(h.g(d["x"])), None
            assert tx0.shape[-1] == 8 and tx0.dtype == BF
        else:
            tx0 = h.g(d["x"][..., :case.C0], None, dt).requires_grad_(True)
            tx1 = h.g(d["x"][..., case.C0:], None, dt).requires_grad_(True) if case.C1 else None
        tw, tb = h.g(d["w"]).requires_grad_(True), h.g(d["b"]).requires_grad_(True)
        y = ops.conv(tx0, tw, tb, ks, 1, x1=tx1)
        y.backward(h.g(d["dy"], None, dt))
        assert y.dtype == dt and tw.grad.dtype == torch.float32 and tb.grad.dtype == torch.float32
        _equal(case, "y", y, e["y"], brick)
        if not padded:
            _equal(case, "dx0", tx0.grad, e["dx0"], brick)
            if case.C1:
                _equal(case, "dx1", tx1.grad, e["dx1"], brick)
        _equal(case, "dw", tw.grad, e["dw"])
        _equal(case, "db", tb.grad, e["db"])
    if fwd.stats_rows > 0:
        with _arena(dev) as h, torch.no_grad():
            tx0 = ops.cast_input(h.g(d["x"])) if padded else h.g(d["x"][..., :case.C0], None, dt)
            tx1 = h.g(d["x"][..., case.C0:], None, dt) if case.C1 else None
            y = ops.conv(tx0, h.g(d["w"]), h.g(d["b"]), ks, 1, x1=tx1, bn_stats=True)
            _equal(case, "y (statistics launch)", y, e["y"], brick)
            _stats_of(case, ops, y, case.O, h)


def _run_pair(case, dev, d, e):
    from vnet_tensorflow_amd import ops
    v = case.v
    dt = BF if v.mode == "bf16" else torch.float32
    # bricks for the mismatch report: the down kernel's tile the coarse volume, the up kernel's (plan_conv, up = 1) the coarse INPUT --
    # a tensor on the fine volume is reported against twice the brick of the kernel that wrote it (down dx: the up kernel; up y likewise)
    direct = v.families[0] == "conv2-direct"
    brick = (1, 1, 16) if direct else S.plan_conv(2, 2, 0, case.C0, case.O, case.B, *case.coarse).brick
    up_brick = (1, 1, 16) if direct else S.plan_conv(2, 2, 1, case.O, case.C0, case.B, *case.coarse).brick
    fine_brick = tuple(2 * t for t in up_brick)
    down = ops.route(*S.launches(case)[0][2])
    with _arena(dev) as h:
        tx, tw, tb = h.g(d["x"], None, dt).requires_grad_(True), h.g(d["w"]).requires_grad_(True), h.g(d["b"]).requires_grad_(True)
        y = ops.conv(tx, tw, tb, 2, 2)
        y.backward(h.g(d["dy"], None, dt))
        _equal(case, "down y", y, e["y"], brick)
        _equal(case, "down dx", tx.grad, e["dx0"], fine_brick)
        _equal(case, "down dw", tw.grad, e["dw"])
        _equal(case, "down db", tb.grad, e["db"])
        txu, twu, tbu = h.g(d["xu"], None, dt).requires_grad_(True), h.g(d["wu"]).requires_grad_(True), h.g(d["bu"]).requires_grad_(True)
        yu = ops.conv_transpose2(txu, twu, tbu, case.dims)
        yu.backward(h.g(d["dyu"], None, dt))
        _equal(case, "up y", yu, e["yu"], fine_brick)
        _equal(case, "up dx", txu.grad, e["dxu"], brick)
        _equal(case, "up dw", twu.grad, e["dwu"])
        _equal(case, "up db", tbu.grad, e["dbu"])
    if down.stats_rows > 0:
        with _arena(dev) as h, torch.no_grad():
            y = ops.conv(h.g(d["x"], None, dt), h.g(d["w"]), h.g(d["b"]), 2, 2, bn_stats=True)
            _equal(case, "down y (statistics launch)", y, e["y"], brick)
            _stats_of(case, ops, y, case.O, h)


def _run_input(case, dev, d, e):
    from vnet_tensorflow_amd import ops
    v = case.v
    brick = v.brick(case.W)
    fwd = ops.route(*S.launches(case)[0][2])
    with _arena(dev) as h:
        timg, mean, invstd = h.g(d["x"]), h.g(d["mean"]), h.g(d["invstd"])
        tg, tbe, tw, tb = (h.g(d[k]).requires_grad_(True) for k in ("gamma", "beta", "w", "b"))
        y = ops.input_conv(timg, tg, tbe, mean, invstd, tw, tb)
        y.backward(h.g(d["dy"]))
        _equal(case, "y", y, e["y"], brick)
        _equal(case, "dw", tw.grad, e["dw"])
        _equal(case, "db", tb.grad, e["db"])
        check_close(case.cid + " dgamma", tg.grad, e["dgamma"], 5e-5)        # (sums above 2^24: tests/test_hip_ops.py's tolerance)
        check_close(case.cid + " dbeta", tbe.grad, e["dbeta"], 5e-5)
    if fwd.stats_rows > 0:
        with _arena(dev) as h, torch.no_grad():
            y = ops.input_conv(h.g(d["x"]), h.g(d["gamma"]), h.g(d["beta"]), h.g(d["mean"]), h.g(d["invstd"]), h.g(d["w"]), h.g(d["b"]),
                               bn_stats=True)
            _equal(case, "y (statistics launch)", y, e["y"], brick)
            _stats_of(case, ops, y, case.O, h)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.cid)
def test_conv_sweep(dev, case, lib_option, monkeypatch):
    d = S.operands(case)
    assert S._cheap_bound(case, d) <= S.LIMIT          # (an upper bound of bound(case), which the host test computes for every case)
    e = S.exact(case, d)
    with contextlib.ExitStack() as stack:
        S.force(case, lib_option, monkeypatch, stack)
        {"pair": _run_pair, "input": _run_input}.get(case.v.op, _run_conv)(case, dev, d, e)


# ---- the f32x3 rows again, on operands that fill all three pieces (S.PROFILES; proved on the host by test_conv_sweep_host.py) ----
X3 = S.x3_runs()


def _db_bounded(case, got, d, exact):
    """The bias gradient where dy is dense and three pieces deep: a column sum, no f32x3 product, whose terms exceed 2^24 units -- held
    per channel to k * 2^-24 * sum |dy| with k the roundings on an element's longest path (S.colsum_roundings), as tier B of
    tests/ew_sweep.py (gamma_k = k u / (1 - k u))."""
    M = case.B * case.D * case.H * case.W
    k = S.colsum_roundings(M, case.O)
    u = 2.0 ** -24
    lim = k * u / (1 - k * u) * np.abs(d["dy"]).reshape(-1, case.O).sum(0)
    err = np.abs(got.detach().cpu().double().numpy() - exact)
    print("%s db: k = %d, max err / bound = %.3g" % (case.cid, k, float((err / lim).max())))
    assert (err <= lim).all(), "%s db: error %s above the counted bound %s (k = %d)" % (case.cid, err, lim, k)


@pytest.mark.parametrize("case,profile", X3, ids=lambda v: v if isinstance(v, str) else v.cid)
def test_conv_sweep_x3_pieces(dev, case, profile, lib_option, monkeypatch):
    """One f32x3 case under one operand profile: forward and backward through ops.conv in the guarded arena, y, dx0, dx1 and dw `==`
    the float64 oracle (db too, except under dy-deep: _db_bounded), all three launches on the f32x3 kernels.  No statistics launch."""
    from vnet_tensorflow_amd import ops
    d = S.operands_x3(case, profile)
    S.check_e1(d, profile)
    assert max(d["bound"].values()) < S.X3_LIMIT
    e = S.exact(case, d)
    brick = case.v.brick(case.W)
    with contextlib.ExitStack() as stack:
        S.force(case, lib_option, monkeypatch, stack)
        with _arena(dev) as h:
            tx0 = h.g(d["x"][..., :case.C0]).requires_grad_(True)
            tx1 = h.g(d["x"][..., case.C0:]).requires_grad_(True) if case.C1 else None
            tw, tb = h.g(d["w"]).requires_grad_(True), h.g(d["b"]).requires_grad_(True)
            ops.profile_start()
            try:
                y = ops.conv(tx0, tw, tb, 5, 1, x1=tx1)
                y.backward(h.g(d["dy"]))
            finally:
                recs = [r[0] for r in ops.profile_stop()]
            assert sum(1 for t in recs if t.startswith("conv-x3")) == 2, recs           # forward and backward-data
            assert sum(1 for t in recs if t.startswith("wgrad-x3")) == 1, recs          # and the filter gradient
            _equal(case, "y", y, e["y"], brick)
            _equal(case, "dx0", tx0.grad, e["dx0"], brick)
            if case.C1:
                _equal(case, "dx1", tx1.grad, e["dx1"], brick)
            _equal(case, "dw", tw.grad, e["dw"])
            if profile == "dy-deep":
                _db_bounded(case, tb.grad, d, e["db"])
            else:
                _equal(case, "db", tb.grad, e["db"])


# ---- the grouped bf16 filter gradient (vnet_conv_wgrad_b16_group) through tests/test_hip_wgrad_group.py's helper -----------------
GROUP = [c for c in CASES if c.variant in ("b16-wgrad-rr", "b16-wgrad-4x4x16", "b16-wgrad-4x8x8", "b16-wgrad-zs") and all(
    k in S.RAGGED for k in S.case_classes(c))]


def test_grouped_filter_gradient_on_sweep_cases(dev, monkeypatch, lib_option):
    """One group that mixes ragged members of different bricks (4x8x32, 4x4x16, 4x8x8 and the z-streaming columns' shapes), integer
    operands, every member `==` the oracle.  The helper is used as it is: only the operands it draws are replaced."""
    from tests import test_hip_wgrad_group as TG
    assert len(set(c.variant for c in GROUP)) >= 3, GROUP
    by_shape = {(c.B, c.D, c.H, c.W, c.C0, c.C1, c.O): c for c in GROUP}

    def ints(shape, seed):
        c = by_shape[tuple(shape)]
        d = S.operands(c)
        return d["x"][..., :c.C0], (d["x"][..., c.C0:] if c.C1 else None), d["w"], d["b"], d["dy"]
    monkeypatch.setattr(TG, "_conv5_inputs", ints)
    ins, outs = TG._run_group(dev, list(by_shape))
    for c, dw in zip(by_shape.values(), outs):
        _equal(c, "grouped dw", dw, S.exact(c, S.operands(c))["dw"])
