"""The same bits from launch to launch: every kernel form of csrc/elementwise.hip and of the convolutions, and whole training steps on
channel counts off the vector paths.  DESIGN 4.6 promises it, the graph-vs-eager test, the resume test and every "bit for bit" A/B
record rest on it, and the exact sweeps cannot see a violation: their operands make every sum exact in any order.

PART 1, kernel forms (-m gpu).  One case for every row of tests/ew_sweep.py's table (the generic rows at C = 12 and 37, the head also
at C = 5, K = 2 and 5; their wide-row branch at C = 300) and for every row of tests/conv_sweep.py's table, plus the grouped (deferred) bf16 filter gradient; the case
builders and the launch code are the sweeps' own.  Operand profile `general`: float32 draws normal() * 2^uniform(-10, 10) in place of
the dyadic / integer values (labels, one-hot targets, seeds and the small per-channel coefficients stay what the family's generator
makes; bf16 tensors get bf16-representable values), so float addition is visibly not associative on them -- the host tests below sum
a column of every reduced operand forwards and in a fixed permutation and require different bits.
Extents: the smallest of 4099, 8209, ... rows at which the launch has at least two workgroups and a thread makes at least two trips
of its grid-stride loop (so all four waves of a block add to one output cell and partial rows of several blocks meet); a row whose
grid grows with its data gets the smallest such extent past the grid cap; a row with one workgroup by design (Row.nocap) keeps 4099
rows, or the most it takes.  A convolution row takes the smallest case of the sweep that has more than one brick -- and more than one
slab where the form splits -- per reduced output, with two sources where the row has them.
The assertion: eight launches from identical inputs, five on an otherwise idle device and three with company (an in-place multiply
of 256 MB on a second stream, enqueued just before the launch, both streams joined afterwards); outputs and scratch hold 0xFF before
the even and 0x00 before the odd launches, so an unwritten byte is a difference too; every output is byte-equal across the eight.
Accuracy is not this file's business.

PART 2, whole steps (-m gpu).  V-Net with NumChannel 12 and U-Net with NumChannel 6, two levels, on a 16^3 patch (levels of 12 / 24 /
48 and 6 / 12 channels: batch-norm backward, bias gradients and the head off the vector kernels), fp32 and fp32_split3, the eager step
and the captured step graph, dropout on in one combination of each network: two fresh models from one seed take three steps on the
same batches -- every loss, the flat gradient after the first step, and after the third every parameter, moving statistic and
optimiser slot are `==` as bytes (the model construction and the comparison are tests/test_hip_resume.py's).

On the parent commit (bn_act_bwd_reduce_kernel<2>, colsum_generic_kernel and head_bwd_generic_kernel added floats with LDS atomics)
this file fails (21 of the 128 GPU tests it had then); profiles/determinism.txt has what differed.  Wall time on the MI355X, this file
alone: 16.7 s for those 128 GPU tests, the slowest 0.8 s (the three C = 300 cases came later); the host tests take 22 s (they draw
every case's operands)."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import conv_sweep as CS
from tests import ew_sweep as S
from tests import guard
from tests import test_hip_ew_sweep as EW

gpu = pytest.mark.gpu
LAUNCHES, IDLE = 8, 5                       # launches per case; the first IDLE of them without company
COMPANY_BYTES = 256 << 20
U8 = torch.uint8


def general(rng, shape, bf16=False):
    """The `general` operand profile: normal() * 2^uniform(-10, 10), float32 (or bf16) representable, as float64."""
    a = (rng.standard_normal(shape) * 2.0 ** rng.uniform(-10.0, 10.0, shape)).astype(np.float32).astype(np.float64)
    return O.round_bf16(a) if bf16 else a


def not_associative(col):
    """Summing the column in float32 forwards and in a fixed permutation gives different bits."""
    col = np.asarray(col, np.float32).reshape(-1)
    perm = np.random.default_rng(len(col)).permutation(len(col))
    a, b = np.cumsum(col, dtype=np.float32)[-1], np.cumsum(col[perm], dtype=np.float32)[-1]
    return a.tobytes() != b.tobytes()


# ---- part 1, elementwise rows: the cases ---------------------------------------------------------------------------------------------
# rotated parameters a row's case is pinned to (everything else: the row's first rotation step, prelu / a residual / no tile where
# the row rotates them, so that dalpha exists and the residual stream is read)
GENERIC = [dict(C=12), dict(C=37)]
WIDE = dict(C=300)                                        # (a row per block and trip: the generic kernels' branch for C > 256)
PINNED = {
    "bn-moments-generic": GENERIC, "bn-reduce-m2": GENERIC + [WIDE], "colsum-generic": GENERIC + [WIDE],
    "head-bwd-generic": [dict(C=12, K=2), dict(C=37, K=5), dict(C=5, K=2), dict(C=5, K=5), dict(C=300, K=2)],
    "bn-bwd-composite": [dict(C=12)],                     # reduce (mode 2) -> apply
    "act-bwd-vec": [dict(C=48)], "act-bwd-scalar": [dict(C=37)],          # dalpha through the reduce kernel of mode 2
    "bn-moments-vec": [dict(C=64)], "bn-reduce-m0": [dict(C=64)], "colsum-vec": [dict(C=64)], "bn-moments-wide": [dict(C=300)],
}
PREFER = (("act", "prelu"), ("res", 1), ("bcast", 0), ("shift", 0), ("K", 2), ("B", 2), ("dev", 1), ("ex", 1), ("wx", 1), ("jac", 1))
EXTENTS = tuple(4099 * 2 ** k + (k > 0) for k in range(10))      # 4099, 8199, 16397, ...: odd, no multiple of a block


class EwCase(object):
    def __init__(self, row, pin, p):
        self.row, self.pin, self.p = row, pin, p
        self.id = "%s-%s%d" % (row, "".join("%s%s-" % kv for kv in sorted(pin.items())), p["M"])

    @property
    def geom(self):
        return S.ROWS[self.row].geom(self.p)


def _params(row, pin, size):
    p = S.params_of(row, 0, size)
    for k, v in PREFER:
        if k in row.rot and v in row.rot[k]:
            p[k] = v
    p.update(pin)
    if row.family == "cast":
        p["Cpad"] = S.cdiv(p["C"], 8) * 8
    p["_row"], p["_family"] = row.name, row.family
    return p


def trips(g):
    return S.cdiv(g.items, g.grid * g.per_block * g.U)


def _ew_case(row, pin):
    """The smallest extent of EXTENTS with >= 2 workgroups and >= 2 trips; a one-workgroup row (nocap): the first extent it accepts,
    from the top of what it takes."""
    for s in EXTENTS:
        for s1 in range(s, s + 8):
            p = _params(row, pin, s1)
            if row.accept(p):
                break
        else:
            continue
        g = row.geom(p)
        if g.grid >= 2 and trips(g) >= 2:
            return EwCase(row.name, pin, p)
    assert row.nocap, "%s %s: no extent gives two workgroups and two trips" % (row.name, pin)
    for s in (4099, 4098, 1021, 256):
        p = _params(row, pin, s)
        if row.accept(p) and (row.family != "partial" or s <= 1024):
            return EwCase(row.name, pin, p)
    raise AssertionError(row.name)


EW_CASES = [_ew_case(row, pin) for row in S.ROWS.values() for pin in PINNED.get(row.name, [{}])]

# the operands a family's generator makes that `general` replaces (the rest keeps its structure: labels, one-hot targets, seeds,
# per-channel coefficients), and those of them a kernel of the row sums over rows
DATA = {"bn": ("x", "dy", "r"), "small_fwd": ("x", "r"), "small_bwd": ("x", "dy", "r"), "bn_head": ("x", "r", "dl", "w", "bias"),
        "partial": ("part",), "head": ("x", "w", "bias", "dy"), "colsum": ("x",), "loss": ("z",), "dice": ("p",), "dropout": ("x", "dy"),
        "opt": ("p", "g", "m", "v", "acc"), "cast": ("x",), "patch": ("patch", "vol")}


def reduced(case):
    p, fam = case.p, S.ROWS[case.row].family
    op = p.get("op")
    if fam in ("bn", "small_fwd", "small_bwd"):
        if op == "moments" or fam == "small_fwd":
            return ("x",)
        if op in ("reduce", "bwd") or fam == "small_bwd" or (op == "act_bwd" and p["act"] == "prelu"):
            return ("dy",)
        return ()
    if fam == "bn_head":
        return {"fwd": ("x",), "reduce": ("dl",)}.get(op, ())
    if fam == "head":
        return ("x", "dy") if op == "bwd" else ()
    if fam in ("loss", "dice"):
        return ("p~",) if op == "fwd" else ()
    return {"partial": ("part",), "colsum": ("x",)}.get(fam, ())


def _first_draw(what, draw, columns):
    """The first of the draws 0, 1, ... (a seed each) whose reduced columns all pass not_associative(): a short column of values 2^20
    apart can sum to the same bits in two orders, and such a draw would show nothing."""
    for attempt in range(8):
        d = draw(attempt)
        if all(not_associative(col) for col in columns(d).values()):
            return d
    raise AssertionError("%s: no draw whose column sums depend on the order" % what)


def ew_operands(case):
    return _first_draw(case.id, lambda attempt: _ew_draw(case, attempt), lambda d: reduced_columns(case, d))


def _ew_draw(case, attempt):
    row = S.ROWS[case.row]
    gen, levels, _ = S.FAMILIES[row.family]
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (case.id, attempt)).encode()))
    d = gen(case.p, levels - 1, rng)
    b16 = bool(case.p.get("b16"))
    for k in DATA[row.family]:
        if k in d:
            d[k] = general(rng, d[k].shape, bf16=b16 and k in ("x", "dy", "r"))
    if "v" in d and row.family == "opt":
        d["v"] = np.abs(d["v"])                                               # (Adam's second moment: sqrtf of it)
    if row.family == "partial":
        d["part"][:, 1] = np.abs(d["part"][:, 1])
    return d


def reduced_columns(case, d):
    """{name: one column of the operand as the kernel sums it}."""
    out = {}
    for k in reduced(case):
        if k == "p~":                                                          # the loss sums p = softmax(z); dice sums p itself
            if "z" in d:
                z = d["z"].astype(np.float32)
                e = np.exp(z - z.max(-1, keepdims=True))
                a = (e / e.sum(-1, keepdims=True))[0]
            else:
                a = d["p"][0]
        else:
            a = d[k]
            if k == "x" and "r" in d and case.p.get("res"):
                a = (a.astype(np.float32) + d["r"].astype(np.float32))
        a = np.asarray(a)
        out[k] = a.reshape(-1, a.shape[-1] if a.ndim > 1 else 1)[:, 0]
    return out


# ---- part 1, convolution rows: the cases ---------------------------------------------------------------------------------------------
def _conv_case(v):
    """The smallest case of the sweep's own list with more than one brick (and, where the form splits, more than one slab) per reduced
    output; two sources where the row has them."""
    # (a bf16 column of a few dozen values sums exactly in float32 in any order: such a case would show nothing)
    voxels = lambda c: c.B * int(np.prod(c.grid_dims))
    cs = [c for c in CS.generate() if c.variant == v.name and (v.mode != "bf16" or voxels(c) >= 128)]
    size = lambda c: c.B * c.D * c.H * c.W * (c.C0 + c.C1 + c.O)
    for cond in (lambda c: v.items(c) > 1 and (v.split(c) or 2) > 1 and (c.C1 > 0 or not v.two_src),
                 lambda c: v.items(c) > 1 and (v.split(c) or 2) > 1, lambda c: v.items(c) > 1, lambda c: True):
        ok = [c for c in cs if cond(c)]
        if ok:
            return min(ok, key=size)
    raise AssertionError(v.name)


CONV_CASES = [_conv_case(v) for v in CS.VARIANTS.values()]
CONV_DATA = ("x", "w", "b", "dy", "xu", "wu", "bu", "dyu")


def conv_columns(c, d):
    return {k: d[k].reshape(-1, d[k].shape[-1])[:, 0] for k in ("dy", "x") + (("dyu", "xu") if c.v.op == "pair" else ())}


def conv_operands(c):
    return _first_draw(c.cid, lambda attempt: _conv_draw(c, attempt), lambda d: conv_columns(c, d))


def _conv_draw(c, attempt):
    rng = np.random.default_rng([c.seed, attempt])
    d = CS._draw(c, 1, 1, 1)                                                     # shapes, and the input block's integer coefficients
    b16 = c.v.mode == "bf16"
    for k in CONV_DATA:
        if k in d:
            d[k] = general(rng, d[k].shape, bf16=b16 and k in ("x", "dy", "xu", "dyu"))
    return d


# the grouped (deferred) bf16 filter gradient: one group of the sweep's ragged members, through tests/test_hip_wgrad_group.py's helper
GROUPED = "b16-wgrad-group"


# ---- host: coverage and the operand profile ------------------------------------------------------------------------------------------
def test_every_row_of_both_tables_has_a_case():
    """As tests/test_abi_ledger.py does for entry points: a new row of either table cannot be left out, and the pinned widths are
    the ones that take the generic kernels."""
    assert set(c.row for c in EW_CASES) == set(S.ROWS) and set(PINNED) <= set(S.ROWS)
    assert set(c.variant for c in CONV_CASES) == set(CS.VARIANTS) and len(CONV_CASES) == len(CS.VARIANTS)
    have = lambda name: set(tuple(sorted(c.pin.items())) for c in EW_CASES if c.row == name)
    for name in ("bn-moments-generic", "bn-reduce-m2", "colsum-generic"):
        assert have(name) >= {(("C", 12),), (("C", 37),)}, name
    assert have("head-bwd-generic") >= {(("C", 12), ("K", 2)), (("C", 37), ("K", 5)), (("C", 5), ("K", 2)), (("C", 5), ("K", 5))}
    assert all(any(("C", 300) in k for k in have(name)) for name in ("bn-reduce-m2", "colsum-generic", "head-bwd-generic"))
    for c in EW_CASES:
        if c.row in ("bn-reduce-m2", "bn-bwd-composite", "act-bwd-vec", "act-bwd-scalar", "colsum-generic", "bn-moments-generic"):
            assert S._red_mode(c.p["C"]) == 2, c.id
        if c.row.startswith("act-bwd"):
            assert c.p["act"] == "prelu", c.id                                 # (no other activation launches the reduce kernel)
    assert any(c.C1 > 0 for c in CONV_CASES) and any((c.v.split(c) or 1) > 1 for c in CONV_CASES)


@pytest.mark.parametrize("case", EW_CASES, ids=lambda c: c.id)
def test_elementwise_extents_and_operands(case):
    """The extent has two workgroups and two trips wherever the row has a grid at all, and every operand a kernel of the row sums
    over rows is visibly not associative."""
    row, g = S.ROWS[case.row], case.geom
    if row.nocap is None or g.grid > 1:
        assert g.grid >= 2 and trips(g) >= 2 and g.items >= 4 * 64, (case.id, g)
    d = ew_operands(case)
    cols = reduced_columns(case, d)
    assert set(cols) == set(reduced(case))
    for k, col in cols.items():
        assert col.size >= 256 and not_associative(col), "%s: the column sum of `%s` does not depend on the order" % (case.id, k)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.cid)
def test_convolution_operands(case):
    d = conv_operands(case)
    for k, col in conv_columns(case, d).items():
        assert not_associative(col), "%s: the column sum of `%s` does not depend on the order" % (case.cid, k)
        if case.v.mode == "bf16":
            assert np.array_equal(O.round_bf16(d[k]), d[k]), (case.cid, k)
    # more than one brick per reduced output, unless no case of the row has more
    assert case.v.items(case) > 1 or all(case.v.items(c) <= 1 for c in CS.generate() if c.variant == case.variant), case.cid


# ---- the eight launches ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def company(dev):
    """(side stream, a 256 MB tensor): busy() enqueues one elementwise pass over it on the side stream."""
    side = torch.cuda.Stream(device=dev)
    big = torch.ones(COMPANY_BYTES // 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    yield side, big
    del big


@contextlib.contextmanager
def _launch(company, k):
    """Launch k of a case: idle for k < IDLE, else next to the company's pass; both streams joined afterwards."""
    side, big = company
    torch.cuda.synchronize()
    if k >= IDLE:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            big.mul_(1.0)
    yield
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def poison(k):
    return 0xFF if k % 2 == 0 else 0x00


def _same_bytes(what, name, ref, got):
    """ref, got: uint8 device tensors of one output of two launches."""
    if ref.shape == got.shape and torch.equal(ref, got):
        return None
    if ref.shape != got.shape:
        return "%s: output `%s` has %d bytes in one launch and %d in another" % (what, name, ref.numel(), got.numel())
    return (name, ref, got)


def _report(what, k, diffs, itemsize):
    lines = []
    for name, ref, got in diffs:
        n = itemsize.get(name, 4)
        bad = torch.nonzero((ref != got).view(-1, n).any(1)).reshape(-1)
        lines.append("output `%s`: %d of %d elements differ, first at index %d" % (name, bad.numel(), ref.numel() // n, int(bad[0])))
    raise AssertionError("%s: launch %d (%s, pre-fill 0x%02X) is not launch 0 bit for bit\n  %s" % (
        what, k, "idle" if k < IDLE else "with company", poison(k), "\n  ".join(lines)))


def _eight(what, company, run):
    """run(k) -> ([(name, tensor)], keep-alive): eight launches, every output byte-equal to the first launch's."""
    ref, size = None, {}
    for k in range(LAUNCHES):
        with _launch(company, k):
            outs, keep = run(k)
        snap = [(n, t.detach().contiguous().view(-1).view(U8).clone()) for n, t in outs]
        size.update((n, t.element_size()) for n, t in outs)
        del outs, keep
        if ref is None:
            ref = snap
            assert ref, what
            continue
        assert [n for n, _ in snap] == [n for n, _ in ref], (what, "the launches made different outputs")
        diffs = [r for r in (_same_bytes(what, n, a, b) for (n, a), (_, b) in zip(ref, snap)) if r is not None]
        if diffs:
            assert all(not isinstance(r, str) for r in diffs), diffs
            _report(what, k, diffs, size)


class Env(EW.Env):
    """tests/test_hip_ew_sweep.py's plain environment with the launch's pre-fill in outputs and scratch."""

    def __init__(self, dev, fill):
        EW.Env.__init__(self, dev)
        self.fill = fill

    def o(self, shape, dtype=EW.F32):
        t = EW.Env.o(self, shape, dtype)
        t.view(-1).view(U8).fill_(self.fill)
        return t

    def ws(self, nbytes):
        t = EW.Env.ws(self, nbytes)
        t.fill_(self.fill)
        return t


@gpu
@pytest.mark.parametrize("case", EW_CASES, ids=lambda c: c.id)
def test_elementwise_row_repeats_itself(dev, company, case):
    row = S.ROWS[case.row]
    d = ew_operands(case)

    def run(k):
        env = Env(dev, poison(k))
        outs = EW.RUN[row.family](env, dict(case.p), d)
        assert set(n for n in row.entries if not n.endswith(("_ws_bytes", "_ok", "_rows"))) & set(env.called), (row.entries, env.called)
        return sorted(outs.items()), env
    _eight(case.id, company, run)


def _conv_run(case, d, h):
    """Forward and backward of the case's layer(s) inside the guarded arena, as tests/test_hip_conv_sweep.py runs them."""
    from vnet_tensorflow_amd import ops
    v = case.v
    dt = EW.BF if v.mode == "bf16" else EW.F32
    if v.op == "pair":
        tx, tw, tb = h.g(d["x"], None, dt).requires_grad_(True), h.g(d["w"]).requires_grad_(True), h.g(d["b"]).requires_grad_(True)
        ops.conv(tx, tw, tb, 2, 2).backward(h.g(d["dy"], None, dt))
        txu, twu, tbu = h.g(d["xu"], None, dt).requires_grad_(True), h.g(d["wu"]).requires_grad_(True), h.g(d["bu"]).requires_grad_(True)
        ops.conv_transpose2(txu, twu, tbu, case.dims).backward(h.g(d["dyu"], None, dt))
    elif v.op == "input":
        timg, mean, invstd = h.g(d["x"]), h.g(d["mean"]), h.g(d["invstd"])
        tg, tbe, tw, tb = (h.g(d[k]).requires_grad_(True) for k in ("gamma", "beta", "w", "b"))
        ops.input_conv(timg, tg, tbe, mean, invstd, tw, tb).backward(h.g(d["dy"]))
    else:
        ks = 3 if v.op == "conv3" else 5
        if v.families[0] == "conv-bf16-padded":
            tx0, tx1 = ops.cast_input(h.g(d["x"])), None
        else:
            tx0 = h.g(d["x"][..., :case.C0], None, dt).requires_grad_(True)
            tx1 = h.g(d["x"][..., case.C0:], None, dt).requires_grad_(True) if case.C1 else None
        tw, tb = h.g(d["w"]).requires_grad_(True), h.g(d["b"]).requires_grad_(True)
        ops.conv(tx0, tw, tb, ks, 1, x1=tx1).backward(h.g(d["dy"], None, dt))
        fwd = ops.route(*CS.launches(case)[0][2])
        if fwd.stats_rows > 0:                                                  # the statistics launch: partial rows of the epilogue
            with torch.no_grad():
                y = ops.conv(tx0.detach(), tw.detach(), tb.detach(), ks, 1, x1=None if tx1 is None else tx1.detach(), bn_stats=True)
                C = case.O
                ops.bn_act(y, h.g(np.ones(C)), h.g(np.zeros(C)), "relu", None, None, False, None, None, want_stats=True)


def _arena_outputs(arena):
    """Every tensor the product code allocated in the arena (results, gradients, statistics, packed images), in allocation order."""
    return [(e.name, e.tensor) for e in arena.entries if e.role in ("out", "inout")]


@gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.cid)
def test_convolution_row_repeats_itself(dev, company, case, lib_option, monkeypatch):
    d = conv_operands(case)
    with contextlib.ExitStack() as stack:
        CS.force(case, lib_option, monkeypatch, stack)

        def run(k):
            arena = guard.Arena(dev, poison=poison(k))
            with guard.guarded(arena) as h:
                _conv_run(case, d, h)
            return _arena_outputs(arena), arena
        _eight(case.cid, company, run)


@gpu
def test_grouped_filter_gradient_repeats_itself(dev, company, monkeypatch):
    """vnet_conv_wgrad_b16_group inside ops.deferred_wgrad_reduce(): the ragged members tests/test_hip_conv_sweep.py groups, general
    bf16 operands, every member's dw."""
    from tests import test_hip_conv_sweep as TCS
    from tests import test_hip_wgrad_group as TG
    by_shape = {(c.B, c.D, c.H, c.W, c.C0, c.C1, c.O): c for c in TCS.GROUP}
    assert len(set(c.variant for c in by_shape.values())) >= 3

    def inputs(shape, seed):
        c = by_shape[tuple(shape)]
        d = conv_operands(c)
        return d["x"][..., :c.C0], (d["x"][..., c.C0:] if c.C1 else None), d["w"], d["b"], d["dy"]
    monkeypatch.setattr(TG, "_conv5_inputs", inputs)

    def run(k):
        arena = guard.Arena(dev, poison=poison(k))
        with guard.guarded(arena, modules=(TG,), g_modules=(TG,)):
            TG._run_group(dev, list(by_shape))
        # (the members' dw: torch.full in the helper.  Their slab buffers are scratch, larger than the slabs the plan fills)
        return [(n, t) for n, t in _arena_outputs(arena) if n.startswith("full#")], arena
    _eight(GROUPED, company, run)


# ---- part 2: whole training steps ------------------------------------------------------------------------------------------------------
def _vnet12(compute, dropout):
    from tests import test_hip_resume as R
    cfg = R._vnet(dropout=dropout, compute=compute, nch=12)
    cfg["TrainingSetting"]["Networks"].update(NumLevels=2, NumConvolutions=[1, 2], BottomConvolutions=1)
    return cfg


def _unet6(compute, dropout):
    from tests.test_hip_unet import _cfg
    return _cfg(dropout=dropout, compute=compute, nch=6, levels=2)


# id -> (network, compute mode, step graph, dropout): every combination of the three, dropout in one combination of each network
STEPS = {"%s-%s-%s" % (net, compute, "graph" if graph else "eager"): (net, compute, graph, 0.05 if (compute == "fp32") == graph else 0.0)
         for net in ("vnet12", "unet6") for compute in ("fp32", "fp32_split3") for graph in (False, True)}


@gpu
@pytest.mark.parametrize("case", list(STEPS))
def test_training_steps_repeat_themselves(dev, monkeypatch, case):
    from tests import test_hip_resume as R
    net, compute, graph, dropout = STEPS[case]
    make = {"vnet12": _vnet12, "unet6": _unet6}[net]
    monkeypatch.setitem(R.CASES, case, (lambda: make(compute, dropout), graph, "torch", False))
    runs = []
    with R._mode(case, monkeypatch):
        batches = R._batches(case, dev)
        for _ in range(2):
            m = R._model(case, dev, 7)
            losses = R._steps(m, batches, 1)
            torch.cuda.synchronize()
            grad = m.flat.grad.clone()
            losses += R._steps(m, batches, 2)
            R._check_path(case, m)
            runs.append((losses, grad, R._snapshot(m)))
            del m
    (la, ga, sa), (lb, gb, sb) = runs
    widths = sorted(set(int(v.shape[-1]) for v in sa["net"].values() if v.dim() >= 1))
    assert any(S._red_mode(C) == 2 for C in widths), (case, widths)             # (the steps did run the generic kernels)
    print("%s: losses %s" % (case, la))
    assert [np.float64(v).tobytes() for v in la] == [np.float64(v).tobytes() for v in lb], (case, la, lb)
    ndiff = int((ga.view(torch.int32) != gb.view(torch.int32)).sum())
    assert bool(ga.any()) and ndiff == 0, "%s: flat gradient after the first step: %d of %d elements differ" % (case, ndiff, ga.numel())
    R._same(sb, sa, case)
