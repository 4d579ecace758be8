"""The exact per-element sweep of csrc/elementwise.hip: variant table, case generator, operand generator, exact oracle and bound().
Host only (NumPy); tests/test_ew_sweep_host.py proves the design on the CPU, tests/test_hip_ew_sweep.py runs the cases on the device.

THE PRINCIPLE.  Almost every formula of elementwise.hip is exact in float32 when its operands are small dyadic rationals: then
neither the summation order nor the contraction of a multiply-add changes a result and the comparison with the float64 oracle is
`==` on every element.  Every checked output has one of three tiers (Row.tiers):
  E  exact: operands dyadic with at most q fractional bits and  sum |terms| * 2^q < 2^24  over the whole column / dot product, so
     every float32 partial sum of every order is exact.  bound(case) evaluates that condition on the case's own operands (the oracle
     on absolute values, as tests/conv_sweep.py does); a case that exceeds it gets the next narrower operand level, never dropped.
     A bf16 output is compared with round_bf16(exact).  Values are compared, not bit patterns (0 * z of the bf16 ReLU is -0).
  R  one rounding, restated: a fixed sequence of individually rounded IEEE operations in which no multiplication feeds an addition
     (0.2f * z, (float)(double quotient), Adam's lr_t * m / (sqrtf(v) + eps) and the subtraction, the bf16 cast): the formula is
     evaluated in NumPy float32 (Arith(f32=True)) and compared with `==`.
  B  bounded: |got - ref| <= k * 2^-24 * magnitude per element, k = the number of roundings of the kernel's formula, counted next to
     each use (invstd, the loss / dice values and their coefficients, the small-tensor backward's ds whose 1 / M is not dyadic).

Each family's formula is written ONCE against an arithmetic object (Arith): float64 for the oracle (recording sum |terms| for
bound()), float32 with the sums taken forward / in reverse / pairwise and each multiply-add rounded twice or once for the host proof.

THE TABLE.  One Row per launchable kernel form (template instantiation + the dispatch branch that selects it).  Row.geom restates
the launcher: the work items handed to ew_blocks(), the items the loop walks, the items a block takes per slot and the unroll
factor; the constants come from the source through test_hip_elementwise_trips._consts().  Shape classes say where the end of the
data falls relative to a unit of the kernel -- `vec` (a thread's vector, where a scalar tail exists), `block` (one block's slot),
`grid` (one slot of the whole grid) and `group` (an unrolled group of U slots) -- as lt / eq / r1 / rm1 / mult (conv_sweep.classify),
plus, for the kernels with clamped duplicate loads, `slot: out` (the last trip has a slot entirely out of range and one in range).
All size axes of a row are functions of ONE extent (M, V or n), so they cannot be combined freely as the three axes of a
convolution can.  The generator (_gen_row) rotates the parameters (act, residual, K, B, C, bcast, face ...) by one position per
case and gives EVERY rotation step a non-degenerate extent -- more than one block's slot and at least five rows -- namely the one that
realises the most classes still missing, preferring an extent past the grid's first slot and a ragged block tail; further cases,
of any extent (one row among them), follow until every class of every axis has occurred; a rotated value whose step collides with a
refused combination (bcast with a residual) gets a later step.  The host test asserts that every rotated value occurs at a
non-degenerate extent.  A class a row cannot realise below the grid cap is listed in
Row.absent with the reason; the host test checks both directions.  Per row one more case past the grid cap (capped=True; `nocap`
says why where a form has no cap), asserted through the trips test's _wraps().

Two things the table states differently from a first reading of the launchers.  red_mode(8) is 0: C = 8 is two quads and takes the
vector kernels, so the row-mode rows use C = 1, 3, 7.  The backward of the leaky ReLU multiplies dy by 0.2f, a rounding in front of
every sum and every multiply-add of the backward formulas: neither E nor R, so the reduce / apply rows rotate none, relu and prelu
and the leaky ReLU is swept forward only (tier R)."""
import collections
import os
import zlib

import numpy as np

from oracle import vnet_oracle as O
from tests.conv_sweep import CLASSES, classify
from tests.test_hip_elementwise_trips import _consts, _red_mode, _wraps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, MAXBLK, RED_U, LOSS_U, CS16_BLOCK, CS16_MAXBLK = _consts()
TRIP = BLOCK * MAXBLK
LIMIT = 1 << 24
U24 = 2.0 ** -24
ACT = {"none": 0, "relu": 1, "prelu": 2, "lrelu": 3}
EPS = float(np.float32(1e-3))
M_TOTAL = 64.0
ITEMS_MAX = 2600                        # the search range of the generator, in loop items (past the largest realisable class)


def cdiv(a, b):
    return -(-a // b)


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------
class Arith(object):
    """float64 (the oracle; sum() records sum |terms| per name) or float32 with a summation order and a contraction mode."""

    def __init__(self, f32=False, fused=True, order="fwd"):
        self.f32, self.fused, self.order = f32, fused, order
        self.dt = np.float32 if f32 else np.float64
        self.mag = {}

    def v(self, a):
        return np.asarray(a, dtype=self.dt)

    def mul(self, a, b):
        return self.v(a) * self.v(b)

    def add(self, a, b):
        return self.v(a) + self.v(b)

    def sub(self, a, b):
        return self.v(a) - self.v(b)

    def div(self, a, b):
        return self.v(a) / self.v(b)

    def fma(self, a, b, c):
        """a * b + c: contracted (computed in float64, rounded once) or not (rounded twice)."""
        if self.f32 and self.fused:
            return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
        return self.add(self.mul(a, b), c)

    def sum(self, name, t, axis=0, q=0):
        """Sum over `axis`; the oracle records sum |terms| * 2^q (q: fractional bits of a term)."""
        t = np.moveaxis(self.v(t), axis, 0)
        if not self.f32:
            self.mag[name] = np.abs(t).sum(0) * 2.0 ** q
            return t.sum(0)
        if t.shape[0] == 0:
            return np.zeros(t.shape[1:], np.float32)
        if self.order == "fwd":
            return np.cumsum(t, axis=0, dtype=np.float32)[-1]
        if self.order == "rev":
            return np.cumsum(t[::-1], axis=0, dtype=np.float32)[-1]
        while t.shape[0] > 1:                                                   # pairwise
            if t.shape[0] & 1:
                t = np.concatenate([t, np.zeros((1,) + t.shape[1:], np.float32)])
            t = t[0::2] + t[1::2]
        return t[0]

    def note(self, name, t, q=0):
        """An elementwise E output counts for bound() like a sum of one term."""
        if not self.f32:
            self.mag[name] = (np.abs(np.asarray(t, np.float64)).max() if np.size(t) else 0.0) * 2.0 ** q
        return t


PROOFS = [(o, f) for o in ("fwd", "rev", "pair") for f in (False, True)]


# ---- geometry ------------------------------------------------------------------------------------------------------------------
Geom = collections.namedtuple("Geom", "launch items per_block U blocks grid vec capped")


def G(launch, items, per_block=None, U=1, blocks=1, grid=None, vec=None, cap=None):
    """ew_blocks(launch) * blocks workgroups (or `grid` of them, cap `cap`), the loop walks `items`, per_block of them per block and
    slot, U slots a trip.  vec = (elements, vector width) where the kernel has a scalar tail."""
    per_block = BLOCK if per_block is None else per_block
    if grid is None:
        grid = min(MAXBLK, max(1, cdiv(launch, BLOCK))) * blocks
        capped = cdiv(launch, BLOCK) >= MAXBLK
    else:
        capped = cap is not None and grid >= cap
    return Geom(launch, items, per_block, U, blocks, grid, vec, capped)


def classes(g):
    """{axis: class} of one launch."""
    stride = g.grid * g.per_block
    out = {"block": classify(g.items, g.per_block), "grid": classify(g.items, stride)}
    if g.U > 1:
        out["group"] = classify(g.items, g.U * stride)
        rem = g.items - (cdiv(g.items, g.U * stride) - 1) * g.U * stride
        out["slot"] = "out" if cdiv(rem, stride) < g.U else "in"
    if g.vec:
        out["vec"] = classify(*g.vec)
    return out


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _ints(rng, m, shape):
    return rng.integers(-m, m + 1, size=shape).astype(np.float64)


def _pick(rng, vals, shape):
    return np.asarray(vals, np.float64)[rng.integers(0, len(vals), size=shape)]


# operand levels of the batch-norm formulas, widest (the ranges the design was checked with) first
# (qa, qi, qg: fractional bits of alpha, invstd, gamma -- what the q of every sum below is made of)
BN_LEVELS = [dict(R=3, mu=2, inv=(0.5, 1, 2), al=(0.125, 0.25, 0.5), ga=(-1.5, -0.5, 0.5, 1, 1.5, 2), be=3, S=64, w=2, qa=3, qi=1, qg=1),
             dict(R=2, mu=1, inv=(0.5, 1, 2), al=(0.25, 0.5), ga=(-1.5, -0.5, 0.5, 1, 1.5, 2), be=2, S=32, w=1, qa=2, qi=1, qg=1),
             dict(R=1, mu=1, inv=(0.5, 1, 2), al=(0.5,), ga=(-1, -0.5, 0.5, 1, 2), be=1, S=16, w=1, qa=1, qi=1, qg=1),
             dict(R=1, mu=1, inv=(1, 2), al=(0.5,), ga=(-1, 1, 2), be=1, S=8, w=1, qa=1, qi=0, qg=0)]


def _bn_operands(p, lv, rng):
    M, C, k = p["M"], p["C"], BN_LEVELS[lv]
    d = {"x": _ints(rng, k["R"], (M, 1 if p.get("bcast") else C)), "dy": _ints(rng, k["R"], (M, C)),
         "mean": _ints(rng, k["mu"], C), "invstd": _pick(rng, k["inv"], C), "gamma": _pick(rng, k["ga"], C),
         "beta": _ints(rng, k["be"], C), "alpha": _pick(rng, k["al"], C), "sdz": _ints(rng, k["S"], C),
         "sdzx": _ints(rng, k["S"], C), "ex": _pick(rng, (0, 0.25, -0.5), C), "q": k}
    if p.get("res"):
        d["r"] = _ints(rng, k["R"], (M, C))
    if "K" in p:                                                              # the fused head
        K = p["K"]
        d.update(w=_ints(rng, k["w"], (C, K)), bias=_ints(rng, 2, K), dl=_ints(rng, k["w"], (M, K)))
    return d


# ---- batch-norm formulas (bn_act_fwd_kernel, bn_act_bwd_reduce_kernel, bn_act_bwd_apply_kernel and their bf16 / fused twins) ------
def _act_fwd(A, z, act, al):
    if act == "relu":
        return np.maximum(z, 0)
    if act == "prelu":                                                        # fmaxf(z, 0) + al * fminf(z, 0)
        return A.fma(al, np.minimum(z, 0), np.maximum(z, 0))
    if act == "lrelu":                                                        # z > 0 ? z : 0.2f * z  (tier R)
        return np.where(z > 0, z, A.mul(A.v(float(np.float32(0.2))), z))
    return z


def _act_grad(A, z, act, al):
    if act == "relu":
        return A.v(z > 0)
    if act == "prelu":                                                        # TF tie rule: 0 at z == 0
        return np.where(z > 0, A.v(1), np.where(z < 0, A.v(al) + 0 * z, A.v(0)))
    assert act == "none", "the leaky ReLU's backward rounds 0.2f * dy: neither E nor R, not in the table"
    return A.v(np.ones_like(z))


def _bn_core(A, p, d):
    M, C = p["M"], p["C"]
    v = A.v(np.broadcast_to(d["x"], (M, C)))
    if p.get("res"):
        v = A.add(v, d["r"])
    if p.get("identity"):
        return v, A.v(np.ones(C)), v
    s = A.mul(d["gamma"], d["invstd"])
    sf = A.fma(-A.v(d["mean"]), s, d["beta"])                                  # beta - mean * s
    return v, s, A.fma(v, s, sf)


def _bn_back(A, p, d, dy):
    """dz, xhat, dy * min(0, z) of the backward kernels."""
    v, s, z = _bn_core(A, p, d)
    dz = A.mul(dy, _act_grad(A, z, p["act"], d["alpha"]))
    if p.get("identity"):
        xh = A.v(np.zeros_like(v))
    else:
        xh = A.mul(A.sub(v, d["mean"]), d["invstd"])
    return v, s, z, dz, xh, A.mul(dy, np.minimum(z, 0))


def _apply(A, s, dz, xh, k1, k2, ex):
    """sc * (dz - k1 - xh * k2) + xh * ex"""
    t = A.fma(-xh, k2, A.sub(dz, k1))
    return A.fma(xh, ex, A.mul(s, t))


def _q(d, what):
    """Fractional bits of a term: the sum of the level's bits of alpha (a), invstd (i), gamma (g), one letter per factor."""
    return sum(d["q"]["q" + ch] for ch in what)


def _invstd_ref(S, Q, M, eps=EPS):
    """invstd = (float)(1 / sqrt(max(Q / M - mu^2, 0) + eps)) from exact sums.  Tier B, k = 2: one float32 rounding of the result
    (2^-24 relative); the float64 steps in front of it add at most 2^-52 * (Q / M + mu^2) / (var + eps) < 2^-35 relative for
    |v| <= 8 and eps = 1e-3, whether or not the compiler contracts mu * mu into the subtraction; the second unit is slack."""
    mu = S / M
    ref = 1.0 / np.sqrt(np.maximum(Q / M - mu * mu, 0.0) + eps)
    return ref, 2 * U24 * np.abs(ref)


def _mean_ref(S, M):
    return np.asarray(np.asarray(S, np.float64) / M, np.float32).astype(np.float64)      # (float)(double quotient): tier R


def f_bn(A, p, d):
    op, M = p["op"], p["M"]
    out = {}
    if op == "moments":
        v = _bn_core(A, dict(p, identity=1), d)[0]
        S, Q = A.sum("sum", v), A.sum("sumsq", A.mul(v, v))
        out["sums"] = np.concatenate([S, Q])
        S, Q = np.asarray(S, np.float64), np.asarray(Q, np.float64)
        out["mean"] = _mean_ref(S, M)
        out["invstd"], out["invstd~"] = _invstd_ref(S, Q, M)
    elif op == "fwd":
        out["y"] = A.note("y", _act_fwd(A, _bn_core(A, p, d)[2], p["act"], d["alpha"]), _q(d, "gia"))
    elif op == "reduce":
        _v, _s, _z, dz, xh, a2 = _bn_back(A, p, d, d["dy"])
        out["dbeta"], out["dgamma"] = A.sum("dbeta", dz, q=_q(d, "a")), A.sum("dgamma", A.mul(dz, xh), q=_q(d, "ai"))
        if p["act"] == "prelu":
            out["dalpha"] = A.sum("dalpha", a2, q=_q(d, "gi"))
    elif op == "apply":
        _v, s, _z, dz, xh, _a2 = _bn_back(A, p, d, d["dy"])
        inv = float(np.float32(1.0 / M_TOTAL))
        ex = d["ex"] if p.get("ex") else np.zeros(p["C"])
        out["ds"] = A.note("ds", _apply(A, s, dz, xh, A.mul(d["sdz"], inv), A.mul(d["sdzx"], inv), ex), _q(d, "giia") + 6)
    elif op == "bwd":                                                         # vnet_bn_act_bwd = reduce + apply, M_total = M = 2^k
        _v, s, _z, dz, xh, a2 = _bn_back(A, p, d, d["dy"])
        out["dbeta"], out["dgamma"] = A.sum("dbeta", dz, q=_q(d, "a")), A.sum("dgamma", A.mul(dz, xh), q=_q(d, "ai"))
        if p["act"] == "prelu":
            out["dalpha"] = A.sum("dalpha", a2, q=_q(d, "gi"))
        inv = float(np.float32(1.0 / M))
        assert inv * M == 1.0, "M_total = M must be a power of two for 1 / M to be dyadic"
        out["ds"] = A.note("ds", _apply(A, s, dz, xh, A.mul(out["dbeta"], inv), A.mul(out["dgamma"], inv), np.zeros(p["C"])),
                           _q(d, "giiaai") + 10)
    elif op == "act_bwd":                                                     # vnet_act_bwd: the identity batch-norm
        _v, _s, _z, dz, _xh, a2 = _bn_back(A, p, d, d["dy"])
        out["dx"] = A.note("dx", dz, _q(d, "a"))
        if p["act"] == "prelu":
            out["dalpha"] = A.sum("dalpha", a2)
    return out


def f_partial(A, p, d):
    """vnet_bn_finalize_partial on hand-made rows [rows][2][C] and vnet_bn_finalize on their float64 sums."""
    S, Q = A.sum("sum", d["part"][:, 0]), A.sum("sumsq", d["part"][:, 1])
    S, Q = np.asarray(S, np.float64), np.asarray(Q, np.float64)
    out = {"mean": _mean_ref(S, M_TOTAL), "mean2": _mean_ref(S, M_TOTAL)}
    out["invstd"], out["invstd~"] = _invstd_ref(S, Q, M_TOTAL)
    out["invstd2"], out["invstd2~"] = out["invstd"], out["invstd~"]
    return out


def _partial_operands(p, lv, rng):
    rows, C = p["M"], p["C"]
    part = np.empty((rows, 2, C))
    part[:, 0] = _ints(rng, 8, (rows, C))
    part[:, 1] = rng.integers(0, 65, size=(rows, C))
    part[0, 1] += 64.0 * rows                                                  # the variance stays positive: Q / M >= mu^2
    return {"part": part}


# ---- the small-tensor bf16 batch-norm (bn_small_fwd_b16_kernel / bn_small_bwd_b16_kernel) -------------------------------------------
def _small_operands(p, lv, rng):
    """s = x (+ r) in {0, +-1, +-2, +-4}, every column in +- pairs: the batch mean is exactly 0 and s * sc is an exact product, so the
    forward's y is a fixed sequence of single roundings of the kernel's OWN invstd (tier R); the backward takes dyadic statistics."""
    M, C = p["M"], p["C"]
    d = _bn_operands(p, max(lv, 1), rng)
    if p.get("shift"):
        # the second variant of the forward: every column is an integer c +- 1 in equal numbers (M even), so mean = c, var = 1 and,
        # with eps = 3, invstd = 1 / sqrt(4) = 1/2 exactly -- a non-zero mean whose use in sf = beta - mean * sc a wrong channel shows
        half = np.ones((M // 2, C))
        s = np.concatenate([half, -half]) + _ints(rng, 2, (1, C)) + (np.arange(C) % 2) * 3
    else:
        half = _pick(rng, (0, 1, 2, 4), (M // 2, C))
        s = np.concatenate([half, -half, np.zeros((M % 2, C))])
    s = np.take_along_axis(s, np.argsort(rng.random((M, C)), axis=0), axis=0)
    if p.get("res"):
        d["r"] = _ints(rng, 1, (M, C))
        d["x"] = s - d["r"]
    else:
        d["x"] = s
    return d


def small_eps(p):
    return 3.0 if p.get("shift") else EPS


def f_small_fwd(A, p, d, invstd=None):
    """mean R (exactly 0), invstd B; y restated in float32 from the invstd the kernel wrote (`invstd`; the host proof passes the
    rounded reference): sc = gamma * is, sf = beta - 0 * sc, z = s * sc + sf (s * sc exact: one rounding either way), act, bf16."""
    M = p["M"]
    v = _bn_core(A, dict(p, identity=1), d)[0]
    S, Q = A.sum("sum", v), A.sum("sumsq", A.mul(v, v))
    S, Q = np.asarray(S, np.float64), np.asarray(Q, np.float64)
    out = {"mean": _mean_ref(S, M)}
    out["invstd"], out["invstd~"] = _invstd_ref(S, Q, M, small_eps(p))
    F = Arith(f32=True, fused=A.fused)
    is32 = F.v(out["invstd"] if invstd is None else invstd)
    sc = F.mul(d["gamma"], is32)
    sf = F.fma(-F.v(out["mean"]), sc, d["beta"])
    y = _act_fwd_r(F, F.fma(v, sc, sf), p["act"], d["alpha"])
    out["y"] = O.round_bf16(y)
    return out


def _act_fwd_r(F, z, act, al):
    """act8_fwd: z > 0 ? z : neg * z, one rounding."""
    neg = {"none": 1.0, "relu": 0.0, "lrelu": float(np.float32(0.2))}.get(act)
    return np.where(z > 0, z, F.mul(al if neg is None else F.v(neg), z))


def f_small_bwd(A, p, d):
    """Sums E.  ds B: o = sc * (dz - S0 * invM - xh * S1 * invM) with invM = 1.f / (float)M, not dyadic.  Roundings: invM 1, k1 1,
    k2 1, xh * k2 1 (0 when contracted), two subtractions 2, sc * () 1 -> at most 8 units of 2^-24 of
    |sc| * (|dz| + |k1| + |xh * k2|) with the invM rounding counted in both k1 and k2, then the bf16 rounding of the stored value."""
    M = p["M"]
    _v, s, _z, dz, xh, a2 = _bn_back(A, p, d, d["dy"])
    out = {"dbeta": A.sum("dbeta", dz, q=_q(d, "a")), "dgamma": A.sum("dgamma", A.mul(dz, xh), q=_q(d, "ai"))}
    if p["act"] == "prelu":
        out["dalpha"] = A.sum("dalpha", a2, q=_q(d, "gi"))
    s64, dz64, xh64 = (np.asarray(t, np.float64) for t in (s, dz, xh))
    k1, k2 = np.asarray(out["dbeta"], np.float64) / M, np.asarray(out["dgamma"], np.float64) / M
    ref = s64 * (dz64 - k1 - xh64 * k2)
    e = 8 * U24 * np.abs(s64) * (np.abs(dz64) + np.abs(k1) + np.abs(xh64 * k2))
    out["ds"], out["ds~"] = ref, 2.0 ** -8 * (np.abs(ref) + e) + e
    return out


# ---- the fused batch-norm + head passes ---------------------------------------------------------------------------------------------
def _head_rows(M, C):
    """Workgroup of every voxel in bn_act_head_fwd_kernel: lane cq == 0 of voxel v is thread v * CQ of the grid-stride walk."""
    CQ = C // 4
    rows = min(MAXBLK, max(1, cdiv(M * C // 4 // 4 + 1, BLOCK)))
    return rows, (np.arange(M) * CQ // BLOCK) % rows


def f_bn_head(A, p, d):
    op, M, C, K = p["op"], p["M"], p["C"], p["K"]
    out = {}
    if op == "fwd":
        y = _act_fwd(A, _bn_core(A, p, d)[2], p["act"], d["alpha"])
        qy = _q(d, "gia")
        out["y"] = A.note("y", y, qy)
        lg = A.add(A.sum("logits", A.mul(y[:, :, None], d["w"][None]), axis=1, q=qy), d["bias"])
        out["logits"] = lg
        rows, blk = _head_rows(M, C)
        st = np.zeros((rows, 2 * K), A.dt)
        if not A.f32:                                                           # (the oracle, vectorised: float64 sums of these terms are exact)
            for k in range(K):
                st[:, k] = np.bincount(blk, weights=lg[:, k], minlength=rows)
                st[:, K + k] = np.bincount(blk, weights=lg[:, k] ** 2, minlength=rows)
            A.mag["statsq"] = st[:, K:].max() * 2.0 ** (2 * qy)
            A.mag["stats"] = max(np.bincount(blk, weights=np.abs(lg[:, k]), minlength=rows).max() for k in range(K)) * 2.0 ** qy
            out["stats"] = st
            return out
        for b in range(rows):
            sel = lg[blk == b]
            st[b, :K], st[b, K:] = A.sum("stats%d" % b, sel, q=qy), A.sum("statsq%d" % b, A.mul(sel, sel), q=2 * qy)
        out["stats"] = st
        return out
    dy = A.sum("dy", A.mul(d["dl"][:, None, :], d["w"][None]), axis=2)        # dy[c] = sum_k W[c][k] dlogits[k]
    v, s, z, dz, xh, a2 = _bn_back(A, p, d, dy)
    if op == "reduce":
        out["dbeta"], out["dgamma"] = A.sum("dbeta", dz, q=_q(d, "a")), A.sum("dgamma", A.mul(dz, xh), q=_q(d, "ai"))
        if p["act"] == "prelu":
            out["dalpha"] = A.sum("dalpha", a2, q=_q(d, "gi"))
        y = _act_fwd(A, z, p["act"], d["alpha"])
        out["dw"] = A.sum("dw", A.mul(y[:, :, None], d["dl"][:, None, :]), q=_q(d, "gia"))
        out["db"] = A.sum("db", d["dl"])
    else:
        inv = float(np.float32(1.0 / M_TOTAL))
        ex = d["ex"] if p.get("ex") else np.zeros(C)
        out["ds"] = A.note("ds", _apply(A, s, dz, xh, A.mul(d["sdz"], inv), A.mul(d["sdzx"], inv), ex), _q(d, "giia") + 6)
    return out


# ---- the 1x1x1 head, column sums ----------------------------------------------------------------------------------------------------
def _head_operands(p, lv, rng):
    M, C, K = p["M"], p["C"], p["K"]
    R = (3, 2, 1)[lv]
    return {"x": _ints(rng, R, (M, C)), "w": _ints(rng, R, (C, K)), "bias": _ints(rng, 3, K), "dy": _ints(rng, R, (M, K))}


def f_head(A, p, d):
    if p["op"] == "fwd":
        return {"y": A.add(A.sum("y", A.mul(d["x"][:, :, None], d["w"][None]), axis=1), d["bias"])}
    return {"dx": A.sum("dx", A.mul(d["dy"][:, None, :], d["w"][None]), axis=2),
            "dw": A.sum("dw", A.mul(d["x"][:, :, None], d["dy"][:, None, :])), "db": A.sum("db", d["dy"])}


def f_colsum(A, p, d):
    return {"out": A.sum("out", d["x"])}


# ---- the loss head ------------------------------------------------------------------------------------------------------------------
LOSS_KINDS = (0, 1, 2, 0 | 16, 1 | 16 | 32, 0 | 32, 1 | 32, 2 | 16)           # VNET_LOSS_* | flags, rotated over the cases


def _loss_operands(p, lv, rng):
    """Voxel kinds that make the softmax exact: an m-way tie, m in {1, 2, 4, 8}, m <= K -- the m largest logits equal, every other
    logit at least 128 below (expf of it is 0 with or without denormals), so p = 1 / m on the tie and 0 elsewhere; m = 1 is the
    saturated voxel.  Labels inside and outside [0, K); class K - 1 is absent from the patch where K > 2."""
    B, V, K = p["B"], p["M"], p["K"]
    ms = [m for m in (1, 2, 4, 8)[:4 - lv] if m <= K]                         # (level 1: ties of at most 4, level 2: of at most 2)
    m = np.asarray(ms)[rng.integers(0, len(ms), size=(B, V))]
    rank = np.argsort(rng.random((B, V, K)), axis=-1)                          # a random permutation of the classes per voxel
    top = rng.integers(-3, 4, size=(B, V, 1)).astype(np.float64)
    z = np.where(rank < m[..., None], top, top - 128.0 - rng.integers(0, 5, size=(B, V, K)))
    hi = K - 1 if K > 2 else K
    lab = rng.integers(0, hi, size=(B, V)).astype(np.int32)
    lab[:, ::7] = -1
    lab[:, 3::11] = K
    d = {"z": z, "lab": lab, "w": _pick(rng, (0.25, 0.5, 1.0), K), "m": m,
         "coef": np.concatenate([_pick(rng, (-0.5, -0.25, -0.125, 0.125, 0.25, 0.375), 2 * B * K), _pick(rng, (0.125, 0.25), 1)]),
         "gs": _pick(rng, (0.5, 2.0), 1)}
    return d


def _softmax(d):
    z = d["z"]
    mx = z.max(-1, keepdims=True)
    return (z == mx) / d["m"][..., None].astype(np.float64), np.argmax(z, -1)           # (argmax: the first of equal maxima)


def f_loss(A, p, d):
    B, V, K, kind = p["B"], p["M"], p["K"], p["kind"]
    jac, wx, mixed, base = (kind & 15) == 1, bool(kind & 16), bool(kind & 32), kind & 15
    pk, pred = _softmax(d)
    lab = d["lab"]
    t = (lab[..., None] == np.arange(K)).astype(np.float64)
    if p["op"] == "bwd":
        gs = d["gs"][0]
        gI, gL = (A.mul(d["coef"][:2 * B * K].reshape(B, 1, K, 2)[..., j], gs) for j in (0, 1))
        xc = A.mul(d["coef"][2 * B * K], gs)
        pv, tv = A.v(pk), A.v(t)
        g = A.fma(gI, tv, A.mul(gL, A.mul(2.0, pv) if jac else A.v(np.ones_like(pk))))
        dot = A.sum("dot", A.mul(g, pv), axis=-1, q=9)[..., None]               # (coef 3 + gscale 1 + 2p 2 bits, times p 3)
        has = (lab >= 0) & (lab < K)
        wv = np.where(has, d["w"][np.clip(lab, 0, K - 1)] if wx else 1.0, 0.0)[..., None]
        return {"dlogits": A.note("dlogits", A.fma(A.mul(xc, wv), A.sub(pv, tv), A.mul(pv, A.sub(g, dot))), 16)}
    out = {"softmax": pk, "pred": pred.astype(np.float64)}
    qp = 3 - d.get("level", 0)                                                  # (p = 1 / m, m <= 8, 4, 2 by level: 3, 2, 1 bits; twice squared)
    I = A.sum("I", (pk * t).reshape(B, V, K), axis=1, q=qp)
    L_ = A.sum("L", (pk * pk if jac else pk), axis=1, q=2 * qp if jac else qp)
    R_ = A.sum("R", t, axis=1)
    out.update(_I=I, _L=L_, _R=R_)
    if A.f32:
        return out
    # the xent sum, tier B.  A term is w * (logf(se) - (z[lab] - mx)): logf 2 units (1 ulp), the subtraction 1, the weight 1; the sum
    # is taken over `per_thread` voxels of a thread, 6 wave steps, 3 additions of the wave totals and one float64 -> float32 cast
    has = (lab >= 0) & (lab < K)
    zl = np.take_along_axis(d["z"], np.clip(lab, 0, K - 1)[..., None], -1)[..., 0]
    term = np.where(has, (d["w"][np.clip(lab, 0, K - 1)] if wx else 1.0) * (np.log(d["m"]) - (zl - d["z"].max(-1))), 0.0)
    xsum, xabs = term.sum(), np.abs(term).sum()
    per_thread = cdiv(V, geom_of(p).grid * BLOCK)
    xtol = (4 + per_thread + 6 + 3 + 1) * U24 * xabs
    smooth = float(np.float32(1e-5))
    I, L_, R_ = (np.asarray(a, np.float64) for a in (I, L_, R_))
    coef = np.zeros(2 * B * K + 1)
    dice, xc = 0.0, 0.0
    xent = xsum / (float(V) * B)
    if base == 2:
        loss, xc = xent, 1.0 / (float(V) * B)
        ltol = xtol / (float(V) * B)
    else:
        if wx:
            for b in range(B):
                num = (2.0 * d["w"] * I[b] + smooth).sum()
                den = (d["w"] * (L_[b] + R_[b]) + smooth).sum()
                dice += num / den / B
                coef[2 * b * K:2 * (b + 1) * K:2] = -2.0 * d["w"] / den / B
                coef[2 * b * K + 1:2 * (b + 1) * K:2] = num / (den * den) * d["w"] / B
        else:
            den, num = L_ + R_ + smooth, 2.0 * I + smooth
            dice = (num / den / (B * K)).sum()
            coef[0:2 * B * K:2] = (-2.0 / den / (B * K)).reshape(-1)
            coef[1:2 * B * K:2] = (num / (den * den) / (B * K)).reshape(-1)
        loss, ltol = 1.0 - dice, 0.0
        if mixed:
            al = float(np.float32(0.5))
            loss += al * xent
            xc = al / (float(V) * B)
            ltol = al * xtol / (float(V) * B)
    coef[2 * B * K] = xc
    # loss, dice, coef: float64 expressions of exact sums cast to float32 once: k = 2 (the cast and a unit of slack for the float64
    # steps, whose cancellation in 1 - dice is bounded by 2^-52 / 2^-24 of a unit), plus the xent sum's own bound
    out.update(loss=np.asarray([loss]), dice=np.asarray([dice]), coef=coef)
    out["loss~"] = np.asarray([2 * U24 * max(abs(loss), 1.0) + ltol])
    out["dice~"] = np.asarray([2 * U24 * max(abs(dice), 1.0)])
    out["coef~"] = 2 * U24 * np.abs(coef)
    return out


def _dice_operands(p, lv, rng):
    B, V, K = p["B"], p["M"], p["K"]
    t = (rng.integers(-1, K + 1, size=(B, V, 1)) == np.arange(K)).astype(np.float64)        # one-hot, some rows all zero
    den = (8.0, 2.0)[lv]                                                       # (probabilities in eighths; level 1: in halves)
    return {"p": rng.integers(0, int(den) + 1, size=(B, V, K)) / den, "t": t, "w": _pick(rng, (0.25, 0.5, 1.0), K),
            "coef": np.concatenate([_pick(rng, (-0.5, -0.25, 0.125, 0.25, 0.375), 2 * B * K), np.zeros(1)]),
            "gs": _pick(rng, (0.5, 2.0), 1)}


def f_dice(A, p, d):
    B, V, K, jac, wx = p["B"], p["M"], p["K"], p["jac"], p["wx"]
    if p["op"] == "bwd":                                                      # -gs * (gI * t + gL * (jac ? 2 p : 1))
        c = d["coef"][:2 * B * K].reshape(B, 1, K, 2)
        inner = A.fma(c[..., 0], d["t"], A.mul(c[..., 1], A.mul(2.0, d["p"]) if jac else A.v(np.ones_like(d["p"]))))
        return {"dout": A.note("dout", A.mul(-d["gs"][0], inner), 8)}
    qp = (3, 1)[d.get("level", 0)]
    I = np.asarray(A.sum("I", A.mul(d["p"], d["t"]), axis=1, q=qp), np.float64)
    L_ = np.asarray(A.sum("L", A.mul(d["p"], d["p"]) if jac else d["p"], axis=1, q=2 * qp if jac else qp), np.float64)
    R_ = np.asarray(A.sum("R", d["t"], axis=1), np.float64)                     # (t * t == t for a one-hot target)
    if A.f32:
        return {"_I": I, "_L": L_, "_R": R_}
    smooth = float(np.float32(1e-5))
    coef = np.zeros(2 * B * K + 1)
    if wx:
        dice = 0.0
        for b in range(B):
            num, den = (2.0 * d["w"] * I[b] + smooth).sum(), (d["w"] * (L_[b] + R_[b]) + smooth).sum()
            dice += num / den / B
            coef[2 * b * K:2 * (b + 1) * K:2] = -2.0 * d["w"] / den / B
            coef[2 * b * K + 1:2 * (b + 1) * K:2] = num / (den * den) * d["w"] / B
    else:
        den, num = L_ + R_ + smooth, 2.0 * I + smooth
        dice = (num / den / (B * K)).sum()
        coef[0:2 * B * K:2] = (-2.0 / den / (B * K)).reshape(-1)
        coef[1:2 * B * K:2] = (num / (den * den) / (B * K)).reshape(-1)
    # k = 2, as for the loss head
    return {"_I": I, "_L": L_, "_R": R_, "dice": np.asarray([dice]), "dice~": np.asarray([2 * U24 * max(abs(dice), 1.0)]), "coef": coef, "coef~": 2 * U24 * np.abs(coef)}


# ---- dropout --------------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
STEP_MUL = 0xD1342543DE82EF95


def mix32(x):
    """elementwise.hip: mix32 on uint64 arrays."""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xff51afd7ed558ccd)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xc4ceb9fe1a85ec53)
        x = x ^ (x >> np.uint64(33))
    return (x & np.uint64(0xffffffff)).astype(np.uint32)


def dropout_mask(seed, n, rate, step=None):
    """keep[i] = (mix32(seed * 0x9E3779B97F4A7C15 + i) >> 8) * 2^-24 >= rate, the seed advanced by step * STEP_MUL with a step state."""
    if step is not None:
        seed = (seed + step * STEP_MUL) & M64
    base = (seed * 0x9E3779B97F4A7C15) & M64
    with np.errstate(over="ignore"):
        h = mix32(np.uint64(base) + np.arange(n, dtype=np.uint64))
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(rate)


def f_dropout(A, p, d):
    n, rate = p["M"] * (8 if p.get("b16") else 1), p["rate"]
    keep = dropout_mask(d["seed"], n, rate, d.get("step"))
    sc = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))         # 1.f / (1.f - rate): 2 or 4
    return {"mask": keep.astype(np.float64), "y": A.note("y", np.where(keep, A.mul(d["x"], sc), A.v(0))),
            "dx": A.note("dx", np.where(keep, A.mul(d["dy"], sc), A.v(0)))}


def _dropout_operands(p, lv, rng):
    n = p["M"] * (8 if p.get("b16") else 1)
    d = {"x": _ints(rng, 3, n), "dy": _ints(rng, 3, n), "seed": int(rng.integers(1, 1 << 62))}
    if p.get("dev"):
        d["step"] = int(rng.integers(1, 1000))
    return d


# ---- optimisers -----------------------------------------------------------------------------------------------------------------------
def _opt_operands(p, lv, rng):
    n = p["M"]
    return {"p": _ints(rng, 8, n) / 4.0, "g": _ints(rng, 4, n), "m": _ints(rng, 4, n) / 2.0, "v": rng.integers(0, 9, size=n) / 4.0,
            "acc": _ints(rng, 4, n) / 2.0}


OPT = dict(lr=0.125, gs=0.5, mom=0.5, b1=0.5, b2=0.75, eps=2.0 ** -10, lr_t=0.25)


def f_opt(A, p, d):
    """sgd / momentum: E (lr, momentum, gscale dyadic).  adam: m, v E (1 - beta = 1/2, 1/4); p R: lr_t * m exact, sqrtf, + eps, the
    division and the subtraction each rounded once and none of them a multiplication feeding an addition."""
    k, o = p["kind"], OPT
    gi = A.mul(d["g"], o["gs"])
    if k == "sgd":                                                            # p -= lr * gs * g
        return {"p": A.note("p", A.sub(d["p"], A.mul(A.mul(o["lr"], o["gs"]), d["g"])), 4)}
    if k in ("momentum", "nesterov"):
        a = A.fma(d["acc"], o["mom"], gi)
        step = A.mul(o["lr"], A.fma(o["mom"], a, gi)) if k == "nesterov" else A.mul(o["lr"], a)
        return {"acc": A.note("acc", a, 2), "p": A.note("p", A.sub(d["p"], step), 6)}
    mi = A.fma(A.sub(gi, d["m"]), 1.0 - o["b1"], d["m"])
    vi = A.fma(A.sub(A.mul(gi, gi), d["v"]), 1.0 - o["b2"], d["v"])
    F = Arith(f32=True)
    m32, v32 = F.v(mi), F.v(vi)
    pn = F.sub(d["p"], F.div(F.mul(o["lr_t"], m32), F.add(np.sqrt(v32), o["eps"])))
    return {"m": A.note("m", mi, 2), "v": A.note("v", vi, 4), "p": np.asarray(pn, np.float64)}


# ---- the rest -------------------------------------------------------------------------------------------------------------------------
def f_cast(A, p, d):
    M, C, Cpad = p["M"], p["C"], p["Cpad"]
    y = np.zeros((M, Cpad))
    y[:, :C] = O.round_bf16(d["x"])                                            # tier R: the bf16 cast
    return {"y": y}


def f_patch(A, p, d):
    pz, py, px = p["M"], p["py"], p["px"]
    D, H, W, z0, y0, x0 = (p[k] for k in ("D", "H", "W", "z0", "y0", "x0"))
    vol, cnt = A.v(d["vol"]).copy(), A.v(d["cnt"]).copy()
    ez, ey, ex = max(0, min(pz, D - z0)), max(0, min(py, H - y0)), max(0, min(px, W - x0))
    vol[z0:z0 + ez, y0:y0 + ey, x0:x0 + ex] += A.v(d["patch"])[:ez, :ey, :ex]
    cnt[z0:z0 + ez, y0:y0 + ey, x0:x0 + ex] += 1
    return {"vol": A.note("vol", vol), "cnt": cnt}


def _patch_operands(p, lv, rng):
    pz, py, px, K = p["M"], p["py"], p["px"], p["K"]
    return {"patch": _ints(rng, 50, (pz, py, px, K)), "vol": _ints(rng, 9, (p["D"], p["H"], p["W"], K)),
            "cnt": rng.integers(0, 4, size=(p["D"], p["H"], p["W"])).astype(np.float64)}


# ---- the table --------------------------------------------------------------------------------------------------------------------
class Row(object):
    def __init__(self, name, family, entries, geom, tiers, fixed=None, rot=None, absent=None, clamped=False, nocap=None,
                 accept=None, kernel="", sizes=None, prior=None):
        self.name, self.family, self.entries, self.geom, self.tiers = name, family, tuple(entries), geom, tiers
        self.fixed, self.rot = dict(fixed or {}), collections.OrderedDict(rot or {})
        self.absent = {k: tuple(v[0]) for k, v in (absent or {}).items()}
        self.absent_why = {k: v[1] for k, v in (absent or {}).items()}
        self.clamped, self.nocap, self.accept, self.kernel = clamped, nocap, accept or (lambda p: True), kernel
        self.sizes = sizes                    # a row that is not swept: exactly these extents, one per rotation step
        # (geometry, absent) the row had when its extents were first chosen, for a kernel whose loop structure changed since: the
        # cases generated against it stay (an extent is a case whatever it was chosen for), and the generator adds what the
        # classes of the present geometry still miss
        self.prior = prior

    def needed(self):
        """The (axis, class) pairs the row's cases must realise."""
        if self.sizes:
            return set()
        g = self.geom(params_of(self, 0, 5))
        axes = ["block", "grid"] + (["group"] if g.U > 1 else []) + (["vec"] if g.vec else [])
        out = set((a, c) for a in axes for c in CLASSES if c not in self.absent.get(a, ()))
        if self.clamped:
            out.add(("slot", "out"))
        return out

    def params(self, i, size):
        p = dict(self.fixed)
        for j, (k, vals) in enumerate(self.rot.items()):
            p[k] = vals[(i + j) % len(vals)]
        p["M"] = size
        return p


FAMILIES = {
    # family: (operand generator, levels, formula)
    "bn": (_bn_operands, len(BN_LEVELS), f_bn), "partial": (_partial_operands, 1, f_partial),
    "small_fwd": (_small_operands, 1, f_small_fwd), "small_bwd": (_small_operands, len(BN_LEVELS), f_small_bwd),
    "bn_head": (_bn_operands, len(BN_LEVELS), f_bn_head),
    "head": (_head_operands, 3, f_head), "colsum": (lambda p, lv, rng: {"x": _ints(rng, (3, 2, 1)[lv], (p["M"], p["C"]))}, 3, f_colsum),
    "loss": (_loss_operands, 3, f_loss), "dice": (_dice_operands, 2, f_dice), "dropout": (_dropout_operands, 1, f_dropout),
    "opt": (_opt_operands, 1, f_opt),
    "cast": (lambda p, lv, rng: {"x": (rng.standard_normal((p["M"], p["C"])) * 30.0).astype(np.float32).astype(np.float64)}, 1, f_cast),
    "patch": (_patch_operands, 1, f_patch),
}

E3 = {"dbeta": "E", "dgamma": "E", "dalpha": "E"}
ONE_THREAD = ("one work item per thread: the grid grows with the data, so below the cap the data ends inside the first slot "
              "(the capped case of the row has the later trips)")

def _stats_geom(p):
    M, Cs = p["M"], 1 if p.get("bcast") else p["C"]
    mode = _red_mode(Cs)
    if mode == 0:
        return G(M * (Cs // 4), M * (Cs // 4))
    if mode == 1:
        return G(M, M)
    return G(M * Cs, M, per_block=1 if Cs > BLOCK else BLOCK // Cs)


def _ew_geom(p):
    M, C = p["M"], p["C"]
    vec = C % 4 == 0
    return G(M * C // 4 // (4 if vec else 1) + 1, M * C // 4 if vec else M * C)


def _red_geom(p):
    M, C = p["M"], p["C"]
    mode = _red_mode(C)
    if mode == 0:
        return G(M * C // 16 + 1, M * C // 4, U=RED_U)
    return G(M, M) if mode == 1 else _rowgroup_geom(M, C)


def _rowgroup_geom(M, C):
    """The fixed-order generic kernels (bn_act_bwd_reduce_kernel<2>, colsum_generic_kernel, head_bwd_generic_kernel): the grid is
    sized for a quarter of the elements (+ 1), the loop walks rows, a block takes 256 / C row groups a trip (one row where C > 256)."""
    return G(M * C // 4 + 1, M, per_block=1 if C > BLOCK else BLOCK // C)


def _b16_geom(p):
    n8 = p["M"] * (p["C"] // 8)
    return G(n8 // 2 + 1, n8, U=2)


def _cs16_geom(p):
    RB = CS16_BLOCK // (p["C"] // 8)
    return G(None, p["M"], per_block=RB, grid=min(CS16_MAXBLK, cdiv(p["M"], RB)), cap=CS16_MAXBLK)


def _table():
    rows = []
    add = lambda *a, **k: rows.append(Row(*a, **k))
    acts3, acts4 = ("prelu", "none", "relu"), ("prelu", "lrelu", "none", "relu")
    grid1 = {"grid": (("r1", "rm1", "mult"), ONE_THREAD)}
    # ---- batch-norm, float32 ----
    mom_t = {"sums": "E", "mean": "R", "invstd": "B"}
    mom_e = ("vnet_bn_moments", "vnet_bn_stats", "vnet_bn_ws_bytes")
    add("bn-moments-vec", "bn", mom_e, _stats_geom, mom_t, dict(op="moments"), dict(C=(4, 8, 64, 256), res=(0, 1)), grid1,
        kernel="bn_stats_vec_kernel")
    add("bn-moments-row", "bn", mom_e, _stats_geom, mom_t, dict(op="moments"), dict(C=(1, 3, 7), res=(1, 0)), grid1,
        accept=lambda p: _red_mode(p["C"]) == 1, kernel="bn_stats_row_kernel (C = 8 is two quads: red_mode() sends it to the vector kernel)")
    add("bn-moments-bcast", "bn", mom_e, _stats_geom, mom_t, dict(op="moments", bcast=1, res=0), dict(C=(16, 5, 12)), grid1,
        kernel="bn_stats_row_kernel, Cs = 1")
    add("bn-moments-generic", "bn", mom_e, _stats_geom, mom_t, dict(op="moments"), dict(C=(12, 37, 255), res=(0, 1)),
        {"grid": (("rm1", "mult"), "the grid is sized for one thread per element: the rows overflow the first slot only by the threads a "
                  "block wastes (256 % C), never by a whole slot")}, kernel="bn_stats_generic_kernel, C <= 256")
    add("bn-moments-wide", "bn", mom_e, _stats_geom, mom_t, dict(op="moments"), dict(C=(257, 300), res=(1, 0)),
        {"grid": (("eq", "r1", "rm1", "mult"), "one row per block and M * C / 256 > M blocks: every row has its own block below the cap"),
         "block": (("lt", "r1", "rm1"), "a block's slot is one row: every extent is a whole number of them")}, kernel="bn_stats_generic_kernel, C > 256")
    for vec, Cs in ((1, (4, 8, 64, 12 * 4)), (0, (1, 3, 37, 6))):
        tag = "vec" if vec else "scalar"
        fwd_t = {"y": "E (lrelu: R, 0.2f * z)"}
        add("bn-fwd-" + tag, "bn", ("vnet_bn_act_fwd",), _ew_geom, fwd_t, dict(op="fwd"), dict(C=Cs, act=acts4, res=(0, 1, 0), bcast=(0, 0, 1, 0, 0)),
            accept=lambda p: not (p["bcast"] and p["res"]), kernel="bn_act_fwd_kernel<%s>" % ("true" if vec else "false"))
        add("bn-apply-" + tag, "bn", ("vnet_bn_act_bwd_apply",), _ew_geom, {"ds": "E"}, dict(op="apply"),
            dict(C=Cs, act=acts3, res=(1, 0), ex=(0, 1, 1), bcast=(0, 0, 0, 1, 0)), accept=lambda p: not (p["bcast"] and p["res"]),
            kernel="bn_act_bwd_apply_kernel<%s>" % ("true" if vec else "false"))
        add("act-fwd-" + tag, "bn", ("vnet_act_fwd",), _ew_geom, fwd_t, dict(op="fwd", identity=1, res=0), dict(C=Cs, act=acts4),
            kernel="bn_act_fwd_kernel<%s>, identity" % ("true" if vec else "false"))
        add("act-bwd-" + tag, "bn", ("vnet_act_bwd",), _ew_geom, {"dx": "E", "dalpha": "E"}, dict(op="act_bwd", identity=1, res=0),
            dict(C=Cs, act=acts3), kernel="bn_act_bwd_apply_kernel<%s> (+ the reduce kernel of the width's mode for dalpha), identity"
            % ("true" if vec else "false"))
    red = dict(op="reduce")
    nores = lambda p: not (p["bcast"] and p["res"])
    add("bn-reduce-m0", "bn", ("vnet_bn_act_bwd_reduce",), _red_geom, E3, red, dict(C=(4, 8, 64, 256), act=acts3, res=(0, 1), bcast=(0, 0, 0, 1, 0)),
        {"group": (("mult",), "the grid is sized for a quarter of the quads (+ 1): two groups of two slots never end exactly on the data")},
        clamped=True, accept=nores, kernel="bn_act_bwd_reduce_kernel<0>")
    add("bn-reduce-m1", "bn", ("vnet_bn_act_bwd_reduce",), _red_geom, E3, red, dict(C=(1, 3, 7), act=acts3, res=(1, 0), bcast=(0, 0, 0, 0, 1)), grid1,
        accept=lambda p: nores(p) and _red_mode(p["C"]) == 1, kernel="bn_act_bwd_reduce_kernel<1>")
    add("bn-reduce-m2", "bn", ("vnet_bn_act_bwd_reduce",), _red_geom, E3, red, dict(C=(12, 37, 255, 300, 13), act=acts3, res=(0, 1), bcast=(0, 0, 0, 0, 1)),
        accept=nores, kernel="bn_act_bwd_reduce_kernel<2>: row groups in a fixed order (C <= 256), a row per block (C = 300)",
        prior=(lambda p: G(p["M"] * p["C"] // 4 + 1, p["M"] * p["C"]), {"block": (("eq",), "one thread per element: M * C == 256 only for "
               "a power-of-two width"), "grid": (("eq", "r1"), "likewise")}))
    add("bn-bwd-composite", "bn", ("vnet_bn_act_bwd",), _red_geom, dict(E3, ds="E"), dict(op="bwd"),
        dict(C=(16, 3, 12), act=acts3, res=(0, 1)), sizes=(64, 256, 1024, 256),
        nocap="not a sweep: the composition reduce -> apply (the sums it wrote, M_total = M), exact only where M is a power of two; "
              "both halves have rows of their own", kernel="bn_act_bwd_reduce_kernel<mode> + sum_finalize_kernel + bn_act_bwd_apply_kernel<VEC>")
    add("bn-finalize-partial", "partial", ("vnet_bn_finalize_partial", "vnet_bn_finalize"), lambda p: G(None, p["M"], grid=1),
        {"mean": "R", "invstd": "B", "mean2": "R", "invstd2": "B"}, {}, dict(C=(1, 5, 16)),
        nocap="one workgroup per channel walks the partial rows: there is no grid cap, and at most 1024 rows exist",
        kernel="bn_finalize_kernel / bn_finalize_sums_kernel")
    # ---- batch-norm, bf16 ----
    C16 = (8, 16, 64, 256)
    g16m = {"group": (("eq", "r1", "rm1", "mult"), "the grid is sized for half of the 16-byte units (+ 1): one group of two slots holds "
                      "them all below the cap"), "grid": (("mult",), "likewise: at most two slots")}
    add("bn16-stats", "bn", ("vnet_bn_moments_b16", "vnet_bn_stats_b16"), _b16_geom, mom_t, dict(op="moments", b16=1), dict(C=C16, res=(0, 1)),
        g16m, clamped=True, kernel="bn_stats_b16_kernel<HASR>")
    for bc, rs in ((0, 0), (0, 1), (1, 0)):
        tag = "-b%dr%d" % (bc, rs)
        fx = dict(b16=1, bcast=bc, res=rs)
        add("bn16-fwd" + tag, "bn", ("vnet_bn_act_fwd_b16",), _b16_geom, {"y": "E -> bf16 (lrelu: R)"}, dict(fx, op="fwd"), dict(C=C16, act=acts4),
            g16m, clamped=True, kernel="bn_act_fwd_b16_kernel<%d, %d>" % (bc, rs))
        add("bn16-reduce" + tag, "bn", ("vnet_bn_act_bwd_reduce_b16",), _b16_geom, E3, dict(fx, op="reduce"), dict(C=C16, act=acts3),
            g16m, clamped=True, kernel="bn_act_bwd_reduce_b16_kernel<%d, %d>" % (bc, rs))
        add("bn16-apply" + tag, "bn", ("vnet_bn_act_bwd_apply_b16",), _b16_geom, {"ds": "E -> bf16"}, dict(fx, op="apply"),
            dict(C=C16, act=acts3, ex=(1, 0)), g16m, clamped=True, kernel="bn_act_bwd_apply_b16_kernel<%d, %d>" % (bc, rs))
    small_no = "one workgroup per channel octet walks all M <= 8192 rows: no grid cap"
    for rs in (0, 1):
        add("bn16-small-fwd-r%d" % rs, "small_fwd", ("vnet_bn_small_fwd_b16", "vnet_bn_small_ok"), lambda p: G(None, p["M"], U=4, grid=1),
            {"mean": "R", "invstd": "B", "y": "R from the kernel's own invstd -> bf16"}, dict(b16=1, res=rs, op="small"), dict(C=(8, 24, 16), act=acts4, shift=(0, 1)),
            clamped=True, nocap=small_no, accept=lambda p: p["M"] <= 8192 and not (p["shift"] and p["M"] % 2),
            kernel="bn_small_fwd_b16_kernel<%d> (shift = 1: columns c +- 1, eps = 3: mean = c, invstd = 1/2 exactly)" % rs)
        add("bn16-small-bwd-r%d" % rs, "small_bwd", ("vnet_bn_small_bwd_b16",), lambda p: G(None, p["M"], U=2, grid=1),
            dict(E3, ds="B (1 / M is not dyadic) -> bf16"), dict(b16=1, res=rs, op="small"), dict(C=(8, 24, 16), act=acts3),
            clamped=True, nocap=small_no, accept=lambda p: p["M"] <= 8192, kernel="bn_small_bwd_b16_kernel<%d>" % rs)
    # ---- the fused head ----
    hk = dict(C=(8, 16), K=tuple(range(1, 9)), act=acts3, res=(0, 1))
    hgeom = lambda p: G(p["M"] * p["C"] // 16 + 1, p["M"] * (p["C"] // 4))
    add("bn-head-fwd", "bn_head", ("vnet_bn_act_head_fwd", "vnet_bn_head_ok", "vnet_bn_head_stats_rows"), hgeom,
        {"y": "E", "logits": "E", "stats": "E"}, dict(op="fwd"), hk,
        {"block": (("r1", "rm1"), "the items are M * CQ quads, CQ = 2 or 4: never one more or less than a multiple of 256"),
         "grid": (("r1", "rm1"), "likewise against the grid's slot")}, kernel="bn_act_head_fwd_kernel<K, CQ>")
    add("bn-head-reduce", "bn_head", ("vnet_bn_act_bwd_reduce_head", "vnet_bn_head_ws_bytes"),
        lambda p: G(p["M"] * p["C"] // 16 + 1, p["M"] * (p["C"] // 4), U=RED_U),
        dict(E3, dw="E", db="E"), dict(op="reduce"), hk,
        {"block": (("r1", "rm1"), "M * CQ quads, CQ = 2 or 4"), "grid": (("r1", "rm1"), "likewise"), "group": (("r1", "rm1", "mult"), "likewise; mult as for bn-reduce-m0")},
        clamped=True, kernel="bn_act_bwd_reduce_head_kernel<K, CQ>")
    add("bn-head-apply", "bn_head", ("vnet_bn_act_bwd_apply_head",), hgeom, {"ds": "E"}, dict(op="apply"), dict(hk, ex=(1, 0, 1)),
        {"block": (("r1", "rm1"), "M * CQ quads, CQ = 2 or 4"), "grid": (("r1", "rm1"), "likewise")}, kernel="bn_act_bwd_apply_head_kernel<K, CQ>")
    # ---- the head ----
    Ks = tuple(range(1, 9))
    hb = {"dx": "E", "dw": "E", "db": "E"}
    add("head-fwd", "head", ("vnet_head_fwd",), lambda p: G(p["M"] // 2 + 1, p["M"]), {"y": "E"}, dict(op="fwd"), dict(K=Ks, C=(16, 5, 4, 12)),
        {"grid": (("mult",), "the launcher asks for half of the rows + 1: two slots always hold them with room to spare")},
        kernel="head_fwd_kernel<K>, both channel loops")
    add("head-bwd-vec", "head", ("vnet_head_bwd", "vnet_head_ws_bytes"), lambda p: G(p["M"] * (p["C"] // 4) // 4 + 1, p["M"] * (p["C"] // 4)), hb,
        dict(op="bwd"), dict(K=Ks, C=(16, 4, 8)), kernel="head_bwd_kernel<K>")
    add("head-bwd-generic", "head", ("vnet_head_bwd",), lambda p: _rowgroup_geom(p["M"], p["C"]), hb, dict(op="bwd"), dict(K=Ks, C=(5, 12)),
        kernel="head_bwd_generic_kernel<K>", prior=(lambda p: G(p["M"] // 4 + 1, p["M"]), None))
    add("head16-fwd", "head", ("vnet_head_fwd_b16",), lambda p: G(p["M"] // 2 + 1, p["M"]), {"y": "E"}, dict(op="fwd", b16=1), dict(K=Ks, C=(16, 8, 24)),
        {"grid": (("mult",), "half of the rows + 1, as head-fwd")}, kernel="head_fwd_b16_kernel<K>")
    add("head16-bwd", "head", ("vnet_head_bwd_b16",), _b16_geom, dict(hb, dx="E -> bf16"), dict(op="bwd", b16=1), dict(K=Ks, C=(16, 8, 64, 32)),
        g16m, clamped=True, kernel="head_bwd_b16_kernel<K>: the DPP branch (C <= 32) and the LDS tree (C = 64)")
    # ---- column sums ----
    add("colsum-vec", "colsum", ("vnet_colsum", "vnet_colsum_ws_bytes"), lambda p: G(p["M"] * (p["C"] // 4) // 4 + 1, p["M"] * (p["C"] // 4)),
        {"out": "E"}, {}, dict(C=(4, 8, 64, 256)), kernel="colsum_vec_kernel")
    add("colsum-generic", "colsum", ("vnet_colsum",), lambda p: _rowgroup_geom(p["M"], p["C"]), {"out": "E"}, {},
        dict(C=(1, 3, 12, 37)), kernel="colsum_generic_kernel", prior=(lambda p: G(p["M"] * p["C"] // 4 + 1, p["M"] * p["C"]), None))
    add("colsum16", "colsum", ("vnet_colsum_b16", "vnet_colsum_b16_ws_bytes"), _cs16_geom, {"out": "E"}, dict(b16=1), dict(C=(8, 16, 24, 64)),
        {"grid": (("r1", "rm1", "mult"), "one block per 256 / CO rows: every row group has its own block below the cap")},
        kernel="colsum_b16_kernel")
    # ---- the loss head ----
    lk = dict(K=Ks, B=(1, 2, 3), kind=LOSS_KINDS)
    lgeom = lambda p: G(p["M"] // 4 + 1, p["M"])
    voxels = lambda p: p["M"] >= 48                 # (every case holds every voxel kind of its K and labels on both sides of [0, K))
    add("loss-fwd", "loss", ("vnet_softmax_dice_fwd", "vnet_loss_ws_bytes"), lambda p: G(p["M"] // 4 + 1, p["M"], U=LOSS_U),
        {"softmax": "E", "pred": "E", "loss": "B", "dice": "B", "coef": "B"}, dict(op="fwd"), lk,
        {"group": (("eq", "r1", "rm1", "mult"), "the grid is sized for V / 4 + 1 voxels and a group is four slots: one group holds all of them "
                   "below the cap")}, clamped=True, accept=voxels, kernel="softmax_dice_fwd_kernel<K> + loss_finalize_kernel")
    add("loss-bwd", "loss", ("vnet_softmax_dice_bwd",), lgeom, {"dlogits": "E"}, dict(op="bwd"), lk, accept=voxels, kernel="softmax_dice_bwd_kernel<K>")
    dk = dict(K=Ks, B=(1, 2, 3), jac=(0, 1), wx=(0, 1, 1))
    add("dice-fwd", "dice", ("vnet_dice_coe_fwd",), lgeom, {"dice": "B", "coef": "B"}, dict(op="fwd"), dk, kernel="dice_sums_kernel<K> + loss_finalize_kernel")
    add("dice-bwd", "dice", ("vnet_dice_coe_bwd",), lambda p: G(p["M"] * p["K"] // 4 + 1, p["M"] * p["K"]), {"dout": "E"}, dict(op="bwd"), dk,
        kernel="dice_grad_kernel")
    # ---- dropout ----
    dr = dict(rate=(0.5, 0.75), dev=(0, 1, 0))
    drt = {"mask": "E (the restated hash)", "y": "E", "dx": "E"}
    add("dropout", "dropout", ("vnet_dropout_fwd", "vnet_dropout_bwd", "vnet_dropout_fwd_dev", "vnet_step_state_set"),
        lambda p: G(p["M"] // 4 + 1, p["M"]), drt, {}, dr, kernel="dropout_fwd_kernel / dropout_bwd_kernel")
    add("dropout16", "dropout", ("vnet_dropout_fwd_b16", "vnet_dropout_bwd_b16"), lambda p: G(p["M"] // 2 + 1, p["M"]), drt, dict(b16=1), dr,
        {"grid": (("mult",), "half of the octets + 1, as head-fwd")}, kernel="dropout_fwd_b16_kernel / dropout_bwd_b16_kernel")
    # ---- optimisers: the 16-byte aligned buffers and a 4-byte-offset view of each ----
    # Only adam_kernel tests the alignment of its buffers: sgd_kernel and momentum_kernel are one scalar loop, so their -aligned and
    # -offset rows launch the SAME kernel form on two kinds of pointer (the issue asks for both) and have no `vec` axis; adam-offset is
    # adam_kernel's scalar loop, adam-aligned its float4 loop with the scalar tail (the only row with a vector unit)
    tail = {"vec": (("eq", "mult"), "n must have a non-empty scalar tail")}
    ogeom = lambda p: G(p["M"] // 4 + 1, p["M"], blocks=2)
    same = " (one scalar loop: the aligned and the offset row run the same code)"
    two = {"grid": (("mult",), "twice ew_blocks(n / 4 + 1) blocks: two slots of the grid always hold n elements below the cap")}
    for kind, ents, tiers in (("sgd", ("vnet_sgd_apply", "vnet_sgd_apply_dev"), {"p": "E"}),
                              ("momentum", ("vnet_momentum_apply", "vnet_momentum_apply_dev"), {"p": "E", "acc": "E"}),
                              ("nesterov", ("vnet_momentum_apply", "vnet_momentum_apply_dev"), {"p": "E", "acc": "E"})):
        for off in (0, 1):
            add("%s-%s" % (kind, "offset" if off else "aligned"), "opt", ents, ogeom, tiers, dict(kind=kind, off=off), dict(dev=(0, 1)), two,
                kernel=("sgd" if kind == "sgd" else "momentum") + "_kernel" + same)
    at = {"m": "E", "v": "E", "p": "R"}
    add("adam-aligned", "opt", ("vnet_adam_apply", "vnet_adam_apply_dev"), lambda p: G(p["M"] // 4 + 1, p["M"] // 4, blocks=2, vec=(p["M"], 4)), at,
        dict(kind="adam", off=0), dict(dev=(0, 1)),
        dict(vec=tail["vec"], grid=(("r1", "rm1", "mult", "eq"), "twice ew_blocks(n / 4 + 1) blocks walk n / 4 float4 items: "
             "they fit the first half of one slot below the cap")), accept=lambda p: p["M"] % 4 != 0,
        kernel="adam_kernel: the float4 loop and its scalar tail")
    add("adam-offset", "opt", ("vnet_adam_apply", "vnet_adam_apply_dev"), ogeom, at, dict(kind="adam", off=1), dict(dev=(0, 1)), two,
        kernel="adam_kernel: the scalar loop")
    # ---- the rest ----
    add("cast-bf16", "cast", ("vnet_cast_bf16",), lambda p: G(p["M"] * (p["Cpad"] // 8) // 2 + 1, p["M"] * (p["Cpad"] // 8)), {"y": "R"}, {},
        dict(C=(1, 3, 4, 8, 11)), {"grid": (("mult",), "half of the units + 1, as head-fwd")}, kernel="cast_pad_bf16_kernel")
    for cnt in (1, 0):
        add("patch-%s" % ("count" if cnt else "nocount"), "patch", ("vnet_accumulate_patch",), lambda p: G(p["M"] * p["py"] * p["px"], p["M"] * p["py"] * p["px"]),
            {"vol": "E", "cnt": "E"}, dict(count=cnt, K=3), dict(face=("z", "y", "x", "zyx", "none")),
            {"grid": (("r1", "rm1", "mult"), ONE_THREAD), "block": (("r1", "rm1"), "the items are pz planes of 8 x 8 voxels")},
            accept=lambda p: p["M"] >= 3 or "z" not in p["face"], kernel="accumulate_patch_kernel")
    return collections.OrderedDict((r.name, r) for r in rows)


ROWS = _table()

# entry points of the two headers that elementwise.hip implements and no row names, with the reason (the host test's ledger)
EXCLUDED = {
    "vnet_bn_chain_coef_fwd": "per-channel float64 kernel: no per-element structure (tests/test_hip_ops.py holds it)",
    "vnet_bn_chain_coef_bwd": "per-channel float64 kernel: no per-element structure",
}


def params_of(row, i, size):
    p = row.params(i, size)
    if row.family == "cast":
        p["Cpad"] = cdiv(p["C"], 8) * 8
    if row.family == "patch":
        f = p["face"]
        p.update(py=8, px=8, D=size + 3, H=12, W=11, z0=2, y0=1, x0=2)
        if "z" in f:
            p["z0"] = 5                                                       # (D = pz + 3: pz - 2 planes inside, 2 outside)
        if "y" in f:
            p["y0"] = 7
        if "x" in f:
            p["x0"] = 6
    return p


Case = collections.namedtuple("Case", "row i size capped")


def case_params(c):
    return params_of(ROWS[c.row], c.i, c.size)


def geom_of(p_or_case):
    if isinstance(p_or_case, Case):
        return ROWS[p_or_case.row].geom(case_params(p_or_case))
    return ROWS[p_or_case["_row"]].geom(p_or_case)


def cid(c):
    p = case_params(c)
    keys = [k for k in ROWS[c.row].rot if k != "face"] + (["face"] if "face" in p else [])
    return "%s-%s%d%s" % (c.row, "".join("%s%s-" % (k, p[k]) for k in keys), c.size, "-cap" if c.capped else "")


def realisable(row):
    """Every (axis, class) some extent below the cap realises under some rotation of the row's parameters (the host test holds
    Row.absent against it in both directions)."""
    out = set()
    nrot = max([len(v) for v in row.rot.values()] or [1])
    for i in range(nrot):
        for s in range(1, ITEMS_MAX + 1):
            p = params_of(row, i, s)
            if not row.accept(p):
                continue
            g = row.geom(p)
            if g.items > ITEMS_MAX:
                break
            if not g.capped and (g.items >= 1 or g.vec):
                out |= set(classes(g).items())
    return out


def nondegenerate(g, size):
    """An extent at which a tail, reduction or indexing defect can show: more than one block's slot, and at least five rows."""
    return g.items > g.per_block and size >= 5


def _extents(row, i, used):
    """[(extent, geometry)] the rotation step i admits below the cap, ascending."""
    out = []
    for s in range(1, ITEMS_MAX + 1):
        p = params_of(row, i, s)
        if not row.accept(p) or (tuple(p[k] for k in row.rot), s) in used:
            continue
        g = row.geom(p)
        if g.items > ITEMS_MAX:
            break
        if not g.capped and (g.items >= 1 or g.vec):
            out.append((s, g))
    return out


def _prior_row(row):
    geom, absent = row.prior
    return Row(row.name, row.family, row.entries, geom, row.tiers, row.fixed, row.rot, absent, row.clamped, row.nocap, row.accept, row.kernel)


def _gen_row(row, seed=()):
    """seed: cases the row keeps from an earlier geometry (Row.prior); they count for what they realise under the present one, phase 1
    is theirs, and phases 2 and 3 add the rest.
    Phase 1: every rotation step (so every value of every rotated parameter) at a NON-DEGENERATE extent -- the one that realises
    the most classes still missing; among equals one past the grid's first slot, then one with a ragged block tail, then the
    smallest.  Phase 2: further steps, any extent, until every needed class (lt and eq among them) has occurred.  Phase 3: a rotated
    value that phase 1 never reached at a non-degenerate extent (its step collides with a refused combination) gets the first
    later step that carries it."""
    need, covered, cases, used = row.needed(), set(), [], set()
    nrot = max([len(v) for v in row.rot.values()] or [1])
    good = {k: set() for k in row.rot}                                       # values seen at a non-degenerate extent

    def take(i, s, g, cl):
        cases.append(Case(row.name, i, s, False))
        p = params_of(row, i, s)
        used.add((tuple(p[k] for k in row.rot), s))
        covered.update(cl)
        if nondegenerate(g, s):
            for k in row.rot:
                good[k].add(p[k])

    def best_of(cands, i):
        def key(sg):
            s, g = sg
            cl = set(classes(g).items()) & need
            stride = g.grid * g.per_block
            return (len(cl - covered), g.items > stride, g.items % g.per_block != 0, len(cl), -s)
        s, g = max(cands, key=key)
        return s, g, set(classes(g).items()) & need

    if row.sizes:
        for i, s in enumerate(row.sizes):
            take(i, s, row.geom(params_of(row, i, s)), set())
        return cases
    for c in seed:
        g = row.geom(params_of(row, c.i, c.size))
        take(c.i, c.size, g, set(classes(g).items()) & need)
    for i in range(0 if seed else nrot):
        cands = [(s, g) for s, g in _extents(row, i, used) if nondegenerate(g, s)]
        if cands:
            take(i, *best_of(cands, i))
    i = nrot
    while need - covered:
        assert i < nrot + 40, "%s: classes %s are not realised by any extent" % (row.name, sorted(need - covered))
        cands = _extents(row, i, used)
        if cands:
            s, g, cl = best_of(cands, i)
            if cl - covered:
                take(i, s, g, cl)
        i += 1
    for k, vals in row.rot.items():
        for v in vals:
            j = i
            while v not in good[k]:
                assert j < i + 400, "%s: %s = %s admits no non-degenerate extent" % (row.name, k, v)
                if params_of(row, j, 1)[k] == v:
                    cands = [(s, g) for s, g in _extents(row, j, used) if nondegenerate(g, s)]
                    if cands:
                        take(j, *best_of(cands, j))
                j += 1
    return cases


def _capped_case(row, i):
    """The smallest extent whose launch reaches the grid cap, makes a second trip and ends inside one, plus 37."""
    def ok(s):
        p = params_of(row, i, s)
        g = row.geom(p)
        return g.capped and g.items > g.grid * g.per_block * g.U
    lo, hi = 1, 2
    while not ok(hi):
        lo, hi = hi, hi * 2
        assert hi < 1 << 26, row.name
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    s = hi + 37
    while not row.accept(params_of(row, i, s)):
        s += 1
    return Case(row.name, i, s, True)


_CASES = []


def generate():
    if not _CASES:
        for row in ROWS.values():
            first = _prior_row(row) if row.prior else row
            cs = _gen_row(first)
            if row.prior:
                cs = _gen_row(row, seed=cs)
            _CASES.extend(cs)
            if row.nocap is None:
                # the cheapest parameters for the big case: the rotation step whose capped extent holds the fewest elements
                # (a row with a prior geometry keeps that geometry's big case: wraps() holds it to the present launch all the same)
                cands = [_capped_case(first, c.i) for c in cs]
                _CASES.append(min(cands, key=lambda c: (case_params(c).get("K", 2) < 2, _elements(c))))     # (not the one-class softmax)
    return list(_CASES)


def _elements(c):
    p = case_params(c)
    return p["M"] * p.get("C", 1) * p.get("K", 1) * p.get("B", 1)


def wraps(c):
    """The trips test's assertions on a capped case: the grid at its cap, at least two trips, the last one partial."""
    g = geom_of(c)
    if g.launch is None:                                                      # vnet_colsum_b16: a cap and a block of its own
        per_trip = g.grid * g.per_block
        assert g.grid == CS16_MAXBLK and g.items > per_trip and g.items % per_trip != 0, cid(c)
        return cdiv(g.items, per_trip)
    return _wraps(cid(c), g.launch, items=g.items, per_block=g.per_block * g.U, blocks=g.blocks)


# ---- operands, oracle, bound ------------------------------------------------------------------------------------------------------
def _with_row(c):
    p = case_params(c)
    p["_row"] = c.row
    return p


def _draw(c, lv):
    gen = FAMILIES[ROWS[c.row].family][0]
    return gen(_with_row(c), lv, np.random.default_rng(zlib.crc32(("%s/%d" % (cid(c), lv)).encode())))


def formula(c, d, A, **kw):
    return FAMILIES[ROWS[c.row].family][2](A, _with_row(c), d, **kw)


def _bound_of(A):
    return max([float(np.max(v)) for v in A.mag.values() if np.size(v)] or [0.0])


def bound(c, d=None):
    """sum |terms| * 2^q over the widest column sum / dot product / element of the case's E outputs: the oracle on absolute values."""
    d = operands(c) if d is None else d
    A = Arith()
    formula(c, d, A)
    return _bound_of(A)


def operands(c):
    """The first operand level whose bound is below 2^24 (a capped case starts at the second: the widest never fits 2^18 rows)."""
    n = FAMILIES[ROWS[c.row].family][1]
    for lv in range(1 if (c.capped and n > 1) else 0, n):
        d = _draw(c, lv)
        d["level"] = lv
        if bound(c, d) < LIMIT:
            return d
    raise AssertionError("%s: no operand level keeps sum |terms| * 2^q below 2^24" % cid(c))


def stored(c, out):
    """What the device stores for the values `out`: a bf16 tensor (y, ds, dx of the bf16 rows) holds one RNE rounding of the result."""
    p, row = case_params(c), ROWS[c.row]
    out = {k: np.asarray(v, np.float64) for k, v in out.items()}
    if p.get("b16"):
        for k in ("y", "ds", "dx"):
            if k in out and k + "~" not in out and not (row.family == "head" and k == "y"):
                out[k] = O.round_bf16(out[k])
    return out


def exact(c, d, invstd=None):
    """{output: expected value (float64)} and, for tier B, {output + '~': bound}: E outputs from the float64 oracle, R outputs from
    the float32 restatement (which equals the oracle wherever the output is also exact)."""
    kw = {"invstd": invstd} if invstd is not None else {}
    e = formula(c, d, Arith(), **kw)
    r = formula(c, d, Arith(f32=True, fused=False), **kw)
    p, row = case_params(c), ROWS[c.row]
    out = {}
    for k, v in e.items():
        t = row.tiers.get(k.rstrip("~"), "")
        if t.startswith("R") or (p.get("act") == "lrelu" and k == "y"):
            v = r[k]
        out[k] = np.asarray(v, np.float64)
    return stored(c, out)


def table(cases=None):
    cases = generate() if cases is None else cases
    lines = ["%-22s %-5s %-60s %s" % ("row", "cases", "tiers", "kernel")]
    for name, row in ROWS.items():
        n = sum(1 for c in cases if c.row == name)
        lines.append("%-22s %-5d %-60s %s" % (name, n, ", ".join("%s: %s" % kv for kv in row.tiers.items()), row.kernel))
    return "\n".join(lines)
