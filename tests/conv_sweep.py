"""Exact-integer ragged-shape sweep of the convolution kernels: the variant table, the case generator and the exact oracle (host
only -- nothing here touches a GPU; tests/test_conv_sweep_host.py checks this module, tests/test_hip_conv_sweep.py runs its cases).

WHY EXACT.  Operands are small integers (x, dy in [-3, 3], w in [-2, 2], bias in [-3, 3]; all bf16-exact).  Every product and every
partial sum of every summation order is then an integer of magnitude <= bound(case), and bound(case) <= 2^20 is REQUIRED of a case
(LIMIT below), so fp32 accumulation -- whatever the split-K plan, the sign alternation of the f32x3 kernels or the MFMA flavour --
produces the exact integer: the comparison with the float64 oracle is `==`.  A bf16 tensor stores round_bf16(exact): one rounding
of an exact integer, also compared with `==`.

LIMIT = 2^20 leaves 4 bits under fp32's 24 for the bf16 MFMA, which aligns the 32 products of a K block to the largest term before
it adds them.  profiles/r06_mfma_round_probe.txt: "c=0: 2^24 - 2^24 + 30 x 1.0" comes out as exactly 30 on v_mfma_f32_16x16x32_bf16
(and is wrong only from 2^28 on), i.e. the internal sum keeps at least 25 bits below its largest term: integer terms below 2^20 are
far inside that, the limit stays at 2^20.  bound(case) is a condition on the INPUTS (the oracle run on |x|, |w|, |dy| + |bias|), not
a measurement of the kernels; a case that exceeds it gets a narrower value range (operands()), it is never dropped or exempted.

THE VARIANT TABLE (VARIANTS) has one row per launchable kernel form: how to force it (compute mode, channels, library options,
ops._X3 / _DIRECT2 / _IN4 / _FUSE switches), its brick (TZ, TY, TX), its channel granularity, whether it is a persistent grid, and the
C function the row was read from.  Which form runs inside a family is decided in C from the shape and the options, so the table's
`accept` predicates restate those C planners in Python (plan_conv, plan_wgrad, plan_conv_bf16, conv_bf16_use_c16 / _r32,
plan_conv_deep, x3_plan_conv, x3_plan_wgrad, zs_shape_ok ...); the host test holds the restatements to the shape-only queries the
library exports (statistics rows, workspace bytes) for every generated case.

GRID.  The persistent kernels launch one workgroup per CU: 256 on the MI355X (conv_x3.hip x3_grid(), conv_kernels.h
conv_fwd_bf16_go: dim3(256)); the ping-pong 16-cout kernel launches two per CU, 512.  Item counts are compared with these numbers.

THE GENERATOR is deterministic (no hypothesis: a failing case is a stable pytest id).  Per variant and axis the extent classes are
lt (e < T), eq (e = T), r1 (e = kT + 1, k >= 1), rm1 (e = kT + T - 1, k >= 1), mult (e = kT, k >= 2); a class an axis cannot realise
under the variant's own shape rule (W == 8, W < 16, extents <= 4, T = 1 ...) is absent from that axis and listed as such by
classes_of().  Classes are combined by an each-choice design with rotated offsets (case i takes class i, i + 1, i + 2 of the three
axes): every (variant, axis, class) triple occurs, plus one case per variant with all three axes ragged, at 5-7 cases per variant.
(Full pairwise covering of 5 x 5 x 5 classes needs 25 cases per variant, about 1300 cases: measured, the 353 cases cost 20 % of the rest
of the GPU suite, four times as many would cost most of it.  pair_coverage() counts the class pairs that are covered.)  Extents start at the smallest k and grow, class preserved, until the variant's `accept` holds (e.g. >= 256 bricks
for the persistent 16-cout kernel).  `extra` rows of a variant are hand-picked shapes for the conditions no class realises: fewer /
more items than workgroups, split 1 / > 1, W = 7 / 8 / 9.

OPERAND PROFILES (PROFILES, operands_x3, x3_runs; further down): the f32x3 rows run a second time on operands with 9-10 and 18
significant bits, which fill the m and l pieces of the split -- exactness argument, limit and sizing are stated there."""
import collections
import functools
import zlib

import numpy as np
import torch

from oracle import torch_ref as T
from oracle import vnet_oracle as O

LIMIT = 1 << 20
GRID = 256
CLASSES = ("lt", "eq", "r1", "rm1", "mult")
RAGGED = ("r1", "rm1")


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


# ---- the C planners, restated (held to the library's shape-only queries by tests/test_conv_sweep_host.py) -----------------------
def pick_ns(CoutP):                                                      # conv_kernels.h: pick_ns
    return 4 if CoutP % 64 == 0 else 2 if CoutP % 32 == 0 else 1


Plan = collections.namedtuple("Plan", "brick nb ncob nsplit nz")


def plan_conv(ks, stride, up, Cin, Cout, B, Do, Ho, Wo, f32_small=2):
    """conv_kernels.h: plan_conv (fp32 MFMA kernels; also the bf16 2^3 pair, which runs them on bf16 tensors).  up: the dims are
    those of the coarse INPUT."""
    CoutP = rup(8 * Cout, 16) if up else rup(Cout, 16)
    ns = pick_ns(CoutP)
    ncob = CoutP // (16 * ns)
    small = Wo < 16
    half = 0
    if stride == 2 and not up:
        brick = (2, 8, 8) if small else (1, 4, 16)
    elif ks == 3 and not up:
        if Do <= 4 and Ho <= 4 and Wo <= 4 and Cin >= 32:
            half, brick = 2, (4, 4, 4)
        else:
            half, brick = 1, (4, 8, 8)
    elif ks == 5 and not up and not small:
        half, brick = 1, (4, 8, 8)
    elif ks == 5 and not up and f32_small >= 2 and Do <= 4 and Ho <= 4 and Wo <= 4 and Cin >= 32:
        half, brick = 2, (4, 4, 4)
    elif ks == 5 and not up and f32_small >= 1:
        half, brick = 1, (4, 8, 8)
    elif up and not small:
        brick = (2, 4, 16)
    else:
        brick = (8, 8, 8) if small else (4, 8, 16)
    nbr = lambda: B * cdiv(Do, brick[0]) * cdiv(Ho, brick[1]) * cdiv(Wo, brick[2])
    nchunks = rup(Cin, 16) // 16
    if ks in (5, 3) and not up:
        nb, ncob1, fill = nbr(), ns * ncob, (512 if half == 2 else 256)
        if nb * ncob < fill and nb * ncob1 >= fill:
            while nb * ncob < fill:
                ns, ncob = ns // 2, ncob * 2
        else:
            while ns > 1 and nb * ncob * nchunks < fill:
                ns, ncob = ns // 2, ncob * 2
    if ks == 2 and not up:
        while ns > 1 and nbr() * ncob < 256:
            ns, ncob = ns // 2, ncob * 2
    if up:
        while ns > 1 and nbr() * ncob < 256:
            ns, ncob = ns // 2, ncob * 2
        if small and nbr() * ncob < 256:
            brick = (2, 8, 8)
    nwg = nbr() * ncob
    nsplit = 1
    if not up and nwg < 256 and nchunks > 1:
        nsplit = min(nchunks, cdiv(512, nwg))
    cps = cdiv(nchunks, nsplit)
    nsplit = cdiv(nchunks, cps)
    nz = ks if (ks in (5, 3) and not up and nwg * nsplit < 256) else 1
    return Plan(brick, nbr(), ncob, nsplit, nz)


def plan_wgrad(ks, kx, Cin, Cout, B, Do, Ho, Wo):
    """conv_kernels.h: plan_wgrad (fp32 and generic bf16 filter gradients; Do.. = dy's dims, the coarse ones of a 2^3 layer)."""
    ns = pick_ns(rup(Cout, 16))
    if ks in (5, 3) and ns == 4:
        ns = 2
    ncob = rup(Cout, 16) // (16 * ns)
    small = Wo < 16
    if ks in (5, 3):
        tw = 4 if (kx == 1 or ks == 3) else 16 // ns
        brick = (4, 8, 8) if small else (4, 4, 16)
    else:
        tw, brick = 1, ((2, 8, 8) if small else (2, 4, 16))
    ntg = cdiv(ks * ks * kx, 8 * tw)
    nb = B * cdiv(Do, brick[0]) * cdiv(Ho, brick[1]) * cdiv(Wo, brick[2])
    base = (rup(Cin, 16) // 16) * ncob * ntg
    return Plan(brick, nb, ncob, max(1, min(nb, cdiv(256, base))), 1)


def use_c16(Cin, Cout, C0, C1, Cy0, Cy1, B, D, H, W):                    # conv_kernels.h: conv_bf16_use_c16
    if Cout > 16 or (Cout & 3) or (C0 & 3) or (C1 & 3) or (Cy0 & 3) or (Cy1 & 3) or W < 16:
        return False
    return B * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 16) >= 256


def use_r32(Cout, Cy0, Cy1, B, D, H, W):                                 # conv_kernels.h: conv_bf16_use_r32
    if (Cout & 31) or (Cy0 & 15) or (Cy1 & 15) or W < 16 or H < 16:
        return False
    return B * cdiv(D, 4) * cdiv(H, 16) * cdiv(W, 16) * (Cout // 32) >= 256


def plan_bf16(Cin, Cout, B, D, H, W):                                    # conv_kernels.h: plan_conv_bf16
    ncob, nchunks = rup(Cout, 32) // 32, rup(Cin, 16) // 16
    small = W < 16
    half = (not small) and B * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 16) <= 256
    brick = (8, 8, 8) if small else (4, 8, 8 if half else 16)
    nb = B * cdiv(D, brick[0]) * cdiv(H, brick[1]) * cdiv(W, brick[2])
    nsb = 2 if (ncob % 2 == 0 and nb * (ncob // 2) >= 256) else 1
    nwg = nb * (ncob // nsb)
    nsplit = 1
    if nwg <= 255 and nchunks > 1:
        nsplit = min(nchunks, cdiv(512, nwg))
    cps = cdiv(nchunks, nsplit)
    nsplit = cdiv(nchunks, cps)
    nz = 5 if nwg * nsplit < 64 else 1
    return Plan(brick, nb, ncob // nsb, nsplit, nz)


def plan_deep(C0, C1, Cy0, Cy1, B, D, H, W, deep=1, target=256):
    """conv_deep.h: plan_conv_deep -> None, or the Plan of the deep-level kernel (bricks of 4x8x8, 32-cout blocks)."""
    Cin, Cout = C0 + C1, Cy0 + Cy1
    if not deep or (Cout & 31) or (C0 & 15) or (C1 & 15) or (Cy0 & 7) or (Cy1 & 7) or Cin < 16:
        return None
    if use_c16(Cin, Cout, C0, C1, Cy0, Cy1, B, D, H, W):
        return None
    nb = B * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 8)
    nwg0 = nb * (Cout // 32)
    if nwg0 > 512:
        return None
    if use_r32(Cout, Cy0, Cy1, B, D, H, W) and nwg0 >= 256:
        g = plan_bf16(Cin, Cout, B, D, H, W)
        if g.nsplit * g.nz == 1:
            return None
    nchunks = Cin // 16
    ns = max(1, min(nchunks, (max(1, target) + nwg0 - 1) // nwg0))
    cps = cdiv(nchunks, ns)
    return Plan((4, 8, 8), nb, Cout // 32, cdiv(nchunks, cps), 1)


def b16_forward(C0, C1, Cy0, Cy1, B, D, H, W, cin_real=0, deep=1, target=256, c16pp=1):
    """conv_b16.hip: conv_fwd_b16_impl + conv_kernels.h: conv_fwd_bf16_go -> (kernel name, Plan).  Tensors 16-byte aligned."""
    Cin, Cout = C0 + C1, Cy0 + Cy1
    in4 = 0 < cin_real <= 4 and C0 == 8 and C1 == 0
    dp = None if in4 else plan_deep(C0, C1, Cy0, Cy1, B, D, H, W, deep, target)
    if dp is not None:
        return "deep", dp
    p = plan_bf16(Cin, Cout, B, D, H, W)
    if use_c16(Cin, Cout, C0, C1, Cy0, Cy1, B, D, H, W):
        nb = B * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 16)
        pp = (not in4) and c16pp and Cin >= 16 and not (C0 & 7) and not (C1 & 7)
        return ("c16pp" if pp else "in4" if in4 else "c16"), Plan((4, 8, 16), nb, 1, 1, 1)
    if use_r32(Cout, Cy0, Cy1, B, D, H, W) and p.nsplit * p.nz == 1:
        return "r32", Plan((4, 16, 16), B * cdiv(D, 4) * cdiv(H, 16) * cdiv(W, 16), Cout // 32, 1, 1)
    return "generic", p


def b16_rows(C0, C1, O_, B, D, H, W, cin_real=0, deep=1, target=256):
    """conv_b16.hip: vnet_conv_b16_stats_rows, from the restated plans (what the host test holds against the library)."""
    name, p = b16_forward(C0, C1, O_, 0, B, D, H, W, 0, deep, target)      # (the query does not know about the padded input)
    if p.nsplit * p.nz > 1:
        return 0 if (O_ > 256 or 256 % O_) else min(2048, cdiv(B * D * H * W * O_, 256))
    return p.nb


def x3_brick(W):                                                         # conv_x3.h: x3_conv_nbz / X3_TY / X3_TX, X3G<true>
    return (4, 8, 8) if W == 8 else (2, 8, 16)


def x3_plan(Cin, Cout, B, D, H, W, nb2_opt=1):
    """conv_x3.h: x3_plan_conv + conv_x3.hip: vnet_conv_fwd_x3 -> (kernel name, Plan, items); Plan.nsplit = K split over workgroups."""
    br = x3_brick(W)
    nb = B * cdiv(D, br[0]) * cdiv(H, br[1]) * cdiv(W, br[2])
    if W < 16 and W != 8:                     # (the plan refuses the shape; a forced launch runs it unsplit on the normal brick)
        return "x3", Plan(br, nb, Cout // 16, 1, 1), nb * (Cout // 16)
    items, nks, cps = nb * (Cout // 16), 1, Cin // 16
    while items * nks < 256 and cps % 2 == 0 and cps >= 4:
        nks, cps = nks * 2, cps // 2
    nb2 = W != 8 and Cout % 32 == 0 and items * nks >= 2 * GRID and nb2_opt
    return ("x3-narrow" if W == 8 else "x3-nb2" if nb2 else "x3"), Plan(br, nb, Cout // 16, nks, 1), (items // 2 if nb2 else items) * nks


def x3_wgrad_plan(Cin, Cout, B, D, H, W):                                # conv_x3.h: x3_plan_wgrad
    br = x3_brick(W)
    nb = B * cdiv(D, br[0]) * cdiv(H, br[1]) * cdiv(W, br[2])
    nblk = (Cin // 16) * (Cout // 16)
    return Plan(br, nb, Cout // 16, max(1, min(nb, cdiv(256, nblk))), 1)


def b16_wgrad(C0, C1, Cout, cin_dw, B, D, H, W, zs=2, rr=1, in4=1):
    """conv_b16.hip: vnet_conv_wgrad_b16 -> (kernel name, Plan)."""
    CinP, CoutP = rup(C0 + C1, 16), rup(Cout, 16)
    in4z = cin_dw <= 4 and C0 == 8 and C1 == 0
    zs_ok = CoutP % 32 == 0 and not (C0 & 7) and not (C1 & 7) and not (Cout & 7) and (C1 == 0 or (C0 & 15) == 0)     # wgrad_zs.h: zs_shape_ok
    if zs == 1 and zs_ok and (W >= 16 or D <= 12) and not in4z:          # wgrad_zs.h: zs_depth_ok
        tx = 32 if W >= 32 else 16 if W >= 16 else 8                     # wgrad_zs.h: zs_tx, zs_geometry
        br = (32 // tx, 8, tx)
        nb = B * cdiv(D, br[0]) * cdiv(H, 8) * cdiv(W, tx)
        return "zs", Plan(br, nb, CoutP // 32, max(1, min(nb, cdiv(256, (CinP // 16) * (CoutP // 32)))), 1)
    p = plan_wgrad(5, 5, C0 + C1, Cout, B, D, H, W)
    rr_nb = B * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 32)
    rr_ns = max(1, min(rr_nb, cdiv(256, (CinP // 16) * (CoutP // 16))))
    if rr and W >= 32 and H >= 8 and rr_ns <= p.nsplit and ((C0 & 15) == 0 or C1 == 0) and (rr == 2 or rr_nb >= rr_ns):
        return ("rr-in4" if (in4z and in4) else "rr"), Plan((4, 8, 32), rr_nb, CoutP // 16, rr_ns, 1)
    return "generic", p


# ---- cases ----------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "variant B D H W C0 C1 O tag")):
    """One problem of a variant.  D, H, W: the layer's input volume (the FINE volume of a 2^3 pair case); C0 | C1 -> O channels (the
    pair: Cf = C0, Cc = O; the padded bf16 input: C0 = the real channel count; the input block: C0 = O = the block's channels)."""
    __slots__ = ()

    @property
    def v(self):
        return VARIANTS[self.variant]

    @property
    def cid(self):
        return "%s-%dx%dx%dx%d-%d+%d-%d%s" % (self.variant, self.B, self.D, self.H, self.W, self.C0, self.C1, self.O,
                                              "-" + self.tag if self.tag else "")

    @property
    def seed(self):
        return zlib.crc32(self.cid.encode())

    @property
    def dims(self):
        return (self.D, self.H, self.W)

    @property
    def coarse(self):
        return tuple((d + 1) // 2 for d in self.dims)

    @property
    def grid_dims(self):
        """The volume the variant's brick tiles: the coarse one for a 2^3 pair, else the layer's."""
        return self.coarse if self.v.op == "pair" else self.dims


class Variant(object):
    """A row of the table.  mode: fp32 | x3 (fp32_split3, ops._X3 forced) | bf16 (bf16 tensors).  op: conv5 | conv3 | pair | input.
    launch: which launch of the case the row is about (fwd | wgrad | up; a case always runs and checks all of them).  brick: (TZ, TY, TX)
    or a function of the case's W.  gran: channel granularity.  opts: library options; flags: ops switches.  rule: shape rule of the
    form (per-axis predicate on the grid dims).  accept(case): the C planners take THIS form for the case.  families: what
    ops.route() must answer for (fwd, bwd, wgrad).  persistent: the grid size of a persistent kernel, else 0.  items(case): work
    items of the launch.  split(case): the split factor (K over workgroups, slabs), None = the form has none.  cite: where in
    csrc/ the row was read.  observe: the shape-only query that tells this option value from its twin, or why none can."""

    def __init__(self, name, mode, op, launch, brick, gran, channels, families, cite, opts=(), flags=(), rule=None, accept=None,
                 persistent=0, items=None, split=None, extra=(), observe="", twin=None, two_src=None):
        self.name, self.mode, self.op, self.launch, self._brick, self.gran = name, mode, op, launch, brick, gran
        self.channels, self.families, self.cite, self.opts, self.flags = channels, families, cite, tuple(opts), tuple(flags)
        self.rule = rule or (lambda d, h, w: True)
        self._accept, self.persistent, self._items, self._split = accept, persistent, items, split
        self.extra, self.observe, self.twin = extra, observe, twin
        # two sources: every 5^3 / 3^3 kernel takes x0 | x1, except the zero-padded network input; the 2^3 pair and the input block take one
        self.two_src = (op in ("conv5", "conv3") and families[0] != "conv-bf16-padded") if two_src is None else two_src

    def brick(self, W):
        return self._brick(W) if callable(self._brick) else self._brick

    def opt(self, name, default):
        return int(dict(self.opts).get(name, default))

    def accept(self, c):
        return self.rule(*c.grid_dims) and (self._accept is None or bool(self._accept(c, self)))

    def items(self, c):
        if self._items is not None:
            return self._items(c, self)
        br, g = self.brick(c.grid_dims[2]), c.grid_dims
        return c.B * cdiv(g[0], br[0]) * cdiv(g[1], br[1]) * cdiv(g[2], br[2])

    def split(self, c):
        return None if self._split is None else self._split(c, self)


def _fwd16(c, v, **kw):
    cin = c.C0 if v.name.startswith("b16-padded") or v.name == "b16-wgrad-in4" else 0
    C0 = 8 if cin else c.C0
    return b16_forward(C0, c.C1, c.O, 0, c.B, c.D, c.H, c.W, cin, v.opt("BF16_DEEP", 1), v.opt("BF16_DEEP_TARGET", 256),
                       v.opt("BF16_C16PP", 1))


def _wg16(c, v):
    cin = c.C0 if v.name == "b16-wgrad-in4" else 0
    return b16_wgrad(8 if cin else c.C0, c.C1, c.O, cin or c.C0 + c.C1, c.B, c.D, c.H, c.W, v.opt("WGRAD_ZS", 2), v.opt("WGRAD_RR", 1),
                     v.opt("CONV_IN4", 1))


def _f32(c, v, ks=5):
    return plan_conv(ks, 1, 0, c.C0 + c.C1, c.O, c.B, c.D, c.H, c.W, v.opt("F32_SMALL", 2))


def _f32w(c, v, ks=5):
    return plan_wgrad(ks, ks, c.C0 + c.C1, c.O, c.B, c.D, c.H, c.W)


def _x3(c, v):
    return x3_plan(c.C0 + c.C1, c.O, c.B, c.D, c.H, c.W, v.opt("X3_NB2", 1))


W16 = lambda d, h, w: w >= 16
W15 = lambda d, h, w: w < 16
W8 = lambda d, h, w: w == 8
LE4 = lambda d, h, w: d <= 4 and h <= 4 and w <= 4
CONV, WG = ("conv", "conv", "wgrad"), ("conv", "conv", "wgrad")
X3F, B16F = ("conv-x3", "conv-x3", "wgrad-x3"), ("conv-bf16", "conv-bf16", "wgrad-bf16")
NOQ = "no shape-only query tells the two option values apart (%s)"


def _table():
    t = []
    add = lambda *a, **k: t.append(Variant(*a, **k))
    # ---- fp32 5^3: conv_kernels.h plan_conv / conv_mfma.hip conv_fwd_impl --------------------------------------------------------
    add("f32-k5-8x8x8", "fp32", "conv5", "fwd", (8, 8, 8), 16, [(16, 0, 16), (16, 16, 16)], CONV, "plan_conv: W < 16 and F32_SMALL = 0 -> brick_counts<8,8,8>",
        opts=[("F32_SMALL", 0)], rule=W15, accept=lambda c, v: _f32(c, v).brick == (8, 8, 8), twin="f32-k5-4x8x8-small",
        observe="vnet_conv_stats_rows counts 8x8x8 bricks (F32_SMALL = 1: 4x8x8) where the launch is not split",
        extra=[(2, 64, 64, 15, 16, 0, 16, "rows")])
    add("f32-k5-4x8x8-small", "fp32", "conv5", "fwd", (4, 8, 8), 16, [(16, 16, 16)], CONV, "plan_conv: W < 16 and F32_SMALL >= 1 -> half = 1, 4x8x8",
        opts=[("F32_SMALL", 1)], rule=W15, accept=lambda c, v: _f32(c, v).brick == (4, 8, 8))
    add("f32-k5-4x4x4", "fp32", "conv5", "fwd", (4, 4, 4), 16, [(32, 0, 32), (32, 32, 32)], CONV, "plan_conv: F32_SMALL >= 2, extents <= 4, Cin >= 32 -> half = 2",
        opts=[("F32_SMALL", 2)], rule=LE4, accept=lambda c, v: _f32(c, v).brick == (4, 4, 4))
    add("f32-k5-wide", "fp32", "conv5", "fwd", (4, 8, 8), 16, [(16, 0, 16), (16, 16, 16)], CONV, "plan_conv: ks = 5, W >= 16 -> half = 1, 4x8x8 (4 waves)",
        rule=W16, accept=lambda c, v: _f32(c, v).brick == (4, 8, 8))
    add("f32-k5-splitk", "fp32", "conv5", "fwd", lambda W: (4, 8, 8), 16, [(64, 0, 32), (32, 32, 32)], CONV,
        "plan_conv: nwg < 256 and nchunks > 1 -> nsplit; nwg * nsplit < 256 -> nz = 5; splitk_reduce_kernel",
        accept=lambda c, v: c.tag == "nosplit" or _f32(c, v).nsplit > 1, split=lambda c, v: _f32(c, v).nsplit * _f32(c, v).nz,
        extra=[(2, 32, 32, 15, 16, 0, 64, "nosplit")])
    add("f32-k5-scalar", "fp32", "conv5", "fwd", lambda W: (4, 8, 8), 1, [(3, 0, 16), (16, 0, 5), (4, 4, 8), (6, 0, 10), (5, 3, 7)], CONV,
        "conv_fwd_impl: vec_in = C0 % 4 == 0 and C1 % 4 == 0, vec_out likewise: the scalar gather / scatter paths", two_src=True)
    add("f32-wgrad-4x4x16", "fp32", "conv5", "wgrad", (4, 4, 16), 16, [(16, 0, 16), (16, 16, 32)], WG, "plan_wgrad: W >= 16 -> 4x4x16",
        rule=W16, split=lambda c, v: _f32w(c, v).nsplit, extra=[(1, 3, 4, 16, 16, 0, 16, "one")])
    add("f32-wgrad-4x8x8", "fp32", "conv5", "wgrad", (4, 8, 8), 16, [(16, 0, 16), (16, 16, 32)], WG, "plan_wgrad: W < 16 -> 4x8x8",
        rule=W15, split=lambda c, v: _f32w(c, v).nsplit, extra=[(1, 4, 7, 8, 16, 0, 16, "one")])
    # ---- fp32 3^3 (U-Net) ------------------------------------------------------------------------------------------------------
    add("f32-k3-4x8x8", "fp32", "conv3", "fwd", (4, 8, 8), 16, [(16, 0, 16), (16, 16, 16), (3, 0, 5)], CONV, "plan_conv: ks = 3 -> half = 1, 4x8x8",
        accept=lambda c, v: _f32(c, v, 3).brick == (4, 8, 8))
    add("f32-k3-4x4x4", "fp32", "conv3", "fwd", (4, 4, 4), 16, [(32, 0, 32), (32, 32, 64)], CONV, "plan_conv: ks = 3, extents <= 4, Cin >= 32 -> half = 2",
        rule=LE4, accept=lambda c, v: _f32(c, v, 3).brick == (4, 4, 4))
    add("f32-k3-wgrad-4x4x16", "fp32", "conv3", "wgrad", (4, 4, 16), 16, [(16, 0, 16), (16, 16, 32)], WG, "vnet_conv_wgrad: ks = 3, W >= 16 -> launch_wgrad<3,1,4,4,16,..>",
        rule=W16, split=lambda c, v: _f32w(c, v, 3).nsplit, extra=[(1, 4, 3, 16, 16, 0, 16, "one")])
    add("f32-k3-wgrad-4x8x8", "fp32", "conv3", "wgrad", (4, 8, 8), 16, [(16, 0, 16), (16, 16, 32)], WG, "vnet_conv_wgrad: ks = 3, W < 16 -> launch_wgrad<3,1,4,8,8,..>",
        rule=W15, split=lambda c, v: _f32w(c, v, 3).nsplit, extra=[(1, 3, 8, 7, 16, 0, 16, "one")])
    # ---- f32x3 (forced): conv_x3.h / conv_x3.hip -------------------------------------------------------------------------------
    x3items = lambda c, v: _x3(c, v)[2]
    add("x3-conv", "x3", "conv5", "fwd", (2, 8, 16), 16, [(16, 16, 16), (16, 0, 48)], X3F, "conv_x3.h: X3_TZ / X3_TY / X3_TX = 2 x 8 x 16; vnet_conv_fwd_x3: NB = 1",
        rule=lambda d, h, w: w != 8, accept=lambda c, v: _x3(c, v)[0] == "x3" and _x3(c, v)[1].nsplit == 1, persistent=GRID, items=x3items,
        extra=[(1, 5, 9, 7, 16, 0, 16, "w7"), (1, 5, 9, 9, 16, 16, 16, "w9"), (2, 22, 41, 65, 16, 0, 16, "more")])
    add("x3-conv-narrow", "x3", "conv5", "fwd", (4, 8, 8), 16, [(16, 16, 16), (32, 0, 32)], X3F, "conv_x3.hip: w8 = (W == 8) -> conv5_x3_kernel<S, 1, true>, X3G<true> 4 x 8 x 8",
        rule=W8, accept=lambda c, v: _x3(c, v)[0] == "x3-narrow", persistent=GRID, items=x3items,
        extra=[(3, 37, 73, 8, 16, 0, 16, "more")])
    add("x3-conv-nb2", "x3", "conv5", "fwd", (2, 8, 16), 32, [(16, 0, 32), (16, 16, 32)], X3F, "conv_x3.hip: nb2 = Cout % 32 == 0 and items * nks >= 2 * grid and X3_NB2",
        opts=[("X3_NB2", 1)], rule=W16, accept=lambda c, v: _x3(c, v)[0] == "x3-nb2", persistent=GRID, items=x3items, twin="x3-conv-nb1",
        observe=NOQ % "statistics rows are per brick, the workspace is the K split's, for one and for two cout blocks per item")
    add("x3-conv-nb1", "x3", "conv5", "fwd", (2, 8, 16), 16, [(16, 0, 32), (16, 16, 32)], X3F, "conv_x3.hip: X3_NB2 = 0 -> conv5_x3_kernel<S, 1, false> on the shapes of x3-conv-nb2",
        opts=[("X3_NB2", 0)], rule=W16, accept=lambda c, v: x3_plan(c.C0 + c.C1, c.O, c.B, c.D, c.H, c.W, 1)[0] == "x3-nb2", persistent=GRID, items=x3items)
    add("x3-conv-ksplit", "x3", "conv5", "fwd", x3_brick, 16, [(64, 0, 16), (32, 32, 32)], X3F, "conv_x3.h: x3_plan_conv: items * nks < 256 -> nks *= 2; splitk_reduce_kernel",
        rule=lambda d, h, w: w >= 16 or w == 8, accept=lambda c, v: c.tag == "nosplit" or _x3(c, v)[1].nsplit > 1, persistent=GRID, items=x3items,
        split=lambda c, v: _x3(c, v)[1].nsplit, extra=[(1, 6, 8, 16, 48, 0, 16, "nosplit"), (1, 26, 40, 16, 128, 0, 16, "more")])
    xw = lambda c, v: x3_wgrad_plan(c.C0 + c.C1, c.O, c.B, c.D, c.H, c.W)
    add("x3-wgrad", "x3", "conv5", "wgrad", (2, 8, 16), 16, [(16, 16, 16), (32, 0, 16)], X3F, "conv_x3.hip: vnet_conv_wgrad_x3 -> wgrad5_x3_kernel<false>; x3_plan_wgrad",
        rule=lambda d, h, w: w != 8, split=lambda c, v: xw(c, v).nsplit, extra=[(1, 2, 7, 16, 16, 0, 16, "one"), (1, 5, 9, 7, 16, 0, 16, "w7"), (1, 5, 9, 9, 16, 0, 16, "w9")])
    add("x3-wgrad-narrow", "x3", "conv5", "wgrad", (4, 8, 8), 16, [(16, 16, 16), (32, 0, 16)], X3F, "conv_x3.hip: with_bool(W == 8) -> wgrad5_x3_kernel<true>, XWG<true>",
        rule=W8, split=lambda c, v: xw(c, v).nsplit, extra=[(1, 3, 8, 8, 16, 0, 16, "one")])
    # ---- bf16 5^3 forward / backward-data: conv_b16.hip conv_fwd_b16_impl, conv_kernels.h conv_fwd_bf16_go ---------------------------
    gen = lambda br: (lambda c, v: _fwd16(c, v) [0] == "generic" and _fwd16(c, v)[1].brick == br)
    add("b16-generic-8x8x8", "bf16", "conv5", "fwd", (8, 8, 8), 32, [(16, 0, 16), (16, 16, 16)], B16F, "plan_conv_bf16: W < 16 -> 8x8x8", rule=W15, accept=gen((8, 8, 8)))
    add("b16-generic-4x8x8", "bf16", "conv5", "fwd", (4, 8, 8), 32, [(16, 16, 16), (8, 8, 32)], B16F, "plan_conv_bf16: half = W >= 16 and <= 256 bricks of 4x8x16",
        rule=W16, accept=gen((4, 8, 8)))
    # (32 couts in rows shorter than 16: no 16-cout, no row-pair form; > 512 bricks of 4x8x8: no deep form.  Power-of-two channels: the
    #  bf16 batch-norm behind the statistics launch takes no others)
    add("b16-generic-4x8x16", "bf16", "conv5", "fwd", (4, 8, 16), 32, [(16, 0, 32), (16, 16, 32)], B16F, "plan_conv_bf16: > 256 bricks of 4x8x16 (and no c16 / row-pair / deep form)",
        rule=lambda d, h, w: w >= 16 and h < 16, accept=gen((4, 8, 16)))
    pers = lambda name: (lambda c, v: _fwd16(c, v)[0] == name)
    add("b16-c16pp", "bf16", "conv5", "fwd", (4, 8, 16), 16, [(16, 0, 16), (8, 8, 16)], B16F, "conv_bf16_use_c16pp -> conv5_bf16_c16pp_kernel (conv_c16pp.h), grid 2 x CUs",
        opts=[("BF16_C16PP", 1)], rule=W16, accept=pers("c16pp"), persistent=2 * GRID, twin="b16-c16",
        observe=NOQ % "conv_bf16_use_c16pp: 'the number of statistics rows stays a function of the shape alone'",
        extra=[(2, 21, 41, 65, 16, 0, 16, "fewer"), (3, 21, 41, 65, 8, 8, 16, "more")])
    add("b16-c16", "bf16", "conv5", "fwd", (4, 8, 16), 16, [(16, 0, 16), (8, 8, 16)], B16F, "conv_bf16_use_c16 -> conv5_bf16_c16_kernel<4,8,16>, grid 256",
        opts=[("BF16_C16PP", 0)], rule=W16, accept=pers("c16"), persistent=GRID, extra=[(1, 32, 64, 64, 16, 0, 16, "exact"), (2, 21, 41, 65, 16, 0, 16, "more")])
    add("b16-r32", "bf16", "conv5", "fwd", (4, 16, 16), 32, [(16, 0, 64), (8, 8, 64)], B16F, "conv_bf16_use_r32 -> conv5_bf16_r32_kernel, bricks 4x16x16, grid 256",
        rule=lambda d, h, w: w >= 16 and h >= 16, accept=pers("r32"), persistent=GRID, items=lambda c, v: _fwd16(c, v)[1].nb * (c.O // 32))
    deep = lambda c, v: _fwd16(c, v)[0] == "deep"
    dsplit = lambda c, v: _fwd16(c, v)[1].nsplit
    add("b16-deep", "bf16", "conv5", "fwd", (4, 8, 8), 32, [(64, 0, 32), (16, 16, 32), (32, 0, 64)], B16F, "conv_deep.h: plan_conv_deep, bricks 4x8x8, K over workgroups",
        opts=[("BF16_DEEP", 1)], accept=deep, split=dsplit, twin="b16-deep-off",
        observe="vnet_conv_b16_stats_rows follows plan_conv_deep under BF16_DEEP (reduce rows / 4x8x8 bricks vs the generic plan's)",
        extra=[(1, 16, 32, 32, 16, 0, 32, "nosplit"), (1, 16, 17, 8, 16, 0, 32, "rows")])
    add("b16-deep-target1", "bf16", "conv5", "fwd", (4, 8, 8), 32, [(64, 0, 32), (16, 16, 32)], B16F, "plan_conv_deep: BF16_DEEP_TARGET = 1 -> nsplit = 1, all chunks in one workgroup",
        opts=[("BF16_DEEP", 1), ("BF16_DEEP_TARGET", 1)], accept=lambda c, v: deep(c, v) and dsplit(c, v) == 1)
    add("b16-deep-off", "bf16", "conv5", "fwd", lambda W: (8, 8, 8) if W < 16 else (4, 8, 8), 32, [(64, 0, 32), (16, 16, 32), (32, 0, 64)], B16F,
        "plan_conv_deep: BF16_DEEP = 0 -> the generic kernels on the deep form's shapes", opts=[("BF16_DEEP", 0)],
        accept=lambda c, v: b16_forward(c.C0, c.C1, c.O, 0, c.B, c.D, c.H, c.W)[0] == "deep" and _fwd16(c, v)[0] == "generic")
    padf = ("conv-bf16-padded", "conv-bf16", "wgrad-bf16")
    add("b16-padded", "bf16", "conv5", "fwd", (4, 8, 16), 16, [(1, 0, 16), (3, 0, 16), (4, 0, 16)], padf,
        "conv_fwd_b16_impl: a.in4 -> conv5_bf16_c16_kernel<4,8,16,S,true> (x-im2col in LDS); ops._IN4 -> vnet_conv_fwd_b16_padded",
        flags=[("_IN4", True)], rule=W16, accept=pers("in4"), persistent=GRID)
    # ---- bf16 filter gradients: conv_b16.hip vnet_conv_wgrad_b16 ------------------------------------------------------------------
    wk = lambda name: (lambda c, v: _wg16(c, v)[0] == name)
    wsplit = lambda c, v: _wg16(c, v)[1].nsplit
    add("b16-wgrad-4x4x16", "bf16", "conv5", "wgrad", (4, 4, 16), 16, [(16, 0, 16), (16, 16, 32)], B16F, "vnet_conv_wgrad_b16: launch_wgrad_bf16<4,4,16,..>",
        opts=[("WGRAD_RR", 0)], rule=W16, accept=wk("generic"), split=wsplit, twin="b16-wgrad-rr",
        observe=NOQ % "vnet_wgrad_bf16_ws_bytes sizes the generic plan's slabs whatever WGRAD_RR / WGRAD_ZS say", extra=[(1, 4, 3, 16, 16, 0, 16, "one")])
    add("b16-wgrad-4x8x8", "bf16", "conv5", "wgrad", (4, 8, 8), 16, [(16, 0, 16), (16, 16, 32)], B16F, "vnet_conv_wgrad_b16: launch_wgrad_bf16<4,8,8,..>",
        rule=W15, accept=wk("generic"), split=wsplit, extra=[(1, 3, 8, 8, 16, 0, 16, "one")])
    add("b16-wgrad-rr", "bf16", "conv5", "wgrad", (4, 8, 32), 16, [(16, 0, 16), (16, 16, 32)], B16F, "vnet_conv_wgrad_b16: WGRAD_RR = 2 -> launch_wgrad_bf16_rr<4>, bricks 4x8x32",
        opts=[("WGRAD_RR", 2)], rule=lambda d, h, w: w >= 32 and h >= 8, accept=wk("rr"), split=wsplit, extra=[(1, 3, 8, 32, 16, 0, 16, "one")])
    add("b16-wgrad-zs", "bf16", "conv5", "wgrad", lambda W: (1, 8, 32) if W >= 32 else (2, 8, 16) if W >= 16 else (4, 8, 8), 32, [(16, 0, 32), (16, 16, 32)], B16F,
        "wgrad_zs.h: WGRAD_ZS = 1, zs_shape_ok / zs_depth_ok; columns of zs_tx(W) = 32 / 16 / 8 voxels, 32 / tx planes per step",
        opts=[("WGRAD_ZS", 1)], rule=lambda d, h, w: w >= 16 or d <= 12, accept=wk("zs"), split=wsplit, twin="b16-wgrad-4x4x16",
        observe=NOQ % "vnet_wgrad_bf16_ws_bytes sizes the generic plan's slabs whatever WGRAD_RR / WGRAD_ZS say", extra=[(1, 1, 7, 32, 16, 0, 32, "one")])
    add("b16-wgrad-in4", "bf16", "conv5", "wgrad", (4, 8, 32), 16, [(1, 0, 16), (3, 0, 16), (4, 0, 16)], padf,
        "vnet_conv_wgrad_b16: in4 = Cin_dw <= 4 and C0 == 8 and CONV_IN4 -> launch_wgrad_bf16_rr<4, true> (x-im2col form)",
        opts=[("WGRAD_RR", 2), ("CONV_IN4", 1)], flags=[("_IN4", True)], rule=lambda d, h, w: w >= 32 and h >= 8, accept=wk("rr-in4"), split=wsplit, extra=[(1, 4, 8, 32, 3, 0, 16, "one")])
    # ---- the 2^3 pair (bricks tile the COARSE volume): conv2_b16.hip, plan_conv / plan_wgrad ----------------------------------------
    d2 = ("conv2-direct",) * 2
    for mode, wf in (("fp32", "wgrad"), ("bf16", "wgrad2-b16")):
        for cf in (16, 32):
            add("%s-conv2-direct-%d" % ("f32" if mode == "fp32" else "b16", cf), mode, "pair", "fwd", (1, 1, 16), cf, [(cf, 0, 2 * cf)], d2 + (wf,),
                "conv2_b16.hip: c2_widths_ok(%d, %d); one wave per segment of 16 coarse voxels along x (segx), grid c2_grid(nseg)" % (cf, 2 * cf),
                flags=[("_DIRECT2", True)])
    add("f32-conv2-generic-wide", "fp32", "pair", "fwd", (1, 4, 16), 16, [(16, 0, 32), (8, 0, 16)], ("conv", "conv", "wgrad"),
        "plan_conv: stride 2, coarse W >= 16 -> 1x4x16 (down), 2x4x16 (up)", flags=[("_DIRECT2", False)], rule=W16)
    add("f32-conv2-generic-small", "fp32", "pair", "fwd", (2, 8, 8), 16, [(16, 0, 32), (64, 0, 128)], ("conv", "conv", "wgrad"),
        "plan_conv: stride 2, coarse W < 16 -> 2x8x8 (down); up: 8x8x8 or (tiny) 2x8x8", flags=[("_DIRECT2", False)], rule=W15)
    add("b16-conv2-wide", "bf16", "pair", "fwd", (1, 4, 16), 16, [(16, 0, 32), (8, 0, 16)], ("conv2-b16", "conv2-b16", "wgrad2-b16"),
        "conv2_b16.hip: vnet_conv2_fwd_b16 -> the fp32 MFMA kernels with IO16, plan_conv's bricks", flags=[("_DIRECT2", False)], rule=W16)
    add("b16-conv2-small", "bf16", "pair", "fwd", (2, 8, 8), 16, [(16, 0, 32), (64, 0, 128)], ("conv2-b16", "conv2-b16", "wgrad2-b16"),
        "conv2_b16.hip: vnet_conv2_fwd_b16, coarse W < 16", flags=[("_DIRECT2", False)], rule=W15)
    add("b16-wgrad2", "bf16", "pair", "wgrad", lambda W: (2, 8, 8) if W < 16 else (2, 4, 16), 16, [(16, 0, 32), (32, 0, 64)], d2 + ("wgrad2-b16",),
        "conv2_b16.hip: vnet_conv2_wgrad_b16 -> wgrad_body<2,2,2,4,16 | 2,8,8,..,true>; plan_wgrad's bricks on the coarse dy",
        split=lambda c, v: plan_wgrad(2, 2, c.C0, c.O, c.B, *c.coarse).nsplit)
    # the transposed (up) kernels -- also the backward-data of the down convolution -- have bricks of their own on the coarse INPUT
    # (plan_conv, up = 1).  No shape-only query exposes their plan (no statistics, no workspace): the rows rest on the restated planner.
    upb = lambda c: plan_conv(2, 2, 1, c.O, c.C0, c.B, *c.coarse).brick
    for pre, mode, fam in (("f32", "fp32", ("conv", "conv", "wgrad")), ("b16", "bf16", ("conv2-b16", "conv2-b16", "wgrad2-b16"))):
        add(pre + "-conv2-up-wide", mode, "pair", "up", (2, 4, 16), 16, [(16, 0, 32), (8, 0, 16)], fam,
            "plan_conv: up and coarse W >= 16 -> brick_counts<2,4,16>; launch_conv_ns<1,1,2,4,16,4,2,true>", flags=[("_DIRECT2", False)], rule=W16,
            accept=lambda c, v: upb(c) == (2, 4, 16))
        add(pre + "-conv2-up-tiny", mode, "pair", "up", (2, 8, 8), 16, [(16, 0, 32), (64, 0, 128)], fam,
            "plan_conv: up, coarse W < 16 and nb * ncob < 256 -> tiny, brick_counts<2,8,8>; launch_conv_ns<1,1,2,8,8,4,2,true>",
            flags=[("_DIRECT2", False)], rule=W15, accept=lambda c, v: upb(c) == (2, 8, 8))
        add(pre + "-conv2-up-cube", mode, "pair", "up", (8, 8, 8), 16, [(64, 0, 128)], fam,
            "plan_conv: up, coarse W < 16 and >= 256 workgroups -> brick_counts<8,8,8>; launch_conv_ns<1,1,8,8,8,8,4,true>",
            flags=[("_DIRECT2", False)], rule=W15, accept=lambda c, v: upb(c) == (8, 8, 8))
    # ---- the input block: input_block.hip ---------------------------------------------------------------------------------------
    ind = ("input-direct", None, "input-wgrad-direct")
    for o in (16, 8):
        add("input-direct-%d" % o, "fp32", "input", "fwd", (4, 4, 64), o, [(o, 0, o)], ind, "input_block.hip: IC_TZ / IC_TY / IC_TX = 4 x 4 x 64; vnet_input_conv_direct_ok(O = %d)" % o,
            flags=[("input_direct", True)], extra=[(1, 1, 9, 70, o, 0, o, "d1")])
    add("input-wgrad-direct", "fp32", "input", "wgrad", (2, 4, 64), 16, [(16, 0, 16)], ind, "input_block.hip: IW_TZ = 2: bricks 2 x 4 x 64, one slab per workgroup, at most 2 x CUs",
        flags=[("input_direct", True)], split=lambda c, v: min(v.items(c), 2 * GRID), extra=[(1, 2, 4, 1, 16, 0, 16, "w1")])
    add("input-im2col", "fp32", "input", "fwd", (4, 8, 8), 16, [(16, 0, 16), (8, 0, 8), (4, 0, 4)], ("conv", None, "wgrad"),
        "ops.route IN_FWD: x-im2col tensor + conv_fwd_impl kx = 1 -> launch_conv_ns<5,1,4,8,8,4,4,false,1>; wgrad<5,1,4,8,8 | 4,4,16,1,4,1>",
        flags=[("input_direct", False)], extra=[(1, 1, 9, 17, 16, 0, 16, "d1")])
    return collections.OrderedDict((v.name, v) for v in t)


VARIANTS = _table()

# Kernel forms in csrc/ that the sweep does NOT reach, and why (read by the host test, printed with the case table)
NOT_REACHED = {
    "fp32 4x8x16 brick (plan_conv's last branch)": "no 5^3 / 3^3 / 2^3 shape reaches it any more: W >= 16 takes 4x8x8, W < 16 the cube or the half bricks",
    "vnet_conv_wgrad_b16_group kernels WG_K2_*": "the grouped 2^3 jobs are covered by tests/test_hip_wgrad_group.py's own helper only with its random operands",
    "conv2-direct up / down kernels, z and y": "their item is a 16-voxel x segment of one coarse row (T = 1 in z and y): only the classes e = 1 and e = k exist there",
    "accumulate launches (vnet_conv_fwd_acc, acc16)": "reached only through a forked tensor's second gradient, not through a single layer's forward + backward",
}


# ---- the generator --------------------------------------------------------------------------------------------------------------
def _extent(cls, T, k):
    if cls == "lt":
        return 0 if T == 1 else max(1, T // 2 + (1 if T > 2 else 0))
    if cls == "eq":
        return T
    if T == 1:
        return k + 1 if cls == "mult" else 0
    return {"r1": k * T + 1, "rm1": k * T + T - 1, "mult": (k + 1) * T}[cls]


def classify(e, T):
    """The class of extent e against brick extent T."""
    if e < T:
        return "lt"
    if e == T:
        return "eq"
    return "mult" if e % T == 0 else "r1" if e % T == 1 else "rm1" if e % T == T - 1 else "other"


def case_classes(c):
    br = c.v.brick(c.grid_dims[2])
    return tuple(classify(e, t) for e, t in zip(c.grid_dims, br))


_KS = tuple(range(1, 9)) + (12, 16, 24, 32, 48, 64, 96, 128, 192, 256)
_WPROBE = (1, 4, 8, 15, 16, 31, 32, 64)


def _candidates(v, axis, cls, W=None):
    """Ascending extents of class cls on the axis (the brick may depend on W: x first, then z and y against the brick of that W)."""
    out = set()
    for k in _KS:
        for w in (_WPROBE if W is None else (W,)):
            T = v.brick(w)[axis]
            e = _extent(cls, T, k)
            if e > 0 and classify(e, T) == cls and (axis != 2 or v.brick(e)[2] == T):
                out.add(e)
    return sorted(out)


def _fine(v, g, odd):
    """Fine dims of a pair case from coarse ones: 2e, or 2e - 1 (odd: SAME pads one voxel on the high side)."""
    return tuple(2 * e - ((odd >> i) & 1) for i, e in enumerate(g)) if v.op == "pair" else tuple(g)


def _build(v, classes, B, ch, tag="", odd=0, cap=1 << 19, min_e=1):
    """The case of variant v with the given class per axis and the fewest voxels that the variant accepts, or None."""
    combos = []
    for W in _candidates(v, 2, classes[2]):
        for D in _candidates(v, 0, classes[0], W):
            for H in _candidates(v, 1, classes[1], W):
                if D * H * W * B <= cap and min(D, H, W) >= min_e:
                    combos.append((D * H * W, D, H, W))
    for _, D, H, W in sorted(combos):
        f = _fine(v, (D, H, W), odd)
        c = Case(v.name, B, f[0], f[1], f[2], ch[0], ch[1], ch[2], tag)
        if c.grid_dims == (D, H, W) and case_classes(c) == tuple(classes) and v.accept(c):
            return c
    return None


@functools.lru_cache(None)
def classes_of(v, axis):
    """The classes axis `axis` of variant v can realise under the variant's own shape rule (with any classes on the other axes)."""
    out = []
    for cls in CLASSES:
        for o1 in CLASSES:
            if any(_build(v, [cls if a == axis else (o1 if a == (axis + 1) % 3 else o2) for a in range(3)], 3, v.channels[0]) is not None
                   for o2 in CLASSES):
                out.append(cls)
                break
    return tuple(out)


@functools.lru_cache(None)
def generate():
    """Every case of the sweep, in a fixed order.  Raises if a variant cannot realise a class its axes list."""
    out, seen = [], set()

    def emit(c):
        if c.cid not in seen:
            seen.add(c.cid)
            out.append(c)
    for v in VARIANTS.values():
        per_axis = [classes_of(v, a) for a in range(3)]
        n = max(len(p) for p in per_axis)
        rows = [[per_axis[a][(i + a) % len(per_axis[a])] for a in range(3)] for i in range(n)]
        if all(set(RAGGED) & set(p) for p in per_axis):
            rows.append([[c for c in p if c in RAGGED][i % 2 if len([c for c in p if c in RAGGED]) > 1 else 0] for i, p in enumerate(per_axis)])
        covered = set()
        for i, cl in enumerate(rows):
            B = (2, 3, 1)[min(i, 2)]
            ch = v.channels[i % len(v.channels)]
            if v.two_src and i == 0 and not ch[1]:
                ch = next(c for c in v.channels if c[1])
            odd = (i * 3 + 5) & 7 if v.op == "pair" else 0
            # (a form that wants few or many workgroups may refuse this batch or these channels: the row's other choices, in order)
            c = next((c for c in (_build(v, cl, b, k, "", odd=odd) for b in (B, 1, 2, 3) for k in [ch] + list(v.channels)) if c is not None), None)
            if c is None:           # (a brick that depends on W: not every combination of classes is jointly realisable)
                continue
            covered.update(enumerate(cl))
            emit(c)
        for axis in range(3):       # a class the rotation missed: with whatever classes of the other axes realise it, ragged ones first
            for cls in per_axis[axis]:
                if (axis, cls) in covered:
                    continue
                pref = RAGGED + tuple(x for x in CLASSES if x not in RAGGED)
                c = next((c for c in (_build(v, [cls if a == axis else (o1 if a == (axis + 1) % 3 else o2) for a in range(3)], 1,
                                             v.channels[-1]) for o1 in pref for o2 in pref) if c is not None), None)
                if c is None:
                    raise AssertionError("variant %s cannot realise class %s on axis %d" % (v.name, cls, axis))
                covered.update(enumerate(case_classes(c)))
                emit(c)
        for B in (2, 3):            # both batch sizes, with whatever classes and channels the form takes them
            if not any(c.variant == v.name and c.B == B for c in out):
                pref = RAGGED + ("mult", "eq", "lt")
                c = next((c for c in (_build(v, [o0, o1, o2], B, k) for k in v.channels for o0 in pref for o1 in pref for o2 in pref)
                          if c is not None), None)
                if c is None:
                    raise AssertionError("variant %s has no case with batch %d" % (v.name, B))
                emit(c)
        if v.op == "pair":          # every fine extent odd and >= 3: SAME pads a real last plane / row / column, the up-conv writes onto it
            pref = RAGGED + ("mult", "eq", "lt")
            c = next((c for c in (_build(v, [o0, o1, o2], 1, v.channels[0], odd=7, min_e=2) for o0 in pref for o1 in pref for o2 in pref)
                      if c is not None), None)
            if c is None:
                raise AssertionError("variant %s has no case with three odd fine extents >= 3" % v.name)
            emit(c)
        for row in v.extra:
            emit(Case(v.name, *row))
    return tuple(out)


# ---- operands and the exact oracle ----------------------------------------------------------------------------------------------
RANGES = ((3, 2, 3), (3, 2, 2), (2, 2, 2), (2, 1, 2), (2, 1, 1), (1, 1, 1))       # (|x|, |w|, |dy|) maxima, tried in this order


def _ints(rng, m, shape):
    return rng.integers(-m, m + 1, shape).astype(np.float64)


def _draw(c, rx, rw, rdy):
    v, rng = c.v, np.random.default_rng(c.seed)
    B, (D, H, W) = c.B, c.dims
    d = {}
    if v.op == "pair":          # down: fine [.., Cf] -> coarse [.., Cc]; up: coarse [.., Cc] -> fine [.., Cf]; both filters [2,2,2,Cf,Cc]
        Cf, Cc, co = c.C0, c.O, c.coarse
        d.update(x=_ints(rng, rx, (B, D, H, W, Cf)), w=_ints(rng, rw, (2, 2, 2, Cf, Cc)), b=_ints(rng, 3, (Cc,)), dy=_ints(rng, rdy, (B,) + co + (Cc,)),
                 xu=_ints(rng, rx, (B,) + co + (Cc,)), wu=_ints(rng, rw, (2, 2, 2, Cf, Cc)), bu=_ints(rng, 3, (Cf,)), dyu=_ints(rng, rdy, (B, D, H, W, Cf)))
    elif v.op == "input":       # y = conv5(gamma * (tile(img) - mean) * invstd + beta) + b: integer gamma, mean, beta, invstd in {1, 2}
        C = c.O
        d.update(x=_ints(rng, rx, (B, D, H, W, 1)), w=_ints(rng, 1, (5, 5, 5, C, C)), b=_ints(rng, 3, (C,)), dy=_ints(rng, rdy, (B, D, H, W, C)),
                 gamma=rng.integers(1, 3, C).astype(np.float64), beta=_ints(rng, 2, (C,)), mean=_ints(rng, 2, (C,)),
                 invstd=rng.integers(1, 3, C).astype(np.float64))
    else:
        ks = 3 if v.op == "conv3" else 5
        d.update(x=_ints(rng, rx, (B, D, H, W, c.C0 + c.C1)), w=_ints(rng, rw, (ks, ks, ks, c.C0 + c.C1, c.O)), b=_ints(rng, 3, (c.O,)),
                 dy=_ints(rng, rdy, (B, D, H, W, c.O)))
    return d


def _cheap_bound(c, d):
    """An upper bound of bound(case) that needs no convolution: taps x channels x maxima for y and dx, Cauchy-Schwarz per channel pair
    for the filter gradient, the L1 norm of a channel for the bias gradient.  operands() narrows the value range with it."""
    l1 = lambda t: np.abs(t).reshape(-1, t.shape[-1]).sum(0).max()
    l2 = lambda t: np.sqrt((t.reshape(-1, t.shape[-1]) ** 2).sum(0).max())

    def one(x, w, dy, b):
        taps, wm = int(np.prod(w.shape[:3])), np.abs(w).max()
        y = taps * x.shape[-1] * np.abs(x).max() * wm + np.abs(b).max()
        dx = taps * dy.shape[-1] * np.abs(dy).max() * wm + np.abs(b).max()
        return max(y, dx, l2(x) * l2(dy), l1(dy), l1(x))
    if c.v.op == "pair":
        return max(one(d["x"], d["w"], d["dy"], d["b"]), one(d["dyu"], d["wu"], d["xu"], d["bu"]))
    if c.v.op == "input":
        C, n = c.O, d["x"].size
        xin = np.abs(d["gamma"] * d["invstd"]).max() * (np.abs(d["x"]).max() + np.abs(d["mean"]).max()) + np.abs(d["beta"]).max()
        return max(125 * C * xin * np.abs(d["w"]).max() + np.abs(d["b"]).max(), np.sqrt(n) * xin * l2(d["dy"]), l1(d["dy"]))
    return one(d["x"], d["w"], d["dy"], d["b"])


def operands(c):
    """The case's integer operands: the widest value range of RANGES whose (cheap, rigorous) bound stays within LIMIT."""
    for r in RANGES:
        d = _draw(c, *r)
        if _cheap_bound(c, d) <= LIMIT:
            d["ranges"] = r
            return d
    raise AssertionError("%s: no value range keeps the partial sums within 2^20" % c.cid)


def _t(a, grad=False):
    return torch.tensor(a, dtype=torch.float64, requires_grad=grad)


def _np(t):
    return t.detach().numpy()


def exact(c, d, magnitude=False):
    """The float64 torch oracle on the operands d: {name: exact float64 array}.  magnitude: on |operands| (bound())."""
    f = (lambda a: np.abs(a)) if magnitude else (lambda a: a)
    v = c.v
    if v.op == "pair":
        x, w, b = _t(f(d["x"]), True), _t(f(d["w"]), True), _t(f(d["b"]), True)
        y = T.convolution(x, w, b, 2)
        y.backward(_t(f(d["dy"])))
        xu, wu, bu = _t(f(d["xu"]), True), _t(f(d["wu"]), True), _t(f(d["bu"]), True)
        yu = T.deconvolution(xu, wu, bu, c.dims)
        yu.backward(_t(f(d["dyu"])))
        return dict(y=_np(y), dx0=_np(x.grad), dw=_np(w.grad), db=_np(b.grad), yu=_np(yu), dxu=_np(xu.grad), dwu=_np(wu.grad), dbu=_np(bu.grad))
    if v.op == "input":
        C = c.O
        g, be, w, b = _t(f(d["gamma"]), True), _t(f(d["beta"]), True), _t(f(d["w"]), True), _t(f(d["b"]), True)
        img, mean, inv = _t(f(d["x"])), _t(f(d["mean"])), _t(f(d["invstd"]))
        xin = g * ((img.expand(-1, -1, -1, -1, C) + mean) if magnitude else (img.expand(-1, -1, -1, -1, C) - mean)) * inv + be
        y = T.convolution(xin, w, b, 1)
        y.backward(_t(f(d["dy"])))
        return dict(y=_np(y), dw=_np(w.grad), db=_np(b.grad), dgamma=_np(g.grad), dbeta=_np(be.grad), xin=_np(xin))
    x, w, b = _t(f(d["x"]), True), _t(f(d["w"]), True), _t(f(d["b"]), True)
    y = T.convolution(x, w, b, 1)
    y.backward(_t(f(d["dy"])))
    dx = _np(x.grad)
    return dict(y=_np(y), dx0=dx[..., :c.C0], dx1=dx[..., c.C0:], dw=_np(w.grad), db=_np(b.grad))


EXACT_NAMES = ("y", "dx0", "dx1", "dw", "db", "yu", "dxu", "dwu", "dbu")        # (dgamma / dbeta of the input block: see below)


def bound(c, d):
    """max over the outputs of the oracle run on |x|, |w|, |dy|, |bias|: every partial sum of every summation order of every kernel
    is at most this.  (The input block's dgamma / dbeta are sums over ALL voxels, taps and channels -- far above 2^24 -- and are
    therefore not part of the exact comparison: the GPU test holds them to the tolerance of tests/test_hip_ops.py::test_input_block.)"""
    m = exact(c, d, magnitude=True)
    return float(max(np.abs(m[n]).max() for n in EXACT_NAMES if n in m and m[n].size))


def stored(c, a):
    """What the device stores for the exact result a: the value itself (fp32 tensors), round_bf16 of it (bf16 tensors)."""
    return O.round_bf16(a) if c.v.mode == "bf16" else a


# ---- operand profiles of the f32x3 rows: operands that fill the m and l pieces ---------------------------------------------------
# The f32x3 kernels (csrc/conv_x3.h) split an fp32 operand exactly into three bf16 pieces h = RNE(x), m = RNE(x - h), l = RNE(x - h - m)
# and form a product from the six streams hh, hm, mh, mm, hl, lh.  Integer operands are bf16-exact: m = l = 0, five streams multiply
# zeros.  The profiles below draw operands with 9+ (depth 2) and 18 (depth 3) significant bits and keep the comparison EXACT:
#
#   every operand is k * 2^-q with an integer k (q = 0 / Q2 / Q3 for depth 1 / 2 / 3), so every product of every stream is a whole
#   multiple of the launch's unit 2^-(qa + qb), and every fp32 partial sum of every summation order is exact when
#     (E1) the three dropped terms ml, lm, ll are identically zero (one side of a launch has no m or the other no l, and no l meets an l);
#     (E2) sum |a| |b| / unit < 2^24 for every output element (bound_x3: the oracle on magnitudes, per output in its own unit).
#   WHY 2^24 AND NOT THE INTEGER SWEEP'S 2^20: a depth-3 value of magnitude ~1 is at least 2^17 units, so 2^20 would leave 8 terms per
#   output, and a filter in which every (tap, input channel) is used has at least 125 Cin / Cout terms per output.  The 4 bits of margin
#   are not needed: v_mfma_f32_16x16x32_bf16 aligns the 32 products and the accumulator of an instruction to the largest term and keeps
#   at least 26 bits from that term's leading bit down -- profiles/r06_mfma_round_probe.txt: "c=0: 2^24 - 2^24 + 30 x 1.0" gives exactly
#   30 and "c=2^24, p0 = -2^24, + 2 x 1.0" exactly 2 (the unit survives 24 bits below the largest term; wrong only from 2^28), and
#   "c=1 + 32 x 0.25 ulp" gives exactly +8 ulp (terms of 2^-25 of the largest are added exactly).  With every term and the accumulator
#   below 2^24 units the unit is at most 23 bits below the largest term's leading bit: two bits inside that window.  Everything
#   outside the instruction -- sign flips, the four-wave and split-K reductions, the bias -- is plain fp32 on multiples of the unit
#   below 2^24 units: exact.
#
# A depth-3 operand is a mix: a share of 18-bit values k in [2^17, 2^18) chosen so that l != 0 ("L" elements, 2^17.6 units each), the
# rest 9-10-bit values k in [2^8, 2^10) with m != 0 (2^9.2 units): m != 0 everywhere, l != 0 in the L share.  The share is what (E2)
# pays for: an output that sums n terms against magnitude-1 partners holds n * share * 2^17.6 units, so share <= 2^24 / (n 2^17.6) / 1.6
# (the largest of many random sums lies about 1.6 x above the mean).  n is at least 125 * max(Cin, Cout) / Cout for the forward launch of a
# filter that uses every (tap, input channel) and every (tap, output channel): 34 % at n = 125, 17 % at 250, 4 % at 1000 (128 -> 16).
# L_FLOOR states that per case; a case over the limit gets sparser operands (the thinning factor), never a wider limit.
X3_LIMIT = float(1 << 24)
Q2, Q3 = 8, 17
PROFILES = ("x-deep", "w-deep", "dy-deep", "mid-dense-x", "mid-dense-w", "mid-mid")
# depth of (x, w, dy) per profile
DEPTHS = {"x-deep": (3, 1, 1), "w-deep": (1, 3, 1), "dy-deep": (1, 1, 3), "mid-dense-x": (2, 1, 1), "mid-dense-w": (1, 2, 1), "mid-mid": (2, 2, 2)}
DEEP = {"x-deep": "x", "w-deep": "w", "dy-deep": "dy", "mid-dense-x": "x", "mid-dense-w": "w"}          # the dense deep operand
QOF = {1: 0, 2: Q2, 3: Q3}
M_FLOOR = 0.90                             # share of the deep operand's elements with m != 0 (the draws give 100 %)
MEAN_L, MEAN_M = 1.5 * 2.0 ** 17, 1.5 * 2.0 ** 9     # mean |k| of an L element, of a two-piece element


def x3_cases():
    return tuple(c for c in generate() if c.v.mode == "x3")


def x3_runs():
    """[(case, profile)] that the tests run: every f32x3 case under the three deep profiles; the mid-dense and mid-mid profiles on one
    case per row, the one with the most ragged axes (all three, except on the narrow rows, whose x extent is always 8) -- measured,
    all 51 cases under all six profiles cost 57 % of the rest of the GPU suite, and the rule is a quarter."""
    cs = x3_cases()
    ragged = {}
    for c in cs:
        n = sum(k in RAGGED for k in case_classes(c))
        if c.variant not in ragged or n > ragged[c.variant][0]:
            ragged[c.variant] = (n, c)
    keep = set(c for _, c in ragged.values())
    return tuple((c, p) for c in cs for p in PROFILES if p in ("x-deep", "w-deep", "dy-deep") or c in keep)


def split3_np(a):
    """(h, m, l) of the f32x3 split, restated: three successive round-to-nearest-even bf16 roundings (float64 arrays)."""
    h = O.round_bf16(a)
    m = O.round_bf16(a - h)
    return h, m, O.round_bf16(a - h - m)


def _signs(rng, shape):
    return rng.integers(0, 2, shape) * 2.0 - 1.0


def _two_piece(rng, shape, hi=10):
    """k in [2^8, 2^hi) with m != 0, random sign (units of the caller's 2^-q)."""
    k = rng.integers(1 << 8, 1 << hi, shape).astype(np.float64)
    for _ in range(64):
        bad = split3_np(k)[1] == 0
        if not bad.any():
            break
        k[bad] = rng.integers(1 << 8, 1 << hi, int(bad.sum()))
    return k * _signs(rng, shape)


def _three_piece(rng, shape):
    """k in [2^17, 2^18) with l != 0, random sign."""
    k = rng.integers(1 << 17, 1 << 18, shape).astype(np.float64)
    for _ in range(256):
        bad = split3_np(k)[2] == 0
        if not bad.any():
            break
        k[bad] = rng.integers(1 << 17, 1 << 18, int(bad.sum()))
    return k * _signs(rng, shape)


def _deep3(rng, shape, share):
    """Depth 3, dense: L elements with probability `share`, two-piece elements elsewhere; in units of 2^-Q3."""
    k = _two_piece(rng, shape)
    mask = rng.random(shape) < share
    k[mask] = _three_piece(rng, int(mask.sum()))
    return k * 2.0 ** -Q3


def _deep2(rng, shape, share=1.0, hi=10):
    """Depth 2: two-piece elements with probability `share`, one-piece fill (|k| <= 3) elsewhere; in units of 2^-Q2."""
    k = rng.integers(1, 4, shape).astype(np.float64) * _signs(rng, shape)
    mask = rng.random(shape) < share
    k[mask] = _two_piece(rng, int(mask.sum()), hi)
    return k * 2.0 ** -Q2


def _bricks_of(shape, brick):
    B, D, H, W = shape[:4]
    return B * cdiv(D, brick[0]) * cdiv(H, brick[1]) * cdiv(W, brick[2])


def _sparse(rng, shape, density, brick, vals, per_channel=None):
    """A sparse [B, D, H, W, C] tensor of the values vals(rng, n): one non-zero in every brick of the tiling (at a random voxel and
    channel of the brick; per_channel caps how many of these a channel may carry -- bricks past the cap stay empty and are counted by
    empty_bricks()), plus independent non-zeros with probability `density`."""
    B, D, H, W, C = shape
    mask = rng.random(shape) < density
    nb = _bricks_of(shape, brick)
    ncover = nb if per_channel is None else min(nb, max(1, int(per_channel)) * C)
    ids = rng.permutation(nb)[:ncover]
    nz, ny, nx = cdiv(D, brick[0]), cdiv(H, brick[1]), cdiv(W, brick[2])
    bx, r = ids % nx, ids // nx
    by, r = r % ny, r // ny
    bz, b = r % nz, r // nz
    lo = lambda i, t, e: i * t + (rng.random(len(ids)) * np.minimum(t, e - i * t)).astype(np.int64)
    mask[b, lo(bz, brick[0], D), lo(by, brick[1], H), lo(bx, brick[2], W), np.arange(len(ids)) % C] = True
    a = np.zeros(shape)
    a[mask] = vals(rng, int(mask.sum()))
    return a


def _cover(rng, shape, n, brick, vals):
    """A sparse tensor with about n non-zeros per channel (what (E2) lets one element of the filter gradient sum): 30 % of them go to
    one voxel per brick, the rest anywhere; where the bricks outnumber that, their part grows to at most half -- density first -- and
    only past that do bricks stay empty (the host test caps their share)."""
    M, C = int(np.prod(shape[:4])), shape[4]
    nb = _bricks_of(shape, brick)
    if 0.3 * n * C >= nb:
        return _sparse(rng, shape, min(1.0, 0.7 * n / M), brick, vals, 0.3 * n)
    part = min(0.5, 1.05 * nb / (n * C))
    return _sparse(rng, shape, min(1.0, (1.0 - part) * n / M), brick, vals, part * n)


def empty_bricks(a, brick):
    """Share of the tiling's bricks in which the [B, D, H, W, C] tensor a is zero everywhere."""
    B, D, H, W, C = a.shape
    nzv = np.abs(a).max(-1) > 0
    pad = [(0, 0)] + [(0, rup(e, t) - e) for e, t in zip((D, H, W), brick)]
    nzv = np.pad(nzv, pad).reshape(B, rup(D, brick[0]) // brick[0], brick[0], rup(H, brick[1]) // brick[1], brick[1], rup(W, brick[2]) // brick[2], brick[2])
    return 1.0 - float(nzv.any(axis=(2, 4, 6)).mean())


def _filter_cover(rng, Cin, O_, vals):
    """A sparse [5, 5, 5, Cin, O] filter with the fewest non-zeros in which every (tap, input channel) has a weight for some output
    channel and every (tap, output channel) one for some input channel: per tap, max(Cin, O) weights on a rotated diagonal."""
    w = np.zeros((125, Cin, O_))
    n = max(Cin, O_)
    j = np.arange(n)
    for t in range(125):
        s = int(rng.integers(0, n))
        w[t, j % Cin, (j + s) % O_] = vals(rng, n)
    return w.reshape(5, 5, 5, Cin, O_)


def _unit_ints(rng, n):
    return _signs(rng, n)


def l_floor(c, profile):
    """The share of l != 0 elements the case's deep operand must reach: 20 %, or what (E2) leaves -- see the header of this section."""
    Cin = c.C0 + c.C1
    n = {"x-deep": 125 * max(Cin, c.O) // c.O, "dy-deep": 125 * max(Cin, c.O) // Cin}.get(profile)
    if n is None:
        return 0.20 if profile == "w-deep" else 0.0
    return min(0.20, 0.5 * X3_LIMIT / (1.6 * n * MEAN_L))


def _draw_x3(c, profile, thin):
    """The operands of (case, profile) at thinning factor `thin` (1 = the design sizes; operands_x3 lowers it until (E2) holds)."""
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (c.cid, profile)).encode()))
    B, (D, H, W), Cin, Co = c.B, c.dims, c.C0 + c.C1, c.O
    xs, ys, M = (B, D, H, W, Cin), (B, D, H, W, Co), B * D * H * W
    brick = x3_brick(W)
    budget = X3_LIMIT * thin / 1.6                       # the expected units of an output's sum of magnitudes
    nfw, nbw = 125 * max(Cin, Co) // Co, 125 * max(Cin, Co) // Cin      # terms of a forward / backward-data output against the cover filter
    share3 = lambda n: float(min(0.5, max(0.0, (budget / n - MEAN_M) / MEAN_L)))
    ones = lambda sh: _signs(rng, sh)
    if profile == "x-deep":
        p = share3(nfw)
        x = _deep3(rng, xs, p)
        w = _filter_cover(rng, Cin, Co, _unit_ints)
        ndy = budget / (p * MEAN_L + MEAN_M)              # non-zeros of a dy channel: the terms of a filter-gradient element
        dy = _cover(rng, ys, ndy, brick, _unit_ints)
    elif profile == "dy-deep":
        p = share3(nbw)
        dy = _deep3(rng, ys, p)
        w = _filter_cover(rng, Cin, Co, _unit_ints)
        nx_ = budget / (p * MEAN_L + MEAN_M)
        x = _cover(rng, xs, nx_, brick, _unit_ints)
    elif profile == "w-deep":
        p = 0.3
        w = _deep3(rng, (5, 5, 5, Cin, Co), p)
        per = budget / (p * MEAN_L + MEAN_M)              # non-zero partners in an output's receptive field
        x = _sparse(rng, xs, min(1.0, per / (125 * Cin)), brick, _unit_ints)
        dy = _sparse(rng, ys, min(1.0, per / (125 * Co)), brick, _unit_ints)
    elif profile == "mid-dense-x":                        # x two-piece everywhere; w and dy integers, dense where (E2) lets them
        x = _deep2(rng, xs)
        w = _sparse(rng, (1, 5, 5, 5, Cin * Co), min(1.0, budget * 1.4 / (125 * Cin * MEAN_M)), (1, 1, 1), _unit_ints).reshape(5, 5, 5, Cin, Co)
        dy = _sparse(rng, ys, min(1.0, budget * 1.4 / (M * MEAN_M)), brick, _unit_ints)
    elif profile == "mid-dense-w":                        # w two-piece everywhere; x and dy integers
        w = _deep2(rng, (5, 5, 5, Cin, Co))
        x = _sparse(rng, xs, min(1.0, budget * 1.4 / (125 * Cin * MEAN_M)), brick, _unit_ints)
        dy = _sparse(rng, ys, min(1.0, budget * 1.4 / (125 * Co * MEAN_M)), brick, _unit_ints)
    elif profile == "mid-mid":                            # all two-piece (k < 2^9): x a share of the tile, w the cover filter, dy sparse
        mm = (1.5 * 2.0 ** 8) ** 2                        # units of one mm product
        two = lambda r, n: _two_piece(r, n, 9) * 2.0 ** -Q2
        p = float(min(1.0, budget / (nfw * mm)))
        x = _deep2(rng, xs, p, 9)
        w = _filter_cover(rng, Cin, Co, two)
        ndy = budget / (p * mm + 2 * 1.5 * 2.0 ** 8)
        dy = _cover(rng, ys, ndy, brick, two)
    else:
        raise KeyError(profile)
    return dict(x=x, w=w, dy=dy, b=_ints(rng, 3, (Co,)))


def bound_x3(c, d, profile):
    """(E2): {output: max over its elements of sum |a| |b| in the output's own unit} -- the oracle on magnitudes.  db is left out where
    dy is the dense deep operand (it is no f32x3 product and is held to a counted bound instead)."""
    qx, qw, qdy = (QOF[k] for k in DEPTHS[profile])
    m = exact(c, d, magnitude=True)
    out = {"y": np.abs(m["y"]).max() * 2.0 ** (qx + qw), "dw": np.abs(m["dw"]).max() * 2.0 ** (qx + qdy),
           "dx": max(np.abs(m["dx0"]).max(), np.abs(m["dx1"]).max() if m["dx1"].size else 0.0) * 2.0 ** (qdy + qw)}
    if profile != "dy-deep":
        out["db"] = np.abs(m["db"]).max() * 2.0 ** qdy
    return out


THINS = tuple(0.75 ** i for i in range(16))


@functools.lru_cache(4)
def operands_x3(c, profile):
    """The operands of (case, profile): the design sizes, thinned until every output's magnitude sum is below 2^24 units.  The dict
    carries 'thin' and 'bound' (bound_x3 of the operands returned)."""
    for thin in THINS:
        d = _draw_x3(c, profile, thin)
        b = bound_x3(c, d, profile)
        if max(b.values()) < X3_LIMIT:
            d["thin"], d["bound"] = thin, b
            return d
    raise AssertionError("%s %s: no thinning keeps the magnitude sums below 2^24 units" % (c.cid, profile))


def check_e1(d, profile):
    """(E1) from the restated split: the split reproduces every operand exactly within its depth, and in each launch (x, w), (dy, w),
    (x, dy) no m meets an l and no l an l.  Returns {operand: (h, m, l)}."""
    pieces = {}
    for name, depth in zip(("x", "w", "dy"), DEPTHS[profile]):
        h, m, l = split3_np(d[name])
        assert np.array_equal(h + m + l, d[name]) and np.array_equal(d[name].astype(np.float32).astype(np.float64), d[name]), name
        k = d[name] * 2.0 ** QOF[depth]
        assert np.array_equal(k, np.round(k)), (name, "not a whole number of units")
        assert depth >= 3 or not l.any(), (name, "l piece in a depth-%d operand" % depth)
        assert depth >= 2 or not m.any(), (name, "m piece in a depth-1 operand")
        pieces[name] = (h, m, l)
    for a, b in (("x", "w"), ("dy", "w"), ("x", "dy")):
        (_, ma, la), (_, mb, lb) = pieces[a], pieces[b]
        assert not (ma.any() and lb.any()) and not (la.any() and mb.any()) and not (la.any() and lb.any()), (a, b)
    return pieces


def colsum_roundings(M, C):
    """fp32 roundings on the longest path of one element through the bias gradient ops.conv's backward calls (csrc/elementwise.hip
    vnet_colsum): colsum_vec_kernel -- a thread adds its trips (the first add, to 0, is exact), block_reduce_vec halves 256 threads down
    to C / 4 -- or, where C / 4 is no power of two, colsum_generic_kernel -- thread (row group, channel) adds its trips (the first add,
    to 0, is exact), thread c then adds the G = 256 / C group sums of its channel in group order (the first, to 0, exact; C > 256: one
    row per block and trip, nothing meets); then sum_finalize_kernel sums the blocks' rows in float64 and rounds once."""
    if C % 4 == 0 and (C // 4) & (C // 4 - 1) == 0 and C // 4 <= 256:
        nq = M * (C // 4)
        nblk = max(1, min(1024, cdiv(nq // 4 + 1, 256)))
        trips = cdiv(nq, nblk * 256)
        return (trips - 1) + (256 // (C // 4)).bit_length() - 1 + 1
    nblk = max(1, min(1024, cdiv(M * C // 4 + 1, 256)))
    G = 256 // C if C <= 256 else 1
    return (cdiv(M, nblk * G) - 1) + (G - 1) + 1


def x3_table(rows):
    """The case-by-profile table of profiles/conv_sweep.txt.  rows: [(case, profile, dict(seconds, bound, m, l, empty, thin))]."""
    out = ["%-44s %-12s %5s %9s %6s %6s %6s %7s" % ("case", "profile", "thin", "bound/2^24", "m!=0", "l!=0", "empty", "seconds")]
    for c, p, r in rows:
        out.append("%-44s %-12s %5.2f %9.3f %6.3f %6.3f %6.3f %7s" % (c.cid, p, r["thin"], r["bound"] / X3_LIMIT, r["m"], r["l"], r["empty"],
                                                                      "%.2f" % r["seconds"] if "seconds" in r else "-"))
    return "\n".join(out)


# ---- routing --------------------------------------------------------------------------------------------------------------------
def launches(c):
    """[(label, family the table claims, ops.route arguments)] of the case's launches."""
    from vnet_tensorflow_amd import ops
    v, B = c.v, c.B
    b16, x3 = v.mode == "bf16", v.mode == "x3"
    out = []
    if v.op == "pair":
        fam = v.families
        for lab, up, (ci, o), (din, dout) in (("down", 0, (c.C0, c.O), (c.dims, c.coarse)), ("up", 1, (c.O, c.C0), (c.coarse, c.dims))):
            for op, f in ((ops.FWD, fam[0]), (ops.BWD, fam[1]), (ops.WGRAD, fam[2])):
                out.append(("%s %s" % (lab, op), f, (op, 2, 2, up, b16, x3, ci, 0, o, B, din, dout, True, o if up else ci)))
        return out
    if v.op == "input":
        return [("input fwd", v.families[0] if c.O in (8, 16) or v.families[0] == "conv" else "conv", (ops.IN_FWD, 5, 1, 0, False, False, 1, 0, c.O, B, c.dims, c.dims)),
                ("input wgrad", v.families[2], (ops.IN_WGRAD, 5, 1, 0, False, False, 1, 0, c.O, B, c.dims, c.dims))]
    ks = 3 if v.op == "conv3" else 5
    padded = v.families[0] == "conv-bf16-padded"
    C0, cin = (8, c.C0) if padded else (c.C0, c.C0 + c.C1)
    for op, f in zip((ops.FWD, ops.BWD, ops.WGRAD), v.families):
        out.append((op, f, (op, ks, 1, 0, b16, x3, C0, c.C1, c.O, B, c.dims, c.dims, True, cin)))
    return out


def force(c, lib_option, monkeypatch, stack):
    """The case's library options, ops switches and compute mode, undone by the three fixtures' owners."""
    from tests import util as TU
    from vnet_tensorflow_amd import ops
    for k, val in c.v.opts:
        lib_option(k, val)
    for k, val in c.v.flags:
        if k == "input_direct":
            monkeypatch.setitem(ops._FUSE, "input_direct", val)
        else:
            monkeypatch.setitem(getattr(ops, k), "on", val)
    if c.v.mode == "x3":
        stack.enter_context(TU.split3(True))


def _reduce_rows(c, Cout):
    return 0 if (Cout > 256 or 256 % Cout) else min(2048, cdiv(c.B * c.D * c.H * c.W * Cout, 256))


def expected_queries(c):
    """(Route.stats_rows, Route.ws) of the case's forward launch as the restated planners give them, None where the forward has no
    plan of its own to restate (the 2^3 pair)."""
    v, nvox = c.v, c.B * c.D * c.H * c.W
    if v.op == "pair":
        return None
    if v.op == "input" and v.families[0] == "input-direct":
        return (c.B * cdiv(c.D, 4) * cdiv(c.H, 4) * cdiv(c.W, 64), 0)
    if v.mode == "fp32":
        Cin, ks = (16, 5) if v.op == "input" else (c.C0 + c.C1, 3 if v.op == "conv3" else 5)
        p = plan_conv(ks, 1, 0, Cin, c.O, c.B, c.D, c.H, c.W, v.opt("F32_SMALL", 2))
        nslab = p.nsplit * p.nz
        rows = 0 if c.O & 3 else (_reduce_rows(c, c.O) if nslab > 1 else p.nb)
        return (rows, nslab * nvox * rup(c.O, 16) * 4 if nslab > 1 else 0)
    if v.mode == "x3":
        name, p, _ = x3_plan(c.C0 + c.C1, c.O, c.B, c.D, c.H, c.W)
        return (_reduce_rows(c, c.O) if p.nsplit > 1 else p.nb, p.nsplit * nvox * c.O * 4 if p.nsplit > 1 else 0)
    padded = v.families[0] == "conv-bf16-padded"
    C0 = 8 if padded else c.C0
    g = plan_bf16(C0 + c.C1, c.O, c.B, c.D, c.H, c.W)
    dp = plan_deep(C0, c.C1, c.O, 0, c.B, c.D, c.H, c.W)
    ws = max(g.nsplit * g.nz * nvox * rup(c.O, 32) * 4 if g.nsplit * g.nz > 1 else 0,
             dp.nsplit * nvox * rup(c.O, 32) * 4 if dp is not None and dp.nsplit > 1 else 0)
    return (b16_rows(C0, c.C1, c.O, c.B, c.D, c.H, c.W, 0, v.opt("BF16_DEEP", 1), v.opt("BF16_DEEP_TARGET", 256)), ws)


def table(cases=None, seconds=None, bounds=None):
    """The printed case table of profiles/conv_sweep.txt."""
    rows = ["%-28s %-22s %-12s %7s %-16s %9s %7s" % ("variant", "shape B x D x H x W", "C0+C1->O", "items", "classes (z,y,x)", "bound", "seconds")]
    for c in cases or generate():
        rows.append("%-28s %-22s %-12s %7d %-16s %9s %7s" % (
            c.variant + ("/" + c.tag if c.tag else ""), "%dx%dx%dx%d" % (c.B, c.D, c.H, c.W), "%d+%d->%d" % (c.C0, c.C1, c.O), c.v.items(c),
            ",".join(case_classes(c)), "%d" % bounds[c.cid] if bounds and c.cid in bounds else "-",
            "%.2f" % seconds[c.cid] if seconds and c.cid in seconds else "-"))
    return "\n".join(rows)


def pair_coverage(cases=None):
    """{variant: {(axis a, axis b): (covered class pairs, realisable class pairs)}}: what the each-choice design covers of a pairwise one."""
    out = collections.OrderedDict()
    for c in cases or generate():
        k = case_classes(c)
        d = out.setdefault(c.variant, {(0, 1): set(), (0, 2): set(), (1, 2): set()})
        for a, b in d:
            d[(a, b)].add((k[a], k[b]))
    return collections.OrderedDict((name, {ab: (len(p), len(classes_of(VARIANTS[name], ab[0])) * len(classes_of(VARIANTS[name], ab[1])))
                                           for ab, p in d.items()}) for name, d in out.items())


if __name__ == "__main__":
    print(table())
