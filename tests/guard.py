"""A guarded arena: the software guard band this project checks memory safety with (GPU AddressSanitizer, XNACK and GPU
debuggers are not available to it).

Arena(device) owns ONE uint8 buffer filled with 0xFF (NaN as fp32, NaN as bf16, -1 as int32) and carves every tensor of a launch
out of it: start 16-byte aligned and deliberately NOT 32-byte aligned (16 bytes is the only alignment include/vnet_hip.h states),
front guard ending at the first byte, back guard starting at the last byte + 1.  A guard is at least 1 MiB and at least three
z-planes of the tensor it guards (a 5^3 halo reaches two planes, two rows and two voxels in front of and behind a volume), so an
overrun of the kind these kernels can produce lands in memory the test owns and is SEEN (a volume flattened to [M, C] gets the
1 MiB floor only: the planes rule reads 5-D shapes).  check() after the launch: every guard
byte still 0xFF, no `in` tensor changed; unwritten() finds `out` elements still holding the poison.

guarded() runs PRODUCT code inside an arena: while it is active every allocation the named modules make through `torch.empty` /
`empty_like` / `zeros` / ... is carved from the arena (role `out`, poisoned), ops.workspace() returns an arena tensor of EXACTLY the
requested byte count, and every call into libvnet_hip.so is recorded; a device pointer that does not lie inside an arena tensor is
an error.  Works on CPU tensors too (tests/test_guard.py)."""
import contextlib
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xFF
MIN_GUARD = 1 << 20
ALIGN = 16
ROLES = ("in", "out", "inout", "ws")


class GuardError(AssertionError):
    pass


class _Entry(object):
    __slots__ = ("name", "role", "off", "nbytes", "front", "back", "tensor", "host", "shape", "dtype")

    def describe(self):
        return "buffer '%s' (%s, %s %s, %d bytes)" % (self.name, self.role, str(self.dtype).replace("torch.", ""), list(self.shape),
                                                      self.nbytes)


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Arena(object):
    def __init__(self, device, capacity=192 << 20, poison=GUARD, min_guard=MIN_GUARD):
        """poison: the byte `out` and `ws` tensors are pre-filled with (0xFF, or 0x00 for the second run of a determinism check);
        guards are always 0xFF."""
        self.device = torch.device(device)
        self.poison = int(poison)
        self.min_guard = int(min_guard)
        self.buf = torch.full((int(capacity),), GUARD, dtype=torch.uint8, device=self.device)
        self.entries = []
        self.cursor = 0
        self.demoted = []             # (entry point, parameter, tensor) of `in` tensors a call took as a destination

    # ---- carving -------------------------------------------------------------------------------------------------------
    def guard_bytes(self, shape, dtype):
        planes = 0
        if len(shape) == 5:
            planes = 3 * int(shape[2]) * int(shape[3]) * int(shape[4]) * _itemsize(dtype)
        return max(self.min_guard, planes)

    def tensor(self, name, shape, dtype, role, fill=None):
        """fill: the caller's values (`in`, `inout`: array-like or tensor); `out` / `ws` hold the poison, or `fill` when given."""
        assert role in ROLES, role
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = int(np.prod(shape, dtype=np.int64)) * _itemsize(dtype)
        guard = self.guard_bytes(shape, dtype)
        base = self.buf.data_ptr()
        off = self.cursor + guard
        off += -(base + off) % ALIGN
        if (base + off) % (2 * ALIGN) == 0:
            off += ALIGN                              # 16-byte aligned and no more
        if off + n + guard > self.buf.numel():
            raise GuardError("arena of %d bytes is full at '%s' (%d bytes + 2 guards of %d)" % (self.buf.numel(), name, n, guard))
        e = _Entry()
        e.name, e.role, e.off, e.nbytes, e.shape, e.dtype = name, role, off, n, shape, dtype
        e.front, e.back = (self.cursor, off), (off + n, off + n + guard)
        # (shares the arena's storage without being an autograd VIEW of it: the ops return these from custom Functions)
        e.tensor = torch.empty(0, dtype=dtype, device=self.device).set_(
            self.buf.untyped_storage(), (self.buf.storage_offset() + off) // _itemsize(dtype), shape)
        e.host = None
        if fill is not None:
            src = fill if isinstance(fill, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(fill))
            e.tensor.copy_(src.to(dtype).reshape(shape))
        elif role in ("out", "ws"):
            self.buf[off:off + n].fill_(self.poison)
        else:
            raise GuardError("'%s': an `%s` tensor needs the caller's values" % (name, role))
        if role == "in":
            e.host = self.buf[off:off + n].cpu().clone()
        self.cursor = off + n + guard
        self.entries.append(e)
        return e.tensor

    def find(self, ptr, nbytes=1):
        """The entry whose tensor holds the address range [ptr, ptr + nbytes), or None."""
        rel = int(ptr) - self.buf.data_ptr()
        for e in self.entries:
            if e.off <= rel and rel + nbytes <= e.off + max(e.nbytes, 1):
                return e
        return None

    def entry(self, name):
        return [e for e in self.entries if e.name == name][0]

    # ---- checking ------------------------------------------------------------------------------------------------------
    def _touched(self, lo, hi):
        if hi <= lo:
            return None
        bad = self.buf[lo:hi] != GUARD
        if not bool(bad.any()):
            return None
        idx = torch.nonzero(bad).reshape(-1)
        return int(idx[0]) + lo, int(idx[-1]) + lo, int(idx.numel())

    def problems(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out = []
        for e in self.entries:
            for side, (lo, hi) in (("front", e.front), ("back", e.back)):
                t = self._touched(lo, hi)
                if t is not None:
                    first, last, count = t
                    out.append("%s: %s guard touched: %d bytes changed, first at byte offset %+d, last at %+d relative to the "
                               "tensor's first byte (%s)" % (
                                   e.describe(), side, count, first - e.off, last - e.off,
                                   "%d .. %d bytes past its end" % (first - e.off - e.nbytes + 1, last - e.off - e.nbytes + 1)
                                   if side == "back" else "%d .. %d bytes before its start" % (e.off - last, e.off - first)))
            if e.role == "in":
                now = self.buf[e.off:e.off + e.nbytes].cpu()
                diff = now != e.host
                if bool(diff.any()):
                    idx = torch.nonzero(diff).reshape(-1)
                    out.append("%s: input modified: %d bytes changed, first at byte offset +%d, last at +%d" % (
                        e.describe(), int(idx.numel()), int(idx[0]), int(idx[-1])))
        return out

    def check(self):
        p = self.problems()
        if p:
            raise GuardError("\n".join(p))

    def unwritten(self, roles=("out",)):
        """[(entry, count, first element index)] of `out` tensors with elements still holding the 0xFF poison.  (An integer element
        legitimately written as -1 reads as unwritten: no kernel here writes one -- labels, predictions and masks are >= 0.)"""
        assert self.poison == GUARD, "only the 0xFF pre-fill can tell an unwritten element from a written one"
        res = []
        for e in self.entries:
            if e.role not in roles or e.nbytes == 0:
                continue
            left = (self.buf[e.off:e.off + e.nbytes].view(-1, _itemsize(e.dtype)) == GUARD).all(1)
            if bool(left.any()):
                idx = torch.nonzero(left).reshape(-1)
                res.append((e, int(idx.numel()), int(idx[0])))
        return res

    def check_written(self, roles=("out",)):
        u = self.unwritten(roles)
        if u:
            raise GuardError("\n".join("%s: %d of %d elements never written (still 0xFF), first at element %d" % (
                e.describe(), n, e.nbytes // _itemsize(e.dtype), first) for e, n, first in u))

    def snapshot(self, roles=("out", "inout")):
        """[(name, bytes)] of the result tensors in allocation order: what two runs with different pre-fills must agree on."""
        return [(e.name, self.buf[e.off:e.off + e.nbytes].cpu().numpy().copy()) for e in self.entries if e.role in roles]


def assert_same_bits(a, b):
    """Two Arena.snapshot()s of the same case, run once on 0xFF- and once on 0x00-filled scratch and outputs."""
    assert [n for n, _ in a] == [n for n, _ in b], ("the two runs allocated different tensors", [n for n, _ in a], [n for n, _ in b])
    bad = []
    for (name, x), (_, y) in zip(a, b):
        if x.shape != y.shape or not np.array_equal(x, y):
            d = np.nonzero(x != y)[0] if x.shape == y.shape else np.zeros(1, np.int64)
            bad.append("'%s': %d bytes differ between the 0xFF and the 0x00 pre-fill, first at byte +%d" % (name, d.size, int(d[0])))
    if bad:
        raise GuardError("result depends on what the memory held before:\n" + "\n".join(bad))


# ---- the C ABI as the header declares it -------------------------------------------------------------------------------------
def header_functions(path=None):
    """{name: [(parameter name, is_pointer, is_const, type text)]} of every function include/vnet_hip.h declares."""
    text = open(path or os.path.join(ROOT, "include", "vnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(vnet_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p in ("void", ""):
                continue
            name = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1]
            params.append((name, "*" in p, p.startswith("const"), p[:p.rfind(name)].strip()))
        out[m.group(1)] = params
    return out


def _is_buffer(p):
    name, ptr, _const, typ = p
    return ptr and name != "stream" and typ.replace(" ", "") != "constchar*"


def pointer_entry_points(path=None):
    """The entry points the guard-band ledger is about: a pointer parameter other than `stream` / `const char*`."""
    return {n: ps for n, ps in header_functions(path).items() if any(_is_buffer(p) for p in ps)}


def abi_pointer_table():
    """pointer_entry_points() of every header the library binds (_lib.HEADERS), merged: what RecordingLib checks calls against."""
    from vnet_tensorflow_amd import _lib
    table = {}
    for header, _sigs in _lib.HEADERS:
        table.update(pointer_entry_points(os.path.join(ROOT, header)))
    return table


# HOST pointers of the ABI (not device buffers): the job array of the grouped filter gradient, the two result ints of vnet_packed_dims,
# the values of vnet_select_bits and the ranks of vnet_list_select (both copied into the kernel's arguments)
HOST_POINTERS = {("vnet_conv_wgrad_b16_group", "jobs"), ("vnet_packed_dims", "CQ"), ("vnet_packed_dims", "NP"),
                 ("vnet_select_bits", "values"), ("vnet_list_select", "ranks")}


class RecordingLib(object):
    """Stands in for _lib.lib(): records every entry point called and requires every device pointer to lie inside the arena."""

    def __init__(self, real, arena, calls):
        self.__dict__.update(_real=real, _arena=arena, _calls=calls, _table=abi_pointer_table())

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        params = self._table.get(name)
        if params is None:
            return fn

        def call(*args):
            self._calls.append(name)
            for (pname, ptr, _const, _typ), a in zip(params, args):
                if not ptr or pname == "stream" or (name, pname) in HOST_POINTERS or a is None or not isinstance(a, int) or a == 0:
                    continue
                e = self._arena.find(a)
                if e is None:
                    raise GuardError("%s: argument `%s` (0x%x) is not a tensor of the arena" % (name, pname, a))
                if not _const and e.role == "in":          # the caller handed one of its tensors over as a destination (y +=, p -=)
                    e.role, e.host = "inout", None
                    self._arena.demoted.append((name, pname, e.name))
            return fn(*args)
        return call


class TorchProxy(object):
    """`torch` for a module under guard: fresh tensors come from the arena, everything else is torch's."""

    def __init__(self, arena):
        self.__dict__.update(_arena=arena, _n=[0])

    def __getattr__(self, name):
        return getattr(torch, name)

    def _carve(self, what, shape, dtype, device, role, fill, requires_grad=False):
        dtype = dtype or torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device("cpu")
        if device.type != self._arena.device.type:               # (meta tensors of shape inference, host staging)
            return None
        self._n[0] += 1
        t = self._arena.tensor("%s#%d" % (what, self._n[0]), shape, dtype, role, fill)
        return t.requires_grad_(True) if requires_grad else t

    @staticmethod
    def _shape(size):
        return tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)

    def empty(self, *size, dtype=None, device=None, **kw):
        t = self._carve("empty", self._shape(size), dtype, device, "out", None, kw.get("requires_grad", False))
        return t if t is not None else torch.empty(*size, dtype=dtype, device=device, **kw)

    def empty_like(self, x, **kw):
        t = self._carve("empty_like", x.shape, kw.get("dtype", x.dtype), kw.get("device", x.device), "out", None)
        return t if t is not None else torch.empty_like(x, **kw)

    def _const(self, what, value, size, dtype, device, kw):
        shape = self._shape(size)
        host = torch.full(shape, value, dtype=dtype or torch.get_default_dtype())
        t = self._carve(what, shape, dtype, device, "inout", host, kw.get("requires_grad", False))
        return t if t is not None else torch.full(shape, value, dtype=dtype, device=device, **kw)

    def full(self, size, value, dtype=None, device=None, **kw):
        host = torch.full(tuple(size), value, dtype=dtype or torch.get_default_dtype())
        t = self._carve("full", tuple(size), dtype, device, "out", host)
        return t if t is not None else torch.full(size, value, dtype=dtype, device=device, **kw)

    def full_like(self, x, value, **kw):
        return self.full(tuple(x.shape), value, dtype=kw.get("dtype", x.dtype), device=kw.get("device", x.device))

    def cat(self, tensors, dim=0):
        r = torch.cat(tensors, dim)                      # (a small vector torch assembles: copied into the arena as an input)
        t = self._carve("cat", r.shape, r.dtype, r.device, "in", r)
        return t if t is not None else r

    def zeros(self, *size, dtype=None, device=None, **kw):
        return self._const("zeros", 0, size, dtype, device, kw)

    def ones(self, *size, dtype=None, device=None, **kw):
        return self._const("ones", 1, size, dtype, device, kw)

    def zeros_like(self, x, **kw):
        return self._const("zeros_like", 0, (tuple(x.shape),), kw.get("dtype", x.dtype), kw.get("device", x.device), {})

    def ones_like(self, x, **kw):
        return self._const("ones_like", 1, (tuple(x.shape),), kw.get("dtype", x.dtype), kw.get("device", x.device), {})


class Guarded(object):
    """What guarded() yields: the arena, the list of entry points called, and arena-backed stand-ins for tests.util.g."""

    def __init__(self, arena):
        self.arena, self.calls, self.ws_requests = arena, [], []
        self._n = 0

    def g(self, a, dev=None, dtype=torch.float32):
        """tests.util.g, but the tensor is an `in` tensor of the arena."""
        self._n += 1
        a = np.ascontiguousarray(a)
        return self.arena.tensor("in#%d" % self._n, a.shape, dtype, "in", torch.as_tensor(a).to(dtype))

    def workspace(self, nbytes, device=None):
        nbytes = int(nbytes)
        self.ws_requests.append(nbytes)
        return self.arena.tensor("ws#%d" % len(self.ws_requests), (nbytes,), torch.uint8, "ws")


@contextlib.contextmanager
def guarded(arena, modules=(), g_modules=()):
    """Inside: `torch` of `modules` allocates from the arena, `g` of `g_modules` makes arena inputs, ops.workspace hands out arena
    scratch of exactly the requested size, and _lib.lib() records calls and refuses device pointers outside the arena."""
    # (model binds _lib.lib by name when it is imported: a first import inside the context would keep this context's stand-in for good)
    from vnet_tensorflow_amd import _lib, model, ops  # noqa: F401
    h = Guarded(arena)
    proxy = TorchProxy(arena)
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    real_lib = _lib.lib
    rec = RecordingLib(real_lib(), arena, h.calls)
    try:
        patch(_lib, "lib", lambda: rec)
        patch(ops, "workspace", h.workspace)
        for m in tuple(modules) + (ops,):
            patch(m, "torch", proxy)
            if getattr(m, "lib", None) is real_lib:            # (a module that imported _lib.lib by name)
                patch(m, "lib", lambda: rec)
        for m in g_modules:
            patch(m, "g", h.g)
            if hasattr(m, "g16"):
                patch(m, "g16", lambda a, dev=None: h.g(a, dev, torch.bfloat16))
        yield h
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)


# ---- the body every tests/test_hip_*_guard.py shares ----------------------------------------------------------------------------
def written_if_returned(arena, ret):
    """`written` of run_case for cases that say themselves whether an all-0xFF output element can be a written value: check if true."""
    if ret:
        arena.check_written()


def run_case(fn, dev, poison, capacity=None, written=None, modules=()):
    """fn(h) inside a guarded arena pre-filled with `poison`; guards and inputs checked, and on the 0xFF pre-fill every output element
    written: arena.check_written(), or written(arena, what fn returned).  -> (snapshot, entry points called)"""
    arena = Arena(dev, poison=poison) if capacity is None else Arena(dev, capacity=capacity, poison=poison)
    with guarded(arena, modules=modules) as h:
        ret = fn(h)
        arena.check()
        if poison == GUARD:
            if written is None:
                arena.check_written()
            else:
                written(arena, ret)
    return arena.snapshot(), h.calls


def check_case(cases, cid, dev, capacity=None, written=None, need_output=True, modules=()):
    """cases[cid] = (entry points the case must reach, fn): run on 0xFF, then on 0x00, and require the same bits."""
    entries, fn = cases[cid]
    snap_ff, calls = run_case(fn, dev, GUARD, capacity, written, modules)
    missing = set(entries) - set(calls)
    assert not missing, "%s never reached %s (called: %s)" % (cid, sorted(missing), sorted(set(calls)))
    if need_output:
        assert snap_ff, "no output was carved from the arena"
    snap_00, _ = run_case(fn, dev, 0x00, capacity, written, modules)
    assert_same_bits(snap_ff, snap_00)
