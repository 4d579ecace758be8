"""torch.autograd bridges over the C ABI of libvnet_hip.so.

PyTorch is plumbing only here: it owns device memory, streams and the autograd tape; every
forward and backward computation below is a call into the HIP library on the current stream.
There is no CPU or eager-PyTorch fallback -- non-GPU tensors raise (meta tensors are accepted
for shape inference only, so a network can create its variables before the first batch).
"""
import collections
import contextlib
import ctypes
import math
import os as _os
import threading
import weakref

import torch

from . import _lib
from ._lib import VnetHipError, check

BN_EPS = 1e-3        # reference networks.py:259 epsilon=0.001
BN_MOMENTUM = 0.99   # reference networks.py:259 momentum=0.99

ACT = {None: 0, "none": 0, "relu": 1, "prelu": 2, "lrelu": 3}
PACK_FWD, PACK_BWD, PACK_UP, PACK_FWD_BF16, PACK_BWD_BF16, PACK_BOTH_BF16, PACK_BOTH = 0, 1, 2, 3, 4, 5, 6
PACK_FWD_X3, PACK_BWD_X3, PACK_BOTH_X3 = 7, 8, 9

# Arithmetic of the 5x5x5 convolutions (forward, backward-data and filter gradient): "fp32" = exact fp32 MFMA (the reference's
# arithmetic), "bf16" = operands rounded to bf16, fp32 accumulation (BASELINE config C5).  Everything else
# (2^3 down/up convolutions, the fused 1-channel input block, batch-norm, loss, optimiser) is fp32 in both modes.
#   "bf16"          (round 3, BASELINE config C5 as SURVEY 8(d) states it): bf16 STORAGE -- activations, skip tensors and their
#                   gradients are torch.bfloat16 tensors, every kernel on them computes in fp32 and rounds once (include/vnet_hip.h,
#                   `*_b16`); 5^3 AND 2^3 convolutions take bf16 operands; statistics, parameter gradients, logits and loss fp32.
#                   The ops below dispatch on the tensor dtype, so the mode only decides what the network input is turned into.
#   (round 2's "bf16_operands" -- fp32 tensors + bf16 shadows, bf16 operands in the 5^3 convolutions only -- was superseded by the
#   storage mode in round 3 and retired in round 5 together with its `*_x16` / `vnet_conv_*_bf16` entry points.)
# ---- per-model state (round 4) ---------------------------------------------------------------------------------------------
# What used to be process globals -- the compute dtype, the parameter-gradient stream and the registry of packed filters -- lives
# in an OpsContext.  image2label owns one and enters it around everything it runs (model.in_context), so a fp32 and a bf16 model
# can coexist in one process and interleave their steps; code that calls the ops directly (tests, tools) works on the default
# context exactly as before.  The switch is per process, not per thread: models take turns, they do not run concurrently.
class OpsContext(object):
    def __init__(self):
        self.compute = {"dtype": "fp32", "store16": False, "name": "fp32", "split3": False}
        self.pg = {"on": False, "streams": {}, "used": set(), "keep": []}
        self.pack_epoch = [0]
        self.pack_reg = {"entries": [], "descs": None, "device": None}     # every (filter, mode) ever packed: repacked in one launch


_DEFAULT_CTX = OpsContext()
_CTX = [_DEFAULT_CTX]
_TEST = {"test_delay": 0}          # (tests) cycles the parameter-gradient stream is held back per layer; shared by every context


class context(object):
    """with ops.context(ctx): ... -- the ops inside use ctx's compute dtype, parameter-gradient stream and pack registry."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.prev = _CTX[0]
        _CTX[0] = self.ctx
        return self.ctx

    def __exit__(self, *a):
        _CTX[0] = self.prev


def current_context():
    return _CTX[0]


class _CtxDict(object):
    """dict-like view of one attribute of the CURRENT context (keeps the module-level names the ops were written with)."""

    def __init__(self, attr, shared=()):
        self._attr, self._shared = attr, shared

    def _d(self, k=None):
        return _TEST if k in self._shared else getattr(_CTX[0], self._attr)

    def __getitem__(self, k):
        return self._d(k)[k]

    def __setitem__(self, k, v):
        self._d(k)[k] = v

    def __delitem__(self, k):
        del self._d(k)[k]

    def __contains__(self, k):
        return k in self._d(k)

    def get(self, k, default=None):
        return self._d(k).get(k, default)


_COMPUTE = _CtxDict("compute")
PACK_ROUND16 = 16


def set_compute_dtype(dtype):
    if dtype not in ("fp32", "fp32_split3", "bf16"):
        raise VnetHipError("compute dtype must be 'fp32', 'fp32_split3' or 'bf16', got %r" % (dtype,))
    _COMPUTE["dtype"] = "fp32" if dtype in ("fp32", "fp32_split3") else "bf16"
    _COMPUTE["store16"] = dtype == "bf16"
    # "fp32_split3" (round 5, csrc/conv_x3.h): fp32 tensors and fp32 accuracy, but the 5^3 convolutions form every product from six
    # bf16 products of exactly split operands (x = h + m + l) on the bf16 matrix pipe; layers the f32x3 kernels do not take
    # (vnet_conv_x3_ok) keep the fp32 MFMA kernels
    _COMPUTE["split3"] = dtype == "fp32_split3"
    _COMPUTE["name"] = dtype


def get_compute_dtype():
    return _COMPUTE["name"]


def storage_is_bf16():
    return _COMPUTE["store16"]


def _is16(t):
    return t is not None and t.dtype == torch.bfloat16
LOSS_KIND = {"sorensen": 0, "jaccard": 1, "xent": 2}
LOSS_WEIGHTED, LOSS_MIXED = 16, 32


def _ptr(t):
    return t.data_ptr() if t is not None else None      # ctypes converts an int to the declared c_void_p itself


_LAUNCH_ON = [None]      # raw handle of the stream the next launches go to instead of torch's current one (parameter-gradient stream)


def _raw_stream():
    """Handle of the stream kernels are launched on: torch's current stream on the current device, unless the
    parameter-gradient section redirected launches.  (torch.cuda.current_stream() builds a Stream object through three Python
    layers, ~8 us, and a torch.cuda.stream() context costs ~20 us; this is called for every kernel launch.)"""
    h = _LAUNCH_ON[0]
    return h if h is not None else torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _stream():
    return _raw_stream()


def _thread_stream(device):
    """torch's current stream of the CALLING thread on `device`, never the _LAUNCH_ON redirect: for the ops that also run on loader
    threads, inside side_work."""
    return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch._C._cuda_getDevice())


# ---- device-resident step state (include/vnet_hip.h: vnet_step_state_set) ---------------------------------
# A captured hipGraph freezes kernel arguments; the learning rate, Adam's bias-corrected lr_t and the dropout stream
# position live in a 32-byte device buffer that one tiny eager kernel rewrites before each replay.
_STEP_STATE = {"buf": {}, "active": None}


def step_state(device):
    buf = _STEP_STATE["buf"].get(device)
    if buf is None:
        buf = torch.zeros(32, dtype=torch.uint8, device=device)
        _STEP_STATE["buf"][device] = buf
    return buf


def set_step_state(state, lr, lr_t, step):
    check(_lib.lib().vnet_step_state_set(_ptr(state), float(lr), float(lr_t), int(step), _stream()), "vnet_step_state_set")


@contextlib.contextmanager
def use_step_state(state):
    """Inside: dropout takes its per-step seed offset from `state` (graph-replayable) instead of a host counter."""
    prev = _STEP_STATE["active"]
    _STEP_STATE["active"] = state
    try:
        yield
    finally:
        _STEP_STATE["active"] = prev


def _need_gpu(t, what, allow16=False, any_dtype=False):
    if not t.is_cuda:
        raise VnetHipError("%s: tensor on %s -- the HIP library is the only compute path (no CPU fallback)" % (what, t.device))
    if not any_dtype and t.dtype != torch.float32 and not (allow16 and t.dtype == torch.bfloat16):
        raise VnetHipError("%s: expected float32%s, got %s" % (what, " or bfloat16" if allow16 else "", t.dtype))


# ---- workspace (caller-owned, per device) -----------------------------------------------------
_WS = {}
_WS_RETIRED = []


def workspace(nbytes, device):
    """One scratch buffer per (device, stream): launches on the parameter-gradient stream never share scratch
    with the main stream's launches."""
    nbytes = int(nbytes)
    key = (device, _raw_stream())
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            # never hand a scratch buffer back: launches on a redirected stream may still be using it (the allocator files the
            # block under torch's current stream), and a captured step graph replays launches that hold its ADDRESS (ADVICE r2:
            # an eager step that needs more scratch after the capture would otherwise free memory the graph still writes)
            _WS_RETIRED.append(buf)
        buf = torch.empty(max(nbytes, 1 << 20) * 5 // 4, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


# ---- parameter-gradient stream --------------------------------------------------------------------------
# The backward critical path is  batch-norm backward -> backward-data conv -> next layer; filter and bias gradients
# only feed the optimiser / the gradient all-reduce.  With this switch on they are enqueued on a second HIP stream,
# so their MFMA work fills the chip while the critical path sits in its short HBM- and latency-bound kernels.
# Only gradients that go straight into the flat gradient buffer (GradSink) take this route.
_PG = _CtxDict("pg", shared=("test_delay",))


def set_param_grad_stream(on):
    _PG["on"] = bool(on)


def param_grad_stream(device, create=True):
    if not _PG["on"]:
        return None
    st = _PG["streams"].get(device)
    if st is None and create:
        st = torch.cuda.Stream(device=device)
        _PG["streams"][device] = st
    return st


def join_param_grad_stream(device=None):
    """Make the current stream wait for every parameter gradient enqueued so far (call before reading gradients)."""
    for dev in list(_PG["used"]):
        if device is None or dev == device:
            torch.cuda.current_stream(dev).wait_stream(_PG["streams"][dev])
            _PG["used"].discard(dev)
    if not _PG["used"]:
        _PG["keep"] = []


# ---- packed-weight cache -------------------------------------------------------------------------
_PACK_EPOCH = _CtxDict("pack_epoch")
_PACK_REG = _CtxDict("pack_reg")


def invalidate_packed():
    """Call after parameters change outside autograd's version counter (optimiser kernels)."""
    _PACK_EPOCH[0] += 1


def _pack_tag(w):
    return (_PACK_EPOCH[0], w._version, w.data_ptr())


def packed_weights(w, mode, taps, I, O):
    """MFMA-fragment-ordered copy of a filter, cached ON the tensor object (a cache keyed by
    data_ptr would go stale when the allocator recycles an address)."""
    cache = getattr(w, "_vnet_packed", None)
    if cache is None:
        cache = {}
        w._vnet_packed = cache
    key = (mode, taps, I, O)
    ent = cache.get(key)
    tag = _pack_tag(w)
    if ent is not None and ent[0] == tag:
        return ent[1]
    L = _lib.lib()
    if ent is None:
        wp = torch.empty(L.vnet_packed_weight_floats(mode, taps, I, O), dtype=torch.float32, device=w.device)
        if isinstance(w, torch.nn.Parameter):                  # long-lived filter: join the batched repack
            _PACK_REG["entries"].append((weakref.ref(w), key, wp))
            _PACK_REG["descs"] = None
    else:
        wp = ent[1]
    check(L.vnet_pack_weights(mode, _ptr(w), _ptr(wp), taps, I, O, _stream()), "vnet_pack_weights")
    cache[key] = (tag, wp)
    return wp


def repack_registered():
    """After an optimiser step: refresh the packed copy of every registered filter in ONE kernel launch
    (instead of ~58 small launches spread over the next forward/backward pass)."""
    reg = _PACK_REG
    alive = [(r(), key, wp) for r, key, wp in reg["entries"]]
    if any(w is None for w, _, _ in alive):                     # networks that were garbage-collected
        reg["entries"] = [(r, key, wp) for (r, key, wp), (w, _, _) in zip(reg["entries"], alive) if w is not None]
        reg["descs"] = None
    ents = [e for e in alive if e[0] is not None]
    if not ents:
        return
    L = _lib.lib()
    dev = ents[0][0].device
    ptrs = tuple(w.data_ptr() for w, _, _ in ents)
    if reg["descs"] is None or reg.get("ptrs") != ptrs:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise VnetHipError("the packed-filter registry changed inside a stream capture (a network was garbage-collected or "
                               "a new filter appeared): call ops.settle_pack_registry() before capturing")
        rows = []
        # a filter with BOTH bf16 images registered (forward + backward-data: every 5^3 filter of a bf16 training step) and whole
        # 32-channel blocks: one descriptor, one read of w for the two images (VNET_PACK_BOTH_BF16; -0.06 ms per C5 step)
        both = {}
        fams = {PACK_FWD_BF16: 0, PACK_BWD_BF16: 0, PACK_FWD: 1, PACK_BWD: 1,       # (the plain fp32 pair the same way: VNET_PACK_BOTH;
                PACK_FWD_X3: 2, PACK_BWD_X3: 2}                                    #  the f32x3 pair: VNET_PACK_BOTH_X3, round 6)
        for w, (mode, taps, I, O), wp in ents:
            if mode in fams and I % 32 == 0 and O % 32 == 0:
                both.setdefault((w.data_ptr(), fams[mode]), {})[mode] = wp
        done = set()
        for w, (mode, taps, I, O), wp in ents:
            key = (w.data_ptr(), fams.get(mode))
            pair = both.get(key, {})
            if mode in fams and len(pair) == 2 and I % 32 == 0 and O % 32 == 0:
                if key not in done:
                    done.add(key)
                    f, bk, mb = ((PACK_FWD_BF16, PACK_BWD_BF16, PACK_BOTH_BF16), (PACK_FWD, PACK_BWD, PACK_BOTH),
                                 (PACK_FWD_X3, PACK_BWD_X3, PACK_BOTH_X3))[fams[mode]]
                    rows.append([w.data_ptr(), pair[f].data_ptr(), mb, taps, I, O, pair[bk].data_ptr(), 0])
                continue
            cq, npad = ctypes.c_int(), ctypes.c_int()
            check(L.vnet_packed_dims(mode, taps, I, O, ctypes.byref(cq), ctypes.byref(npad)), "vnet_packed_dims")
            rows.append([w.data_ptr(), wp.data_ptr(), mode, taps, I, O, cq.value, npad.value])
        reg["descs"] = torch.tensor(rows, dtype=torch.int64).to(dev)
        reg["nrows"] = len(rows)
        reg["ptrs"] = ptrs
    check(L.vnet_pack_weights_batched(_ptr(reg["descs"]), reg["nrows"], _stream()), "vnet_pack_weights_batched")
    for w, key, wp in ents:
        w._vnet_packed[key] = (_pack_tag(w), wp)


def settle_pack_registry():
    """Before a stream capture: collect garbage (torch.cuda.graph does it on entry anyway -- a network that dies THERE would
    change the registry inside the capture), drop dead filters and rebuild the descriptor table now, while host-to-device
    copies are still allowed."""
    import gc
    gc.collect()
    repack_registered()


def clear_pack_registry():
    _PACK_REG["entries"] = []
    _PACK_REG["descs"] = None


def _same_out(n, s):
    return -(-n // s)


# ---- gradient sinks ---------------------------------------------------------------------------------
class GradSink(object):
    """Registered on a Parameter by optim.FlatParams: backward kernels write that parameter's gradient
    straight into its slice of the flat gradient buffer (no temporary, no autograd accumulate kernel) and
    then call `ready` (the data-parallel bucket countdown).  `written` guards against a parameter that is
    used twice in one backward pass: the second use falls back to autograd's accumulation."""
    __slots__ = ("view", "written", "ready", "ws")

    def __init__(self, view):
        self.view, self.written, self.ready = view, False, None
        self.ws = None           # this parameter's own slab buffer of the deferred filter-gradient reduce (lives as long as the sink)


def _grad_out(p):
    s = getattr(p, "_vnet_sink", None)
    if s is not None and not s.written:
        return s.view, s
    return torch.empty_like(p), None


def _grad_ret(t, s):
    if s is None:
        return t
    s.written = True
    if s.ready is not None:
        s.ready()
    return None


# ---- optional per-launch timing (bench.py): HIP events on the launch stream ---------------------
_PROFILE = {"on": False, "records": [], "only": None}


def profile_start(only=None):
    """`only`: set of launch tags to time (None = every conv-family launch).  Each timed launch costs two event
    packets on the stream (~5.6 us of idle GPU each on MI355X), so a throughput run times only the kernels it reports."""
    _PROFILE["records"] = []
    _PROFILE["only"] = set(only) if only is not None else None
    _PROFILE["on"] = True


def profile_stop():
    """Returns [(tag, flops, algorithmic_bytes, milliseconds)] after synchronising."""
    _PROFILE["on"] = False
    torch.cuda.synchronize()
    out = [(t, f, b, e0.elapsed_time(e1)) for (t, f, b, e0, e1) in _PROFILE["records"]]
    _PROFILE["records"] = []
    return out


def _timed_tag(tag):
    return _PROFILE["on"] and (_PROFILE["only"] is None or tag in _PROFILE["only"])


class _Timed(object):
    """HIP events around one launch.  Not under stream capture: on this runtime (ROCm 7.0 libamdhip64 bundled with torch
    2.10) an event recorded into a capture cannot be timed afterwards -- hipEventRecordWithFlags(hipEventRecordExternal)
    is refused with hipErrorInvalidValue and hipEventElapsedTime on captured events returns hipErrorInvalidHandle
    (profiles/probes/graph_event_probe.py) -- so bench.py times the reported kernel family in eager steps."""

    def __init__(self, tag, flops, nbytes):
        self.rec = (tag, flops, nbytes)
        self.on = _timed_tag(tag) and not torch.cuda.is_current_stream_capturing()

    def __enter__(self):
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()          # torch's current stream == the stream the kernel is launched on
        return self

    def __exit__(self, *a):
        if self.on:
            self.e1.record()
            _PROFILE["records"].append(self.rec + (self.e0, self.e1))


# ---- convolution routing ---------------------------------------------------------------------------
# Every launch of the convolution family -- forward, backward-data and filter gradient of _ConvFn, the fused input block -- is chosen
# by route() and only there: the statistics buffer a forward needs, the side-stream guard of a filter gradient and the launch itself
# all read the one record it returns.
FWD, BWD, WGRAD, IN_FWD, IN_WGRAD = "fwd", "bwd", "wgrad", "input-fwd", "input-wgrad"
# (tests / A-B runs; read by route() alone)  _X3 force: the f32x3 kernels for every shape they can run, not only where they pay;
# _IN4: the zero-padded bf16 network input through vnet_conv_fwd_b16_padded;  _DIRECT2: False = the generic 2^3 kernels everywhere
_X3 = {"force": False}
_IN4 = {"on": True}
_DIRECT2 = {"on": True}


class Route(collections.namedtuple("Route", "family pack ws stats_rows tag flops nbytes ks kx stride up din dout cin")):
    """One launch as route() chose it.  family: the entry point; pack: (mode, taps, I, O) of the packed filter, None = the raw
    filter; ws: workspace bytes; stats_rows: partial batch-norm rows the forward's epilogue writes (0 = none); tag, flops, nbytes:
    the profile record.  Geometry of the launch: x [B, din, .] -> y [B, dout, .] (a filter gradient: x and dy [B, dout, .]) -- for
    a backward-data launch the forward's input and output swap roles; cin: the filter's input channels."""
    __slots__ = ()


def _nvox(dims):
    return dims[0] * dims[1] * dims[2]


def route(op, ks, stride, up, bf16, split3, C0, C1, O, B, din, dout, aligned=True, cin=0, res=False):
    """The launch for `op` of the convolution y [B, dout, O] = conv(x [B, din, C0 | C1]): ks^3 stride `stride`, or (up) the 2^3
    transposed convolution.  bf16: bf16 storage; split3: the fp32_split3 mode; aligned: the filter is 16-byte aligned; cin: the
    filter's input channels when x carries zero-padded channels behind them (the cast network input); res: a residual joins the
    epilogue statistics.  IN_FWD / IN_WGRAD: the fused 1-channel input block (C0 = 1, O outputs, din = dout)."""
    L = _lib.lib()
    din, dout = tuple(int(v) for v in din), tuple(int(v) for v in dout)
    I, kx, esz = cin or C0 + C1, 0, (2 if bf16 else 4)
    if op in (IN_FWD, IN_WGRAD):
        N = B * _nvox(din)
        if _FUSE["input_direct"] and L.vnet_input_conv_direct_ok(O, B, *din) == 1:
            # packed fp32 FMAs straight from the image: no im2col tensor, no filter repack
            fwd = op == IN_FWD
            return Route("input-direct" if fwd else "input-wgrad-direct", None,
                         0 if fwd else L.vnet_input_wgrad_direct_slabs(B, *din) * 25 * 16 * O * 4,
                         L.vnet_input_conv_direct_stats_rows(B, *din) if fwd else 0,
                         "%s %d^3x%d 1->%d" % ("input-direct" if fwd else "input-wgrad-direct", din[2], B, O),
                         2.0 * N * 125 * O, 4.0 * N * (1 + O), 5, 0, 1, 0, din, dout, 1)
        # rounds 1-5: the x-im2col tensor (16 channels) through the 5x5x1 fp32 MFMA kernels
        op, kx, I, C0, C1 = (FWD if op == IN_FWD else WGRAD), 1, 16, 16, 0
    taps = 8 if ks == 2 else ks * ks * (kx or ks)
    if op == WGRAD:
        if up:      # dw[a][o][ci] = sum_i dy[2i+a][o] * x[i][ci] == the filter gradient of the 2^3 down conv (fine dy -> coarse x)
            C0, C1, O, din, dout, up = O, 0, C0, dout, din, 0
        cx, nin, nout = C0 + C1, B * _nvox(din), B * _nvox(dout)
        if bf16:
            fam, pre = ("wgrad2-b16", "wgrad-b16") if ks == 2 else ("wgrad-bf16", "wgrad-bf16")
        elif ks == 5 and stride == 1 and kx == 0 and split3 and (
                (C0 % 16 == 0 and C1 % 16 == 0 and O % 16 == 0) if _X3["force"] else L.vnet_wgrad_x3_ok(C0, C1, O, B, *din) == 1):
            fam = pre = "wgrad-x3"
        else:
            fam = pre = "wgrad"
        ws = (L.vnet_wgrad_x3_ws_bytes(cx, O, B, *din) if fam == "wgrad-x3" else
              L.vnet_wgrad_bf16_ws_bytes(cx, O, B, *din) if fam == "wgrad-bf16" else
              L.vnet_wgrad_ws_bytes(ks, kx, stride, cx, O, B, *dout))
        # (the 2^3 bf16 kernel counts the fine tensor as 8 voxels per coarse one)
        nbytes = esz * ((8 * nout if fam == "wgrad2-b16" else nin) * cx + nout * O) + 4.0 * taps * cx * O
        return Route(fam, None, ws, 0, "%s k%d%s s%d %d^3x%d %d->%d" % (pre, ks, "x%d" % kx if kx else "", stride, dout[2], B, cx, O),
                     2.0 * nout * taps * cx * O, nbytes, ks, kx, stride, 0, din, dout, cx if ks == 2 else I)
    pair = ks == 2 and (bf16 or op == BWD or (C1 == 0 and (up or not res)))       # the 2^3 stride-2 down / up pair
    if op == BWD:   # backward-data: x = dy, y = dx; of a 2^3 layer the other member of the pair with the same filter
        (X0, X1), (Y0, Y1), din, dout, up = (O, 0), (C0, C1), dout, din, (not up if ks == 2 else 0)
    else:
        (X0, X1), (Y0, Y1) = (C0, C1), (O, 0)
    cx, cy, nin, nout, up = X0 + X1, Y0 + Y1, B * _nvox(din), B * _nvox(dout), int(up)
    if pair:
        Cf, Cc = (cy, cx) if up else (cx, cy)
        if _DIRECT2["on"] and L.vnet_conv2_direct_ok(Cf, Cc) and aligned:
            # levels 1-2 of the V-Net (Cf 16 / 32): the LDS-free direct kernels on the raw filter (one 16-byte load = one MFMA operand)
            fam, pack = "conv2-direct", None
        else:
            fam, pack = ("conv2-b16" if bf16 else "conv"), ((PACK_UP if up else PACK_FWD) | (PACK_ROUND16 if bf16 else 0), 8, cx, cy)
        pre = "conv-b16" if bf16 else "conv"
    elif bf16:
        fam = "conv-bf16-padded" if op == FWD and C1 == 0 and 0 < cin < C0 and _IN4["on"] else "conv-bf16"
        pack, pre = (PACK_BWD_BF16 if op == BWD else PACK_FWD_BF16, 125, I, O), "conv-bf16"
    elif ks == 5 and stride == 1 and not up and kx == 0 and split3 and (
            (X0 % 16 == 0 and X1 % 16 == 0 and Y0 % 16 == 0 and Y1 % 16 == 0) if _X3["force"] else
            L.vnet_conv_x3_ok(X0, X1, Y0, Y1, B, *dout) == 1):
        fam = pre = "conv-x3"
        pack = (PACK_BWD_X3 if op == BWD else PACK_FWD_X3, 125, I, O)
    else:
        fam = pre = "conv"
        pack = ((PACK_UP, 8, cx, cy) if up else (PACK_BWD, taps, I, O) if op == BWD else (PACK_FWD, taps, I, O))
    ws = (0 if fam == "conv2-direct" else
          L.vnet_conv_x3_ws_bytes(cx, cy, B, *dout) if fam == "conv-x3" else
          L.vnet_conv_b16_ws_bytes(X0, X1, Y0, Y1, B, *dout) if pre == "conv-bf16" else
          L.vnet_conv_ws_bytes(ks, kx, stride, up, cx, cy, B, *dout))
    rows = 0
    if op == FWD and not up and not (bf16 and pair and O % 4):
        if pre == "conv-bf16":
            rows = L.vnet_conv_b16_stats_rows(C0, C1, O, 0, B, *dout)     # (the kernels that stage bf16 sources: one row per brick)
        else:
            rows = (L.vnet_conv_x3_stats_rows(cx, O, B, *dout) if fam == "conv-x3" else          # one row per brick or reduce block
                    L.vnet_conv2_direct_stats_rows(cx, O, B, *dout) if fam == "conv2-direct" else 0)   # one row per workgroup
            if rows <= 0:
                rows = L.vnet_conv_stats_rows(ks, kx, stride, 0, cx, O, 0, B, *dout)    # the fp32 MFMA kernels' brick rows
    nbytes = (esz * (nin * cx + nout * cy) + (2.0 if pre == "conv-bf16" else 4.0) * taps * cx * cy
              + (4.0 * cy if fam in ("conv", "conv-x3") else 0))
    return Route(fam, pack, ws, max(rows, 0),
                 "%s k%d%s s%d%s %d^3x%d %d->%d" % (pre, ks, "x%d" % kx if kx else "", stride, " up" if up else "", dout[2], B, cx, cy),
                 2.0 * (nin if up else nout) * taps * cx * cy, nbytes, ks, kx, stride, up, din, dout, I)


def _conv_launch(r, x0, x1, w, bias, y0, y1=None, accum=False, stats=None, res=None, acc_src=None, wp=None):
    """Run a FWD / BWD route: y0 | y1 (+)= conv(x0 | x1) (+ bias).  stats: the epilogue's partial sums of y (+ res); acc_src: the
    bf16 kernel adds this tensor instead of y0; wp: the packed filter when the caller made it (default: w's cached image)."""
    L = _lib.lib()
    B, C0, C1 = x0.shape[0], x0.shape[-1], (x1.shape[-1] if x1 is not None else 0)
    Cy0, Cy1 = y0.shape[-1], (y1.shape[-1] if y1 is not None else 0)
    if wp is None:
        wp = packed_weights(w, *r.pack) if r.pack is not None else w
    nb, f = r.ws, r.family
    ws = workspace(nb, x0.device) if nb else None
    with _Timed(r.tag, r.flops, r.nbytes):
        if f == "conv2-direct":
            down = not r.up
            fine, coarse, Cf, Cc = (r.din, r.dout, C0, Cy0) if down else (r.dout, r.din, Cy0, C0)
            fn, what = (L.vnet_conv2_direct_b16, "vnet_conv2_direct_b16") if _is16(x0) else (L.vnet_conv2_direct_f32, "vnet_conv2_direct_f32")
            check(fn(int(down), _ptr(x0), _ptr(y0), _ptr(wp), _ptr(bias), Cf, Cc, B, *fine, *coarse, int(bool(accum)), _ptr(stats),
                     _stream()), what)
        elif f == "conv2-b16":
            check(L.vnet_conv2_fwd_b16(r.up, _ptr(x0), C0, _ptr(wp), _ptr(bias), _ptr(y0), Cy0, B, *r.din, *r.dout, int(bool(accum)),
                                       _ptr(stats), _ptr(ws), nb, _stream()), "vnet_conv2_fwd_b16")
        elif f == "conv-bf16-padded":
            check(L.vnet_conv_fwd_b16_padded(_ptr(x0), C0, r.cin, _ptr(wp), _ptr(bias), _ptr(y0), Cy0, B, *r.dout,
                                             _ptr(res), _ptr(stats), _ptr(ws), nb, _stream()), "vnet_conv_fwd_b16_padded")
        elif f == "conv-bf16":
            acc = acc_src if acc_src is not None else (y0 if accum else None)
            check(L.vnet_conv_fwd_b16(_ptr(x0), C0, _ptr(x1), C1, _ptr(wp), _ptr(bias), _ptr(y0), Cy0, _ptr(y1), Cy1, B, *r.dout,
                                      _ptr(acc), _ptr(res), _ptr(stats), _ptr(ws), nb, _stream()), "vnet_conv_fwd_b16")
        elif f == "conv-x3":
            check(L.vnet_conv_fwd_x3(_ptr(x0), C0, _ptr(x1), C1, _ptr(wp), _ptr(bias), _ptr(y0), Cy0, _ptr(y1), Cy1, B, *r.dout,
                                     _ptr(y0) if accum else None, _ptr(res), _ptr(stats), _ptr(ws), nb, _stream()), "vnet_conv_fwd_x3")
        elif stats is not None:        # the fp32 MFMA kernels with batch-norm statistics of y (+ res) from the epilogue
            check(L.vnet_conv_fwd_stats(r.ks, r.kx, r.stride, _ptr(x0), C0, _ptr(x1), C1, _ptr(wp), _ptr(bias), _ptr(y0), Cy0,
                                        B, *r.din, *r.dout, _ptr(res), _ptr(stats), _ptr(ws), nb, _stream()), "vnet_conv_fwd_stats")
        else:
            fn = L.vnet_conv_fwd_acc if accum else L.vnet_conv_fwd
            check(fn(r.ks, r.kx, r.stride, r.up, _ptr(x0), C0, _ptr(x1), C1, _ptr(wp), _ptr(bias),
                     _ptr(y0), Cy0, _ptr(y1), Cy1, B, *r.din, *r.dout, _ptr(ws), nb, _stream()), "vnet_conv_fwd")


def cast_input(img):
    """bf16-storage mode: the fp32 network input [.., Cin] as a bf16 tensor [.., Cin padded to a multiple of 8] (zero channels);
    the filters' packed images are zero-padded to 16 input channels anyway (vnet_cast_bf16).  Not differentiable: the reference's
    input is a placeholder (model.py:262)."""
    _need_gpu(img, "cast_input")
    img = img.contiguous()
    C = int(img.shape[-1])
    Cp = -(-C // 8) * 8
    y = torch.empty(img.shape[:-1] + (Cp,), dtype=torch.bfloat16, device=img.device)
    check(_lib.lib().vnet_cast_bf16(_ptr(img), _ptr(y), img.numel() // C, C, Cp, _stream()), "vnet_cast_bf16")
    return y


def colsum16(x16, C, out):
    """Per-channel fp32 sum of a bf16 channels-last tensor (bias gradients outside the networks' closed form): written by a kernel
    on the launch stream straight into `out` (a raw-pointer write like colsum(): no copy_ on torch's current stream, no version
    bump of a gradient-sink view)."""
    L = _lib.lib()
    M = x16.numel() // C
    nb = L.vnet_colsum_b16_ws_bytes(C)
    ws = workspace(nb, x16.device)
    check(L.vnet_colsum_b16(_ptr(x16), _ptr(out), M, C, _ptr(ws), nb, _stream()), "vnet_colsum_b16")
    return out


# ---- deferred reduces of the filter-gradient slabs (include/vnet_hip.h: vnet_wgrad_defer / vnet_wgrad_flush) ------------------
# Inside `deferred_wgrad_reduce()` the filter-gradient launches leave their partial slabs in a per-layer buffer and ONE batched
# launch reduces all of them when the context ends (26 reduce launches of ~7 us per V-Net step otherwise).  Only for a backward
# pass whose filter gradients nobody reads before it ends (model.image2label: not the eager data-parallel step, whose bucket
# all-reduces start from the gradient hooks).
_DEFER = {"on": False, "jobs": [], "dy_ptrs": set(), "stream": None}
# grouped launch of the 5^3 filter gradients of a deferring pass (layers up to 128^3 voxels; measured: 32^3 and below -0.23 ms,
# all levels -0.33 ms per C5 step) (bf16 storage; include/vnet_hip.h:
# vnet_conv_wgrad_b16_group).  VNET_WGRAD_GROUP=0: every layer launches its own kernel as it did through round 3.
_GROUP = {"on": _os.environ.get("VNET_WGRAD_GROUP", "1") != "0", "max_voxels": 128 ** 3, "max_bytes": 4 << 30,
          "k2": True}
# (k2: the 2^3 stride-2 filter gradients join too -- -0.05 ms per C5 step.  Round 4 also built the group for fp32 tensors and let the
#  zero-padded network input join; both measured no gain -- DESIGN 4.5 -- and were removed in round 5)


WGRAD_GROUP_TAG = "wgrad-group"


def set_wgrad_group(on):
    _GROUP["on"] = bool(on)


def _group_pinned(*tensors):
    """Byte budget of the grouped launch: the activations and gradients of every layer that joins stay alive until the
    group is launched, where autograd used to release them layer by layer; the footprint grows with the batch size.  Once the
    tensors waiting exceed `_GROUP["max_bytes"]` the layers collected so far are launched mid-pass (their slabs' reduces still join
    the one batched flush) and their tensors are let go.  An upper bound: a tensor two layers share is counted twice."""
    _DEFER["pinned"] = _DEFER.get("pinned", 0) + sum(t.numel() * t.element_size() for t in tensors if t is not None)
    if _DEFER["pinned"] > _GROUP["max_bytes"]:
        _flush_wgrad_group()


def _flush_wgrad_group(launch=True):
    """Launch the collected filter gradients (the reduces of their slabs join the deferred queue) and let go of their tensors."""
    jobs, _DEFER["jobs"] = _DEFER["jobs"], []
    _DEFER["dy_ptrs"] = set()
    _DEFER["pinned"] = 0
    if not jobs or not launch:
        return
    _launch_wgrad_group(jobs, "vnet_conv_wgrad_b16_group")


def _launch_wgrad_group(jobs, entry):
    L = _lib.lib()
    arr = (_lib.WgradJob * len(jobs))()
    for k, (x0, x1, dy, dw, ws, nb, cin_dw, B, dims, _fl, _by, ks) in enumerate(jobs):
        j = arr[k]
        j.x0, j.x1, j.dy, j.dw, j.ws, j.ws_bytes = _ptr(x0), _ptr(x1), _ptr(dy), _ptr(dw), _ptr(ws), int(nb)
        j.C0, j.C1, j.Cout, j.Cin_dw = int(x0.shape[-1]), (int(x1.shape[-1]) if x1 is not None else 0), int(dy.shape[-1]), cin_dw
        j.B, j.D, j.H, j.W, j.ks = int(B), int(dims[0]), int(dims[1]), int(dims[2]), ks
    # (a layer that is being timed on its own -- profile_start(only=...) with its tag -- has not joined; "wgrad-group" times this launch)
    with _Timed(WGRAD_GROUP_TAG, sum(j[9] for j in jobs), sum(j[10] for j in jobs)):
        check(getattr(L, entry)(ctypes.addressof(arr), len(jobs), _stream()), entry)


@contextlib.contextmanager
def deferred_wgrad_reduce(on=True):
    if not on or _DEFER["on"]:
        yield
        return
    L = _lib.lib()
    st = _stream()                            # the library's queues are per stream: this pass defers on the stream it launches on
    _DEFER["on"] = True
    _DEFER["stream"] = st
    L.vnet_wgrad_defer(1, st)
    try:
        yield
    except BaseException:
        # the pass failed (e.g. an invalidated stream capture): drain the queue without raising a SECOND error from here, so that
        # the caller sees the original one (model._train_step_graph turns a refused capture into eager steps)
        _DEFER["on"] = False
        _flush_wgrad_group(launch=False)
        L.vnet_wgrad_defer(0, st)
        L.vnet_wgrad_flush(st)
        raise
    else:
        try:
            _flush_wgrad_group()                  # (still deferring: the reduces of its slabs join the one batched launch below)
        finally:
            _DEFER["on"] = False
            L.vnet_wgrad_defer(0, st)
        check(L.vnet_wgrad_flush(st), "vnet_wgrad_flush")


def _wgrad_workspace(dw, nbytes, immediate, owner):
    """Scratch for the partial slabs: the shared workspace, or (deferred reduce) a buffer of this layer's own, kept on the
    parameter's gradient sink so that it lives exactly as long as the parameter does (a captured step graph holds its address)."""
    if not _DEFER["on"] or immediate or owner is None:
        return workspace(nbytes, dw.device)
    if owner.ws is None or owner.ws.numel() < nbytes or owner.ws.device != dw.device:
        if owner.ws is not None:
            _WS_RETIRED.append(owner.ws)          # (a captured graph may hold the old address: keep it alive, see workspace())
        owner.ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dw.device)
    return owner.ws


@contextlib.contextmanager
def _immediate_reduce(immediate):
    """A filter gradient that is consumed right away (the fused input block's G): reduce it now even inside a deferring pass."""
    if not (immediate and _DEFER["on"]):
        yield
        return
    L = _lib.lib()
    st = _DEFER.get("stream")
    L.vnet_wgrad_defer(0, st)
    try:
        yield
    finally:
        L.vnet_wgrad_defer(1, st)


def _wgrad_launch(r, x0, x1, dy, dw, owner=None):
    """Run a WGRAD route: dw = the filter gradient of x0 | x1 against dy.  owner: the parameter's gradient sink, whose buffer keeps
    the partial slabs of a deferred reduce; None = a gradient consumed right away (reduced now even inside a deferring pass)."""
    L = _lib.lib()
    immediate = owner is None
    B, C0, C1, Co = x0.shape[0], x0.shape[-1], (x1.shape[-1] if x1 is not None else 0), dy.shape[-1]
    nb, f = r.ws, r.family
    ws = _wgrad_workspace(dw, nb, immediate, owner)
    if (f in ("wgrad-bf16", "wgrad2-b16") and _DEFER["on"] and not immediate and _GROUP["on"] and not _timed_tag(r.tag)
            and _LAUNCH_ON[0] is None and _nvox(r.din) <= _GROUP["max_voxels"]
            and (_GROUP["k2"] and r.dout == tuple((d + 1) // 2 for d in r.din) if r.ks == 2 else
                 not (r.cin <= 4 and C0 == 8 and C1 == 0))):
        # a deep-level layer of a pass whose filter gradients nobody reads before it ends: launched together with the others when the
        # pass ends (vnet_conv_wgrad_b16_group; ks = 2: x = the fine tensor, dy = the coarse one); the tensors stay alive -- and
        # unmodified, see _ConvFn.backward -- until then
        _DEFER["jobs"].append((x0, x1, dy, dw, ws, nb, int(r.cin), B, r.din, r.flops, r.nbytes, r.ks))
        _DEFER["dy_ptrs"].add(dy.data_ptr())
        _group_pinned(x0, x1, dy)
        return
    with _Timed(r.tag, r.flops, r.nbytes), _immediate_reduce(immediate):
        if f == "wgrad-x3":
            check(L.vnet_conv_wgrad_x3(_ptr(x0), C0, _ptr(x1), C1, _ptr(dy), Co, _ptr(dw), B, *r.din, _ptr(ws), nb, _stream()),
                  "vnet_conv_wgrad_x3")
        elif f == "wgrad-bf16":
            check(L.vnet_conv_wgrad_b16(_ptr(x0), C0, _ptr(x1), C1, _ptr(dy), Co, _ptr(dw), int(r.cin), B, *r.din, _ptr(ws), nb,
                                        _stream()), "vnet_conv_wgrad_b16")
        elif f == "wgrad2-b16":
            check(L.vnet_conv2_wgrad_b16(_ptr(x0), C0, _ptr(dy), Co, _ptr(dw), B, *r.din, *r.dout, _ptr(ws), nb, _stream()),
                  "vnet_conv2_wgrad_b16")
        else:
            check(L.vnet_conv_wgrad(r.ks, r.kx, r.stride, _ptr(x0), C0, _ptr(x1), C1, _ptr(dy), Co, _ptr(dw),
                                    B, *r.din, *r.dout, _ptr(ws), nb, _stream()), "vnet_conv_wgrad")


# ---- one family's launch on explicit tensors (tests and profile scripts reach a kernel through these) -------------------------
# Each asks route() for the layer and refuses a shape the named family does not take: no quiet fall-back to another kernel.
def _family(r, *families):
    if r.family not in families:
        raise VnetHipError("%s: routed to %s, not %s" % (r.tag, r.family, " / ".join(families)))
    return r


def _conv_x3_call(x0, x1, wp, bias, y0, y1, dims, accum=False, stats=None, res=None):
    """5^3 stride-1 conv on the f32x3 kernels (vnet_conv_fwd_x3); wp: the PACK_FWD_X3 / PACK_BWD_X3 image; y1: a two-destination
    (backward-data shaped) launch."""
    C0, C1, Cy0, Cy1 = x0.shape[-1], (x1.shape[-1] if x1 is not None else 0), y0.shape[-1], (y1.shape[-1] if y1 is not None else 0)
    op, (a0, a1, o) = (FWD, (C0, C1, Cy0)) if y1 is None else (BWD, (Cy0, Cy1, C0))
    r = _family(route(op, 5, 1, 0, False, True, a0, a1, o, x0.shape[0], dims, dims), "conv-x3")
    _conv_launch(r, x0, x1, None, bias, y0, y1, accum=accum, stats=stats, res=res, wp=wp)


def _conv5_b16_call(x0, x1, wp, bias, y0, y1, dims, accum=False, stats=None, res=None, acc_src=None, cin_real=0):
    """5^3 stride-1 conv on bf16 tensors (vnet_conv_fwd_b16; vnet_conv_fwd_b16_padded for an input whose filter has cin_real < C0
    channels); wp: the PACK_FWD_BF16 / PACK_BWD_BF16 image."""
    C0, C1, Cy0, Cy1 = x0.shape[-1], (x1.shape[-1] if x1 is not None else 0), y0.shape[-1], (y1.shape[-1] if y1 is not None else 0)
    op, (a0, a1, o) = (FWD, (C0, C1, Cy0)) if y1 is None else (BWD, (Cy0, Cy1, C0))
    cin = int(cin_real) if not accum and acc_src is None else 0
    r = _family(route(op, 5, 1, 0, True, False, a0, a1, o, x0.shape[0], dims, dims, True, cin), "conv-bf16", "conv-bf16-padded")
    _conv_launch(r, x0, x1, None, bias, y0, y1, accum=accum, stats=stats, res=res, acc_src=acc_src, wp=wp)


def _conv2_b16(down, x, w, bias, y, dims_fine, dims_coarse, Cf, Cc, accum=False, stats=None):
    """The 2^3 stride-2 pair (fp32 or bf16 tensors, by the dtype of x).  down: coarse y = conv(fine x); else fine y (+)= transposed
    conv(coarse x).  w: the fp32 filter in TF layout, [2,2,2,Cf,Cc] for both."""
    r = route(FWD, 2, 2, 0 if down else 1, _is16(x), False, Cf if down else Cc, 0, Cc if down else Cf, x.shape[0],
              dims_fine if down else dims_coarse, dims_coarse if down else dims_fine, w.data_ptr() % 16 == 0)
    _conv_launch(_family(r, "conv2-direct", "conv2-b16", "conv"), x, None, w, bias, y, accum=accum, stats=stats if down else None)


def _wgrad5_b16_call(x0, x1, dy, dw, dims, cin_dw, owner=None):
    """Filter gradient of the 5^3 stride-1 conv on bf16 tensors (vnet_conv_wgrad_b16, or the grouped launch of a deferring pass)."""
    r = route(WGRAD, 5, 1, 0, True, False, x0.shape[-1], (x1.shape[-1] if x1 is not None else 0), dy.shape[-1], x0.shape[0], dims, dims,
              True, int(cin_dw))
    _wgrad_launch(_family(r, "wgrad-bf16"), x0, x1, dy, dw, owner)


def _wgrad2_b16_call(xfine, dycoarse, dw, dims_fine, dims_coarse, owner=None):
    """Filter gradient of the 2^3 stride-2 conv on bf16 tensors (vnet_conv2_wgrad_b16, or the grouped launch of a deferring pass)."""
    r = route(WGRAD, 2, 2, 0, True, False, xfine.shape[-1], 0, dycoarse.shape[-1], xfine.shape[0], dims_fine, dims_coarse)
    _wgrad_launch(_family(r, "wgrad2-b16"), xfine, None, dycoarse, dw, owner)


def colsum(x2d_like, C, out=None):
    """Per-channel sum over all leading axes of a channels-last tensor."""
    L = _lib.lib()
    M = x2d_like.numel() // C
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=x2d_like.device)
    nb = L.vnet_colsum_ws_bytes(C)
    ws = workspace(nb, x2d_like.device)
    check(L.vnet_colsum(_ptr(x2d_like), _ptr(out), M, C, _ptr(ws), nb, _stream()), "vnet_colsum")
    return out


# ---- tensors with two consumers: the second gradient is accumulated by the kernel that produces it ---------------------
# The skip connection (networks.py:276 -> 325: block output feeds the down convolution AND the decoder's concat) and the
# residual blocks (networks.py:314-318: block input feeds conv_1 AND the add in front of the last batch-norm) give autodiff
# two gradient contributions per tensor, which it sums with an add kernel (tf.add_n / torch's accumulation: 8 full-tensor
# adds per step, 134 MB each at level 1).  `fork` hands the two consumers separate views that share a slot; the consumer
# whose backward runs FIRST leaves its gradient tensor in the slot, the second one runs its backward-data kernel in
# accumulate mode (y += ...) on that tensor and reports no gradient of its own, so the sum costs no extra pass.
class _GradSlot(object):
    __slots__ = ("first", "total")

    def __init__(self):
        self.first = None
        self.total = None        # the SUM of both gradients, written out of place by the second consumer (see _ConvFn.backward)


class _ForkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slot):
        ctx.set_materialize_grads(False)
        ctx.slot = slot
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        total, ctx.slot.total = ctx.slot.total, None
        ctx.slot.first = None    # drop the slot's reference: a leaf behind this node can then take the gradient without a copy
        if total is not None:
            return total, None   # one consumer's kernel already added the other's gradient (out of place)
        if gb is None:
            return ga, None
        if ga is None:
            return gb, None
        return ga + gb, None     # both consumers reported a gradient (accumulation not possible there)


def fork(x):
    """Two handles of `x` for its two consumers (see above); plain (x, x) when no gradient is being recorded."""
    if _meta(x) or not (torch.is_grad_enabled() and x.requires_grad):
        return x, x
    slot = _GradSlot()
    a, b = _ForkFn.apply(x, slot)
    a._vnet_slot = b._vnet_slot = slot
    return a, b


def cut(x, registry):
    """Backward cut point (data-parallel step graphs): returns a LEAF that shares x's storage; `registry` collects
    (x, leaf).  A first backward pass stops at the leaves (their .grad holds what arrived), a second one continues from the
    recorded tensors: torch.autograd.backward([x...], [leaf.grad...]).  model.image2label uses it to end the first gradients
    graph where 81 % of the gradient bytes exist, so that their all-reduce travels under the rest of backward."""
    if _meta(x) or not (torch.is_grad_enabled() and x.requires_grad):
        return x
    leaf = x.detach().requires_grad_(True)
    registry.append((x, leaf))
    return leaf


def _slot_target(slot, dy, shape):
    """The tensor an accumulating backward-data kernel may add into: the other consumer's gradient, unless the parameter-
    gradient stream is on (its filter-gradient launches may still be reading that tensor) or it IS this kernel's input."""
    if slot is None or slot.first is None or _PG["on"]:
        return None
    t = slot.first
    if t.data_ptr() == dy.data_ptr() or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        return None
    return t


# ---- conv bias in front of a batch-norm ----------------------------------------------------------------------------------
# Every convolution of the V-Net (both wirings) feeds a train-mode batch-norm (networks.py:259...361; decoder chains
# included), and a batch-norm's output does not change when a per-channel constant is added to its input -- the batch mean
# absorbs it.  So dLoss/dbias == 0 IDENTICALLY for every conv bias of the network; what the reference's autodiff computes
# there (sum of dy over voxels, with dy the batch-norm's input gradient) is the floating-point residue of a sum that is zero
# in exact arithmetic (the fp64 oracle gets ~1e-12).  Inside this context the convolutions take the closed form: the bias
# gradient is left at exactly 0 in the flat gradient buffer and the 29 column-sum + 29 finalize launches per step are not
# made.  Stand-alone layers2.convolution (outside the networks) keeps the generic column sum.
_FUSE = {"zero_bias_grad": False, "bn_stats": True,
         # round 6: the single-modality input block on the vector pipe straight from the image (csrc/input_block.hip:
         # input_conv_direct_kernel / input_wgrad_direct_kernel); False = rounds 1-5: x-im2col tensor + 5x5x1 fp32-MFMA kernels (A/B runs)
         "input_direct": _os.environ.get("VNET_INPUT_DIRECT", "1") != "0"}


def set_epilogue_bn_stats(on, fp32_direct=True):
    """Switch for the batch-norm statistics in the convolution epilogues (on by default; off = separate statistics pass).
    fp32_direct: the non-split fp32 MFMA kernels write them too -- always (worth 0.07 ms per 128^3 step); False is refused."""
    if not fp32_direct:
        raise VnetHipError("set_epilogue_bn_stats: the fp32 MFMA kernels always write the epilogue statistics (fp32_direct=False was retired)")
    _FUSE["bn_stats"] = bool(on)


@contextlib.contextmanager
def zero_bias_gradients(on=True):
    prev = _FUSE["zero_bias_grad"]
    _FUSE["zero_bias_grad"] = bool(on)
    try:
        yield
    finally:
        _FUSE["zero_bias_grad"] = prev


def _conv_route(op, x0, x1, w, ks, stride, up, dout, res=False):
    """route() for `op` of the layer with filter w ([k,k,k,I,O]; up: [2,2,2,O,I]) on the forward inputs x0 | x1."""
    O, I = (w.shape[-2], w.shape[-1]) if up else (w.shape[-1], w.shape[-2])
    return route(op, ks, stride, up, _is16(x0), _COMPUTE["split3"], x0.shape[-1], (x1.shape[-1] if x1 is not None else 0), O,
                 x0.shape[0], x0.shape[1:4], dout, w.data_ptr() % 16 == 0, I, res)


def _side_stream(dev, wr, db, sb, dw, sw):
    """The parameter-gradient stream for a node's bias / filter gradient (wr: the filter gradient's route), or None: a gradient
    autograd has to hand on stays on the main stream, and so does a filter gradient whose launch is being timed (bench.py roofline)."""
    side = param_grad_stream(dev)
    if side is None or (db is not None and sb is None) or (dw is not None and sw is None):
        return None
    if dw is not None and _timed_tag(wr.tag):
        return None
    return side


class _ConvFn(torch.autograd.Function):
    """conv (ks=5,s=1 | ks=2,s=2) or 2^3 transposed conv (up) + bias, two-source input; r: the forward's route."""

    @staticmethod
    def forward(ctx, x0, x1, w, b, r, stats=None, res=None):
        slot0, slot1 = getattr(x0, "_vnet_slot", None), getattr(x1, "_vnet_slot", None)
        x0 = x0.contiguous()
        x1 = x1.contiguous() if x1 is not None else None
        B, C0 = x0.shape[0], x0.shape[-1]
        C1 = x1.shape[-1] if x1 is not None else 0
        O, I = (w.shape[-2], w.shape[-1]) if r.up else (w.shape[-1], w.shape[-2])
        b16 = _is16(x0)            # bf16-storage mode: bf16 tensors in and out (the network input may be zero-padded to 8 channels)
        if I != C0 + C1 and not (b16 and x1 is None and C0 == -(-I // 8) * 8):
            raise VnetHipError("conv: filter expects %d input channels, got %d" % (I, C0 + C1))
        if b16 and (_is16(x1) != (x1 is not None) or (res is not None and not _is16(res))):
            raise VnetHipError("conv: bf16 and float32 tensors mixed")
        if b16 and x1 is not None and (r.up or r.ks != 5):
            raise VnetHipError("conv: the two-source form exists for the 5^3 convolution only")
        y = torch.empty((B,) + r.dout + (O,), dtype=torch.bfloat16 if b16 else torch.float32, device=x0.device)
        _conv_launch(r, x0, x1, w, b, y, stats=stats, res=res.contiguous() if res is not None else None)
        ctx.save_for_backward(x0, x1, w)
        ctx.params = (w, b)
        ctx.cfg = (r.ks, r.stride, r.up, r.din, r.dout, C0, O)
        ctx.bf16 = b16 and r.ks == 5 and r.stride == 1 and not r.up
        ctx.b16 = b16
        ctx.bias_zero = _FUSE["zero_bias_grad"] and b is not None
        ctx.slots = (slot0, slot1)
        ctx.opsctx = current_context()
        return y

    @staticmethod
    def backward(ctx, dy):
        # the backward pass runs in the OpsContext of the forward pass (a user-driven loss.backward() outside
        # model.in_context would otherwise pick the default context's compute mode, stream and pack registry)
        with context(ctx.opsctx):
            return _ConvFn._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        x0, x1, w = ctx.saved_tensors
        ks, stride, up, din, dout, C0, O = ctx.cfg
        dy = dy.contiguous()
        dev = x0.device
        wref, bref = ctx.params
        db = dw = None
        sb = sw = None
        bias_zero = False
        if ctx.needs_input_grad[3]:
            if ctx.bias_zero and getattr(bref, "_vnet_sink", None) is not None and not bref._vnet_sink.written:
                bias_zero, sb = True, bref._vnet_sink      # closed form: the flat gradient buffer already holds the exact 0
            else:
                db, sb = _grad_out(bref)
        wr = None
        if ctx.needs_input_grad[2]:
            dw, sw = _grad_out(wref)
            wr = _conv_route(WGRAD, x0, x1, w, ks, stride, up, dout)
        side = _side_stream(dev, wr, db, sb, dw, sw)
        if side is not None:
            main = torch.cuda.current_stream(dev)
            side.wait_stream(main)                       # dy is complete on the main stream
            for t in (x0, x1, dy):
                if t is not None:
                    t.record_stream(side)                # keep the allocator from recycling them under the side stream
            # dy of a residual block is ALSO the gradient of the block input (one tensor, two autograd edges); once this
            # node has returned autograd holds the last reference and accumulates the next gradient INTO it in place
            # (input_buffer.cpp: use_count == 1), on the main stream, while the filter gradient may still be reading it.
            # A live reference until the join makes that accumulation out of place.
            if not _PG["used"]:
                # first side-stream launch of this backward pass: join when the pass ends, whoever drives it (a user
                # loop calling loss.backward() directly would otherwise keep every dy alive and could read filter
                # gradients before the side stream has written them)
                torch.autograd.Variable._execution_engine.queue_callback(join_param_grad_stream)
            _PG["keep"].append(dy)
            _PG["used"].add(dev)
            if _PG["test_delay"]:
                with torch.cuda.stream(side):
                    torch.cuda._sleep(int(_PG["test_delay"]))    # tests: let the side stream lag far behind
            _LAUNCH_ON[0] = side.cuda_stream             # launches (and their scratch buffer) go to the side stream
        b16 = ctx.b16
        try:
            if db is not None:
                if b16:
                    colsum16(dy, O, db)
                else:
                    colsum(dy, O, out=db)
            if dw is not None and up:      # the transposed conv's filter gradient: fine dy against coarse x (see route)
                _wgrad_launch(wr, dy, None, x0, dw, owner=sw)
            elif dw is not None:
                _wgrad_launch(wr, x0, x1, dy, dw, owner=sw)
        finally:
            _LAUNCH_ON[0] = None
        dx0 = dx1 = None
        r0 = r1 = None
        if ctx.needs_input_grad[0] or (x1 is not None and ctx.needs_input_grad[1]):
            slot0, slot1 = ctx.slots
            # x0 has a second consumer whose gradient exists already: add this one into it (single-source convs only)
            acc = _slot_target(slot0, dy, x0.shape) if x1 is None else None
            # one-convolution residual block: the other gradient of x0 IS this node's dy (batch-norm's ds serves the conv
            # output and the residual) -- no in-place sum, but the bf16 kernels can add it on the way out: dx0 = conv(dy) + dy
            oop = None
            if (acc is None and x1 is None and ctx.bf16 and slot0 is not None and slot0.first is not None
                    and slot0.first.data_ptr() == dy.data_ptr() and tuple(dy.shape) == tuple(x0.shape)
                    and b16 and C0 % 8 == 0):
                oop = dy
            if acc is not None and b16 and ks == 5 and stride == 1 and not up and acc.data_ptr() in _DEFER["dy_ptrs"]:
                # the other gradient of x0 is ALSO the dy of a filter gradient that waits for the grouped launch (a residual block's
                # ds serves its last convolution and the block input): add it on the way out into a fresh tensor instead of in place
                # -- the same arithmetic, RNE(accumulator + stored gradient), so the bits do not change
                oop, acc = acc, None
            dx0 = acc if acc is not None else torch.empty_like(x0)
            dx1 = torch.empty_like(x1) if x1 is not None else None
            accum = acc is not None
            # backward-data of the transposed conv = the 2^3 stride-2 conv with the same filter and vice versa
            _conv_launch(_conv_route(BWD, x0, x1, w, ks, stride, up, dout), dy, None, w, None, dx0, dx1, accum=accum, acc_src=oop)
            if oop is not None:
                slot0.total = dx0
            r0, r1 = (None if accum else dx0), dx1
            if not accum and slot0 is not None and slot0.first is None:
                slot0.first = dx0                      # first of the two gradients of a forked tensor
            if slot1 is not None and slot1.first is None:
                slot1.first = dx1
        gb = _grad_ret(db, sb) if (db is not None or bias_zero) else None
        return r0, r1, _grad_ret(dw, sw), gb, None, None, None


def _meta(*ts):
    return any(t is not None and t.device.type == "meta" for t in ts)


class _InputConvFn(torch.autograd.Function):
    """conv5^3(BN(tile(img))) + b for a 1-channel image without the 16x redundant work (csrc/input_block.hip):
    forward = 5x5x1 conv over the x-im2col of (img, inside-indicator) with BN-folded filters; backward needs only
    the 2-channel filter gradient G -- dw, and the conv-path parts of the input BN's dgamma/dbeta follow from it.
    r: the IN_FWD route."""

    @staticmethod
    def forward(ctx, img, gamma, beta, mean, invstd, w, b, r, stats=None, res=None):
        L = _lib.lib()
        img = img.contiguous()
        if res is not None:
            res = res.contiguous()
        B, D, H, W, _ = img.shape
        C, O = w.shape[-2], w.shape[-1]
        dev = img.device
        wv = torch.empty((25, 16, O), dtype=torch.float32, device=dev)
        check(L.vnet_input_conv_fold(_ptr(w), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(wv), C, O, _stream()),
              "vnet_input_conv_fold")
        y = torch.empty((B, D, H, W, O), dtype=torch.float32, device=dev)
        if r.family == "input-direct":
            xv = img
            border = torch.empty(9 * 26 * O, dtype=torch.float32, device=dev)      # wbc [9][25][O] | cbc [9][O]
            check(L.vnet_input_conv_fold_border(_ptr(wv), O, _ptr(border), _ptr(border[9 * 25 * O:]), _stream()), "vnet_input_conv_fold_border")
            with _Timed(r.tag, r.flops, r.nbytes):
                check(L.vnet_input_conv_direct_fwd(_ptr(img), _ptr(wv), _ptr(border), _ptr(border[9 * 25 * O:]), _ptr(b), _ptr(res), _ptr(y),
                                                   _ptr(stats), O, B, D, H, W, _stream()), "vnet_input_conv_direct_fwd")
        else:
            xv = torch.empty((B, D, H, W, 16), dtype=torch.float32, device=dev)
            check(L.vnet_tile_im2col_x(_ptr(img), _ptr(xv), B, D, H, W, _stream()), "vnet_tile_im2col_x")
            wp = torch.empty(L.vnet_packed_weight_floats(*r.pack), dtype=torch.float32, device=dev)
            check(L.vnet_pack_weights(r.pack[0], _ptr(wv), _ptr(wp), *r.pack[1:], _stream()), "vnet_pack_weights")
            _conv_launch(r, xv, None, None, b, y, stats=stats, res=res, wp=wp)
        ctx.wroute = route(IN_WGRAD, 5, 1, 0, False, False, 1, 0, O, B, (D, H, W), (D, H, W))     # (the same reading of the switch)
        ctx.save_for_backward(xv, gamma, beta, mean, invstd, w)
        ctx.params = (w, b)
        ctx.gb = (gamma, beta)
        ctx.bias_zero = _FUSE["zero_bias_grad"]
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        xv, gamma, beta, mean, invstd, w = ctx.saved_tensors
        wref, bref = ctx.params
        dy = dy.contiguous()
        B, D, H, W = xv.shape[:4]
        C, O = w.shape[-2], w.shape[-1]
        dev = dy.device
        if ctx.bias_zero and getattr(bref, "_vnet_sink", None) is not None and not bref._vnet_sink.written:
            db, sb = None, bref._vnet_sink               # closed form (see zero_bias_gradients)
        else:
            db, sb = _grad_out(bref)
            colsum(dy, O, out=db)
        G = torch.empty((25, 16, O), dtype=torch.float32, device=dev)
        wr = ctx.wroute
        if wr.family == "input-wgrad-direct":          # xv IS the image here
            ws = workspace(wr.ws, dev)
            with _Timed(wr.tag, wr.flops, wr.nbytes):
                check(L.vnet_input_wgrad_direct(_ptr(xv), _ptr(dy), _ptr(G), O, B, D, H, W, _ptr(ws), wr.ws, _stream()), "vnet_input_wgrad_direct")
        else:
            _wgrad_launch(wr, xv, None, dy, G)         # (no owner: G is folded right below)
        dw, sw = _grad_out(wref)
        gpar, bpar = ctx.gb
        gs, bs = getattr(gpar, "_vnet_sink", None), getattr(bpar, "_vnet_sink", None)
        if (sw is not None and gs is not None and bs is not None and not gs.written and not bs.written
                and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]):
            # gamma / beta of the input batch-norm get two contributions: this one (through the folded filter) and the
            # batch-norm's own.  The batch-norm's backward runs later in this pass and WRITES its part into the flat buffer;
            # this kernel is deferred until then and ADDS its part (accumulate = 1) -- no autodiff add kernels, one launch.
            def deferred(accumulate, L=L, G=G, w=w, gamma=gamma, beta=beta, mean=mean, invstd=invstd, dw=dw, sw=sw, gs=gs, bs=bs):
                check(L.vnet_input_conv_grads(_ptr(G), _ptr(w), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(dw),
                                              _ptr(gs.view), _ptr(bs.view), C, O, int(accumulate), _stream()), "vnet_input_conv_grads")
                _grad_ret(dw, sw)
                if not accumulate:          # the batch-norm's backward never came: these sinks are complete now
                    _grad_ret(gs.view, gs)
                    _grad_ret(bs.view, bs)
            gpar._vnet_deferred = deferred

            def flush(gpar=gpar):
                th = getattr(gpar, "_vnet_deferred", None)
                if th is not None:
                    del gpar._vnet_deferred
                    th(0)
            torch.autograd.Variable._execution_engine.queue_callback(flush)
            return None, None, None, None, None, None, _grad_ret(db, sb), None, None, None
        dgamma = torch.empty(C, dtype=torch.float32, device=dev)
        dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        check(L.vnet_input_conv_grads(_ptr(G), _ptr(w), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(dw),
                                      _ptr(dgamma), _ptr(dbeta), C, O, 0, _stream()), "vnet_input_conv_grads")
        return None, dgamma, dbeta, None, None, _grad_ret(dw, sw), _grad_ret(db, sb), None, None, None


class _EpilogueStats(object):
    """Partial batch-norm sums a convolution wrote in its epilogue for its output y: rows x [sum(C) | sum of squares(C)] of
    v = y (+ residual).  Attached to y as `_vnet_stats`; the batch-norm that normalises (y + residual) runs only its finalize."""
    __slots__ = ("partial", "rows", "residual")

    def __init__(self, partial, rows, residual):
        self.partial, self.rows, self.residual = partial, rows, residual


def _with_epilogue_stats(fn, args, r, O, bn_stats, bn_residual, device):
    """fn.apply(*args) for the forward route r; with bn_stats (and the fused statistics on) its epilogue also writes the partial sums
    of the batch-norm behind it into a buffer of r.stats_rows rows (cross-replica statistics need the raw moments of the whole
    tensor: the generic path)."""
    if not (bn_stats and _FUSE["bn_stats"] and _SYNC_BN is None and r.stats_rows > 0):
        return fn.apply(*args)
    stats = torch.empty((r.stats_rows, 2 * O), dtype=torch.float32, device=device)
    y = fn.apply(*args, stats, bn_residual)
    y._vnet_stats = _EpilogueStats(stats, r.stats_rows, bn_residual)
    return y


def input_conv(img, gamma, beta, mean, invstd, w, b, bn_stats=False, bn_residual=None):
    """convolution(BN(tf.tile(img)), [5,5,5,C,C]) for a 1-channel `img` (networks.py:254-259 + 316)."""
    if _meta(img):
        return torch.empty(img.shape[:-1] + (w.shape[-1],), device="meta")
    _need_gpu(img, "input_conv")
    B, D, H, W, _ = img.shape
    r = route(IN_FWD, 5, 1, 0, False, False, 1, 0, w.shape[-1], B, (D, H, W), (D, H, W))
    return _with_epilogue_stats(_InputConvFn, (img, gamma, beta, mean, invstd, w, b, r), r, w.shape[-1], bn_stats, bn_residual, img.device)


def conv(x0, w, b, ks, stride=1, x1=None, bn_stats=False, bn_residual=None):
    """tf.nn.convolution(concat(x0,x1), w, 'SAME', strides) + b (reference layers2.py:63).
    bn_stats: the output feeds tf.layers.batch_normalization(y [+ bn_residual]) -- the convolution's epilogue also produces
    that batch-norm's partial sums (include/vnet_hip.h: vnet_conv_fwd_stats), so its statistics pass over y is not needed."""
    if x0.dim() != 5:
        raise NotImplementedError("only the 3-D (NDHWC) path is built; 2-D is out of scope (SURVEY section 2 row 11)")
    if _meta(x0):
        B, D, H, W, _ = x0.shape
        return torch.empty((B, _same_out(D, stride), _same_out(H, stride), _same_out(W, stride), w.shape[-1]), device="meta")
    _need_gpu(x0, "conv", allow16=True)
    fused = bn_stats and _FUSE["bn_stats"] and _SYNC_BN is None
    r = _conv_route(FWD, x0, x1, w, ks, stride, False, tuple(_same_out(int(v), stride) for v in x0.shape[1:4]),
                    res=fused and bn_residual is not None)
    return _with_epilogue_stats(_ConvFn, (x0, x1, w, b, r), r, w.shape[-1], bn_stats, bn_residual, x0.device)


def conv_transpose2(x, w, b, out_spatial):
    """tf.nn.conv3d_transpose(x, w, output_shape, [1,2,2,2,1], 'SAME') + b (reference layers2.py:73)."""
    if x.dim() != 5:
        raise NotImplementedError("only the 3-D (NDHWC) path is built")
    if _meta(x):
        return torch.empty((x.shape[0],) + tuple(out_spatial) + (w.shape[-2],), device="meta")
    _need_gpu(x, "conv_transpose2", allow16=True)
    return _ConvFn.apply(x, None, w, b, _conv_route(FWD, x, None, w, 2, 2, True, out_spatial))


# ---- batch-norm (+residual, +tile, +activation) -------------------------------------------------------
# ---- cross-replica batch-norm ---------------------------------------------------------
# Default data-parallel semantics are per-replica statistics (== the reference run with BatchSize=1 per patch).
# With a group set here every batch-norm reduces its moments over all ranks, which reproduces the reference's
# single-device BatchSize=N numbers (networks.py:319 reduces over the batch axis as well).  Every rank must hold
# the same number of rows per layer (equal per-rank batch), as data-parallel training does.
_SYNC_BN = None      # (all_reduce callable, world size) or None


def set_sync_batch_norm(group=None, enabled=True):
    """Enable (or, with enabled=False, disable) cross-replica batch-norm statistics over `group`
    (default: the world group of torch.distributed)."""
    global _SYNC_BN
    if not enabled:
        _SYNC_BN = None
        return
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise VnetHipError("set_sync_batch_norm needs an initialised torch.distributed process group")
    world = dist.get_world_size(group)
    _SYNC_BN = ((lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)), world) if world > 1 else None


# bf16 storage, tiny tensors (the 8^3 level: <= 512 rows): statistics + finalize + normalise in ONE launch, and reduce + finalize +
# apply in one (vnet_bn_small_*_b16; `_SMALL_BN["on"] = False`: the streaming kernels everywhere).  Measured (profiles/ab_env.sh, C5 step):
# <= 512 rows -0.015 ms, <= 1024 the same, <= 8192 (the 16^3 level too) +0.13 ms -- one workgroup per channel octet uses 16 bytes
# of every 256-byte row it touches, on 16-32 CUs; the five launch-bound streaming launches on 128+ workgroups are faster there.
_SMALL_BN = {"on": True, "rows": 512}


class BnRoute(collections.namedtuple("BnRoute", "stats stats16 apply16 allreduce")):
    """How one batch-norm runs, as bn_route() chose it.  stats: where mean / invstd come from -- "epilogue" (finalize the partial
    sums the producing convolution wrote), "stream" (a statistics pass over x (+ r)), "moments" (raw moments all-reduced over the
    replicas, then finalize) or "small" (the one-launch bf16 kernels, forward and backward); stats16 / apply16: the statistics
    kernels / the normalise and backward kernels are the bf16-storage (`_b16`) entries; allreduce: the backward all-reduces its sums
    [sum_dz | sum_dz_xhat] before the apply."""
    __slots__ = ()


def bn_route(op, M, C, bcast=False, x16=False, r16=None, epilogue=False, store16=None, sync=None):
    """The kernels of batch-norm `op` ("act": bn_act, "chain": bn_chain, "stats": the moving-average update of a dead batch-norm)
    over s = x (+ r), M rows of C channels.  bcast: x has one channel, tiled to C; x16 / r16: x / the residual is bf16 (r16 None: no
    residual); epilogue: x carries its producer's partial sums of exactly s (_epilogue_of); store16: bf16-storage mode; sync:
    cross-replica statistics (store16 / sync None: the current setting)."""
    store16 = _COMPUTE["store16"] if store16 is None else store16
    sync = _SYNC_BN is not None if sync is None else sync
    # (tried before the epilogue sums, which it does not use; per-replica only)
    if (op == "act" and not bcast and x16 and r16 is not False and not sync and _SMALL_BN["on"] and M <= _SMALL_BN["rows"]
            and _lib.lib().vnet_bn_small_ok(int(M), int(C))):
        return BnRoute("small", True, True, False)
    stats = "moments" if sync else "epilogue" if epilogue and not bcast else "stream"
    # bf16 storage: a bf16 input, or the tiled fp32 1-channel image in that mode (C = 8 * 2^k; the 2..5-class batch-norm of the
    # logits stays on the fp32 kernels).  The image's statistics stay on the fp32 kernels.
    apply16 = x16 or (bcast and store16 and C % 8 == 0)
    return BnRoute(stats, x16 and stats != "epilogue", apply16, sync and op != "stats")


def _epilogue_of(x, r, C):
    """The _EpilogueStats the producing convolution attached to x when they cover exactly x + r (r: the same object) over C
    channels, else None."""
    pre = getattr(x, "_vnet_stats", None)
    return pre if pre is not None and pre.residual is r and pre.partial.shape[1] == 2 * C else None


def _bn_stats(rt, x, r, bcast, M, C, mm, mv, pre=None):
    """mean / invstd (+ the moving-average update) of s = x (+ r) the way route rt says (pre: _epilogue_of x); returns mean, invstd
    and the row count they cover."""
    L = _lib.lib()
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    nb = L.vnet_bn_ws_bytes(C)
    ws = workspace(nb, x.device)
    if rt.stats == "epilogue":
        check(L.vnet_bn_finalize_partial(_ptr(pre.partial), pre.rows, C, float(M), BN_EPS, BN_MOMENTUM, _ptr(mean), _ptr(invstd),
                                         _ptr(mm), _ptr(mv), _stream()), "vnet_bn_finalize_partial")
        return mean, invstd, float(M)
    sfx, tile = ("_b16", ()) if rt.stats16 else ("", (int(bcast),))       # (the bf16 statistics kernels take no tile flag)
    if rt.stats == "stream":
        name = "vnet_bn_stats" + sfx
        check(getattr(L, name)(_ptr(x), _ptr(r), *tile, M, C, BN_EPS, BN_MOMENTUM, _ptr(mean), _ptr(invstd), _ptr(mm), _ptr(mv),
                               _ptr(ws), nb, _stream()), name)
        return mean, invstd, float(M)
    all_reduce, world = _SYNC_BN
    sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
    name = "vnet_bn_moments" + sfx
    check(getattr(L, name)(_ptr(x), _ptr(r), *tile, M, C, _ptr(sums), _ptr(ws), nb, _stream()), name)
    all_reduce(sums)
    check(L.vnet_bn_finalize(_ptr(sums), float(M) * world, C, BN_EPS, BN_MOMENTUM, _ptr(mean), _ptr(invstd),
                             _ptr(mm), _ptr(mv), _stream()), "vnet_bn_finalize")
    return mean, invstd, float(M) * world


def _bn_forward(op, x, r, bcast, C, pre, scale, shift, act, alpha, mm, mv, coef=None, head=None):
    """Forward of y = act(scale * xhat + shift), xhat the normalised s = x (+ r) (both contiguous; pre: _epilogue_of the caller's x):
    the route, the statistics and ONE normalise launch -- every batch-norm's forward goes through here.  coef(mean, invstd) runs between
    the two and returns the (scale, shift) to use (the chain's coefficients, _BnFn).  head = (w, b, stats): the launch is the fused
    head's -- it returns the logits y W + b in place of y, which it does not store, and writes the logits' partial sums into stats
    (None: not) (include/vnet_hip_head.h; float32 only).
    Returns the plan _bn_backward takes -- (route, bcast, M, C, act, rows the statistics cover, the backward's all-reduce or None) --
    and y, mean, invstd, scale, shift."""
    L = _lib.lib()
    M = x.numel() if bcast else x.numel() // C
    rt = bn_route(op, M, C, bcast, _is16(x), None if r is None else _is16(r), pre is not None)
    if rt.apply16 and r is not None and not _is16(r):
        raise VnetHipError("bn_act: bf16 and float32 tensors mixed")
    dev = x.device
    if rt.stats == "small":
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty(C, dtype=torch.float32, device=dev)
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=dev)
        check(L.vnet_bn_small_fwd_b16(_ptr(x), _ptr(r), M, C, BN_EPS, BN_MOMENTUM, _ptr(scale), _ptr(shift), act, _ptr(alpha),
                                      _ptr(mean), _ptr(invstd), _ptr(mm), _ptr(mv), _ptr(y), _stream()), "vnet_bn_small_fwd_b16")
        m_total = float(M)
    else:
        mean, invstd, m_total = _bn_stats(rt, x, r, bcast, M, C, mm, mv, pre)
        if coef is not None:
            scale, shift = coef(mean, invstd)
        bn = (M, C, _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), act, _ptr(alpha))
        if head is not None:
            w, b, stats = head
            K = int(w.shape[-1])
            y = torch.empty(x.shape[:-1] + (K,), dtype=torch.float32, device=dev)
            check(L.vnet_bn_act_head_fwd(_ptr(x), _ptr(r), *bn, _ptr(w), _ptr(b), K, None, _ptr(y), _ptr(stats), _stream()),
                  "vnet_bn_act_head_fwd")
        else:
            y = torch.empty(x.shape[:-1] + (C,), dtype=torch.bfloat16 if rt.apply16 else torch.float32, device=dev)
            name = "vnet_bn_act_fwd" + ("_b16" if rt.apply16 else "")
            check(getattr(L, name)(_ptr(x), _ptr(r), int(bcast), *bn, _ptr(y), _stream()), name)
    return (rt, bcast, M, C, act, m_total, _SYNC_BN[0] if rt.allreduce else None), y, mean, invstd, scale, shift


def _bn_backward(plan, dy, x, r, mean, invstd, scale, shift, alpha, dscale, dshift, dalpha, ds, coef=None, head=None):
    """Backward of _bn_forward's y (plan: what it returned): the sums sum_dz_xhat -> dscale, sum_dz -> dshift (and dalpha), all-reduced
    when the route says so, then ds (None: no data gradient) from them.  coef(sum_dz_xhat) runs between the two and returns the apply's
    xhat coefficient (the chain's, _BnFn).
    head = (w, dw, db): y fed the 1x1x1 head y W + b and `dy` is the gradient of its LOGITS -- both passes form dy = dlogits W^T
    per voxel and the first one also sums the head's dw / db (include/vnet_hip_head.h; float32, the route not "small")."""
    L = _lib.lib()
    rt, bcast, M, C, act, m_total, all_reduce = plan
    if head is not None:
        w, dw, db = head
        K = int(w.shape[-1])
        nb = L.vnet_bn_head_ws_bytes(C, K)
        ws = workspace(nb, dy.device)
        sfx = "_head"
        args = (_ptr(dy), _ptr(w), K, _ptr(x), _ptr(r), M, C, _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), act, _ptr(alpha))
        check(L.vnet_bn_act_bwd_reduce_head(*args, _ptr(dscale), _ptr(dshift), _ptr(dalpha), _ptr(dw), _ptr(db), _ptr(ws), nb, _stream()),
              "vnet_bn_act_bwd_reduce_head")
    else:
        nb = L.vnet_bn_ws_bytes(C)
        ws = workspace(nb, dy.device)
        if rt.stats == "small":
            check(L.vnet_bn_small_bwd_b16(_ptr(dy), _ptr(x), _ptr(r), M, C, _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), act,
                                          _ptr(alpha), _ptr(dscale), _ptr(dshift), _ptr(dalpha), _ptr(ds), _stream()), "vnet_bn_small_bwd_b16")
            return
        sfx = "_b16" if rt.apply16 else ""
        args = (_ptr(dy), _ptr(x), _ptr(r), int(bcast), M, C, _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), act, _ptr(alpha))
        name = "vnet_bn_act_bwd_reduce" + sfx
        check(getattr(L, name)(*args, _ptr(dscale), _ptr(dshift), _ptr(dalpha), _ptr(ws), nb, _stream()), name)
    sdz, sdzx = dshift, dscale
    if rt.allreduce and (ds is not None or coef is not None):
        # this replica's parameter gradients stay local (the gradient all-reduce averages them); the data gradient needs the sums
        # over the whole cross-replica batch
        sdz = torch.cat([dshift.reshape(-1), dscale.reshape(-1)])
        all_reduce(sdz)
        sdzx = sdz[C:]
    extra = coef(sdzx) if coef is not None else None
    if ds is not None:
        name = "vnet_bn_act_bwd_apply" + sfx
        check(getattr(L, name)(*args, _ptr(sdz), _ptr(sdzx), m_total, _ptr(extra), _ptr(ds), _stream()), name)


class _BnFn(torch.autograd.Function):
    """The batch-norm behind bn_act, bn_chain and bn_head: one statistics pass + one normalise pass forward, one reduce + one apply pass
    backward.  kind -1: y = act(BN(x (+ r))) with (g1, b1), x tiled from one channel when bcast.  The decoder's chains in closed form
    (include/vnet_hip.h, vnet_bn_chain_*) -- kind 0: act(BN3(BN1(x) + BN2(BN1(x)))) (networks.py:333-337), kind 1: act(BNb(x + BNa(x)))
    with (g1, b1) = a, (g2, b2) = b (networks.py:358-361).  bufs: the moving averages (mm1, mv1, ... mv3).
    With w (float32 only) the result is logits = head_conv(y, w, b) from the same normalise pass, which also writes the partial sums of
    the logits into `stats` (None: not) for the batch-norm behind the head.  y is then not stored: nothing but the head reads it, and
    the backward rebuilds it from x; its two passes read dlogits (K floats per voxel) in place of a [M][C] gradient of y, and the reduce
    also sums the head's dw / db.  Returns (y or logits, mean, invstd)."""

    @staticmethod
    def forward(ctx, x, r, kind, act, bcast, stats, bufs, alpha, w, b, g1, b1, g2, b2, g3, b3):
        L = _lib.lib()
        ctx.slot_r = getattr(r, "_vnet_slot", None)
        C = g1.numel()
        pre = _epilogue_of(x, r, C)
        x = x.contiguous()
        r = r.contiguous() if r is not None else None
        mm1, mv1, mm2, mv2, mm3, mv3 = bufs

        def coef(mean, invstd):     # the chain as ONE scale / shift per channel, and the moving averages of its derived layers
            ceff = torch.empty(C, dtype=torch.float32, device=x.device)
            deff = torch.empty(C, dtype=torch.float32, device=x.device)
            name = "vnet_bn_chain_coef_fwd"
            check(getattr(L, name)(kind, C, BN_EPS, BN_MOMENTUM, _ptr(mean), _ptr(invstd), _ptr(g1), _ptr(b1), _ptr(g2), _ptr(b2), _ptr(g3),
                                   _ptr(b3), _ptr(ceff), _ptr(deff), _ptr(mm2), _ptr(mv2), _ptr(mm3), _ptr(mv3), _stream()), name)
            return ceff, deff
        ctx.plan, y, mean, invstd, scale, shift = _bn_forward("act" if kind < 0 else "chain", x, r, bcast, C, pre, g1, b1, act, alpha,
                                                              mm1, mv1, coef if kind >= 0 else None, (w, b, stats) if w is not None else None)
        ctx.save_for_backward(x, r, alpha, w, g1, g2, g3, mean, invstd, scale, shift)
        ctx.params = (g1, b1, g2, b2, g3, b3, alpha, w, b)
        ctx.kind = kind
        ctx.mark_non_differentiable(mean, invstd)
        ctx.set_materialize_grads(False)      # no zero-filled gradients for the (non-differentiable) statistics outputs
        return y, mean, invstd

    @staticmethod
    def backward(ctx, dy, _gmean, _ginvstd):
        L = _lib.lib()
        x, r, alpha, w, g1, g2, g3, mean, invstd, scale, shift = ctx.saved_tensors
        rt, bcast, _, C, _, m_total, _ = ctx.plan
        kind = ctx.kind
        dy = dy.contiguous()
        if rt.apply16 and not _is16(dy):
            raise VnetHipError("bn_act backward: expected a bfloat16 gradient")
        dev = dy.device
        # every parameter's gradient goes straight into its sink where there is one (_grad_out here, _grad_ret below)
        outs = [_grad_out(p) if p is not None else (None, None) for p in ctx.params]
        dg1, db1, dg2, db2, dg3, db3, dalpha, dw, db = (o[0] for o in outs)
        dscale, dshift, coef = dg1, db1, None
        if kind >= 0:
            dscale = torch.empty(C, dtype=torch.float32, device=dev)
            dshift = torch.empty(C, dtype=torch.float32, device=dev)
            extra = torch.empty(C, dtype=torch.float32, device=dev)

            def coef(dCg):        # every gamma / beta gradient of the chain, and the xhat coefficient of the apply
                name = "vnet_bn_chain_coef_bwd"
                check(getattr(L, name)(kind, C, BN_EPS, m_total, _ptr(mean), _ptr(invstd), _ptr(g1), _ptr(g2), _ptr(g3), _ptr(dscale),
                                       _ptr(dshift), _ptr(dCg), _ptr(dg1), _ptr(db1), _ptr(dg2), _ptr(db2), _ptr(dg3), _ptr(db3), _ptr(extra),
                                       _stream()), name)
                return extra
        need_ds = ctx.needs_input_grad[0] or (r is not None and ctx.needs_input_grad[1])
        ds = torch.empty(x.shape[:-1] + (C,), dtype=torch.bfloat16 if rt.apply16 else torch.float32, device=dev) if need_ds else None
        _bn_backward(ctx.plan, dy, x, r, mean, invstd, scale, shift, alpha, dscale, dshift, dalpha, ds, coef,
                     (w, dw, db) if w is not None else None)
        th = getattr(ctx.params[0], "_vnet_deferred", None)
        if th is not None and outs[0][1] is not None and outs[1][1] is not None:
            del ctx.params[0]._vnet_deferred
            th(1)                                          # the fused input conv adds its share of dgamma / dbeta (see _InputConvFn)
        dx = ds
        if bcast and ds is not None:
            dx = colsum_rows(ds)
        if r is not None and ds is not None and ctx.slot_r is not None and ctx.slot_r.first is None:
            ctx.slot_r.first = ds                      # the block input's other consumer (conv_1) adds its gradient into this
        rets = [_grad_ret(t, s) if p is not None else None for (t, s), p in zip(outs, ctx.params)]
        return (dx, (ds if r is not None else None), None, None, None, None, None, rets[6], rets[7], rets[8]) + tuple(rets[:6])


def _bn_apply(what, x, r, kind, a, alpha, bcast, g, moving, w=None, b=None, stats=None):
    """The argument checks bn_act, bn_chain and bn_head (`what`) share, then _BnFn; g = (g1, b1, g2, b2, g3, b3)."""
    _need_gpu(x, what, allow16=w is None)
    if a == 2 and alpha is None:
        raise VnetHipError("prelu needs alpha")
    if kind == 0 and (g[4] is None or g[5] is None):
        raise VnetHipError("bn_chain kind 0 needs three batch-norm layers")
    return _BnFn.apply(x, r, int(kind), a, bool(bcast), stats, tuple(moving), alpha if a == 2 else None, w, b, *g)


def bn_chain(x, kind, act, alpha, g1, b1, g2, b2, g3=None, b3=None, moving=(None,) * 6):
    """kind 0: act(BN3(BN1(x) + BN2(BN1(x)))) with (g1,b1),(g2,b2),(g3,b3); kind 1: act(BNb(x + BNa(x))) with (g1,b1)=a, (g2,b2)=b.
    moving = (mm1, mv1, mm2, mv2, mm3, mv3) moving-average buffers (None to skip)."""
    a = ACT[act]
    if _meta(x):
        return torch.empty(x.shape, device="meta")
    return _bn_apply("bn_chain", x, None, kind, a, alpha, False, (g1, b1, g2, b2, g3, b3), moving)[0]


def colsum_rows(ds):
    """Gradient of tf.tile over channels: sum over the channel axis (1-channel input)."""
    # rows are tiny (C floats); reuse the column-sum kernel on the transposed problem is not worth it:
    # the 1-channel image never requires grad in the reference (placeholder), so this is only reached in tests.
    return ds.sum(dim=-1, keepdim=True)


def bn_act(x, gamma, beta, act=None, alpha=None, residual=None, tile=False, moving_mean=None, moving_var=None, want_stats=False):
    """tf.layers.batch_normalization(x (+ residual), training=True) followed by `act`.
    tile=True: x has one channel and is broadcast to gamma.numel() channels (tf.tile, networks.py:258)."""
    a = ACT[act]
    if _meta(x):
        y = torch.empty(x.shape[:-1] + (gamma.numel(),), device="meta")
        return (y, None, None) if want_stats else y
    y, mean, invstd = _bn_apply("bn_act", x, residual, -1, a, alpha, tile, (gamma, beta) + (None,) * 4,
                                (moving_mean, moving_var) + (None,) * 4)
    return (y, mean, invstd) if want_stats else y


def bn_update_only(x, C, moving_mean, moving_var):
    """A batch-norm layer whose output is unused ('dead', networks.py:358): only its moving-average
    update op runs (it is in UPDATE_OPS, model.py:665-666)."""
    if _meta(x):
        return
    pre = _epilogue_of(x, None, C)
    x = x.contiguous()
    M = x.numel() // C
    _bn_stats(bn_route("stats", M, C, x16=_is16(x), epilogue=pre is not None), x, None, False, M, C, moving_mean, moving_var, pre)


# ---- batch-norm over a channel concat (U-Net decoder, reference networks.py:64-65) -------------------------------------------
# Batch-norm is per channel, so BN(concat(x0, x1)) == concat(BN(x0), BN(x1)) with the matching slices of the ONE variable set
# gamma / beta / moving_* [C0 + C1]: two ordinary launches per pass, no concat tensor; the convolution behind reads the two results
# as its two sources.  The parameter gradients land in the matching slices of the variables' gradient (one sink each).
class _BnConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x1, gamma, beta, mm, mv):
        ctx.slot1 = getattr(x1, "_vnet_slot", None)
        ys, saved, ctx.halves, off = [], [], [], 0
        for x in (x0.contiguous(), x1.contiguous()):
            C = x.shape[-1]
            sl = slice(off, off + C)
            plan, y, mean, invstd, _, _ = _bn_forward("act", x, None, False, C, None, gamma[sl], beta[sl], 0, None,
                                                      mm[sl] if mm is not None else None, mv[sl] if mv is not None else None)
            ys.append(y)
            saved += [x, mean, invstd]
            ctx.halves.append((plan, sl))
            off += C
        ctx.save_for_backward(gamma, beta, *saved)
        ctx.params = (gamma, beta)
        return ys[0], ys[1]

    @staticmethod
    def backward(ctx, dy0, dy1):
        gamma, beta = ctx.saved_tensors[:2]
        gref, bref = ctx.params
        dgamma, sg = _grad_out(gref)
        dbeta, sbt = _grad_out(bref)
        out = []
        for k, (dy, (plan, sl)) in enumerate(zip((dy0, dy1), ctx.halves)):
            x, mean, invstd = ctx.saved_tensors[2 + 3 * k:5 + 3 * k]
            dy = dy.contiguous()
            ds = torch.empty_like(dy) if ctx.needs_input_grad[k] else None
            _bn_backward(plan, dy, x, None, mean, invstd, gamma[sl], beta[sl], None, dgamma[sl], dbeta[sl], None, ds)
            out.append(ds)
        if out[1] is not None and ctx.slot1 is not None and ctx.slot1.first is None:
            ctx.slot1.first = out[1]                     # the skip feature's other consumer (the max-pooling) adds its gradient into this
        return out[0], out[1], _grad_ret(dgamma, sg), _grad_ret(dbeta, sbt), None, None


def bn_concat(x0, x1, gamma, beta, moving_mean=None, moving_var=None):
    """tf.layers.batch_normalization(tf.concat((x0, x1), -1), training=True) (reference networks.py:64-65) as its two halves
    (y0, y1): gamma / beta / moving_* have C0 + C1 elements."""
    if gamma.numel() != x0.shape[-1] + x1.shape[-1] or tuple(x0.shape[:-1]) != tuple(x1.shape[:-1]):
        raise VnetHipError("bn_concat: %s | %s against %d batch-norm channels" % (tuple(x0.shape), tuple(x1.shape), gamma.numel()))
    if _meta(x0):
        return torch.empty(x0.shape, device="meta"), torch.empty(x1.shape, device="meta")
    _need_gpu(x0, "bn_concat")
    _need_gpu(x1, "bn_concat")
    return _BnConcatFn.apply(x0, x1, gamma, beta, moving_mean, moving_var)


# ---- 2x2x2 stride-2 VALID max-pooling (U-Net encoder, reference networks.py:120; include/vnet_hip_unet.h) --------------------
class _MaxPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        L = _lib.lib()
        ctx.slot = getattr(x, "_vnet_slot", None)
        x = x.contiguous()
        B, D, H, W, C = x.shape
        y = torch.empty((B, D // 2, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
        with _Timed("maxpool2 fwd %d^3x%d %d" % (W, B, C), 0.0, 4.0 * (x.numel() + y.numel())):
            check(L.vnet_maxpool2_fwd(_ptr(x), _ptr(y), C, B, D, H, W, _stream()), "vnet_maxpool2_fwd")
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, y = ctx.saved_tensors
        dy = dy.contiguous()
        B, D, H, W, C = x.shape
        # x's other consumer (the decoder's skip connection) reported its gradient already: add this one into it (ops.fork)
        acc = _slot_target(ctx.slot, dy, x.shape)
        dx = acc if acc is not None else torch.empty_like(x)
        with _Timed("maxpool2 bwd %d^3x%d %d" % (W, B, C), 0.0, 4.0 * (2 * dy.numel() + (3 if acc is not None else 2) * x.numel())):
            check(L.vnet_maxpool2_bwd(_ptr(dy), _ptr(x), _ptr(y), _ptr(dx), C, B, D, H, W, int(acc is not None), _stream()),
                  "vnet_maxpool2_bwd")
        if acc is None and ctx.slot is not None and ctx.slot.first is None:
            ctx.slot.first = dx
        return None if acc is not None else dx


def max_pool2(x):
    """tf.nn.max_pool3d(x, [1,2,2,2,1], [1,2,2,2,1], 'VALID') (reference networks.py:120): odd axes floor.  The gradient of a window
    goes to its first maximum in (z, y, x) scan order."""
    if x.dim() != 5:
        raise NotImplementedError("only the 3-D (NDHWC) path is built; 2-D is out of scope (SURVEY section 2 row 11)")
    if min(int(v) for v in x.shape[1:4]) < 2:
        raise VnetHipError("max_pool2: every spatial axis must be at least 2, got %s" % (tuple(x.shape[1:4]),))
    if _meta(x):
        return torch.empty((x.shape[0],) + tuple(int(v) // 2 for v in x.shape[1:4]) + (x.shape[-1],), device="meta")
    _need_gpu(x, "max_pool2")
    return _MaxPool2Fn.apply(x)


# ---- resampling onto a grid of another voxel spacing (include/vnet_hip_resample.h; rules: vnet_tensorflow_amd/resample.py) -----
def resample(x, out_size, ratio, mode="linear", divisor=None):
    """The reference's `Resample` geometry on device tensors, no autograd: output index i_a reads x at the continuous index
    i_a * ratio[a] (ratio = output spacing / source spacing, doubles); samples at or past n_a - 0.5 are 0.
    mode "linear": x float32 [X,Y,Z,C] or [X,Y,Z] -> float32 out_size (+ C); divisor float32 [X,Y,Z]: every tap is x / divisor in
    double (0 where the divisor is 0) -- the sliding window's count map.  mode "nearest": x int32 [X,Y,Z] -> int32 out_size."""
    if mode not in ("linear", "nearest"):
        raise ValueError("resample: mode %r (linear | nearest)" % (mode,))
    out_size, ratio = tuple(int(v) for v in out_size), tuple(float(v) for v in ratio)
    if len(out_size) != 3 or len(ratio) != 3:
        raise ValueError("resample: out_size and ratio take three values each")
    if x.dim() not in ((3,) if mode == "nearest" else (3, 4)):
        raise VnetHipError("resample: %s takes %s, got a %d-d tensor" % (mode, "[X,Y,Z]" if mode == "nearest" else "[X,Y,Z] or [X,Y,Z,C]", x.dim()))
    if divisor is not None and (mode != "linear" or tuple(divisor.shape) != tuple(x.shape[:3])):
        raise VnetHipError("resample: the divisor goes with mode 'linear' and has the shape of x's voxels")
    shape = out_size + tuple(x.shape[3:])
    if _meta(x):
        return torch.empty(shape, dtype=x.dtype, device="meta")
    if not x.is_cuda or (divisor is not None and not divisor.is_cuda):
        raise VnetHipError("resample: tensor on %s -- the HIP library is the only compute path (no CPU fallback)" % (x.device,))
    want = torch.float32 if mode == "linear" else torch.int32
    if x.dtype != want or (divisor is not None and divisor.dtype != torch.float32):
        raise VnetHipError("resample: mode %r expects %s, got %s" % (mode, want, x.dtype))
    L = _lib.lib()
    x = x.contiguous()
    X, Y, Z = (int(v) for v in x.shape[:3])
    y = torch.empty(shape, dtype=want, device=x.device)
    if mode == "nearest":
        with _Timed("resample nearest %dx%dx%d" % out_size, 0.0, 8.0 * y.numel()):
            check(L.vnet_resample_nearest_i32(_ptr(x), _ptr(y), X, Y, Z, *out_size, *ratio, _stream()), "vnet_resample_nearest_i32")
        return y
    C = int(x.shape[3]) if x.dim() == 4 else 1
    dv = divisor.contiguous() if divisor is not None else None
    with _Timed("resample linear %dx%dx%d %d" % (out_size + (C,)), 0.0, 4.0 * (x.numel() + y.numel() + (dv.numel() if dv is not None else 0))):
        check(L.vnet_resample_linear(_ptr(x), _ptr(dv), _ptr(y), C, X, Y, Z, *out_size, *ratio, _stream()), "vnet_resample_linear")
    return y


# ---- free-form deformation (include/vnet_hip_deform.h; rules: vnet_tensorflow_amd/deform.py) ------------------------------------
def bspline_deform(x, coef, spacing, kind="image"):
    """The reference's `BSplineDeformation` on device tensors, no autograd: every voxel reads x at its own index plus the cubic B-spline
    displacement of the 13^3 control grid `coef` (6591 doubles in ITK's layout; a float64 tensor on x's device, or anything
    torch.as_tensor takes, which is then uploaded), linear interpolation, 0 outside.  kind "image": x float32 [X,Y,Z,C] or [X,Y,Z] ->
    float32; kind "label": x int32 [X,Y,Z] -> int32, the blend truncated toward zero.  x keeps its storage when it is dense (a view
    that starts off a 16-byte boundary takes the one-channel path).  Launches on torch's current stream of the calling thread."""
    if kind not in ("image", "label"):
        raise ValueError("bspline_deform: kind %r (image | label)" % (kind,))
    spacing = tuple(float(v) for v in spacing)
    if len(spacing) != 3:
        raise ValueError("bspline_deform: spacing takes three values")
    if x.dim() not in ((3,) if kind == "label" else (3, 4)):
        raise VnetHipError("bspline_deform: %s takes %s, got a %d-d tensor" % (kind, "[X,Y,Z]" if kind == "label" else "[X,Y,Z] or [X,Y,Z,C]", x.dim()))
    ncoef = int(coef.numel()) if isinstance(coef, torch.Tensor) else int(len(coef))
    if ncoef != 3 * 13 ** 3:
        raise ValueError("bspline_deform: the control grid has %d parameters, got %d" % (3 * 13 ** 3, ncoef))
    if _meta(x):
        return torch.empty(tuple(x.shape), dtype=x.dtype, device="meta")
    if not x.is_cuda:
        raise VnetHipError("bspline_deform: tensor on %s -- the HIP library is the only compute path (no CPU fallback)" % (x.device,))
    want = torch.float32 if kind == "image" else torch.int32
    if x.dtype != want:
        raise VnetHipError("bspline_deform: kind %r expects %s, got %s" % (kind, want, x.dtype))
    if not (isinstance(coef, torch.Tensor) and coef.device == x.device and coef.dtype == torch.float64):
        coef = torch.as_tensor(coef, dtype=torch.float64).to(x.device)
    L = _lib.lib()
    x, coef = x.contiguous(), coef.contiguous()
    X, Y, Z = (int(v) for v in x.shape[:3])
    C = int(x.shape[3]) if x.dim() == 4 else 1
    y = torch.empty(tuple(x.shape), dtype=want, device=x.device)
    stream = _thread_stream(x.device)          # (this op also runs on loader threads, inside side_work)
    entry = "vnet_bspline_deform_f32" if kind == "image" else "vnet_bspline_deform_i32"
    with _Timed("bspline_deform %s %dx%dx%d %d" % (kind, X, Y, Z, C), 0.0, 4.0 * (x.numel() + y.numel())):
        check(getattr(L, entry)(_ptr(x), _ptr(y), X, Y, Z, C, _ptr(coef), *spacing, stream), entry)
    return y


# ---- device work of a thread other than the training loop's (loader threads) -----------------------------------------------------
# The training step is captured into a hipGraph once and replayed; a launch, an allocation or a copy that another thread makes while
# the capture is open can end up inside it or invalidate it.  side_work() is the one door for such threads: a process-wide lock that
# model._build_step_graph holds around its capture, so nothing of a loader thread can fall inside a capture by construction; a
# stream of the thread's own, so its work orders against nothing of the step's streams; and a synchronise of that stream alone
# before the lock is released, so what the thread enqueued is finished -- its tensors can be freed and its pinned results read --
# before a capture can begin.
_SIDE_LOCK = threading.RLock()
_SIDE_LOCAL = threading.local()


def capture_lock():
    """The lock of side_work(): hold it around a stream capture."""
    return _SIDE_LOCK


@contextlib.contextmanager
def side_work(device):
    """Inside: torch's current stream (of this thread) is this thread's side stream on `device`, and no stream capture of
    model._build_step_graph is open or can begin.  Yields the stream.  On exit the stream is synchronised, then the lock released."""
    device = torch.device(device)
    if device.type != "cuda":
        raise VnetHipError("side_work: device %s -- the HIP library is the only compute path (no CPU fallback)" % (device,))
    with _SIDE_LOCK:
        streams = _SIDE_LOCAL.__dict__.setdefault("streams", {})
        st = streams.get(device)
        if st is None:
            st = streams[device] = torch.cuda.Stream(device=device)
        try:
            with torch.cuda.stream(st):
                yield st
        finally:
            st.synchronize()


def pinned_staging(name, shape, dtype):
    """A pinned host tensor of this thread, kept and reused under `name` (grown when a larger one is asked for): the source and the
    destination of side_work's asynchronous copies.  Valid until the thread's next request under the same name."""
    bufs = _SIDE_LOCAL.__dict__.setdefault("pinned", {})
    n = 1
    for v in shape:
        n *= int(v)
    buf = bufs.get((name, dtype))
    if buf is None or buf.numel() < n:
        buf = bufs[(name, dtype)] = torch.empty(max(n, 1), dtype=dtype, pin_memory=True)
    return buf[:n].view(tuple(int(v) for v in shape))


# ---- connected components and the two label filters of evaluate (include/vnet_hip_components.h) -------------------------------
def _cc_label(label, what):
    """The label map as the kernels take it: int32 [X,Y,Z], contiguous.  Foreground is label != 0 whatever the class, so a map of another
    dtype goes in as its 0/1 mask (exact for every dtype; a cast of the values could wrap a class to 0)."""
    if label.dim() != 3 or label.numel() == 0:
        raise VnetHipError("%s: takes a non-empty [X,Y,Z] label map, got %s" % (what, tuple(label.shape)))
    _need_gpu(label, what, any_dtype=True)
    return (label if label.dtype == torch.int32 else (label != 0).to(torch.int32)).contiguous()


def _cc_host(label, fn, *args):
    """The host function of model.py on a device label map (the route of volumes the kernels' int32 index cannot hold, and of class
    counts past the reference's uint8 cast); the 0/1 result goes back to the label's device."""
    return torch.from_numpy(fn(label.cpu().numpy(), *args)).to(label.device)


def _voxel_volume(spacing):
    import numpy as np
    return float(np.prod(spacing))                   # the double the host function forms (model.volume_threshold)


def component_roots(label, sizes=False):
    """Face-connected (6 neighbours) components of label != 0, all non-zero classes one mask: int32 [X,Y,Z], every foreground voxel
    holds its component's smallest linear index, the background -1.  sizes=True: also int32 [X,Y,Z] with the component's voxel
    count at its representative and 0 elsewhere."""
    x = _cc_label(label, "component_roots")
    X, Y, Z = (int(v) for v in x.shape)
    roots = torch.empty((X, Y, Z), dtype=torch.int32, device=x.device)
    cnt = torch.empty((X, Y, Z), dtype=torch.int32, device=x.device) if sizes else None
    with _Timed("cc roots %dx%dx%d" % (X, Y, Z), 0.0, 4.0 * x.numel() * (4 if sizes else 3)):
        check(_lib.lib().vnet_cc_roots(_ptr(x), _ptr(roots), _ptr(cnt), X, Y, Z, _stream()), "vnet_cc_roots")
    return (roots, cnt) if sizes else roots


def _cc_filter(x, entry, *args):
    L = _lib.lib()
    X, Y, Z = (int(v) for v in x.shape)
    need = L.vnet_cc_ws_bytes(X, Y, Z)
    if need == 0:
        return None                                  # more voxels than an int32 indexes: the caller takes the host function
    fn = getattr(L, entry)
    out = torch.empty((X, Y, Z), dtype=torch.uint8, device=x.device)
    ws = workspace(need, x.device)
    with _Timed("%s %dx%dx%d" % (entry[5:], X, Y, Z), 0.0, 25.0 * x.numel()):
        check(fn(_ptr(x), _ptr(out), X, Y, Z, *args, _ptr(ws), need, _stream()), entry)
    return out


def largest_component(label, classes=None, min_volume=None, spacing=(1.0, 1.0, 1.0)):
    """model.ExtractLargestConnectedComponents on a device label map: uint8 [X,Y,Z], 1 on the face-connected component of label != 0
    with the most voxels (of equal counts the one whose first voxel comes first in C order), 0 elsewhere.
    min_volume: model.volume_threshold(result, min_volume, spacing) applied as well -- the result is one component, so it stays iff
    count * prod(spacing) > min_volume.
    classes: the number of classes K (labels in [0, K)).  The reference casts the label to uint8 first; for K <= 255 that changes
    nothing, a larger K takes the host function.  Not given: the label's range is read back from the device to decide."""
    from . import model as _model
    x = _cc_label(label, "largest_component")
    if classes is None:
        lo, hi = (int(v) for v in torch.aminmax(label))
        classes = 256 if (lo < -255 or hi > 255) else 2
    out = None
    if int(classes) <= 255:
        out = _cc_filter(x, "vnet_cc_largest", int(min_volume is not None), float(min_volume) if min_volume is not None else 0.0,
                         _voxel_volume(spacing) if min_volume is not None else 1.0)
    if out is None:
        out = _cc_host(label, _model.ExtractLargestConnectedComponents, spacing)
        if min_volume is not None:
            out = _cc_host(out, _model.volume_threshold, min_volume, spacing)
    return out


def volume_threshold(label, volume, spacing=(1.0, 1.0, 1.0)):
    """model.volume_threshold on a device label map: uint8 [X,Y,Z], 1 on every face-connected component of label != 0 whose voxel
    count times prod(spacing) exceeds `volume` (compared in double, strictly), 0 elsewhere."""
    from . import model as _model
    x = _cc_label(label, "volume_threshold")
    out = _cc_filter(x, "vnet_cc_volume_threshold", float(volume), _voxel_volume(spacing))
    return out if out is not None else _cc_host(label, _model.volume_threshold, volume, spacing)


# ---- the training pipeline's random tail on device-resident cases (include/vnet_hip_sample.h; rules: vnet_tensorflow_amd/sample.py) ----
# These run on loader threads inside side_work: they launch on torch's current stream of the CALLING thread, never on the redirect of
# the parameter-gradient section (_LAUNCH_ON is process-wide and belongs to the training step).
CC_ROW = 8                 # VNET_CC_ROW: representative, count, lo[3], hi[3]


def _sample_label(label, what):
    if label.dim() != 3 or label.numel() == 0:
        raise VnetHipError("%s: takes a non-empty [X,Y,Z] label map, got %s" % (what, tuple(label.shape)))
    _need_gpu(label, what, any_dtype=True)
    if label.dtype != torch.int32 or not label.is_contiguous():
        raise VnetHipError("%s: the label map is a contiguous int32 tensor, got %s" % (what, label.dtype))
    return tuple(int(v) for v in label.shape)


def _three(v, what):
    v = tuple(int(x) for x in v)
    if len(v) != 3:
        raise ValueError("%s takes three values" % what)
    return v


def component_table(label, max_components=4096, ws=None):
    """The face-connected components of label != 0 (int32 [X,Y,Z] on the device) as a table: (n, int32 NumPy array
    [min(n, max_components), 8]), row k = {representative, voxel count, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z} (hi inclusive) of
    scipy.ndimage.label's component k + 1; n is the true number of components also when it exceeds max_components.  One read-back.
    ws: a uint8 device tensor of at least vnet_cc_table_ws_bytes; None = ops.workspace (the training loop's thread only: a loader
    thread passes its own)."""
    X, Y, Z = _sample_label(label, "component_table")
    cap = int(max_components)
    if cap < 1:
        raise ValueError("component_table: max_components %d" % cap)
    L = _lib.lib()
    need = L.vnet_cc_table_ws_bytes(X, Y, Z)
    if need == 0:
        raise VnetHipError("component_table: %dx%dx%d has more voxels than an int32 indexes" % (X, Y, Z))
    if ws is None:
        ws = workspace(need, label.device)
    elif ws.numel() * ws.element_size() < need:
        raise VnetHipError("component_table: ws holds %d bytes, %d needed" % (ws.numel() * ws.element_size(), need))
    out = torch.empty(cap * CC_ROW + 1, dtype=torch.int32, device=label.device)       # the rows, then n: one copy brings both
    with _Timed("cc table %dx%dx%d" % (X, Y, Z), 0.0, 4.0 * label.numel() * 7):
        check(L.vnet_cc_table(_ptr(label), out.data_ptr() + 4 * cap * CC_ROW, _ptr(out), cap, X, Y, Z, _ptr(ws), need,
                              _thread_stream(label.device)), "vnet_cc_table")
    host = out.cpu().numpy()
    n = int(host[-1])
    return n, host[:min(n, cap) * CC_ROW].reshape(-1, CC_ROW).copy()


def window_count(label, start, size, lo, hi):
    """(number of voxels with lo <= label <= hi, sum of the labels) over the window start .. start + size of an int32 [X,Y,Z] device
    label map, as Python ints.  One read-back."""
    X, Y, Z = _sample_label(label, "window_count")
    start, size = _three(start, "window_count: start"), _three(size, "window_count: size")
    out = torch.empty(2, dtype=torch.int64, device=label.device)
    check(_lib.lib().vnet_window_count(_ptr(label), _ptr(out), X, Y, Z, *start, *size, int(lo), int(hi), _thread_stream(label.device)),
          "vnet_window_count")
    c, s = out.tolist()
    return int(c), int(s)


def sample_patch(image, label, start, patch, flip, sigma, seed, out_image, out_label):
    """One sample of a batch, written in place: out_image (float32 [P0,P1,P2,C]) and out_label (int32 [P0,P1,P2] or [P0,P1,P2,1]) get
    the window of `patch` voxels at `start` of image (float32 [X,Y,Z,C]) and label (int32 [X,Y,Z]), axis a reversed within the patch
    where bit a of `flip` is set, plus sigma * N(0, 1) on the image, the deviates a function of (seed, output element) alone
    (vnet_tensorflow_amd/sample.py).  sigma 0: the crop bit for bit.  The outputs are the caller's slots: dense, any 4-byte offset (an
    image slot off a 16-byte boundary takes the one-channel path, with the same values)."""
    X, Y, Z = _sample_label(label, "sample_patch")
    start, patch = _three(start, "sample_patch: start"), _three(patch, "sample_patch: patch")
    if image.dim() != 4 or tuple(image.shape[:3]) != (X, Y, Z):
        raise VnetHipError("sample_patch: image %s does not go with label %s" % (tuple(image.shape), (X, Y, Z)))
    C = int(image.shape[3])
    for t in (image, out_image):
        _need_gpu(t, "sample_patch")
    _need_gpu(out_label, "sample_patch", any_dtype=True)
    if out_label.dtype != torch.int32:
        raise VnetHipError("sample_patch: out_label is int32, got %s" % (out_label.dtype,))
    if tuple(out_image.shape) != patch + (C,) or tuple(out_label.shape) not in (patch, patch + (1,)):
        raise VnetHipError("sample_patch: outputs %s / %s for a patch %s of %d channel(s)" % (tuple(out_image.shape), tuple(out_label.shape), patch, C))
    if not (image.is_contiguous() and out_image.is_contiguous() and out_label.is_contiguous()):
        raise VnetHipError("sample_patch: image and both slots are dense")
    if any(s < 0 or s + p > n for s, p, n in zip(start, patch, (X, Y, Z))):
        raise ValueError("sample_patch: window %s + %s leaves the volume %s" % (start, patch, (X, Y, Z)))
    with _Timed("sample patch %dx%dx%d %d" % (patch + (C,)), 0.0, 8.0 * out_image.numel() + 8.0 * out_label.numel()):
        check(_lib.lib().vnet_sample_patch(_ptr(image), _ptr(label), _ptr(out_image), _ptr(out_label), X, Y, Z, C, *start, *patch,
                                           int(flip), float(sigma), int(seed) & (2 ** 64 - 1), _thread_stream(image.device)),
              "vnet_sample_patch")


def deform_sample_patch(image, deformed_label, coef, spacing, start, patch, flip, sigma, seed, out_image, out_label):
    """One sample of a batch cut THROUGH the free-form deformation, written in place (include/vnet_hip_deform_sample.h): out_image
    (float32 [P0,P1,P2,C]) gets, bit for bit, what sample_patch(bspline_deform(image, coef, spacing), ...) writes for the same window,
    flip, sigma and seed -- only the window's voxels are deformed, the deformed image is never formed --, out_label (int32 [P0,P1,P2] or
    [P0,P1,P2,1]) the flipped window of deformed_label, the caller's bspline_deform(label, coef, spacing, "label").  image is the
    UNDEFORMED case (float32 [X,Y,Z,C]); coef the 6591 doubles of the control grid, a float64 tensor on the image's device.  The
    restatement is vnet_tensorflow_amd.sample.deform_patch.  On meta tensors: the checks of shapes and dtypes, nothing written."""
    spacing = tuple(float(v) for v in spacing)
    if len(spacing) != 3:
        raise ValueError("deform_sample_patch: spacing takes three values")
    start, patch = _three(start, "deform_sample_patch: start"), _three(patch, "deform_sample_patch: patch")
    tensors = (image, deformed_label, coef, out_image, out_label)
    meta = _meta(*tensors)
    if meta and not all(t.device.type == "meta" for t in tensors):
        raise VnetHipError("deform_sample_patch: meta tensors go with meta tensors")
    if not meta:
        for t in (image, out_image):
            _need_gpu(t, "deform_sample_patch")
        for t in (deformed_label, coef, out_label):
            _need_gpu(t, "deform_sample_patch", any_dtype=True)
    if deformed_label.dim() != 3 or deformed_label.numel() == 0 or deformed_label.dtype != torch.int32 or out_label.dtype != torch.int32:
        raise VnetHipError("deform_sample_patch: the label map is a non-empty int32 [X,Y,Z] tensor and out_label int32, got %s %s / %s" % (
            deformed_label.dtype, tuple(deformed_label.shape), out_label.dtype))
    if image.dtype != torch.float32 or out_image.dtype != torch.float32:
        raise VnetHipError("deform_sample_patch: expected float32, got %s / %s" % (image.dtype, out_image.dtype))
    X, Y, Z = (int(v) for v in deformed_label.shape)
    if image.dim() != 4 or tuple(image.shape[:3]) != (X, Y, Z):
        raise VnetHipError("deform_sample_patch: image %s does not go with label %s" % (tuple(image.shape), (X, Y, Z)))
    C = int(image.shape[3])
    if coef.dtype != torch.float64 or coef.numel() != 3 * 13 ** 3:
        raise VnetHipError("deform_sample_patch: the control grid is %d float64 values, got %d %s" % (3 * 13 ** 3, coef.numel(), coef.dtype))
    if tuple(out_image.shape) != patch + (C,) or tuple(out_label.shape) not in (patch, patch + (1,)):
        raise VnetHipError("deform_sample_patch: outputs %s / %s for a patch %s of %d channel(s)" % (
            tuple(out_image.shape), tuple(out_label.shape), patch, C))
    if not all(t.is_contiguous() for t in tensors):
        raise VnetHipError("deform_sample_patch: image, label, control grid and both slots are dense")
    if any(s < 0 or s + p > n for s, p, n in zip(start, patch, (X, Y, Z))):
        raise ValueError("deform_sample_patch: window %s + %s leaves the volume %s" % (start, patch, (X, Y, Z)))
    if not all(math.isfinite(s) and s > 0 for s in spacing):
        raise ValueError("deform_sample_patch: spacing must be three finite positive values, got %s" % (spacing,))
    if meta:
        return
    # 8 taps per element at worst (neighbouring voxels share them through the caches), the label window, both outputs
    with _Timed("deform sample patch %dx%dx%d %d" % (patch + (C,)), 0.0, 36.0 * out_image.numel() + 8.0 * out_label.numel()):
        check(_lib.lib().vnet_deform_sample_patch(_ptr(image), _ptr(deformed_label), _ptr(coef), _ptr(out_image), _ptr(out_label),
                                                  X, Y, Z, C, *spacing, *start, *patch, int(flip), float(sigma),
                                                  int(seed) & (2 ** 64 - 1), _thread_stream(image.device)),
              "vnet_deform_sample_patch")


# ---- scoring a label map against its ground truth (include/vnet_hip_score.h; rules: vnet_tensorflow_amd/score.py) -----------------
# No autograd.  They launch on the stream the label filters of evaluate launch on, and take their scratch from ops.workspace.
OVERLAP_MAX_LABELS = 1024  # VNET_OVERLAP_MAX_LABELS


def label_overlap(a, b, L):
    """Per-label overlap counts of two int32 device label maps of one shape, labels 0 .. L - 1: an int64 NumPy array [L + 1, 3], row
    l < L = {#(a == l and b == l), #(a == l), #(b == l)}, row L = {0, #(a outside [0, L)), #(b outside [0, L))}.  One read-back."""
    for t in (a, b):
        _need_gpu(t, "label_overlap", any_dtype=True)
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() == 0:
            raise VnetHipError("label_overlap: the label maps are contiguous, non-empty int32 tensors, got %s %s" % (t.dtype, tuple(t.shape)))
    if tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise VnetHipError("label_overlap: maps %s on %s and %s on %s" % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    L = int(L)
    if not 1 <= L <= OVERLAP_MAX_LABELS:
        raise ValueError("label_overlap: 1 <= L <= %d, got %d" % (OVERLAP_MAX_LABELS, L))
    out = torch.empty((L + 1, 3), dtype=torch.int64, device=a.device)
    with _Timed("label overlap %d L%d" % (a.numel(), L), 0.0, 8.0 * a.numel()):
        check(_lib.lib().vnet_label_overlap(_ptr(a), _ptr(b), _ptr(out), a.numel(), L, _stream()), "vnet_label_overlap")
    return out.cpu().numpy()


def component_shapes(label, max_components=4096):
    """component_table with the index sums that make a centroid of a row: (n, int32 NumPy array [m, 8], int64 NumPy array [m, 3]), m =
    min(n, max_components); row k = {representative, voxel count, lo[3], hi[3]} of scipy.ndimage.label's component k + 1 of label != 0
    (int32 [X,Y,Z] on the device), sums[k] = {sum x, sum y, sum z} over its voxels; n is the true number of components also when it
    exceeds max_components.  Scratch from ops.workspace; the table and the sums come down, nothing else."""
    X, Y, Z = _sample_label(label, "component_shapes")
    cap = int(max_components)
    if cap < 1:
        raise ValueError("component_shapes: max_components %d" % cap)
    L = _lib.lib()
    need = L.vnet_cc_shape_ws_bytes(X, Y, Z)
    if need == 0:
        raise VnetHipError("component_shapes: %dx%dx%d has more voxels than an int32 indexes" % (X, Y, Z))
    ws = workspace(need, label.device)
    out = torch.empty(cap * CC_ROW + 1, dtype=torch.int32, device=label.device)       # the rows, then n: one copy brings both
    sums = torch.empty((cap, 3), dtype=torch.int64, device=label.device)
    with _Timed("cc shape %dx%dx%d" % (X, Y, Z), 0.0, 4.0 * label.numel() * 7):
        check(L.vnet_cc_shape(_ptr(label), out.data_ptr() + 4 * cap * CC_ROW, _ptr(out), _ptr(sums), cap, X, Y, Z, _ptr(ws), need,
                              _stream()), "vnet_cc_shape")
    host = out.cpu().numpy()
    n = int(host[-1])
    m = min(n, cap)
    return n, host[:m * CC_ROW].reshape(-1, CC_ROW).copy(), sums[:m].cpu().numpy()


# ---- the image summaries of a step as uint8 slices (include/vnet_hip_summary.h; rules: vnet_tensorflow_amd/summary.py) ------------
# No autograd, no scratch.  They launch on torch's current stream of the calling thread.  `out`: None = a new uint8 tensor, or the
# caller's dense uint8 tensor of exactly the result's size (model.py hands out views of ONE buffer, which then leaves in one copy).
SUMMARY_MAX_BLOCKS = 4096  # VNET_SUMMARY_MAX_BLOCKS


def _summary_args(src, what, dtypes, out, shape_of):
    _need_gpu(src, what, any_dtype=True)
    if src.dtype not in dtypes or src.dim() != 5 or src.numel() == 0 or not src.is_contiguous():
        raise VnetHipError("%s: takes a dense, non-empty [B,X,Y,Z,C] tensor of %s, got %s %s" % (
            what, " / ".join(str(d).replace("torch.", "") for d in dtypes), src.dtype, tuple(src.shape)))
    dims = tuple(int(v) for v in src.shape)
    if src.numel() > 2 ** 31 - 1:
        raise VnetHipError("%s: %s has more elements than an int32 counts" % (what, dims))
    shape = shape_of(*dims)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.device != src.device or not out.is_contiguous() or out.numel() != math.prod(shape):
        raise VnetHipError("%s: out is a dense uint8 tensor of %d bytes on the source's device" % (what, math.prod(shape)))
    return dims, out


def summary_slices_intensity(images, out=None):
    """float32 device tensor [B,X,Y,Z,C] -> uint8 [B,C,Z,X,Y]: plane [b][c][z] is the image of height X and width Y the reference logs
    for slice z of channel c (tf.cast to uint8: truncation; below 0 and NaN give 0, above 255 gives 255 -- summary.slices_intensity)."""
    dims, out = _summary_args(images, "summary_slices_intensity", (torch.float32,), out, lambda B, X, Y, Z, C: (B, C, Z, X, Y))
    with _Timed("summary slices f32 %dx%dx%dx%dx%d" % dims, 0.0, 5.0 * images.numel()):
        check(_lib.lib().vnet_summary_slices_f32(_ptr(images), _ptr(out), *dims, _stream()), "vnet_summary_slices_f32")
    return out


def summary_slices_index(index, factor, out=None):
    """int32 (label) or int64 (prediction) device tensor [B,X,Y,Z,C] -> uint8 [B,C,Z,X,Y] = (index * factor) mod 256, the planes
    as summary_slices_intensity orders them (summary.slices_index; factor: summary.index_factor)."""
    dims, out = _summary_args(index, "summary_slices_index", (torch.int32, torch.int64), out, lambda B, X, Y, Z, C: (B, C, Z, X, Y))
    factor = int(factor)
    if not -2 ** 31 <= factor < 2 ** 31:
        raise ValueError("summary_slices_index: factor %d is no int32" % factor)
    L = _lib.lib()
    with _Timed("summary slices index %dx%dx%dx%dx%d" % dims, 0.0, (index.element_size() + 1.0) * index.numel()):
        if index.dtype == torch.int32:
            check(L.vnet_summary_slices_i32(_ptr(index), _ptr(out), factor, *dims, _stream()), "vnet_summary_slices_i32")
        else:
            check(L.vnet_summary_slices_i64(_ptr(index), _ptr(out), factor, *dims, _stream()), "vnet_summary_slices_i64")
    return out


def summary_slices_rainbow(softmax, out=None):
    """float32 device tensor [B,X,Y,Z,K] (the loss head's softmax: fp32 in every ComputeDtype) -> uint8 [B,K,Z,X,Y,3]: the reference's
    grayscale_to_rainbow, times 255, cast to uint8, every fp32 operation rounded on its own (summary.slices_rainbow)."""
    dims, out = _summary_args(softmax, "summary_slices_rainbow", (torch.float32,), out, lambda B, X, Y, Z, K: (B, K, Z, X, Y, 3))
    with _Timed("summary rainbow %dx%dx%dx%dx%d" % dims, 0.0, 7.0 * softmax.numel()):
        check(_lib.lib().vnet_summary_rainbow_f32(_ptr(softmax), _ptr(out), *dims, _stream()), "vnet_summary_rainbow_f32")
    return out


# ---- the bounding-box tool (csrc/vnet_bbox.h, the package's own entry points; rules: vnet_tensorflow_amd/bounding_box.py) ----------
# No autograd.  They launch on torch's current stream of the calling thread, like resample.
def slice_stack(x, axis):
    """float32 or int32 device tensor [X,Y,Z] -> the stack of its slices [S,V,U] along `axis` (2 axial: (Z,Y,X); 1 coronal: (Y,Z,X);
    0 sagittal: (X,Z,Y)), bit for bit (bounding_box.stack)."""
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise ValueError("slice_stack: axis %d (0, 1, 2)" % axis)
    if x.dim() != 3 or x.numel() == 0:
        raise VnetHipError("slice_stack: takes a non-empty [X,Y,Z] tensor, got %s" % (tuple(x.shape),))
    X, Y, Z = (int(v) for v in x.shape)
    shape = {2: (Z, Y, X), 1: (Y, Z, X), 0: (X, Z, Y)}[axis]
    if _meta(x):
        return torch.empty(shape, dtype=x.dtype, device="meta")
    _need_gpu(x, "slice_stack", any_dtype=True)
    if x.dtype not in (torch.float32, torch.int32):
        raise VnetHipError("slice_stack: expected float32 or int32, got %s" % (x.dtype,))
    if x.numel() > 2 ** 31 - 1:
        raise VnetHipError("slice_stack: %dx%dx%d has more voxels than an int32 indexes" % (X, Y, Z))
    x = x.contiguous()
    y = torch.empty(shape, dtype=x.dtype, device=x.device)
    entry = "vnet_slice_stack_f32" if x.dtype == torch.float32 else "vnet_slice_stack_i32"
    with _Timed("slice stack %dx%dx%d axis %d" % (X, Y, Z, axis), 0.0, 8.0 * x.numel()):
        check(getattr(_lib.lib(), entry)(_ptr(x), _ptr(y), X, Y, Z, axis, _thread_stream(x.device)), entry)
    return y


def plane_component_table(stack, max_components=65536, ws=None):
    """The components of an int32 device stack [S,V,U] -- maximal sets of one value > 0 inside one slice, joined through u +- 1 /
    v +- 1 -- as (n, int32 NumPy rows [n, 8], int32 NumPy classes [n]): row k = {representative, count, lo_s, lo_v, lo_u, hi_s, hi_v,
    hi_u} in ascending representative order (bounding_box.plane_components), classes[k] the value at its representative.  One
    read-back; when n exceeds max_components the table is made once more with capacity n.
    ws: a uint8 device tensor of at least vnet_plane_cc_table_ws_bytes; None = ops.workspace."""
    S, V, U = _sample_label(stack, "plane_component_table")
    cap = int(max_components)
    if cap < 1:
        raise ValueError("plane_component_table: max_components %d" % cap)
    L = _lib.lib()
    need = L.vnet_plane_cc_table_ws_bytes(S, V, U)
    if need == 0:
        raise VnetHipError("plane_component_table: %dx%dx%d has more voxels than an int32 indexes" % (S, V, U))
    if ws is None:
        ws = workspace(need, stack.device)
    elif ws.numel() * ws.element_size() < need:
        raise VnetHipError("plane_component_table: ws holds %d bytes, %d needed" % (ws.numel() * ws.element_size(), need))
    for _ in range(2):
        out = torch.empty(cap * CC_ROW + 1, dtype=torch.int32, device=stack.device)   # the rows, then n
        with _Timed("plane cc table %dx%dx%d" % (S, V, U), 0.0, 4.0 * stack.numel() * 7):
            check(L.vnet_plane_cc_table(_ptr(stack), out.data_ptr() + 4 * cap * CC_ROW, _ptr(out), cap, S, V, U, _ptr(ws), need,
                                        _thread_stream(stack.device)), "vnet_plane_cc_table")
        # the class of every row, gathered at the representatives (rows past n hold 0: voxel 0, dropped below): one copy brings all
        cls = stack.reshape(-1)[out[:cap * CC_ROW].reshape(cap, CC_ROW)[:, 0].long()]
        host = torch.cat([out, cls]).cpu().numpy()
        n = int(host[cap * CC_ROW])
        if n <= cap:
            break
        cap = n
    return n, host[:n * CC_ROW].reshape(-1, CC_ROW).copy(), host[cap * CC_ROW + 1:cap * CC_ROW + 1 + n].copy()


def bbox_render(image, label, boxes, first, wmin, wmax, opacity):
    """The picture of every slice, uint8 [S,V,U,3] on the device (bounding_box.render): image float32 and label int32 stacks [S,V,U],
    boxes int32 [nb, 5] rows {x, y, w, h, label} grouped by slice (nb 0: an empty tensor), first int32 [S + 1] offsets into them."""
    S, V, U = _sample_label(label, "bbox_render")
    _need_gpu(image, "bbox_render")
    if tuple(image.shape) != (S, V, U) or not image.is_contiguous():
        raise VnetHipError("bbox_render: image %s does not go with label %s" % (tuple(image.shape), (S, V, U)))
    for t, shape, what in ((boxes, (int(boxes.shape[0]), 5), "boxes [nb, 5]"), (first, (S + 1,), "first [S + 1]")):
        if t.dtype != torch.int32 or t.device != label.device or tuple(t.shape) != shape or not t.is_contiguous():
            raise VnetHipError("bbox_render: %s is a dense int32 tensor on the label's device, got %s %s" % (what, t.dtype, tuple(t.shape)))
    alpha = int(round(float(opacity) * 256))
    if not 0 <= alpha <= 256:
        raise ValueError("bbox_render: opacity %r outside [0, 1]" % (opacity,))
    # float32 arithmetic on the host: scale = float32(255) / (float32(wmax) - float32(wmin)), each operation rounded once
    lo, hi = (torch.tensor(float(v), dtype=torch.float32, device="cpu") for v in (wmin, wmax))
    scale = torch.tensor(255.0, dtype=torch.float32, device="cpu") / (hi - lo)
    rgb = torch.empty((S, V, U, 3), dtype=torch.uint8, device=label.device)
    with _Timed("bbox render %dx%dx%d" % (S, V, U), 0.0, 11.0 * label.numel()):
        check(_lib.lib().vnet_bbox_render(_ptr(image), _ptr(label), _ptr(boxes) if boxes.numel() else None, _ptr(first), _ptr(rgb),
                                          S, V, U, float(lo), float(hi), float(scale), alpha, _thread_stream(label.device)),
              "vnet_bbox_render")
    return rgb


# ---- a case of evaluate on the device (include/vnet_hip_prepare.h; rules: vnet_tensorflow_amd/prepare.py) -------------------------
# No autograd.  They launch on torch's current stream of the calling thread, like resample.
STATS_MAX_BLOCKS = 1024    # VNET_STATS_MAX_BLOCKS: a channel's voxels are spread over at most this many blocks of 256 threads


def _channels_last(x, what):
    """(n, C) of a dense float32 device tensor [..., C] with at least one voxel."""
    _need_gpu(x, what)
    if x.dim() < 2 or x.numel() == 0 or not x.is_contiguous():
        raise VnetHipError("%s: takes a dense, non-empty [..., C] tensor, got %s" % (what, tuple(x.shape)))
    C = int(x.shape[-1])
    return x.numel() // C, C


def _rows(t, C, width, device, what):
    """A per-channel parameter table as the kernels take it: float64 [C, width] on `device` (anything torch.as_tensor takes is uploaded)."""
    if not (isinstance(t, torch.Tensor) and t.device == device and t.dtype == torch.float64):
        t = torch.as_tensor(t, dtype=torch.float64).to(device)
    if tuple(t.shape) != (C, width):
        raise VnetHipError("%s: expected a [%d, %d] table, got %s" % (what, C, width, tuple(t.shape)))
    return t.contiguous()


def channel_stats(image, pre=None):
    """Per-channel statistics of a float32 device tensor [..., C]: a float64 device tensor [C, 4] = {sum, css, min, max} of
    v = (x - a) / b in double, pre = [C, 2] rows {a, b} (None: v = x); css = sum (v - sum / n)^2, the mean formed on the device.
    Summed in a fixed order that differs from NumPy's pairwise one: equal to it where the sums are exact, else within rounding."""
    n, C = _channels_last(image, "channel_stats")
    L = _lib.lib()
    need = L.vnet_channel_stats_ws_bytes(C)
    if need == 0:
        raise VnetHipError("channel_stats: %d channels (at most 65535)" % C)
    if pre is not None:
        pre = _rows(pre, C, 2, image.device, "channel_stats: pre")
    out = torch.empty((C, 4), dtype=torch.float64, device=image.device)
    ws = workspace(need, image.device)
    with _Timed("channel stats %d %d" % (n, C), 0.0, 8.0 * image.numel()):
        check(L.vnet_channel_stats(_ptr(image), _ptr(pre), _ptr(out), n, C, _ptr(ws), need, _stream()), "vnet_channel_stats")
    return out


def window_intensity(image, prm, out=None):
    """transforms._window on a float32 device tensor [..., C], per channel: prm = [C, 5] rows {a, b, wmin, scale, flag}
    (vnet_tensorflow_amd/prepare.py: window_params); v = (x - a) / b, then clip((v - wmin) * scale + 0, 0, 255), or for flag != 0
    v < wmin ? 0 : 255, rounded to float once.  out: None = a new tensor; `image` itself = in place."""
    n, C = _channels_last(image, "window_intensity")
    prm = _rows(prm, C, 5, image.device, "window_intensity: prm")
    if out is None:
        out = torch.empty(tuple(image.shape), dtype=torch.float32, device=image.device)
    elif out is not image:
        if _channels_last(out, "window_intensity") != (n, C) or out.device != image.device:
            raise VnetHipError("window_intensity: out %s for an image %s" % (tuple(out.shape), tuple(image.shape)))
    with _Timed("window intensity %d %d" % (n, C), 0.0, 8.0 * image.numel()):
        check(_lib.lib().vnet_window_intensity(_ptr(image), _ptr(out), _ptr(prm), n, C, _stream()), "vnet_window_intensity")
    return out


def crop_window(src, start, size, out=None):
    """The window of `size` voxels at `start` of a dense device tensor, zero where it reaches past the extent (np.pad, then slice):
    float32 [X,Y,Z,C] -> [P0,P1,P2,C] or int32 [X,Y,Z] -> [P0,P1,P2].  0 <= start < extent on every axis.  out: the caller's slot
    (dense, any 4-byte offset: off a 16-byte boundary it takes the one-word path, with the same values), or None = a new tensor."""
    start, size = _three(start, "crop_window: start"), _three(size, "crop_window: size")
    _need_gpu(src, "crop_window", any_dtype=True)
    if not ((src.dim() == 4 and src.dtype == torch.float32) or (src.dim() == 3 and src.dtype == torch.int32)):
        raise VnetHipError("crop_window: takes float32 [X,Y,Z,C] or int32 [X,Y,Z], got %s %s" % (src.dtype, tuple(src.shape)))
    if src.numel() == 0 or not src.is_contiguous():
        raise VnetHipError("crop_window: the source is dense and not empty")
    X, Y, Z = (int(v) for v in src.shape[:3])
    C = int(src.shape[3]) if src.dim() == 4 else 1
    if any(s < 0 or s >= n or p < 1 for s, p, n in zip(start, size, (X, Y, Z))):
        raise ValueError("crop_window: window %s + %s on a volume %s" % (start, size, (X, Y, Z)))
    shape = size + tuple(src.shape[3:])
    if out is None:
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
    elif tuple(out.shape) != shape or out.dtype != src.dtype or out.device != src.device or not out.is_contiguous():
        raise VnetHipError("crop_window: out is a dense %s tensor %s on the source's device" % (src.dtype, shape))
    with _Timed("crop window %dx%dx%d %d" % (size + (C,)), 0.0, 8.0 * out.numel()):
        check(_lib.lib().vnet_crop_words(_ptr(src), _ptr(out), X, Y, Z, C, *start, *size, _stream()), "vnet_crop_words")
    return out


def argmax_label(vol):
    """float32 device tensor [..., K] -> int32 [...]: the first index of the largest value, a NaN larger than every number
    (torch.argmax(vol, -1) as int32, in one pass and 4 bytes per voxel)."""
    n, K = _channels_last(vol, "argmax_label")
    out = torch.empty(tuple(vol.shape[:-1]), dtype=torch.int32, device=vol.device)
    with _Timed("argmax label %d %d" % (n, K), 0.0, 4.0 * (vol.numel() + n)):
        check(_lib.lib().vnet_argmax_label(_ptr(vol), _ptr(out), n, K, _stream()), "vnet_argmax_label")
    return out


# ---- stand-alone activation (API parity with layers2.prelu; the networks use the fused bn_act) ------------
class _ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha, act):
        L = _lib.lib()
        x = x.contiguous()
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty_like(x)
        check(L.vnet_act_fwd(_ptr(x), M, C, act, _ptr(alpha), _ptr(y), _stream()), "vnet_act_fwd")
        ctx.save_for_backward(x, alpha)
        ctx.act = act
        ctx.aref = alpha
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, alpha = ctx.saved_tensors
        C = x.shape[-1]
        M = x.numel() // C
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dalpha, sa = _grad_out(ctx.aref) if alpha is not None else (None, None)      # straight into the flat gradient buffer when there is one
        nb = L.vnet_bn_ws_bytes(C)
        ws = workspace(nb, x.device)
        check(L.vnet_act_bwd(_ptr(dy), _ptr(x), M, C, ctx.act, _ptr(alpha), _ptr(dalpha), _ptr(dx), _ptr(ws), nb, _stream()),
              "vnet_act_bwd")
        return dx, (_grad_ret(dalpha, sa) if alpha is not None else None), None


def activation(x, act, alpha=None):
    if _meta(x):
        return x
    _need_gpu(x, "activation")
    return _ActFn.apply(x, alpha if ACT[act] == 2 else None, ACT[act])


# ---- 1x1x1 head --------------------------------------------------------------------------------------------
class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        L = _lib.lib()
        x = x.contiguous()
        C, K = w.shape[-2], w.shape[-1]
        M = x.numel() // C
        y = torch.empty(x.shape[:-1] + (K,), dtype=torch.float32, device=x.device)        # logits stay fp32 in every mode
        if _is16(x):
            check(L.vnet_head_fwd_b16(_ptr(x), _ptr(w), _ptr(b), _ptr(y), M, C, K, _stream()), "vnet_head_fwd_b16")
        else:
            check(L.vnet_head_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), M, C, K, _stream()), "vnet_head_fwd")
        ctx.save_for_backward(x, w)
        ctx.params = (w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, w = ctx.saved_tensors
        C, K = w.shape[-2], w.shape[-1]
        M = x.numel() // C
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw, sw = _grad_out(ctx.params[0])
        db, sb = _grad_out(ctx.params[1])
        nb = L.vnet_head_ws_bytes(C, K)
        ws = workspace(nb, x.device)
        if _is16(x):
            check(L.vnet_head_bwd_b16(_ptr(x), _ptr(w), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db), M, C, K, _ptr(ws), nb, _stream()),
                  "vnet_head_bwd_b16")
        else:
            check(L.vnet_head_bwd(_ptr(x), _ptr(w), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db), M, C, K, _ptr(ws), nb, _stream()),
                  "vnet_head_bwd")
        return dx, _grad_ret(dw, sw), _grad_ret(db, sb)


def head_conv(x, w, b):
    """convolution(x, [1,1,1,C,K]) of the output layer (reference networks.py:298-302)."""
    if _meta(x):
        return torch.empty(x.shape[:-1] + (w.shape[-1],), device="meta")
    _need_gpu(x, "head_conv", allow16=True)
    return _HeadFn.apply(x, w, b)


# ---- the decoder's last batch-norm with the head folded in (include/vnet_hip_head.h) ---------------------------------------------
# "stats": the normalise pass also writes the statistics rows of the logits, so the batch-norm behind the head runs only its finalize
# (12 us and a launch at 128^3).  Off: those rows group the voxels differently from vnet_bn_stats, mean / invstd move in the last
# bit, and with them the round-off that is all there is of the head bias's gradient (analytically 0 in front of a batch-norm) --
# which Adam turns into full-size steps of that parameter.  Without it the fused step computes the unfused step's bits.
_HEAD_FUSE = {"on": True, "stats": False}


def set_head_fusion(on, stats=None):
    """on=False: bn_head() runs the unfused sequence (bn_chain / bn_act, then head_conv); stats (None: unchanged): the fused
    normalise pass also produces the logits' batch-norm partial sums.  Returns the previous (on, stats)."""
    prev = (_HEAD_FUSE["on"], _HEAD_FUSE["stats"])
    _HEAD_FUSE["on"] = bool(on)
    if stats is not None:
        _HEAD_FUSE["stats"] = bool(stats)
    return prev


def bn_head(x, w, b, kind, act, alpha, g1, b1, g2=None, b2=None, g3=None, b3=None, residual=None, moving=(None,) * 6):
    """head_conv(y, w, b) of y = bn_chain(x, kind, act, alpha, g1, b1, g2, b2, g3, b3, moving) (kind 0 / 1) or of
    y = bn_act(x, g1, b1, act, alpha, residual, moving_mean=moving[0], moving_var=moving[1]) (kind -1), for a y nothing else reads.
    float32 tensors of 8 or 16 channels run the fused passes of include/vnet_hip_head.h (set_head_fusion(False): never); every
    other case runs the two ops one after the other."""
    a = ACT[act]
    K = int(w.shape[-1])
    C = int(w.shape[-2])
    if _meta(x):
        return torch.empty(x.shape[:-1] + (K,), device="meta")
    fused = (_HEAD_FUSE["on"] and x.dtype == torch.float32 and not storage_is_bf16() and (residual is None or residual.dtype == torch.float32)
             and int(x.shape[-1]) == C and (kind < 0 or residual is None) and _lib.lib().vnet_bn_head_ok(C, K))
    if not fused:
        if kind < 0:
            y = bn_act(x, g1, b1, act, alpha, residual, False, moving[0], moving[1])
        else:
            y = bn_chain(x, kind, act, alpha, g1, b1, g2, b2, g3, b3, moving)
        return head_conv(y, w, b)
    stats = rows = None
    if _HEAD_FUSE["stats"] and _SYNC_BN is None:
        rows = _lib.lib().vnet_bn_head_stats_rows(x.numel() // C, C)
        stats = torch.empty((rows, 2 * K), dtype=torch.float32, device=x.device)
    logits = _bn_apply("bn_head", x, residual, kind, a, alpha, False, (g1, b1, g2, b2, g3, b3), moving, w, b, stats)[0]
    if stats is not None:
        logits._vnet_stats = _EpilogueStats(stats, rows, None)      # the batch-norm behind the head runs only its finalize
    return logits


# ---- fused softmax + Dice / cross-entropy loss ---------------------------------------------------------------
def parse_loss(name):
    """Loss.Name -> kind bits (reference model.py:495-558)."""
    valid = ("xent", "weighted_xent", "sorensen", "weighted_sorensen", "jaccard", "weighted_jaccard",
             "mixed_sorensen", "mixed_weighted_sorensen", "mixed_jaccard", "mixed_weighted_jaccard")
    if name not in valid:
        raise SystemExit("Invalid loss function")
    kind = LOSS_KIND["xent"] if name.endswith("xent") else (LOSS_KIND["sorensen"] if "sorensen" in name else LOSS_KIND["jaccard"])
    if "weighted" in name:
        kind |= LOSS_WEIGHTED
    if name.startswith("mixed_"):
        kind |= LOSS_MIXED
    return kind


_CONST_VEC = {}


def _const_vector(values, device):
    """Small constant vector (Loss.Weights) on the device, uploaded once: a pageable host-to-device copy is not allowed
    inside a stream capture."""
    key = (tuple(float(v) for v in values), device)
    t = _CONST_VEC.get(key)
    if t is None:
        t = _CONST_VEC[key] = torch.as_tensor(list(key[0]), dtype=torch.float32).to(device)
    return t


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, kind, weights, alpha, smooth, want_softmax, want_pred):
        L = _lib.lib()
        logits = logits.contiguous()
        labels = labels.contiguous()
        B, K = logits.shape[0], logits.shape[-1]
        V = logits.numel() // (B * K)
        dev = logits.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        dice = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(2 * B * K + 1, dtype=torch.float32, device=dev)
        sm = torch.empty_like(logits) if want_softmax else None
        pred = torch.empty(logits.shape[:-1], dtype=torch.int64, device=dev) if want_pred else None
        nb = L.vnet_loss_ws_bytes(B, K)
        ws = workspace(nb, dev)
        check(L.vnet_softmax_dice_fwd(_ptr(logits), _ptr(labels), B, V, K, kind, _ptr(weights), alpha, smooth,
                                      _ptr(sm), _ptr(pred), _ptr(loss), _ptr(dice), _ptr(coef), _ptr(ws), nb, _stream()),
              "vnet_softmax_dice_fwd")
        ctx.save_for_backward(logits, labels, weights, coef)
        ctx.cfg = (kind, alpha, B, V, K)
        ctx.mark_non_differentiable(dice)
        ctx.set_materialize_grads(False)
        outs = [loss, dice]
        if sm is not None:
            ctx.mark_non_differentiable(sm)
        if pred is not None:
            ctx.mark_non_differentiable(pred)
        return loss, dice, sm, pred

    @staticmethod
    def backward(ctx, gloss, gdice, gsm, gpred):
        L = _lib.lib()
        logits, labels, weights, coef = ctx.saved_tensors
        kind, alpha, B, V, K = ctx.cfg
        g = gloss.contiguous().to(torch.float32)
        dl = torch.empty_like(logits)
        check(L.vnet_softmax_dice_bwd(_ptr(logits), _ptr(labels), B, V, K, kind, _ptr(weights), alpha, _ptr(coef),
                                      _ptr(g), _ptr(dl), _stream()), "vnet_softmax_dice_bwd")
        return dl, None, None, None, None, None, None, None


def softmax_loss(logits, labels, loss_name="sorensen", weights=None, alpha=1.0, smooth=1e-5,
                 want_softmax=False, want_pred=False):
    """softmax (model.py:447) + one_hot (model.py:474-477) + the loss switch (model.py:495-558).
    labels: int32 [B,D,H,W,1] or [B,D,H,W].  Returns (loss, dice_value, softmax|None, pred|None)."""
    _need_gpu(logits, "softmax_loss")
    kind = parse_loss(loss_name)
    K = logits.shape[-1]
    wt = None
    if kind & LOSS_WEIGHTED:
        if weights is None or len(weights) != K:
            raise AssertionError("Length of DICE weight is {}, should be {}".format(0 if weights is None else len(weights), K))
        wt = _const_vector(weights, logits.device)
    if labels.dtype != torch.int32:
        labels = labels.to(torch.int32)
    return _LossFn.apply(logits, labels, kind, wt, float(alpha), float(smooth), want_softmax, want_pred)


def softmax_argmax(logits):
    """Inference fetches of evaluate (model.py:914-917): 'softmax:0' and 'predicted_label/prediction:0'."""
    _need_gpu(logits, "softmax_argmax")
    lab = torch.zeros(logits.shape[:-1], dtype=torch.int32, device=logits.device)
    with torch.no_grad():
        _, _, sm, pred = _LossFn.apply(logits, lab, 0, None, 1.0, 1e-5, True, True)
    return sm, pred


# ---- dropout ------------------------------------------------------------------------------------------------------
class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rate, seed):
        L = _lib.lib()
        x = x.contiguous()
        mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        st = _STEP_STATE["active"]
        if _is16(x):
            y = torch.empty_like(x)
            check(L.vnet_dropout_fwd_b16(_ptr(x), _ptr(y), _ptr(mask), x.numel(), rate, seed, _ptr(st), _stream()), "vnet_dropout_fwd_b16")
        else:
            y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            check(L.vnet_dropout_fwd_dev(_ptr(x), _ptr(y), _ptr(mask), x.numel(), rate, seed, _ptr(st), _stream()), "vnet_dropout_fwd")
        ctx.save_for_backward(mask)
        ctx.rate = rate
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        (mask,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        if _is16(dy):
            check(L.vnet_dropout_bwd_b16(_ptr(dy), _ptr(mask), _ptr(dx), dy.numel(), ctx.rate, _stream()), "vnet_dropout_bwd_b16")
            return dx, None, None
        check(L.vnet_dropout_bwd(_ptr(dy), _ptr(mask), _ptr(dx), dy.numel(), ctx.rate, _stream()), "vnet_dropout_bwd")
        return dx, None, None


_DROP_SEED = [0x5EED, 0]


def dropout(x, rate):
    """tf.nn.dropout(x, rate=rate) (reference networks.py:321): identity when rate == 0."""
    rate = float(rate)
    if rate == 0.0 or _meta(x):
        return x
    _need_gpu(x, "dropout", allow16=True)
    if _STEP_STATE["active"] is not None:
        # graph-replayable: the seed of a layer is its position in the pass, the step number comes from the device state
        _DROP_SEED[1] += 1
        return _DropoutFn.apply(x, rate, 0x5EED0000 + _DROP_SEED[1])
    _DROP_SEED[0] += 1
    return _DropoutFn.apply(x, rate, _DROP_SEED[0])


def begin_dropout_pass():
    """Reset the per-pass layer counter of the state-driven dropout (called at the start of a step)."""
    _DROP_SEED[1] = 0


# ---- optimiser apply + sliding-window accumulate (no autograd) ----------------------------------------------------
def adam_apply(p, g, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, gscale=1.0, state=None):
    """state: device step-state buffer holding lr_t (then the `lr_t` argument is ignored) -- the graph-replayable form."""
    if state is not None:
        check(_lib.lib().vnet_adam_apply_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(state), beta1, beta2, eps, gscale,
                                             _stream()), "vnet_adam_apply_dev")
        return
    check(_lib.lib().vnet_adam_apply(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr_t, beta1, beta2, eps, gscale, _stream()),
          "vnet_adam_apply")


def sgd_apply(p, g, lr, gscale=1.0, state=None):
    if state is not None:
        check(_lib.lib().vnet_sgd_apply_dev(_ptr(p), _ptr(g), p.numel(), _ptr(state), gscale, _stream()), "vnet_sgd_apply_dev")
        return
    check(_lib.lib().vnet_sgd_apply(_ptr(p), _ptr(g), p.numel(), lr, gscale, _stream()), "vnet_sgd_apply")


def momentum_apply(p, g, acc, lr, momentum, nesterov=False, gscale=1.0, state=None):
    if state is not None:
        check(_lib.lib().vnet_momentum_apply_dev(_ptr(p), _ptr(g), _ptr(acc), p.numel(), _ptr(state), momentum, int(nesterov), gscale,
                                                 _stream()), "vnet_momentum_apply_dev")
        return
    check(_lib.lib().vnet_momentum_apply(_ptr(p), _ptr(g), _ptr(acc), p.numel(), lr, momentum, int(nesterov), gscale, _stream()),
          "vnet_momentum_apply")


def hard_metrics(pred, labels, K):
    """Accuracy and per-class tp/tn/fp/fn, sensitivity, specificity, hard Dice (reference model.py:588-626) from
    the K x K confusion matrix computed on the GPU.  pred int64 [...], labels int32 [...] (class indices)."""
    L = _lib.lib()
    pred = pred.contiguous().reshape(-1)
    labels = labels.to(torch.int32).contiguous().reshape(-1)
    cm = torch.empty(K * K, dtype=torch.float64, device=pred.device)
    nb = L.vnet_confusion_ws_bytes(K)
    ws = workspace(nb, pred.device)
    check(L.vnet_confusion_matrix(_ptr(pred), _ptr(labels), pred.numel(), K, _ptr(cm), _ptr(ws), nb, _stream()),
          "vnet_confusion_matrix")
    return metrics_from_confusion(cm.cpu().numpy().reshape(K, K))


# ---- tf.metrics.auc (reference model.py:607,613,624) ------------------------------------------------------------------
def tf_auc_thresholds(num_thresholds=200):
    """TF 1.15 metrics_impl.auc: kepsilon = 1e-7; [0 - eps] + [(i + 1) / (n - 1) for i in range(n - 2)] + [1 + eps], used as
    float32 constants against float32 predictions."""
    import numpy as np
    eps = 1e-7
    th = [0.0 - eps] + [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)] + [1.0 + eps]
    return np.asarray(th, dtype=np.float32)


def auc_histogram(softmax, labels, K, cls, num_thresholds=200):
    """Counts behind tf.metrics.auc(one_hot(labels)[..., cls], softmax[..., cls]): float64 [2][T+1] on the device --
    row 0 the voxels of class `cls`, row 1 all others; bin = number of thresholds strictly below the prediction."""
    L = _lib.lib()
    sm = softmax.contiguous()
    lab = labels.to(torch.int32).contiguous().reshape(-1)
    n = lab.numel()
    th = _const_vector(tf_auc_thresholds(num_thresholds), sm.device)
    hist = torch.empty((2, num_thresholds + 1), dtype=torch.float64, device=sm.device)
    nb = L.vnet_auc_ws_bytes(num_thresholds)
    ws = workspace(nb, sm.device)
    check(L.vnet_auc_histogram(_ptr(sm), _ptr(lab), n, K, cls, _ptr(th), num_thresholds, _ptr(hist), _ptr(ws), nb, _stream()),
          "vnet_auc_histogram")
    return hist


def auc_from_hist(hist):
    """ROC AUC the way tf.metrics.auc(curve='ROC', summation_method='trapezoidal') evaluates it from its per-threshold
    counters: tp[t] = #{positive, p > thr[t]}, rec = (tp + eps) / (tp + fn + eps), fpr = fp / (fp + tn + eps),
    auc = sum((fpr[:-1] - fpr[1:]) * (rec[:-1] + rec[1:]) / 2)."""
    import numpy as np
    h = np.asarray(hist, dtype=np.float64)
    eps = 1e-7
    tp = h[0][::-1].cumsum()[::-1][1:]          # tp[t] = sum_{b > t} hist_pos[b]
    fp = h[1][::-1].cumsum()[::-1][1:]
    fn, tn = h[0].sum() - tp, h[1].sum() - fp
    rec = (tp + eps) / (tp + fn + eps)
    fpr = fp / (fp + tn + eps)
    return float(((fpr[:-1] - fpr[1:]) * (rec[:-1] + rec[1:]) / 2.0).sum())


class StreamingMetrics(object):
    """The tf.metrics of reference model.py:588-626: accumulating (like TF's local variables, over every update since
    construction) confusion counts and AUC counters; result() gives accuracy of the LAST batch (model.py:590 is not
    streaming) and per class i > 0: tp/tn/fp/fn, sensitivity, specificity, hard Dice 2tp/(2tp+fp+fn) and the ROC AUC."""

    def __init__(self, K, num_thresholds=200):
        self.K, self.T = K, num_thresholds
        self.cm = None
        self.hist = [None] * K
        self.last_accuracy = None

    def update(self, pred, labels, softmax=None):
        import numpy as np
        m = hard_metrics(pred, labels, self.K)
        self.last_accuracy = m["accuracy"]
        self.cm = m["confusion"] if self.cm is None else self.cm + m["confusion"]
        if softmax is not None:
            for c in range(1, self.K):
                h = auc_histogram(softmax, labels, self.K, c, self.T).cpu().numpy()
                self.hist[c] = h if self.hist[c] is None else self.hist[c] + h
        return self

    def result(self):
        out = metrics_from_confusion(self.cm)
        out["accuracy"] = self.last_accuracy
        for c in range(1, self.K):
            if self.hist[c] is not None:
                out[c]["auc"] = auc_from_hist(self.hist[c])
        return out


def metrics_from_confusion(cm):
    K = cm.shape[0]
    n = cm.sum()
    out = {"accuracy": float(cm.trace() / max(n, 1.0)), "confusion": cm}
    for c in range(K):
        tp = cm[c, c]; fn = cm[c].sum() - tp; fp = cm[:, c].sum() - tp; tn = n - tp - fn - fp
        out[c] = {"tp": tp, "tn": tn, "fp": fp, "fn": fn,
                  "sensitivity": float(tp / max(tp + fn, 1e-30)), "specificity": float(tn / max(tn + fp, 1e-30)),
                  "dice": float(2 * tp / max(2 * tp + fp + fn, 1e-30))}
    return out


def accumulate_patch(patch, vol, count, origin):
    """vol[z0:z0+pz, ...] += patch ; count += 1 (reference model.py:919-929)."""
    pz, py, px, K = patch.shape
    D, H, W = vol.shape[:3]
    check(_lib.lib().vnet_accumulate_patch(_ptr(patch.contiguous()), _ptr(vol), _ptr(count), K, pz, py, px,
                                           int(origin[0]), int(origin[1]), int(origin[2]), D, H, W, _stream()),
          "vnet_accumulate_patch")
