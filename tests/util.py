import contextlib

import numpy as np
import torch


def g(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def max_abs(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def check_close(name, got, ref, rtol_l2=2e-5, atol=None):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == tuple(np.asarray(ref).shape), "%s: shape %s vs %s" % (name, got.shape, np.asarray(ref).shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % name
    r, m = rel_l2(got, ref), max_abs(got, ref)
    ok = r <= rtol_l2 or (atol is not None and m <= atol)
    assert ok, "%s: rel-L2 %.3e (tol %.1e), max-abs %.3e (atol %s), ref-norm %.3e" % (name, r, rtol_l2, m, atol, np.linalg.norm(ref))
    return r, m


# ---- fp32_split3 (the f32x3 convolution kernels, csrc/conv_x3.h) in the system tests -------------------------------------------
# The 5^3 fp32 kernels the f32x3 family replaces: a forced fp32_split3 run must launch none of them.
NATIVE_K5_TAGS = ("conv k5 s1 ", "wgrad k5 s1 ")


@contextlib.contextmanager
def split3(force=True):
    """ComputeDtype "fp32_split3" on the current ops context, and (force) the f32x3 kernels for every 5^3 stride-1 layer whose channels
    are whole 16-blocks, not only where they pay (ops._X3["force"]).  _X3 is a module global that ops.OpsContext does not scope, so
    both are restored on the way out: a leak would silently reroute every later test."""
    from vnet_tensorflow_amd import ops
    prev_force = ops._X3["force"]
    ops.set_compute_dtype("fp32_split3")
    ops._X3["force"] = bool(force)
    try:
        yield ops
    finally:
        ops._X3["force"] = prev_force
        ops.set_compute_dtype("fp32")


def _whole_blocks(tag):
    """'... Cin->Cout' of a launch tag: both sides whole 16-channel blocks (what the f32x3 kernels take)."""
    cin, cout = tag.rsplit(" ", 1)[1].split("->")
    return int(cin) % 16 == 0 and int(cout) % 16 == 0


def x3_profile_check(recs, forced):
    """The dispatch check on ops.profile_start() / profile_stop() records of one EAGER step (launches inside a captured graph carry no
    records).  forced: at least one conv-x3 and one wgrad-x3 launch and no native 5^3 fp32 launch of a layer whose channels are whole
    16-blocks; unforced: at least one conv-x3 launch.  The input block (1 channel: input-direct*; or a few image channels -> 16), the
    2^3 kernels and the 1^3 head stay native by design.  Returns the counts."""
    tags = [r[0] for r in recs]
    n_conv = sum(1 for t in tags if t.startswith("conv-x3 "))
    n_wgrad = sum(1 for t in tags if t.startswith("wgrad-x3 "))
    native = sorted(set(t for t in tags if t.startswith(NATIVE_K5_TAGS) and _whole_blocks(t)))
    assert n_conv >= 1, ("no conv-x3 launch", sorted(set(tags)))
    if forced:
        assert n_wgrad >= 1, ("no wgrad-x3 launch", sorted(set(tags)))
        assert not native, ("native 5^3 fp32 launches in a forced fp32_split3 step", native)
    return n_conv, n_wgrad
