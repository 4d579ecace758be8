"""The three fallback reductions of csrc/elementwise.hip for channel counts off the vector paths, one launch sequence at a time, at
64^3 rows, C = 12, K = 2:   [VNET_HIP_LIB=.../libvnet_hip_<tag>.so] python profiles/bench_generic_reduce.py [iters]
    bn reduce   vnet_bn_act_bwd_reduce  (bn_act_bwd_reduce_kernel<2> + sum_finalize_kernel), PReLU, no residual
    colsum      vnet_colsum             (colsum_generic_kernel + sum_finalize_kernel)
    head bwd    vnet_head_bwd           (head_bwd_generic_kernel<2> + head_finalize_kernel), dx written
Each figure = `iters` back-to-back calls between two HIP events on the launch stream, us per call.  For an A/B against another
revision build its library with profiles/build_rev_lib.sh and alternate the two processes (profiles/determinism.txt)."""
import os
import sys

import torch

sys.path.insert(0, '.')
from vnet_tensorflow_amd import _lib, ops  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device('cuda', 0)
L = _lib.lib()
st = ops._stream()
P = ops._ptr
M, C, K = 64 ** 3, 12, 2


def timed(fn):
    for _ in range(5):
        assert fn() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


x, dy = torch.randn(M, C, device=dev), torch.randn(M, C, device=dev)
dl, w = torch.randn(M, K, device=dev), torch.randn(C, K, device=dev)
dx = torch.empty_like(x)
mean, invstd, gamma, beta = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
alpha = torch.full((C,), 0.25, device=dev)
dg, db, da, out = (torch.zeros(C, device=dev) for _ in range(4))
dw, dbias = torch.zeros(C, K, device=dev), torch.zeros(K, device=dev)
nb, nc, nh = L.vnet_bn_ws_bytes(C), L.vnet_colsum_ws_bytes(C), L.vnet_head_ws_bytes(C, K)
ws = torch.empty(max(nb, nc, nh), dtype=torch.uint8, device=dev)
runs = (("bn reduce", lambda: L.vnet_bn_act_bwd_reduce(P(dy), P(x), None, 0, M, C, P(mean), P(invstd), P(gamma), P(beta), 2, P(alpha),
                                                       P(dg), P(db), P(da), P(ws), nb, st)),
        ("colsum", lambda: L.vnet_colsum(P(dy), P(out), M, C, P(ws), nc, st)),
        ("head bwd", lambda: L.vnet_head_bwd(P(x), P(w), P(dl), P(dx), P(dw), P(dbias), M, C, K, P(ws), nh, st)))
print("%-28s %s" % (os.path.basename(_lib.LIB_PATH), "  ".join("%s %7.1f us" % (tag, timed(fn)) for tag, fn in runs)))
