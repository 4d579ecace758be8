"""No-GPU checks of the third public header, include/vnet_hip_head.h (the decoder's last batch-norm with the 1x1x1 head folded in):
its ledger, and the variable names and order of a network built with the fused head."""
import os

import numpy as np
import torch

from tests import guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_HEADER = os.path.join(ROOT, "include", "vnet_hip_head.h")


def test_head_header_ledger():
    """include/vnet_hip_head.h beyond tests/test_abi_ledger.py: the entry points that take buffers are the three every guarded case
    of tests/test_hip_head_guard.py must reach."""
    from tests import test_hip_head_guard as TG
    assert set(guard.pointer_entry_points(HEAD_HEADER)) == set(TG.FUSED)


def test_fused_head_creates_the_same_variables():
    """A deferred batch-norm (chain) creates its variables where the reference does: names and order do not depend on fuse_head."""
    from vnet_tensorflow_amd import networks
    names = {}
    for fuse in (True, False):
        for nconv, chains in (((1, 2), True), ((2, 2), True), ((1, 2), False), ((2, 3), False)):
            np.random.seed(1)
            net = networks.VNet(3, 0.0, 8, 2, nconv, 2, True, "prelu", device=torch.device("cpu"))
            net.fuse_head, net.fuse_bn_chains = fuse, chains
            net.build((1, 16, 16, 16, 1))
            names[(fuse, nconv, chains)] = [(n, tuple(p.shape)) for n, p in net.named_parameters()] + sorted(net.state_dict())
    for (fuse, nconv, chains), v in names.items():
        assert v == names[(False, nconv, chains)], (nconv, chains)
        assert any(n == "vnet/output_layer/weights" for n, _ in v[:len(v) // 2])
