"""Pins the WIRING and the VARIABLE NAMES of the U-Net restatement against the reference's own graph-building code.

    python tests/golden/make_ref_wiring_unet.py     (build container only: needs /root/reference, which is read here and NEVER copied)

Runs the reference's `networks.UNet(...).GetNetwork` (networks.py:4-150) -- its real source, imported from /root/reference at
generation time -- against the NumPy-eager `tf` stand-in of make_ref_wiring.py (imported, unchanged), to which this file adds the one
symbol the U-Net needs on top: tf.nn.max_pool3d.  As there, the stand-in's arithmetic and TF naming rules are this repo's: the
fixtures pin which layers exist, their creation order and names (mind the decoder block's batch-norms OUTSIDE the conv_i scopes,
networks.py:65,84), how they are wired, and the logits / moving statistics of that wiring with injected weights -- NOT TensorFlow's
numerics: parity stays "partial -- unpinned by the reference" (DESIGN.md section 2).
(The files are NOT named ref_wiring_*.npz: tests/test_oracle.py runs every file of that pattern through the V-Net oracle.)
Output: tests/golden/unet_ref_wiring_<case>.npz (names, shapes, trainable flags in creation order, input, injected values, logits,
moving statistics after one step's update ops).  tests/test_unet_host.py compares."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_wiring as W  # noqa: E402


def nn_max_pool3d(x, ksize, strides, padding, **k):
    assert list(ksize) == [1, 2, 2, 2, 1] and list(strides) == [1, 2, 2, 2, 1] and padding == 'VALID'
    x = np.asarray(x)
    d, h, w = x.shape[1] // 2, x.shape[2] // 2, x.shape[3] // 2
    y = x[:, :2 * d, :2 * h, :2 * w, :].reshape(x.shape[0], d, 2, h, 2, w, 2, x.shape[-1]).max(axis=(2, 4, 6))
    return W._t(y)


def load_reference():
    tf = W.make_tf()
    tf.nn.max_pool3d = nn_max_pool3d
    sys.modules["tensorflow"] = tf
    sys.path.insert(0, W.REF)
    try:
        for name in ("layers2", "networks"):
            sys.modules.pop(name, None)
        return importlib.import_module("networks")
    finally:
        sys.path.remove(W.REF)
        for name in ("layers2", "networks", "tensorflow"):
            sys.modules.pop(name, None)


#        name      cin K  C  levels convs bottom patch
CASES = {
    "c1k2": (1, 2, 4, 2, 2, 2, (8, 8, 8)),
    "c3k3": (3, 3, 4, 2, 1, 2, (8, 8, 8)),
    # non-cubic, C = 8, a one-conv bottom at 1 x 2 x 3.  (A patch with an ODD level size, e.g. (6, 10, 12), does not build: the VALID
    # pooling floors 3 -> 1 and the SAME conv3d_transpose back to 3 needs 2 coarse voxels -- TF 1.15 rejects that graph, and so does
    # this stand-in's conv3d_transpose.  The pooling kernels' odd sizes are covered by their own tests.)
    "odd":  (1, 2, 8, 2, 2, 1, (4, 8, 12)),
}


def build(networks, K, C, levels, convs, bottom, x, values=None):
    W.G[0] = W.Graph(values)
    net = networks.UNet(K, 0.0, C, levels, convs, bottom, True, "relu")       # model.py:417-427
    logits = net.GetNetwork(W._t(x))
    return W.G[0], np.asarray(logits)


def main():
    networks = load_reference()
    for cname, (cin, K, C, levels, convs, bottom, patch) in CASES.items():
        rng = np.random.default_rng(1000 + sum(map(ord, cname)))
        x = rng.standard_normal((2,) + patch + (cin,))
        np.random.seed(0)
        g0, _ = build(networks, K, C, levels, convs, bottom, x)
        values = {}
        for name, v, tr in g0.vars:
            if name.endswith(("moving_variance", "gamma")):
                values[name] = 0.5 + rng.random(v.shape)
            elif name.endswith("weights"):
                values[name] = rng.standard_normal(v.shape) * (2.0 / np.prod(v.shape[:-1])) ** 0.5
            else:
                values[name] = 0.1 * rng.standard_normal(v.shape)
        values = {k: v.astype(np.float32).astype(np.float64) for k, v in values.items()}
        x = x.astype(np.float32).astype(np.float64)
        g, logits = build(networks, K, C, levels, convs, bottom, x, values)
        assert [n for n, _, _ in g.vars] == [n for n, _, _ in g0.vars]
        lab = rng.integers(0, K, logits.shape[:-1])
        out = {"names": np.array([n for n, _, _ in g.vars]), "trainable": np.array([t for _, _, t in g.vars]),
               "shapes": np.array([",".join(map(str, v.shape)) for _, v, _ in g.vars]),
               "x": x.astype(np.float32), "labels": lab.astype(np.int8), "logits": logits,
               "config": np.array([str(cin), str(K), str(C), str(levels), str(convs), str(bottom)])}
        for n, v, _ in g.vars:
            out["v:" + n] = np.asarray(v).astype(np.float32)
        for n, v in g.updates.items():
            out["u:" + n] = np.asarray(v)
        path = os.path.join(HERE, "unet_ref_wiring_%s.npz" % cname)
        np.savez_compressed(path, **out)
        print("%-6s %3d variables (%d trainable)  logits %s  ->  %s (%.0f KB)" % (
            cname, len(g.vars), sum(t for _, _, t in g.vars), logits.shape, os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
