"""-m gpu: the 3-D U-Net as a whole at the sizes its layer table times (profiles/unet_layer_table.txt: NumChannel 16, 4 levels, 2 + 2
convolutions): logits, loss, soft-Dice sums, argmax, moving statistics and every parameter gradient of one training step against the
fp64 oracle fixtures tests/golden/unet_128cube.npz, unet_64cube_b2.npz and two more draws of each under tests/golden/spread/
(tests/golden/make_golden_full_unet.py; ORACLE outputs), in both fp32 modes; run-to-run bit-identity and batch duplication at 128^3;
and six 3^3 layers + the level-1 pooling teacher-forced on the operands of the 128^3 oracle run.

Forward-side bounds are the BASELINE ones tests/test_hip_golden_full.py holds the V-Net to, unchanged: logits allclose 1e-3 / 1e-3 and
rel-L2 1e-4, loss 1e-5, Dice sums rtol 1e-5, argmax agreement >= 99.99 % on the strided sample; moving statistics as
tests/test_hip_unet.py::test_unet_fixture_configurations (1e-4, atol 1e-6).

GRADIENTS.  The small-net bounds (rel-L2 1e-3 / 5e-3) do not carry over: fp32 arithmetic through the batch-norms loses more than that
at this size whoever does it (the cancellation tests/test_hip_golden_full.py documents for the V-Net).  The bounds are therefore
MEASURED ON THE REFERENCE ARITHMETIC, never on the HIP path: profiles/unet_golden_full_errors_cpu.py runs the PyTorch-CPU fp32
restatement tests/unet_torch.py on every committed draw and reports the figures below with this file's own code; each bound is 2 x the
maximum over ALL six draws, one set for both sizes as the V-Net test has one set for its configurations (the maxima all come from the
64^3 B = 2 draws, so the 128^3 cases are held to about 4 x their own yardstick figure rather than 2 x; a pooled maximum of a chaotic
quantity over six draws was preferred to two maxima over three) (the factor tests/test_hip_unet.py states for the U-Net: wide enough for another summation order of the same
fp32 arithmetic, tight enough that a wrong layer -- errors of order 1 -- cannot hide).  The figures are recorded in
profiles/unet_golden_full_errors.txt, with the HIP path's own appended for the record.

The only tensors a gradient check skips are the analytically zero ones, by name: the .../biases variables (every U-Net convolution
feeds a batch-norm), 23 of the 100 variables, each still held to max|g| < 1e-4; 77 tensors are compared."""
import os

import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import unet_oracle as U
from tests.golden import make_golden_full_unet as G
from tests.golden.make_golden_full import STRIDE, sample_indices
from tests.util import g, check_close, rel_l2

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FIGURES = ("tensor", "median", "norm", "head", "vector")
# 2 x the maximum over the six committed draws of tests/unet_torch.py in fp32 (profiles/unet_golden_full_errors.txt, section
# "torch-cpu fp32"): per-tensor sampled rel-L2, its median over tensors, norm error, first-8-elements error, whole gradient vector.
# Maxima: tensor 2.437e-2 (draw u64b2s3), median 5.793e-3 (u64b2s2), norm 4.317e-3, head 6.329e-3, vector 5.195e-3 (u64b2s3).
FULL_BOUNDS = {"tensor": 2 * 2.437e-2, "median": 2 * 5.793e-3, "norm": 2 * 4.317e-3, "head": 2 * 6.329e-3, "vector": 2 * 5.195e-3}
N_COMPARED, N_BIASES = 77, 23
# batch duplication, flat gradient B = 2 against B = 1: test_network_c3_full_size_properties holds the V-Net to 1e-3; the U-Net's fp32
# yardstick on the CPU does not meet that itself (1.470e-3: profiles/unet_golden_full_errors.txt, "batch duplication"), so the bound
# is 2 x its figure.  Logits 2e-4 and loss 1e-6 it does meet (1.66e-4, 0.0); they stay.
DUP_GRADIENT_BOUND = 2 * 1.470e-3


def grad_errors(z, grads):
    """(per compared tensor (name, sampled rel-L2, norm error, first-8 error) of `grads` {name: array or None} against fixture z, at
    the fixture's seeded sample positions; {bias name: max|g|}).  Nothing is asserted here, so that a caller can print first.
    A bias whose gradient is None counts as 0.0: inside a network the HIP path takes the closed form of DESIGN.md section 4.1b
    (ops.zero_bias_gradients) and never makes a gradient tensor for a convolution bias in front of a batch-norm."""
    out, biases = [], {}
    for i, n in enumerate(map(str, z["names"])):
        gn = float(z["grad_norm"][i])
        got = grads[n]
        if n.endswith("/biases"):
            biases[n] = 0.0 if got is None else float(np.abs(np.asarray(got)).max())
            continue
        got = np.asarray(got, dtype=np.float64).ravel()
        idx = sample_indices(i, got.size)
        ref = z["grad_sample"][i][:len(idx)].astype(np.float64)
        out.append((n, rel_l2(got[idx], ref), abs(np.linalg.norm(got) - gn) / gn,
                    np.abs(np.resize(got[:8], 8) - z["grad_head"][i]).max() / max(gn, np.abs(z["grad_head"][i]).max())))
    return out, biases


def check_counts(z, errs, biases):
    """Exactly the .../biases variables are left out of the comparison (their oracle gradient is zero), each held to 1e-4."""
    assert (len(errs), len(biases)) == (N_COMPARED, N_BIASES), (len(errs), len(biases))
    for n, gn in zip(map(str, z["names"]), z["grad_norm"]):
        assert (float(gn) < 1e-7) == (n in biases), (n, float(gn))
    for n, m in biases.items():
        assert m < 1e-4, (n, m)


def summarize(z, errs):
    names = list(map(str, z["names"]))
    num = sum((e[1] * float(z["grad_norm"][names.index(e[0])])) ** 2 for e in errs)
    den = sum(float(v) ** 2 for v in z["grad_norm"])
    return {"tensor": max(e[1] for e in errs), "median": float(np.median([e[1] for e in errs])), "norm": max(e[2] for e in errs),
            "head": max(e[3] for e in errs), "vector": (num / den) ** 0.5}


def _net(dev, values, shape):
    from vnet_tensorflow_amd import networks
    K, drop, C, levels, convs, bottom, act = G.CONFIG
    net = networks.UNet(K, drop, C, levels, convs, bottom, True, act, device=dev)
    net.variables.values = values
    return net.build(shape)


def _dice_sums(sm, lab, K):
    oh = torch.nn.functional.one_hot(torch.from_numpy(lab[..., 0]).long().to(sm.device), K).to(torch.float64)
    s = sm.to(torch.float64)
    ax = (1, 2, 3)
    return (s * oh).sum(ax).cpu().numpy(), s.sum(ax).cpu().numpy(), oh.sum(ax).cpu().numpy()


@pytest.mark.parametrize("compute", ["fp32", "fp32_split3"])
@pytest.mark.parametrize("case", list(G.CASES))
def test_full_size_unet(dev, case, compute):
    from vnet_tensorflow_amd import ops
    fname, P, B, seed = G.CASES[case]
    K = G.CONFIG[0]
    z = np.load(os.path.join(GOLD, fname))
    names, values = G.creation_order(G.WEIGHT_SEED[case])
    assert names == [str(n) for n in z["names"]]
    x, lab = O.synthetic_batch(B, P, 1, K, seed=seed)
    ops.set_compute_dtype(compute)
    try:
        net = _net(dev, values, x.shape)
        logits = net.GetNetwork(g(x, dev))
        loss, dice, sm, pred = ops.softmax_loss(logits, g(lab, dev, torch.int32), "sorensen", want_softmax=True, want_pred=True)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype("fp32")
    loss = float(loss.detach())
    s = (slice(None),) + (slice(None, None, STRIDE),) * 3
    got, ref = logits.detach()[s].cpu().numpy(), z["logits_sample"]
    agree = float((pred[s].cpu().numpy() == z["pred_sample"]).mean())
    errs, biases = grad_errors(z, {n: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for n, p in net.named_parameters()})
    fig = summarize(z, errs)
    wn = max(errs, key=lambda e: e[1])
    print("%-8s HIP %-11s: loss err %.2e | logits rel-L2 %.2e max-abs %.2e | argmax agreement %.4f %% | %d tensors, %d biases max|g| %.1e "
          "| %s | worst %s" % (case, compute, abs(loss - float(z["loss"])), rel_l2(got, ref), np.abs(got - ref).max(), 100.0 * agree,
                               len(errs), len(biases), max(biases.values()), "  ".join("%s %.3e" % (k, fig[k]) for k in FIGURES), wn[0]))
    check_counts(z, errs, biases)
    assert got.shape == ref.shape
    assert np.allclose(got, ref, rtol=1e-3, atol=1e-3), np.abs(got - ref).max()
    assert rel_l2(got, ref) < 1e-4, rel_l2(got, ref)
    assert abs(loss - float(z["loss"])) < 1e-5, (loss, float(z["loss"]))
    I, L, R = _dice_sums(sm.detach(), lab, K)
    for a, b, nm in ((I, z["dice_I"], "I"), (L, z["dice_L"], "L"), (R, z["dice_R"], "R")):
        assert np.allclose(a, b, rtol=1e-5, atol=1e-2), (nm, a, b)
    assert abs((1.0 - ((2 * I + 1e-5) / (L + R + 1e-5)).mean()) - float(z["loss"])) < 1e-5
    assert agree >= 0.9999, agree
    for n in z.files:
        if n.startswith("state:"):
            check_close(n, net.variables.buffers[n[len("state:"):]], z[n], 1e-4, atol=1e-6)
    for n, e_sample, e_norm, e_head in errs:
        assert e_sample < FULL_BOUNDS["tensor"] and e_norm < FULL_BOUNDS["norm"] and e_head < FULL_BOUNDS["head"], (n, e_sample, e_norm, e_head)
    assert fig["median"] < FULL_BOUNDS["median"], fig
    assert fig["vector"] < FULL_BOUNDS["vector"], fig


def test_unet_full_size_properties(dev):
    """128^3, one forward + loss + backward: bit-identical run to run (logits, loss, flat gradient: no atomics on the path); the patch
    duplicated in the batch leaves train-mode batch-norm statistics, hence logits and loss, unchanged and (mean over the batch) the
    gradient too: B = 2 equals B = 1 at test_network_c3_full_size_properties's figures."""
    from vnet_tensorflow_amd import ops, optim
    names, values = G.creation_order(42)
    x, lab = O.synthetic_batch(1, 128, 1, G.CONFIG[0], seed=1000)
    tx, tl = g(x, dev), g(lab, dev, torch.int32)

    net = _net(dev, values, x.shape)
    flat = optim.FlatParams(net.named_parameters())

    def run(xb, lb):
        flat.zero_grad()
        logits = net.GetNetwork(xb)
        loss, _, _, _ = ops.softmax_loss(logits, lb, "sorensen")
        loss.backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), float(loss.detach()), flat.grad.clone()

    l1, loss1, g1 = run(tx, tl)
    l1b, loss1b, g1b = run(tx, tl)
    assert torch.equal(l1, l1b) and loss1 == loss1b and torch.equal(g1, g1b)
    assert np.isfinite(loss1) and 0.0 < loss1 < 1.0 and bool(torch.isfinite(g1).all())
    l2, loss2, g2 = run(torch.cat((tx, tx)), torch.cat((tl, tl)))
    e_l = max(float((l2[0:1] - l1).abs().max()), float((l2[1:2] - l1).abs().max()))
    e_g = float((g2 - g1).norm() / g1.norm())
    print("unet 128^3 batch duplication HIP fp32: logits max-abs %.2e | loss %.2e | flat gradient rel %.3e" % (e_l, abs(loss2 - loss1), e_g))
    assert e_l < 2e-4
    assert abs(loss2 - loss1) < 1e-6
    assert e_g < DUP_GRADIENT_BOUND


def test_unet_teacher_forced_layers(dev):
    """Per-layer parity on REAL operands -- post-ReLU (half of them zero), non-zero mean, gradients spanning decades -- without the
    network's chaotic amplification.  The fixture holds, rounded to float32, a crop of the tensor each layer read in the 128^3 oracle
    run and of the gradient that arrived at its output.  Each layer is run alone on that data and compared with the oracle's fp64
    convolution of the same float32 operands: forward, dx, dw at the kernel bound 2e-6 (dw with atol 2e-6 max|dw|, as the bf16
    teacher-forced test); the level-1 pooling bit for bit."""
    from vnet_tensorflow_amd import ops
    names, values = G.creation_order(G.WEIGHT_SEED[G.TF_CASE])
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    for name, (tag, origin) in G.TF_LAYERS.items():
        x, dy, lo = G.load_tf(tag)
        w, b = f32(values[name]), f32(values[name[:-len("weights")] + "biases"])
        assert x.shape[:4] == dy.shape[:4] and x.shape[-1] == w.shape[-2] and dy.shape[-1] == w.shape[-1], (name, x.shape, dy.shape)
        assert float(np.abs(x).max()) > 0 and float(np.abs(dy).max()) > 0
        y_ex = O.conv_nd_fwd(x, w, 1) + b
        dx_ex, dw_ex = O.conv_nd_bwd(x, w, dy, 1)
        two = name.startswith("unet/decoder") and name.endswith("conv_1/weights")       # concat(up-convolved, skip): two sources
        C0 = x.shape[-1] // 2 if two else x.shape[-1]
        tx = g(x[..., :C0], dev).requires_grad_(True)
        tx1 = g(x[..., C0:], dev).requires_grad_(True) if two else None
        tw, tb = g(w, dev).requires_grad_(True), g(b, dev).requires_grad_(True)
        y = ops.conv(tx, tw, tb, 3, 1, x1=tx1)
        y.backward(g(dy, dev))
        dxg = torch.cat((tx.grad, tx1.grad), -1) if two else tx.grad
        fig = [rel_l2(a.detach().cpu().numpy(), r) for a, r in ((y, y_ex), (dxg, dx_ex), (tw.grad, dw_ex))]
        print("teacher-forced %-40s x %s zero fraction %.2f: fwd %.2e dx %.2e dw %.2e" % (name, x.shape, float((x == 0).mean()), *fig))
        check_close("teacher-forced %s fwd" % name, y, y_ex, 2e-6)
        check_close("teacher-forced %s dx" % name, dxg, dx_ex, 2e-6)
        check_close("teacher-forced %s dw" % name, tw.grad, dw_ex, 2e-6, atol=2e-6 * float(np.abs(dw_ex).max()))
    tag, _, origin = G.TF_POOL
    x, dy, _ = G.load_tf(tag)
    v = O.Var(x)
    yo = U.max_pool2(v)
    O.backward(yo, seed=dy)
    assert float((yo.v == 0).mean()) > 0                           # all-zero windows: the tie case is in the data
    xg = g(x, dev).requires_grad_(True)
    y = ops.max_pool2(xg)
    y.backward(g(dy, dev))
    assert np.array_equal(y.detach().cpu().numpy(), yo.v) and np.array_equal(xg.grad.cpu().numpy(), v.g)
