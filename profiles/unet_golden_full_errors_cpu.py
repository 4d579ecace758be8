"""What does the reference arithmetic -- fp32 through PyTorch-CPU autograd, tests/unet_torch.py -- measure against the fp64 U-Net
fixtures of tests/golden/make_golden_full_unet.py?  Same recipe weights / inputs and the same figures, with the fixture's own sampling,
as tests/test_hip_golden_full_unet.py (its grad_errors / summarize are used here).  The gradient bounds of that test are 2 x the
maximum over the committed draws of each figure this prints; the HIP path's own figures never feed back into them.  CPU only.

    python profiles/unet_golden_full_errors_cpu.py [case ...] [dup]  >  profiles/unet_golden_full_errors.txt

dup: the batch-duplication yardstick (B = 2 of the same 128^3 patch against B = 1) in the same fp32 arithmetic."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vnet_oracle as O  # noqa: E402
from tests import unet_torch as UT  # noqa: E402
from tests.golden import make_golden_full_unet as G  # noqa: E402
from tests.golden.make_golden_full import STRIDE  # noqa: E402
from tests.test_hip_golden_full_unet import FIGURES, GOLD, check_counts, grad_errors, summarize  # noqa: E402
from tests.util import rel_l2  # noqa: E402

K, _, C, LEVELS, CONVS, BOTTOM, _ = G.CONFIG


def run_case(case, dtype=torch.float32):
    fname, P, B, seed = G.CASES[case]
    z = np.load(os.path.join(GOLD, fname))
    names, values = G.creation_order(G.WEIGHT_SEED[case])
    assert names == [str(n) for n in z["names"]]
    x, lab = O.synthetic_batch(B, P, 1, K, seed=seed)
    loss, logits, grads = UT.run(values, x.astype(np.float64), lab[..., 0], K, C, LEVELS, CONVS, BOTTOM, dtype)
    return z, loss, logits, grads


def main(argv):
    cases = [a for a in argv if a != "dup"] or list(G.CASES)
    worst = dict((k, 0.0) for k in FIGURES)
    for case in cases:
        z, loss, logits, grads = run_case(case)
        s = (slice(None),) + (slice(None, None, STRIDE),) * 3
        got, ref = logits[s], z["logits_sample"]
        agree = float((got.argmax(-1) == z["pred_sample"]).mean())
        errs, biases = grad_errors(z, grads)
        check_counts(z, errs, biases)
        fig = summarize(z, errs)
        wn = max(errs, key=lambda e: e[1])
        print("%-8s torch-cpu fp32: loss err %.2e | logits rel-L2 %.2e max-abs %.2e | argmax agreement %.4f %% (>= 99.99 required: %s) | "
              "%d tensors | %s | worst %s" % (case, abs(loss - float(z["loss"])), rel_l2(got, ref), np.abs(got - ref).max(), 100.0 * agree,
                                              "met" if agree >= 0.9999 else "NOT MET -- replace this draw", len(errs),
                                              "  ".join("%s %.3e" % (k, fig[k]) for k in FIGURES), wn[0]), flush=True)
        for k in FIGURES:
            worst[k] = max(worst[k], fig[k])
    print("maximum over %d draws:  %s" % (len(cases), "  ".join("%s %.3e" % (k, worst[k]) for k in FIGURES)))
    print("bounds = 2 x maximum:   %s" % "  ".join("%s %.2e" % (k, 2.0 * worst[k]) for k in FIGURES))
    if "dup" in argv:
        names, values = G.creation_order(42)
        x, lab = O.synthetic_batch(1, 128, 1, K, seed=1000)
        l1, z1, g1 = UT.run(values, x, lab[..., 0], K, C, LEVELS, CONVS, BOTTOM, torch.float32)
        l2, z2, g2 = UT.run(values, np.concatenate((x, x)), np.concatenate((lab, lab))[..., 0], K, C, LEVELS, CONVS, BOTTOM, torch.float32)
        f1, f2 = (np.concatenate([g[n].ravel() for n in names]) for g in (g1, g2))
        print("batch duplication 128^3, torch-cpu fp32: logits max-abs %.2e | loss %.2e | flat gradient rel %.3e (bound of "
              "test_network_c3_full_size_properties: 2e-4 / 1e-6 / 1e-3)" % (max(np.abs(z2[0] - z1[0]).max(), np.abs(z2[1] - z1[0]).max()),
                                                                              abs(l2 - l1), np.linalg.norm(f2 - f1) / np.linalg.norm(f1)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
