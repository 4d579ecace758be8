"""The label filters of evaluate on the device against the host functions, at the sizes of the input file's grid (256^3, 512^3):
    device path: ops.largest_component(label, min_volume=...) on the device label, then the download of the uint8 0/1 map
    host path  : what evaluate() did before: download of the unfiltered label (int16), model.ExtractLargestConnectedComponents, then
                 model.volume_threshold on its result (scipy.ndimage.label + np.bincount, one thread)
on two label maps built from a seed: a compact blob plus a few hundred small islands (the realistic case) and Bernoulli noise at
p = 0.35 (the adversarial case: just above the cubic lattice's site-percolation threshold).  The two results must be equal.
For the kernels alone (HIP events after warm-up; label resident): the time and the algorithmic bytes -- the int32 label read once, the
uint8 map written once -- over 8 TB/s; the link pass is latency- and atomic-bound and far from that roof.
Every (size, map) step is a child process under its own time limit; the first failure ends the run.
Usage: python profiles/bench_components.py [outfile]   (default profiles/components_bench.txt)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
SPACING = (0.25, 0.25, 0.25)
STEPS = [(256, "blob", 180), (256, "noise", 240), (512, "blob", 420), (512, "noise", 600)]


def label_map(n, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (rng.random((n, n, n), dtype=np.float32) < 0.35).astype(np.int32)
    ax = np.arange(n, dtype=np.float32) - 0.5 * n
    lab = ((ax[:, None, None] / (0.30 * n)) ** 2 + (ax[None, :, None] / (0.22 * n)) ** 2 + (ax[None, None, :] / (0.26 * n)) ** 2 < 1.0)
    lab = lab.astype(np.int32)
    for _ in range(300):                                        # islands of 1..4 voxels a side, class 2, anywhere
        s = int(rng.integers(1, 5))
        x, y, z = (int(v) for v in rng.integers(0, n - s, size=3))
        lab[x:x + s, y:y + s, z:z + s] = 2
    return lab


def step(n, kind):
    import torch
    from vnet_tensorflow_amd import model, ops
    dev = torch.device("cuda", 0)
    lab = label_map(n, kind)
    t = torch.from_numpy(lab).to(dev)
    vt = 100.0 * float(np.prod(SPACING))                        # a threshold of 100 voxels

    def events(fn, warm=2, reps=5):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), r

    k_roots = events(lambda: ops.component_roots(t, sizes=True))
    k_big = events(lambda: ops.largest_component(t, classes=3, min_volume=vt, spacing=SPACING))
    k_thr = events(lambda: ops.volume_threshold(t, vt, SPACING))
    d_ms, got = wall(lambda: ops.largest_component(t, classes=3, min_volume=vt, spacing=SPACING).cpu().numpy(), 3)

    def host():
        lab_np = t.to(torch.int16).cpu().numpy().astype(np.int64)
        return model.volume_threshold(model.ExtractLargestConnectedComponents(lab_np, SPACING), vt, SPACING)
    h_ms, ref = wall(host, 1)
    same = bool(np.array_equal(got, ref)) and bool(np.array_equal(ops.volume_threshold(t, vt, SPACING).cpu().numpy(),
                                                                  model.volume_threshold(lab, vt, SPACING)))
    nbytes = 5.0 * lab.size
    fg = float((lab != 0).mean())
    print("RESULT %d^3 %-5s foreground %4.1f %%   kernels: roots+sizes %8.3f ms, largest+threshold %8.3f ms (%5.1f MB algorithmic, %4.1f %% of "
          "8 TB/s), threshold %8.3f ms   device path with the download %9.1f ms   host path (download + scipy) %9.1f ms   host / device "
          "%6.1fx   results equal: %s" % (n, kind, 100.0 * fg, k_roots, k_big, nbytes / 1e6, 100.0 * nbytes / (k_big * 1e-3) / PEAK, k_thr,
                                        d_ms, h_ms, h_ms / d_ms, same), flush=True)
    return 0 if same else 1


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), sys.argv[3])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "components_bench.txt")
    out = ["label filters of evaluate: device (csrc/components.hip) against the host functions (scipy.ndimage.label, one thread); "
           "spacing %s, threshold 100 voxels" % (SPACING,)]
    rc = 0
    for n, kind, limit in STEPS:
        # one child per step, each under its own time limit; a step that fails or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(n), kind]
        res = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l[7:] for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        out += lines
        print("\n".join(lines), flush=True)
        if res.returncode != 0:
            out.append("%d^3 %s: step ended with status %d; the run stops here\n%s" % (n, kind, res.returncode, res.stderr[-2000:]))
            print(out[-1], flush=True)
            rc = res.returncode
            break
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
