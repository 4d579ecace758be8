"""Run once on an MI355X: profiles/score_bench.txt (one run, median of 5 repetitions after 2 warm-up calls; no spread was measured).

The two kernels of include/vnet_hip_score.h and one score.Accuracy call at 256^3, against the host path:
    kernels     : vnet_label_overlap (L = 3) and vnet_cc_shape on resident int32 maps and buffers made once, HIP events after warm-up, with the
                  algorithmic bytes over the time -- overlap: both maps read once (8 bytes per voxel); shapes: the label read once, the
                  representative map written and read, the counts written (the passes of vnet_cc_roots are latency- and atomic-bound
                  and far from the roof; the figure says how far)
    device path : score.Accuracy(mode DICE + ITEM) on the two device tensors, wall clock with its read-backs
    host path   : what a file-based scorer does: both maps downloaded as int16, then score.Accuracy on the arrays (np.bincount,
                  scipy.ndimage.label, one thread)
on two pairs built from a seed: a compact blob with a few hundred islands against itself shifted by two voxels (the realistic case),
and Bernoulli noise at p = 0.35 against another draw (the adversarial case for the component pass).  The two results must be equal.
Every step is a child process under its own time limit; the first failure ends the run.
Usage: python profiles/bench_score.py [outfile]   (default profiles/score_bench.txt)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
SPACING = (0.25, 0.25, 0.25)
STEPS = [(256, "blob", 300), (256, "noise", 420)]


def pair(n, kind, seed=0):
    from profiles.bench_components import label_map
    gt = label_map(n, kind, seed)
    out = np.roll(gt, 2, axis=0) if kind == "blob" else label_map(n, kind, seed + 1)
    return gt, np.ascontiguousarray(out)


def step(n, kind):
    import torch
    from vnet_tensorflow_amd import ops, score
    dev = torch.device("cuda", 0)
    gt, out = pair(n, kind)
    tg, to = torch.from_numpy(gt).to(dev), torch.from_numpy(out).to(dev)
    mode = ("DICE", "ITEM")

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

    # the kernels alone: the entry points on buffers made once, nothing read back inside the timed window
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    cap = max(4096, score.shapes_of(to)[0])
    counts = torch.empty((4, 3), dtype=torch.int64, device=dev)
    need = L.vnet_cc_shape_ws_bytes(n, n, n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    table = torch.empty(cap * 8 + 1, dtype=torch.int32, device=dev)
    sums = torch.empty((cap, 3), dtype=torch.int64, device=dev)
    k_over = events(lambda: _lib.check(L.vnet_label_overlap(tg.data_ptr(), to.data_ptr(), counts.data_ptr(), gt.size, 3, None),
                                       "vnet_label_overlap"))
    k_shape = events(lambda: _lib.check(L.vnet_cc_shape(to.data_ptr(), table.data_ptr() + 32 * cap, table.data_ptr(), sums.data_ptr(), cap,
                                                        n, n, n, ws.data_ptr(), need, None), "vnet_cc_shape"))
    assert np.array_equal(counts.cpu().numpy(), ops.label_overlap(tg, to, 3)) and int(table[-1]) == score.shapes_of(to)[0]
    d_ms, got = wall(lambda: score.Accuracy(tg, to, spacing=SPACING, tolerence=3, mode=mode), 3)

    def host():
        a, b = tg.to(torch.int16).cpu().numpy().astype(np.int32), to.to(torch.int16).cpu().numpy().astype(np.int32)
        return score.Accuracy(a, b, spacing=SPACING, tolerence=3, mode=mode)
    h_ms, ref = wall(host, 1)
    same = got == ref
    b_over, b_shape = 8.0 * gt.size, 16.0 * gt.size
    print("RESULT %d^3 %-5s kernels: label_overlap %8.3f ms (%5.1f MB algorithmic, %4.1f %% of 8 TB/s), component_shapes %8.3f ms "
          "(%5.1f MB, %4.1f %%)   Accuracy DICE+ITEM on the device %9.1f ms   host path (download + NumPy / scipy) %9.1f ms   host / device "
          "%6.1fx   results equal: %s   %s" % (n, kind, k_over, b_over / 1e6, 100.0 * b_over / (k_over * 1e-3) / PEAK, k_shape, b_shape / 1e6,
                                             100.0 * b_shape / (k_shape * 1e-3) / PEAK, d_ms, h_ms, h_ms / d_ms, same, got), flush=True)
    return 0 if same else 1


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), sys.argv[3])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "score_bench.txt")
    out = ["scoring a label against its ground truth: device (csrc/score.hip) against the host path (NumPy, scipy.ndimage.label, one "
           "thread); spacing %s, tolerance 3" % (SPACING,)]
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
