"""Run once on an MI355X: profiles/window_bench.txt (one run; kernels: medians of 9 timings of 20 back-to-back launches each after 3
warm-up rounds, HIP events; the spread is read off two timings of the parent's kernel in the same run, taken before and after the new
kernel's).

The glue of a mirrored or weighted sliding-window evaluation (csrc/vnet_window.h):
    accumulate : vnet_window_accumulate at 128^3 x K = 2 and K = 5 into a 256^3 volume at (64, 64, 64) -- null weights, Gaussian
                 weights, Gaussian weights with mask 7 -- and vnet_accumulate_patch (the parent's kernel) on the same tensors.
    crop       : vnet_window_crop_flip (mask 0 and mask 7) against vnet_crop_words, 128^3 x 1 from a 256^3 case.
    end to end : evaluate_single_3D on a synthetic 256^3 x 1 case that lives on the device (full-width V-Net, PatchShape 128, stride
                 64, batch 2, fp32_split3: 27 windows plus the duplicated last batch) -- plain, Gaussian weights, and Mirror [0, 1, 2]
                 (8 passes) -- wall clock with a synchronize, after a warm-up on a 192^3 corner; and the share of the glue in a pass:
                 (crop + accumulate of one window) / (seconds per window and pass).
The kernel timings launch on the same tensors again and again: 67 MB (K = 2) and 143 MB (K = 5) per window stay in the 256 MB last-level
cache, for the parent's kernel and the new one alike.  No target is fixed for any of these figures.
Usage: python profiles/bench_window.py [outfile [kernels]]   (default profiles/window_bench.txt; `kernels`: skip the end-to-end part)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, D, AT, INNER = (128, 128, 128), (256, 256, 256), (64, 64, 64), 20


def main(out_path, end_to_end=True):
    import torch
    from vnet_tensorflow_amd import ops, window as W
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    def events(fn, warm=3, reps=9):
        """Median and extremes of `reps` timings of INNER back-to-back launches, in ms per launch."""
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / INNER)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    say("window glue, window %dx%dx%d in a volume %dx%dx%d at %s; device %s" % (P + D + (AT, torch.cuda.get_device_name(0))))
    say("ms per launch: median (min .. max) of 9 timings of %d launches" % INNER)
    rng = np.random.default_rng(0)
    wg = W.device_weights(W.weight_vectors("gaussian", P), dev)
    glue = {}
    for K in (2, 5):
        patch = torch.from_numpy(rng.random(P + (K,), dtype=np.float32)).to(dev)
        vol, cnt = torch.zeros(D + (K,), device=dev), torch.zeros(D, device=dev)
        nbytes = 4.0 * P[0] * P[1] * P[2] * (3 * K + 2)                  # patch read, vol and cnt read and written
        fmt = lambda t: "%8.4f (%.4f .. %.4f) ms  %6.0f GB/s" % (t + (nbytes / t[0] / 1e6,))      # noqa: E731
        parent_a = events(lambda: ops.accumulate_patch(patch, vol, cnt, AT))
        new = events(lambda: W.accumulate(patch, vol, cnt, AT, 0, None))
        parent_b = events(lambda: ops.accumulate_patch(patch, vol, cnt, AT))
        gauss = events(lambda: W.accumulate(patch, vol, cnt, AT, 0, wg))
        gauss7 = events(lambda: W.accumulate(patch, vol, cnt, AT, 7, wg))
        say("K = %d (%.0f MB per window)" % (K, nbytes / 1e6))
        say("  vnet_accumulate_patch, first timing          %s" % fmt(parent_a))
        say("  vnet_window_accumulate, null weights, mask 0 %s" % fmt(new))
        say("  vnet_accumulate_patch, second timing         %s" % fmt(parent_b))
        say("  vnet_window_accumulate, gaussian, mask 0     %s" % fmt(gauss))
        say("  vnet_window_accumulate, gaussian, mask 7     %s" % fmt(gauss7))
        spread = abs(parent_a[0] - parent_b[0])
        worse = new[0] - max(parent_a[0], parent_b[0])
        say("  the parent's two medians differ by %.4f ms; the new kernel with null weights and mask 0 is %s" % (
            spread, "SLOWER than both by %.4f ms (more than that spread: %s)" % (worse, worse > spread) if worse > 0 else
            "not slower than the parent's slower timing (%.2f x its faster one)" % (new[0] / min(parent_a[0], parent_b[0]))))
        glue[K] = gauss7[0]
    case = torch.from_numpy(rng.random(D + (1,), dtype=np.float32)).to(dev)
    slot = torch.empty(P + (1,), device=dev)
    cbytes = 8.0 * P[0] * P[1] * P[2]
    cfmt = lambda t: "%8.4f (%.4f .. %.4f) ms  %6.0f GB/s" % (t + (cbytes / t[0] / 1e6,))      # noqa: E731
    crop_a = events(lambda: ops.crop_window(case, AT, P, out=slot))
    flip0 = events(lambda: W.crop_flip(case, AT, P, 0, out=slot))
    crop_b = events(lambda: ops.crop_window(case, AT, P, out=slot))
    flip7 = events(lambda: W.crop_flip(case, AT, P, 7, out=slot))
    say("crop 128^3 x 1")
    say("  vnet_crop_words, first timing                %s" % cfmt(crop_a))
    say("  vnet_window_crop_flip, mask 0                %s" % cfmt(flip0))
    say("  vnet_crop_words, second timing               %s" % cfmt(crop_b))
    say("  vnet_window_crop_flip, mask 7                %s" % cfmt(flip7))
    if not end_to_end:
        return

    import bench
    from vnet_tensorflow_amd import model as M
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = bench.config(128, 2, 1, 2, "fp32_split3")
    cfg["EvaluationSetting"] = {"Stride": [64, 64, 64], "BatchSize": 2, "ProbabilityOutput": False}
    m = M.image2label(None, cfg, device=dev, verbose=False)
    m.read_config()
    m.build_model_graph()
    vol = torch.from_numpy(np.clip(127.5 + 40 * np.random.default_rng(0).standard_normal(D + (1,)), 0, 255).astype(np.float32)).to(dev)
    K = m.output_channel_num
    say("evaluate_single_3D, 256^3 x 1 on the device, V-Net 128^3 patches, stride 64, batch 2, fp32_split3, K = %d (28 windows a pass)" % K)
    base = None
    for name, mirror, kind in (("plain", [], "uniform"), ("gaussian", [], "gaussian"), ("Mirror [0, 1, 2]", [0, 1, 2], "uniform"),
                               ("Mirror [0, 1, 2], gaussian", [0, 1, 2], "gaussian")):
        m.evaluate_mirror, m.evaluate_window_weights = mirror, kind
        m.evaluate_single_3D(vol[:192, :192, :192].contiguous())                 # warm-up: 8 windows, every kernel of the pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        label, _ = m.evaluate_single_3D(vol)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        passes = len(W.flip_sets(mirror))
        base = base if base is not None else (dt, label)
        say("  %-28s %7.3f s  %d pass%s, %.2f ms per window and pass, %.2f x plain; %d voxels differ from the plain label" % (
            name, dt, passes, "es" if passes > 1 else "", dt * 1e3 / (28 * passes), dt / base[0], int((label != base[1]).sum())))
        if name.startswith("Mirror") and K in glue:
            share = (glue[K] + flip7[0]) / (dt * 1e3 / (28 * passes))
            say("    the glue of one window (crop_flip mask 7 %.4f ms + accumulate gaussian mask 7, K = %d, %.4f ms): %.1f %% of a pass" % (
                flip7[0], K, glue[K], 100 * share))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "window_bench.txt"),
         end_to_end=not (len(sys.argv) > 2 and sys.argv[2] == "kernels"))
