"""evaluate_single_3D on a 256^3 x 1 volume (full-width V-Net, PatchShape 128, stride 64, batch 2, fp32_split3: 27 windows plus the
duplicated last batch), the case as an array (windows cut on worker threads into pinned memory and uploaded, torch.argmax as int64 --
the code of the parent commit, which this commit leaves as it was) against the case as a device tensor (ops.crop_window into the batch,
ops.argmax_label), and the four kernels of include/vnet_hip_prepare.h alone at 256^3 x 4 channels.
    evaluate : wall clock of one call after a warm-up call, each measurement a child process of its own, the two paths interleaved
               (array, device, array, device, ...) on one box as profiles/ab.sh does; the device path's time includes the one upload of
               the volume, the array path's the crop and the upload of every window.
    kernels  : HIP events after warm-up, median of 7, as GB/s over the algorithmic bytes (stats: the volume read twice; window: read
               once and written once; crop: a 128^3 x 4 window read and written; argmax: 256^3 x 4 logits read, int32 labels written).
    pipeline : the reference's evaluate pipeline on a 128^3 file resampled to 256^3, evaluate()'s host path against prepare_on_device.
There is no gate: the numbers go next to the hbm_kernels range of the bench line.
Every step is a child process under its own time limit; a step that fails or runs out of time ends the run.
Usage: python profiles/bench_prepare.py [outfile]   (default profiles/prepare_bench.txt)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
REPS = 3
LIMIT = {"array": 240, "device": 240, "kernels": 120, "pipeline": 240}


def _model():
    import torch
    import bench
    from vnet_tensorflow_amd import model as M
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = bench.config(128, 2, 1, 2, "fp32_split3")
    cfg["EvaluationSetting"] = {"Stride": [64, 64, 64], "BatchSize": 2, "ProbabilityOutput": False}
    m = M.image2label(None, cfg, device=torch.device("cuda", 0), verbose=False)
    m.read_config()
    m.build_model_graph()
    return m


def _evaluate(on_device):
    import hashlib
    import torch
    m = _model()
    vol = np.clip(127.5 + 40 * np.random.default_rng(0).standard_normal((256, 256, 256, 1)), 0, 255).astype(np.float32)
    case = lambda v: torch.from_numpy(v).to(m.device) if on_device else v
    m.evaluate_single_3D(case(vol[:192, :192, :192]))                 # warm-up: 8 windows, every kernel of the pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    label, _ = m.evaluate_single_3D(case(vol))
    torch.cuda.synchronize()
    return {"seconds": time.perf_counter() - t0, "label_sha": hashlib.sha256(label.tobytes()).hexdigest()[:16]}


def step_array(_):
    return _evaluate(False)


def step_device(_):
    return _evaluate(True)


def _timed(fn, reps=7, warm=3):
    import torch
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


def step_kernels(_):
    import torch
    from vnet_tensorflow_amd import ops
    dev = torch.device("cuda", 0)
    n, C = 256 ** 3, 4
    x = torch.empty((256, 256, 256, C), dtype=torch.float32, device=dev).normal_(100.0, 40.0)
    y = torch.empty_like(x)
    slot = torch.empty((128, 128, 128, C), dtype=torch.float32, device=dev)
    prm = torch.tensor([[0.0, 1.0, -20.0, 255.0 / 220.0, 0.0]] * C, dtype=torch.float64, device=dev)
    pre = torch.tensor([[100.0, 40.0]] * C, dtype=torch.float64, device=dev)
    res = {"stats_ms": _timed(lambda: ops.channel_stats(x)), "stats_pre_ms": _timed(lambda: ops.channel_stats(x, pre)),
           "window_ms": _timed(lambda: ops.window_intensity(x, prm, out=y)),
           "crop_ms": _timed(lambda: ops.crop_window(x, (64, 64, 64), (128, 128, 128), out=slot)),
           "argmax_ms": _timed(lambda: ops.argmax_label(x)),
           "torch_argmax_ms": _timed(lambda: torch.argmax(x, dim=-1).to(torch.int32))}
    x1 = torch.empty((256, 256, 256, 1), dtype=torch.float32, device=dev).normal_(100.0, 40.0)
    res["stats_c1_ms"] = _timed(lambda: ops.channel_stats(x1))
    prm1 = prm[:1].contiguous()
    res["window_c1_ms"] = _timed(lambda: ops.window_intensity(x1, prm1, out=x1))
    res.update(stats_bytes=8.0 * n * C, window_bytes=8.0 * n * C, crop_bytes=8.0 * 128 ** 3 * C, argmax_bytes=4.0 * n * (C + 1),
               stats_c1_bytes=8.0 * n, window_c1_bytes=8.0 * n)
    return res


def step_pipeline(_):
    """The reference's evaluate pipeline (StatisticalNormalization 2.5, Resample to 0.25 mm, Padding 128) on a 128^3 x 1 file of 0.5 mm
    voxels -> 256^3: evaluate()'s host path (NumPy normalisation, Resample up and down again, image and dummy label) against
    prepare_on_device (the upload of the file included), wall clock, the median of 5 after a warm-up."""
    import torch
    from vnet_tensorflow_amd import prepare as P, transforms as T
    dev = torch.device("cuda", 0)
    image = np.clip(127.5 + 40 * np.random.default_rng(1).standard_normal((128, 128, 128, 1)), 0, 255).astype(np.float32)
    spacing = (0.5, 0.5, 0.5)
    tf = [T.StatisticalNormalization(2.5), T.Resample(0.25, device=dev), T.Padding(128)]

    def host():
        return T.run_pipeline(tf, {'image': image, 'label': np.zeros(image.shape[:3], np.int32), 'spacing': spacing}, None)['image']

    def device():
        out = P.prepare_on_device(tf, torch.from_numpy(image).to(dev), spacing)[0]
        torch.cuda.synchronize()
        return out
    res = {}
    for name, fn in (("host", host), ("device", device)):
        fn()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        res[name + "_s"] = float(np.median(ts))
        res[name + "_shape"] = list(r.shape)
    a, b = host(), device().cpu().numpy()
    res["max_abs_diff"] = float(np.abs(a.astype(np.float64) - b).max())
    return res


STEPS = {"array": step_array, "device": step_device, "kernels": step_kernels, "pipeline": step_pipeline}


def child(step):
    """One step in a process of its own; None when it failed or ran out of time."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=LIMIT[step])
    except subprocess.TimeoutExpired:
        return None, "ran past its limit of %d s" % LIMIT[step]
    if r.returncode != 0:
        return None, "exit status %d: %s" % (r.returncode, " ".join((r.stderr or r.stdout).strip().splitlines()[-1:]))
    return json.loads(r.stdout.strip().splitlines()[-1]), None


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        print(json.dumps(STEPS[sys.argv[2]](None)), flush=True)
        return
    out = ["evaluate_single_3D, 256^3 x 1, V-Net 128^3 patches, stride 64, batch 2, fp32_split3 (28 patches): the case as an array against "
           "the case as a device tensor (csrc/prepare.hip), interleaved"]
    times, shas, done = {"array": [], "device": []}, set(), True
    for rep in range(REPS):
        for step in ("array", "device"):
            r, why = child(step)
            if r is None:
                out.append("%s, repetition %d: %s -- run ended" % (step, rep + 1, why))
                done = False
                break
            times[step].append(r["seconds"])
            shas.add(r["label_sha"])
            print("%s %.3f s" % (step, r["seconds"]), flush=True)
        if not done:
            break
    if done:
        a, d = float(np.median(times["array"])), float(np.median(times["device"]))
        for step in ("array", "device"):
            out.append("%-7s %s s   median %.3f s = %.1f patches/s" % (step, "  ".join("%.3f" % t for t in times[step]),
                                                                        float(np.median(times[step])), 28 / float(np.median(times[step]))))
        out.append("device / array = %.3f (%s); the labels of all %d runs are %s" % (
            d / a, "the device path is faster" if d < a else "THE DEVICE PATH IS SLOWER", 2 * REPS, "equal" if len(shas) == 1 else "NOT EQUAL"))
        k, why = child("kernels")
        if k is None:
            out.append("kernels: %s -- run ended" % why)
            done = False
        else:
            gbs = lambda b, ms: b / (ms * 1e-3) / 1e9
            row = lambda name, b, ms: "%-28s %8.3f ms  %7.0f GB/s  %4.1f %% of 8 TB/s" % (name, k[ms], gbs(k[b], k[ms]), 100 * gbs(k[b], k[ms]) * 1e9 / PEAK)
            out.append("kernels alone, 256^3 x 4 channels (x 1 where said), algorithmic bytes:")
            out.append(row("channel_stats", "stats_bytes", "stats_ms"))
            out.append(row("channel_stats, pre-map", "stats_bytes", "stats_pre_ms"))
            out.append(row("channel_stats x 1", "stats_c1_bytes", "stats_c1_ms"))
            out.append(row("window_intensity", "window_bytes", "window_ms"))
            out.append(row("window_intensity x 1", "window_c1_bytes", "window_c1_ms"))
            out.append(row("crop_window 128^3", "crop_bytes", "crop_ms"))
            out.append(row("argmax_label", "argmax_bytes", "argmax_ms"))
            out.append("torch.argmax + .to(int32)     %8.3f ms  (what argmax_label replaces)" % k["torch_argmax_ms"])
            p, why = child("pipeline")
            if p is None:
                out.append("pipeline: %s -- run ended" % why)
                done = False
            else:
                out.append("the evaluate pipeline (StatisticalNormalization 2.5, Resample 0.5 -> 0.25 mm, Padding 128) on a 128^3 x 1 file -> %s: "
                           "host path %.2f ms, prepare_on_device (upload included) %.2f ms = %.1f x; max |difference| of the prepared images %.3g"
                           % ("x".join(str(v) for v in p["device_shape"]), 1e3 * p["host_s"], 1e3 * p["device_s"], p["host_s"] / p["device_s"],
                              p["max_abs_diff"]))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prepare_bench.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out), flush=True)
    sys.exit(0 if done else 1)


if __name__ == "__main__":
    main()
