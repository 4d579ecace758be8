"""Run once on an MI355X: profiles/summary_bench.txt (one run; medians of 7 repetitions after 3 warm-up calls; no spread was measured).

The image summaries of a 128^3 step (include/vnet_hip_summary.h) at BASELINE's C3 shape (1 input channel, 2 classes,
fp32) and C5 shape (4 input channels, 5 classes, bf16 storage), batch 1:
    kernels      : ops.summary_slices_intensity (images), _index (int32 label, int64 prediction) and _rainbow (softmax) on resident
                   tensors into resident outputs, HIP events; the bytes each moves (source read once, output written once) over the time,
                   and that rate as a fraction of a device-to-device copy of 64 MiB timed the same way in the same process
    copy         : the one asynchronous copy of a summary's bytes into pinned host memory, HIP events
    host PNG     : summary.image_value over every slice of the summary (zlib level summary.PNG_LEVEL), one thread, wall clock
    steps        : image2label.train_step at that shape: a plain replayed step against a summary step (SummaryInterval 1, ImageLog),
                   wall clock on the training thread with a device synchronisation after each step, and the time close() then needs to
                   drain the writer's queue
No target is fixed for any of these figures.  Every configuration is a child process under its own time limit; the first failure ends
the run.   Usage: python profiles/bench_summary.py [outfile]   (default profiles/summary_bench.txt)"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 128
STEPS = [("c3", 1, 2, "fp32", 400), ("c5", 4, 5, "bf16", 400)]


def step(name, channels, classes, compute):
    import torch
    import bench
    from vnet_tensorflow_amd import model as M
    from vnet_tensorflow_amd import ops, summary as S
    from vnet_tensorflow_amd.data import synthetic_case
    dev = torch.device("cuda", 0)

    def events(fn, warm=3, reps=7):
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

    im, lb = synthetic_case([P] * 3, channels, classes, 1000)
    images = torch.from_numpy(im[None]).to(dev)
    labels = torch.from_numpy(lb[None, ..., None].astype(np.int32)).to(dev)
    logits = torch.from_numpy(np.random.default_rng(0).normal(0, 2, (1, P, P, P, classes)).astype(np.float32)).to(dev)
    sm, pred = ops.softmax_argmax(logits)
    pred = pred.reshape(1, P, P, P, 1)
    n = P ** 3
    factor = S.index_factor(classes, list(range(classes)))
    outs = [torch.empty(k, dtype=torch.uint8, device=dev) for k in (n * channels, n, n, 3 * n * classes)]
    a, b = torch.empty(64 << 20, dtype=torch.uint8, device=dev), torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    t_copy = events(lambda: b.copy_(a))
    rate = 2.0 * (64 << 20) / (t_copy * 1e-3)
    rows = [("intensity  f32 x%d" % channels, 5.0 * n * channels, lambda: ops.summary_slices_intensity(images, out=outs[0])),
            ("label      i32", 5.0 * n, lambda: ops.summary_slices_index(labels, factor, out=outs[1])),
            ("prediction i64", 9.0 * n, lambda: ops.summary_slices_index(pred, factor, out=outs[2])),
            ("rainbow    f32 x%d" % classes, 7.0 * n * classes, lambda: ops.summary_slices_rainbow(sm, out=outs[3]))]
    print("RESULT %s: 128^3, %d input channel(s), %d classes, %s; device-to-device copy of 64 MiB %.3f ms = %.2f TB/s (read + write)"
          % (name, channels, classes, compute, t_copy, rate / 1e12), flush=True)
    total_ms, total_bytes = 0.0, 0.0
    for what, nbytes, fn in rows:
        ms = events(fn)
        total_ms += ms
        total_bytes += nbytes
        print("RESULT   kernel %-20s %7.3f ms  %6.1f MB  %5.2f TB/s  %4.2f of the copy rate" % (
            what, ms, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12, nbytes / (ms * 1e-3) / rate), flush=True)
    print("RESULT   kernels together        %7.3f ms  %6.1f MB" % (total_ms, total_bytes / 1e6), flush=True)
    assert np.array_equal(outs[3].cpu().numpy().reshape(1, classes, P, P, P, 3)[0, :, :2], S.slices_rainbow(sm[:, :, :, :2].cpu().numpy())[0])
    flat = torch.cat(outs)
    host = torch.empty(flat.numel(), dtype=torch.uint8, pin_memory=True)
    t_d2h = events(lambda: host.copy_(flat, non_blocking=True))
    print("RESULT   device-to-host copy     %7.3f ms  %6.1f MB  %5.1f GB/s (pinned, asynchronous)" % (
        t_d2h, flat.numel() / 1e6, flat.numel() / (t_d2h * 1e-3) / 1e9), flush=True)
    torch.cuda.synchronize()
    arr = host.numpy()
    grey = arr[:n * (channels + 2)].reshape(-1, P, P)
    rgb = arr[n * (channels + 2):].reshape(-1, P, P, 3)
    t0 = time.perf_counter()
    png_bytes = sum(len(S.image_value(s)[3]) for s in grey) + sum(len(S.image_value(s)[3]) for s in rgb)
    t_png = (time.perf_counter() - t0) * 1e3
    print("RESULT   host PNG per summary    %7.1f ms  %d images, %.1f MB of pixels -> %.1f MB of PNG (zlib level %d, one thread)" % (
        t_png, len(grey) + len(rgb), arr.size / 1e6, png_bytes / 1e6, S.PNG_LEVEL), flush=True)
    del outs, flat, a, b, logits, sm, pred

    # a summary step against a plain replayed step
    np.random.seed(42)
    cfg = bench.config(P, 1, channels, classes, compute)
    with tempfile.TemporaryDirectory() as tmp:
        cfg["TrainingSetting"].update(LogDir=os.path.join(tmp, "log"), ImageLog=True, SummaryInterval=1)
        m = M.image2label(None, cfg, device=dev, verbose=False)
        m.read_config()
        m.build_model_graph()
        m._setup_training()

        def timed(k):
            ts = []
            for _ in range(k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.train_step(images, labels, dropout=0.0)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))
        timed(6)                                        # warm-up steps and the capture
        assert m.step_mode() == "whole" and m._graphs is not None
        plain = timed(10)
        with ops.context(m.ctx):
            m._open_summaries()
        try:
            timed(2)
            with_summary = timed(5)
            t0 = time.perf_counter()
        finally:
            m._close_summaries()
        drain = (time.perf_counter() - t0) * 1e3
        size = sum(os.path.getsize(f) for f in S.event_files(tmp))
        steps = [e[1] for f in S.event_files(tmp) for e in S.read_events(f)][1:]
    print("RESULT   train_step, training thread: replayed %.2f ms   summary step (eager enqueue + render + metrics read-backs) %.2f ms   "
          "close() drained the queue of the last steps in %.0f ms   %d events, %.1f MB on disk, read back CRC-clean"
          % (plain, with_summary, drain, len(steps), size / 1e6), flush=True)
    return 0


def main():
    if len(sys.argv) == 6 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "summary_bench.txt")
    out = ["image summaries of a 128^3 step (csrc/summary.hip, vnet_tensorflow_amd/summary.py): kernels, copy, PNG encoding, step time"]
    rc = 0
    for name, channels, classes, compute, limit in STEPS:
        # one child per configuration, each under its own time limit; a step that fails or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, str(channels), str(classes), compute]
        res = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l[7:] for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        out += lines
        print("\n".join(lines), flush=True)
        if res.returncode != 0:
            out.append("%s: step ended with status %d; the run stops here\n%s" % (name, res.returncode, res.stderr[-2000:]))
            print(out[-1], flush=True)
            rc = res.returncode
            break
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
