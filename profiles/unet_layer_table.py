"""U-Net numbers on one box (writes profiles/unet_layer_table.txt style output to stdout):
  * per-layer table of one eager U-Net step (128^3, 1 channel, 2 classes, NumChannel 16, 4 levels, 2 + 2 convolutions, fp32, B = 1) through
    ops.profile_start;
  * 3^3 forward / filter gradient against the 5^3 fp32 kernels at the same tensor shape in the same run, TF/s of algorithmic flops;
  * the pooling kernels against bn_act_fwd on the same fine tensor, GB/s of algorithmic bytes.
    python profiles/unet_layer_table.py"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from oracle.vnet_oracle import synthetic_batch
from vnet_tensorflow_amd import ops
from vnet_tensorflow_amd.model import image2label

dev = torch.device("cuda", 0)


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def step_table():
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": "synthetic", "TestingDataDirectory": "synthetic", "ImageFilenames": ["image.npy"],
                 "LabelFilename": "label.npy", "Synthetic": {"Cases": 2}},
        "SegmentationClasses": [0, 1], "BatchSize": 1, "PatchShape": [128] * 3, "ComputeDtype": "fp32",
        "Networks": {"Name": "UNet", "Dropout": 0.0, "NumChannel": 16, "NumLevels": 4, "NumConvolutions": 2, "BottomConvolutions": 2},
        "Loss": {"Name": "sorensen"}, "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-3, "Decay": {"Factor": 0.99, "Steps": 100}}}}
    import os
    os.environ["VNET_STEP_GRAPH"] = "0"
    m = image2label(None, cfg, device=dev, verbose=False)
    m.read_config(); m.build_model_graph(); m._setup_training()
    x, l = synthetic_batch(1, 128, 1, 2, seed=1)
    x, l = torch.from_numpy(x).to(dev), torch.from_numpy(l).to(dev)
    for _ in range(3):
        m.train_step(x, l)
    torch.cuda.synchronize()
    ms = timed(lambda: m.train_step(x, l), n=5, warm=0)
    ops.profile_start()
    m.train_step(x, l)
    recs = ops.profile_stop()
    print("U-Net step 128^3 x 1, 1 -> 2 classes, NumChannel 16, 4 levels, 2 + 2 convolutions, fp32, eager: %.2f ms per step (5 steps)" % ms)
    agg = collections.OrderedDict()
    for tag, fl, nb, t in recs:
        a = agg.setdefault(tag, [0, 0.0, fl, nb])
        a[0] += 1; a[1] += t
    print("%-44s %3s %9s %8s %8s" % ("launch", "n", "ms total", "TF/s", "GB/s"))
    tot = 0.0
    for tag, (n, t, fl, nb) in agg.items():
        tot += t
        print("%-44s %3d %9.3f %8.1f %8.0f" % (tag, n, t, fl * n / t / 1e9 if t else 0, nb * n / t / 1e6 if t else 0))
    print("timed conv-family + pooling launches: %.2f ms" % tot)
    del m
    torch.cuda.empty_cache()


def conv_vs_5():
    print("\n3^3 against the 5^3 fp32 kernel at the same tensor shape (TF/s of algorithmic flops; ratio = 3^3 / 5^3)")
    print("%-26s %10s %10s %6s | %10s %10s %6s" % ("shape", "fwd 3^3", "fwd 5^3", "ratio", "wgrad 3^3", "wgrad 5^3", "ratio"))
    for (P, C0, C1, Co) in ((128, 16, 0, 16), (64, 32, 0, 32), (64, 32, 32, 32), (32, 64, 0, 64), (16, 128, 0, 128), (8, 256, 0, 256)):
        x0 = torch.randn(1, P, P, P, C0, device=dev)
        x1 = torch.randn(1, P, P, P, C1, device=dev) if C1 else None
        dy = torch.randn(1, P, P, P, Co, device=dev)
        row = []
        for ks in (3, 5):
            w = torch.randn(ks, ks, ks, C0 + C1, Co, device=dev) * 0.05
            y = torch.empty(1, P, P, P, Co, device=dev)
            dw = torch.empty_like(w)
            r = ops.route(ops.FWD, ks, 1, 0, False, False, C0, C1, Co, 1, (P,) * 3, (P,) * 3)
            rw = ops.route(ops.WGRAD, ks, 1, 0, False, False, C0, C1, Co, 1, (P,) * 3, (P,) * 3)
            tf = timed(lambda: ops._conv_launch(r, x0, x1, w, None, y))
            tw = timed(lambda: ops._wgrad_launch(rw, x0, x1, dy, dw))
            row.append((r.flops / tf / 1e9, rw.flops / tw / 1e9, tf, tw))
        print("%-26s %10.1f %10.1f %6.2f | %10.1f %10.1f %6.2f   (fwd %.3f / %.3f ms, wgrad %.3f / %.3f ms)" % (
            "%d^3 %d%s->%d" % (P, C0, "+%d" % C1 if C1 else "", Co), row[0][0], row[1][0], row[0][0] / row[1][0],
            row[0][1], row[1][1], row[0][1] / row[1][1], row[0][2], row[1][2], row[0][3], row[1][3]))


def pool_vs_bn():
    print("\npooling against bn_act_fwd on the same fine tensor (GB/s of algorithmic bytes)")
    for (P, C) in ((128, 16), (64, 32), (32, 64)):
        x = torch.randn(1, P, P, P, C, device=dev)
        gamma, beta, mean, invstd = (torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev))
        L = __import__("vnet_tensorflow_amd")._lib.lib()
        y = torch.empty(1, P // 2, P // 2, P // 2, C, device=dev)
        dyc, dx, out = torch.randn_like(y), torch.empty_like(x), torch.empty_like(x)
        s = lambda: torch.cuda.current_stream().cuda_stream
        M = P ** 3
        tb = timed(lambda: L.vnet_bn_act_fwd(x.data_ptr(), None, 0, M, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1, None, out.data_ptr(), s()))
        tf = timed(lambda: L.vnet_maxpool2_fwd(x.data_ptr(), y.data_ptr(), C, 1, P, P, P, s()))
        tbw = timed(lambda: L.vnet_maxpool2_bwd(dyc.data_ptr(), x.data_ptr(), y.data_ptr(), dx.data_ptr(), C, 1, P, P, P, 0, s()))
        n = x.numel() * 4.0
        print("%d^3 x %d: bn_act_fwd %.0f GB/s (%.3f ms) | maxpool2 fwd %.0f GB/s (%.3f ms) | maxpool2 bwd %.0f GB/s (%.3f ms)" % (
            P, C, 2 * n / tb / 1e6, tb, 1.125 * n / tf / 1e6, tf, 2.25 * n / tbw / 1e6, tbw))


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    conv_vs_5()
    pool_vs_bn()
    step_table()
