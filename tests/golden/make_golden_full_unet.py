"""Full-size golden vectors of the 3-D U-Net from the CPU oracle (oracle/vnet_oracle.py + tests/unet_oracle.py, numpy float64): the
configuration profiles/unet_layer_table.py times, UNetOracle(K = 2, dropout 0, NumChannel 16, 4 levels, 2 + 2 convolutions, relu), one
training step on oracle.synthetic_batch with weights from ParamStore(rng = default_rng(weight seed)):

    unet_128cube.npz             128^3, B = 1, weight seed 42, input seed 1000   (105 s, 17 GB on 8 cores)
    unet_64cube_b2.npz           64^3,  B = 2, weight seed 42, input seed 3000   (30 s)
    spread/unet_128cube_s{1,2}.npz, spread/unet_64cube_b2_s{2,3}.npz             weight seed 42 + 101 s, input seed ... + 17 s

The stored quantities are those of make_golden_full.py (same SAMPLE / STRIDE / sample_indices), except that logits_sample and
grad_sample are float64: tests/test_unet_host.py holds tests/unet_torch.py in float64 to these files at 1e-9 / 1e-7, which float32
storage could not express.

The 128^3 fixture also carries teacher-forcing crops (O.CAPTURE), ROUNDED TO FLOAT32: for six 3^3 layers the tensor the layer actually
read and the gradient that actually arrived at its output, on a TF_BOX of output voxels + 1 voxel of halo, and for the level-1
max-pooling the fine input crop and the coarse gradient crop.  They are one file per layer and operand under unet_tf/ so that no
committed file passes 1 MiB (the 128 -> 128 gradient crop alone is 0.8 MB).

The argmax bound of tests/test_hip_golden_full_unet.py (>= 99.99 % agreement on the strided sample) is a condition on the draws, not a
measurement: profiles/unet_golden_full_errors_cpu.py checks that tests/unet_torch.py in fp32 meets it on every committed draw; a draw
that does not is replaced by the next s (SPREAD below names the one that was).

    python tests/golden/make_golden_full_unet.py [u128 | u64b2 | u128s1 | ...]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import vnet_oracle as O  # noqa: E402
from tests import unet_oracle as U  # noqa: E402
from tests.golden.make_golden_full import SAMPLE, STRIDE, TF_BOX, sample_indices, tf_crop  # noqa: E402

CONFIG = (2, 0.0, 16, 4, 2, 2, "relu")          # K, dropout, NumChannel, levels, convolutions, bottom convolutions, activation

CASES = {
    # name: (file, P, B, input seed)
    "u128": ("unet_128cube.npz", 128, 1, 1000),
    "u64b2": ("unet_64cube_b2.npz", 64, 2, 3000),
}
WEIGHT_SEED = {"u128": 42, "u64b2": 42}
# two more draws of each on make_golden_full.py's scheme (weight seed 42 + 101 s, input seed ... + 17 s).  The 64^3 draws are s = 2, 3:
# on s = 1 the fp32 yardstick itself disagrees with the oracle's argmax in 1 of the 8192 sampled voxels (99.9878 %), which the
# 99.99 % condition does not allow, so that draw was replaced by the next one.
SPREAD = {"u128": (1, 2), "u64b2": (2, 3)}
for _c, _draws in SPREAD.items():
    for _s in _draws:
        _f, _P, _B, _seed = CASES[_c]
        CASES["%ss%d" % (_c, _s)] = ("spread/%s_s%d.npz" % (_f[:-len(".npz")], _s), _P, _B, _seed + 17 * _s)
        WEIGHT_SEED["%ss%d" % (_c, _s)] = 42 + 101 * _s

# teacher-forcing crops (case u128): layer -> (short tag, origin of a TF_BOX of OUTPUT voxels, clipped to the level's size)
TF_CASE = "u128"
TF_DIR = "unet_tf"
TF_LAYERS = {
    "unet/encoder/level_1/conv_1/weights": ("enc1_conv1", (0, 60, 56)),        # 1 -> 16 @128^3, on the z = 0 face
    "unet/encoder/level_1/conv_2/weights": ("enc1_conv2", (60, 120, 112)),     # 16 -> 16 @128^3, high y / x faces
    "unet/decoder/level_1/conv_1/weights": ("dec1_conv1", (33, 47, 21)),       # 16 + 16 -> 16 @128^3: the two bn_concat halves
    "unet/encoder/level_2/conv_2/weights": ("enc2_conv2", (28, 30, 40)),       # 32 -> 32 @64^3
    "unet/encoder/level_4/conv_2/weights": ("enc4_conv2", (4, 8, 0)),          # 128 -> 128 @16^3, y high and both x faces
    "unet/bottom_level/conv_2/weights": ("bottom_conv2", (0, 0, 0)),           # 256 -> 256 @8^3: the whole volume
}
# the level-1 max-pooling: origin of a TF_BOX of COARSE voxels (the fine crop is the 2x box at 2x the origin).  Its output is the
# tensor encoder/level_2/conv_1 reads, so CAPTURE of that layer gives the pooled Var, its gradient and (through the tape) its input.
TF_POOL = ("pool1", "unet/encoder/level_2/conv_1/weights", (8, 16, 16))


def make_net(weight_seed):
    ps = O.ParamStore(rng=np.random.default_rng(weight_seed))
    return U.UNetOracle(*CONFIG, ps), ps


def creation_order(weight_seed=42):
    """(names of the trainables in creation order, {name: float64 value}) of the configuration."""
    net, ps = make_net(weight_seed)
    net.GetNetwork(np.zeros((1, 16, 16, 16, 1)))
    return list(ps.vars.keys()), {k: v.v for k, v in ps.vars.items()}


def tf_path(tag, operand, root=HERE):
    return os.path.join(root, TF_DIR, "%s.%s.npz" % (tag, operand))


def load_tf(tag, root=HERE):
    """(x, dy, low corner of the crop) of a teacher-forcing entry, float64 arrays holding float32 values."""
    zx, zd = np.load(tf_path(tag, "x", root)), np.load(tf_path(tag, "dy", root))
    return zx["a"].astype(np.float64), zd["a"].astype(np.float64), [int(v) for v in zx["lo"]]


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def make(case, root=HERE, P=None, teacher=None):
    """One oracle step of `case` -> root/<file>.  P overrides the patch size (tests/test_unet_host.py runs the recipe at 16^3);
    teacher: store the teacher-forcing crops (default: the TF_CASE at its own size)."""
    fname, P0, B, seed = CASES[case]
    teacher = (case == TF_CASE and P is None) if teacher is None else teacher
    P = P or P0
    K = CONFIG[0]
    t0 = time.time()
    net, ps = make_net(WEIGHT_SEED[case])
    x, lab = O.synthetic_batch(B, P, 1, K, seed=seed)
    O.CAPTURE = {} if teacher else None
    try:
        res = O.run_step(x.astype(np.float64), lab, net, "sorensen")
        if teacher:
            os.makedirs(os.path.join(root, TF_DIR), exist_ok=True)
            for name, (tag, origin) in TF_LAYERS.items():
                xin, yout = O.CAPTURE[name]
                cx, lo = tf_crop(xin.v, origin, halo=1)
                cg, _ = tf_crop(yout.g, origin, halo=1)
                np.savez_compressed(tf_path(tag, "x", root), a=_f32(cx), lo=np.asarray(lo, dtype=np.int32))
                np.savez_compressed(tf_path(tag, "dy", root), a=_f32(cg), lo=np.asarray(lo, dtype=np.int32))
            tag, name, origin = TF_POOL
            pooled = O.CAPTURE[name][0]
            fine = pooled._parents[0]
            co = (slice(None),) + tuple(slice(origin[a], origin[a] + TF_BOX[a]) for a in range(3))
            fi = (slice(None),) + tuple(slice(2 * origin[a], 2 * (origin[a] + TF_BOX[a])) for a in range(3))
            assert fine.v.shape[1] == 2 * pooled.v.shape[1]
            np.savez_compressed(tf_path(tag, "x", root), a=_f32(fine.v[fi]), lo=np.asarray(origin, dtype=np.int32))
            np.savez_compressed(tf_path(tag, "dy", root), a=_f32(pooled.g[co]), lo=np.asarray(origin, dtype=np.int32))
    finally:
        O.CAPTURE = None
    sm = res["softmax"]
    oh = (lab[..., 0][..., None] == np.arange(K)).astype(np.float64)
    ax = (1, 2, 3)
    names = list(ps.vars.keys())
    grads = [res["grads"][k] for k in names]
    s = (slice(None),) + (slice(None, None, STRIDE),) * 3
    out = {"loss": np.float64(res["loss"]),
           "config": np.array([P, B, WEIGHT_SEED[case], seed], dtype=np.int64),
           "dice_I": (sm * oh).sum(ax), "dice_L": sm.sum(ax), "dice_R": oh.sum(ax),
           "logits_sample": res["logits"][s].astype(np.float64), "pred_sample": res["pred"][s].astype(np.int8),
           "logits_absmax": np.float64(np.abs(res["logits"]).max()),
           "names": np.array(names),
           "grad_norm": np.array([np.linalg.norm(g) for g in grads]),
           "grad_sum": np.array([g.sum() for g in grads]),
           "grad_head": np.stack([np.resize(g.ravel()[:8], 8) for g in grads]),
           "grad_sample": np.stack([np.resize(g.ravel()[sample_indices(i, g.size)], SAMPLE) for i, g in enumerate(grads)]).astype(np.float64),
           "oracle_seconds": np.float64(time.time() - t0)}
    for k, v in ps.state.items():
        out["state:" + k] = v.astype(np.float32)
    path = os.path.join(root, fname)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(case, "loss %.9f" % res["loss"], "seconds %.0f" % (time.time() - t0), flush=True)
    return path


if __name__ == "__main__":
    for c in (sys.argv[1:] or list(CASES)):
        make(c)
