"""No GPU: the rules of mirrored passes and window weights (vnet_tensorflow_amd/window.py) against independent statements -- flip_sets'
order and refusals, the weight vectors against a float64 evaluation element by element, the two NumPy restatements against brute-force
triple loops (with ASYMMETRIC weight vectors: symmetric ones would hide weights indexed in the mirrored frame), the ledger of
csrc/vnet_window.h against the ctypes table and the entry points' error codes (both need the built library, no device), the ops on
CPU tensors, evaluate_case on a CPU model whose stand-in network is NOT mirror-equivariant, and the config keys and flags.  Every
comparison is `==`."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import guard
from tests.test_abi_ledger import RULE, _result_types
from vnet_tensorflow_amd import _lib, window as W
from vnet_tensorflow_amd._lib import VnetHipError

ROOT = guard.ROOT
SP = (0.7, 0.8, 2.5)


# ---- flip_sets --------------------------------------------------------------------------------------------------------------------------------
def test_flip_sets_order():
    assert W.flip_sets(None) == [0] and W.flip_sets([]) == [0] and W.flip_sets(()) == [0]
    assert W.flip_sets([0]) == [0, 1] and W.flip_sets([2]) == [0, 4]
    assert W.flip_sets([0, 2]) == [0, 1, 4, 5]
    assert W.flip_sets([2, 0]) == [0, 4, 1, 5]                       # binary counting order of the LISTED axes
    assert W.flip_sets([0, 1, 2]) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert W.flip_sets([[0, 1]]) == [0, 3]                           # the one joint flip RandomFlip(axes=[1, 1, 0]) trains
    assert W.flip_sets([[2], [0, 1], [1, 0, 2]]) == [0, 4, 3, 7]     # the given order
    assert W.flip_sets(np.array([0, 1]).tolist()) == [0, 1, 2, 3]


@pytest.mark.parametrize("bad, word", [
    ([3], "axis 3"), ([-1], "axis -1"), ([0, 1.5], "axis 1.5"), ([True], "axis True"), (["x"], "axis 'x'"),
    ([0, 0], "axis 0 twice"), ([[0, 1], [2, 2]], "axis 2 twice"), ([[0, 1], [1, 0]], "twice"), ([[0], []], "empty set"),
    ([[0], [4]], "axis 4"), ([0, [1]], "mixes"), ("012", "not a list"), (2, "not a list")])
def test_flip_sets_refusals(bad, word):
    with pytest.raises(ValueError, match=word):
        W.flip_sets(bad)


# ---- weight_vectors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps, sigma", [((8, 8, 8), 0.125), ((16, 16, 16), 0.125), ((128, 128, 128), 0.125), ((5, 16, 33), (0.2, 0.125, 0.5)),
                                       ((1, 2, 3), 0.25)])
def test_weight_vectors_formula(ps, sigma):
    w = W.weight_vectors("gaussian", ps, sigma)
    sig = (sigma,) * 3 if isinstance(sigma, float) else sigma
    assert len(w) == 3
    for v, P, s in zip(w, ps, sig):
        want = np.array([np.float32(math.exp(-0.5 * ((i - (P - 1) / 2.0) / (s * P)) ** 2)) for i in range(P)], dtype=np.float32)
        assert v.dtype == np.float32 and v.shape == (P,) and np.array_equal(v, want)
        assert np.array_equal(v, v[::-1]) and v.max() <= 1.0 and v.min() > 0.0            # symmetric; the centre weighs most
        assert int(np.argmax(v)) == (P - 1) // 2
    corner = np.float32(np.float32(w[0][0] * w[1][0]) * w[2][0])
    assert corner >= np.float32(2.0 ** -100)


def test_weight_vectors_corner_at_the_default_sigma():
    for P, want in ((8, 1.0e-8), (16, 6.9e-10), (128, 5.5e-11)):
        w = W.weight_vectors("gaussian", (P, P, P))
        corner = float(np.float32(np.float32(w[0][0] * w[1][0]) * w[2][0]))
        assert abs(corner / want - 1) < 0.05, (P, corner)


def test_weight_vectors_uniform_and_refusals():
    assert W.weight_vectors("uniform", (16, 16, 16)) is None and W.weight_vectors("uniform", (16, 16, 16), 1e-9) is None
    with pytest.raises(ValueError, match="WindowWeights"):
        W.weight_vectors("hann", (16, 16, 16))
    with pytest.raises(ValueError, match="WindowSigma"):
        W.weight_vectors("gaussian", (16, 16, 16), 0.0)
    with pytest.raises(ValueError, match="WindowSigma"):
        W.weight_vectors("gaussian", (16, 16, 16), (0.1, 0.1))
    with pytest.raises(ValueError, match="window shape"):
        W.weight_vectors("gaussian", (16, 16), 0.125)
    # the corner weight in float32 below 2^-100: exp(-3 * 0.5 * (7.5 / (16 s))^2) < 2^-100  <=>  s < 0.0689...
    assert W.weight_vectors("gaussian", (16, 16, 16), 0.07) is not None
    with pytest.raises(ValueError, match="2\\^-100"):
        W.weight_vectors("gaussian", (16, 16, 16), 0.068)
    with pytest.raises(ValueError, match="2\\^-100"):
        W.weight_vectors("gaussian", (128, 128, 128), 0.01)           # (the float32 product underflows to 0: refused all the same)


# ---- the restatements against triple loops --------------------------------------------------------------------------------------------------
def _f(a, n, flip):
    return n - 1 - a if flip else a


def brute_crop_flip(src, start, size, mask):
    out = np.zeros(tuple(size) + src.shape[3:], dtype=src.dtype)
    for i in range(size[0]):
        for j in range(size[1]):
            for k in range(size[2]):
                at = (start[0] + _f(i, size[0], mask & 1), start[1] + _f(j, size[1], mask & 2), start[2] + _f(k, size[2], mask & 4))
                if all(a < n for a, n in zip(at, src.shape[:3])):
                    out[i, j, k] = src[at]
    return out


def brute_accumulate(patch, vol, cnt, origin, mask, weights):
    P = patch.shape[:3]
    for i in range(P[0]):
        for j in range(P[1]):
            for k in range(P[2]):
                g = (origin[0] + i, origin[1] + j, origin[2] + k)
                if any(a >= n for a, n in zip(g, vol.shape[:3])):
                    continue
                p = patch[_f(i, P[0], mask & 1), _f(j, P[1], mask & 2), _f(k, P[2], mask & 4)]
                if weights is None:
                    vol[g] = vol[g] + p
                    if cnt is not None:
                        cnt[g] = cnt[g] + np.float32(1)
                else:
                    w = np.float32(np.float32(weights[0][i] * weights[1][j]) * weights[2][k])
                    vol[g] = vol[g] + w * p
                    if cnt is not None:
                        cnt[g] = cnt[g] + w


def asymmetric_weights(P, seed=0):
    """Three random float32 vectors in [2^-20, 1): no symmetry, so a weight indexed in the patch's frame gives another result."""
    rng = np.random.default_rng(seed)
    return tuple((rng.random(p) * (1 - 2.0 ** -20) + 2.0 ** -20).astype(np.float32) for p in P)


def softmax_like(shape, seed=0, zeros=0.1):
    """float32 values in [2^-20, 1] or exactly 0."""
    rng = np.random.default_rng(seed)
    x = np.exp2(-20 * rng.random(shape)).astype(np.float32)
    x[rng.random(shape) < zeros] = 0
    return x


@pytest.mark.parametrize("mask", range(8))
def test_crop_flip_np_is_the_triple_loop(mask):
    rng = np.random.default_rng(mask)
    for C in (None, 1, 3):
        src = rng.random((7, 6, 9) + (() if C is None else (C,))).astype(np.float32)
        for start, size in (((5, 3, 6), (4, 5, 6)), ((0, 0, 0), (7, 6, 9)), ((1, 2, 3), (2, 1, 3)), ((6, 5, 8), (3, 3, 3))):
            got = W.crop_flip_np(src, start, size, mask)
            assert got.dtype == src.dtype and np.array_equal(got, brute_crop_flip(src, start, size, mask)), (C, start, size)
    lab = rng.integers(0, 5, size=(7, 6, 9)).astype(np.int32)
    assert np.array_equal(W.crop_flip_np(lab, (5, 3, 6), (4, 5, 6), mask), brute_crop_flip(lab, (5, 3, 6), (4, 5, 6), mask))
    # inside the volume a mirrored crop is the flipped slice
    inside = W.crop_flip_np(src, (1, 1, 2), (4, 3, 5), mask)
    assert np.array_equal(inside, np.flip(src[1:5, 1:4, 2:7], axis=[a for a in range(3) if mask >> a & 1]))
    with pytest.raises(ValueError, match="window"):
        W.crop_flip_np(src, (7, 0, 0), (2, 2, 2), mask)


@pytest.mark.parametrize("mask", range(8))
def test_accumulate_np_is_the_triple_loop(mask):
    P, D, K = (4, 5, 6), (7, 6, 9), 3
    for kind in ("none", "asymmetric", "gaussian"):
        weights = {"none": None, "asymmetric": asymmetric_weights(P, mask), "gaussian": W.weight_vectors("gaussian", P, 0.3)}[kind]
        for origin in ((0, 0, 0), (2, 1, 3), (5, 3, 6), (7, 0, 0)):              # inside, inside, partly outside, wholly outside
            for with_cnt in (True, False):
                patch = softmax_like(P + (K,), seed=mask)
                vol = softmax_like(D + (K,), seed=50 + mask, zeros=0.5)
                cnt = softmax_like(D, seed=90 + mask, zeros=0.5) if with_cnt else None
                vol_b, cnt_b = vol.copy(), None if cnt is None else cnt.copy()
                W.accumulate_np(patch, vol, cnt, origin, mask, weights)
                brute_accumulate(patch, vol_b, cnt_b, origin, mask, weights)
                assert np.array_equal(vol, vol_b) and (cnt is None or np.array_equal(cnt, cnt_b)), (kind, origin, with_cnt)
    # the weights live in the volume's frame: mirroring the weight vectors with the patch is another result
    patch, weights = softmax_like(P + (K,), seed=1, zeros=0), asymmetric_weights(P, 3)
    a, b = np.zeros(D + (K,), np.float32), np.zeros(D + (K,), np.float32)
    W.accumulate_np(patch, a, None, (0, 0, 0), mask, weights)
    W.accumulate_np(patch, b, None, (0, 0, 0), mask, tuple(w[::-1] if mask >> i & 1 else w for i, w in enumerate(weights)))
    assert (mask == 0) == np.array_equal(a, b)


# ---- csrc/vnet_window.h: declared == bound == exported ----------------------------------------------------------------------------------------
def test_window_header_ledger():
    path = os.path.join(ROOT, W.HEADER)
    fns = guard.header_functions(path)
    assert set(fns) == set(W.SIGNATURES_WINDOW) == {"vnet_window_crop_flip", "vnet_window_accumulate"}
    exported = ctypes.CDLL(W.LIB_PATH)
    assert not [n for n in fns if not hasattr(exported, n)]
    results = _result_types(path)
    for name, params in fns.items():
        res, args = W.SIGNATURES_WINDOW[name]
        want = [ctypes.c_void_p if p[1] else RULE[p[3]] for p in params]
        assert args == want, (name, args, want)
        assert res is RULE[results[name]] and res is ctypes.c_int, name
    pointer = guard.pointer_entry_points(path)
    assert set(pointer) == set(fns) and all(ps[-1][0] == "stream" for ps in pointer.values())
    # a library of its own: none of these names is in the training library's registry, the header is not published
    assert not set(fns) & set(_lib.all_signatures()) and W.HEADER not in [h for h, _ in _lib.HEADERS]
    assert not os.path.exists(os.path.join(ROOT, "include", "vnet_window.h")) and os.path.basename(W.LIB_PATH) == "libvnet_window.so"
    main = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in fns if hasattr(main, n)]
    from vnet_tensorflow_amd import postprocess as PP
    post = ctypes.CDLL(PP.LIB_PATH)
    assert not [n for n in fns if hasattr(post, n)]
    mk = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "Makefile")).read()
    for word in ("WINDOW_SRCS = window.hip", "WINDOW_OBJS = $(WINDOW_SRCS:.hip=.o)", "WINDOW_LIB  = ../libvnet_window.so",
                 "$(WINDOW_OBJS): vnet_window.h", "-ffp-contract=off", "all: $(LIB) $(BIN) $(POST_LIB) $(WINDOW_LIB)",
                 "$(POST_OBJS) $(POST_LIB) $(WINDOW_OBJS) $(WINDOW_LIB)",
                 # the lines of libvnet_post.so, character for character
                 "POST_SRCS = postprocess.hip\nPOST_OBJS = $(POST_SRCS:.hip=.o)\nPOST_LIB  = ../libvnet_post.so\n",
                 "$(POST_OBJS): vnet_post.h\n\n$(POST_LIB): $(POST_OBJS)\n\t$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(POST_OBJS) -o $@\n"):
        assert word in mk, word
    srcs = [l for l in mk.splitlines() if l.startswith("SRCS = ")][0].split()[2:]
    assert len(srcs) == 18 and "window.hip" not in srcs
    unit = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "window.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and "fused multiply-add" in open(path).read()
    assert W.lib().vnet_window_accumulate.argtypes == W.SIGNATURES_WINDOW["vnet_window_accumulate"][1]


def test_error_codes_need_no_device():
    """Before any launch, in the documented order: VNET_E_BADARG (-1), then VNET_E_UNSUPPORTED (-2)."""
    L = W.lib()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    big = (2048, 1024, 1024)

    def crop(src=one, dst=two, vol=(7, 6, 9), C=1, start=(0, 0, 0), size=(4, 5, 6), mask=0):
        return L.vnet_window_crop_flip(src, dst, *vol, C, *start, *size, mask, None)

    assert crop(src=None) == -1 and crop(dst=None) == -1 and crop(dst=one) == -1 and crop(C=0) == -1
    assert crop(vol=(7, 0, 9)) == -1 and crop(size=(4, 5, 0)) == -1 and crop(size=(-1, 5, 6)) == -1
    assert crop(start=(-1, 0, 0)) == -1 and crop(start=(7, 0, 0)) == -1 and crop(start=(0, 6, 0)) == -1 and crop(start=(0, 0, 9)) == -1
    assert crop(mask=8) == -1 and crop(mask=-1) == -1
    assert crop(vol=big) == -2 and crop(size=big) == -2
    assert crop(vol=big, mask=8) == -1 and crop(size=big, start=(7, 0, 0)) == -1                # BADARG before UNSUPPORTED

    def acc(patch=one, vol=two, cnt=two, K=2, P=(4, 5, 6), o=(0, 0, 0), D=(7, 6, 9), mask=0, w=(None, None, None)):
        return L.vnet_window_accumulate(patch, vol, cnt, K, *P, *o, *D, mask, *w, None)

    assert acc(patch=None) == -1 and acc(vol=None) == -1 and acc(K=0) == -1 and acc(K=65536) == -1
    assert acc(P=(0, 5, 6)) == -1 and acc(D=(7, 6, 0)) == -1 and acc(o=(0, -1, 0)) == -1 and acc(mask=8) == -1 and acc(mask=-2) == -1
    assert acc(w=(one, None, None)) == -1 and acc(w=(one, one, None)) == -1 and acc(w=(None, one, one)) == -1
    assert acc(D=big) == -2 and acc(P=big) == -2 and acc(D=big, cnt=None, w=(one, one, one)) == -2
    assert acc(D=big, K=0) == -1 and acc(P=big, w=(one, None, one)) == -1                       # BADARG before UNSUPPORTED


# ---- the ops on CPU tensors -------------------------------------------------------------------------------------------------------------------
def test_ops_take_cpu_tensors_to_the_rules():
    rng = np.random.default_rng(2)
    src = rng.random((7, 6, 9, 3)).astype(np.float32)
    for mask in (0, 3, 7):
        got = W.crop_flip(torch.from_numpy(src), (5, 3, 6), (4, 5, 6), mask)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), W.crop_flip_np(src, (5, 3, 6), (4, 5, 6), mask))
        slot = torch.full((2, 4, 5, 6, 3), -1.0)
        assert W.crop_flip(torch.from_numpy(src), (5, 3, 6), (4, 5, 6), mask, out=slot[1]) is not None
        assert np.array_equal(slot[1].numpy(), got.numpy()) and (slot[0] == -1).all()
    lab = torch.from_numpy(rng.integers(0, 4, size=(7, 6, 9)).astype(np.int32))
    assert W.crop_flip(lab, (1, 1, 1), (3, 3, 3), 5).dtype == torch.int32
    P, D, K = (4, 5, 6), (7, 6, 9), 3
    patch, weights = softmax_like(P + (K,), 4), asymmetric_weights(P, 4)
    vol, cnt = torch.zeros(D + (K,)), torch.zeros(D)
    want_v, want_c = np.zeros(D + (K,), np.float32), np.zeros(D, np.float32)
    for origin, mask, w in (((2, 1, 3), 6, weights), ((5, 3, 6), 1, None)):
        W.accumulate(torch.from_numpy(patch), vol, cnt, origin, mask, None if w is None else tuple(torch.from_numpy(v) for v in w))
        W.accumulate_np(patch, want_v, want_c, origin, mask, w)
    assert np.array_equal(vol.numpy(), want_v) and np.array_equal(cnt.numpy(), want_c) and want_c.any()


def test_ops_refuse_mismatched_devices_and_dtypes():
    src = torch.zeros(7, 6, 9, 2)
    for bad in (torch.zeros(7, 6, 9, 2, dtype=torch.float64), torch.zeros(7, 6, 9, dtype=torch.float32), torch.zeros(7, 6, 9, dtype=torch.int64),
                torch.zeros(7, 6, 9, 2)[:, :, ::2], np.zeros((7, 6, 9, 2), np.float32)):
        with pytest.raises(VnetHipError, match="crop_flip"):
            W.crop_flip(bad, (0, 0, 0), (2, 2, 2), 0)
    for out in (torch.zeros(2, 2, 2, 2, dtype=torch.float64), torch.zeros(2, 2, 3, 2), torch.zeros(2, 2, 2, 2, device="meta"),
                torch.zeros(2, 2, 2, 4)[..., ::2]):
        with pytest.raises(VnetHipError, match="crop_flip: out"):
            W.crop_flip(src, (0, 0, 0), (2, 2, 2), 0, out=out)
    with pytest.raises(ValueError, match="window"):
        W.crop_flip(src, (7, 0, 0), (2, 2, 2), 0)
    with pytest.raises(ValueError, match="mask"):
        W.crop_flip(src, (0, 0, 0), (2, 2, 2), 8)
    P, D, K = (4, 5, 6), (7, 6, 9), 3
    ok = dict(patch=torch.zeros(P + (K,)), vol=torch.zeros(D + (K,)), cnt=torch.zeros(D), origin=(0, 0, 0), mask=0,
              weights=tuple(torch.ones(p) for p in P))
    W.accumulate(**ok)
    for key, bad, word in (("patch", torch.zeros(P + (K,), dtype=torch.float64), "patch is torch.float64"),
                           ("patch", torch.zeros(P + (K,), device="meta"), "patch is on meta"),
                           ("patch", torch.zeros(P + (K + 1,)), "patch .* and vol"),
                           ("cnt", torch.zeros(D, dtype=torch.int32), "cnt is torch.int32"),
                           ("cnt", torch.zeros(D, device="meta"), "cnt is on meta"),
                           ("cnt", torch.zeros(D + (1,)), "cnt .* for a volume"),
                           ("vol", torch.zeros(D + (K,))[:, :, ::2], "dense"),
                           ("weights", tuple(torch.ones(p, dtype=torch.float64) for p in P), "w0 is torch.float64"),
                           ("weights", (torch.ones(4), torch.ones(5), torch.ones(6, device="meta")), "w2 is on meta"),
                           ("weights", (torch.ones(4), torch.ones(5)), "three vectors"),
                           ("weights", (torch.ones(4), torch.ones(6), torch.ones(6)), "weight vectors"),
                           ("weights", (np.ones(4, np.float32),) * 3, "takes a tensor")):
        with pytest.raises(VnetHipError, match=word):
            W.accumulate(**dict(ok, **{key: bad}))
    with pytest.raises(ValueError, match="origin"):
        W.accumulate(**dict(ok, origin=(0, -1, 0)))


# ---- evaluate on a CPU model ------------------------------------------------------------------------------------------------------------------
VOLUME, PATCH, STRIDE, BATCH, K = (24, 20, 18), (16, 16, 16), (8, 8, 8), 4, 3


def _config(**evaluation):
    E = {"Data": {"EvaluateDataDirectory": ".", "ImageFilenames": ["image.nii"], "LabelFilename": "label_tf.nii"},
         "CheckpointPath": "ckpt", "Stride": list(STRIDE), "BatchSize": BATCH}
    E.update(evaluation)
    return {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": ".", "TestingDataDirectory": ".", "ImageFilenames": ["image.nii"], "LabelFilename": "label.nii"},
        "BatchSize": 1, "PatchShape": list(PATCH), "SegmentationClasses": [0, 1, 2], "Epoches": 1,
        "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 1], "BottomConvolutions": 1},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}},
        "Loss": {"Name": "sorensen"}}, "EvaluationSetting": E}


def stand_in_infer(batch):
    """A softmax that depends on the position inside the window: NOT mirror-equivariant, so un-mirroring, the pass order and the frame
    of the weights all show in the sums."""
    x = batch[..., 0]
    r = [torch.arange(p, dtype=torch.float32).view([1] + [p if a == b else 1 for b in range(3)]) / p for a, p in enumerate(PATCH)]
    logits = torch.stack([2 * x + r[0], 3 * x * r[1] + 0.5, 1.5 - x + r[2] * r[0]], dim=-1)
    return torch.softmax(logits, dim=-1)


def windows(dims, ps, st, batch):
    """The reference's enumeration (model.py:866-905): [[(s0, s1, s2)]] in batches, the last batch once more."""
    nums = [int(math.ceil((dims[a] - ps[a]) / float(st[a]))) + 1 for a in range(3)]
    flat = [tuple(min(n * st[a], dims[a] - ps[a]) for a, n in enumerate(ijk)) for ijk in np.ndindex(*nums)]
    out = [flat[i:i + batch] for i in range(0, len(flat), batch)]
    return out + [out[-1]]


def reference_sums(image, masks, weights, infer):
    """The independent loop: for each batch, for each mask (identity first), the mirrored batch through `infer` as a batch of its own,
    each window's softmax mirrored back, weighted in the volume's frame and added -- plain slicing, float32."""
    dims = tuple(max(s, p) for s, p in zip(image.shape[:3], PATCH))
    padded = np.zeros(dims + image.shape[3:], np.float32)
    padded[:image.shape[0], :image.shape[1], :image.shape[2]] = image
    vol, cnt = np.zeros(dims + (K,), np.float32), np.zeros(dims, np.float32)
    if weights is None:
        w = np.ones(PATCH, np.float32)
    else:
        w = (weights[0][:, None, None] * weights[1][None, :, None]) * weights[2][None, None, :]
    for batch in windows(dims, PATCH, STRIDE, BATCH):
        for mask in masks:
            axes = [a for a in range(3) if mask >> a & 1]
            crops = np.stack([np.flip(padded[tuple(slice(s, s + p) for s, p in zip(at, PATCH))], axis=axes) for at in batch])
            sm = infer(torch.from_numpy(np.ascontiguousarray(crops))).numpy()
            for at, p in zip(batch, sm):
                sl = tuple(slice(s, s + n) for s, n in zip(at, PATCH))
                back = np.flip(p, axis=axes)
                vol[sl] = vol[sl] + (back if weights is None else w[..., None] * back)
                cnt[sl] = cnt[sl] + w
    return vol, cnt


@pytest.fixture()
def cpu_model(monkeypatch):
    """A model on the CPU whose network is stood in for; ops.accumulate_patch, which has no CPU path, is stood in for as
    tests/test_postprocess_host.py does, and counts its calls."""
    from vnet_tensorflow_amd import model, ops
    m = model.image2label(None, _config(ProbabilityOutput=True), device=torch.device("cpu"), verbose=False)
    m.read_config()
    m.build_model_graph()
    calls = []

    def accumulate(patch, vol, cnt, origin):
        calls.append(origin)
        sl = tuple(slice(o, o + n) for o, n in zip(origin, patch.shape[:3]))
        vol[sl] += patch
        cnt[sl] += 1
    monkeypatch.setattr(m, "_infer", stand_in_infer)
    monkeypatch.setattr(ops, "accumulate_patch", accumulate)
    image = np.random.default_rng(5).random(VOLUME + (1,)).astype(np.float32)
    return m, image, calls


@pytest.mark.parametrize("mirror, kind, sigma", [([0, 2], "gaussian", 0.125), ([[0, 1]], "uniform", 0.125), ([], "gaussian", (0.2, 0.125, 0.3)),
                                                 ([0, 1, 2], "uniform", 0.125)])
def test_evaluate_case_on_a_cpu_model(cpu_model, mirror, kind, sigma):
    m, image, calls = cpu_model
    assert (m.evaluate_mirror, m.evaluate_window_weights, m.evaluate_window_sigma) == ([], "uniform", 0.125)
    plain, plain_prob = m.evaluate_case(image, SP, None, False)
    n_plain = len(calls)
    assert plain.shape == VOLUME and n_plain == sum(len(b) for b in windows(VOLUME, PATCH, STRIDE, BATCH)) and n_plain == 12     # 8 windows, the last batch of 4 once more
    vol, cnt = reference_sums(image, [0], None, stand_in_infer)
    assert np.array_equal(plain, np.argmax(vol, -1)) and np.array_equal(plain_prob, np.moveaxis(vol, -1, 0) / cnt)

    m.evaluate_mirror, m.evaluate_window_weights, m.evaluate_window_sigma = mirror, kind, sigma
    seen = []
    got, prob = m.evaluate_case(image, SP, None, False, on_label=lambda t: seen.append(t.numpy().copy()))
    assert len(calls) == n_plain                             # (the feature's passes do not go through ops.accumulate_patch)
    vol, cnt = reference_sums(image, W.flip_sets(mirror), W.weight_vectors(kind, PATCH, sigma), stand_in_infer)
    want, want_prob = np.argmax(vol, -1), np.moveaxis(vol, -1, 0) / cnt
    assert got.dtype == plain.dtype and np.array_equal(got, want) and prob.dtype == np.float32 and np.array_equal(prob, want_prob)
    assert len(seen) == 1 and seen[0].dtype == np.int32 and np.array_equal(seen[0], want)
    assert (prob != plain_prob).any() and (got != plain).any()

    # off again -- absent, [] or None, "uniform" or None: what it was, byte for byte, through ops.accumulate_patch
    for off in (dict(evaluate_mirror=[], evaluate_window_weights="uniform"), dict(evaluate_mirror=None, evaluate_window_weights=None), None):
        if off is None:
            del m.evaluate_mirror, m.evaluate_window_weights, m.evaluate_window_sigma
        else:
            m.__dict__.update(off)
        before = len(calls)
        again, again_prob = m.evaluate_case(image, SP, None, False)
        assert len(calls) == before + n_plain
        assert again.dtype == plain.dtype and again.tobytes() == plain.tobytes() and again_prob.tobytes() == plain_prob.tobytes()


# ---- the config keys and the command line -------------------------------------------------------------------------------------------------
def test_the_config_keys_and_the_command_line(tmp_path):
    from vnet_tensorflow_amd import batch_evaluate as BE, model
    p = inspect.signature(model.image2label.evaluate_single_3D).parameters
    assert list(p) == ["self", "images_np", "back_size", "back_ratio", "largest_component", "volume_threshold", "spacing", "extent",
                       "postprocess", "on_label"]
    m = model.image2label(None, _config(Mirror=[[0, 1]], WindowWeights="gaussian", WindowSigma=[0.2, 0.2, 0.1]), device=torch.device("cpu"),
                          verbose=False)
    m.read_config()
    assert (m.evaluate_mirror, m.evaluate_window_weights, m.evaluate_window_sigma) == ([[0, 1]], "gaussian", [0.2, 0.2, 0.1])
    args = ["-cd", str(tmp_path), "-d", str(tmp_path), "-o", str(tmp_path)]
    a = BE.get_args(args)
    assert a.mirror is None and a.window_weights is None and a.window_sigma is None
    a = BE.get_args(args + ["--mirror", "0", "1", "2", "--window_weights", "uniform", "gaussian", "--window_sigma", "0.2"])
    assert a.mirror == [0, 1, 2] and a.window_weights == ["uniform", "gaussian"] and a.window_sigma == 0.2
    with pytest.raises(SystemExit):
        BE.get_args(args + ["--mirror", "3"])
    with pytest.raises(SystemExit):
        BE.get_args(args + ["--window_weights", "hann"])
    cfg = {"TrainingSetting": {"PatchShape": [16, 16, 16]}, "EvaluationSetting": {"Mirror": [2], "WindowSigma": 0.3}}
    keep = BE.Batch_Evaluate(config_json=cfg, patch_size=None, patch_layer=None).config()["EvaluationSetting"]
    assert keep == {"Mirror": [2], "WindowSigma": 0.3}
    over = BE.Batch_Evaluate(config_json=cfg, patch_size=None, patch_layer=None, mirror=[0, 1], window_weights="gaussian", window_sigma=0.2)
    assert over.config()["EvaluationSetting"] == {"Mirror": [0, 1], "WindowSigma": 0.2} and cfg["EvaluationSetting"]["Mirror"] == [2]
    assert over.window_weights == ["gaussian"]
    with pytest.raises(ValueError, match="axis 3"):
        BE.Batch_Evaluate(mirror=[3])
    with pytest.raises(ValueError, match="twice"):
        BE.Batch_Evaluate(mirror=[1, 1])
    with pytest.raises(AssertionError):
        BE.Batch_Evaluate(window_weights=["hann"])
    name = BE.Batch_Evaluate.csv_name
    assert name(7, 8, 4) == "result_checkpoint-7_stride_inplane-8_stride_layer-4.csv" == name(7, 8, 4, "uniform", [0])
    assert name(7, 8, 4, "gaussian", [0]) == "result_checkpoint-7_stride_inplane-8_stride_layer-4_window-gaussian.csv"
    assert name(7, 8, 4, "gaussian", W.flip_sets([0, 1, 2])) == "result_checkpoint-7_stride_inplane-8_stride_layer-4_window-gaussian_mirror-012.csv"
    assert name(7, 8, 4, "uniform", W.flip_sets([[0, 1]])) == "result_checkpoint-7_stride_inplane-8_stride_layer-4_window-uniform_mirror-01.csv"


def test_batch_evaluate_sweeps_the_window_weights(tmp_path, monkeypatch):
    """The window weights are a further dimension inside the stride loop: set on the model per combination like the stride, one CSV
    each, and the best-result dictionaries name them only when they are swept."""
    from tests.test_score_host import CFG, StandIn, _sweep_folders
    from vnet_tensorflow_amd import batch_evaluate as BE
    ck, dat, out = _sweep_folders(tmp_path)

    class Weighted(StandIn):
        def evaluate_case(self, image, spacing, tf, regrid, on_label=None):
            self.calls.append((self.step, tuple(self.evaluate_stride), self.evaluate_window_weights))
            label = self.label_of(image, self.step + (7 if self.evaluate_window_weights == "gaussian" else 0), self.evaluate_stride)
            on_label(torch.from_numpy(label.astype(np.int32)))
            return label, None

    def sweep(**kw):
        models = []
        monkeypatch.setattr(BE.Batch_Evaluate, "build_model", lambda self, cfg: models.append(Weighted(cfg)) or models[-1])
        sub = out / ("run%d" % len(os.listdir(str(out)) if out.exists() else []))
        be = BE.Batch_Evaluate(config_json=CFG, model_folder=str(ck), output_folder=str(sub), data_folder=str(dat),
                               ground_truth_filename="label.npy", stride_layer_min=4, stride_layer_max=4, stride_inplane_min=8,
                               stride_inplane_max=10, patch_size=None, patch_layer=None, step=2, checkpoint_min=6, checkpoint_max=12,
                               batch_size=3, **kw)
        best = be.Execute()
        return best, models[0], sorted(os.listdir(str(sub)))

    out.mkdir(exist_ok=True)
    best, model, files = sweep()
    assert files == ["result_checkpoint-10_stride_inplane-%d_stride_layer-4.csv" % a for a in (10, 8)]
    assert set(best[0]) == {"ckpt", "stride_inplane", "stride_layer"} and [c[2] for c in model.calls] == ["uniform"] * 4
    best, model, files = sweep(window_weights=["uniform", "gaussian"], mirror=[0, 2])
    assert files == sorted("result_checkpoint-10_stride_inplane-%d_stride_layer-4_window-%s_mirror-02.csv" % (a, k)
                           for a in (8, 10) for k in ("uniform", "gaussian"))
    assert [c[1:] for c in model.calls[::2]] == [((a, a, 4), k) for a in (8, 10) for k in ("uniform", "gaussian")]   # inside the stride loop
    assert model.cfg["EvaluationSetting"]["Mirror"] == [0, 2]
    for b in best:
        assert set(b) == {"ckpt", "stride_inplane", "stride_layer", "window_weights", "mirror"} and b["window_weights"] in ("uniform", "gaussian")
    best, model, files = sweep(window_weights="gaussian")
    assert files == ["result_checkpoint-10_stride_inplane-%d_stride_layer-4_window-gaussian.csv" % a for a in (10, 8)]
    assert set(best[0]) == {"ckpt", "stride_inplane", "stride_layer"}
