"""-m gpu: training resumed from a checkpoint is the same training, bit for bit.

The state that has to survive a save / load is spread over the flat parameter buffer (parameters are views into it), the
optimiser's slots (updated in place: a captured step graph holds their addresses), the device step state (learning rate, Adam's
lr_t, the step number that selects the dropout masks -- all derived from global_step and optimizer.t on every step), the moving
statistics, the packed filter images (a captured graph reads them without checking their tags) and the warm-up / capture
counters of the step graph.  Each can be wrong while every tensor in the file still round-trips, so the comparison here is the
TRAJECTORY: the steps taken after the load against the steps the uninterrupted run takes, with torch.equal / == and no
tolerance anywhere.

Per case (an each-choice table: every network, optimiser, compute mode, dropout, loss, step path and container at least once,
every compute mode with the graph), with N = 4 steps before the checkpoint and M = 5 after it:
  A  one model, N + M steps                                               (the uninterrupted run)
  B  model 1 takes N steps and saves; a second model, built under another np.random.seed, loads and takes M steps
  C  (graph cases) model A itself -- N + M steps old, holding its captured graph and settled packed filters -- loads the
     checkpoint of step N and takes M steps again, replaying its old graph straight away.
Negative controls, each a test of its own, show that the comparison can fail: a load without the optimiser, packed images left
stale under the captured graph, a step counter set back by one.

The train()-level test does the same through the loop, the loaders and the checkpoint files, at an epoch boundary.

Wall time on the MI355X, both files alone in one visit: this file 8.9 s (16 tests), its slowest test 1.2 s (adam-eager, the first
to build a model); tests/test_hip_step_graph.py 64.7 s (14 tests).  Being the cheaper one, it keeps run C in every graph case."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, M, P = 4, 5, 16


def _vnet(dropout=0.0, opt="Adam", compute="fp32", cin=1, K=2, loss="sorensen", nch=8, narrow=False):
    net = {"Name": "VNet", "Dropout": dropout, "NumChannel": nch, "NumLevels": 3, "NumConvolutions": [1, 2, 2], "BottomConvolutions": 2}
    if narrow:               # (the network of tests/test_hip_train_loop.py: the TF container's CRC-32C is pure Python)
        net = {"Name": "VNet", "Dropout": dropout, "NumChannel": 4, "NumLevels": 2, "NumConvolutions": [1, 2], "BottomConvolutions": 1}
    return {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": "synthetic", "TestingDataDirectory": "synthetic",
                 "ImageFilenames": ["image%d.npy" % i for i in range(cin)], "LabelFilename": "label.npy", "Synthetic": {"Cases": 4}},
        "SegmentationClasses": list(range(K)), "BatchSize": 2, "PatchShape": [P] * 3, "ComputeDtype": compute,
        "Networks": net,
        "Loss": {"Name": loss, "Weights": [0.3, 0.7, 1.0, 0.5, 0.2][:K], "Alpha": 0.5},
        "Optimizer": {"Name": opt, "InitialLearningRate": 1e-2, "Momentum": 0.9, "Decay": {"Factor": 0.9, "Steps": 3}}}}


def _unet():
    from tests.test_hip_unet import _cfg
    return _cfg(dropout=0.05)              # Adam, Decay 0.9 / 3 steps, sorensen, 1 modality, 2 classes


# id -> (config, step graph, container, forced f32x3)
CASES = {
    "adam-eager": (lambda: _vnet(), False, "torch", False),
    "adam-graph-dropout": (lambda: _vnet(dropout=0.05), True, "torch", False),
    "momentum-graph": (lambda: _vnet(opt="Momentum"), True, "torch", False),
    "nesterov-mixed-eager": (lambda: _vnet(dropout=0.05, opt="NesterovMomentum", loss="mixed_weighted_jaccard", cin=2, K=3), False, "torch", False),
    "sgd-bf16-graph": (lambda: _vnet(opt="SGD", compute="bf16", cin=4, K=5), True, "torch", False),
    "adam-bf16-graph-dropout": (lambda: _vnet(dropout=0.05, compute="bf16", cin=4, K=5), True, "torch", False),
    "adam-x3-forced-graph": (lambda: _vnet(nch=16, compute="fp32_split3"), True, "torch", True),
    "unet-adam-graph": (_unet, True, "torch", False),
    "adam-tf": (lambda: _vnet(dropout=0.05, narrow=True), True, "tf", False),
    "momentum-tf": (lambda: _vnet(opt="Momentum", narrow=True), False, "tf", False),
}


@contextlib.contextmanager
def _mode(case, monkeypatch):
    """The step path of the case (read by the model on every step) and, for fp32_split3, the f32x3 kernels on every 5^3 layer."""
    from tests.util import split3
    _, graph, _, force = CASES[case]
    monkeypatch.setenv("VNET_STEP_GRAPH", "1" if graph else "0")
    with (split3(force=True) if force else contextlib.nullcontext()):
        yield


def _model(case, dev, seed):
    from vnet_tensorflow_amd.model import image2label
    np.random.seed(seed)
    m = image2label(None, CASES[case][0](), device=dev, verbose=False)
    m.read_config()
    m.build_model_graph()
    m._setup_training()
    return m


def _batches(case, dev):
    from oracle.vnet_oracle import synthetic_batch
    T = CASES[case][0]()["TrainingSetting"]
    cin, K = len(T["Data"]["ImageFilenames"]), len(T["SegmentationClasses"])
    out = [synthetic_batch(2, P, cin, K, seed=40 + i) for i in range(3)]
    return [(torch.from_numpy(x).to(dev), torch.from_numpy(l).to(dev)) for x, l in out]


def _steps(m, batches, n):
    """n training steps; the batch is chosen by the GLOBAL step, so a restored counter picks the batch the uninterrupted run had."""
    losses = []
    for _ in range(n):
        x, l = batches[m.global_step % 3]
        losses.append(float(m.train_step(x, l)))
    return losses


def _snapshot(m):
    torch.cuda.synchronize()
    return {"flat": m.flat.data.clone(),
            "net": {k: v.clone() for k, v in m.network.state_dict().items()},
            "opt": {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in m.optimizer.state_dict().items()},
            "global_step": m.global_step}


def _check_path(case, m):
    graph = CASES[case][1]
    assert m._graph_mode() == ("whole" if graph else "off")
    if graph:
        assert m._graphs is not None and len(m._graphs) == 1, "the step was never captured"


def _save(case, m, tmp):
    if CASES[case][2] == "tf":
        return m.save_tf_checkpoint(os.path.join(tmp, "tf", "checkpoint-%d" % m.global_step))
    m.ckpt_dir = os.path.join(tmp, "ckpt")
    m.save_checkpoint()
    return os.path.join(m.ckpt_dir, "checkpoint-%d" % m.global_step)


def _load(case, m, path, **kw):
    if CASES[case][2] == "tf":
        return m.load_tf_checkpoint(path, **kw)
    return m.load_checkpoint(path, **kw)


def _x3_ran(case, dev, monkeypatch):
    """One EAGER step of the configuration under ops.profile_start(): the f32x3 kernels are what it launches (a captured graph
    records nothing, so this runs apart from the steps compared bit for bit)."""
    from vnet_tensorflow_amd import ops
    from tests.util import x3_profile_check
    with monkeypatch.context() as mp:
        mp.setenv("VNET_STEP_GRAPH", "0")
        m = _model(case, dev, 7)
        x, l = _batches(case, dev)[0]
        ops.profile_start()
        try:
            m.train_step(x, l)
        finally:
            recs = ops.profile_stop()
        assert m._graph_mode() == "off"
    x3_profile_check(recs, forced=True)


class _Refs(dict):
    """case -> the uninterrupted run A (losses of its N + M steps, final state, the model itself) and the checkpoint model 1 wrote
    after N steps.  Computed once per case, shared by the case's test and its controls; only model A is ever stepped again (run C
    begins with a load), the recorded tensors are clones nobody writes."""

    def get_case(self, case, dev, monkeypatch, tmp_factory):
        if case not in self:               # (the caller is inside _mode(case))
            batches = _batches(case, dev)
            a = _model(case, dev, 7)
            losses = _steps(a, batches, N + M)
            _check_path(case, a)
            one = _model(case, dev, 7)
            first = _steps(one, batches, N)
            _check_path(case, one)                 # (graph: 2 eager steps, capture, a replay -- then the save)
            path = _save(case, one, str(tmp_factory.mktemp("resume")))
            assert first == losses[:N] and one.global_step == N
            self[case] = {"losses": losses, "state": _snapshot(a), "model": a, "ckpt": path, "batches": batches}
        return self[case]


@pytest.fixture(scope="module")
def refs():
    r = _Refs()
    yield r
    r.clear()


def _same(got, ref, what):
    assert got["global_step"] == ref["global_step"], what
    assert torch.equal(got["flat"], ref["flat"]), (what, "flat.data")
    assert list(got["net"]) == list(ref["net"])
    for k in ref["net"]:
        assert torch.equal(got["net"][k], ref["net"][k]), (what, k)
    assert list(got["opt"]) == list(ref["opt"])
    for k, v in ref["opt"].items():
        assert (torch.equal(got["opt"][k], v) if isinstance(v, torch.Tensor) else got["opt"][k] == v), (what, "optimizer", k)


@pytest.mark.parametrize("case", list(CASES))
def test_restored_run_continues_the_uninterrupted_one(dev, monkeypatch, tmp_path_factory, refs, case):
    """Runs B and C against A: the losses of steps N .. N+M-1, flat.data, every entry of network.state_dict() (moving statistics
    included) and of optimizer.state_dict(), global_step -- equal, bit for bit."""
    graph, force = CASES[case][1], CASES[case][3]
    with _mode(case, monkeypatch):
        if force:
            _x3_ran(case, dev, monkeypatch)
        ref = refs.get_case(case, dev, monkeypatch, tmp_path_factory)
        a, batches = ref["model"], ref["batches"]
        assert ref["losses"][-1] < ref["losses"][0], ref["losses"]                  # the run is also training
        # B: a fresh model whose own initial weights are others
        b = _model(case, dev, 1234)
        assert not torch.equal(b.flat.data, ref["state"]["flat"]) and b.global_step == 0
        ptrs = [p.data_ptr() for p in b.flat.params]
        _load(case, b, ref["ckpt"])
        assert b.global_step == N
        assert [p.data_ptr() for p in b.flat.params] == ptrs                        # written through the views, not re-pointed
        got = _steps(b, batches, M)
        _check_path(case, b)                                                        # (graph: warm-up, capture, replays)
        print("%s B: %s\n%s A: %s" % (case, got, case, ref["losses"][N:]))
        assert got == ref["losses"][N:], ("B", got, ref["losses"][N:])
        _same(_snapshot(b), ref["state"], "B")
        del b
        # C: the old model, rolled back in place (every graph case; the ones to keep if this file ever has to get cheaper are those
        # whose captured graph reads packed images: adam-graph-dropout, adam-bf16-graph-dropout, adam-x3-forced-graph, unet-adam-graph)
        if graph:
            assert a.global_step == N + M
            g = a._graphs[0]
            _load(case, a, ref["ckpt"])
            assert a.global_step == N
            got = _steps(a, batches, M)
            assert a._graphs is not None and a._graphs[0] is g, "the rolled-back model must replay the graph it holds"
            print("%s C: %s" % (case, got))
            assert got == ref["losses"][N:], ("C", got, ref["losses"][N:])
            _same(_snapshot(a), ref["state"], "C")


# ---- negative controls: the comparison above can fail --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["adam-eager", "momentum-graph"])
def test_control_load_without_the_optimizer_leaves_the_trajectory(dev, monkeypatch, tmp_path_factory, refs, case):
    """with_optimizer=False: the slots and t stay exactly what the fresh model had (zeros, t = 0), the variables and counters are
    loaded -- and the continued run is another run.  (SGD has no slots, so it is not here.)"""
    with _mode(case, monkeypatch):
        ref = refs.get_case(case, dev, monkeypatch, tmp_path_factory)
        b = _model(case, dev, 1234)
        fresh = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.optimizer.state_dict().items()}
        assert fresh and all((not v.any()) if isinstance(v, torch.Tensor) else v == 0 for v in fresh.values())
        _load(case, b, ref["ckpt"], with_optimizer=False)
        now = b.optimizer.state_dict()
        assert all((torch.equal(now[k], v) if isinstance(v, torch.Tensor) else now[k] == v) for k, v in fresh.items())
        assert b.global_step == N
        got = _steps(b, ref["batches"], M)
        assert got[0] == ref["losses"][N]           # (the first loss is formed before any slot is read ...)
        assert got[1:] != ref["losses"][N + 1:]     # ... the update behind it is not the uninterrupted run's
        assert not torch.equal(b.flat.data, ref["state"]["flat"])


@pytest.mark.parametrize("case", ["adam-bf16-graph-dropout", "adam-x3-forced-graph"])
def test_control_stale_packed_images_under_the_graph_show(dev, monkeypatch, tmp_path_factory, refs, case):
    """Run C with ops.repack_registered doing nothing during the load: the captured graph then reads the packed filters of step
    N + M (valid buffers, old contents), and the first loss after the load is not A's."""
    from vnet_tensorflow_amd import ops
    with _mode(case, monkeypatch):
        ref = refs.get_case(case, dev, monkeypatch, tmp_path_factory)
        a = ref["model"]
        if a.global_step != N + M:                     # (whatever ran before: bring A back to where run C finds it)
            _load(case, a, ref["ckpt"])
            _steps(a, ref["batches"], M)
        assert a.global_step == N + M and a._graphs is not None
        with monkeypatch.context() as mp:
            mp.setattr(ops, "repack_registered", lambda: None)
            _load(case, a, ref["ckpt"])
        stale = _steps(a, ref["batches"], 1)
        assert stale[0] != ref["losses"][N], (stale, ref["losses"][N])
        # leave model A as the other tests expect it: a proper load, M steps, A's state again
        _load(case, a, ref["ckpt"])
        assert _steps(a, ref["batches"], M) == ref["losses"][N:]
        _same(_snapshot(a), ref["state"], "C after the control")


def test_control_step_counter_set_back_by_one_shows(dev, monkeypatch, tmp_path_factory, refs):
    """adam-graph-dropout with global_step put to N - 1 by hand after the load: another batch index, another learning rate and
    other dropout masks -- the losses differ, so the masks and the learning rate follow the restored counter."""
    case = "adam-graph-dropout"
    with _mode(case, monkeypatch):
        ref = refs.get_case(case, dev, monkeypatch, tmp_path_factory)
        b = _model(case, dev, 1234)
        _load(case, b, ref["ckpt"])
        b.global_step = N - 1
        x, l = ref["batches"][N % 3]                   # the batch A had at step N: only the counter is wrong
        got = [float(b.train_step(x, l))]
        assert got[0] != ref["losses"][N], (got, ref["losses"][N])


# ---- train(): through the loop, the loaders and the checkpoint files -------------------------------------------------------------------
def _train_cfg(tmp, **over):
    cfg = _vnet(dropout=0.05, narrow=True)
    T = cfg["TrainingSetting"]
    T["Data"]["Synthetic"] = {"Cases": 4, "Shape": [20, 20, 20]}          # larger than the patch: the crop seeds matter
    T.update({"Restore": False, "LogDir": str(tmp / "log"), "CheckpointDir": str(tmp / "ckpt"), "Testing": False, "Epoches": 3,
              "MaxIterations": 100, "LogInterval": 1000, "LoaderThreads": 2})
    T.update(over)
    return cfg


def _train(cfg, dev, seed):
    from vnet_tensorflow_amd.model import image2label
    np.random.seed(seed)
    m = image2label(None, cfg, device=dev, verbose=False)
    lines = []
    m._print = lambda *a: lines.append(" ".join(str(v) for v in a))
    m.train()
    return m, [ln.split("Segmentation training loss: ")[1] for ln in lines if "Segmentation training loss: " in ln]


def test_train_restored_at_an_epoch_boundary_is_the_uninterrupted_run(dev, tmp_path, monkeypatch):
    """A: train() for 3 epochs.  B: train() for 2 epochs, then a new object with Restore: true and Epoches 3.  4 synthetic cases,
    batch 2, 16^3 crops of 20^3 volumes, dropout 0.05, 2 loader threads, the step graph at its default, checkpoints at epoch ends
    only.  The two checkpoint-6 files hold equal variables, Adam slots and t, global_step and start_epoch, bit for bit, and epoch 3
    printed the same losses.
    Testing is false: the test pass moves the moving averages (batch statistics are always used), and the position of its
    iterator is not part of a checkpoint, so with it a restored run is not the uninterrupted one.
    This is what the dataset's epoch rule is for: a training set that starts at epoch 0 after every restore replays epoch 0's
    shuffle and crop seeds, and this test fails at the first loss of epoch 3."""
    monkeypatch.delenv("VNET_STEP_GRAPH", raising=False)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    ma, la = _train(_train_cfg(tmp_path / "a"), dev, 7)
    assert ma.global_step == 6 and ma.start_epoch == 3 and len(la) == 6 and ma._graph_mode() == "whole" and ma._graphs is not None
    m1, l1 = _train(_train_cfg(tmp_path / "b", Epoches=2), dev, 7)
    assert m1.global_step == 4 and l1 == la[:4]
    m2, l2 = _train(_train_cfg(tmp_path / "b", Epoches=3, Restore=True), dev, 99)
    assert m2.global_step == 6 and m2.start_epoch == 3
    print("epoch 3, uninterrupted: %s\nepoch 3, restored:      %s" % (la[4:], l2))
    assert l2 == la[4:], (l2, la[4:])
    a = torch.load(tmp_path / "a" / "ckpt" / "checkpoint-6", weights_only=True)
    b = torch.load(tmp_path / "b" / "ckpt" / "checkpoint-6", weights_only=True)
    assert a["global_step"] == b["global_step"] == 6 and a["start_epoch"] == b["start_epoch"] == 3
    assert a["opt_names"] == b["opt_names"] and list(a["variables"]) == list(b["variables"])
    for k in a["variables"]:
        assert torch.equal(a["variables"][k], b["variables"][k]), k
    assert a["optimizer"]["t"] == b["optimizer"]["t"] == 6
    assert torch.equal(a["optimizer"]["m"], b["optimizer"]["m"]) and torch.equal(a["optimizer"]["v"], b["optimizer"]["v"])
