"""CPU: the host side of "a restored run continues the uninterrupted one" (tests/test_hip_resume.py holds the device side).
The dataset's epoch rule -- the plan of epoch e is the same whether or not the run was restored (data.VolumeDataset(epoch=) /
skip_epochs) --, train() handing start_epoch to the training set, and a torch-container checkpoint that lacks a variable."""
import numpy as np
import pytest
import torch

from vnet_tensorflow_amd import data

CASES, BATCH, EPOCHS = 12, 2, 4


def _dataset(train=True, rank=0, world=1, **kw):
    return data.VolumeDataset("synthetic", ["image.npy"], "label.npy", [0, 1], (8, 8, 8), BATCH, train=train, seed=3,
                              synthetic={"Cases": CASES, "Shape": [12, 12, 12]}, rank=rank, world=world, **kw)


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1)])
def test_plan_of_epoch_e_does_not_depend_on_where_the_dataset_started(world, rank):
    """epoch_plan() of a dataset advanced to epoch e == the e-th plan of a fresh dataset, e = 0 .. 3: cases and crop seeds, exactly;
    through the constructor argument and through skip_epochs, in one stride and one epoch at a time."""
    fresh = _dataset(rank=rank, world=world)
    plans = [fresh.epoch_plan() for _ in range(EPOCHS + 1)]
    assert all(len(p) == CASES // (world * BATCH) for p in plans)
    # the sequence is worth comparing: no two epochs share an order or a crop seed
    assert len(set(tuple(c for cs, _ in p for c in cs) for p in plans)) > 1
    seeds = [s for p in plans for _, ss in p for s in ss]
    assert len(set(seeds)) == len(seeds)
    for e in range(EPOCHS):
        by_arg = _dataset(rank=rank, world=world, epoch=e)
        by_call = _dataset(rank=rank, world=world)
        by_call.skip_epochs(e)
        by_steps = _dataset(rank=rank, world=world)
        for _ in range(e):
            by_steps.skip_epochs(1)
        for name, d in (("epoch=", by_arg), ("skip_epochs(e)", by_call), ("skip_epochs(1) x e", by_steps)):
            assert d.epoch == e, (name, e)
            got = d.epoch_plan()
            assert got == plans[e], (name, e, got, plans[e])
            assert d.epoch_plan() == plans[e + 1], (name, e)             # ... and it goes on like the uninterrupted one
    if world == 2:
        # (the two ranks' shards of an epoch stay disjoint and share the shuffle, wherever the datasets started)
        a, b = _dataset(rank=0, world=2, epoch=2).epoch_plan(), _dataset(rank=1, world=2, epoch=2).epoch_plan()
        ca, cb = [c for cs, _ in a for c in cs], [c for cs, _ in b for c in cs]
        assert not set(ca) & set(cb) and len(ca) == len(cb) == CASES // 2


def test_batches_of_a_restored_epoch_are_the_uninterrupted_ones():
    """One level down from the plan: the arrays of epoch 2, image and label, byte for byte."""
    fresh = _dataset()
    for _ in range(2):
        fresh.epoch_plan()
    ref, got = list(fresh), list(_dataset(epoch=2))
    assert len(ref) == len(got) == CASES // BATCH
    for (ri, rl), (gi, gl) in zip(ref, got):
        assert ri.tobytes() == gi.tobytes() and rl.tobytes() == gl.tobytes()
    first = list(_dataset())
    assert any(a[0].tobytes() != b[0].tobytes() for a, b in zip(first, ref))       # (epoch 0 is another epoch)


def _train_config(tmp, **over):
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": "synthetic", "TestingDataDirectory": "synthetic", "ImageFilenames": ["image.npy"],
                 "LabelFilename": "label.npy", "Synthetic": {"Cases": 6, "Shape": [12, 12, 12]}},
        "Restore": False, "SegmentationClasses": [0, 1], "LogDir": str(tmp / "log"), "CheckpointDir": str(tmp / "ckpt"),
        "BatchSize": 2, "PatchShape": [8, 8, 8], "Testing": False, "Epoches": 2, "MaxIterations": 4, "LogInterval": 5,
        "LoaderThreads": 2,
        "Networks": {"Name": "VNet", "Dropout": 0.01, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 2], "BottomConvolutions": 1},
        "Loss": {"Name": "sorensen", "Weights": [], "Alpha": 1},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}}}}
    cfg["TrainingSetting"].update(over)
    return cfg


def _stand_in_model(cfg, seen, sets):
    """image2label on the CPU whose train_step only counts the step and keeps the batch it was given (the kernels need a GPU; the loop,
    the checkpoints and the loaders do not), and whose datasets are kept for inspection."""
    from vnet_tensorflow_amd.model import image2label
    m = image2label(None, cfg, device="cpu", verbose=False)

    def train_step(images, labels, dropout=None):
        seen.append((m.global_step, images.clone().numpy(), labels.clone().numpy()))
        m.global_step += 1
        return torch.zeros(())
    make = m._dataset

    def dataset(*a, **kw):
        d = make(*a, **kw)
        sets.append(d)
        return d
    m.train_step, m._dataset = train_step, dataset
    return m


def test_train_restored_from_a_mid_epoch_checkpoint_starts_that_epochs_plan(tmp_path):
    """6 cases, batch 2: 3 steps per epoch.  The first run stops by MaxIterations after step 5, whose checkpoint (LogInterval 5) was
    written in the middle of epoch 1 (start_epoch 1, global_step 5).  The restored run starts epoch 1 again from its first batch, like
    the reference -- and that is the first batch of EPOCH 1's plan, the one the first run saw at its step 3, not epoch 0's."""
    import os
    seen, sets = [], []
    _stand_in_model(_train_config(tmp_path), seen, sets).train()
    assert [s for s, _, _ in seen] == [0, 1, 2, 3, 4]
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["checkpoint-3", "checkpoint-5", "checkpoint-latest"]
    ck = torch.load(tmp_path / "ckpt" / "checkpoint-5", weights_only=True)
    assert ck["global_step"] == 5 and ck["start_epoch"] == 1

    again, sets2 = [], []
    m = _stand_in_model(_train_config(tmp_path, Restore=True, MaxIterations=100), again, sets2)
    m.train()
    assert [s for s, _, _ in again] == [5, 6, 7] and m.start_epoch == 2 and m.global_step == 8
    assert len(sets2) == 1 and sets2[0].train and sets2[0].epoch == 2            # (started at 1, planned one epoch)
    # the plans of a dataset nobody restored
    fresh = data.VolumeDataset("synthetic", ["image.npy"], "label.npy", [0, 1], (8, 8, 8), 2, train=True,
                               synthetic={"Cases": 6, "Shape": [12, 12, 12]})
    epoch0, epoch1 = list(fresh), list(fresh)
    for (_, gi, gl), (ri, rl) in zip(again, epoch1):
        assert gi.tobytes() == ri.tobytes() and gl.tobytes() == rl.tobytes()
    assert again[0][1].tobytes() == seen[3][1].tobytes() and again[0][2].tobytes() == seen[3][2].tobytes()
    assert again[0][1].tobytes() != epoch0[0][0].tobytes()
    # the test set is built as before: a restored run's starts at its first plan
    t = m._dataset(m.test_data_dir, False)
    assert not t.train and t.epoch == 0
    ref = data.VolumeDataset("synthetic", ["image.npy"], "label.npy", [0, 1], (8, 8, 8), 2, train=False,
                             synthetic={"Cases": 6, "Shape": [12, 12, 12]})
    assert t.epoch_plan() == ref.epoch_plan()


def test_test_set_is_unaffected():
    """train=False: no shuffle, every case, and the same plans as before -- the constructor's default adds no draw."""
    t = _dataset(train=False)
    assert t.epoch == 0
    rng = np.random.default_rng(3)
    for e in range(3):
        plan = t.epoch_plan()
        assert [c for cs, _ in plan for c in cs] == list(range(CASES))
        assert [s for _, ss in plan for s in ss] == [int(v) for _ in range(CASES // BATCH) for v in rng.integers(0, 2 ** 62, size=BATCH)]


def test_torch_checkpoint_that_lacks_a_variable_is_refused(tmp_path):
    """Both containers refuse a checkpoint without one of the network's variables, naming it, before anything is written: the model
    keeps every value, its counters and its optimiser slots."""
    from vnet_tensorflow_amd.model import image2label
    cfg = _train_config(tmp_path)
    np.random.seed(1)
    a = image2label(None, cfg, device="cpu", verbose=False)
    a.read_config(); a.build_model_graph(); a._setup_training()
    with torch.no_grad():
        a.optimizer.m.normal_(); a.optimizer.v.uniform_(); a.optimizer.t = 9
    a.global_step, a.start_epoch = 9, 3
    a.save_checkpoint()
    path = str(tmp_path / "ckpt" / "checkpoint-9")
    np.random.seed(2)
    b = image2label(None, cfg, device="cpu", verbose=False)
    b.read_config(); b.build_model_graph(); b._setup_training()
    before = {k: v.clone() for k, v in b.network.state_dict().items()}
    assert any(not torch.equal(v, a.network.state_dict()[k]) for k, v in before.items())
    for gone in ("vnet/output_layer/weights", "vnet/input_layer/batch_normalization/moving_mean"):
        ck = torch.load(path, weights_only=True)
        assert gone in ck["variables"]
        del ck["variables"][gone]
        torch.save(ck, path + "-short")
        with pytest.raises(KeyError, match=gone):
            b.load_checkpoint(path + "-short")
        assert all(torch.equal(v, before[k]) for k, v in b.network.state_dict().items())
        assert b.global_step == 0 and b.start_epoch == 0 and b.optimizer.t == 0 and not b.optimizer.m.any()
    # the reference's container, same file content: the same refusal
    from vnet_tensorflow_amd import tf_checkpoint as tfc
    prefix = a.save_tf_checkpoint(str(tmp_path / "tfck" / "checkpoint-9"))
    tensors = tfc.read(prefix)
    del tensors["vnet/output_layer/weights"]
    tfc.write(prefix + "-short", tensors)
    with pytest.raises(KeyError, match="vnet/output_layer/weights"):
        b.load_tf_checkpoint(prefix + "-short")
    assert all(torch.equal(v, before[k]) for k, v in b.network.state_dict().items()) and b.global_step == 0
    # and an unknown variable is refused before anything is written, too
    ck = torch.load(path, weights_only=True)
    ck["variables"]["vnet/nowhere/weights"] = torch.zeros(3)
    torch.save(ck, path + "-long")
    with pytest.raises(KeyError, match="vnet/nowhere/weights"):
        b.load_checkpoint(path + "-long")
    assert all(torch.equal(v, before[k]) for k, v in b.network.state_dict().items())
    # the whole file still loads
    b.load_checkpoint(path)
    assert all(torch.equal(v, a.network.state_dict()[k]) for k, v in b.network.state_dict().items())
    assert b.global_step == 9 and b.start_epoch == 3 and b.optimizer.t == 9 and torch.equal(b.optimizer.m, a.optimizer.m)
