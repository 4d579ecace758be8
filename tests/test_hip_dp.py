"""-m gpu: the data-parallel step end to end on the HIP path.  The GPU box has one MI355X, so two ranks share
cuda:0 and exchange gradients over gloo (VNET_DIST_BACKEND=gloo) -- RCCL itself cannot be exercised with one
device, but everything around it is the production code: gradient sinks -> bucket countdown -> async
all-reduce launched from backward on the side stream -> 1/world scaling in the fused Adam kernel.
Checks SURVEY 8(e): all-reduced gradient == sum of the per-rank single-process gradients (per-replica BN),
replicas stay bit-identical, and the update equals single-process Adam on the mean gradient."""
import contextlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
NET = dict(K=2, C0=4, levels=2, ncv=(1, 2), nb=1, P=16)

# Every multi-rank test runs (a) over gloo with both ranks on cuda:0 -- always possible -- and (b) over RCCL (backend
# "nccl") with ONE RANK PER DEVICE whenever the box has at least two GPUs (skipped, and reported as skipped, otherwise):
# rank r's loss == the single-GPU B=1 run of its patch, reduced gradient == sum of the per-rank gradients, replicas stay
# bit-identical after Adam, sync-BN == single-device batch of N.
BACKENDS = [pytest.param("gloo", id="gloo-2-ranks-on-one-gpu"),
            pytest.param("nccl", id="rccl-one-rank-per-gpu",
                         marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs (RCCL between devices)"))]


def _rank_env(rank, world, port, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank if backend == "nccl" else 0), VNET_DIST_BACKEND=backend)
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    return dev


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(dev, seed):
    from vnet_tensorflow_amd import networks, ops
    np.random.seed(seed)
    compute = os.environ.get("VNET_TEST_COMPUTE", "fp32")      # "bf16": bf16 tensors end to end (needs 8 * 2^k channels)
    ops.set_compute_dtype(compute)
    C0 = {"bf16": 8, "fp32_split3": 16}.get(compute, NET["C0"])     # (fp32_split3: whole 16-channel blocks, the f32x3 kernels' unit)
    net = networks.VNet(NET["K"], 0.0, C0, NET["levels"], NET["ncv"], NET["nb"], True, "prelu", device=dev)
    net.build((1, NET["P"], NET["P"], NET["P"], 1))
    return net


def _batch(rank, dev):
    from oracle.vnet_oracle import synthetic_batch
    x, lab = synthetic_batch(1, NET["P"], 1, NET["K"], seed=500 + rank)
    return torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)


def _sync_bn_worker(rank, world, port, out, backend="gloo"):
    """Cross-replica batch-norm: one patch per rank, statistics over both."""
    dev = _rank_env(rank, world, port, backend)
    import torch.distributed as dist
    from vnet_tensorflow_amd import ops, optim, parallel
    parallel.init_from_env()
    assert dist.get_backend() == backend and dist.get_world_size() == world
    ops.set_sync_batch_norm()
    net = _build(dev, seed=100)                        # same seed: identical replicas
    flat = optim.FlatParams(net.named_parameters())
    sync = parallel.BucketedGradAllReduce(flat, bucket_bytes=16 << 10)
    x, lab = _batch(rank, dev)
    for step in range(2):
        flat.zero_grad()
        sync.begin_step()
        logits = net.GetNetwork(x)
        loss, _, _, _ = ops.softmax_loss(logits, lab, "sorensen")
        loss.backward()
        sync.finish()
        torch.cuda.synchronize()
    mm = dict(net.named_buffers()) if hasattr(net, "named_buffers") else {}
    torch.save({"gsum": flat.grad.cpu(), "logits": logits.detach().cpu(), "loss": float(loss.detach()),
                "moving": {k: v.cpu() for k, v in mm.items()}}, os.path.join(out, "s%d.pt" % rank))
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", BACKENDS)
def test_sync_batch_norm_equals_single_device_batch(tmp_path, dev, backend):
    """2 ranks x 1 patch with cross-replica statistics == the single-device BatchSize=2 step of the reference
    (networks.py:319 reduces the batch axis too): same logits per patch, loss = mean, gradient sum = 2 x."""
    from vnet_tensorflow_amd import ops, optim
    mp.spawn(_sync_bn_worker, args=(2, _free_port(), str(tmp_path), backend), nprocs=2, join=True)
    r = [torch.load(tmp_path / ("s%d.pt" % k)) for k in range(2)]
    assert torch.equal(r[0]["gsum"], r[1]["gsum"])
    net = _build(dev, seed=100)
    flat = optim.FlatParams(net.named_parameters())
    xs, labs = zip(*[_batch(k, dev) for k in range(2)])
    x, lab = torch.cat(xs), torch.cat(labs)
    flat.zero_grad()
    logits = net.GetNetwork(x)
    loss, _, _, _ = ops.softmax_loss(logits, lab, "sorensen")
    loss.backward()
    torch.cuda.synchronize()
    for k in range(2):
        assert float((logits[k:k + 1].detach().cpu() - r[k]["logits"]).abs().max()) < 1e-4
    assert abs(float(loss.detach()) - 0.5 * (r[0]["loss"] + r[1]["loss"])) < 1e-6
    ref = 2.0 * flat.grad.cpu()
    err = float((r[0]["gsum"] - ref).norm() / ref.norm())
    assert err < 1e-4, err
    # and it is NOT what per-replica statistics give (the two modes differ measurably on this input)
    net1 = _build(dev, seed=100)
    l0 = net1.GetNetwork(xs[0]).detach().cpu()
    assert float((l0 - r[0]["logits"]).abs().max()) > 1e-3


def _worker(rank, world, port, out, backend="gloo"):
    dev = _rank_env(rank, world, port, backend)
    import torch.distributed as dist
    from vnet_tensorflow_amd import ops, optim, parallel
    from tests.util import split3, x3_profile_check
    x3 = os.environ.get("VNET_TEST_COMPUTE") == "fp32_split3"
    keep = contextlib.ExitStack()
    if x3:
        keep.enter_context(split3(force=True))   # every 5^3 layer on the f32x3 kernels: a spawned worker does not inherit ops._X3
    parallel.init_from_env()
    assert dist.get_backend() == backend and dist.get_world_size() == world
    net = _build(dev, seed=100 + rank)                 # replicas start different ...
    flat = optim.FlatParams(net.named_parameters())
    parallel.broadcast_parameters(flat.data)           # ... rank 0's weights win
    ops.invalidate_packed()
    opt = optim.AdamOptimizer(flat)
    opt.gscale = 1.0 / world
    ops.set_param_grad_stream(os.environ.get("VNET_TEST_PG", "1") == "1")   # filter/bias gradients on their own stream, as in model.train_step
    ops._PG["test_delay"] = 200000 * rank            # rank 1's side stream lags ~0.1 ms per layer: bucket/stream ordering holes show
    sync = parallel.BucketedGradAllReduce(flat, bucket_bytes=16 << 10, comm_dtype=os.environ.get("VNET_TEST_COMM", "fp32"))
    assert len(sync.buckets) >= 3 and sync.overlap
    x, lab = _batch(rank, dev)
    for step in range(2):                              # step 0 calibrates the event counts, step 1 overlaps
        flat.zero_grad()
        sync.begin_step()
        if x3 and step == 0:
            ops.profile_start()
        loss, _, _, _ = ops.softmax_loss(net.GetNetwork(x), lab, "sorensen")
        loss.backward()
        if step == 1:
            assert sum(sync._launched) >= len(sync.buckets) - 1      # buckets went out DURING backward
        sync.finish()
        ops.join_param_grad_stream()
        if x3 and step == 0:
            x3_profile_check(ops.profile_stop(), forced=True)      # the gradients the hooks exchanged came from the f32x3 kernels
        torch.cuda.synchronize()
        gsum = flat.grad.clone()
        opt.apply(1e-2)
    torch.cuda.synchronize()
    torch.save({"gsum": gsum.cpu(), "data": flat.data.cpu(), "loss": float(loss.detach())}, os.path.join(out, "r%d.pt" % rank))
    dist.destroy_process_group()
    keep.close()


@pytest.mark.parametrize("compute", ["fp32", "bf16", "bf16+bf16comm", "fp32_split3"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_two_ranks(tmp_path, dev, backend, compute, monkeypatch):
    from vnet_tensorflow_amd import ops, optim
    from tests.util import split3
    comm16 = compute.endswith("bf16comm")                  # round 6: GradCommDtype "bf16" -- bf16 buckets on the links, fp32 accumulation on receipt
    compute = compute.split("+")[0]
    monkeypatch.setenv("VNET_TEST_COMPUTE", compute)       # (bf16: bf16 storage -- the per-GPU arithmetic of BASELINE config C5)
    if compute == "bf16":
        monkeypatch.setenv("VNET_TEST_PG", "0")            # as the product step: no side stream, gradients accumulate in the epilogues
    if comm16:
        monkeypatch.setenv("VNET_TEST_COMM", "bf16")
    # (bf16 buckets: the single-process reference applies the SAME exchange arithmetic to its per-rank gradients -- RNE to bf16 per
    #  rank, fp32 sum in rank order, one rounding -- so the tolerances stay those of the bf16 mode.  Against the fp32 sum the second
    #  step would differ by ~1e-2: Adam's first step moves every parameter by ~lr x sign(g), and the rounding flips signs of the
    #  near-zero gradients.)
    tol = (1e-5, 1e-4, 1e-5) if compute in ("fp32", "fp32_split3") else (2e-4, 2e-3, 2e-4)
    try:
        with (split3(force=True) if compute == "fp32_split3" else contextlib.nullcontext()):     # (the single-process reference too)
            _two_ranks(tmp_path, dev, backend, tol=tol, comm16=comm16)
    finally:
        ops.set_compute_dtype("fp32")


def _two_ranks(tmp_path, dev, backend, tol, comm16=False):
    from vnet_tensorflow_amd import ops, optim
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), backend), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert torch.equal(r0["gsum"], r1["gsum"]) and torch.equal(r0["data"], r1["data"])     # replicas identical
    # single-process reference: per-rank gradients from rank 0's initial weights, summed
    net = _build(dev, seed=100)
    flat = optim.FlatParams(net.named_parameters())
    opt = optim.AdamOptimizer(flat)
    opt.gscale = 0.5
    for step in range(2):
        tot = torch.zeros_like(flat.grad)
        for rank in range(2):
            x, lab = _batch(rank, dev)
            flat.zero_grad()
            loss, _, _, _ = ops.softmax_loss(net.GetNetwork(x), lab, "sorensen")
            loss.backward()
            if step == 1:
                assert abs(float(loss.detach()) - (r0, r1)[rank]["loss"]) < tol[0]      # per-replica BN: same loss as B=1 alone
            tot += flat.grad.to(torch.bfloat16).to(torch.float32) if comm16 else flat.grad
        if comm16:
            tot = tot.to(torch.bfloat16).to(torch.float32)       # parallel.BucketedGradAllReduce(comm_dtype="bf16"): one rounding of the fp32 sum
        flat.grad.copy_(tot)
        opt.apply(1e-2)               # single-process TF-Adam on the mean gradient
    ref = tot.cpu()
    err = float((r0["gsum"] - ref).norm() / ref.norm())
    assert err < tol[1], err
    assert float((flat.data.cpu() - r0["data"]).abs().max()) < tol[2]


def _rccl_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as dist
    from vnet_tensorflow_amd import ops, optim, parallel
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)       # backend "nccl" IS RCCL on ROCm
    net = _build(dev, seed=100)
    flat = optim.FlatParams(net.named_parameters())
    parallel.broadcast_parameters(flat.data)
    ops.set_param_grad_stream(True)
    sync = parallel.BucketedGradAllReduce(flat, bucket_bytes=16 << 10, force=True)
    assert sync.active and sync.overlap and len(sync.buckets) >= 3
    x, lab = _batch(0, dev)
    for step in range(3):
        flat.zero_grad()
        sync.begin_step()
        loss, _, _, _ = ops.softmax_loss(net.GetNetwork(x), lab, "sorensen")
        loss.backward()
        if step >= 1:
            assert sum(sync._launched) >= len(sync.buckets) - 1
        sync.finish()
        ops.join_param_grad_stream()
    torch.cuda.synchronize()
    t = torch.ones(8, device=dev)
    dist.all_reduce(t)
    dist.barrier()
    torch.save({"gsum": flat.grad.cpu(), "loss": float(loss.detach()), "t": t.cpu()}, os.path.join(out, "rccl.pt"))
    dist.destroy_process_group()


def test_rccl_group_of_one(tmp_path, dev):
    """RCCL itself (process group "nccl", device-bound, async all-reduce of every bucket on the side stream while the
    backward kernels run) in a group of ONE rank -- all a 1-GPU box can host: the reduced gradient must be the plain
    single-process gradient."""
    from vnet_tensorflow_amd import ops, optim
    mp.spawn(_rccl_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / "rccl.pt")
    net = _build(dev, seed=100)
    flat = optim.FlatParams(net.named_parameters())
    x, lab = _batch(0, dev)
    flat.zero_grad()
    loss, _, _, _ = ops.softmax_loss(net.GetNetwork(x), lab, "sorensen")
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - r["loss"]) < 1e-6
    assert torch.equal(r["gsum"], flat.grad.cpu())              # same kernels, same order: bit-identical
    assert torch.equal(r["t"], torch.ones(8))


@pytest.fixture(scope="module")
def bench_two_ranks():
    """ONE run of `python bench.py --gpus 2` with no launcher (the way the driver runs the N = 1 bench; round 5: the two tests below
    shared nothing and each paid ~60-100 s of process start-up, graph capture and data-parallel autotune).  The parent starts
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 ... bench.py --gpus 2 ...` as a child --
    the driver's own N > 1 command line -- so that the inner run IS the driver-launched path."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["VNET_DIST_BACKEND"] = "gloo"
    env["VNET_DP_AUTOTUNE_STEPS"] = "1"       # (every step all-reduces 176 MB through the host here: 9 tuning steps instead of 45)
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "2", "--patch", "32"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), cmd, root, env


def test_bench_contract_two_ranks(bench_two_ranks):
    """bench.py with one rank per "GPU" under torch.distributed.run -- here two ranks share the single device over gloo: barrier +
    max-over-ranks timing, rank 0 prints ONE JSON line whose value is the whole-job rate."""
    out = bench_two_ranks[0]
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 2 and out["scaling"] == "weak"
    assert out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 2
    assert out["config"]["ranks"] == 2 and out["config"]["backend"] == "gloo"          # the process group really has N ranks
    assert out["step_enqueue"].startswith(("hipGraph(gradients)", "eager")) and sorted(out["dp_autotune_ms"]) == ["off", "segmented", "serial"]
    assert abs(out["value"] - 2 * 1 * 1000.0 / out["ms_per_step"]) < 1e-2 * out["value"]
    assert out["roofline"] is None or out["roofline"]["frac"] > 0
    assert "cpu_baseline" not in out                     # rank 0 at N=1 only


def test_bench_starts_its_own_ranks(bench_two_ranks):
    """`python bench.py --gpus 2` with NO launcher: the parent must start two ranks itself (a child torch.distributed.run; it never
    touches the GPU and execs nothing) and relay rank 0's single JSON line.  With fewer devices than ranks and no test hook it
    must refuse."""
    import subprocess
    out, cmd, root, env = bench_two_ranks
    assert out["n_gpus"] == 2 and out["config"]["ranks"] == 2 and out["config"]["backend"] == "gloo"
    if torch.cuda.device_count() < 2:
        env = dict(env)
        env.pop("VNET_DIST_BACKEND")
        r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "device(s) visible" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]
