"""CPU, world_size 2 (gloo): the bucketed gradient reducer averages gradients like DDP,
tolerates parameters that never get a gradient, and skips sync under no_sync()."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from task_support import _free_port


def _worker(rank, world, port, q, algo):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from speech2text_amd.ddp import GradReducer, broadcast_parameters
    from speech2text_amd.flat import FlatStore
    torch.manual_seed(100 + rank)                       # different init per rank on purpose
    net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16),
                              torch.nn.Tanh(), torch.nn.Linear(16, 3))
    unused = torch.nn.Parameter(torch.ones(5))
    params = list(net.parameters()) + [unused]
    store = FlatStore(params)
    broadcast_parameters(store)                         # rank 0's weights everywhere
    red = GradReducer(store, bucket_bytes=4 * 200, algo=algo)      # several small buckets
    g = torch.Generator().manual_seed(7)
    xs = torch.randn(4, 8, 6, generator=g)
    ys = torch.randn(4, 8, 3, generator=g)
    outs = []
    for step in range(3):
        store.zero_grad()
        # accumulation micro-step without sync, then a synced one
        with red.no_sync():
            ((net(xs[rank]) - ys[rank]) ** 2).mean().backward()
        red.prepare()
        ((net(xs[2 + rank]) - ys[2 + rank]) ** 2).mean().backward()
        red.finish()
        outs.append([p.grad.clone() for p in params])
    # single-process oracle: accumulate both micro-batches, average over the two ranks
    ref = []
    with red.no_sync():                                 # the reducer's hooks stay registered
        for r in range(world):
            for p in net.parameters():
                p.grad = None
            ((net(xs[r]) - ys[r]) ** 2).mean().backward()
            first = [p.grad.clone() for p in net.parameters()]
            for p in net.parameters():
                p.grad = None
            ((net(xs[2 + r]) - ys[2 + r]) ** 2).mean().backward()
            ref.append((first, [p.grad.clone() for p in net.parameters()]))
    # expected on rank: own first micro-batch grad (unsynced) is part of the buffer that gets
    # all-reduced, so result = mean over ranks of (first + second)
    exp = [sum(ref[r][0][i] + ref[r][1][i] for r in range(world)) / world
           for i in range(len(ref[0][0]))]
    exp.append(torch.zeros(5))
    ok = all(all(torch.allclose(a, e, atol=1e-6) for a, e in zip(o, exp)) for o in outs)
    # every tensor of the store starts on a 16-byte boundary; the padding stays zero
    ok = ok and all(o % 4 == 0 for o in store.offsets) and float(store.flat_g.abs().sum()) > 0
    q.put((rank, ok, len(red.buckets), sorted(red._expected) == list(range(len(params) - 1))))
    dist.destroy_process_group()


import pytest


@pytest.mark.parametrize("algo", ["allreduce", "rs_ag"])
def test_grad_reducer_world2_gloo(algo):
    """Both exchange forms: in-place all-reduce, and reduce-scatter + shard divide + all-gather."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, algo)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=90) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, ok, nb, learned in res:
        assert ok, f"rank {rank}: gradients differ from the 2-replica average"
        assert nb >= 3
        assert learned, "unused parameter should be excluded from the expected set"


def _late_worker(rank, world, port, q):
    """A parameter that starts to receive gradients at step 2, on rank 0 only, and whose
    gradient arrives after its bucket was launched."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from speech2text_amd.ddp import GradReducer, broadcast_parameters
    from speech2text_amd.flat import FlatStore
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16),
                              torch.nn.Tanh(), torch.nn.Linear(16, 3))
    gate = torch.nn.Parameter(torch.ones(6))            # last in the store -> first bucket
    params = list(net.parameters()) + [gate]
    store = FlatStore(params)
    broadcast_parameters(store)
    red = GradReducer(store, bucket_bytes=4 * 120)
    g = torch.Generator().manual_seed(11)
    xs = torch.randn(2, 8, 6, generator=g)
    ys = torch.randn(2, 8, 3, generator=g)

    def loss_fn(r, use_gate):
        x = xs[r] * gate if use_gate else xs[r]         # used FIRST in forward: gradient comes last
        return ((net(x) - ys[r]) ** 2).mean()

    norms, gate_grads = [], []
    for step in range(5):
        store.zero_grad()
        red.prepare()
        loss_fn(rank, step >= 2 and rank == 0).backward()
        red.finish()
        norms.append(float(store.flat_g.abs().sum()))
        gate_grads.append(gate.grad.clone())
    dropped = red.poll_dropped()
    # oracle for the steps after the drop: plain average of the two ranks' gradients
    with red.no_sync():
        ref = []
        for r in range(world):
            store.zero_grad()
            loss_fn(r, r == 0).backward()
            ref.append(store.flat_g.clone())
        store.zero_grad()
        red.prepare()
        loss_fn(rank, rank == 0).backward()
    exp = (ref[0] + ref[1]) / world
    # redo the last step synchronised and compare with the oracle
    store.zero_grad()
    red.prepare()
    loss_fn(rank, rank == 0).backward()
    red.finish()
    ok_last = torch.allclose(store.flat_g, exp, atol=1e-6)
    q.put((rank, norms, dropped, ok_last, float(gate_grads[4].abs().sum())))
    dist.destroy_process_group()


def test_late_parameter_does_not_hang_or_raise():
    """a parameter that begins to fire late must neither raise on one rank (hang) nor
    corrupt the step: all ranks zero that step's gradient, then wait for it from then on."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_late_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=90) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, norms, dropped, ok_last, gate_abs in res:
        assert norms[0] > 0 and norms[1] > 0
        assert norms[2] == 0.0, f"rank {rank}: the step with the late gradient must be zeroed"
        assert norms[3] > 0 and norms[4] > 0
        assert dropped == 1, (rank, dropped)
        assert ok_last, f"rank {rank}: gradients after the drop differ from the 2-rank average"
        assert gate_abs > 0, "the late parameter's gradient is averaged from then on (rank 1 too)"


def _late4_worker(rank, world, port, q):
    """World 4, two parameters that begin to fire late on DIFFERENT ranks at DIFFERENT steps; the
    late rank's gradient buffer also holds a NaN (the late write races with the collective already
    in flight): every rank must zero that step's gradient (NaN included), the optimizer step of a
    dropped step must leave parameters and optimizer state alone, and later steps must be the
    4-rank average."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from speech2text_amd.ddp import GradReducer, broadcast_parameters
    from speech2text_amd.flat import FlatStore
    from speech2text_amd.optimizer.scaled_adam import ScaledAdam
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16),
                              torch.nn.Tanh(), torch.nn.Linear(16, 3))
    gate_a = torch.nn.Parameter(torch.ones(6))          # last in the store -> first bucket
    gate_b = torch.nn.Parameter(torch.ones(6))
    params = list(net.parameters()) + [gate_b, gate_a]
    opt = ScaledAdam(params, lr=0.02, clipping_scale=None)
    opt.zero_grad_in_step = True
    store = opt.store if getattr(opt, "store", None) is not None else FlatStore(params)
    broadcast_parameters(store)
    red = GradReducer(store, bucket_bytes=4 * 100)
    g = torch.Generator().manual_seed(13)
    xs = torch.randn(world, 8, 6, generator=g)
    ys = torch.randn(world, 8, 3, generator=g)

    def loss_fn(r, step):
        x = xs[r]
        if step >= 2 and r == 1:
            x = x * gate_a                               # used first in forward: gradient comes last
        if step >= 4 and r == 3:
            x = x * gate_b
        return ((net(x) - ys[r]) ** 2).mean()

    norms, moved, flags = [], [], []
    for step in range(7):
        red.prepare()
        loss_fn(rank, step).backward()
        if red._late:                                    # what the race can leave behind
            store.flat_g[store.offsets[-1]] = float("nan")
        red.finish()
        norms.append(float(store.flat_g.abs().sum()))
        flags.append(float(red.last_drop) if red.last_drop is not None else 0.0)
        before = store.flat_p.clone()
        opt.skip_flag = red.last_drop
        opt.step()
        moved.append(float((store.flat_p - before).abs().sum()))
    dropped = red.poll_dropped()
    # replicas must still be identical (every rank applied the same updates)
    mine = store.flat_p.clone()
    ref = mine.clone()
    dist.broadcast(ref, src=0)
    q.put((rank, norms, moved, flags, dropped, bool(torch.equal(mine, ref)),
           bool(torch.isfinite(store.flat_p).all())))
    dist.destroy_process_group()


def test_world4_uneven_late_parameters_drop_steps_cleanly():
    """VERDICT r3 item 8 / ADVICE r3: late parameters on different ranks at different steps, a NaN
    left in the buffer by the race, optimizer step of a dropped step is a no-op."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_late4_worker, args=(r, 4, port, q)) for r in range(4)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, norms, moved, flags, dropped, same, finite in res:
        assert dropped == 2, (rank, dropped, flags)
        for step in range(7):
            if step in (2, 4):
                assert flags[step] > 0 and norms[step] == 0.0, (rank, step, norms, flags)
                assert moved[step] == 0.0, f"rank {rank}: dropped step {step} moved the parameters"
            else:
                assert flags[step] == 0.0 and norms[step] > 0 and moved[step] > 0, (rank, step)
        assert same, f"rank {rank}: replicas diverged"
        assert finite


class _ValTask(torch.nn.Module):
    """Stand-in for a task's validation surface (task_factory/*_task.py validation_step): the
    metric of a batch is its mean, so the expected job-wide result is known in closed form."""
    current_epoch, global_step = 0, 0

    def validation_step(self, batch, i):
        return {"val_loss": batch["x"].mean(), "wer": batch["x"].max()}


def _val_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from speech2text_amd.trainer import Trainer
    tr = Trainer()
    tr.device = torch.device("cpu")
    task = _ValTask()
    task.train()
    # rank 0: a batch of 3 samples (all 1.0) and one of 1 sample (5.0); rank 1: NO batch at all
    batches = [{"x": torch.full((3, 2), 1.0)}, {"x": torch.full((1, 2), 5.0)}] if rank == 0 else []
    res = tr.validate(task, batches)
    empty = tr.validate(task, [])                       # nobody has a batch: {} on every rank, no hang
    q.put((rank, res.get("val_loss"), res.get("wer"), empty, task.training))
    dist.destroy_process_group()


def test_validate_every_rank_reduces_and_weights_by_batch_size():
    """Trainer.validate in a data-parallel job: a rank whose validation shard is empty still takes
    part in the all-reduce (no hang) and gets the job-wide result; the mean is over SAMPLES
    (Lightning's epoch-level reduction): (3 * 1.0 + 1 * 5.0) / 4 = 2.0, not the batch mean 3.0."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_val_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, vl, wer, empty, training in got:
        assert vl == pytest.approx(2.0) and wer == pytest.approx(2.0)
        assert empty == {} and training
