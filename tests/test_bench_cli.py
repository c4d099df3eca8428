"""CPU: bench.py's CLI contract -- the oracle-only cpu_baseline leg runs, the roofline kernel
names are real C entry points, and `--gpus 2` starts its own two ranks (gloo rehearsal)."""
import json
import os
import subprocess
import sys

import torch

import bench
from speech2text_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_c3():
    cfg = bench.c3_config(64)
    cfg["encoder"]["config"].update({"downsampling_factor": [1, 2], "num_encoder_layers": [1, 1],
                                     "feedforward_dim": [96, 128], "encoder_dim": [48, 64],
                                     "encoder_unmasked_dim": [32, 48], "num_heads": [4, 4],
                                     "query_head_dim": 8, "value_head_dim": 4, "pos_dim": 16,
                                     "cnn_module_kernel": [15, 7]})
    cfg["predictor"]["config"].update({"output_dim": 64, "symbol_embedding_dim": 32})
    cfg["joiner"].update({"input_dim": 64})
    return cfg


def test_cpu_baseline_runs_on_oracle_only(monkeypatch):
    from speech2text_amd import zip_kernels as zk
    from speech2text_amd.build_task import TaskFactory

    def boom(*a, **k):
        raise AssertionError("cpu_baseline must not call product kernels")

    cfg = _tiny_c3()
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(cfg)
    sd = task.state_dict()
    for name in ("linear", "swoosh_forward", "bias_norm", "relpos_attention_weights"):
        monkeypatch.setattr(zk, name, boom)
    r = bench.cpu_baseline(cfg, sd, seconds=1.5, batch=2, n_labels=4, vocab=64, steps=3, warmup=1)
    assert r["kind"] == "port" and r["cores"] >= 1 and r["value"] > 0
    assert "3 timed steps" in r["sample"]


def test_cpu_baseline_c2_runs():
    from speech2text_amd.build_task import TaskFactory
    cfg = bench.c2_config(32, layers=2)
    cfg["encoder"]["config"].update({"input_dim": 32, "ffn_dim": 64, "output_dim": 32})
    cfg["decoder"]["config"].update({"input_dim": 32})
    torch.manual_seed(0)
    task = TaskFactory.get("CTC")(cfg)
    r = bench.cpu_baseline_c2(cfg, task.state_dict(), seconds=1.5, batch=2, n_labels=4, vocab=32,
                              steps=1, warmup=0)
    assert r["value"] > 0


def test_roofline_kernel_names_are_entry_points():
    protos = _native.parse_header()
    args = bench.parse_args([])
    assert args.gpus == 1 and args.steps >= 1 and args.config == "C3"
    assert args.roofline_kernel == "auto" or args.roofline_kernel in protos
    assert "s2t_relpos_attn_fwd" in protos          # the fallback used when "auto" finds nothing
    try:
        _native.profile_begin("relpos_attn_weights_fwd")
    except ValueError:
        pass
    else:
        raise AssertionError("profile_begin accepted a name that is not an entry point")


def test_gpus2_self_launch_gloo_rehearsal():
    env = dict(os.environ, MASTER_PORT="29731")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps",
                        "3", "--warmup", "1", "--launcher-selftest"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["backend"] == "gloo"


def test_plain_run_is_the_default():
    args = bench.parse_args([])
    assert not args.full and args.dump_outputs is None
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full


def test_start_state_restore_keep_gradient_and_dump(tmp_path):
    """The dumped step's inputs: StartState.restore puts the weights back THROUGH the flat store (and marks
    the bf16 pieces stale), resets module state and the optimizer / scheduler, and replays the random
    streams; keep_gradient copies the reduced gradient at the optimizer step; dump_outputs writes the same
    fixed sample of parameters and gradient in every run."""
    import random

    import numpy as np
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.layer.scaling import Whiten
    from speech2text_amd.trainer import Trainer
    cpu = torch.device("cpu")
    cfg = _tiny_c3()
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(cfg)
    trainer = Trainer(**cfg["trainer"]).setup(task, cpu)
    st = trainer.store
    random.seed(5)
    start = bench.StartState(task, cpu)
    draws = [random.random(), float(torch.rand(()))]
    ref = {n: p.detach().clone() for n, p in task.named_parameters()}
    whitens = [m for m in task.modules() if isinstance(m, Whiten)]
    assert whitens
    with torch.no_grad():
        for p in task.parameters():
            p.add_(1.0)
    for m in whitens:
        m.prob = m.min_prob / 2
    task.global_step = 7
    st.flat_g.fill_(3.0)
    old_opt, old_sched, epoch = trainer.optimizer, trainer.scheduler, st.epoch
    start.restore(trainer)
    for n, p in task.named_parameters():
        assert torch.equal(p, ref[n]), n
    i = next(j for j, q in enumerate(st.params) if q.numel() > 1)
    assert torch.equal(st.flat_p[st.offsets[i]:st.offsets[i] + st.lengths[i]], st.params[i].reshape(-1))
    assert st.epoch == epoch + 1 and not st.flat_g.any()
    assert all(m.prob == m.max_prob for m in whitens) and task.global_step == 0
    assert trainer.optimizer is not old_opt and trainer.scheduler is not old_sched
    assert trainer.optimizer.zero_grad_in_step == old_opt.zero_grad_in_step
    assert [random.random(), float(torch.rand(()))] == draws
    kept = bench.StartState.keep_gradient(trainer)
    g = torch.randn(st.flat_g.shape, generator=torch.Generator().manual_seed(1))
    st.flat_g.copy_(g)
    trainer.optimizer.step()
    assert torch.equal(kept["grad"], g) and "step_keeping_gradient" not in repr(trainer.optimizer.step)
    assert not all(torch.equal(p, ref[n]) for n, p in task.named_parameters())   # the update moved them
    names = [n for n, p in task.named_parameters() if p.requires_grad]
    total = sum(dict(task.named_parameters())[n].numel() for n in names)
    n, nbytes = bench.dump_outputs(str(tmp_path / "a"), torch.tensor(1.5), task, st, kept["grad"])
    assert n == 3 and nbytes == 8 + 8 * total                          # under the cap: every element
    par, gr = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "a" / "grads.npy")
    first = dict(task.named_parameters())[names[0]]
    np.testing.assert_array_equal(par[:first.numel()], first.detach().reshape(-1).numpy())
    o = st.offsets[next(j for j, q in enumerate(st.params) if q is first)]
    np.testing.assert_array_equal(gr[:first.numel()], g[o:o + first.numel()].numpy())
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [1.5]
    cap = 8 * total // 3                                               # over the cap: a seeded sample
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(1.5), task, st, kept["grad"], cap_bytes=cap)
    b = np.load(tmp_path / "b" / "params.npy")
    assert b.size == cap // 8 and b.dtype == np.float32
    np.testing.assert_array_equal(b, np.load(tmp_path / "c" / "params.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "grads.npy"), np.load(tmp_path / "c" / "grads.npy"))
    assert np.isin(b, par).all()
