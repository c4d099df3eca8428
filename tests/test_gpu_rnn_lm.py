"""GPU: the RNN language model and its task end to end -- RnnLm on the step-launched LSTM kernel,
NnLmTask, the trainer and the checkpoint -- against the reference's own outputs
(tests/golden/rnn_lm_ref.npz) and the float64 restatement tests/rnn_lm_f64.py.

Bounds.  Tiny fixture (V = 16, E = H = 8): max |got - ref| <= TINY x max |ref| per tensor with
TINY = 2e-5, the floor of the LSTM kernels' rule (rnn_lm_cases.FLOOR; the fp32 figures of every
case stay below a tenth of it), times the arith_bound factor because the Linears around the
recurrence run on the bf16-split GEMMs (tests/conftest.py).  YAML widths: the bounds of
test_lstm_predictor_at_the_yaml_dims_with_dropout, output atol 5e-5 / rtol 2e-4, gradients
3e-3 max|ref| + 5e-5.  Training run: see test_run_task_three_steps_follow_the_float64_replay.
"""
import copy
import os

import numpy as np
import pytest
import torch
import yaml

import rnn_lm_cases as LC
import rnn_lm_f64 as RF
from oracle import conformer as OC

pytestmark = pytest.mark.gpu

TINY = LC.FLOOR
LS = 0.1
STEP_NODE = "_LstmSeqBackward"


# ------------------------------------------------------------------ shared data (computed once)
@pytest.fixture(scope="module")
def fix(golden_dir):
    z = np.load(os.path.join(golden_dir, "rnn_lm_ref.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    return z, sd, torch.from_numpy(z["tokens"]), torch.from_numpy(z["lengths"])


def _task_cfg(V, E, L, dropout=0.0):
    return {"dataset": {}, "nnlm": dict(num_symbols=V, symbol_embedding_dim=E, num_rnn_layer=L,
                                        dropout=dropout, bidirectional=False),
            "loss": {"model": "MaskedKLDiv", "config": dict(num_classes=V, scale_factor=1.0,
                                                             label_smoothing=LS)},
            "metric": {"top_ks": [1, 5]}}


def _tiny_task(fix, dev):
    from speech2text_amd.task_factory.nnlm_task import NnLmTask
    _, sd, _, _ = fix
    task = NnLmTask(_task_cfg(16, 8, 2))
    task._nnlm.load_state_dict(sd, strict=True)
    return task.to(dev)


def _hold(what, got, ref, tol):
    ref = torch.as_tensor(np.asarray(ref))
    err = LC.rel_err(got, ref)
    print(f"{what}: err {err:.3e} bound {tol:.3e}")
    assert err <= tol, f"{what}: err {err:.3e} > bound {tol:.3e}"


def _ragged_text(B, T, V, seed, dev=None):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, T + 1, (B,), generator=g)
    lens[seed % B] = T
    text = torch.randint(1, V, (B, T), generator=g)
    for b in range(B):
        text[b, lens[b]:] = 0
    return text, lens


# ------------------------------------------------------------------ the model against the fixture
def test_forward_score_and_score_steps_equal_the_reference(dev, fix, arith_bound):
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    z, sd, tokens, lens = fix
    m = RnnLm(RnnLmConfig(num_symbols=16, symbol_embedding_dim=8, num_rnn_layer=2))
    assert list(m.state_dict()) == list(sd)
    m.load_state_dict(sd, strict=True)
    m.to(dev).eval()
    tol = TINY * arith_bound
    logits, out_lens = m(tokens.to(dev), lens.to(dev))
    assert logits.shape == (4, 9, 16) and torch.equal(out_lens.cpu(), lens)
    _hold("logits", logits, z["logits"], tol)
    score = m.score(tokens.to(dev), lens.to(dev))
    assert score.shape == (4,) and not score.requires_grad
    _hold("score", score, z["score"], tol)
    st = m.init_states(4)
    assert st[0].shape == st[1].shape == (2, 4, 8) and st[0].is_cuda and not st[0].any()
    for i in range(2):
        lp, st = m.score_step(tokens[:, i].to(dev), st)
        assert lp.shape == (4, 16) and st[0].shape == (2, 4, 8)
        _hold(f"step{i} log_probs", lp, z[f"step{i}_log_probs"], tol)
        _hold(f"step{i} h", st[0], z[f"step{i}_h"], tol)
        _hold(f"step{i} c", st[1], z[f"step{i}_c"], tol)


def test_training_step_equals_the_reference_loss_and_gradients(dev, fix, arith_bound):
    z, _, tokens, lens = fix
    task = _tiny_task(fix, dev).train()
    loss = task.training_step({"text": tokens.to(dev), "text_length": lens.to(dev)}, 0)
    assert "train_loss" in task.logged and loss.dim() == 0
    loss.backward()
    tol = TINY * arith_bound
    _hold("loss", loss.detach(), z["loss"], tol)
    names = [k[5:] for k in z.files if k.startswith("grad.")]
    assert sorted(names) == sorted(k for k, _ in task._nnlm.named_parameters())
    for k, p in task._nnlm.named_parameters():
        _hold("d " + k, p.grad, z["grad." + k], tol)


def test_validation_step_equals_the_restatement(dev, fix, arith_bound):
    _, sd, tokens, lens = fix
    task = _tiny_task(fix, dev).eval()
    info = task.validation_step({"text": tokens.to(dev), "text_length": lens.to(dev)}, 0)
    assert set(info) == {"val_loss", "top_1_acc", "top_5_acc"} and set(info) <= set(task.logged)
    sd64 = {k: v.double() for k, v in sd.items()}
    inp, lab, ll = RF.nnlm_io(tokens, lens)
    logits, _ = RF.logits_ref(sd64, inp)
    _hold("val_loss", info["val_loss"], RF.masked_kl_ref(logits, lab, ll, LS), TINY * arith_bound)
    for k in (1, 5):
        ref = float(RF.topk_acc_ref(logits, lab, ll, k))
        got = float(info[f"top_{k}_acc"])
        print(f"top_{k}_acc {got:.6f} ref {ref:.6f}")
        assert abs(got - ref) < 1e-6, (k, got, ref)       # a count over 19 positions: 1 / 19 apart


# ------------------------------------------------------------------ the YAML widths
@pytest.mark.parametrize("path,p", [("auto", 0.0), ("auto", 0.3), ("seq", 0.0)],
                         ids=["step_kernel", "step_kernel_dropout", "per_utterance_kernel"])
def test_training_step_at_the_yaml_widths(dev, monkeypatch, path, p):
    """E = H = 512, 3 layers, V = 128 at B = 5, T = 12 with ragged lengths: loss and every gradient
    against the float64 restatement.  The wrapper's own dispatch puts every layer on the
    step-launched kernel (checked at the autograd node); `per_utterance_kernel` raises the
    small-batch threshold above B to hold the same model on the dispatch's other kernel.  With
    dropout 0.3 the seeds are recorded at draw_seed and the keep masks rebuilt with
    oracle.conformer.keep_scale: L - 1 draw sites, none after the last layer."""
    from speech2text_amd import conf_kernels as ck
    from speech2text_amd.task_factory.nnlm_task import NnLmTask
    V, E, L, B, T = 128, 512, 3, 5, 12
    torch.manual_seed(21)
    task = NnLmTask(_task_cfg(V, E, L, dropout=p))
    sd = {k: v.detach().double().clone() for k, v in task._nnlm.state_dict().items()}
    task.to(dev).train()
    text, lens = _ragged_text(B, T + 1, V, 5)
    if path == "seq":
        monkeypatch.setattr(ck, "LSTM_STEP_MIN_BATCH", B + 1)
    seeds, nodes = [], []
    real_seed, real_lstm = ck.draw_seed, ck.lstm
    monkeypatch.setattr(ck, "draw_seed", lambda: seeds.append(real_seed()) or seeds[-1])

    def lstm(*a, **k):
        out = real_lstm(*a, **k)
        nodes.append(type(out[0].grad_fn).__name__)
        return out
    monkeypatch.setattr(ck, "lstm", lstm)
    loss = task.training_step({"text": text.to(dev), "text_length": lens.to(dev)}, 0)
    loss.backward()
    assert nodes == [STEP_NODE if path == "auto" else "_LnLstmBackward"] * L, nodes
    assert len(seeds) == (L - 1 if p > 0 else 0), seeds
    keep = None
    if p > 0:
        keep = [OC.keep_scale(s, (T, B, E), p).double() for s in seeds]
        assert all(0.6 < (k > 0).double().mean() < 0.8 for k in keep)
    ref_loss, ref_grads = RF.grads_ref(sd, lambda s: RF.nnlm_loss_ref(s, text, lens, LS, keep=keep))
    loss = float(loss.detach())
    print(f"loss {loss:.7f} ref {float(ref_loss):.7f}")
    np.testing.assert_allclose(loss, float(ref_loss), atol=5e-5, rtol=2e-4)
    for k, q in task._nnlm.named_parameters():
        ref = ref_grads[k].numpy()
        err = np.abs(q.grad.cpu().numpy() - ref).max()
        print(f"{k}: err {err:.3e} max|ref| {np.abs(ref).max():.3e}")
        assert err <= 3e-3 * np.abs(ref).max() + 5e-5, (k, err, np.abs(ref).max())


def test_eval_mode_draws_no_dropout(dev, monkeypatch):
    from speech2text_amd import conf_kernels as ck
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    m = RnnLm(RnnLmConfig(num_symbols=16, symbol_embedding_dim=8, num_rnn_layer=3, dropout=0.5)).to(dev).eval()
    monkeypatch.setattr(ck, "draw_seed", lambda: pytest.fail("dropout drew a seed in eval mode"))
    text, lens = _ragged_text(17, 6, 16, 2)
    a = m.score(text.to(dev), lens.to(dev))
    assert torch.equal(a, m.score(text.to(dev), lens.to(dev)))


# ------------------------------------------------------------------ trainer and checkpoint
def _yaml_cfg(golden_dir):
    root = os.path.join(golden_dir, "reference_configs")
    c = yaml.safe_load(open(os.path.join(root, "config", "training", "rnn_lm.yaml")))
    for k in ("spm_model", "spm_vocab"):
        c["tokenizer"]["config"][k] = os.path.join(root, c["tokenizer"]["config"][k])
    c["trainer"]["max_epochs"] = 1
    return c


RUN_BATCHES = [(17, 10, 31), (18, 9, 32), (17, 11, 33)]       # (B, T, seed): two batch tiles each


def replay(sd0, batches, dtype, clip=5.0):
    """The YAML's optimisation on the CPU in `dtype`: AdamW(lr 1e-3, weight decay 5e-4) under the
    project's Warmup(2000) schedule, gradient-norm clip 5.0 as the trainer applies it
    (coef = min(1, clip / (norm + 1e-6))) -> the loss of every step."""
    from speech2text_amd.optimizer.optim_setup import WarmupLR
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-3, weight_decay=5e-4)
    sched = WarmupLR(opt, warmup_steps=2000)
    losses = []
    for text, lens in batches:
        opt.zero_grad()
        loss = RF.nnlm_loss_ref(sd, text, lens, LS)
        loss.backward()
        norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in sd.values()))
        coef = float(torch.clamp(clip / (norm + 1e-6), max=1.0))
        for p in sd.values():
            p.grad.mul_(coef)
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    return losses


# |float32 replay - float64 replay| of the three losses, measured on the CPU (1 and 16 threads):
# at most 3.02e-7 (losses 4.044, 4.043, 4.043; one float32 ulp of them is 4.8e-7).  The margin of the device run is 8 x that, the project's factor
# between what fp32 costs the reference and what a kernel may cost (rnn_lm_cases.MARGIN), times the
# arith_bound factor for the Linears on the bf16-split GEMMs.
REPLAY_SPREAD = 3.1e-7


def test_run_task_three_steps_follow_the_float64_replay(dev, golden_dir, monkeypatch, arith_bound, tmp_path):
    """build_task.run_task on the reference YAML (tokenizer paths re-rooted, one epoch) over three
    small synthetic `text` batches: three optimizer steps of AdamW + Warmup + clip 5.0 through the
    trainer.  Every step's LOSS is held to the float64 CPU replay from the same initial parameters
    (not the parameters: AdamW's normalised first updates amplify the sign noise of near-zero
    gradients).  Then the checkpoint: written by checkpoint.py, loaded into a fresh task: the
    same parameters bit for bit, and the same `score` at the bound of the other model outputs
    (the trained task's Linears read the flat store, the fresh task's do not, and which GEMM kernel
    serves a small Linear is the plan cache's timed choice: equal inputs, last-bit differences)."""
    from speech2text_amd import build_task, checkpoint as C
    from speech2text_amd import conf_kernels as ck
    from speech2text_amd.trainer import Trainer
    cfg = _yaml_cfg(golden_dir)
    torch.manual_seed(1234)                          # run_task's own seed: the same initial parameters
    sd0 = {k[len("_nnlm."):]: v for k, v in build_task.TaskFactory.get("NNLM")(copy.deepcopy(cfg)).state_dict().items()}
    cpu_batches = [_ragged_text(B, T, 128, s) for B, T, s in RUN_BATCHES]
    ref = replay(sd0, cpu_batches, torch.float64)
    spread = max(abs(a - b) for a, b in zip(replay(sd0, cpu_batches, torch.float32), ref))
    print(f"replay losses {ref} fp32 spread {spread:.3e}")
    assert spread <= 4 * REPLAY_SPREAD and REPLAY_SPREAD <= 40 * spread, spread
    losses, nodes = [], []
    real_step, real_lstm = Trainer.training_step, ck.lstm

    def step(self, batch, i):
        out = real_step(self, batch, i)
        losses.append(float(out))
        return out

    def lstm(*a, **k):
        out = real_lstm(*a, **k)
        nodes.append(type(out[0].grad_fn).__name__)
        return out
    monkeypatch.setattr(Trainer, "training_step", step)
    monkeypatch.setattr(ck, "lstm", lstm)
    batches = [{"text": t, "text_length": n} for t, n in cpu_batches]      # the trainer moves them
    task, trainer = build_task.run_task(cfg, batches)
    assert task.global_step == 3 and len(losses) == 3
    assert nodes == [STEP_NODE] * 9, nodes
    assert all(p.is_cuda for p in task.parameters())
    margin = 8 * REPLAY_SPREAD * arith_bound
    for i, (a, b) in enumerate(zip(losses, ref)):
        print(f"step {i}: loss {a:.7f} replay {b:.7f} diff {abs(a - b):.3e} margin {margin:.3e}")
    for a, b in zip(losses, ref):
        assert abs(a - b) <= margin, (losses, ref, margin)
    # ---- checkpoint round trip
    path = str(tmp_path / "nnlm.ckpt")
    assert C.save_checkpoint(trainer, path)
    torch.manual_seed(99)
    fresh = build_task.TaskFactory.get("NNLM")(copy.deepcopy(cfg))
    missing, unexpected = C.load_from_checkpoint(fresh, path, strict=True)
    assert not missing and not unexpected
    for (k, v), (k2, v2) in zip(task.state_dict().items(), fresh.state_dict().items()):
        assert k == k2 and torch.equal(v.cpu(), v2), k
    fresh.to(dev).eval()
    task.eval()
    text, lens = cpu_batches[0]
    a = task._nnlm.score(text.to(dev), lens.to(dev))
    b = fresh._nnlm.score(text.to(dev), lens.to(dev))
    assert torch.isfinite(a).all() and a.shape == (len(lens),)
    _hold("score after the round trip", b, a.cpu(), TINY * arith_bound)
