"""GPU: every BASELINE.json configuration at its FULL size.

C3 (zipformer YAML dims, 500 BPE, prune_range 5): 2 x 10 s against the oracle (features,
encoder activations, simple / pruned loss within the north-star 1e-3, prune ranges); the bench's
padded geometry against the oracle with eight utterances ragged: 64 x 10 s in evaluation mode
(every utterance's losses), the bench's training step at 32 x 10 s and chunked at 16 x 10 s (loss,
every gradient); then the per-rank batch of 64 through size-independent properties (finite, lengths,
ranges monotone and in bounds, loss decreasing under the real optimizer).  C2 (conformer-CTC, 12 layers, d = 256),
C4 (CTC_Hybrid_Rnnt, B = 16, U = 60) and C5 (BEST-RQ, 30 s, 8192 x 16 codebook, KL over 8193
classes) likewise: a small-batch comparison with the oracle at full model size plus the full
batch through properties.  The oracle for k2 / torchaudio / lhotse arithmetic is our restatement
(PARITY UNPINNED for those parts, see oracle/*.py headers).
"""
import random

import numpy as np
import pytest
import torch
from torch.utils.checkpoint import checkpoint

import bench
from oracle import conformer as OC
from oracle import fbank as ofb
from oracle import heads as H
from oracle import k2_rnnt as K2
from oracle import zipformer as Z

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(float(a) - float(b)) / max(1e-12, abs(float(b)))


def _c2(layers=12):
    cfg = bench.c2_config(128, layers=layers)
    cfg["optim_setup"]["lr_scheduler"]["config"]["warmup_steps"] = 10      # reach a real lr quickly
    return cfg


def _cpu_sd(task):
    return {k: v.detach().cpu().clone() for k, v in task.state_dict().items()}


# ------------------------------------------------------------------------------------ C3
def test_c3_yaml_dims_two_utterances_vs_oracle(dev):
    from speech2text_amd.build_task import TaskFactory
    cfg = bench.c3_config(500)
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("Pruned_Rnnt")(cfg)
    sd = _cpu_sd(task)
    task.to(dev).eval()
    batch = bench.make_batch(0, 2, 10.0, 50, 500, dev)
    batch["pcm_length"][1] = 131000                         # ragged: 8.2 s
    batch["label_length"][1] = 37
    with torch.no_grad():
        feat, feat_len = task.features(batch)
        enc, enc_len = task._encoder(feat, feat_len)
        pred, pred_len, _ = task._predictor(batch["label"], batch["label_length"],
                                            task._predictor.init_state())
        lattice, boundary, ranges, simple = task._joiner(enc, enc_len, pred, pred_len, batch["label"])
        pruned = task._loss({"logits": lattice, "logits_length": enc_len, "targets": batch["label"],
                             "targets_length": batch["label_length"], "boundary": boundary,
                             "ranges": ranges})
    # ---- oracle on the same parameters and PCM (lhotes_fbank: 16-bit scale, high_freq -400)
    pcm = batch["pcm"].cpu().numpy()
    n = batch["pcm_length"].cpu().numpy()
    fo = [ofb.fbank(pcm[i, :n[i]] * 32768.0, 80, high_freq=-400.0) for i in range(2)]
    assert [f.shape[0] for f in fo] == feat_len.cpu().tolist() == [998, 817]
    for i in range(2):
        np.testing.assert_allclose(feat[i, :fo[i].shape[0]].cpu().numpy(), fo[i], atol=5e-3)
    x = torch.zeros(2, 998, 80)
    for i in range(2):
        x[i, :fo[i].shape[0]] = torch.from_numpy(fo[i])
    enc_sd = {k[len("_encoder.encoder."):]: v for k, v in sd.items() if k.startswith("_encoder.encoder.")}
    lab, lab_len = batch["label"].cpu(), batch["label_length"].cpu()
    with torch.no_grad():
        yo, ylo = Z.zipformer_forward(enc_sd, bench._zcfg(cfg["encoder"]["config"]), x,
                                      feat_len.cpu(), Z.Ctl(False), -1, -1)
        po = H.stateless_predictor(sd, "_predictor.predictor.", lab, 5)
        am, lm = H.joiner_projections(sd, "_joiner.", yo, po)
        lo, bo, ro, so = K2.joiner_pruned(am, lm, lab, lab_len, ylo, 5)
        pro = K2.rnnt_loss_pruned(lo, lab, ro, 0, bo)
    assert enc_len.cpu().tolist() == ylo.tolist() == [248, 203]
    # encoder activations: stated fp32 tolerance (12 layers deep, features differ by ~1e-3)
    err = (enc.cpu() - yo).abs().max().item()
    assert err <= 2e-3 * max(1.0, yo.abs().max().item()), err
    # north star: loss parity within 1e-3 relative
    assert _rel(simple, so) <= 1e-3, (float(simple), float(so))
    assert _rel(pruned, pro) <= 1e-3, (float(pruned), float(pro))
    same = (ranges.cpu() == ro).float().mean().item()
    assert same >= 0.98, same                               # argmax ties can move a window by one


def _warm_gemm_plans(cfg, fb, dev, rv):
    """One untimed training step on a SECOND task object of the same shapes: the first step of a
    process runs the Python layer executor, which times the step's GEMM shape buckets
    (zip_kernels.lt_matmul -> s2t_zl_plan_put); the table is per process, not per model, so the step
    that is compared afterwards is served by the native executor (csrc/zip_layer.hip) -- the code
    bench.py times from its second step on -- while the compared task's own state (Whiten.prob,
    Balancer counters, parameters) is untouched."""
    from speech2text_amd import flat
    from speech2text_amd.build_task import TaskFactory
    st = random.getstate()
    warm = TaskFactory.get("Pruned_Rnnt")(cfg).to(dev)
    flat.get_store([p for p in warm.parameters() if p.requires_grad])
    warm.train()
    warm.training_step(fb, 0).backward()
    torch.cuda.synchronize()
    del warm
    random.setstate(st)


@pytest.mark.parametrize("rv,chunk,native", [(0.0, (-1, -1), True), (0.2, (-1, -1), True),
                                             (0.2, (32, 128), True), (0.0, (16, 64), True),
                                             (0.2, (64, 256), True), (0.2, (-1, -1), False)])
def test_c3_yaml_dims_training_step_gradients_vs_oracle(dev, monkeypatch, rv, chunk, native):
    """The code the bench times -- the NATIVE per-layer executor (csrc/zip_layer.hip; `native`
    False: the Python executor of the same launch sequence, zip_layer._LayerFn, so that both stay
    pinned to the oracle) -- i.e. the layer executor's backward at D = 192 / 256, H = 4 / 8,
    K = 31 / 15, T = 495 ... 62, the stateless predictor, the joiner with the simple loss, prune
    ranges and the fused pruned lattice -- in TRAINING mode at the YAML dims: 2 x 10 s (ragged),
    Python `random` pinned (0.0: every Balancer / Whiten / limit_param_value and the attention
    score penalty fire; 0.2: the default-probability Balancers and every Whiten), positional
    dropout off, feature masks from the same CPU generator.  Loss (0.5 simple + 0.5 pruned,
    task_factory/rnnt_task.py:496-499) and EVERY parameter gradient against oracle/zipformer.py
    + oracle/heads.py + oracle/k2_rnnt.py (k2 part parity unpinned).
    `chunk` = (chunk_size, left_context_frames) of the YAML's training mode
    (config/training/zipformer_stateless_pruned_rnnt.yaml:65-66, reference
    model/encoder/zipformer.py:290-317,409-448): the chunk-masked attention forward / backward
    tiles and the chunk-causal depthwise conv's edge scaling (model/layer/scaling.py:622-681) at
    T = 495 ... 62, H = 4 / 8, K = 31 / 15."""
    from speech2text_amd import flat, rng, zip_layer, zip_native
    from speech2text_amd.build_task import TaskFactory
    monkeypatch.setattr(rng, "rand", lambda *s, device=None, dtype=torch.float32:
                        torch.rand(*s, dtype=dtype).to(device))
    cfg = bench.c3_config(500)
    cs, lcf = chunk
    cfg["encoder"]["config"]["chunk_size"] = [cs]
    cfg["encoder"]["config"]["left_context_frames"] = [lcf]
    lcc = -1 if cs < 0 else max(1, lcf // cs)
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("Pruned_Rnnt")(cfg)
    pnames = {n for n, _ in task.named_parameters()}
    sd = {k: v.detach().cpu().clone().requires_grad_(k in pnames and v.dtype.is_floating_point)
          for k, v in task.state_dict().items()}
    task.to(dev)
    flat.get_store([p for p in task.parameters() if p.requires_grad])
    batch = bench.make_batch(0, 2, 10.0, 50, 500, dev)
    batch["pcm_length"][1] = 131000
    batch["label_length"][1] = 37
    task.eval()
    with torch.no_grad():
        feat, feat_len = task.features(batch)
    task.train()
    for mod in task.modules():
        if mod.__class__.__name__ == "CompactRelPositionalEncoding":
            mod.dropout.p = 0.0
    fb = {"feat": feat, "feat_length": feat_len, "label": batch["label"],
          "label_length": batch["label_length"]}
    monkeypatch.setattr(random, "random", lambda: rv)
    monkeypatch.setattr(zip_native, "ENABLED", native)
    if native:
        _warm_gemm_plans(cfg, fb, dev, rv)
    calls0, nat0 = zip_layer.CALLS[0], list(zip_native.CALLS)
    torch.manual_seed(7)
    loss = task.training_step(fb, 0)
    loss.backward()
    torch.cuda.synchronize()
    assert zip_layer.CALLS[0] - calls0 == 12, "the layer executor did not serve every layer"
    moved = [zip_native.CALLS[0] - nat0[0], zip_native.CALLS[1] - nat0[1]]
    assert moved == ([12, 12] if native else [0, 0]), \
        f"native executor served {moved} forward / backward layer calls of 12 / 12"
    # ---- oracle, same parameters / features / decisions
    enc_sd = {k[len("_encoder.encoder."):]: v for k, v in sd.items() if k.startswith("_encoder.encoder.")}
    lab, lab_len = batch["label"].cpu(), batch["label_length"].cpu()
    torch.manual_seed(7)
    yo, ylo = Z.zipformer_forward(enc_sd, bench._zcfg(cfg["encoder"]["config"]), feat.cpu(),
                                  feat_len.cpu(), Z.Ctl(True, lambda: rv, pos_dropout=0.0), cs, lcc)
    po = H.stateless_predictor(sd, "_predictor.predictor.", lab, 5)
    am, lm = H.joiner_projections(sd, "_joiner.", yo, po)
    lo, bo, ro, so = K2.joiner_pruned(am, lm, lab, lab_len, ylo, 5)
    pro = K2.rnnt_loss_pruned(lo, lab, ro, 0, bo)
    ref = H.pruned_rnnt_task_loss(so, pro, 0.5, 0.5)
    ref.backward()
    assert _rel(loss, ref) <= 1e-3, (float(loss), float(ref))
    worst, worst_name = 0.0, None
    for n, p in task.named_parameters():
        r = sd[n].grad
        r = torch.zeros_like(sd[n]) if r is None else r
        g = torch.zeros_like(r) if p.grad is None else p.grad.detach().cpu()
        e = (g - r).abs().max().item() / (r.abs().max().item() + 1e-6)
        if e > worst:
            worst, worst_name = e, n
    assert worst <= 5e-3, (worst_name, worst)


# The bench's geometry: bench.make_batch(0, B, 10.0, 50, 500) keeps its padded shape (998 frames, 50
# labels), so every product runs in the bench's shape buckets; eight utterances spread over the batch
# are shorter.  Their PCM lengths (6.25 ... 9.875 s) give encoder lengths 245 232 220 207 195 182 169
# 154, one of every remainder modulo 8: partial last groups in every down / upsampling ratio.  Their
# label lengths run from 50 down to 2, the last below prune_range 5 (the padding branch of the prune
# ranges).
_RAGGED_PCM = (158000, 150000, 142000, 134000, 126000, 118000, 109500, 100000)
_RAGGED_LABELS = (50, 43, 36, 29, 22, 15, 8, 2)


def _ragged_bench_batch(B, dev):
    """-> (bench.make_batch(0, B, 10.0, 50, 500, dev) with the eight ragged utterances, their rows)."""
    batch = bench.make_batch(0, B, 10.0, 50, 500, dev)
    rows = [1 + k * (B - 2) // 7 for k in range(8)]
    for b, n, s in zip(rows, _RAGGED_PCM, _RAGGED_LABELS):
        batch["pcm_length"][b] = n
        batch["label_length"][b] = s
    return batch, rows


def _oracle_c3_train_step(sd, cfg, feat, feat_len, lab, lab_len, rv, cs, lcc, recompute=True):
    """The oracle's C3 training step on `sd` (CPU tensors, the trainable ones requiring grad):
    oracle/zipformer.py + heads.py + k2_rnnt.py forward, 0.5 simple + 0.5 pruned loss, backward
    (gradients land in sd[name].grad) -> loss.  With `recompute` the subsampling frontend and every
    encoder layer keep only their inputs and run again in backward (torch.utils.checkpoint): the plain
    graph of 64 x 10 s would hold ~26 GB of host memory.  The recomputation repeats the arithmetic --
    the step's random decisions are the pinned `rv` and the feature masks drawn outside those pieces
    -- so the gradients are the plain graph's bit for bit (measured at B = 4, plain and chunked)."""
    def recomputed(fn):
        return lambda *a: checkpoint(fn, *a, use_reentrant=False)

    nt = torch.get_num_threads()
    torch.set_num_threads(bench.host_threads())
    try:
        with pytest.MonkeyPatch.context() as mp:
            if recompute:
                mp.setattr(Z, "conv2d_subsampling", recomputed(Z.conv2d_subsampling))
                mp.setattr(Z, "encoder_layer", recomputed(Z.encoder_layer))
            enc_sd = {k[len("_encoder.encoder."):]: v for k, v in sd.items()
                      if k.startswith("_encoder.encoder.")}
            yo, ylo = Z.zipformer_forward(enc_sd, bench._zcfg(cfg["encoder"]["config"]), feat, feat_len,
                                          Z.Ctl(True, lambda: rv, pos_dropout=0.0), cs, lcc)
            po = H.stateless_predictor(sd, "_predictor.predictor.", lab, 5)
            am, lm = H.joiner_projections(sd, "_joiner.", yo, po)
            lo, bo, ro, so = K2.joiner_pruned(am, lm, lab, lab_len, ylo, 5)
            pro = K2.rnnt_loss_pruned(lo, lab, ro, 0, bo)
            ref = H.pruned_rnnt_task_loss(so, pro, 0.5, 0.5)
            del yo, po, am, lm, lo
            ref.backward()
    finally:
        torch.set_num_threads(nt)
    return ref.detach()


def _worst(err):
    """err (B,) -> (worst value, its utterance)."""
    b = int(torch.argmax(err))
    return float(err[b]), b


def test_c3_bench_geometry_eval_vs_oracle(dev):
    """The B = 2 comparison above at the bench's geometry: 64 x 10 s padded, eight utterances ragged
    (_ragged_bench_batch), so the six stacks run 31 680 / 15 872 / 7 936 / 3 968 / 7 936 / 15 872 rows --
    GEMM plan buckets, batch-sized workspaces and grids that B = 2 never reaches.  The plans of this
    geometry are timed first by one training step of a second task; the task's parameters live in a
    FlatStore as the bench's do, so the plans' own kernels serve the products.  Features, encoder
    lengths, the encoder output on each utterance's valid frames, prune ranges, and the simple and
    pruned loss of EVERY utterance against the oracle: a batch mean dilutes one wrong utterance 64-fold."""
    from speech2text_amd import flat
    from speech2text_amd import kernels as K
    from speech2text_amd import zip_kernels as zk
    from speech2text_amd.build_task import TaskFactory
    B = 64
    cfg = bench.c3_config(500)
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("Pruned_Rnnt")(cfg)
    sd = _cpu_sd(task)
    task.to(dev)
    flat.get_store([p for p in task.parameters() if p.requires_grad])
    batch, rows = _ragged_bench_batch(B, dev)
    task.eval()
    with torch.no_grad():
        feat, feat_len = task.features(batch)
    _warm_gemm_plans(cfg, {"feat": feat, "feat_length": feat_len, "label": batch["label"],
                           "label_length": batch["label_length"]}, dev, 0.0)
    bucket = zk._half_octave(B * 495)                        # stack 0: 495 frames x 64 utterances
    assert bucket == 29 and any(k[1] == bucket for k in zk._PLANS), \
        ("no GEMM plan in the 31 680-row bucket", sorted({k[1] for k in zk._PLANS}))
    task.eval()
    lab, lab_len = batch["label"].cpu(), batch["label_length"].cpu()
    with torch.no_grad():
        enc, enc_len = task._encoder(feat, feat_len)
        pred, pred_len, _ = task._predictor(batch["label"], batch["label_length"],
                                            task._predictor.init_state())
        lattice, boundary, ranges, simple = task._joiner(enc, enc_len, pred, pred_len, batch["label"])
        pruned = task._loss({"logits": lattice, "logits_length": enc_len, "targets": batch["label"],
                             "targets_length": batch["label_length"], "boundary": boundary,
                             "ranges": ranges})
        # the same kernels, per utterance (the task reduces them with a mean)
        sym = batch["label"].to(torch.int64).contiguous()
        simple_u = K.rnnt_simple_loss(lattice.lm.float(), lattice.am.float(), sym, boundary, 0)[0].cpu()
        pruned_u = K.rnnt_pruned_joiner_loss(lattice.am, lattice.lm, ranges, sym, boundary, 0,
                                             lattice.activation).cpu()
    assert _rel(simple_u.mean(), simple) <= 1e-6 and _rel(pruned_u.mean(), pruned) <= 1e-6
    assert enc.shape == (B, 248, 256)
    # ---- oracle on the same parameters and PCM
    pcm = batch["pcm"].cpu().numpy()
    n = batch["pcm_length"].cpu().numpy()
    fo = [ofb.fbank(pcm[i, :n[i]] * 32768.0, 80, high_freq=-400.0) for i in range(B)]
    frames = [f.shape[0] for f in fo]
    assert frames == feat_len.cpu().tolist()
    assert [frames[b] for b in rows] == [986, 936, 886, 836, 786, 736, 682, 623]
    feat_err = torch.tensor([np.abs(feat[i, :frames[i]].cpu().numpy() - fo[i]).max() for i in range(B)])
    x = torch.zeros(B, 998, 80)
    for i in range(B):
        x[i, :frames[i]] = torch.from_numpy(fo[i])
    enc_sd = {k[len("_encoder.encoder."):]: v for k, v in sd.items() if k.startswith("_encoder.encoder.")}
    nt = torch.get_num_threads()
    torch.set_num_threads(bench.host_threads())
    try:
        with torch.no_grad():
            yo, ylo = Z.zipformer_forward(enc_sd, bench._zcfg(cfg["encoder"]["config"]), x,
                                          feat_len.cpu(), Z.Ctl(False), -1, -1)
            po = H.stateless_predictor(sd, "_predictor.predictor.", lab, 5)
            am, lm = H.joiner_projections(sd, "_joiner.", yo, po)
            lo, bo, ro, so = K2.joiner_pruned(am, lm, lab, lab_len, ylo, 5)
            so_u = K2.rnnt_loss_smoothed(lm.float(), am.float(), lab, 0, bo, reduction="none")[0]
            pro_u = K2.rnnt_loss_pruned(lo, lab, ro, 0, bo, reduction="none")
    finally:
        torch.set_num_threads(nt)
    el = ylo.tolist()
    enc_err = torch.tensor([(enc[b, :el[b]].cpu() - yo[b, :el[b]]).abs().max().item()
                            / max(1.0, yo[b, :el[b]].abs().max().item()) for b in range(B)])
    simple_err = (simple_u - so_u).abs() / so_u.abs()
    pruned_err = (pruned_u - pro_u).abs() / pro_u.abs()
    same = (ranges.cpu() == ro).float().mean().item()
    print(f"\n[c3 bench geometry eval, B = {B}] worst (error, utterance): features "
          f"{_worst(feat_err)}, encoder {_worst(enc_err)} of max, simple {_worst(simple_err)}, pruned "
          f"{_worst(pruned_err)} relative; batch means simple {_rel(simple, so_u.mean()):.2e} pruned "
          f"{_rel(pruned, pro_u.mean()):.2e}; prune ranges {same:.4f} identical")
    assert _worst(feat_err)[0] <= 5e-3, ("features", _worst(feat_err))
    assert enc_len.cpu().tolist() == el and [el[b] for b in rows] == [245, 232, 220, 207, 195, 182, 169, 154]
    assert _worst(enc_err)[0] <= 2e-3, ("encoder output, valid frames", _worst(enc_err))
    assert _worst(simple_err)[0] <= 1e-3, ("simple loss of an utterance", _worst(simple_err))
    assert _worst(pruned_err)[0] <= 1e-3, ("pruned loss of an utterance", _worst(pruned_err))
    assert _rel(simple, so_u.mean()) <= 1e-3, (float(simple), float(so_u.mean()))
    assert _rel(pruned, pro_u.mean()) <= 1e-3, (float(pruned), float(pro_u.mean()))
    assert same >= 0.98, same                               # argmax ties can move a window by one


@pytest.mark.parametrize("B,rv,chunk", [(32, 0.0, (-1, -1)), (16, 0.2, (32, 128))])
def test_c3_bench_geometry_training_step_vs_oracle(dev, monkeypatch, B, rv, chunk):
    """The training step as bench.main runs and times it -- Trainer.setup, bench.StartState, two warm
    steps (the first times the GEMM plans of this geometry on the Python layer executor, the second runs
    on the native one), StartState.restore, StartState.keep_gradient, one Trainer.training_step -- against
    the oracle: the loss and the reduced flat gradient, parameter by parameter, at the B = 2 test's bounds.
    The batch is the bench's padded one (_ragged_bench_batch), fed the way the B = 2 test feeds it:
    features computed once in evaluation mode, feature masks drawn on the host, Python `random` pinned
    (0.0: every Balancer / Whiten / limit_param_value and the score penalty fire), positional dropout off.
    B = 32 runs 15 840 / 7 936 / 3 968 / 1 984 rows in stacks 0-3.  The oracle's host memory decides
    that batch: with the frontend and the layers recomputed in backward (_oracle_c3_train_step) the
    oracle half peaks at 8.9 GiB host RSS at B = 32 (158 s on 8 threads, measured without a GPU) and at
    15.5 GiB at 64 -- over the 12 GB a test may hold on a shared host.  The second case is the YAML's
    chunked training mode (chunk 32, left context 128 frames) at B = 16 (7 920 rows in stack 0): the
    chunk-masked attention tiles and chunk-causal conv edges against padding; 4.7 GiB, 14 s."""
    from speech2text_amd import rng, zip_native
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer
    monkeypatch.setattr(rng, "rand", lambda *s, device=None, dtype=torch.float32:
                        torch.rand(*s, dtype=dtype).to(device))
    cfg = bench.c3_config(500)
    cs, lcf = chunk
    cfg["encoder"]["config"]["chunk_size"] = [cs]
    cfg["encoder"]["config"]["left_context_frames"] = [lcf]
    lcc = -1 if cs < 0 else max(1, lcf // cs)
    random.seed(1234)
    np.random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("Pruned_Rnnt")(cfg)
    pnames = {n for n, _ in task.named_parameters()}
    sd = {k: v.detach().cpu().clone().requires_grad_(k in pnames and v.dtype.is_floating_point)
          for k, v in task.state_dict().items()}
    trainer = Trainer(**cfg["trainer"]).setup(task, dev)
    batch, _ = _ragged_bench_batch(B, dev)
    task.eval()
    with torch.no_grad():
        feat, feat_len = task.features(batch)
    task.train()
    for mod in task.modules():
        if mod.__class__.__name__ == "CompactRelPositionalEncoding":
            mod.dropout.p = 0.0
    fb = {"feat": feat, "feat_length": feat_len, "label": batch["label"],
          "label_length": batch["label_length"]}
    monkeypatch.setattr(random, "random", lambda: rv)
    torch.manual_seed(1234)
    start = bench.StartState(task, dev)
    for i in range(2):
        trainer.training_step(fb, i)
    torch.cuda.synchronize()
    start.restore(trainer)
    kept = start.keep_gradient(trainer)
    host_rng = torch.get_rng_state()                         # the feature masks' generator
    nat0 = list(zip_native.CALLS)
    loss = trainer.training_step(fb, 2)
    torch.cuda.synchronize()
    moved = [zip_native.CALLS[0] - nat0[0], zip_native.CALLS[1] - nat0[1]]
    assert moved == [12, 12], f"native executor served {moved} forward / backward layer calls of 12 / 12"
    store = trainer.store
    where = {id(p): (o, n) for p, o, n in zip(store.params, store.offsets, store.lengths)}
    grads = {n: kept["grad"][where[id(p)][0]:sum(where[id(p)])].view_as(p).cpu()
             for n, p in task.named_parameters()}
    # ---- oracle, same parameters / features / decisions
    torch.set_rng_state(host_rng)
    ref = _oracle_c3_train_step(sd, cfg, feat.cpu(), feat_len.cpu(), batch["label"].cpu(),
                                batch["label_length"].cpu(), rv, cs, lcc)
    # The output downsample's bias is a softmax over 2 taps: its gradient is 0.25 (dw0 - dw1), the
    # difference of the two taps' sums g * src over B x 248 x 256 terms.  At B = 32 the taps' sums are
    # 4e4 - 9e4 times larger than that difference (measured: taps 131.24 / 131.26, bias gradient
    # 3.3e-3), so ONE fp32 rounding of a tap sum moves the bias gradient by ~1e-3 of itself -- in the
    # oracle as in the kernel, whose tap sums match a float64 sum of its own inputs to 7e-7 and whose
    # float-atomic order alone moved that gradient by 3.4e-3 between two calls on identical inputs.
    # That parameter gets 2e-2 (a few roundings of the taps); every other one the B = 2 test's 5e-3.
    ill, ill_bound, ill_err = "_encoder.encoder.downsample_output.bias", 2e-2, 0.0
    worst, worst_name = 0.0, None
    for n, g in grads.items():
        r = sd[n].grad
        r = torch.zeros_like(sd[n]) if r is None else r
        e = (g - r).abs().max().item() / (r.abs().max().item() + 1e-6)
        if n == ill:
            ill_err = e
        elif e > worst:
            worst, worst_name = e, n
    print(f"\n[c3 bench geometry training step, B = {B}, rv {rv}, chunk {chunk}] loss {float(loss):.4f} "
          f"oracle {float(ref):.4f} ({_rel(loss, ref):.2e} relative); worst gradient {worst:.2e} of its "
          f"max at {worst_name}; {ill} {ill_err:.2e}")
    assert _rel(loss, ref) <= 1e-3, (float(loss), float(ref))
    assert worst <= 5e-3, (worst_name, worst)
    assert ill_err <= ill_bound, (ill, ill_err)


def test_c3_yaml_size_prune_ranges_bit_exact_given_the_oracles_gradients(dev):
    """Index work is bit-exact GIVEN identical float inputs (model/joiner/joiner.py:112-118 ->
    k2.get_rnnt_prune_ranges): at the YAML size (T = 248, S = 50, C = 500, prune_range 5, ragged
    lengths) the oracle's px_grad / py_grad go into s2t_rnnt_prune_ranges and every window must
    equal the oracle's -- 100 %, not the >= 98 % of the end-to-end comparison above, where the
    product's own fp32 gradients differ from the oracle's in the last bits."""
    from speech2text_amd import kernels as k
    g = torch.Generator().manual_seed(11)
    B, T, S, C, R = 8, 248, 50, 500, 5
    am = torch.randn(B, T, C, generator=g) * 2
    lm = torch.randn(B, S + 1, C, generator=g) * 2
    sym = torch.randint(1, C, (B, S), generator=g)
    tl = torch.randint(20, S + 1, (B,), generator=g)
    tl[0] = S
    el = torch.randint(150, T + 1, (B,), generator=g)
    el[0] = T
    bnd = torch.zeros(B, 4, dtype=torch.int64)
    bnd[:, 2] = tl
    bnd[:, 3] = el
    _, (gx, gy) = K2.rnnt_loss_smoothed(lm, am, sym, 0, bnd)
    ref = K2.get_rnnt_prune_ranges(gx, gy, bnd, R)
    out = k.rnnt_prune_ranges(gx.to(dev).contiguous(), gy.to(dev).contiguous(), bnd.to(dev), R)
    assert out.dtype == torch.int64 and tuple(out.shape) == (B, T, R)
    assert torch.equal(out.cpu(), ref), float((out.cpu() == ref).float().mean())
    # monotone, in bounds (k2's invariants)
    s0 = out[:, :, 0].cpu()
    assert (s0[:, 1:] >= s0[:, :-1]).all() and (s0 >= 0).all() and (s0 + R - 1 <= S).all()


@pytest.mark.parametrize("B,T,S,R", [(3, 600, 20, 5), (2, 257, 7, 3), (4, 31, 12, 13)])
def test_prune_ranges_long_sequences_vs_oracle(dev, B, T, S, R):
    """The window adjustment (two reverse running minima + clamp) is a workgroup-wide scan in the
    kernel: sequences longer than the 256 threads of its workgroup (several frames per thread),
    one frame over, and a window as wide as the label axis -- random gradients, ragged lengths."""
    from speech2text_amd import kernels as k
    g = torch.Generator().manual_seed(T + S)
    gx = torch.randn(B, S, T + 1, generator=g)
    gy = torch.randn(B, S + 1, T, generator=g)
    bnd = torch.zeros(B, 4, dtype=torch.int64)
    bnd[:, 2] = torch.randint(max(1, R - 1), S + 1, (B,), generator=g)
    bnd[:, 3] = torch.randint(T // 2, T + 1, (B,), generator=g)
    bnd[0, 2], bnd[0, 3] = S, T
    ref = K2.get_rnnt_prune_ranges(gx, gy, bnd, R)
    out = k.rnnt_prune_ranges(gx.to(dev), gy.to(dev), bnd.to(dev), R)
    assert torch.equal(out.cpu(), ref), float((out.cpu() == ref).float().mean())


def test_c3_full_batch_properties(dev):
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer
    cfg = bench.c3_config(500)
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("Pruned_Rnnt")(cfg)
    tr = Trainer(**cfg["trainer"]).setup(task, dev)
    task.train()
    batch = bench.make_batch(0, 64, 10.0, 50, 500, dev)
    batch["pcm_length"][5] = 99000
    batch["label_length"][5] = 21
    losses = [float(tr.training_step(batch, i)) for i in range(4)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    task.eval()
    with torch.no_grad():
        feat, feat_len = task.features(batch)
        enc, enc_len = task._encoder(feat, feat_len)
        pred, pred_len, _ = task._predictor(batch["label"], batch["label_length"],
                                            task._predictor.init_state())
        lattice, boundary, ranges, simple = task._joiner(enc, enc_len, pred, pred_len, batch["label"])
    assert enc.shape == (64, 248, 256) and torch.isfinite(enc).all()
    assert enc_len.cpu().tolist() == [((int(f) - 7) // 2 + 1) // 2 for f in feat_len.cpu()]
    r = ranges.cpu()
    assert r.shape == (64, 248, 5) and int(r.min()) >= 0
    for b in range(64):                                      # k2 prune-range invariants
        S, T = int(batch["label_length"][b]), int(enc_len[b])
        rb = r[b, :T]
        assert int(rb.max()) <= S and (rb[:, 1:] - rb[:, :-1] == 1).all()
        assert (rb[1:, 0] >= rb[:-1, 0]).all() and (rb[1:, 0] - rb[:-1, 0] <= 4).all()
        assert int(rb[0, 0]) == 0 and int(rb[T - 1, 4]) == S
    assert lattice.shape == (64, 248, 5, 500)


# ------------------------------------------------------------------------------------ C2
def test_c2_conformer_ctc_full_size(dev):
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer
    cfg = _c2()
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("CTC")(cfg)
    sd = _cpu_sd(task)
    task.to(dev).eval()
    batch = bench.make_batch(0, 2, 10.0, 40, 128, dev)
    batch["pcm_length"][1] = 120000
    with torch.no_grad():
        feat, feat_len = task.features(batch)
        enc, enc_len = task._encoder(feat, feat_len)
        dec, dec_len = task._decoder(enc, enc_len)
        loss = task._loss({"logits": dec, "logits_length": dec_len, "targets": batch["label"],
                           "targets_length": batch["label_length"]})
    pcm, n = batch["pcm"].cpu().numpy(), batch["pcm_length"].cpu().numpy()
    x = torch.zeros(2, 998, 80)
    for i in range(2):
        f = ofb.fbank(pcm[i, :n[i]], 80)
        x[i, :f.shape[0]] = torch.from_numpy(f)
    enc_sd = {k[len("_encoder.encoder."):]: v for k, v in sd.items() if k.startswith("_encoder.encoder.")}
    with torch.no_grad():
        yo, ylo = OC.conformer_forward(enc_sd, x, feat_len.cpu(), 12, 4, training=False)
        lg = H.projector(sd, "_decoder.decoder.", yo)
        ref = torch.nn.functional.ctc_loss(lg.log_softmax(-1).transpose(0, 1), batch["label"].cpu(),
                                           ylo, batch["label_length"].cpu(), blank=0,
                                           reduction="mean", zero_infinity=True)
    assert enc.shape == (2, 248, 256) and enc_len.cpu().tolist() == ylo.tolist()
    # frames past an utterance's length are unspecified in both; compare the valid ones
    for i in range(2):
        L = int(ylo[i])
        err = (enc[i, :L].cpu() - yo[i, :L]).abs().max().item()
        assert err <= 2e-3 * max(1.0, yo[i, :L].abs().max().item()), (i, err)
    assert _rel(loss, ref) <= 1e-3, (float(loss), float(ref))
    # ---- the full batch of 32 under the optimizer
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("CTC")(cfg)
    tr = Trainer(**cfg["trainer"]).setup(task, dev)
    task.train()
    big = bench.make_batch(0, 32, 10.0, 40, 128, dev)
    losses = [float(tr.training_step(big, i)) for i in range(4)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------------ C4
def _c4_cfg():
    cfg = _c2()
    cfg["task"] = {"type": "CTC_Hybrid_Rnnt", "name": "c4", "export_path": "/tmp"}
    cfg["predictor"] = {"model": "Lstm", "config": {"num_symbols": 128, "output_dim": 256,
                                                    "symbol_embedding_dim": 256, "num_lstm_layers": 2,
                                                    "lstm_hidden_dim": 256, "lstm_layer_norm": True,
                                                    "lstm_layer_norm_epsilon": 1e-3,
                                                    "lstm_dropout": 0.0}}
    cfg["joiner"] = {"input_dim": 256, "output_dim": 128, "inner_dim": 256, "activation": "tanh",
                     "prune_range": -1}
    cfg["loss"] = {"rnnt_weight": 0.8, "ctc_weight": 0.2,
                   "rnnt_loss": {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}},
                   "ctc_loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean"}}}
    return cfg


def test_c4_hybrid_full_size(dev):
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer
    cfg = _c4_cfg()
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("CTC_Hybrid_Rnnt")(cfg)
    task.to(dev).eval()
    batch = bench.make_batch(0, 2, 10.0, 60, 128, dev)
    batch["label_length"][1] = 44
    with torch.no_grad():
        feat, feat_len = task.features(batch)
        enc, enc_len = task._encoder(feat, feat_len)
        dec, dec_len = task._decoder(enc, enc_len)
        pred, pred_len, _ = task._predictor(batch["label"], batch["label_length"],
                                            task._predictor.init_state())
        joint, _, _, _ = task._joiner(enc, enc_len, pred, pred_len)
        l_rnnt = task._rnnt_loss({"logits": joint, "logits_length": enc_len,
                                  "targets": batch["label"], "targets_length": batch["label_length"]})
        l_ctc = task._ctc_loss({"logits": dec, "logits_length": dec_len, "targets": batch["label"],
                                "targets_length": batch["label_length"]})
    assert joint.shape == (2, 248, 61, 128)
    # the joiner (projections, broadcast add, tanh, 2-Linear out-projection) against the oracle
    # joiner on the product's encoder / predictor outputs, then the lattice loss on the ORACLE's
    # lattice
    sd = _cpu_sd(task)
    with torch.no_grad():
        jo = H.joiner_full(sd, "_joiner.", enc.cpu(), pred.cpu(), "tanh")
    assert (joint.cpu() - jo).abs().max().item() <= 2e-4 * max(1.0, jo.abs().max().item())
    ref = K2.rnnt_loss_full(jo, batch["label"].cpu(), enc_len.cpu(), batch["label_length"].cpu())
    assert _rel(l_rnnt, ref) <= 1e-3, (float(l_rnnt), float(ref))
    ref_ctc = torch.nn.functional.ctc_loss(dec.cpu().log_softmax(-1).transpose(0, 1),
                                           batch["label"].cpu(), dec_len.cpu(),
                                           batch["label_length"].cpu(), blank=0, reduction="mean",
                                           zero_infinity=True)
    assert _rel(l_ctc, ref_ctc) <= 1e-3
    # ---- full batch: B = 16, U = 60 (lattice 16 x 248 x 61 x 128)
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("CTC_Hybrid_Rnnt")(cfg)
    tr = Trainer(**cfg["trainer"]).setup(task, dev)
    task.train()
    big = bench.make_batch(0, 16, 10.0, 60, 128, dev)
    losses = [float(tr.training_step(big, i)) for i in range(3)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    lg = {k: float(v) for k, v in task.logged.items()}
    assert abs(lg["train_loss"] - (0.8 * lg["train_loss/loss_rnnt"] + 0.2 * lg["train_loss/loss_ctc"])) \
        <= 1e-4 * abs(lg["train_loss"])


# ------------------------------------------------------------------------------------ C5
def test_c5_bestrq_ssl_full_size(dev):
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer
    from oracle import best_rq as OB
    cfg = _c2()
    cfg["task"] = {"type": "SSL", "name": "c5", "export_path": "/tmp"}
    cfg["ssl_layer"] = {"model": "Best-RQ",
                        "layer_config": {"cnn_kernel_size": [3, 3], "cnn_stride": [2, 2], "feat_dim": 80,
                                         "num_codebooks": 1, "codebook_dim": 16, "codebook_size": 8192,
                                         "label_basis": "cosine"},
                        "masking_config": {"mask_proportion": 0.5, "mean_span_length": 1,
                                           "span_select_type": "static", "min_num_spans": 1,
                                           "no_overlap": False, "min_space": 0, "seed": 1234}}
    cfg["logits_layer"] = {"model": "Projector", "config": {"input_dim": 256, "output_dim": 8193,
                                                           "dropout_p": 0.0}}
    cfg["loss"] = {"loss_select": "mask_loss", "model": "MaskedKLDiv",
                   "config": {"num_classes": 8193, "scale_factor": 1.0, "label_smoothing": 0.1}}
    random.seed(1234)
    np.random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("SSL")(cfg)
    tr = Trainer(**cfg["trainer"]).setup(task, dev)
    task.train()
    batch = bench.make_batch(0, 8, 30.0, 1, 128, dev)       # 30 s clips -> 2998 frames -> 748 labels
    batch["pcm_length"][3] = 400000
    # labels of the quantizer are bit-exact against the oracle on the features the task computes
    with torch.no_grad():
        feat, feat_len = task.features(batch)
        out = task._ssl_layer(feat, feat.clone(), feat_len)
    assert feat.shape == (8, 2998, 80) and out["labels"].shape == (1, 8, 748)
    proj = task._ssl_layer.state_dict()
    pk = [k for k in proj if "project" in k.lower()][0]
    ck = [k for k in proj if "codebook" in k.lower()][0]
    ref = OB.make_labels(feat.cpu().numpy().astype(np.float64), proj[pk].cpu().numpy(),
                         proj[ck].cpu().numpy().reshape(1, 8192, 16))
    lens = OB.label_lengths(feat_len.cpu().numpy())
    got = out["labels"].cpu().numpy()
    for b in range(8):
        assert (got[0, b, :lens[b]] == ref[0, b, :lens[b]]).all(), b     # bit-exact indices
    losses = [float(tr.training_step(batch, i)) for i in range(3)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert 0.3 < float(task.logged["mask_rate"]) < 0.7


def test_c5_conformer_forward_30s_vs_oracle(dev):
    """The C5 encoder at its own length: 1 x 30 s + 1 x 25 s -> 2998 frames -> T = 748 (the
    comparison of the conformer with the oracle otherwise stops at T = 498): Subsampling,
    12 conformer blocks (s2t_mhsa_fwd at T = 748, conv module, LayerNorms) in evaluation mode vs
    oracle/conformer.py on the same parameters and oracle features."""
    from speech2text_amd.build_task import TaskFactory
    cfg = _c2()
    random.seed(1234)
    torch.manual_seed(1234)
    task = TaskFactory.get("CTC")(cfg)
    sd = _cpu_sd(task)
    task.to(dev).eval()
    batch = bench.make_batch(0, 2, 30.0, 1, 128, dev)
    batch["pcm_length"][1] = 400000
    with torch.no_grad():
        feat, feat_len = task.features(batch)
        enc, enc_len = task._encoder(feat, feat_len)
    assert feat.shape == (2, 2998, 80)
    pcm, n = batch["pcm"].cpu().numpy(), batch["pcm_length"].cpu().numpy()
    x = torch.zeros(2, 2998, 80)
    for i in range(2):
        f = ofb.fbank(pcm[i, :n[i]], 80)
        x[i, :f.shape[0]] = torch.from_numpy(f)
    enc_sd = {k[len("_encoder.encoder."):]: v for k, v in sd.items() if k.startswith("_encoder.encoder.")}
    with torch.no_grad():
        yo, ylo = OC.conformer_forward(enc_sd, x, feat_len.cpu(), 12, 4, training=False)
    assert enc.shape == (2, 748, 256) and enc_len.cpu().tolist() == ylo.tolist() == [748, 623]
    for b in range(2):
        L = int(ylo[b])
        err = (enc[b, :L].cpu() - yo[b, :L]).abs().max().item()
        assert err <= 2e-3 * max(1.0, yo[b, :L].abs().max().item()), (b, err)


def test_checkpoint_save_resume_continues_the_trajectory(dev, tmp_path):
    """f4 checkpoint interchange: train 2 steps, save (Lightning layout), train 2 more; a fresh
    task + trainer resumed from the file repeats those 2 steps (same losses, same parameters)."""
    import random
    import bench
    from speech2text_amd import checkpoint as ck
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer

    def make(seed):
        cfg = bench.c3_config(64)
        cfg["encoder"]["config"].update({"downsampling_factor": [1, 2], "num_encoder_layers": [1, 1],
                                         "feedforward_dim": [96, 128], "encoder_dim": [48, 64],
                                         "encoder_unmasked_dim": [32, 48], "num_heads": [4, 4],
                                         "query_head_dim": 8, "value_head_dim": 4, "pos_dim": 16,
                                         "cnn_module_kernel": [15, 7]})
        cfg["predictor"]["config"].update({"output_dim": 64, "symbol_embedding_dim": 32})
        cfg["joiner"].update({"input_dim": 64})
        random.seed(5)
        torch.manual_seed(seed)
        task = TaskFactory.get("Pruned_Rnnt")(cfg)
        tr = Trainer(**cfg["trainer"]).setup(task, dev)
        task.train()
        return task, tr

    def steps(tr, lo, hi):
        out = []
        for i in range(lo, hi):
            batch = bench.make_batch(i, 2, 2.0, 5, 64, dev)
            random.seed(100 + i)
            torch.manual_seed(200 + i)
            out.append(float(tr.training_step(batch, i)))
        return out

    task, tr = make(1234)
    steps(tr, 0, 2)
    path = str(tmp_path / "epoch0.ckpt")
    tracker = ck.BestK(monitor="wer", save_top_k=2, mode="min")
    assert ck.save_checkpoint(tr, path, score=0.5, tracker=tracker)
    lr_at_save = tr.optimizer.param_groups[0]["lr"]
    la = steps(tr, 2, 4)
    torch.cuda.synchronize()
    pa = tr.store.p().detach().cpu().clone()

    saved = torch.load(path, weights_only=False)
    assert saved["global_step"] == 2 and list(saved["callbacks"])[0].startswith("ModelCheckpoint")
    assert all(not v.is_cuda for v in saved["state_dict"].values())

    task2, tr2 = make(999)                                   # different init: the file must win
    ck.resume(tr2, path)
    assert task2.global_step == 2
    assert tr2.optimizer.param_groups[0]["lr"] == pytest.approx(lr_at_save, rel=1e-6)
    lb = steps(tr2, 2, 4)
    torch.cuda.synchronize()
    pb = tr2.store.p().detach().cpu()
    np.testing.assert_allclose(lb, la, rtol=1e-4)
    np.testing.assert_allclose(pb.numpy(), pa.numpy(), rtol=5e-4, atol=2e-5)
    # finetune start: parameters only, by name
    task3, _ = make(7)
    res = ck.load_from_checkpoint(task3, path, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
