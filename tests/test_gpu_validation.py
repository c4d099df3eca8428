"""GPU: every task's validation_step (reference task_factory/ctc_task.py:159-190,
rnnt_task.py:244-284 / 365-420 / 516-594, ssl_task.py:182-254) on a synthetic batch: logged
scalar names, and the metric against the oracle's decoders / a restatement of the reference's
top-k accuracy."""
import copy

import numpy as np
import pytest
import torch

from oracle import decoding as OD
from task_support import _base_cfg, _CONF, _pcm_batch, _pruned_cfg, _refs, _task, _TOK, _V

pytestmark = pytest.mark.gpu


def test_ctc_validation_step_vs_oracle(dev):
    cfg = _base_cfg()
    cfg.update({"task": {"type": "CTC"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Projector", "config": {"input_dim": 64, "output_dim": _V, "dropout_p": 0.1}},
                "loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean", "zero_infinity": True}},
                "metric": {"decode_method": "ctc_greedy_search", "max_token_step": 5}})
    task = _task("CTC", cfg, dev)
    batch = _pcm_batch(dev, V=_V)
    info = task.validation_step(batch, 0)
    assert set(task.logged) >= {"val_loss", "wer"} and np.isfinite(float(info["val_loss"]))
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
        dec, dl = task._decoder(enc, el)
    hyps = [task._tokenizer.decode(torch.tensor(OD.ctc_greedy(dec[b].cpu().numpy(), int(dl[b]))))
            for b in range(dec.shape[0])]
    assert info["wer"] == pytest.approx(OD.word_error_rate(hyps, _refs(task, batch["label"])))
    # training still works after a validation pass (no stale no_grad state, BatchNorm untouched)
    task.train()
    assert task.training_step(batch, 0).requires_grad


def test_pruned_rnnt_validation_step_vs_oracle(dev):
    cfg = _pruned_cfg()
    task = _task("Pruned_Rnnt", cfg, dev)
    with torch.no_grad():
        for p in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            p.mul_(3.0)
    batch = _pcm_batch(dev, V=_V)
    info = task.validation_step(batch, 0)
    assert set(task.logged) >= {"val_loss", "val_loss/simple_loss", "val_loss/pruned_loss",
                                "val_loss/ctc_loss", "wer"}
    assert np.isfinite(float(info["val_loss"]))
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
        dec, dl = task._decoder(enc, el)
    sd = {"p." + k: v.detach().cpu() for k, v in task._predictor.predictor.state_dict().items()}
    sd.update({"j." + k: v.detach().cpu() for k, v in task._joiner.state_dict().items()})
    ctx = cfg["predictor"]["config"]["context_size"]
    hyps = []
    for b in range(dec.shape[0]):
        ids = OD.rnnt_greedy_stateless(sd, "p.", "j.", dec[b].cpu(), int(dl[b]), ctx,
                                       cfg["joiner"].get("activation", "relu"), 1)
        hyps.append(task._tokenizer.decode(torch.tensor(ids, dtype=torch.int64)))
    assert info["wer"] == pytest.approx(OD.word_error_rate(hyps, _refs(task, batch["label"])))


def test_hybrid_and_rnnt_validation_steps(dev):
    cfg = _base_cfg()
    cfg.update({"task": {"type": "CTC_Hybrid_Rnnt"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Projector", "config": {"input_dim": 64, "output_dim": _V, "dropout_p": 0.1}},
                "predictor": {"model": "Lstm", "config": {"num_symbols": _V, "output_dim": 64,
                                                          "symbol_embedding_dim": 32, "num_lstm_layers": 2,
                                                          "lstm_hidden_dim": 48, "lstm_layer_norm": True,
                                                          "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.1}},
                "joiner": {"input_dim": 64, "output_dim": _V, "inner_dim": 48, "activation": "tanh",
                           "prune_range": -1},
                "metric": {"decode_method": "rnnt_greedy_search", "max_token_step": 2},
                "loss": {"rnnt_weight": 0.8, "ctc_weight": 0.2,
                         "rnnt_loss": {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}},
                         "ctc_loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean"}}}})
    batch = _pcm_batch(dev, B=2, sec=1.0, V=_V)
    task = _task("CTC_Hybrid_Rnnt", cfg, dev)
    info = task.validation_step(batch, 0)
    assert set(task.logged) >= {"val_loss", "val_loss/loss_rnnt", "val_loss/loss_ctc", "wer"}
    assert float(info["val_loss"]) == pytest.approx(
        0.8 * float(info["val_loss/loss_rnnt"]) + 0.2 * float(info["val_loss/loss_ctc"]), rel=1e-5)
    # the LSTM predictor takes the reference's per-utterance lattice walk (model/decoding.py:237-271):
    # the task's WER must equal the one of hypotheses decoded one utterance at a time
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
    sess = task._metric._decode_sess
    hyps = [sess.decode(enc[b:b + 1, :int(el[b])]) for b in range(enc.shape[0])]
    assert info["wer"] == pytest.approx(OD.word_error_rate(hyps, _refs(task, batch["label"])))
    cfg2 = copy.deepcopy(cfg)
    cfg2["task"] = {"type": "Rnnt"}
    cfg2["decoder"] = {"model": "Identity", "config": {"dummy": -1}}
    cfg2["loss"] = {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}}
    task2 = _task("Rnnt", cfg2, dev)
    info2 = task2.validation_step(batch, 0)
    assert set(task2.logged) >= {"val_loss", "wer"} and np.isfinite(float(info2["val_loss"]))


def _ref_topk_acc(logits, labels, masked_dim, k):
    """reference model/utils.py:153-181, restated in numpy."""
    top = np.argsort(-logits, axis=-1, kind="stable")[..., :k]
    top = np.where((1 - masked_dim)[..., None].astype(bool), -1, top)
    valid = (masked_dim * labels)[..., None]
    return float((top == valid).sum() / (masked_dim.sum() + 1e-7))


def test_ssl_validation_step_topk(dev):
    cfg = _base_cfg()
    cfg.update({"task": {"type": "SSL"}, "encoder": _CONF, "metric": {"top_ks": [1, 5]},
                "ssl_layer": {"model": "Best-RQ",
                              "layer_config": {"cnn_kernel_size": [3, 3], "cnn_stride": [2, 2], "feat_dim": 80,
                                               "num_codebooks": 2, "codebook_dim": 16, "codebook_size": 256,
                                               "label_basis": "cosine"},
                              "masking_config": {"mask_proportion": 0.5, "mean_span_length": 1,
                                                 "span_select_type": "static", "min_num_spans": 1,
                                                 "no_overlap": False, "min_space": 0, "seed": 1234}},
                "logits_layer": {"model": "Projector", "config": {"input_dim": 64, "output_dim": 257, "dropout_p": 0.0}},
                "loss": {"loss_select": "mask_loss", "model": "MaskedKLDiv",
                         "config": {"num_classes": 257, "scale_factor": 1.0, "label_smoothing": 0.1}}})
    task = _task("SSL", cfg, dev)
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(3, 203, 80, generator=g).to(dev)
    batch = {"raw_feat": feats, "auged_feat": feats.clone(), "feat_length": torch.tensor([203, 180, 151]).to(dev)}
    info = task.validation_step(batch, 0)
    assert set(task.logged) >= {"val_loss", "val_loss/tot_loss", "val_loss/mask_loss", "top_1_acc", "top_5_acc"}
    assert float(info["val_loss"]) == pytest.approx(float(info["val_loss/mask_loss"]))
    assert 0.0 <= float(info["top_1_acc"]) <= float(info["top_5_acc"]) <= 1.0
    # the metric itself against the reference's formula on random logits
    from speech2text_amd.model.utils import SslMetric, SslMetricConfig
    rng = np.random.default_rng(0)
    lg = rng.standard_normal((3, 17, 40)).astype(np.float32)
    lab = rng.integers(1, 40, (3, 17))
    md = (rng.random((3, 17)) < 0.5).astype(np.float32)
    m = SslMetric(SslMetricConfig(top_ks=(1, 5)))(torch.from_numpy(lg).to(dev), torch.from_numpy(lab).to(dev),
                                                   torch.from_numpy(md).to(dev))
    for k in (1, 5):
        assert float(m[f"top_{k}_acc"]) == pytest.approx(_ref_topk_acc(lg, lab, md, k), rel=1e-6)


def test_trainer_fit_runs_validation_passes(dev):
    """Trainer.fit(..., val_batches=...) (reference: Lightning's validation loop at val_check_interval):
    a float interval is a fraction of the training epoch, an int a number of training batches; every
    pass leaves one dict of batch-averaged metrics in val_history, the task is back in training mode
    afterwards and training continues."""
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer
    cfg = _base_cfg()
    cfg.update({"task": {"type": "CTC"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Projector", "config": {"input_dim": 64, "output_dim": _V, "dropout_p": 0.1}},
                "loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean", "zero_infinity": True}},
                "metric": {"decode_method": "ctc_greedy_search", "max_token_step": 5}})
    cfg["trainer"].update({"max_epochs": 2, "accumulate_grad_batches": 1, "val_check_interval": 0.5})
    torch.manual_seed(0)
    task = TaskFactory.get("CTC")(cfg)
    trainer = Trainer(**cfg["trainer"])
    batch = _pcm_batch(dev, V=_V)
    trainer.fit(task, [batch] * 4, device=dev, val_batches=[batch, batch])
    assert len(trainer.val_history) == 4                      # twice per epoch, two epochs
    for h in trainer.val_history:
        assert {"val_loss", "wer", "epoch", "global_step"} <= set(h) and np.isfinite(h["val_loss"])
    assert [h["global_step"] for h in trainer.val_history] == [2, 4, 6, 8]
    assert trainer.val_history[-1]["val_loss"] < trainer.val_history[0]["val_loss"]
    assert task.training
    # an integer interval counts training batches; a pass is added at the end of an epoch that had none
    trainer2 = Trainer(**dict(cfg["trainer"], max_epochs=1, val_check_interval=3))
    trainer2.fit(TaskFactory.get("CTC")(cfg), [batch] * 4, device=dev, val_batches=[batch])
    assert [h["global_step"] for h in trainer2.val_history] == [3, 4]


def test_run_task_checkpoints_resume_and_finetune(dev, tmp_path):
    """run_task as the reference's (build_task.py:44-148) around the accelerated path: validation at
    val_check_interval, ModelCheckpoint's top-k table on the monitored metric (files that fall out
    are removed), `resume` continues the counters and the optimizer, `finetune.base_model` = the
    checkpoint DIRECTORY starts from the average of its top-k files."""
    import glob
    import os
    from speech2text_amd import build_task
    cfg = _base_cfg()
    cfg.update({"task": {"type": "CTC"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Projector", "config": {"input_dim": 64, "output_dim": _V, "dropout_p": 0.1}},
                "loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean", "zero_infinity": True}},
                "metric": {"decode_method": "ctc_greedy_search", "max_token_step": 5},
                "callbacks": {"model_chkpt_config": {"monitor": "val_loss", "mode": "min", "save_top_k": 2}},
                "finetune": {"base_model": None}, "resume": None})
    cfg["trainer"].update({"max_epochs": 3, "accumulate_grad_batches": 1, "val_check_interval": 1.0})
    batch = _pcm_batch(dev, V=_V)
    exp = str(tmp_path / "exp")
    task, trainer = build_task.run_task(cfg, [batch] * 3, [batch], export_dir=exp, name="ctc")
    files = sorted(glob.glob(os.path.join(exp, "checkpoints", "*.ckpt")))
    assert len(trainer.val_history) == 3 and len(files) == 2          # top-2 of three passes
    assert all(os.path.basename(f).startswith("ctc-epoch=") and "val_loss=" in f for f in files)
    ck = torch.load(max(files, key=os.path.getctime), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 9 and len(next(iter(ck["callbacks"].values()))["best_k_models"]) == 2
    assert set(ck["state_dict"]) == set(task.state_dict())
    # the reference's file name template always carries the monitor field (build_task.py:94-95)
    assert all(os.path.basename(f).count("val_loss=") == 2 for f in files)
    # resume (Lightning's fit(ckpt_path=...)): counters, optimizer state AND the epoch loop continue
    # -- the epoch-2 file resumed with max_epochs 4 trains exactly one more epoch (epoch 3), the
    # top-k table of the resumed file stays in force (2 files on disk, the old worst one evicted)
    cfg2 = copy.deepcopy(cfg)
    cfg2["resume"] = max(files, key=os.path.getctime)
    cfg2["trainer"]["max_epochs"] = 4
    task2, trainer2 = build_task.run_task(cfg2, [batch] * 3, [batch], export_dir=exp, name="ctc")
    assert task2.global_step == 12 and task2.current_epoch == 3
    assert [h["global_step"] for h in trainer2.val_history] == [12]
    assert trainer2.val_history[-1]["val_loss"] < trainer.val_history[0]["val_loss"]
    files2 = sorted(glob.glob(os.path.join(exp, "checkpoints", "*.ckpt")))
    assert len(files2) == 2 and any("epoch=3" in os.path.basename(f) for f in files2)
    ck2 = torch.load(max(files2, key=os.path.getctime), map_location="cpu", weights_only=False)
    assert set(next(iter(ck2["callbacks"].values()))["best_k_models"]) == set(files2)
    # resuming a finished run trains nothing
    cfg2b = copy.deepcopy(cfg2)
    cfg2b["trainer"]["max_epochs"] = 3
    task2b, trainer2b = build_task.run_task(cfg2b, [batch] * 3, [batch])
    assert task2b.global_step == 9 and trainer2b.val_history == []
    # finetune from the directory: the average of the top-k files is written and loaded
    cfg3 = copy.deepcopy(cfg)
    cfg3["finetune"]["base_model"] = os.path.join(exp, "checkpoints")
    cfg3["trainer"]["max_epochs"] = 1
    task3, trainer3 = build_task.run_task(cfg3, [batch], [batch])
    assert os.path.exists(os.path.join(exp, "checkpoints", "averaged.chkpt"))
    assert task3.global_step == 1 and trainer3.val_history[0]["val_loss"] < trainer.val_history[0]["val_loss"]
