"""Task and configuration builders shared by the task-level tests.

Test infrastructure (not a test file): what one test module used to take from another.  Module
builders and chunk drivers are in tests/decode_support.py.
"""
import os
import socket

import torch
import yaml


def _base_cfg(feat_type="fbank"):
    return {"dataset": {"feat_type": feat_type,
                        "feat_config": {"num_mel_bins": 80, "frame_length": 25, "frame_shift": 10,
                                        "dither": 0.0} if feat_type == "fbank" else
                        {"num_mel_bins": 80, "snip_edges": True}},
            "optim_setup": {"seperate_lr": {"apply": False},
                            "optimizer": {"type": "ScaledAdam", "config": {"lr": 0.045, "clipping_scale": 2.0}},
                            "lr_scheduler": {"type": "Eden", "config": {"lr_batches": 7000},
                                             "step_config": {"interval": "step", "frequency": 1}}},
            "trainer": {"accelerator": "gpu", "devices": 1, "strategy": "ddp", "precision": "32-true",
                        "max_epochs": 1, "accumulate_grad_batches": 2, "gradient_clip_val": 5.0,
                        "gradient_clip_algorithm": "norm"}}


_CONF = {"model": "Conformer", "config": {"bn_cmvn": False, "feats_dim": 80, "subsampling_rate": 4,
                                          "input_dim": 64, "num_heads": 4, "ffn_dim": 128,
                                          "num_layers": 2, "depthwise_conv_kernel_size": 15,
                                          "dropout": 0.1, "output_dim": 64}}


def _pcm_batch(dev, B=3, sec=2.0, U=6, V=32):
    g = torch.Generator().manual_seed(1)
    n = int(sec * 16000)
    return {"pcm": (torch.randn(B, n, generator=g) * 0.1).to(dev),
            "pcm_length": torch.tensor([n, n - 3000, n - 8000][:B]).to(dev),
            "label": torch.randint(1, V - 1, (B, U), generator=g).to(dev),
            "label_length": torch.tensor([U, U - 1, U - 3][:B]).to(dev)}


_V = 32
_TOK = {"type": "char", "config": {"labels": [chr(97 + i) for i in range(_V - 3)]}}


def _task(name, cfg, dev):
    from speech2text_amd.build_task import TaskFactory
    torch.manual_seed(0)
    task = TaskFactory.get(name)(cfg).to(dev)
    task.eval()
    return task


def _refs(task, labels):
    from speech2text_amd.model.decoding import reference_decoder
    return reference_decoder(labels, task._tokenizer)


def _pruned_cfg():
    import bench
    cfg = bench.c3_config(_V)
    cfg["encoder"]["config"].update({"downsampling_factor": [1, 2], "num_encoder_layers": [1, 1],
                                     "feedforward_dim": [96, 128], "encoder_dim": [48, 64],
                                     "encoder_unmasked_dim": [32, 48], "num_heads": [4, 4],
                                     "query_head_dim": 8, "value_head_dim": 4, "pos_dim": 16,
                                     "cnn_module_kernel": [15, 7], "chunk_size": [-1],
                                     "left_context_frames": [-1]})
    cfg["predictor"]["config"].update({"output_dim": 64, "symbol_embedding_dim": 32})
    cfg["joiner"].update({"input_dim": 64})
    cfg["tokenizer"] = _TOK
    cfg["metric"] = {"decode_method": "rnnt_greedy_search", "max_token_step": 1}
    return cfg


def _pruned_beam_cfg(V):
    """A tiny Pruned_Rnnt task: the construction of _pruned_cfg for any vocabulary, with the beam search as its metric."""
    import bench
    cfg = bench.c3_config(V)
    cfg["encoder"]["config"].update({"downsampling_factor": [1, 2], "num_encoder_layers": [1, 1],
                                     "feedforward_dim": [96, 128], "encoder_dim": [48, 64],
                                     "encoder_unmasked_dim": [32, 48], "num_heads": [4, 4],
                                     "query_head_dim": 8, "value_head_dim": 4, "pos_dim": 16,
                                     "cnn_module_kernel": [15, 7], "chunk_size": [-1],
                                     "left_context_frames": [-1]})
    cfg["predictor"]["config"].update({"output_dim": 64, "symbol_embedding_dim": 32})
    cfg["joiner"].update({"input_dim": 64})
    cfg["tokenizer"] = {"type": "char", "config": {"labels": [chr(97 + i) for i in range(V - 3)]}}
    cfg["metric"] = {"decode_method": "rnnt_beam_search", "beam_size": 3, "cutoff_top_k": 2}
    return cfg


def _ctc_cfg(golden_dir):
    root = os.path.join(golden_dir, "reference_configs")
    cfg = yaml.safe_load(open(os.path.join(root, "config", "training", "conformer_ctc.yaml")))
    for k in ("spm_model", "spm_vocab"):
        cfg["tokenizer"]["config"][k] = os.path.join(root, cfg["tokenizer"]["config"][k])
    cfg["encoder"]["config"].update({"input_dim": 64, "ffn_dim": 128, "num_layers": 2, "output_dim": 64,
                                     "depthwise_conv_kernel_size": 15})
    cfg["decoder"]["config"]["input_dim"] = 64
    return cfg, cfg["decoder"]["config"]["output_dim"]


def _ctc_zipformer_cfg(V, chunk):
    cfg = _pruned_beam_cfg(V)
    for k in ("predictor", "joiner"):
        cfg.pop(k)
    cfg["task"]["type"] = "CTC"
    cfg["encoder"]["config"].update({"chunk_size": [chunk], "left_context_frames": [16]})
    cfg["decoder"] = {"model": "Projector", "config": {"input_dim": 64, "output_dim": V, "dropout_p": 0.1}}
    cfg["loss"] = {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean"}}
    cfg["metric"] = {"decode_method": "ctc_prefix_beam_search", "beam_size": 3, "cutoff_top_k": 2, "lm_weight": 0.5,
                     "lm_start_token": V - 1,
                     "lm": {"config": {"num_symbols": V, "symbol_embedding_dim": 16, "num_rnn_layer": 1},
                            "checkpoint": None}}
    return cfg


def _rnnt_cfg():
    cfg = _base_cfg()
    cfg.update({"task": {"type": "Rnnt"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Identity", "config": {"dummy": -1}},
                "predictor": {"model": "Lstm", "config": {"num_symbols": _V, "output_dim": 64,
                                                          "symbol_embedding_dim": 32, "num_lstm_layers": 2,
                                                          "lstm_hidden_dim": 48, "lstm_layer_norm": True,
                                                          "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.1}},
                "joiner": {"input_dim": 64, "output_dim": _V, "inner_dim": 48, "activation": "tanh",
                           "prune_range": -1},
                "metric": {"decode_method": "rnnt_beam_search", "beam_size": 3, "cutoff_top_k": 3},
                "loss": {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}}})
    return cfg, _V


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p
