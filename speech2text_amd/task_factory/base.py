"""Task plumbing shared by the *_task modules.

The reference tasks are pytorch_lightning.LightningModules driven by pl.Trainer
(build_task.py:143-148).  Lightning is not part of this stack: `TaskBase` keeps the subset of
the LightningModule surface the reference's tasks use on the training path (training_step,
configure_optimizers, log / log_dict, current_epoch / global_step) and speech2text_amd.trainer
drives it.  Data loading, tokenisers and decoding metrics are outside the accelerated path
(SURVEY.md section 8f); tasks accept batches that already follow the reference's batch-dict
contract (dataset/utils.py:182-202) or carry raw PCM for the on-GPU frontend.
"""
import copy

import torch
import torch.nn as nn

from speech2text_amd.dataset.frontend.frontend import FeatType
from speech2text_amd.model.layer.global_cmvn import GlobalCmvnLayer


class TaskBase(nn.Module):
    def __init__(self, config) -> None:
        super().__init__()
        self._dataset_config = config["dataset"]
        self._optim_config = config.get("optim_setup")
        # the reference builds the tokenizer unconditionally (ctc_task.py:49); synthetic-batch
        # harnesses (bench.py) carry token ids and no tokenizer section
        self._tokenizer = None
        if config.get("tokenizer") is not None:
            from speech2text_amd.dataset.utils import TokenizerSetup
            self._tokenizer = TokenizerSetup(config["tokenizer"])
        self._metric_config = config.get("metric")
        self._metric_lm_config = None
        if self._metric_config is not None and "lm" in self._metric_config:
            # metric: {lm: {config: {<RnnLmConfig>}, checkpoint: <path|null>}}: the language model the
            # beam searches are shallow-fused with, or {lm: {arpa: <path>, missing_logp: ..}}: a back-off
            # n-gram over the tokenizer's pieces (CTC prefix beam search); the rest is AsrMetricConfig's
            self._metric_config = dict(self._metric_config)
            self._metric_lm_config = self._metric_config.pop("lm")
        self._metric_hotwords_config = None
        if self._metric_config is not None and "hotwords" in self._metric_config:
            # metric: {hotwords: {phrases: [...] | file: <one phrase a line>, context_score:, context_weight:}}:
            # the phrases the CTC prefix beam search is biased towards (model/lm/context_graph.py)
            self._metric_config = dict(self._metric_config)
            self._metric_hotwords_config = self._metric_config.pop("hotwords")
        self._metric = None
        if "feat_type" in self._dataset_config:
            self._frontend = self._get_frontend(copy.deepcopy(config["dataset"]))
            self._global_cmvn = GlobalCmvnLayer(config=self._dataset_config)
        else:       # a text task (NNLM): its dataset section describes no acoustic features
            self._frontend = None
            self._global_cmvn = None
        self.logged = {}
        self.current_epoch = 0
        self.global_step = 0

    @staticmethod
    def _get_frontend(config):
        if config["feat_type"] == "fbank":
            config["feat_config"]["dither"] = 0.0
        return FeatType[config["feat_type"]].value(**config["feat_config"])

    # ---- Lightning-like logging hooks (values are reduced by the trainer)
    def log(self, name, value, **kwargs):
        self.logged[name] = value

    def log_dict(self, d, **kwargs):
        self.logged.update(d)

    # ---- features: reference contract ("feat"/"feat_length") or raw PCM on the GPU
    def features(self, batch):
        if "feat" in batch:
            return self._global_cmvn(batch["feat"]), batch["feat_length"]
        pcm, n = batch["pcm"], batch["pcm_length"]
        mean = getattr(self._global_cmvn, "global_mean", None)
        istd = getattr(self._global_cmvn, "global_istd", None)
        feats, frames = self._frontend.forward_batch(pcm, n, mean, istd)
        return feats, frames

    def audio_streaming_recognizer(self, batch_size=1, max_chunk_samples=5120, **kw):
        """An AudioStreamingRecognizer (model/encoder/zipformer_audio_streaming.py): audio in arbitrary
        cuts of at most max_chunk_samples samples in, text out, over this task's own frontend and its
        `streaming_recognizer(batch_size, **kw)` (the CTC and RNN-T tasks have one)."""
        from speech2text_amd.model.encoder.zipformer_audio_streaming import AudioStreamingRecognizer
        if not hasattr(self, "streaming_recognizer"):
            raise NotImplementedError(f"{type(self).__name__} has no streaming_recognizer to put audio in front of")
        if self._frontend is None:
            raise RuntimeError("audio_streaming_recognizer needs the YAML's `dataset:` feat_type / feat_config")
        return AudioStreamingRecognizer(self.streaming_recognizer(batch_size=batch_size, **kw),
                                        self._frontend, max_chunk_samples=max_chunk_samples)

    def _asr_metric(self, predictor=None, joiner=None):
        """AsrMetric of the YAML's `metric:` section (reference ctc_task.py:56-57,
        rnnt_task.py:65-69), or None when the config carries no tokenizer / metric."""
        if self._tokenizer is None or self._metric_config is None:
            return None
        from speech2text_amd.model.utils import AsrMetric, AsrMetricConfig
        return AsrMetric(tokenizer=self._tokenizer, config=AsrMetricConfig(**self._metric_config),
                         predictor=predictor, joiner=joiner, lm=self._metric_lm(), **self._metric_context())

    def _metric_context(self):
        """The hotword arguments of `metric.hotwords` -> {} without the key, else {context: the ContextGraph
        of the phrases (`phrases:` a list, or `file:` with one phrase a line) encoded with the task's
        tokenizer, context_weight:}.  Like the LM it is handed to the metric object or the recogniser,
        never held by the task."""
        cfg = self._metric_hotwords_config
        if not cfg:
            return {}
        if self._tokenizer is None:
            raise RuntimeError("metric.hotwords needs the YAML's `tokenizer:` section: the phrases are encoded with it")
        if (cfg.get("phrases") is None) == (cfg.get("file") is None):
            raise ValueError("metric.hotwords names either `phrases:` (a list) or `file:` (one phrase a line)")
        phrases = cfg.get("phrases")
        if phrases is None:
            with open(cfg["file"], encoding="utf-8") as fh:
                phrases = [line.strip() for line in fh if line.strip()]
        from speech2text_amd.model.lm.context_graph import ContextGraph
        graph = ContextGraph.from_texts(list(phrases), self._tokenizer,
                                        context_score=float(cfg.get("context_score", 1.0)))
        return dict(context=graph, context_weight=float(cfg.get("context_weight", 1.0)))

    def _metric_lm(self):
        """The frozen RnnLm of `metric.lm`, or None: built from `lm.config`, loaded from the `_nnlm.*`
        keys of a checkpoint the NNLM task wrote when `lm.checkpoint` names one.  With `lm.arpa` instead
        the NgramLm of that ARPA file over the task's tokenizer (`lm.missing_logp` for a class without
        a unigram).  The caller hands it
        to the metric object; it is never an attribute of the task, so the task's state_dict(),
        parameters() and optimizer groups do not know it.  It follows the inputs to their device on
        first use (model/decoding.py)."""
        if not self._metric_lm_config:
            return None
        if self._metric_lm_config.get("arpa"):
            from speech2text_amd.model.lm.ngram_lm import NgramLm
            if self._metric_lm_config.get("config") or self._metric_lm_config.get("checkpoint"):
                raise ValueError("metric.lm names either an ARPA n-gram (arpa:) or an RNN LM (config:, checkpoint:)")
            if self._tokenizer is None:
                raise RuntimeError("metric.lm.arpa needs the YAML's `tokenizer:` section: its pieces are the words")
            return NgramLm.from_arpa(self._metric_lm_config["arpa"], tokenizer=self._tokenizer,
                                     missing_logp=self._metric_lm_config.get("missing_logp", -30.0))
        from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
        with torch.random.fork_rng(devices=[]):            # its init draws nothing from the task's stream
            lm = RnnLm(config=RnnLmConfig(**(self._metric_lm_config.get("config") or {})))
        path = self._metric_lm_config.get("checkpoint")
        if path:
            sd = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
            lm.load_state_dict({k[len("_nnlm."):]: v for k, v in sd.items() if k.startswith("_nnlm.")},
                               strict=True)
        return lm.eval().requires_grad_(False)

    def _wer(self, hidden_states, lengths, labels):
        if self._metric is None:
            raise RuntimeError("validation_step needs the YAML's `tokenizer:` and `metric:` sections "
                               "(reference task_factory/ctc_task.py:39-57)")
        return self._metric(hidden_states, lengths, labels)

    def configure_optimizers(self):
        from speech2text_amd.optimizer.optim_setup import OptimSetup
        Optimizer, LR_Scheduler = OptimSetup(self._optim_config)
        optimizer = Optimizer(self._optimizer_params(), **self._optim_config["optimizer"]["config"])
        sched = LR_Scheduler(optimizer=optimizer, **self._optim_config["lr_scheduler"]["config"])
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": sched,
                                 **self._optim_config["lr_scheduler"]["step_config"]}}

    def _optimizer_params(self):
        return self.parameters()
