"""CTC task (reference task_factory/ctc_task.py:32-227): cmvn -> encoder -> decoder -> CTC."""
import torch
import torch.nn.functional as F

from speech2text_amd.model.decoder.decoder import Decoder
from speech2text_amd.model.encoder.encoder import Encoder
from speech2text_amd.model.loss.loss import Loss
from speech2text_amd.task_factory.base import TaskBase


class CtcTask(TaskBase):
    def __init__(self, config) -> None:
        super().__init__(config)
        self._encoder = Encoder(config["encoder"])
        self._decoder = Decoder(config["decoder"])
        self._loss = Loss(config["loss"])
        self._metric = self._asr_metric()

    def _optimizer_params(self):
        """reference ctc_task.py:201-213: encoder / decoder groups under seperate_lr."""
        sep = self._optim_config["seperate_lr"]
        if sep["apply"]:
            c = sep["config"]
            return [{"params": self._encoder.parameters(), "name": "encoder_lr", "lr": c["encoder_lr"]},
                    {"params": self._decoder.parameters(), "name": "decoder_lr", "lr": c["decoder_lr"]}]
        return self.parameters()

    def training_step(self, batch, batch_idx):
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        loss = self._loss({"logits": dec, "logits_length": dec_len, "targets": batch["label"],
                           "targets_length": batch["label_length"]})
        self.log("train_loss", loss, sync_dist=True, prog_bar=True, logger=True)
        return loss.mean()

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """reference ctc_task.py:159-190: loss + greedy-search WER on log-softmax of the head."""
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        loss = self._loss({"logits": dec, "logits_length": dec_len, "targets": batch["label"],
                           "targets_length": batch["label_length"]})
        wer = self._wer(F.log_softmax(dec, dim=-1), dec_len, batch["label"])
        self.log_dict({"val_loss": loss, "wer": wer}, sync_dist=True, prog_bar=True)
        return {"val_loss": loss, "wer": wer}

    @torch.no_grad()
    def align(self, batch, frame_seconds=None):
        """Forced alignment of batch["label"] / batch["label_length"] against this task's own logits
        (features -> encoder -> decoder -> model/alignment.py CtcForcedAligner): one Alignment per
        utterance with token spans in frames of the head's output, words where the task has a tokenizer,
        and seconds where frame_seconds (the duration of one output frame) is given."""
        from speech2text_amd.model.alignment import CtcForcedAligner
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        aligner = CtcForcedAligner(self._tokenizer, blank=0, frame_seconds=frame_seconds)
        return aligner.align(dec, dec_len, batch["label"].to(dec.device), batch["label_length"].to(dec.device))

    def streaming_recognizer(self, batch_size=1, method=None, **kw):
        """A CtcStreamingRecognizer (model/encoder/zipformer_streaming.py) over this task's encoder, CTC
        head, tokenizer and global CMVN: features in, text out, a chunk at a time.  method ("greedy" |
        "beam") comes from the `metric:` section's decode_method when not given (ctc_greedy_search /
        ctc_prefix_beam_search), beam_size and cutoff_top_k from there too, and with `metric.lm` and the
        beam method the search is shallow-fused with that LM (`metric.lm_weight`,
        `metric.lm_start_token`), as the validation search is; an ARPA `metric.lm` is not taken by default
        (a ValueError): pass lm=<NgramLm>, lm_weight= explicitly for the fused n-gram search
        (CtcNgramStreamingSearch).  With `metric.hotwords` and the beam method the search is biased with
        those phrases (CtcBiasStreamingSearch; context=, context_weight= override).  The task must be on the GPU and in eval
        mode; its head is the encoder's own projection (for_ctc, Identity decoder) or the Projector."""
        from speech2text_amd.model.decoder.decoder import Identity, Projector
        from speech2text_amd.model.encoder.zipformer_streaming import CtcStreamingRecognizer
        from speech2text_amd.model.utils import AsrMetricConfig
        if self._tokenizer is None:
            raise RuntimeError("streaming_recognizer needs the YAML's `tokenizer:` section")
        head = self._decoder.decoder
        if isinstance(head, Identity):
            head = None
        elif not isinstance(head, Projector):
            raise NotImplementedError("streaming_recognizer serves the Identity and Projector decoders only")
        cfg = AsrMetricConfig(**(self._metric_config or {}))
        if method is None:
            method = {"ctc_prefix_beam_search": "beam", "ctc_greedy_search": "greedy"}.get(cfg.decode_method)
            if method is None:
                raise ValueError(f"metric decode_method {cfg.decode_method!r} names no CTC search: pass method=")
        for k in ("beam_size", "cutoff_top_k"):
            kw.setdefault(k, getattr(cfg, k))
        if method == "beam" and "lm" not in kw:            # the LM the validation search is fused with
            lm = self._metric_lm()
            from speech2text_amd.model.lm.ngram_lm import NgramLm
            if isinstance(lm, NgramLm):
                raise ValueError("metric.lm names an ARPA n-gram: pass it as lm=<NgramLm> (and lm_weight=) to "
                                 "stream with CtcNgramStreamingSearch, or lm=None / an RnnLm to stream without it")
            if lm is not None:
                kw["lm"] = lm
                kw.setdefault("lm_weight", cfg.lm_weight)
                kw.setdefault("lm_start_token", cfg.lm_start_token)
        if method == "beam" and "context" not in kw:       # the hotwords the validation search is biased with
            for k, v in self._metric_context().items():
                kw.setdefault(k, v)
        return CtcStreamingRecognizer(self._encoder, self._tokenizer, head=head, cmvn=self._global_cmvn,
                                      batch_size=batch_size, method=method, **kw)
