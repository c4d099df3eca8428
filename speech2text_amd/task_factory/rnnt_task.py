"""RNN-T family tasks (reference task_factory/rnnt_task.py): the per-step call sequence
cmvn -> encoder -> decoder -> predictor -> joiner -> loss and the loss-combination formulas
(:349, :496-499) with the same attribute names (state_dict prefixes) and logged scalars."""
import torch

from speech2text_amd.model.decoder.decoder import Decoder
from speech2text_amd.model.encoder.encoder import Encoder
from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
from speech2text_amd.model.loss.loss import Loss
from speech2text_amd.model.predictor.predictor import Predictor
from speech2text_amd.task_factory.base import TaskBase


class BaseRnntTask(TaskBase):
    def __init__(self, config) -> None:
        super().__init__(config)
        self._encoder = Encoder(config["encoder"])
        self._decoder = Decoder(config["decoder"])
        self._predictor = Predictor(config["predictor"])
        self._joiner = Joiner(config=JoinerConfig(**config["joiner"]))
        # reference rnnt_task.py:65-69: the metric decodes with this task's predictor / joiner
        self._metric = self._asr_metric(predictor=self._predictor, joiner=self._joiner)

    def _optimizer_params(self):
        sep = self._optim_config["seperate_lr"]
        if sep["apply"]:
            c = sep["config"]
            return [{"params": self._encoder.parameters(), "name": "encoder_lr", "lr": c["encoder_lr"]},
                    {"params": self._decoder.parameters(), "name": "decoder_lr", "lr": c["decoder_lr"]},
                    {"params": self._predictor.parameters(), "name": "predictor_lr", "lr": c["predictor_lr"]},
                    {"params": self._joiner.parameters(), "name": "joiner_lr", "lr": c["joiner_lr"]}]
        return self.parameters()

    # what the joiner's encoder projection takes in this task's training step: decoder_out, or
    # encoder_out where the decoder is the CTC head (CtcHybridRnnt)
    _JOINS_ENCODER_OUT = False

    def _align_rnnt_type(self) -> str:
        """The lattice this task trains on: regular unless the loss configuration says otherwise."""
        return "regular"

    @torch.no_grad()
    def align(self, batch, frame_seconds=None):
        """Forced alignment of batch["label"] / batch["label_length"] on the frames of this task's own
        RNN-T (features -> encoder -> decoder, then model/alignment.py RnntForcedAligner over the predictor
        and the joiner): one Alignment per utterance; every token is emitted at one frame (begin, end =
        begin + 1), words where the task has a tokenizer, seconds where frame_seconds (the duration of one
        joiner input frame) is given.  The lattice is the one the task's loss trains on; a delay penalty is
        a training device and never enters."""
        from speech2text_amd.model.alignment import RnntForcedAligner
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        x, n = (enc, enc_len) if self._JOINS_ENCODER_OUT else (dec, dec_len)
        aligner = RnntForcedAligner(self._predictor, self._joiner, self._tokenizer, blank=self._joiner.blank_token,
                                    frame_seconds=frame_seconds, rnnt_type=self._align_rnnt_type())
        return aligner.align(x, n, batch["label"].to(x.device), batch["label_length"].to(x.device))

    def streaming_recognizer(self, batch_size=1, method=None, **kw):
        """A StreamingRecognizer (model/encoder/zipformer_streaming.py) over this task's encoder,
        predictor, joiner, tokenizer and global CMVN: features in, text out, a chunk at a time.
        method ("greedy" | "beam"), max_token_step, beam_size and cutoff_top_k come from the task's
        `metric:` section when not given.  The task must be on the GPU and in eval mode; its decoder
        must be the identity (the search reads the encoder output through joiner._enc_proj), or the task is
        CtcHybridRnnt, whose RNN-T branch joins the encoder output beside its CTC head.  The
        search is the one that serves the task's predictor (model/decoding.py rnnt_streaming_search):
        stateless with a projection-free joiner, or `predictor.model: Lstm` with either joiner.  With
        `metric.lm` and the beam method the search is shallow-fused with that LM (`metric.lm_weight`,
        `metric.lm_start_token`), as the validation search is; the stateless predictor then takes
        either joiner.  `metric.lm: {arpa:}` (an NgramLm) builds RnntNgramStreamingSearch for the stateless
        predictor with a projection-free joiner and RnntLstmNgramStreamingSearch for the LSTM predictor
        (no `metric.lm_start_token` with either).  With `metric.hotwords` and the beam method the search is biased
        with those phrases (RnntBiasStreamingSearch; context=, context_weight= override)."""
        from speech2text_amd.model.decoder.decoder import Identity
        from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
        from speech2text_amd.model.utils import AsrMetricConfig
        if self._tokenizer is None:
            raise RuntimeError("streaming_recognizer needs the YAML's `tokenizer:` section")
        if not (self._JOINS_ENCODER_OUT or isinstance(self._decoder.decoder, Identity)):
            raise NotImplementedError("streaming_recognizer serves the Identity decoder only (and CtcHybridRnnt, whose "
                                      "RNN-T branch joins the encoder output itself)")
        cfg = AsrMetricConfig(**(self._metric_config or {}))
        if method is None:
            method = {"rnnt_beam_search": "beam", "rnnt_greedy_search": "greedy"}.get(cfg.decode_method)
            if method is None:
                raise ValueError(f"metric decode_method {cfg.decode_method!r} names no RNN-T search: pass method=")
        for k in ("max_token_step", "beam_size", "cutoff_top_k"):
            kw.setdefault(k, getattr(cfg, k))
        if method == "beam" and "lm" not in kw:            # the LM the validation search is fused with
            lm = self._metric_lm()
            if lm is not None:
                kw["lm"] = lm
                kw.setdefault("lm_weight", cfg.lm_weight)
                kw.setdefault("lm_start_token", cfg.lm_start_token)
        if method == "beam" and "context" not in kw:       # the hotwords the validation search is biased with
            for k, v in self._metric_context().items():
                kw.setdefault(k, v)
        return StreamingRecognizer(self._encoder, self._predictor, self._joiner, self._tokenizer,
                                   cmvn=self._global_cmvn, batch_size=batch_size, method=method, **kw)


class RnntTask(BaseRnntTask):
    def __init__(self, config) -> None:
        super().__init__(config)
        assert config["loss"]["model"] == "Rnnt"
        self._loss = Loss(config["loss"])

    def training_step(self, batch, batch_idx):
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        pred, pred_len, _ = self._predictor(batch["label"], batch["label_length"],
                                            self._predictor.init_state())
        joint, _, _, _ = self._joiner(dec, dec_len, pred, pred_len)
        loss = self._loss({"logits": joint, "logits_length": dec_len, "targets": batch["label"],
                           "targets_length": batch["label_length"]})
        self.log("train_loss", loss, sync_dist=True, prog_bar=True, logger=True)
        return loss.mean()


    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """reference rnnt_task.py:244-284."""
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        pred, pred_len, _ = self._predictor(batch["label"], batch["label_length"],
                                            self._predictor.init_state())
        joint, _, _, _ = self._joiner(dec, dec_len, pred, pred_len, batch["label"])
        loss = self._loss({"logits": joint, "logits_length": dec_len, "targets": batch["label"],
                           "targets_length": batch["label_length"]})
        wer = self._wer(dec, dec_len, batch["label"])
        self.log_dict({"val_loss": loss, "wer": wer}, sync_dist=True, prog_bar=True)
        return {"val_loss": loss, "wer": wer}


class CtcHybridRnnt(BaseRnntTask):
    """Shared encoder, CTC head on decoder_out, RNN-T branch on encoder_out (reference :287-420)."""
    _JOINS_ENCODER_OUT = True

    def __init__(self, config) -> None:
        super().__init__(config)
        self._rnnt_weight = config["loss"]["rnnt_weight"]
        self._ctc_weight = config["loss"]["ctc_weight"]
        self._ctc_loss = Loss(config["loss"]["ctc_loss"])
        self._rnnt_loss = Loss(config["loss"]["rnnt_loss"])

    def training_step(self, batch, batch_idx):
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        pred, pred_len, _ = self._predictor(batch["label"], batch["label_length"],
                                            self._predictor.init_state())
        joint, _, _, _ = self._joiner(enc, enc_len, pred, pred_len)
        loss_rnnt = self._rnnt_loss({"logits": joint, "logits_length": enc_len,
                                     "targets": batch["label"],
                                     "targets_length": batch["label_length"]})
        loss_ctc = self._ctc_loss({"logits": dec, "logits_length": dec_len,
                                   "targets": batch["label"],
                                   "targets_length": batch["label_length"]})
        loss = self._rnnt_weight * loss_rnnt + self._ctc_weight * loss_ctc
        self.log_dict({"train_loss": loss, "train_loss/loss_rnnt": loss_rnnt,
                       "train_loss/loss_ctc": loss_ctc}, sync_dist=True, prog_bar=True,
                      logger=True)
        return loss.mean()


    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """reference rnnt_task.py:365-420: the WER decodes encoder_out (the RNN-T branch's input)."""
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        pred, pred_len, _ = self._predictor(batch["label"], batch["label_length"],
                                            self._predictor.init_state())
        joint, _, _, _ = self._joiner(enc, enc_len, pred, pred_len, batch["label"])
        loss_rnnt = self._rnnt_loss({"logits": joint, "logits_length": enc_len,
                                     "targets": batch["label"],
                                     "targets_length": batch["label_length"]})
        loss_ctc = self._ctc_loss({"logits": dec, "logits_length": dec_len,
                                   "targets": batch["label"],
                                   "targets_length": batch["label_length"]})
        loss = self._rnnt_weight * loss_rnnt + self._ctc_weight * loss_ctc
        wer = self._wer(enc, enc_len, batch["label"])
        info = {"val_loss": loss, "val_loss/loss_rnnt": loss_rnnt, "val_loss/loss_ctc": loss_ctc,
                "wer": wer}
        self.log_dict(info, sync_dist=True, prog_bar=True, logger=True)
        return info


class PrunedRnntTask(BaseRnntTask):
    def __init__(self, config) -> None:
        super().__init__(config)
        assert config["loss"]["model"] == "Pruned_Rnnt"
        self._loss_config = config["loss"]
        self._simple_loss_scale = config["loss"]["simple_loss_scale"]
        self._pruned_loss_scale = config["loss"]["pruned_loss_scale"]
        self._loss = Loss(self._loss_config)
        self._enable_ctc = self._loss_config["enable_ctc"]
        if self._enable_ctc:
            self._ctc_loss = Loss({"model": "CTC", "config": {**self._loss_config["ctc_config"]}})
            self._ctc_projector = Decoder(config["ctc_projector"])

    def _align_rnnt_type(self) -> str:
        return (self._loss_config.get("config") or {}).get("rnnt_type", "regular")

    def _optimizer_params(self):
        """reference rnnt_task.py:596-630: the CTC head is a fifth group when enable_ctc."""
        params = super()._optimizer_params()
        sep = self._optim_config["seperate_lr"]
        if sep["apply"] and self._enable_ctc:
            params.append({"params": self._ctc_projector.parameters(), "name": "ctc_projector_lr",
                           "lr": sep["config"]["ctc_projector_lr"]})
        return params

    def training_step(self, batch, batch_idx):
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        pred, pred_len, _ = self._predictor(batch["label"], batch["label_length"],
                                            self._predictor.init_state())
        joint, boundary, ranges, simple_loss = self._joiner(dec, dec_len, pred, pred_len,
                                                            batch["label"])
        pruned_loss = self._loss({"logits": joint, "logits_length": dec_len,
                                  "targets": batch["label"],
                                  "targets_length": batch["label_length"],
                                  "boundary": boundary, "ranges": ranges})
        loss = self._simple_loss_scale * simple_loss + self._pruned_loss_scale * pruned_loss
        ctc_loss = 0.0
        if self._enable_ctc:
            logits, logits_len = self._ctc_projector(dec, dec_len)
            ctc_loss = self._ctc_loss({"logits": logits, "logits_length": logits_len,
                                       "targets": batch["label"],
                                       "targets_length": batch["label_length"]})
            loss = loss + ctc_loss
        self.log_dict({"train_loss": loss, "train_loss/simple_loss": simple_loss,
                       "train_loss/pruned_loss": pruned_loss, "train_loss/ctc_loss": ctc_loss},
                      sync_dist=True, prog_bar=True, logger=True)
        return loss.mean()

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """reference rnnt_task.py:516-594."""
        feat, feat_len = self.features(batch)
        enc, enc_len = self._encoder(feat, feat_len)
        dec, dec_len = self._decoder(enc, enc_len)
        pred, pred_len, _ = self._predictor(batch["label"], batch["label_length"],
                                            self._predictor.init_state())
        joint, boundary, ranges, simple_loss = self._joiner(dec, dec_len, pred, pred_len,
                                                            batch["label"])
        pruned_loss = self._loss({"logits": joint, "logits_length": dec_len,
                                  "targets": batch["label"],
                                  "targets_length": batch["label_length"],
                                  "boundary": boundary, "ranges": ranges})
        loss = self._simple_loss_scale * simple_loss + self._pruned_loss_scale * pruned_loss
        ctc_loss = 0.0
        if self._enable_ctc:
            logits, logits_len = self._ctc_projector(dec, dec_len)
            ctc_loss = self._ctc_loss({"logits": logits, "logits_length": logits_len,
                                       "targets": batch["label"],
                                       "targets_length": batch["label_length"]})
            loss = loss + ctc_loss
        wer = self._wer(dec, dec_len, batch["label"])
        info = {"val_loss": loss, "val_loss/simple_loss": simple_loss,
                "val_loss/pruned_loss": pruned_loss, "val_loss/ctc_loss": ctc_loss, "wer": wer}
        self.log_dict(info, sync_dist=True, prog_bar=True, logger=True)
        return info
