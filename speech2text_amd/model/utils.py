"""Metrics for evaluation (mirror of the reference's model/utils.py:23-136): word / character
error rate over decoded texts and the AsrMetric callable the tasks' validation_step uses."""
import dataclasses
from typing import List, Optional, Tuple

import torch

from speech2text_amd.model.decoding import (CtcGreedyDecoding, CtcPrefixBeamDecoding, RnntBeamDecoding,
                                            RnntGreedyDecoding, batch_search, reference_decoder)


def _levenshtein(a: List, b: List) -> int:
    """Edit distance with O(min(n, m)) memory (two rolling rows)."""
    if len(a) > len(b):
        a, b = b, a
    row = list(range(len(a) + 1))
    for i, y in enumerate(b, 1):
        prev, row = row, [i] + [0] * len(a)
        for j, x in enumerate(a, 1):
            row[j] = min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (x != y))
    return row[len(a)]


def word_error_rate(hypotheses: List[str], references: List[str], show_on_screen=True,
                    use_cer=False) -> float:
    if len(hypotheses) != len(references):
        raise ValueError("In word error rate calculation, hypotheses and references lists must "
                         "have the same number of elements. But I got:{0} and {1} "
                         "correspondingly".format(len(hypotheses), len(references)))
    scores = words = 0
    for h, r in zip(hypotheses, references):
        hl, rl = (list(h), list(r)) if use_cer else (h.split(), r.split())
        words += len(rl)
        scores += _levenshtein(hl, rl)
    return 1.0 * scores / words if words != 0 else float("inf")


@dataclasses.dataclass
class AsrMetricConfig:
    """decode_method: "ctc_greedy_search" / "rnnt_greedy_search" as in the reference, and
    "rnnt_beam_search" (a name of this project: the reference's AsrMetric knows the greedy
    decoders only), which scores with RnntBeamDecoding(beam_size, cutoff_top_k); given a language
    model (AsrMetric's `lm`) it is shallow-fused with lm_weight / lm_start_token.
    "ctc_prefix_beam_search" (also a name of this project: the reference's CTC beam decoder needs a
    lexicon decoder of a library) scores a CTC head with CtcPrefixBeamDecoding(beam_size,
    cutoff_top_k), lexicon-free and with equal prefixes merged; it takes the same `lm`, lm_weight and
    lm_start_token.  Both beam methods take AsrMetric's `context` / `context_weight` (hotwords: the
    `metric.hotwords` key; CtcBiasPrefixBeamDecoding / RnntBiasBeamDecoding); the greedy methods raise for one."""
    decode_method: str = "ctc_greedy_search"
    max_token_step: int = 5
    beam_size: int = 4
    cutoff_top_k: int = 4
    lm_weight: float = 0.0
    lm_start_token: Optional[int] = None


class AsrMetric(object):
    def __init__(self, tokenizer, config: AsrMetricConfig, predictor=None, joiner=None, lm=None, context=None,
                 context_weight=1.0):
        self._tokenizer = tokenizer
        if context is not None and config.decode_method not in ("ctc_prefix_beam_search", "rnnt_beam_search"):
            raise ValueError("hotwords bias the beam searches: metric.decode_method must be ctc_prefix_beam_search or "
                             "rnnt_beam_search")
        self._lm = lm                  # held here, not by the task: no parameter of the task
        if config.decode_method == "ctc_greedy_search":
            self._decode_sess = CtcGreedyDecoding(tokenizer=tokenizer)
        elif config.decode_method == "rnnt_greedy_search":
            self._decode_sess = RnntGreedyDecoding(tokenizer=tokenizer, predictor=predictor,
                                                   joiner=joiner,
                                                   max_token_step=config.max_token_step)
        elif config.decode_method == "rnnt_beam_search":
            from speech2text_amd.model.rnnt_bias import RnntBiasBeamDecoding
            search = RnntBeamDecoding if context is None else RnntBiasBeamDecoding
            bias = {} if context is None else dict(context=context, context_weight=context_weight)
            self._decode_sess = search(tokenizer=tokenizer, predictor=predictor,
                                       joiner=joiner, beam_size=config.beam_size,
                                       cutoff_top_k=config.cutoff_top_k, lm=lm,
                                       lm_weight=config.lm_weight,
                                       lm_start_token=config.lm_start_token, **bias)
        elif config.decode_method == "ctc_prefix_beam_search":
            from speech2text_amd.model.ctc_bias import CtcBiasPrefixBeamDecoding
            search = CtcPrefixBeamDecoding if context is None else CtcBiasPrefixBeamDecoding
            bias = {} if context is None else dict(context=context, context_weight=context_weight)
            self._decode_sess = search(tokenizer=tokenizer, beam_size=config.beam_size,
                                       cutoff_top_k=config.cutoff_top_k, lm=lm, lm_weight=config.lm_weight,
                                       lm_start_token=config.lm_start_token, **bias)
        else:
            raise NotImplementedError(config.decode_method)

    def __call__(self, hidden_states, inputs_length, ground_truth):
        references = reference_decoder(ground_truth, self._tokenizer)
        hypotheses = batch_search(hidden_states, inputs_length, self._decode_sess)
        return word_error_rate(hypotheses=hypotheses, references=references)


@dataclasses.dataclass
class SslMetricConfig:
    top_ks: Tuple[int] = (1, 5)


class SslMetric(object):
    """Top-k accuracy of the SSL task over the masked label positions (reference
    model/utils.py:139-191): a position counts when its label is among the k largest logits;
    the denominator is the number of masked positions (+1e-7)."""

    def __init__(self, config: SslMetricConfig):
        self._top_ks = tuple(config.top_ks)

    @staticmethod
    def _accuracy(logits, labels, masked_dim, top_k):
        top = logits.topk(top_k, dim=-1, largest=True, sorted=True).indices       # (B,T,k)
        keep = masked_dim.to(torch.bool)
        hit = (top == labels.unsqueeze(-1)).any(dim=-1) & keep
        # (a masked-out position never matches in the reference either: its candidates are set
        # to -1 and its label to 0)
        return hit.sum().float() / (masked_dim.sum() + 1e-7)

    def __call__(self, logits, labels, masked_dim):
        return {"top_{}_acc".format(k): self._accuracy(logits, labels, masked_dim, k)
                for k in self._top_ks}
