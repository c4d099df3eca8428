"""Hotword (contextual) biasing of the one-launch RNN-T beam search: the Python surface over
s2t_rnnt_beam_stateless_bias, s2t_rnnt_beam_stateless_ngram_bias and their _chunk partners (csrc/decode_rnnt.hip,
csrc/decode_search.h).  The phrases are a ContextGraph (model/lm/context_graph.py).  It stands beside
model/decoding.py, whose public names and signatures are pinned, and extends it:

    rnnt_beam_bias_tokens_from_am   the whole-utterance call, through decoding._whole_utterance
    RnntBiasBeamDecoding            RnntBeamDecoding(..., context=None, context_weight=1.0); the search, host
                                    loops and dispatch are the base class', which reads the `_context` set here
    RnntBiasStreamingSearch         the chunk-carried search, with or without an NgramLm
    rnnt_bias_streaming_search      rnnt_streaming_search(..., context=None, context_weight=1.0)
"""
import torch

from speech2text_amd import _native as N
from speech2text_amd.model.ctc_bias import _context_arguments
from speech2text_amd.model.decoding import (RnntBeamDecoding, RnntStreamingSearch, _is_ngram, _ngram_arguments,
                                            _ngram_beside, _ngram_on, _stateless_weights, _whole_utterance,
                                            rnnt_streaming_search)


def rnnt_beam_bias_tokens_from_am(am, lengths, predictor, joiner, graph, bias_weight=1.0, lm=None, lm_weight=0.0,
                                  beam_size=4, cutoff_top_k=4):
    """rnnt_beam_tokens_from_am (lm None) or rnnt_beam_ngram_tokens_from_am (lm: an NgramLm) with hotword biasing
    (graph: a ContextGraph whose fp32 tables are on am's device), still ONE launch: a live beam also carries a
    graph state and bias_sum, the candidate of class c != blank scores bias_weight * (the graph's look-up) more,
    behind the LM term, and the reported hypothesis is the live beam that is best once every unfinished match
    has been paid back.  -> (tokens, frames, out_len, score, [lm_score,] bias_score (B) fp32: the reported
    beam's bias_sum without the loan of an unfinished match), or None where the entry refuses.
    HIP: decode_rnnt.hip, decode_search.h, ngram_lookup.h."""
    def plan(am, n):
        if graph.device != am.device:
            raise RuntimeError(f"the context graph's tables are on {graph.device}, am on {am.device}: "
                               "ContextGraph.to(device)")
        (B, T, V), beam, topk = am.shape, int(beam_size), int(cutoff_top_k)
        nbytes = N.lib().s2t_rnnt_beam_ngram_workspace_bytes(B, T, V, beam)   # (= the plain one's, within the limits)
        if nbytes <= 0:
            return None
        g_desc, keep = graph.desc()
        w, E, D, ctx, act = _stateless_weights(predictor, joiner)
        if lm is None:
            return nbytes, lambda tail: N.lib().s2t_rnnt_beam_stateless_bias(
                g_desc, N.fp(am), N.lp(n), *[N.fp(t) for t in w], B, T, V, E, D, ctx, act, 0, beam, topk,
                float(bias_weight), *tail), (w, keep)
        _ngram_beside(lm, am, "am")
        lm_desc, lm_keep = lm.desc()
        return nbytes, lambda tail: N.lib().s2t_rnnt_beam_stateless_ngram_bias(
            lm_desc, g_desc, N.fp(am), N.lp(n), *[N.fp(t) for t in w], B, T, V, E, D, ctx, act, 0, beam, topk,
            float(lm_weight), int(lm.start_ctx), float(bias_weight), *tail), (w, keep, lm_keep)
    entry = "s2t_rnnt_beam_stateless_bias" if lm is None else "s2t_rnnt_beam_stateless_ngram_bias"
    return _whole_utterance(entry, "fused RNN-T beam search", am, lengths, plan, frames=True, lm_score=lm is not None,
                            bias_score=True)


class RnntBiasBeamDecoding(RnntBeamDecoding):
    """RnntBeamDecoding with hotwords: `context` (a ContextGraph, or None for the base class' search as it is) and
    `context_weight` behind the base class' arguments.  Device inputs, the stateless predictor with a
    projection-free Joiner and no LM or an fp32 NgramLm without `lm_start_token` run the fused bias entries, the
    graph following the inputs to their device as the n-gram does; everything else with a context -- an RnnLm, the
    LSTM predictor, a joiner with output projection, CPU tensors, refused shapes -- runs the host loop, which has
    the same term and the same finalisation through the ContextGraph protocol.  `beam_tokens` returns (tokens,
    frames, out_len, score, [lm_score,] bias_score)."""

    def __init__(self, tokenizer, predictor, joiner, beam_size=4, cutoff_top_k=4, lm=None, lm_weight=0.0,
                 lm_start_token=None, context=None, context_weight=1.0) -> None:
        super().__init__(tokenizer, predictor, joiner, beam_size, cutoff_top_k, lm, lm_weight, lm_start_token)
        if context is not None:
            self._context, self._context_weight = _context_arguments(context, context_weight, "RnntBiasBeamDecoding")


class RnntBiasStreamingSearch(RnntStreamingSearch):
    """RnntStreamingSearch's beam search with hotword biasing, without an LM or fused with a back-off n-gram
    (csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_bias_chunk, s2t_rnnt_beam_stateless_ngram_bias_chunk):
    rnnt_beam_bias_tokens_from_am fed am a chunk at a time, still ONE launch per chunk.  However the frames are
    cut, the result after a chunk is rnnt_beam_bias_tokens_from_am's on the frames fed so far, bit for bit,
    `bias_score` included, while `overflow` is 0: the finalisation that takes back the loan of an unfinished
    match touches the outputs only, the carried beams are what they would be without it.

    Same attributes, `reset(rows)` (a reset row restarts in the graph's root, and in the LM's start context) and
    `step(am_chunk, chunk_len)` as RnntStreamingSearch with method="beam", `lm_score` (B) with an LM, and
    `bias_score` (B), which reset zeroes.  Beam only.  The graph's (and the n-gram's) tables are copied to the
    search's device when they live elsewhere; the graph must not change while a stream is live.  A `context`
    that is not a ContextGraph with fp32 tables, an `lm` that is neither None nor an NgramLm with fp32 tables, a
    weight that is not finite or a shape the entry refuses are a ValueError at construction.  No host-loop
    fallback."""

    def __init__(self, predictor, joiner, batch_size=1, beam_size=4, cutoff_top_k=4, max_tokens=1024, device=None,
                 lm=None, lm_weight=0.0, context=None, context_weight=1.0):
        self._context, self._context_weight = _context_arguments(context, context_weight, "RnntBiasStreamingSearch")
        if self._context.dtype != torch.float32:
            raise ValueError("the device bias search needs fp32 tables")
        self._construct_rnnt(predictor, joiner, batch_size, "beam", 0, beam_size, cutoff_top_k, max_tokens, device,
                             lm, lm_weight)

    def _lm_arguments(self, lm, lm_weight, lm_start_token, method):
        return (None, 0.0, -1) if lm is None else _ngram_arguments(lm, lm_weight, "RnntBiasStreamingSearch")

    def _allocate(self, predictor, joiner, dev):
        super()._allocate(predictor, joiner, dev)          # the plain search's checks and weights
        lib = N.lib()
        size = lib.s2t_rnnt_bias_stream_state_bytes if self._lm is None else lib.s2t_rnnt_ngram_bias_stream_state_bytes
        ok = self._context.num_classes == self.V and (self._lm is None or self._lm.num_classes == self.V)
        n = size(self.batch_size, self.V, self.ctx, self.beam_size, self.max_tokens) if ok else 0
        if n <= 0:
            raise ValueError(f"the chunk-carried bias beam search does not take this shape: B {self.batch_size} "
                             f"V {self.V} beam {self.beam_size} max_tokens {self.max_tokens}, graph V "
                             f"{self._context.num_classes}" + ("" if self._lm is None else
                                                                f", LM V {self._lm.num_classes}") +
                             " (limits: include/s2t_mi355.h)")
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)   # the partner's row, then bstate, bsum
        self._context = _ngram_on(self._context, dev)
        self._graph_desc, self._graph_keep = self._context.desc()
        if self._lm is not None:
            self._lm = _ngram_on(self._lm, dev)
            self._lm_desc, self._lm_keep = self._lm.desc()
        self.bias_score = torch.zeros((self.batch_size,), dtype=torch.float32, device=dev)

    def _construct(self, *args, **kw):
        super()._construct(*args, **kw)
        self._outputs.append(self.bias_score)              # (reset zeroes it with the others)

    def _reset_state(self, mask):
        tail = (N.ptr(self.state), N.ip(mask), self.batch_size, self.V, self.ctx, self.beam_size, self.max_tokens, 0)
        if self._lm is None:
            N.check(N.lib().s2t_rnnt_bias_stream_reset(*tail, N.stream()), "s2t_rnnt_bias_stream_reset")
        else:
            N.check(N.lib().s2t_rnnt_ngram_bias_stream_reset(*tail, int(self._lm.start_ctx), N.stream()),
                    "s2t_rnnt_ngram_bias_stream_reset")

    def _chunk(self, am_chunk, chunk_len, Tc):
        head = (N.fp(am_chunk), N.lp(chunk_len), *[N.fp(t) for t in self._w], self.batch_size, Tc, self.V, self.E,
                self.D, self.ctx, self._act, 0, self.beam_size, self.cutoff_top_k)
        if self._lm is None:
            N.check(N.lib().s2t_rnnt_beam_stateless_bias_chunk(
                self._graph_desc, *head, self._context_weight, self.max_tokens, N.ptr(self.state), N.lp(self.tokens),
                N.lp(self.frames), N.lp(self.out_len), N.fp(self.score), N.fp(self.bias_score), N.lp(self.stable_len),
                N.ip(self.overflow), N.stream()), "s2t_rnnt_beam_stateless_bias_chunk")
        else:
            N.check(N.lib().s2t_rnnt_beam_stateless_ngram_bias_chunk(
                self._lm_desc, self._graph_desc, *head, self._lm_weight, self._context_weight, self.max_tokens,
                N.ptr(self.state), N.lp(self.tokens), N.lp(self.frames), N.lp(self.out_len), N.fp(self.score),
                N.fp(self.lm_score), N.fp(self.bias_score), N.lp(self.stable_len), N.ip(self.overflow), N.stream()),
                "s2t_rnnt_beam_stateless_ngram_bias_chunk")


def rnnt_bias_streaming_search(predictor, joiner, batch_size=1, method="greedy", max_token_step=5, beam_size=4,
                               cutoff_top_k=4, max_tokens=1024, device=None, lm=None, lm_weight=0.0,
                               lm_start_token=None, context=None, context_weight=1.0, **kw):
    """rnnt_streaming_search with hotwords: without a `context` exactly that; with one (a ContextGraph) an
    RnntBiasStreamingSearch, which is the beam method of the stateless predictor with no LM or an NgramLm (no
    `lm_start_token`); anything else with a context is a ValueError."""
    if context is None:
        return rnnt_streaming_search(predictor, joiner, batch_size, method, max_token_step, beam_size, cutoff_top_k,
                                     max_tokens, device, lm=lm, lm_weight=lm_weight, lm_start_token=lm_start_token,
                                     **kw)
    if method != "beam" or lm_start_token is not None or not (lm is None or _is_ngram(lm)) or kw:
        raise ValueError("hotword biasing is fused into the beam method of the stateless predictor with no LM or an "
                         "NgramLm (which takes no lm_start_token)")
    return RnntBiasStreamingSearch(predictor, joiner, batch_size, beam_size, cutoff_top_k, max_tokens, device, lm=lm,
                                   lm_weight=lm_weight, context=context, context_weight=context_weight)
