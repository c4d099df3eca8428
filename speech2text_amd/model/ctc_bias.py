"""Hotword (contextual) biasing of the CTC prefix beam search: the Python surface over s2t_ctc_prefix_beam_bias,
s2t_ctc_prefix_beam_ngram_bias and their _chunk partners (csrc/decode_ctc.hip).  The phrases are a
ContextGraph (model/lm/context_graph.py).  It stands beside model/decoding.py, whose public names and signatures
are pinned, and extends it:

    ctc_prefix_beam_bias_tokens     the whole-utterance call, through decoding._whole_utterance
    CtcBiasPrefixBeamDecoding       CtcPrefixBeamDecoding(..., context=None, context_weight=1.0); the search, host
                                    loop and dispatch are the base class', which reads the `_context` set here
    CtcBiasStreamingSearch          the chunk-carried search, with or without an NgramLm
    ctc_bias_streaming_search       ctc_streaming_search(..., context=None, context_weight=1.0)
"""
import math

import torch

from speech2text_amd import _native as N
from speech2text_amd.model.decoding import (CtcPrefixBeamDecoding, CtcStreamingSearch, _ngram_arguments, _ngram_beside,
                                            _ngram_on, _is_ngram, _whole_utterance, ctc_streaming_search)


def _is_context(graph):
    from speech2text_amd.model.lm.context_graph import ContextGraph
    return isinstance(graph, ContextGraph)


def _context_arguments(context, context_weight, name):
    """The hotword arguments of `name`, checked -> (graph, weight)."""
    if not _is_context(context):
        raise ValueError(f"{name} needs a ContextGraph, got {type(context).__name__}")
    if not math.isfinite(float(context_weight)):
        raise ValueError(f"context_weight must be finite, got {context_weight!r}")
    return context, float(context_weight)


def ctc_prefix_beam_bias_tokens(logits, lengths, graph, bias_weight=1.0, lm=None, lm_weight=0.0, beam_size=4,
                                cutoff_top_k=4, blank=0):
    """ctc_prefix_beam_tokens (lm None) or ctc_prefix_beam_ngram_tokens (lm: an NgramLm) with hotword biasing
    (graph: a ContextGraph whose fp32 tables are on the logits' device), still ONE launch: a live prefix
    also carries a graph state and bias_sum, candidates rank with bias_weight * bias_sum added, and the
    reported hypothesis is the live prefix that is best once every unfinished match has been paid back.
    -> (tokens, out_len, score, [lm_score,] bias_score (B) fp32: the reported prefix' bias_sum without the
    loan of an unfinished match), or None where the entry refuses.  HIP: decode_ctc.hip, ngram_lookup.h."""
    def plan(x, n):
        if graph.device != x.device:
            raise RuntimeError(f"the context graph's tables are on {graph.device}, the logits on {x.device}: "
                               "ContextGraph.to(device)")
        (B, T, V), beam, topk = x.shape, int(beam_size), int(cutoff_top_k)
        nbytes = N.lib().s2t_ctc_prefix_beam_workspace_bytes(B, T, V, beam)
        if nbytes <= 0:
            return None
        g_desc, keep = graph.desc()
        if lm is None:
            return nbytes, lambda tail: N.lib().s2t_ctc_prefix_beam_bias(
                g_desc, N.fp(x), N.lp(n), B, T, V, int(blank), beam, topk, float(bias_weight), *tail), keep
        _ngram_beside(lm, x, "the logits")
        lm_desc, lm_keep = lm.desc()
        return nbytes, lambda tail: N.lib().s2t_ctc_prefix_beam_ngram_bias(
            lm_desc, g_desc, N.fp(x), N.lp(n), B, T, V, int(blank), beam, topk, float(lm_weight), int(lm.start_ctx),
            float(bias_weight), *tail), keep + lm_keep
    entry = "s2t_ctc_prefix_beam_bias" if lm is None else "s2t_ctc_prefix_beam_ngram_bias"
    return _whole_utterance(entry, "device CTC prefix beam search", logits, lengths, plan, lm_score=lm is not None,
                            bias_score=True)


class CtcBiasStreamingSearch(CtcStreamingSearch):
    """CtcStreamingSearch's beam search with hotword biasing, without an LM or fused with a back-off n-gram
    (csrc/decode_ctc.hip s2t_ctc_prefix_beam_bias_chunk, s2t_ctc_prefix_beam_ngram_bias_chunk):
    ctc_prefix_beam_bias_tokens fed the frames' scores a chunk at a time, still ONE launch per chunk.
    However the frames are cut, the result after a chunk is ctc_prefix_beam_bias_tokens' on the frames fed
    so far, bit for bit, `bias_score` included, while `overflow` is 0: the finalisation that takes back
    the loan of an unfinished match touches the outputs only, the carried beam is what it would be
    without it.

    Same attributes, `reset(rows)` (a reset row restarts in the graph's root, and in the LM's start
    context) and `step(logits_chunk, chunk_len)` as CtcStreamingSearch, and `bias_score` (B).  Beam only.
    The graph's (and the n-gram's) tables are copied to the search's device when they live elsewhere; the
    graph must not change while a stream is live.  A `context` that is not a ContextGraph with fp32
    tables, an `lm` that is neither None nor an NgramLm with fp32 tables, a weight that is not finite or a
    shape the entry refuses are a ValueError at construction.  No host-loop fallback."""

    def __init__(self, num_classes, batch_size=1, beam_size=4, cutoff_top_k=4, max_tokens=1024, max_nodes=4096,
                 blank=0, device=None, lm=None, lm_weight=0.0, context=None, context_weight=1.0):
        self._context, self._context_weight = _context_arguments(context, context_weight, "CtcBiasStreamingSearch")
        if self._context.dtype != torch.float32:
            raise ValueError("the device bias search needs fp32 tables")
        super().__init__(num_classes, batch_size, "beam", beam_size, cutoff_top_k, max_tokens, max_nodes, blank,
                         device, lm, lm_weight)

    def _lm_arguments(self, lm, lm_weight, lm_start_token, method):
        return (None, 0.0, -1) if lm is None else _ngram_arguments(lm, lm_weight, "CtcBiasStreamingSearch")

    def _allocate(self, num_classes, dev):
        B, V, lib = self.batch_size, self.V, N.lib()
        ok = self._shape_ok() and self._context.num_classes == V and (self._lm is None or self._lm.num_classes == V)
        size = lib.s2t_ctc_bias_stream_state_bytes if self._lm is None else lib.s2t_ctc_ngram_bias_stream_state_bytes
        n = size(B, V, self.beam_size, self.max_nodes) if ok else 0
        if n <= 0:
            raise self._refuse("bias beam", f", graph V {self._context.num_classes}" + (
                "" if self._lm is None else f", LM V {self._lm.num_classes}"))
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)   # the partner's state, then bstate, bsum
        self._context = _ngram_on(self._context, dev)
        self._graph_desc, self._graph_keep = self._context.desc()
        if self._lm is not None:
            self._lm = _ngram_on(self._lm, dev)
            self._lm_desc, self._lm_keep = self._lm.desc()
        self.bias_score = torch.zeros((B,), dtype=torch.float32, device=dev)

    def _construct(self, *args, **kw):
        super()._construct(*args, **kw)
        self._outputs.append(self.bias_score)              # (reset zeroes it with the others)

    def _reset_state(self, mask):
        tail = (N.ptr(self.state), N.ip(mask), self.batch_size, self.V, self.beam_size, self.max_nodes)
        if self._lm is None:
            N.check(N.lib().s2t_ctc_bias_stream_reset(*tail, N.stream()), "s2t_ctc_bias_stream_reset")
        else:
            N.check(N.lib().s2t_ctc_ngram_bias_stream_reset(*tail, int(self._lm.start_ctx), N.stream()),
                    "s2t_ctc_ngram_bias_stream_reset")

    def _chunk(self, logits_chunk, chunk_len, Tc):
        if self._lm is None:
            N.check(N.lib().s2t_ctc_prefix_beam_bias_chunk(
                self._graph_desc, N.fp(logits_chunk), N.lp(chunk_len), self.batch_size, Tc, self.V, self.blank,
                self.beam_size, self.cutoff_top_k, self._context_weight, self.max_tokens, self.max_nodes,
                N.ptr(self.state), N.lp(self.tokens), N.lp(self.out_len), N.fp(self.score), N.fp(self.bias_score),
                N.lp(self.stable_len), N.ip(self.overflow), N.stream()), "s2t_ctc_prefix_beam_bias_chunk")
        else:
            N.check(N.lib().s2t_ctc_prefix_beam_ngram_bias_chunk(
                self._lm_desc, self._graph_desc, N.fp(logits_chunk), N.lp(chunk_len), self.batch_size, Tc, self.V,
                self.blank, self.beam_size, self.cutoff_top_k, self._lm_weight, self._context_weight, self.max_tokens,
                self.max_nodes, N.ptr(self.state), N.lp(self.tokens), N.lp(self.out_len), N.fp(self.score),
                N.fp(self.lm_score), N.fp(self.bias_score), N.lp(self.stable_len), N.ip(self.overflow), N.stream()),
                "s2t_ctc_prefix_beam_ngram_bias_chunk")


class CtcBiasPrefixBeamDecoding(CtcPrefixBeamDecoding):
    """CtcPrefixBeamDecoding with hotwords: `context` (a ContextGraph, or None for the base class' search as it
    is) and `context_weight` behind the base class' arguments.  Device logits with no LM or an fp32 NgramLm run
    the fused bias entries, the graph following the logits to their device as the n-gram does; an RnnLm or a
    foreign LM with a context, CPU tensors and refused shapes run `_module_loop`, which has the same term and the
    same finalisation through the ContextGraph protocol.  `beam_tokens` returns (tokens, out_len, score,
    [lm_score,] bias_score)."""

    def __init__(self, tokenizer, beam_size=4, cutoff_top_k=4, lm=None, lm_weight=0.0, lm_start_token=None,
                 context=None, context_weight=1.0) -> None:
        super().__init__(tokenizer, beam_size, cutoff_top_k, lm, lm_weight, lm_start_token)
        if context is not None:
            self._context, self._context_weight = _context_arguments(context, context_weight,
                                                                     "CtcBiasPrefixBeamDecoding")


def ctc_bias_streaming_search(num_classes, batch_size=1, method="beam", beam_size=4, cutoff_top_k=4, max_tokens=1024,
                              max_nodes=4096, blank=0, device=None, lm=None, lm_weight=0.0, lm_start_token=None,
                              context=None, context_weight=1.0):
    """ctc_streaming_search with hotwords: without a `context` exactly that; with one (a ContextGraph) a
    CtcBiasStreamingSearch, which is the beam method with no LM or an NgramLm (no `lm_start_token`); anything
    else with a context is a ValueError."""
    if context is None:
        return ctc_streaming_search(num_classes, batch_size, method, beam_size, cutoff_top_k, max_tokens, max_nodes,
                                    blank, device, lm=lm, lm_weight=lm_weight, lm_start_token=lm_start_token)
    if method != "beam" or lm_start_token is not None or not (lm is None or _is_ngram(lm)):
        raise ValueError("hotword biasing is fused into the beam method with no LM or an NgramLm (which takes no "
                         "lm_start_token)")
    return CtcBiasStreamingSearch(num_classes, batch_size, beam_size, cutoff_top_k, max_tokens, max_nodes, blank,
                                  device, lm=lm, lm_weight=lm_weight, context=context, context_weight=context_weight)
