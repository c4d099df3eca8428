"""Validation-time decoding (mirror of the reference's model/decoding.py:19-82, 157-177,
196-271, 295-435): DecodingMethod / batch_search / reference_decoder / CtcGreedyDecoding /
RnntGreedyDecoding / RnntBeamDecoding / DecodingFactory with the same constructor arguments and
`decode(hidden_states[1,T,D]) -> str`.

The reference decodes one utterance at a time with Python loops over frames (and, for RNN-T,
predictor / joiner module calls per lattice move, per beam for the beam search).  Here
`batch_search` hands the WHOLE batch to one HIP launch: per-frame argmax + repeat/blank collapse
for CTC (csrc/decode.hip); for RNN-T with the stateless predictor and a projection-free joiner the
whole greedy lattice walk (csrc/decode.hip) and the whole beam search (csrc/decode_rnnt.hip) run
on the device, one workgroup per utterance.  With the LSTM predictor (joiner with or without
output projection: every LSTM YAML of the reference) both searches run on the device in lockstep
over the batch (csrc/decode_lstm.hip): per round one lattice move of every live row, a predictor
step for the rows that emitted, no host synchronisation per move.  Both families are also carried
across chunks of a stream (RnntStreamingSearch, csrc/decode_rnnt.hip; RnntLstmStreamingSearch,
csrc/decode_lstm.hip; rnnt_streaming_search picks the class).  Other predictor / joiner
combinations (the stateless predictor with an out-projection joiner, foreign classes, shapes a
kernel refuses) keep the module-by-module loop.  RnntBeamDecoding takes an RNN language model
for shallow fusion (`lm=`, `lm_weight=`): with the LSTM predictor and with the stateless predictor
(joiner with or without output projection) the LM is stepped inside the lockstep device search
(s2t_rnnt_beam_lstm_lm, s2t_rnnt_beam_stateless_lm), everything else runs `_module_loop_lm`; the
chunk-carried beam searches take the same LM (RnntLstmStreamingSearch with `lm=`,
RnntStatelessLmStreamingSearch; s2t_rnnt_beam_lstm_lm_chunk, s2t_rnnt_beam_stateless_lm_chunk).
An NgramLm is fused into the one-workgroup search of the stateless predictor instead, one launch, and
into its chunk-carried form (rnnt_beam_ngram_tokens_from_am, RnntNgramStreamingSearch;
s2t_rnnt_beam_stateless_ngram, s2t_rnnt_beam_stateless_ngram_chunk), and into the lockstep beam search of the
LSTM predictor, whose rounds then launch no LM step (rnnt_beam_lstm_ngram_tokens_from_am,
RnntLstmNgramStreamingSearch; s2t_rnnt_beam_lstm_ngram, s2t_rnnt_beam_lstm_ngram_chunk).
CtcPrefixBeamDecoding is a lexicon-free CTC prefix beam search with equal prefixes merged and the same
optional RNN-LM term, on the device for the whole batch (csrc/decode_ctc.hip: s2t_ctc_prefix_beam,
s2t_ctc_prefix_beam_lm) and, in one launch again, a back-off n-gram over the model's classes
(model/lm/ngram_lm.py NgramLm, s2t_ctc_prefix_beam_ngram; chunk-carried: CtcNgramStreamingSearch,
s2t_ctc_prefix_beam_ngram_chunk, built by ctc_streaming_search); CtcStreamingSearch carries the plain and the
RNN-LM search across chunks with a trie that does not grow with the stream (s2t_ctc_prefix_beam_chunk,
s2t_ctc_prefix_beam_lm_chunk).  The plain and the n-gram search also take hotwords, a ContextGraph of phrases
to boost: that surface is model/ctc_bias.py (this module's public names and signatures are pinned), which sets
the `_context` that CtcPrefixBeamDecoding's host loop and dispatch read.
The one-launch RNN-T beam search of the stateless predictor takes hotwords the same way, without an LM or with
the n-gram: model/rnnt_bias.py, which sets the `_context` that RnntBeamDecoding's host loops and dispatch read.
The lexicon CTC beam decoder (it wraps flashlight) and the CIF decoder are
not here."""
import abc
import copy
import ctypes
import math
from enum import Enum, unique
from typing import List

import torch

from speech2text_amd import _native as N


class DecodingMethod(abc.ABC):
    @abc.abstractmethod
    def decode(self, hidden_states: torch.Tensor) -> str:
        pass

    def decode_batch(self, hidden_states: torch.Tensor, inputs_length: torch.Tensor) -> List[str]:
        return [self.decode(hidden_states[i:i + 1, :int(inputs_length[i]), :])
                for i in range(hidden_states.shape[0])]


class _BatchDecoding(DecodingMethod):
    """A method whose decode_batch is the search: one utterance is a batch of one."""

    @torch.no_grad()
    def decode(self, hidden_states: torch.Tensor) -> str:
        assert hidden_states.shape[0] == 1, "Support BatchSize = 1 only."
        n = torch.tensor([hidden_states.shape[1]], dtype=torch.int64)
        return self.decode_batch(hidden_states, n)[0]


def batch_search(hidden_states: torch.Tensor, inputs_length: torch.Tensor,
                 decode_session: DecodingMethod) -> List[str]:
    """hidden_states (B,T,D), inputs_length (B) -> list of decoded texts (reference :27-48)."""
    return decode_session.decode_batch(hidden_states, inputs_length)


def reference_decoder(tensor: torch.Tensor, tokenizer) -> List[str]:
    """Label rows (0-padded) -> texts (reference :157-177)."""
    refs = []
    rows = tensor.long().cpu()
    for b in range(rows.shape[0]):
        ids = []
        for u in rows[b].tolist():
            if u == 0:
                break
            ids.append(u)
        refs.append(tokenizer.decode(torch.tensor(ids, dtype=torch.int64)))
    return refs


def ctc_greedy_tokens(logits: torch.Tensor, lengths: torch.Tensor, blank: int = 0):
    """(B,T,V) device logits -> (tokens (B,T) int64, out_len (B) int64).  HIP: decode.hip."""
    if not logits.is_cuda:
        raise RuntimeError("speech2text_amd decoding runs on the GPU only (no CPU fallback)")
    logits = logits.contiguous().float()
    B, T, V = logits.shape
    lengths = lengths.to(device=logits.device, dtype=torch.int64).contiguous()
    tokens = torch.zeros((B, T), dtype=torch.int64, device=logits.device)
    out_len = torch.zeros((B,), dtype=torch.int64, device=logits.device)
    N.check(N.lib().s2t_ctc_greedy(N.fp(logits), N.lp(lengths), B, T, V, int(blank),
                                   N.lp(tokens), N.lp(out_len), N.stream()), "s2t_ctc_greedy")
    return tokens, out_len


def _to_texts(tokens, out_len, tokenizer):
    tok, n = tokens.cpu(), out_len.cpu().tolist()
    return [tokenizer.decode(tok[b, :n[b]]) for b in range(tok.shape[0])]


class CtcGreedyDecoding(_BatchDecoding):
    def __init__(self, tokenizer, dummy=-1) -> None:
        self._tokenizer = tokenizer

    def decode_batch(self, hidden_states, inputs_length):
        assert hidden_states.shape[-1] == len(self._tokenizer.labels)
        return _to_texts(*ctc_greedy_tokens(hidden_states, inputs_length), self._tokenizer)


def _whole_utterance(entry, what, scores, lengths, plan, frames=False, score=True, lm_score=False, per_frame=1,
                     bias_score=False):
    """The one calling path of the whole-utterance device searches.  scores (B,T,V) must be on the device
    (RuntimeError: the `what` runs on the GPU only), lengths (B) follow them.  The outputs are zeroed --
    tokens (B, T * per_frame) int64, [frames (B,T) int64,] out_len (B) int64, [score (B) fp32,] [lm_score
    (B) fp32,] [bias_score (B) fp32] -- and are the answer for an empty batch.  Then `plan(scores, lengths)` states the search:
    None where it refuses, else (workspace bytes, call, keep).  `call(tail)` makes the C call, `tail` being
    the entry's last arguments: workspace, the outputs in the order above, stream.  `keep` is what the
    call's pointers need alive (descriptors and the tensors behind them); it is held here until the call
    has returned.  -> the outputs, or None for bytes <= 0 and for rc -1 (the caller runs its host loop);
    any other rc raises."""
    if not scores.is_cuda:
        raise RuntimeError(f"the {what} runs on the GPU only")
    scores = scores.contiguous().float()
    B, T, _ = scores.shape
    dev = scores.device
    lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
    out = [torch.zeros((B, T * per_frame), dtype=torch.int64, device=dev)]
    if frames:
        out.append(torch.zeros((B, T), dtype=torch.int64, device=dev))
    out.append(torch.zeros((B,), dtype=torch.int64, device=dev))
    out += [torch.zeros((B,), dtype=torch.float32, device=dev) for has in (score, lm_score, bias_score) if has]
    out = tuple(out)
    if B == 0 or T == 0:
        return out
    planned = plan(scores, lengths)
    if planned is None or planned[0] <= 0:
        return None
    nbytes, call, keep = planned                           # (keep: a local until this function returns)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    rc = call([N.ptr(ws)] + [N.lp(t) if t.dtype is torch.int64 else N.fp(t) for t in out] + [N.stream()])
    if rc == -1:
        return None
    N.check(rc, entry)
    return out


def _lm_start_arg(lm_start_token):
    """lm_start_token as the C entries take it: -1 for None, else the token id; a negative id is a ValueError."""
    start = -1 if lm_start_token is None else int(lm_start_token)
    if lm_start_token is not None and start < 0:
        raise ValueError(f"lm_start_token must be None or a token id, got {lm_start_token!r}")
    return start


def _is_ngram(lm):
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return isinstance(lm, NgramLm)


def _ngram_arguments(lm, lm_weight, name):
    """The LM arguments of the device n-gram search `name`, checked -> (lm, lm_weight, -1: it starts in
    its own <s> context and takes no start token)."""
    if not _is_ngram(lm):
        raise ValueError(f"{name} needs an NgramLm, got {type(lm).__name__}")
    if lm.dtype != torch.float32:
        raise ValueError("the device n-gram search needs fp32 tables")
    if not math.isfinite(float(lm_weight)):
        raise ValueError(f"lm_weight must be finite, got {lm_weight!r}")
    return lm, float(lm_weight), -1


def _ngram_on(lm, dev):
    """lm itself where its tables are on `dev`, else a copy moved there: the caller's object stays where it is."""
    dev = torch.empty(0, device=dev).device                # (with its index, as a tensor's device reads)
    if lm.device == dev:
        return lm
    lm = copy.copy(lm)
    lm._cache = {}
    return lm.to(dev)


def _ngram_beside(lm, scores, what):
    if lm.device != scores.device:
        raise RuntimeError(f"the n-gram tables are on {lm.device}, {what} on {scores.device}: NgramLm.to(device)")


def _lm_follows(lm, dev):
    """A decoding class' LM follows the inputs to their device on first use (the task does not own it)."""
    if isinstance(lm, torch.nn.Module):
        p = next(lm.parameters(), None)
        if p is not None and p.device != dev:
            lm.to(dev)
    elif _is_ngram(lm):
        lm.to(dev)


def ctc_prefix_beam_tokens(logits, lengths, beam_size=4, cutoff_top_k=4, blank=0):
    """CTC prefix beam search with equal prefixes merged: (B,T,V) device logits (raw or normalised) ->
    (tokens (B,T) int64, out_len (B) int64, score (B) fp32: log-probability of the best prefix summed
    over its alignments), or None when the kernel does not take the shape.  HIP: decode_ctc.hip."""
    def plan(x, n):
        (B, T, V), beam, topk = x.shape, int(beam_size), int(cutoff_top_k)
        return N.lib().s2t_ctc_prefix_beam_workspace_bytes(B, T, V, beam), lambda tail: N.lib().s2t_ctc_prefix_beam(
            N.fp(x), N.lp(n), B, T, V, int(blank), beam, topk, *tail), None
    return _whole_utterance("s2t_ctc_prefix_beam", "device CTC prefix beam search", logits, lengths, plan)


def ctc_prefix_beam_lm_tokens(logits, lengths, lm, lm_weight, beam_size=4, cutoff_top_k=4, blank=0,
                              lm_start_token=None):
    """ctc_prefix_beam_tokens with RNN-LM shallow fusion: prefixes rank by their log-probability plus
    lm_weight * (the LM's log-probability of their tokens).  lm_start_token as in
    rnnt_beam_lstm_lm_tokens_from_am.  -> (tokens, out_len, score (the acoustic part), lm_score (B) fp32:
    the best prefix' unweighted LM sum), or None when the kernels do not take the shape."""
    def plan(x, n):
        start = _lm_start_arg(lm_start_token)
        lm_desc, keep = rnn_lm_desc(lm)
        (B, T, V), beam, topk = x.shape, int(beam_size), int(cutoff_top_k)
        if lm_desc is None:
            return None
        return N.lib().s2t_ctc_prefix_beam_lm_workspace_bytes(lm_desc, B, T, V, beam), \
            lambda tail: N.lib().s2t_ctc_prefix_beam_lm(lm_desc, N.fp(x), N.lp(n), B, T, V, int(blank), beam, topk,
                                                        float(lm_weight), start, *tail), keep
    return _whole_utterance("s2t_ctc_prefix_beam_lm", "device CTC prefix beam search", logits, lengths, plan,
                            lm_score=True)


def ctc_prefix_beam_ngram_tokens(logits, lengths, lm, lm_weight, beam_size=4, cutoff_top_k=4, blank=0):
    """ctc_prefix_beam_tokens with back-off n-gram shallow fusion (lm: an NgramLm whose fp32 tables are on
    the logits' device), in ONE launch: an extension is scored by the n-gram look-up inside the frame
    body and a kept prefix carries the context that look-up returned.  The search starts in the LM's
    own start context, so the first token is scored too.  -> (tokens, out_len, score (the acoustic
    part), lm_score (B) fp32: the best prefix' unweighted LM sum), or None where the entry refuses.
    HIP: decode_ctc.hip, ngram_lookup.h."""
    def plan(x, n):
        _ngram_beside(lm, x, "the logits")
        (B, T, V), beam, topk = x.shape, int(beam_size), int(cutoff_top_k)
        nbytes = N.lib().s2t_ctc_prefix_beam_ngram_workspace_bytes(B, T, V, beam)
        if nbytes <= 0:
            return None
        lm_desc, keep = lm.desc()
        return nbytes, lambda tail: N.lib().s2t_ctc_prefix_beam_ngram(
            lm_desc, N.fp(x), N.lp(n), B, T, V, int(blank), beam, topk, float(lm_weight), int(lm.start_ctx), *tail), keep
    return _whole_utterance("s2t_ctc_prefix_beam_ngram", "device CTC prefix beam search", logits, lengths, plan,
                            lm_score=True)


def _logaddexp(a, b):
    """Of two Python floats; -inf is the empty sum."""
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


class CtcPrefixBeamDecoding(_BatchDecoding):
    """Lexicon-free CTC prefix beam search (the reference's CTC beam decoder wraps a lexicon decoder of
    a library that is not here; this one searches the model's own classes).  A live prefix carries
    the log-probabilities of its alignments ending in blank and in a non-blank; per frame the
    `cutoff_top_k` classes by (logit descending, class ascending) extend every prefix, candidates that
    spell the same tokens are merged into one, the `beam_size` best survive.

    With `lm` (an RnnLm, an NgramLm, or anything with init_states / score_step) prefixes rank by their
    log-probability plus `lm_weight` times the LM's log-probability of their tokens; `lm_start_token`
    as in RnntBeamDecoding.  An LM that has `start_scores` (NgramLm) scores the first token too, from
    its own start state, and takes no `lm_start_token`.  Device logits run the fused search
    (csrc/decode_ctc.hip; with an LM when it is this project's RnnLm, in lockstep rounds, or NgramLm, in
    one launch, its tables following the logits to their device); CPU tensors, shapes the kernels
    refuse and foreign LMs run `_module_loop`.
    `beam_tokens` returns (tokens, out_len, score) and with an LM a fourth tensor, the best prefix'
    unweighted LM sum.

    The subclass CtcBiasPrefixBeamDecoding (model/ctc_bias.py) gives the search a context (a ContextGraph:
    hotwords): prefixes then rank with `context_weight` times their bias_sum added and the reported prefix is
    the best one once every unfinished match has been paid back (the bias statement and the finalisation:
    model/lm/context_graph.py, include/s2t_mi355.h); `beam_tokens` then returns one more tensor at the end, the
    reported prefix' bias_score.  The search itself, host loop and dispatch, is this class' either way."""

    def __init__(self, tokenizer, beam_size=4, cutoff_top_k=4, lm=None, lm_weight=0.0, lm_start_token=None) -> None:
        self._tokenizer = tokenizer
        self._beam_size = int(beam_size)
        self._cutoff_top_k = int(cutoff_top_k)
        self._lm = lm
        self._lm_weight = float(lm_weight)
        self._lm_start_token = None if lm_start_token is None else _lm_start_arg(lm_start_token)
        if self._beam_size < 1 or self._cutoff_top_k < 1:
            raise ValueError(f"beam_size and cutoff_top_k must be at least 1, got {beam_size!r}, {cutoff_top_k!r}")
        if self._lm_start_token is not None and _is_ngram(lm):
            raise ValueError("an NgramLm starts in its own <s> context: lm_start_token must be None")
        self._context, self._context_weight = None, 0.0    # (hotwords: CtcBiasPrefixBeamDecoding sets them)

    def _module_loop(self, hidden_states, blank=0):
        """(1,T,V) -> (tokens, score, lm_score) of the best prefix, with a context (tokens, score, lm_score,
        bias_score) of the reported one: the same search on the host.  The
        log-softmax, the top-k and the LM run in torch on the inputs' device (in their dtype, fp32 at
        least); the per-prefix recursion runs on Python floats keyed by token tuples."""
        x = hidden_states[0]
        x = x.to(torch.promote_types(x.dtype, torch.float32))
        T, V = x.shape
        dev = x.device
        k = min(self._cutoff_top_k, V)
        lm, weight = self._lm, self._lm_weight
        graph, bias_weight = self._context, self._context_weight
        bias = {(): (0, 0.0)}                              # live prefix -> (graph state, bias_sum)
        info = {}                                          # live prefix -> (q as a list, LM state, lm_sum)
        if lm is not None:
            state, q = lm.init_states(1), [0.0] * V
            if hasattr(lm, "start_scores"):                # (an n-gram scores the first token too)
                q = lm.start_scores(state)[0].double().tolist()
            elif self._lm_start_token is not None:
                qt, state = lm.score_step(torch.full((1,), self._lm_start_token, dtype=torch.int64, device=dev),
                                          state)
                q = qt[0].double().tolist()
            info[()] = (q, state, 0.0)
        beam = [((), 0.0, -math.inf)]
        if T > 0:
            order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :k]
            lps = torch.log_softmax(x, dim=-1).gather(1, order).double().tolist()
            order = order.tolist()
        for t in range(T):
            live = {p for p, _, _ in beam}
            cand = {}                                      # tokens -> [pb, pnb, key, parent prefix]
            for i, (p, pb, pnb) in enumerate(beam):
                s = _logaddexp(pb, pnb)
                for r, (c, lp) in enumerate(zip(order[t], lps[t])):
                    if c == blank:
                        e = cand.setdefault(p, [-math.inf, -math.inf, (i, 0, 0)])
                        e[0] = _logaddexp(e[0], s + lp)
                        continue
                    if p and c == p[-1]:
                        if pnb + lp != -math.inf:
                            e = cand.setdefault(p, [-math.inf, -math.inf, (i, 0, 0)])
                            e[1] = _logaddexp(e[1], pnb + lp)
                        v = pb + lp
                    else:
                        v = s + lp
                    if v != -math.inf:
                        e = cand.setdefault(p + (c,), [-math.inf, -math.inf, (i, 1, r)])
                        e[1] = _logaddexp(e[1], v)
            ranked = []
            for tokens, (pb, pnb, key) in cand.items():
                lm_sum = 0.0
                if lm is not None:
                    lm_sum = info[tokens][2] if tokens in live else info[tokens[:-1]][2] + info[tokens[:-1]][0][tokens[-1]]
                total = _logaddexp(pb, pnb) + weight * lm_sum
                bias_of = None
                if graph is not None:
                    if tokens in live:
                        bias_of = bias[tokens]
                    else:
                        state, bias_sum = bias[tokens[:-1]]
                        hit, nxt = graph._row(state)
                        bias_of = (int(nxt[tokens[-1]]), bias_sum + float(hit[tokens[-1]]))
                    total = total + bias_weight * bias_of[1]
                ranked.append((-total, key, tokens, pb, pnb, lm_sum, bias_of))
            ranked.sort(key=lambda e: e[:2])
            ranked = ranked[:self._beam_size]
            bias = {e[2]: e[6] for e in ranked}
            if lm is not None:
                new_info = {}
                for _, _, tokens, _, _, lm_sum, _ in ranked:
                    if tokens in live:
                        new_info[tokens] = info[tokens]
                    else:
                        qt, state = lm.score_step(torch.full((1,), tokens[-1], dtype=torch.int64, device=dev),
                                                  info[tokens[:-1]][1])
                        new_info[tokens] = (qt[0].double().tolist(), state, lm_sum)
                info = new_info
            beam = [(e[2], e[3], e[4]) for e in ranked]
        if graph is not None:                              # the finalisation: the loan of an unfinished match goes back
            final = graph.final_scores(torch.tensor([bias[p][0] for p, _, _ in beam])).double().tolist()
            totals = [(_logaddexp(pb, pnb) + weight * (info[p][2] if lm is not None else 0.0))
                      + bias_weight * (bias[p][1] + f) for (p, pb, pnb), f in zip(beam, final)]
            pos = max(range(len(beam)), key=lambda i: (totals[i], -i))
            p, pb, pnb = beam[pos]
            return list(p), _logaddexp(pb, pnb), (info[p][2] if lm is not None else 0.0), bias[p][1] + final[pos]
        p, pb, pnb = beam[0]
        return list(p), _logaddexp(pb, pnb), (info[p][2] if lm is not None else 0.0)

    def _fused(self, hidden_states, inputs_length):
        from speech2text_amd.model.lm.rnn_lm import RnnLm
        if not hidden_states.is_cuda:
            return None
        if self._context is not None:
            if self._context.dtype != torch.float32 or not (self._lm is None or (
                    _is_ngram(self._lm) and self._lm.dtype == torch.float32)):
                return None
            from speech2text_amd.model.ctc_bias import ctc_prefix_beam_bias_tokens
            return ctc_prefix_beam_bias_tokens(hidden_states, inputs_length, self._context, self._context_weight,
                                               self._lm, self._lm_weight, self._beam_size, self._cutoff_top_k)
        if self._lm is None:
            return ctc_prefix_beam_tokens(hidden_states, inputs_length, self._beam_size, self._cutoff_top_k)
        if _is_ngram(self._lm):
            if self._lm.dtype != torch.float32:
                return None
            return ctc_prefix_beam_ngram_tokens(hidden_states, inputs_length, self._lm, self._lm_weight,
                                                self._beam_size, self._cutoff_top_k)
        if not isinstance(self._lm, RnnLm):
            return None
        return ctc_prefix_beam_lm_tokens(hidden_states, inputs_length, self._lm, self._lm_weight, self._beam_size,
                                         self._cutoff_top_k, lm_start_token=self._lm_start_token)

    @torch.no_grad()
    def beam_tokens(self, hidden_states, inputs_length, fused=True):
        """(B,T,V) logits -> (tokens (B,T), out_len (B), score (B)) of the best prefix per utterance, and
        with an LM its lm_score (B).  The fused device search where it applies (and `fused` is left
        on), else the host loop per utterance."""
        dev = hidden_states.device
        _lm_follows(self._lm, dev)
        if self._context is not None:
            self._context.to(dev)
        if fused:
            out = self._fused(hidden_states, inputs_length)
            if out is not None:
                return out
        B, T = hidden_states.shape[0], hidden_states.shape[1]
        tokens = torch.zeros((B, T), dtype=torch.int64)
        out_len = torch.zeros((B,), dtype=torch.int64)
        score = torch.zeros((B,), dtype=torch.float32)
        lm_score = torch.zeros((B,), dtype=torch.float32)
        bias_score = torch.zeros((B,), dtype=torch.float32)
        for b in range(B):
            n = max(0, min(int(inputs_length[b]), T))
            res = self._module_loop(hidden_states[b:b + 1, :n, :])
            tok, score[b], lm_score[b] = res[:3]
            if self._context is not None:
                bias_score[b] = res[3]
            out_len[b] = len(tok)
            tokens[b, :len(tok)] = torch.tensor(tok, dtype=torch.int64)
        out = (tokens.to(dev), out_len.to(dev), score.to(dev))
        out = out + (lm_score.to(dev),) if self._lm is not None else out
        return out + (bias_score.to(dev),) if self._context is not None else out

    @torch.no_grad()
    def decode_batch(self, hidden_states, inputs_length):
        out = self.beam_tokens(hidden_states, inputs_length)
        return _to_texts(out[0], out[1], self._tokenizer)


def _is_lstm_pair(predictor, joiner):
    """The modules csrc/decode_lstm.hip serves: LstmPredictor + Joiner (any out-projection)."""
    from speech2text_amd.model.joiner.joiner import Joiner
    from speech2text_amd.model.predictor.lstm_predictor import LstmPredictor
    return isinstance(getattr(predictor, "predictor", predictor), LstmPredictor) and isinstance(joiner, Joiner)


def _kept_f32(keep, address=N.fp):
    """-> a(t): the address of t detached, contiguous and fp32 (t itself where it is that already), which is
    appended to `keep`; None stays None.  N.fp raises for a tensor off the device."""
    def a(t):
        if t is None:
            return None
        t = t.detach().contiguous().float()
        keep.append(t)
        return address(t)
    return a


def rnnt_lstm_desc(predictor, joiner):
    """-> (S2tRnntLstmDesc of the two modules' fp32 device parameters, the tensors it points to:
    keep them alive while the descriptor is in use)."""
    p = getattr(predictor, "predictor", predictor)._predictor
    keep = []
    a = _kept_f32(keep)
    d = N.struct("S2tRnntLstmDesc")()
    layers = list(p.lstm_layers)
    if len(layers) > N.const("S2T_RNNT_LSTM_MAX_LAYERS") or p.embedding.num_embeddings < joiner._output_dim:
        return None, keep                                  # (every class must have an embedding row)
    ln = isinstance(layers[0].g_norm, torch.nn.LayerNorm)
    d.V, d.E, d.H, d.D = joiner._output_dim, p.embedding.embedding_dim, layers[0].hidden_dim, \
        p.linear.out_features
    d.inner = joiner._inner_dim if joiner._use_out_project else 0
    d.num_layers, d.layer_norm, d.act = len(layers), int(ln), 0 if joiner._act_name == "relu" else 1
    d.in_eps, d.out_eps = p.input_layer_norm.eps, p.output_layer_norm.eps
    d.lstm_eps = layers[0].g_norm.eps if ln else 0.0
    d.emb, d.in_gamma, d.in_beta = a(p.embedding.weight), a(p.input_layer_norm.weight), \
        a(p.input_layer_norm.bias)
    for i, m in enumerate(layers):
        L = d.layers[i]
        L.x2g_w, L.x2g_b, L.p2g_w = a(m.x2g.weight), a(m.x2g.bias), a(m.p2g.weight)
        if ln:
            L.g_gamma, L.g_beta, L.c_gamma, L.c_beta = a(m.g_norm.weight), a(m.g_norm.bias), \
                a(m.c_norm.weight), a(m.c_norm.bias)
    d.lin_w, d.lin_b = a(p.linear.weight), a(p.linear.bias)
    d.out_gamma, d.out_beta = a(p.output_layer_norm.weight), a(p.output_layer_norm.bias)
    d.pre_w, d.pre_b = a(joiner._pre_proj.weight), a(joiner._pre_proj.bias)
    if joiner._use_out_project:
        o1, o2 = joiner._out_projection[0], joiner._out_projection[1]
        d.out1_w, d.out1_b, d.out2_w, d.out2_b = a(o1.weight), a(o1.bias), a(o2.weight), a(o2.bias)
    keep.append(d)
    return ctypes.byref(d), keep


def _beam_in_range(beam):
    return 1 <= beam <= N.const("S2T_RNNT_LSTM_MAX_BEAM")


def rnnt_greedy_lstm_tokens_from_am(am, lengths, predictor, joiner, max_token_step=10):
    """Lockstep device greedy search on a given am = joiner._enc_proj(encoder_out), (B,T,V) fp32, LSTM
    predictor.  -> (tokens (B, T (max_token_step + 1)) int64, out_len (B) int64), or None when the
    kernels do not take the shape (the caller runs the module loop).  HIP: decode_lstm.hip."""
    def plan(am, n):
        B, T, _ = am.shape
        desc, keep = rnnt_lstm_desc(predictor, joiner)
        nbytes = N.lib().s2t_rnnt_lstm_workspace_bytes(desc, B, T, 0) if desc is not None else 0
        if nbytes <= 0 or max_token_step < 0:
            return None
        return nbytes, lambda tail: N.lib().s2t_rnnt_greedy_lstm(desc, N.fp(am), N.lp(n), B, T, int(max_token_step),
                                                                 *tail), keep
    return _whole_utterance("s2t_rnnt_greedy_lstm", "device RNN-T greedy search", am, lengths, plan, score=False,
                            per_frame=int(max_token_step) + 1)


def rnnt_beam_lstm_tokens_from_am(am, lengths, predictor, joiner, beam_size=4, cutoff_top_k=4):
    """rnnt_beam_tokens_from_am for the LSTM predictor (joiner with or without out-projection):
    same outputs, or None when the kernels do not take the shape.  HIP: decode_lstm.hip."""
    def plan(am, n):
        B, T, _ = am.shape
        desc, keep = rnnt_lstm_desc(predictor, joiner)
        beam, topk = int(beam_size), int(cutoff_top_k)
        if desc is None or not _beam_in_range(beam):
            return None
        return N.lib().s2t_rnnt_lstm_workspace_bytes(desc, B, T, beam), lambda tail: N.lib().s2t_rnnt_beam_lstm(
            desc, N.fp(am), N.lp(n), B, T, beam, topk, *tail), keep
    return _whole_utterance("s2t_rnnt_beam_lstm", "device RNN-T beam search", am, lengths, plan, frames=True)


def rnn_lm_desc(lm):
    """-> (S2tRnnLmDesc of an RnnLm's fp32 device parameters, the tensors it points to: keep them
    alive while the descriptor is in use).  A layer's two biases are summed once into a kept tensor."""
    keep = []
    a = _kept_f32(keep)
    st = lm._rnn_layer
    if st.num_layers > N.const("S2T_RNNT_LSTM_MAX_LAYERS"):
        return None, keep
    d = N.struct("S2tRnnLmDesc")()
    d.V, d.E, d.H, d.num_layers = lm._num_symbols, st.input_size, st.hidden_size, st.num_layers
    d.emb = a(lm._embedding.weight)
    for k in range(st.num_layers):
        L = d.layers[k]
        L.x2g_w, L.p2g_w = a(getattr(st, f"weight_ih_l{k}")), a(getattr(st, f"weight_hh_l{k}"))
        L.x2g_b = a(getattr(st, f"bias_ih_l{k}").detach().float() + getattr(st, f"bias_hh_l{k}").detach().float())
    d.out_w, d.out_b = a(lm._logits_layer.weight), a(lm._logits_layer.bias)
    keep.append(d)
    return ctypes.byref(d), keep


def rnnt_beam_lstm_lm_tokens_from_am(am, lengths, predictor, joiner, lm, lm_weight, beam_size=4, cutoff_top_k=4,
                                     lm_start_token=None):
    """rnnt_beam_lstm_tokens_from_am with RNN-LM shallow fusion: a candidate of class c != blank scores
    lm_weight * log p_lm(c | the beam's tokens) more.  lm_start_token None: the LM starts from zero
    state and the first token carries no LM term (RnnLm.score's convention); a token: the LM is first
    stepped on it.  -> (tokens, frames, out_len, score, lm_score (B) fp32: the best beam's unweighted
    LM sum), or None when the kernels do not take the shape.  HIP: decode_lstm.hip."""
    def plan(am, n):
        B, T, _ = am.shape
        desc, keep = rnnt_lstm_desc(predictor, joiner)
        lm_desc, lm_keep = rnn_lm_desc(lm)
        beam, topk = int(beam_size), int(cutoff_top_k)
        start = _lm_start_arg(lm_start_token)
        if desc is None or lm_desc is None or not _beam_in_range(beam):
            return None
        return N.lib().s2t_rnnt_beam_lstm_lm_workspace_bytes(desc, lm_desc, B, T, beam), \
            lambda tail: N.lib().s2t_rnnt_beam_lstm_lm(desc, lm_desc, N.fp(am), N.lp(n), B, T, beam, topk,
                                                       float(lm_weight), start, *tail), (keep, lm_keep)
    return _whole_utterance("s2t_rnnt_beam_lstm_lm", "device RNN-T beam search", am, lengths, plan, frames=True,
                            lm_score=True)


def rnnt_beam_lstm_ngram_tokens_from_am(am, lengths, predictor, joiner, lm, lm_weight, beam_size=4, cutoff_top_k=4):
    """rnnt_beam_lstm_tokens_from_am with back-off n-gram shallow fusion (lm: an NgramLm whose fp32 tables
    are on am's device): the lockstep rounds in their n-gram mode, a look-up per candidate inside the expand
    launch and no LM step.  The search starts in the LM's own start context, so the first token is scored
    too.  -> (tokens, frames, out_len, score, lm_score (B) fp32: the best beam's unweighted LM sum), or
    None where the entry refuses.  HIP: decode_lstm.hip, ngram_lookup.h."""
    def plan(am, n):
        B, T, _ = am.shape
        _ngram_beside(lm, am, "am")
        desc, keep = rnnt_lstm_desc(predictor, joiner)
        beam, topk = int(beam_size), int(cutoff_top_k)
        if desc is None or lm.dtype != torch.float32:
            return None
        lm_desc, lm_keep = lm.desc()
        return N.lib().s2t_rnnt_beam_lstm_ngram_workspace_bytes(desc, lm_desc, B, T, beam), \
            lambda tail: N.lib().s2t_rnnt_beam_lstm_ngram(desc, lm_desc, N.fp(am), N.lp(n), B, T, beam, topk,
                                                          float(lm_weight), int(lm.start_ctx), *tail), (keep, lm_keep)
    return _whole_utterance("s2t_rnnt_beam_lstm_ngram", "device RNN-T beam search", am, lengths, plan, frames=True,
                            lm_score=True)


def _is_stateless_pair(predictor, joiner):
    """The modules s2t_rnnt_beam_stateless_lm serves: StatelessPredictor + Joiner (any out-projection)."""
    from speech2text_amd.model.joiner.joiner import Joiner
    from speech2text_amd.model.predictor.predictor import StatelessPredictor
    return isinstance(getattr(predictor, "predictor", predictor), StatelessPredictor) and isinstance(joiner, Joiner)


def rnnt_stateless_desc(predictor, joiner):
    """rnnt_lstm_desc for the stateless predictor -> (S2tRnntStatelessDesc of the two modules' fp32
    parameters, the tensors it points to: keep them alive while the descriptor is in use), or
    (None, []) for anything that is not StatelessPredictor + Joiner."""
    keep = []
    if not _is_stateless_pair(predictor, joiner):
        return None, keep
    p = getattr(predictor, "predictor", predictor)
    a = _kept_f32(keep, torch.Tensor.data_ptr)             # (host modules describe too: the searches check)
    if p._embedding.num_embeddings < joiner._output_dim:   # (every class must have an embedding row)
        return None, keep
    d = N.struct("S2tRnntStatelessDesc")()
    d.V, d.E, d.D, d.ctx = joiner._output_dim, p._embedding_dim, p._output_dim, p._context_size
    d.inner = joiner._inner_dim if joiner._use_out_project else 0
    d.act = 0 if joiner._act_name == "relu" else 1
    d.emb, d.conv_w = a(p._embedding.weight), a(p._conv.weight.reshape(p._embedding_dim, p._context_size))
    d.lin_w, d.lin_b = a(p._output_linear.weight), a(p._output_linear.bias)
    d.pre_w, d.pre_b = a(joiner._pre_proj.weight), a(joiner._pre_proj.bias)
    if joiner._use_out_project:
        o1, o2 = joiner._out_projection[0], joiner._out_projection[1]
        d.out1_w, d.out1_b, d.out2_w, d.out2_b = a(o1.weight), a(o1.bias), a(o2.weight), a(o2.bias)
    keep.append(d)
    return ctypes.byref(d), keep


def rnnt_beam_stateless_lm_tokens_from_am(am, lengths, predictor, joiner, lm, lm_weight, beam_size=4,
                                          cutoff_top_k=4, lm_start_token=None):
    """rnnt_beam_lstm_lm_tokens_from_am for the stateless predictor (joiner with or without
    out-projection): the same lockstep rounds, LM step and outputs, the predictor step being one row
    kernel and two tiled products.  -> (tokens, frames, out_len, score, lm_score), or None when the
    kernels do not take the modules or the shape.  HIP: decode_lstm.hip."""
    def plan(am, n):
        B, T, _ = am.shape
        start = _lm_start_arg(lm_start_token)
        desc, keep = rnnt_stateless_desc(predictor, joiner)
        lm_desc, lm_keep = rnn_lm_desc(lm)
        beam, topk = int(beam_size), int(cutoff_top_k)
        if desc is None or lm_desc is None or not _beam_in_range(beam):
            return None
        if any(not t.is_cuda for t in keep[:-1]):
            raise RuntimeError("the device RNN-T beam search runs on the GPU only: the modules are not on it")
        return N.lib().s2t_rnnt_beam_stateless_lm_workspace_bytes(desc, lm_desc, B, T, beam), \
            lambda tail: N.lib().s2t_rnnt_beam_stateless_lm(desc, lm_desc, N.fp(am), N.lp(n), B, T, beam, topk,
                                                            float(lm_weight), start, *tail), (keep, lm_keep)
    return _whole_utterance("s2t_rnnt_beam_stateless_lm", "device RNN-T beam search", am, lengths, plan, frames=True,
                            lm_score=True)


def _am_per_utterance(joiner, hidden_states, inputs_length):
    """am (B,T,V) = enc_proj(encoder_out), formed utterance by utterance on the frames an utterance
    has: the product decode() forms for the same utterance alone, so that a batched search and a
    per-utterance one see the same bits.  -> (am, lengths clamped to [0, T])."""
    B, T = hidden_states.shape[0], hidden_states.shape[1]
    lens = [max(0, min(int(n), T)) for n in inputs_length.tolist()]
    am = torch.zeros((B, T, joiner._output_dim), dtype=torch.float32, device=hidden_states.device)
    for b, n in enumerate(lens):
        if n:
            am[b, :n] = joiner._enc_proj(hidden_states[b:b + 1, :n, :])[0].float()
    return am, torch.tensor(lens, dtype=torch.int64)


class RnntGreedyDecoding(DecodingMethod):
    def __init__(self, tokenizer, predictor, joiner, max_token_step=10):
        self._tokenizer = tokenizer
        self._predictor = predictor
        self._joiner = joiner
        self._max_token_step = max_token_step
        assert hasattr(self._predictor, "streaming_step") and hasattr(self._joiner, "streaming_step"), \
            "Predictor and Joiner should impl streaming_step for decoding."

    def _fusable(self):
        from speech2text_amd.model.predictor.predictor import StatelessPredictor
        p = getattr(self._predictor, "predictor", self._predictor)
        return isinstance(p, StatelessPredictor) and not self._joiner._use_out_project

    def _fused(self):
        """The fused device search serves these modules: fusable, and the kernel's rules hold (its
        per-utterance vectors of E + D + V floats and the ctx-token state fit 60 KB of shared
        memory, ctx <= 64 -- csrc/decode.hip).  Otherwise: the module-by-module lattice walk."""
        if not self._fusable():
            return False
        p = getattr(self._predictor, "predictor", self._predictor)
        need = 4 * (p._embedding_dim + p._output_dim + self._joiner._output_dim) + 4 * p._context_size
        return need <= 60 * 1024 and p._context_size <= 64

    def greedy_tokens(self, hidden_states, inputs_length):
        """(B,T,D) encoder output -> (tokens (B,max_out), out_len (B)); fused device search."""
        am = self._joiner._enc_proj(hidden_states).contiguous().float()          # (B,T,V), one GEMM
        B, T, V = am.shape
        dev = am.device
        n = inputs_length.to(device=dev, dtype=torch.int64).contiguous()
        max_out = T * (self._max_token_step + 1)
        tokens = torch.zeros((B, max_out), dtype=torch.int64, device=dev)
        out_len = torch.zeros((B,), dtype=torch.int64, device=dev)
        w, E, D, ctx, act = _stateless_weights(self._predictor, self._joiner)
        N.check(N.lib().s2t_rnnt_greedy_stateless(
            N.fp(am), N.lp(n), *[N.fp(t) for t in w], B, T, V, E, D, ctx, act, int(self._max_token_step), max_out, 0,
            N.lp(tokens), N.lp(out_len), N.stream()), "s2t_rnnt_greedy_stateless")
        return tokens, out_len

    def _lstm_search(self):
        """The lockstep device search of csrc/decode_lstm.hip serves these modules."""
        return _is_lstm_pair(self._predictor, self._joiner)

    def greedy_tokens_lstm(self, hidden_states, inputs_length):
        """(B,T,D) encoder output -> (tokens (B,max_out), out_len (B)) by the lockstep device
        search, or None when the kernels refuse the shape."""
        am, lens = _am_per_utterance(self._joiner, hidden_states, inputs_length)
        return rnnt_greedy_lstm_tokens_from_am(am, lens, self._predictor, self._joiner,
                                               self._max_token_step)

    @torch.no_grad()
    def decode_batch(self, hidden_states, inputs_length):
        if self._fused():
            return _to_texts(*self.greedy_tokens(hidden_states, inputs_length), self._tokenizer)
        if self._lstm_search() and hidden_states.is_cuda:
            out = self.greedy_tokens_lstm(hidden_states, inputs_length)
            if out is not None:
                return _to_texts(*out, self._tokenizer)
            return [self._module_loop(hidden_states[i:i + 1, :int(inputs_length[i]), :])
                    for i in range(hidden_states.shape[0])]
        return super().decode_batch(hidden_states, inputs_length)

    @torch.no_grad()
    def decode(self, hidden_states: torch.Tensor) -> str:
        assert hidden_states.shape[0] == 1, "Support BatchSize = 1 only."
        if self._fused() or (self._lstm_search() and hidden_states.is_cuda):
            n = torch.tensor([hidden_states.shape[1]], dtype=torch.int64)
            return self.decode_batch(hidden_states, n)[0]
        return self._module_loop(hidden_states)

    def _module_loop(self, hidden_states: torch.Tensor) -> str:
        """module-by-module lattice walk (reference :237-271) for the combinations no device search
        serves, and for the shapes one refuses"""
        pred_state = self._predictor.init_state()
        T = hidden_states.shape[1]
        t = 0
        cur = torch.zeros((1, 1), dtype=torch.int64, device=hidden_states.device)
        nts = 0
        pred_out, pred_state = self._predictor.streaming_step(cur, pred_state)
        out = []
        while t < T:
            logp = self._joiner.streaming_step(hidden_states[:, t:t + 1, :], pred_out)
            tok = int(logp.argmax(dim=-1))
            if tok == 0 or nts > self._max_token_step:
                t += 1
                nts = 0
            else:
                nts += 1
                cur = torch.full((1, 1), tok, dtype=torch.int64, device=hidden_states.device)
                pred_out, pred_state = self._predictor.streaming_step(cur, pred_state)
                out.append(tok)
        return self._tokenizer.decode(torch.tensor(out, dtype=torch.int64))


def _stateless_weights(predictor, joiner, dev=None):
    """The six parameter tensors of the one-workgroup searches (embedding, conv [E][ctx], linear w / b,
    pre_proj w / b), fp32 and contiguous, on `dev` (None: where they are) -> (list, E, D, ctx, act).  The
    only place that gathers them: the whole-utterance greedy and beam searches and the chunk-carried ones
    call it.  A module held in another dtype is cast here (the greedy and the plain beam search used to
    raise for one)."""
    p = getattr(predictor, "predictor", predictor)
    # .to() and .contiguous() return the tensor itself for an fp32 contiguous parameter that is on `dev`:
    # the kernels then get the module's own pointers and a call makes no copy (the reshaped conv weight is
    # a view of the parameter's storage)
    f32 = lambda t: t.detach().to(device=dev or t.device, dtype=torch.float32).contiguous()   # noqa: E731
    w = [f32(p._embedding.weight), f32(p._conv.weight.reshape(p._embedding_dim, p._context_size)),
         f32(p._output_linear.weight), f32(p._output_linear.bias),
         f32(joiner._pre_proj.weight), f32(joiner._pre_proj.bias)]
    return w, p._embedding_dim, p._output_dim, p._context_size, 0 if joiner._act_name == "relu" else 1


def rnnt_beam_tokens_from_am(am, lengths, predictor, joiner, beam_size=4, cutoff_top_k=4):
    """Fused device beam search on a given am = joiner._enc_proj(encoder_out), (B,T,V) fp32.
    -> (tokens (B,T) int64, frames (B,T) int64, out_len (B) int64, score (B) fp32): the best
    beam's tokens, the frame at which each was emitted, their count and the beam's score.
    Returns None when the kernel does not take the shape (rc -1: the caller runs the module
    loop).  HIP: decode_rnnt.hip."""
    def plan(am, n):
        B, T, V = am.shape
        nbytes = max(1, N.lib().s2t_rnnt_beam_workspace_bytes(B, T, V, int(beam_size)))   # (the entry refuses, not this)
        w, E, D, ctx, act = _stateless_weights(predictor, joiner)
        return nbytes, lambda tail: N.lib().s2t_rnnt_beam_stateless(
            N.fp(am), N.lp(n), *[N.fp(t) for t in w], B, T, V, E, D, ctx, act, 0, int(beam_size), int(cutoff_top_k),
            *tail), w
    return _whole_utterance("s2t_rnnt_beam_stateless", "fused RNN-T beam search", am, lengths, plan, frames=True)


def rnnt_beam_ngram_tokens_from_am(am, lengths, predictor, joiner, lm, lm_weight, beam_size=4, cutoff_top_k=4):
    """rnnt_beam_tokens_from_am with back-off n-gram shallow fusion (lm: an NgramLm whose fp32 tables are
    on am's device), still ONE launch: the candidate of class c != blank scores lm_weight * log p_lm(c |
    the beam's context) more, looked up inside the frame body, and a kept beam carries the context the
    look-up returned.  The search starts in the LM's own start context, so the first token is scored
    too.  -> (tokens, frames, out_len, score, lm_score (B) fp32: the best beam's unweighted LM sum), or
    None where the entry refuses.  HIP: decode_rnnt.hip, decode_search.h, ngram_lookup.h."""
    def plan(am, n):
        B, T, V = am.shape
        _ngram_beside(lm, am, "am")
        beam, topk = int(beam_size), int(cutoff_top_k)
        nbytes = N.lib().s2t_rnnt_beam_ngram_workspace_bytes(B, T, V, beam)
        if nbytes <= 0:
            return None
        lm_desc, lm_keep = lm.desc()
        w, E, D, ctx, act = _stateless_weights(predictor, joiner)
        return nbytes, lambda tail: N.lib().s2t_rnnt_beam_stateless_ngram(
            lm_desc, N.fp(am), N.lp(n), *[N.fp(t) for t in w], B, T, V, E, D, ctx, act, 0, beam, topk,
            float(lm_weight), int(lm.start_ctx), *tail), (w, lm_keep)
    return _whole_utterance("s2t_rnnt_beam_stateless_ngram", "fused RNN-T beam search", am, lengths, plan,
                            frames=True, lm_score=True)


class RnntBeamDecoding(_BatchDecoding):
    """Beam search of the RNN-T (reference :295-425): at most one symbol per frame per beam, the
    `cutoff_top_k` best classes of every beam are expanded, the `beam_size` best candidates
    survive, equal hypotheses are not merged.  The orders the reference leaves to its library are
    fixed: top-k by (log-probability descending, class ascending), candidates by (score
    descending, parent beam position ascending, rank in the parent's top-k ascending).

    With `lm` (an RnnLm, an NgramLm, or anything with init_states / score_step) the search is
    shallow-fused: the candidate of class c != blank scores `lm_weight * log p_lm(c | the beam's tokens)`
    more, the cut to `cutoff_top_k` classes is still the RNN-T's own, blank carries no LM term.
    `lm_start_token` None: the LM starts from its initial state and, unless it has `start_scores`, a
    hypothesis' first token carries no LM term (how RnnLm.score scores a sequence); an LM with
    `start_scores` (NgramLm) scores the first token too, from its own start state; a token id: the LM
    is first stepped on it.  The LSTM predictor and the stateless predictor (with the project's Joiner
    and an RnnLm) run the fused device search (csrc/decode_lstm.hip); the stateless predictor with a
    projection-free Joiner and an NgramLm (no `lm_start_token`) runs the one-launch search fused with
    the n-gram (csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_ngram), the tables following the inputs to
    their device; everything else, and a shape the kernels refuse, `_module_loop_lm`.
    `beam_tokens` then returns a fifth tensor, the best beam's unweighted LM sum."""

    def __init__(self, tokenizer, predictor, joiner, beam_size=4, cutoff_top_k=4, lm=None, lm_weight=0.0,
                 lm_start_token=None) -> None:
        self._tokenizer = tokenizer
        self._predictor = predictor
        self._joiner = joiner
        self._beam_size = beam_size
        self._cutoff_top_k = cutoff_top_k
        self._lm = lm
        self._lm_weight = float(lm_weight)
        self._lm_start_token = None if lm_start_token is None else _lm_start_arg(lm_start_token)
        self._context, self._context_weight = None, 0.0    # (hotwords: RnntBiasBeamDecoding sets them)
        assert hasattr(self._predictor, "streaming_step") and hasattr(self._joiner, "streaming_step"), \
            "Predictor and Joiner should impl streaming_step for decoding."

    def _fusable(self):
        from speech2text_amd.model.joiner.joiner import Joiner
        from speech2text_amd.model.predictor.predictor import StatelessPredictor
        p = getattr(self._predictor, "predictor", self._predictor)
        return isinstance(p, StatelessPredictor) and isinstance(self._joiner, Joiner) \
            and not self._joiner._use_out_project

    def _lstm_search(self):
        """The lockstep device search of csrc/decode_lstm.hip serves these modules."""
        return _is_lstm_pair(self._predictor, self._joiner)

    def _module_loop(self, hidden_states):
        """(1,T,D) -> (tokens, frames, score) of the best beam: the reference's loop (:350-425)
        against init_state / streaming_step only, in plain torch on whatever device the inputs
        live.  Scores are accumulated in fp32 on that device (beam score + log-probability).  With a
        context (RnntBiasBeamDecoding): `_module_loop_lm` without the LM term, and its five results."""
        if self._context is not None:
            return self._module_loop_lm(hidden_states)
        dev = hidden_states.device
        blk = torch.zeros((1, 1), dtype=torch.int64, device=dev)
        pred_out, pred_state = self._predictor.streaming_step(blk, self._predictor.init_state())
        beams = [((), (), pred_state, pred_out)]            # (tokens, frames, state, pred_out)
        scores = torch.zeros((1,), dtype=torch.float32, device=dev)
        for t in range(hidden_states.shape[1]):
            log_probs = self._joiner.streaming_step(hidden_states[:, t:t + 1, :],
                                                    torch.cat([b[3] for b in beams], dim=0)).float()
            k = min(int(self._cutoff_top_k), log_probs.shape[-1])
            vals, cls = torch.sort(log_probs, dim=-1, descending=True, stable=True)
            cand = (scores.unsqueeze(1) + vals[:, :k]).flatten()      # index = parent * k + rank
            scores, pick = torch.sort(cand, descending=True, stable=True)
            scores, pick = scores[:self._beam_size], pick[:self._beam_size]
            new_beams = []
            for q, c in zip(pick.tolist(), cls[:, :k].flatten()[pick].tolist()):
                tokens, frames, state, out = beams[q // k]
                if c != 0:
                    out, state = self._predictor.streaming_step(
                        torch.full((1, 1), c, dtype=torch.int64, device=dev), state)
                    tokens, frames = tokens + (c,), frames + (t,)
                new_beams.append((tokens, frames, state, out))
            beams = new_beams
        return list(beams[0][0]), list(beams[0][1]), float(scores[0])

    def _module_loop_lm(self, hidden_states):
        """_module_loop with the LM term -> (tokens, frames, score, lm_score) of the best beam, over
        predictor.streaming_step, joiner.streaming_step and lm.score_step.  Scores are accumulated
        on the inputs' device in fp32 (fp64 where the modules compute in it) as (beam score +
        log-probability) + lm_weight * q, the order of the device search.
        With a context (a ContextGraph, through init_states / start_scores / score_step / final_scores; the LM
        may then be None): a candidate of class c != blank scores bias_weight * d more, behind the LM term,
        d = the graph's look-up from the beam's state; the reported beam is the one with the largest score +
        bias_weight * final_scores(state), ties to the lower position -> (tokens, frames, that value, lm_score,
        bias_score = the beam's sum of d + final_scores(state))."""
        dev = hidden_states.device
        lm, weight = self._lm, self._lm_weight
        graph, bias_weight = self._context, self._context_weight
        blk = torch.zeros((1, 1), dtype=torch.int64, device=dev)
        pred_out, pred_state = self._predictor.streaming_step(blk, self._predictor.init_state())
        lm_state, q = (lm.init_states(1), None) if lm is not None else (None, None)   # q None: all zeros
        bstates = graph.init_states(1).to(dev) if graph is not None else None
        bias_sums = None
        if lm is None:
            pass
        elif self._lm_start_token is not None:
            q, lm_state = lm.score_step(torch.full((1,), self._lm_start_token, dtype=torch.int64, device=dev),
                                        lm_state)
        elif hasattr(lm, "start_scores"):                  # (an n-gram scores the first token too)
            q = lm.start_scores(lm_state)
        beams = [((), (), pred_state, pred_out, lm_state, q)]   # (tokens, frames, state, pred_out, LM state, q (1,V))
        scores = lm_sums = None
        for t in range(hidden_states.shape[1]):
            log_probs = self._joiner.streaming_step(hidden_states[:, t:t + 1, :],
                                                    torch.cat([b[3] for b in beams], dim=0))
            log_probs = log_probs.to(torch.promote_types(log_probs.dtype, torch.float32))
            if scores is None:
                scores, lm_sums = log_probs.new_zeros(1), log_probs.new_zeros(1)
                bias_sums = log_probs.new_zeros(1)
            k = min(int(self._cutoff_top_k), log_probs.shape[-1])
            vals, cls = torch.sort(log_probs, dim=-1, descending=True, stable=True)
            vals, cls = vals[:, :k], cls[:, :k]
            qs = torch.cat([torch.zeros_like(log_probs[:1]) if b[5] is None else b[5].to(log_probs.dtype)
                            for b in beams], dim=0)
            qv = torch.where(cls != 0, qs.gather(1, cls), torch.zeros_like(vals))   # blank: no LM term
            cand = scores.unsqueeze(1) + vals                      # index = parent * k + rank
            if lm is not None:
                cand = cand + weight * qv
            if graph is not None:
                ds = graph.start_scores(bstates).to(device=dev, dtype=log_probs.dtype)
                dv = torch.where(cls != 0, ds.gather(1, cls), torch.zeros_like(vals))   # blank: no bias term
                cand = cand + bias_weight * dv
                cand_bias = (bias_sums.unsqueeze(1) + dv).flatten()
            cand = cand.flatten()
            cand_lm = (lm_sums.unsqueeze(1) + qv).flatten()
            scores, pick = torch.sort(cand, descending=True, stable=True)
            scores, pick = scores[:self._beam_size], pick[:self._beam_size]
            lm_sums = cand_lm[pick]
            new_beams, new_bstates = [], []
            for p, c in zip(pick.tolist(), cls.flatten()[pick].tolist()):
                tokens, frames, state, out, lm_state, q = beams[p // k]
                bstate = bstates[p // k:p // k + 1] if graph is not None else None
                if c != 0:
                    tok = torch.full((1, 1), c, dtype=torch.int64, device=dev)
                    out, state = self._predictor.streaming_step(tok, state)
                    if lm is not None:
                        q, lm_state = lm.score_step(tok.reshape(1), lm_state)
                    if graph is not None:
                        bstate = graph.score_step(tok.reshape(1), bstate)[1].to(dev)
                    tokens, frames = tokens + (c,), frames + (t,)
                new_beams.append((tokens, frames, state, out, lm_state, q))
                new_bstates.append(bstate)
            beams = new_beams
            if graph is not None:
                bias_sums, bstates = cand_bias[pick], torch.cat(new_bstates)
        if graph is not None:
            if scores is None:
                return [], [], 0.0, 0.0, 0.0
            fin = graph.final_scores(bstates).to(device=dev, dtype=scores.dtype)
            total = scores + bias_weight * fin
            pos = int(torch.sort(total, descending=True, stable=True)[1][0])
            return (list(beams[pos][0]), list(beams[pos][1]), float(total[pos]), float(lm_sums[pos]),
                    float(bias_sums[pos] + fin[pos]))
        if scores is None:
            return [], [], 0.0, 0.0
        return list(beams[0][0]), list(beams[0][1]), float(scores[0]), float(lm_sums[0])

    def _lm_to(self, dev):
        _lm_follows(self._lm, dev)

    def _device_searches(self):
        """The fused searches in the order they are tried: (serves these modules and this LM?, am formed for
        the whole batch by one _enc_proj (else per utterance, the lockstep searches' am), the
        whole-utterance function, its arguments after the modules).  A new search is a row here."""
        from speech2text_amd.model.lm.rnn_lm import RnnLm
        lm, lstm, sizes = self._lm, self._lstm_search(), (self._beam_size, self._cutoff_top_k)
        if self._context is not None:                      # hotwords: the one-workgroup search alone
            from speech2text_amd.model.rnnt_bias import rnnt_beam_bias_tokens_from_am
            serves = self._fusable() and self._context.dtype == torch.float32 and (lm is None or (
                _is_ngram(lm) and self._lm_start_token is None and lm.dtype == torch.float32))
            return [(serves, True, rnnt_beam_bias_tokens_from_am,
                     (self._context, self._context_weight, lm, self._lm_weight) + sizes)]
        if lm is None:
            return [(self._fusable(), True, rnnt_beam_tokens_from_am, sizes),
                    (lstm, False, rnnt_beam_lstm_tokens_from_am, sizes)]
        rnn = isinstance(lm, RnnLm)
        ngram = _is_ngram(lm) and self._lm_start_token is None and lm.dtype == torch.float32
        fused_lm, started = (lm, self._lm_weight) + sizes, (self._lm_start_token,)
        return [(lstm and rnn, False, rnnt_beam_lstm_lm_tokens_from_am, fused_lm + started),
                (lstm and ngram, False, rnnt_beam_lstm_ngram_tokens_from_am, fused_lm),
                (rnn and _is_stateless_pair(self._predictor, self._joiner), False,
                 rnnt_beam_stateless_lm_tokens_from_am, fused_lm + started),
                (ngram and self._fusable(), True, rnnt_beam_ngram_tokens_from_am, fused_lm)]

    @torch.no_grad()
    def beam_tokens(self, hidden_states, inputs_length, fused=True):
        """(B,T,D) encoder output -> (tokens (B,T), frames (B,T), out_len (B), score (B)) of the
        best beam per utterance, and with an LM its lm_score (B).  The fused device search where the
        modules allow it (and `fused` is left on), else the module loop per utterance."""
        dev, with_lm, with_bias = hidden_states.device, self._lm is not None, self._context is not None
        if with_lm:
            self._lm_to(dev)
        if with_bias:
            self._context.to(dev)
        searches = self._device_searches() if fused and hidden_states.is_cuda else []
        for serves, whole_batch, search, args in searches:
            if not serves:
                continue
            if whole_batch:
                am, lens = self._joiner._enc_proj(hidden_states), inputs_length   # (B,T,V), one GEMM
            else:
                am, lens = _am_per_utterance(self._joiner, hidden_states, inputs_length)
            out = search(am, lens, self._predictor, self._joiner, *args)
            if out is not None:
                return out
        B, T = hidden_states.shape[0], hidden_states.shape[1]
        tokens = torch.zeros((B, T), dtype=torch.int64)
        frames = torch.zeros((B, T), dtype=torch.int64)
        out_len = torch.zeros((B,), dtype=torch.int64)
        score = torch.zeros((B,), dtype=torch.float32)
        lm_score = torch.zeros((B,), dtype=torch.float32)
        bias_score = torch.zeros((B,), dtype=torch.float32)
        for b in range(B):
            n = max(0, min(int(inputs_length[b]), T))
            if with_bias:
                tok, frm, score[b], lm_score[b], bias_score[b] = self._module_loop_lm(hidden_states[b:b + 1, :n, :])
            elif with_lm:
                tok, frm, score[b], lm_score[b] = self._module_loop_lm(hidden_states[b:b + 1, :n, :])
            else:
                tok, frm, score[b] = self._module_loop(hidden_states[b:b + 1, :n, :])
            out_len[b] = len(tok)
            tokens[b, :len(tok)] = torch.tensor(tok, dtype=torch.int64)
            frames[b, :len(frm)] = torch.tensor(frm, dtype=torch.int64)
        out = (tokens.to(dev), frames.to(dev), out_len.to(dev), score.to(dev))
        out = out + (lm_score.to(dev),) if with_lm else out
        return out + (bias_score.to(dev),) if with_bias else out

    @torch.no_grad()
    def decode_batch(self, hidden_states, inputs_length):
        out = self.beam_tokens(hidden_states, inputs_length)
        return _to_texts(out[0], out[2], self._tokenizer)


def _method_arg(method):
    if method not in ("greedy", "beam"):
        raise ValueError(f"method must be 'greedy' or 'beam', got {method!r}")
    return method


def _stream_lm_arguments(lm, lm_weight, lm_start_token, method):
    """The LM arguments of a chunk-carried search, checked -> (lm, lm_weight, the C start token)."""
    if lm is None:
        return None, 0.0, -1
    from speech2text_amd.model.lm.rnn_lm import RnnLm
    if method == "greedy":
        raise ValueError("the greedy searches take no language model: use method='beam' or lm=None")
    if _is_ngram(lm):
        raise ValueError("this chunk-carried search is not fused with an NgramLm: the chunk-carried n-gram searches "
                         "are CtcNgramStreamingSearch (ctc_streaming_search), RnntLstmNgramStreamingSearch (the "
                         "LSTM predictor) and RnntNgramStreamingSearch (the stateless predictor with a "
                         "projection-free Joiner); pass an RnnLm, or lm=None")
    if not isinstance(lm, RnnLm):
        raise ValueError(f"the chunk-carried search is fused with an RnnLm only, got {type(lm).__name__} "
                         "(there is no module-loop fallback here)")
    start = _lm_start_arg(lm_start_token)
    if not math.isfinite(float(lm_weight)):
        raise ValueError(f"lm_weight must be finite, got {lm_weight!r}")
    return lm, float(lm_weight), start


class _ChunkCarriedSearch:
    """What every chunk-carried search is, RNN-T or CTC: the settings, the fixed output tensors (`frames`
    for RNN-T only, `lm_score` with an LM, else None), `reset` and `step` around the library calls.  A
    subclass' __init__ hands its arguments to `_construct`; it says what it takes and which class count
    follows (`_check_modules`), which shapes, and where its state and workspace live (`_allocate`: `state`,
    `_ws` and its descriptors), and makes the calls (`_reset_state`, `_chunk`).  `_lm_arguments` checks the
    LM (an RnnLm here; the n-gram classes override it) and `_views` is what `step` returns."""

    _input, _has_frames = "am", True                       # (the CTC classes: "logits", no frames)

    def _construct(self, what, batch_size, method, beam_size, cutoff_top_k, max_tokens, device, lm=None,
                   lm_weight=0.0, lm_start_token=None):
        """what: the arguments of _check_modules and _allocate, (predictor, joiner) or (num_classes,)."""
        self._lm, self._lm_weight, self._lm_start = self._lm_arguments(lm, lm_weight, lm_start_token, method)
        self.method = _method_arg(method)
        self.V, on_gpu = self._check_modules(*what)
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda" or any(t.device.type != "cuda" for t in on_gpu):
            raise RuntimeError("the chunk-carried search runs on the GPU only: modules, LM and device must be cuda")
        self.batch_size, self.max_tokens = int(batch_size), int(max_tokens)
        self.beam_size, self.cutoff_top_k = int(beam_size), int(cutoff_top_k)
        self._ws = None
        self._allocate(*what, dev)                         # raises for a shape the kernels refuse
        B = self.batch_size
        self.tokens = torch.zeros((B, self.max_tokens), dtype=torch.int64, device=dev)
        self.frames = torch.zeros((B, self.max_tokens), dtype=torch.int64, device=dev) if self._has_frames else None
        self.out_len = torch.zeros((B,), dtype=torch.int64, device=dev)
        self.score = torch.zeros((B,), dtype=torch.float32, device=dev)
        self.stable_len = torch.zeros((B,), dtype=torch.int64, device=dev)
        self.overflow = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.lm_score = None if self._lm is None else torch.zeros((B,), dtype=torch.float32, device=dev)
        self._outputs = [t for t in (self.tokens, self.frames, self.out_len, self.score, self.stable_len,
                                     self.overflow, self.lm_score) if t is not None]
        self._step_views = self._views()
        self._full = {}                                    # Tc -> chunk_len of a whole chunk
        self.reset()

    def _construct_rnnt(self, predictor, joiner, batch_size, method, max_token_step, beam_size, cutoff_top_k,
                        max_tokens, device, lm=None, lm_weight=0.0, lm_start_token=None):
        """_construct with the settings of an RNN-T search: `max_token_step`, and beam_size 0 for greedy."""
        self.max_token_step = int(max_token_step)
        self._construct((predictor, joiner), batch_size, method, beam_size if method == "beam" else 0, cutoff_top_k,
                        max_tokens, device, lm, lm_weight, lm_start_token)

    def _lm_arguments(self, lm, lm_weight, lm_start_token, method):
        return _stream_lm_arguments(lm, lm_weight, lm_start_token, method)

    def _lm_on_gpu(self):
        """The LM's tensors that must be on the GPU already (an n-gram's tables are copied over instead)."""
        return [] if self._lm is None or _is_ngram(self._lm) else [self._lm._embedding.weight]

    def _views(self):
        if self.method == "greedy":
            return self.tokens, self.out_len
        return self.tokens, self.frames, self.out_len, self.score, self.stable_len

    def reset(self, rows=None):
        """Rows become the empty hypothesis; their outputs read zero until their next chunk.  The others
        are not touched.  rows: None for all; a list of row indices (the mask is then built on the host
        and copied over: not for a graph capture); or a device mask, an int32 tensor (B) on the search's
        device with 1 for the rows to reset, which is used as it is -- then, as with None, reset
        enqueues kernels only and can be captured."""
        mask = self._reset_mask(rows)
        self._reset_state(mask)
        for t in self._outputs:
            if mask is None:
                t.zero_()
            else:
                t.masked_fill_(mask.bool().reshape(-1, *[1] * (t.dim() - 1)), 0)

    def _reset_mask(self, rows):
        mask = None
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            if rows.dtype != torch.int32 or tuple(rows.shape) != (self.batch_size,):
                raise ValueError(f"a device mask is int32 of shape ({self.batch_size},), got {rows.dtype} "
                                 f"{tuple(rows.shape)}")
            mask = rows.contiguous()
        elif rows is not None:
            mask = torch.zeros((self.batch_size,), dtype=torch.int32)
            mask[torch.as_tensor(rows, dtype=torch.int64)] = 1
            mask = mask.to(self.state.device)
        return mask

    def step(self, am_chunk, chunk_len=None):
        """am_chunk (B, Tc, V) fp32 on the device, Tc <= 256; chunk_len (B) int64 on the device
        (None: Tc frames for every row; 0 leaves a row as it is).  -> greedy (tokens, out_len),
        beam (tokens, frames, out_len, score, stable_len): views of the fixed output tensors."""
        B, V = self.batch_size, self.V
        if am_chunk.dim() != 3 or am_chunk.shape[0] != B or am_chunk.shape[2] != V \
                or not 1 <= am_chunk.shape[1] <= 256:
            raise ValueError(f"expected {self._input} of shape ({B}, 1..256, {V}), got {tuple(am_chunk.shape)}")
        Tc = am_chunk.shape[1]
        if chunk_len is None:
            chunk_len = self._full.get(Tc)
            if chunk_len is None:
                chunk_len = self._full[Tc] = torch.full((B,), Tc, dtype=torch.int64, device=self.state.device)
        self._chunk(am_chunk, chunk_len, Tc)
        return self._step_views


class RnntStreamingSearch(_ChunkCarriedSearch):
    """Chunk-carried RNN-T search on the device (csrc/decode_rnnt.hip): the fused greedy / beam
    search of the stateless predictor and a projection-free joiner, fed `am = joiner._enc_proj(
    encoder_out)` a chunk at a time.  However the frames are cut, the result after a chunk is the
    whole-utterance search's on the frames fed so far, bit for bit (the kernels share their walk).

    Owns the state buffer (one row per stream, size independent of the stream's length) and fixed
    output tensors; `step` returns views of them, and makes no host synchronisation, so a step can
    be captured into a graph.  There is no module-loop fallback: a predictor / joiner pair or a
    shape the fused search does not take is an error at construction."""

    def __init__(self, predictor, joiner, batch_size=1, method="greedy", max_token_step=5,
                 beam_size=4, cutoff_top_k=4, max_tokens=1024, device=None):
        self._construct_rnnt(predictor, joiner, batch_size, method, max_token_step, beam_size, cutoff_top_k,
                             max_tokens, device)

    def _check_modules(self, predictor, joiner):
        from speech2text_amd.model.joiner.joiner import Joiner
        from speech2text_amd.model.predictor.predictor import StatelessPredictor
        p = getattr(predictor, "predictor", predictor)
        if not isinstance(p, StatelessPredictor):
            raise ValueError("RnntStreamingSearch takes the stateless predictor only, got "
                             f"{type(p).__name__} (the LSTM predictor is carried across chunks by "
                             "RnntLstmStreamingSearch; rnnt_streaming_search picks the class)")
        if not isinstance(joiner, Joiner) or joiner._use_out_project:
            raise ValueError("the chunk-carried search takes a Joiner without output projection")
        return joiner._output_dim, [p._embedding.weight]

    def _allocate(self, predictor, joiner, dev):
        p = getattr(predictor, "predictor", predictor)
        B, V, E, D, ctx = self.batch_size, self.V, p._embedding_dim, p._output_dim, p._context_size
        n = N.lib().s2t_rnnt_stream_state_bytes(B, V, ctx, self.beam_size, self.max_tokens) if B > 0 else 0
        if self.method == "beam":
            ok = 1 <= self.beam_size <= 16 and 1 <= min(self.cutoff_top_k, V) <= 16 \
                and 16 * (E + D) + 128 * ctx <= 60 * 1024
        else:
            ok = self.max_token_step >= 0 and 4 * (E + D + V + ctx) <= 60 * 1024
        if n <= 0 or not ok or p._embedding.num_embeddings < V:
            raise ValueError(f"the chunk-carried {self.method} search does not take this shape: B {B} V {V} "
                             f"E {E} D {D} ctx {ctx} beam {self.beam_size} top-k {self.cutoff_top_k} "
                             f"max_tokens {self.max_tokens} (limits: include/s2t_mi355.h)")
        self._w, self.E, self.D, self.ctx, self._act = _stateless_weights(predictor, joiner, dev)
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)

    def _reset_state(self, mask):
        N.check(N.lib().s2t_rnnt_stream_reset(N.ptr(self.state), N.ip(mask), self.batch_size, self.V, self.ctx,
                                              self.beam_size, self.max_tokens, 0, N.stream()),
                "s2t_rnnt_stream_reset")

    def _chunk(self, am_chunk, chunk_len, Tc):
        B, V = self.batch_size, self.V
        w = [N.fp(t) for t in self._w]
        if self.method == "greedy":
            N.check(N.lib().s2t_rnnt_greedy_stateless_chunk(
                N.fp(am_chunk), N.lp(chunk_len), *w, B, Tc, V, self.E, self.D, self.ctx, self._act,
                self.max_token_step, self.max_tokens, 0, N.ptr(self.state), N.lp(self.tokens),
                N.lp(self.out_len), N.ip(self.overflow), N.stream()), "s2t_rnnt_greedy_stateless_chunk")
            return
        N.check(N.lib().s2t_rnnt_beam_stateless_chunk(
            N.fp(am_chunk), N.lp(chunk_len), *w, B, Tc, V, self.E, self.D, self.ctx, self._act, 0,
            self.beam_size, self.cutoff_top_k, self.max_tokens, N.ptr(self.state), N.lp(self.tokens),
            N.lp(self.frames), N.lp(self.out_len), N.fp(self.score), N.lp(self.stable_len),
            N.ip(self.overflow), N.stream()), "s2t_rnnt_beam_stateless_chunk")


class RnntLstmStreamingSearch(_ChunkCarriedSearch):
    """RnntStreamingSearch for the LSTM predictor and a Joiner with or without output projection
    (csrc/decode_lstm.hip, s2t_rnnt_*_lstm_chunk): the lockstep device searches fed `am` a chunk at
    a time.  A round's launches are the whole-utterance calls' own, so however the frames are cut
    the result after a chunk is rnnt_greedy_lstm_tokens_from_am / rnnt_beam_lstm_tokens_from_am on
    the frames fed so far, bit for bit.

    Same surface: `state`, `tokens`, `frames`, `out_len`, `score`, `stable_len`, `overflow`,
    `reset(rows)` (zero LSTM state, one predictor step on blank), `step(am_chunk, chunk_len)`
    returning views without a host synchronisation.
    `capturable=True` (the default) enqueues every greedy round, so a step can be captured into a
    graph; `capturable=False` lets the greedy step read the device's live counter every 32 rounds
    and stop early (the same bits; a beam step never synchronises either way).  Greedy past
    `max_tokens` drops symbols and sets `overflow` but goes on walking, as the whole-utterance LSTM
    search does.  There is no module-loop fallback: other modules or a shape the kernels refuse are
    an error at construction.

    `lm` (an RnnLm) with `method="beam"`: RNN-LM shallow fusion carried across chunks
    (s2t_rnnt_beam_lstm_lm_chunk): the state buffer also holds the LM's (h, c), q and lm_sum per beam,
    the result after a chunk is rnnt_beam_lstm_lm_tokens_from_am on the frames fed so far, bit for
    bit, and `lm_score` (B, fp32) beside `score` is the best beam's unweighted LM sum (`step` returns
    the same five views; `reset(rows)` zeroes it for those rows and resets their LM state, stepping
    the LM on `lm_start_token` when one is given).  `lm` None: the object and its calls are exactly
    those without the argument.  `method="greedy"` with an `lm`, an `lm` that is not an RnnLm, or an
    LM shape outside the limits is a ValueError: the greedy searches take no LM and there is no
    module-loop fallback here."""

    def __init__(self, predictor, joiner, batch_size=1, method="greedy", max_token_step=5,
                 beam_size=4, cutoff_top_k=4, max_tokens=1024, device=None, capturable=True, lm=None,
                 lm_weight=0.0, lm_start_token=None):
        self.capturable = bool(capturable)
        self._construct_rnnt(predictor, joiner, batch_size, method, max_token_step, beam_size, cutoff_top_k,
                             max_tokens, device, lm, lm_weight, lm_start_token)

    def _check_modules(self, predictor, joiner):
        if not _is_lstm_pair(predictor, joiner):
            raise ValueError("RnntLstmStreamingSearch takes LstmPredictor + Joiner, got "
                             f"{type(getattr(predictor, 'predictor', predictor)).__name__} + "
                             f"{type(joiner).__name__} (the stateless predictor: RnntStreamingSearch)")
        return joiner._output_dim, [joiner._pre_proj.weight, next(predictor.parameters())] + self._lm_on_gpu()

    def _allocate(self, predictor, joiner, dev):
        B, V = self.batch_size, self.V
        self._desc, self._keep = rnnt_lstm_desc(predictor, joiner)
        lib = N.lib()
        n = ws = 0
        self._lm_desc = None
        if self._lm is not None:
            self._lm_desc, self._lm_keep = rnn_lm_desc(self._lm)
            if self._desc is not None and self._lm_desc is not None and B > 0 and self._lm_start < V:
                n = lib.s2t_rnnt_lstm_lm_stream_state_bytes(self._desc, self._lm_desc, B, self.beam_size,
                                                            self.max_tokens)
                ws = lib.s2t_rnnt_lstm_lm_stream_workspace_bytes(self._desc, self._lm_desc, B, 256, self.beam_size)
        elif self._desc is not None and B > 0:
            n = lib.s2t_rnnt_lstm_stream_state_bytes(self._desc, B, self.beam_size, self.max_tokens)
            ws = lib.s2t_rnnt_lstm_stream_workspace_bytes(self._desc, B, 256, self.beam_size)
        if self.method == "beam":
            ok = _beam_in_range(self.beam_size) and _beam_in_range(min(self.cutoff_top_k, V))
        else:
            ok = self.max_token_step >= 0
        if n <= 0 or ws <= 0 or not ok:
            raise ValueError(f"the chunk-carried LSTM {self.method} search does not take this shape: B {B} V {V} "
                             f"beam {self.beam_size} top-k {self.cutoff_top_k} max_token_step "
                             f"{self.max_token_step} max_tokens {self.max_tokens}"
                             + ("" if self._lm is None else f", with an LM of V {self._lm._num_symbols} "
                                f"start token {self._lm_start}") + " (limits: include/s2t_mi355.h)")
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self._ws = torch.zeros((ws,), dtype=torch.uint8, device=dev)

    def _reset_state(self, mask):
        if self._lm is not None:
            N.check(N.lib().s2t_rnnt_lstm_lm_stream_reset(
                self._desc, self._lm_desc, self._lm_start, N.ptr(self.state), N.ip(mask), self.batch_size,
                self.beam_size, self.max_tokens, N.ptr(self._ws), N.stream()), "s2t_rnnt_lstm_lm_stream_reset")
            return
        N.check(N.lib().s2t_rnnt_lstm_stream_reset(self._desc, N.ptr(self.state), N.ip(mask), self.batch_size,
                                                   self.beam_size, self.max_tokens, N.ptr(self._ws), N.stream()),
                "s2t_rnnt_lstm_stream_reset")

    def _chunk(self, am_chunk, chunk_len, Tc):
        B = self.batch_size
        if self.method == "greedy":
            N.check(N.lib().s2t_rnnt_greedy_lstm_chunk(
                self._desc, N.fp(am_chunk), N.lp(chunk_len), B, Tc, self.max_token_step, self.max_tokens,
                0 if self.capturable else 1, N.ptr(self.state), N.ptr(self._ws), N.lp(self.tokens),
                N.lp(self.out_len), N.ip(self.overflow), N.stream()), "s2t_rnnt_greedy_lstm_chunk")
            return
        if self._lm is not None:
            N.check(N.lib().s2t_rnnt_beam_lstm_lm_chunk(
                self._desc, self._lm_desc, N.fp(am_chunk), N.lp(chunk_len), B, Tc, self.beam_size,
                self.cutoff_top_k, self._lm_weight, self.max_tokens, N.ptr(self.state), N.ptr(self._ws),
                N.lp(self.tokens), N.lp(self.frames), N.lp(self.out_len), N.fp(self.score), N.fp(self.lm_score),
                N.lp(self.stable_len), N.ip(self.overflow), N.stream()), "s2t_rnnt_beam_lstm_lm_chunk")
            return
        N.check(N.lib().s2t_rnnt_beam_lstm_chunk(
            self._desc, N.fp(am_chunk), N.lp(chunk_len), B, Tc, self.beam_size, self.cutoff_top_k,
            self.max_tokens, N.ptr(self.state), N.ptr(self._ws), N.lp(self.tokens), N.lp(self.frames),
            N.lp(self.out_len), N.fp(self.score), N.lp(self.stable_len), N.ip(self.overflow), N.stream()),
            "s2t_rnnt_beam_lstm_chunk")


class RnntLstmNgramStreamingSearch(RnntLstmStreamingSearch):
    """RnntLstmStreamingSearch's beam search fused with a back-off n-gram (csrc/decode_lstm.hip
    s2t_rnnt_beam_lstm_ngram_chunk): the lockstep rounds in their n-gram mode, carried across chunks; the
    state buffer also holds a context id and lm_sum per beam, and no LM step is launched.  However the
    frames are cut, the result after a chunk is rnnt_beam_lstm_ngram_tokens_from_am on the frames fed so
    far, bit for bit, `lm_score` included.

    Same surface as RnntLstmStreamingSearch with method="beam" and an LM: `step` returns the five beam
    views, `lm_score` (B, fp32) is the best beam's unweighted LM sum, `reset(rows)` restarts those rows in
    the LM's start context.  Beam only, no `lm_start_token`.  The tables are copied to the search's device
    when they live elsewhere.  Other modules, an `lm` that is not an NgramLm with fp32 tables, a weight
    that is not finite or a shape the entries refuse are a ValueError at construction; modules off the GPU
    a RuntimeError.  No module-loop fallback."""

    def __init__(self, predictor, joiner, batch_size=1, beam_size=4, cutoff_top_k=4, max_tokens=1024, device=None,
                 lm=None, lm_weight=0.0):
        super().__init__(predictor, joiner, batch_size, "beam", 0, beam_size, cutoff_top_k, max_tokens, device,
                         True, lm, lm_weight)

    def _lm_arguments(self, lm, lm_weight, lm_start_token, method):
        return _ngram_arguments(lm, lm_weight, "RnntLstmNgramStreamingSearch")

    def _allocate(self, predictor, joiner, dev):
        B, V = self.batch_size, self.V
        self._desc, self._keep = rnnt_lstm_desc(predictor, joiner)
        self._lm = _ngram_on(self._lm, dev)
        lib = N.lib()
        n = ws = 0
        if self._desc is not None and B > 0 and self._lm.num_classes == V:
            self._lm_desc, self._lm_keep = self._lm.desc()
            n = lib.s2t_rnnt_lstm_ngram_stream_state_bytes(self._desc, self._lm_desc, B, self.beam_size,
                                                           self.max_tokens)
            ws = lib.s2t_rnnt_lstm_ngram_stream_workspace_bytes(self._desc, self._lm_desc, B, 256, self.beam_size)
        if n <= 0 or ws <= 0 or not _beam_in_range(min(self.cutoff_top_k, V)):
            raise ValueError(f"the chunk-carried LSTM n-gram beam search does not take this shape: B {B} V {V} beam "
                             f"{self.beam_size} top-k {self.cutoff_top_k} max_tokens {self.max_tokens}, LM V "
                             f"{self._lm.num_classes} (limits: include/s2t_mi355.h)")
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)   # the plain state, then ctx and lm_sum per beam
        self._ws = torch.zeros((ws,), dtype=torch.uint8, device=dev)

    def _reset_state(self, mask):
        N.check(N.lib().s2t_rnnt_lstm_ngram_stream_reset(
            self._desc, self._lm_desc, int(self._lm.start_ctx), N.ptr(self.state), N.ip(mask), self.batch_size,
            self.beam_size, self.max_tokens, N.ptr(self._ws), N.stream()), "s2t_rnnt_lstm_ngram_stream_reset")

    def _chunk(self, am_chunk, chunk_len, Tc):
        N.check(N.lib().s2t_rnnt_beam_lstm_ngram_chunk(
            self._desc, self._lm_desc, N.fp(am_chunk), N.lp(chunk_len), self.batch_size, Tc, self.beam_size,
            self.cutoff_top_k, self._lm_weight, self.max_tokens, N.ptr(self.state), N.ptr(self._ws),
            N.lp(self.tokens), N.lp(self.frames), N.lp(self.out_len), N.fp(self.score), N.fp(self.lm_score),
            N.lp(self.stable_len), N.ip(self.overflow), N.stream()), "s2t_rnnt_beam_lstm_ngram_chunk")


class RnntStatelessLmStreamingSearch(_ChunkCarriedSearch):
    """The chunk-carried beam search of StatelessPredictor + Joiner (with or without output projection)
    + RnnLm on the lockstep rounds of csrc/decode_lstm.hip (s2t_rnnt_beam_stateless_lm_chunk): however
    the frames are cut, the result after a chunk is rnnt_beam_stateless_lm_tokens_from_am on the frames
    fed so far, bit for bit.  This is the ONLY chunk-carried search of the stateless predictor with an
    out-projection joiner, and it needs an LM: the lockstep rounds over this predictor exist as the
    fused search alone (without an LM and without out-projection: RnntStreamingSearch, on the
    one-workgroup kernels).

    Same surface as RnntLstmStreamingSearch with an `lm`: `state`, `tokens`, `frames`, `out_len`,
    `score`, `lm_score`, `stable_len`, `overflow`, `reset(rows)`, `step(am_chunk, chunk_len)` returning
    the five beam views without a host synchronisation, so a step can be captured into a graph.  Beam
    only.  Other modules, `method="greedy"`, a missing or foreign `lm`, or a shape the kernels refuse
    are a ValueError at construction; modules off the GPU a RuntimeError.  No module-loop fallback."""

    def __init__(self, predictor, joiner, batch_size=1, method="beam", max_token_step=5, beam_size=4,
                 cutoff_top_k=4, max_tokens=1024, device=None, lm=None, lm_weight=0.0, lm_start_token=None):
        if lm is None:
            raise ValueError("RnntStatelessLmStreamingSearch needs an lm (without one: RnntStreamingSearch)")
        self._construct_rnnt(predictor, joiner, batch_size, method, max_token_step, beam_size, cutoff_top_k,
                             max_tokens, device, lm, lm_weight, lm_start_token)

    def _check_modules(self, predictor, joiner):
        if not _is_stateless_pair(predictor, joiner):
            raise ValueError("RnntStatelessLmStreamingSearch takes StatelessPredictor + Joiner, got "
                             f"{type(getattr(predictor, 'predictor', predictor)).__name__} + "
                             f"{type(joiner).__name__} (the LSTM predictor: RnntLstmStreamingSearch)")
        return joiner._output_dim, [joiner._pre_proj.weight,
                                    getattr(predictor, "predictor", predictor)._embedding.weight] + self._lm_on_gpu()

    def _allocate(self, predictor, joiner, dev):
        B, V = self.batch_size, self.V
        self._desc, self._keep = rnnt_stateless_desc(predictor, joiner)
        self._lm_desc, self._lm_keep = rnn_lm_desc(self._lm)
        lib = N.lib()
        n = ws = 0
        if self._desc is not None and self._lm_desc is not None and B > 0 and self._lm_start < V:
            n = lib.s2t_rnnt_stateless_lm_stream_state_bytes(self._desc, self._lm_desc, B, self.beam_size,
                                                             self.max_tokens)
            ws = lib.s2t_rnnt_stateless_lm_stream_workspace_bytes(self._desc, self._lm_desc, B, 256, self.beam_size)
        if n <= 0 or ws <= 0 or not _beam_in_range(min(self.cutoff_top_k, V)):
            raise ValueError(f"the chunk-carried stateless beam search with an LM does not take this shape: B {B} "
                             f"V {V} beam {self.beam_size} top-k {self.cutoff_top_k} max_tokens {self.max_tokens}, "
                             f"LM V {self._lm._num_symbols} start token {self._lm_start} "
                             "(limits: include/s2t_mi355.h)")
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self._ws = torch.zeros((ws,), dtype=torch.uint8, device=dev)

    def _reset_state(self, mask):
        N.check(N.lib().s2t_rnnt_stateless_lm_stream_reset(
            self._desc, self._lm_desc, self._lm_start, N.ptr(self.state), N.ip(mask), self.batch_size,
            self.beam_size, self.max_tokens, N.ptr(self._ws), N.stream()), "s2t_rnnt_stateless_lm_stream_reset")

    def _chunk(self, am_chunk, chunk_len, Tc):
        N.check(N.lib().s2t_rnnt_beam_stateless_lm_chunk(
            self._desc, self._lm_desc, N.fp(am_chunk), N.lp(chunk_len), self.batch_size, Tc, self.beam_size,
            self.cutoff_top_k, self._lm_weight, self.max_tokens, N.ptr(self.state), N.ptr(self._ws),
            N.lp(self.tokens), N.lp(self.frames), N.lp(self.out_len), N.fp(self.score), N.fp(self.lm_score),
            N.lp(self.stable_len), N.ip(self.overflow), N.stream()), "s2t_rnnt_beam_stateless_lm_chunk")


class RnntNgramStreamingSearch(RnntStreamingSearch):
    """RnntStreamingSearch's beam search fused with a back-off n-gram (csrc/decode_rnnt.hip
    s2t_rnnt_beam_stateless_ngram_chunk): the one-workgroup search of the stateless predictor and a
    projection-free Joiner, a look-up per candidate inside the frame body, carried across chunks.
    However the frames are cut, the result after a chunk is rnnt_beam_ngram_tokens_from_am on the frames
    fed so far, bit for bit, `lm_score` included.

    Same surface as RnntStreamingSearch with method="beam": `state`, `tokens`, `frames`, `out_len`,
    `score`, `stable_len`, `overflow`, `reset(rows)` (a reset row restarts in the LM's start context),
    `step(am_chunk, chunk_len)` returning the five beam views without a host synchronisation, plus
    `lm_score` (B, fp32), the best beam's unweighted LM sum.  Beam only.  The tables are copied to the
    search's device when they live elsewhere.  Other modules, an `lm` that is not an NgramLm with fp32
    tables, a weight that is not finite or a shape the entry refuses are a ValueError at construction;
    modules off the GPU a RuntimeError.  No module-loop fallback."""

    def __init__(self, predictor, joiner, batch_size=1, beam_size=4, cutoff_top_k=4, max_tokens=1024, device=None,
                 lm=None, lm_weight=0.0):
        self._construct_rnnt(predictor, joiner, batch_size, "beam", 0, beam_size, cutoff_top_k, max_tokens, device,
                             lm, lm_weight)

    def _lm_arguments(self, lm, lm_weight, lm_start_token, method):
        return _ngram_arguments(lm, lm_weight, "RnntNgramStreamingSearch")

    def _allocate(self, predictor, joiner, dev):
        super()._allocate(predictor, joiner, dev)          # the plain search's checks and weights
        n = N.lib().s2t_rnnt_ngram_stream_state_bytes(self.batch_size, self.V, self.ctx, self.beam_size,
                                                      self.max_tokens)
        if n <= 0 or self._lm.num_classes != self.V:
            raise ValueError(f"the chunk-carried n-gram beam search does not take this shape: B {self.batch_size} "
                             f"V {self.V} beam {self.beam_size} max_tokens {self.max_tokens}, LM V "
                             f"{self._lm.num_classes} (limits: include/s2t_mi355.h)")
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)   # the plain row + ctx and lm_sum per beam
        self._lm = _ngram_on(self._lm, dev)
        self._lm_desc, self._lm_keep = self._lm.desc()

    def _reset_state(self, mask):
        N.check(N.lib().s2t_rnnt_ngram_stream_reset(N.ptr(self.state), N.ip(mask), self.batch_size, self.V, self.ctx,
                                                    self.beam_size, self.max_tokens, 0, int(self._lm.start_ctx),
                                                    N.stream()), "s2t_rnnt_ngram_stream_reset")

    def _chunk(self, am_chunk, chunk_len, Tc):
        N.check(N.lib().s2t_rnnt_beam_stateless_ngram_chunk(
            self._lm_desc, N.fp(am_chunk), N.lp(chunk_len), *[N.fp(t) for t in self._w], self.batch_size, Tc,
            self.V, self.E, self.D, self.ctx, self._act, 0, self.beam_size, self.cutoff_top_k, self._lm_weight,
            self.max_tokens, N.ptr(self.state), N.lp(self.tokens), N.lp(self.frames), N.lp(self.out_len),
            N.fp(self.score), N.fp(self.lm_score), N.lp(self.stable_len), N.ip(self.overflow), N.stream()),
            "s2t_rnnt_beam_stateless_ngram_chunk")


def rnnt_streaming_search(predictor, joiner, batch_size=1, method="greedy", max_token_step=5, beam_size=4,
                          cutoff_top_k=4, max_tokens=1024, device=None, lm=None, lm_weight=0.0,
                          lm_start_token=None, **kw):
    """The chunk-carried search that serves the pair: RnntLstmStreamingSearch for LstmPredictor +
    Joiner (kw: capturable), with or without an `lm`; for the stateless predictor
    RnntStatelessLmStreamingSearch with an RnnLm (joiner with or without output projection),
    RnntNgramStreamingSearch with an NgramLm (beam search, projection-free joiner, no `lm_start_token`)
    and RnntStreamingSearch without an `lm` (which raises for what it does not take).  An NgramLm with
    the LSTM pair raises here (existing callers are pinned to that): build RnntLstmNgramStreamingSearch
    directly, as StreamingRecognizer and the tasks do; with method="greedy" it raises: the greedy searches
    take no LM."""
    if _is_ngram(lm) and method == "beam" and not _is_lstm_pair(predictor, joiner):
        if lm_start_token is not None:
            raise ValueError("an NgramLm starts in its own <s> context: lm_start_token must be None")
        return RnntNgramStreamingSearch(predictor, joiner, batch_size, beam_size, cutoff_top_k, max_tokens, device,
                                        lm=lm, lm_weight=lm_weight, **kw)
    if _is_lstm_pair(predictor, joiner):
        if lm is not None:
            kw.update(lm=lm, lm_weight=lm_weight, lm_start_token=lm_start_token)
        return RnntLstmStreamingSearch(predictor, joiner, batch_size, method, max_token_step, beam_size,
                                       cutoff_top_k, max_tokens, device, **kw)
    if lm is not None:
        return RnntStatelessLmStreamingSearch(predictor, joiner, batch_size, method, max_token_step, beam_size,
                                              cutoff_top_k, max_tokens, device, lm=lm, lm_weight=lm_weight,
                                              lm_start_token=lm_start_token, **kw)
    return RnntStreamingSearch(predictor, joiner, batch_size, method, max_token_step, beam_size,
                               cutoff_top_k, max_tokens, device, **kw)


class CtcStreamingSearch(_ChunkCarriedSearch):
    """Chunk-carried CTC prefix beam search on the device (csrc/decode_ctc.hip s2t_ctc_prefix_beam_chunk,
    with an `lm` s2t_ctc_prefix_beam_lm_chunk): ctc_prefix_beam_tokens / ctc_prefix_beam_lm_tokens fed the
    frames' scores (B, Tc, V) a chunk at a time.  The frame body is the whole-utterance entries' own, so
    however the frames are cut the result after a chunk is theirs on the frames fed so far, bit for bit,
    while `overflow` is 0.  The trie is compacted at the end of every chunk to the paths between the live
    prefixes' common ancestor and the live prefixes, so the state's size (`max_nodes` nodes a stream)
    and a chunk's cost do not grow with the stream; a row needs `kept + beam_size * n <= max_nodes` to
    consume n frames, else `overflow` gets bit 1 (value 2) and the row is inert until `reset`.  A best
    prefix past `max_tokens` keeps its first `max_tokens` tokens, bit 0 (value 1).

    Owns the state buffer and the fixed output tensors `tokens` (B, max_tokens), `out_len`, `score`,
    `stable_len` (`tokens[b, :stable_len[b]]` can no longer change), `overflow` and, with an `lm`,
    `lm_score` (else None).  `step` makes no host synchronisation, so it can be captured into a graph.
    `method="greedy"` is beam_size = cutoff_top_k = 1 through the same kernel (ctc_greedy_tokens' tokens)
    and takes no LM.  A shape the entries refuse, an `lm` that is not an RnnLm, or greedy with an `lm` is
    a ValueError at construction: there is no host-loop fallback."""

    _input, _has_frames = "logits", False

    def __init__(self, num_classes, batch_size=1, method="beam", beam_size=4, cutoff_top_k=4, max_tokens=1024,
                 max_nodes=4096, blank=0, device=None, lm=None, lm_weight=0.0, lm_start_token=None):
        beam = _method_arg(method) == "beam"               # (here a method's error comes before an LM's)
        self.max_nodes, self.blank = int(max_nodes), int(blank)
        self._construct((num_classes,), batch_size, method, beam_size if beam else 1, cutoff_top_k if beam else 1,
                        max_tokens, device, lm, lm_weight, lm_start_token)

    def _check_modules(self, num_classes):
        return int(num_classes), self._lm_on_gpu()

    def _views(self):
        return self.tokens, self.out_len, self.score, self.stable_len

    def _refuse(self, what, lm_note):
        """-> the ValueError for a shape the entries refuse; the entries say 0 bytes for what the kernels
        do not take, `_shape_ok` is what they are not asked."""
        return ValueError(f"the chunk-carried CTC {what} search does not take this shape: B {self.batch_size} V "
                          f"{self.V} blank {self.blank} beam {self.beam_size} top-k {self.cutoff_top_k} max_tokens "
                          f"{self.max_tokens} max_nodes {self.max_nodes}{lm_note} (limits: include/s2t_mi355.h)")

    def _shape_ok(self):
        return self.batch_size > 0 and 0 <= self.blank < self.V and self.max_tokens >= 1 \
            and self.cutoff_top_k >= 1 and _beam_in_range(min(self.cutoff_top_k, self.V))

    def _allocate(self, num_classes, dev):
        B, V, lib = self.batch_size, self.V, N.lib()
        n, ws = 0, 1
        self._lm_desc = None
        if self._shape_ok() and self._lm is not None:
            self._lm_desc, self._lm_keep = rnn_lm_desc(self._lm)
            if self._lm_desc is not None and self._lm_start < V:
                n = lib.s2t_ctc_lm_stream_state_bytes(self._lm_desc, B, V, self.beam_size, self.max_nodes)
                ws = lib.s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(self._lm_desc, B, V, self.beam_size)
        elif self._shape_ok():
            n = lib.s2t_ctc_stream_state_bytes(B, V, self.beam_size, self.max_nodes)
        if n <= 0 or ws <= 0:
            raise self._refuse(self.method, "" if self._lm is None else
                               f", with an LM of V {self._lm._num_symbols} start token {self._lm_start}")
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self._ws = None if self._lm is None else torch.zeros((ws,), dtype=torch.uint8, device=dev)

    def _reset_state(self, mask):
        B, V = self.batch_size, self.V
        if self._lm is not None:
            N.check(N.lib().s2t_ctc_lm_stream_reset(self._lm_desc, self._lm_start, N.ptr(self.state), N.ip(mask), B, V,
                                                    self.beam_size, self.max_nodes, N.ptr(self._ws), N.stream()),
                    "s2t_ctc_lm_stream_reset")
        else:
            N.check(N.lib().s2t_ctc_stream_reset(N.ptr(self.state), N.ip(mask), B, V, self.beam_size, self.max_nodes,
                                                 N.stream()), "s2t_ctc_stream_reset")

    def step(self, logits_chunk, chunk_len=None):
        """logits_chunk (B, Tc, V) fp32 on the device, raw or normalised, Tc <= 256; chunk_len (B) int64
        on the device (None: Tc frames for every row; 0 leaves a row as it is).  -> (tokens, out_len,
        score, stable_len): views of the fixed output tensors."""
        return super().step(logits_chunk, chunk_len)

    def _chunk(self, logits_chunk, chunk_len, Tc):
        B, V = self.batch_size, self.V
        if self._lm is not None:
            N.check(N.lib().s2t_ctc_prefix_beam_lm_chunk(
                self._lm_desc, N.fp(logits_chunk), N.lp(chunk_len), B, Tc, V, self.blank, self.beam_size,
                self.cutoff_top_k, self._lm_weight, self._lm_start, self.max_tokens, self.max_nodes,
                N.ptr(self.state), N.ptr(self._ws), N.lp(self.tokens), N.lp(self.out_len), N.fp(self.score),
                N.fp(self.lm_score), N.lp(self.stable_len), N.ip(self.overflow), N.stream()),
                "s2t_ctc_prefix_beam_lm_chunk")
        else:
            N.check(N.lib().s2t_ctc_prefix_beam_chunk(
                N.fp(logits_chunk), N.lp(chunk_len), B, Tc, V, self.blank, self.beam_size, self.cutoff_top_k,
                self.max_tokens, self.max_nodes, N.ptr(self.state), N.lp(self.tokens), N.lp(self.out_len),
                N.fp(self.score), N.lp(self.stable_len), N.ip(self.overflow), N.stream()),
                "s2t_ctc_prefix_beam_chunk")


class CtcNgramStreamingSearch(CtcStreamingSearch):
    """CtcStreamingSearch's beam search fused with a back-off n-gram (csrc/decode_ctc.hip
    s2t_ctc_prefix_beam_ngram_chunk): ctc_prefix_beam_ngram_tokens fed the frames' scores a chunk at a
    time, still ONE launch per chunk, the look-up inside the frame body.  However the frames are cut,
    the result after a chunk is ctc_prefix_beam_ngram_tokens' on the frames fed so far, bit for bit,
    `lm_score` included, while `overflow` is 0.

    Same attributes, `reset(rows)` (a reset row restarts in the LM's start context) and
    `step(logits_chunk, chunk_len)` as CtcStreamingSearch with an LM.  Beam only; an NgramLm starts in its
    own <s> context, so there is no `lm_start_token`.  The tables are copied to the search's device when
    they live elsewhere.  An `lm` that is not an NgramLm with fp32 tables, a weight that is not finite or
    a shape the entry refuses are a ValueError at construction.  No host-loop fallback."""

    def __init__(self, num_classes, batch_size=1, beam_size=4, cutoff_top_k=4, max_tokens=1024, max_nodes=4096,
                 blank=0, device=None, lm=None, lm_weight=0.0):
        super().__init__(num_classes, batch_size, "beam", beam_size, cutoff_top_k, max_tokens, max_nodes, blank,
                         device, lm, lm_weight)

    def _lm_arguments(self, lm, lm_weight, lm_start_token, method):
        return _ngram_arguments(lm, lm_weight, "CtcNgramStreamingSearch")

    def _allocate(self, num_classes, dev):
        B, V = self.batch_size, self.V
        ok = self._shape_ok() and self._lm.num_classes == V
        n = N.lib().s2t_ctc_ngram_stream_state_bytes(B, V, self.beam_size, self.max_nodes) if ok else 0
        if n <= 0:
            raise self._refuse("n-gram beam", f", LM V {self._lm.num_classes}")
        self.state = torch.zeros((n,), dtype=torch.uint8, device=dev)   # the plain state, then ctx per prefix
        self._lm = _ngram_on(self._lm, dev)
        self._lm_desc, self._lm_keep = self._lm.desc()

    def _reset_state(self, mask):
        N.check(N.lib().s2t_ctc_ngram_stream_reset(N.ptr(self.state), N.ip(mask), self.batch_size, self.V,
                                                   self.beam_size, self.max_nodes, int(self._lm.start_ctx),
                                                   N.stream()), "s2t_ctc_ngram_stream_reset")

    def _chunk(self, logits_chunk, chunk_len, Tc):
        N.check(N.lib().s2t_ctc_prefix_beam_ngram_chunk(
            self._lm_desc, N.fp(logits_chunk), N.lp(chunk_len), self.batch_size, Tc, self.V, self.blank,
            self.beam_size, self.cutoff_top_k, self._lm_weight, self.max_tokens, self.max_nodes, N.ptr(self.state),
            N.lp(self.tokens), N.lp(self.out_len), N.fp(self.score), N.fp(self.lm_score), N.lp(self.stable_len),
            N.ip(self.overflow), N.stream()), "s2t_ctc_prefix_beam_ngram_chunk")


def ctc_streaming_search(num_classes, batch_size=1, method="beam", beam_size=4, cutoff_top_k=4, max_tokens=1024,
                         max_nodes=4096, blank=0, device=None, lm=None, lm_weight=0.0, lm_start_token=None):
    """The chunk-carried CTC search that serves the LM: CtcNgramStreamingSearch for an NgramLm with the
    beam method (no `lm_start_token`), CtcStreamingSearch for everything else (which raises for what it
    does not take)."""
    if _is_ngram(lm) and method == "beam":
        if lm_start_token is not None:
            raise ValueError("an NgramLm starts in its own <s> context: lm_start_token must be None")
        return CtcNgramStreamingSearch(num_classes, batch_size, beam_size, cutoff_top_k, max_tokens, max_nodes,
                                       blank, device, lm=lm, lm_weight=lm_weight)
    return CtcStreamingSearch(num_classes, batch_size, method, beam_size, cutoff_top_k, max_tokens, max_nodes,
                              blank, device, lm=lm, lm_weight=lm_weight, lm_start_token=lm_start_token)


@unique
class DecodingFactory(Enum):
    """Decoding methods by the reference's names (:428-435), so that an inference YAML's
    `decoding.type` / `decoding.config` resolves as there: DecodingFactory[type].value(**config)."""
    ctc_greedy_decoding = CtcGreedyDecoding
    rnnt_greedy_decoding = RnntGreedyDecoding
    rnnt_beam_decoding = RnntBeamDecoding
