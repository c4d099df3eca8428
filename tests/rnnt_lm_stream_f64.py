"""Plain-torch restatement of the chunk-carried RNN-T beam search with RNN-LM shallow fusion: the
yardstick of `stable_len` and of the tokens in tests/test_gpu_rnnt_lm_stream.py (csrc/decode_lstm.hip
s2t_rnnt_beam_lstm_lm_chunk, s2t_rnnt_beam_stateless_lm_chunk).

Test infrastructure (not a test file).  `search_chunk` is rnnt_lm_fusion_f64.search statement for
statement, with what that keeps in local variables between two frames (the beams: tokens, frames,
score, predictor state, lm vector, LM state, q, lm_sum) carried between two calls instead;
tests/test_rnnt_lm_stream_f64.py holds `chunked` to the whole-utterance function for every case and
cut.  Both predictors go through that function's own hooks (`start`, `step`, `log_probs`), built here
as rnnt_lm_fusion_f64.beam_search_lm and rnnt_stateless_lm_f64.beam_search_lm build them.  It works in
the dtype of the weights, as those modules do.
"""
import torch

import rnn_lm_f64 as R
import rnnt_lm_fusion_f64 as F
import rnnt_lstm_search_f64 as S
import rnnt_stateless_lm_f64 as SF
from rnnt_lstm_stream_f64 import common_prefix_len, cuts_of  # noqa: F401


def lstm_hooks(w, act):
    """(start, step, log_probs, dtype) of the LSTM predictor: rnnt_lm_fusion_f64.beam_search_lm's."""
    return (lambda: S.pred_step(w, torch.zeros(1, dtype=torch.int64), S.zero_state(w, 1)),
            lambda c, st: S.pred_step(w, torch.tensor([c]), st),
            lambda am_t, lm: torch.log_softmax(S.joint(w, am_t, lm, act)[0], dim=-1),
            w["emb"].dtype)


def stateless_hooks(p, ctx, act):
    """(start, step, log_probs, dtype) of the stateless predictor: rnnt_stateless_lm_f64.beam_search_lm's."""
    vec = lambda st: SF.lm_vectors(p, torch.tensor([st], dtype=torch.int64))       # noqa: E731
    return (lambda: (vec((0,) * ctx), (0,) * ctx),
            lambda c, st: (vec(st[1:] + (c,)), st[1:] + (c,)),
            lambda am_t, lm: SF.log_probs(p, am_t, lm, act),
            p["emb"].dtype)


def beam_start(hooks, sd, lm_start_token=None):
    """The beams of an empty stream: one beam of score 0 (tokens, frames, score, state, lm, LM state, q,
    lm_sum), as rnnt_lm_fusion_f64.search starts."""
    start, _, _, dtype = hooks
    lm, state = start()
    q, ls = F.lm_start(sd, lm_start_token)
    zero = torch.zeros((), dtype=dtype)
    return [((), (), zero, state, lm, ls, q, zero)]


@torch.no_grad()
def search_chunk(beams, t0, am, hooks, beam_size, cutoff_top_k, sd, lm_weight):
    """The frames am (Tc,V) of a stream that has seen t0 frames -> (beams, margin of this chunk)."""
    _, step, log_probs, dtype = hooks
    am = am.to(dtype)
    T, V = am.shape
    k = min(int(cutoff_top_k), V)
    margin = float("inf")
    for t in range(T):
        lps = log_probs(am[t], torch.cat([b[4] for b in beams], 0))
        cands = []
        for (tokens, frames, score, st, lmv, ls, q, lm_sum), lp in zip(beams, lps):
            vals, order = torch.sort(lp, descending=True, stable=True)   # value desc, class asc
            if k < V:
                margin = min(margin, float(vals[k - 1] - vals[k]))
            for v, c in zip(vals[:k], order[:k].tolist()):
                if c == 0:
                    cands.append((tokens, frames, score + v, st, lmv, ls, q, lm_sum, 0))
                else:
                    cands.append((tokens + (c,), frames + (t0 + t,), (score + v) + lm_weight * q[c], st, lmv, ls, q,
                                  lm_sum + q[c], c))
        cands.sort(key=lambda x: float(x[2]), reverse=True)  # stable: parent position, then rank
        if len(cands) > beam_size:
            margin = min(margin, float(cands[beam_size - 1][2] - cands[beam_size][2]))
        beams = []
        for tokens, frames, score, st, lmv, ls, q, lm_sum, c in cands[:beam_size]:
            if c != 0:
                lmv, st = step(c, st)
                qq, ls = R.score_step_ref(sd, torch.tensor([c]), ls)
                q = qq[0]
            beams.append((tokens, frames, score, st, lmv, ls, q, lm_sum))
    return beams, margin


def chunked(am, cuts, hooks, beam_size, cutoff_top_k, sd, lm_weight, lm_start_token=None, every=None):
    """am (T,V) fed in the pieces [cuts[i], cuts[i+1]) -> (tokens, score, lm_score, frames, margin,
    stable, best): rnnt_lm_fusion_f64.search's five, the common-prefix length of the live beams' token
    sequences after every piece, and the best beam's (tokens, frames, score, lm_sum) after every piece.
    every(beams): called after each piece."""
    beams, margin, stable, best = beam_start(hooks, sd, lm_start_token), float("inf"), [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        beams, m = search_chunk(beams, a, am[a:b], hooks, beam_size, cutoff_top_k, sd, lm_weight)
        margin = min(margin, m)
        stable.append(common_prefix_len([x[0] for x in beams]))
        best.append((list(beams[0][0]), list(beams[0][1]), float(beams[0][2]), float(beams[0][7])))
        if every is not None:
            every(beams)
    if len(beams) > 1:
        margin = min(margin, float(beams[0][2] - beams[1][2]))
    tokens, frames, score = beams[0][:3]
    return list(tokens), float(score), float(beams[0][7]), list(frames), margin, stable, best
