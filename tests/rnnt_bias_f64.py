"""Plain restatement of the one-launch RNN-T beam search of the stateless predictor with hotword (contextual)
biasing, without and with the back-off n-gram (csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_bias,
s2t_rnnt_beam_stateless_ngram_bias and their chunk forms), keyed by Python token tuples: the yardstick of
tests/test_rnnt_bias_f64.py, tests/test_gpu_rnnt_bias.py and tests/test_gpu_rnnt_bias_stream.py.

Test infrastructure (not a test file).  It is tests/rnnt_ngram_f64.py's beam search (the predictor and joiner
arithmetic and the two orders of tests/rnnt_beam_restatement.py, the dict n-gram of tests/ctc_ngram_f64.py on the
hypothesis' whole history) with the bias term of tests/ctc_bias_f64.py's statement: `Hotwords` keeps the phrases
as a plain list and evaluates match, bias_sum and final_bias on a hypothesis' WHOLE token history by comparing
slices.  No trie, no fail links, no graph state, no table shared with the code under test.

The statement: a beam is (tokens, frames, score, predictor state, lm_sum), the empty hypothesis has score 0.  Per
frame and beam the cutoff_top_k classes of lp = log_softmax(act(am[t] + lm(state))) give one candidate each
(neither the LM nor the bias enters the cut): blank keeps everything and scores score + lp; class c != blank
appends c and scores ((score + lp) + lm_weight * q) + bias_weight * d with q = log p_lm(c | tokens) (no LM: no LM
term) and d = bias_sum(tokens + c) - bias_sum(tokens).  The beam_size best candidates survive, equal hypotheses
are not merged.  FINALISATION: when the frames are used up (or after a chunk) the reported hypothesis is the live
beam with the largest score + bias_weight * (final_bias(tokens) - bias_sum(tokens)), ties to the lower position;
that value is its score, bias_score is final_bias(tokens), lm_score its own lm_sum.  Nothing of the pick enters
the beams.  Everything is computed in the dtype given.

Besides the result the search reports its decision margin (the smallest gap at a top-k cut, at a beam cut and
at the finalisation's pick) and, on the reported hypothesis' own history, the named events:
    completions   phrase ends
    nested        a phrase ending inside a longer match (its bonus is paid on the longer phrase's arc)
    lost1, lost2  an unfinished match of 1 / of >= 2 tokens lost to a miss (the loan is paid back; from >= 2 tokens
                  through a fail hop)
    midphrase     the history ends inside an unfinished match (1 or 0)
    final_pos     the beam position the finalisation reported
"""
import collections
import itertools

import numpy as np

from ctc_bias_f64 import Hotwords  # noqa: F401  (the statement on whole histories; re-exported for the cases)
from rnnt_beam_restatement import PARAM_KEYS, lm_vector, log_softmax
from rnnt_stream_restatement import common_prefix_len

Result = collections.namedtuple("Result", "tokens score lm_score bias_score frames margin completions nested lost1 "
                                          "lost2 midphrase final_pos")


def events(hot, h):
    """On the history h -> (completions, nested, lost1, lost2, midphrase)."""
    h = tuple(h)
    completions = nested = lost1 = lost2 = 0
    for k in range(1, len(h) + 1):
        before, now = hot.match_len(h[:k - 1]), hot.match_len(h[:k])
        if before > 0 and now < before + 1 and h[k - 1 - before:k - 1] not in hot.bonus:
            lost1 += before == 1
            lost2 += before >= 2
        for p in hot.ending(h[:k]):
            completions += 1
            nested += len(p) < now
    n = hot.match_len(h)
    return completions, nested, lost1, lost2, int(n > 0 and h[len(h) - n:] not in hot.bonus)


class Search:
    """The weights, the phrases, the n-gram (or None) and the settings of one search in one dtype; `chunk`
    advances a beam list, `result` finalises one without changing it."""

    def __init__(self, params, ctx, act, beam_size, cutoff_top_k, hot, bias_weight, ng=None, lm_weight=0.0,
                 dtype=np.float64):
        assert hot.dt is dtype and (ng is None or ng.dt is dtype)
        self.p = {k: np.asarray(params[k]).astype(dtype) for k in PARAM_KEYS}
        self.ctx, self.beam, self.topk, self.dt = ctx, int(beam_size), int(cutoff_top_k), dtype
        self.hot, self.ng, self.bw, self.w = hot, ng, dtype(bias_weight), dtype(lm_weight)
        self.fn = (lambda z: np.maximum(z, dtype(0.0))) if act == "relu" else np.tanh
        self.cache = {}

    def initial(self):
        """The empty hypothesis: (tokens, frames, score, predictor state = ctx blanks, lm_sum)."""
        return [((), (), self.dt(0.0), (0,) * self.ctx, self.dt(0.0))]

    def _lm(self, state):
        if state not in self.cache:
            self.cache[state] = lm_vector(state, self.p)
        return self.cache[state]

    def chunk(self, beams, t0, am):
        """beams after frames [0, t0) + am [Tc][V] = frames [t0, t0 + Tc) -> (beams after them, the smallest
        decision gap inside the chunk: the top-k cuts and the beam cuts)."""
        am = np.asarray(am).astype(self.dt)
        Tc, V = am.shape
        k = min(self.topk, V)
        margin = np.inf
        for t in range(Tc):
            cands = []
            for tokens, frames, score, state, lm_sum in beams:
                lp = log_softmax(self.fn(am[t] + self._lm(state)))
                order = np.argsort(-lp, kind="stable")     # value descending, class ascending
                if k < V:
                    margin = min(margin, float(lp[order[k - 1]] - lp[order[k]]))
                for c in order[:k].tolist():
                    if c == 0:                             # blank: no LM term, no bias term
                        cands.append((tokens, frames, score + lp[c], state, lm_sum))
                        continue
                    v = score + lp[c]
                    if self.ng is not None:
                        q = self.ng.score(tokens, c)[0]
                        v, lm_sum_c = v + self.w * q, lm_sum + q
                    else:
                        lm_sum_c = lm_sum
                    d = self.hot.bias_sum(tokens + (c,)) - self.hot.bias_sum(tokens)
                    cands.append((tokens + (c,), frames + (t0 + t,), v + self.bw * d, state[1:] + (c,), lm_sum_c))
            cands.sort(key=lambda x: x[2], reverse=True)   # stable: parent position, then top-k rank
            if len(cands) > self.beam:
                margin = min(margin, float(cands[self.beam - 1][2] - cands[self.beam][2]))
            beams = cands[:self.beam]
        return beams, margin

    def result(self, beams, margin, T):
        if T == 0:
            return Result([], 0.0, 0.0, 0.0, [], float("inf"), 0, 0, 0, 0, 0, 0)
        final = [b[2] + self.bw * (self.hot.final_bias(b[0]) - self.hot.bias_sum(b[0])) for b in beams]
        pos = max(range(len(beams)), key=lambda i: (float(final[i]), -i))
        if len(beams) > 1:
            margin = min(margin, float(final[pos]) - max(float(final[i]) for i in range(len(beams)) if i != pos))
        tokens, frames, _, _, lm_sum = beams[pos]
        return Result(list(tokens), float(final[pos]), float(lm_sum), float(self.hot.final_bias(tokens)),
                      list(frames), float(margin), *events(self.hot, tokens), pos)


def beam_search(am, params, ctx, act, beam_size, cutoff_top_k, hot, bias_weight, ng=None, lm_weight=0.0,
                dtype=np.float64):
    """am [T][V], cut to the utterance's length; hot: Hotwords, ng: a DictNgram or None, in `dtype` -> Result."""
    s = Search(params, ctx, act, beam_size, cutoff_top_k, hot, bias_weight, ng, lm_weight, dtype)
    T = len(am)
    if T == 0:
        return s.result(None, np.inf, 0)
    beams, margin = s.chunk(s.initial(), 0, am)
    return s.result(beams, margin, T)


def beam_search_chunked(am, cuts, params, ctx, act, beam_size, cutoff_top_k, hot, bias_weight, ng=None,
                        lm_weight=0.0, dtype=np.float64):
    """am [T][V] fed as the pieces [cuts[i], cuts[i+1]) (an empty piece is an idle call) -> ([the Result after
    every piece: the finalisation of the beams as they stand], [the live beams' common-prefix length then])."""
    s = Search(params, ctx, act, beam_size, cutoff_top_k, hot, bias_weight, ng, lm_weight, dtype)
    beams, margin, results, stable = s.initial(), np.inf, [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            beams, m = s.chunk(beams, a, am[a:b])
            margin = min(margin, m)
        results.append(s.result(beams, margin, b))
        stable.append(common_prefix_len(beams))
    return results, stable


def brute_force(am, params, ctx, act, hot, bias_weight, ng=None, lm_weight=0.0):
    """All V^T frame labellings (blank or one symbol per frame) in float64: path log-probability + lm_weight x the
    dict n-gram's score of the emitted tokens + bias_weight x final_bias(tokens) -> (tokens, frames, total, the
    n-gram score, final_bias, distance to the second best labelling) of the best one."""
    p = {k: np.asarray(params[k], dtype=np.float64) for k in PARAM_KEYS}
    am = np.asarray(am, dtype=np.float64)
    T, V = am.shape
    fn = (lambda z: np.maximum(z, 0.0)) if act == "relu" else np.tanh
    rows = []
    for path in itertools.product(range(V), repeat=T):
        state, tokens, frames, total = (0,) * ctx, (), (), 0.0
        for t, c in enumerate(path):
            total += log_softmax(fn(am[t] + lm_vector(state, p)))[c]
            if c != 0:
                state, tokens, frames = state[1:] + (c,), tokens + (c,), frames + (t,)
        lms = float(ng.sentence(tokens)) if ng is not None else 0.0
        fb = float(hot.final_bias(tokens))
        rows.append((total + lm_weight * lms + bias_weight * fb, tokens, frames, lms, fb))
    rows.sort(key=lambda r: -r[0])
    return (list(rows[0][1]), list(rows[0][2]), float(rows[0][0]), rows[0][3], rows[0][4],
            float(rows[0][0] - rows[1][0]))
