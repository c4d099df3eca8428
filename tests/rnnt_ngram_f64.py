"""Plain restatement of the RNN-T beam search of the stateless predictor with back-off n-gram shallow
fusion (csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_ngram and
s2t_rnnt_beam_stateless_ngram_chunk), keyed by Python token tuples, over a dict-based n-gram: the
yardstick of tests/test_rnnt_ngram_f64.py, tests/test_gpu_rnnt_ngram.py and
tests/test_gpu_rnnt_ngram_stream.py.

Test infrastructure (not a test file).  The predictor and joiner arithmetic and the two orders are
tests/rnnt_beam_restatement.py's (lm_vector, log_softmax; top-k by (log-probability descending, class
ascending), candidates by (score descending, parent position, rank in the parent's top-k)); the chunked
form is tests/rnnt_stream_restatement.py's.  The language model is tests/ctc_ngram_f64.py's DictNgram,
which reads the ARPA text with a parser of its own and evaluates the back-off rule on the hypothesis'
WHOLE token history from `<s>`: it shares the text with the code under test, no table and no context id.

The statement: a beam is (tokens, frames, score, predictor state, lm_sum), the empty hypothesis has score
0 and lm_sum 0.  Per frame and beam the cutoff_top_k classes of lp = log_softmax(act(am[t] + lm(state)))
give one candidate each (the LM does not enter the cut): blank keeps tokens, state and lm_sum and scores
score + lp; class c != blank appends c, takes q = log p_lm(c | tokens) -- the first token is scored too,
there is no end term -- and scores (score + lp) + lm_weight * q, lm_sum + q.  The beam_size best
candidates survive, equal hypotheses are not merged.  Everything is computed in the dtype given.

Besides the result the search reports its decision margin (the smallest gap at a top-k cut, at a beam
cut, and between the two best beams at the end) and which numbers of back-offs through listed contexts
the look-ups took (`hops`) and whether one reached the unigrams (`root`).
"""
import collections
import itertools

import numpy as np

from rnnt_beam_restatement import PARAM_KEYS, lm_vector, log_softmax
from rnnt_stream_restatement import common_prefix_len

Result = collections.namedtuple("Result", "tokens score lm_score frames margin hops root")


class Search:
    """The weights, the n-gram and the settings of one search in one dtype; `chunk` advances a beam list."""

    def __init__(self, params, ctx, act, beam_size, cutoff_top_k, ng, lm_weight, dtype=np.float64):
        assert ng.dt is dtype
        self.p = {k: np.asarray(params[k]).astype(dtype) for k in PARAM_KEYS}
        self.ctx, self.beam, self.topk, self.ng, self.dt = ctx, int(beam_size), int(cutoff_top_k), ng, dtype
        self.w = dtype(lm_weight)
        self.fn = (lambda z: np.maximum(z, dtype(0.0))) if act == "relu" else np.tanh
        self.cache, self.hops, self.root = {}, set(), False

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
                    if c == 0:                             # blank: no LM term, no look-up
                        cands.append((tokens, frames, score + lp[c], state, lm_sum))
                        continue
                    q, n, at_root = self.ng.score(tokens, c)
                    self.hops.add(n)
                    self.root = self.root or at_root
                    cands.append((tokens + (c,), frames + (t0 + t,), (score + lp[c]) + self.w * q,
                                  state[1:] + (c,), lm_sum + q))
            cands.sort(key=lambda x: x[2], reverse=True)   # stable: parent position, then top-k rank
            if len(cands) > self.beam:
                margin = min(margin, float(cands[self.beam - 1][2] - cands[self.beam][2]))
            beams = cands[:self.beam]
        return beams, margin

    def result(self, beams, margin, T):
        if T == 0:
            return Result([], 0.0, 0.0, [], float("inf"), set(), False)
        if len(beams) > 1:
            margin = min(margin, float(beams[0][2] - beams[1][2]))
        tokens, frames, score, _, lm_sum = beams[0]
        return Result(list(tokens), float(score), float(lm_sum), list(frames), float(margin), set(self.hops),
                      self.root)


def beam_search(am, params, ctx, act, beam_size, cutoff_top_k, ng, lm_weight, dtype=np.float64):
    """am [T][V], cut to the utterance's length; ng: a DictNgram in `dtype` -> Result."""
    s = Search(params, ctx, act, beam_size, cutoff_top_k, ng, lm_weight, dtype)
    T = len(am)
    if T == 0:
        return s.result(None, np.inf, 0)
    beams, margin = s.chunk(s.initial(), 0, am)
    return s.result(beams, margin, T)


def beam_search_chunked(am, cuts, params, ctx, act, beam_size, cutoff_top_k, ng, lm_weight, dtype=np.float64):
    """am [T][V] fed as the pieces [cuts[i], cuts[i+1]) (0 = c0 <= c1 <= ... = T; an empty piece is an idle
    call) -> (Result of the whole, [the live beams' common-prefix length after every piece])."""
    s = Search(params, ctx, act, beam_size, cutoff_top_k, ng, lm_weight, dtype)
    beams, margin, stable = s.initial(), np.inf, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            beams, m = s.chunk(beams, a, am[a:b])
            margin = min(margin, m)
        stable.append(common_prefix_len(beams))
    return s.result(beams, margin, cuts[-1]), stable


def brute_force(am, params, ctx, act, ng, lm_weight):
    """All V^T frame labellings (blank or one symbol per frame) in float64: path log-probability +
    lm_weight x the dict n-gram's score of the emitted tokens from `<s>` -> (tokens, frames, total, the
    n-gram score, distance to the second best labelling) of the best one."""
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
        lms = float(ng.sentence(tokens))
        rows.append((total + lm_weight * lms, tokens, frames, lms))
    rows.sort(key=lambda r: -r[0])
    return list(rows[0][1]), list(rows[0][2]), float(rows[0][0]), rows[0][3], float(rows[0][0] - rows[1][0])
