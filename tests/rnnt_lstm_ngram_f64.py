"""Plain restatement of the RNN-T beam search of the LSTM predictor with back-off n-gram shallow fusion
(csrc/decode_lstm.hip s2t_rnnt_beam_lstm_ngram, s2t_rnnt_beam_lstm_ngram_chunk), keyed by Python token
tuples, over a dict-based n-gram: the yardstick of tests/test_rnnt_lstm_ngram_f64.py and
tests/test_gpu_rnnt_lstm_ngram.py.

Test infrastructure (not a test file).  Written from the header's statement, not from the kernels: the
frame of tests/rnnt_ngram_f64.Search (candidates, the LM term, the two orders, the margins, the chunked
form) with the predictor and joiner arithmetic of tests/rnnt_lstm_search_f64.py (pred_step, joint) in place
of the stateless predictor's.  The language model is tests/ctc_ngram_f64.py's DictNgram on the hypothesis'
WHOLE token history from `<s>`: no shared table and no context id.

A beam is (tokens, frames, score, predictor state, lm vector, lm_sum).  Per frame and beam the cutoff_top_k
classes of lp = log_softmax(joint(am[t], lm)) give one candidate each (the LM does not enter the cut):
blank keeps everything and scores score + lp; class c != blank appends c, takes q = log p_lm(c | tokens)
and scores (score + lp) + lm_weight * q, lm_sum + q; a kept candidate that emitted steps the predictor.
Everything is computed in the dtype given.
"""
import itertools

import numpy as np
import torch

import rnnt_lstm_search_f64 as S
from rnnt_ngram_f64 import Result
from rnnt_stream_restatement import common_prefix_len


class Search:
    def __init__(self, w, act, beam_size, cutoff_top_k, ng, lm_weight, dtype=torch.float64):
        self.w, self.act, self.dtype = S.cast(w, dtype), act, dtype
        self.dt = {torch.float64: np.float64, torch.float32: np.float32}[dtype]
        assert ng.dt is self.dt
        self.beam, self.topk, self.ng = int(beam_size), int(cutoff_top_k), ng
        self.wt = torch.tensor(lm_weight, dtype=dtype)
        self.hops, self.root = set(), False

    def initial(self):
        lm, state = S._start(self.w)
        return [((), (), torch.zeros((), dtype=self.dtype), state, lm, self.dt(0.0))]

    @torch.no_grad()
    def chunk(self, beams, t0, am):
        am = am.to(self.dtype)
        Tc, V = am.shape
        k = min(self.topk, V)
        margin = float("inf")
        for t in range(Tc):
            z, _ = S.joint(self.w, am[t], torch.cat([b[4] for b in beams], 0), self.act)
            lps = torch.log_softmax(z, dim=-1)
            cands = []
            for (tokens, frames, score, st, lmv, lm_sum), lp in zip(beams, lps):
                vals, order = torch.sort(lp, descending=True, stable=True)   # value desc, class asc
                if k < V:
                    margin = min(margin, float(vals[k - 1] - vals[k]))
                for v, c in zip(vals[:k], order[:k].tolist()):
                    if c == 0:                             # blank: no LM term, no look-up
                        cands.append((tokens, frames, score + v, st, lmv, lm_sum, 0))
                        continue
                    q, n, at_root = self.ng.score(tokens, c)
                    self.hops.add(n)
                    self.root = self.root or at_root
                    total = (score + v) + self.wt * torch.tensor(q, dtype=self.dtype)
                    cands.append((tokens + (c,), frames + (t0 + t,), total, st, lmv, lm_sum + q, c))
            cands.sort(key=lambda x: float(x[2]), reverse=True)  # stable: parent position, then rank
            if len(cands) > self.beam:
                margin = min(margin, float(cands[self.beam - 1][2] - cands[self.beam][2]))
            beams = []
            for tokens, frames, score, st, lmv, lm_sum, c in cands[:self.beam]:
                if c != 0:
                    lmv, st = S.pred_step(self.w, torch.tensor([c]), st)
                beams.append((tokens, frames, score, st, lmv, lm_sum))
        return beams, margin

    def result(self, beams, margin, T):
        if T == 0:
            return Result([], 0.0, 0.0, [], float("inf"), set(), False)
        if len(beams) > 1:
            margin = min(margin, float(beams[0][2] - beams[1][2]))
        tokens, frames, score = beams[0][:3]
        return Result(list(tokens), float(score), float(beams[0][5]), list(frames), float(margin), set(self.hops),
                      self.root)


def beam_search(am, w, act, beam_size, cutoff_top_k, ng, lm_weight, dtype=torch.float64):
    """am (T,V), cut to the utterance's length; ng: a DictNgram in `dtype` -> rnnt_ngram_f64.Result."""
    s = Search(w, act, beam_size, cutoff_top_k, ng, lm_weight, dtype)
    T = am.shape[0]
    if T == 0:
        return s.result(None, float("inf"), 0)
    beams, margin = s.chunk(s.initial(), 0, am)
    return s.result(beams, margin, T)


def beam_search_chunked(am, cuts, w, act, beam_size, cutoff_top_k, ng, lm_weight, dtype=torch.float64):
    """am (T,V) fed as the pieces [cuts[i], cuts[i+1]) (an empty piece is an idle call) -> (Result of the
    whole, [Result after every piece], [the live beams' common-prefix length after every piece])."""
    s = Search(w, act, beam_size, cutoff_top_k, ng, lm_weight, dtype)
    beams, margin, after, stable = s.initial(), float("inf"), [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            beams, m = s.chunk(beams, a, am[a:b])
            margin = min(margin, m)
        after.append(s.result(beams, margin, b))
        stable.append(common_prefix_len(beams))
    return s.result(beams, margin, cuts[-1]), after, stable


@torch.no_grad()
def brute_force(am, w, act, ng, lm_weight):
    """All V^T frame labellings (blank or one symbol per frame) in float64: path log-probability +
    lm_weight x the dict n-gram's score of the emitted tokens from `<s>` -> (tokens, frames, total, the
    n-gram score, distance to the second best labelling) of the best one."""
    w, am = S.cast(w, torch.float64), am.double()
    T, V = am.shape
    rows = []
    for path in itertools.product(range(V), repeat=T):
        (lm, state), tokens, frames, total = S._start(w), (), (), 0.0
        for t, c in enumerate(path):
            total += float(torch.log_softmax(S.joint(w, am[t], lm, act)[0], dim=-1)[0, c])
            if c != 0:
                lm, state = S.pred_step(w, torch.tensor([c]), state)
                tokens, frames = tokens + (c,), frames + (t,)
        lms = float(ng.sentence(tokens))
        rows.append((total + lm_weight * lms, tokens, frames, lms))
    rows.sort(key=lambda r: -r[0])
    return list(rows[0][1]), list(rows[0][2]), float(rows[0][0]), rows[0][3], float(rows[0][0] - rows[1][0])
