"""Plain restatement of the CTC prefix beam search with hotword (contextual) biasing, with or without the
back-off n-gram (csrc/decode_ctc.hip s2t_ctc_prefix_beam_bias, s2t_ctc_prefix_beam_ngram_bias), keyed by
Python token tuples: the yardstick of tests/test_ctc_bias_f64.py, tests/test_gpu_ctc_bias.py and
tests/test_gpu_ctc_bias_stream.py.

Test infrastructure (not a test file).  Written from the statement, not from the kernel, and it shares no
table and no automaton with the code under test: no trie, no fail links.  `Hotwords` holds the phrases as
a plain list and evaluates, on a hypothesis' WHOLE token history h,

    match(h)      the longest suffix of h that is a prefix (proper or whole) of some phrase
    bias_sum(h) = context_score * len(match(h)) + sum over k in 1..len(h), over every phrase p that h[:k]
                  ends with, of bonus(p)
    final_bias(h) = bias_sum(h) without the first term

by comparing slices of h with slices of the phrases; bonus(p) is phrase_scores[p] if given, else
context_score * len(p); a phrase listed twice counts once.

The search is tests/ctc_prefix_f64.py's (tests/ctc_ngram_f64.py's with an n-gram): candidates rank by
(logaddexp(pb, pnb) + lm_weight * lm_sum) + bias_weight * bias_sum(tokens); when the frames are used up the
reported hypothesis is the live prefix with the largest (logaddexp(pb, pnb) + lm_weight * lm_sum) +
bias_weight * final_bias(tokens), ties to the lower beam position.  It works in the dtype it is given and
reports, besides tokens and the three scores, the smallest decision margin (top-k cuts, beam cuts, the
finalisation's choice) and what occurred: `merged` (an extension landed on a live prefix), `reentered`,
and on the reported hypothesis' own history `cancelled` (a partial match lost to a miss), `completions`
(phrase ends), `overlaps` (a phrase ending inside a longer match), and `final_pos`, the beam position
the finalisation reported.
"""
import collections
import itertools

import numpy as np
import torch

from ctc_prefix_f64 import _Cand, _lae

Result = collections.namedtuple("Result", "tokens score lm_score bias_score margin merged reentered cancelled "
                                          "completions overlaps final_pos")


class Hotwords:
    def __init__(self, phrases, context_score=1.0, phrase_scores=None, dtype=np.float64):
        self.dt, self.cs = dtype, dtype(context_score)
        self.bonus = {}
        for k, p in enumerate(phrases):
            p = tuple(int(t) for t in p)
            self.bonus.setdefault(p, dtype(context_score * len(p)) if phrase_scores is None else dtype(phrase_scores[k]))
        self._memo = {}

    def match_len(self, h):
        for n in range(len(h), 0, -1):
            if any(p[:n] == h[len(h) - n:] for p in self.bonus if len(p) >= n):
                return n
        return 0

    def ending(self, h):
        """The phrases h ends with."""
        return [p for p in self.bonus if len(p) <= len(h) and h[len(h) - len(p):] == p]

    def final_bias(self, h):
        h = tuple(h)
        if h not in self._memo:
            total = self.dt(0.0)
            for k in range(1, len(h) + 1):
                for p in self.ending(h[:k]):
                    total = total + self.bonus[p]
            self._memo[h] = total
        return self._memo[h]

    def bias_sum(self, h):
        h = tuple(h)
        return self.cs * self.dt(self.match_len(h)) + self.final_bias(h)

    def events(self, h):
        """On the history h -> (cancelled partial matches, phrase ends, phrase ends inside a longer match)."""
        h = tuple(h)
        cancelled = completions = overlaps = 0
        for k in range(1, len(h) + 1):
            before, now = self.match_len(h[:k - 1]), self.match_len(h[:k])
            if before > 0 and now < before + 1 and h[k - 1 - before:k - 1] not in self.bonus:
                cancelled += 1
            for p in self.ending(h[:k]):
                completions += 1
                overlaps += len(p) < now
        return cancelled, completions, overlaps


@torch.no_grad()
def prefix_beam_search(logits, beam_size, cutoff_top_k, hot, bias_weight, ng=None, lm_weight=0.0, blank=0):
    """logits (T,V), cut to the utterance's length; hot: Hotwords, ng: a ctc_ngram_f64.DictNgram or None, both
    in the dtype of logits -> Result."""
    T, V = logits.shape
    dt = {torch.float64: np.float64, torch.float32: np.float32}[logits.dtype]
    assert hot.dt is dt and (ng is None or (ng.dt is dt and ng.V == V))
    ninf, zero, w, bw = dt(-np.inf), dt(0.0), dt(lm_weight), dt(bias_weight)
    k = min(int(cutoff_top_k), V)
    lm = {(): zero}                                              # live prefix -> lm_sum
    beam = [((), zero, ninf)]                                    # (tokens, pb, pnb) in beam order
    ever, margin, merged, reentered = {()}, float("inf"), 0, 0
    with_lm = lambda pb, pnb, s: _lae(pb, pnb) + w * s if ng is not None else _lae(pb, pnb)   # noqa: E731
    for t in range(T):
        row = logits[t]
        order = sorted(range(V), key=lambda c: (-float(row[c]), c))
        if k < V:
            margin = min(margin, float(row[order[k - 1]]) - float(row[order[k]]))
        lp = torch.log_softmax(row, dim=-1).numpy()
        live = {p: i for i, (p, _, _) in enumerate(beam)}
        cand = {}

        def add(tokens, key, parent):
            if tokens not in cand:
                cand[tokens] = _Cand(ninf, key, parent, tokens in live)
            return cand[tokens]

        for i, (p, pb, pnb) in enumerate(beam):
            s = _lae(pb, pnb)
            for r, c in enumerate(order[:k]):
                if c == blank:
                    x = add(p, (i, 0, 0), i)
                    x.pb = _lae(x.pb, s + lp[c])
                    continue
                if p and c == p[-1]:
                    if pnb + lp[c] != -np.inf:
                        x = add(p, (i, 0, 0), i)
                        x.pnb = _lae(x.pnb, pnb + lp[c])
                    v = pb + lp[c]
                else:
                    v = s + lp[c]
                if v != -np.inf:
                    ext = p + (c,)
                    merged += ext in live
                    x = add(ext, (i, 1, r), i)
                    x.pnb = _lae(x.pnb, v)
        scored = []
        for tokens, x in cand.items():
            lm_sum = zero
            if ng is not None:
                lm_sum = lm[tokens] if x.live else lm[tokens[:-1]] + ng.score(tokens[:-1], tokens[-1])[0]
            total = with_lm(x.pb, x.pnb, lm_sum) + bw * hot.bias_sum(tokens)
            scored.append((total, x.key, tokens, x, lm_sum))
        scored.sort(key=lambda e: (-float(e[0]), e[1]))
        if len(scored) > beam_size:
            margin = min(margin, float(scored[beam_size - 1][0]) - float(scored[beam_size][0]))
        kept = scored[:beam_size]
        names = {e[2] for e in kept}
        for _, _, tokens, x, _ in kept:
            if not x.live and tokens in ever and any(o[:-1] == tokens for o in names if o):
                reentered += 1
            ever.add(tokens)
        beam = [(e[2], e[3].pb, e[3].pnb) for e in kept]
        lm = {e[2]: e[4] for e in kept}
    if T == 0:
        return Result([], 0.0, 0.0, 0.0, margin, 0, 0, 0, 0, 0, 0)
    final = [with_lm(pb, pnb, lm[p]) + bw * hot.final_bias(p) for p, pb, pnb in beam]
    pos = max(range(len(beam)), key=lambda i: (float(final[i]), -i))
    if len(beam) > 1:
        rest = max(float(final[i]) for i in range(len(beam)) if i != pos)
        margin = min(margin, float(final[pos]) - rest)
    p, pb, pnb = beam[pos]
    cancelled, completions, overlaps = hot.events(p)
    return Result(list(p), float(_lae(pb, pnb)), float(lm[p]), float(hot.final_bias(p)), margin, merged, reentered,
                  cancelled, completions, overlaps, pos)


def brute_force(logits, hot, bias_weight, ng=None, lm_weight=0.0, blank=0):
    """All V^T alignments, summed per label sequence in float64; the labels that maximise logsumexp(alignments)
    + lm_weight * (the n-gram's score of the labels) + bias_weight * final_bias(labels) -> (the best labelling,
    its acoustic log-probability, its n-gram score, its final_bias, its distance to the second best)."""
    T, V = logits.shape
    lp = torch.log_softmax(logits.double(), dim=-1).numpy()
    prob = collections.defaultdict(float)
    for path in itertools.product(range(V), repeat=T):
        lab, last = [], blank
        for c in path:
            if c != blank and c != last:
                lab.append(c)
            last = c
        prob[tuple(lab)] += float(np.exp(sum(lp[t, c] for t, c in enumerate(path))))
    lms = {s: float(ng.sentence(s)) if ng is not None else 0.0 for s in prob}
    tot = {s: float(np.log(prob[s])) + lm_weight * lms[s] + bias_weight * float(hot.final_bias(s)) for s in prob}
    ranked = sorted(tot, key=lambda s: -tot[s])
    best = ranked[0]
    gap = tot[best] - tot[ranked[1]] if len(ranked) > 1 else float("inf")
    return list(best), float(np.log(prob[best])), lms[best], float(hot.final_bias(best)), gap
