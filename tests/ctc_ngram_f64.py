"""Plain restatement of the CTC prefix beam search with back-off n-gram shallow fusion
(csrc/decode_ctc.hip s2t_ctc_prefix_beam_ngram), keyed by Python token tuples, over a dict-based n-gram:
the yardstick of tests/test_ctc_ngram_f64.py and tests/test_gpu_ctc_ngram.py.

Test infrastructure (not a test file).  Written from the statement of the search, not from the kernel,
and it shares no table with the code under test: DictNgram reads an ARPA text with a parser of its own
into {n-gram tuple: value} dicts and evaluates the back-off rule on the hypothesis' whole token history
(`<s>` in front when the text lists it): p(c | h) is the listed value of h + c where there is one, else
back-off(h) (0 where none is listed) plus p(c | h without its oldest token); a class without a unigram
takes `missing_logp`.  Entries with `</s>` are dropped: there is no end term.

The search is tests/ctc_prefix_f64.py's with the LM term changed: an extension p + c that is not live has
lm_sum(p) + p(c | p), from the start of the sentence on (the first token is scored too); a candidate that
is a live prefix keeps its lm_sum.  It works in the dtype it is given and reports, besides what
ctc_prefix_f64.Result holds, how often the look-ups of candidates backed off (`hops`: the set of
back-off counts through listed contexts that occurred) and whether one reached the unigrams (`root`).
"""
import collections
import itertools
import math

import numpy as np
import torch

from ctc_prefix_f64 import _Cand, _lae

Result = collections.namedtuple("Result", "tokens score lm_score margin merged reentered hops root")
BOS = "<s>"
_LN10 = math.log(10.0)


class DictNgram:
    def __init__(self, text, num_classes, token_to_id=None, missing_logp=-30.0, dtype=np.float64):
        """text: a well-formed ARPA text whose words are decimal class ids, or keys of token_to_id."""
        self.V, self.dt = num_classes, dtype
        self.probs, self.backoffs, self.order, self.bos = {}, {}, 0, False
        self.missing = dtype(missing_logp)
        k = 0
        for line in text.split("\n"):
            line = line.strip()
            if line.endswith("-grams:"):
                k = int(line[1:-7])
                self.order = max(self.order, k)
                continue
            if not line or line.startswith("\\") or line.startswith("ngram ") or k == 0:
                continue
            parts = line.split()
            words = parts[1:1 + k]
            if "</s>" in words:
                continue
            ids = []
            for w in words:
                if w == BOS:
                    ids.append(BOS)
                elif token_to_id is not None:
                    ids.append(token_to_id.get(w))
                else:
                    ids.append(int(w))
            if None in ids:                                # an <unk> the classes do not have
                assert set(w for w, i in zip(words, ids) if i is None) == {"<unk>"}
                continue
            g = tuple(ids)
            if g == (BOS,):
                self.bos = True
            else:
                self.probs[g] = dtype(np.float64(parts[0]) * _LN10)
            if len(parts) == k + 2:
                self.backoffs[g] = dtype(np.float64(parts[-1]) * _LN10)
        ctx = {g[:-1] for g in self.probs if len(g) > 1} | {h for h, b in self.backoffs.items()
                                                            if b != 0 and len(h) < self.order}
        for h in list(ctx):                                # what the statement calls a context: listed, or a suffix
            for i in range(1, len(h)):
                ctx.add(h[i:])
        self.contexts = ctx

    def history(self, tokens):
        return ((BOS,) if self.bos else ()) + tuple(tokens)

    def score(self, tokens, c):
        """log p(c | the sentence so far) -> (value, back-offs through listed contexts, reached the unigrams)."""
        return self.score_in(self.history(tokens), c)

    def score_in(self, h, c):
        """The same after an explicit history h (BOS where a sentence starts)."""
        h = h[max(0, len(h) - (self.order - 1)):] if self.order > 1 else ()
        acc, hops = self.dt(0.0), 0
        while True:
            if h + (c,) in self.probs:
                return acc + self.probs[h + (c,)], hops, not h
            if not h:
                return acc + self.missing, hops, True
            if h in self.contexts:
                acc = acc + self.backoffs.get(h, self.dt(0.0))
                hops += 1
            h = h[1:]

    def sentence(self, tokens):
        """The sum over a token sequence, from the start of the sentence."""
        total = self.dt(0.0)
        for i, c in enumerate(tokens):
            total = total + self.score(tokens[:i], c)[0]
        return total


@torch.no_grad()
def prefix_beam_search(logits, beam_size, cutoff_top_k, ng, lm_weight, blank=0):
    """logits (T,V), cut to the utterance's length; ng: a DictNgram in the dtype of logits -> Result."""
    T, V = logits.shape
    dt = {torch.float64: np.float64, torch.float32: np.float32}[logits.dtype]
    assert ng.dt is dt and ng.V == V
    ninf, zero, w = dt(-np.inf), dt(0.0), dt(lm_weight)
    k = min(int(cutoff_top_k), V)
    lm = {(): zero}                                              # live prefix -> lm_sum
    beam = [((), zero, ninf)]                                    # (tokens, pb, pnb) in beam order
    ever, margin, merged, reentered, hops, root = {()}, float("inf"), 0, 0, set(), False
    total = lambda pb, pnb, s: _lae(pb, pnb) + w * s             # noqa: E731
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
            if x.live:
                lm_sum = lm[tokens]
            else:
                q, n, at_root = ng.score(tokens[:-1], tokens[-1])
                hops.add(n)
                root = root or at_root
                lm_sum = lm[tokens[:-1]] + q
            scored.append((total(x.pb, x.pnb, lm_sum), x.key, tokens, x, lm_sum))
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
    p, pb, pnb = beam[0]
    if T == 0:
        return Result([], 0.0, 0.0, margin, 0, 0, hops, root)
    if len(beam) > 1:
        tot = [total(b[1], b[2], lm[b[0]]) for b in beam[:2]]
        margin = min(margin, float(tot[0]) - float(tot[1]))
    return Result(list(p), float(_lae(pb, pnb)), float(lm[p]), margin, merged, reentered, hops, root)


def brute_force(logits, ng, lm_weight, blank=0):
    """All V^T alignments, summed per label sequence in float64, plus lm_weight x the dict n-gram's score of
    the labels -> (the best labelling, its acoustic log-probability, its n-gram score, its distance to
    the second best)."""
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
    lms = {s: float(ng.sentence(s)) for s in prob}
    tot = {s: float(np.log(prob[s])) + lm_weight * lms[s] for s in prob}
    ranked = sorted(tot, key=lambda s: -tot[s])
    best = ranked[0]
    gap = tot[best] - tot[ranked[1]] if len(ranked) > 1 else float("inf")
    return list(best), float(np.log(prob[best])), lms[best], gap
