"""Plain restatement of the CTC prefix beam search of csrc/decode_ctc.hip, keyed by Python token
tuples: the yardstick of tests/test_ctc_prefix_f64.py and tests/test_gpu_ctc_prefix_beam.py.

Test infrastructure (not a test file).  Written from the statement of the search, not from the kernel:
a live prefix carries pb / pnb, the log-probabilities of its alignments that end in blank / in a
non-blank; per frame the k = min(cutoff_top_k, V) classes by (logit descending, class ascending)
contribute to the staying prefix (blank, repeat of the last token) and to its extensions, candidates
with equal token sequences are ONE candidate, the beam_size best by logaddexp(pb, pnb) + lm_weight *
lm_sum survive.  A dict keyed by the token tuple makes the merge exact by construction.

It works in the dtype it is given (numpy scalars of that dtype: float64 for the reference, float32 to
measure what fp32 costs) and reports per utterance the tokens, score, lm_score, the decision margin
(the smallest gap at any top-k cut, at any beam cut and between the final two prefixes) and two
counters: `merged` (an extension landed on a live prefix) and `reentered` (a prefix that had left the
beam was kept again while one of its one-token extensions is kept with it).
"""
import collections

import numpy as np
import torch

import rnn_lm_f64 as R
import rnnt_lm_fusion_f64 as LF

Result = collections.namedtuple("Result", "tokens score lm_score margin merged reentered")


def _lae(a, b):
    """logaddexp in the dtype of a and b; -inf is the empty sum and never meets -inf - -inf."""
    if a == -np.inf:
        return b
    if b == -np.inf:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return hi + np.log1p(np.exp(lo - hi))


class _Cand:
    __slots__ = ("pb", "pnb", "key", "parent", "live")

    def __init__(self, ninf, key, parent, live):
        self.pb, self.pnb, self.key, self.parent, self.live = ninf, ninf, key, parent, live


@torch.no_grad()
def prefix_beam_search(logits, beam_size, cutoff_top_k, blank=0, sd=None, lm_weight=0.0, lm_start_token=None):
    """logits (T,V), cut to the utterance's length, raw or already normalised; sd: an RNN-LM state dict
    in the dtype of logits, or None -> Result."""
    T, V = logits.shape
    dt = {torch.float64: np.float64, torch.float32: np.float32}[logits.dtype]
    ninf, zero, w = dt(-np.inf), dt(0.0), dt(lm_weight)
    k = min(int(cutoff_top_k), V)
    fused = sd is not None
    if fused:
        q0, st0 = LF.lm_start(sd, lm_start_token)
        lm = {(): (q0.numpy().astype(dt), st0, zero)}           # live prefix -> (q (V), LM state, lm_sum)
    beam = [((), zero, ninf)]                                    # (tokens, pb, pnb) in beam order
    ever, margin, merged, reentered = {()}, float("inf"), 0, 0
    total = lambda pb, pnb, s: _lae(pb, pnb) + (w * s if fused else zero)   # noqa: E731
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
                lm_sum = lm[tokens][2] if fused else zero
            else:
                lm_sum = lm[tokens[:-1]][2] + lm[tokens[:-1]][0][tokens[-1]] if fused else zero
            scored.append((total(x.pb, x.pnb, lm_sum), x.key, tokens, x, lm_sum))
        scored.sort(key=lambda e: (-float(e[0]), e[1]))
        if len(scored) > beam_size:
            margin = min(margin, float(scored[beam_size - 1][0]) - float(scored[beam_size][0]))
        kept = scored[:beam_size]
        names = {e[2] for e in kept}
        new_lm = {}
        for _, _, tokens, x, lm_sum in kept:
            if not x.live:
                if tokens in ever and any(o[:-1] == tokens for o in names if o):
                    reentered += 1
                if fused:
                    q, st = R.score_step_ref(sd, torch.tensor([tokens[-1]]), lm[tokens[:-1]][1])
                    new_lm[tokens] = (q[0].numpy().astype(dt), st, lm_sum)
            elif fused:
                new_lm[tokens] = lm[tokens]
            ever.add(tokens)
        beam = [(e[2], e[3].pb, e[3].pnb) for e in kept]
        if fused:
            lm = new_lm
    p, pb, pnb = beam[0]
    if T == 0:
        return Result([], 0.0, 0.0, margin, 0, 0)
    if len(beam) > 1:
        tot = [total(b[1], b[2], lm[b[0]][2] if fused else zero) for b in beam[:2]]
        margin = min(margin, float(tot[0]) - float(tot[1]))
    return Result(list(p), float(_lae(pb, pnb)), float(lm[p][2]) if fused else 0.0, margin, merged, reentered)


def greedy_collapse(logits, blank=0):
    """The arg-max per frame (first index wins), repeats collapsed, blanks dropped."""
    out, last = [], blank
    for t in range(logits.shape[0]):
        row = logits[t]
        c = min(range(row.shape[0]), key=lambda j: (-float(row[j]), j))
        if c != blank and c != last:
            out.append(c)
        last = c
    return out


def brute_force(logits, blank=0):
    """All V^T alignments, summed per label sequence in float64 -> (the most probable labelling, its
    log-probability, its distance to the second most probable one)."""
    import itertools
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
    ranked = sorted(prob, key=lambda s: -prob[s])
    best = ranked[0]
    gap = float(np.log(prob[best]) - np.log(prob[ranked[1]])) if len(ranked) > 1 else float("inf")
    return list(best), float(np.log(prob[best])), gap
