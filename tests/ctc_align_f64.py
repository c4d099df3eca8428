"""The statement of CTC forced alignment (include/s2t_mi355.h, above s2t_ctc_align) restated in plain
Python / torch over ONE utterance, in the dtype of its input.  Test infrastructure (not a test file).

    align(x, targets, blank) -> Result

x (Tb, V): the utterance's own frames (raw logits or log-probabilities), targets: a list of U labels.
The recursion is the statement's, a frame at a time over all states at once: every value is one maximum
of up to three candidates and one addition in x's dtype, the backpointer the first maximum in the order
stay, step, skip.  In float32 that is the arithmetic of csrc/ctc_align.hip, so path, spans and raw_score
of the float32 run are the kernel's bit for bit; score and tok_logp involve a log-sum-exp and are
compared with the float64 run under a bound.
"""
import collections
import math

import torch

Result = collections.namedtuple(
    "Result", ["ok", "path", "tok_begin", "tok_end", "tok_logp", "raw_score", "score", "ties"])
# ok: bool; path: list of Tb states ([] when infeasible); tok_begin / tok_end: lists of U frames (-1 when
# infeasible); tok_logp: list of U Python floats (the dtype's values); raw_score, score: Python floats;
# ties: decisions ON THE BEST PATH in which two live candidates were equal (the end state's included).


def _shift(v, n, neg):
    return torch.cat([neg[:n], v[:-n]]) if n < v.shape[0] else neg[:v.shape[0]]


def align(x, targets, blank=0):
    dtype = x.dtype
    Tb, V = x.shape
    U = len(targets)
    S = 2 * U + 1
    inf = math.inf
    if Tb == 0:
        ok = U == 0
        return Result(ok, [], [-1] * U, [-1] * U, [0.0] * U, 0.0 if ok else -inf, 0.0 if ok else -inf, 0)
    lab = torch.tensor([blank if s % 2 == 0 else targets[s >> 1] for s in range(S)], dtype=torch.int64)
    e = x[:, lab]                                                        # (Tb, S), gathered exactly
    skip = torch.zeros(S, dtype=torch.bool)
    for s in range(3, S, 2):
        skip[s] = targets[s >> 1] != targets[(s >> 1) - 1]
    neg = torch.full((S + 2,), -inf, dtype=dtype)
    v = neg[:S].clone()
    v[0] = e[0, 0]
    if S > 1:
        v[1] = e[0, 1]
    back = [None]
    tied = [None]
    for t in range(1, Tb):
        c0 = v
        c1 = _shift(v, 1, neg)
        c2 = torch.where(skip, _shift(v, 2, neg), neg[:S])
        k = torch.zeros(S, dtype=torch.int64)
        m = c0
        g = c1 > m
        m = torch.where(g, c1, m)
        k = torch.where(g, torch.ones_like(k), k)
        g = c2 > m
        m = torch.where(g, c2, m)
        k = torch.where(g, torch.full_like(k, 2), k)
        tied.append((((c0 == m).int() + (c1 == m).int() + (c2 == m).int()) >= 2) & (m > -inf))
        back.append(k)
        v = m + e[t]
    s = S - 1
    ties = 0
    if U > 0:
        if not bool(v[S - 1] > v[S - 2]):
            s = S - 2
        ties += int(bool(v[S - 1] == v[S - 2]) and bool(v[S - 1] > -inf))
    raw = float(v[s])
    if not raw > -inf:
        return Result(False, [], [-1] * U, [-1] * U, [0.0] * U, raw, -inf, 0)
    path = [s]
    for t in range(Tb - 1, 0, -1):
        ties += int(tied[t][s])
        s -= int(back[t][s])
        path.append(s)
    path.reverse()
    lse = torch.logsumexp(x, dim=-1)
    begin, end, logp = [-1] * U, [-1] * U, []
    for t, s in enumerate(path):
        if s & 1:
            if begin[s >> 1] < 0:
                begin[s >> 1] = t
            end[s >> 1] = t + 1
    for u in range(U):
        acc = torch.zeros((), dtype=dtype)
        for t in range(begin[u], end[u]):                                # in frame order, in the dtype
            acc = acc + (e[t, 2 * u + 1] - lse[t])
        logp.append(float(acc))
    score = float(v[path[-1]] - lse.sum())
    return Result(True, path, begin, end, logp, raw, score, ties)


def ctc_log_likelihood(x, targets, blank=0):
    """log P(targets | x) summed over all alignments: the CTC forward in float64 (x: (Tb, V) any dtype)."""
    lp = torch.log_softmax(x.double(), dim=-1)
    Tb = lp.shape[0]
    U = len(targets)
    S = 2 * U + 1
    if Tb == 0:
        return 0.0 if U == 0 else -math.inf
    lab = [blank if s % 2 == 0 else targets[s >> 1] for s in range(S)]
    e = lp[:, torch.tensor(lab, dtype=torch.int64)]
    skip = torch.zeros(S, dtype=torch.bool)
    for s in range(3, S, 2):
        skip[s] = targets[s >> 1] != targets[(s >> 1) - 1]
    neg = torch.full((S + 2,), -math.inf, dtype=torch.float64)
    a = neg[:S].clone()
    a[0] = e[0, 0]
    if S > 1:
        a[1] = e[0, 1]
    for t in range(1, Tb):
        c = torch.stack([a, _shift(a, 1, neg), torch.where(skip, _shift(a, 2, neg), neg[:S])])
        a = torch.logsumexp(c, dim=0) + e[t]
        a = torch.where(torch.isnan(a), neg[:S], a)                      # logsumexp of three -inf
    return float(torch.logsumexp(a[-2:], dim=0)) if S > 1 else float(a[0])


def collapse(path, targets, blank=0):
    """The per-frame labels of a path of lattice states, CTC-collapsed: equal neighbours merged, then
    blanks dropped."""
    out, prev = [], None
    for s in path:
        c = targets[s >> 1] if s & 1 else blank
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out
