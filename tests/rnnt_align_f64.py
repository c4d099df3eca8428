"""The statement of RNN-T forced alignment (include/s2t_mi355.h, above s2t_rnnt_align) restated in plain
Python / torch over ONE utterance, in the dtype of its input.  Test infrastructure (not a test file).

    align(px, py, Sb, Tb, rnnt_type) -> Result

px (S, T+1) on the regular lattice and (S, T) on the two others, py (S+1, T): the utterance's own slices
of the operands of the mutual-information recursion; only the cells with s <= Sb, t <= Tb are touched.
The recursion is the statement's, an anti-diagonal (regular) or a frame (modified / constrained) at a time
over all rows at once: every candidate is one addition in the dtype, every value the maximum of the two,
the backpointer "symbol" exactly when cu > cl.  In float32 that is the arithmetic of csrc/rnnt_align.hip,
so every output of the float32 run is the kernel's bit for bit.
"""
import collections
import itertools
import math

import torch

Result = collections.namedtuple("Result", ["ok", "tok_frame", "tok_logp", "score", "ties"])
# ok: bool; tok_frame: list of Sb frames ([-1] * Sb when infeasible); tok_logp: list of Sb Python floats
# (the dtype's values; 0.0 when infeasible); score: Python float; ties: decisions ON THE BEST PATH in
# which the two candidates were equal and above -inf.


def align(px, py, Sb, Tb, rnnt_type="regular"):
    dtype = px.dtype
    inf = math.inf
    reg = rnnt_type == "regular"
    px = px[:Sb, :Tb + 1] if reg else px[:Sb, :Tb]         # nothing outside the utterance's cells exists
    py = py[:Sb + 1, :Tb]
    # The operands of step i laid out per row: regular walks the anti-diagonals d = i (cell (s, d - s)),
    # the others the frames t = i; X[s][i] is the symbol arc INTO the cell, Y[s][i] the blank arc into it,
    # -inf where the cell or the arc does not exist.  A gather: the values are the inputs' own.
    steps = Sb + Tb if reg else Tb
    s = torch.arange(Sb + 1).unsqueeze(1)
    i = torch.arange(steps + 1).unsqueeze(0)
    t = i - s if reg else i + 0 * s
    cell = (t >= 0) & (t <= Tb)
    neg = torch.full((Sb + 1, steps + 1), -inf, dtype=dtype)
    X, Y = neg.clone(), neg.clone()
    hasx = cell & (s >= 1) & ((t >= 0) if reg else (t >= 1))
    hasy = cell & (t >= 1)
    if Sb and px.shape[1]:
        tx = (t if reg else t - 1).clamp(0, px.shape[1] - 1)
        X = torch.where(hasx, px[(s - 1).clamp(min=0).expand_as(tx), tx], neg)
    if Tb:
        Y = torch.where(hasy, py[s.expand_as(t), (t - 1).clamp(0, Tb - 1)], neg)
    v = torch.full((Sb + 1,), -inf, dtype=dtype)
    v[0] = 0.0
    low = torch.full((1,), -inf, dtype=dtype)
    sym, tie = [None], [None]
    for k in range(1, steps + 1):
        cl = v + Y[:, k]                                   # one addition each
        cu = torch.cat([low, v[:-1]]) + X[:, k]
        g = cu > cl                                        # "symbol" exactly when cu > cl
        v = torch.where(g, cu, cl)
        sym.append(g)
        tie.append((cu == cl) & (cl > -inf))
    score = float(v[Sb])
    if not score > -inf:
        return Result(False, [-1] * Sb, [0.0] * Sb, -inf, 0)
    sym = torch.stack(sym[1:]).tolist() if steps else []
    tie = torch.stack(tie[1:]).tolist() if steps else []
    frames, logp, ties = [-1] * Sb, [0.0] * Sb, 0
    s, t = Sb, Tb
    while s > 0 or t > 0:
        k = s + t if reg else t
        ties += int(tie[k - 1][s])
        if sym[k - 1][s]:
            f = t if reg else t - 1
            frames[s - 1] = f
            logp[s - 1] = float(px[s - 1, f])
            s, t = (s - 1, t) if reg else (s - 1, t - 1)
        else:
            t -= 1
    return Result(True, frames, logp, score, ties)


def path_score(px, py, Sb, Tb, frames, rnnt_type="regular"):
    """The float64 score of the path that emits symbol s at frames[s] and ends at (Sb, Tb): its symbol
    arcs and every blank arc between them, summed in float64 (-inf for a path the lattice does not have)."""
    reg = rnnt_type == "regular"
    px, py = px.double(), py.double()
    total, t = 0.0, 0
    for s in range(Sb):
        f = frames[s]
        if f < t or f > (Tb if reg else Tb - 1):
            return -math.inf
        total += float(py[s, t:f].sum()) + float(px[s, f])
        t = f if reg else f + 1
    return total + float(py[Sb, t:Tb].sum())


def enumerate_best(px, py, Sb, Tb, rnnt_type="regular"):
    """The best float64 score over ALL paths of a small lattice, each listed explicitly as the frames of
    its Sb symbols (non-decreasing for regular, strictly increasing otherwise)."""
    reg = rnnt_type == "regular"
    if reg:
        combos = itertools.combinations_with_replacement(range(Tb + 1), Sb)
    else:
        combos = itertools.combinations(range(Tb), Sb)
    best = -math.inf
    for frames in combos:
        best = max(best, path_score(px, py, Sb, Tb, list(frames), rnnt_type))
    return best
