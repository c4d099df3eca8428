"""RNN-T lattice losses restated in plain torch float64 with autograd.

Test infrastructure (not a test file): the float64 yardstick for csrc/rnnt.hip, pinned to
oracle/k2_rnnt.py and to brute-force path enumeration by tests/test_lattice_f64.py before any
kernel is compared with it.  Nothing here is shared with the kernels or with the oracle: the
recursion is written over anti-diagonals with torch ops and every gradient is autograd's.

Conventions (k2's): am (B,T,C), lm (B,S+1,C), symbols (B,S) int64, boundary (B,4) =
(0, 0, S_b, T_b), px (B,S,T+1) with column T = -inf, py (B,S+1,T).  Every loss function returns the
per-utterance NEGATIVE score (B,), float64; the caller applies its own weights and reduction.

What is dropped from k2.get_rnnt_logprobs_smoothed, and why that is invisible in float64:
  * `tiny` (the smallest normal number, added to the max-shifted normaliser product before the
    log).  The product is sum_c exp(lm_c - max lm) exp(am_c - max am) >= exp(-(spread of am))
    taken at lm's arg-max class; for the seeded N(0, <=3) inputs of these tests that is above
    1e-20, so `tiny` (1.2e-38 in fp32, 2.2e-308 in float64) changes it by less than 1e-18
    relative -- far below float64's 1.1e-16.
  * the lm-only / am-only smoothing terms.  With both scales 0 (the only setting the model uses)
    k2 multiplies them by 1e-20 and the combined term by exactly 1.0: they add at most
    1e-20 * |log-prob| <= 1e-17 to log-probs of magnitude >= 1e-2, again below float64 resolution
    (and 9 orders below fp32's).
"""
import torch

NEG_INF = float("-inf")
F64 = torch.float64


def make_boundary(target_lengths, frame_lengths):
    tl = torch.as_tensor(target_lengths, dtype=torch.int64)
    el = torch.as_tensor(frame_lengths, dtype=torch.int64)
    b = torch.zeros((tl.shape[0], 4), dtype=torch.int64)
    b[:, 2] = tl
    b[:, 3] = el
    return b


def _safe_logaddexp(a, b):
    """logaddexp that is -inf, with zero gradient, where both operands are -inf."""
    ok = torch.isfinite(a) | torch.isfinite(b)
    zero = torch.zeros((), dtype=a.dtype)
    out = torch.logaddexp(torch.where(ok, a, zero), torch.where(ok, b, zero))
    return torch.where(ok, out, torch.full((), NEG_INF, dtype=a.dtype))


def lattice_scores(px, py, boundary):
    """p[s,t] = logaddexp(p[s-1,t] + px[s-1,t], p[s,t-1] + py[s,t-1]), p[0,0] = 0, restricted to
    s <= S_b, t <= T_b; returns p[S_b, T_b] per utterance (B,).  One step per anti-diagonal
    d = s + t, all (b, s) of a diagonal at once."""
    B, S, T1 = px.shape
    T = T1 - 1
    assert py.shape == (B, S + 1, T) and px.dtype == F64 and py.dtype == F64
    Sb = boundary[:, 2].reshape(B, 1)
    Tb = boundary[:, 3].reshape(B, 1)
    ninf = torch.full((), NEG_INF, dtype=F64)
    # X[b,s,t] = px[b,s-1,t] (arc entering (s,t) from below), Y[b,s,t] = py[b,s,t-1] (from the left)
    X = torch.cat((torch.full((B, 1, T + 1), NEG_INF, dtype=F64), px), dim=1)
    Y = torch.cat((torch.full((B, S + 1, 1), NEG_INF, dtype=F64), py), dim=2)
    D = S + T
    s_idx = torch.arange(S + 1).reshape(1, S + 1, 1)
    t_of = torch.arange(D + 1).reshape(1, 1, D + 1) - s_idx               # (1,S+1,D+1)
    inside = (t_of >= 0) & (t_of <= Tb.reshape(B, 1, 1)) & (s_idx <= Sb.reshape(B, 1, 1))
    gidx = t_of.clamp(0, T).expand(B, S + 1, D + 1)
    # one (B,S+1) slab per diagonal; unbind, so that autograd stacks the slabs' gradients once
    XD = torch.where(inside, torch.gather(X, 2, gidx), ninf).unbind(2)
    YD = torch.where(inside, torch.gather(Y, 2, gidx), ninf).unbind(2)
    p = torch.full((B, S + 1), NEG_INF, dtype=F64)
    p = torch.where((torch.arange(S + 1) == 0).reshape(1, S + 1), torch.zeros((), dtype=F64), p)
    final_d = (Sb + Tb).reshape(B)
    ends = set(final_d.tolist())
    score = torch.gather(p, 1, Sb).reshape(B)                             # d = 0 (S_b = T_b = 0)
    score = torch.where(final_d == 0, score, ninf)
    for d in range(1, D + 1):
        below = torch.cat((torch.full((B, 1), NEG_INF, dtype=F64), p[:, :-1]), dim=1)
        p = _safe_logaddexp(below + XD[d], p + YD[d])
        if d in ends:
            score = torch.where(final_d == d, torch.gather(p, 1, Sb).reshape(B), score)
    return score


def mutual_information(px, py, boundary):
    """(scores, d scores.sum() / d px, d scores.sum() / d py) -- the occupation counts."""
    px = px.detach().to(F64).requires_grad_(True)
    py = py.detach().to(F64).requires_grad_(True)
    sc = lattice_scores(px, py, boundary)
    gx, gy = torch.autograd.grad(sc.sum(), (px, py))
    return sc.detach(), gx, gy


def _fix_for_boundary(px, boundary):
    """px[b, :, T_b] = -inf: no symbol may be emitted after the last frame."""
    B, S, T1 = px.shape
    at_end = torch.arange(T1).reshape(1, 1, T1) == boundary[:, 3].reshape(B, 1, 1)
    return torch.where(at_end, torch.full((), NEG_INF, dtype=px.dtype), px)


def simple_pxpy(am, lm, symbols, boundary, blank=0):
    """log_softmax_c(am[b,t,c] + lm[b,s,c]) at the symbol (px) and at the blank (py); the
    normaliser is a max-shifted matmul, so no (B,S+1,T,C) tensor exists."""
    assert am.dtype == F64 and lm.dtype == F64
    B, T, C = am.shape
    S = lm.shape[1] - 1
    am_max = am.max(dim=2, keepdim=True)[0].detach()
    lm_max = lm.max(dim=2, keepdim=True)[0].detach()
    prod = torch.matmul((lm - lm_max).exp(), (am - am_max).exp().transpose(1, 2))   # (B,S+1,T)
    norm = prod.log() + lm_max + am_max.transpose(1, 2)
    am_sym = torch.gather(am, 2, symbols.reshape(B, 1, S).expand(B, T, S)).transpose(1, 2)
    lm_sym = torch.gather(lm[:, :S], 2, symbols.reshape(B, S, 1))
    px = am_sym + lm_sym - norm[:, :S]
    px = torch.cat((px, torch.full((B, S, 1), NEG_INF, dtype=F64)), dim=2)
    py = am[:, :, blank].reshape(B, 1, T) + lm[:, :, blank].reshape(B, S + 1, 1) - norm
    return _fix_for_boundary(px, boundary), py


def simple_neg(am, lm, symbols, boundary, blank=0):
    px, py = simple_pxpy(am, lm, symbols, boundary, blank)
    return -lattice_scores(px, py, boundary)


def pruned_logits(am, lm, ranges, activation="relu"):
    """act(am[b,t] + lm[b, ranges[b,t,0] + i]) -> (B,T,R,C)."""
    B, T, R = ranges.shape
    C = am.shape[2]
    act = {"relu": torch.relu, "tanh": torch.tanh}[activation]
    lm_p = torch.gather(lm.unsqueeze(1).expand(B, T, lm.shape[1], C), 2,
                        ranges.reshape(B, T, R, 1).expand(B, T, R, C))
    return act(am.unsqueeze(2) + lm_p)


def logits_pxpy(logits, symbols, ranges, boundary, blank=0):
    """k2.get_rnnt_logprobs_pruned: row i of frame t is lattice row s = ranges[b,t,i]; rows a frame
    does not hold are -inf.  ranges None = the full lattice (R = S+1, row i is s = i)."""
    assert logits.dtype == F64
    B, T, R, C = logits.shape
    S = symbols.shape[1]
    if ranges is None:
        assert R == S + 1
        ranges = torch.arange(S + 1).reshape(1, 1, S + 1).expand(B, T, S + 1)
    lp = torch.log_softmax(logits, dim=3)
    sym_ext = torch.cat((symbols, torch.full((B, 1), blank, dtype=symbols.dtype)), dim=1)
    row_sym = torch.gather(sym_ext.unsqueeze(1).expand(B, T, S + 1), 2, ranges)     # (B,T,R)
    vx = torch.gather(lp, 3, row_sym.unsqueeze(3)).squeeze(3)
    vy = lp[:, :, :, blank]
    empty = torch.full((B, T, S + 1), NEG_INF, dtype=F64)
    px = empty.scatter(2, ranges, vx)[:, :, :S].transpose(1, 2)
    py = empty.scatter(2, ranges, vy).transpose(1, 2)
    px = torch.cat((px, torch.full((B, S, 1), NEG_INF, dtype=F64)), dim=2)
    return _fix_for_boundary(px, boundary), py


def lattice_neg(logits, ranges, symbols, boundary, blank=0):
    """Materialised lattice (pruned with `ranges`, or full with ranges None)."""
    px, py = logits_pxpy(logits, symbols, ranges, boundary, blank)
    return -lattice_scores(px, py, boundary)


def pruned_neg(am, lm, ranges, symbols, boundary, blank=0, activation="relu"):
    return lattice_neg(pruned_logits(am, lm, ranges, activation), ranges, symbols, boundary, blank)
