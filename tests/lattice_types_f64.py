"""k2.rnnt_loss_pruned's rnnt_type ("regular" / "modified" / "constrained") and delay_penalty restated
in plain torch with autograd.

Test infrastructure (not a test file): the float64 yardstick for the typed kernels of csrc/rnnt.hip
(mi_mod_*_kernel, the TYPE instantiations of pruned_* / lattice_*), pinned by brute-force path
enumeration in tests/test_lattice_types_f64.py before any kernel is compared with it.  Nothing here
is shared with the kernels, with oracle/ or with tests/lattice_f64.py: the modified recursion walks
the frames with torch ops, the regular one the anti-diagonals, every gradient is autograd's.  Every
function takes its dtype from its floating inputs (float64 is the yardstick; the same code in fp32
measures what fp32 costs the restatement).

Semantics (k2's rnnt_loss.py / mutual_information.py), with lp = log_softmax(logits[b,t,i,:]) and
s = ranges[b,t,0] + i:
  py[b,s,t] = lp[blank], (B,S+1,T), -inf outside the band -- all types
  regular:      px[b,s,t] = lp[symbols[b,s]], (B,S,T+1), column T and column T_b = -inf
  modified:     the same entries, (B,S,T), no boundary fix
  constrained:  modified, then px[b,s,t] += py[b,s+1,t]  (-inf where row s+1 is outside the band)
  delay_penalty > 0: px[b,s,t] += delay_penalty * ((T_b - 1) / 2 - t), a constant
  regular recursion:   p[s,t] = logadd(p[s-1,t] + px[s-1,t], p[s,t-1] + py[s,t-1])
  modified recursion:  p[s,t] = logadd(p[s-1,t-1] + px[s-1,t-1], p[s,t-1] + py[s,t-1])
                       (k2 selects it by px.shape[2] == T; "constrained" uses it too)
  p[0,0] = 0, s <= S_b, t <= T_b; the score is p[S_b,T_b], the loss its negative; an utterance
  without a path scores -inf (loss +inf) and has zero gradients.
"""
import torch

NEG_INF = float("-inf")
TYPES = ("regular", "modified", "constrained")


def make_boundary(target_lengths, frame_lengths):
    tl = torch.as_tensor(target_lengths, dtype=torch.int64)
    el = torch.as_tensor(frame_lengths, dtype=torch.int64)
    b = torch.zeros((tl.shape[0], 4), dtype=torch.int64)
    b[:, 2] = tl
    b[:, 3] = el
    return b


def band_ranges(tl, el, S, T, R):
    """A diagonal band that a one-symbol-per-frame path can follow:
    s0(t) = min(max(0, min(t,T_b) * S_b // max(T_b,1) - (R-1)//2), S+1-R)."""
    tl = torch.as_tensor(tl, dtype=torch.int64).reshape(-1, 1)
    el = torch.as_tensor(el, dtype=torch.int64).reshape(-1, 1)
    t = torch.arange(T).reshape(1, T)
    s0 = torch.minimum(t, el) * tl // el.clamp(min=1) - (R - 1) // 2
    s0 = s0.clamp(min=0).clamp(max=S + 1 - R)
    return (s0.unsqueeze(2) + torch.arange(R).reshape(1, 1, R)).contiguous()


def _logadd(a, b):
    """logaddexp that is -inf, with zero gradient, where both operands are -inf."""
    ok = torch.isfinite(a) | torch.isfinite(b)
    zero = torch.zeros((), dtype=a.dtype)
    out = torch.logaddexp(torch.where(ok, a, zero), torch.where(ok, b, zero))
    return torch.where(ok, out, torch.full((), NEG_INF, dtype=a.dtype))


def modified_scores(px, py, boundary):
    """px (B,S,T), py (B,S+1,T) -> p[S_b,T_b] (B,): one step per frame, all (b, s) at once."""
    B, S, T = px.shape
    dt = px.dtype
    assert py.shape == (B, S + 1, T) and py.dtype == dt
    Sb = boundary[:, 2].reshape(B, 1)
    Tb = boundary[:, 3].reshape(B)
    ninf = torch.full((), NEG_INF, dtype=dt)
    p = torch.where((torch.arange(S + 1) == 0).reshape(1, S + 1), torch.zeros((), dtype=dt), ninf)
    p = p.expand(B, S + 1)
    score = torch.where(Tb == 0, torch.gather(p, 1, Sb).reshape(B), ninf)
    pad = torch.full((B, 1), NEG_INF, dtype=dt)
    ends = set(Tb.tolist())
    for t in range(1, T + 1):
        sym = torch.cat((pad, p[:, :-1] + px[:, :, t - 1]), dim=1)      # from (s-1, t-1)
        p = _logadd(sym, p + py[:, :, t - 1])                           # from (s, t-1)
        if t in ends:
            score = torch.where(Tb == t, torch.gather(p, 1, Sb).reshape(B), score)
    return score


def regular_scores(px, py, boundary):
    """px (B,S,T+1), py (B,S+1,T) -> p[S_b,T_b] (B,): one step per anti-diagonal d = s + t."""
    B, S, T1 = px.shape
    T = T1 - 1
    dt = px.dtype
    assert py.shape == (B, S + 1, T) and py.dtype == dt
    Sb = boundary[:, 2].reshape(B, 1)
    Tb = boundary[:, 3].reshape(B, 1)
    ninf = torch.full((), NEG_INF, dtype=dt)
    below = torch.cat((torch.full((B, 1, T + 1), NEG_INF, dtype=dt), px), dim=1)   # px[s-1,t]
    left = torch.cat((torch.full((B, S + 1, 1), NEG_INF, dtype=dt), py), dim=2)    # py[s,t-1]
    D = S + T
    s_idx = torch.arange(S + 1).reshape(1, S + 1, 1)
    t_of = torch.arange(D + 1).reshape(1, 1, D + 1) - s_idx
    inside = (t_of >= 0) & (t_of <= Tb.reshape(B, 1, 1)) & (s_idx <= Sb.reshape(B, 1, 1))
    gidx = t_of.clamp(0, T).expand(B, S + 1, D + 1)
    XD = torch.where(inside, torch.gather(below, 2, gidx), ninf).unbind(2)
    YD = torch.where(inside, torch.gather(left, 2, gidx), ninf).unbind(2)
    p = torch.where((torch.arange(S + 1) == 0).reshape(1, S + 1), torch.zeros((), dtype=dt), ninf)
    p = p.expand(B, S + 1)
    final_d = (Sb + Tb).reshape(B)
    score = torch.where(final_d == 0, torch.gather(p, 1, Sb).reshape(B), ninf)
    ends = set(final_d.tolist())
    pad = torch.full((B, 1), NEG_INF, dtype=dt)
    for d in range(1, D + 1):
        p = _logadd(torch.cat((pad, p[:, :-1]), dim=1) + XD[d], p + YD[d])
        if d in ends:
            score = torch.where(final_d == d, torch.gather(p, 1, Sb).reshape(B), score)
    return score


def scores(px, py, boundary):
    """The topology follows from the shapes, as in k2."""
    return modified_scores(px, py, boundary) if px.shape[2] == py.shape[2] \
        else regular_scores(px, py, boundary)


def mutual_information(px, py, boundary, dtype=torch.float64):
    """(scores, d scores.sum() / d px, d scores.sum() / d py) -- the occupation counts."""
    px = px.detach().to(dtype).requires_grad_(True)
    py = py.detach().to(dtype).requires_grad_(True)
    sc = scores(px, py, boundary)
    if not sc.requires_grad:                      # S = 0 and T_b = 0 everywhere: nothing depends
        return sc.detach(), torch.zeros_like(px), torch.zeros_like(py)
    gx, gy = torch.autograd.grad(sc.sum(), (px, py), allow_unused=True)
    gx = torch.zeros_like(px) if gx is None else gx
    gy = torch.zeros_like(py) if gy is None else gy
    return sc.detach(), gx, gy


def typed_pxpy(logits, symbols, ranges, boundary, blank=0, rnnt_type="regular", delay_penalty=0.0):
    """logits (B,T,R,C) -> (px, py) of the given type; ranges None = the full lattice."""
    assert rnnt_type in TYPES and delay_penalty >= 0.0
    B, T, R, C = logits.shape
    S = symbols.shape[1]
    dt = logits.dtype
    if ranges is None:
        assert R == S + 1
        ranges = torch.arange(S + 1).reshape(1, 1, S + 1).expand(B, T, S + 1)
    lp = torch.log_softmax(logits, dim=3)
    sym_ext = torch.cat((symbols, torch.full((B, 1), blank, dtype=symbols.dtype)), dim=1)
    row_sym = torch.gather(sym_ext.unsqueeze(1).expand(B, T, S + 1), 2, ranges)
    empty = torch.full((B, T, S + 1), NEG_INF, dtype=dt)
    px = empty.scatter(2, ranges, torch.gather(lp, 3, row_sym.unsqueeze(3)).squeeze(3))
    px = px[:, :, :S].transpose(1, 2)                                       # (B,S,T)
    py = empty.scatter(2, ranges, lp[:, :, :, blank]).transpose(1, 2)       # (B,S+1,T)
    Tb = boundary[:, 3].reshape(B, 1, 1)
    if rnnt_type == "regular":
        px = torch.cat((px, torch.full((B, S, 1), NEG_INF, dtype=dt)), dim=2)
        at_end = torch.arange(T + 1).reshape(1, 1, T + 1) == Tb
        px = torch.where(at_end, torch.full((), NEG_INF, dtype=dt), px)
    elif rnnt_type == "constrained":
        px = px + py[:, 1:, :]
    if delay_penalty > 0.0:
        t = torch.arange(px.shape[2]).reshape(1, 1, -1)
        px = px + (delay_penalty * ((Tb - 1).to(dt) / 2 - t)).to(dt)
    return px, py


def joiner_logits(am, lm, ranges, activation="relu"):
    """act(am[b,t] + lm[b, ranges[b,t,0] + i]) -> (B,T,R,C); ranges None = every row."""
    B, T, C = am.shape
    if ranges is None:
        ranges = torch.arange(lm.shape[1]).reshape(1, 1, -1).expand(B, T, lm.shape[1])
    R = ranges.shape[2]
    act = {"relu": torch.relu, "tanh": torch.tanh}[activation]
    rows = torch.gather(lm.unsqueeze(1).expand(B, T, lm.shape[1], C), 2,
                        ranges.reshape(B, T, R, 1).expand(B, T, R, C))
    return act(am.unsqueeze(2) + rows)


def lattice_neg(logits, ranges, symbols, boundary, blank=0, rnnt_type="regular", delay_penalty=0.0):
    """Materialised logits -> per-utterance negative score (B,)."""
    px, py = typed_pxpy(logits, symbols, ranges, boundary, blank, rnnt_type, delay_penalty)
    return -scores(px, py, boundary)


def pruned_neg(am, lm, ranges, symbols, boundary, blank=0, activation="relu", rnnt_type="regular",
               delay_penalty=0.0):
    """Fused-joiner form -> per-utterance negative score (B,)."""
    return lattice_neg(joiner_logits(am, lm, ranges, activation), ranges, symbols, boundary, blank,
                       rnnt_type, delay_penalty)
