"""k2.rnnt_loss_smoothed with non-zero lm_only_scale / am_only_scale, restated in torch float64.

Test infrastructure (not a test file): the float64 yardstick for csrc/rnnt_smooth.hip, pinned to
oracle/k2_rnnt.py by tests/test_lattice_smoothed_f64.py before any kernel is compared with it.
Nothing here is shared with the kernels or with the oracle: the three log-prob terms are written
with log_softmax / logsumexp, the recursion is lattice_f64.lattice_scores and every gradient is
autograd's.

With lam = lm_only_scale, mu = am_only_scale, alpha = 1 - lam - mu, y the arc's symbol (px) or the
blank (py):

    joint   = log_softmax_c(am[b,t,:] + lm[b,s,:])[y]          (lattice_f64.simple_pxpy)
    lm_only = log_softmax_c(lm[b,s,:])[y]
    am_only = log_softmax_c(am[b,t,:] + log u)[y],   u = mean of softmax(lm) over ALL B (S+1) rows
    px / py = alpha joint + lam lm_only + mu am_only

u is taken over the padded tensor, rows s > S_b included (k2: torch.mean(..., dim=(0,1))), so with
mu != 0 the utterances of a batch are coupled and this cannot be evaluated an utterance at a time.
A scale that is exactly 0 drops its term: k2 multiplies it by 1e-20 instead, the argument of
lattice_f64's docstring.  k2's `tiny` added to u (1.2e-38) is dropped as well: u >= 1/(B (S+1) C)
times e^-(spread of lm) for the seeded inputs of these tests, more than 1e-15.
"""
import torch

import lattice_f64 as L

F64 = L.F64


def unigram(lm):
    """(C,) mean over every (b, s) row of softmax(lm), padded rows included."""
    return torch.softmax(lm, dim=2).mean(dim=(0, 1))


def smoothed_pxpy(am, lm, symbols, boundary, blank=0, lm_only_scale=0.0, am_only_scale=0.0):
    assert am.dtype == F64 and lm.dtype == F64
    lam, mu = float(lm_only_scale), float(am_only_scale)
    B, T, C = am.shape
    S = lm.shape[1] - 1
    px, py = L.simple_pxpy(am, lm, symbols, boundary, blank)
    px, py = (1.0 - lam - mu) * px, (1.0 - lam - mu) * py
    pad = torch.zeros((B, S, 1), dtype=F64)            # column T of px is -inf already
    if lam != 0.0:
        lp = torch.log_softmax(lm, dim=2)                                     # (B,S+1,C)
        x = torch.gather(lp[:, :S], 2, symbols.reshape(B, S, 1))              # (B,S,1)
        px = px + lam * torch.cat((x.expand(B, S, T), pad), dim=2)
        py = py + lam * lp[:, :, blank].reshape(B, S + 1, 1)
    if mu != 0.0:
        ap = torch.log_softmax(am + unigram(lm).log().reshape(1, 1, C), dim=2)   # (B,T,C)
        x = torch.gather(ap, 2, symbols.reshape(B, 1, S).expand(B, T, S)).transpose(1, 2)
        px = px + mu * torch.cat((x, pad), dim=2)
        py = py + mu * ap[:, :, blank].reshape(B, 1, T)
    return L._fix_for_boundary(px, boundary), py


def smoothed_neg(am, lm, symbols, boundary, blank=0, lm_only_scale=0.0, am_only_scale=0.0):
    """Per-utterance negative score (B,), float64."""
    px, py = smoothed_pxpy(am, lm, symbols, boundary, blank, lm_only_scale, am_only_scale)
    return -L.lattice_scores(px, py, boundary)


def occupation(am, lm, symbols, boundary, blank=0, lm_only_scale=0.0, am_only_scale=0.0):
    """(px_grad, py_grad): d scores.sum() / d px, py -- what rnnt_loss_smoothed(return_grad=True)
    hands to get_rnnt_prune_ranges."""
    with torch.no_grad():
        px, py = smoothed_pxpy(am.detach(), lm.detach(), symbols, boundary, blank, lm_only_scale,
                               am_only_scale)
    _, gx, gy = L.mutual_information(px, py, boundary)
    return gx, gy
