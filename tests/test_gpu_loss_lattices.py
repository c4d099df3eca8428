"""GPU: csrc/ctc.hip and csrc/rnnt.hip against float64 at every dispatch edge.

Every kernel is reached through speech2text_amd.kernels and compared with float64: oracle.ctc for
CTC, tests/lattice_f64.py (pinned by tests/test_lattice_f64.py) for RNN-T.  Inputs are seeded.

Bounds.  Small cases use the bounds tests/test_gpu_frontend_losses.py already holds for the same
quantity: loss rtol 2e-5 (CTC) / 1e-4 (RNN-T); gradients atol 3e-5, rtol 2e-3 where the weights sum
to about one (a mean), atol 3e-3 for CTC with unit weights (a sum); raw mutual-information
gradients atol 2e-4.  Large cases (CTC at U >= 255, the C3 bench geometry, lattices of 64 rows and
more) take 4x what fp32 costs
the REFERENCE on the same inputs (tests/loss_cases.py FP32_COST, measured and asserted on the CPU by
tests/test_lattice_f64.py), never tighter than the small-case bound; the factor covers a different
summation order over the classes and along the lattice and a different expf, no more:

  case        quantity            fp32 reference vs float64   bound used
  CTC U255    per-utt loss, rel   7.7e-7                      2e-5   (floor)
              d logits, abs       1.3e-3                      5.2e-3
  CTC U256    per-utt loss, rel   2.0e-7                      2e-5   (floor)
              d logits, abs       6.9e-4                      3e-3   (floor)
  CTC U511    per-utt loss, rel   7.6e-7                      2e-5   (floor)
              d logits, abs       2.3e-3                      9.2e-3
  CTC U512    per-utt loss, rel   3.3e-7                      2e-5   (floor)
              d logits, abs       1.3e-3                      5.2e-3
  CTC U1023   per-utt loss, rel   4.1e-7                      2e-5   (floor)
              d logits, abs       4.5e-3                      1.8e-2
  RNN-T C3    simple loss, rel    4.4e-7                      1e-4   (floor)
  (B=64)      pruned loss, rel    6.5e-7                      1e-4   (floor)
              d am, abs           7.0e-6                      3e-5   (floor)
              d lm, abs           8.1e-4                      3.24e-3
  rows 64     recursion px/py grad 2.6e-5 / 1.5e-5            2e-4   (floor)
  (S+1 rows,  simple d am / d lm  1.3e-4 / 1.7e-4             5.2e-4 / 6.8e-4
  T=20)
  rows 65     recursion px/py grad 2.3e-5 / 2.2e-5            2e-4   (floor)
              simple d am / d lm  1.3e-5 / 1.7e-5             5.2e-5 / 6.8e-5
  rows 128    recursion px/py grad 3.4e-5 / 2.1e-5            2e-4   (floor)
              simple d am / d lm  3.1e-4 / 1.5e-4             1.24e-3 / 6.0e-4
  rows 129    recursion px/py grad 5.9e-5 / 4.6e-5            2.36e-4 / 2e-4 (floor)
              simple d am / d lm  4.2e-4 / 1.5e-4             1.68e-3 / 6.0e-4
  rows 1024   recursion px/py grad 1.5e-3 / 6.8e-4            6.0e-3 / 2.72e-3
              simple d am / d lm  5.4e-2 / 1.3e-3             2.16e-1 / 5.2e-3
  (at every row count the scores and simple losses deviate by < 6e-7 rel: floors 2e-5 and 1e-4)
(the CTC reference is torch.nn.functional.ctc_loss on an fp32 log_softmax, the RNN-T reference is
oracle.k2_rnnt in fp32; all gradient bounds also carry rtol 2e-3).  The bench-geometry case runs at
the bench's own B = 64: its float64 side takes a few seconds on 16 CPUs.

No element is left out of a comparison; exact-zero and bit-exact assertions are conditions.
"""
import functools

import numpy as np
import pytest
import torch

import lattice_f64 as L
import loss_cases as LC
from loss_cases import G_ATOL, G_RTOL, _assert_grad, _kern, _np
from oracle import ctc as octc
from oracle import k2_rnnt as K

pytestmark = pytest.mark.gpu

CTC_SUM_ATOL = 3e-3                    # CTC gradients under unit weights
CTC_RTOL, RNNT_RTOL = 2e-5, 1e-4       # losses
BIG = 3.0e4                            # "large finite" filler of padded frames


# ================================================================== CTC
def _ctc_run(dev, logits, tg, il, tl, blank, reduction, zero_infinity=True, w=None):
    """(loss as float64 numpy, d logits numpy); reduction 'none' is contracted with w."""
    k = _kern()
    lg = torch.as_tensor(logits).to(dev).requires_grad_(True)
    as_dev = lambda a: a.to(dev) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).to(dev)
    out = k.ctc_loss(lg, as_dev(tg), as_dev(il), as_dev(tl), blank=blank, reduction=reduction,
                     zero_infinity=zero_infinity)
    if reduction == "none":
        assert out.shape == (lg.shape[0],)
        (out * torch.as_tensor(w, dtype=torch.float32, device=dev)).sum().backward()
    else:
        out.backward()
    return _np(out), lg.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ctc_edge_reference(name):
    logits, tg, il, tl, blank = LC.ctc_case(name)
    _, grad, per = octc.ctc_loss(logits, tg, il, tl, blank=blank, reduction="sum")
    return grad, per


@pytest.mark.parametrize("name", list(LC.CTC_EDGES))
def test_ctc_label_width_at_every_dispatch_edge(dev, name):
    """2U+1 on both sides of 256 / 512 / 1024 and at the limit: ctc_alpha_beta_kernel<2> (U127),
    <4> (U128, U255), <8> (U256, U511), <16> (U512, U1023)."""
    logits, tg, il, tl, blank = LC.ctc_case(name)
    ref_grad, ref_per = _ctc_edge_reference(name)
    per, grad = _ctc_run(dev, logits, tg, il, tl, blank, "none", w=np.ones(len(il)))
    cost = LC.FP32_COST.get(name)
    l_rtol = LC.bound(cost["loss_rel"], CTC_RTOL) if cost else CTC_RTOL
    g_atol = LC.bound(cost["grad_abs"], CTC_SUM_ATOL) if cost else CTC_SUM_ATOL
    print(f"{name}: loss rel {np.max(np.abs(per - ref_per) / ref_per):.3e} (bound {l_rtol:.1e}) "
          f"grad abs {np.abs(grad - ref_grad).max():.3e} (bound {g_atol:.1e})")
    np.testing.assert_allclose(per, ref_per, rtol=l_rtol)
    np.testing.assert_allclose(grad, ref_grad, atol=g_atol, rtol=G_RTOL)


def test_ctc_label_width_above_the_limit_is_refused(dev):
    """U = 1024: refused on the host, before anything is launched."""
    k = _kern()
    lg = torch.zeros(1, 1100, 4, device=dev)
    tg = torch.ones(1, 1024, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="1024"):
        k.ctc_loss(lg, tg, torch.tensor([1100], device=dev), torch.tensor([3], device=dev))


def _ctc_small(seed, V, blank, B=5, T=60, U=12):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
    tg = rng.integers(0, V - 1, size=(B, U))
    tg = tg + (tg >= blank)
    tl = np.array([U, 0, 1, 7, 10])[:B]
    il = np.array([T, 33, 1, 2 * 7 + 3, 41])[:B]          # >= 2 tl - 1: feasible even if V = 2
    return logits, tg.astype(np.int64), il.astype(np.int64), tl.astype(np.int64)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("V", [2, 63, 64, 65, 5003])
def test_ctc_vocabulary_blank_and_reduction(dev, V, where):
    blank = {"first": 0, "middle": V // 2, "last": V - 1}[where]
    logits, tg, il, tl = _ctc_small(V, V, blank)
    assert (tg != blank).all()
    w = np.array([1.5, 0.0, -2.0, 0.7, 1.0])
    _, g_sum, per = octc.ctc_loss(logits, tg, il, tl, blank=blank, reduction="sum")
    l_mean, g_mean, _ = octc.ctc_loss(logits, tg, il, tl, blank=blank, reduction="mean")
    loss, grad = _ctc_run(dev, logits, tg, il, tl, blank, "mean")
    np.testing.assert_allclose(loss, l_mean, rtol=CTC_RTOL)
    np.testing.assert_allclose(grad, g_mean, atol=G_ATOL, rtol=G_RTOL)
    loss, grad = _ctc_run(dev, logits, tg, il, tl, blank, "sum")
    np.testing.assert_allclose(loss, per.sum(), rtol=CTC_RTOL)
    np.testing.assert_allclose(grad, g_sum, atol=CTC_SUM_ATOL, rtol=G_RTOL)
    loss, grad = _ctc_run(dev, logits, tg, il, tl, blank, "none", w=w)
    np.testing.assert_allclose(loss, per, rtol=CTC_RTOL)
    np.testing.assert_allclose(grad, g_sum * w[:, None, None], atol=CTC_SUM_ATOL, rtol=G_RTOL)
    assert (grad[1] == 0).all()                             # the zero weight


@pytest.mark.parametrize("zero_infinity", [True, False])
def test_ctc_infeasible_utterances_inside_a_feasible_batch(dev, zero_infinity):
    V, blank = 17, 4
    logits, tg, il, tl = _ctc_small(77, V, blank)
    il[0] = tl[0] - 1                                       # fewer frames than labels
    tg[3, :7] = 9; il[3] = 2 * 7 - 2                        # 7 repeats need 13 frames, it has 12
    bad = np.array([True, False, False, True, False])
    _, rg, per = octc.ctc_loss(logits, tg, il, tl, blank=blank, reduction="sum",
                               zero_infinity=zero_infinity)
    w = np.array([0.5, 1.0, -1.5, 2.0, 0.25])
    loss, grad = _ctc_run(dev, logits, tg, il, tl, blank, "none", zero_infinity, w=w)
    if zero_infinity:
        assert (loss[bad] == 0).all()
    else:
        assert np.isposinf(loss[bad]).all()
    # csrc/ctc.hip documents an all-zero gradient for an infeasible utterance under EITHER flag
    # (nn.CTCLoss without zero_infinity would give NaN there): asserted as documented
    assert (grad[bad] == 0).all()
    np.testing.assert_allclose(loss[~bad], per[~bad], rtol=CTC_RTOL)
    np.testing.assert_allclose(grad[~bad], (rg * w[:, None, None])[~bad], atol=CTC_SUM_ATOL,
                               rtol=G_RTOL)
    if zero_infinity:
        l_mean, g_mean, _ = octc.ctc_loss(logits, tg, il, tl, blank=blank, reduction="mean")
        loss, grad = _ctc_run(dev, logits, tg, il, tl, blank, "mean")
        np.testing.assert_allclose(loss, l_mean, rtol=CTC_RTOL)
        np.testing.assert_allclose(grad, g_mean, atol=G_ATOL, rtol=G_RTOL)
        assert (grad[bad] == 0).all()


def test_ctc_padding_is_not_read(dev):
    """Targets past tgt_len hold the last real label (a read one past the end would clear a skip
    flag, not fault) and frames past in_len hold large values: same result as zero padding.  The
    labels of an utterance are distinct, so every class's occupancy is a single term and the
    gradient kernel's LDS sums have no order to differ in: the comparison is bit for bit."""
    V, blank, B, T, U = 19, 6, 4, 50, 10
    rng = np.random.default_rng(8)
    tl = np.array([U, 0, 4, 9]); il = np.array([T, 20, 31, 9 + 6])
    tg = np.stack([rng.permutation(np.setdiff1d(np.arange(V), [blank]))[:U] for _ in range(B)])
    logits = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
    tg0, tg1, lg0, lg1 = tg.copy(), tg.copy(), logits.copy(), logits.copy()
    for b in range(B):
        tg0[b, tl[b]:] = 0
        tg1[b, tl[b]:] = tg[b, tl[b] - 1] if tl[b] else 1
        lg0[b, il[b]:] = 0
        lg1[b, il[b]:] = BIG * np.sign(rng.standard_normal((T - il[b], V)))
    w = np.array([1.0, -0.5, 2.0, 0.75])
    p0, g0 = _ctc_run(dev, lg0, tg0, il, tl, blank, "none", w=w)
    p1, g1 = _ctc_run(dev, lg1, tg1, il, tl, blank, "none", w=w)
    assert np.array_equal(p0, p1)
    assert np.array_equal(g0, g1)
    for b in range(B):
        assert (g1[b, il[b]:] == 0).all()
    _, rg, per = octc.ctc_loss(lg0, tg0, il, tl, blank=blank, reduction="sum")
    np.testing.assert_allclose(p1, per, rtol=CTC_RTOL)
    np.testing.assert_allclose(g1, rg * w[:, None, None], atol=CTC_SUM_ATOL, rtol=G_RTOL)


def test_ctc_int32_and_non_contiguous_index_tensors(dev):
    V, blank = 23, 11
    logits, tg, il, tl = _ctc_small(5, V, blank)
    B, U = tg.shape
    wide = torch.full((B, 2 * U), 3, dtype=torch.int32)
    wide[:, ::2] = torch.from_numpy(tg).int()
    lens = torch.full((B, 4), 5, dtype=torch.int32)
    lens[:, 1] = torch.from_numpy(il).int(); lens[:, 2] = torch.from_numpy(tl).int()
    tg_nc, il_nc, tl_nc = wide.to(dev)[:, ::2], lens.to(dev)[:, 1], lens.to(dev)[:, 2]
    assert not tg_nc.is_contiguous() and not il_nc.is_contiguous() and not tl_nc.is_contiguous()
    l_mean, g_mean, _ = octc.ctc_loss(logits, tg, il, tl, blank=blank, reduction="mean")
    loss, grad = _ctc_run(dev, logits, tg_nc, il_nc, tl_nc, blank, "mean")
    ref_loss, _ = _ctc_run(dev, logits, tg, il, tl, blank, "mean")
    assert loss == ref_loss                                  # same numbers as int64 contiguous
    np.testing.assert_allclose(loss, l_mean, rtol=CTC_RTOL)
    np.testing.assert_allclose(grad, g_mean, atol=G_ATOL, rtol=G_RTOL)


# ================================================================== RNN-T
def _rnnt_inputs(seed, B, T, S, C, blank, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    am = torch.randn(B, T, C, generator=g) * scale
    lm = torch.randn(B, S + 1, C, generator=g) * scale
    return am, lm, LC.draw_symbols(g, B, S, C, blank)


_weights = LC.weights


def _pad_frames(am, el, value):
    am = am.clone()
    for b in range(am.shape[0]):
        n = am.shape[1] - int(el[b])
        if n and value == 0.0:
            am[b, int(el[b]):] = 0.0
        elif n:
            sign = 1.0 - 2.0 * ((torch.arange(n * am.shape[2]) % 3) == 0).float()
            am[b, int(el[b]):] = value * sign.reshape(n, am.shape[2])
    return am


def _check_ranges(rg, S, R, gx, gy, bnd):
    """Invariants that need no oracle, the k2 step bound, and bit-exact agreement with
    oracle.k2_rnnt fed the SAME gradient tensors (integer work on identical inputs)."""
    rg = rg.cpu()
    s0 = rg[:, :, 0]
    assert (s0[:, 0] == 0).all()
    assert (s0[:, 1:] >= s0[:, :-1]).all()
    assert (rg >= 0).all() and (rg <= S).all()
    assert (s0[:, 1:] - s0[:, :-1] < rg.shape[2]).all()
    assert torch.equal(rg, K.get_rnnt_prune_ranges(gx.cpu(), gy.cpu(), bnd.cpu(), R))


def _simple_ranges_pruned(dev, am, lm, sym, tl, el, R, blank, act, w, check_ranges=True):
    """simple -> ranges -> fused pruned joiner on the device, each held to float64 under the
    per-utterance weights w; returns the device results for further assertions."""
    k = _kern()
    B, T, C = am.shape
    S = sym.shape[1]
    bnd = L.make_boundary(tl, el)
    bnd_g = k.make_boundary(tl, el, dev)
    wg = w.float().to(dev)
    am_g = am.to(dev).requires_grad_(True); lm_g = lm.to(dev).requires_grad_(True)
    neg, gx, gy = k.rnnt_simple_loss(lm_g, am_g, sym.to(dev), bnd_g, blank)
    d_am_s, d_lm_s = torch.autograd.grad((wg * neg).sum(), (am_g, lm_g))
    rg = k.rnnt_prune_ranges(gx, gy, bnd_g, R)
    if check_ranges:
        _check_ranges(rg, S, R, gx, gy, bnd)
    pl = k.rnnt_pruned_joiner_loss(am_g, lm_g, rg, sym.to(dev), bnd_g, blank, act)
    d_am_p, d_lm_p = torch.autograd.grad((wg * pl).sum(), (am_g, lm_g))

    a = am.double().requires_grad_(True); l = lm.double().requires_grad_(True)
    s_ref = L.simple_neg(a, l, sym, bnd, blank)
    ra_s, rl_s = torch.autograd.grad((w * s_ref).sum(), (a, l))
    p_ref = L.pruned_neg(a, l, rg.cpu(), sym, bnd, blank, act)
    ra_p, rl_p = torch.autograd.grad((w * p_ref).sum(), (a, l))
    assert torch.isfinite(s_ref).all() and torch.isfinite(p_ref).all()
    np.testing.assert_allclose(_np(neg), _np(s_ref), rtol=RNNT_RTOL)
    np.testing.assert_allclose(_np(pl), _np(p_ref), rtol=RNNT_RTOL)
    _assert_grad(d_am_s, ra_s, what="simple d_am"); _assert_grad(d_lm_s, rl_s, what="simple d_lm")
    _assert_grad(d_am_p, ra_p, what="pruned d_am"); _assert_grad(d_lm_p, rl_p, what="pruned d_lm")
    return dict(neg=neg, pl=pl, rg=rg, d_am_s=d_am_s, d_am_p=d_am_p, d_lm_s=d_lm_s,
                d_lm_p=d_lm_p, gx=gx, gy=gy)


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_rnnt_per_utterance_weights_simple_and_pruned(dev, act):
    """gscale[b] in simple_w / simple_dam / simple_dlm / pruned_dam / pruned_dlm."""
    B, T, S, C, R = 5, 40, 12, 33, 5
    am, lm, sym = _rnnt_inputs(21, B, T, S, C, 0, 0.8 if act == "tanh" else 2.0)
    tl = torch.tensor([S, 7, 12, 9, 3]); el = torch.tensor([T, 31, 25, T, 18])
    _simple_ranges_pruned(dev, am, lm, sym, tl, el, R, 0, act, _weights(B))


@pytest.mark.parametrize("V,pruned", [(31, False), (33, True), (5003, True)])
def test_rnnt_materialised_lattice_gradient_under_weights(dev, V, pruned):
    """rnnt_lattice_loss from given logits (lattice_fwd / lattice_bwd, gscale[b] included): the
    full lattice, and the pruned one (the use_out_project=True path) with d logits."""
    k = _kern()
    B, T, S, R = 4, 14, 6, 3
    g = torch.Generator().manual_seed(V)
    blank = V // 3
    sym = LC.draw_symbols(g, B, S, V, blank)
    tl = torch.tensor([S, 3, 0, 5]); el = torch.tensor([T, 9, 6, T])
    if pruned:
        # a valid band per utterance: starts at 0, rises one row at a time, holds S_b at the end
        top = (tl - R + 1).clamp(min=0).reshape(B, 1)
        s0 = torch.minimum(top, (torch.arange(T).reshape(1, T) * (top + 1)) // el.reshape(B, 1))
        ranges = (s0.reshape(B, T, 1) + torch.arange(R).reshape(1, 1, R)).contiguous()
        logits = torch.randn(B, T, R, V, generator=g) * 2
    else:
        ranges = None
        logits = torch.randn(B, T, S + 1, V, generator=g) * 2
    w = _weights(B)
    bnd = L.make_boundary(tl, el)
    ref_l = logits.double().requires_grad_(True)
    ref = L.lattice_neg(ref_l, ranges, sym, bnd, blank)
    assert torch.isfinite(ref).all()
    (w * ref).sum().backward()
    lg = logits.to(dev).requires_grad_(True)
    out = k.rnnt_lattice_loss(lg, None if ranges is None else ranges.to(dev), sym.to(dev),
                              k.make_boundary(tl, el, dev), blank)
    (w.float().to(dev) * out).sum().backward()
    np.testing.assert_allclose(_np(out), _np(ref), rtol=RNNT_RTOL)
    _assert_grad(lg.grad, ref_l.grad, what=f"d logits V={V}")
    assert (lg.grad[1, 9:] == 0).all() and (lg.grad[2, 6:] == 0).all()     # frames past T_b


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("C", [128, 129, 256, 257, 512, 513, 1024])
def test_fused_pruned_joiner_at_every_width(dev, C, act):
    """pruned_{fwd,dam,dlm}_kernel<2> (C=128), <4> (129, 256), <8> (257, 512), <16> (513, 1024);
    the blank moves with the width (first / middle / last class)."""
    B, T, S, R = 3, 30, 10, 4
    blank = {0: 0, 1: C // 2, 2: C - 1}[C % 3]
    am, lm, sym = _rnnt_inputs(C, B, T, S, C, blank, 0.8 if act == "tanh" else 2.0)
    tl = torch.tensor([S, 6, 2]); el = torch.tensor([T, 22, 13])
    _simple_ranges_pruned(dev, am, lm, sym, tl, el, R, blank, act, _weights(B))


def test_fused_pruned_joiner_above_its_width_is_refused(dev):
    k = _kern()
    B, T, S, C, R = 1, 6, 3, 1025, 2
    am = torch.zeros(B, T, C, device=dev); lm = torch.zeros(B, S + 1, C, device=dev)
    ranges = torch.zeros(B, T, R, dtype=torch.int64, device=dev)
    sym = torch.ones(B, S, dtype=torch.int64, device=dev)
    bnd = k.make_boundary(torch.tensor([S]), torch.tensor([T]), dev)
    with pytest.raises(ValueError, match="1025"):
        k.rnnt_pruned_joiner_loss(am, lm, ranges, sym, bnd)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_rnnt_blank_position_simple_pruned_full(dev, where):
    k = _kern()
    B, T, S, C, R = 3, 26, 8, 37, 4
    blank = {"first": 0, "middle": 18, "last": C - 1}[where]
    am, lm, sym = _rnnt_inputs(50, B, T, S, C, blank)
    assert (sym != blank).all()
    tl = torch.tensor([S, 5, 1]); el = torch.tensor([T, 17, 9])
    w = _weights(B)
    _simple_ranges_pruned(dev, am, lm, sym, tl, el, R, blank, "relu", w)
    logits = torch.randn(B, T, S + 1, C, generator=torch.Generator().manual_seed(51)) * 2
    ref_l = logits.double().requires_grad_(True)
    ref = L.lattice_neg(ref_l, None, sym, L.make_boundary(tl, el), blank)
    (w * ref).sum().backward()
    lg = logits.to(dev).requires_grad_(True)
    out = k.rnnt_lattice_loss(lg, None, sym.to(dev), k.make_boundary(tl, el, dev), blank)
    (w.float().to(dev) * out).sum().backward()
    np.testing.assert_allclose(_np(out), _np(ref), rtol=RNNT_RTOL)
    _assert_grad(lg.grad, ref_l.grad, what="full d logits")


def _length_mix(S, T, R):
    """(S_b, T_b) over S_b in {0, 1, R-2, S} x T_b in {1, S_b+1, T} where the pruned band can hold
    it (T_b = 1 needs S_b < R), plus S_b + T_b in {8k-1, 8k, 8k+1}."""
    pairs = []
    for sb in sorted({0, 1, min(max(R - 2, 0), S), S}):
        for tb in sorted({1, sb + 1, T}):
            if tb == 1 and sb >= min(R, S + 1):
                continue
            pairs.append((sb, tb))
    k8 = 8 * ((S + S + 1 + 7) // 8 + 1)
    pairs += [(S, k8 - 1 - S), (S, k8 - S), (S, k8 + 1 - S)]
    assert all(1 <= tb <= T for _, tb in pairs)
    return pairs


@pytest.mark.parametrize("S,R", [(12, 5), (3, 5)])
def test_rnnt_length_edges_and_padded_frames(dev, S, R):
    """Empty transcripts, T_b = 1, S_b < R-1 (pad = 0), S < R (the clamp to S+1, one block),
    S_b + T_b around a multiple of the recursion's 8-diagonal look-ahead; padded am frames hold
    large values: losses bit-identical to zero padding and d_am exactly zero there."""
    T, C = 40, 17
    pairs = _length_mix(S, T, R)
    B = len(pairs)
    tl = torch.tensor([p[0] for p in pairs]); el = torch.tensor([p[1] for p in pairs])
    am, lm, sym = _rnnt_inputs(60 + S, B, T, S, C, 0)
    w = _weights(B)
    r0 = _simple_ranges_pruned(dev, _pad_frames(am, el, 0.0), lm, sym, tl, el, R, 0, "relu", w)
    r1 = _simple_ranges_pruned(dev, _pad_frames(am, el, BIG), lm, sym, tl, el, R, 0, "relu", w)
    assert r0["rg"].shape[2] == min(R, S + 1)
    assert torch.equal(r0["neg"], r1["neg"]) and torch.equal(r0["pl"], r1["pl"])
    assert torch.equal(r0["rg"], r1["rg"])
    for b in range(B):
        assert (r1["d_am_s"][b, int(el[b]):] == 0).all()
        assert (r1["d_am_p"][b, int(el[b]):] == 0).all()


def _mi_case(seed, B, S, T):
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(B, S, T + 1, generator=g) - 2.0
    py = torch.randn(B, S + 1, T, generator=g) - 2.0
    return px, py


def _check_raw_mi(dev, px, py, bnd):
    k = _kern()
    px = L._fix_for_boundary(px, bnd)
    px[:, :, -1] = L.NEG_INF
    ans, _, gx, gy = k.mutual_information(px.to(dev).contiguous(), py.to(dev).contiguous(),
                                          bnd.to(dev))
    sc, rgx, rgy = L.mutual_information(px, py, bnd)
    np.testing.assert_allclose(_np(ans), _np(sc), rtol=2e-5, atol=1e-4)
    _assert_grad(gx, rgx, atol=2e-4, rtol=1e-7, what="px_grad")
    _assert_grad(gy, rgy, atol=2e-4, rtol=1e-7, what="py_grad")


@pytest.mark.parametrize("S,R", [(12, 5), (3, 5)])
def test_raw_mutual_information_length_edges(dev, S, R):
    T = 40
    pairs = _length_mix(S, T, R) + [(S, 1)]
    px, py = _mi_case(70 + S, len(pairs), S, T)
    _check_raw_mi(dev, px, py, L.make_boundary([p[0] for p in pairs], [p[1] for p in pairs]))


@pytest.mark.parametrize("rows", LC.ROW_EDGES)
def test_lattice_rows_at_the_thread_count_edges(dev, rows):
    """S+1 lattice rows = threads of the recursion's workgroup, rounded up to whole waves:
    64 | 65 -> 64 | 128 threads, 128 | 129 -> 128 | 192, 1024 = the limit.  Raw recursion and,
    through it, the weighted simple loss (blank 2), with S_b = 0 and T_b = 1 utterances.  These
    lattices are taller than any the small-case bounds were set on: bounds from FP32_COST."""
    k = _kern()
    c = LC.rows_case(rows)
    ref = LC.rows_reference(c)
    cost = LC.FP32_COST[f"rows{rows}"]
    ans, _, gx, gy = k.mutual_information(c["px"].to(dev), c["py"].to(dev), c["mi_bnd"].to(dev))
    np.testing.assert_allclose(_np(ans), _np(ref["sc"]), rtol=LC.bound(cost["mi_rel"], 2e-5),
                               atol=1e-4)
    _assert_grad(gx, ref["gx"], atol=LC.bound(cost["mi_gx_abs"], 2e-4), rtol=1e-7, what="px_grad")
    _assert_grad(gy, ref["gy"], atol=LC.bound(cost["mi_gy_abs"], 2e-4), rtol=1e-7, what="py_grad")
    am_g = c["am"].to(dev).requires_grad_(True); lm_g = c["lm"].to(dev).requires_grad_(True)
    neg, _, _ = k.rnnt_simple_loss(lm_g, am_g, c["sym"].to(dev),
                                   k.make_boundary(c["tl"], c["el"], dev), c["blank"])
    (c["w"].float().to(dev) * neg).sum().backward()
    np.testing.assert_allclose(_np(neg), _np(ref["simple"]),
                               rtol=LC.bound(cost["simple_rel"], RNNT_RTOL))
    _assert_grad(am_g.grad, ref["d_am"], atol=LC.bound(cost["d_am_abs"], G_ATOL), what="simple d_am")
    _assert_grad(lm_g.grad, ref["d_lm"], atol=LC.bound(cost["d_lm_abs"], G_ATOL), what="simple d_lm")


def test_lattice_rows_above_the_limit_are_refused(dev):
    k = _kern()
    S, T = 1024, 4
    px = torch.zeros(1, S, T + 1, device=dev); py = torch.zeros(1, S + 1, T, device=dev)
    bnd = k.make_boundary(torch.tensor([S]), torch.tensor([T]), dev)
    with pytest.raises(ValueError, match="1024"):
        k.mutual_information(px, py, bnd)
    with pytest.raises(ValueError, match="1024"):
        k.rnnt_simple_loss(torch.zeros(1, S + 1, 8, device=dev), torch.zeros(1, T, 8, device=dev),
                           torch.ones(1, S, dtype=torch.int64, device=dev), bnd)


def _grid(x, bits=20):
    """Round to multiples of 2^-bits: sums of a few such values are exact in fp32, so the order
    in which a window is added cannot matter."""
    return torch.round(x * 2 ** bits) / 2 ** bits


@pytest.mark.parametrize("S,R", [(20, 5), (3, 5)])
@pytest.mark.parametrize("T", [255, 256, 257, 600, 1500])
def test_prune_ranges_on_synthetic_gradients(dev, T, S, R):
    """Each of block_suffix_min's 256 threads owns ceil(T/256) frames: 1, 1, 2, 3 and 6 here.
    Utterances 0-2 carry a ridge of occupation along a monotone path plus noise (the ranges follow
    it), 3-5 pure noise (the arg-max jumps and the two monotone passes do all the work)."""
    k = _kern()
    B = 6
    g = torch.Generator().manual_seed(T + S)
    tl = torch.tensor([S, S - 1, 2, S, 0, S]); el = torch.tensor([T, T - 1, T // 2, T, 77, 1])
    s_ax = torch.arange(S + 1).reshape(1, S + 1, 1).float()
    t_ax = torch.arange(T).reshape(1, 1, T).float()
    path = t_ax * (tl.reshape(B, 1, 1).float() / el.reshape(B, 1, 1).float().clamp(min=1))
    ridge = torch.exp(-0.5 * (s_ax - path) ** 2)
    ridge[3:] = 0
    gy = _grid(ridge + 0.3 * torch.rand(B, S + 1, T, generator=g))
    gx = _grid(0.5 * torch.rand(B, S, T + 1, generator=g))
    bnd = L.make_boundary(tl, el)
    rg = k.rnnt_prune_ranges(gx.to(dev), gy.to(dev), bnd.to(dev), R)
    assert rg.shape == (B, T, min(R, S + 1))
    _check_ranges(rg, S, R, gx, gy, bnd)


def test_loss_at_the_c3_bench_geometry(dev):
    """T=248, S=50, C=500, R=5 at the bench's B=64, ragged, simple -> ranges -> fused pruned,
    0.5 / 0.5 of the batch means."""
    k = _kern()
    c = LC.bench_case()
    B, S, R = c["B"], c["S"], c["R"]
    sym = c["sym"].to(dev)
    bnd = L.make_boundary(c["tl"], c["el"])
    bnd_g = k.make_boundary(c["tl"], c["el"], dev)
    am_g = c["am"].to(dev).requires_grad_(True); lm_g = c["lm"].to(dev).requires_grad_(True)
    neg, gx, gy = k.rnnt_simple_loss(lm_g, am_g, sym, bnd_g)
    rg = k.rnnt_prune_ranges(gx, gy, bnd_g, R)
    _check_ranges(rg, S, R, gx, gy, bnd)
    pl = k.rnnt_pruned_joiner_loss(am_g, lm_g, rg, sym, bnd_g)
    (0.5 * neg.mean() + 0.5 * pl.mean()).backward()
    ref = LC.bench_reference(c, rg.cpu())
    cost = LC.FP32_COST["rnnt_bench"]
    for name, got, key in (("simple", neg, "simple_rel"), ("pruned", pl, "pruned_rel")):
        rel = np.max(np.abs(_np(got) - _np(ref[name])) / _np(ref[name]))
        print(f"B={B} {name} loss: max rel dev {rel:.3e}")
        np.testing.assert_allclose(_np(got), _np(ref[name]), rtol=LC.bound(cost[key], RNNT_RTOL))
    _assert_grad(am_g.grad, ref["d_am"], atol=LC.bound(cost["d_am_abs"], G_ATOL), what="d_am")
    _assert_grad(lm_g.grad, ref["d_lm"], atol=LC.bound(cost["d_lm_abs"], G_ATOL), what="d_lm")
