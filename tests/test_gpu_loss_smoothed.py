"""GPU: csrc/rnnt_smooth.hip -- the simple RNN-T loss with non-zero lm_only_scale / am_only_scale
-- against float64.

Every case goes through speech2text_amd.kernels.rnnt_simple_loss under the per-utterance weights
LC.weights(B) and is compared with tests/lattice_smoothed_f64.py (pinned to oracle.k2_rnnt by
tests/test_lattice_smoothed_f64.py): per-utterance loss, d_am, d_lm, and px_grad / py_grad against
the restatement's occupation counts.  The float64 side is whole-batch (the unigram u couples the
utterances) and is computed once per case (loss_smoothed_cases.reference).

Bounds: those tests/test_gpu_loss_lattices.py holds for the same quantities -- loss rtol 1e-4,
gradients atol 3e-5 with rtol 2e-3, raw occupation counts atol 2e-4 -- each widened to
loss_cases.bound(measured, floor) = max(4 x what fp32 costs the REFERENCE on that case, the floor)
from loss_smoothed_cases.FP32_COST.  At these sizes the table lifts d_lm on most cases (the
reference's own fp32 deviation there is 1.7e-6 ... 1.3e-4, so 4x it passes the 3e-5 floor from
7.5e-6 on), d_am and the occupation counts on rows_lm130_am64 (2.76e-4, 2.36e-4 for px_grad), and
everything on T257, a 257-frame lattice under a weight of 0.65: d_am 2.24e-4, d_lm 2.68e-2,
px_grad 3.64e-4, py_grad 1.6e-3.  Every comparison prints its deviation next to its bound.

No element is left out of a comparison; bit-exact assertions are conditions.
"""
import numpy as np
import pytest
import torch

import lattice_f64 as L
import lattice_smoothed_f64 as LS
import loss_cases as LC
import loss_smoothed_cases as SC
from loss_cases import _kern, _np
from oracle import k2_rnnt as K

pytestmark = pytest.mark.gpu

G_ATOL, G_RTOL = 3e-5, 2e-3            # gradients under weights that sum to about one
RNNT_RTOL = 1e-4                       # losses
OCC_ATOL = 2e-4                        # raw occupation counts
BIG = 3.0e4                            # "large finite" filler of padded frames


def _run(dev, c, am=None, scales=True):
    """rnnt_simple_loss on the device under c's weights -> neg, gx, gy, d_am, d_lm (device)."""
    k = _kern()
    am_g = (c["am"] if am is None else am).to(dev).requires_grad_(True)
    lm_g = c["lm"].to(dev).requires_grad_(True)
    bnd_g = k.make_boundary(c["tl"], c["el"], dev)
    args = (c["lam"], c["mu"]) if scales else ()
    neg, gx, gy = k.rnnt_simple_loss(lm_g, am_g, c["sym"].to(dev), bnd_g, c["blank"], *args)
    d_am, d_lm = torch.autograd.grad((c["w"].float().to(dev) * neg).sum(), (am_g, lm_g))
    return dict(neg=neg, gx=gx, gy=gy, d_am=d_am, d_lm=d_lm, bnd_g=bnd_g, am_g=am_g, lm_g=lm_g)


def _hold(got, ref, b, what):
    for key, atol, rtol in (("d_am", b["d_am"], G_RTOL), ("d_lm", b["d_lm"], G_RTOL),
                            ("gx", b["gx"], 1e-7), ("gy", b["gy"], 1e-7)):
        print(f"{what} {key}: max abs dev {np.abs(_np(got[key]) - _np(ref[key])).max():.3e} "
              f"(atol {atol:.1e})")
    rel = np.max(np.abs(_np(got["neg"]) - _np(ref["neg"])) / np.abs(_np(ref["neg"])))
    print(f"{what} loss: max rel dev {rel:.3e} (rtol {b['loss']:.1e})")
    assert torch.isfinite(ref["neg"]).all()
    np.testing.assert_allclose(_np(got["neg"]), _np(ref["neg"]), rtol=b["loss"])
    np.testing.assert_allclose(_np(got["d_am"]), _np(ref["d_am"]), atol=b["d_am"], rtol=G_RTOL)
    np.testing.assert_allclose(_np(got["d_lm"]), _np(ref["d_lm"]), atol=b["d_lm"], rtol=G_RTOL)
    np.testing.assert_allclose(_np(got["gx"]), _np(ref["gx"]), atol=b["gx"], rtol=1e-7)
    np.testing.assert_allclose(_np(got["gy"]), _np(ref["gy"]), atol=b["gy"], rtol=1e-7)


def _bounds(name):
    return SC.bounds(name, RNNT_RTOL, G_ATOL, OCC_ATOL)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_smoothed_simple_loss_vs_float64(dev, name):
    """lam / mu / both / heavy: the scales (0.25, 0), (0, 0.3), (0.25, 0.1), (0.5, 0.4) at B=4,
    T=20, S=7, C=33, ragged with an S_b = 0 and a T_b = 1 utterance (mu = 0 takes
    smooth_dam_kernel<false> / smooth_dlm_kernel<false> and no unigram launch).
    C63 ... C500: the lane-stride edges of the wave-per-row kernels and the C3 joiner width.
    blank_*: blank first / middle / last at C = 33.
    T257: one step over the 256-frame tile of the px/py pass.
    rows_lmX_amY: B (S+1) = X lm rows and B T = Y am rows on both sides of the slabs of the two
    column reductions: 63 | 64 | 65 | 130 around S2T_RNNT_SMOOTH_LM_SLAB = 64 (u), 31 | 32 | 33 | 35
    | 64 around S2T_RNNT_SMOOTH_AM_SLAB = 32 (dlogu)."""
    k = _kern()
    assert (SC.LM_SLAB, SC.AM_SLAB) == (k._SMOOTH_LM_SLAB, k._SMOOTH_AM_SLAB)
    c = SC.case(name)
    _hold(_run(dev, c), SC.reference(name), _bounds(name), name)


def test_padded_frames_feed_nothing(dev):
    """Frames t >= T_b filled with 0 and with +-3e4: bit-equal results (they feed neither the
    lattice nor u nor dlogu), d_am exactly zero there."""
    c = SC.case("both")
    b = _bounds("both")
    out = []
    for fill in (0.0, BIG):
        am = c["am"].clone()
        for i in range(c["B"]):
            n = c["T"] - int(c["el"][i])
            sign = 1.0 - 2.0 * ((torch.arange(n * c["C"]) % 3) == 0).float()
            am[i, int(c["el"][i]):] = fill * sign.reshape(n, c["C"])
        got = _run(dev, c, am=am)
        ref = SC.reference_of(am, c["lm"], c["sym"], c["tl"], c["el"], c["blank"], c["lam"],
                              c["mu"], c["w"])
        _hold(got, ref, b, f"fill {fill:g}")
        for i in range(c["B"]):
            assert (got["d_am"][i, int(c["el"][i]):] == 0).all()
        out.append(got)
    for key in ("neg", "gx", "gy", "d_am", "d_lm"):
        assert torch.equal(out[0][key], out[1][key]), key


def test_smoothed_simple_then_ranges_then_fused_pruned_joiner(dev):
    """The whole chain at (0.25, 0.1): ranges bit-equal to oracle.get_rnnt_prune_ranges fed the
    SAME device gx, gy; the pruned loss and its gradients against lattice_f64.pruned_neg on
    those ranges (at test_gpu_loss_lattices.py's small-case bounds: the pruned loss itself is
    not smoothed)."""
    k = _kern()
    c = SC.case("both")
    R = 5
    assert all(int(s) < R for s, t in zip(c["tl"], c["el"]) if int(t) == 1)
    got = _run(dev, c)
    _hold(got, SC.reference("both"), _bounds("both"), "simple")
    bnd = L.make_boundary(c["tl"], c["el"])
    rg = k.rnnt_prune_ranges(got["gx"], got["gy"], got["bnd_g"], R)
    assert rg.shape == (c["B"], c["T"], R)
    assert torch.equal(rg.cpu(), K.get_rnnt_prune_ranges(got["gx"].cpu(), got["gy"].cpu(), bnd, R))
    wg = c["w"].float().to(dev)
    pl = k.rnnt_pruned_joiner_loss(got["am_g"], got["lm_g"], rg, c["sym"].to(dev), got["bnd_g"],
                                   c["blank"], "relu")
    d_am, d_lm = torch.autograd.grad((wg * pl).sum(), (got["am_g"], got["lm_g"]))
    a = c["am"].double().requires_grad_(True); l = c["lm"].double().requires_grad_(True)
    p_ref = L.pruned_neg(a, l, rg.cpu(), c["sym"], bnd, c["blank"], "relu")
    ra, rl = torch.autograd.grad((c["w"] * p_ref).sum(), (a, l))
    assert torch.isfinite(p_ref).all()
    np.testing.assert_allclose(_np(pl), _np(p_ref), rtol=RNNT_RTOL)
    np.testing.assert_allclose(_np(d_am), _np(ra), atol=G_ATOL, rtol=G_RTOL)
    np.testing.assert_allclose(_np(d_lm), _np(rl), atol=G_ATOL, rtol=G_RTOL)


@pytest.mark.parametrize("use_out_project", [False, True])
def test_joiner_forward_with_lm_scale(dev, use_out_project):
    """Joiner.forward on the device at (0.25, 0): simple_loss is the restatement's mean on the
    module's own projections, on both returns."""
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig, PrunedLattice
    B, T, S, D, C, R = 3, 12, 5, 16, 33, 5
    torch.manual_seed(11)
    j = Joiner(JoinerConfig(input_dim=D, output_dim=C, inner_dim=8, prune_range=R, lm_scale=0.25,
                            use_out_project=use_out_project))
    with torch.no_grad():
        for p in j.parameters():
            p.mul_(3.0)
    j.to(dev)
    g = torch.Generator().manual_seed(12)
    enc = torch.randn(B, T, D, generator=g).to(dev)
    pred = torch.randn(B, S + 1, D, generator=g).to(dev)
    sym = LC.draw_symbols(g, B, S, C, 0)
    tl, el = SC.lengths(B, S, T)
    logits, boundary, ranges, simple_loss = j(enc, el.to(dev), pred, tl.to(dev), sym.to(dev))
    assert isinstance(logits, PrunedLattice) != use_out_project
    assert tuple(logits.shape) == (B, T, R, C) and tuple(ranges.shape) == (B, T, R)
    with torch.no_grad():
        am = j._enc_proj(enc).cpu().double(); lm = j._pre_proj(pred).cpu().double()
    ref = LS.smoothed_neg(am, lm, sym, L.make_boundary(tl, el), 0, 0.25, 0.0).mean()
    print(f"simple_loss {float(simple_loss.detach()):.6f} restatement {float(ref):.6f}")
    np.testing.assert_allclose(float(simple_loss), float(ref), rtol=RNNT_RTOL)


def test_explicit_zero_scales_are_the_unsmoothed_launches(dev):
    """(0.0, 0.0) passed explicitly: loss, px_grad, py_grad bit-equal to the call without scales
    (the same launches); the gradients, which add through LDS atomics, to the usual bounds."""
    c = dict(SC.case("both"), lam=0.0, mu=0.0)
    a = _run(dev, c, scales=True)
    b = _run(dev, c, scales=False)
    for key in ("neg", "gx", "gy"):
        assert torch.equal(a[key], b[key]), key
    np.testing.assert_allclose(_np(a["d_am"]), _np(b["d_am"]), atol=G_ATOL, rtol=G_RTOL)
    np.testing.assert_allclose(_np(a["d_lm"]), _np(b["d_lm"]), atol=G_ATOL, rtol=G_RTOL)
    am = c["am"].double().requires_grad_(True); lm = c["lm"].double().requires_grad_(True)
    ref = L.simple_neg(am, lm, c["sym"], L.make_boundary(c["tl"], c["el"]), c["blank"])
    np.testing.assert_allclose(_np(a["neg"]), _np(ref), rtol=RNNT_RTOL)
