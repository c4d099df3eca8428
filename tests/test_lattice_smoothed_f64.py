"""CPU: tests/lattice_smoothed_f64.py (the float64 yardstick of the smoothed simple loss) pinned to
oracle/k2_rnnt.py, and what fp32 costs the oracle on the cases of tests/loss_smoothed_cases.py:
the figures recorded in FP32_COST there are asserted here, so the GPU file's bounds (4x the figure,
never tighter than the floors) cannot drift.  Also the Joiner's construction-time contract for
lm_scale / am_scale.
"""
import numpy as np
import pytest
import torch

import lattice_f64 as L
import lattice_smoothed_f64 as LS
import loss_cases as LC
import loss_smoothed_cases as SC
from oracle import k2_rnnt as K


_oracle = SC.oracle


def _dev(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("name", list(SC.CASES))
def test_restatement_vs_oracle_f64(name):
    """Same mathematics in the same precision, written independently: 1e-10, which leaves room for
    k2's `tiny` and its 1e-20-scaled terms only."""
    c = SC.case(name)
    ref = SC.reference(name)
    got = _oracle(c, torch.float64)
    assert torch.isfinite(ref["neg"]).all()
    for k in ("neg", "d_am", "d_lm", "gx", "gy"):
        np.testing.assert_allclose(got[k].numpy(), ref[k].numpy(), rtol=1e-10, atol=1e-10, err_msg=k)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_recorded_fp32_is_the_oracles_output(name):
    """tests/golden/loss_smoothed_fp32.npz against the live oracle in fp32.  Loose on purpose: two
    fp32 evaluations on different hosts differ by what fp32 costs either of them (1e-6 ... 1e-2
    here, FP32_COST), a wrong or stale recording by the size of the quantities themselves."""
    got, rec = _oracle(SC.case(name), torch.float32), SC.recorded_fp32(name)
    for k in SC.QUANTITIES:
        assert got[k].shape == rec[k].shape and rec[k].dtype == torch.float32
        scale = float(rec[k].abs().max())
        np.testing.assert_allclose(got[k].numpy(), rec[k].numpy(), rtol=1e-3, atol=2e-2 * scale,
                                   err_msg=k)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_fp32_cost_of_the_smoothed_reference(name):
    """The recorded fp32 output of the oracle against the float64 restatement (live): the figures
    of FP32_COST, reproducible on any host."""
    ref = SC.reference(name)
    got = SC.recorded_fp32(name)
    fig = dict(loss_rel=float(((got["neg"].double() - ref["neg"]).abs() / ref["neg"].abs()).max()),
               d_am_abs=_dev(got["d_am"], ref["d_am"]), d_lm_abs=_dev(got["d_lm"], ref["d_lm"]),
               gx_abs=_dev(got["gx"], ref["gx"]), gy_abs=_dev(got["gy"], ref["gy"]))
    print(f'    # {" ".join(f"{v:.3e}" for v in fig.values())}\n    "{name}": dict('
          + ", ".join(f"{k}={v:.3e}" for k, v in fig.items()) + "),")
    rec = SC.FP32_COST[name]
    for k, v in fig.items():
        assert v <= rec[k], (k, v, rec[k])


@pytest.mark.parametrize("name", ["lam", "C65", "rows_lm65_am35"])
def test_zero_scales_are_the_unsmoothed_loss(name):
    c = SC.case(name)
    am, lm = c["am"].double(), c["lm"].double()
    bnd = L.make_boundary(c["tl"], c["el"])
    got = LS.smoothed_neg(am, lm, c["sym"], bnd, c["blank"], 0.0, 0.0)
    ref = L.simple_neg(am, lm, c["sym"], bnd, c["blank"])
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-12, atol=1e-12)


def test_padded_lm_rows_reach_other_utterances_through_the_unigram():
    """u is the mean over the PADDED lm tensor: a row s > S_b of utterance 1 (S_b = 0) moves
    utterance 0's loss when mu != 0, and nobody's when mu = 0."""
    c = SC.case("both")
    assert int(c["tl"][1]) == 0
    am, lm = c["am"].double(), c["lm"].double()
    bnd = L.make_boundary(c["tl"], c["el"])
    lm2 = lm.clone()
    lm2[1, 3, 5] += 1.5
    for lam, mu, moves in ((0.25, 0.1, True), (0.0, 0.3, True), (0.25, 0.0, False)):
        a = LS.smoothed_neg(am, lm, c["sym"], bnd, c["blank"], lam, mu)
        b = LS.smoothed_neg(am, lm2, c["sym"], bnd, c["blank"], lam, mu)
        if moves:
            assert abs(float(a[0] - b[0])) > 1e-9 * abs(float(a[0]))     # float64: 1e-16
            assert not torch.equal(LS.unigram(lm), LS.unigram(lm2))
        else:
            assert torch.equal(a, b)
        # the oracle agrees on which way it goes
        o = [K.rnnt_loss_smoothed(x, am, c["sym"], c["blank"], bnd, lam, mu, reduction="none",
                                  return_grad=False) for x in (lm, lm2)]
        np.testing.assert_allclose((o[1] - o[0]).numpy(), (b - a).numpy(), rtol=1e-7, atol=1e-12)


def test_joiner_accepts_smoothing_scales_and_refuses_invalid_ones():
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd import kernels
    j = Joiner(JoinerConfig(input_dim=16, output_dim=12, lm_scale=0.25))
    assert j._lm_scale == 0.25 and j._am_scale == 0.0
    Joiner(JoinerConfig(input_dim=16, output_dim=12, lm_scale=0.25, am_scale=0.1, use_out_project=False))
    with pytest.raises(ValueError, match="lm_only_scale"):
        Joiner(JoinerConfig(input_dim=16, output_dim=12, lm_scale=-0.1))
    with pytest.raises(ValueError, match="sum below 1"):
        Joiner(JoinerConfig(input_dim=16, output_dim=12, lm_scale=0.6, am_scale=0.4))
    z = torch.zeros(1, 2, 4)
    for lam, mu in ((-0.1, 0.0), (0.0, -0.2), (0.6, 0.4), (float("nan"), 0.0)):
        with pytest.raises(ValueError):    # refused before any tensor is looked at
            kernels.rnnt_simple_loss(z, z, None, None, 0, lam, mu)
