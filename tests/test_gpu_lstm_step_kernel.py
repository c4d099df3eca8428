"""GPU: the step-launched LSTM kernel (csrc/lstm_step.hip) called directly through
conf_kernels.lstm on device tensors -- no Linear in front -- against the float64 restatement
tests/rnn_lm_f64.lstm_ref, forward and backward under a random dhs, at every dispatch edge of its
tiling (tests/rnn_lm_cases.py: partial / exact / several batch tiles, partial hidden slices, partial
K chunks, T = 1, initial state, saturated gates, the small-batch threshold and the branch below
it, the composed path).

Error = max |got - ref| / max |ref| per tensor; allowed = max(2e-5, 8 x the case's fp32 figure)
(rnn_lm_cases.bound; the figure is torch.nn.LSTM in float32 on the CPU against float64, asserted
by tests/test_rnn_lm_f64.py).  d weight_hh comes from the bf16-split weight-gradient GEMM: its bound
is the arith_bound factor times that (tests/conftest.py).
"""
import pytest
import torch

import rnn_lm_cases as LC

pytestmark = pytest.mark.gpu

STEP_NODE, SEQ_NODE = "_LstmSeqBackward", "_LnLstmBackward"


def _forward(name, dev, store=False):
    from speech2text_amd import conf_kernels as ck
    from speech2text_amd import flat
    t = LC.make(name)
    whh = torch.nn.Parameter(t["whh"].to(dev))
    if store:
        flat.get_store([whh]).zero_grad()
        assert flat.owned(whh)
    gx = t["gx"].to(dev).requires_grad_(True)
    h0 = None if t["h0"] is None else t["h0"].to(dev)
    c0 = None if t["c0"] is None else t["c0"].to(dev)
    hs, hT, cT = ck.lstm(gx, whh, h0, c0)
    return dict(gx=gx, whh=whh, hs=hs, hT=hT, cT=cT, dhs=t["dhs"].to(dev))


def _hold(name, got, ref, kind, whh_factor, what):
    for k, v in got.items():
        assert torch.isfinite(v).all(), f"{name} {what} {k}: not finite"
        err = LC.rel_err(v, ref[k])
        tol = LC.bound(name, kind) * (whh_factor if k == "d_whh" else 1.0)
        print(f"{name} {what} {k}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, f"{name} {what} {k}: err {err:.3e} > bound {tol:.3e}"


def _check(name, dev, node, whh_factor, stores=(False,)):
    ref = LC.reference(name)
    for store in stores:
        what = "slots" if store else "returned"
        r = _forward(name, dev, store)
        assert type(r["hs"].grad_fn).__name__ == node, type(r["hs"].grad_fn).__name__
        _hold(name, {k: r[k] for k in LC.TENSORS_FWD}, ref, "fwd", 1.0, what)
        (r["hs"] * r["dhs"]).sum().backward()
        torch.cuda.synchronize()
        _hold(name, dict(d_gx=r["gx"].grad, d_whh=r["whh"].grad), ref, "bwd", whh_factor, what)


def test_threshold_is_the_one_the_cases_were_laid_out_for():
    from speech2text_amd import conf_kernels as ck
    assert ck.LSTM_STEP_MIN_BATCH == LC.THRESHOLD


@pytest.mark.parametrize("name", LC.STEP_CASES)
def test_step_kernel_vs_float64(dev, name, arith_bound, monkeypatch):
    """The step kernel itself at every tile edge, with the small-batch threshold pinned to 1 (its
    measured value; pinned so that a later re-measurement cannot move these cases off the kernel
    they are laid out for): the new autograd node must have run.  Plain parameter (gradient
    returned) and a parameter of a flat store (gradient lands in its slot)."""
    from speech2text_amd import conf_kernels as ck
    monkeypatch.setattr(ck, "LSTM_STEP_MIN_BATCH", 1)
    _check(name, dev, STEP_NODE, arith_bound, stores=(False, True))


def test_both_sides_of_the_small_batch_threshold(dev, arith_bound, monkeypatch):
    """The wrapper's own dispatch at B = threshold runs the step kernel.  The measured threshold
    is 1, so no batch lies below it; the branch below -- the per-utterance sequence kernel
    (csrc/lstm.hip, NULL norms) -- is held to the same reference with the threshold raised above
    the case's B = 15."""
    from speech2text_amd import conf_kernels as ck
    (at,), (seq,) = LC.AUTO_CASES, LC.SEQ_CASES
    assert LC.CASES[at]["B"] == ck.LSTM_STEP_MIN_BATCH
    _check(at, dev, STEP_NODE, arith_bound)
    monkeypatch.setattr(ck, "LSTM_STEP_MIN_BATCH", LC.CASES[seq]["B"] + 1)
    _check(seq, dev, SEQ_NODE, arith_bound)


@pytest.mark.parametrize("name", LC.COMPOSED_CASES)
def test_widths_outside_the_kernels_rule(dev, name):
    """H % 4 != 0 or H > 1024: the recurrence composed from torch's device ops, at the kernel's
    bounds."""
    ref = LC.reference(name)
    r = _forward(name, dev)
    assert r["hs"].is_cuda and r["hs"].dtype == torch.float32
    assert type(r["hs"].grad_fn).__name__ not in (STEP_NODE, SEQ_NODE)
    assert not r["hT"].requires_grad and not r["cT"].requires_grad
    _hold(name, {k: r[k] for k in LC.TENSORS_FWD}, ref, "fwd", 1.0, "composed")
    (r["hs"] * r["dhs"]).sum().backward()
    _hold(name, dict(d_gx=r["gx"].grad, d_whh=r["whh"].grad), ref, "bwd", 1.0, "composed")


@pytest.mark.parametrize("name", ["h20_b15_t2", "h4_b1_t1", "h260_b17_t9", "seq_kernel"])
def test_state_contract(dev, name, monkeypatch):
    """h_T / c_T are the last step and carry no gradient; h0 / c0 are constants: one that requires
    grad raises instead of silently getting None.  On both kernels."""
    from speech2text_amd import conf_kernels as ck
    seq = LC.CASES[name]["path"] == "seq"
    monkeypatch.setattr(ck, "LSTM_STEP_MIN_BATCH", LC.CASES[name]["B"] + 1 if seq else 1)
    r = _forward(name, dev)
    assert type(r["hs"].grad_fn).__name__ == (SEQ_NODE if seq else STEP_NODE)
    assert torch.equal(r["hT"], r["hs"][-1])
    assert not r["hT"].requires_grad and not r["cT"].requires_grad and r["hs"].requires_grad
    assert LC.rel_err(r["cT"], LC.reference(name)["cT"]) <= LC.bound(name, "fwd")
    t = LC.make(name)
    B, H = LC.CASES[name]["B"], LC.CASES[name]["H"]
    h0, c0 = torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)
    for hr, cr in ((True, False), (False, True)):
        with pytest.raises(RuntimeError, match="h0 / c0"):
            ck.lstm(t["gx"].to(dev).requires_grad_(True), r["whh"], h0.clone().requires_grad_(hr),
                    c0.clone().requires_grad_(cr))
    with torch.no_grad():           # nothing to differentiate: accepted
        ck.lstm(t["gx"].to(dev), r["whh"], h0.clone().requires_grad_(True), c0)


def test_empty_sequence_and_cpu_tensors(dev):
    from speech2text_amd import conf_kernels as ck
    H, B = 8, 17
    h0, c0 = torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)
    hs, hT, cT = ck.lstm(torch.zeros(0, B, 4 * H, device=dev), torch.randn(4 * H, H, device=dev), h0, c0)
    assert hs.shape == (0, B, H) and torch.equal(hT, h0) and torch.equal(cT, c0)
    with pytest.raises(RuntimeError, match="device tensors"):
        ck.lstm(torch.zeros(2, B, 4 * H), torch.randn(4 * H, H))
