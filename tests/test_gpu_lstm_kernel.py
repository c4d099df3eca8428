"""GPU: the layer-norm LSTM sequence kernel (csrc/lstm.hip) called directly through
conf_kernels.lnlstm on device tensors -- no Linear in front -- against the float64 restatement
tests/lstm_f64.py, at every dispatch edge of the kernel (tests/lstm_cases.py: Q = 1..4 gate rows
per thread, exact and inexact k-group / row-group splits, T = 1, initial state, saturated gates).

Error = max |got - ref| / max |ref| per tensor; allowed = max(2e-5, 8 x the case's fp32 figure)
(lstm_cases.bound; the figure is the float32 CPU evaluation of the REFERENCE against float64,
asserted by tests/test_lstm_f64.py).  d p2g.weight comes from the bf16-split weight-gradient
GEMM: its bound is the arith_bound factor times that (tests/conftest.py).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lstm_cases as LC
import lstm_f64 as LF
from oracle import conformer as OC

pytestmark = pytest.mark.gpu


def _modules(name, dev, store):
    """-> (wp Parameter, g_norm, c_norm) on the device holding the case's parameters; `store`:
    registered in a flat store, so that the backward writes the gradients into its slots."""
    from speech2text_amd import flat
    c, t = LC.CASES[name], LC.make(name)
    H = c["H"]
    wp = torch.nn.Parameter(t["wp"].to(dev))
    params = [wp]
    if c["ln"]:
        gn = torch.nn.LayerNorm(4 * H, eps=LC.EPS).to(dev)
        cn = torch.nn.LayerNorm(H, eps=LC.EPS).to(dev)
        with torch.no_grad():
            gn.weight.copy_(t["gg"]); gn.bias.copy_(t["gb"])
            cn.weight.copy_(t["cg"]); cn.bias.copy_(t["cb"])
        params += [gn.weight, gn.bias, cn.weight, cn.bias]
    else:
        gn = cn = torch.nn.Identity()
    if store:
        st = flat.get_store(params)
        st.zero_grad()
        assert all(flat.owned(p) for p in params)
    return wp, gn, cn


def _forward(name, dev, store):
    from speech2text_amd import conf_kernels as ck
    t = LC.make(name)
    wp, gn, cn = _modules(name, dev, store)
    gx = t["gx"].to(dev).requires_grad_(True)
    h0 = None if t["h0"] is None else t["h0"].to(dev)
    c0 = None if t["c0"] is None else t["c0"].to(dev)
    hs, hT, cT = ck.lnlstm(gx, wp, gn, cn, h0, c0)
    return dict(gx=gx, wp=wp, gn=gn, cn=cn, hs=hs, hT=hT, cT=cT, dhs=t["dhs"].to(dev))


def _grads(r, ln):
    out = dict(d_gx=r["gx"].grad, d_wp=r["wp"].grad)
    if ln:
        out.update(d_gg=r["gn"].weight.grad, d_gb=r["gn"].bias.grad, d_cg=r["cn"].weight.grad,
                   d_cb=r["cn"].bias.grad)
    return {k: v.detach().clone() for k, v in out.items()}


def _hold(name, got, ref, kind, wp_factor, what, scale=1.0):
    for k, v in got.items():
        assert torch.isfinite(v).all(), f"{name} {what} {k}: not finite"
        err = LC.rel_err(v, scale * ref[k])
        tol = LC.bound(name, kind) * (wp_factor if k == "d_wp" else 1.0)
        print(f"{name} {what} {k}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, f"{name} {what} {k}: err {err:.3e} > bound {tol:.3e}"


@pytest.mark.parametrize("name", LC.KERNEL_CASES)
def test_lnlstm_kernel_vs_float64(dev, name, arith_bound):
    """Forward, and the backward under a random dhs, on plain parameters (gradients returned)
    and on parameters of a flat store (gradients land in the slots).  A second backward into the
    same slots doubles them: the LayerNorm gradients are ACCUMULATED (one atomic per channel and
    workgroup), so with one workgroup (B = 1: one add per slot and pass, a + a) twice is exact;
    with B > 1 the B adds of the second pass meet the first pass's sum in an order the hardware
    picks, so (s + a) + b need not round to 2 (a + b) and half the result is held to the
    reference at the case's bound instead."""
    c, ref = LC.CASES[name], LC.reference(name)
    for store in (False, True):
        what = "slots" if store else "returned"
        r = _forward(name, dev, store)
        assert type(r["hs"].grad_fn).__name__ == "_LnLstmBackward", "the sequence kernel did not run"
        _hold(name, {k: r[k] for k in LC.TENSORS_FWD}, ref, "fwd", 1.0, what)
        (r["hs"] * r["dhs"]).sum().backward(retain_graph=store)
        torch.cuda.synchronize()
        first = _grads(r, c["ln"])
        _hold(name, first, ref, "bwd", arith_bound, what)
        if store:
            (r["hs"] * r["dhs"]).sum().backward()
            torch.cuda.synchronize()
            second = _grads(r, c["ln"])
            _hold(name, second, ref, "bwd", arith_bound, "slots, second pass", scale=2.0)
            if c["B"] == 1:
                for k in ("d_gg", "d_gb", "d_cg", "d_cb"):
                    assert torch.equal(second[k], 2 * first[k]), f"{name} {k}: second pass != 2 x first"


@pytest.mark.parametrize("name", ["h20_state", "h8_t1", "h260"])
def test_lnlstm_state_contract(dev, name):
    """h_T / c_T are the last step and carry no gradient; h0 / c0 are constants: one that requires
    grad raises instead of silently getting None."""
    from speech2text_amd import conf_kernels as ck
    r = _forward(name, dev, False)
    assert torch.equal(r["hT"], r["hs"][-1])
    assert not r["hT"].requires_grad and not r["cT"].requires_grad and r["hs"].requires_grad
    ref = LC.reference(name)
    assert LC.rel_err(r["cT"], ref["cT"]) <= LC.bound(name, "fwd")
    t = LC.make(name)
    B, H = LC.CASES[name]["B"], LC.CASES[name]["H"]
    h0 = torch.randn(B, H, device=dev)
    c0 = torch.randn(B, H, device=dev)
    for hr, cr in ((True, False), (False, True)):
        with pytest.raises(RuntimeError, match="h0 / c0"):
            ck.lnlstm(t["gx"].to(dev).requires_grad_(True), r["wp"], r["gn"], r["cn"],
                      h0.clone().requires_grad_(hr), c0.clone().requires_grad_(cr))
    with torch.no_grad():           # nothing to differentiate: accepted
        ck.lnlstm(t["gx"].to(dev), r["wp"], r["gn"], r["cn"], h0.clone().requires_grad_(True), c0)


@pytest.mark.parametrize("name", LC.FALLBACK_CASES)
def test_lnlstm_widths_outside_the_kernels_rule(dev, name):
    """H % 4 != 0 or H > 1024: conf_kernels.lnlstm composes the recurrence from torch's device ops
    (it used to fail with -2); held to float64 at the kernel's bounds."""
    ref = LC.reference(name)
    r = _forward(name, dev, False)
    assert r["hs"].is_cuda and r["hs"].dtype == torch.float32
    assert not r["hT"].requires_grad and not r["cT"].requires_grad
    _hold(name, {k: r[k] for k in LC.TENSORS_FWD}, ref, "fwd", 1.0, "composed")
    (r["hs"] * r["dhs"]).sum().backward()
    _hold(name, _grads(r, LC.CASES[name]["ln"]), ref, "bwd", 1.0, "composed")


def test_lstm_predictor_at_the_yaml_dims_with_dropout(dev, monkeypatch):
    """The reference YAMLs' predictor (3 layers, E = H = 512, output 1024, layer norm, dropout 0.3)
    in train mode: output and every parameter gradient against the stacked float64 restatement
    under the same keep masks (seeds recorded at draw_seed, masks rebuilt with
    oracle.conformer.keep_scale), at test_lstm_predictor_vs_oracle's bounds."""
    from speech2text_amd import conf_kernels as ck
    from speech2text_amd.model.predictor.predictor import Predictor
    torch.manual_seed(11)
    V, E, H, D, L, B, U, p = 128, 512, 512, 1024, 3, 2, 20, 0.3
    m = Predictor({"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": D, "symbol_embedding_dim": E, "num_lstm_layers": L,
        "lstm_hidden_dim": H, "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3,
        "lstm_dropout": p}})
    with torch.no_grad():
        for n, q in m.named_parameters():
            if "norm" in n:
                q.add_(0.2 * torch.randn_like(q))
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m.to(dev).train()
    lab = torch.randint(1, V - 1, (B, U))
    seeds = []
    real = ck.draw_seed
    monkeypatch.setattr(ck, "draw_seed", lambda: seeds.append(real()) or seeds[-1])
    y, _, _ = m(lab.to(dev), torch.full((B,), U, device=dev), m.init_state())
    assert len(seeds) == L, seeds                      # one dropout site after every layer
    keep = [OC.keep_scale(s, (U + 1, B, H), p).double() for s in seeds]
    assert all(0.6 < (k > 0).double().mean() < 0.8 for k in keep)
    pf = "predictor._predictor."
    tok = torch.cat((torch.zeros(B, 1, dtype=torch.int64), lab), dim=1)
    x = F.layer_norm(F.embedding(tok.t(), sd[pf + "embedding.weight"]), (E,),
                     sd[pf + "input_layer_norm.weight"], sd[pf + "input_layer_norm.bias"])
    layers = []
    for l in range(L):
        q = f"{pf}lstm_layers.{l}."
        layers.append(dict(x2g_w=sd[q + "x2g.weight"], wp=sd[q + "p2g.weight"],
                           gg=sd[q + "g_norm.weight"], gb=sd[q + "g_norm.bias"],
                           cg=sd[q + "c_norm.weight"], cb=sd[q + "c_norm.bias"], eps=1e-3))
    hs = LF.lnlstm_stack_ref(x, layers, keep)
    yo = F.layer_norm(F.linear(hs, sd[pf + "linear.weight"], sd[pf + "linear.bias"]), (D,),
                      sd[pf + "output_layer_norm.weight"], sd[pf + "output_layer_norm.bias"]).permute(1, 0, 2)
    assert y.shape == (B, U + 1, D)
    np.testing.assert_allclose(y.detach().cpu().numpy(), yo.detach().numpy(), atol=5e-5, rtol=2e-4)
    w = torch.randn(B, U + 1, D)
    (y * w.to(dev)).sum().backward()
    (yo * w.double()).sum().backward()
    for k, v in m.named_parameters():
        ref = sd[k].grad.numpy()
        err = np.abs(v.grad.cpu().numpy() - ref).max()
        print(f"{k}: err {err:.3e} max|ref| {np.abs(ref).max():.3e}")
        assert err <= 3e-3 * np.abs(ref).max() + 5e-5, (k, err, np.abs(ref).max())
