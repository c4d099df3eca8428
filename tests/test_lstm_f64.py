"""CPU tests of tests/lstm_f64.py, the float64 yardstick of tests/test_gpu_lstm_kernel.py.

The restatement is pinned three ways before the kernel is compared with it: torch.nn.LSTM in
float64 (no layer norm; same i, f, g, o gate order), torch.autograd.gradcheck (layer norm), and
oracle.heads.lstm_predictor on a one-layer state dict (layer norm).

The last part measures what fp32 costs the REFERENCE on every case of tests/lstm_cases.py: the
figures recorded in lstm_cases.FP32_COST are checked here (to the factor by which they move from
host to host), so the GPU file's bounds (max(2e-5, 8 x figure)) cannot drift.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lstm_cases as LC
import lstm_f64 as LF
from oracle import heads as OH


@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("E,H,B,T", [(5, 4, 2, 3), (7, 12, 3, 6)])
def test_without_layer_norm_equals_torch_lstm(E, H, B, T, state):
    g = torch.Generator().manual_seed(E + H + T)
    ref = torch.nn.LSTM(E, H).double()
    x = torch.randn(T, B, E, generator=g, dtype=torch.float64)
    w = torch.randn(T, B, H, generator=g, dtype=torch.float64)
    wh, wc = (torch.randn(B, H, generator=g, dtype=torch.float64) for _ in range(2))
    st = [torch.randn(B, H, generator=g, dtype=torch.float64) for _ in range(2)] if state else None
    x1 = x.clone().requires_grad_(True)
    s1 = None if st is None else tuple(s.clone().unsqueeze(0).requires_grad_(True) for s in st)
    y1, (h1, c1) = ref(x1, s1)
    ((y1 * w).sum() + (h1[0] * wh).sum() + (c1[0] * wc).sum()).backward()
    p = {k: v.detach().clone().requires_grad_(True) for k, v in ref.named_parameters()}
    x2 = x.clone().requires_grad_(True)
    s2 = (None, None) if st is None else tuple(s.clone().requires_grad_(True) for s in st)
    gx = F.linear(x2, p["weight_ih_l0"], p["bias_ih_l0"] + p["bias_hh_l0"])
    y2, h2, c2 = LF.lnlstm_ref(gx, p["weight_hh_l0"], h0=s2[0], c0=s2[1])
    ((y2 * w).sum() + (h2 * wh).sum() + (c2 * wc).sum()).backward()
    tol = dict(atol=1e-12, rtol=1e-12)
    np.testing.assert_allclose(y2.detach().numpy(), y1.detach().numpy(), **tol)
    np.testing.assert_allclose(h2.detach().numpy(), h1[0].detach().numpy(), **tol)
    np.testing.assert_allclose(c2.detach().numpy(), c1[0].detach().numpy(), **tol)
    np.testing.assert_allclose(x2.grad.numpy(), x1.grad.numpy(), **tol)
    for k, v in ref.named_parameters():
        np.testing.assert_allclose(p[k].grad.numpy(), v.grad.numpy(), err_msg=k, **tol)
    if state:
        for a, b in zip(s2, s1):
            np.testing.assert_allclose(a.grad.numpy(), b.grad[0].numpy(), **tol)


def test_with_layer_norm_gradcheck():
    H, T, B = 4, 3, 2
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    args = [rn(T, B, 4 * H), rn(4 * H, H) / 2, 1 + 0.2 * rn(4 * H), 0.2 * rn(4 * H),
            1 + 0.2 * rn(H), 0.2 * rn(H)]
    args = [a.requires_grad_(True) for a in args]
    h0, c0 = rn(B, H).requires_grad_(True), rn(B, H).requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda gx, wp, gg, gb, cg, cb, h, c: LF.lnlstm_ref(gx, wp, gg, gb, cg, cb, 1e-3, h, c),
        args + [h0, c0], eps=1e-6, atol=1e-7, rtol=1e-6)


def test_with_layer_norm_agrees_with_the_oracle_predictor():
    """One layer of oracle.heads.lstm_predictor in float64: the restatement is fed the oracle's
    normalised embedding through x2g, then the same output Linear and LayerNorm."""
    V, E, H, D, B, U = 11, 6, 8, 10, 3, 5
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    pfx, l0 = "p.", "p.lstm_layers.0."
    sd = {pfx + "embedding.weight": rn(V, E),
          pfx + "input_layer_norm.weight": 1 + 0.2 * rn(E), pfx + "input_layer_norm.bias": 0.2 * rn(E),
          l0 + "x2g.weight": rn(4 * H, E) / E ** 0.5, l0 + "p2g.weight": rn(4 * H, H) / H ** 0.5,
          l0 + "g_norm.weight": 1 + 0.2 * rn(4 * H), l0 + "g_norm.bias": 0.2 * rn(4 * H),
          l0 + "c_norm.weight": 1 + 0.2 * rn(H), l0 + "c_norm.bias": 0.2 * rn(H),
          pfx + "linear.weight": rn(D, H) / H ** 0.5, pfx + "linear.bias": 0.2 * rn(D),
          pfx + "output_layer_norm.weight": 1 + 0.2 * rn(D), pfx + "output_layer_norm.bias": 0.2 * rn(D)}
    lab = torch.randint(1, V, (B, U), generator=g)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # the oracle creates its zero state in the default type
    try:
        yo = OH.lstm_predictor(sd, pfx, lab, 1, True, 1e-3)
    finally:
        torch.set_default_dtype(prev)
    assert yo.dtype == torch.float64
    tok = torch.cat((torch.zeros(B, 1, dtype=torch.int64), lab), dim=1)
    x = F.layer_norm(F.embedding(tok.t(), sd[pfx + "embedding.weight"]), (E,),
                     sd[pfx + "input_layer_norm.weight"], sd[pfx + "input_layer_norm.bias"])
    hs = LF.lnlstm_stack_ref(x, [dict(x2g_w=sd[l0 + "x2g.weight"], wp=sd[l0 + "p2g.weight"],
                                      gg=sd[l0 + "g_norm.weight"], gb=sd[l0 + "g_norm.bias"],
                                      cg=sd[l0 + "c_norm.weight"], cb=sd[l0 + "c_norm.bias"], eps=1e-3)])
    y = F.layer_norm(F.linear(hs, sd[pfx + "linear.weight"], sd[pfx + "linear.bias"]), (D,),
                     sd[pfx + "output_layer_norm.weight"], sd[pfx + "output_layer_norm.bias"])
    np.testing.assert_allclose(y.permute(1, 0, 2).numpy(), yo.numpy(), atol=1e-12, rtol=1e-12)


def test_stack_applies_the_keep_masks_after_every_layer():
    g = torch.Generator().manual_seed(4)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    T, B, E, H = 3, 2, 5, 4
    layers = [dict(x2g_w=rn(4 * H, E), x2g_b=rn(4 * H), wp=rn(4 * H, H)),
              dict(x2g_w=rn(4 * H, H), x2g_b=rn(4 * H), wp=rn(4 * H, H))]
    x = rn(T, B, E)
    keep = [(torch.rand(T, B, H, generator=g) < 0.7).double() / 0.7 for _ in range(2)]
    y = LF.lnlstm_stack_ref(x, layers, keep)
    h1, _, _ = LF.lnlstm_ref(F.linear(x, layers[0]["x2g_w"], layers[0]["x2g_b"]), layers[0]["wp"])
    h2, _, _ = LF.lnlstm_ref(F.linear(h1 * keep[0], layers[1]["x2g_w"], layers[1]["x2g_b"]), layers[1]["wp"])
    assert torch.equal(y, h2 * keep[1])
    assert (y[keep[1] == 0] == 0).all()


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", list(LC.CASES))
def test_fp32_cost_of_the_reference(name):
    """lstm_f64.lnlstm_ref in float32 on the CPU against itself in float64, forward and backward.
    The figure is a maximum over a tensor at the end of a recurrence through two layer norms per
    step, and it moves with the host: 1.4 x between 1 and 16 threads of one CPU (matmul summation
    order), up to 2.9 x on a CPU with another vector maths library (H = 256, backward; even
    H = 4, where no matmul is involved, gave 1.4 x).  So the check is of the order of magnitude,
    both ways: the measurement within 4 x the record, and the record within 4 x the measurement
    (the GPU bounds are 8 x the record: a record far above what fp32 really costs would loosen
    them)."""
    ref = LC.reference(name)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    fwd, bwd = LC.fp32_figures(name)
    print(f"fp32 cost {name}: fwd={fwd:.3e} bwd={bwd:.3e}")
    rec = LC.FP32_COST[name]
    assert fwd <= 4 * rec["fwd"] and bwd <= 4 * rec["bwd"], (fwd, bwd, rec)
    assert rec["fwd"] <= 4 * fwd and rec["bwd"] <= 4 * bwd, (fwd, bwd, rec)


def test_case_inputs_are_what_the_table_says():
    for name, c in LC.CASES.items():
        t = LC.make(name)
        assert t["gx"].shape == (c["T"], c["B"], 4 * c["H"]) and t["gx"].dtype == torch.float32
        if c["ln"]:
            assert t["gg"][1] == 0 and t["gg"][2] < 0 and t["cg"][1] == 0 and t["cg"][2] < 0
        if c["spike"]:
            share = (t["gx"].abs() == c["spike"]).float().mean().item()
            assert 0.005 <= share <= 0.011 and t["gx"].max() == c["spike"] and t["gx"].min() == -c["spike"]
        assert (t["h0"] is not None) == c["state"]
    assert set(LC.CASES) == set(LC.FP32_COST)
