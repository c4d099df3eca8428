"""CPU tests of tests/conf_f64.py, the float64 yardstick of tests/test_gpu_conf_kernels.py.

The restatements are pinned against torch in float64 at 1e-12 before any kernel is compared with
them: layernorm_ref against F.layer_norm, bn_silu_ref against torch.nn.BatchNorm1d (training with
the running statistics after one and two batches, momentum 0.1 and None, and evaluation), attn_ref
against F.scaled_dot_product_attention and, with a keep mask, against oracle.conformer's
_mha_dropout; torch.autograd.gradcheck on one tiny shape each.

The last part measures what float32 costs the REFERENCE on every case of tests/conf_cases.py: the
figures recorded in conf_cases.FP32_COST are checked here (to the factor by which they move from
host to host), so the GPU file's bounds (max(2e-5, 8 x figure)) cannot drift.
"""
import pytest
import torch
import torch.nn.functional as F

import conf_cases as CC
import conf_f64 as CF
from oracle import conformer as OC
from yardstick import F64, _rn, _same


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows,C,add", [(5, 4, False), (7, 36, True), (3, 260, True)])
def test_layernorm_ref_equals_torch(rows, C, add):
    rn = _rn(rows + C)
    x, y, g, b = (v.requires_grad_(True) for v in (rn(rows, C) * 2 + 0.5, rn(rows, C), rn(C), rn(C)))
    dy = rn(rows, C)
    xsum, out = CF.layernorm_ref(x, y if add else None, 0.5, g, b, 1e-5)
    (out * dy).sum().backward()
    x2, y2, g2, b2 = (v.detach().clone().requires_grad_(True) for v in (x, y, g, b))
    xin = x2 + 0.5 * y2 if add else x2
    ref = F.layer_norm(xin, (C,), g2, b2, 1e-5)
    (ref * dy).sum().backward()
    _same(out, ref, "out")
    _same(xsum, xin, "xsum")
    for a, r, k in ((x, x2, "dx"), (g, g2, "dgamma"), (b, b2, "dbeta")) + (((y, y2, "dy"),) if add else ()):
        _same(a.grad, r.grad, k)
    mean, rstd = CF.layernorm_stats(xin.detach(), 1e-5)
    _same(mean, xin.detach().mean(-1), "mean")
    _same(rstd, 1 / torch.sqrt(xin.detach().var(-1, unbiased=False) + 1e-5), "rstd")
    # without the affine parameters
    _same(CF.layernorm_ref(x, None, 0.0, None, None, 1e-5)[1], F.layer_norm(x, (C,), None, None, 1e-5))
    _same(CF.layernorm_ref(x, None, 0.0, g, None, 1e-5)[1], F.layer_norm(x, (C,), g, None, 1e-5))


def test_layernorm_ref_gradcheck():
    rn = _rn(1)
    args = [v.requires_grad_(True) for v in (rn(3, 8), rn(3, 8), rn(8), rn(8))]
    assert torch.autograd.gradcheck(lambda x, y, g, b: CF.layernorm_ref(x, y, 0.5, g, b, 1e-3), args,
                                    eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------ SiLU
def test_silu_ref_equals_torch_and_its_closed_form_gradient():
    x = torch.cat((_rn(2)(500) * 4, torch.tensor(CC.SAT, dtype=F64))).requires_grad_(True)
    a = CF.silu_ref(x)
    _same(a, F.silu(x.detach()))
    a.sum().backward()
    assert torch.isfinite(x.grad).all() and torch.isfinite(a).all()
    _same(x.grad, CF.silu_grad_ref(x.detach()))
    x32 = x.detach().float()
    assert torch.isfinite(CF.silu_ref(x32)).all() and torch.isfinite(CF.silu_grad_ref(x32)).all()
    y = (_rn(3)(12) * 3).requires_grad_(True)
    assert torch.autograd.gradcheck(CF.silu_ref, [y], eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------ BatchNorm + SiLU
@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("rows,C", [(2, 4), (19, 12)])
def test_bn_silu_ref_equals_torch_batchnorm(rows, C, momentum):
    rn = _rn(rows + C)
    bn = torch.nn.BatchNorm1d(C, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(rn(C)); bn.bias.copy_(rn(C))
        bn.running_mean.copy_(rn(C)); bn.running_var.copy_(rn(C).abs() + 0.5)
    g, b = bn.weight.detach().clone().requires_grad_(True), bn.bias.detach().clone().requires_grad_(True)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for i in range(2):
        x = (rn(rows, C) * 1.7 + rn(C)).requires_grad_(True)
        ds = rn(rows, C)
        bn.zero_grad()
        ref = F.silu(bn(x))
        (ref * ds).sum().backward()
        x2 = x.detach().clone().requires_grad_(True)
        g.grad = b.grad = None
        y, mean, var, unb = CF.bn_silu_ref(x2, g, b, bn.eps)
        (y * ds).sum().backward()
        mom = 1.0 / (i + 1) if momentum is None else momentum
        rm = (1 - mom) * rm + mom * mean.detach()
        rv = (1 - mom) * rv + mom * unb.detach()
        _same(y, ref, f"y, batch {i}")
        _same(x2.grad, x.grad, "dx"); _same(g.grad, bn.weight.grad, "dgamma"); _same(b.grad, bn.bias.grad, "dbeta")
        _same(rm, bn.running_mean, f"running_mean after batch {i}")
        _same(rv, bn.running_var, f"running_var after batch {i}")
        _same(var, x.detach().var(0, unbiased=False), "biased variance")
    assert int(bn.num_batches_tracked) == 2
    bn.eval()
    xe = rn(rows, C)
    _same(CF.bn_silu_eval_ref(xe, rm, rv, g.detach(), b.detach(), bn.eps), F.silu(bn(xe)), "eval")
    # without running statistics the batch's own are used in evaluation as well
    bn2 = torch.nn.BatchNorm1d(C, track_running_stats=False).double().eval()
    with torch.no_grad():
        bn2.weight.copy_(g); bn2.bias.copy_(b)
    _same(CF.bn_silu_ref(xe, g.detach(), b.detach(), bn2.eps)[0], F.silu(bn2(xe)), "eval, no tracking")


def test_bn_silu_ref_gradcheck():
    rn = _rn(5)
    args = [v.requires_grad_(True) for v in (rn(6, 4) + rn(4), rn(4), rn(4))]
    assert torch.autograd.gradcheck(lambda x, g, b: CF.bn_silu_ref(x, g, b, 1e-3)[0], args,
                                    eps=1e-6, atol=1e-7, rtol=1e-6)
    ev = [v.requires_grad_(True) for v in (rn(6, 4), rn(4), rn(4).abs() + 0.5, rn(4), rn(4))]
    assert torch.autograd.gradcheck(lambda x, m, v, g, b: CF.bn_silu_eval_ref(x, m, v, g, b, 1e-3), ev,
                                    eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------ attention
@pytest.mark.parametrize("T,B,H,dh,lens", [(9, 2, 2, 4, None), (13, 3, 2, 8, (13, 5, 1)), (6, 2, 1, 4, (9, 3))])
def test_attn_ref_equals_torch_attention(T, B, H, dh, lens):
    rn = _rn(T + B)
    D = H * dh
    qkv = rn(T, B, 3 * D).requires_grad_(True)
    do = rn(T, B, D)
    lt = None if lens is None else torch.tensor(lens)
    o = CF.attn_ref(qkv, lt, H)
    (o * do).sum().backward()
    q2 = qkv.detach().clone().requires_grad_(True)
    q, k, v = (t.reshape(T, B, H, dh).permute(1, 2, 0, 3) for t in q2.chunk(3, dim=-1))
    mask = None if lt is None else (torch.arange(T)[None, :] < lt[:, None])[:, None, None, :]
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=mask).permute(2, 0, 1, 3).reshape(T, B, D)
    (ref * do).sum().backward()
    _same(o, ref, "o")
    _same(qkv.grad, q2.grad, "dqkv")
    # and against nn.MultiheadAttention with identity projections
    mha = torch.nn.MultiheadAttention(D, H, bias=False).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(D, dtype=F64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(D, dtype=F64))
    x = rn(T, B, D)
    kpm = None if lt is None else torch.arange(T)[None, :] >= lt[:, None]
    _same(CF.attn_ref(torch.cat((x, x, x), -1), lt, H), mha(x, x, x, key_padding_mask=kpm, need_weights=False)[0])


def test_attn_ref_gives_zeros_for_an_empty_utterance():
    rn = _rn(7)
    T, B, H, dh = 5, 3, 2, 4
    qkv = rn(T, B, 3 * H * dh).requires_grad_(True)
    lens = torch.tensor([5, 0, 2])
    o = CF.attn_ref(qkv, lens, H)
    (o * rn(T, B, H * dh)).sum().backward()
    assert torch.isfinite(o).all() and torch.isfinite(qkv.grad).all()
    assert (o[:, 1] == 0).all() and (qkv.grad[:, 1] == 0).all()
    assert (o[:, 0] != 0).all() and (qkv.grad[:, 2] != 0).any()
    # the other utterances are what they are alone
    _same(o[:, [0, 2]], CF.attn_ref(qkv.detach()[:, [0, 2]], lens[[0, 2]], H))


def test_attn_ref_with_a_mask_equals_the_oracles_dropout_attention():
    rn = _rn(8)
    T, B, H, dh, p, seed = 7, 2, 2, 4, 0.3, 99
    D = H * dh
    y = rn(T, B, D)
    sd = {"self_attn.in_proj_weight": rn(3 * D, D) / D ** 0.5, "self_attn.in_proj_bias": rn(3 * D),
          "self_attn.out_proj.weight": torch.eye(D, dtype=F64), "self_attn.out_proj.bias": torch.zeros(D, dtype=F64)}
    lens = torch.tensor([7, 4])
    kpm = torch.arange(T)[None, :] >= lens[:, None]
    ref = OC._mha_dropout(sd, "", y, H, kpm, OC._Drop(p, [seed]))
    qkv = F.linear(y, sd["self_attn.in_proj_weight"], sd["self_attn.in_proj_bias"])
    mask = OC.keep_scale(seed, (B, H, T, T), p).double()
    assert 0 < (mask == 0).double().mean() < 1
    _same(CF.attn_ref(qkv, lens, H, mask), ref)


def test_attn_ref_gradcheck():
    rn = _rn(9)
    T, B, H, dh = 4, 2, 2, 2
    qkv = rn(T, B, 3 * H * dh).requires_grad_(True)
    mask = OC.keep_scale(5, (B, H, T, T), 0.25).double()
    assert torch.autograd.gradcheck(lambda q: CF.attn_ref(q, torch.tensor([4, 2]), H, mask), [qkv],
                                    eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", list(CC.CASES))
def test_fp32_cost_of_the_reference(name):
    """The yardstick in float32 on the CPU against itself in float64, per output tensor.  A figure
    is a maximum over a tensor and moves with the host (summation order of the CPU's reductions and
    matmuls, its vector maths library); tests/test_lstm_f64.py measured up to 2.9 x between hosts.
    So the check is of the order of magnitude, both ways: the measurement within 4 x the record,
    and the record within 4 x the measurement (the GPU bounds are 8 x the record: a record far above
    what float32 really costs would loosen them).  Both are raised to one float32 rounding (conf_cases.UNIT) first:
    below it a figure is luck of the rounding, not cost."""
    ref = CC.reference(name)
    for k, v in ref.items():
        for w in (v if isinstance(v, list) else [v]):
            assert torch.isfinite(w).all(), k
    fig = CC.fp32_figures(name)
    rec = CC.FP32_COST[name]
    print(f"fp32 cost {name}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    assert set(fig) == set(rec), (sorted(fig), sorted(rec))
    for k in fig:
        f, r = max(fig[k], CC.UNIT), max(rec[k], CC.UNIT)
        assert f <= 4 * r and r <= 4 * f, (name, k, fig[k], rec[k])


def test_case_inputs_are_what_the_table_says():
    assert set(CC.CASES) == set(CC.FP32_COST)
    for name in CC.names("bn"):
        assert CC.bn_mean_over_std(name) <= 8.0, name
        assert 1.0 <= CC.bn_kappa(name) <= 65.0, name
    assert CC.bn_mean_over_std("bn_offset8") > 7.9
    t = CC.make("ln_constrow")
    assert t["x"][18].unique().numel() == 1 and t["y"][18].unique().numel() == 1
    assert abs(float(CC.make("ln_offset")["x"].mean()) - 100) < 0.1
    for name in ("silu_sat", "silu_sat100"):
        t, c = CC.make(name), CC.CASES[name]
        assert sorted(t["h"][t["sat_idx"]].tolist()) == sorted(list(c["sat"]) * 4)
    q = CC.make("attn_peaky")
    D = q["qkv"].shape[-1] // 3
    T, B = q["qkv"].shape[:2]
    qq, kk = (q["qkv"][..., i * D:(i + 1) * D].reshape(T, B, 2, 32).double() for i in range(2))
    s = torch.einsum("tbhd,sbhd->bhts", qq, kk) / 32 ** 0.5
    assert 59 < float(s.abs().max()) < 61
    last = (s.argmax(-1) == T - 3).float().mean()
    assert 0.4 < last < 0.6, last                       # the maximum in the last tile, and elsewhere
    for name in CC.names("attn"):
        c = CC.CASES[name]
        assert (c["dh"] in (16, 32, 64)) == c["kernel"]
    assert CC.CASES["silu_overcap"]["n"] // 4 > CC.STREAM_CAP
    assert CC.CASES["bn_overcap"]["rows"] * 256 // 4 > CC.STREAM_CAP
