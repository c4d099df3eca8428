"""CPU tests of tests/zip_f64.py, the float64 yardstick of tests/test_gpu_zip_stream_kernels.py.

The restatements are pinned in float64 at 1e-12 before any kernel is compared with them: against
oracle.zipformer where the oracle states the operation (swoosh_l / swoosh_r, bias_norm, bypass,
simple_downsample, simple_upsample, _LimitParam, _Balancer), against plain torch autograd or an
index-by-index loop where it does not; torch.autograd.gradcheck on the differentiable ones.  The
Balancer's restatement (autograd through the loss) equals the closed form
zip_f64.balancer_bwd_closed_form on live channels and differs from it on a constant one, where the closed
form divides by the clamped variance.

The last part measures what float32 costs the REFERENCE on every case of tests/zip_cases.py: the
figures recorded in zip_cases.FP32_COST are checked here (to the factor by which they move from
host to host), so the GPU file's bounds (max(2e-5, 8 x figure)) cannot drift.
"""
import numpy as np
import pytest
import torch

import zip_cases as ZC
import zip_f64 as ZF
from oracle import zipformer as OZ
from yardstick import F64, _grads, _rn, _same

GC = dict(eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------ Swoosh
@pytest.mark.parametrize("is_l", [True, False])
def test_swoosh_ref_equals_the_oracle_and_its_closed_form_gradient(is_l):
    x = torch.cat((_rn(1)(500) * 4, torch.tensor(ZC.SAT, dtype=F64))).requires_grad_(True)
    y = ZF.swoosh_ref(x, is_l)
    _same(y, (OZ.swoosh_l if is_l else OZ.swoosh_r)(x.detach()))
    # and the form the kernel uses, which the restatement does not
    z = x.detach() - ZF.SWOOSH[is_l][0]
    _same(y, z.clamp(min=0) + torch.log1p(torch.exp(-z.abs())) - 0.08 * x.detach() - ZF.SWOOSH[is_l][1])
    y.sum().backward()
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    _same(x.grad, ZF.swoosh_grad_ref(x.detach(), is_l))
    x32 = x.detach().float()
    assert torch.isfinite(ZF.swoosh_ref(x32, is_l)).all() and torch.isfinite(ZF.swoosh_grad_ref(x32, is_l)).all()
    v = (_rn(2)(12) * 3).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: ZF.swoosh_ref(t, is_l), [v], **GC)


# ------------------------------------------------------------------ BiasNorm, bypass
def test_biasnorm_ref_equals_the_oracle():
    rn = _rn(3)
    x, b, ls = (rn(5, 7, 12) * 2 + 0.5).requires_grad_(True), rn(12).requires_grad_(True), rn(()).requires_grad_(True)
    g = rn(5, 7, 12)
    y, scales = ZF.biasnorm_ref(x, b, ls)
    ref = OZ.bias_norm(x, b, ls, OZ.Ctl())
    _same(y, ref)
    _same(scales, (y / x).detach().mean(-1))
    for a, r in zip(_grads(y, g, x, b, ls), _grads(ref, g, x, b, ls)):
        _same(a, r)
    # batch-major in, time-major out: the plain one plus a transpose
    yt, st = ZF.biasnorm_tb_ref(x, b, ls)
    assert yt.shape == (7, 5, 12) and st.shape == (5, 7)
    _same(yt, ref.transpose(0, 1))
    args = [v.requires_grad_(True) for v in (rn(3, 6) + 0.5, rn(6), rn(()))]
    assert torch.autograd.gradcheck(lambda *a: ZF.biasnorm_ref(*a), args, **GC)


def test_bypass_refs_equal_the_oracle():
    rn = _rn(4)
    T, B, C = 6, 3, 8
    o, s, k = (v.requires_grad_(True) for v in (rn(T, B, C), rn(T, B, C), torch.rand(C, dtype=F64)))
    g, fm, acc = rn(T, B, C), torch.rand(B, C, dtype=F64), rn(T, B, C)
    ref = OZ.bypass({"bypass_scale": k}, "", o, s, OZ.Ctl())
    out = ZF.bypass_ref(o, s, k)
    _same(out, ref)
    plain = _grads(ref, g, o, s, k)
    for a, r in zip(_grads(out, g, o, s, k), plain):
        _same(a, r)
    # the feature mask: a (B,C) factor on every frame, given per row as the kernels index it
    rows = ZC.fm_rows(fm, T * B).view(T, B, C)
    _same(rows, fm.expand(T, B, C))
    outm = ZF.bypass_ref(o, s, k, rows)
    _same(outm, ref * fm)
    for a, r in zip(_grads(outm, g, o, s, k), _grads(ref * fm, g, o, s, k)):
        _same(a, r)
    # acc_in: d_orig receives it, nothing else moves
    out2, extra = ZF.bypass_acc_ref(o, s, k, acc)
    for v in (o, s, k):
        v.grad = None
    ((out2 * g).sum() + extra).backward()
    _same(o.grad, plain[0] + acc)
    _same(s.grad, plain[1])
    _same(k.grad, plain[2])
    # BiasNorm + bypass + feature mask is the composition
    x, b, ls = (rn(T, B, C) + 0.5).requires_grad_(True), rn(C).requires_grad_(True), rn(()).requires_grad_(True)
    comp = OZ.bypass({"bypass_scale": k}, "", o, OZ.bias_norm(x, b, ls, OZ.Ctl()), OZ.Ctl()) * fm
    fused, scales = ZF.norm_bypass_ref(x, b, ls, o, k, rows)
    _same(fused, comp)
    _same(scales, ZF.biasnorm_ref(x, b, ls)[1])
    for a, r in zip(_grads(fused, g, x, b, ls, o, k), _grads(comp, g, x, b, ls, o, k)):
        _same(a, r)
    args = [v.requires_grad_(True) for v in (rn(2, 2, 4) + 0.5, rn(4), rn(()), rn(2, 2, 4), torch.rand(4, dtype=F64))]
    fm2 = rn(2, 4)
    assert torch.autograd.gradcheck(lambda *a: ZF.norm_bypass_ref(*a, fm=fm2)[0], args, **GC)


# ------------------------------------------------------------------ resampling
@pytest.mark.parametrize("ds,T", [(1, 3), (2, 1), (2, 7), (4, 3), (4, 4), (4, 13), (8, 9)])
def test_downsample_ref_equals_the_oracle(ds, T):
    rn = _rn(ds + T)
    src, bias, g = rn(T, 2, 3).requires_grad_(True), rn(ds).requires_grad_(True), rn((T + ds - 1) // ds, 2, 3)
    ref = OZ.simple_downsample(src, bias, ds)
    out = ZF.downsample_ref(src, bias.softmax(0), ds)
    _same(out, ref)
    for a, r in zip(_grads(out, g, src, bias), _grads(ref, g, src, bias)):
        _same(a, r)
    _same(ZF.downsample_ref(src, bias.softmax(0), ds, True), ref.transpose(0, 1))
    w = torch.rand(ds, dtype=F64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda s, ww: ZF.downsample_ref(s, ww, ds), [src, w], **GC)


@pytest.mark.parametrize("up,T", [(2, 10), (2, 7), (4, 9), (8, 15), (4, 3), (8, 1), (3, 10)])
def test_upsample_bypass_ref_equals_the_oracle(up, T):
    rn = _rn(up + T)
    Ts = (T + up - 1) // up
    o, s, k = (v.requires_grad_(True) for v in (rn(T, 2, 4), rn(Ts, 2, 4), torch.rand(4, dtype=F64)))
    g = rn(T, 2, 4)
    ref = OZ.bypass({"bypass_scale": k}, "", o, OZ.simple_upsample(s, up)[:T], OZ.Ctl())
    out = ZF.upsample_bypass_ref(o, s, k, up)
    _same(out, ref)
    for a, r in zip(_grads(out, g, o, s, k), _grads(ref, g, o, s, k)):
        _same(a, r)
    assert torch.autograd.gradcheck(lambda *a: ZF.upsample_bypass_ref(*a, up), [o, s, k], **GC)


# ------------------------------------------------------------------ nonlinear attention and glue
def test_nonlin_refs_equal_an_index_by_index_loop():
    rn = _rn(5)
    T, B, C = 4, 3, 5
    u, z = rn(T, B, 3 * C).requires_grad_(True), rn(B, T, C).requires_grad_(True)
    xs, o = ZF.nonlin_gate_ref(u), ZF.nonlin_out_ref(z, u)
    assert xs.shape == (B, T, C) and o.shape == (T, B, C)
    xv, ov, uv, zv = (v.detach().numpy() for v in (xs, o, u, z))
    for t in range(T):
        for b in range(B):
            for c in range(C):
                assert abs(xv[b, t, c] - uv[t, b, C + c] * np.tanh(uv[t, b, c])) < 1e-12
                assert abs(ov[t, b, c] - zv[b, t, c] * uv[t, b, 2 * C + c]) < 1e-12
    # the gradients in the closed forms the kernels state
    dxs, g = rn(B, T, C), rn(T, B, C)
    ((xs * dxs).sum() + (o * g).sum()).backward()
    s, x, y = u.detach().chunk(3, -1)
    d = dxs.transpose(0, 1)
    _same(u.grad, torch.cat((d * x * (1 - torch.tanh(s) ** 2), d * torch.tanh(s), g * z.detach().transpose(0, 1)), -1))
    _same(z.grad, (g * y).transpose(0, 1))
    assert torch.autograd.gradcheck(ZF.nonlin_gate_ref, [u], **GC)
    assert torch.autograd.gradcheck(ZF.nonlin_out_ref, [z, u], **GC)


def test_attn_delta_pairs_ref_equals_softmax_backwards_row_constant():
    """delta = sum_j W dW over the row, where dW collects what every consumer of the attention weights
    sends back: O = W V per consumer gives dW = dO V^T, so sum_j W dW = sum_d dO O; head 0 also feeds
    the nonlinear attention, whose dW0 arrives as a matrix."""
    rn = _rn(6)
    T, B, H, dv1, dv2 = 5, 2, 3, 4, 2
    W = rn(H, B, T, T).softmax(-1)
    V1, V2, dW0 = rn(H, B, T, dv1), rn(H, B, T, dv2), rn(B, T, T)
    dO1, dO2 = rn(T, B, H * dv1), rn(T, B, H * dv2)
    lay = lambda o: o.permute(2, 1, 0, 3).reshape(T, B, -1)          # noqa: E731  (H,B,T,dv) -> (T,B,H dv)
    unl = lambda d, dv: d.reshape(T, B, H, dv).permute(2, 1, 0, 3)   # noqa: E731
    O1, O2 = lay(W @ V1), lay(W @ V2)
    dW = unl(dO1, dv1) @ V1.transpose(-1, -2) + unl(dO2, dv2) @ V2.transpose(-1, -2)
    dW[0] += dW0
    _same(ZF.attn_delta_pairs_ref(W, dW0, [(dO1, O1), (dO2, O2)], T, B, H), (W * dW).sum(-1))
    dW[0] -= dW0
    _same(ZF.attn_delta_pairs_ref(W, None, [(dO1, O1), (dO2, O2)], T, B, H), (W * dW).sum(-1))
    _same(ZF.attn_delta_pairs_ref(W, None, [(dO1, O1)], T, B, H), (W * (unl(dO1, dv1) @ V1.transpose(-1, -2))).sum(-1))


@pytest.mark.parametrize("limit", [True, False])
def test_commit_ref_equals_the_oracles_limit_param(limit):
    rn = _rn(7)
    x, d, grad = rn(400).requires_grad_(True), rn(400), rn(400)
    new, cleared = ZF.commit_ref(x.detach(), d, grad, ZC.LO, ZC.HI, limit)
    y = OZ._LimitParam.apply(x, ZC.LO, ZC.HI) if limit else x
    y.backward(d)
    _same(new, grad + x.grad)
    assert (cleared == 0).all()
    below, above = x.detach() < ZC.LO, x.detach() > ZC.HI
    for m in (below, above, ~below & ~above):          # every region with both signs of d
        assert bool((d[m] > 0).any()) and bool((d[m] < 0).any())
    assert bool((x.grad != d).any()) == limit


def test_add_ref():
    rn = _rn(8)
    a, b = rn(9), rn(9)
    _same(ZF.add_ref(a, b), torch.stack((a, b)).sum(0))


# ------------------------------------------------------------------ Balancer
def _bal_x(rn, rows, C):
    """Channels on both sides of every clamp, as the cases have them."""
    mu = torch.tensor([ZC.BAL_MU[i % len(ZC.BAL_MU)] for i in range(C)], dtype=F64)
    sd = torch.tensor([ZC.BAL_SD[i % len(ZC.BAL_SD)] for i in range(C)], dtype=F64)
    return (ZC._standardised(rn(rows, C)) + mu) * sd


@pytest.mark.parametrize("swoosh", [None, True, False])
def test_balancer_ref_equals_the_oracle_and_the_closed_form_on_live_channels(monkeypatch, swoosh):
    rn = _rn(9)
    x, g = _bal_x(rn, 50, 24), rn(50, 24)
    out = ZF.balancer_bwd_ref(x, g, *ZC.BAL_CFG, swoosh=swoosh)
    ge = g if swoosh is None else g * ZF.swoosh_grad_ref(x, swoosh)
    # the oracle's own backward, with its cast to float32 switched off so that it runs in float64
    monkeypatch.setattr(torch.Tensor, "float", lambda self: self)
    xo = x.clone().requires_grad_(True)
    OZ._Balancer.apply(xo, *ZC.BAL_CFG, -1).backward(ge)
    monkeypatch.undo()
    assert xo.grad.dtype == F64
    _same(out, xo.grad)
    assert float((out - ge).abs().max()) > 1e-3 * float(out.abs().max())        # the update is really there
    cf = ZF.balancer_bwd_closed_form(x, g, *ZC.BAL_CFG, swoosh if swoosh is None else bool(swoosh))
    if swoosh is not False:           # (the closed form of that file knows SwooshL only)
        np.testing.assert_allclose(out.numpy(), cf.numpy(), atol=1e-12 * float(out.abs().max()), rtol=1e-9)
    # channels on both sides of every clamp
    m = x.mean(0) / x.std(0, unbiased=False)
    rms = (x * x).mean(0).sqrt()
    lo_m, hi_m, lo_r, hi_r, _ = ZC.BAL_CFG
    for cond in (m < lo_m, m > hi_m, (m > lo_m) & (m < hi_m), rms < lo_r, rms > hi_r, (rms > lo_r) & (rms < hi_r)):
        assert bool(cond.any())


def test_balancer_ref_and_the_closed_form_differ_on_a_constant_channel():
    """A constant channel has E[x^2] - mean^2 at the 1e-20 clamp: autograd sees a constant there
    (derivative zero), so the loss gradient is s_m / (n std) and the update is +-grad_scale |g|.  The
    closed form multiplies by 1 / (std var) = 1e30 and cancels it again in float64 rounding noise.
    An all-zero channel gets no update from either."""
    rn = _rn(10)
    x, g = _bal_x(rn, 64, 6), rn(64, 6)
    x[:, 1] = 0.75
    x[:, 2] = 0.0
    out = ZF.balancer_bwd_ref(x, g, *ZC.BAL_CFG)
    cf = ZF.balancer_bwd_closed_form(x, g, *ZC.BAL_CFG, None)
    _same(out[:, 1], g[:, 1] + ZC.BAL_CFG[4] * g[:, 1].abs())       # mean / std = +inf side: s_m = +1
    _same(out[:, 2], g[:, 2])
    live = [0, 3, 4, 5]
    np.testing.assert_allclose(out[:, live].numpy(), cf[:, live].numpy(), atol=1e-12, rtol=1e-9)
    d = (cf[:, 1] - out[:, 1]).abs().max()
    assert not torch.isfinite(d) or float(d) > 1e-3 * float(g[:, 1].abs().max()), float(d)


def test_balancer_ref_gradcheck_of_its_inner_loss_is_what_it_applies():
    """The update direction is d loss / dx of the Balancer's loss, normalised per channel."""
    rn = _rn(11)
    x, g = _bal_x(rn, 9, 6), rn(9, 6)
    lo_m, hi_m, lo_r, hi_r, gs = ZC.BAL_CFG

    def loss(xx):
        uvar, mean = (xx ** 2).mean(0), xx.mean(0)
        m = mean / (uvar - mean * mean).sqrt()
        return ((m - m.clamp(lo_m, hi_m)).abs() + (uvar.sqrt().clamp(lo_r, hi_r) / uvar.sqrt()).log().abs()).sum()

    xx = x.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(loss, [xx], **GC)
    lg, = torch.autograd.grad(loss(xx), xx)
    lg = lg * (gs / (lg ** 2).mean(0).sqrt().clamp(min=1e-20))
    _same(ZF.balancer_bwd_ref(x, g, *ZC.BAL_CFG), g + g.abs() * lg)


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", list(ZC.CASES))
def test_fp32_cost_of_the_reference(name):
    """The yardstick in float32 on the CPU against itself in float64, per output tensor.  A figure
    is a maximum over a tensor and moves with the host (tests/test_conf_f64.py), so the check is of
    the order of magnitude, both ways: the measurement within 4 x the record, and the record within
    4 x the measurement (the GPU bounds are 8 x the record: a record far above what float32 really
    costs would loosen them).  Both are raised to one float32 rounding (zip_cases.UNIT) first."""
    ref = ZC.reference(name)
    for k, v in ref.items():
        for w in (v if isinstance(v, list) else [v]):
            assert torch.isfinite(w).all(), k
    fig = ZC.fp32_figures(name)
    rec = ZC.FP32_COST[name]
    print(f"fp32 cost {name}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    assert set(fig) == set(rec), (sorted(fig), sorted(rec))
    for k in fig:
        f, r = max(fig[k], ZC.UNIT), max(rec[k], ZC.UNIT)
        assert f <= 4 * r and r <= 4 * f, (name, k, fig[k], rec[k])


def test_case_inputs_are_what_the_table_says():
    assert set(ZC.CASES) == set(ZC.FP32_COST)
    assert len({c["seed"] for c in ZC.CASES.values()}) == len(ZC.CASES)
    lo_m, hi_m, lo_r, hi_r, _ = ZC.BAL_CFG
    for name in ZC.names("bal"):
        c, x = ZC.CASES[name], ZC.make(name)["x"].double()
        k = ZC.bal_kappa(name)
        assert 1.0 <= k <= 65.0, (name, k)
        if c["rows"] >= 3 and c["C"] >= 42 and c["kind"] == "plain":     # every (mean / std, rms) pairing
            m, rms = x.mean(0) / x.std(0, unbiased=False), (x * x).mean(0).sqrt()
            for cond in (m < lo_m, m > hi_m, (m > lo_m) & (m < hi_m), rms < lo_r, rms > hi_r,
                         (rms > lo_r) & (rms < hi_r)):
                assert bool(cond.any()), name
            # and none within float32's reach of a clamp, where the sign of the update would be luck
            assert float(torch.stack(((m - lo_m).abs(), (m - hi_m).abs())).min()) > 1e-3
            assert float(torch.stack(((rms - lo_r).abs(), (rms - hi_r).abs())).min()) > 1e-3
    assert ZC.bal_kappa("bal_offset8") > 64.0
    for name in ("bal_dead_gen", "bal_dead_small"):
        x = ZC.make(name)["x"]
        assert bool((x[:, 1] == 0.5).all()) and bool((x[:, 2] == 0).all())
        ref = ZC.reference(name)["upd"]
        g = ZC.make(name)["g"].double()
        _same(ref[:, 1], ZC.BAL_CFG[4] * g[:, 1].abs())
        assert bool((ref[:, 2] == 0).all())
    assert abs(float(ZC.make("bn_offset")["x"].mean()) - 100) < 0.1
    assert not ZC.make("bn_zerog")["g"].any()
    assert not ZC.make("nb_fmzero")["fm"][2].any()
    for name in ("sw_sat_l", "sw_sat_r", "sw_sat100_l", "sw_sat100_r"):
        t, c = ZC.make(name), ZC.CASES[name]
        assert sorted(t["x"][t["sat_idx"]].tolist()) == sorted(list(c["sat"]) * 4)
    assert float(ZC.make("nl_sat")["u"][..., :64].abs().max()) == 20.0
    for name in ("sw_overcap", "add_overcap"):
        assert ZC.CASES[name]["n"] // 4 > ZC.STREAM_CAP
    assert ZC.CASES["by_overcap"]["rows"] > ZC.STREAM_CAP
    c = ZC.CASES["nl_overcap"]
    assert c["T"] * c["B"] * c["C"] > ZC.STREAM_CAP
    for it, lim in zip(ZC.make("cm_n8")["items"][3:4], (0,)):
        x, d = it["x"], it["d"]
        for m in (x < ZC.LO, x > ZC.HI, (x > ZC.LO) & (x < ZC.HI)):
            assert bool((d[m] > 0).any()) and bool((d[m] < 0).any())
