"""GPU: the conformer block's kernels (csrc/conf_elem.hip: LayerNorm forward / backward / fold, SiLU,
the hashed dropout passes, BatchNorm + SiLU; csrc/conf_attn.hip: flash-style MHSA forward, dQ and
dK / dV) called through the C ABI on device buffers of the test's own, against the float64 yardstick
tests/conf_f64.py, at every dispatch edge (tests/conf_cases.py names why each shape is there).

Error = max |got - ref| / max |ref| per tensor; allowed = conf_cases.bound(case, tensor) =
max(2e-5, 8 x the case's float32 figure of the YARDSTICK, asserted by tests/test_conf_f64.py).
Every buffer a kernel writes is a guarded buffer of tests/guarded.py holding the sentinel SENT, with a
guard of at least one row of SENT behind it, which must be intact afterwards (the LayerNorm partial sums and statistics, the BatchNorm save vectors, running
statistics and workspace included): an over-run shows here, without any sanitizer.
"""
import functools
import math

import pytest
import torch

import conf_cases as CC
import guarded
from guarded import SENT, env, hold
from oracle import conformer as OC

pytestmark = pytest.mark.gpu

Buf = functools.partial(guarded.Buf, fill=SENT)


def _hold(name, got, ref=None):
    """guarded.hold on tensors that already have the reference's shapes: this file hands every tensor over
    in the yardstick's own layout, so a reshape would hide a mistake of the test's."""
    ref = CC.reference(name) if ref is None else ref
    for k, v in got.items():
        if k in ref and not isinstance(v, list):
            assert v.shape == ref[k].shape, (name, k, v.shape, ref[k].shape)
    hold(CC, name, got, ref=ref)


# ------------------------------------------------------------------ LayerNorm
def _ln_forward(dev, x, y, gamma, beta):
    """-> (xsum | None, out, stats) in guarded buffers."""
    N, lib, st = env()
    R, C = x.shape
    out, stats = Buf(dev, (R, C)), Buf(dev, (R, 2))
    xsum = Buf(dev, (R, C)) if y is not None else None
    N.check(lib.s2t_layernorm_fwd(N.fp(x), N.fp(y), 0.5, N.fp(gamma), N.fp(beta), R, C, CC.EPS,
                                  N.fp(xsum.t) if xsum else None, N.fp(out.t), N.fp(stats.t), st),
            "s2t_layernorm_fwd")
    return xsum, out, stats


def _ln_backward(dev, x, stats, gamma, dy, resid):
    """-> (dx, partial) in guarded buffers; partial is (workgroups, 2C)."""
    N, lib, st = env()
    R, C = x.shape
    nwg = lib.s2t_layernorm_bwd_partial_floats(R, C) // (2 * C)
    dx, partial = Buf(dev, (R, C)), Buf(dev, (nwg, 2 * C))
    N.check(lib.s2t_layernorm_bwd(N.fp(x), N.fp(stats), N.fp(gamma), N.fp(dy), N.fp(resid), R, C,
                                  N.fp(dx.t), N.fp(partial.t), st), "s2t_layernorm_bwd")
    return dx, partial


@pytest.mark.parametrize("name", CC.names("ln"))
def test_layernorm_forward_backward_vs_float64(dev, name):
    """Forward without and with the fused add (alpha 0.5), backward without and with resid, the
    parameter gradients through the fold."""
    from speech2text_amd import conf_kernels as ck
    c = CC.CASES[name]
    R, C = c["rows"], c["C"]
    t = {k: v.to(dev) for k, v in CC.make(name).items()}
    got = {}
    for add in (False, True):
        sfx = "_add" if add else ""
        xsum, out, stats = _ln_forward(dev, t["x"], t["y"] if add else None, t["gamma"], t["beta"])
        xs = xsum.t if add else t["x"]
        dx, partial = _ln_backward(dev, xs, stats.t, t["gamma"], t["dy"], t["resid"] if add else None)
        grads = Buf(dev, (2, C), src=torch.zeros(2, C))
        ck.ln_param_grad([(partial.t, R, grads.t[0], grads.t[1])], C)
        torch.cuda.synchronize()
        for g, what in ((out, "out"), (stats, "stats"), (dx, "dx"), (partial, "partial"), (grads, "dgamma / dbeta")):
            g.intact(f"{name}{sfx} {what}")
        got["out" + sfx], got["dgamma" + sfx], got["dbeta" + sfx] = out.t, grads.t[0], grads.t[1]
        if add:
            xsum.intact(f"{name} xsum")
            got["xsum"], got["dx_add"] = xsum.t, dx.t
        else:
            got["dx"], got["mean"], got["rstd"] = dx.t, stats.t[:, 0], stats.t[:, 1]
        if c["kind"] == "constrow":
            # a constant row: its sum and mean are exact, every centred value is 0, the output is beta
            r = R // 2
            assert torch.equal(out.t[r], t["beta"]), f"{name}{sfx}: the constant row is not beta"
            assert abs(float(stats.t[r, 1]) * math.sqrt(CC.EPS) - 1) <= CC.FLOOR, float(stats.t[r, 1])
    _hold(name, got)


@pytest.mark.parametrize("name", CC.names("fold"))
def test_layernorm_fold_vs_float64(dev, name):
    """Several LayerNorms' partial sums folded by ONE s2t_layernorm_param_grad call into pre-filled
    gradients: the 8-item chunking, items of different row counts (and partial-row counts) in one
    launch, more partial rows than thread groups."""
    from speech2text_amd import conf_kernels as ck
    c = CC.CASES[name]
    C, n = c["C"], len(c["rows"])
    items = CC.make(name)["items"]
    dg, db = Buf(dev, (n, C)), Buf(dev, (n, C))
    keep, call = [], []
    for i, it in enumerate(items):
        d = {k: v.to(dev) for k, v in it.items()}
        _, _, stats = _ln_forward(dev, d["x"], None, d["gamma"], d["beta"])
        _, partial = _ln_backward(dev, d["x"], stats.t, d["gamma"], d["dy"], None)
        dg.t[i].copy_(d["dg0"])
        db.t[i].copy_(d["db0"])
        keep.append(partial)
        call.append((partial.t, it["x"].shape[0], dg.t[i], db.t[i]))
    ck.ln_param_grad(call, C)
    torch.cuda.synchronize()
    for i, p in enumerate(keep):
        p.intact(f"{name} partial {i}")
    dg.intact(f"{name} dgamma")
    db.intact(f"{name} dbeta")
    _hold(name, dict(dgamma=list(dg.t), dbeta=list(db.t)))


# ------------------------------------------------------------------ SiLU
@pytest.mark.parametrize("name", CC.names("silu", kernel=True))
def test_silu_kernels_vs_float64(dev, name):
    """silu_fwd and silu_bwd (scale 0.5) through the ABI; the backward written over da (the form
    the layer executor uses) equals the out-of-place one bit for bit."""
    N, lib, st = env()
    from speech2text_amd import conf_kernels as ck
    n = CC.CASES[name]["n"]
    t = CC.make(name)
    h, da = t["h"].to(dev), t["da"].to(dev)
    a, dh, inp = Buf(dev, n), Buf(dev, n), Buf(dev, n)
    inp.t.view(-1).copy_(da)
    N.check(lib.s2t_silu_fwd(N.fp(h), n, N.fp(a.t), st), "s2t_silu_fwd")
    N.check(lib.s2t_silu_bwd(N.fp(h), N.fp(da), n, 0.5, N.fp(dh.t), st), "s2t_silu_bwd")
    same = ck.silu_bwd(h, inp.t.view(-1), 0.5, inplace=True)
    torch.cuda.synchronize()
    for g, what in ((a, "a"), (dh, "dh"), (inp, "dh in place")):
        g.intact(f"{name} {what}")
    assert same.data_ptr() == inp.t.data_ptr()
    assert torch.equal(inp.t, dh.t), f"{name}: in-place backward differs from the out-of-place one"
    assert torch.equal(ck.silu_fwd(h), a.t.view(-1)) and torch.equal(ck.silu_bwd(h, da, 0.5, inplace=False), dh.t.view(-1))
    if "sat_idx" in t:
        i = t["sat_idx"].to(dev)
        assert bool(torch.isfinite(a.t.view(-1)[i]).all()) and bool(torch.isfinite(dh.t.view(-1)[i]).all())
    _hold(name, dict(a=a.t.view(-1), dh=dh.t.view(-1)))


# ------------------------------------------------------------------ dropout streams
@pytest.mark.parametrize("name", CC.names("drop"))
def test_dropout_streams_vs_float64(dev, name):
    """dropout_add without and with x, silu_drop_fwd, silu_drop_bwd (scale 0.5): the keep pattern is
    oracle.conformer.keep_scale's at every element, the values are the yardstick's under that mask."""
    N, lib, st = env()
    c = CC.CASES[name]
    n, p, seed = c["n"], c["p"], c["dseed"]
    t = {k: v.to(dev) for k, v in CC.make(name).items()}
    mask, add, grad, fwd, bwd = (Buf(dev, n) for _ in range(5))
    ones = torch.ones(n, device=dev)
    N.check(lib.s2t_dropout_add(None, N.fp(ones), n, 1.0, p, seed, N.fp(mask.t), st), "s2t_dropout_add")
    N.check(lib.s2t_dropout_add(N.fp(t["x"]), N.fp(t["y"]), n, 0.5, p, seed, N.fp(add.t), st), "s2t_dropout_add")
    N.check(lib.s2t_dropout_add(None, N.fp(t["y"]), n, 0.5, p, seed, N.fp(grad.t), st), "s2t_dropout_add")
    N.check(lib.s2t_silu_drop_fwd(N.fp(t["h"]), n, p, seed, N.fp(fwd.t), st), "s2t_silu_drop_fwd")
    N.check(lib.s2t_silu_drop_bwd(N.fp(t["h"]), N.fp(t["da"]), n, 0.5, p, seed, N.fp(bwd.t), st),
            "s2t_silu_drop_bwd")
    torch.cuda.synchronize()
    for g, what in ((mask, "mask"), (add, "add"), (grad, "grad"), (fwd, "sd_fwd"), (bwd, "sd_bwd")):
        g.intact(f"{name} {what}")
    want = OC.keep_scale(seed, (n,), p)
    m = mask.t.view(-1).cpu()
    assert torch.equal(m != 0, want != 0), f"{name}: keep pattern differs at {int(((m != 0) != (want != 0)).sum())} elements"
    if p in (0.1, 0.5):
        assert torch.equal(m, want), f"{name}: mask values differ"
    for g in (grad, fwd, bwd):          # the same elements are dropped by every pass
        assert bool((g.t.view(-1)[(want == 0).to(dev)] == 0).all())
    _hold(name, dict(add=add.t.view(-1), grad=grad.t.view(-1), sd_fwd=fwd.t.view(-1), sd_bwd=bwd.t.view(-1)))


# ------------------------------------------------------------------ BatchNorm + SiLU
@pytest.mark.parametrize("name", CC.names("bn"))
def test_batchnorm_silu_vs_float64(dev, name):
    """Training forward (save vectors, running statistics, batch counter), backward into pre-filled
    dgamma / dbeta, and the evaluation pass, through the ABI; then the module path
    (conf_kernels.bn_silu_fwd / batchnorm_silu) must give the same bits, its momentum included."""
    N, lib, st = env()
    from speech2text_amd import conf_kernels as ck
    c = CC.CASES[name]
    R, C = c["rows"], c["C"]
    t = CC.make(name)
    gamma, beta, ds = t["gamma"].to(dev), t["beta"].to(dev), t["ds"].to(dev)
    rm, rv = Buf(dev, (1, C), t["rm0"]), Buf(dev, (1, C), t["rv0"])
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = Buf(dev, (N.const("S2T_BN_PARTIALS") + 1, 2 * C))
    assert ws.t.numel() == lib.s2t_bn_workspace_floats(C)
    bn = torch.nn.BatchNorm1d(C, eps=CC.EPS, momentum=c["momentum"], track_running_stats=c["track"]).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        if c["track"]:
            bn.running_mean.copy_(t["rm0"]); bn.running_var.copy_(t["rv0"])
    for i, x0 in enumerate(t["xs"]):
        x = x0.to(dev)
        y, mean, rstd = Buf(dev, (R, C)), Buf(dev, (1, C)), Buf(dev, (1, C))
        mom = 1.0 / (i + 1) if c["momentum"] is None else c["momentum"]
        N.check(lib.s2t_bn_silu_fwd(N.fp(x), N.fp(gamma), N.fp(beta), CC.EPS, mom if c["track"] else 0.0,
                                    N.fp(rm.t) if c["track"] else None, N.fp(rv.t) if c["track"] else None,
                                    N.lp(nbt) if c["track"] else None, R, C, N.fp(y.t), N.fp(mean.t),
                                    N.fp(rstd.t), N.fp(ws.t), st), "s2t_bn_silu_fwd")
        y2, mean2, rstd2 = ck.bn_silu_fwd(x, bn)
        assert torch.equal(y2, y.t) and torch.equal(mean2, mean.t[0]) and torch.equal(rstd2, rstd.t[0])
    dx, grads = Buf(dev, (R, C)), Buf(dev, (2, C))
    grads.t[0].copy_(t["dg0"]); grads.t[1].copy_(t["db0"])
    N.check(lib.s2t_bn_silu_bwd(N.fp(x), N.fp(ds), N.fp(mean.t), N.fp(rstd.t), N.fp(gamma), N.fp(beta), R, C,
                                N.fp(dx.t), N.fp(grads.t[0]), N.fp(grads.t[1]), N.fp(ws.t), st), "s2t_bn_silu_bwd")
    torch.cuda.synchronize()
    for g, what in ((y, "y"), (mean, "save_mean"), (rstd, "save_rstd"), (rm, "running_mean"),
                    (rv, "running_var"), (ws, "workspace"), (dx, "dx"), (grads, "dgamma / dbeta")):
        g.intact(f"{name} {what}")
    got = dict(y=y.t, mean=mean.t[0], rstd=rstd.t[0], dgamma=grads.t[0], dbeta=grads.t[1])
    if R == 2:
        got["dx_plus_ds"] = dx.t.double() + ds.double()
    else:
        got["dx"] = dx.t
    xe = ds * 1.7
    if c["track"]:
        assert int(nbt) == c["batches"] and int(bn.num_batches_tracked) == c["batches"]
        assert torch.equal(bn.running_mean, rm.t[0]) and torch.equal(bn.running_var, rv.t[0])
        got["running_mean"], got["running_var"] = rm.t[0], rv.t[0]
        ye = Buf(dev, (R, C))
        ers = torch.rsqrt(rv.t[0] + CC.EPS)
        N.check(lib.s2t_bn_silu_apply(N.fp(xe), N.fp(rm.t[0]), N.fp(ers), N.fp(gamma), N.fp(beta), R, C,
                                      N.fp(ye.t), st), "s2t_bn_silu_apply")
        torch.cuda.synchronize()
        ye.intact(f"{name} y_eval")
        assert torch.equal(ck.batchnorm_silu(xe, bn.eval()), ye.t)
        got["y_eval"] = ye.t
    else:
        assert bn.running_mean is None
        got["y_eval"] = ck.batchnorm_silu(xe, bn.eval())
    _hold(name, got)


# ------------------------------------------------------------------ attention
def _mhsa_abi(dev, c, qkv_buf, ld, offs, lens, do_buf, ldo, seed):
    """s2t_mhsa_fwd + s2t_mhsa_bwd on a (T*B [+ guard], ld) buffer holding q, k, v at column offsets
    `offs` -> guarded (o, lse, delta, dqkv), o and dqkv with rows of ldo / ld floats."""
    N, lib, st = env()
    T, B, H, dh = c["T"], c["B"], c["H"], c["dh"]
    o, dqkv = Buf(dev, (T * B, ldo)), Buf(dev, (T * B, ld))
    lse, delta = Buf(dev, (B * H, T)), Buf(dev, (B * H, T))
    sc = 1.0 / math.sqrt(dh)
    N.check(lib.s2t_mhsa_fwd(N.fp(qkv_buf), ld, offs[0], offs[1], offs[2], N.lp(lens), T, B, H, dh, sc,
                             c["p"], seed, N.fp(o.t), ldo, N.fp(lse.t), st), "s2t_mhsa_fwd")
    N.check(lib.s2t_mhsa_bwd(N.fp(qkv_buf), ld, offs[0], offs[1], offs[2], N.lp(lens), T, B, H, dh, sc,
                             c["p"], seed, N.fp(o.t), N.fp(do_buf), ldo, N.fp(lse.t), N.fp(delta.t),
                             N.fp(dqkv.t), st), "s2t_mhsa_bwd")
    torch.cuda.synchronize()
    return o, lse, delta, dqkv


def _attn_tensors(c, o, dqkv):
    T, B, D = c["T"], c["B"], c["H"] * c["dh"]
    o, dqkv = o.reshape(T, B, D), dqkv.reshape(T, B, 3 * D)
    if T == 1:
        return dict(o=o, dqkv=dqkv)
    dq, dk, dv = dqkv.chunk(3, dim=-1)
    return dict(o=o, dq=dq, dk=dk, dv=dv)


def _packed(dev, name):
    c, t = CC.CASES[name], CC.make(name)
    T, B, D = c["T"], c["B"], c["H"] * c["dh"]
    qkv = t["qkv"].to(dev).view(T * B, 3 * D)
    do = t["do"].to(dev).view(T * B, D)
    lens = None if t["lens"] is None else t["lens"].to(dev)
    seed = CC.attn_seed(name) if c["p"] > 0 else 0
    return c, t, qkv, do, lens, seed


@pytest.mark.parametrize("name", CC.names("attn", kernel=True))
def test_mhsa_kernels_vs_float64(dev, name, monkeypatch):
    """mhsa_fwd / mhsa_bwd through the ABI (packed layout) and the autograd wrapper conf_kernels.mhsa:
    forward, dQ, dK and dV each within bound, under the restated dropout mask where the case has
    dropout; an utterance of length 0 gives exact zeros everywhere."""
    from speech2text_amd import conf_kernels as ck
    c, t, qkv, do, lens, seed = _packed(dev, name)
    T, B, D = c["T"], c["B"], c["H"] * c["dh"]
    o, lse, delta, dqkv = _mhsa_abi(dev, c, qkv, 3 * D, (0, D, 2 * D), lens, do, D, seed)
    for g, what in ((o, "o"), (lse, "lse"), (delta, "delta"), (dqkv, "dqkv")):
        g.intact(f"{name} {what}")
    _hold(name, _attn_tensors(c, o.t, dqkv.t))
    monkeypatch.setattr(ck, "draw_seed", lambda: seed)
    qg = t["qkv"].to(dev).requires_grad_(True)
    og = ck.mhsa(qg, lens, c["H"], c["p"])
    assert type(og.grad_fn).__name__ == "_MhsaBackward", "the attention kernel did not run"
    (og * t["do"].to(dev)).sum().backward()
    assert torch.equal(og.detach().view(T * B, D), o.t) and torch.equal(qg.grad.view(T * B, 3 * D), dqkv.t)
    if c["lens"] is not None:
        for b, n in enumerate(c["lens"]):
            if n == 0:
                assert bool((o.t.view(T, B, D)[:, b] == 0).all()) and bool((dqkv.t.view(T, B, 3 * D)[:, b] == 0).all()), \
                    f"{name}: utterance {b} of length 0 is not exactly zero"
                assert bool((lse.t.view(B, c["H"], T)[b] == 0).all())


@pytest.mark.parametrize("name", ["attn_t65", "attn_len_b", "attn_drop_dh32_t200"])
def test_mhsa_strided_and_permuted_layout(dev, name):
    """The layout arguments of the ABI: qkv embedded in rows of ld = 3D + 8 floats with the column
    blocks ordered v, q, k; o / dO in rows of ldo = D + 4; dqkv in rows of ld.  Pad columns and the
    guard rows hold a sentinel: the results equal the packed layout's bit for bit and no sentinel
    is touched (the pad columns of the INPUTS hold it too: a kernel reading them would differ)."""
    c, t, qkv, do, lens, seed = _packed(dev, name)
    T, B, D = c["T"], c["B"], c["H"] * c["dh"]
    o0, _, _, dqkv0 = _mhsa_abi(dev, c, qkv, 3 * D, (0, D, 2 * D), lens, do, D, seed)
    ld, ldo = 3 * D + 8, D + 4
    buf, dob = Buf(dev, (T * B, ld)), Buf(dev, (T * B, ldo))
    voff, qoff, koff = 0, D, 2 * D
    buf.t[:, qoff:qoff + D] = qkv[:, :D]
    buf.t[:, koff:koff + D] = qkv[:, D:2 * D]
    buf.t[:, voff:voff + D] = qkv[:, 2 * D:]
    dob.t[:, :D] = do
    o, lse, delta, dqkv = _mhsa_abi(dev, c, buf.t, ld, (qoff, koff, voff), lens, dob.t, ldo, seed)
    for g, what in ((o, "o"), (lse, "lse"), (delta, "delta"), (dqkv, "dqkv")):
        g.intact(f"{name} {what}")
    assert bool((o.t[:, D:] == SENT).all()), f"{name}: pad columns of o were written"
    assert bool((dqkv.t[:, 3 * D:] == SENT).all()), f"{name}: pad columns of dqkv were written"
    assert torch.equal(o.t[:, :D], o0.t), f"{name}: o differs from the packed layout"
    for what, a, b in (("dq", qoff, 0), ("dk", koff, D), ("dv", voff, 2 * D)):
        assert torch.equal(dqkv.t[:, a:a + D], dqkv0.t[:, b:b + D]), f"{name}: {what} differs from the packed layout"


# ------------------------------------------------------------------ outside the kernels' rules
@pytest.mark.parametrize("name", CC.names("lnmod"))
def test_layer_norm_wrapper_outside_the_kernels_rules(dev, name):
    """Row lengths off the kernel's rule, LayerNorms without affine parameters or without a bias, a
    row-strided input and one at an address that is no multiple of 16: conf_kernels.layer_norm
    realigns or takes torch's device op; values and gradients against the yardstick."""
    from speech2text_amd import conf_kernels as ck
    c, t = CC.CASES[name], CC.make(name)
    C = c["C"]
    ln = torch.nn.LayerNorm(C, eps=CC.EPS, elementwise_affine=c["affine"], bias=c["bias"]).to(dev)
    with torch.no_grad():
        if c["affine"]:
            ln.weight.copy_(t["gamma"])
        if c["bias"]:
            ln.bias.copy_(t["beta"])
    x, dy = t["x"], t["dy"].to(dev)
    if c["how"] == "strided":
        wide = torch.zeros(5, 7, 2 * C, device=dev)
        wide[..., :C] = x.to(dev)
        x = wide[..., :C].detach().requires_grad_(True)
        assert not x.is_contiguous()
    elif c["how"] == "misaligned":
        flat = torch.zeros(x.numel() + 1, device=dev)
        flat[1:] = x.to(dev).view(-1)
        x = flat[1:].view(5, 7, C).detach().requires_grad_(True)
        assert x.data_ptr() % 16 == 4
    else:
        x = x.to(dev).requires_grad_(True)
    out = ck.layer_norm(x, ln)
    assert out.is_cuda and out.dtype == torch.float32
    (out * dy).sum().backward()
    got = dict(out=out.detach(), dx=x.grad)
    if c["affine"]:
        got["dgamma"] = ln.weight.grad
    if c["bias"]:
        got["dbeta"] = ln.bias.grad
    _hold(name, got)


def test_silu_wrapper_with_a_size_off_the_float4_rule(dev):
    from speech2text_amd import conf_kernels as ck
    t = CC.make("silu_odd")
    h = t["h"].to(dev).view(3, 7).requires_grad_(True)
    a = ck.silu(h)
    (a * t["da"].to(dev).view(3, 7)).sum().backward()
    _hold("silu_odd", dict(a=a.detach().view(-1), dh=0.5 * h.grad.view(-1)))


def test_dropout_module_on_a_view_off_the_alignment_rule(dev, monkeypatch):
    """conf_kernels.Dropout in training on a [1:4097] view of a 4100-float buffer (contiguous, numel
    a multiple of 4, address 4 past a multiple of 16), and the same for the incoming gradient: the
    wrapper realigns instead of failing with -2, and the mask is still keep_scale of the drawn seed
    (mask indices are element indices of the tensor, whatever its address)."""
    from speech2text_amd import conf_kernels as ck
    name = "dropmod_view"
    c, t = CC.CASES[name], CC.make(name)
    n = c["n"]
    seeds = []
    real = ck.draw_seed
    monkeypatch.setattr(ck, "draw_seed", lambda: seeds.append(real()) or seeds[-1])
    buf, gbuf = t["buf"].to(dev), t["gbuf"].to(dev)
    x = buf[1:n + 1].detach().requires_grad_(True)
    g = gbuf[1:n + 1]
    assert x.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 4 and x.is_contiguous()
    m = ck.Dropout(c["p"]).train()
    out = m(x)
    assert type(out.grad_fn).__name__ == "_DropoutBackward", "the hashed-mask kernel did not run"
    out.backward(g)
    assert len(seeds) == 1
    mask = OC.keep_scale(seeds[0], (n,), c["p"])
    assert torch.equal(out.detach().cpu() != 0, mask != 0) and torch.equal(x.grad.cpu() != 0, mask != 0)
    assert 0 < int((mask == 0).sum()) < n
    ref = CC._eval_dropmod(c, t, torch.float64, seed=seeds[0])
    _hold(name, dict(out=out.detach(), grad=x.grad), ref)


def test_mhsa_wrapper_with_a_head_width_off_the_rule_and_an_empty_utterance(dev):
    """dh = 36 takes torch's device attention; an utterance of length 0 gives zeros there as on the
    kernel path (output and gradient), not NaN."""
    from speech2text_amd import conf_kernels as ck
    name = "attn_dh36_len0"
    c, t = CC.CASES[name], CC.make(name)
    T, B, D = c["T"], c["B"], c["H"] * c["dh"]
    qg = t["qkv"].to(dev).requires_grad_(True)
    o = ck.mhsa(qg, t["lens"].to(dev), c["H"])
    (o * t["do"].to(dev)).sum().backward()
    got = _attn_tensors(c, o.detach(), qg.grad)
    _hold(name, got)
    assert bool((o[:, 1] == 0).all()) and bool((qg.grad[:, 1] == 0).all())
