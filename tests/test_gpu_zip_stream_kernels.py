"""GPU: the zipformer's streaming kernels (csrc/zip_elem.hip: Swoosh, BiasNorm, BiasNorm + bypass, the
Balancer's statistics and update; csrc/zip_glue.hip: bypass, SimpleDownsample, upsample + bypass, the
nonlinear attention's gate / out passes, the attention's row constants, the parameter gradient commit,
the add) called through the C ABI on device buffers of the test's own, against the float64 yardstick
tests/zip_f64.py, at every dispatch edge (tests/zip_cases.py names why each shape is there).

Error = max |got - ref| / max |ref| per tensor; allowed = zip_cases.bound(case, tensor) =
max(2e-5, 8 x the case's float32 figure of the YARDSTICK, asserted by tests/test_zip_f64.py).
Every buffer a kernel writes is a guarded buffer of tests/guarded.py holding the sentinel SENT, with a
guard of SENT behind it (and one word in front where it is misaligned), which must be intact afterwards; accumulators are pre-filled and must hold pre-fill + reference; a call the entry point
must refuse returns -1 and leaves its outputs at the sentinel.
"""
import ctypes
import functools

import pytest
import torch

import guarded
import zip_cases as ZC
import zip_f64 as ZF
from guarded import SENT, env, hold

pytestmark = pytest.mark.gpu

Buf = functools.partial(guarded.Buf, fill=SENT)
_hold = functools.partial(hold, ZC)


def _intact(name, **bufs):
    for k, b in bufs.items():
        b.intact(f"{name} {k}")


def _dev(dev, t, *keys):
    return [None if t[k] is None else t[k].to(dev) for k in keys]


# ------------------------------------------------------------------ Swoosh
@pytest.mark.parametrize("name", ZC.names("sw"))
def test_swoosh_kernels_vs_float64(dev, name):
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    n = c["n"]
    off, cst = ZF.SWOOSH[c["is_l"]]
    x, g = _dev(dev, t, "x", "g")
    y, d = Buf(dev, n), Buf(dev, n)
    N.check(lib.s2t_swoosh_fwd(N.fp(x), N.fp(y.t), n, off, cst, st), "s2t_swoosh_fwd")
    N.check(lib.s2t_swoosh_bwd(N.fp(x), N.fp(g), N.fp(d.t), n, off, st), "s2t_swoosh_bwd")
    torch.cuda.synchronize()
    _intact(name, y=y, d=d)
    _hold(name, dict(y=y.t, d=d.t))


def test_swoosh_wrappers_on_a_view_off_the_alignment_rule(dev):
    from speech2text_amd import zip_kernels as zk
    name = "sw_view"
    c, t = ZC.CASES[name], ZC.make(name)
    n = c["n"]
    x, g = t["buf"].to(dev)[1:n + 1], t["gbuf"].to(dev)[1:n + 1]
    assert x.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 4 and x.is_contiguous()
    _hold(name, dict(y=zk.swoosh_forward(x, c["is_l"]), d=zk.swoosh_backward(x, g, c["is_l"])))
    xg = x.detach().requires_grad_(True)
    zk.swoosh(xg, c["is_l"]).backward(g)
    _hold(name, dict(d=xg.grad), partial=True)


# ------------------------------------------------------------------ BiasNorm
@pytest.mark.parametrize("name", ZC.names("bn"))
def test_biasnorm_kernels_vs_float64(dev, name):
    """Forward (y and the per-row scales) and backward into pre-filled dbias / dls; the _tb cases
    through s2t_biasnorm_fwd_tb / _bwd_tb."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    R, D = c["rows"], c["D"]
    x, bias, ls, g = _dev(dev, t, "x", "bias", "ls", "g")
    y, scales, dx = Buf(dev, (R, D)), Buf(dev, R), Buf(dev, (R, D))
    dbias, dls = Buf(dev, D, t["db0"]), Buf(dev, 1, t["dl0"])
    if c["kind"] == "fwdonly":
        N.check(lib.s2t_biasnorm_fwd(N.fp(x), N.fp(bias), N.fp(ls), R, D, N.fp(y.t), N.fp(scales.t), st),
                "s2t_biasnorm_fwd")
        torch.cuda.synchronize()
        _intact(name, y=y, scales=scales)
        return _hold(name, dict(y=y.t, scales=scales.t))
    if c["tb"]:
        B, T = c["tb"]
        N.check(lib.s2t_biasnorm_fwd_tb(N.fp(x), N.fp(bias), N.fp(ls), T, B, D, N.fp(y.t), N.fp(scales.t), st),
                "s2t_biasnorm_fwd_tb")
        N.check(lib.s2t_biasnorm_bwd_tb(N.fp(x), N.fp(bias), N.fp(scales.t), N.fp(g), T, B, D, N.fp(dx.t),
                                        N.fp(dbias.t), N.fp(dls.t), st), "s2t_biasnorm_bwd_tb")
    else:
        N.check(lib.s2t_biasnorm_fwd(N.fp(x), N.fp(bias), N.fp(ls), R, D, N.fp(y.t), N.fp(scales.t), st),
                "s2t_biasnorm_fwd")
        N.check(lib.s2t_biasnorm_bwd(N.fp(x), N.fp(bias), N.fp(scales.t), N.fp(g), R, D, N.fp(dx.t),
                                     N.fp(dbias.t), N.fp(dls.t), st), "s2t_biasnorm_bwd")
    torch.cuda.synchronize()
    _intact(name, y=y, scales=scales, dx=dx, dbias=dbias, dls=dls)
    if c["kind"] == "zerog":
        assert torch.equal(dbias.t.cpu(), t["db0"]) and torch.equal(dls.t.cpu(), t["dl0"])
        assert not bool(dx.t.any())
    _hold(name, dict(y=y.t, scales=scales.t, dx=dx.t, dbias=dbias.t, dls=dls.t))


def test_biasnorm_backward_refuses_a_row_longer_than_1024(dev):
    N, lib, st = env()
    R, D = 3, 1028
    x, bias, g = torch.randn(R, D, device=dev), torch.zeros(D, device=dev), torch.randn(R, D, device=dev)
    scales = torch.ones(R, device=dev)
    dx, dbias, dls = Buf(dev, (R, D)), Buf(dev, D), Buf(dev, 1)
    assert lib.s2t_biasnorm_bwd(N.fp(x), N.fp(bias), N.fp(scales), N.fp(g), R, D, N.fp(dx.t), N.fp(dbias.t),
                                N.fp(dls.t), st) == -1
    assert lib.s2t_biasnorm_bwd_tb(N.fp(x), N.fp(bias), N.fp(scales), N.fp(g), R, 1, D, N.fp(dx.t),
                                   N.fp(dbias.t), N.fp(dls.t), st) == -1
    torch.cuda.synchronize()
    for b in (dx, dbias, dls):
        b.untouched("s2t_biasnorm_bwd at D = 1028")


# ------------------------------------------------------------------ BiasNorm + bypass
@pytest.mark.parametrize("name", ZC.names("nb"))
def test_norm_bypass_kernels_vs_float64(dev, name):
    """s2t_norm_bypass_fwd and _bwd: out, the scales, dx, d_orig and the three pre-filled parameter
    gradients, each against float64."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    R, B, D, mis = c["rows"], c["B"], c["D"], c["mis"]
    bias, ls, bscale, fm = _dev(dev, t, "bias", "ls", "bscale", "fm")
    x, orig, g = (Buf(dev, (R, D), t[k], mis) for k in ("x", "orig", "g"))
    out, dx, d_orig = (Buf(dev, (R, D), mis=mis) for _ in range(3))
    scales = Buf(dev, R)
    dk, db, dl = Buf(dev, D, t["dk0"]), Buf(dev, D, t["db0"]), Buf(dev, 1, t["dl0"])
    N.check(lib.s2t_norm_bypass_fwd(N.fp(x.t), N.fp(bias), N.fp(ls), N.fp(orig.t), N.fp(bscale), N.fp(fm), B, R, D,
                                    N.fp(out.t), N.fp(scales.t), st), "s2t_norm_bypass_fwd")
    N.check(lib.s2t_norm_bypass_bwd(N.fp(x.t), N.fp(bias), N.fp(scales.t), N.fp(orig.t), N.fp(bscale), N.fp(g.t),
                                    N.fp(fm), B, R, D, N.fp(dx.t), N.fp(d_orig.t), N.fp(dk.t), N.fp(db.t),
                                    N.fp(dl.t), st), "s2t_norm_bypass_bwd")
    torch.cuda.synchronize()
    _intact(name, out=out, scales=scales, dx=dx, d_orig=d_orig, d_bscale=dk, dbias=db, dls=dl, x=x, orig=orig, g=g)
    if c["fmzero"]:
        dead = (torch.arange(R) % B == B - 1).to(dev)
        for what, b in (("out", out), ("d_orig", d_orig), ("dx", dx)):
            assert not bool(b.t[dead].any()), f"{name}: {what} of a row whose feature mask is zero"
    _hold(name, dict(out=out.t, scales=scales.t, dx=dx.t, d_orig=d_orig.t, d_bscale=dk.t, dbias=db.t, dls=dl.t))


def test_norm_bypass_refuses_a_row_longer_than_1024_and_an_empty_batch(dev):
    N, lib, st = env()
    R = 3
    for D, B, fwd_too in ((1028, 1, False), (64, 0, True)):
        x, orig, g = (torch.randn(R, D, device=dev) for _ in range(3))
        bias, bscale, ls = torch.zeros(D, device=dev), torch.ones(D, device=dev), torch.zeros(1, device=dev)
        scales = torch.ones(R, device=dev)
        outs = [Buf(dev, (R, D)), Buf(dev, (R, D)), Buf(dev, D), Buf(dev, D), Buf(dev, 1)]
        assert lib.s2t_norm_bypass_bwd(N.fp(x), N.fp(bias), N.fp(scales), N.fp(orig), N.fp(bscale), N.fp(g), None, B,
                                       R, D, *(N.fp(b.t) for b in outs), st) == -1
        if fwd_too:
            outs += [Buf(dev, (R, D)), Buf(dev, R)]
            assert lib.s2t_norm_bypass_fwd(N.fp(x), N.fp(bias), N.fp(ls), N.fp(orig), N.fp(bscale), None, B, R, D,
                                           N.fp(outs[-2].t), N.fp(outs[-1].t), st) == -1
        torch.cuda.synchronize()
        for b in outs:
            b.untouched(f"s2t_norm_bypass at D = {D}, B = {B}")


# ------------------------------------------------------------------ Balancer
def _bal_operands(dev, c, t):
    """x, g and two outputs in guarded buffers of row lengths ldx, ldg, ldo (the case's, or C); pad
    columns hold the sentinel in inputs and outputs alike."""
    R, C = c["rows"], c["C"]
    ldx, ldg, ldo = c["ld"] or (C, C, C)
    x, g = Buf(dev, (R, ldx)), Buf(dev, (R, ldg))
    x.t[:, :C] = t["x"].to(dev)
    g.t[:, :C] = t["g"].to(dev)
    return x, g, Buf(dev, (R, ldo)), Buf(dev, (R, ldo)), (ldx, ldg, ldo)


def _bal_got(c, t, out, sfx=""):
    C = c["C"]
    x, g = t["x"].double(), t["g"].double()
    ge = g if c["swoosh"] is None else g * ZF.swoosh_grad_ref(x, c["swoosh"])
    o = out.t[:, :C]
    return {"out" + sfx: o, "upd" + sfx: o.double().cpu() - ge}


def _act_off(c):
    return -1.0 if c["swoosh"] is None else ZF.SWOOSH[c["swoosh"]][0]


@pytest.mark.parametrize("name", ZC.names("bal"))
def test_balancer_kernels_vs_float64(dev, name):
    """s2t_balancer_bwd (statistics + update in one call, alternating accumulators) and the pair
    s2t_balancer_stats + s2t_balancer_apply, each against the autograd restatement: the output and the
    update alone.  Dead channels (variance or E[x^2] at the 1e-20 clamp) included."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    R, C = c["rows"], c["C"]
    x, g, out, out2, (ldx, ldg, ldo) = _bal_operands(dev, c, t)
    assert lib.s2t_balancer_bwd_workspace_floats() == 4096
    ws, stats = Buf(dev, 4096, torch.zeros(4096)), Buf(dev, 2048, torch.zeros(2048))
    N.check(lib.s2t_balancer_bwd(N.fp(x.t), ldx, N.fp(g.t), ldg, R, C, *ZC.BAL_CFG, N.fp(out.t), ldo, N.fp(ws.t), 0,
                                 _act_off(c), st), "s2t_balancer_bwd")
    N.check(lib.s2t_balancer_stats(N.fp(x.t), ldx, R, C, N.fp(stats.t), st), "s2t_balancer_stats")
    N.check(lib.s2t_balancer_apply(N.fp(x.t), ldx, N.fp(g.t), ldg, R, C, *ZC.BAL_CFG, N.fp(out2.t), ldo,
                                   N.fp(stats.t), _act_off(c), st), "s2t_balancer_apply")
    torch.cuda.synchronize()
    _intact(name, out=out, out2=out2, workspace=ws, stats=stats)
    for b in (out, out2):
        assert bool((b.t[:, C:] == SENT).all()), f"{name}: pad columns of the output were written"
    assert not bool(ws.t[2048:].any()), f"{name}: the next call's accumulator is not clean"
    assert not bool(ws.t[C:1024].any()) and not bool(ws.t[1024 + C:2048].any())
    got = _bal_got(c, t, out)
    got.update(_bal_got(c, t, out2, "@split"))
    _hold(name, got, alias={"out@split": "out", "upd@split": "upd"})
    if c["kind"] == "dead":
        gs, gd = ZC.BAL_CFG[4], t["g"].to(dev)
        for o in (out.t, out2.t):
            assert torch.equal(o[:, 2], gd[:, 2]), f"{name}: the all-zero channel received an update"
            assert ZC.rel_err(o[:, 1], (t["g"][:, 1] + gs * t["g"][:, 1].abs()).double()) <= ZC.FLOOR


def test_balancer_bwd_leaves_the_other_accumulator_clean_after_a_wider_user(dev):
    """Two successive s2t_balancer_bwd calls on alternating parity, the first with C = 1024 and the
    second with C = 64: the second must clear the WHOLE accumulator the first one used (2048 floats),
    and a third call on that accumulator is right again."""
    N, lib, st = env()
    ws = Buf(dev, 4096, torch.zeros(4096))
    for parity, name in ((0, "bal_c1024"), (1, "bal_c64"), (0, "bal_c64")):
        c, t = ZC.CASES[name], ZC.make(name)
        R, C = c["rows"], c["C"]
        x, g, out, _, (ldx, ldg, ldo) = _bal_operands(dev, c, t)
        N.check(lib.s2t_balancer_bwd(N.fp(x.t), ldx, N.fp(g.t), ldg, R, C, *ZC.BAL_CFG, N.fp(out.t), ldo,
                                     N.fp(ws.t), parity, -1.0, st), "s2t_balancer_bwd")
        torch.cuda.synchronize()
        other = ws.t[2048:] if parity == 0 else ws.t[:2048]
        assert not bool(other.any()), f"after {name} on parity {parity}: the other accumulator holds {int((other != 0).sum())} words"
        _intact(name, out=out, workspace=ws)
        _hold(name, _bal_got(c, t, out))


def test_balancer_refuses_more_than_1024_channels(dev):
    N, lib, st = env()
    R, C = 3, 1025
    x, g = torch.randn(R, C, device=dev), torch.randn(R, C, device=dev)
    out, ws = Buf(dev, (R, C)), Buf(dev, 4096)
    assert lib.s2t_balancer_bwd(N.fp(x), C, N.fp(g), C, R, C, *ZC.BAL_CFG, N.fp(out.t), C, N.fp(ws.t), 0, -1.0, st) == -1
    assert lib.s2t_balancer_stats(N.fp(x), C, R, C, N.fp(ws.t), st) == -1
    assert lib.s2t_balancer_apply(N.fp(x), C, N.fp(g), C, R, C, *ZC.BAL_CFG, N.fp(out.t), C, N.fp(ws.t), -1.0, st) == -1
    torch.cuda.synchronize()
    out.untouched("s2t_balancer at C = 1025")
    ws.untouched("s2t_balancer at C = 1025")


# ------------------------------------------------------------------ bypass
@pytest.mark.parametrize("name", ZC.names("by"))
def test_bypass_kernels_vs_float64(dev, name):
    """s2t_bypass_fwd / _fwd_mask (refused when C % 4 != 0), s2t_bypass_bwd / _bwd_mask / _bwd_acc into
    a pre-filled d_scale."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    R, C, B = c["rows"], c["C"], c["B"]
    orig, src, scale, g, fm, acc_in = _dev(dev, t, "orig", "src", "scale", "g", "fm", "acc_in")
    out, outm = Buf(dev, (R, C)), Buf(dev, (R, C))
    rc = lib.s2t_bypass_fwd(N.fp(orig), N.fp(src), N.fp(scale), R, C, N.fp(out.t), st)
    rcm = lib.s2t_bypass_fwd_mask(N.fp(orig), N.fp(src), N.fp(scale), N.fp(fm), B, R, C, N.fp(outm.t), st)
    got = {}
    if C % 4:
        assert rc == -1 and rcm == -1
        torch.cuda.synchronize()
        out.untouched(f"{name} s2t_bypass_fwd")
        outm.untouched(f"{name} s2t_bypass_fwd_mask")
    else:
        assert rc == 0 and rcm == 0
        got.update(out=out.t, out_m=outm.t)
    bufs = {}
    for sfx in ("", "_m", "_acc"):
        do, dsrc, dk = Buf(dev, (R, C)), Buf(dev, (R, C)), Buf(dev, C, t["dk0"])
        a = (N.fp(orig), N.fp(src), N.fp(scale), N.fp(g))
        o = (R, C, N.fp(do.t), N.fp(dsrc.t), N.fp(dk.t), st)
        if sfx == "":
            N.check(lib.s2t_bypass_bwd(*a, *o), "s2t_bypass_bwd")
        elif sfx == "_m":
            N.check(lib.s2t_bypass_bwd_mask(*a, N.fp(fm), B, *o), "s2t_bypass_bwd_mask")
        else:
            N.check(lib.s2t_bypass_bwd_acc(*a, N.fp(acc_in), *o), "s2t_bypass_bwd_acc")
        bufs.update({"d_orig" + sfx: do, "d_src" + sfx: dsrc, "d_scale" + sfx: dk})
    torch.cuda.synchronize()
    _intact(name, out=out, out_m=outm, **bufs)
    got.update({k: b.t for k, b in bufs.items()})
    assert torch.equal(bufs["d_src_acc"].t, bufs["d_src"].t), f"{name}: acc_in changed d_src"
    _hold(name, got, alias={"d_src_acc": "d_src", "d_scale_acc": "d_scale"}, partial=bool(C % 4))


# ------------------------------------------------------------------ downsample
@pytest.mark.parametrize("name", ZC.names("ds"))
def test_downsample_kernels_vs_float64(dev, name):
    """s2t_downsample_fwd / _fwd_bt and s2t_downsample_bwd / _bwd_bt (dw pre-filled): time-major and
    batch-major output and gradient give the same values."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    ds, T, B, C, mis = c["ds"], c["T"], c["B"], c["C"], c["mis"]
    dT = (T + ds - 1) // ds
    w = t["w"].to(dev)
    src, g = Buf(dev, (T, B, C), t["src"], mis), Buf(dev, (dT, B, C), t["g"], mis)
    gbt = Buf(dev, (B, dT, C), t["g"].transpose(0, 1).contiguous(), mis)
    out, outbt = Buf(dev, (dT, B, C)), Buf(dev, (B, dT, C))
    dsrc, dsrc2 = Buf(dev, (T, B, C), mis=mis), Buf(dev, (T, B, C), mis=mis)
    dw, dw2 = Buf(dev, ds, t["dw0"]), Buf(dev, ds, t["dw0"])
    N.check(lib.s2t_downsample_fwd(N.fp(src.t), N.fp(w), ds, T, B, C, N.fp(out.t), st), "s2t_downsample_fwd")
    N.check(lib.s2t_downsample_fwd_bt(N.fp(src.t), N.fp(w), ds, T, B, C, N.fp(outbt.t), st), "s2t_downsample_fwd_bt")
    N.check(lib.s2t_downsample_bwd(N.fp(src.t), N.fp(w), N.fp(g.t), ds, T, B, C, N.fp(dsrc.t), N.fp(dw.t), st),
            "s2t_downsample_bwd")
    N.check(lib.s2t_downsample_bwd_bt(N.fp(src.t), N.fp(w), N.fp(gbt.t), ds, T, B, C, N.fp(dsrc2.t), N.fp(dw2.t), st),
            "s2t_downsample_bwd_bt")
    torch.cuda.synchronize()
    _intact(name, out=out, out_bt=outbt, d_src=dsrc, d_src_bt=dsrc2, dw=dw, dw_bt=dw2)
    assert torch.equal(outbt.t.transpose(0, 1), out.t), f"{name}: the batch-major output differs"
    assert torch.equal(dsrc2.t, dsrc.t), f"{name}: d_src from the batch-major gradient differs"
    _hold(name, {"out": out.t, "out_bt": outbt.t, "d_src": dsrc.t, "dw": dw.t, "dw@bt": dw2.t}, alias={"dw@bt": "dw"})


def test_downsample_refuses_a_factor_above_8(dev):
    N, lib, st = env()
    T, B, C, ds = 10, 2, 8, 9
    src, g, w = torch.randn(T, B, C, device=dev), torch.randn(2, B, C, device=dev), torch.ones(ds, device=dev) / ds
    out, dsrc, dw = Buf(dev, (2, B, C)), Buf(dev, (T, B, C)), Buf(dev, ds)
    for bt in ("", "_bt"):
        assert getattr(lib, "s2t_downsample_fwd" + bt)(N.fp(src), N.fp(w), ds, T, B, C, N.fp(out.t), st) == -1
        assert getattr(lib, "s2t_downsample_bwd" + bt)(N.fp(src), N.fp(w), N.fp(g), ds, T, B, C, N.fp(dsrc.t),
                                                       N.fp(dw.t), st) == -1
    torch.cuda.synchronize()
    for b in (out, dsrc, dw):
        b.untouched("s2t_downsample at ds = 9")


# ------------------------------------------------------------------ upsample + bypass
@pytest.mark.parametrize("name", ZC.names("up"))
def test_upsample_bypass_kernels_vs_float64(dev, name):
    """s2t_bypass_up_fwd (refused when C % 4 != 0; its float4 stream has no scalar form, so the
    misaligned case runs the backward only) and s2t_bypass_up_bwd into a pre-filled d_scale."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    up, T, B, C, mis = c["up"], c["T"], c["B"], c["C"], c["mis"]
    Ts = (T + up - 1) // up
    scale = t["scale"].to(dev)
    orig, g, src = Buf(dev, (T, B, C), t["orig"], mis), Buf(dev, (T, B, C), t["g"], mis), Buf(dev, (Ts, B, C), t["src"], mis)
    out, do, dsrc, dk = Buf(dev, (T, B, C)), Buf(dev, (T, B, C), mis=mis), Buf(dev, (Ts, B, C), mis=mis), Buf(dev, C, t["dk0"])
    got = {}
    if not mis:
        rc = lib.s2t_bypass_up_fwd(N.fp(orig.t), N.fp(src.t), N.fp(scale), up, T, B, C, N.fp(out.t), st)
        if C % 4:
            assert rc == -1
            torch.cuda.synchronize()
            out.untouched(f"{name} s2t_bypass_up_fwd")
        else:
            assert rc == 0
            got["out"] = out.t
    N.check(lib.s2t_bypass_up_bwd(N.fp(orig.t), N.fp(src.t), N.fp(scale), N.fp(g.t), up, T, B, C, N.fp(do.t),
                                  N.fp(dsrc.t), N.fp(dk.t), st), "s2t_bypass_up_bwd")
    torch.cuda.synchronize()
    _intact(name, out=out, d_orig=do, d_src=dsrc, d_scale=dk)
    got.update(d_orig=do.t, d_src=dsrc.t, d_scale=dk.t)
    _hold(name, got, partial="out" not in got)


# ------------------------------------------------------------------ nonlinear attention glue
@pytest.mark.parametrize("name", ZC.names("nl"))
def test_nonlin_gate_and_out_kernels_vs_float64(dev, name):
    """s2t_nonlin_gate_fwd / _out_fwd / _out_bwd / _gate_bwd on u = [s | x | y]; du is written in
    thirds: [ds | dx] by the gate's backward, [dy] by the out's, and neither touches the other's."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    T, B, C = c["T"], c["B"], c["C"]
    u, z, g, dxs = _dev(dev, t, "u", "z", "g", "dxs")
    xs, o, dz = Buf(dev, (B, T, C)), Buf(dev, (T, B, C)), Buf(dev, (B, T, C))
    du, du_out, du_gate = (Buf(dev, (T * B, 3 * C)) for _ in range(3))
    N.check(lib.s2t_nonlin_gate_fwd(N.fp(u), T, B, C, N.fp(xs.t), st), "s2t_nonlin_gate_fwd")
    N.check(lib.s2t_nonlin_out_fwd(N.fp(z), N.fp(u), T, B, C, N.fp(o.t), st), "s2t_nonlin_out_fwd")
    N.check(lib.s2t_nonlin_out_bwd(N.fp(g), N.fp(z), N.fp(u), T, B, C, N.fp(dz.t), N.fp(du_out.t), st), "s2t_nonlin_out_bwd")
    N.check(lib.s2t_nonlin_gate_bwd(N.fp(dxs), N.fp(u), T, B, C, N.fp(du_gate.t), st), "s2t_nonlin_gate_bwd")
    N.check(lib.s2t_nonlin_out_bwd(N.fp(g), N.fp(z), N.fp(u), T, B, C, N.fp(dz.t), N.fp(du.t), st), "s2t_nonlin_out_bwd")
    N.check(lib.s2t_nonlin_gate_bwd(N.fp(dxs), N.fp(u), T, B, C, N.fp(du.t), st), "s2t_nonlin_gate_bwd")
    torch.cuda.synchronize()
    _intact(name, xs=xs, o=o, dz=dz, du=du, du_out=du_out, du_gate=du_gate)
    assert bool((du_out.t[:, :2 * C] == SENT).all()), f"{name}: the out backward wrote into [ds | dx]"
    assert bool((du_gate.t[:, 2 * C:] == SENT).all()), f"{name}: the gate backward wrote into [dy]"
    assert torch.equal(du.t[:, 2 * C:], du_out.t[:, 2 * C:]) and torch.equal(du.t[:, :2 * C], du_gate.t[:, :2 * C])
    _hold(name, dict(xs=xs.t, o=o.t, dz=dz.t, du=du.t))


# ------------------------------------------------------------------ attention row constants
def _delta_call(dev, c, t, delta):
    N, lib, st = env()
    keep = [t["W"].to(dev), None if t["dW0"] is None else t["dW0"].to(dev)]
    args = []
    for p, dv in zip(t["pairs"], (c["dv1"], c["dv2"])):
        p = (None, None) if p is None else (p[0].to(dev), p[1].to(dev))
        keep += list(p)
        args += [N.fp(p[0]), N.fp(p[1]), dv]
    return lib.s2t_attn_delta_pairs(N.fp(keep[0]), N.fp(keep[1]), *args, c["T"], c["B"], c["H"], N.fp(delta.t), st), keep


@pytest.mark.parametrize("name", ZC.names("dp"))
def test_attn_delta_pairs_vs_float64(dev, name):
    c, t = ZC.CASES[name], ZC.make(name)
    delta = Buf(dev, (c["H"], c["B"], c["T"]))
    rc, keep = _delta_call(dev, c, t, delta)
    assert rc == 0
    torch.cuda.synchronize()
    _intact(name, delta=delta)
    _hold(name, dict(delta=delta.t))
    if c["dw0"] and c["H"] > 1:         # only head 0 receives the dW0 term
        d2 = Buf(dev, (c["H"], c["B"], c["T"]))
        rc, keep = _delta_call(dev, c, dict(t, dW0=None), d2)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(d2.t[1:], delta.t[1:]) and not torch.equal(d2.t[0], delta.t[0])


def test_attn_delta_pairs_refuses_a_value_width_above_64(dev):
    c = dict(ZC.CASES["dp_dv4_t1"], dv1=65, dv2=65)
    g = torch.Generator().manual_seed(1)
    t = dict(W=torch.rand(3, 2, 1, 1, generator=g), dW0=None,
             pairs=[(torch.randn(1, 2, 3 * 65, generator=g), torch.randn(1, 2, 3 * 65, generator=g))] * 2)
    delta = Buf(dev, (3, 2, 1))
    rc, keep = _delta_call(dev, c, t, delta)
    torch.cuda.synchronize()
    assert rc == -1
    delta.untouched("s2t_attn_delta_pairs at dv = 65")


# ------------------------------------------------------------------ parameter gradient commit
def _commit_items(dev, N, items, limits):
    Commit = N.struct("S2tCommit")
    arr = (Commit * max(1, len(items)))()
    bufs = []
    for i, (it, lim) in enumerate(zip(items, limits)):
        n = it["x"].numel()
        x, d, grad = Buf(dev, n, it["x"]), Buf(dev, n, it["d"]), Buf(dev, n, it["grad"])
        arr[i].x, arr[i].d, arr[i].grad = x.t.data_ptr(), d.t.data_ptr(), grad.t.data_ptr()
        arr[i].lo, arr[i].hi, arr[i].limit, arr[i].n = ZC.LO, ZC.HI, lim, n
        bufs.append((x, d, grad))
    return arr, bufs


@pytest.mark.parametrize("name", ZC.names("cm"))
def test_param_grad_commit_vs_float64(dev, name):
    """grad += d (after limit_param_value's sign flip where asked) for up to 8 parameters in one
    launch; d is exactly zero afterwards, x is not written."""
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    arr, bufs = _commit_items(dev, N, t["items"], c["limit"])
    N.check(lib.s2t_param_grad_commit_n(len(bufs), ctypes.cast(arr, ctypes.c_void_p), st), "s2t_param_grad_commit_n")
    torch.cuda.synchronize()
    for i, ((x, d, grad), it) in enumerate(zip(bufs, t["items"])):
        _intact(f"{name} item {i}", x=x, d=d, grad=grad)
        assert not bool(d.t.any()), f"{name} item {i}: d is not cleared"
        assert torch.equal(x.t.cpu(), it["x"])
    _hold(name, dict(grad=[b[2].t for b in bufs]))


def test_param_grad_commit_refuses_nine_items_and_does_nothing_for_none(dev):
    N, lib, st = env()
    g = torch.Generator().manual_seed(2)
    items = [dict(x=torch.randn(5, generator=g), d=torch.randn(5, generator=g), grad=torch.randn(5, generator=g))
             for _ in range(9)]
    arr, bufs = _commit_items(dev, N, items, [1] * 9)
    assert lib.s2t_param_grad_commit_n(9, ctypes.cast(arr, ctypes.c_void_p), st) == -1
    assert lib.s2t_param_grad_commit_n(0, ctypes.cast(arr, ctypes.c_void_p), st) == 0
    torch.cuda.synchronize()
    for (x, d, grad), it in zip(bufs, items):
        assert torch.equal(d.t.cpu(), it["d"]) and torch.equal(grad.t.cpu(), it["grad"]) and torch.equal(x.t.cpu(), it["x"])


# ------------------------------------------------------------------ add
@pytest.mark.parametrize("name", ZC.names("add"))
def test_add_kernel_vs_float64(dev, name):
    N, lib, st = env()
    n = ZC.CASES[name]["n"]
    t = ZC.make(name)
    a, b = _dev(dev, t, "a", "b")
    out, inplace = Buf(dev, n), Buf(dev, n, t["a"])
    N.check(lib.s2t_add_f32(N.fp(a), N.fp(b), N.fp(out.t), n, st), "s2t_add_f32")
    N.check(lib.s2t_add_f32(N.fp(inplace.t), N.fp(b), N.fp(inplace.t), n, st), "s2t_add_f32")
    torch.cuda.synchronize()
    _intact(name, out=out, inplace=inplace)
    assert torch.equal(out.t, inplace.t), f"{name}: out == a differs from the out-of-place sum"
    _hold(name, dict(out=out.t))


def test_add_refuses_an_operand_off_16_bytes(dev):
    N, lib, st = env()
    a, b, out = Buf(dev, 8, mis=True), Buf(dev, 8), Buf(dev, 8)
    for args in ((a, b, out), (b, a, out), (b, b, a)):
        assert lib.s2t_add_f32(*(N.fp(v.t) for v in args), 8, st) == -1
    torch.cuda.synchronize()
    a.untouched("s2t_add_f32 off 16 bytes")
    out.untouched("s2t_add_f32 off 16 bytes")


def test_every_case_is_used():
    groups = {"sw", "swmod", "bn", "nb", "bal", "by", "ds", "up", "nl", "dp", "cm", "add"}
    assert {c["group"] for c in ZC.CASES.values()} == groups
