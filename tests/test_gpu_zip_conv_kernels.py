"""GPU: the zipformer's convolution kernels (csrc/zip_conv.hip: the conv module's gate + padding mask +
chunk-causal depthwise conv, forward, activation output, data and parameter gradients; csrc/zip_front.hip:
the frontend's 1 -> 8 and 8 -> 32 convs, the channel-last depthwise conv and its weight gradient, col2im)
against the float64 yardstick tests/zipconv_f64.py, at every launch-time branch (tests/zipconv_cases.py
names why each shape is there).

Error = max |got - ref| / max |ref| per tensor; allowed = zipconv_cases.bound(case, tensor) =
max(2e-5, 8 x the case's float32 figure of the YARDSTICK, asserted by tests/test_zipconv_f64.py).  On the
exactly representable inputs the device must equal the reference bit for bit.  Where the test calls the
C ABI itself, every output and the workspace are guarded buffers of tests/guarded.py: they start as NaN
(with a NaN guard behind them) and must come out finite: every element is written and no partial-sum slot is read before it is written.  Accumulated
gradients start from N(0,1) and are compared as got - prefill.  A call the entry point must refuse
returns its code and leaves its outputs NaN.
"""
import functools
import types

import pytest
import torch

import zip_f64 as ZF
import zipconv_cases as ZC
from guarded import NAN, Buf, env, hold, ptr

pytestmark = pytest.mark.gpu

_hold = functools.partial(hold, ZC)

GRADS = ("dwc", "dbc", "dwk", "dbk", "dscale")

COVER = dict(cm_run=ZC.names("cm", via="wrapper") + ZC.names("cm", via="direct"), cm_glu=ZC.names("cm", via="glu"),
             cm_split=ZC.names("cm", via="split"), cm_act=ZC.names("cm", via="act"), dw=ZC.names("dw"),
             wg=ZC.names("wg"), c1=ZC.names("c1"), s2=ZC.names("s2"), c2i=ZC.names("c2i"))
RUNS = dict(test_conv_module_vs_float64="cm_run", test_conv_module_through_the_autograd_wrapper="cm_glu",
            test_conv_module_split_backward_equals_the_joint_one="cm_split",
            test_conv_module_activation_output="cm_act", test_dwconv2d_forward_vs_float64="dw",
            test_dwconv2d_weight_gradient_vs_float64="wg", test_conv3x3_c1_vs_float64="c1",
            test_conv3x3_s2_vs_float64="s2", test_col2im3x3_vs_float64="c2i")


def _to(dev, t, *keys):
    return [None if t[k] is None else t[k].to(dev) for k in keys]


# ------------------------------------------------------------------ conv module
def _cm_operands(dev, c, t):
    """-> (u (T,B,ld) in the case's device layout, m8, dy, wc, bc, wk, bk, scale)."""
    T, B, C, ld, go = c["T"], c["B"], c["C"], c["ld"], c["gate_off"]
    if T * B * ld * 4 >= 0x7FFFFF00:
        u = torch.empty((T, B, ld), dtype=torch.float32, device=dev)          # allocated, not touched
    else:
        off = 1 if c["u_mis"] else 0
        u = torch.full((off + T * B * ld,), NAN, dtype=torch.float32, device=dev)[off:].view(T, B, ld)
        assert u.data_ptr() % 16 == (4 if c["u_mis"] else 0)
    u[..., :C] = t["x"].to(dev)
    if c["gate"]:
        u[..., go:go + C] = t["gate"].to(dev)
    m8 = None if t["mask"] is None else t["mask"].to(torch.uint8).to(dev).contiguous()
    return (u, m8) + tuple(_to(dev, t, "dy", "wc", "bc", "wk", "bk", "scale"))


def _cm_prefill(dev, c, t, exact):
    """The accumulators of the parameter gradients: N(0,1) (small integers on the exact run), or None."""
    want = dict(dwc=c["causal"], dbc=c["causal"] and c["bias"], dwk=True, dbk=c["bias"],
                dscale=c["scale"] and c["dscale"])
    pre = {k: ((t["pre_" + k] * 3).round() if exact else t["pre_" + k]).to(dev) for k in GRADS if want[k]}
    return pre, [Buf(dev, pre[k].shape, src=pre[k]) if k in pre else None for k in GRADS]


def _cm_run(dev, name, exact, monkeypatch):
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name, exact)
    if c["blocks"] is None:
        monkeypatch.delenv("S2T_CONV_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("S2T_CONV_BLOCKS", str(c["blocks"]))
    T, B, C, K, ld, go = c["T"], c["B"], c["C"], c["K"], c["ld"], c["gate_off"]
    chunk = c["chunk"] or T
    u, m8, dy, wc, bc, wk, bk, scale = _cm_operands(dev, c, t)
    pre, acc = _cm_prefill(dev, c, t, exact)
    nout = 2 * C if c["gate"] else C
    if c["via"] == "wrapper":
        from speech2text_amd import zip_kernels as zk
        y = zk.zipconv_forward(u, go, m8, chunk, K, wc, bc, wk, bk, scale)
        du = zk.zipconv_backward(u, go, m8, chunk, K, wc, wk, bk, scale, dy,
                                 [None if a is None else a.t for a in acc], side=False)
        assert y.shape == (T, B, C) and du.shape == (T, B, nout)
    else:
        yo, duo = Buf(dev, (T, B, C), mis=c["out_mis"]), Buf(dev, (T, B, nout), mis=c["out_mis"])
        ws = Buf(dev, lib.s2t_zipconv_bwd_workspace_floats(T, B, C, K))
        N.check(lib.s2t_zipconv_fwd(ptr(u), ld, go, ptr(m8), T, B, C, K, chunk, ptr(wc), ptr(bc), ptr(wk), ptr(bk),
                                    ptr(scale), ptr(yo), st), "s2t_zipconv_fwd")
        N.check(lib.s2t_zipconv_bwd(ptr(u), ld, go, ptr(m8), T, B, C, K, chunk, ptr(wc), ptr(wk), ptr(bk), ptr(scale),
                                    ptr(dy), ptr(duo), *[ptr(a) for a in acc], ptr(ws), st), "s2t_zipconv_bwd")
        torch.cuda.synchronize()
        for what, o in (("y", yo), ("du", duo), ("workspace", ws)):
            o.intact(f"{name} {what}")
        y, du = yo.t, duo.t
    torch.cuda.synchronize()
    got = dict(y=y, du=du)
    for k, a in zip(GRADS, acc):
        if a is not None:
            a.intact(f"{name} {k}")
            got[k] = a.t - pre[k]
    _hold(name, got, exact=exact)
    return got


@pytest.mark.parametrize("name", COVER["cm_run"])
def test_conv_module_vs_float64(dev, monkeypatch, name):
    """s2t_zipconv_fwd and s2t_zipconv_bwd, through zk.zipconv_forward / zipconv_backward(side=False)
    where the wrapper can express the case and through the C ABI on NaN-filled buffers of the test's own
    where it cannot (or where what is written matters: frame edges, the reduction's partial slots).
    Then once more in the same layout on the exactly representable inputs (gate pre-activation 100, a
    sigmoid of exactly 1): y, du and the tap / bias gradients bit-equal to the reference."""
    got = _cm_run(dev, name, False, monkeypatch)
    if name == "op_allpad":
        assert not bool(got["du"][:, 1].any()), "the gradient of an all-padding utterance is exactly zero"
    if ZC.has_exact(name) and name not in ZC.EXACT_DROPPED:
        _cm_run(dev, name, True, monkeypatch)


@pytest.mark.parametrize("name", COVER["cm_glu"])
def test_conv_module_through_the_autograd_wrapper(dev, monkeypatch, name):
    """glu_chunk_causal_dwconv with chunk_size > T: the wrapper folds it to one chunk of T frames."""
    from speech2text_amd import zip_kernels as zk
    monkeypatch.delenv("S2T_CONV_BLOCKS", raising=False)
    c, t = ZC.CASES[name], ZC.make(name)
    T, C, K = c["T"], c["C"], c["K"]
    P = torch.nn.Parameter
    x, gate, dy, wc, bc, wk, bk, scale = _to(dev, t, "x", "gate", "dy", "wc", "bc", "wk", "bk", "scale")
    conv = types.SimpleNamespace(
        kernel_size=K, causal_conv=types.SimpleNamespace(weight=P(wc.view(C, 1, -1)), bias=P(bc)),
        chunkwise_conv=types.SimpleNamespace(weight=P(wk.view(C, 1, K)), bias=P(bk)), chunkwise_conv_scale=P(scale))
    u = torch.cat((x, gate), -1).requires_grad_(True)
    y = zk.glu_chunk_causal_dwconv(u, C, t["mask"].to(dev), conv, T + 24)
    y.backward(dy)
    _hold(name, dict(y=y, du=u.grad, dwc=conv.causal_conv.weight.grad, dbc=conv.causal_conv.bias.grad,
                     dwk=conv.chunkwise_conv.weight.grad, dbk=conv.chunkwise_conv.bias.grad,
                     dscale=conv.chunkwise_conv_scale.grad))


@pytest.mark.parametrize("name", COVER["cm_split"])
def test_conv_module_split_backward_equals_the_joint_one(dev, monkeypatch, name):
    """s2t_zipconv_bwd against s2t_zipconv_bwd_data + s2t_zipconv_bwd_params: the same kernels and a
    deterministic reduction, so du and the tap / bias gradients are bit-equal; dscale goes through float
    atomics and is held to its bound in both."""
    N, lib, st = env()
    monkeypatch.delenv("S2T_CONV_BLOCKS", raising=False)
    c, t = ZC.CASES[name], ZC.make(name)
    T, B, C, K, ld, go = c["T"], c["B"], c["C"], c["K"], c["ld"], c["gate_off"]
    chunk = c["chunk"] or T
    u, m8, dy, wc, bc, wk, bk, scale = _cm_operands(dev, c, t)
    yo = Buf(dev, (T, B, C))
    N.check(lib.s2t_zipconv_fwd(ptr(u), ld, go, ptr(m8), T, B, C, K, chunk, ptr(wc), ptr(bc), ptr(wk), ptr(bk),
                                ptr(scale), ptr(yo), st), "s2t_zipconv_fwd")
    res = []
    for split in (False, True):
        pre, acc = _cm_prefill(dev, c, t, False)
        duo, ws = Buf(dev, (T, B, 2 * C)), Buf(dev, lib.s2t_zipconv_bwd_workspace_floats(T, B, C, K))
        head = (ptr(u), ld, go, ptr(m8), T, B, C, K, chunk, ptr(wc), ptr(wk), ptr(bk), ptr(scale), ptr(dy))
        gp = [ptr(a) for a in acc]
        if split:
            N.check(lib.s2t_zipconv_bwd_data(*head, ptr(duo), st), "s2t_zipconv_bwd_data")
            N.check(lib.s2t_zipconv_bwd_params(*head, *gp, ptr(ws), st), "s2t_zipconv_bwd_params")
        else:
            N.check(lib.s2t_zipconv_bwd(*head, ptr(duo), *gp, ptr(ws), st), "s2t_zipconv_bwd")
        torch.cuda.synchronize()
        for what, o in [("du", duo), ("workspace", ws)] + [(k, a) for k, a in zip(GRADS, acc) if a is not None]:
            o.intact(f"{name} {what}")
        raw = dict(du=duo.t.clone(), **{k: a.t.clone() for k, a in zip(GRADS, acc) if a is not None})
        _hold(name, dict(y=yo.t, du=duo.t, **{k: raw[k] - pre[k] for k in pre}))
        res.append(raw)
    for k in res[0]:
        if k != "dscale":
            assert torch.equal(res[0][k], res[1][k]), f"{name} {k}: the split backward differs from the joint one"


@pytest.mark.parametrize("name", COVER["cm_act"])
def test_conv_module_activation_output(dev, name):
    """s2t_zipconv_fwd_act: y as the plain forward's, y_act bit-equal to the standalone Swoosh forward of
    the kernel's own y ("the same instruction sequence") and within the bound of float64 Swoosh of it."""
    from speech2text_amd import zip_kernels as zk
    N, lib, st = env()
    c, t = ZC.CASES[name], ZC.make(name)
    T, B, C, K, ld, go = c["T"], c["B"], c["C"], c["K"], c["ld"], c["gate_off"]
    u, m8, _, wc, bc, wk, bk, scale = _cm_operands(dev, c, t)
    yo, ya, y0 = Buf(dev, (T, B, C)), Buf(dev, (T, B, C)), Buf(dev, (T, B, C))
    head = (ptr(u), ld, go, ptr(m8), T, B, C, K, c["chunk"], ptr(wc), ptr(bc), ptr(wk), ptr(bk), ptr(scale))
    N.check(lib.s2t_zipconv_fwd_act(*head, ptr(yo), ptr(ya), 1 if c["is_l"] else 2, st), "s2t_zipconv_fwd_act")
    N.check(lib.s2t_zipconv_fwd(*head, ptr(y0), st), "s2t_zipconv_fwd")
    torch.cuda.synchronize()
    for what, o in (("y", yo), ("y_act", ya), ("y (plain)", y0)):
        o.intact(f"{name} {what}")
    _hold(name, dict(y=yo.t, y_act=ya.t))
    assert torch.equal(yo.t, y0.t)
    assert torch.equal(ya.t, zk.swoosh_forward(yo.t.contiguous(), c["is_l"]).view(T, B, C))
    err = ZC.rel_err(ya.t, ZF.swoosh_ref(yo.t.double().cpu(), c["is_l"]))
    print(f"{name} y_act against float64 Swoosh of the kernel's y: err {err:.3e}")
    assert err <= ZC.bound(name, "y_act")
    n = len(ZC.SAT10)
    assert float((yo.t[7, 0, :n].cpu() - torch.tensor(ZC.SAT10)).abs().max()) < 0.05      # on the saturation points


@pytest.mark.parametrize("bad", ZC.CM_REFUSALS, ids=lambda d: "_".join(f"{k}{v}" for k, v in d.items()))
def test_conv_module_refusals(dev, bad):
    N, lib, st = env()
    a = dict(T=8, B=2, C=8, K=7, chunk=4)
    a.update(bad)
    T, B, C, K, chunk = (a[k] for k in ("T", "B", "C", "K", "chunk"))
    z = lambda *s: torch.zeros(*s, device=dev)                                  # noqa: E731
    u, dy, wc, bc, wk, bk, scale = z(8, 2, 16), z(8, 2, 8), z(8, 16), z(8), z(8, 31), z(8), z(2, 8, 31)
    yo, ya, duo, ws = Buf(dev, (8, 2, 8)), Buf(dev, (8, 2, 8)), Buf(dev, (8, 2, 16)), Buf(dev, 1 << 16)
    acc = [Buf(dev, s) for s in ((8, 16), (8,), (8, 31), (8,), (2, 8, 31))]
    head = (ptr(u), 16, 8, None, T, B, C, K, chunk, ptr(wc))
    assert lib.s2t_zipconv_fwd(*head, ptr(bc), ptr(wk), ptr(bk), ptr(scale), ptr(yo), st) == -1
    assert lib.s2t_zipconv_fwd_act(*head, ptr(bc), ptr(wk), ptr(bk), ptr(scale), ptr(yo), ptr(ya), 1, st) == -1
    assert lib.s2t_zipconv_bwd(*head, ptr(wk), ptr(bk), ptr(scale), ptr(dy), ptr(duo), *[ptr(o) for o in acc], ptr(ws), st) == -1
    assert lib.s2t_zipconv_bwd_data(*head, ptr(wk), ptr(bk), ptr(scale), ptr(dy), ptr(duo), st) == -1
    torch.cuda.synchronize()
    for o in [yo, ya, duo, ws] + acc:
        o.untouched(f"refused {bad}")


def test_conv_module_activation_refusals(dev):
    N, lib, st = env()
    z = lambda *s: torch.zeros(*s, device=dev)                                  # noqa: E731
    u, wc, bc, wk, bk, scale = z(8, 2, 16), z(8, 4), z(8), z(8, 7), z(8), z(2, 8, 7)
    yo, ya = Buf(dev, (8, 2, 8)), Buf(dev, (8, 2, 8))
    head = (ptr(u), 16, 8, None, 8, 2, 8, 7, 4, ptr(wc), ptr(bc), ptr(wk), ptr(bk), ptr(scale))
    assert lib.s2t_zipconv_fwd_act(*head, ptr(yo), ptr(ya), 3, st) == -1
    assert lib.s2t_zipconv_fwd_act(*head, ptr(yo), ptr(ya), 0, st) == -1
    assert lib.s2t_zipconv_fwd_act(*head, ptr(yo), None, 1, st) == -1
    torch.cuda.synchronize()
    yo.untouched("refused activation")
    ya.untouched("refused activation")


# ------------------------------------------------------------------ frontend: depthwise conv
@pytest.mark.parametrize("name", COVER["dw"])
def test_dwconv2d_forward_vs_float64(dev, name):
    """s2t_dwconv2d_nhwc_fwd / _fwd_add (the roll kernel for 7x7, the strip kernel for 3x3) with flip = 0
    and flip = 1, on the random and on the exact inputs."""
    N, lib, st = env()
    c = ZC.CASES[name]
    Nn, H, W, C, K = c["N"], c["H"], c["W"], c["C"], c["K"]
    for exact in (False, True):
        x, w, b, add = _to(dev, ZC.make(name, exact), "x", "w", "bias", "add")
        got = {}
        for flip in (0, 1):
            y = Buf(dev, (Nn, H, W, C))
            if c["add"]:
                rc = lib.s2t_dwconv2d_nhwc_fwd_add(ptr(x), ptr(w), ptr(b), ptr(add), Nn, H, W, C, K, K, flip, ptr(y), st)
            else:
                rc = lib.s2t_dwconv2d_nhwc_fwd(ptr(x), ptr(w), ptr(b), Nn, H, W, C, K, K, flip, ptr(y), st)
            assert rc == 0
            torch.cuda.synchronize()
            y.intact(f"{name} flip {flip}")
            got[f"y{flip}"] = y.t
        _hold(name, got, exact=exact)


def test_dwconv2d_forward_refusals(dev):
    N, lib, st = env()
    x, w3, w5, add = (torch.zeros(*s, device=dev) for s in ((1, 4, 4, 8), (8, 3, 3), (8, 5, 5), (1, 4, 4, 8)))
    y = Buf(dev, (1, 4, 4, 8))
    assert lib.s2t_dwconv2d_nhwc_fwd_add(ptr(x), ptr(w3), None, ptr(add), 1, 4, 4, 8, 3, 3, 1, ptr(y), st) == -2
    assert lib.s2t_dwconv2d_nhwc_fwd(ptr(x), ptr(w5), None, 1, 4, 4, 8, 5, 5, 0, ptr(y), st) == -1
    assert lib.s2t_dwconv2d_nhwc_fwd(ptr(x), ptr(w3), None, 0, 4, 4, 8, 3, 3, 0, ptr(y), st) == 0       # N = 0: nothing to do
    torch.cuda.synchronize()
    y.untouched("refused depthwise conv")


@pytest.mark.parametrize("name", COVER["wg"])
def test_dwconv2d_weight_gradient_vs_float64(dev, name):
    """s2t_dwconv2d_nhwc_wgrad on a NaN workspace of exactly s2t_dwconv2d_wgrad_workspace_floats with a
    guard of the same size behind it; the path (ring / roll MODE 2 / generic) is zipconv_cases.wgrad_path's,
    asserted on the CPU."""
    N, lib, st = env()
    c = ZC.CASES[name]
    Nn, H, W, C, K = c["N"], c["H"], c["W"], c["C"], c["K"]
    x, dy = _to(dev, ZC.make(name), "x", "dy")
    nws = lib.s2t_dwconv2d_wgrad_workspace_floats(Nn, H, C, K, K)
    assert nws == (H + 7) // 8 * Nn * ((C + 63) // 64) * 64 * (K * K + 1)
    ws = Buf(dev, nws)
    dw, db = Buf(dev, (C, K, K)), (Buf(dev, C) if c["db"] else None)
    assert lib.s2t_dwconv2d_nhwc_wgrad(ptr(x), ptr(dy), Nn, H, W, C, K, K, ptr(ws), ptr(dw), ptr(db), st) == 0
    torch.cuda.synchronize()
    ws.intact(f"{name} workspace")
    dw.intact(f"{name} dw")
    got = dict(dw=dw.t)
    if db is not None:
        db.intact(f"{name} db")
        got["db"] = db.t
    _hold(name, got)


# ------------------------------------------------------------------ frontend: the two subsampling convs
@pytest.mark.parametrize("name", COVER["c1"])
def test_conv3x3_c1_vs_float64(dev, name):
    """s2t_conv3x3_c1 modes 0 (y), 1 (dw / db accumulated into N(0,1)) and 2 (dx); forward and data
    gradient also on the exact inputs."""
    N, lib, st = env()
    c = ZC.CASES[name]
    B, H, W, pw = c["B"], c["H"], c["W"], c["pw"]
    Ho, Wo = H - 2, W + 2 * pw - 2
    for exact in (False, True):
        t = ZC.make(name, exact)
        x, w, b, g, pdw, pdb = _to(dev, t, "x", "w", "bias", "g", "pre_dw", "pre_db")
        y, dx = Buf(dev, (B, Ho, Wo, 8)), Buf(dev, (B, H, W))
        tail = (B, H, W, pw, 8)
        assert lib.s2t_conv3x3_c1(0, ptr(x), ptr(w), ptr(b), None, *tail, ptr(y), None, None, None, st) == 0
        assert lib.s2t_conv3x3_c1(2, None, ptr(w), None, ptr(g), *tail, None, None, None, ptr(dx), st) == 0
        torch.cuda.synchronize()
        y.intact(f"{name} y")
        dx.intact(f"{name} dx")
        got = dict(y=y.t, dx=dx.t)
        if not exact:
            dw, db = Buf(dev, 72, src=pdw), Buf(dev, 8, src=pdb)
            assert lib.s2t_conv3x3_c1(1, ptr(x), None, None, ptr(g), *tail, None, ptr(dw), ptr(db), None, st) == 0
            torch.cuda.synchronize()
            dw.intact(f"{name} dw")
            db.intact(f"{name} db")
            got.update(dw=dw.t - pdw, db=db.t - pdb)
        _hold(name, got, exact=exact, partial=exact)


def test_conv3x3_c1_refusals(dev):
    N, lib, st = env()
    x, w, b, g = (torch.zeros(*s, device=dev) for s in ((2, 5, 4), (16, 1, 3, 3), (16,), (2, 3, 4, 16)))
    y, dw, db, dx = Buf(dev, (2, 3, 4, 16)), Buf(dev, 144), Buf(dev, 16), Buf(dev, (2, 5, 4))
    call = lambda mode, W, pw, CO: lib.s2t_conv3x3_c1(mode, ptr(x), ptr(w), ptr(b), ptr(g), 2, 5, W, pw, CO, ptr(y),     # noqa: E731
                                                      ptr(dw), ptr(db), ptr(dx), st)
    assert call(0, 2, 0, 8) == -1          # no output column
    assert call(0, 4, 1, 16) == -2         # only CO = 8 is instantiated
    assert call(0, 4, 2, 8) == -2
    assert call(3, 4, 1, 8) == -1
    torch.cuda.synchronize()
    for o in (y, dw, db, dx):
        o.untouched("refused conv3x3_c1")


@pytest.mark.parametrize("name", COVER["s2"])
def test_conv3x3_s2_vs_float64(dev, name):
    """s2t_conv3x3_s2 modes 0 and 2; an even H's last row and an even W's last column receive no tap and
    come out exactly zero."""
    N, lib, st = env()
    c = ZC.CASES[name]
    B, H, W = c["B"], c["H"], c["W"]
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    for exact in (False, True):
        x, w, b, g = _to(dev, ZC.make(name, exact), "x", "w", "bias", "g")
        y, dx = Buf(dev, (B, Ho, Wo, 32)), Buf(dev, (B, H, W, 8))
        assert lib.s2t_conv3x3_s2(0, ptr(x), ptr(w), ptr(b), None, B, H, W, 8, 32, ptr(y), None, st) == 0
        assert lib.s2t_conv3x3_s2(2, None, ptr(w), None, ptr(g), B, H, W, 8, 32, None, ptr(dx), st) == 0
        torch.cuda.synchronize()
        y.intact(f"{name} y")
        dx.intact(f"{name} dx")
        _hold(name, dict(y=y.t, dx=dx.t), exact=exact)
        if H % 2 == 0:
            assert not bool(dx.t[:, -1].any())
        if W % 2 == 0:
            assert not bool(dx.t[:, :, -1].any())


def test_conv3x3_s2_refusals(dev):
    N, lib, st = env()
    x, w, b, g = (torch.zeros(*s, device=dev) for s in ((2, 5, 5, 8), (32, 8, 3, 3), (32,), (2, 2, 2, 32)))
    y, dx = Buf(dev, (2, 2, 2, 32)), Buf(dev, (2, 5, 5, 8))
    assert lib.s2t_conv3x3_s2(0, ptr(x), ptr(w), ptr(b), ptr(g), 2, 5, 5, 4, 32, ptr(y), ptr(dx), st) == -2
    assert lib.s2t_conv3x3_s2(0, ptr(x), ptr(w), ptr(b), ptr(g), 2, 5, 2, 8, 32, ptr(y), ptr(dx), st) == -1
    assert lib.s2t_conv3x3_s2(2, ptr(x), ptr(w), ptr(b), ptr(g), 2, 5, 2, 8, 32, ptr(y), ptr(dx), st) == -1
    torch.cuda.synchronize()
    y.untouched("refused conv3x3_s2")
    dx.untouched("refused conv3x3_s2")


@pytest.mark.parametrize("name", COVER["c2i"])
def test_col2im3x3_vs_float64(dev, name):
    N, lib, st = env()
    c = ZC.CASES[name]
    B, H, W, C, sh, sw = (c[k] for k in ("B", "H", "W", "C", "sh", "sw"))
    Ho, Wo = (H - 3) // sh + 1, (W - 3) // sw + 1
    for exact in (False, True):
        dc, = _to(dev, ZC.make(name, exact), "dc")
        dx = Buf(dev, (B, H, W, C))
        assert lib.s2t_col2im3x3_nhwc(ptr(dc), B, H, W, C, Ho + 1, Wo, sh, sw, ptr(dx), st) == -1
        torch.cuda.synchronize()
        dx.untouched(f"{name}: a wrong Ho")
        assert lib.s2t_col2im3x3_nhwc(ptr(dc), B, H, W, C, Ho, Wo, sh, sw, ptr(dx), st) == 0
        torch.cuda.synchronize()
        dx.intact(f"{name} dx")
        _hold(name, dict(dx=dx.t), exact=exact)
