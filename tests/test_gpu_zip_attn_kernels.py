"""GPU: the zipformer's attention kernels (csrc/zip_attn.hip: the relative-position attention weights on the
MFMA and on the general kernel, the penalty flag, the three-launch backward with factored dW, the value apply
in its 16-byte and scalar form) and the Whiten / limit_param_value kernels (csrc/whiten.hip: all ten entry
points) against the float64 yardstick tests/zipattn_f64.py, through the C ABI, at every launch-time branch
(tests/zipattn_cases.py names why each shape is there).

Error = max |got - ref| / max |ref| per tensor; allowed = zipattn_cases.bound(case, tensor) = max(2e-5, 8 x the
case's float32 figure of the YARDSTICK, asserted by tests/test_zipattn_f64.py).  Every output and workspace
is a guarded buffer of tests/guarded.py: it starts as NaN with a NaN guard behind it and one word in front,
and must come out finite with the guards intact; dpos starts NaN (the entry point clears it); accumulators start from N(0,1) and are compared as
got - prefill.  A call the entry point must refuse returns its code and leaves its outputs NaN.
"""
import functools

import pytest
import torch

import zipattn_cases as ZA
from guarded import NAN, Buf, env, hold, ptr

pytestmark = pytest.mark.gpu

_hold = functools.partial(hold, ZA, partial=True)

COVER = dict(fw=ZA.names("fw"), fl=ZA.names("fl"), bw=ZA.names("bw"), ap=ZA.names("ap"), wm=ZA.names("wm"),
             wx=ZA.names("wx"), wd=ZA.names("wd"), wa=ZA.names("wa"), lp=ZA.names("lp"))
# test -> (the COVER key it is parametrised over, the entry points it calls itself or through HELPERS)
RUNS = dict(
    test_attention_weights_vs_float64=("fw", ("s2t_relpos_attn_fwd",)),
    test_attention_penalty_flag=("fl", ("s2t_relpos_attn_fwd_flag",)),
    test_attention_backward_vs_float64=("bw", ("s2t_relpos_attn_bwd", "s2t_relpos_attn_bwd_workspace_floats")),
    test_attention_apply_vs_float64=("ap", ("s2t_attn_apply",)),
    test_whiten_metric_vs_float64=("wm", ("s2t_whiten_metric",)),
    test_whiten_metric_after_the_xtx_product=("wx", ("s2t_whiten_metric",)),
    test_whiten_dcov_and_prep_vs_float64=("wd", ("s2t_whiten_dcov", "s2t_whiten_prep")),
    test_whiten_streams_vs_float64=("wa", ("s2t_whiten_combine64", "s2t_whiten_apply", "s2t_whiten_combine")),
    test_limit_param_grad_is_bit_exact=("lp", ("s2t_limit_param_grad",)))
HELPERS = dict(test_attention_weights_vs_float64=("_fw_run",), test_attention_penalty_flag=("_fw_run",),
               test_attention_backward_vs_float64=("_bw_run",), test_whiten_metric_vs_float64=("_metric",),
               test_whiten_metric_after_the_xtx_product=("_metric",))


def _in(dev, v, mis=False):
    """A float32 device copy of v; mis: its first element is 4 bytes past a multiple of 16."""
    if v is None:
        return None
    buf = torch.full((v.numel() + 1,), NAN, dtype=torch.float32, device=dev)
    o = buf[1:] if mis else buf[:-1]
    o = o.view(v.shape)
    o.copy_(v)
    assert o.data_ptr() % 16 == (4 if mis else 0)
    return o


def _u8(dev, m):
    return None if m is None else m.to(torch.uint8).to(dev).contiguous()


# ------------------------------------------------------------------ attention weights
def _fw_run(dev, name, flag=None):
    _, lib, st = env()
    c, t = ZA.CASES[name], ZA.make(name)
    T, B, H, qd, pd = c["T"], c["B"], c["H"], c["qd"], c["pd"]
    qkp, pos = _in(dev, t["qkp"], "qkp" in c["mis"]), _in(dev, t["pos"], "pos" in c["mis"])
    if pd == 0:
        pos = torch.full((8,), NAN, dtype=torch.float32, device=dev)          # not NULL, and never read
    k8, a8 = _u8(dev, t["kpm"]), _u8(dev, t["amask"])
    W = Buf(dev, (H, B, T, T))
    if flag is None:
        rc = lib.s2t_relpos_attn_fwd(ptr(qkp), ptr(pos), ptr(k8), ptr(a8), T, B, H, qd, pd, ptr(W), st)
    else:
        rc = lib.s2t_relpos_attn_fwd_flag(ptr(qkp), ptr(pos), ptr(k8), ptr(a8), T, B, H, qd, pd, ptr(W), ZA.LIMIT, ptr(flag), st)
    torch.cuda.synchronize()
    return rc, W


def _masked_rows_exact(name, W):
    c = ZA.CASES[name]
    rows, utts = ZA.masked_rows(c)
    if rows:
        inv = torch.tensor(1.0 / c["T"], dtype=torch.float32, device=W.device)
        assert bool((W[:, :, rows] == inv).all()), f"{name}: a row masked by the attention mask is not float32(1 / T)"
        assert bool((W[:, utts] == inv).all()), f"{name}: the rows of an all-padding utterance are not float32(1 / T)"


@pytest.mark.parametrize("name", COVER["fw"])
def test_attention_weights_vs_float64(dev, name):
    """s2t_relpos_attn_fwd on the kernel the case names; rows without a live key are exactly float32(1 / T)
    (__expf(0) == 1 and the row sum is T); pd == 0 ignores a non-NULL pos."""
    rc, W = _fw_run(dev, name)
    assert rc == 0
    W.intact(f"{name} W")
    _hold(name, dict(W=W.t))
    _masked_rows_exact(name, W.t)


@pytest.mark.parametrize("name", COVER["fl"])
def test_attention_penalty_flag(dev, name):
    """s2t_relpos_attn_fwd_flag: the flag is 1 exactly when a raw score of the float64 yardstick exceeds the
    limit (before masking, rows and keys past T not counted); W as the plain entry's."""
    flag = Buf(dev, 1, src=torch.zeros(1))
    rc, W = _fw_run(dev, name, flag)
    assert rc == 0
    W.intact(f"{name} W")
    flag.intact(f"{name} flag")
    _hold(name, dict(W=W.t))
    assert float(flag.t[0]) == (1.0 if ZA.flag_expected(name) else 0.0), name
    rc, W2 = _fw_run(dev, name)
    assert rc == 0 and torch.equal(W.t, W2.t)


def test_attention_penalty_flag_is_refused_outside_the_mfma_kernel(dev):
    flag = Buf(dev, 1, src=torch.zeros(1))
    rc, W = _fw_run(dev, "fw_g_qd4", flag)
    assert rc == -3
    W.untouched("flag on the general kernel")
    assert float(flag.t[0]) == 0.0


@pytest.mark.parametrize("bad", ZA.FW_REFUSALS, ids=lambda d: "_".join(f"{k}{v}" for k, v in d.items()))
def test_attention_forward_refusals(dev, bad):
    _, lib, st = env()
    a = dict(T=8, B=2, H=2, qd=8, pd=4)
    a.update(bad)
    qkp, pos = torch.zeros(8, 2, 2 * 80, device=dev), torch.zeros(15, 16, device=dev)
    W, flag = Buf(dev, (2, 2, 8, 8)), Buf(dev, 1)
    head = (ptr(qkp), ptr(pos), None, None, a["T"], a["B"], a["H"], a["qd"], a["pd"], ptr(W))
    assert lib.s2t_relpos_attn_fwd(*head, st) == -1
    assert lib.s2t_relpos_attn_fwd_flag(*head, ZA.LIMIT, ptr(flag), st) == -1
    torch.cuda.synchronize()
    W.untouched(f"refused {bad}")
    flag.untouched(f"refused {bad}")


# ------------------------------------------------------------------ attention backward
def _bw_run(dev, name, dead_scale=1.0, bad=None):
    """s2t_relpos_attn_bwd on the case (W and delta = the float64 ones rounded) -> (rc, {name: Buf}).
    dead_scale multiplies dW, dO and delta of the rows without a live key."""
    _, lib, st = env()
    c, t, ref = ZA.CASES[name], ZA.make(name), ZA.reference(name)
    T, B, H, qd, pd = c["T"], c["B"], c["H"], c["qd"], c["pd"]
    Dp = H * (2 * qd + pd)
    qkp, pos = _in(dev, t["qkp"]), _in(dev, t["pos"])
    if pd == 0:
        pos = torch.full((8,), NAN, dtype=torch.float32, device=dev)          # not NULL, and never read
    k8, a8 = _u8(dev, t["kpm"]), _u8(dev, t["amask"])
    W = _in(dev, ref["_W"].float())
    dW, dW0 = _in(dev, t["dW"]), _in(dev, t["dW0"])
    pairs = [(_in(dev, a), _in(dev, b), dv) for (a, b), dv in zip(t["pairs"], c["dvs"])]
    dl = ref["_delta"].float()
    if dead_scale != 1.0:
        rows, utts = ZA.masked_rows(c)
        for x in [dW, dl.unsqueeze(-1)]:
            x[:, :, rows] *= dead_scale
            x[:, utts] *= dead_scale
        for a, _, _ in pairs:
            a[rows] *= dead_scale
            a[:, utts] *= dead_scale
    pairs += [(None, None, 0)] * (2 - len(pairs))
    given = int(c["given"])
    o = dict(delta=Buf(dev, (H, B, T), src=dl if given else None), dqkp=Buf(dev, (T, B, Dp)))
    nws = lib.s2t_relpos_attn_bwd_workspace_floats(T, B, H, pd)
    nj = (T + 31) // 32
    assert nws == B * H * nj * (nj + 1) * 32 * pd
    if pos is not None and pd > 0:
        o.update(dpos=Buf(dev, (2 * T - 1, H * pd)), ws=Buf(dev, nws))
    if bad == "cd33":
        pairs = [(pairs[0][0], pairs[0][1], 17), (pairs[0][0], pairs[0][1], 16)]
    if bad == "no_dw_no_delta":
        dW, given = None, 0
    if bad == "pos_no_workspace":
        o.pop("ws")
    if bad == "qd0":
        qd = 0
    if bad == "pd9":
        pd = 9
    rc = lib.s2t_relpos_attn_bwd(ptr(qkp), ptr(pos), ptr(k8), ptr(a8), T, B, H, qd, pd, ptr(W), ptr(dW), ptr(dW0),
                                 ptr(pairs[0][0]), ptr(pairs[0][1]), pairs[0][2], ptr(pairs[1][0]), ptr(pairs[1][1]),
                                 pairs[1][2], given, ptr(o["delta"]), ptr(o["dqkp"]), ptr(o.get("dpos")), ptr(o.get("ws")), st)
    torch.cuda.synchronize()
    return rc, o


@pytest.mark.parametrize("name", COVER["bw"])
def test_attention_backward_vs_float64(dev, name):
    """s2t_relpos_attn_bwd: dqkp and dpos fully written from NaN, the workspace (exactly
    s2t_relpos_attn_bwd_workspace_floats, NaN at the start) fully written, delta written when it is not given.
    Rows without a live key: dq and dp exactly zero, and nothing of them in dk or dpos (their dW x 1e6 leaves
    every output bit-identical).  pos NULL: the p columns of dqkp are exactly zero."""
    c = ZA.CASES[name]
    rc, o = _bw_run(dev, name)
    assert rc == 0
    for k, v in o.items():
        v.intact(f"{name} {k}")
        assert bool(torch.isfinite(v.t).all()), f"{name} {k}: not fully written"
    got = dict(dqkp=o["dqkp"].t)
    if "dpos" in o:
        got["dpos"] = o["dpos"].t
    if not c["given"]:
        got["delta"] = o["delta"].t
    _hold(name, got)
    H, qd = c["H"], c["qd"]
    if not c["pos"]:
        assert not bool(o["dqkp"].t[..., 2 * H * qd:].any()), f"{name}: dp without a position term"
    rows, utts = ZA.masked_rows(c)
    if rows:
        for sl in (slice(0, H * qd), slice(2 * H * qd, None)):
            assert not bool(o["dqkp"].t[rows][..., sl].any()) and not bool(o["dqkp"].t[:, utts][..., sl].any()), name
        rc, o2 = _bw_run(dev, name, dead_scale=1.0e6)
        assert rc == 0
        for k in ("dqkp", "dpos"):
            assert torch.equal(o[k].t, o2[k].t), f"{name} {k}: a row without a live key reached the result"


@pytest.mark.parametrize("bad", ZA.BW_REFUSALS)
def test_attention_backward_refusals(dev, bad):
    rc, o = _bw_run(dev, "bw_cd12", bad=bad)
    assert rc == -1
    for k, v in o.items():
        if k != "delta":                                     # given: an input
            v.untouched(f"refused {bad}: {k}")


# ------------------------------------------------------------------ value apply
@pytest.mark.parametrize("name", COVER["ap"])
def test_attention_apply_vs_float64(dev, name):
    """s2t_attn_apply, transpose 0 and 1, in the form the case names."""
    _, lib, st = env()
    c, t = ZA.CASES[name], ZA.make(name)
    T, B, H, dv = c["T"], c["B"], c["H"], c["dv"]
    W, v = _in(dev, t["W"]), _in(dev, t["v"], c["mis"] == "v")
    got = {}
    for tr in (0, 1):
        out = Buf(dev, (T, B, H * dv), mis=c["mis"] == "out")
        assert lib.s2t_attn_apply(ptr(W), ptr(v), T, B, H, dv, tr, ptr(out), st) == 0
        torch.cuda.synchronize()
        out.intact(f"{name} transpose {tr}")
        got[f"out{tr}"] = out.t
    _hold(name, got)


@pytest.mark.parametrize("name", ZA.PERM_CASES)
def test_attention_apply_of_a_permutation_is_exact(dev, name):
    """W = a permutation matrix per (h, b): out is the permuted v bit for bit, both ways."""
    _, lib, st = env()
    c, t = ZA.CASES[name], ZA.make(name)
    T, B, H, dv = c["T"], c["B"], c["H"], c["dv"]
    g = torch.Generator().manual_seed(c["seed"])
    perm = torch.stack([torch.randperm(T, generator=g) for _ in range(H * B)]).view(H, B, T)
    Wp = torch.zeros(H, B, T, T).scatter_(3, perm.unsqueeze(-1), 1.0)
    v4 = t["v"].view(T, B, H, dv)
    ref0, ref1 = torch.empty_like(v4), torch.empty_like(v4)
    for h in range(H):
        for b in range(B):
            ref0[:, b, h] = v4[perm[h, b], b, h]             # out0[i] = v[perm(i)]
            ref1[perm[h, b], b, h] = v4[:, b, h]             # out1[perm(i)] = v[i]
    W, v = _in(dev, Wp), _in(dev, t["v"], c["mis"] == "v")
    for tr, ref in ((0, ref0), (1, ref1)):
        out = Buf(dev, (T, B, H * dv), mis=c["mis"] == "out")
        assert lib.s2t_attn_apply(ptr(W), ptr(v), T, B, H, dv, tr, ptr(out), st) == 0
        torch.cuda.synchronize()
        out.intact(f"{name} transpose {tr}")
        assert torch.equal(out.t.cpu(), ref.view(T, B, H * dv)), f"{name} transpose {tr}"


@pytest.mark.parametrize("dv", [17, 0])
def test_attention_apply_refusals(dev, dv):
    _, lib, st = env()
    W, v, out = torch.zeros(2, 2, 8, 8, device=dev), torch.zeros(8, 2, 2 * 17, device=dev), Buf(dev, (8, 2, 2 * 17))
    for tr in (0, 1):
        assert lib.s2t_attn_apply(ptr(W), ptr(v), 8, 2, 2, dv, tr, ptr(out), st) == -1
    torch.cuda.synchronize()
    out.untouched(f"refused dv {dv}")


# ------------------------------------------------------------------ Whiten statistics
STATS = ("cov", "mean", "md", "covsq", "denom", "metric")


def _metric(dev, c, xtx, colsum, ws, host=True):
    """s2t_whiten_metric on NaN outputs -> {tensor: value}, the raw scal and host_metric."""
    _, lib, st = env()
    G, cg = c["G"], c["cg"]
    C = G * cg
    cov, mean, scal, hm = Buf(dev, (G, cg, cg)), Buf(dev, C), Buf(dev, 4), (Buf(dev, 1) if host else None)
    assert lib.s2t_whiten_metric(ptr(xtx), ptr(colsum), ZA.ROWS, G, cg, ptr(cov), ptr(mean), ptr(scal), ptr(hm), ptr(ws), st) == 0
    torch.cuda.synchronize()
    for what, o in (("xtx", xtx), ("colsum", colsum), ("cov", cov), ("mean", mean), ("scal", scal), ("workspace", ws)):
        o.intact(what)
    assert not bool(xtx.t.any()) and not bool(colsum.t.any()), "xtx and colsum are consumed: left exactly zero"
    assert int(ws.t[:1].view(torch.int32)[0]) == 0, "the ticket resets itself"
    assert bool(torch.isfinite(ws.t[4:]).all())
    if hm is not None:
        hm.intact("host_metric")
        assert torch.equal(hm.t, scal.t[3:4])
    s = scal.t
    return dict(cov=cov.t, mean=mean.t, md=s[0:1], covsq=s[1:2], denom=s[2:3], metric=s[3:4])


def _metric_ws(dev, C):
    ws = Buf(dev, 4 + 2 * C)                                 # the partial-sum slots start NaN
    ws.t[0] = 0.0                                            # the ticket: zeroed once when allocated
    return ws


@pytest.mark.parametrize("name", COVER["wm"])
def test_whiten_metric_vs_float64(dev, name):
    """s2t_whiten_metric on xtx holding ONLY the tiles s2t_gemm_xtx writes (every other element NaN), then on
    the full symmetric matrix: bit-equal; a second call on the same workspace, not re-zeroed: bit-equal."""
    c, t = ZA.CASES[name], ZA.make(name)
    C = c["G"] * c["cg"]
    need = ZA.xtx_needed(c["G"], c["cg"])
    tiles = torch.where(need, t["xtx"], torch.tensor(NAN))
    ws = _metric_ws(dev, C)
    res = []
    for src, host in ((tiles, True), (t["xtx"], False), (tiles, True)):
        got = _metric(dev, c, Buf(dev, (C, C), src=src), Buf(dev, C, src=t["colsum"]), ws, host)
        _hold(name, got)
        res.append(got)
    for k in STATS:
        assert torch.equal(res[0][k], res[1][k]), f"{name} {k}: the kernel read outside the tiles of s2t_gemm_xtx"
        assert torch.equal(res[0][k], res[2][k]), f"{name} {k}: a second call on the same workspace differs"


def test_whiten_metric_refusals(dev):
    _, lib, st = env()
    xtx, colsum, ws = torch.zeros(8, 8, device=dev), torch.zeros(8, device=dev), torch.zeros(20, device=dev)
    cov, mean, scal = Buf(dev, (1, 8, 8)), Buf(dev, 8), Buf(dev, 4)
    call = lambda n, G, w: lib.s2t_whiten_metric(ptr(xtx), ptr(colsum), n, G, 8, ptr(cov), ptr(mean), ptr(scal), None, w, st)  # noqa: E731
    assert call(0, 1, ptr(ws)) == -1 and call(10, 0, ptr(ws)) == -1 and call(10, 1, None) == -1
    x65, o65 = torch.zeros(8, 65, device=dev), Buf(dev, (65, 65))
    assert lib.s2t_gemm_xtx(ptr(x65), 65, 8, 65, 65, ptr(o65), 65, ptr(colsum), st) == -2       # C % 4: no wx case at (1, 65)
    torch.cuda.synchronize()
    for o in (cov, mean, scal, o65):
        o.untouched("refused whiten_metric")


@pytest.mark.parametrize("name", COVER["wx"])
def test_whiten_metric_after_the_xtx_product(dev, name):
    """s2t_gemm_xtx -> s2t_whiten_metric from x itself, against the reference's centred form; the product
    leaves everything outside its tiles alone."""
    _, lib, st = env()
    c, t = ZA.CASES[name], ZA.make(name)
    G, cg = c["G"], c["cg"]
    C = G * cg
    x = _in(dev, t["x"])
    xtx, colsum = Buf(dev, (C, C), src=torch.zeros(C, C)), Buf(dev, C, src=torch.zeros(C))
    assert lib.s2t_gemm_xtx(ptr(x), C, ZA.ROWS, C, cg, ptr(xtx), C, ptr(colsum), st) == 0
    torch.cuda.synchronize()
    assert not bool(xtx.t.cpu()[~ZA.xtx_needed(G, cg)].any()), f"{name}: s2t_gemm_xtx wrote outside its tiles"
    _hold(name, _metric(dev, c, xtx, colsum, _metric_ws(dev, C)))


@pytest.mark.parametrize("name", COVER["wd"])
def test_whiten_dcov_and_prep_vs_float64(dev, name):
    """s2t_whiten_dcov and s2t_whiten_prep: dcov from NaN, exactly zero off the block diagonal, symmetric bit
    for bit; sums[0..1] (all 128 slots for _prep) zeroed from NaN."""
    _, lib, st = env()
    c, t = ZA.CASES[name], ZA.make(name)
    G, cg = c["G"], c["cg"]
    C = G * cg
    cov, mean, scal = _in(dev, t["cov"]), _in(dev, t["mean"]), _in(dev, t["scal"])
    i = torch.arange(C, device=dev) // cg
    same = i.unsqueeze(1) == i.unsqueeze(0)
    res = []
    for prep in (False, True):
        dcov, bias, sums = Buf(dev, (C, C)), Buf(dev, C), Buf(dev, 128 if prep else 2)
        fn = lib.s2t_whiten_prep if prep else lib.s2t_whiten_dcov
        assert fn(ptr(cov), ptr(mean), ptr(scal), G, cg, ptr(dcov), ptr(bias), ptr(sums), st) == 0
        torch.cuda.synchronize()
        for what, o in (("dcov", dcov), ("bias", bias), ("sums", sums)):
            o.intact(f"{name} {what}")
        _hold(name, dict(dcov=dcov.t, bias=bias.t))
        assert not bool(dcov.t[~same].any()), f"{name}: dcov off the block diagonal"
        assert torch.equal(dcov.t, dcov.t.t()), f"{name}: dcov is not symmetric"
        assert not bool(sums.t.any()), f"{name}: sums not zeroed"
        res.append((dcov.t, bias.t))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    dcov, bias = Buf(dev, (C, C)), Buf(dev, C)
    assert lib.s2t_whiten_prep(ptr(cov), ptr(mean), ptr(scal), G, cg, ptr(dcov), ptr(bias), None, st) == -1
    assert lib.s2t_whiten_dcov(ptr(cov), ptr(mean), ptr(scal), 0, cg, ptr(dcov), ptr(bias), None, st) == -1
    torch.cuda.synchronize()
    dcov.untouched(f"{name}: refused")
    bias.untouched(f"{name}: refused")


# ------------------------------------------------------------------ Whiten streams, limit_param_grad
@pytest.mark.parametrize("name", COVER["wa"])
def test_whiten_streams_vs_float64(dev, name):
    """s2t_whiten_combine64 on the yardstick's two sums (as float32, in one slot of each row of the [2][64]
    slots, the others zero); s2t_whiten_apply (its own sums pass) and s2t_whiten_combine on those sums."""
    _, lib, st = env()
    c, t = ZA.CASES[name], ZA.make(name)
    n, gs = c["n"], ZA.GRAD_SCALE
    g, pg = _in(dev, t["g"]), _in(dev, t["pg"])
    ref = ZA.reference(name)
    s64 = torch.zeros(128)
    s64[5], s64[64 + 41] = float(ref["ssg"]), float(ref["sspg"])
    clean = Buf(dev, 128, src=s64)
    o64, oa, oc, sums = Buf(dev, n), Buf(dev, n), Buf(dev, n), Buf(dev, 2, src=torch.zeros(2))
    assert lib.s2t_whiten_combine64(ptr(g), ptr(pg), n, gs, ptr(clean), ptr(o64), st) == 0
    assert lib.s2t_whiten_apply(ptr(g), ptr(pg), n, gs, ptr(sums), ptr(oa), st) == 0
    assert lib.s2t_whiten_combine(ptr(g), ptr(pg), n, gs, ptr(sums), ptr(oc), st) == 0
    torch.cuda.synchronize()
    for what, o in (("sums64", clean), ("combine64", o64), ("apply", oa), ("combine", oc), ("sums", sums)):
        o.intact(f"{name} {what}")
    assert torch.equal(clean.t.cpu(), s64), f"{name}: combine64 wrote to its sums"
    _hold(name, dict(ssg=sums.t[0:1], sspg=sums.t[1:2], out=oa.t))
    _hold(name, dict(out=o64.t))
    assert torch.equal(oa.t, oc.t), f"{name}: combine differs from apply on the same sums"
    if c["kind"] == "pgzero":
        assert torch.equal(oa.t, g) and torch.equal(o64.t, g)
    if c["kind"] == "gzero":
        assert not bool(oa.t.any()) and not bool(o64.t.any())


def test_whiten_streams_refuse_misaligned_operands(dev):
    _, lib, st = env()
    n = 64
    al, mis = _in(dev, torch.ones(n)), _in(dev, torch.ones(n), True)
    sums, s64 = Buf(dev, 2, src=torch.zeros(2)), Buf(dev, 128, src=torch.zeros(128))
    for g, pg, out in ((mis, al, Buf(dev, n)), (al, mis, Buf(dev, n)), (al, al, Buf(dev, n, mis=True))):
        assert lib.s2t_whiten_apply(ptr(g), ptr(pg), n, 0.05, ptr(sums), ptr(out), st) == -1
        assert lib.s2t_whiten_combine(ptr(g), ptr(pg), n, 0.05, ptr(sums), ptr(out), st) == -1
        assert lib.s2t_whiten_combine64(ptr(g), ptr(pg), n, 0.05, ptr(s64), ptr(out), st) == -1
        torch.cuda.synchronize()
        out.untouched("misaligned operand")
    out = Buf(dev, n)
    assert lib.s2t_whiten_combine(ptr(al), ptr(al), n, 0.05, None, ptr(out), st) == -1
    assert lib.s2t_whiten_combine64(ptr(al), ptr(al), n, 0.05, None, ptr(out), st) == -1
    torch.cuda.synchronize()
    out.untouched("NULL sums")
    assert not bool(sums.t.any()) and not bool(s64.t.any())


@pytest.mark.parametrize("name", COVER["lp"])
def test_limit_param_grad_is_bit_exact(dev, name):
    _, lib, st = env()
    c, t = ZA.CASES[name], ZA.make(name)
    x, g, out = _in(dev, t["x"]), _in(dev, t["g"]), Buf(dev, c["n"])
    assert lib.s2t_limit_param_grad(ptr(x), ptr(g), c["lo"], c["hi"], c["n"], ptr(out), st) == 0
    torch.cuda.synchronize()
    out.intact(name)
    ref = ZA.reference(name)["out"].float()
    assert torch.equal(out.t.cpu().view(torch.int32), ref.view(torch.int32)), name      # the sign of a zero too
