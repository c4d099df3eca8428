"""CPU tests of tests/zipattn_f64.py, the float64 yardstick of tests/test_gpu_zip_attn_kernels.py.

The restatements are pinned in float64 at 1e-12 before any kernel is compared with them: the attention
weights against oracle.zipformer.attn_weights (identity projections) and its autograd, against index loops
for the relative-to-absolute shift, and torch.autograd.gradcheck on a tiny shape; the value apply against
oracle.zipformer.self_attn; the Whiten pieces against oracle.zipformer.whitening_metric / whiten and their
autograd; limit_param_grad against autograd through oracle.zipformer.limit_param_value.

The last part measures what float32 costs the REFERENCE on every case of tests/zipattn_cases.py (the figures
recorded in zipattn_cases.FP32_COST are checked to a factor 4 both ways, so the GPU file's bounds cannot drift),
checks that each case reaches the kernel, threshold or mask its name says, and that the GPU file runs every case
and calls every extern "C" symbol of the two sources.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import zipattn_cases as ZA
import zipattn_f64 as ZR
from oracle import zipformer as OZ
from yardstick import F64, _rn, _same

GC = dict(eps=1e-6, atol=1e-7, rtol=1e-6)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech2text_amd", "csrc")


def _masks(T, B, am, kp):
    amask = ZA.chunk_mask(T) if am else None
    if am:
        amask[T - 1] = True                                  # a row that masks every key
    kpm = None
    if kp:
        lens = torch.tensor([T, 1, 0][:B] + [T // 2 + 1] * max(0, B - 3))
        kpm = torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)
    return amask, kpm


# ------------------------------------------------------------------ attention
@pytest.mark.parametrize("T,B,H,qd,pd,use_pos,am,kp", [(9, 2, 2, 3, 2, True, True, True), (17, 3, 1, 4, 1, True, False, True),
                                                        (1, 2, 2, 2, 4, True, False, False), (20, 4, 3, 5, 3, False, True, True),
                                                        (33, 1, 2, 8, 4, True, True, False)])
def test_attn_weights_equals_the_oracle_and_its_autograd(T, B, H, qd, pd, use_pos, am, kp):
    """oracle.zipformer.attn_weights with identity in_proj / linear_pos (its own matmul + advanced-index
    shift, masked_fill twice, softmax), forward and both gradients; masks that leave a row without a key."""
    rn = _rn(T * 10 + qd)
    Dp = H * (2 * qd + pd)
    qkp, pos, dW = rn(T, B, Dp), rn(2 * T - 1, H * pd), rn(H, B, T, T)
    amask, kpm = _masks(T, B, am, kp)
    sd = {"p.in_proj.weight": torch.eye(Dp, dtype=F64), "p.in_proj.bias": torch.zeros(Dp, dtype=F64),
          "p.linear_pos.weight": torch.eye(H * pd, dtype=F64)}
    q1, p1 = qkp.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    if use_pos:
        ref = OZ.attn_weights(sd, "p.", q1, p1.unsqueeze(0), H, qd, pd, amask, kpm, OZ.Ctl())
    else:                                                    # the oracle always adds the term: a zero table
        ref = OZ.attn_weights(sd, "p.", q1, torch.zeros_like(pos).unsqueeze(0), H, qd, pd, amask, kpm, OZ.Ctl())
    W, raw = ZR.attn_weights(qkp, pos if use_pos else None, kpm, amask, H, qd, pd)
    _same(W, ref)
    (ref * dW).sum().backward()
    dq, dp = ZR.attn_grads(qkp, pos if use_pos else None, kpm, amask, H, qd, pd, dW)
    _same(dq, q1.grad)
    if use_pos:
        _same(dp, p1.grad)
    else:
        assert dp is None
    if am:
        assert torch.equal(W[:, :, T - 1], torch.full((H, B, T), 1.0 / T, dtype=F64))
        assert not dq[T - 1, :, :H * qd].any() and not dq[T - 1, :, 2 * H * qd:].any()
    assert raw.shape == (H, B, T, T) and float(raw.abs().max()) < 100.0           # before the -1000 fills


def test_attn_raw_scores_index_by_index():
    rn = _rn(3)
    T, B, H, qd, pd = 5, 2, 2, 3, 2
    qkp, pos = rn(T, B, H * (2 * qd + pd)), rn(2 * T - 1, H * pd)
    ref = torch.zeros(H, B, T, T, dtype=F64)
    for h in range(H):
        for b in range(B):
            for i in range(T):
                for j in range(T):
                    a = sum(float(qkp[i, b, h * qd + d]) * float(qkp[j, b, H * qd + h * qd + d]) for d in range(qd))
                    a += sum(float(qkp[i, b, 2 * H * qd + h * pd + d]) * float(pos[(T - 1) - i + j, h * pd + d])
                             for d in range(pd))
                    ref[h, b, i, j] = a
    _same(ZR.raw_scores(qkp, pos, H, qd, pd), ref)
    _same(ZR.raw_scores(qkp, pos, H, qd, pd), ZR.attn_weights(qkp, pos, None, None, H, qd, pd)[1])
    # pd == 0: no p columns, the table is ignored
    q0 = qkp[..., :2 * H * qd].contiguous()
    _same(ZR.raw_scores(q0, pos, H, qd, 0), ZR.raw_scores(q0, None, H, qd, 0))


def test_attn_weights_gradcheck():
    rn = _rn(4)
    T, B, H, qd, pd = 4, 2, 2, 2, 2
    qkp, pos = rn(T, B, H * (2 * qd + pd)).requires_grad_(True), rn(2 * T - 1, H * pd).requires_grad_(True)
    amask, kpm = _masks(T, B, True, True)
    amask[T - 1] = False
    amask[1, 2] = True
    assert torch.autograd.gradcheck(lambda q, p: ZR.attn_weights(q, p, kpm, amask, H, qd, pd)[0], (qkp, pos), **GC)


def test_factored_dw_is_the_sum_of_its_parts():
    rn = _rn(5)
    T, B, H = 6, 2, 3
    pairs = [(rn(T, B, H * 4), rn(T, B, H * 4)), (rn(T, B, H * 5), rn(T, B, H * 5))]
    dW, dW0 = rn(H, B, T, T), rn(B, T, T)
    ref = dW.clone()
    ref[0] += dW0
    for dO, V in pairs:
        for h in range(H):
            dv = dO.shape[-1] // H
            ref[h] += torch.einsum("ibd,jbd->bij", dO[..., h * dv:(h + 1) * dv], V[..., h * dv:(h + 1) * dv])
    _same(ZR.factored_dw(T, B, H, dW, dW0, pairs), ref)
    _same(ZR.factored_dw(T, B, H, dW, None, []), dW)


@pytest.mark.parametrize("T,B,H,dv", [(7, 2, 3, 4), (1, 1, 1, 1), (12, 3, 2, 5)])
def test_attn_apply_equals_the_oracle_and_its_gradient(T, B, H, dv):
    rn = _rn(T + dv)
    C = H * dv
    W, v, g = rn(H, B, T, T).softmax(-1), rn(T, B, C).requires_grad_(True), rn(T, B, C)
    sd = {"p.in_proj.weight": torch.eye(C, dtype=F64), "p.in_proj.bias": torch.zeros(C, dtype=F64),
          "p.out_proj.weight": torch.eye(C, dtype=F64), "p.out_proj.bias": torch.zeros(C, dtype=F64)}
    ref = OZ.self_attn(sd, "p.", v, W, OZ.Ctl())
    _same(ZR.attn_apply(W, v, H, False), ref)
    (ref * g).sum().backward()
    _same(ZR.attn_apply(W, g, H, True), v.grad)
    out = torch.zeros(T, B, C, dtype=F64)
    for h in range(H):
        for b in range(B):
            out[:, b, h * dv:(h + 1) * dv] = W[h, b] @ v.detach()[:, b, h * dv:(h + 1) * dv]
    _same(ZR.attn_apply(W, v, H, False), out)


# ------------------------------------------------------------------ Whiten, limit_param_value
@pytest.mark.parametrize("n,G,cg", [(50, 1, 6), (40, 3, 4), (30, 2, 5)])
def test_whiten_pieces_equal_the_oracle_and_its_autograd(n, G, cg):
    rn = _rn(n + cg)
    C = G * cg
    x = rn(n, C) @ (torch.eye(C, dtype=F64) + 0.3 * rn(C, C)) + 0.3 * rn(C)
    cov, mean, scal = ZR.whiten_from_x(x, G)
    xl = x.clone().requires_grad_(True)
    metric = OZ.whitening_metric(xl, G)
    _same(scal[3], metric)
    cov2, mean2, scal2 = ZR.whiten_stats(x.t() @ x, x.sum(0), n, G, cg)
    _same(cov2, cov)
    _same(mean2, mean)
    np.testing.assert_allclose(scal2.numpy(), scal.numpy(), rtol=1e-12)
    for g in range(G):                                       # one group, element by element
        xc = x[:, g * cg:(g + 1) * cg] - x[:, g * cg:(g + 1) * cg].mean(0)
        _same(cov[g], xc.t() @ xc)
    metric.backward()
    dcov, bias = ZR.whiten_dcov(cov, mean, scal, G, cg)
    _same((x - mean) @ dcov, xl.grad)
    _same(x @ dcov + bias, xl.grad)
    assert torch.equal(dcov, dcov.t())
    same = (torch.arange(C) // cg).unsqueeze(1) == (torch.arange(C) // cg).unsqueeze(0)
    assert not dcov[~same].any()
    # the whole backward of the module, through the oracle's Function
    gr, xo = rn(n, C), x.clone().requires_grad_(True)
    (OZ.whiten(xo, OZ.Ctl(training=True, rand=lambda: 0.0), G, 1.0, 0.05) * gr).sum().backward()
    out, sums = ZR.whiten_apply(gr, xl.grad, 0.05)
    np.testing.assert_allclose(out.numpy(), xo.grad.numpy(), rtol=1e-5, atol=1e-6 * float(out.abs().max()))    # the oracle's penalty gradient is float32
    out64, _ = ZR.whiten_apply(gr, xl.grad, 0.05)
    _same(out64, gr + xl.grad * (0.05 * gr.norm() / (xl.grad.norm() + 1e-20)))
    _same(sums, torch.stack((gr.norm() ** 2, xl.grad.norm() ** 2)))
    z = torch.zeros_like(gr)
    assert torch.equal(ZR.whiten_apply(gr, z, 0.05)[0], gr) and not ZR.whiten_apply(z, gr, 0.05)[0].any()


@pytest.mark.parametrize("lo,hi", [(-0.5, 0.5), (0.5, -0.5)])
def test_limit_param_grad_equals_autograd_through_the_oracle(lo, hi):
    rn = _rn(9)
    x, g = rn(300), rn(300)
    x[:4] = torch.tensor([lo, hi, lo - 1, hi + 1], dtype=F64)
    g[4:8] = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=F64)
    xl = x.clone().requires_grad_(True)
    (OZ.limit_param_value(xl, OZ.Ctl(training=True, rand=lambda: 0.0), lo, hi) * g).sum().backward()
    got = ZR.limit_param_grad(x, g, lo, hi)
    assert torch.equal(got, xl.grad)
    assert torch.equal(got.abs(), g.abs()) and bool((got != g).any())
    if lo < hi:
        assert got[0] == g[0] and got[1] == g[1]             # exactly on a bound: no flip


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", list(ZA.CASES))
def test_fp32_cost_of_the_reference(name):
    """The yardstick in float32 on the CPU against itself in float64, per output tensor: within 4 x the
    record and the record within 4 x the measurement, both raised to one float32 rounding first."""
    ref = ZA.reference(name)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    fig = ZA.fp32_figures(name)
    rec = ZA.FP32_COST[name]
    print(f"fp32 cost {name}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    assert set(fig) == set(rec), (sorted(fig), sorted(rec))
    for k in fig:
        f, r = max(fig[k], ZA.UNIT), max(rec[k], ZA.UNIT)
        assert f <= 4 * r and r <= 4 * f, (name, k, fig[k], rec[k])


def test_case_inputs_are_what_the_table_says():
    assert set(ZA.CASES) == set(ZA.FP32_COST)
    assert len({c["seed"] for c in ZA.CASES.values()}) == len(ZA.CASES)
    P = lambda n, **kw: ZA.fwd_path(*(ZA.CASES[n][k] for k in ("T", "H", "qd", "pd")), **kw)      # noqa: E731
    inst = {1: (2, 1), 31: (2, 1), 32: (2, 1), 33: (2, 1), 64: (2, 1), 65: (4, 1), 128: (4, 1), 129: (8, 1), 256: (8, 1),
            257: (8, 2), 511: (8, 2), 512: (8, 2)}
    for T, i in inst.items():
        assert P(f"fw_t{T}") == ("mfma",) + i
    for n in ZA.names("fw") + ZA.names("fl"):
        c = ZA.CASES[n]
        want = "gen" if (n.startswith("fw_g_") or n.endswith("_gen") or n.endswith("_gen513")) else "mfma"
        assert P(n, aligned="qkp" not in c["mis"])[0] == want, n
    for n in ZA.names("fl"):
        assert P(n)[0] == "mfma", n
    assert P("fw_g_qkpmis")[0] == "mfma" and P("fw_g_qkpmis", aligned=False)[0] == "gen"
    c = ZA.CASES["fw_g_dp19"]
    assert c["H"] * (2 * c["qd"] + c["pd"]) == 19 and c["qd"] % 8 == 0 and c["pd"] <= 4
    c = ZA.CASES["fw_pd3"]
    assert c["H"] * (2 * c["qd"] + c["pd"]) == 76
    assert [P(f"fw_g_t{T}")[1:] for T in (128, 129, 256, 257, 513, 1025)] == [(2, 1), (4, 1), (4, 1), (8, 1), (8, 2), (8, 3)]
    assert 513 % 512 == 1 and 1025 % 512 == 1                # a last tile of one key
    assert P("fw_v0_t65")[1:] == (4, 1) and P("fw_v0_t257")[1:] == (8, 2)         # KT = 4 (byte reads) | 16 (bits)
    # masks
    for n in [m for m in ZA.CASES if ZA.CASES[m].get("am") == "special"]:
        c, t = ZA.CASES[n], ZA.make(n)
        rows, utts = ZA.masked_rows(c)
        assert len(rows) == 2 and utts == [1]
        assert bool(t["amask"][rows].all()) and bool(t["kpm"][1].all()) and int((~t["kpm"][2]).sum()) == 1
        assert bool((t["kpm"][2] & t["amask"][0]).any())     # a key both padded and masked
        W = ZA.reference(n)["W"] if "W" in ZA.reference(n) else ZA.reference(n)["_W"]
        assert torch.equal(W[:, :, rows], torch.full_like(W[:, :, rows], 1.0 / c["T"]))
        assert torch.equal(W[:, 1], torch.full_like(W[:, 1], 1.0 / c["T"]))
    for n in ("fw_big30_mfma", "fw_big30_gen"):
        raw = ZA.reference(n)["_raw"]
        assert abs(float(raw.abs().max()) - 30.0) < 1e-3 and float(raw.min()) < -20 and float(raw.max()) > 20
        assert bool(ZA.make(n)["kpm"].any()) and bool(ZA.make(n)["amask"].any())
    for n in ("fw_pd0_mfma", "fw_pd0_gen"):
        assert ZA.CASES[n]["pd"] == 0 and ZA.make(n)["pos"] is None
    # the penalty flag: the largest raw score is 5 % away from the limit or more, and sits where the name says
    L = ZA.LIMIT
    want = dict(fl_under=False, fl_over=True, fl_masked=True, fl_partner=True, fl_ragged=True, fl_clamped=False)
    for n, w in want.items():
        c, t, raw = ZA.CASES[n], ZA.make(n), ZA.reference(n)["_raw"].abs()
        assert ZA.flag_expected(n) == w, n
        assert abs(float(raw.max()) / L - 1.0) > 0.05, (n, float(raw.max()))
        over = raw > L
        if n == "fl_masked":
            assert bool(t["amask"].expand_as(over)[over].all()) and float(raw[~t["amask"].expand_as(raw)].max()) < 0.97 * L
        if n == "fl_partner":
            idx = over.nonzero()
            assert c["T"] == 300 and bool((idx[:, 3] == ZA.PARTNER_KEY).all()) and ZA.PARTNER_KEY >= 256
        if n == "fl_ragged":
            idx = over.nonzero()
            assert bool((idx[:, 2] == c["T"] - 1).all()) and c["T"] % 32 == 6
        if n == "fl_clamped":
            T, qd = c["T"], c["qd"]
            qk = float(t["qkp"][T - 1, 0, :qd].double() @ t["qkp"][ZA.CLAMP_KEY, 0, qd:2 * qd].double())
            assert qk > 1.15 * L and float(raw.max()) < 0.95 * L and T % 32 != 0
    # backward
    cds = {n: sum(ZA.CASES[n]["dvs"]) for n in ZA.names("bw")}
    assert [ZA.bwd_ns(cds[f"bw_cd{k}"]) for k in (0, 4, 12, 13, 24, 25, 32)] == [0, 6, 6, 12, 12, 16, 16]
    assert [cds[f"bw_cd{k}"] for k in (0, 4, 12, 13, 24, 25, 32)] == [0, 4, 12, 13, 24, 25, 32]
    assert ZA.CASES["bw_cd0"]["dw"] and not ZA.CASES["bw_cd0"]["given"]
    assert ZA.CASES["bw_cd12"]["dw"] and ZA.CASES["bw_cd12"]["dw0"] and any(d % 2 for d in ZA.CASES["bw_cd13"]["dvs"])
    assert [ZA.CASES[f"bw_bh{k}"]["B"] * ZA.CASES[f"bw_bh{k}"]["H"] for k in (1, 7, 8, 9, 17)] == [1, 7, 8, 9, 17]
    for T in (511, 512, 513):
        assert ZA.make(f"bw_t{T}")["amask"] is not None      # AM_MAXT decides only under a mask
    r = ZA.reference("bw_m_rows")
    rows, _ = ZA.masked_rows(ZA.CASES["bw_m_rows"])
    c = ZA.CASES["bw_m_rows"]
    for sl in (slice(0, c["H"] * c["qd"]), slice(2 * c["H"] * c["qd"], None)):
        assert not r["dqkp"][rows][..., sl].any() and not r["dqkp"][:, 1, sl].any() and bool(r["dqkp"][:, 0, sl].any())
    assert "dpos" not in ZA.reference("bw_nopos_pd4") and "dpos" not in ZA.reference("bw_pd0")
    assert ZA.CASES["bw_pd0"]["pd"] == 0 and ZA.CASES["bw_pd0"]["pos"]
    # apply
    for n in ZA.names("ap"):
        c = ZA.CASES[n]
        wide = c["T"] >= 4 and c["dv"] % 4 == 0 and c["mis"] is None
        assert wide == (re.fullmatch(r"ap_dv(4|8|12|16)_t\d+", n) is not None), n
    assert set(ZA.PERM_CASES) <= set(ZA.names("ap"))
    # Whiten
    for n in ZA.names("wm") + ZA.names("wx"):
        k = ZA.kappa(n)
        assert (24.0 < k < 28.0) if n.endswith("off5") else (k <= 1.0 + 9.0), (n, k)
    for G, cg in ((4, 48), (2, 96), (3, 100)):               # a 64 x 64 tile holds channels of two groups
        assert any((64 * a) // cg != (64 * a + 63) // cg for a in range(G * cg // 64))
        need = ZA.xtx_needed(G, cg)
        assert not bool(need.all()) and not bool(torch.tril(need, -64).any())
    assert bool(ZA.xtx_needed(1, 192)[0, 191]) and not bool(ZA.xtx_needed(1, 192)[191, 0])
    assert ZA.CASES["wa_cap"]["n"] == 4 * 2048 * 256 + 5
    assert not ZA.make("wa_pgzero")["pg"].any() and not ZA.make("wa_gzero")["g"].any()
    for n in ZA.names("lp"):
        c, t = ZA.CASES[n], ZA.make(n)
        r = ZA.reference(n)["out"]
        assert torch.equal(r.abs(), t["g"].double().abs())
        if c["n"] >= 20 and c["lo"] < c["hi"]:
            assert bool((r[:8] == t["g"][:8].double()).all()) and bool((r[8:20] != t["g"][8:20].double()).any())
    t = ZA.make("lp_swapped")
    inside = (t["x"] < 0.5) & (t["x"] > -0.5)
    # lo > hi: inside (hi, lo) a positive g is flipped twice and comes back, a negative one once
    assert bool((inside & (t["g"] > 0)).any()) and bool((inside & (t["g"] < 0)).any())
    assert torch.equal(ZA.reference("lp_swapped")["out"][inside], t["g"].double().abs()[inside])


def _symbols(fname):
    with open(os.path.join(CSRC, fname)) as f:
        return set(re.findall(r'^extern "C" \w+ (s2t_\w+)\(', f.read(), re.M))


def test_the_gpu_file_runs_every_case_and_every_entry_point():
    import test_gpu_zip_attn_kernels as G
    used = [n for names in G.COVER.values() for n in names]
    assert sorted(used) == sorted(ZA.CASES), set(used) ^ set(ZA.CASES)
    called = set()
    for fn, (key, syms) in G.RUNS.items():
        test = getattr(G, fn)
        if key is not None:
            marks = [m for m in test.pytestmark if m.name == "parametrize"]
            assert marks and list(marks[0].args[1]) == G.COVER[key], fn
        src = "".join(inspect.getsource(getattr(G, h)) for h in (fn,) + G.HELPERS.get(fn, ()))
        for s in syms:
            assert re.search(r"lib\." + s + r"\(", src), (fn, s)
        called |= set(syms)
    assert {k for k, _ in G.RUNS.values() if k is not None} == set(G.COVER)
    want = _symbols("zip_attn.hip") | _symbols("whiten.hip")
    assert len(want) == 12, sorted(want)
    assert want <= called, sorted(want - called)
