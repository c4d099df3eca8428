"""CPU tests of tests/zipconv_f64.py, the float64 yardstick of tests/test_gpu_zip_conv_kernels.py.

The restatements are pinned in float64 at 1e-12 before any kernel is compared with them: the conv
module against oracle.zipformer.chunk_causal_dwconv (gate and mask composed as tests/test_gpu_zip_ops.py
does) and against F.conv1d, the frontend convs against F.conv2d with autograd, col2im against F.fold,
and each against an index-by-index loop on one tiny case; torch.autograd.gradcheck on a small conv-module
case.

The last part measures what float32 costs the REFERENCE on every case of tests/zipconv_cases.py (the
figures recorded in zipconv_cases.FP32_COST are checked to the factor by which they move from host to
host, so the GPU file's bounds cannot drift), checks that the float32 and float64 references agree bit
for bit on the exactly representable inputs, that the launch arithmetic of the weight gradient gives
the path each case names, and that the GPU file runs every case.
"""
import pytest
import torch
import torch.nn.functional as F

import zipconv_cases as ZC
import zipconv_f64 as ZR
from oracle import zipformer as OZ
from yardstick import F64, _grads, _rn, _same

GC = dict(eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------ conv module
@pytest.mark.parametrize("T,B,C,K,chunk", [(23, 2, 5, 7, -1), (23, 2, 5, 7, 4), (24, 3, 4, 7, 8), (20, 2, 3, 15, 15),
                                           (30, 2, 3, 15, 20), (9, 2, 3, 31, 1), (5, 1, 2, 15, -1), (17, 2, 3, 3, 2),
                                           (40, 2, 4, 5, 64)])
def test_conv_module_ref_equals_the_oracle(T, B, C, K, chunk):
    """Gate, padding mask and ChunkCausalDepthwiseConv1d, forward and every gradient; chunk below K
    (sliced scale), equal to it, between K and 2K, not dividing T, above T, and a single chunk."""
    rn = _rn(T * 100 + K + max(chunk, 0))
    Kh = (K + 1) // 2
    u, g = rn(T, B, 2 * C).requires_grad_(True), rn(T, B, C)
    wc, bc, wk, bk, sc = (v.requires_grad_(True) for v in (rn(C, Kh), rn(C), rn(C, K), rn(C), rn(2, C, K) * 0.3))
    lens = torch.tensor([T] + [T // 2 + 1] * (B - 1))
    mask = torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)
    sd = {"p.causal_conv.weight": wc.unsqueeze(1), "p.causal_conv.bias": bc,
          "p.chunkwise_conv.weight": wk.unsqueeze(1), "p.chunkwise_conv.bias": bk, "p.chunkwise_conv_scale": sc}
    x = u[..., :C] * torch.sigmoid(u[..., C:])
    x = x.permute(1, 2, 0).masked_fill(mask.unsqueeze(1), 0.0)
    ref = OZ.chunk_causal_dwconv(sd, "p.", x, chunk, K).permute(2, 0, 1)
    got = ZR.conv_module_ref(u, C, C, mask, T if (chunk < 0 or chunk > T) else chunk, K, wc, bc, wk, bk, sc)
    _same(got, ref)
    leaves = (u, wc, bc, wk, bk, sc)
    for a, r, n in zip(_grads(got, g, *leaves), _grads(ref, g, *leaves), ("u", "wc", "bc", "wk", "bk", "scale")):
        _same(a, r, n)


@pytest.mark.parametrize("T,K,ld,gate_off", [(19, 7, 6, -1), (4, 15, 11, 6), (33, 3, 8, 4)])
def test_conv_module_ref_without_causal_conv_and_scale_is_conv1d(T, K, ld, gate_off):
    """nn.Conv1d(C, C, K, groups=C, padding=K // 2) on the gated input, any row width and gate offset."""
    rn, C = _rn(T + K), 4
    u, wk, bk, g = rn(T, 2, ld).requires_grad_(True), rn(C, K).requires_grad_(True), rn(C).requires_grad_(True), rn(T, 2, C)
    x = u[..., :C] * (torch.sigmoid(u[..., gate_off:gate_off + C]) if gate_off >= 0 else 1.0)
    ref = F.conv1d(x.permute(1, 2, 0), wk.unsqueeze(1), bk, padding=K // 2, groups=C).permute(2, 0, 1)
    got = ZR.conv_module_ref(u, C, gate_off, None, T, K, None, None, wk, bk, None)
    _same(got, ref)
    for a, r in zip(_grads(got, g, u, wk, bk), _grads(ref, g, u, wk, bk)):
        _same(a, r)
    _same(ZR.conv_module_ref(u, C, gate_off, None, T, K, None, None, wk, None, None), ref - bk)


def test_conv_module_ref_index_by_index():
    rn = _rn(5)
    T, B, C, K, chunk = 11, 2, 3, 5, 4
    Kh, halo = 3, 2
    u, wc, bc, wk, bk, sc = rn(T, B, 2 * C), rn(C, Kh), rn(C), rn(C, K), rn(C), rn(2, C, K)
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[1, 8:] = True
    ref = torch.zeros(T, B, C, dtype=F64)

    def xg(t, b, c):
        if t < 0 or t >= T or mask[b, t]:
            return 0.0
        return float(u[t, b, c] * torch.sigmoid(u[t, b, C + c]))

    for t in range(T):
        for b in range(B):
            for c in range(C):
                cs, pos = t // chunk * chunk, t % chunk
                a = float(bk[c])
                for j in range(K):
                    tt = t - halo + j
                    if cs <= tt < cs + chunk:
                        a += float(wk[c, j]) * xg(tt, b, c)
                s = 1.0 + float(sc[0, c, pos]) + float(sc[1, c, K - chunk + pos])      # chunk < K: both edges
                cz = float(bc[c])
                for j in range(Kh):
                    cz += float(wc[c, j]) * xg(t - halo + j, b, c)
                ref[t, b, c] = a * s + cz
    _same(ZR.conv_module_ref(u, C, C, mask, chunk, K, wc, bc, wk, bk, sc), ref)


def test_conv_module_ref_gradcheck():
    rn = _rn(6)
    T, B, C, K = 7, 2, 2, 5
    args = [v.requires_grad_(True) for v in (rn(T, B, 2 * C), rn(C, 3), rn(C), rn(C, K), rn(C), rn(2, C, K))]
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[1, 5:] = True
    assert torch.autograd.gradcheck(lambda u, *p: ZR.conv_module_ref(u, C, C, mask, 3, K, *p), args, **GC)


# ------------------------------------------------------------------ frontend
@pytest.mark.parametrize("K,N,H,W,C", [(7, 2, 5, 9, 3), (7, 1, 1, 1, 2), (3, 2, 4, 6, 5)])
def test_dwconv2d_ref_equals_conv2d_and_its_gradients(K, N, H, W, C):
    rn = _rn(K * 100 + H)
    x, w, b, g, add = rn(N, H, W, C).requires_grad_(True), rn(C, K, K).requires_grad_(True), rn(C).requires_grad_(True), \
        rn(N, H, W, C), rn(N, H, W, C)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w.unsqueeze(1), b, padding=K // 2, groups=C).permute(0, 2, 3, 1)
    got = ZR.dwconv2d_ref(x, w, b)
    _same(got, ref)
    gx, gw, gb = _grads(ref, g, x, w, b)
    for a, r in zip(_grads(got, g, x, w, b), (gx, gw, gb)):
        _same(a, r)
    dw, db = ZR.dwconv2d_wgrad_ref(x.detach(), g, K, K)
    _same(dw, gw)
    _same(db, gb)
    # the flipped taps are the data gradient; the addend is added
    _same(ZR.dwconv2d_ref(g, w.detach(), None, flip=True), gx)
    _same(ZR.dwconv2d_ref(x, w, None, add=add), ref - b + add)


def test_dwconv2d_ref_index_by_index():
    rn = _rn(8)
    N, H, W, C, K = 1, 3, 4, 2, 3
    x, w, b = rn(N, H, W, C), rn(C, K, K), rn(C)
    for flip in (False, True):
        ref = torch.zeros(N, H, W, C, dtype=F64)
        for h in range(H):
            for ww in range(W):
                for c in range(C):
                    a = float(b[c])
                    for i in range(K):
                        for j in range(K):
                            hh, wj = h + i - 1, ww + j - 1
                            if 0 <= hh < H and 0 <= wj < W:
                                a += float(w[c, K - 1 - i, K - 1 - j] if flip else w[c, i, j]) * float(x[0, hh, wj, c])
                    ref[0, h, ww, c] = a
        _same(ZR.dwconv2d_ref(x, w, b, flip), ref)


@pytest.mark.parametrize("B,H,W,pw", [(2, 5, 6, 0), (2, 3, 1, 1), (1, 4, 7, 1)])
def test_conv3x3_c1_ref_equals_conv2d_and_its_gradients(B, H, W, pw):
    rn = _rn(H * 10 + W + pw)
    x, w, b = rn(B, H, W).requires_grad_(True), rn(8, 1, 3, 3).requires_grad_(True), rn(8).requires_grad_(True)
    ref = F.conv2d(x.unsqueeze(1), w, b, padding=(0, pw)).permute(0, 2, 3, 1)
    got = ZR.conv3x3_c1_ref(x, w, b, pw)
    assert got.shape == (B, H - 2, W + 2 * pw - 2, 8)
    _same(got, ref)
    g = rn(*ref.shape)
    for a, r in zip(_grads(got, g, x, w, b), _grads(ref, g, x, w, b)):
        _same(a, r)
    # one output, index by index
    ho, wo, co = H - 3, W + 2 * pw - 3, 5
    x, w, b = x.detach(), w.detach(), b.detach()
    a = float(b[co])
    for kh in range(3):
        for kw in range(3):
            wi = wo + kw - pw
            if 0 <= wi < W:
                a += float(w[co, 0, kh, kw]) * float(x[B - 1, ho + kh, wi])
    assert abs(float(got.detach()[B - 1, ho, wo, co]) - a) < 1e-12


@pytest.mark.parametrize("H,W", [(3, 3), (4, 5), (8, 9), (9, 8)])
def test_conv3x3_s2_ref_equals_conv2d_and_its_gradients(H, W):
    rn = _rn(H * 10 + W)
    x, w, b = rn(2, H, W, 8).requires_grad_(True), rn(32, 8, 3, 3).requires_grad_(True), rn(32).requires_grad_(True)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=2).permute(0, 2, 3, 1)
    got = ZR.conv3x3_s2_ref(x, w, b)
    _same(got, ref)
    g = rn(*ref.shape)
    for a, r in zip(_grads(got, g, x, w, b), _grads(ref, g, x, w, b)):
        _same(a, r)
    ho, wo, co = ref.shape[1] - 1, ref.shape[2] - 1, 17
    x, w, b = x.detach(), w.detach(), b.detach()
    a = float(b[co]) + sum(float(w[co, ci, kh, kw]) * float(x[1, 2 * ho + kh, 2 * wo + kw, ci])
                           for ci in range(8) for kh in range(3) for kw in range(3))
    assert abs(float(got.detach()[1, ho, wo, co]) - a) < 1e-12


@pytest.mark.parametrize("H,W,sh,sw", [(5, 6, 1, 1), (7, 8, 2, 2), (4, 9, 1, 2), (3, 3, 1, 1)])
def test_col2im3x3_ref_equals_fold_and_an_index_loop(H, W, sh, sw):
    rn, B, C = _rn(H + W + sh), 2, 3
    Ho, Wo = (H - 3) // sh + 1, (W - 3) // sw + 1
    dc = rn(B, Ho, Wo, 3, 3, C)
    got = ZR.col2im3x3_ref(dc, H, W, sh, sw)
    cols = dc.permute(0, 5, 3, 4, 1, 2).reshape(B, C * 9, Ho * Wo)
    _same(got, F.fold(cols, (H, W), 3, stride=(sh, sw)).permute(0, 2, 3, 1))
    ref = torch.zeros(B, H, W, C, dtype=F64)
    for ho in range(Ho):
        for wo in range(Wo):
            for kh in range(3):
                for kw in range(3):
                    ref[:, ho * sh + kh, wo * sw + kw] += dc[:, ho, wo, kh, kw]
    _same(got, ref)


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", list(ZC.CASES))
def test_fp32_cost_of_the_reference(name):
    """The yardstick in float32 on the CPU against itself in float64, per output tensor: within 4 x the
    record and the record within 4 x the measurement, both raised to one float32 rounding first (as
    tests/test_zip_f64.py).  On the exact inputs the two agree bit for bit."""
    ref = ZC.reference(name)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    fig = ZC.fp32_figures(name)
    rec = ZC.FP32_COST[name]
    print(f"fp32 cost {name}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    assert set(fig) == set(rec), (sorted(fig), sorted(rec))
    for k in fig:
        f, r = max(fig[k], ZC.UNIT), max(rec[k], ZC.UNIT)
        assert f <= 4 * r and r <= 4 * f, (name, k, fig[k], rec[k])
    if ZC.has_exact(name) and name not in ZC.EXACT_DROPPED:
        e64, e32 = ZC.reference(name, True), ZC.evaluate(name, torch.float32, True)
        for k in e64:
            if k in ZC.EXACT_TENSORS:
                assert e32[k].dtype == torch.float32 and torch.equal(e32[k].double(), e64[k]), (name, k)
                assert float(e64[k].abs().max()) > 0, (name, k)


def test_case_inputs_are_what_the_table_says():
    assert set(ZC.CASES) == set(ZC.FP32_COST)
    assert len({c["seed"] for c in ZC.CASES.values()}) == len(ZC.CASES)
    # the launch arithmetic of the weight gradient gives the path each case names
    for name in ZC.names("wg"):
        c = ZC.CASES[name]
        p = ZC.wgrad_path(c["N"], c["H"], c["W"], c["C"], c["K"])
        assert p["path"] == c["path"], (name, p)
        assert p["gx"] <= (c["H"] + 7) // 8, (name, p)                 # the workspace holds the blocks
    P = lambda n: ZC.wgrad_path(*(ZC.CASES[n][k] for k in ("N", "H", "W", "C", "K")))      # noqa: E731
    assert P("wg_ring_nrr3")["nrr"] == 3 and P("wg_ring_tall")["rrt"] == 40 and P("wg_gen_rows12")["rows_per_blk"] == 12
    assert [P(f"wg_red_n{n}")["nblk"] for n in (16, 17, 48, 49, 65, 113)] == [16, 17, 48, 49, 65, 113]
    assert P("wg_roll_w35")["gx"] == 3 and P("wg_fix_roll_c64")["gx"] == 4
    # the shapes where the unfixed kernels wrote 2 ceil(C / 128) tiles into ceil(C / 64)
    for name in ("wg_fix_c64", "wg_fix_h37_c64", "wg_fix_roll_c64"):
        c, p = ZC.CASES[name], P(name)
        assert 1 <= c["C"] % 128 <= 64
        assert 2 * ((c["C"] + 127) // 128) * p["gx"] > ((c["C"] + 63) // 64) * ((c["H"] + 7) // 8), name
    # conv module
    c = ZC.CASES["op_2gib"]
    assert c["ld"] % 4 == 0 and c["T"] * c["B"] * c["ld"] * 4 >= 0x7FFFFF00 > c["T"] * c["B"] * (c["ld"] - 4) * 4
    for name in ("op_c66_tail", "op_nogate_c6_tail"):
        c = ZC.CASES[name]
        assert c["C"] % 4 and c["mask"] == "none" and c["ld"] == (2 if c["gate"] else 1) * c["C"]
    t = ZC.make("op_allpad")
    assert bool(t["mask"][1].all()) and not bool(t["mask"][0].any())
    r = ZC.reference("op_allpad")
    assert not r["du"][:, 1].any() and bool(r["du"][:, 0].any())
    for name in ZC.names("cm", via="act"):
        y, n = ZC.reference(name)["y"], len(ZC.SAT10)
        # interior frames of a chunk (no edge scale): y on the saturation points to the small input
        assert float((y[7, 0, :n] - torch.tensor(ZC.SAT10, dtype=F64)).abs().max()) < 0.05, name
    c = ZC.CASES["c1_cap"]
    assert c["B"] * (c["H"] - 2) * (c["W"] - 2) == 524416 > ZC.C1_CAP and c["B"] * c["H"] * c["W"] > ZC.C1_CAP
    for name in ("c1_small_pw0", "c1_small_pw1", "c1_h3", "c1_w1_pw1"):
        c = ZC.CASES[name]
        assert c["B"] * (c["H"] - 2) * (c["W"] + 2 * c["pw"] - 2) < 256
    for name in ZC.names("s2"):                    # an even H / W: the last row / column receives no tap
        c, dx = ZC.CASES[name], ZC.reference(name)["dx"]
        if c["H"] % 2 == 0:
            assert not dx[:, -1].any(), name
        if c["W"] % 2 == 0:
            assert not dx[:, :, -1].any(), name


def test_the_gpu_file_runs_every_case():
    import test_gpu_zip_conv_kernels as G
    used = [n for names in G.COVER.values() for n in names]
    assert sorted(used) == sorted(ZC.CASES), set(used) ^ set(ZC.CASES)
    for fn, key in G.RUNS.items():
        marks = [m for m in getattr(G, fn).pytestmark if m.name == "parametrize"]
        assert marks and list(marks[0].args[1]) == G.COVER[key], fn
    assert set(G.RUNS.values()) == set(G.COVER)
