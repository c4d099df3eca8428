"""CPU tests of tests/front_f64.py, the float64 yardstick of tests/test_gpu_front_kernels.py.

The restatements are pinned in float64 at 1e-12 before any kernel is compared with them: the fbank
against oracle.fbank promoted to float64 (its numpy running with float32 replaced by float64, its
constants still rounded through float32 as the kernel holds them), the tables of kernels.FbankTables
against oracle.fbank bit for bit, the augmentations against oracle.augment promoted the same way with
the draws fixed, the smoothed NLL against oracle.heads.masked_kl_div / masked_ce row by row, the
predictor context against nn.Embedding -> depthwise nn.Conv1d; torch.autograd.gradcheck on the
differentiable ones.  Then: every case of tests/front_cases.py reaches the branch it is named for;
every float32 figure of front_cases.FP32_COST is re-measured; and the GPU file calls all ten
extern "C" symbols of the five sources.
"""
import inspect
import os
import random
import re
import types

import numpy as np
import pytest
import torch

import front_cases as FC
import front_f64 as FF
from oracle import augment as OA
from oracle import best_rq as OB
from oracle import fbank as OF
from oracle import heads as OH
from yardstick import F64, TOL, _rn

GC = dict(eps=1e-6, atol=1e-7, rtol=1e-6)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, what=""):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), err_msg=what, **TOL)


class _Up(np.float64):
    """np.float32 for a promoted oracle: a float64 whose scalar constructor still rounds through
    float32 (0.97, eps: the constants stay the float32 ones); as a dtype it is float64."""

    def __new__(cls, x=0.0):
        return np.float64(np.float32(x))


def _promote(monkeypatch, module, constants32=True):
    """Run `module`'s numpy arithmetic in float64: its name `np` sees float32 as _Up, or as plain
    float64 where the module casts computed scalars, not constants (oracle.augment's gains)."""
    shim = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    shim.float32 = _Up if constants32 else np.float64
    monkeypatch.setattr(module, "np", shim)


# ------------------------------------------------------------------ fbank
@pytest.mark.parametrize("M,hf", [(80, 0.0), (23, -400.0), (64, 7600.0), (128, 0.0), (1, 0.0), (65, 0.0)])
def test_fbank_tables_equal_the_oracles_bit_for_bit(M, hf):
    tab = FC.tables(M, hf)
    assert np.array_equal(tab.window.numpy(), OF.povey_window())
    dense = OF.mel_banks(M, high_freq=hf)
    assert dense.shape == (M, 257) and not dense[:, 256].any()
    assert np.array_equal(tab.dense, dense[:, :256])
    # the compact form the kernel reads is the dense one
    off, k0, w = tab.mel_off.tolist(), tab.mel_k0.tolist(), tab.mel_w.numpy()
    back = np.zeros((M, 256), np.float32)
    for m in range(M):
        back[m, k0[m]:k0[m] + off[m + 1] - off[m]] = w[off[m]:off[m + 1]]
    assert np.array_equal(back, tab.dense) and tab.nnz == off[-1] <= 1024
    tw = tab.twiddle.double().numpy()
    ang = 2 * np.pi * np.arange(512) / 512
    assert np.abs(tw[:, 0] - np.cos(ang)).max() < 6e-8 and np.abs(tw[:, 1] + np.sin(ang)).max() < 6e-8


@pytest.mark.parametrize("name", ["fb_ragged", "fb_m23", "fb_m128", "fb_square", "fb_loudsilent_i16", "fb_scale"])
def test_fbank_ref_equals_the_oracle_promoted_to_float64(monkeypatch, name):
    c, t = FC.CASES[name], FC.make(name)
    banks32, win32 = OF.mel_banks(c["M"], high_freq=c["hf"]), OF.povey_window()     # the float32 tables
    _promote(monkeypatch, OF)
    monkeypatch.setattr(OF, "mel_banks", lambda *a, **k: banks32.astype(np.float64))
    monkeypatch.setattr(OF, "povey_window", lambda: win32.astype(np.float64))
    frames = 0
    for b, n in enumerate(t["lens"]):
        x = t["pcm"][b, :n].double() * c["scale"]
        # (the oracle's entry casts its argument to float32: that line alone is promoted by _Up as a dtype)
        ref = OF.fbank(x.numpy(), c["M"], high_freq=c["hf"])
        assert ref.dtype == np.float64 and ref.shape == (FF.fbank_frames(n), c["M"])
        e = FC.reference(name)["energy"][b]
        assert e.dtype == F64 and e.shape == ref.shape
        scale = max(float(e.max()), 1.0) if e.numel() else 1.0
        np.testing.assert_allclose(e.numpy(), np.where(ref > np.log(FF.EPS), np.exp(ref), e.numpy()),
                                   atol=1e-12 * scale, rtol=1e-10)
        np.testing.assert_allclose(np.log(np.maximum(e.numpy(), FF.EPS)), ref, atol=1e-10, rtol=0)
        frames += ref.shape[0]
    assert frames > 0


def test_fbank_frame_count_and_measure():
    for n in (0, 399, 400, 559, 560, 561, 719, 720, 16000):
        assert FF.fbank_frames(n) == OF.num_frames(n) == len(range(0, n - 399, 160))
    e = torch.tensor([[1.0, 4.0], [0.0, 1e-9]], dtype=F64)
    out = torch.log(torch.tensor([[1.0, 4.4], [FF.EPS, FF.EPS * 3]], dtype=F64))
    # frame 0: 0.4 / 4; frame 1: both below the floor -> (3 eps - eps) / eps
    assert abs(FF.fbank_err(out, e) - 2.0) < 1e-12
    assert abs(FF.fbank_err(out[:1], e[:1]) - 0.1) < 1e-12


# ------------------------------------------------------------------ augmentation
def test_row_energy_and_mix_refs_equal_the_oracle_with_the_draws_fixed(monkeypatch):
    rn = _rn(1)
    _promote(monkeypatch, OA, constants32=False)
    # MixFeats: the oracle draws snr, then start
    for T, NT in ((9, 30), (9, 4), (5, 1)):
        src, noise = rn(T, 6) * 2 - 4, rn(NT, 6) * 2 - 5
        random.seed(T * 100 + NT)
        ref = OA.mix_feats(src.numpy(), noise.numpy())
        random.seed(T * 100 + NT)
        snr = random.uniform(10, 20)
        reps = NT if T <= NT else NT * (T // NT + 1)
        start = random.randint(0, reps - T)
        se = FF.row_energy_ref(src.reshape(1, -1), [T], 6, 0)
        ne = FF.row_energy_ref(noise.reshape(1, -1), [NT], 6, 0)
        _same(se[0], np.exp(src.numpy()).sum())
        out = FF.mix_ref(src[None], [T], noise[None], [NT], [start], torch.tensor([snr], dtype=F64), se, ne, 0)
        assert ref.dtype == np.float64
        _same(out[0], ref, f"mix_feats {T} {NT}")
    # AddNoise: PCM (1, n)
    for n, nn_, mg in ((50, 200, 300.0), (50, 7, 300.0), (50, 20, -20.0)):
        pcm, noise = rn(1, n) * 0.4, rn(1, nn_) * 0.2
        random.seed(n + nn_)
        ref = OA.add_noise(pcm.numpy(), noise.numpy(), max_gain_db=mg)
        random.seed(n + nn_)
        snr = random.uniform(10, 50)
        reps = nn_ if n <= nn_ else nn_ * (n // nn_ + 1)
        start = random.randint(0, reps - n)
        se, ne = FF.row_energy_ref(pcm, [n], 1, 1), FF.row_energy_ref(noise, [nn_], 1, 1)
        _same(se[0], (pcm.numpy() ** 2).sum())
        out = FF.mix_ref(pcm.reshape(1, n, 1), [n], noise.reshape(1, nn_, 1), [nn_], [start],
                         torch.tensor([snr], dtype=F64), se, ne, 1, mg)
        _same(out.reshape(1, n), ref, f"add_noise {n} {nn_}")
    # frames past slen and an utterance without noise are the source's
    src, noise = rn(2, 5, 3), rn(2, 4, 3)
    out = FF.mix_ref(src, [3, 5], noise, [4, 0], [1, 0], torch.tensor([10.0, 10.0], dtype=F64),
                     torch.ones(2, dtype=F64), torch.ones(2, dtype=F64), 0)
    assert torch.equal(out[0, 3:], src[0, 3:]) and torch.equal(out[1], src[1]) and not torch.equal(out[0, :3], src[0, :3])


def test_specaug_and_pad_rows_refs_equal_the_oracle_and_the_loop():
    rn = _rn(2)
    feat = rn(20, 9)
    random.seed(5)
    ref = OA.spec_augment(feat.numpy(), 2, 2, 6, 3)
    random.seed(5)
    ts, fs = [], []
    for lst, size, mx in ((ts, 20, 6), (fs, 9, 3)):
        for _ in range(2):
            s = random.randint(0, size - 1)
            lst.append([s, min(size, s + random.randint(1, mx))])
    out = FF.specaug_ref(feat[None], torch.tensor([ts]), torch.tensor([fs]))
    assert np.array_equal(out[0].numpy(), ref)
    packed = rn(3 * 2 + 0 + 4 * 2)
    pad = FF.pad_rows_ref(packed, [0, 6, 6, 14], 2, 5)
    assert pad.shape == (3, 5, 2)
    assert torch.equal(pad[0, :3].reshape(-1), packed[:6]) and not pad[0, 3:].any() and not pad[1].any()
    assert torch.equal(pad[2, :4].reshape(-1), packed[6:]) and not pad[2, 4:].any()


# ------------------------------------------------------------------ smoothed NLL
@pytest.mark.parametrize("kind,eps,scale", [("kl", 0.1, 1.0), ("kl", 0.0, 8.0), ("ce", 0.1, 0.5), ("ce", 0.0, 1.0)])
def test_smoothed_nll_ref_equals_the_oracle_heads_row_by_row(kind, eps, scale):
    rn = _rn(3)
    K, R = 37, 6
    x = (rn(R, K) * 2 + 50.0).requires_grad_(True)
    labels = torch.randint(0, K, (R,), generator=torch.Generator().manual_seed(4))
    cst = FF.nll_consts(K, eps, kind)
    row = FF.smoothed_nll_ref(x, labels, scale, *cst)
    fn = OH.masked_kl_div if kind == "kl" else OH.masked_ce
    for r in range(R):       # the oracle reduces over a mask: one row at a time is that row's loss
        mask = torch.zeros(1, R, dtype=torch.bool)
        mask[0, r] = True
        _same(row[r].detach(), fn(x.detach()[None], labels[None], mask, K, scale, eps).double(), f"row {r}")
    w = rn(R).abs()
    full = sum(w[r] * fn(x[None], labels[None], torch.eye(R, dtype=torch.bool)[r][None], K, scale, eps) for r in range(R))
    g_or, = torch.autograd.grad(full, x)
    _same(FF.smoothed_nll_grad_ref(x.detach(), labels, w, scale, *cst), g_or)
    _same(FF.smoothed_nll_grad_ref(x.detach(), labels, w, scale, *cst, stated=True), g_or)
    v = rn(3, 5).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: FF.smoothed_nll_ref(t, labels[:3] % 5, scale, *FF.nll_consts(5, eps, kind)),
                                    [v], **GC)


def test_smoothed_nll_ref_on_a_label_outside_the_classes_is_the_stated_form():
    x = _rn(5)(2, 9)
    labels = torch.tensor([-1, 9])
    a, b, c0 = FF.nll_consts(9, 0.1, "kl")
    row = FF.smoothed_nll_ref(x, labels, 1.0, a, b, c0)
    _same(row, c0 - a * torch.log_softmax(x, -1).sum(-1))
    g = FF.smoothed_nll_grad_ref(x, labels, torch.ones(2, dtype=F64), 1.0, a, b, c0, stated=True)
    _same(g, torch.softmax(x, -1) - a)


# ------------------------------------------------------------------ BEST-RQ, predictor
@pytest.mark.parametrize("name", FC.names("rq"))
def test_bestrq_cases_have_no_near_tie_but_the_planted_ones(name):
    c, t = FC.CASES[name], FC.make(name)
    labels, gap, dup = FF.bestrq_gap(t["feats"].numpy(), t["proj"].numpy(), t["codebooks"].numpy())
    ref = FC.reference(name)["labels"].numpy()
    assert ref.shape == (c["ncb"], c["B"], t["T2"]) and np.array_equal(labels, ref)
    assert t["T2"] == int(OB.label_lengths(c["T"]))
    if c["plant"] == "zero":
        assert (ref == 1).all() and (gap == 0).all()
        return
    assert ((gap > 1e-9) | ((gap == 0) & dup)).all(), (name, gap.min())
    if c["plant"] in ("lane", "neigh", "ends"):
        tied = (gap[0] == 0) & dup[0]
        assert tied.any(), name
        cb = t["codebooks"][0].numpy()
        lower_wins = 0
        for lab in ref[0][tied]:
            twins = np.nonzero((cb == cb[lab - 1]).all(-1))[0]
            assert len(twins) >= 2 and lab - 1 == twins.min()
            if c["plant"] == "ends":
                assert twins.min() == 0 and twins.max() == c["K"] - 1, (name, twins)
            else:
                assert {"lane": 64, "neigh": 1}[c["plant"]] in np.diff(twins), (name, twins)
            lower_wins += 1
        assert lower_wins
        assert (gap[0][~tied] > 1e-9).all()
    if c["plant"] == "scale":
        assert np.array_equal(ref, FC.reference(c["base"])["labels"].numpy())
        assert not torch.equal(t["codebooks"], FC.make(c["base"])["codebooks"])
    if c["nanpad"]:
        assert bool(torch.isnan(t["feats"][:, 7:]).all()) and c["T"] == 10


def test_predictor_ctx_ref_equals_embedding_then_depthwise_conv():
    rn = _rn(6)
    B, L, K, D, V = 3, 9, 4, 5, 7
    tok = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(7))
    emb = torch.nn.Embedding(V, D).double()
    conv = torch.nn.Conv1d(D, D, K, groups=D, bias=False).double()
    ref = conv(emb(tok).transpose(1, 2)).transpose(1, 2)
    e, w = emb.weight.detach().clone().requires_grad_(True), conv.weight.detach().reshape(D, K).clone().requires_grad_(True)
    out = FF.predictor_ctx_ref(tok, e, w)
    _same(out.detach(), ref.detach())
    g = rn(B, L - K + 1, D)
    (ref * g).sum().backward()
    (out * g).sum().backward()
    _same(e.grad, emb.weight.grad)
    _same(w.grad, conv.weight.grad.reshape(D, K))
    # the clamp the kernel states
    wild = tok.clone()
    wild[0, 0], wild[1, 3] = -1, V
    _same(FF.predictor_ctx_ref(wild, e, w).detach(), FF.predictor_ctx_ref(wild.clamp(0, V - 1), e, w).detach())
    assert torch.autograd.gradcheck(lambda a, b: FF.predictor_ctx_ref(tok, a, b), [e, w], **GC)


# ------------------------------------------------------------------ the cases
def test_case_inputs_reach_the_branches_they_are_named_for():
    assert set(FC.CASES) == set(FC.FP32_COST)
    assert len({c["seed"] for c in FC.CASES.values()}) == len(FC.CASES)
    # fbank
    assert [FF.fbank_frames(n) for n in FC.CASES["fb_ragged"]["lens"]] == [0, 1, 1, 2, 31, 32, 33, 65, 8]
    assert (1597 - 400) % 160
    for name in FC.names("fb"):
        c, t = FC.CASES[name], FC.make(name)
        for b, n in enumerate(t["lens"]):
            assert bool(torch.isfinite(t["pcm"][b, :n]).all()) and bool(torch.isnan(t["pcm"][b, n:]).all())
            assert t["pcm"].shape[1] > max(t["lens"])
    nat = max(FF.fbank_frames(n) for n in FC.CASES["fb_mf_below"]["lens"])
    assert FC.CASES["fb_mf_below"]["mf"] < nat < FC.CASES["fb_mf_above"]["mf"]
    d128 = FC.tables(128, 0.0).dense
    empty = [m for m in range(128) if not d128[m].any()]
    assert empty and all(bool((e[:, empty] == 0).all()) for e in FC.reference("fb_m128")["energy"])
    assert not any((~FC.tables(M, hf).dense.any(1)).any() for M, hf in ((80, 0.0), (65, 0.0), (23, -400.0)))
    assert FC.tables(128, 0.0).nnz <= 1024
    for name in ("fb_zero", "fb_dc"):
        assert all(float(e.max()) < 1e-25 for e in FC.reference(name)["energy"]), name
    on, off = FC.reference("fb_tone_on")["energy"][0], FC.reference("fb_tone_off")["energy"][0]
    assert float(on.max()) > 1.0 and float(off.max()) > 1.0
    for name, amp in (("fb_loudsilent", 1.0), ("fb_loudsilent_i16", 32768.0)):
        e = FC.reference(name)["energy"]
        silent = [(x.max(1).values == 0).tolist() for x in e]
        assert silent[0] == [False] * 3 + [True] * 7               # pair (2,3): silence as frame B
        assert silent[1] == [True] * 3 + [False] * 7               # pair (2,3): silence as frame A
        assert silent[2] == [False] * 3 + [True] * 3 + [False] * 4   # (2,3) B, (4,5) A
        assert float(e[0].max()) > 10.0 * amp * amp
    assert float(FC.reference("fb_loudsilent_i16")["energy"][0].max()) > 1e10
    assert float(FC.make("fb_quiet")["pcm"][0, :400].abs().max()) < 1e-3
    # row energy
    for name in FC.names("re"):
        c = FC.CASES[name]
        assert sorted(n * c["D"] for n in c["lens"]) in ([0, 255, 256, 257, 100003], [0, 80, 240, 320, 100080])
        e = FC.reference(name)["e"]
        assert float(e[0]) == 0.0 and float(e[1:].min()) > 0.2 and float(e.max()) < 5.0
        x = FC.make(name)["x"]
        assert all(bool(torch.isnan(x[b, n * c["D"]:]).all()) for b, n in enumerate(c["lens"]))
    # mix
    for name in FC.names("mx"):
        c, t = FC.CASES[name], FC.make(name)
        for b in range(len(c["slen"])):
            assert bool(torch.isnan(t["noise"][b, c["nlen"][b]:]).all()) and bool(torch.isfinite(t["src"]).all())
            if c["nlen"][b] >= c["slen"][b] and name != "mx1_silent":
                assert c["start"][b] <= c["nlen"][b] - c["slen"][b]
    c = FC.CASES["mx0_wrap"]
    assert 0 in c["nlen"] and 1 in c["nlen"] and 0 in c["slen"] and c["start"][4] == c["nlen"][4] - c["slen"][4]
    assert c["slen"][3] > 4 * c["nlen"][3] and min(c["slen"]) < c["rows"]
    for name in ("mx0_cap", "mx1_cap"):
        c = FC.CASES[name]
        assert c["rows"] * c["D"] == FC.CAP + 257 and c["slen"][0] < c["rows"] and c["start"][0] == c["nlen"][0] - 1
    t, out = FC.make("mx0_floor"), FC.reference("mx0_floor")["out"]
    assert bool((out[0] == np.log(1e-10)).all())                                    # the floor
    assert float(t["se"][1]) == 0.0 and float(t["ne"][1]) > 0.0                      # the gain = 1 branch
    assert float(t["se"][2]) > 0.0 and float(t["ne"][2]) > 0.0
    t, c, out = FC.make("mx1_clip"), FC.CASES["mx1_clip"], FC.reference("mx1_clip")["out"]
    assert bool((out[0] == 1.0).any()) and bool((out[0] == -1.0).any())
    want = [10 * np.log10(float(t["se"][b]) / c["slen"][b]) - 10 * np.log10(float(t["ne"][b]) / c["nlen"][b])
            - float(t["snr"][b]) for b in range(3)]
    assert want[1] > c["max_gain"] + 5 and want[0] < c["max_gain"] - 5 and want[2] < c["max_gain"] - 5
    t, out = FC.make("mx1_silent"), FC.reference("mx1_silent")["out"]
    assert [float(v) == 0.0 for v in t["se"]] == [True, False, True]
    assert [float(v) == 0.0 for v in t["ne"]] == [False, True, True]
    assert torch.equal(out, t["src"].double())
    # specaug, pad_rows
    seen = set()
    for name in FC.names("sa"):
        c, t = FC.CASES[name], FC.make(name)
        seen.add((c["nt"], c["nf"]))
        assert t["tspan"].shape == (c["B"], c["nt"], 2) and t["fspan"].shape == (c["B"], c["nf"], 2)
        ref = FC.reference(name)["out"]
        assert bool(torch.isnan(t["feats"]).any()) == bool(c["nt"] + c["nf"]) and not bool(torch.isnan(ref).any())
        assert bool((ref[t["hit"]] == 0).all()) and torch.equal(ref[~t["hit"]], t["feats"][~t["hit"]])
        for sp, size in ((t["tspan"], c["T"]), (t["fspan"], c["F"])):
            if sp.shape[1] and c["B"] == 3:
                assert sp[0, 0].tolist() == [size - 1, size] and sp[1, 0, 0] == sp[1, 0, 1]
            if sp.shape[1] >= 5:
                assert sp[2, 4].tolist() == [0, size]
            if sp.shape[1]:
                assert len({tuple(sp[b].reshape(-1).tolist()) for b in range(c["B"])}) == c["B"]
    assert {a for a, _ in seen} == {b for _, b in seen} == {0, 1, 2, 5}
    c = FC.CASES["sa_cap"]
    assert FC.CAP < c["T"] * c["F"] < FC.CAP + 512
    for name in FC.names("pr"):
        assert 0 in FC.CASES[name]["rows"]
    assert FC.CASES["pr_cap"]["Lmax"] * FC.CASES["pr_cap"]["D"] > FC.CAP
    # smoothed NLL
    cs = [FC.CASES[n] for n in FC.names("nll")]
    assert {c["K"] for c in cs} >= {2, 255, 256, 257, 1025, 8193} and {c["rows"] for c in cs} == {1, 5}
    assert {(c["kind"], c["eps"]) for c in cs} == {("kl", 0.0), ("kl", 0.1), ("ce", 0.0), ("ce", 0.1)}
    assert {c["scale"] for c in cs} == {0.5, 1.0, 8.0} and {c["off"] for c in cs} == {0.0, 100.0, -100.0, 1000.0, -1000.0}
    for name in ("nll_peak", "nll_peak3_p1000", "nll_peak3_m1000"):
        t = FC.make(name)
        top = t["x"].topk(4, -1)
        n = 1 if name == "nll_peak" else 3
        assert bool((top.values[:, n - 1] - top.values[:, n] > 50).all())
        assert not bool((top.indices[:, :n] == t["labels"][:, None]).any())
        assert abs(float(t["x"].median()) - FC.CASES[name]["off"]) < 0.2
    assert FC.make("nll_w0")["w"].tolist() == [1.0, 0.0, 0.5, 0.0, 2.0]
    assert not FC.reference("nll_w0")["grad"][[1, 3]].any() and bool(FC.reference("nll_w0")["grad"][[0, 2, 4]].any())
    assert FC.make("nll_badlabel")["labels"][[1, 3]].tolist() == [-1, 257]
    # predictor
    cs = {n: FC.CASES[n] for n in FC.names("pc")}
    assert {c["D"] for c in cs.values()} >= {1, 50, 64, 65, 256, 257, 512} and {c["K"] for c in cs.values()} == {1, 2, 8}
    rows = lambda c: c["B"] * (c["L"] - c["K"] + 1)                         # noqa: E731
    assert rows(cs["pc_d50_k2"]) == 8 and cs["pc_d50_k2"]["L"] == cs["pc_d50_k2"]["K"]
    assert rows(cs["pc_d64_k8"]) == 64 and rows(cs["pc_d65_k2"]) == 8 * 257
    assert not FC.make("pc_blank")["tok"].any() and not FC.make("pc_v1")["tok"].any()
    tok = FC.make("pc_clamp")["tok"]
    assert int(tok.min()) == -1 and int(tok.max()) == cs["pc_clamp"]["V"]


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", list(FC.CASES))
def test_fp32_cost_of_the_reference(name):
    """The yardstick in float32 on the CPU against itself in float64 (fbank: oracle.fbank, float32),
    per output tensor; the order of magnitude is checked both ways, as tests/test_zip_f64.py does."""
    fig = FC.fp32_figures(name)
    rec = FC.FP32_COST[name]
    print(f"fp32 cost {name}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    assert set(fig) == set(rec), (sorted(fig), sorted(rec))
    assert (not fig) == (FC.CASES[name]["group"] in FC.EXACT)
    for k in fig:
        f, r = max(fig[k], FC.UNIT), max(rec[k], FC.UNIT)
        assert f <= 4 * r and r <= 4 * f, (name, k, fig[k], rec[k])
        assert FC.bound(name, k) == max(2e-5, 8 * rec[k])


# ------------------------------------------------------------------ census
SOURCES = ("fbank.hip", "augment.hip", "ssl_loss.hip", "bestrq.hip", "predictor.hip")


def test_the_gpu_file_runs_every_case_and_calls_every_entry_point():
    import test_gpu_front_kernels as G
    syms = set()
    for f in SOURCES:
        with open(os.path.join(ROOT, "speech2text_amd", "csrc", f)) as fh:
            syms |= set(re.findall(r'^extern "C" \w+ (s2t_\w+)\(', fh.read(), re.M))
    assert len(syms) == 10, sorted(syms)
    src = inspect.getsource(G)
    for s in syms:
        assert re.search(r"\blib\." + s + r"\(", src), f"{s} is not called by tests/test_gpu_front_kernels.py"
    used = []
    for fn, grp in G.RUNS.items():
        marks = [m for m in getattr(G, fn).pytestmark if m.name == "parametrize"]
        assert marks and list(marks[0].args[1]) == FC.names(grp), fn
        used += FC.names(grp)
    assert sorted(used) == sorted(FC.CASES)
    assert [m.name for m in G.pytestmark] == ["gpu"] if isinstance(G.pytestmark, list) else G.pytestmark.name == "gpu"
