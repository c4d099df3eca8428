"""GPU: the first and last stops of the data path, called through the C ABI on device buffers of the
test's own, against the float64 yardstick tests/front_f64.py at every dispatch edge
(tests/front_cases.py names why each shape is there): csrc/fbank.hip (s2t_fbank_f32), csrc/augment.hip
(s2t_row_energy, s2t_mix, s2t_specaug, s2t_pad_rows), csrc/ssl_loss.hip (s2t_smoothed_nll_fwd / _bwd),
csrc/bestrq.hip (s2t_bestrq_labels), csrc/predictor.hip (s2t_predictor_ctx_fwd / _bwd).

Error = max |got - ref| / max |ref| per tensor; allowed = front_cases.bound(case, tensor) =
max(2e-5, 8 x the case's float32 figure of the YARDSTICK, asserted by tests/test_front_f64.py).  The
fbank is measured per frame in the energy domain (front_f64.fbank_err).  Frame counts, labels,
SpecAugment, pad_rows and every copied-through frame are compared exactly.  Every buffer a kernel
writes is a guarded buffer of tests/guarded.py, full of NaN (int64 outputs: of ISENT) with a guard of the
same behind it, which must be intact afterwards; inputs carry
NaN wherever a kernel must not read; accumulators are pre-filled and must hold pre-fill + reference;
a call the entry point must refuse returns -1 and leaves its outputs untouched.
"""
import functools
import math

import numpy as np
import pytest
import torch

import front_cases as FC
import front_f64 as FF
from guarded import ISENT, Buf, env, hold

pytestmark = pytest.mark.gpu

LOG_EPS = float(np.float32(math.log(FF.EPS)))
LOG_EPS_ULP = 2.0 ** -20                    # one float32 ulp at 15.94
IBuf = functools.partial(Buf, fill=ISENT, dtype=torch.int64)      # labels, frame counts
_hold = functools.partial(hold, FC)
RUNS = dict(test_fbank_vs_float64="fb", test_row_energy_vs_float64="re", test_mix_vs_float64="mx",
            test_specaug_exact="sa", test_pad_rows_exact="pr", test_smoothed_nll_vs_float64="nll",
            test_bestrq_labels_exact="rq", test_predictor_context_vs_float64="pc")


# ------------------------------------------------------------------ fbank
def _fbank_call(dev, tab, pcm, lens, M, scale, mf, mean=None, istd=None):
    N, lib, st = env()
    B = pcm.shape[0]
    out, frames = Buf(dev, (B, mf, M)), IBuf(dev, B)
    N.check(lib.s2t_fbank_f32(N.fp(pcm), pcm.stride(0), N.lp(lens), B, N.fp(tab.window), N.fp(tab.twiddle),
                              N.ip(tab.mel_off), N.ip(tab.mel_k0), N.fp(tab.mel_w), tab.nnz, M, FF.EPS,
                              float(scale), N.fp(mean), N.fp(istd), N.fp(out.t), mf, N.lp(frames.t), st),
            "s2t_fbank_f32")
    torch.cuda.synchronize()
    out.intact("fbank out"), frames.intact("fbank frames")
    return out.t, frames.t


@pytest.mark.parametrize("name", FC.names("fb"))
def test_fbank_vs_float64(dev, name):
    """Frame counts exactly; every valid frame within the bound under the per-frame energy measure;
    a frame or a filter without energy exactly log(eps); rows past an utterance's frames exactly 0;
    the CMVN epilogue equal to (plain - mean) * istd of the plain output of the same call; scale_in
    equal to prescaling."""
    from speech2text_amd.kernels import FbankTables
    c, t = FC.CASES[name], FC.make(name)
    M, lens = c["M"], t["lens"]
    tab = FbankTables(M, high_freq=c["hf"], device=dev)
    pcm, nsamp = t["pcm"].to(dev), torch.tensor(lens, device=dev)
    nat = [FF.fbank_frames(n) for n in lens]
    mf = c["mf"] or max(nat)
    out, frames = _fbank_call(dev, tab, pcm, nsamp, M, c["scale"], mf)
    assert frames.tolist() == nat
    ref, tol, worst, leak = FC.reference(name)["energy"], FC.bound(name, "feat"), 0.0, 0.0
    cpu = out.cpu()
    empty = torch.from_numpy(~tab.dense.any(1))
    for b, nf in enumerate(nat):
        k = min(nf, mf)
        assert bool(torch.isfinite(cpu[b]).all()), (name, b)
        assert not bool(cpu[b, k:].any()), f"{name}: rows past the {k} frames of utterance {b} are not zero"
        worst = max(worst, FF.fbank_err(cpu[b, :k], ref[b][:k]))
        dark = (ref[b][:k] == 0)
        dark[:, empty] = True
        if bool(dark.any()):
            leak = max(leak, float(torch.exp(cpu[b, :k][dark].double()).max()))
    print(f"{name} feat: err {worst:.3e} bound {tol:.3e} ratio {worst / tol:.3f}; "
          f"largest energy where the reference has none: {leak:.3e} (eps {FF.EPS:.3e})")
    assert worst <= tol, f"{name}: err {worst:.3e} > bound {tol:.3e}"
    floor = set()
    for b, nf in enumerate(nat):
        k = min(nf, mf)
        dark = (ref[b][:k] == 0)
        dark[:, empty] = True
        floor |= set(cpu[b, :k][dark].tolist())
    # one value, the device's logf(eps) (within an ulp of the correctly rounded one)
    assert len(floor) <= 1 and all(abs(v - LOG_EPS) <= LOG_EPS_ULP for v in floor), \
        f"{name}: no energy must give log(eps) = {LOG_EPS}: {sorted(floor)}"
    if c["cmvn"]:
        mean, istd = t["mean"].to(dev), t["istd"].to(dev)
        normed, frames2 = _fbank_call(dev, tab, pcm, nsamp, M, c["scale"], mf, mean, istd)
        assert frames2.tolist() == nat
        assert torch.equal(normed, (out - mean) * istd)
    if c["scale"] != 1.0:
        pre = torch.where(torch.isnan(pcm), pcm, pcm * c["scale"])
        assert bool(((pre / c["scale"] == pcm) | torch.isnan(pcm)).all())           # (the scaling is exact)
        out1, _ = _fbank_call(dev, tab, pre, nsamp, M, 1.0, mf)
        assert torch.equal(out1, out)


def test_fbank_refuses_129_bins_and_1025_filter_weights(dev):
    from speech2text_amd.kernels import FbankTables
    N, lib, st = env()
    tab = FbankTables(80, device=dev)
    pcm, nsamp = torch.zeros(1, 800, device=dev), torch.tensor([800], device=dev)
    w = torch.zeros(1025, device=dev)
    for M, nnz in ((129, tab.nnz), (80, 1025), (0, tab.nnz)):
        out, frames = Buf(dev, (1, 3, 129)), IBuf(dev, 1)
        assert lib.s2t_fbank_f32(N.fp(pcm), 800, N.lp(nsamp), 1, N.fp(tab.window), N.fp(tab.twiddle),
                                 N.ip(tab.mel_off), N.ip(tab.mel_k0), N.fp(w), nnz, M, FF.EPS, 1.0, None, None,
                                 N.fp(out.t), 3, N.lp(frames.t), st) == -1
        torch.cuda.synchronize()
        out.untouched(f"s2t_fbank_f32 at M = {M}, nnz = {nnz}"), frames.untouched("frames")


# ------------------------------------------------------------------ augmentation
@pytest.mark.parametrize("name", FC.names("re"))
def test_row_energy_vs_float64(dev, name):
    N, lib, st = env()
    c, t = FC.CASES[name], FC.make(name)
    x, lens = t["x"].to(dev), torch.tensor(t["lens"], device=dev)
    out = Buf(dev, len(t["lens"]))
    N.check(lib.s2t_row_energy(N.fp(x), x.stride(0), N.lp(lens), len(t["lens"]), c["D"], c["mode"], N.fp(out.t), st),
            "s2t_row_energy")
    torch.cuda.synchronize()
    out.intact(name)
    assert float(out.t[0]) == 0.0
    _hold(name, dict(e=out.t))


@pytest.mark.parametrize("name", FC.names("mx"))
def test_mix_vs_float64(dev, name):
    """Rows of stride rows_max D + 5 (NaN in the pad of the source, which the output's pad must keep);
    noise rows past nlen are NaN; frames past slen, and utterances without noise, bit for bit."""
    N, lib, st = env()
    c, t = FC.CASES[name], FC.make(name)
    B, R, D, ss = len(c["slen"]), c["rows"], c["D"], t["sstride"]
    src = Buf(dev, (B, ss))
    src.t[:, :R * D] = t["src"].reshape(B, -1).to(dev)
    out = Buf(dev, (B, ss))
    noise = t["noise"].reshape(B, -1).to(dev)
    slen, nlen, start, snr, se, ne = (t[k].to(dev) for k in ("slen", "nlen", "start", "snr", "se", "ne"))
    N.check(lib.s2t_mix(N.fp(src.t), ss, N.lp(slen), N.fp(noise), noise.stride(0), N.lp(nlen), N.lp(start), N.fp(snr),
                        N.fp(se), N.fp(ne), B, R, D, c["mode"], c["max_gain"], N.fp(out.t), st), "s2t_mix")
    torch.cuda.synchronize()
    out.intact(name), src.intact(name)
    assert bool(torch.isnan(out.t[:, R * D:]).all()), f"{name}: the pad behind a row was written"
    got = out.t[:, :R * D].reshape(B, R, D).cpu()
    for b in range(B):
        keep = 0 if c["nlen"][b] == 0 else c["slen"][b]
        assert torch.equal(got[b, keep:], t["src"][b, keep:]), f"{name}: utterance {b}: frames past slen"
    if c["kind"] == "silent":
        assert torch.equal(got, t["src"])
    _hold(name, dict(out=got))


@pytest.mark.parametrize("name", FC.names("sa"))
def test_specaug_exact(dev, name):
    N, lib, st = env()
    c, t = FC.CASES[name], FC.make(name)
    feats = Buf(dev, (c["B"], c["T"], c["F"]), t["feats"])
    tspan = t["tspan"].to(dev) if c["nt"] else None
    fspan = t["fspan"].to(dev) if c["nf"] else None
    N.check(lib.s2t_specaug(N.fp(feats.t), c["B"], c["T"], c["F"], N.ip(tspan), c["nt"], N.ip(fspan), c["nf"], st),
            "s2t_specaug")
    torch.cuda.synchronize()
    feats.intact(name)
    assert torch.equal(feats.t.cpu(), FC.reference(name)["out"])          # (no NaN is left: all sat in spans)


@pytest.mark.parametrize("name", FC.names("pr"))
def test_pad_rows_exact(dev, name):
    N, lib, st = env()
    c, t = FC.CASES[name], FC.make(name)
    B = len(c["rows"])
    packed, offs = t["packed"].to(dev), torch.tensor(t["offsets"], device=dev)
    out = Buf(dev, (B, c["Lmax"], c["D"]))
    N.check(lib.s2t_pad_rows(N.fp(packed), N.lp(offs), B, c["Lmax"], c["D"], N.fp(out.t), st), "s2t_pad_rows")
    torch.cuda.synchronize()
    out.intact(name)
    assert torch.equal(out.t.cpu(), FC.reference(name)["out"])


def test_augment_entries_refuse_bad_settings(dev):
    N, lib, st = env()
    x, n = torch.zeros(1, 8, device=dev), torch.tensor([8], device=dev)
    f, z = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    out = Buf(dev, 8)
    assert lib.s2t_row_energy(N.fp(x), 8, N.lp(n), 1, 1, 2, N.fp(out.t), st) == -1
    assert lib.s2t_row_energy(N.fp(x), 8, N.lp(n), 1, 0, 0, N.fp(out.t), st) == -1
    assert lib.s2t_mix(N.fp(x), 8, N.lp(n), N.fp(x), 8, N.lp(n), N.lp(z), N.fp(f), N.fp(f), N.fp(f), 1, 8, 1, 2, 0.0,
                       N.fp(out.t), st) == -1
    assert lib.s2t_pad_rows(N.fp(x), N.lp(torch.tensor([0, 8], device=dev)), 1, 8, 0, N.fp(out.t), st) == -1
    assert lib.s2t_specaug(N.fp(out.t), 1, 8, 1, None, -1, None, 0, st) == -1
    torch.cuda.synchronize()
    out.untouched("augment.hip")


# ------------------------------------------------------------------ smoothed NLL
@pytest.mark.parametrize("name", FC.names("nll"))
def test_smoothed_nll_vs_float64(dev, name):
    """Row losses and the gradient (through the saved row statistics of the forward)."""
    N, lib, st = env()
    c, t = FC.CASES[name], FC.make(name)
    R, K = c["rows"], c["K"]
    a, b, c0 = FF.nll_consts(K, c["eps"], c["kind"])
    x, labels, w = t["x"].to(dev), t["labels"].to(dev), t["w"].to(dev)
    row, stats, grad = Buf(dev, R), Buf(dev, (R, N.const("S2T_NLL_STATS"))), Buf(dev, (R, K))
    N.check(lib.s2t_smoothed_nll_fwd(N.fp(x), N.lp(labels), R, K, c["scale"], a, b, c0, N.fp(row.t), N.fp(stats.t), st),
            "s2t_smoothed_nll_fwd")
    N.check(lib.s2t_smoothed_nll_bwd(N.fp(x), N.lp(labels), N.fp(stats.t), N.fp(w), R, K, c["scale"], a, b,
                                     N.fp(grad.t), st), "s2t_smoothed_nll_bwd")
    torch.cuda.synchronize()
    row.intact(name), stats.intact(name), grad.intact(name)
    assert bool(torch.isfinite(stats.t).all())
    for r in (t["w"] == 0).nonzero().reshape(-1).tolist():
        assert not bool(grad.t[r].any()), f"{name}: row {r} has weight 0"
    _hold(name, dict(row=row.t, grad=grad.t))


# ------------------------------------------------------------------ BEST-RQ
@pytest.mark.parametrize("name", FC.names("rq"))
def test_bestrq_labels_exact(dev, name):
    N, lib, st = env()
    c, t = FC.CASES[name], FC.make(name)
    feats, proj, cb = (t[k].to(dev) for k in ("feats", "proj", "codebooks"))
    labels = IBuf(dev, (c["ncb"], c["B"], t["T2"]))
    N.check(lib.s2t_bestrq_labels(N.fp(feats), c["B"], c["T"], c["F"], N.fp(proj), c["D"], N.fp(cb), c["ncb"], c["K"],
                                  t["T2"], N.lp(labels.t), st), "s2t_bestrq_labels")
    torch.cuda.synchronize()
    labels.intact(name)
    assert torch.equal(labels.t.cpu(), FC.reference(name)["labels"]), name


def test_bestrq_refuses_a_bad_width_and_too_many_labels(dev):
    N, lib, st = env()
    feats, proj, cb = torch.zeros(1, 11, 4, device=dev), torch.zeros(36, 128, device=dev), torch.zeros(1, 4, 128, device=dev)
    for D, T, T2 in ((3, 11, 2), (48, 11, 2), (128, 11, 2), (16, 11, 3), (16, 10, 2), (16, 6, 1)):
        labels = IBuf(dev, (1, 1, 3))
        assert lib.s2t_bestrq_labels(N.fp(feats), 1, T, 4, N.fp(proj), D, N.fp(cb), 1, 4, T2, N.lp(labels.t), st) == -1
        torch.cuda.synchronize()
        labels.untouched(f"s2t_bestrq_labels at D = {D}, T = {T}, T2 = {T2}")


# ------------------------------------------------------------------ predictor context
def _pc_call(dev, name, want_emb=True, want_w=True):
    N, lib, st = env()
    c, t = FC.CASES[name], FC.make(name)
    B, L, K, D, V = (c[k] for k in ("B", "L", "K", "D", "V"))
    Lo = L - K + 1
    tok, emb, w, g = (t[k].to(dev) for k in ("tok", "emb", "w", "g"))
    out, de, dw = Buf(dev, (B, Lo, D)), Buf(dev, (V, D), t["de0"]), Buf(dev, (D, K), t["dw0"])
    N.check(lib.s2t_predictor_ctx_fwd(N.ip(tok), N.fp(emb), N.fp(w), B, L, K, D, V, N.fp(out.t), st),
            "s2t_predictor_ctx_fwd")
    N.check(lib.s2t_predictor_ctx_bwd(N.ip(tok), N.fp(emb), N.fp(w), N.fp(g), B, L, K, D, V,
                                      N.fp(de.t) if want_emb else None, N.fp(dw.t) if want_w else None, st),
            "s2t_predictor_ctx_bwd")
    torch.cuda.synchronize()
    out.intact(name), de.intact(name), dw.intact(name)
    return t, out.t, de.t, dw.t


@pytest.mark.parametrize("name", FC.names("pc"))
def test_predictor_context_vs_float64(dev, name):
    """Forward, and both gradients accumulated into pre-filled buffers."""
    _, out, de, dw = _pc_call(dev, name)
    _hold(name, dict(out=out, d_emb=de, d_w=dw))


@pytest.mark.parametrize("name", ["pc_d64_k8", "pc_d65_k2"])
def test_predictor_context_backward_with_one_gradient_absent(dev, name):
    ref = FC.reference(name)
    t, _, de, dw = _pc_call(dev, name, want_emb=False)
    assert torch.equal(de.cpu(), t["de0"]) and FC.rel_err(dw, ref["d_w"]) <= FC.bound(name, "d_w")
    t, _, de, dw = _pc_call(dev, name, want_w=False)
    assert torch.equal(dw.cpu(), t["dw0"]) and FC.rel_err(de, ref["d_emb"]) <= FC.bound(name, "d_emb")


def test_predictor_context_refuses_nine_taps_and_a_row_shorter_than_the_taps(dev):
    N, lib, st = env()
    tok, emb, g = torch.zeros(2, 12, dtype=torch.int32, device=dev), torch.zeros(5, 8, device=dev), torch.zeros(2, 12, 8, device=dev)
    w = torch.zeros(8, 9, device=dev)
    for K, L, V in ((9, 12, 5), (4, 3, 5), (0, 12, 5), (2, 12, 0)):
        out, de, dw = Buf(dev, (2, 12, 8)), Buf(dev, (5, 8)), Buf(dev, (8, 9))
        assert lib.s2t_predictor_ctx_fwd(N.ip(tok), N.fp(emb), N.fp(w), 2, L, K, 8, V, N.fp(out.t), st) == -1
        assert lib.s2t_predictor_ctx_bwd(N.ip(tok), N.fp(emb), N.fp(w), N.fp(g), 2, L, K, 8, V, N.fp(de.t), N.fp(dw.t),
                                         st) == -1
        torch.cuda.synchronize()
        for b in (out, de, dw):
            b.untouched(f"s2t_predictor_ctx at K = {K}, L = {L}, V = {V}")
