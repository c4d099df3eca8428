"""Plain restatements of the first and last stops of the data path, the yardstick of
tests/test_gpu_front_kernels.py: csrc/fbank.hip (kaldi fbank), csrc/augment.hip (row energy, MixFeats /
AddNoise, SpecAugment, batch padding), csrc/ssl_loss.hip (the smoothed-target NLL of the BEST-RQ
heads), csrc/bestrq.hip (labels) and csrc/predictor.hip (embedding + depthwise context convolution).

Test infrastructure (not a test file).  Every function takes the kernel's own inputs and runs in the
dtype it is given: float64 is the reference, float32 measures what float32 costs the reference
(tests/front_cases.py FP32_COST).  tests/test_front_f64.py pins each one in float64 against the
oracle's form of the same operation before any kernel is compared with it.
"""
import math

import numpy as np
import torch

FRAME, HOP, NFFT = 400, 160, 512
EPS = 1.1920928955078125e-07            # float32 epsilon, the fbank's energy floor
PREEMPH = float(np.float32(0.97))        # the coefficient as the kernel and the oracle hold it (float32)


# ------------------------------------------------------------------ fbank
def fbank_frames(n):
    return 0 if n < FRAME else 1 + (n - FRAME) // HOP


def fbank_energy_ref(pcm, n, tables, scale_in=1.0):
    """Mel energies before the floor and the log, (frames, M) in pcm's dtype, of the first n samples of
    the row `pcm`.  tables: kernels.FbankTables (its float32 window and dense mel matrix are the
    kernel's own inputs, cast up exactly); the transform is a 512-point DFT by its definition, with
    cos / sin of the exactly reduced angle, so nothing of an FFT's structure is shared with the kernel."""
    dt = pcm.dtype
    m = fbank_frames(n)
    M = tables.dense.shape[0]
    if m == 0:
        return torch.zeros((0, M), dtype=dt)
    x = pcm[:n] * scale_in
    fr = x.unfold(0, FRAME, HOP)[:m]
    fr = fr - fr.mean(1, keepdim=True)
    prev = torch.cat((fr[:, :1], fr[:, :-1]), 1)
    fr = (fr - PREEMPH * prev) * tables.window.detach().cpu().to(dt)
    k = torch.arange(NFFT // 2 + 1, dtype=torch.int64)[:, None]
    j = torch.arange(FRAME, dtype=torch.int64)[None, :]
    ang = ((k * j) % NFFT).to(torch.float64) * (2.0 * math.pi / NFFT)
    re, im = fr @ torch.cos(ang).to(dt).t(), fr @ torch.sin(ang).to(dt).t()
    power = re * re + im * im                                           # (m, 257)
    dense = torch.from_numpy(np.asarray(tables.dense)).to(dt)           # (M, 256): bin 256 has no weight
    return power[:, :NFFT // 2] @ dense.t()


def fbank_err(log_out, energy64, eps=EPS):
    """The fbank's error measure, per frame in the energy domain:
    max over frames and bins of |max(exp(out), eps) - max(E, eps)| / max_m max(E[m], eps)."""
    e = energy64.double().clamp(min=eps)
    if e.numel() == 0:
        return 0.0
    got = torch.exp(log_out.double()).clamp(min=eps)
    assert got.shape == e.shape, (got.shape, e.shape)
    return float(((got - e).abs() / e.max(1, keepdim=True).values).max())


# ------------------------------------------------------------------ augmentation
def row_energy_ref(x, lens, D, mode):
    """x (B, stride): out[b] = sum over the first lens[b] * D elements of exp(x) (mode 0) or x^2 (1)."""
    out = []
    for b, n in enumerate(lens):
        v = x[b, :int(n) * D]
        out.append((torch.exp(v) if mode == 0 else v * v).sum())
    return torch.stack(out) if out else x.new_zeros(0)


def mix_gain_ref(se, ne, snr, mode, max_gain_db=0.0, sn=1, nn=1):
    """The gain of one utterance (scalars of the working dtype; sn, nn: element counts of mode 1).
    mode 1 as the kernel states it: a silent source gives gain 0, and a gain_db that is +inf or not a
    number (noise silent; both silent) is held at max_gain_db, as fminf does."""
    if mode == 0:
        if float(se) > 0.0 and float(ne) > 0.0:
            return se * 10.0 ** (-snr / 10.0) / ne
        return torch.ones_like(se)
    with np.errstate(all="ignore"):
        gdb = 10.0 * torch.log10(se / sn) - 10.0 * torch.log10(ne / nn) - snr
    if bool(torch.isnan(gdb)) or float(gdb) > max_gain_db:
        gdb = torch.full_like(gdb, max_gain_db)
    return 10.0 ** (gdb / 20.0)


def mix_ref(src, slen, noise, nlen, start, snr, se, ne, mode, max_gain_db=0.0):
    """src (B, rows, D), noise (B, nrows, D): out[b,t] = mix(src[b,t], noise[b,(start+t) % nlen]) for
    t < slen[b] when nlen[b] > 0; every other frame is src's."""
    out = src.clone()
    B, _, D = src.shape
    for b in range(B):
        L, NL = int(slen[b]), int(nlen[b])
        if L == 0 or NL == 0:
            continue
        g = mix_gain_ref(se[b], ne[b], snr[b], mode, max_gain_db, L * D, NL * D)
        nz = noise[b, (int(start[b]) + torch.arange(L)) % NL]
        a = src[b, :L]
        if mode == 0:
            out[b, :L] = torch.log((torch.exp(a) + g * torch.exp(nz)).clamp(min=1.0e-10))
        else:
            out[b, :L] = (a + nz * g).clamp(-1.0, 1.0)
    return out


def specaug_ref(feats, tspan, fspan):
    """feats (B,T,F); tspan (B,nt,2), fspan (B,nf,2) int (start, end), end exclusive: an index loop."""
    out = feats.clone()
    for b in range(feats.shape[0]):
        for s, e in tspan[b].tolist():
            out[b, max(s, 0):max(e, 0)] = 0
        for s, e in fspan[b].tolist():
            out[b, :, max(s, 0):max(e, 0)] = 0
    return out


def pad_rows_ref(packed, offsets, D, Lmax):
    """packed elements + element offsets [B+1] -> zero-padded (B, Lmax, D)."""
    B = len(offsets) - 1
    out = packed.new_zeros((B, Lmax * D))
    for b in range(B):
        n = offsets[b + 1] - offsets[b]
        out[b, :n] = packed[offsets[b]:offsets[b + 1]]
    return out.view(B, Lmax, D)


# ------------------------------------------------------------------ smoothed NLL
def nll_consts(K, eps, kind):
    """(t_other, t_label, c0) of model/loss/loss.py: "kl" MaskedKLDivergence, "ce" MaskedCELoss."""
    if kind == "ce":
        return eps / K, 1.0 - eps + eps / K, 0.0
    a, b = eps / (K - 1), 1.0 - eps
    return a, b, (K - 1) * (a * math.log(a) if a > 0 else 0.0) + (b * math.log(b) if b > 0 else 0.0)


def smoothed_nll_ref(x, labels, scale, t_other, t_label, c0):
    """row[r] = c0 - sum_c t_c log_softmax(scale x[r])_c, t_c = t_label at the label, t_other elsewhere.
    A label outside [0, K) has no label term at all (every t_c = t_other), as the kernel states."""
    K = x.shape[1]
    lp = torch.log_softmax(x * scale, -1)
    ok = (labels >= 0) & (labels < K)
    lab = lp.gather(1, labels.clamp(0, K - 1)[:, None])[:, 0]
    return c0 - (t_other * lp.sum(-1) + (t_label - t_other) * torch.where(ok, lab, torch.zeros_like(lab)))


def smoothed_nll_grad_ref(x, labels, w, scale, t_other, t_label, c0, stated=False):
    """d sum_r w[r] row[r] / dx by autograd.  stated: the closed form w s (softmax - t) the backward
    kernel states, which is the same thing whenever sum_c t_c = 1 and is what a label outside [0, K)
    gets (t_c = t_other everywhere, which does not sum to one: pinned, not derived)."""
    if stated:
        t = torch.full_like(x, t_other)
        ok = (labels >= 0) & (labels < x.shape[1])
        t[ok, labels[ok]] = t_label
        return w[:, None] * scale * (torch.softmax(x * scale, -1) - t)
    xx = x.detach().clone().requires_grad_(True)
    (smoothed_nll_ref(xx, labels, scale, t_other, t_label, c0) * w).sum().backward()
    return xx.grad


# ------------------------------------------------------------------ BEST-RQ
def bestrq_gap(feats, proj, codebooks):
    """(labels (ncb,B,T2) by first index, gap (ncb,B,T2) = best - second-best cosine similarity (inf at
    K = 1), dup (ncb,B,T2) bool: the second-best codeword is bit for bit the best one), in float64 on
    the float32 inputs, product by product (no BLAS: equal codewords give equal similarities)."""
    from oracle import best_rq as OB
    st = OB.stack_frames(np.asarray(feats, np.float32)).astype(np.float64)
    tg = st @ np.asarray(proj, np.float32).astype(np.float64)
    tg = tg / np.maximum(np.linalg.norm(tg, axis=-1, keepdims=True), 1e-12)
    labs, gaps, dups = [], [], []
    for cb in codebooks:
        c32 = np.asarray(cb, np.float32)
        c = c32.astype(np.float64)
        c = c / np.maximum(np.linalg.norm(c, axis=-1, keepdims=True), 1e-12)
        sim = (tg[:, :, None, :] * c[None, None]).sum(-1)              # (B,T2,K)
        order = np.argsort(-sim, axis=-1, kind="stable")
        best = order[..., 0]
        if c.shape[0] == 1:
            gap, dup = np.full(best.shape, np.inf), np.zeros(best.shape, bool)
        else:
            second = order[..., 1]
            gap = np.take_along_axis(sim, best[..., None], -1)[..., 0] - np.take_along_axis(sim, second[..., None], -1)[..., 0]
            dup = (c32[best] == c32[second]).all(-1)
        labs.append(best + 1), gaps.append(gap), dups.append(dup)
    return np.stack(labs).astype(np.int64), np.stack(gaps), np.stack(dups)


# ------------------------------------------------------------------ predictor context
def predictor_ctx_ref(tok, emb, w):
    """out[b,u,d] = sum_k w[d,k] emb[tok[b,u+k], d], u < L - K + 1; tokens clamped to [0, V-1]."""
    V, D = emb.shape
    K = w.shape[1]
    Lo = tok.shape[1] - K + 1
    t = tok.long().clamp(0, V - 1)
    out = 0
    for k in range(K):
        out = out + emb[t[:, k:k + Lo]] * w[:, k]
    return out
