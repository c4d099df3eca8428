"""Seeded cases shared by tests/test_front_f64.py (CPU) and tests/test_gpu_front_kernels.py (GPU).

Test infrastructure (not a test file).  Every case fixes a seed and a shape; FP32_COST holds what
float32 costs the REFERENCE on exactly these inputs, per output tensor: tests/front_f64.py evaluated
in float32 on the CPU against float64, and for the fbank oracle.fbank (float32) against the float64
restatement under the fbank's own measure (front_f64.fbank_err).  The CPU file measures and checks
the figures; the GPU file takes its bounds from them (bound(): max(2e-5, 8 x figure), FLOOR and
MARGIN of tests/yardstick.py), so a figure is never anything a kernel produced.  Error measure:
max |got - ref| / max |ref| per tensor; integer and copied outputs are compared exactly.

Why each case is there (the launch code of the five sources names the numbers):

fbank (group "fb"; csrc/fbank.hip: a workgroup takes 32 frames of one utterance, its 4 waves pack
  frames (2i, 2i+1) into one complex 8x8x8 FFT, lanes stride the mel bins by 64; rows past an
  utterance's frames are 0 up to max_frames; pcm rows are padded with NaN behind each count and
  the row stride is wider than the longest row):
    fb_ragged     399 (no frame), 400, 559 (one), 560 (two), 400 + 160 {30, 31, 32} (31 / 32 / 33
                  frames: an odd last pair, one full workgroup, a second workgroup of one frame),
                  400 + 160 * 64 (65 frames) and 1597 samples (off the hop grid); noise + sine, 80 bins
    fb_mf_below, fb_mf_above   max_frames 20 and 40 on 33 / 2 frames: truncated rows; rows of zeros
    fb_m1, fb_m23 (high_freq -400), fb_m64 (high_freq 7600), fb_m65 (second trip of the lane loop),
    fb_m128       (the filters below bin 1 of the 128-bin table are empty: exactly log(eps))
    fb_tone_on, fb_tone_off    1000 Hz (bin 32 exactly) and 1234.5 Hz
    fb_quiet      noise of amplitude 1e-4            fb_zero   all zero: every value log(eps)
    fb_dc         0.5 everywhere (the mean takes everything)
    fb_square     +-1 in runs of 37 samples          fb_impulse   a few unit samples
    fb_loudsilent, fb_loudsilent_i16   noise next to exact silence so that an all-zero frame is
                  packed with a loud one as frame A and as frame B, at unit and at int16 sample scale
                  (scale_in = 1 in both: LhotseKaldiFeatFbank's energies reach 1e11 against eps)
    fb_scale      int16-scaled samples with scale_in = 2^-15: bit-identical to prescaled input
row energy (group "re"; one workgroup of 256 per row, threads stride the row):
    re_exp_d1, re_sq_d1        len * D = 0, 255, 256, 257, 100003 at D = 1
    re_exp_d80, re_sq_d80      0, 80, 240, 320, 100080 at D = 80; NaN behind every row; the rows are
                  scaled so that every sum is of order one (a short row weighs as much as a long one)
mix (group "mx"; grid min(1024, ceil(rows_max D / 256)) x B, grid-stride):
    mx0_wrap      MixFeats, D = 80, rows_max 20: (slen, nlen, start) = (20, 0, 0) copy-through,
                  (0, 5, 0), (7, 1, 0), (13, 3, 2) wrapping four times, (13, 40, 27) start at its maximum
    mx0_floor     values near -30 (the 1e-10 floor) and a row at -200 (exp = 0: energy 0, gain = 1)
    mx0_cap       rows_max D = 1024 * 256 + 257 (D = 3): a partial second trip
    mx1_clip      AddNoise: the clip on both sides; max_gain_db = 10 holding a quiet noise
    mx1_silent    src silent, noise silent, both silent: the output is the source, bit for bit
    mx1_cap       rows_max = 1024 * 256 + 257 at D = 1, slen shorter than rows_max
specaug (group "sa"; exact): sa_t0f0 ... sa_t5f5  (nt, nf) over {0, 1, 2, 5}, B = 3, T = 11, F = 7,
    spans per row among empty, [T-1, T), the full range and random ones; NaN inside a span
    sa_cap        T F = 3281 * 80 just past 1024 * 256
pad_rows (group "pr"; exact): pr_d1, pr_d80 ragged with an empty row; pr_cap Lmax D past the cap
smoothed NLL (group "nll"; one workgroup per row, 256 threads stride K):
    nll_k2 ... nll_k8193   K = 2, 255, 256, 257, 1025, 8193 with rows 5 / 1, KL / CE, eps 0 / 0.1
                  and scale 0.5 / 1 / 8 spread over them
    nll_peak      one logit 60 above the rest, the label elsewhere
    nll_p100, nll_m100, nll_p1000, nll_m1000   rows offset by +-100 and +-1000
    nll_peak3_p1000, nll_peak3_m1000   three logits 60 above the rest (0, -0.3, -0.9 apart) on an
                  offset row: the largest gradient entries sit where the exponent's rounding lands
    nll_w0        row weights 1, 0, 0.5, 0, 2: a gradient row of exact zeros
    nll_badlabel  labels -1 and K: no label term in the loss; the gradient is w s (softmax - t_other)
BEST-RQ (group "rq"; one wave per label, 4 per workgroup, lanes stride the codebook by 64; exact):
    rq_d1_k1, rq_d1_k2 (opposite signs: at D = 1 every similarity is +-1), rq_d2_k63, rq_d16_k64,
    rq_d64_k65, rq_d16_k8192   (D, F, K, ncb, B, T): B T2 = 1, 1, 4, 5, 4, 4; T = 10 with NaN frames
    rq_tie_lane, rq_tie_neigh, rq_tie_ends   each label's winner duplicated 64 away / next to it / at
                  0 and K - 1: the lowest index wins
    rq_zero       zero features: label 1           rq_scale1000   winners scaled by 1000 keep the label
predictor context (group "pc"; forward one workgroup per (b,u); dw on min(64, max(1, rows / 32))
  row splits; d_emb by atomics; both gradients pre-filled):
    pc_d1_k1, pc_d50_k2 (Lo = 1), pc_d64_k8 (64 rows: 2 splits), pc_d65_k2 (8 * 257 rows: 64 splits),
    pc_d256_k2, pc_d257_k8, pc_d512_k1
    pc_blank      every token blank: one hot atomic row
    pc_clamp      tokens -1 and V           pc_v1   V = 1
"""
import functools
import math

import numpy as np
import torch

import front_f64 as FF
from yardstick import FLOOR, MARGIN, UNIT, bound_of, rel_err  # noqa: F401  (the rule of tests/yardstick.py)

CAP = 1024 * 256                      # elements one trip of an augment.hip stream covers


def _fb(seed, sig, lens, M=80, hf=0.0, amp=1.0, scale=1.0, mf=None, cmvn=False):
    return dict(group="fb", seed=seed, sig=sig, lens=lens, M=M, hf=hf, amp=amp, scale=scale, mf=mf, cmvn=cmvn)


def _nll(seed, K, rows, kind, eps, scale, shape="plain", off=0.0, w=None, bad=False):
    return dict(group="nll", seed=seed, K=K, rows=rows, kind=kind, eps=eps, scale=scale, shape=shape, off=off,
                w=w, bad=bad)


def _rq(seed, D, F, K, ncb, B, T, plant=None, nanpad=False, base=None):
    return dict(group="rq", seed=seed, D=D, F=F, K=K, ncb=ncb, B=B, T=T, plant=plant, nanpad=nanpad, base=base)


def _pc(seed, D, K, B, L, V=11, tok="rand"):
    return dict(group="pc", seed=seed, D=D, K=K, B=B, L=L, V=V, tok=tok)


F6 = [400 + 160 * 5 + 3, 400 + 160 * 2]
CASES = {
    # ---------------------------------------------------------------- fbank
    "fb_ragged": _fb(1, "noise_sine", [399, 400, 559, 560, 400 + 160 * 30, 400 + 160 * 31, 400 + 160 * 32,
                                       400 + 160 * 64, 1597], cmvn=True),
    "fb_mf_below": _fb(2, "noise_sine", [400 + 160 * 32, 560], mf=20, cmvn=True),
    "fb_mf_above": _fb(3, "noise_sine", [400 + 160 * 32, 560], mf=40, cmvn=True),
    "fb_m1": _fb(4, "noise_sine", F6, M=1), "fb_m23": _fb(5, "noise_sine", F6, M=23, hf=-400.0),
    "fb_m64": _fb(6, "noise_sine", F6, M=64, hf=7600.0), "fb_m65": _fb(7, "noise_sine", F6, M=65),
    "fb_m128": _fb(8, "noise_sine", F6, M=128),
    "fb_tone_on": _fb(9, "tone_on", F6), "fb_tone_off": _fb(10, "tone_off", F6),
    "fb_quiet": _fb(11, "quiet", F6), "fb_zero": _fb(12, "zero", F6), "fb_dc": _fb(13, "dc", F6),
    "fb_square": _fb(14, "square", F6), "fb_impulse": _fb(15, "impulse", F6),
    "fb_loudsilent": _fb(16, "loudsilent", [400 + 160 * 9] * 3),
    "fb_loudsilent_i16": _fb(18,"loudsilent", [400 + 160 * 9] * 3, amp=32768.0),
    "fb_scale": _fb(17, "noise_sine", F6, amp=32768.0, scale=2.0 ** -15),
    # ---------------------------------------------------------------- row energy
    "re_exp_d1": dict(group="re", seed=20, D=1, mode=0, lens=[0, 255, 256, 257, 100003]),
    "re_sq_d1": dict(group="re", seed=21, D=1, mode=1, lens=[0, 255, 256, 257, 100003]),
    "re_exp_d80": dict(group="re", seed=22, D=80, mode=0, lens=[0, 1, 3, 4, 1251]),
    "re_sq_d80": dict(group="re", seed=23, D=80, mode=1, lens=[0, 1, 3, 4, 1251]),
    # ---------------------------------------------------------------- mix
    "mx0_wrap": dict(group="mx", seed=30, mode=0, D=80, rows=20, kind="plain", max_gain=0.0,
                     slen=[20, 0, 7, 13, 13], nlen=[0, 5, 1, 3, 40], start=[0, 0, 0, 2, 27], nrows=40),
    "mx0_floor": dict(group="mx", seed=31, mode=0, D=80, rows=9, kind="floor", max_gain=0.0,
                      slen=[9, 6, 9], nlen=[9, 4, 12], start=[0, 3, 3], nrows=12),
    "mx0_cap": dict(group="mx", seed=32, mode=0, D=3, rows=(CAP + 257) // 3, kind="plain", max_gain=0.0,
                    slen=[(CAP + 257) // 3 - 100], nlen=[5000], start=[4999], nrows=5000),
    "mx1_clip": dict(group="mx", seed=33, mode=1, D=1, rows=700, kind="clip", max_gain=10.0,
                     slen=[700, 650, 700], nlen=[300, 1, 2000], start=[299, 0, 1300], nrows=2000),
    "mx1_silent": dict(group="mx", seed=34, mode=1, D=1, rows=300, kind="silent", max_gain=300.0,
                       slen=[300, 300, 300], nlen=[100, 100, 100], start=[0, 5, 99], nrows=100),
    "mx1_cap": dict(group="mx", seed=35, mode=1, D=1, rows=CAP + 257, kind="plain", max_gain=300.0,
                    slen=[CAP + 200], nlen=[7001], start=[7000], nrows=7001),
    # ---------------------------------------------------------------- specaug
    **{f"sa_t{nt}f{nf}": dict(group="sa", seed=40 + i, B=3, T=11, F=7, nt=nt, nf=nf)
       for i, (nt, nf) in enumerate(((0, 0), (1, 0), (0, 1), (2, 2), (5, 1), (1, 5), (5, 5), (2, 0), (0, 2)))},
    "sa_cap": dict(group="sa", seed=49, B=1, T=3281, F=80, nt=2, nf=2),
    # ---------------------------------------------------------------- pad_rows
    "pr_d1": dict(group="pr", seed=50, D=1, Lmax=9, rows=[3, 0, 9, 1]),
    "pr_d80": dict(group="pr", seed=51, D=80, Lmax=7, rows=[3, 0, 7, 1]),
    "pr_cap": dict(group="pr", seed=52, D=1, Lmax=CAP + 257, rows=[CAP + 257, 0, 5]),
    # ---------------------------------------------------------------- smoothed NLL
    "nll_k2": _nll(60, 2, 5, "kl", 0.1, 1.0), "nll_k255": _nll(61, 255, 1, "ce", 0.0, 0.5),
    "nll_k256": _nll(62, 256, 5, "kl", 0.0, 8.0), "nll_k257": _nll(63, 257, 5, "ce", 0.1, 1.0),
    "nll_k1025": _nll(64, 1025, 1, "kl", 0.1, 8.0), "nll_k8193": _nll(65, 8193, 5, "kl", 0.1, 1.0),
    "nll_k8193_ce": _nll(66, 8193, 5, "ce", 0.1, 0.5),
    "nll_peak": _nll(67, 1025, 5, "ce", 0.1, 1.0, shape="peak"),
    "nll_p100": _nll(68, 1025, 5, "kl", 0.1, 1.0, off=100.0), "nll_m100": _nll(69, 100, 5, "ce", 0.1, 1.0, off=-100.0),
    "nll_p1000": _nll(70, 8193, 5, "kl", 0.1, 1.0, off=1000.0),
    "nll_m1000": _nll(71, 1025, 5, "ce", 0.1, 1.0, off=-1000.0),
    "nll_peak3_p1000": _nll(72, 1025, 5, "kl", 0.1, 1.0, shape="peak3", off=1000.0),
    "nll_peak3_m1000": _nll(73, 8193, 5, "ce", 0.1, 1.0, shape="peak3", off=-1000.0),
    "nll_w0": _nll(74, 257, 5, "kl", 0.1, 1.0, w=[1.0, 0.0, 0.5, 0.0, 2.0]),
    "nll_badlabel": _nll(75, 257, 5, "kl", 0.1, 1.0, bad=True),
    # ---------------------------------------------------------------- BEST-RQ
    "rq_d1_k1": _rq(80, 1, 1, 1, 1, 1, 7), "rq_d1_k2": _rq(81, 1, 1, 2, 2, 1, 10, nanpad=True),
    "rq_d2_k63": _rq(82, 2, 83, 63, 2, 4, 10, nanpad=True), "rq_d16_k64": _rq(83, 16, 80, 64, 1, 5, 7),
    "rq_d64_k65": _rq(84, 64, 80, 65, 1, 2, 11), "rq_d16_k8192": _rq(85, 16, 80, 8192, 2, 2, 11),
    "rq_tie_lane": _rq(86, 16, 80, 130, 1, 3, 11, plant="lane"),
    "rq_tie_neigh": _rq(87, 16, 80, 130, 1, 3, 11, plant="neigh"),
    "rq_tie_ends": _rq(88, 16, 80, 130, 1, 3, 11, plant="ends"),
    "rq_zero": _rq(89, 16, 80, 65, 2, 2, 11, plant="zero"),
    "rq_scale1000": _rq(90, 16, 80, 64, 1, 5, 7, plant="scale", base="rq_d16_k64"),
    # ---------------------------------------------------------------- predictor context
    "pc_d1_k1": _pc(100, 1, 1, 2, 4), "pc_d50_k2": _pc(101, 50, 2, 8, 2), "pc_d64_k8": _pc(102, 64, 8, 4, 23),
    "pc_d65_k2": _pc(103, 65, 2, 8, 258), "pc_d256_k2": _pc(104, 256, 2, 3, 5),
    "pc_d257_k8": _pc(105, 257, 8, 2, 11), "pc_d512_k1": _pc(106, 512, 1, 2, 3),
    "pc_blank": _pc(107, 64, 2, 8, 9, tok="blank"), "pc_clamp": _pc(108, 64, 2, 4, 9, tok="clamp"),
    "pc_v1": _pc(109, 50, 2, 2, 6, V=1),
}
EXACT = ("sa", "pr", "rq")            # groups whose outputs are integers or copies: compared exactly


def names(group):
    return [k for k, v in CASES.items() if v["group"] == group]


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def tables(M, hf):
    """kernels.FbankTables on the CPU: the kernel's window, twiddles and compact mel filters."""
    from speech2text_amd.kernels import FbankTables
    return FbankTables(M, high_freq=hf, device="cpu")


def _signal(sig, n, rn, row):
    t = torch.arange(n, dtype=torch.float64)
    if sig == "noise_sine":
        return (0.1 * rn(n) + 0.3 * torch.sin(2 * math.pi * 440.0 * t / 16000.0).float())
    if sig in ("tone_on", "tone_off"):
        f = 1000.0 if sig == "tone_on" else 1234.5
        return (0.5 * torch.sin(2 * math.pi * f * t / 16000.0 + 0.3 * row)).float()
    if sig == "quiet":
        return 1.0e-4 * rn(n)
    if sig == "zero":
        return torch.zeros(n)
    if sig == "dc":
        return torch.full((n,), 0.5)
    if sig == "square":
        return 1.0 - 2.0 * ((torch.arange(n) // 37) % 2).float()
    if sig == "impulse":
        x = torch.zeros(n)
        x[[5, 399, 400, 561, n - 1]] = 1.0
        return x
    if sig == "loudsilent":
        x = 0.3 * rn(n)
        if row == 0:
            x[480:] = 0.0            # frames 3 ... silent: pair (2,3) has the silence as frame B
        elif row == 1:
            x[:720] = 0.0            # frames 0, 1, 2 silent: pair (2,3) has the silence as frame A
        else:
            x[480:1200] = 0.0        # frames 3, 4, 5 silent between loud ones: both positions
        return x
    raise KeyError(sig)


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict of the case's float32 / integer CPU inputs (shared: do not modify)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(7000 + c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)                        # noqa: E731
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g)      # noqa: E731
    grp = c["group"]
    if grp == "fb":
        lens = c["lens"]
        stride = max(lens) + 13
        pcm = torch.full((len(lens), stride), float("nan"))
        for b, n in enumerate(lens):
            pcm[b, :n] = _signal(c["sig"], n, rn, b) * c["amp"]
        t = dict(pcm=pcm, lens=lens, mean=None, istd=None)
        if c["cmvn"]:
            t.update(mean=rn(c["M"]) - 8.0, istd=0.2 + ru(c["M"]))
        return t
    if grp == "re":
        D, lens = c["D"], c["lens"]
        stride = max(lens) * D + 7
        x = torch.full((len(lens), stride), float("nan"))
        for b, n in enumerate(lens):
            n *= D
            if n:
                x[b, :n] = (rn(n) - math.log(n)) if c["mode"] == 0 else rn(n) / math.sqrt(n)
        return dict(x=x, lens=lens)
    if grp == "mx":
        B, R, D, NR, mode = len(c["slen"]), c["rows"], c["D"], c["nrows"], c["mode"]
        sstride = R * D + 5
        if mode == 0:
            src, noise = rn(B, R, D) * 2 - 4, rn(B, NR, D) * 2 - 5
            if c["kind"] == "floor":
                src[0], noise[0] = rn(R, D) * 0.5 - 30, rn(NR, D) * 0.5 - 31
                src[1] = -200.0
        else:
            src, noise = 0.1 * rn(B, R, D), 0.05 * rn(B, NR, D)
            if c["kind"] == "clip":
                src[0], noise[0] = 0.6 * rn(R, D), 0.5 * rn(NR, D)
                noise[1] = 1.0e-3 * rn(NR, D)            # wants +28 dB at snr 5; max_gain_db = 10 holds it
            if c["kind"] == "silent":
                src[0] = 0.0
                noise[1] = 0.0
                src[2], noise[2] = 0.0, 0.0
        slen, nlen = torch.tensor(c["slen"]), torch.tensor(c["nlen"])
        for b in range(B):
            noise[b, int(nlen[b]):] = float("nan")
        snr = 5.0 + 10.0 * ru(B)
        se = FF.row_energy_ref(src.double().reshape(B, -1), c["slen"], D, 1 if mode else 0).float()
        ne = FF.row_energy_ref(noise.double().reshape(B, -1), c["nlen"], D, 1 if mode else 0).float()
        return dict(src=src, noise=noise, slen=slen, nlen=nlen, start=torch.tensor(c["start"]), snr=snr, se=se,
                    ne=ne, sstride=sstride)
    if grp == "sa":
        B, T, F, nt, nf = c["B"], c["T"], c["F"], c["nt"], c["nf"]
        feats = rn(B, T, F)

        def spans(n, size):
            s = torch.zeros(B, max(n, 1), 2, dtype=torch.int32)
            for b in range(B):
                for k in range(n):
                    a = int(ri(0, size, 1))
                    s[b, k] = torch.tensor([a, min(size, a + int(ri(1, max(2, size // 2), 1)))])
            if n:                                       # the edges, a different one per row
                s[0, 0] = torch.tensor([size - 1, size])
            if n and B >= 3:
                s[1, 0] = torch.tensor([3, 3])
                s[2, 0] = torch.tensor([1, size - 2])
                if n >= 5:
                    s[2, 4] = torch.tensor([0, size])
            return s[:, :n].contiguous()
        tspan, fspan = spans(nt, T), spans(nf, F)
        hit = FF.specaug_ref(torch.ones(B, T, F), tspan, fspan) == 0
        idx = hit.nonzero()
        if len(idx):
            for i in idx[:: max(1, len(idx) // 5)]:
                feats[tuple(i.tolist())] = float("nan")
        return dict(feats=feats, tspan=tspan, fspan=fspan, hit=hit)
    if grp == "pr":
        offs = [0]
        for r in c["rows"]:
            offs.append(offs[-1] + r * c["D"])
        return dict(packed=rn(max(offs[-1], 1)), offsets=offs)
    if grp == "nll":
        K, R = c["K"], c["rows"]
        x = rn(R, K)
        labels = ri(0, K, R)
        if c["shape"] in ("peak", "peak3"):
            for r in range(R):
                p = int(ri(0, K - 3, 1))
                x[r, p] += 60.0
                if c["shape"] == "peak3":
                    x[r, p + 1] = x[r, p] - 0.3
                    x[r, p + 2] = x[r, p] - 0.9
                labels[r] = (p + 7) % K
        x = x + c["off"]
        if c["bad"]:
            labels[1], labels[3] = -1, K
        w = torch.tensor(c["w"]) if c["w"] else 0.5 + ru(R)
        return dict(x=x, labels=labels, w=w)
    if grp == "rq":
        if c["base"]:
            t = dict(make(c["base"]))
            cb = t["codebooks"].clone()
            for i in range(c["ncb"]):
                for k in np.unique(FF.bestrq_gap(t["feats"], t["proj"], t["codebooks"])[0][i]) - 1:
                    cb[i, k] *= 1000.0
            t["codebooks"] = cb
            return t
        D, F, K, ncb, B, T = (c[k] for k in ("D", "F", "K", "ncb", "B", "T"))
        feats, proj, cb = rn(B, T, F), rn(F * 9, D), rn(ncb, K, D)
        if c["nanpad"]:
            feats[:, 7:] = float("nan")
        if c["plant"] == "zero":
            feats.zero_()
        if name == "rq_d1_k2":
            cb[:, 0], cb[:, 1] = cb[:, 0].abs() + 0.1, -cb[:, 1].abs() - 0.1
        if c["plant"] in ("lane", "neigh", "ends"):
            win = FF.bestrq_gap(feats, proj, cb)[0][0].reshape(-1) - 1
            for i, w in enumerate(win.tolist()):
                if c["plant"] == "ends":
                    cb[0, 0] = cb[0, K - 1] = cb[0, w]
                    break
                step = 64 if c["plant"] == "lane" else 1
                j = w + step if (i % 2 == 0 and w + step < K) or w - step < 0 else w - step
                if j not in win.tolist():
                    cb[0, j] = cb[0, w]
        return dict(feats=feats, proj=proj, codebooks=cb, T2=((T - 3) // 2 + 1 - 3) // 2 + 1)
    if grp == "pc":
        D, K, B, L, V = (c[k] for k in ("D", "K", "B", "L", "V"))
        tok = ri(0, V, B, L).to(torch.int32)
        if c["tok"] == "blank":
            tok.zero_()
        if c["tok"] == "clamp":
            tok[0, 1], tok[1, 0], tok[2, L - 1], tok[3, 4] = -1, V, V, -1
        Lo = L - K + 1
        return dict(tok=tok, emb=rn(V, D), w=rn(D, K) * 0.5, g=rn(B, Lo, D), de0=rn(V, D), dw0=rn(D, K))
    raise KeyError(grp)


# ------------------------------------------------------------------ the yardstick on a case
def evaluate(name, dtype):
    """The yardstick (tests/front_f64.py) on the case's inputs cast to `dtype` -> {tensor name: tensor}.
    fbank: {"energy": [per utterance (frames, M) mel energies]} (float64 only; see fp32_figures)."""
    c, t = CASES[name], make(name)
    grp = c["group"]
    if grp == "fb":
        tab = tables(c["M"], c["hf"])
        return dict(energy=[FF.fbank_energy_ref(t["pcm"][b].to(dtype), n, tab, c["scale"])
                            for b, n in enumerate(t["lens"])])
    if grp == "re":
        return dict(e=FF.row_energy_ref(t["x"].to(dtype), t["lens"], c["D"], c["mode"]))
    if grp == "mx":
        return dict(out=FF.mix_ref(t["src"].to(dtype), t["slen"], t["noise"].to(dtype), t["nlen"], t["start"],
                                   t["snr"].to(dtype), t["se"].to(dtype), t["ne"].to(dtype), c["mode"],
                                   c["max_gain"]))
    if grp == "sa":
        return dict(out=FF.specaug_ref(t["feats"], t["tspan"], t["fspan"]))
    if grp == "pr":
        return dict(out=FF.pad_rows_ref(t["packed"], t["offsets"], c["D"], c["Lmax"]))
    if grp == "nll":
        cst = FF.nll_consts(c["K"], c["eps"], c["kind"])
        x, w = t["x"].to(dtype), t["w"].to(dtype)
        return dict(row=FF.smoothed_nll_ref(x, t["labels"], c["scale"], *cst).detach(),
                    grad=FF.smoothed_nll_grad_ref(x, t["labels"], w, c["scale"], *cst, stated=c["bad"]))
    if grp == "rq":
        from oracle import best_rq as OB
        return dict(labels=torch.from_numpy(OB.make_labels(t["feats"].numpy(), t["proj"].numpy(),
                                                           t["codebooks"].numpy())))
    if grp == "pc":
        emb, w = (t[k].to(dtype).clone().requires_grad_(True) for k in ("emb", "w"))
        out = FF.predictor_ctx_ref(t["tok"], emb, w)
        (out * t["g"].to(dtype)).sum().backward()
        return dict(out=out.detach(), d_emb=t["de0"].to(dtype) + emb.grad, d_w=t["dw0"].to(dtype) + w.grad)
    raise KeyError(grp)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


def fp32_figures(name):
    """{tensor: error of the float32 CPU evaluation against float64}; fbank: oracle.fbank (float32)
    against the float64 energies under front_f64.fbank_err, the largest over the utterances."""
    c, ref = CASES[name], reference(name)
    if c["group"] == "fb":
        from oracle import fbank as OF
        t = make(name)
        worst = 0.0
        for b, n in enumerate(t["lens"]):
            x = (t["pcm"][b, :n] * c["scale"]).numpy()
            worst = max(worst, FF.fbank_err(torch.from_numpy(OF.fbank(x, c["M"], high_freq=c["hf"])), ref["energy"][b]))
        return dict(feat=worst)
    if c["group"] in EXACT:
        return {}
    f32 = evaluate(name, torch.float32)
    return {k: rel_err(f32[k], ref[k]) for k in ref}


def bound(name, tensor):
    """Allowed error of device tensor `tensor` of case `name`: max(FLOOR, MARGIN x the float32 figure of
    the yardstick) = max(2e-5, 8 x figure).  No derived exception is needed."""
    return bound_of(FP32_COST[name][tensor])


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figures(name), rounded up to two digits; tests/test_front_f64.py re-measures every one to a
# factor 4 both ways after raising both to UNIT (yardstick.UNIT, one float32 rounding).
FP32_COST = {
    "fb_ragged": dict(feat=4.2e-07),
    "fb_mf_below": dict(feat=3.9e-07),
    "fb_mf_above": dict(feat=5.0e-07),
    "fb_m1": dict(feat=2.1e-07),
    "fb_m23": dict(feat=3.1e-07),
    "fb_m64": dict(feat=2.1e-07),
    "fb_m65": dict(feat=2.4e-07),
    "fb_m128": dict(feat=2.5e-07),
    "fb_tone_on": dict(feat=2.2e-07),
    "fb_tone_off": dict(feat=2.6e-07),
    "fb_quiet": dict(feat=4.6e-07),
    "fb_zero": dict(feat=4.4e-07),
    "fb_dc": dict(feat=4.4e-07),
    "fb_square": dict(feat=3.7e-07),
    "fb_impulse": dict(feat=4.4e-07),
    "fb_loudsilent": dict(feat=4.4e-07),
    "fb_loudsilent_i16": dict(feat=9.1e-07),
    "fb_scale": dict(feat=2.1e-07),
    "re_exp_d1": dict(e=7.1e-08),
    "re_sq_d1": dict(e=6.5e-08),
    "re_exp_d80": dict(e=4.9e-08),
    "re_sq_d80": dict(e=2.2e-08),
    "mx0_wrap": dict(out=3.4e-08),
    "mx0_floor": dict(out=3.2e-09),
    "mx0_cap": dict(out=5.2e-08),
    "mx1_clip": dict(out=4.3e-08),
    "mx1_silent": dict(out=0.0e+00),
    "mx1_cap": dict(out=7.4e-08),
    "sa_t0f0": dict(),
    "sa_t1f0": dict(),
    "sa_t0f1": dict(),
    "sa_t2f2": dict(),
    "sa_t5f1": dict(),
    "sa_t1f5": dict(),
    "sa_t5f5": dict(),
    "sa_t2f0": dict(),
    "sa_t0f2": dict(),
    "sa_cap": dict(),
    "pr_d1": dict(),
    "pr_d80": dict(),
    "pr_cap": dict(),
    "nll_k2": dict(row=8.7e-08, grad=6.2e-08),
    "nll_k255": dict(row=7.7e-08, grad=1.1e-08),
    "nll_k256": dict(row=2.1e-08, grad=7.4e-08),
    "nll_k257": dict(row=1.2e-07, grad=6.8e-08),
    "nll_k1025": dict(row=5.2e-08, grad=6.3e-07),
    "nll_k8193": dict(row=8.3e-08, grad=6.5e-08),
    "nll_k8193_ce": dict(row=4.1e-08, grad=5.7e-08),
    "nll_peak": dict(row=6.9e-08, grad=8.5e-07),
    "nll_p100": dict(row=6.4e-08, grad=4.7e-08),
    "nll_m100": dict(row=7.5e-08, grad=5.7e-08),
    "nll_p1000": dict(row=1.3e-07, grad=8.7e-08),
    "nll_m1000": dict(row=6.7e-08, grad=4.9e-08),
    "nll_peak3_p1000": dict(row=6.8e-08, grad=2.9e-07),
    "nll_peak3_m1000": dict(row=7.5e-08, grad=5.3e-06),
    "nll_w0": dict(row=8.6e-08, grad=6.7e-08),
    "nll_badlabel": dict(row=6.7e-08, grad=9.1e-08),
    "rq_d1_k1": dict(),
    "rq_d1_k2": dict(),
    "rq_d2_k63": dict(),
    "rq_d16_k64": dict(),
    "rq_d64_k65": dict(),
    "rq_d16_k8192": dict(),
    "rq_tie_lane": dict(),
    "rq_tie_neigh": dict(),
    "rq_tie_ends": dict(),
    "rq_zero": dict(),
    "rq_scale1000": dict(),
    "pc_d1_k1": dict(out=1.5e-08, d_emb=3.1e-08, d_w=3.4e-07),
    "pc_d50_k2": dict(out=4.4e-08, d_emb=3.8e-08, d_w=1.2e-07),
    "pc_d64_k8": dict(out=7.2e-08, d_emb=1.5e-07, d_w=7.7e-08),
    "pc_d65_k2": dict(out=6.3e-08, d_emb=3.2e-07, d_w=1.9e-07),
    "pc_d256_k2": dict(out=5.1e-08, d_emb=5.1e-08, d_w=7.2e-08),
    "pc_d257_k8": dict(out=8.2e-08, d_emb=1.2e-07, d_w=8.6e-08),
    "pc_d512_k1": dict(out=4.3e-08, d_emb=3.6e-08, d_w=8.0e-08),
    "pc_blank": dict(out=7.1e-08, d_emb=6.2e-08, d_w=6.9e-08),
    "pc_clamp": dict(out=6.1e-08, d_emb=1.1e-07, d_w=7.8e-08),
    "pc_v1": dict(out=4.5e-08, d_emb=3.5e-08, d_w=4.9e-08),
}
