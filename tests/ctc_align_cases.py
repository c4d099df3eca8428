"""Seeded cases shared by tests/test_ctc_align_f64.py (CPU) and tests/test_gpu_ctc_align.py (GPU): CTC
forced alignment, csrc/ctc_align.hip.

Test infrastructure (not a test file).  A case is logits (B,T,V) = scale x normal (raw logits; rows that
are already log-probabilities where `special` says so; multiples of 0.25 where `quant`), lengths, targets
(B, Umax + pad) and target lengths.  Frames at or beyond lengths[b] are NaN: nothing may read them.  The
shapes are the smallest at which the kernel can still go wrong:

  U    0, 1; 63 / 64 (2U+1 = 127 / 129: one / two states per thread of the 128-thread recursion), 127 / 128
       (255 / 257: two / four), 255 / 256 (511 / 513: four / eight), 511 / 512 (1023 / 1025: eight / sixteen)
       and S2T_CTC_MAX_LABELS = 1023, with T just large enough to be feasible;
  T    1; U + repeats exactly (the tight feasible alignment of a transcript with doubled labels, which
       need a blank between them), U + repeats - 1 (infeasible), below U;
  rows kinds cycled over the batch (ROW KINDS below): full, tight, one frame too few, no frames, a length
       above T, fewer frames than labels, random; batches of 1, 17 and 33;
  tgt  a target row stride above Umax; target lengths ragged with 0 and a negative entry;
  V    3, 65, 300; a blank that is not class 0;
  -inf rows of log-probabilities with classes at -inf: an utterance with T >= U that is still infeasible,
       one forced through a single path;
  form the backpointers in LDS and through the workspace (S2T_CTC_ALIGN_LDS_BYTES decides): at U 255 the
       edge lies between T 315 and 316, at U 256 between 280 and 281, at U 5 between 2275 and 2276; U 511,
       512 and 1023 are workspace shapes of several blocks.  FORMS records what s2t_ctc_align_form must
       answer for every case.

The conditions, with no exclusions (tests/test_ctc_align_f64.py asserts them; seeds and scales were chosen
on the CPU so that the restatement alone satisfies them): the float32 and the float64 run of the
restatement return the same ok, path and spans on every utterance of every case; every TIES case has at
least one tied decision on its best path.

COST holds what float32 costs the RESTATEMENT (tests/ctc_align_f64.py in float32 on the CPU against
float64) on exactly these inputs, in the sense of yardstick.rel_err over the feasible rows, the larger of
score's and tok_logp's; the GPU bounds are max(FLOOR, MARGIN x figure), the rule of tests/yardstick.py.
"""
import functools

import torch

import ctc_align_f64 as A
from yardstick import FLOOR, MARGIN, bound_of, clamp, rel_err  # noqa: F401  (the rule of tests/yardstick.py)

KINDS = ("full", "tight", "less", "zero", "above", "short", "rand")


def _c(seed, V, B, U, T=None, slack=0, rows=("full",), tl="full", blank=0, pad=0, scale=2.0, quant=False,
       special=None, doubled=True):
    return dict(seed=seed, V=V, B=B, U=U, T=T, slack=slack, rows=rows, tl=tl, blank=blank, pad=pad, scale=scale,
                quant=quant, special=special, doubled=doubled)


CASES = {
    "u0_t1": _c(0, 3, 1, 0, T=1),
    "u0_b17_ragged": _c(1, 65, 17, 0, T=5, rows=KINDS),
    "u1_t1": _c(2, 3, 1, 1, T=1, doubled=False),
    "u1_b3_t1_blank2": _c(3, 3, 3, 1, T=1, blank=2, doubled=False),
    "u3_tight_aab": _c(4, 3, 3, 3, rows=("tight", "less", "short")),
    "u7_v65_b17_ragged": _c(5, 65, 17, 7, slack=3, rows=KINDS, tl="ragged", pad=3),
    "u12_v300_b33_ragged_blank7": _c(6, 300, 33, 12, slack=5, rows=KINDS, tl="ragged", blank=7, pad=1),
    "u9_v11_logp_inf": _c(7, 11, 4, 9, slack=6, special="inf"),
    "u63_v3": _c(8, 3, 2, 63, rows=("tight", "full"), slack=4),
    "u64_v65": _c(9, 65, 3, 64, rows=("tight", "less", "full"), slack=2, tl="ragged"),
    "u127_v65": _c(10, 65, 2, 127, rows=("full", "tight"), slack=3),
    "u128_v3": _c(11, 3, 2, 128, rows=("tight", "less")),
    "u255_t315_lds": _c(12, 300, 2, 255, T=315, rows=("full", "tight")),
    "u255_t316_ws": _c(12, 300, 2, 255, T=316, rows=("full", "tight")),
    "u256_t280_lds": _c(13, 300, 1, 256, T=280),
    "u256_t281_ws": _c(13, 300, 2, 256, T=281, rows=("full", "rand")),
    "u5_t2275_lds": _c(14, 3, 1, 5, T=2275),
    "u5_t2276_ws": _c(14, 3, 2, 5, T=2276, rows=("full", "rand")),
    "u511_ws": _c(15, 65, 1, 511, slack=2),
    "u512_ws": _c(16, 65, 2, 512, slack=1, rows=("full", "tight")),
    "u1023_max_tight": _c(17, 65, 1, 1023, rows=("tight",)),
    "ties_v3": _c(20, 3, 3, 4, slack=6, scale=1.0, quant=True),
    "ties_v11_b17": _c(21, 11, 17, 6, slack=7, rows=KINDS, tl="ragged", scale=1.0, quant=True),
    "ties_u64_v3": _c(22, 3, 2, 64, slack=9, scale=1.0, quant=True),
}
TIES = [k for k, v in CASES.items() if v["quant"]]
_WS = 256                                                  # S2T_CTC_ALIGN_FORM_WORKSPACE
FORMS = {                                                  # what s2t_ctc_align_form(T, Umax) answers
    "u0_t1": 1, "u0_b17_ragged": 1, "u1_t1": 1, "u1_b3_t1_blank2": 1, "u3_tight_aab": 1, "u7_v65_b17_ragged": 1,
    "u12_v300_b33_ragged_blank7": 1, "u9_v11_logp_inf": 1, "u63_v3": 1, "u64_v65": 2, "u127_v65": 2, "u128_v3": 4,
    "u255_t315_lds": 4, "u255_t316_ws": 4 + _WS, "u256_t280_lds": 8, "u256_t281_ws": 8 + _WS, "u5_t2275_lds": 1,
    "u5_t2276_ws": 1 + _WS, "u511_ws": 8 + _WS, "u512_ws": 16 + _WS, "u1023_max_tight": 16 + _WS,
    "ties_v3": 1, "ties_v11_b17": 1, "ties_u64_v3": 2,
}


def need(targets):
    """The fewest frames a transcript can be aligned to: its labels and a blank between doubled ones."""
    return len(targets) + sum(a == b for a, b in zip(targets, targets[1:]))


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict(x (B,T,V) float32, NaN at and beyond lengths[b]; lens (B); targets (B, U + pad), the first
    U columns are the labels' (U = the case's padded width); tl (B) target lengths (0 and negative
    entries where ragged); blank; U; T).  Computed once per process and shared (do not modify)."""
    c = CASES[name]
    V, B, U, blank = c["V"], c["B"], c["U"], c["blank"]
    g = torch.Generator().manual_seed(7000 + c["seed"])
    r = torch.randint(0, V - 1, (B, U + c["pad"]), generator=g)
    targets = r + (r >= blank).long()                      # any class but blank
    if c["doubled"] and U >= 2:
        targets[:, 1] = targets[:, 0]                      # "a a b": a blank must stand between
    if c["tl"] == "full":
        tl = torch.full((B,), U, dtype=torch.int64)
    else:
        tl = torch.randint(1, U + 1, (B,), generator=g)
        tl[0] = U
        if B > 1:
            tl[1] = 0
        if B > 2:
            tl[2] = -2
    rows = [targets[b, :max(int(tl[b]), 0)].tolist() for b in range(B)]
    needs = [need(t) for t in rows]
    T = c["T"] if c["T"] is not None else max(max(needs), 1) + c["slack"]
    lens = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        kind = c["rows"][b % len(c["rows"])]
        assert kind in KINDS
        lens[b] = {"full": T, "tight": needs[b], "less": needs[b] - 1, "zero": 0, "above": T + 3,
                   "short": len(rows[b]) // 2,
                   "rand": int(torch.randint(1, T + 1, (1,), generator=g))}[kind]
    assert int(lens.max()) >= 0 and all(n <= T for n in needs)
    x = c["scale"] * torch.randn(B, T, V, generator=g)
    if c["quant"]:
        x = torch.round(x * 4.0) / 4.0
    if c["special"] == "inf":
        x = torch.log_softmax(x, dim=-1)
        x[0, :, rows[0][2]] = -float("inf")                # a label that no frame can emit: infeasible at T >= U
        path = []                                          # row 1: every frame allows one class only
        for u, lab in enumerate(rows[1]):
            if u and lab == rows[1][u - 1]:
                path.append(blank)
            path.append(lab)
            if u == 3:
                path += [lab, blank, blank]
        path += [blank] * (T - len(path))
        assert len(path) == T
        only = torch.full((T, V), -float("inf"))
        only[torch.arange(T), torch.tensor(path)] = x[1][torch.arange(T), torch.tensor(path)]
        x[1] = only
    for b in range(B):
        x[b, clamp(lens[b], T):] = float("nan")
    return dict(x=x, lens=lens, targets=targets, tl=tl, blank=blank, U=U, T=T)


def evaluate(name, dtype):
    """The restatement on a case in `dtype` -> per utterance a ctc_align_f64.Result."""
    m = make(name)
    out = []
    for b in range(m["x"].shape[0]):
        n = clamp(m["lens"][b], m["T"])
        u = min(max(int(m["tl"][b]), 0), m["U"])
        out.append(A.align(m["x"][b, :n].to(dtype), m["targets"][b, :u].tolist(), m["blank"]))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The float32 results of a case: the kernel's path, spans and raw_score bit for bit (do not modify)."""
    return evaluate(name, torch.float32)


def dense(results, T, U):
    """Per-utterance Results -> the entry's output tensors with its sentinels: (path (B,T) int32, tok_begin,
    tok_end (B,U) int32, tok_logp (B,U) float64, raw_score, score (B) float64, ok (B) int32)."""
    B = len(results)
    path = torch.full((B, T), -1, dtype=torch.int32)
    tb = torch.full((B, U), -1, dtype=torch.int32)
    te = torch.full((B, U), -1, dtype=torch.int32)
    lp = torch.zeros((B, U), dtype=torch.float64)
    raw = torch.tensor([r.raw_score for r in results], dtype=torch.float64)
    score = torch.tensor([r.score for r in results], dtype=torch.float64)
    ok = torch.tensor([int(r.ok) for r in results], dtype=torch.int32)
    for b, r in enumerate(results):
        if r.ok:
            n = len(r.tok_begin)
            path[b, :len(r.path)] = torch.tensor(r.path, dtype=torch.int32)
            tb[b, :n] = torch.tensor(r.tok_begin, dtype=torch.int32)
            te[b, :n] = torch.tensor(r.tok_end, dtype=torch.int32)
            lp[b, :n] = torch.tensor(r.tok_logp, dtype=torch.float64)
    return path, tb, te, lp, raw, score, ok


def errors(got_score, got_logp, name):
    """(rel_err of score over the feasible rows, rel_err of tok_logp) of tensors laid out as `dense`
    against the float64 reference of the case; 0.0 where a case has nothing to compare."""
    m = make(name)
    _, _, _, lp, _, score, ok = dense(reference(name), m["T"], m["U"])
    good = ok.bool()
    es = rel_err(got_score.cpu()[good], score[good]) if bool(good.any()) else 0.0
    el = rel_err(got_logp.cpu(), lp) if lp.numel() else 0.0
    return es, el


def fp32_figure(name):
    m = make(name)
    _, _, _, lp, _, score, _ = dense(restated(name), m["T"], m["U"])
    return max(errors(score, lp, name))


def bound(name):
    """Allowed rel_err of the device's score and tok_logp in case `name`."""
    return bound_of(COST[name])


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figure(name), rounded up to two digits, the value itself behind.
COST = {
    "u0_t1": 4.3e-07,                         # 4.291e-07
    "u0_b17_ragged": 4.1e-08,                 # 4.089e-08
    "u1_t1": 3.6e-08,                         # 3.570e-08
    "u1_b3_t1_blank2": 3.9e-08,               # 3.849e-08
    "u3_tight_aab": 2.9e-08,                  # 2.897e-08
    "u7_v65_b17_ragged": 1.3e-07,             # 1.203e-07
    "u12_v300_b33_ragged_blank7": 1.3e-07,    # 1.215e-07
    "u9_v11_logp_inf": 6.4e-08,               # 6.393e-08
    "u63_v3": 6.2e-08,                        # 6.186e-08
    "u64_v65": 5.3e-08,                       # 5.278e-08
    "u127_v65": 1.2e-07,                      # 1.130e-07
    "u128_v3": 5.4e-08,                       # 5.312e-08
    "u255_t315_lds": 3.0e-08,                 # 2.916e-08
    "u255_t316_ws": 5.1e-08,                  # 5.066e-08
    "u256_t280_lds": 6.2e-08,                 # 6.128e-08
    "u256_t281_ws": 1.1e-07,                  # 1.078e-07
    "u5_t2275_lds": 1.6e-07,                  # 1.574e-07
    "u5_t2276_ws": 4.4e-07,                   # 4.348e-07
    "u511_ws": 7.8e-08,                       # 7.798e-08
    "u512_ws": 7.6e-08,                       # 7.566e-08
    "u1023_max_tight": 5.7e-08,               # 5.646e-08
    "ties_v3": 8.4e-08,                       # 8.343e-08
    "ties_v11_b17": 1.7e-07,                  # 1.628e-07
    "ties_u64_v3": 1.1e-07,                   # 1.036e-07
}
