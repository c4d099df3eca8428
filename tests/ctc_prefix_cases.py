"""Seeded cases shared by tests/test_ctc_prefix_f64.py (CPU) and tests/test_gpu_ctc_prefix_beam.py (GPU):
the CTC prefix beam search of csrc/decode_ctc.hip, plain and with RNN-LM shallow fusion.

Test infrastructure (not a test file).  A case is logits (B,T,V) = scale x normal (rows of raw logits, or
rows that are already log-probabilities where `norm`), lengths (T, 0, above T, ragged), the search's
settings and for the fused entry a language model of tests/rnnt_lm_fusion_cases.py (LM_MODELS, paired by
V), lm_weight and the start token.  Frames at or beyond lengths[b] are NaN: nothing may read them.  The
shapes are the smallest at which the kernel can still go wrong: V 3, 11, 63, 65, 128 around the wave,
V 300 above the workgroup's 256 threads (a thread then owns two columns of the frame; a frame is staged
in LDS whole at every V the entry accepts, there is no spill path), batches of 1, 17 and 33, beams 1, 2,
4, 16, cutoff_top_k 1, 3, 16 and above V.

The conditions, with no exclusions (tests/test_ctc_prefix_f64.py asserts them; seeds and scales were
chosen on the CPU so that the restatement alone satisfies them): every utterance of every case is
decided by at least rnnt_lstm_search_f64.MARGIN in float64 and the float32 CPU run of the restatement
returns the same tokens; across the cases extensions land on live prefixes; in REENTER cases a prefix
that had left the beam is kept again next to one of its own extensions (what an inexact prefix identity
gets wrong); in LM_CHANGES cases the LM changes a hypothesis against lm_weight = 0.

COST holds what float32 costs the RESTATEMENT (tests/ctc_prefix_f64.py in float32 on the CPU against
float64) on exactly these inputs, in the sense of yardstick.rel_err, the larger of score's and
lm_score's; the GPU bounds are max(2e-5, 8 x figure), the rule of tests/yardstick.py.
"""
import functools

import torch

import ctc_prefix_f64 as P
import rnnt_lm_fusion_cases as L
from yardstick import FLOOR, MARGIN, bound_of, clamp, rel_err  # noqa: F401  (the rule of tests/yardstick.py)


def _c(seed, V, T, B, beam, topk, scale, lens="full", norm=False, lm=None, lm_seed=0, weight=0.0, start=None):
    return dict(seed=seed, V=V, T=T, B=B, beam=beam, topk=topk, scale=scale, lens=lens, norm=norm, lm=lm,
                lm_seed=lm_seed, weight=weight, start=start)


CASES = {
    "p_v3_beam4_kV": _c(0, 3, 9, 1, 4, 5, 1.0),                       # cutoff_top_k above V
    "p_v11_b17_beam2_k3": _c(2, 11, 13, 17, 2, 3, 2.0, lens="ragged"),
    "p_v63_beam16_k16": _c(18, 63, 20, 2, 16, 16, 2.0, lens="above"),
    "p_v65_b33_beam4_k3_norm": _c(23, 65, 12, 33, 4, 3, 2.0, lens="ragged", norm=True),
    "p_v128_beam1_k1": _c(0, 128, 40, 3, 1, 1, 2.0, lens="ragged"),
    "p_v128_beam4_k4": _c(3, 128, 40, 2, 4, 4, 1.0),
    "p_v300_beam4_k4": _c(2, 300, 10, 2, 4, 4, 2.0),
    "p_v6_reenter": _c(56, 6, 24, 1, 3, 3, 0.6),
    "p_v5_reenter": _c(41, 5, 30, 1, 2, 3, 0.3),
    "l_v63_lm20_beam4": _c(1, 63, 14, 3, 4, 4, 1.0, lens="ragged", lm="lm20", lm_seed=0, weight=0.5),
    "l_v65_lm48_b17_beam4_k3": _c(2, 65, 10, 17, 4, 3, 1.0, lens="ragged", lm="lm48", lm_seed=0, weight=0.5),
    "l_v128_lm64_beam16_start": _c(10, 128, 12, 2, 16, 4, 1.0, lm="lm64", lm_seed=1, weight=0.3, start=127),
    "l_v11_lm20_beam1_k1": _c(0, 11, 15, 2, 1, 1, 2.0, lm="lm20_v11", lm_seed=1, weight=0.5),
}
PLAIN_CASES = [k for k, v in CASES.items() if v["lm"] is None]
LM_CASES = [k for k, v in CASES.items() if v["lm"] is not None]
REENTER = ["p_v6_reenter", "p_v5_reenter"]
LM_CHANGES = ["l_v63_lm20_beam4", "l_v65_lm48_b17_beam4_k3", "l_v128_lm64_beam16_start"]


def lengths_of(c):
    B, T = c["B"], c["T"]
    if c["lens"] == "full":
        return torch.full((B,), T, dtype=torch.int64)
    if c["lens"] == "above":
        return torch.tensor([T + 3] + [T] * (B - 1), dtype=torch.int64)
    lens = torch.tensor([T - (5 * b) % (T - 1) for b in range(B)], dtype=torch.int64)    # ragged, 2..T
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = T + 3
    return lens


def make(name):
    """-> (logits (B,T,V) float32, NaN at and beyond lengths[b]; lengths (B); LM state dict or None)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    x = c["scale"] * torch.randn(c["B"], c["T"], c["V"], generator=g)
    if c["norm"]:
        x = torch.log_softmax(x, dim=-1)
    lens = lengths_of(c)
    for b in range(c["B"]):
        x[b, clamp(lens[b], c["T"]):] = float("nan")
    sd = L.lm_weights(c["lm"], c["lm_seed"]) if c["lm"] else None
    assert sd is None or L.LM_MODELS[c["lm"]]["V"] == c["V"]
    return x, lens, sd


def evaluate(name, dtype, lm_weight=None):
    """The restatement on a case in `dtype` -> per utterance a ctc_prefix_f64.Result."""
    c = CASES[name]
    x, lens, sd = make(name)
    if sd is not None:
        sd = L.cast(sd, dtype)
    w = c["weight"] if lm_weight is None else lm_weight
    return [P.prefix_beam_search(x[b, :clamp(lens[b], c["T"])].to(dtype), c["beam"], c["topk"], 0, sd, w, c["start"])
            for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


@functools.lru_cache(maxsize=None)
def unfused(name):
    """The float64 results of an LM case at lm_weight = 0 (do not modify)."""
    return evaluate(name, torch.float64, lm_weight=0.0)


def fp32_figure(name):
    ref, f32 = reference(name), evaluate(name, torch.float32)
    fields = (1, 2) if CASES[name]["lm"] else (1,)
    f64 = lambda rows, i: torch.tensor([r[i] for r in rows], dtype=torch.float64)    # noqa: E731
    return max(rel_err(f64(f32, i), f64(ref, i)) for i in fields)


def bound(name):
    """Allowed rel_err of the device's score and lm_score in case `name`."""
    return bound_of(COST[name])


# ------------------------------------------------------------------ the exhaustive cases
BRUTE = ((3, 3, 100), (6, 2, 100))    # (T, V, seeds): beam 16 holds every reachable prefix, the search is exact


def brute_logits(T, V, n):
    g = torch.Generator().manual_seed(9000 + 10 * T + V)
    return 2.0 * torch.randn(n, T, V, generator=g)


@functools.lru_cache(maxsize=None)
def brute_reference(T, V, n):
    """Per seed ctc_prefix_f64.brute_force over all V^T alignments (do not modify)."""
    x = brute_logits(T, V, n)
    return [P.brute_force(x[i]) for i in range(n)]


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figure(name), rounded up to two digits, the value itself behind.
COST = {
    "p_v3_beam4_kV": 2.5e-08,                 # 2.459e-08
    "p_v11_b17_beam2_k3": 1.2e-07,            # 1.136e-07
    "p_v63_beam16_k16": 1.1e-07,              # 1.036e-07
    "p_v65_b33_beam4_k3_norm": 1.3e-07,       # 1.299e-07
    "p_v128_beam1_k1": 5.0e-08,               # 4.937e-08
    "p_v128_beam4_k4": 1.7e-07,               # 1.690e-07
    "p_v300_beam4_k4": 1.2e-07,               # 1.134e-07
    "p_v6_reenter": 8.8e-08,                  # 8.794e-08
    "p_v5_reenter": 8.2e-09,                  # 8.156e-09
    "l_v63_lm20_beam4": 1.7e-07,              # 1.679e-07
    "l_v65_lm48_b17_beam4_k3": 9.3e-08,       # 9.211e-08
    "l_v128_lm64_beam16_start": 1.3e-07,      # 1.292e-07
    "l_v11_lm20_beam1_k1": 1.4e-07,           # 1.320e-07
}
