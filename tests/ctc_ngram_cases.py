"""Seeded cases shared by tests/test_ctc_ngram_f64.py (CPU) and tests/test_gpu_ctc_ngram.py (GPU): the CTC
prefix beam search fused with a back-off n-gram (csrc/decode_ctc.hip s2t_ctc_prefix_beam_ngram).

Test infrastructure (not a test file).  A case is an ARPA text and logits.  The text is an order-`order`
model estimated (NgramLm.estimate, written by to_arpa) on `n_tokens` seeded tokens of a sparse
first-order source over the non-blank classes, so that its tables are sparse and every back-off depth
occurs; the code under test reads the text with NgramLm.from_arpa, the restatement with its own parser
into its own dicts (tests/ctc_ngram_f64.py): they share the text, no table.  The logits (B,T,V) are scale x
normal with a bump of `plant` on a path that spells a training sentence (token, blank, token, ...), so
that hypotheses walk into deep contexts while the noise's classes back off from them; rows that are
already log-probabilities where `norm`; lengths T, 0, above T, ragged; frames at or beyond lengths[b]
are NaN: nothing may read them.  The shapes are tests/ctc_prefix_cases.py's: V 3, 11, 63, 65, 128 around
the wave, V 300 where a thread owns two columns, batches of 1, 17 and 33, beams 1, 4, 16, cutoff_top_k
1, 3, 16 and above V; orders 1, 2, 3, 5.

The conditions, with no exclusions (tests/test_ctc_ngram_f64.py asserts them; seeds and scales were
chosen on the CPU so that the restatement alone satisfies them): every utterance of every case is
decided by at least rnnt_lstm_search_f64.MARGIN in float64 and the float32 run of the restatement
returns the same tokens; in LM_CHANGES cases the n-gram changes a hypothesis against lm_weight = 0;
across the cases a look-up backs off 0, 1 and order - 1 times and reaches the dense root; in REENTER
cases a prefix that had left the beam is kept again next to one of its own extensions; extensions
land on live prefixes.

COST holds what float32 costs the RESTATEMENT (float32 on the CPU against float64) on exactly these
inputs, in the sense of yardstick.rel_err, the larger of score's and lm_score's; the GPU bounds are
max(2e-5, 8 x figure), the rule of tests/yardstick.py.
"""
import functools

import numpy as np
import torch

import ctc_ngram_f64 as G
from ctc_prefix_cases import lengths_of
from yardstick import FLOOR, MARGIN, bound_of, clamp, rel_err  # noqa: F401  (the rule of tests/yardstick.py)


def _c(seed, V, T, B, beam, topk, scale, order, lens="full", norm=False, n_tokens=300, lm_seed=0, weight=0.5,
       plant=3.0):
    return dict(seed=seed, V=V, T=T, B=B, beam=beam, topk=topk, scale=scale, order=order, lens=lens, norm=norm,
                n_tokens=n_tokens, lm_seed=lm_seed, weight=weight, plant=plant)


CASES = {
    "n_v3_o3_beam4_kV": _c(0, 3, 9, 1, 4, 5, 1.0, 3, n_tokens=60),          # cutoff_top_k above V
    "n_v11_o2_b17_beam4_k3": _c(2, 11, 13, 17, 4, 3, 2.0, 2, lens="ragged", n_tokens=120),
    "n_v63_o5_beam16_k16": _c(0, 63, 20, 2, 16, 16, 2.0, 5, lens="above"),
    "n_v65_o3_b33_beam4_k3_norm": _c(3, 65, 12, 33, 4, 3, 2.0, 3, lens="ragged", norm=True),
    "n_v128_o1_beam1_k1": _c(0, 128, 40, 3, 1, 1, 2.0, 1, lens="ragged"),
    "n_v11_o1_b2_beam4_k3": _c(0, 11, 13, 2, 4, 3, 2.0, 1, n_tokens=120, plant=0.0),
    "n_v128_o3_beam4_k4": _c(2, 128, 40, 2, 4, 4, 1.0, 3, weight=0.3),
    "n_v300_o3_beam4_k4": _c(0, 300, 10, 2, 4, 4, 2.0, 3, n_tokens=400),
    "n_v6_o3_reenter": _c(26, 6, 24, 1, 3, 3, 0.6, 3, n_tokens=100, weight=0.2, plant=0.0),
}
LM_CHANGES = ["n_v11_o2_b17_beam4_k3", "n_v65_o3_b33_beam4_k3_norm", "n_v63_o5_beam16_k16"]
REENTER = ["n_v6_o3_reenter"]
ORDER_ONE = ["n_v128_o1_beam1_k1", "n_v11_o1_b2_beam4_k3"]


def lm_sequences(V, n_tokens, seed):
    """Seeded synthetic token text: sentences of 12 tokens of a first-order source over the classes 1..V-1
    in which a class has three likely successors."""
    g = torch.Generator().manual_seed(7000 + seed)
    hi = max(V, 2)
    succ = torch.randint(1, hi, (V, 3), generator=g)
    draw = lambda: int(torch.randint(1, hi, (1,), generator=g))                   # noqa: E731
    seqs, cur, tok = [], [], draw()
    for _ in range(n_tokens):
        cur.append(tok)
        if len(cur) == 12:
            seqs.append(cur)
            cur, tok = [], draw()
        elif float(torch.rand((), generator=g)) < 0.8:
            tok = int(succ[tok, int(torch.randint(0, 3, (1,), generator=g))])
        else:
            tok = draw()
    return seqs + ([cur] if cur else [])


@functools.lru_cache(maxsize=None)
def lm_text(V, order, n_tokens, seed):
    """The ARPA text of a case's model (words are decimal class ids)."""
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.estimate(lm_sequences(V, n_tokens, seed), V, order=order).to_arpa()


def text_of(name):
    c = CASES[name]
    return lm_text(c["V"], c["order"], c["n_tokens"], c["lm_seed"])


@functools.lru_cache(maxsize=None)
def model(name):
    """The NgramLm of a case, read from its text (CPU tables; do not move: copy with from_arpa)."""
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.from_arpa(text_of(name), num_classes=CASES[name]["V"])


@functools.lru_cache(maxsize=None)
def dict_model(name, dtype):
    return G.DictNgram(text_of(name), CASES[name]["V"], dtype=dtype)


def make(name):
    """-> (logits (B,T,V) float32, NaN at and beyond lengths[b]; lengths (B))."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    x = c["scale"] * torch.randn(c["B"], c["T"], c["V"], generator=g)
    if c["plant"]:
        seqs = lm_sequences(c["V"], c["n_tokens"], c["lm_seed"])
        for b in range(c["B"]):
            s = seqs[b % len(seqs)]
            for t in range(c["T"]):
                x[b, t, s[(t // 2) % len(s)] if t % 2 == 0 else 0] += c["plant"]
    if c["norm"]:
        x = torch.log_softmax(x, dim=-1)
    lens = lengths_of(c)
    for b in range(c["B"]):
        x[b, clamp(lens[b], c["T"]):] = float("nan")
    return x, lens


def evaluate(name, dtype, lm_weight=None):
    """The restatement on a case in `dtype` -> per utterance a ctc_ngram_f64.Result."""
    c = CASES[name]
    x, lens = make(name)
    ng = dict_model(name, {torch.float64: np.float64, torch.float32: np.float32}[dtype])
    w = c["weight"] if lm_weight is None else lm_weight
    return [G.prefix_beam_search(x[b, :clamp(lens[b], c["T"])].to(dtype), c["beam"], c["topk"], ng, w)
            for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


@functools.lru_cache(maxsize=None)
def unfused(name):
    """The float64 results of a case at lm_weight = 0 (do not modify)."""
    return evaluate(name, torch.float64, lm_weight=0.0)


def fp32_figure(name):
    ref, f32 = reference(name), evaluate(name, torch.float32)
    f64 = lambda rows, i: torch.tensor([r[i] for r in rows], dtype=torch.float64)    # noqa: E731
    return max(rel_err(f64(f32, i), f64(ref, i)) for i in (1, 2))


def bound(name):
    """Allowed rel_err of the device's score and lm_score in case `name`."""
    return bound_of(COST[name])


# ------------------------------------------------------------------ the exhaustive cases
# (T, V, seeds, the model's order, lm_weight): beam 16 holds every reachable prefix, the search is exact
BRUTE = ((3, 3, 100, 3, 0.5), (5, 2, 100, 2, 0.5))


def brute_logits(T, V, n):
    g = torch.Generator().manual_seed(9100 + 10 * T + V)
    return 2.0 * torch.randn(n, T, V, generator=g)


def brute_text(V, order):
    return lm_text(V, order, 60, 1)


@functools.lru_cache(maxsize=None)
def brute_reference(T, V, n, order, weight):
    """Per seed ctc_ngram_f64.brute_force over all V^T alignments (do not modify)."""
    x = brute_logits(T, V, n)
    ng = G.DictNgram(brute_text(V, order), V)
    return [G.brute_force(x[i], ng, weight) for i in range(n)]


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figure(name), rounded up to two digits, the value itself behind.
COST = {
    "n_v3_o3_beam4_kV": 4.0e-08,              # 3.986e-08
    "n_v11_o2_b17_beam4_k3": 1.6e-07,         # 1.526e-07
    "n_v63_o5_beam16_k16": 8.6e-08,           # 8.542e-08
    "n_v65_o3_b33_beam4_k3_norm": 1.3e-07,    # 1.242e-07
    "n_v128_o1_beam1_k1": 8.7e-08,            # 8.601e-08
    "n_v11_o1_b2_beam4_k3": 4.3e-08,          # 4.281e-08
    "n_v128_o3_beam4_k4": 1.3e-07,           # 1.244e-07
    "n_v300_o3_beam4_k4": 7.1e-08,            # 7.065e-08
    "n_v6_o3_reenter": 9.9e-08,               # 9.851e-08
}
