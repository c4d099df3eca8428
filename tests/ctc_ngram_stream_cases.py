"""Seeded cases shared by tests/test_ctc_ngram_stream_f64.py (CPU) and tests/test_gpu_ctc_ngram_stream.py (GPU):
the chunk-carried CTC prefix beam search fused with a back-off n-gram (csrc/decode_ctc.hip
s2t_ctc_prefix_beam_ngram_chunk).

Test infrastructure (not a test file).  The inputs are tests/ctc_ngram_cases.py's, unchanged (ARPA text,
logits, lengths, weights: V 3, 11, 63, 65, 128, 300; B 1, 17, 33; beams 1, 4, 16; cutoff_top_k 1, 3, 16 and
above V; orders 1, 2, 3, 5; T <= 40), each under the four cuts of tests/ctc_stream_cases.CUTS: one frame a
call, regular chunks of 4 and 7, and ragged (a different sequence of chunk sizes per row with idle calls
in between).  A call is (Tc, chunk_len (B)); frames of the chunk tensor at and beyond chunk_len[b] are
NaN.

Each case has a `max_nodes`: the whole-utterance bound 1 + T * beam_size, except in the COMPACTS cases,
where it lies BELOW the number of sequences some utterance ever keeps and at or above what every call of
every cut needs (kept + beam_size * n): a run of such a case without overflow proves that compaction
happened and was exact (tests/test_ctc_ngram_stream_f64.py asserts the inequalities; the figures were
measured with the restatement on the CPU).

The float32 cost of score and lm_score is ctc_ngram_cases.COST: the inputs are the same and a cut changes
no arithmetic (tests/test_ctc_ngram_stream_f64.py holds the float32 stream to that table).  The GPU test
needs no bound of its own for the chunk entry: its yardstick is the one-shot entry, bit for bit.
"""
import functools

import numpy as np
import torch

import ctc_ngram_cases as G
import ctc_ngram_stream_f64 as S
from ctc_stream_cases import CUTS, RAGGED  # noqa: F401  (CUTS: the tests parametrise over it)
from yardstick import clamp

CASES = G.CASES
LM_CHANGES, REENTER = G.LM_CHANGES, G.REENTER
COST = G.COST

# max_nodes below the sequences ever kept (see the module docstring); every other case: 1 + T * beam
MAX_NODES = {                               # largest need over the four cuts / most sequences ever kept by a row
    "n_v63_o5_beam16_k16": 200,             # 193 / 220
    "n_v65_o3_b33_beam4_k3_norm": 38,       # 36 / 45
    "n_v128_o1_beam1_k1": 8,                # 8 / 37
    "n_v128_o3_beam4_k4": 60,               # 55 / 97
    "n_v6_o3_reenter": 26,                  # 25 / 32
}
COMPACTS = list(MAX_NODES)


def max_nodes(name):
    c = CASES[name]
    return MAX_NODES.get(name, 1 + c["T"] * c["beam"])


def calls(name, cut):
    """-> [(Tc, [n_0, .., n_{B-1}])]: the calls of a cut, n_b frames of row b in that call."""
    c = CASES[name]
    left = [clamp(n, c["T"]) for n in G.make(name)[1]]
    out, k = [], 0
    while any(left) or not out:
        if cut == "ragged":
            want = [RAGGED[(b + k) % len(RAGGED)] for b in range(c["B"])]
        else:
            want = [{"one": 1, "r4": 4, "r7": 7}[cut]] * c["B"]
        ns = [min(w, n) for w, n in zip(want, left)]
        left = [n - m for n, m in zip(left, ns)]
        out.append((max(1, max(want)), ns))
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def chunks(name, cut):
    """-> [(chunk (B,Tc,V) float32 with NaN beyond chunk_len, chunk_len (B) int64, fed (B) frames fed
    after the call)] for the calls of a cut.  Shared: do not modify."""
    x, _ = G.make(name)
    B, _, V = x.shape
    pos, out = [0] * B, []
    for Tc, ns in calls(name, cut):
        ch = torch.full((B, Tc, V), float("nan"))
        for b, n in enumerate(ns):
            ch[b, :n] = x[b, pos[b]:pos[b] + n]
            pos[b] += n
        out.append((ch, torch.tensor(ns, dtype=torch.int64), list(pos)))
    return out


def streams(name, dtype=torch.float64, limit=None, lm_weight=None):
    c = CASES[name]
    ng = G.dict_model(name, {torch.float64: np.float64, torch.float32: np.float32}[dtype])
    w = c["weight"] if lm_weight is None else lm_weight
    return [S.Stream(c["beam"], c["topk"], ng, w, 0, dtype, limit) for _ in range(c["B"])]


def run(name, cut, dtype=torch.float64, limit=None, lm_weight=None):
    """The restatement fed the calls of a cut -> (per call, per row, a ctc_stream_f64.Report; the streams)."""
    x, _ = G.make(name)
    st = streams(name, dtype, limit, lm_weight)
    pos, out = [0] * len(st), []
    for _, ns in calls(name, cut):
        reps = []
        for b, n in enumerate(ns):
            reps.append(st[b].feed(x[b, pos[b]:pos[b] + n].to(dtype)))
            pos[b] += n
        out.append(reps)
    return out, st


@functools.lru_cache(maxsize=None)
def stream_reports(name, cut, limit=None, lm_weight=None):
    """The float64 reports of run() (computed once per process and shared: do not modify)."""
    return run(name, cut, torch.float64, limit, lm_weight)[0]


def row_needs(name, cut):
    """Per row the largest kept + beam * n of its calls, by the unbounded restatement."""
    c = CASES[name]
    kept, most = [1] * c["B"], [0] * c["B"]
    for (_, ns), row in zip(calls(name, cut), stream_reports(name, cut)):
        for b, n in enumerate(ns):
            if n:
                most[b] = max(most[b], kept[b] + c["beam"] * n)
            kept[b] = row[b].kept
    return most


def need(name, cut):
    """-> (the largest kept + beam * n any call of the cut asks of any row, per row the sequences ever
    kept at the end)."""
    return max(row_needs(name, cut)), [r.ever for r in stream_reports(name, cut)[-1]]
