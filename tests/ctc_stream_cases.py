"""Seeded cases shared by tests/test_ctc_stream_f64.py (CPU) and tests/test_gpu_ctc_stream.py (GPU): the
chunk-carried CTC prefix beam search of csrc/decode_ctc.hip, plain and with RNN-LM shallow fusion.

Test infrastructure (not a test file).  Every case of tests/ctc_prefix_cases.py, plus longer
blank-biased ones (`bias` is added to the blank's logit: most frames stay, so the live prefixes share
a long prefix and the unstable region is a few tokens, as in speech), each under four cuts of its
frames into calls:

    one     one frame a call
    r4, r7  regular chunks of 4 and 7 frames (the last one short; a row that ended idles)
    ragged  a different sequence of chunk sizes per row, with idle calls (size 0) in between; rows
            end at different calls, and the ragged-length cases' rows of length 0 never start

A call is (Tc, chunk_len (B)), row b's frames the next chunk_len[b] of its utterance; frames of the
chunk tensor at and beyond chunk_len[b] are NaN.  Each case has a `max_nodes`: the whole-utterance
bound 1 + T * beam_size, except in the COMPACTS cases, where it lies BELOW the number of sequences some
utterance ever keeps and at or above what every call of every cut needs (kept + beam_size * n): a run
of such a case without overflow proves that compaction happened and was exact
(tests/test_ctc_stream_f64.py asserts the inequality; the figures were measured with the restatement
on the CPU).
"""
import functools

import torch

import ctc_prefix_cases as C
import ctc_prefix_f64 as P
import ctc_stream_f64 as S
import rnnt_lm_fusion_cases as L

CUTS = ("one", "r4", "r7", "ragged")
RAGGED = (3, 0, 1, 5, 0, 2, 7, 1)          # chunk sizes a row cycles through, row b starting at entry b


def _s(seed, V, T, B, beam, topk, scale, bias, lens="full"):
    return dict(C._c(seed, V, T, B, beam, topk, scale, lens=lens), bias=bias)


NEW = {
    "s_v11_t60_beam4_blank": _s(0, 11, 60, 1, 4, 4, 2.0, 2.0),
    "s_v29_t90_b3_beam4_blank": _s(4, 29, 90, 3, 4, 4, 2.0, 2.0, lens="ragged"),
    "s_v13_t70_b2_beam8_k5_blank": _s(2, 13, 70, 2, 8, 5, 2.0, 1.5),
}
CASES = {**{k: dict(v, bias=0.0) for k, v in C.CASES.items()}, **NEW}
PLAIN_CASES = [k for k, v in CASES.items() if v["lm"] is None]
LM_CASES = [k for k, v in CASES.items() if v["lm"] is not None]
REENTER = C.REENTER

# max_nodes below the sequences ever kept (see the module docstring); every other case: 1 + T * beam
MAX_NODES = {                               # largest need over the four cuts / most sequences ever kept by a row
    "p_v6_reenter": 32,                     # 31 / 43
    "p_v5_reenter": 22,                     # 21 / 30
    "p_v63_beam16_k16": 240,                # 232 / 321
    "p_v128_beam4_k4": 140,                 # 136 / 161
    "s_v11_t60_beam4_blank": 120,           # 110 / 175
    "s_v29_t90_b3_beam4_blank": 200,        # 184 / 277
    "s_v13_t70_b2_beam8_k5_blank": 300,     # 291 / 370
}
COMPACTS = list(MAX_NODES)


def max_nodes(name):
    c = CASES[name]
    return MAX_NODES.get(name, 1 + c["T"] * c["beam"])


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (logits (B,T,V) float32, NaN at and beyond lengths[b]; lengths (B); LM state dict or None).
    Shared: do not modify."""
    if name in C.CASES:
        return C.make(name)
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    x = c["scale"] * torch.randn(c["B"], c["T"], c["V"], generator=g)
    x[..., 0] += c["bias"]
    lens = C.lengths_of(c)
    for b in range(c["B"]):
        x[b, C.clamp(lens[b], c["T"]):] = float("nan")
    return x, lens, None


def calls(name, cut):
    """-> [(Tc, [n_0, .., n_{B-1}])]: the calls of a cut, n_b frames of row b in that call."""
    c = CASES[name]
    left = [C.clamp(n, c["T"]) for n in make(name)[1]]
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


def chunks(name, cut):
    """-> [(chunk (B,Tc,V) float32 with NaN beyond chunk_len, chunk_len (B) int64, fed (B) frames fed
    after the call)] for the calls of a cut."""
    x, _, _ = make(name)
    B, _, V = x.shape
    pos, out = [0] * B, []
    for Tc, ns in calls(name, cut):
        ch = torch.full((B, Tc, V), float("nan"))
        for b, n in enumerate(ns):
            ch[b, :n] = x[b, pos[b]:pos[b] + n]
            pos[b] += n
        out.append((ch, torch.tensor(ns, dtype=torch.int64), list(pos)))
    return out


@functools.lru_cache(maxsize=None)
def stream_reports(name, cut, limit=None, lm_weight=None):
    """The float64 restatement fed the calls of a cut -> per call, per row, a ctc_stream_f64.Report
    (computed once per process and shared: do not modify).  limit: max_nodes (None: unbounded)."""
    c = CASES[name]
    x, _, sd = make(name)
    if sd is not None:
        sd = L.cast(sd, torch.float64)
    w = c["weight"] if lm_weight is None else lm_weight
    streams = [S.Stream(c["beam"], c["topk"], 0, sd, w, c["start"], torch.float64, limit) for _ in range(c["B"])]
    pos, out = [0] * c["B"], []
    for _, ns in calls(name, cut):
        reps = []
        for b, n in enumerate(ns):
            reps.append(streams[b].feed(x[b, pos[b]:pos[b] + n].double()))
            pos[b] += n
        out.append(reps)
    return out


def whole(name, dtype, lm_weight=None):
    """ctc_prefix_f64.prefix_beam_search on the whole utterances of a case in `dtype`."""
    c = CASES[name]
    x, lens, sd = make(name)
    if sd is not None:
        sd = L.cast(sd, dtype)
    w = c["weight"] if lm_weight is None else lm_weight
    return [P.prefix_beam_search(x[b, :C.clamp(lens[b], c["T"])].to(dtype), c["beam"], c["topk"], 0, sd, w, c["start"])
            for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 whole-utterance results of a case (shared: do not modify)."""
    return C.reference(name) if name in C.CASES else whole(name, torch.float64)


def need(name, cut):
    """-> (the largest kept + beam * n any call of the cut asks of any row, per row the sequences ever
    kept at the end), by the unbounded restatement."""
    c = CASES[name]
    reps, cl = stream_reports(name, cut), calls(name, cut)
    most, kept = 0, [1] * c["B"]
    for (_, ns), row in zip(cl, reps):
        for b, n in enumerate(ns):
            if n > 0:
                most = max(most, kept[b] + c["beam"] * n)
            kept[b] = row[b].kept
    return most, [r.ever for r in reps[-1]]
