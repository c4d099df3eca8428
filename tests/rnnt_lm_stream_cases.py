"""Seeded cases of the chunk-carried RNN-T beam search with RNN-LM shallow fusion (csrc/decode_lstm.hip
s2t_rnnt_beam_lstm_lm_chunk, s2t_rnnt_beam_stateless_lm_chunk), shared by
tests/test_rnnt_lm_stream_f64.py (CPU) and tests/test_gpu_rnnt_lm_stream.py (GPU).

Test infrastructure (not a test file).  Every case of tests/rnnt_lm_fusion_cases.py (LSTM predictor) and
tests/rnnt_stateless_lm_cases.py (stateless predictor), imported and not edited -- T 3..12, B up to 33
across the 16-row tile, beam 1 and 16, a start token, the out-projection, the YAML dimensions -- and six
longer ones by exactly those files' recipes (`make` / `evaluate` here ARE those modules' functions, run
with the case's entry visible to them):
    fs_h20_t40    s_h20_t40 of tests/rnnt_lstm_stream_cases.py (5 utterances of up to 40 frames, beam 3,
                  top-k 3) + lm20, LM seed 0, weight 0.5
    fs_h64o_t40   s_h64o_t40 (out-projection, beam 4, top-k 3) + lm64_v65, LM seed 0, weight 0.5
    fl_h20_t90    l_h20_t90 (90, 0 and 93 frames, beam 3, top-k 3) + lm20, LM seed 0, weight 0.5
    ss_t40        stateless, B 5, T 40, V 65, E 12, D 20, ctx 2, beam 4, top-k 3, lm48, seed 0
    ss_inner_t40  the same with top-k 4 and the out-projection: inner 24, oscale 4.0, blank 1.0
    sl_t90        stateless, B 3, T 90, V 63, E 12, D 20, ctx 5, beam 3, top-k 3, lm20, seed 0
The 90-frame rows are longer than one block of the staged trace-back (csrc/decode_records.h: 64 frames
of records per step).

tests/test_rnnt_lm_stream_f64.py asserts what the GPU file relies on, with no exclusions: in each of
the six, float64 decides every node of every utterance by at least 1e-3, float32 walks the same tokens
and frames, the LM changes at least two utterances against lm_weight = 0, the best beam of row 0 of a
90-frame case emits before frame 26 and after frame 64, and in every 40-frame case the common prefix
of the live beams is strictly between 0 and the best beam's length at a boundary of the 7-frame cut.
"""
import contextlib
import functools

import torch

import rnnt_lm_fusion_cases as L
import rnnt_lm_stream_f64 as F
import rnnt_lstm_search_cases as C
import rnnt_lstm_search_f64 as S
import rnnt_lstm_stream_cases as SC
import rnnt_stateless_lm_cases as SL
import rnnt_stateless_lm_f64 as SF

LSTM_STREAM = {
    "fs_h20_t40": L._f("s_h20_t40", "lm20", 0, 0.5, 3, 3),
    "fs_h64o_t40": L._f("s_h64o_t40", "lm64_v65", 0, 0.5, 4, 3),
}
LSTM_LONG = {"fl_h20_t90": L._f("l_h20_t90", "lm20", 0, 0.5, 3, 3)}
STATELESS_STREAM = {
    "ss_t40": SL._s(0, 5, 40, 65, 12, 20, 2, 4, 3, "lm48"),
    "ss_inner_t40": SL._s(0, 5, 40, 65, 12, 20, 2, 4, 4, "lm48", inner=24, oscale=4.0, blank=1.0),
}
STATELESS_LONG = {"sl_t90": SL._s(0, 3, 90, 63, 12, 20, 5, 3, 3, "lm20")}

LSTM_CASES = dict(L.CASES, **LSTM_STREAM, **LSTM_LONG)
STATELESS_CASES = dict(SL.CASES, **STATELESS_STREAM, **STATELESS_LONG)
CASES = dict(LSTM_CASES, **STATELESS_CASES)
STREAM_CASES = list(LSTM_STREAM) + list(STATELESS_STREAM)             # the four 40-frame cases
LONG_CASES = list(LSTM_LONG) + list(STATELESS_LONG)                   # the two 90-frame cases
NEW_CASES = STREAM_CASES + LONG_CASES
SHORT_CASES = list(L.CASES) + list(SL.CASES)
YAML_CASES = ["f_yaml", SL.YAML]
PARTITIONS = ("1", "7", "16", "irregular")
clamp = C.clamp


def is_lstm(name):
    return name in LSTM_CASES


@contextlib.contextmanager
def _visible(name):
    """The imported modules look a case up in their own CASES: a case of this module (and, for the LSTM
    family, its base case of rnnt_lstm_stream_cases) is there for the call only."""
    tables = [(L.CASES if is_lstm(name) else SL.CASES, name, CASES[name])]
    if is_lstm(name):
        base = CASES[name]["base"]
        tables.append((C.CASES, base, SC.CASES[base]))
    added = [(t, k) for t, k, _ in tables if k not in t]
    for t, k, v in tables:
        t.setdefault(k, v)
    try:
        yield
    finally:
        for t, k in added:
            del t[k]


def settings(name):
    """-> (beam, top-k, lm_weight, start token or None, T)."""
    c = CASES[name]
    T = SC.CASES[c["base"]]["T"] if is_lstm(name) else c["T"]
    return c["beam"], c["topk"], c["weight"], c["start"], T


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (predictor / joiner weights, act, am (B,T,V), lengths (B), LM state dict; float32, do not modify).
    LSTM family: the weights of rnnt_lstm_search_f64; stateless: those of rnnt_stateless_lm_f64."""
    with _visible(name):
        if is_lstm(name):
            return L.make(name)
        p, am, lens, sd = SL.make(name)
        return p, CASES[name]["act"], am, lens, sd


def lengths(name):
    """The frames each utterance of a case has, clamped to [0, T]."""
    am, lens = make(name)[2:4]
    return [clamp(n, am.shape[1]) for n in lens]


def evaluate(name, dtype, lm_weight=None):
    """The whole-utterance restatement -> per utterance (tokens, score, lm_score, frames, margin)."""
    with _visible(name):
        return (L if is_lstm(name) else SL).evaluate(name, dtype, lm_weight)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    if name in L.CASES:
        return L.reference(name)
    if name in SL.CASES:
        return SL.reference(name)
    return evaluate(name, torch.float64)


def hooks(name, dtype):
    """-> (the predictor's hooks of rnnt_lm_stream_f64, the LM state dict) in `dtype`."""
    w, act, _, _, sd = make(name)
    sd = L.cast(sd, dtype)
    if is_lstm(name):
        return F.lstm_hooks(S.cast(w, dtype), act), sd
    return F.stateless_hooks(SF.cast(w, dtype), CASES[name]["ctx"], act), sd


@functools.lru_cache(maxsize=None)
def chunked(name, b, how):
    """rnnt_lm_stream_f64.chunked in float64 on utterance b cut by `how` (do not modify)."""
    beam, topk, weight, start, _ = settings(name)
    n = lengths(name)[b]
    h, sd = hooks(name, torch.float64)
    return F.chunked(make(name)[2][b, :n], F.cuts_of(n, how, seed=b), h, beam, topk, sd, weight, start)
