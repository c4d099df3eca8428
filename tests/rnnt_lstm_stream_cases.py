"""Seeded cases of the chunk-carried LSTM-predictor RNN-T search (csrc/decode_lstm.hip,
s2t_rnnt_*_lstm_chunk), shared by tests/test_rnnt_lstm_stream_f64.py (CPU) and
tests/test_gpu_rnnt_lstm_stream.py (GPU).

Test infrastructure (not a test file).  The cases of tests/rnnt_lstm_search_cases.py (imported, not
edited) and two longer beam cases by exactly its recipe -- `make`, `evaluate` and `reference` here
ARE that module's functions, run with the case's entry visible to them:
    s_h64o_t40  h64o, 5 utterances of up to 40 frames, beam 4, top-k 3
    s_h20_t40   h20, the same lengths, beam 3, top-k 3
Their lengths are 40, 0, 43 (clamped to 40) and two ragged ones: a zero-length row and a clamped
row.  tests/test_rnnt_lstm_stream_f64.py asserts what the GPU file relies on: float64 decides every
node of every utterance by at least 1e-3, float32 keeps the token sequences of ALL live beams at
every frame, and the common prefix of the live beams is strictly between 0 and the best beam's
length at chunk boundaries of the 7-frame partition, so `stable_len` is neither trivially 0 nor
out_len.

LONG_CASES are longer than one block of the staged trace-back (csrc/decode_records.h: 64 frames of
records per step), which no case above is:
    l_h20_t90   h20, 3 utterances of 90, 0 and 93 (clamped to 90) frames, beam 3, top-k 3
    l_h64o_t90  h64o, the same lengths, beam 4, top-k 3
A 90-frame row is walked back in the blocks [26, 90) and [0, 26).  tests/test_rnnt_lstm_stream_f64.py
asserts the margin, that float32 gives float64's tokens and frames, and that the best beam of row 0
emits on both sides of both block edges (a frame < 26 and a frame >= 64).  They are in CASES only:
the parametrised tests over BEAM_CASES do not grow by them.
"""
import contextlib
import functools

import torch

import rnnt_lstm_search_cases as C

STREAM_CASES = {
    "s_h64o_t40": C._c("h64o", 21, 5, 40, beam=4, topk=3, blank=1.3),
    "s_h20_t40": C._c("h20", 22, 5, 40, beam=3, topk=3),
}
LONG_CASES = {
    "l_h20_t90": C._c("h20", 43, 3, 90, beam=3, topk=3),
    "l_h64o_t90": C._c("h64o", 40, 3, 90, beam=4, topk=3),
}
GREEDY_CASES, BEAM_CASES = C.GREEDY_CASES, dict(C.BEAM_CASES, **STREAM_CASES)
CASES = dict(C.CASES, **STREAM_CASES, **LONG_CASES)
MODELS, clamp = C.MODELS, C.clamp


@contextlib.contextmanager
def _visible(name):
    """C.make / C.evaluate look a case up in C.CASES: a case of this module is there for the call only."""
    added = name not in C.CASES
    if added:
        C.CASES[name] = CASES[name]
    try:
        yield
    finally:
        if added:
            del C.CASES[name]


def make(name):
    with _visible(name):
        return C.make(name)


def evaluate(name, dtype):
    with _visible(name):
        return C.evaluate(name, dtype)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return C.reference(name) if name in C.CASES else evaluate(name, torch.float64)


def lengths(name):
    """The frames each utterance of a case has, clamped to [0, T]."""
    return [clamp(n, CASES[name]["T"]) for n in make(name)[3]]
