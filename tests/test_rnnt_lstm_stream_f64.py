"""CPU: the chunked float64 restatement of tests/rnnt_lstm_stream_f64.py is the whole-utterance
restatement of tests/rnnt_lstm_search_f64.py however the frames are cut, and the two longer beam
cases and the two 90-frame cases of tests/rnnt_lstm_stream_cases.py are what the GPU file takes them
for."""
import pytest
import torch

import rnnt_lstm_search_f64 as S
import rnnt_lstm_stream_cases as SC
import rnnt_lstm_stream_f64 as F

PARTITIONS = ("1", "7", "16", "irregular")


def _utterances(name):
    w, act, am, lens = SC.make(name)
    c = SC.CASES[name]
    return c, S.cast(w, torch.float64), act, [am[b, :SC.clamp(lens[b], c["T"])] for b in range(c["B"])]


def _some(name, utts):
    """The wide batches repeat one model over many short utterances: five of them say the same."""
    return list(enumerate(utts))[:5] if len(utts) > 5 else list(enumerate(utts))


@pytest.mark.parametrize("name", list(SC.BEAM_CASES))
def test_chunked_beam_restatement_is_the_whole_utterance_one(name):
    c, w, act, utts = _utterances(name)
    ref = SC.reference(name)
    for b, a in _some(name, utts):
        tok, score, frm, _ = ref[b]
        for how in PARTITIONS:
            got = F.beam_search_chunked(a, F.cuts_of(len(a), how, b), w, act, c["beam"], c["topk"])
            assert got[0] == tok and got[2] == frm, (name, b, how)
            assert abs(got[1] - score) <= 1e-12, (name, b, how, got[1], score)
            assert len(got[4]) == len(F.cuts_of(len(a), how, b)) - 1
            assert got[4] == sorted(got[4]) and (not got[4] or got[4][-1] <= len(tok)), (name, b, how)


@pytest.mark.parametrize("name", list(SC.GREEDY_CASES))
def test_chunked_greedy_restatement_is_the_whole_utterance_one(name):
    c, w, act, utts = _utterances(name)
    ref = SC.reference(name)
    for b, a in _some(name, utts):
        for how in PARTITIONS:
            got = F.greedy_chunked(a, F.cuts_of(len(a), how, b), w, act, c["mts"])
            assert got[0] == ref[b][0] and got[2] == ref[b][2], (name, b, how)
            assert got[3] == sorted(got[3]) and (not got[3] or got[3][-1] == len(ref[b][0]))


@pytest.mark.parametrize("name", list(SC.STREAM_CASES))
def test_the_longer_cases_are_decided_and_not_trivial(name):
    """Margin >= 1e-3 on every utterance; the float32 evaluation keeps the token sequences of ALL
    live beams at every frame; 0 < stable < out_len at some chunk boundary of the 7-frame partition;
    a zero-length and a clamped row."""
    c, w, act, utts = _utterances(name)
    ref = SC.reference(name)
    lens = SC.make(name)[3].tolist()
    assert [len(a) for a in utts][:3] == [40, 0, 40] and lens[2] == 43
    assert ref[1][0] == [] and ref[1][1] == 0.0
    w32 = S.cast(w, torch.float32)
    between = frames = boundaries = 0
    for b, a in enumerate(utts):
        assert ref[b][3] >= S.MARGIN, (name, b, ref[b][3])
        hist = {}
        for key, ww in (("f64", w), ("f32", w32)):
            seen = hist[key] = []
            F.beam_search_chunked(a, F.cuts_of(len(a), "1"), ww, act, c["beam"], c["topk"],
                                  every=lambda beams: seen.append([x[0] for x in beams]))
        assert hist["f32"] == hist["f64"], (name, b)
        frames += len(a)
        between += sum(0 < F.common_prefix_len(h) < len(h[0]) for h in hist["f64"])
        best7 = []
        got = F.beam_search_chunked(a, F.cuts_of(len(a), "7"), w, act, c["beam"], c["topk"],
                                    every=lambda beams: best7.append(len(beams[0][0])))
        boundaries += sum(0 < s < n for s, n in zip(got[4], best7))
    print(f"{name}: 0 < common prefix < best length on {between} of {frames} frames")
    assert between > frames // 4 and boundaries > 0


@pytest.mark.parametrize("name", list(SC.LONG_CASES))
def test_the_long_cases_cross_the_trace_blocks(name):
    """Rows of 90, 0 and 90 (93 clamped) frames; margin >= 1e-3 on every utterance; float32 gives
    float64's tokens and frames; the best beam of row 0 has a token at a frame < 26 and one at a
    frame >= 64, the edges of the 64-frame blocks a 90-frame trace-back is staged in."""
    c = SC.CASES[name]
    lens = SC.make(name)[3].tolist()
    assert SC.lengths(name) == [90, 0, 90] and lens[2] == 93
    ref, f32 = SC.reference(name), SC.evaluate(name, torch.float32)
    for b, (r, q) in enumerate(zip(ref, f32)):
        print(f"{name} row {b}: {len(r[0])} tokens, first frame {r[2][:1]}, margin {r[3]:.2e}")
        assert r[3] >= S.MARGIN, (name, b, r[3])
        assert q[0] == r[0] and q[2] == r[2], (name, b)
    assert ref[1][0] == [] and ref[1][1] == 0.0
    frames = ref[0][2]
    assert min(frames) < 26 and max(frames) >= 64, (name, frames)
