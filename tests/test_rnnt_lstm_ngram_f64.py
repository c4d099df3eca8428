"""CPU: the yardstick of the lockstep RNN-T beam search of the LSTM predictor fused with a back-off n-gram
(csrc/decode_lstm.hip s2t_rnnt_beam_lstm_ngram, s2t_rnnt_beam_lstm_ngram_chunk).

tests/rnnt_lstm_ngram_f64.py is pinned against what exists: the exhaustive arg-max over all V^T frame
labellings plus the LM term on the tiny lattices of rnnt_ngram_cases.BRUTE's sizes; with lm_weight = 0 the
plain restatement tests/rnnt_lstm_search_f64.py; chunked under any partition equals whole, after every
piece.  Then the conditions every case of tests/rnnt_lstm_ngram_cases.py must meet, with no exclusions
(margins, float32 on the same path, the LM changes a hypothesis, every back-off depth and the dense
root) and the recorded float32 costs to a factor 4.
"""
import pytest
import torch

import ctc_ngram_f64 as G
import rnnt_lstm_ngram_cases as C
import rnnt_lstm_ngram_f64 as R
import rnnt_lstm_search_f64 as S
import rnnt_ngram_cases as SN


# ------------------------------------------------------------------ 1. the restatement itself
def test_brute_sizes_are_the_stateless_family_s():
    assert C.BRUTE == SN.BRUTE


@pytest.mark.parametrize("V,T,n,order,weight", C.BRUTE)
def test_restatement_is_the_exhaustive_arg_max(V, T, n, order, weight):
    w, am = C.brute_inputs(V, T, n)
    ng = G.DictNgram(C.brute_text(V, order), V)
    assert n >= 100 and ng.order == order
    changed = 0
    for i, (tokens, frames, total, lms, gap) in enumerate(C.brute_reference(V, T, n, order, weight)):
        r = R.beam_search(am[i], w, C.BRUTE_MODEL["act"], 16, V, ng, weight)
        assert gap >= C.MARGIN, (i, gap)                   # (what lets a float32 search be held to it)
        assert (r.tokens, r.frames) == (tokens, frames), (V, T, i)
        assert r.score == pytest.approx(total, abs=1e-9) and r.lm_score == pytest.approx(lms, abs=1e-9)
        changed += tokens != S.beam_search(am[i], S.cast(w, torch.float64), C.BRUTE_MODEL["act"], 16, V)[0]
    assert changed > 0, "the LM term decides nothing on these inputs"


@pytest.mark.parametrize("name", list(C.CASES))
def test_weight_zero_is_the_plain_restatement(name):
    c = C.CASES[name]
    w, act, am, _ = C.make(name)
    w64 = S.cast(w, torch.float64)
    for b, (r, n) in enumerate(zip(C.unfused(name), C.lengths(name))):
        if n == 0:
            assert (r.tokens, r.score, r.lm_score) == ([], 0.0, 0.0)
            continue
        tokens, score, frames, _ = S.beam_search(am[b, :n], w64, act, c["beam"], c["topk"])
        assert (r.tokens, r.frames, r.score) == (tokens, frames, score), (name, b)


@pytest.mark.parametrize("how", C.PARTITIONS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_chunked_equals_whole_after_every_piece(name, how):
    c = C.CASES[name]
    w, act, am, _ = C.make(name)
    ng = C.dict_model(name, torch.float64)
    for b, (ref, n) in enumerate(zip(C.reference(name), C.lengths(name))):
        if b > 2 and b % 5:                                # (a fifth of a large batch: the restatement per row)
            continue
        whole, after, stable = C.chunked(name, b, how)
        cuts = C.cuts_of(name, b, how)
        assert len(after) == len(stable) == len(cuts) - 1
        assert whole[:4] == ref[:4], (name, how, b)
        for k, (cut, r) in enumerate(zip(cuts[1:], after)):
            if k % 4 and cut != n:                         # the whole restatement on a prefix: every fourth piece
                continue
            p = R.beam_search(am[b, :cut], w, act, c["beam"], c["topk"], ng, c["weight"])
            assert r[:4] == p[:4], (name, how, b, cut)
        assert all(x <= y for x, y in zip(stable, stable[1:]))


# ------------------------------------------------------------------ 2. the conditions on the cases
@pytest.mark.parametrize("name", list(C.CASES))
def test_every_utterance_of_the_case_is_decided(name):
    ref, f32 = C.reference(name), C.reference32(name)
    print(f"{name}: smallest float64 margin {min(r.margin for r in ref):.3e}, back-offs "
          f"{sorted(set().union(*[r.hops for r in ref]))}")
    for b, (r, s) in enumerate(zip(ref, f32)):
        assert r.margin >= C.MARGIN, (name, b, r.margin)
        assert (r.tokens, r.frames) == (s.tokens, s.frames), (name, b)


def test_cases_cover_what_the_issue_names():
    cs = C.CASES.values()
    assert {11, 63, 65} == {c["m"]["V"] for c in cs} and {20} == {c["m"]["H"] for c in cs}
    assert {1, 2} == {c["m"]["L"] for c in cs} and {0, 24} == {c["m"]["inner"] for c in cs}
    assert {1, 3, 17} <= {c["B"] for c in cs} and {1, 4, 16} <= {c["beam"] for c in cs}
    assert {1, 3} <= {c["topk"] for c in cs} and any(c["topk"] > c["m"]["V"] for c in cs)
    assert sorted(c["T"] for c in cs)[-2:] == [40, 90] and C.CASES[C.LONG]["T"] == 90
    assert C.PARTITIONS == ("1", "7", "16", "irregular")
    assert any(0 in C.lengths(n) for n in C.CASES) and any(int(C.make(n)[3].max()) > C.CASES[n]["T"] for n in C.CASES)
    for name in C.LM_CHANGES:
        assert any(a.tokens != b.tokens for a, b in zip(C.reference(name), C.unfused(name))), name
    hops = {name: set().union(*[r.hops for r in C.reference(name)]) for name in C.CASES}
    assert any({0, 1, C.CASES[n]["order"] - 1} <= h and C.CASES[n]["order"] >= 3 for n, h in hops.items())
    assert any(r.root for n in C.CASES for r in C.reference(n))
    assert any(a != b for b in range(2) for a, b in [(C.cuts_of(C.LONG, b, "irregular"), C.cuts_of(C.LONG, b, "16"))])
    c = C.cuts_of(C.LONG, 0, "irregular")
    assert any(x == y for x, y in zip(c, c[1:]))           # idle calls


@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_cost_of_the_scores(name):
    fig = C.fp32_figure(name)
    print(f"fp32 cost of score / lm_score, {name}: {fig:.3e}")
    rec = C.COST[name]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)
    assert C.bound(name) == max(C.FLOOR, C.COST_MARGIN * rec)
