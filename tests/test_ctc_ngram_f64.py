"""CPU: the yardstick of the CTC prefix beam search fused with a back-off n-gram (csrc/decode_ctc.hip
s2t_ctc_prefix_beam_ngram) and the host loop around it.

tests/ctc_ngram_f64.py is pinned against the exhaustive sum over all V^T alignments plus lm_weight x the dict
n-gram's score of the labelling, where the beam holds every reachable prefix.  Then the conditions every
case of tests/ctc_ngram_cases.py must meet, with no exclusions (margins, float32 on the same path, the LM
changes a hypothesis, every back-off depth, re-entries, merges), the recorded float32 costs to a
factor 4, and CtcPrefixBeamDecoding._module_loop with an NgramLm against the restatement.
"""
import numpy as np
import pytest
import torch

import ctc_ngram_cases as C
import ctc_ngram_f64 as G
import ctc_prefix_f64 as P
from rnnt_lstm_search_f64 import MARGIN
from yardstick import _Ids


# ------------------------------------------------------------------ 1. the restatement itself
@pytest.mark.parametrize("T,V,n,order,weight", C.BRUTE)
def test_restatement_is_the_exhaustive_sum_plus_the_lm_term(T, V, n, order, weight):
    x = C.brute_logits(T, V, n).double()
    ng = G.DictNgram(C.brute_text(V, order), V)
    assert n >= 100 and ng.order == order
    changed = 0
    for i, (labels, logp, lm, gap) in enumerate(C.brute_reference(T, V, n, order, weight)):
        r = G.prefix_beam_search(x[i], 16, V, ng, weight)
        assert gap >= MARGIN, (i, gap)                     # (what lets a float32 search be held to it)
        assert r.tokens == labels, (T, V, i)
        assert r.score == pytest.approx(logp, abs=1e-9) and r.lm_score == pytest.approx(lm, abs=1e-9)
        changed += labels != P.prefix_beam_search(x[i], 16, V).tokens
    if V > 2:                                              # (with one non-blank class the LM only weighs lengths)
        assert changed > 0, "the LM term decides nothing on these inputs"


def test_weight_zero_is_the_plain_restatement_and_lm_score_is_the_sentence_score():
    name = "n_v65_o3_b33_beam4_k3_norm"
    c = C.CASES[name]
    x, lens = C.make(name)
    ng = C.dict_model(name, np.float64)
    for b, r in enumerate(C.unfused(name)):
        plain = P.prefix_beam_search(x[b, :C.clamp(lens[b], c["T"])].double(), c["beam"], c["topk"])
        assert r.tokens == plain.tokens and r.score == plain.score
    for r in C.reference(name):
        assert r.lm_score == pytest.approx(float(ng.sentence(tuple(r.tokens))), abs=1e-9)


@pytest.mark.parametrize("name", C.ORDER_ONE)
def test_order_one_is_a_constant_row(name):
    """An order-1 model has no context: one q row for every prefix, the first token included."""
    ng = C.dict_model(name, np.float64)
    assert ng.order == 1 and not ng.contexts
    for r in C.reference(name):
        assert r.lm_score == pytest.approx(sum(float(ng.probs[(t,)]) for t in r.tokens), abs=1e-9)
        assert r.hops <= {0}


# ------------------------------------------------------------------ 2. the conditions on the cases
@pytest.mark.parametrize("name", list(C.CASES))
def test_every_utterance_of_the_case_is_decided(name):
    ref, f32 = C.reference(name), C.evaluate(name, torch.float32)
    print(f"{name}: smallest float64 margin {min(r.margin for r in ref):.3e}, merged "
          f"{sum(r.merged for r in ref)}, re-entered {sum(r.reentered for r in ref)}, back-offs "
          f"{sorted(set().union(*[r.hops for r in ref]))}")
    for b, (r, s) in enumerate(zip(ref, f32)):
        assert r.margin >= MARGIN, (name, b, r.margin)
        assert r.tokens == s.tokens, (name, b)
    assert min(r.margin for r in C.unfused(name)) >= MARGIN, name
    x, lens = C.make(name)
    for b in range(x.shape[0]):                            # NaN exactly at and beyond the length
        n = C.clamp(lens[b], x.shape[1])
        assert bool(torch.isfinite(x[b, :n]).all()) and bool(torch.isnan(x[b, n:]).all())


def test_cases_cover_what_the_issue_names():
    cs = C.CASES.values()
    assert {3, 11, 63, 65, 128} <= {c["V"] for c in cs} and any(c["V"] > 256 for c in cs)
    assert {1, 17, 33} <= {c["B"] for c in cs} and {1, 4, 16} <= {c["beam"] for c in cs}
    assert {1, 3, 16} <= {c["topk"] for c in cs} and any(c["topk"] > c["V"] for c in cs)
    assert {1, 2, 3, 5} <= {c["order"] for c in cs} and max(c["T"] for c in cs) == 40
    lens = torch.cat([C.lengths_of(c) - c["T"] for c in cs])
    assert bool((lens == 0).any()) and bool((lens > 0).any()) and bool((lens < 0).any())
    assert any(int(n) == 0 for c in cs for n in C.lengths_of(c))
    for name in C.LM_CHANGES:
        assert any(a.tokens != b.tokens for a, b in zip(C.reference(name), C.unfused(name))), name
    hops = {name: set().union(*[r.hops for r in C.reference(name)]) for name in C.CASES}
    assert any({0, 1, C.CASES[name]["order"] - 1} <= h and C.CASES[name]["order"] >= 3 for name, h in hops.items())
    deep = "n_v63_o5_beam16_k16"
    assert {0, 1, 2, 3, 4} <= hops[deep] and any(r.root for r in C.reference(deep))
    assert sum(r.merged for name in C.CASES for r in C.reference(name)) > 0
    for name in C.REENTER:
        assert sum(r.reentered for r in C.reference(name)) > 0, name
    for name in C.CASES:                                   # sparse tables: a context lists few of the classes
        m = C.model(name)
        assert m.order == C.CASES[name]["order"]
        if m.order > 1 and m.num_classes >= 63:
            assert m.num_arcs < 0.1 * m.num_ctx * m.num_classes, name


@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_cost_of_the_scores(name):
    fig = C.fp32_figure(name)
    print(f"fp32 cost of score / lm_score, {name}: {fig:.3e}")
    rec = C.COST[name]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)


# ------------------------------------------------------------------ 3. the host loop
@pytest.mark.parametrize("name", ["n_v3_o3_beam4_kV", "n_v11_o2_b17_beam4_k3", "n_v63_o5_beam16_k16",
                                  "n_v128_o1_beam1_k1", "n_v6_o3_reenter"])
def test_module_loop_with_an_ngram_lm_is_the_restatement(name):
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    c = C.CASES[name]
    x, lens = C.make(name)
    lm = NgramLm.from_arpa(C.text_of(name), num_classes=c["V"], dtype=torch.float64)
    dec = CtcPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"])
    ref = C.reference(name)
    out = dec.beam_tokens(x.double(), lens)
    assert len(out) == 4
    for b, r in enumerate(ref):
        n = int(out[1][b])
        assert out[0][b, :n].tolist() == r.tokens and int(out[0][b, n:].sum()) == 0, (name, b)
        got = dec._module_loop(x[b:b + 1, :C.clamp(lens[b], c["T"])].double())
        assert got[0] == r.tokens
        assert got[1] == pytest.approx(r.score, abs=1e-9) and got[2] == pytest.approx(r.lm_score, abs=1e-9)
    assert dec.decode_batch(x.double(), lens) == [r.tokens for r in ref]
    f32 = CtcPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=C.model(name),
                                lm_weight=c["weight"])
    assert f32.decode_batch(x, lens) == [r.tokens for r in ref]
