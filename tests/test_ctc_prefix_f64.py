"""CPU: the yardstick of the CTC prefix beam search (csrc/decode_ctc.hip s2t_ctc_prefix_beam,
s2t_ctc_prefix_beam_lm) and the Python surface around it.

tests/ctc_prefix_f64.py is pinned against the exhaustive sum over all V^T alignments where the beam
holds every reachable prefix (a search that does not merge equal prefixes fails there) and against the
greedy collapse at beam 1 / top-1.  Then the conditions every case of tests/ctc_prefix_cases.py must meet,
with no exclusions (margins, float32 on the same path, merges, re-entries, the LM changes a hypothesis),
the recorded float32 costs to a factor 4, CtcPrefixBeamDecoding._module_loop against the restatement and
the metric's new method name.
"""
import pytest
import torch

import ctc_prefix_cases as C
import ctc_prefix_f64 as P
import rnnt_lm_fusion_cases as L
import rnnt_lm_fusion_f64 as F
from rnnt_lstm_search_f64 import MARGIN
from yardstick import _Ids


# ------------------------------------------------------------------ 1. the restatement itself
@pytest.mark.parametrize("T,V,n", C.BRUTE)
def test_restatement_is_the_exhaustive_sum(T, V, n):
    x = C.brute_logits(T, V, n).double()
    assert n >= 100
    for i, (labels, logp, gap) in enumerate(C.brute_reference(T, V, n)):
        r = P.prefix_beam_search(x[i], 16, V)
        assert gap >= MARGIN, (i, gap)                     # (what lets a float32 search be held to it)
        assert r.tokens == labels, (T, V, i)
        assert r.score == pytest.approx(logp, abs=1e-9)


def test_the_exhaustive_cases_need_the_merge():
    """On some of them the best single alignment spells another labelling than the most probable one,
    and extensions do land on live prefixes: a search that keeps equal prefixes apart fails above."""
    T, V, n = C.BRUTE[0]
    x = C.brute_logits(T, V, n).double()
    ref = C.brute_reference(T, V, n)
    assert sum(P.prefix_beam_search(x[i], 16, V).merged for i in range(n)) > 0
    assert sum(P.greedy_collapse(x[i]) != ref[i][0] for i in range(n)) > 0


@pytest.mark.parametrize("name", list(C.CASES))
def test_beam1_top1_is_the_greedy_collapse(name):
    x, lens, _ = C.make(name)
    for b in range(x.shape[0]):
        row = x[b, :C.clamp(lens[b], x.shape[1])].double()
        assert P.prefix_beam_search(row, 1, 1).tokens == P.greedy_collapse(row), (name, b)


def test_already_normalised_rows_change_nothing():
    x, lens, _ = C.make("p_v63_beam16_k16")
    row = x[1].double()
    a, b = P.prefix_beam_search(row, 16, 16), P.prefix_beam_search(torch.log_softmax(row, -1), 16, 16)
    assert a.tokens == b.tokens and a.score == pytest.approx(b.score, abs=1e-9)


def test_lm_weight_zero_is_the_plain_search_and_lm_score_is_the_lms():
    name = "l_v65_lm48_b17_beam4_k3"
    c = C.CASES[name]
    x, lens, sd = C.make(name)
    sd64 = L.cast(sd, torch.float64)
    for b, r in enumerate(C.unfused(name)):
        row = x[b, :C.clamp(lens[b], c["T"])].double()
        plain = P.prefix_beam_search(row, c["beam"], c["topk"])
        assert r.tokens == plain.tokens and r.score == plain.score
    for r in C.reference(name):
        assert r.lm_score == pytest.approx(F.lm_score_ref(sd64, r.tokens, c["start"]), abs=1e-9)
    name = "l_v128_lm64_beam16_start"
    sd64 = L.cast(C.make(name)[2], torch.float64)
    for r in C.reference(name):                            # with a start token the first token is scored too
        assert r.lm_score == pytest.approx(F.lm_score_ref(sd64, r.tokens, 127), abs=1e-9)


# ------------------------------------------------------------------ 2. the conditions on the cases
@pytest.mark.parametrize("name", list(C.CASES))
def test_every_utterance_of_the_case_is_decided(name):
    ref, f32 = C.reference(name), C.evaluate(name, torch.float32)
    print(f"{name}: smallest float64 margin {min(r.margin for r in ref):.3e}, merged "
          f"{sum(r.merged for r in ref)}, re-entered {sum(r.reentered for r in ref)}")
    for b, (r, s) in enumerate(zip(ref, f32)):
        assert r.margin >= MARGIN, (name, b, r.margin)
        assert r.tokens == s.tokens, (name, b)
    if name in C.LM_CASES:                                 # the plain entry is held to the un-fused search on them
        assert min(r.margin for r in C.unfused(name)) >= MARGIN, name
    x, lens, _ = C.make(name)
    for b in range(x.shape[0]):                            # NaN exactly at and beyond the length
        n = C.clamp(lens[b], x.shape[1])
        assert bool(torch.isfinite(x[b, :n]).all()) and bool(torch.isnan(x[b, n:]).all())


def test_cases_cover_what_the_issue_names():
    cs = C.CASES.values()
    assert {3, 11, 63, 65, 128} <= {c["V"] for c in cs} and any(c["V"] > 256 for c in cs)
    assert {1, 17, 33} <= {c["B"] for c in cs} and {1, 2, 4, 16} <= {c["beam"] for c in cs}
    assert {1, 3, 16} <= {c["topk"] for c in cs} and any(c["topk"] > c["V"] for c in cs)
    assert any(c["norm"] for c in cs) and any(not c["norm"] for c in cs)
    assert max(c["T"] for c in cs) == 40
    lens = torch.cat([C.lengths_of(c) - c["T"] for c in cs])
    assert bool((lens == 0).any()) and bool((lens > 0).any()) and bool((lens < 0).any())
    assert any(int(n) == 0 for c in cs for n in C.lengths_of(c))
    assert any(c["start"] is not None for c in cs)
    assert sum(r.merged for name in C.CASES for r in C.reference(name)) > 0
    assert len(C.REENTER) >= 2
    for name in C.REENTER:
        assert sum(r.reentered for r in C.reference(name)) > 0, name
    assert sum(r.merged for name in C.LM_CASES for r in C.reference(name)) > 0
    for name in C.LM_CHANGES:
        assert any(a.tokens != b.tokens for a, b in zip(C.reference(name), C.unfused(name))), name


@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_cost_of_the_scores(name):
    fig = C.fp32_figure(name)
    print(f"fp32 cost of score / lm_score, {name}: {fig:.3e}")
    rec = C.COST[name]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)


# ------------------------------------------------------------------ 3. the class
@pytest.mark.parametrize("name", ["p_v3_beam4_kV", "p_v63_beam16_k16", "p_v6_reenter", "p_v5_reenter",
                                  "l_v63_lm20_beam4", "l_v128_lm64_beam16_start"])
def test_module_loop_on_cpu_tensors_is_the_restatement(name):
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding
    c = C.CASES[name]
    x, lens, sd = C.make(name)
    lm = F.PlainLm(L.cast(sd, torch.float64)) if sd is not None else None
    dec = CtcPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"],
                                lm_start_token=c["start"])
    ref = C.reference(name)
    out = dec.beam_tokens(x.double(), lens)
    assert len(out) == (4 if lm is not None else 3)
    for b, r in enumerate(ref):
        n = int(out[1][b])
        assert out[0][b, :n].tolist() == r.tokens and int(out[0][b, n:].sum()) == 0, (name, b)
        assert float(out[2][b]) == pytest.approx(r.score, rel=1e-6, abs=1e-6)
        got = dec._module_loop(x[b:b + 1, :C.clamp(lens[b], c["T"])].double())
        assert got[0] == r.tokens
        assert got[1] == pytest.approx(r.score, abs=1e-9) and got[2] == pytest.approx(r.lm_score, abs=1e-9)
    assert dec.decode_batch(x.double(), lens) == [r.tokens for r in ref]
    assert dec.decode(x[:1, :C.clamp(lens[0], c["T"])].double()) == ref[0].tokens


def test_argument_checks_and_defaults():
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding, DecodingMethod
    dec = CtcPrefixBeamDecoding(tokenizer=_Ids())
    assert isinstance(dec, DecodingMethod)
    assert (dec._beam_size, dec._cutoff_top_k, dec._lm, dec._lm_weight, dec._lm_start_token) == (4, 4, None, 0.0, None)
    with pytest.raises(ValueError):
        CtcPrefixBeamDecoding(_Ids(), lm=object(), lm_start_token=-2)
    with pytest.raises(ValueError):
        CtcPrefixBeamDecoding(_Ids(), beam_size=0)
    with pytest.raises(AssertionError):
        dec.decode(torch.zeros(2, 3, 4))


def test_metric_builds_for_the_new_method_name():
    from speech2text_amd.model.decoding import CtcGreedyDecoding, CtcPrefixBeamDecoding
    from speech2text_amd.model.utils import AsrMetric, AsrMetricConfig
    assert AsrMetricConfig().decode_method == "ctc_greedy_search"
    assert isinstance(AsrMetric(_Ids(), AsrMetricConfig())._decode_sess, CtcGreedyDecoding)
    lm = object()
    m = AsrMetric(_Ids(), AsrMetricConfig(decode_method="ctc_prefix_beam_search", beam_size=3, cutoff_top_k=5,
                                          lm_weight=0.4, lm_start_token=7), lm=lm)
    s = m._decode_sess
    assert isinstance(s, CtcPrefixBeamDecoding) and s._lm is lm and m._lm is lm
    assert (s._beam_size, s._cutoff_top_k, s._lm_weight, s._lm_start_token) == (3, 5, 0.4, 7)
    with pytest.raises(NotImplementedError):
        AsrMetric(_Ids(), AsrMetricConfig(decode_method="ctc_lexicon_beam_search"))
