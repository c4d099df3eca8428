"""CPU: the yardstick of the chunk-carried CTC prefix beam search fused with a back-off n-gram
(csrc/decode_ctc.hip s2t_ctc_prefix_beam_ngram_chunk).

tests/ctc_ngram_stream_f64.Stream is pinned against what exists: fed under any cut it is the whole-utterance
restatement tests/ctc_ngram_f64.py (itself pinned against the exhaustive sum) on the frames fed so far; with
lm_weight = 0 it is the plain chunked restatement tests/ctc_stream_f64.py, stable / kept / ever included;
on the exhaustive lattices of ctc_ngram_cases.BRUTE, one frame a call, it is the arg-max over all V^T
alignments plus the LM term.  Then the conditions every case must meet, with no exclusions: margins,
float32 on the same path, the LM changes a hypothesis, every back-off depth and the dense root,
re-entries, and in the COMPACTS cases a max_nodes that every call fits into and the sequences ever kept do
not; the float32 stream's cost is held to ctc_ngram_cases.COST.
"""
import numpy as np
import pytest
import torch

import ctc_ngram_cases as G
import ctc_ngram_f64 as NG
import ctc_ngram_stream_cases as C
import ctc_ngram_stream_f64 as S
import ctc_stream_f64 as PS
from rnnt_lstm_search_f64 import MARGIN
from yardstick import rel_err


# ------------------------------------------------------------------ 1. the restatement itself
@pytest.mark.parametrize("T,V,n,order,weight", G.BRUTE)
def test_stream_is_the_exhaustive_arg_max(T, V, n, order, weight):
    x = G.brute_logits(T, V, n).double()
    ng = NG.DictNgram(G.brute_text(V, order), V)
    for i, (labels, logp, lm, gap) in enumerate(G.brute_reference(T, V, n, order, weight)):
        s = S.Stream(16, V, ng, weight)
        for t in range(T):
            r = s.feed(x[i, t:t + 1])
        assert gap >= MARGIN and r.tokens == labels, (T, V, i)
        assert r.score == pytest.approx(logp, abs=1e-9) and r.lm_score == pytest.approx(lm, abs=1e-9)
        assert r.ever >= r.kept >= 1 and not r.overflow


@pytest.mark.parametrize("cut", C.CUTS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_chunked_equals_whole_after_every_call(name, cut):
    """After every call the stream reports the whole-utterance restatement on the frames fed so far."""
    c = C.CASES[name]
    x, lens = G.make(name)
    ng = G.dict_model(name, np.float64)
    reports, chunks = C.stream_reports(name, cut), C.chunks(name, cut)
    every = max(1, len(chunks) // 3)                       # (the whole restatement on a prefix: some calls, the last)
    for i, (_, _, fed) in enumerate(chunks):
        if i % every and i + 1 != len(chunks):
            continue
        for b in range(c["B"]):
            w = NG.prefix_beam_search(x[b, :fed[b]].double(), c["beam"], c["topk"], ng, c["weight"])
            r = reports[i][b]
            assert (r.tokens, r.score, r.lm_score) == (w.tokens, w.score, w.lm_score), (name, cut, i, b)
    for r, w in zip(reports[-1], G.reference(name)):
        assert (r.tokens, r.score, r.lm_score) == (w.tokens, w.score, w.lm_score), (name, cut)
    assert not any(r.overflow for row in reports for r in row)


@pytest.mark.parametrize("name", list(C.CASES))
def test_weight_zero_is_the_plain_chunked_restatement(name):
    c = C.CASES[name]
    x, _ = G.make(name)
    fused = C.stream_reports(name, "ragged", None, 0.0)
    plain = [PS.Stream(c["beam"], c["topk"]) for _ in range(c["B"])]
    pos = [0] * c["B"]
    for i, (_, ns) in enumerate(C.calls(name, "ragged")):
        for b, n in enumerate(ns):
            p = plain[b].feed(x[b, pos[b]:pos[b] + n].double())
            pos[b] += n
            f = fused[i][b]
            assert (f.tokens, f.score, f.stable, f.kept, f.ever) == (p.tokens, p.score, p.stable, p.kept, p.ever), \
                (name, i, b)


def test_admission_rule_and_inert_row():
    """A feed that does not fit consumes nothing, sets overflow, and the stream stays as it was."""
    name, cut = "n_v128_o3_beam4_k4", "r7"
    needs = C.row_needs(name, cut)
    limit = max(needs) - 1
    reports = C.stream_reports(name, cut, limit)
    b = needs.index(max(needs))
    first = next(i for i, row in enumerate(reports) if row[b].overflow)
    assert first > 0
    for row in reports[first:]:
        assert row[b] == reports[first - 1][b]._replace(overflow=True)
    free = C.stream_reports(name, cut)
    for i in range(first):
        assert reports[i][b] == free[i][b]


# ------------------------------------------------------------------ 2. the conditions on the cases
@pytest.mark.parametrize("name", list(C.CASES))
def test_every_utterance_of_the_case_is_decided(name):
    ref = G.reference(name)
    f32, _ = C.run(name, "r7", torch.float32)
    for b, (r, s) in enumerate(zip(ref, f32[-1])):
        assert r.margin >= MARGIN, (name, b, r.margin)
        assert r.tokens == s.tokens, (name, b)
    assert min(r.margin for r in G.unfused(name)) >= MARGIN, name
    f64 = lambda rows, k: torch.tensor([getattr(r, k) for r in rows], dtype=torch.float64)    # noqa: E731
    fig = max(rel_err(f64(f32[-1], k), f64(ref, k)) for k in ("score", "lm_score"))
    print(f"fp32 cost of score / lm_score, {name} streamed: {fig:.3e} (recorded {C.COST[name]:.1e})")
    assert fig <= 4 * C.COST[name]


def test_cases_cover_what_the_issue_names():
    cs = C.CASES.values()
    assert {3, 11, 63, 65, 128, 300} <= {c["V"] for c in cs}
    assert {1, 17, 33} <= {c["B"] for c in cs} and {1, 4, 16} <= {c["beam"] for c in cs}
    assert {1, 3, 16} <= {c["topk"] for c in cs} and any(c["topk"] > c["V"] for c in cs)
    assert {1, 2, 3, 5} <= {c["order"] for c in cs} and max(c["T"] for c in cs) <= 40
    assert C.CUTS == ("one", "r4", "r7", "ragged")
    assert any(0 in ns and max(ns) > 0 for name in C.CASES for _, ns in C.calls(name, "ragged"))   # idle rows
    for name in C.LM_CHANGES:
        a, b = C.stream_reports(name, "ragged")[-1], C.stream_reports(name, "ragged", None, 0.0)[-1]
        assert any(r.tokens != s.tokens for r, s in zip(a, b)), name
    hops, root = {}, {}
    for name in C.CASES:
        _, st = C.run(name, "one")
        hops[name] = set().union(*[s.hops for s in st])
        root[name] = any(s.root for s in st)
    assert any({0, 1, C.CASES[name]["order"] - 1} <= h and C.CASES[name]["order"] >= 3 for name, h in hops.items())
    deep = "n_v63_o5_beam16_k16"
    assert {0, 1, 2, 3, 4} <= hops[deep] and root[deep]
    for name in C.REENTER:
        assert sum(s.reentered for s in C.run(name, "r4")[1]) > 0, name


@pytest.mark.parametrize("name", C.COMPACTS)
def test_compacts_cases_fit_every_call_but_not_the_sequences_ever_kept(name):
    limit = C.max_nodes(name)
    most, ever = 0, []
    for cut in C.CUTS:
        m, ever = C.need(name, cut)
        most = max(most, m)
        reports = C.stream_reports(name, cut)
        assert any(r.kept < r.ever for row in reports for r in row), (name, cut)   # kept after a compaction
        bounded = C.stream_reports(name, cut, limit)
        assert bounded == reports, (name, cut)             # no call is refused under the limit
    print(f"{name}: max_nodes {limit}, largest need {most}, sequences ever kept {max(ever)}")
    assert most <= limit < max(ever), (name, most, limit, ever)
    assert limit < 1 + C.CASES[name]["T"] * C.CASES[name]["beam"]
