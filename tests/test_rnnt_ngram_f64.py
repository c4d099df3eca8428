"""CPU: the conditions of tests/rnnt_ngram_cases.py, the restatement of tests/rnnt_ngram_f64.py against an
exhaustive search, and the host side of the RNN-T beam search fused with a back-off n-gram
(model/decoding.py RnntBeamDecoding._module_loop_lm, rnnt_streaming_search).

    1. every utterance of every case is decided by at least 1e-3 at every ranking cut in float64, the
       float32 run walks the same tokens and frames, with beam > 1 the LM changes a hypothesis, every
       back-off depth 0 .. order - 1 occurs; the recorded float32 figures still cover what is measured
    2. at (V 2, T 4) and (V 3, T 2), beam 16 and top-k V, the search drops nothing: its best hypothesis
       is the arg-max over all V^T frame labellings of path log-probability + lm_weight x the dict
       n-gram's score of the emitted tokens from <s> -- the first-token term and "blank carries no LM
       term", independently of the restatement's own loop
    3. RnntBeamDecoding(lm=NgramLm) on CPU tensors is the restatement, the first token scored; an LM
       without start_scores is driven as before
    4. what the chunk-carried searches refuse of an NgramLm
"""
import numpy as np
import pytest
import torch

import ctc_ngram_f64 as G
import rnnt_ngram_cases as C
import rnnt_ngram_f64 as R


# ------------------------------------------------------------------ 1. the cases' conditions
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_conditions(name):
    c = C.CASES[name]
    ref, f32 = C.reference(name), C.reference32(name)
    lens = C.make(name)[2].tolist()
    assert lens[0] == c["T"] and (c["B"] < 2 or lens[1] == 0) and (c["B"] < 3 or lens[2] > c["T"])
    for b, (r, s) in enumerate(zip(ref, f32)):
        assert r.margin >= C.MARGIN, (name, b, r.margin)
        assert (r.tokens, r.frames) == (s.tokens, s.frames), (name, b)
        assert len(r.tokens) == len(r.frames) <= C.clamp(lens[b], c["T"])
    assert any(len(r.tokens) >= 2 for r in ref)
    if c["beam"] > 1:
        assert any(r.tokens != u.tokens for r, u in zip(ref, C.unfused(name))), name
    else:
        assert all(r.tokens == u.tokens and r.frames == u.frames for r, u in zip(ref, C.unfused(name)))
    fig = C.fp32_figure(name)
    print(f"{name}: float32 costs the restatement {fig:.3e}, recorded {C.COST[name]:.1e}, bound {C.bound(name):.1e}")
    assert fig <= C.COST[name]


def test_every_back_off_depth_occurs():
    seen = {}
    for name, c in C.CASES.items():
        got = seen.setdefault(c["order"], [set(), False])
        for r in C.reference(name):
            got[0] |= r.hops
            got[1] = got[1] or r.root
    assert sorted(seen) == [1, 2, 3, 5]
    for order, (hops, root) in seen.items():
        assert hops == set(range(order)) and root, (order, hops, root)


def test_shapes_cover_what_the_kernels_branch_on():
    V = {c["V"] for c in C.CASES.values()}
    assert {63, 65} <= V and any(v > 512 for v in V)
    assert {c["ctx"] for c in C.CASES.values()} >= {1, 2, 5}
    assert any(c["B"] == 17 for c in C.CASES.values())
    assert any(c["beam"] == 16 and c["topk"] == 16 for c in C.CASES.values())
    assert any(c["beam"] == 1 and c["topk"] == 1 for c in C.CASES.values())
    assert any(c["topk"] > c["V"] == 11 for c in C.CASES.values())
    c = C.CASES[C.LARGE]                                   # the lm rows do not fit 60 KiB next to the fixed part
    assert 16 * (c["E"] + c["D"]) + 128 * c["ctx"] + 4 * c["beam"] * c["V"] > 60 * 1024
    assert C.CASES[C.LONG]["T"] > 64 and len(C.reference(C.LONG)[0].tokens) > 16
    y = C.CASES[C.YAML]
    assert (y["V"], y["E"], y["D"], y["ctx"], y["B"], y["T"]) == (128, 512, 256, 5, 4, 12)


def test_chunked_restatement_is_the_whole_one():
    for name in ("g_v65_o3_b17", C.LONG):
        c = C.CASES[name]
        p, am, lens = C.make(name)
        p = {k: v.numpy() for k, v in p.items()}
        for b in range(min(c["B"], 4)):
            L = C.clamp(lens[b], c["T"])
            for kind in (1, 7, "ragged"):
                got, stable = R.beam_search_chunked(am[b, :L].numpy(), C.cuts_of(name, b, kind), p, c["ctx"], c["act"],
                                                    c["beam"], c["topk"], C.dict_model(name, np.float64), c["weight"])
                want = C.reference(name)[b]
                assert got[:4] == want[:4], (name, b, kind)
                assert all(x <= y for x, y in zip(stable, stable[1:])) and (not stable or stable[-1] <= len(got.tokens))


# ------------------------------------------------------------------ 2. the exhaustive check
@pytest.mark.parametrize("V, T, n, order, weight", C.BRUTE)
def test_search_is_the_argmax_over_all_labellings(V, T, n, order, weight):
    ng = G.DictNgram(C.brute_text(V, order), V)
    ctx, clear, emitted = C.BRUTE_DIMS["ctx"], 0, 0
    for p, am in C.brute_inputs(V, T, n):
        got = R.beam_search(am, p, ctx, "relu", 16, V, ng, weight)
        tokens, frames, total, lms, gap = R.brute_force(am, p, ctx, "relu", ng, weight)
        assert abs(got.score - total) <= 1e-9
        if gap > 1e-9:
            clear += 1
            emitted += len(tokens) > 0
            assert (got.tokens, got.frames) == (tokens, frames)
            assert abs(got.lm_score - lms) <= 1e-9
    assert clear >= n - 2 and emitted >= n // 4            # (the first-token term is exercised)


# ------------------------------------------------------------------ 3. the host loop
def _decode(name, lm, dtype=torch.float64, **kw):
    from speech2text_amd.model.decoding import RnntBeamDecoding
    c = C.CASES[name]
    pred, join = C.plain_modules(name, dtype)
    _, am, lens = C.make(name)
    args = dict(beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"])
    args.update(kw)
    dec = RnntBeamDecoding(C.Ids(), pred, join, **args)
    return dec.beam_tokens(am.to(dtype), lens), dec


def _model64(name):
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.from_arpa(C.text_of(name), num_classes=C.CASES[name]["V"], dtype=torch.float64)


@pytest.mark.parametrize("name", ["g_v11_o2_kV", "g_v65_o3_b17"])
def test_module_loop_scores_the_first_token(name):
    (tokens, frames, out_len, score, lm_score), _ = _decode(name, _model64(name))
    ref = C.reference(name)
    for b, r in enumerate(ref):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == r.tokens and frames[b, :n].tolist() == r.frames, (name, b)
    want = lambda i: torch.tensor([r[i] for r in ref], dtype=torch.float64)          # noqa: E731
    assert C.rel_err(score, want(1)) <= 1e-6 and C.rel_err(lm_score, want(2)) <= 1e-6   # (outputs are stored in fp32)
    assert any(r.tokens and abs(r.lm_score) > 0 for r in ref)


class _NoStartScores:
    """An NgramLm of which only init_states / score_step show."""

    def __init__(self, lm):
        self._lm = lm

    def init_states(self, n):
        return self._lm.init_states(n)

    def score_step(self, tokens, states):
        return self._lm.score_step(tokens, states)


class _FirstTokenFree:
    """A DictNgram whose first token of a sentence carries no term: how a host loop that does not know
    start_scores drives an LM (q = 0 until the LM was stepped once)."""

    def __init__(self, ng):
        self.ng, self.dt = ng, ng.dt

    def score(self, tokens, c):
        return (self.dt(0.0), 0, False) if not tokens else self.ng.score(tokens, c)


@pytest.mark.parametrize("name", ["g_v11_o2_kV", "g_v65_o3_b17"])
def test_an_lm_without_start_scores_is_driven_as_before(name):
    c = C.CASES[name]
    (tokens, frames, out_len, score, lm_score), _ = _decode(name, _NoStartScores(_model64(name)))
    p, am, lens = C.make(name)
    p = {k: v.numpy() for k, v in p.items()}
    ng = _FirstTokenFree(C.dict_model(name, np.float64))
    differs = False
    for b in range(c["B"]):
        want = R.beam_search(am[b, :C.clamp(lens[b], c["T"])].numpy(), p, c["ctx"], c["act"], c["beam"], c["topk"], ng,
                             c["weight"])
        n = int(out_len[b])
        assert want.margin >= C.MARGIN, (name, b, want.margin)
        assert tokens[b, :n].tolist() == want.tokens and frames[b, :n].tolist() == want.frames, (name, b)
        assert abs(float(score[b]) - want.score) <= 1e-5 * max(1.0, abs(want.score))
        assert abs(float(lm_score[b]) - want.lm_score) <= 1e-5 * max(1.0, abs(want.lm_score))
        differs = differs or abs(want.lm_score - C.reference(name)[b].lm_score) > 1e-3
    assert differs                                         # (the two protocols are told apart on these inputs)


def test_a_start_token_still_steps_the_lm():
    """With lm_start_token the loop steps the LM on it, start_scores or not: both spellings agree."""
    name = "g_v11_o2_kV"
    a, _ = _decode(name, _model64(name), lm_start_token=3)
    b, _ = _decode(name, _NoStartScores(_model64(name)), lm_start_token=3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 4. refusals
def test_chunk_carried_searches_refuse_an_ngram_where_it_is_not_fused():
    from speech2text_amd.model.decoding import CtcStreamingSearch, rnnt_streaming_search
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    name = "g_v11_o2_kV"
    lm = C.model(name)
    pred, join = C.build_modules("cpu", 11, 12, 24, 1)
    with pytest.raises(ValueError, match="greedy"):
        rnnt_streaming_search(pred, join, method="greedy", lm=lm, lm_weight=0.5)
    lstm = Predictor({"model": "Lstm", "config": {
        "num_symbols": 11, "output_dim": 24, "symbol_embedding_dim": 8, "num_lstm_layers": 1, "lstm_hidden_dim": 8,
        "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}}).eval()
    j2 = Joiner(JoinerConfig(input_dim=24, output_dim=11, inner_dim=8, activation="relu", use_out_project=False)).eval()
    with pytest.raises(ValueError, match="NgramLm"):
        rnnt_streaming_search(lstm, j2, method="beam", lm=lm, lm_weight=0.5)
    with pytest.raises(ValueError, match="lm_start_token"):
        rnnt_streaming_search(pred, join, method="beam", lm=lm, lm_weight=0.5, lm_start_token=3)
    with pytest.raises(ValueError, match="NgramLm"):
        CtcStreamingSearch(11, lm=lm, lm_weight=0.5)
