"""GPU: the one-launch RNN-T beam search of the stateless predictor with hotword biasing, without an LM and fused
with a back-off n-gram (csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_bias, s2t_rnnt_beam_stateless_ngram_bias;
the frame body is csrc/decode_search.h beam_walk's bias mode, the look-up csrc/ngram_lookup.h) against the float64
restatement of tests/rnnt_bias_f64.py on the seeded cases of tests/rnnt_bias_cases.py.

Tokens, counts and emission frames are compared for exact equality: tests/test_rnnt_bias_f64.py asserts that
float64 decides every ranking cut and every finalisation pick of every utterance of every case by at least 1e-3
and that float32 walks the same path.  score, lm_score and bias_score are held to yardstick.bound_of(what float32
costs the restatement itself), figures recorded in the cases file.  The searches are fed `am` directly (the
joiner's enc_proj replaced by the identity).
"""
import numpy as np
import pytest
import torch

import rnnt_bias_cases as C
import rnnt_ngram_cases as NC
from decode_support import _beam_modules, _lm_module, _lstm_build, _ngram_case
from rnnt_beam_restatement import load_fixture

pytestmark = pytest.mark.gpu


def _column(rows, i):
    return torch.tensor([r[i] for r in rows], dtype=torch.float64)


def _same_path(out, ref, what, zeroed=True):
    tokens, frames, out_len = (x.cpu() for x in out[:3])
    for b, r in enumerate(ref):
        n = len(r.tokens)
        assert int(out_len[b]) == n, (what, b, int(out_len[b]), n)
        assert tokens[b, :n].tolist() == r.tokens and frames[b, :n].tolist() == r.frames, (what, b)
        assert not zeroed or ((tokens[b, n:] == 0).all() and (frames[b, n:] == 0).all())


# ------------------------------------------------------------------ 1. both entries against float64
@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_search_exact(dev, name):
    case = C.device_case(dev, name)
    c, am, ref = case[0], case[5], case[7]
    out = C.fused(case)
    with_lm = c["order"] > 0
    assert out is not None and len(out) == (6 if with_lm else 5)
    assert out[0].shape == out[1].shape == am.shape[:2] and out[0].dtype == torch.int64
    assert all(x.dtype == torch.float32 for x in out[3:])
    _same_path(out, ref, name)
    _same_path(out, C.reference32(name), name + " float32 restatement")
    errs = {"score": C.rel_err(out[3], _column(ref, 1)), "bias_score": C.rel_err(out[-1], _column(ref, 3))}
    if with_lm:
        errs["lm_score"] = C.rel_err(out[4], _column(ref, 2))
    limit = C.bound(name)
    print(f"{name}: " + " ".join(f"{k} rel_err {v:.2e}" for k, v in errs.items()) + f" bound {limit:.2e}")
    assert max(errs.values()) <= limit, (name, errs, limit)
    if am.shape[0] > 1:                                    # no frames: no tokens, all scores 0
        assert int(out[2][1]) == 0 and all(float(x[1]) == 0.0 for x in out[3:])
    if c["beam"] > 1:                                      # and the bias term is not inert
        assert not torch.equal(C.fused(case, bias_weight=0.0)[0], out[0])


def test_the_long_cases_trace_back_from_another_position(dev):
    """The reported beam is not position 0 and its tokens lie in both 64-frame blocks of the records."""
    for name in C.LONG:
        case = C.device_case(dev, name)
        r = case[7][0]
        assert r.final_pos != 0 and r.frames[0] < 6 and r.frames[-1] >= 6
        out = C.fused(case)
        _same_path(out, case[7], name)
        partner = C.fused(case, bias_weight=0.0)
        assert not torch.equal(partner[0], out[0])


# ------------------------------------------------------------------ 2. the exhaustive cases
@pytest.mark.parametrize("i", range(len(C.BRUTE)))
def test_search_is_the_argmax_over_all_labellings(dev, i):
    """Every input of rnnt_bias_cases.brute_decided(i) (chosen on the CPU, where tests/test_rnnt_bias_f64.py asserts
    that all BRUTE_N seeds are decided by 1e-3): tokens and frames are the exhaustive arg-max's, the three scores
    are held to yardstick.bound_of(what float32 costs the restatement on these inputs)."""
    from speech2text_amd.model.lm.context_graph import ContextGraph
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    from speech2text_amd.model.rnnt_bias import rnnt_beam_bias_tokens_from_am
    V, T, _, order, weight, phrases, bias_weight = C.BRUTE[i]
    lm = NgramLm.from_arpa(C.brute_text(V, order), num_classes=V).to(dev) if order else None
    graph = ContextGraph([list(p) for p in phrases], V, context_score=1.0).to(dev)
    rows, got = C.brute_decided(i), []
    assert len(rows) == C.BRUTE_N
    for p, am, best, _, _ in rows:
        cfg = dict(V=V, act="relu", **C.BRUTE_DIMS, **{k: np.asarray(v, dtype=np.float32) for k, v in p.items()})
        pred, join = _beam_modules(cfg, dev)
        join._enc_proj = torch.nn.Identity()
        out = rnnt_beam_bias_tokens_from_am(torch.from_numpy(am).float().unsqueeze(0).to(dev), torch.tensor([T]), pred,
                                            join, graph, bias_weight, lm, weight, 16, V)
        k = int(out[2][0])
        assert out[0][0, :k].tolist() == best[0] and out[1][0, :k].tolist() == best[1]
        got.append((float(out[3][0]), float(out[4][0]) if order else 0.0, float(out[-1][0])))
    col = lambda xs, j: torch.tensor([x[j] for x in xs], dtype=torch.float64)        # noqa: E731
    errs = [C.rel_err(col(got, j), col([r[2][2:5] for r in rows], j)) for j in range(3)]
    limit = C.bound_of(C.BRUTE_COST[i])
    print(f"exhaustive {C.BRUTE[i][:2]} order {order}: score {errs[0]:.2e} lm_score {errs[1]:.2e} bias_score "
          f"{errs[2]:.2e} bound {limit:.2e}")
    assert max(errs) <= limit, (errs, limit)


# ------------------------------------------------------------------ 3. an inert bias is the partner entry, bit for bit
def _inert(dev, p, j, am, lens, lm, weight, beam, topk, V):
    """The partner entry's outputs and, with bias_weight 0 and with a graph of no phrases, the bias entry's."""
    from speech2text_amd.model.decoding import rnnt_beam_ngram_tokens_from_am, rnnt_beam_tokens_from_am
    from speech2text_amd.model.lm.context_graph import ContextGraph
    from speech2text_amd.model.rnnt_bias import rnnt_beam_bias_tokens_from_am
    if lm is None:
        partner = rnnt_beam_tokens_from_am(am, lens, p, j, beam, topk)
    else:
        partner = rnnt_beam_ngram_tokens_from_am(am, lens, p, j, lm, weight, beam, topk)
    phrases = [[1, 2], [2, 1, 1]] if V > 2 else [[1, 1]]
    zero = rnnt_beam_bias_tokens_from_am(am, lens, p, j, ContextGraph(phrases, V).to(dev), 0.0, lm, weight, beam, topk)
    empty = rnnt_beam_bias_tokens_from_am(am, lens, p, j, ContextGraph([], V).to(dev), 1.5, lm, weight, beam, topk)
    assert partner is not None and int(partner[2].sum()) > 0
    for got, what in ((zero, "bias_weight 0"), (empty, "no phrases")):
        assert got is not None and len(got) == len(partner) + 1
        for x, y, k in zip(got, partner, ("tokens", "frames", "out_len", "score", "lm_score")):
            assert torch.equal(x, y), (what, k)
    assert float(empty[-1].abs().max()) == 0.0
    return zero


@pytest.mark.parametrize("name", list(NC.CASES))
def test_inert_bias_is_the_partner_entry_on_the_ngram_cases(dev, name):
    c, p, j, lm, am, lens, _ = _ngram_case(dev, name)
    _inert(dev, p, j, am, lens, None, 0.0, c["beam"], c["topk"], c["V"])
    _inert(dev, p, j, am, lens, lm, c["weight"], c["beam"], c["topk"], c["V"])


def test_inert_bias_is_the_partner_entry_on_the_golden_configurations(dev, golden_dir):
    import ctc_ngram_cases as CN
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    configs = load_fixture(golden_dir)
    assert len(configs) == 5
    for c in configs:
        pred, join = _beam_modules({k: v for k, v in c.items() if k not in ("enc_w", "enc_b")}, dev)
        join._enc_proj = torch.nn.Identity()
        am, lens = torch.from_numpy(c["am"]).to(dev), torch.from_numpy(c["lengths"]).to(dev)
        _inert(dev, pred, join, am, lens, None, 0.0, c["beam"], c["topk"], c["V"])
        lm = NgramLm.estimate(CN.lm_sequences(c["V"], 200, 4), c["V"], order=3).to(dev)
        _inert(dev, pred, join, am, lens, lm, 0.4, c["beam"], c["topk"], c["V"])


# ------------------------------------------------------------------ 4. batch invariance
@pytest.mark.parametrize("name", ["h_v65_b17", "h_v65_b17_o3", "h_yaml_o3"])
def test_a_row_alone_is_the_row_in_its_batch(dev, name):
    case = C.device_case(dev, name)
    am, lens = case[5], case[6]
    whole = C.fused(case)
    for b in (0, 2, am.shape[0] - 1):
        alone = C.fused(case, am=am[b:b + 1].contiguous(), lens=lens[b:b + 1])
        for x, y in zip(alone, whole):
            assert torch.equal(x[0], y[b]), (name, b)


# ------------------------------------------------------------------ 5. refusals of the wrapper
def test_wrapper_refuses(dev):
    import math
    case = C.device_case(dev, "h_v11_kV_o2")
    with pytest.raises(RuntimeError, match="ContextGraph.to"):
        C.fused(case, graph=C.graph_of("h_v11_kV_o2"))
    assert C.fused(case, beam_size=17) is None
    assert C.fused(case, bias_weight=math.nan) is None
    assert C.fused(case, graph=C.graph_of("h_v63_beam1_k1").to(dev)) is None       # graph.V != V


# ------------------------------------------------------------------ 6. RnntBiasBeamDecoding
def _decoder(case, p=None, j=None, **kw):
    from speech2text_amd.model.rnnt_bias import RnntBiasBeamDecoding
    c, p0, j0, g, lm = case[:5]
    args = dict(beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"], context=g,
                context_weight=c["bias_weight"])
    args.update(kw)
    return RnntBiasBeamDecoding(C.Ids(), p0 if p is None else p, j0 if j is None else j, **args)


def _counted(monkeypatch):
    """Counts the calls of the fused wrapper the class makes."""
    from speech2text_amd.model import rnnt_bias as B
    calls, real = [], B.rnnt_beam_bias_tokens_from_am

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(B, "rnnt_beam_bias_tokens_from_am", spy)
    return calls


@pytest.mark.parametrize("name", ["h_v65_b17", "h_v65_b17_o3"])
def test_class_takes_the_fused_entry_and_agrees_with_its_host_loop(dev, monkeypatch, name):
    from speech2text_amd import _native as N
    case = C.device_case(dev, name)
    c, am, lens, ref = case[0], case[5], case[6], case[7]
    graph, lm = C.graph_of(name), C.model_of(name)         # CPU tables: they follow the inputs
    calls = _counted(monkeypatch)
    dec = _decoder(case, context=graph, lm=lm)
    out = dec.beam_tokens(am, lens)
    assert calls == [True] and graph.device.type == "cuda" and len(out) == (6 if lm is not None else 5)
    _same_path(out, ref, name)
    assert dec.decode_batch(am[:3], lens[:3]) == [C.Ids().decode(r.tokens) for r in ref[:3]]
    assert N.lib().s2t_gemm_arith_set(3) == 0              # the modules' own GEMMs in fp32 arithmetic
    try:
        loop = dec.beam_tokens(am[:6], lens[:6], fused=False)
    finally:
        N.lib().s2t_gemm_arith_set(0)
    assert calls == [True, True]
    _same_path(loop, ref[:6], name + " host loop")
    for x, y in zip(loop[3:], out[3:]):
        assert C.rel_err(x, y[:6].double()) <= C.bound(name)


def test_fallbacks_reach_the_host_loop(dev, monkeypatch):
    """An out-projection joiner, the LSTM predictor and an RnnLm with a context: no fused call, the result is the
    host loop's, and its bias_score is the statement's final_bias of the tokens it reports."""
    name = "h_v11_kV"
    case = C.device_case(dev, name)
    c, am, lens = case[0], case[5], case[6]
    hot = C.hot_of(name, np.float64)
    torch.manual_seed(3)
    _, jo = C.build_modules(dev, c["V"], c["E"], c["D"], c["ctx"], c["act"], inner=16)
    pl, jl = _lstm_build(dev, c["V"], 8, 16, c["D"], 1, True, 0, c["act"])
    rnn = _lm_module(dev, V=c["V"], H=16, layers=1)
    calls, biased = _counted(monkeypatch), []
    for what, dec in (("out-projection", _decoder(case, j=jo)), ("lstm", _decoder(case, p=pl, j=jl)),
                      ("rnn-lm", _decoder(case, lm=rnn, lm_weight=0.3))):
        out = dec.beam_tokens(am[:1], lens[:1])
        direct = dec._module_loop_lm(am[:1])
        n = int(out[2][0])
        assert calls == [] and len(out) == (6 if what == "rnn-lm" else 5), what
        assert out[0][0, :n].tolist() == direct[0] and out[1][0, :n].tolist() == direct[1], what
        assert float(out[-1][0]) == float(torch.tensor(direct[4], dtype=torch.float32)), what   # (stored in fp32)
        want = torch.tensor([float(hot.final_bias(tuple(direct[0])))], dtype=torch.float64)
        assert C.rel_err(out[-1].double().cpu(), want) <= C.bound(name), what
        biased.append(float(want) != 0.0)
    assert any(biased)                                     # (a reported hypothesis that kept a bonus is among them)
