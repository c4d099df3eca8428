"""GPU: the hotword graph's look-up (csrc/ngram_lookup.h, s2t_context_score) and the CTC prefix beam search
with hotword biasing in one launch, without and with the back-off n-gram (csrc/decode_ctc.hip
s2t_ctc_prefix_beam_bias, s2t_ctc_prefix_beam_ngram_bias), against the float64 restatement
tests/ctc_bias_f64.py on the cases of tests/ctc_bias_cases.py, whose conditions (every decision, the
finalisation's included, made by at least 1e-3 in float64; the named events) tests/test_ctc_bias_f64.py
asserts on the CPU.  The look-up is held to the host's fp32 evaluation of the header's statement bit for
bit; tokens and out_len must equal the restatement's; score, lm_score and bias_score are bounded by
max(2e-5, 8 x what float32 costs the restatement), relative to the largest reference value of the case.
Frames at and beyond an utterance's length are NaN in every case.
"""
import numpy as np
import pytest
import torch

import ctc_bias_cases as C
import ctc_ngram_cases as NC
import ctc_prefix_cases as PC
from yardstick import _Ids

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(dev, name):
    """-> (case dict, logits, lengths, the case's graph and n-gram (or None) on the device)."""
    if name not in _CACHE:
        x, lens = C.make(name)
        lm = C.model_of(name)
        _CACHE[name] = (C.CASES[name], x.to(dev), lens.to(dev), C.graph_of(name).to(dev),
                        None if lm is None else lm.to(dev))
    return _CACHE[name]


def _fused(c, x, lens, graph, lm, **kw):
    from speech2text_amd.model.ctc_bias import ctc_prefix_beam_bias_tokens
    args = dict(bias_weight=c.get("bias_weight", 1.0), lm=lm, lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"])
    args.update(kw)
    out = ctc_prefix_beam_bias_tokens(x, lens, graph, **args)
    assert out is not None and len(out) == (4 if args["lm"] is None else 5)
    return out


def _partner(c, x, lens, lm):
    from speech2text_amd.model.decoding import ctc_prefix_beam_ngram_tokens, ctc_prefix_beam_tokens
    if lm is None:
        return ctc_prefix_beam_tokens(x, lens, c["beam"], c["topk"])
    return ctc_prefix_beam_ngram_tokens(x, lens, lm, c["weight"], c["beam"], c["topk"])


# ------------------------------------------------------------------ 1. the look-up on its own
@pytest.mark.parametrize("name", list(C.GRAPHS))
def test_lookup_is_the_hosts_fp32_statement_bit_for_bit(dev, name):
    """Every (state, class) pair of the graph: score and next."""
    from speech2text_amd.model.lm.context_graph import ContextGraph
    phrases, V, cs, scores = C.GRAPHS[name]
    host = ContextGraph(phrases, V, context_score=cs, phrase_scores=scores)
    g = ContextGraph(phrases, V, context_score=cs, phrase_scores=scores).to(dev)
    nc = host.num_ctx
    st = torch.arange(nc, dtype=torch.int32, device=dev).repeat_interleave(V)
    tok = torch.arange(V, dtype=torch.int32, device=dev).repeat(nc)
    score, nxt = g._device_score(st, tok)
    want = [host._row(n) for n in range(nc)]
    assert torch.equal(score.cpu().reshape(nc, V), torch.from_numpy(np.stack([w[0] for w in want])))
    assert torch.equal(nxt.cpu().reshape(nc, V), torch.from_numpy(np.stack([w[1] for w in want])))
    for n in range(0, nc, max(1, nc // 7)):                # (the row form is the scalar statement)
        for c in range(V):
            sc, nx = host.score(n, c)
            assert float(score[n * V + c]) == float(sc) and int(nxt[n * V + c]) == nx
    # rows outside the ranges are clamped into them; the protocol on the device is the same rows
    sc, _ = g._device_score(torch.tensor([-5, nc + 3], dtype=torch.int32, device=dev),
                            torch.tensor([-1, V + 9], dtype=torch.int32, device=dev))
    assert float(sc[0]) == float(host.score(0, 0)[0]) and float(sc[1]) == float(host.score(nc - 1, V - 1)[0])
    rows, new = g.score_step(torch.tensor([V - 1, 1], device=dev), g.init_states(2))
    hrows, hnew = host.score_step(torch.tensor([V - 1, 1]), host.init_states(2))
    assert torch.equal(rows.cpu(), hrows) and torch.equal(new.cpu(), hnew) and rows.is_cuda
    assert torch.equal(g.final_scores(new).cpu(), host.final_scores(hnew))


# ------------------------------------------------------------------ 2. the fused entries
def _check(name, out, ref, lm):
    out = [t.cpu() for t in out]
    tokens, out_len, score = out[:3]
    lm_score = out[3] if lm is not None else torch.zeros_like(score)
    bias_score = out[-1]
    for b, r in enumerate(ref):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == r.tokens, (name, b, tokens[b, :n].tolist(), r.tokens)
        assert int(tokens[b, n:].sum()) == 0
        if not r.tokens and r.score == 0.0:                # no frames: no tokens, all three scores 0
            assert float(score[b]) == 0.0 and float(lm_score[b]) == 0.0 and float(bias_score[b]) == 0.0
    f64 = lambda i: torch.tensor([r[i] for r in ref], dtype=torch.float64)    # noqa: E731
    for what, got, i in (("score", score, 1), ("lm_score", lm_score, 2), ("bias_score", bias_score, 3)):
        err = C.rel_err(got, f64(i))
        print(f"{name}: {what} rel_err {err:.3e} (bound {C.bound(name):.1e})")
        assert err <= C.bound(name), (name, what, err)


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_entries_against_the_float64_restatement(dev, name):
    """The entry without an LM on the cases of order 0, the n-gram entry on the others; every named event
    has a case of each (tests/test_ctc_bias_f64.py)."""
    c, x, lens, graph, lm = _case(dev, name)
    out = _fused(c, x, lens, graph, lm)
    _check(name, out, C.reference(name), lm)
    if name in C.EVENTS["changes"]:
        assert not torch.equal(out[0], _partner(c, x, lens, lm)[0]), "the bias changes no hypothesis"
    if name in C.EVENTS["final_pos"]:                      # the reported prefix is not the one at position 0
        assert any(r.final_pos > 0 for r in C.reference(name))


@pytest.mark.parametrize("T,V,n,order,weight,phrases,bias_weight", C.BRUTE)
def test_exhaustive_cases_through_the_kernels(dev, T, V, n, order, weight, phrases, bias_weight):
    """The reported labels maximise logsumexp(alignments) + lm + weight * final_bias over all label sequences
    (tests/test_ctc_bias_f64.py: the exhaustive sum decides every row by at least 1e-3 in float64)."""
    from speech2text_amd.model.lm.context_graph import ContextGraph
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    x = NC.brute_logits(T, V, n)
    ref = C.brute_reference(x.double(), order, weight, phrases, bias_weight)
    graph = ContextGraph([list(p) for p in phrases], V).to(dev)
    lm = NgramLm.from_arpa(C.lm_text(V, order, 60, 1), num_classes=V).to(dev) if order else None
    out = [t.cpu() for t in _fused(dict(beam=16, topk=V, weight=weight, bias_weight=bias_weight), x.to(dev),
                                   torch.full((n,), T, device=dev), graph, lm)]
    for i, r in enumerate(ref):
        assert out[0][i, :int(out[1][i])].tolist() == r[0], (T, V, i)
    pick = lambda t, k: (t, torch.tensor([r[k] for r in ref], dtype=torch.float64))   # noqa: E731
    assert C.rel_err(*pick(out[2], 1)) <= C.FLOOR and C.rel_err(*pick(out[-1], 3)) <= C.FLOOR
    if lm is not None:
        assert C.rel_err(*pick(out[3], 2)) <= C.FLOOR


def _invariants(dev, c, x, lens, lm):
    """bias_weight 0 with a graph that matches, and no phrases at weight 1: the partner's bits."""
    from speech2text_amd.model.lm.context_graph import ContextGraph
    V = c["V"]
    want = _partner(c, x, lens, lm)
    busy = ContextGraph([[1, 2], [2, 1, 2], [V - 1]], V, context_score=1.5).to(dev)
    empty = ContextGraph([], V).to(dev)
    for graph, w in ((busy, 0.0), (empty, 1.0)):
        out = _fused(c, x, lens, graph, lm, bias_weight=w)
        for a, b in zip(want, out[:-1]):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(out[-1]).all())
        if graph is empty:
            assert not out[-1].any()


@pytest.mark.parametrize("name", PC.PLAIN_CASES)
def test_weight_zero_and_no_phrases_are_the_plain_entry_bit_for_bit(dev, name):
    x, lens, _ = PC.make(name)
    _invariants(dev, PC.CASES[name], x.to(dev), lens.to(dev), None)


@pytest.mark.parametrize("name", list(NC.CASES))
def test_weight_zero_and_no_phrases_are_the_ngram_entry_bit_for_bit(dev, name):
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    x, lens = NC.make(name)
    lm = NgramLm.from_arpa(NC.text_of(name), num_classes=NC.CASES[name]["V"]).to(dev)
    _invariants(dev, NC.CASES[name], x.to(dev), lens.to(dev), lm)


@pytest.mark.parametrize("name", ["b_v8_changes", "b_v9_o3_changes"])
def test_batch_invariance(dev, name):
    c, x, lens, graph, lm = _case(dev, name)
    whole = _fused(c, x, lens, graph, lm)
    for b in range(c["B"]):
        alone = _fused(c, x[b:b + 1], lens[b:b + 1], graph, lm)
        for a, w in zip(alone, whole):
            assert torch.equal(a[0], w[b]), b
    both = _fused(c, x.flip(0).contiguous(), lens.flip(0).contiguous(), graph, lm)
    for a, w in zip(both, whole):
        assert torch.equal(a.flip(0), w)


# ------------------------------------------------------------------ 3. the class
@pytest.mark.parametrize("name", ["b_v7_midphrase", "b_v7_o3_midphrase", "b_v6_o3_overlap", "b_v63_o3_beam16_k16"])
def test_class_fused_path_is_the_module_loop(dev, name):
    from speech2text_amd.model.ctc_bias import CtcBiasPrefixBeamDecoding
    c, x, lens, _, _ = _case(dev, name)
    graph, lm = C.graph_of(name), C.model_of(name)          # on the CPU: they follow the logits
    dec = CtcBiasPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"],
                                    context=graph, context_weight=c["bias_weight"])
    fused = dec.beam_tokens(x, lens)
    assert graph.device == x.device and (lm is None or lm.device == x.device)
    loop = dec.beam_tokens(x, lens, fused=False)
    assert len(fused) == len(loop) == (4 if lm is None else 5) and fused[0].is_cuda and loop[0].is_cuda
    assert torch.equal(fused[0], loop[0]) and torch.equal(fused[1], loop[1])
    for a, b in zip(fused[2:], loop[2:]):
        assert C.rel_err(a, b) <= 1e-4
    ref = C.reference(name)
    assert dec.decode_batch(x, lens) == [r.tokens for r in ref]
    wide = CtcBiasPrefixBeamDecoding(_Ids(), beam_size=17, cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"],
                                     context=graph, context_weight=c["bias_weight"])
    assert wide._fused(x, lens) is None                    # a refused shape takes the host loop
    assert len(wide.beam_tokens(x[:1], lens[:1])) == len(fused)
