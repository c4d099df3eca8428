"""CPU: ContextGraph (model/lm/context_graph.py), the hotword phrases compiled to an Aho-Corasick automaton
in the n-gram's table form, against the statement on whole histories as tests/ctc_bias_f64.py evaluates it
(slices of the history against slices of the phrases: no trie, no fail links): for every reachable state
and every class, `score` / `_row` add what bias_sum gains and lead to the state of the longer history, and
`final_scores` is what separates bias_sum from final_bias.  Then what `validate()` refuses, the limits of
the constructor, the protocol, and the C entries' refusals (they return before any launch, so they need
the library and no GPU).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import ctc_bias_cases as C
import ctc_bias_f64 as H

from speech2text_amd import _native as N
from speech2text_amd.model.lm.context_graph import ContextGraph, max_depth_limit


def _graph(name, dtype=torch.float64):
    phrases, V, cs, scores = C.GRAPHS[name]
    dt = {torch.float64: np.float64, torch.float32: np.float32}[dtype]
    return ContextGraph(phrases, V, context_score=cs, phrase_scores=scores, dtype=dtype), \
        H.Hotwords(phrases, cs, scores, dtype=dt), V


@pytest.mark.parametrize("name", list(C.GRAPHS))
def test_tables_are_the_history_statement(name):
    g, hot, V = _graph(name)
    assert g.states[0] == () and len(set(g.states)) == g.num_ctx == len(g.states)
    assert g.max_depth == max(len(h) for h in g.states) <= max_depth_limit()
    for n, h in enumerate(g.states):                       # every reachable state, by the history that names it
        assert hot.match_len(h) == len(h)                  # (a state is a suffix that begins a phrase)
        row, nxt = g._row(n)
        assert float(g.final_scores(torch.tensor([n]))[0]) == float(hot.final_bias(h) - hot.bias_sum(h))
        for c in range(V):
            ext = h + (c,)
            want = float(hot.bias_sum(ext) - hot.bias_sum(h))
            score, to = g.score(n, c)
            assert float(score) == pytest.approx(want, abs=1e-12), (name, h, c)
            assert g.states[to] == ext[len(ext) - hot.match_len(ext):], (name, h, c)
            assert float(row[c]) == float(score) and int(nxt[c]) == to
    # along a walk the sums telescope to the statement on the whole history, as the searches use them
    rng = np.random.default_rng(3)
    for _ in range(20):
        walk = tuple(int(t) for t in rng.integers(0, V, size=30))
        state, total = 0, 0.0
        for k, c in enumerate(walk):
            s, state = g.score(state, c)
            total += float(s)
            assert total == pytest.approx(float(hot.bias_sum(walk[:k + 1])), abs=1e-9)
        assert total + float(g.ctx_final[state]) == pytest.approx(float(hot.final_bias(walk)), abs=1e-9)


def test_named_graphs_are_what_they_are_named_for():
    g, hot, _ = _graph("overlap")
    assert float(hot.final_bias((1, 2, 3))) == 0.75 + 2.5   # [2, 3] ends inside the match of [1, 2, 3, 4]
    assert float(hot.bias_sum((1, 2, 3))) == 3.0 + 0.75 + 2.5
    assert g.states[g.score(g.states.index((1, 2)), 3)[1]] == (1, 2, 3)
    g, hot, _ = _graph("twice")
    assert float(hot.final_bias((2, 3))) == 1.75 + 0.5      # listed twice: once, with its first score
    g, _, V = _graph("deepest")
    assert g.max_depth == max_depth_limit() == N.const("S2T_CONTEXT_MAX_DEPTH") == 64 and g.num_ctx == 65
    g, _, V = _graph("empty")
    assert g.num_ctx == 1 and g.num_arcs == V and g.max_depth == 0
    assert not g.arc_score.any() and not g.arc_next.any() and g.score(0, V - 1) == (0.0, 0)
    g, _, V = _graph("one")                                 # a root arc of a class no phrase starts with
    assert [float(g.arc_score[c]) for c in range(V)] == [0.0, 0.0, 1.0, 0.0, 0.0] and g.arc_next[:V].tolist()[2] == 1


def test_fp32_tables_hold_the_same_values():
    for name in C.GRAPHS:
        a, b = _graph(name, torch.float32)[0], _graph(name, torch.float64)[0]
        assert a.dtype == torch.float32 and a.ctx_begin.dtype == torch.int32
        for k in ContextGraph._TABLES:
            assert torch.equal(getattr(a, k).double(), getattr(b, k).double()), (name, k)


def _broken(change):
    g = _graph("shared_prefix")[0]
    change(g)
    return g


def test_validate_refuses_what_the_kernels_trust():
    _graph("shared_prefix")[0].validate()
    V = 6

    def unsorted(g):
        n = g.states.index((1,))
        lo = int(g.ctx_begin[n])
        g.arc_token[lo], g.arc_token[lo + 1] = g.arc_token[lo + 1].clone(), g.arc_token[lo].clone()

    def sparse_root(g):
        g.arc_token[2] = 3

    def short_root(g):
        g.ctx_begin[1] = V - 1

    def deeper_fail(g):
        g.ctx_fail[g.states.index((1,))] = g.states.index((1, 2))

    def self_fail(g):
        n = g.states.index((1, 2))
        g.ctx_fail[n] = n

    for change, what in ((unsorted, "sorted by token"), (sparse_root, "root is dense"), (short_root, "exactly V arcs"),
                         (deeper_fail, "shallower"), (self_fail, "shallower")):
        with pytest.raises(ValueError, match=what):
            _broken(change).validate()
    with pytest.raises(ValueError, match="loans"):
        _broken(lambda g: g.ctx_backoff.__setitem__(1, 0.25)).validate()
    with pytest.raises(ValueError, match="outside"):
        _broken(lambda g: g.arc_next.__setitem__(0, 99)).validate()


def test_constructor_limits():
    with pytest.raises(ValueError, match="S2T_CONTEXT_MAX_DEPTH"):
        ContextGraph([[1] * 65], 4)
    ContextGraph([[1] * 64], 4)
    for bad in ([[4]], [[-1]], [[1, 2, 7]]):
        with pytest.raises(ValueError, match="outside"):
            ContextGraph(bad, 4)
    with pytest.raises(ValueError, match="empty"):
        ContextGraph([[1], []], 4)
    with pytest.raises(ValueError, match="one score per phrase"):
        ContextGraph([[1], [2]], 4, phrase_scores=[1.0])
    with pytest.raises(ValueError, match="finite"):
        ContextGraph([[1]], 4, context_score=math.inf)
    with pytest.raises(RuntimeError, match="GPU"):
        ContextGraph([[1]], 4).desc()


def test_protocol_and_from_texts():
    g, hot, V = _graph("shared_prefix")
    st = g.init_states(3)
    assert st.tolist() == [0, 0, 0] and st.dtype == torch.int64
    rows, new = g.score_step(torch.tensor([1, 5, 1]), st)
    assert [g.states[n] for n in new.tolist()] == [(1,), (), (1,)] and rows.shape == (3, V)
    assert torch.equal(rows[0], torch.from_numpy(g._row(int(new[0]))[0]))
    assert torch.equal(g.start_scores(st)[1], torch.from_numpy(g._row(0)[0]))
    assert g.final_scores(new).tolist() == [-0.5, 0.0, -0.5]

    class Tok:
        labels = ["_", "a", "b", "c"]

        def encode(self, text):
            return [self.labels.index(ch) for ch in text]

    t = ContextGraph.from_texts(["ab", "c"], Tok(), context_score=2.0)
    assert t.num_classes == 4 and t.states == [(), (1,), (3,), (1, 2)]
    assert t.to("cpu") is t


# ------------------------------------------------------------------ the C entries' refusals: no launch, no GPU
_V = 8


def _desc(g):
    """A descriptor over host tables: a refusing entry follows none of its pointers."""
    d = N.struct("S2tContextGraphDesc")()
    d.V, d.max_depth, d.num_ctx, d.num_arcs = g.num_classes, g.max_depth, g.num_ctx, g.num_arcs
    for k in ContextGraph._TABLES:
        setattr(d, k, getattr(g, k).data_ptr())
    return d


def _lm_desc(lm):
    d = N.struct("S2tNgramLmDesc")()
    d.V, d.order, d.num_ctx, d.num_arcs = lm.num_classes, lm.order, lm.num_ctx, lm.num_arcs
    for k in lm._TABLES:
        setattr(d, k, getattr(lm, k).data_ptr())
    return d


@pytest.mark.parametrize("change", [dict(graph=None), dict(gV=_V + 1), dict(max_depth=-1), dict(max_depth=65),
                                    dict(num_ctx=0), dict(num_arcs=_V - 1), dict(weight=math.inf),
                                    dict(weight=math.nan), dict(bias_score=None), dict(beam=17), dict(ws=None),
                                    dict(null="ctx_begin"), dict(null="ctx_fail"), dict(null="ctx_backoff"),
                                    dict(null="ctx_final"), dict(null="arc_token"), dict(null="arc_score"),
                                    dict(null="arc_next")], ids=str)
def test_entries_refuse_before_any_launch(change):
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    lib = N.lib()
    g = ContextGraph([[1, 2], [3]], _V)
    lm = NgramLm.from_arpa(C.lm_text(_V, 2), num_classes=_V)
    d, ld = _desc(g), _lm_desc(lm)
    if "gV" in change:
        d.V = change["gV"]
    for k in ("max_depth", "num_ctx", "num_arcs"):
        if k in change:
            setattr(d, k, change[k])
    if "null" in change:
        setattr(d, change["null"], None)
    gd = None if "graph" in change else ctypes.byref(d)
    host = torch.zeros(64)                                  # stands in for every buffer: nothing reads or writes it
    p = host.data_ptr()
    beam, w = change.get("beam", 4), change.get("weight", 1.0)
    ws = None if "ws" in change else p
    bs = None if "bias_score" in change else p
    assert lib.s2t_ctc_prefix_beam_bias(gd, p, p, 1, 2, _V, 0, beam, 3, w, ws, p, p, p, bs, None) == -1
    assert lib.s2t_ctc_prefix_beam_ngram_bias(ctypes.byref(ld), gd, p, p, 1, 2, _V, 0, beam, 3, 0.5, 0, w, ws, p, p, p,
                                              p, bs, None) == -1
    st = None if "ws" in change else p
    assert lib.s2t_ctc_prefix_beam_bias_chunk(gd, p, p, 1, 2, _V, 0, beam, 3, w, 8, 64, st, p, p, p, bs, p, p,
                                              None) == -1
    assert lib.s2t_ctc_prefix_beam_ngram_bias_chunk(ctypes.byref(ld), gd, p, p, 1, 2, _V, 0, beam, 3, 0.5, w, 8, 64, st,
                                                    p, p, p, p, bs, p, p, None) == -1
    if {"graph", "max_depth", "num_ctx", "num_arcs", "null"} & set(change):   # the look-up's own entry refuses them too
        assert lib.s2t_context_score(gd, 4, p, p, p, p, None) == -1
    assert not host.any()


def test_partner_refusals_sizes_and_empty_batches():
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    lib = N.lib()
    g = ContextGraph([[1, 2], [3]], _V)
    d = _desc(g)
    gd = ctypes.byref(d)
    host = torch.zeros(64)
    p = host.data_ptr()
    ld = _lm_desc(NgramLm.from_arpa(C.lm_text(_V, 2), num_classes=_V))
    # what the n-gram partner refuses of its own arguments
    for lmd, lw, start in ((None, 0.5, 0), (ctypes.byref(ld), math.nan, 0), (ctypes.byref(ld), 0.5, -1),
                           (ctypes.byref(ld), 0.5, ld.num_ctx)):
        assert lib.s2t_ctc_prefix_beam_ngram_bias(lmd, gd, p, p, 1, 2, _V, 0, 4, 3, lw, start, 1.0, p, p, p, p, p, p,
                                                  None) == -1
    assert lib.s2t_ctc_prefix_beam_ngram_bias(ctypes.byref(ld), gd, p, p, 1, 2, _V, 0, 4, 3, 0.5, 0, 1.0, p, p, p, p,
                                              None, p, None) == -1            # lm_score NULL
    assert lib.s2t_ctc_prefix_beam_bias(gd, p, p, 1, 2, _V, _V, 4, 3, 1.0, p, p, p, p, p, None) == -1     # blank
    assert lib.s2t_ctc_prefix_beam_bias_chunk(gd, p, p, 1, 257, _V, 0, 4, 3, 1.0, 8, 64, p, p, p, p, p, p, p,
                                              None) == -1                     # Tc
    assert lib.s2t_ctc_bias_stream_reset(None, None, 1, _V, 4, 64, None) == -1
    assert lib.s2t_ctc_ngram_bias_stream_reset(p, None, 1, _V, 4, 64, -1, None) == -1
    # B <= 0 returns 0; the sizes: the partner's layout and two arrays of R behind it
    assert lib.s2t_ctc_prefix_beam_bias(None, None, None, 0, 2, _V, 0, 99, 99, 1.0, None, None, None, None, None,
                                        None) == 0
    assert lib.s2t_context_score(None, 0, None, None, None, None, None) == 0
    for B, beam in ((1, 4), (3, 16), (40, 16)):
        extra = 2 * (-(-4 * B * beam // 256) * 256)
        assert lib.s2t_ctc_bias_stream_state_bytes(B, _V, beam, 64) == \
            lib.s2t_ctc_stream_state_bytes(B, _V, beam, 64) + extra
        assert lib.s2t_ctc_ngram_bias_stream_state_bytes(B, _V, beam, 64) == \
            lib.s2t_ctc_ngram_stream_state_bytes(B, _V, beam, 64) + extra
    assert lib.s2t_ctc_bias_stream_state_bytes(1, _V, 17, 64) == 0
    assert lib.s2t_ctc_ngram_bias_stream_state_bytes(0, _V, 4, 64) == 0
    assert not host.any()
