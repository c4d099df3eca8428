"""CPU: the back-off n-gram LM of model/lm/ngram_lm.py: the ARPA reader against a dict-based back-off
evaluation of the same text (tests/ctc_ngram_f64.py DictNgram, a parser and an evaluation of its own), the
to_arpa round trip, malformed files, the estimator's normalisation, the validation of hand-made tables,
the state invariant, the host loops' LM protocol and the YAML section that builds the model.
"""
import copy

import numpy as np
import pytest
import torch

import ctc_ngram_cases as C
import ctc_ngram_f64 as G
from speech2text_amd.model.lm.ngram_lm import BOS, NgramLm
from task_support import _base_cfg, _CONF, _TOK, _V

# order 3, pieces as words; `d` and the blank have no unigram; `c` is a context without a back-off column,
# `<unk>` has a back-off and nothing after it; three entries predict </s>
_IDS = {"<blank_id>": 0, "<unk>": 1, "▁a": 2, "b": 3, "c": 4, "d": 5}
_ARPA = """
\\data\\
ngram 1=6
ngram 2=6
ngram 3=3

\\1-grams:
-99\t<s>\t-0.30
-1.0\t</s>
-1.2\t<unk>\t-0.25
-0.5\t▁a\t-0.40
-0.7\tb\t-0.35
-0.9\tc

\\2-grams:
-0.3\t<s> ▁a\t-0.20
-0.4\t▁a b\t-0.15
-0.6\tb c
-0.8\tb </s>
-0.5\tc ▁a
-1.1\t▁a <unk>

\\3-grams:
-0.2\t<s> ▁a b
-0.25\t▁a b c
-0.9\t▁a b </s>

\\end\\
"""
_TABLES = NgramLm._TABLES


def _hand(dtype=torch.float32, **kw):
    return NgramLm.from_arpa(_ARPA, token_to_id=_IDS, num_classes=6, dtype=dtype, **kw)


# ------------------------------------------------------------------ 1. the reader
def test_hand_written_arpa_is_the_dict_evaluation_of_its_text():
    lm = _hand(torch.float64)
    ref = G.DictNgram(_ARPA, 6, token_to_id=_IDS)
    a, b, c = _IDS["▁a"], _IDS["b"], _IDS["c"]
    assert lm.order == 3 and lm.num_classes == 6 and lm.dtype == torch.float64
    assert set(lm.contexts) == {(), (BOS,), (1,), (a,), (b,), (c,), (BOS, a), (a, b)}
    assert lm.contexts[0] == () and lm.contexts[lm.start_ctx] == (BOS,)
    assert lm.num_arcs == 6 + 5 + 2                        # the dense root; nothing predicts </s> or <s>
    for n, h in enumerate(lm.contexts):
        hist = tuple(G.BOS if x == BOS else x for x in h)
        for cls in range(6):
            got, nxt = lm.score(n, cls)
            assert float(got) == pytest.approx(float(ref.score_in(hist, cls)[0]), abs=1e-12), (h, cls)
            full = h + (cls,)                              # next: the longest suffix that is a context
            want = next(full[i:] for i in range(len(full) - 2, len(full) + 1) if full[i:] in lm.contexts)
            assert lm.contexts[nxt] == want, (h, cls)
            assert lm._row(n)[0][cls] == got and lm._row(n)[1][cls] == nxt
    ln10 = np.log(10.0)
    assert float(lm.score(0, 5)[0]) == -30.0 and float(lm.score(0, 0)[0]) == -30.0       # no unigram
    assert float(_hand(torch.float64, missing_logp=-12.5).score(0, 5)[0]) == -12.5
    assert float(lm.score(0, 1)[0]) == pytest.approx(-1.2 * ln10)                        # <unk> has an id here
    # (a, b) does not list d: back off through (a, b) and (b,) to the root
    ab = lm.contexts.index((a, b))
    assert float(lm.score(ab, 5)[0]) == pytest.approx(-0.15 * ln10 + -0.35 * ln10 + -30.0)
    assert float(lm.score(lm.contexts.index((c,)), b)[0]) == pytest.approx(-0.7 * ln10)   # no back-off column: 0
    total, state = 0.0, lm.start_ctx                       # <s> a b c: every token at the highest order
    for tok in (a, b, c):
        lp, state = lm.score(state, tok)
        total += float(lp)
    assert total == pytest.approx((-0.3 - 0.2 - 0.25) * ln10)


def test_float32_tables_and_round_trip_through_to_arpa():
    lm = _hand()
    assert lm.dtype == torch.float32 and lm.ctx_begin.dtype == torch.int32 and lm.arc_next.dtype == torch.int32
    back = NgramLm.from_arpa(lm.to_arpa(), token_to_id=_IDS, num_classes=6)
    for k in _TABLES:
        assert torch.equal(getattr(lm, k), getattr(back, k)), k
    assert back.contexts == lm.contexts and back.start_ctx == lm.start_ctx
    for name in C.CASES:
        c = C.CASES[name]
        est = NgramLm.estimate(C.lm_sequences(c["V"], c["n_tokens"], c["lm_seed"]), c["V"], order=c["order"])
        for k in _TABLES:
            assert torch.equal(getattr(est, k), getattr(C.model(name), k)), (name, k)


def test_unk_without_an_id_and_files_from_a_path(tmp_path):
    ids = {k: v for k, v in _IDS.items() if k != "<unk>"}
    lm = NgramLm.from_arpa(_ARPA, token_to_id=ids, num_classes=6)
    assert float(lm.score(0, 1)[0]) == -30.0 and (1,) not in lm.contexts
    path = tmp_path / "lm.arpa"
    path.write_text(_ARPA, encoding="utf-8")
    again = NgramLm.from_arpa(str(path), token_to_id=ids, num_classes=6)
    for k in _TABLES:
        assert torch.equal(getattr(lm, k), getattr(again, k))

    class _Tok:
        labels = list(_IDS)
    by_tok = NgramLm.from_arpa(path, tokenizer=_Tok())
    assert by_tok.num_classes == 6 and torch.equal(by_tok.arc_logp, _hand().arc_logp)


@pytest.mark.parametrize("change, what", [
    (("\\data\\", "\\date\\"), "line 2"),
    (("-0.6\tb c", "-0.x6\tb c"), "line 18"),
    (("-0.6\tb c", "-0.6\tb"), "line 18"),
    (("-0.6\tb c", "-0.6\tb c -0.1 -0.2"), "line 18"),
    (("-0.6\tb c", "-inf\tb c"), "line 18"),
    (("-0.6\tb c", "-0.6\tb e"), "line 18"),
    (("-0.6\tb c", "-0.6\tb <s>"), "line 18"),
    (("-0.6\tb c", "-0.4\t▁a b"), "line 18"),
    (("\\3-grams:", "\\4-grams:"), "line 23"),
    (("\\3-grams:", "\\three:"), "line 23"),
    (("ngram 3=3", "ngram 9=3"), "line 5"),
    (("ngram 3=3", "ngram three"), "line 5"),
    (("ngram 3=3", "ngram 3=4"), "section 3"),
    (("\\end\\", ""), "end"),
    (("\\end\\", "\\end\\\nmore"), "line 29"),
], ids=lambda v: v[1][:14] if isinstance(v, tuple) else None)
def test_malformed_files_raise_value_error(change, what):
    text = _ARPA.replace(*change)
    assert text != _ARPA
    with pytest.raises(ValueError, match=what):
        NgramLm.from_arpa(text, token_to_id=_IDS, num_classes=6)


def test_missing_names_and_empty_text():
    with pytest.raises(ValueError):
        NgramLm.from_arpa(_ARPA)
    with pytest.raises(ValueError, match="data"):
        NgramLm.from_arpa("\n\n", num_classes=6)


# ------------------------------------------------------------------ 2. the estimator
@pytest.mark.parametrize("V, order, n", [(3, 3, 60), (11, 2, 120), (63, 5, 300), (128, 1, 300), (300, 3, 400),
                                         (2, 2, 60), (6, 8, 100)])
def test_estimate_is_normalised_in_every_context(V, order, n):
    """sum_c exp(score(ctx, c)) = 1: a property of back-off with discounting, not a measurement."""
    lm = NgramLm.estimate(C.lm_sequences(V, n, 0), V, order=order, dtype=torch.float64)
    assert lm.order == order and lm.dtype == torch.float64
    depth = max(len(h) for h in lm.contexts)
    assert depth == order - 1
    for ctx in range(lm.num_ctx):
        total = float(np.exp(lm._row(ctx)[0]).sum())
        assert abs(total - 1.0) <= 1e-9, (lm.contexts[ctx], total)


def test_estimate_argument_checks():
    for kw in (dict(order=0), dict(order=9), dict(discount=0.0), dict(discount=1.0)):
        with pytest.raises(ValueError):
            NgramLm.estimate([[1, 2]], 3, **kw)
    with pytest.raises(ValueError):
        NgramLm.estimate([[1, 3]], 3)


# ------------------------------------------------------------------ 3. validation
def _parts(lm):
    return dict(num_classes=lm.num_classes, order=lm.order, start_ctx=lm.start_ctx,
                **{k: getattr(lm, k).clone() for k in _TABLES})


def test_validation_rejects_what_the_kernel_would_trust():
    lm = C.model("n_v11_o2_b17_beam4_k3")
    deep = C.model("n_v63_o5_beam16_k16")
    NgramLm(**_parts(lm))                                  # the parts as they are: accepted
    wide = next(n for n in range(1, lm.num_ctx) if lm.ctx_begin[n + 1] - lm.ctx_begin[n] >= 2)
    first = int(lm.ctx_begin[wide])

    def broken(src=lm, **kw):
        p = _parts(src)
        for k, (i, v) in kw.items():
            if k in ("order", "start_ctx"):
                p[k] = v
            else:
                p[k][i] = v
        return p

    swapped = _parts(lm)
    swapped["arc_token"][first], swapped["arc_token"][first + 1] = lm.arc_token[first + 1], lm.arc_token[first]
    d4 = next(n for n, h in enumerate(deep.contexts) if len(h) == 4)
    d2 = next(n for n, h in enumerate(deep.contexts) if len(h) == 2)
    for what, p in [("sorted", swapped),
                    ("sorted", broken(arc_token=(first + 1, int(lm.arc_token[first])))),          # a duplicate
                    ("next", broken(arc_next=(3, lm.num_ctx))),
                    ("next", broken(arc_next=(3, -1))),
                    ("shorten", broken(ctx_fail=(wide, wide))),
                    ("shorten", broken(deep, ctx_fail=(d2, d4))),                                 # to a deeper one
                    ("fail link", broken(ctx_fail=(wide, lm.num_ctx))),
                    ("dense", broken(arc_token=(2, 3))),
                    ("token", broken(arc_token=(first, 11))),
                    ("ctx_begin", broken(ctx_begin=(1, 10))),
                    ("ctx_begin", broken(ctx_begin=(lm.num_ctx, lm.num_arcs + 1))),
                    ("finite", broken(arc_logp=(0, float("-inf")))),
                    ("finite", broken(ctx_backoff=(1, float("nan")))),
                    ("start_ctx", broken(start_ctx=(0, lm.num_ctx))),
                    ("order", broken(order=(0, 9))),
                    ("shorten", broken(deep, order=(0, 3)))]:
        with pytest.raises(ValueError, match=what):
            NgramLm(**p)


# ------------------------------------------------------------------ 4. the state, the protocol
@pytest.mark.parametrize("name", ["n_v3_o3_beam4_kV", "n_v11_o2_b17_beam4_k3", "n_v63_o5_beam16_k16",
                                  "n_v128_o1_beam1_k1"])
def test_state_is_the_longest_suffix_that_is_a_context(name):
    lm = C.model(name)
    V = lm.num_classes
    ids = {h: n for n, h in enumerate(lm.contexts)}
    g = torch.Generator().manual_seed(3)
    train = C.lm_sequences(V, C.CASES[name]["n_tokens"], C.CASES[name]["lm_seed"])
    deepest = 0
    for trial in range(40):
        seq = torch.randint(0, V, (12,), generator=g).tolist()
        if trial % 2:                                      # half of them walk the training text, then leave it
            seq = train[trial % len(train)][:8] + seq[:4]
        state, hist = lm.start_ctx, (BOS,)
        for tok in seq:
            _, state = lm.score(state, tok)
            hist = hist + (tok,)
            want = next(hist[i:] for i in range(max(0, len(hist) - (lm.order - 1)), len(hist) + 1) if hist[i:] in ids)
            assert lm.contexts[state] == want, (seq, hist)
            deepest = max(deepest, len(want))
    assert deepest == lm.order - 1


def test_lm_protocol_of_the_host_loops():
    lm = C.model("n_v63_o5_beam16_k16")
    V = lm.num_classes
    st = lm.init_states(3)
    assert st.dtype == torch.int64 and st.tolist() == [lm.start_ctx] * 3
    q0 = lm.start_scores(st)
    assert q0.shape == (3, V) and q0.dtype == torch.float32
    assert torch.equal(q0[1], torch.from_numpy(lm._row(lm.start_ctx)[0]))
    toks = torch.tensor([5, 9, 62])
    q, new = lm.score_step(toks, st)
    assert q.shape == (3, V) and new.dtype == torch.int64
    for r in range(3):
        assert int(new[r]) == lm.score(lm.start_ctx, int(toks[r]))[1]
        for c in (0, 1, 17, 62):
            assert float(q[r, c]) == float(lm.score(int(new[r]), c)[0])
    assert lm.to("cpu") is lm


def test_classes_refuse_what_is_not_fused():
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding, CtcStreamingSearch
    lm = C.model("n_v11_o2_b17_beam4_k3")

    class _Ids:
        def decode(self, t):
            return [int(x) for x in t]
    with pytest.raises(ValueError, match="lm_start_token"):
        CtcPrefixBeamDecoding(_Ids(), lm=lm, lm_weight=0.5, lm_start_token=3)
    assert CtcPrefixBeamDecoding(_Ids(), lm=lm, lm_weight=0.5)._lm is lm
    with pytest.raises(ValueError, match="NgramLm"):
        CtcStreamingSearch(11, lm=lm, lm_weight=0.5)


# ------------------------------------------------------------------ 5. the YAML section
def _ctc_cfg():
    cfg = _base_cfg()
    cfg.update({"task": {"type": "CTC"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Projector", "config": {"input_dim": 64, "output_dim": _V, "dropout_p": 0.1}},
                "loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean", "zero_infinity": True}},
                "metric": {"decode_method": "ctc_prefix_beam_search", "beam_size": 3, "cutoff_top_k": 3,
                           "lm_weight": 0.4}})
    return cfg, _V


def test_yaml_arpa_section_builds_an_ngram_lm_and_config_still_an_rnn_lm(tmp_path):
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding
    from speech2text_amd.model.lm.rnn_lm import RnnLm
    cfg, V = _ctc_cfg()
    plain = TaskFactory.get("CTC")(copy.deepcopy(cfg))
    labels = plain._tokenizer.labels
    est = NgramLm.estimate(C.lm_sequences(V, 200, 4), V, order=3)
    est.names = list(labels)
    path = tmp_path / "pieces.arpa"
    path.write_text(est.to_arpa(), encoding="utf-8")
    cfg_n = copy.deepcopy(cfg)
    cfg_n["metric"]["lm"] = {"arpa": str(path), "missing_logp": -20.0}
    task = TaskFactory.get("CTC")(cfg_n)
    sess = task._metric._decode_sess
    assert isinstance(sess, CtcPrefixBeamDecoding) and isinstance(sess._lm, NgramLm)
    assert (sess._lm_weight, sess._beam_size, sess._cutoff_top_k) == (0.4, 3, 3)
    assert sess._lm.num_classes == V == len(labels) and sess._lm.names == list(labels)
    for k in _TABLES:                                      # (every class has a unigram: missing_logp enters nowhere)
        assert torch.equal(getattr(sess._lm, k), getattr(est, k)), k
    assert list(task.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError, match="n-gram"):
        task.streaming_recognizer()
    cfg_r = copy.deepcopy(cfg)
    cfg_r["metric"]["lm"] = {"config": {"num_symbols": V, "symbol_embedding_dim": 16, "num_rnn_layer": 1},
                             "checkpoint": None}
    assert isinstance(TaskFactory.get("CTC")(cfg_r)._metric._decode_sess._lm, RnnLm)
    cfg_b = copy.deepcopy(cfg_n)
    cfg_b["metric"]["lm"]["config"] = {"num_symbols": V}
    with pytest.raises(ValueError, match="either"):
        TaskFactory.get("CTC")(cfg_b)
