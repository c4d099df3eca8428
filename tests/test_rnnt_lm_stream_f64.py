"""CPU: the yardstick of the chunk-carried RNN-T beam search with RNN-LM shallow fusion (csrc/decode_lstm.hip
s2t_rnnt_beam_lstm_lm_chunk, s2t_rnnt_beam_stateless_lm_chunk) and the Python surface around it.

The chunked restatement of tests/rnnt_lm_stream_f64.py equals the whole-utterance one for every case of
tests/rnnt_lm_stream_cases.py and every cut, exactly; the six longer cases meet their conditions with no
exclusions; the new entry points are in the header with ctypes prototypes; their size functions and
refusals are pure host code (they precede any launch, so the library answers them without a GPU); the
Python classes refuse on the CPU what their docstrings say they refuse.
"""
import ctypes
import math

import pytest
import torch

import rnnt_lm_stream_cases as K
import rnnt_lm_stream_f64 as F
import rnnt_lstm_search_f64 as S

ENTRIES = [f"s2t_rnnt_{fam}_lm_stream_{what}" for fam in ("lstm", "stateless")
           for what in ("state_bytes", "workspace_bytes", "reset")] + \
    ["s2t_rnnt_beam_lstm_lm_chunk", "s2t_rnnt_beam_stateless_lm_chunk"]


# ------------------------------------------------------------------ 1. chunked == whole-utterance
@pytest.mark.parametrize("name", list(K.CASES))
def test_chunked_restatement_equals_the_whole_utterance_one(name):
    """tokens, frames, and the float64 score and lm_score exactly, for the cuts "1", "7", "16" and
    "irregular"; after every piece the best beam is the whole-utterance search's on the prefix (checked on
    the 7-frame cut of utterance 0)."""
    ref = K.reference(name)
    beam, topk, weight, start, _ = K.settings(name)
    for b, r in enumerate(ref):
        for how in K.PARTITIONS:
            tok, score, lm_score, frm, margin, stable, best = K.chunked(name, b, how)
            assert tok == r[0] and frm == r[3], (name, b, how)
            assert score == r[1] and lm_score == r[2], (name, b, how, score, r[1], lm_score, r[2])
            assert margin == r[4], (name, b, how)
            n = K.lengths(name)[b]
            assert len(stable) == len(F.cuts_of(n, how, seed=b)) - 1
            assert all(0 <= s <= len(t[0]) for s, t in zip(stable, best))
    n = K.lengths(name)[0]
    if name in K.STREAM_CASES and n:
        h, sd = K.hooks(name, torch.float64)
        am = K.make(name)[2][0]
        best = K.chunked(name, 0, "7")[6]
        for p, got in zip(F.cuts_of(n, "7")[1:], best):
            whole = F.chunked(am[:p], [0, p], h, beam, topk, sd, weight, start)
            assert got == (whole[0], whole[3], whole[1], whole[2]), (name, p)


# ------------------------------------------------------------------ 2. the longer cases' conditions
@pytest.mark.parametrize("name", K.NEW_CASES)
def test_longer_cases_meet_their_conditions(name):
    ref, f32, plain = K.reference(name), K.evaluate(name, torch.float32), K.evaluate(name, torch.float64, 0.0)
    lens = K.lengths(name)
    changed = 0
    for b, (r, s, u) in enumerate(zip(ref, f32, plain)):
        print(f"{name} utterance {b}: length {lens[b]} tokens {r[0]} (lm_weight 0: {u[0]}) lm_score {r[2]:.4f} "
              f"margin {r[4]:.3e}")
        assert r[4] >= S.MARGIN, f"{name} utterance {b}: float64 decides a node by {r[4]:.2e} only"
        assert s[0] == r[0] and s[3] == r[3], f"{name} utterance {b}: float32 walks another path"
        assert len(r[0]) == 0 if lens[b] == 0 else True
        changed += r[0] != u[0]
    assert changed >= 2, f"{name}: the LM changes {changed} utterances only"
    if name in K.LONG_CASES:
        frames = ref[0][3]
        assert lens[0] == 90 and min(frames) < 26 and max(frames) >= 64, (name, frames)
    else:
        inside = []
        for b in range(len(lens)):
            _, _, _, _, _, stable, best = K.chunked(name, b, "7")
            pairs = [(s, len(t[0])) for s, t in zip(stable, best)]
            print(f"{name} row {b}: (stable, length) at the 7-frame boundaries {pairs}")
            inside += [0 < s < n for s, n in pairs]
        assert any(inside), f"{name}: stable_len is trivial at every boundary"
        _, _, _, _, _, stable, best = K.chunked(name, 0, "7")
        assert any(0 < s < len(t[0]) for s, t in zip(stable, best)), f"{name} row 0"


def test_the_cases_are_the_imported_ones_and_the_six():
    import rnnt_lm_fusion_cases as L
    import rnnt_stateless_lm_cases as SL
    assert set(K.CASES) == set(L.CASES) | set(SL.CASES) | set(K.NEW_CASES) and len(K.NEW_CASES) == 6
    assert len(K.CASES) == len(L.CASES) + len(SL.CASES) + 6
    before = (dict(L.CASES), dict(SL.CASES))
    for name in K.NEW_CASES:
        K.make(name)
    assert (L.CASES, SL.CASES) == before                   # (a case is visible for the call only)
    for name in K.STREAM_CASES:
        assert K.settings(name)[4] == 40 and max(K.lengths(name)) == 40 and 0 in K.lengths(name)
    for name in K.LONG_CASES:
        assert K.settings(name)[4] == 90 and K.lengths(name) == [90, 0, 90]


# ------------------------------------------------------------------ 3. header, prototypes
def test_entry_points_are_in_the_header_with_prototypes():
    from speech2text_amd import _native as N
    protos = N.parse_header()
    for name in ENTRIES:
        assert name in protos, name
        ret, args = protos[name]
        assert ret is (ctypes.c_long if name.endswith("_bytes") else ctypes.c_int), name
    assert protos["s2t_rnnt_lstm_lm_stream_state_bytes"][1] == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3
    assert protos["s2t_rnnt_stateless_lm_stream_workspace_bytes"][1] == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3
    for fam in ("lstm", "stateless"):
        assert protos[f"s2t_rnnt_{fam}_lm_stream_reset"][1] == \
            [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
        chunk = protos[f"s2t_rnnt_beam_{fam}_lm_chunk"][1]
        assert chunk == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_int] + \
            [ctypes.c_void_p] * 10
    lib = N.lib()
    for name in ENTRIES:
        assert getattr(lib, name) is not None
    # the existing chunk entry points keep their prototypes
    assert len(protos["s2t_rnnt_beam_lstm_chunk"][1]) == 17 and len(protos["s2t_rnnt_lstm_stream_reset"][1]) == 8


# ------------------------------------------------------------------ 4. size functions and refusals: host code
def _descs(family, **change):
    """Descriptors with NULL parameters (never followed): a predictor / joiner pair and an LM, `change`
    applied (lm_X: the LM's field X)."""
    from speech2text_amd import _native as N
    if family == "lstm":
        d = N.struct("S2tRnntLstmDesc")()
        d.V, d.E, d.H, d.D, d.inner, d.num_layers, d.layer_norm, d.act = 11, 12, 8, 20, 0, 2, 1, 0
    else:
        d = N.struct("S2tRnntStatelessDesc")()
        d.V, d.E, d.D, d.ctx, d.inner, d.act = 11, 12, 20, 2, 0, 0
    lm = N.struct("S2tRnnLmDesc")()
    lm.V, lm.E, lm.H, lm.num_layers = 11, 8, 8, 1
    for k, v in change.items():
        if k.startswith("lm_"):
            setattr(lm, k[3:], v)
        elif hasattr(d, k):
            setattr(d, k, v)
    return d, lm


def _fns(family):
    from speech2text_amd import _native as N
    lib = N.lib()
    return (getattr(lib, f"s2t_rnnt_{family}_lm_stream_state_bytes"),
            getattr(lib, f"s2t_rnnt_{family}_lm_stream_workspace_bytes"),
            getattr(lib, f"s2t_rnnt_{family}_lm_stream_reset"), getattr(lib, f"s2t_rnnt_beam_{family}_lm_chunk"))


@pytest.mark.parametrize("family", ["lstm", "stateless"])
def test_size_functions_inside_the_limits(family):
    state_bytes, ws_bytes, _, _ = _fns(family)
    inside = [dict(), dict(V=8192, lm_V=8192), dict(V=1, lm_V=1), dict(inner=24), dict(lm_H=1024), dict(lm_E=1024),
              dict(lm_num_layers=8)] + ([dict(H=1024), dict(num_layers=8)] if family == "lstm" else
                                        [dict(ctx=64), dict(ctx=1)])
    for change in inside:
        d, lm = _descs(family, **change)
        pd, plm = ctypes.byref(d), ctypes.byref(lm)
        for beam in (1, 16):
            B, MT, R = 3, 10, 3 * beam
            n = state_bytes(pd, plm, B, beam, MT)
            pred = 2 * d.num_layers * R * d.H if family == "lstm" else R * d.ctx
            carried = pred + R * d.V + 2 * lm.num_layers * R * lm.H + R * lm.V + R + 4 * R * MT
            assert n > 0 and n % 256 == 0 and n >= 4 * carried, (change, beam)
            assert state_bytes(pd, plm, B, beam, 2 * MT) > n
            for Tc in (1, 7, 256):
                m = ws_bytes(pd, plm, B, Tc, beam)
                assert m > 0 and m % 256 == 0 and m >= 4 * (carried - R - 4 * R * MT + B * Tc * beam), (change, Tc)
            assert ws_bytes(pd, plm, B, 256, beam) >= ws_bytes(pd, plm, B, 7, beam) >= ws_bytes(pd, plm, B, 1, beam)
    # no argument of the state's size is a count of chunks or frames: the same call, the same bytes
    d, lm = _descs(family)
    assert len({state_bytes(ctypes.byref(d), ctypes.byref(lm), 2, 4, 10) for _ in range(3)}) == 1


_OUTSIDE = [dict(V=8193, lm_V=8193), dict(V=0, lm_V=0), dict(D=0), dict(inner=-1), dict(E=1025), dict(act=2),
            dict(lm_V=12), dict(lm_H=1028), dict(lm_H=6), dict(lm_E=1025), dict(lm_num_layers=9), dict(lm_num_layers=0),
            dict(no_lm=1), dict(start=11), dict(weight=math.inf), dict(weight=math.nan), dict(beam=17), dict(beam=0),
            dict(topk=0), dict(topk=17, V=32, lm_V=32), dict(Tc=0), dict(Tc=257), dict(mt=0), dict(no_ws=1),
            dict(no_state=1)]


@pytest.mark.parametrize("change", _OUTSIDE, ids=str)
@pytest.mark.parametrize("family", ["lstm", "stateless"])
def test_limits_just_outside_are_refused_before_any_launch(family, change):
    """Every refusal is made on the host from the descriptors' integers: the parameter pointers are NULL
    and the data pointers are not device memory, so a call that got past its checks would not return."""
    state_bytes, ws_bytes, reset, chunk = _fns(family)
    d, lm = _descs(family, **change)
    pd, plm = ctypes.byref(d), None if "no_lm" in change else ctypes.byref(lm)
    beam, topk, Tc, mt = change.get("beam", 4), change.get("topk", 4), change.get("Tc", 7), change.get("mt", 10)
    shape = any(k in change for k in ("V", "D", "inner", "E", "act", "beam", "no_lm")) or \
        any(k.startswith("lm_") for k in change)
    if "topk" not in change and (shape or "mt" in change):
        assert state_bytes(pd, plm, 3, beam, mt) == 0
    if "topk" not in change and (shape or "Tc" in change):
        assert ws_bytes(pd, plm, 3, Tc, beam) == 0
    st, ws = None if "no_state" in change else 1, None if "no_ws" in change else 1
    if not any(k in change for k in ("topk", "weight", "Tc")):
        assert reset(pd, plm, change.get("start", -1), st, None, 3, beam, mt, ws, None) == -1
    if "start" not in change:
        assert chunk(pd, plm, 1, 1, 3, Tc, beam, topk, change.get("weight", 0.3), mt, st, ws, 1, 1, 1, 1, 1, 1, 1,
                     None) == -1


@pytest.mark.parametrize("family", ["lstm", "stateless"])
def test_empty_batches(family):
    state_bytes, ws_bytes, reset, chunk = _fns(family)
    d, lm = _descs(family)
    pd, plm = ctypes.byref(d), ctypes.byref(lm)
    assert state_bytes(pd, plm, 0, 4, 10) == 0 and ws_bytes(pd, plm, 0, 7, 4) == 0
    assert state_bytes(None, plm, 3, 4, 10) == 0 and ws_bytes(pd, None, 3, 7, 4) == 0
    assert reset(pd, plm, -1, 1, None, 0, 4, 10, 1, None) == 0                                   # B = 0
    assert chunk(pd, plm, 1, 1, 0, 7, 4, 4, 0.3, 10, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == 0


# ------------------------------------------------------------------ 5. the Python classes on the CPU
def _lstm_pair(V=11):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    pred = Predictor({"model": "Lstm", "config": {"num_symbols": V, "output_dim": 20, "symbol_embedding_dim": 12,
                                                  "num_lstm_layers": 1, "lstm_hidden_dim": 8, "lstm_layer_norm": True,
                                                  "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}})
    return pred, Joiner(JoinerConfig(input_dim=20, output_dim=V, inner_dim=1, activation="relu", use_out_project=False))


def _stateless_pair(V=11, inner=0):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": 20, "symbol_embedding_dim": 12,
                                                       "context_size": 2}})
    return pred, Joiner(JoinerConfig(input_dim=20, output_dim=V, inner_dim=max(inner, 1), activation="relu",
                                     use_out_project=inner > 0))


def _rnn_lm(V=11):
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    return RnnLm(config=RnnLmConfig(num_symbols=V, symbol_embedding_dim=8, num_rnn_layer=1)).eval()


def test_classes_refuse_on_the_cpu_what_their_docstrings_say():
    import rnnt_lm_fusion_cases as L
    import rnnt_lm_fusion_f64 as FF
    from speech2text_amd.model.decoding import (RnntLstmStreamingSearch, RnntStatelessLmStreamingSearch,
                                                rnnt_streaming_search)
    lm = _rnn_lm()
    foreign = FF.PlainLm(L.lm_weights("lm20_v11", 0))
    p, j = _lstm_pair()
    sp, sj = _stateless_pair(inner=24)
    with pytest.raises(ValueError, match="greedy"):
        RnntLstmStreamingSearch(p, j, 2, "greedy", lm=lm)
    with pytest.raises(ValueError, match="greedy"):
        rnnt_streaming_search(p, j, 2, "greedy", lm=lm)
    with pytest.raises(ValueError, match="RnnLm"):
        RnntLstmStreamingSearch(p, j, 2, "beam", lm=foreign)
    with pytest.raises(ValueError, match="lm_start_token"):
        RnntLstmStreamingSearch(p, j, 2, "beam", lm=lm, lm_start_token=-2)
    with pytest.raises(ValueError, match="finite"):
        RnntLstmStreamingSearch(p, j, 2, "beam", lm=lm, lm_weight=math.nan)
    with pytest.raises(RuntimeError, match="GPU"):                       # CPU modules
        RnntLstmStreamingSearch(p, j, 2, "beam", lm=lm, lm_weight=0.3)
    with pytest.raises(ValueError, match="needs an lm"):
        RnntStatelessLmStreamingSearch(sp, sj, 2, "beam")
    with pytest.raises(ValueError, match="greedy"):
        RnntStatelessLmStreamingSearch(sp, sj, 2, "greedy", lm=lm)
    with pytest.raises(ValueError, match="greedy"):
        rnnt_streaming_search(sp, sj, 2, "greedy", lm=lm)
    with pytest.raises(ValueError, match="RnnLm"):
        RnntStatelessLmStreamingSearch(sp, sj, 2, "beam", lm=foreign)
    with pytest.raises(ValueError, match="StatelessPredictor"):
        RnntStatelessLmStreamingSearch(p, j, 2, "beam", lm=lm)
    with pytest.raises(ValueError, match="method"):
        RnntStatelessLmStreamingSearch(sp, sj, 2, "viterbi", lm=lm)
    with pytest.raises(RuntimeError, match="GPU"):                       # CPU modules
        RnntStatelessLmStreamingSearch(sp, sj, 2, "beam", lm=lm)
    with pytest.raises(RuntimeError, match="GPU"):                       # the factory reaches the same class
        rnnt_streaming_search(sp, sj, 2, "beam", lm=lm, lm_weight=0.5)
    with pytest.raises(ValueError, match="output projection"):          # without an LM: today's class and refusal
        rnnt_streaming_search(sp, sj, 2, "beam")
