"""CPU: the conditions of tests/rnnt_bias_cases.py, the restatement of tests/rnnt_bias_f64.py against an exhaustive
search, the host side of hotword biasing in the RNN-T beam search (model/rnnt_bias.py RnntBiasBeamDecoding over
model/decoding.py RnntBeamDecoding._module_loop / _module_loop_lm, rnnt_bias_streaming_search) and what the eight C
entries of csrc/decode_rnnt.hip refuse, called without a device.

    1. every utterance of every case is decided by at least 1e-3 at every ranking cut and at the finalisation's
       pick in float64, the float32 run walks the same tokens and frames, with beam > 1 the bias changes a
       hypothesis, every named event occurs in a case of each entry, the long cases report a beam other than
       position 0; the recorded float32 figures still cover what is measured
    2. at (V 2, T 4) and (V 3, T 2), beam 16 and top-k V, the search drops nothing: its reported hypothesis is
       the arg-max over all V^T frame labellings of path log-probability + lm_weight x the dict n-gram's score +
       bias_weight x final_bias of the emitted tokens, independently of the restatement's own loop
    3. RnntBiasBeamDecoding on CPU tensors is the restatement; without a context it is RnntBeamDecoding bit for
       bit; the argument errors of the new classes
    4. the refusals and size queries of the eight entries
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import ctc_ngram_f64 as G
import rnnt_bias_cases as C
import rnnt_bias_f64 as R
import rnnt_ngram_cases as NC
from speech2text_amd import _native
from yardstick import TOL, UNIT


# ------------------------------------------------------------------ 1. the cases' conditions
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_conditions(name):
    c = C.CASES[name]
    ref, f32, un = C.reference(name), C.reference32(name), C.unbiased(name)
    lens = C.make(name)[2].tolist()
    assert lens[0] == c["T"] and (c["B"] < 2 or lens[1] == 0) and (c["B"] < 3 or lens[2] > c["T"])
    for b, (r, s) in enumerate(zip(ref, f32)):
        assert r.margin >= C.MARGIN, (name, b, r.margin)
        assert (r.tokens, r.frames) == (s.tokens, s.frames), (name, b)
        assert len(r.tokens) == len(r.frames) <= C.clamp(lens[b], c["T"])
    assert any(len(r.tokens) >= 2 for r in ref) and any(abs(r.bias_score) > 0 for r in ref)
    if c["beam"] > 1:
        assert any(r.tokens != u.tokens for r, u in zip(ref, un)), name
    else:
        assert all(r.tokens == u.tokens and r.frames == u.frames and r.final_pos == 0 for r, u in zip(ref, un))
    fig = C.fp32_figure(name)
    print(f"{name}: float32 costs the restatement {fig:.3e}, recorded {C.COST[name]:.1e}, bound {C.bound(name):.1e}")
    assert fig <= C.COST[name]


@pytest.mark.parametrize("names", [C.PLAIN, C.NGRAM], ids=["bias", "ngram_bias"])
@pytest.mark.parametrize("event", C.EVENTS)
def test_every_event_occurs_in_a_case_of_each_entry(names, event):
    assert any(C.occurred(n, event) for n in names), event


def test_shapes_cover_what_the_kernels_branch_on():
    assert len(C.PLAIN) == len(C.NGRAM) == 8 and set(C.COST) == set(C.CASES)
    assert all(2 <= len(p) <= 6 for p in C.PHRASES) and C.PHRASES.count([2, 3]) == 2
    assert [1, 2, 3, 4][1:3] == [2, 3]                     # a suffix of another phrase's prefix
    for names in (C.PLAIN, C.NGRAM):
        cs = [C.CASES[n] for n in names]
        assert {63, 65, 11, 520, 1000, 128} <= {c["V"] for c in cs}
        assert any(c["B"] == 17 for c in cs) and any(c["beam"] == c["topk"] == 16 and c["V"] == 63 for c in cs)
        assert any(c["beam"] == c["topk"] == 1 for c in cs) and any(c["topk"] > c["V"] == 11 for c in cs)
    for n in C.LARGE:                                      # the lm rows do not fit 60 KiB next to the fixed part
        c = C.CASES[n]
        assert 16 * (c["E"] + c["D"]) + 128 * c["ctx"] + 4 * c["beam"] * c["V"] > 60 * 1024
    for n in C.LONG:                                       # the trace-back from a non-zero position, over two blocks
        r = C.reference(n)[0]
        assert C.CASES[n]["T"] > 64 and r.final_pos != 0 and len(r.tokens) > 16 and r.frames[0] < 6
    for n in C.YAML:
        y = C.CASES[n]
        assert (y["V"], y["E"], y["D"], y["ctx"], y["B"], y["T"]) == (128, 512, 256, 5, 4, 12)


def test_chunked_restatement_is_the_whole_one():
    for name in ("h_v65_b17_o3", C.LONG[0]):
        c = C.CASES[name]
        p, am, lens = C.make(name)
        p = {k: v.numpy() for k, v in p.items()}
        for b in range(min(c["B"], 4)):
            L = C.clamp(lens[b], c["T"])
            for kind in (1, 7, "ragged"):
                results, stable = R.beam_search_chunked(
                    am[b, :L].numpy(), C.cuts_of(name, b, kind), p, c["ctx"], c["act"], c["beam"], c["topk"],
                    C.hot_of(name, np.float64), c["bias_weight"], C.dict_model(name, np.float64), c["weight"])
                if L:
                    assert results[-1][:5] == C.reference(name)[b][:5], (name, b, kind)
                assert all(x <= y for x, y in zip(stable, stable[1:]))


# ------------------------------------------------------------------ 2. the exhaustive check
@pytest.mark.parametrize("V, T, n, order, weight, phrases, bias_weight", C.BRUTE)
def test_search_is_the_argmax_over_all_labellings(V, T, n, order, weight, phrases, bias_weight):
    assert (V, T) in [(v, t) for v, t, *_ in NC.BRUTE]
    ng = G.DictNgram(C.brute_text(V, order), V) if order else None
    hot = R.Hotwords([list(p) for p in phrases], 1.0)
    ctx, clear, biased = C.BRUTE_DIMS["ctx"], 0, 0
    for p, am in C.brute_inputs(V, T, n):
        got = R.beam_search(am, p, ctx, "relu", 16, V, hot, bias_weight, ng, weight)
        tokens, frames, total, lms, fb, gap = R.brute_force(am, p, ctx, "relu", hot, bias_weight, ng, weight)
        assert abs(got.score - total) <= 1e-9
        if gap > 1e-9:
            clear += 1
            biased += fb != 0
            assert (got.tokens, got.frames) == (tokens, frames)
            assert abs(got.lm_score - lms) <= 1e-9 and abs(got.bias_score - fb) <= 1e-9
    assert clear >= n - 2 and biased >= n // 4


@pytest.mark.parametrize("i", range(len(C.BRUTE)))
def test_the_exhaustive_inputs_the_device_runs_are_all_decided(i):
    """Every one of the first BRUTE_N seeds leads its second best labelling by 1e-3 and decides every cut by 1e-3, so
    the device test skips none; the float32 restatement finds the same labelling; the recorded figure covers it."""
    rows = C.brute_decided(i)
    assert len(rows) == C.BRUTE_N
    for _, _, best, r64, r32 in rows:
        assert (r64.tokens, r64.frames) == (best[0], best[1]) == (r32.tokens, r32.frames)
    assert sum(r[2][4] != 0 for r in rows) >= C.BRUTE_N // 2
    fig = C.brute_fp32_figure(i)
    print(f"exhaustive {C.BRUTE[i][:2]}: float32 costs the restatement {fig:.3e}, recorded {C.BRUTE_COST[i]:.1e}")
    assert fig <= C.BRUTE_COST[i]


# ------------------------------------------------------------------ 3. the host loop
def _graph64(name):
    from speech2text_amd.model.lm.context_graph import ContextGraph
    c = C.CASES[name]
    return ContextGraph(C.PHRASES, c["V"], context_score=c["cs"], dtype=torch.float64)


def _model64(name):
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.from_arpa(C.text_of(name), num_classes=C.CASES[name]["V"], dtype=torch.float64)


@pytest.mark.parametrize("name", ["h_v11_kV", "h_long_o3", "h_v65_b17", "h_v65_b17_o3"])
def test_host_loop_is_the_restatement(name):
    from speech2text_amd.model.rnnt_bias import RnntBiasBeamDecoding
    c = C.CASES[name]
    pred, join = C.plain_modules(name, torch.float64)
    _, am, lens = C.make(name)
    lm = _model64(name) if c["order"] else None
    dec = RnntBiasBeamDecoding(C.Ids(), pred, join, c["beam"], c["topk"], lm, c["weight"], None, _graph64(name),
                               c["bias_weight"])
    out = dec.beam_tokens(am.double(), lens)
    assert len(out) == (6 if lm is not None else 5)
    ref = C.reference(name)
    for b, r in enumerate(ref):
        n = int(out[2][b])
        assert out[0][b, :n].tolist() == r.tokens and out[1][b, :n].tolist() == r.frames, (name, b)
    want = lambda i: torch.tensor([r[i] for r in ref], dtype=torch.float64)          # noqa: E731
    # the loop computes in float64 (against the restatement: yardstick.TOL's 1e-12) and beam_tokens stores its
    # results in fp32 tensors: one float32 rounding of each value, yardstick.UNIT relative to the largest
    stored = UNIT + TOL["rtol"]
    assert C.rel_err(out[3], want(1)) <= stored and C.rel_err(out[-1], want(3)) <= stored
    if lm is not None:
        assert C.rel_err(out[4], want(2)) <= stored
    assert any(r.final_pos for r in ref) and any(r.bias_score for r in ref)


@pytest.mark.parametrize("name", ["h_v11_kV", "h_v11_kV_o2"])
def test_without_a_context_it_is_the_base_class_bit_for_bit(name):
    from speech2text_amd.model.decoding import RnntBeamDecoding
    from speech2text_amd.model.rnnt_bias import RnntBiasBeamDecoding
    c = C.CASES[name]
    _, am, lens = C.make(name)
    outs = []
    for cls in (RnntBeamDecoding, RnntBiasBeamDecoding):
        pred, join = C.plain_modules(name, torch.float32)
        lm = C.model_of(name)
        outs.append(cls(C.Ids(), pred, join, c["beam"], c["topk"], lm, c["weight"]).beam_tokens(am, lens))
    assert len(outs[0]) == len(outs[1]) == (5 if c["order"] else 4) and int(outs[0][2].sum()) > 0
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_argument_errors_of_the_new_classes():
    from speech2text_amd.model.decoding import RnntStreamingSearch
    from speech2text_amd.model.rnnt_bias import (RnntBiasBeamDecoding, RnntBiasStreamingSearch,
                                                 rnnt_bias_streaming_search)
    name = "h_v11_kV_o2"
    pred, join = C.build_modules("cpu", 11, 12, 24, 1)
    graph, lm = C.graph_of(name), C.model_of(name)
    with pytest.raises(ValueError, match="ContextGraph"):
        RnntBiasBeamDecoding(C.Ids(), pred, join, context=[[1, 2]])
    with pytest.raises(ValueError, match="finite"):
        RnntBiasBeamDecoding(C.Ids(), pred, join, context=graph, context_weight=math.nan)
    assert RnntBiasBeamDecoding(C.Ids(), pred, join)._context is None
    with pytest.raises(ValueError, match="ContextGraph"):
        RnntBiasStreamingSearch(pred, join, context=None)
    with pytest.raises(ValueError, match="fp32"):
        RnntBiasStreamingSearch(pred, join, context=_graph64(name))
    with pytest.raises(ValueError, match="NgramLm"):
        RnntBiasStreamingSearch(pred, join, context=graph, lm=object())
    for kw in (dict(method="greedy"), dict(method="beam", lm=lm, lm_start_token=3), dict(method="beam", lm=object())):
        with pytest.raises(ValueError, match="hotword"):
            rnnt_bias_streaming_search(pred, join, context=graph, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):    # without a context it is rnnt_streaming_search
        rnnt_bias_streaming_search(pred, join, method="beam", device="cpu")
    assert issubclass(RnntBiasStreamingSearch, RnntStreamingSearch)


# ------------------------------------------------------------------ 4. the C entries, called without a device
FAKE = 0x1000                      # a non-null address no entry follows on the host
W = ["emb", "conv_w", "lin_w", "lin_b", "pre_w", "pre_b"]
_HEAD = ["am", "lengths", *W, "B", "T", "V", "E", "D", "ctx", "act", "blank", "beam_size", "cutoff_top_k"]
_OUT = ["tokens", "frames", "out_len", "score"]
BIAS, NGRAM_BIAS = "s2t_rnnt_beam_stateless_bias", "s2t_rnnt_beam_stateless_ngram_bias"
BIAS_CHUNK, NGRAM_BIAS_CHUNK = BIAS + "_chunk", NGRAM_BIAS + "_chunk"
BIAS_RESET, NGRAM_BIAS_RESET = "s2t_rnnt_bias_stream_reset", "s2t_rnnt_ngram_bias_stream_reset"
BIAS_BYTES, NGRAM_BIAS_BYTES = "s2t_rnnt_bias_stream_state_bytes", "s2t_rnnt_ngram_bias_stream_state_bytes"
ENTRIES = {
    BIAS: ["graph", *_HEAD, "bias_weight", "workspace", *_OUT, "bias_score", "stream"],
    NGRAM_BIAS: ["lm", "graph", *_HEAD, "lm_weight", "start_ctx", "bias_weight", "workspace", *_OUT, "lm_score",
                 "bias_score", "stream"],
    BIAS_CHUNK: ["graph", *_HEAD, "bias_weight", "max_tokens", "state", *_OUT, "bias_score", "stable_len", "overflow",
                 "stream"],
    NGRAM_BIAS_CHUNK: ["lm", "graph", *_HEAD, "lm_weight", "bias_weight", "max_tokens", "state", *_OUT, "lm_score",
                       "bias_score", "stable_len", "overflow", "stream"],
    BIAS_RESET: ["state", "rows", "B", "V", "ctx", "beam_size", "max_tokens", "blank", "stream"],
    NGRAM_BIAS_RESET: ["state", "rows", "B", "V", "ctx", "beam_size", "max_tokens", "blank", "start_ctx", "stream"],
}
VALID = dict(B=2, T=9, V=11, E=12, D=24, ctx=2, act=0, blank=0, beam_size=4, cutoff_top_k=4, max_tokens=16,
             lm_weight=0.5, start_ctx=0, bias_weight=1.0)
NUM_CTX = 12
NAN, INF = math.nan, math.inf
E_BEAM = (60 * 1024 - 128 * VALID["ctx"]) // 16 - VALID["D"] + 1                # one past beam_fixed_lds's rule


def _desc(kind, V, broken=None):
    d = _native.struct(kind)()
    d.V, d.num_ctx, d.num_arcs = V, NUM_CTX, 40
    if kind == "S2tNgramLmDesc":
        d.order = 2
    else:
        d.max_depth = 6
    for k, _ in d._fields_:
        if k.startswith(("ctx_", "arc_")):
            setattr(d, k, FAKE)
    if broken:
        setattr(d, broken[0], broken[1])
    return d


def call(lib, entry, arg=None, value=None, batch=None):
    """The entry on its valid tuple with `arg` set to `value` (and B to `batch`).  A descriptor's V follows the
    call's; lm / graph = None: NULL, "V-1": its V one off, (field, value): that field set."""
    a = dict(VALID)
    if arg in a:
        a[arg] = value
    if batch is not None:
        a["B"] = batch
    held, args = [], []
    for name in ENTRIES[entry]:
        if name in ("lm", "graph"):
            kind = "S2tNgramLmDesc" if name == "lm" else "S2tContextGraphDesc"
            d = _desc(kind, a["V"])
            if arg == name:
                d = None if value is None else _desc(kind, a["V"] - 1) if value == "V-1" else _desc(kind, a["V"], value)
            held.append(d)
            args.append(None if d is None else ctypes.byref(d))
        elif name in a:
            args.append(a[name])
        else:                                              # a pointer: NULL when it is the broken one
            args.append(None if name == arg else FAKE)
    return getattr(lib, entry)(*args)


_BEAM = dict(V=[0, -1, 8193], E=[0, -1, E_BEAM], D=[0, -1], ctx=[0, -1, 65], act=[-1, 2], blank=[-1, 11],
             beam_size=[0, -1, 17], cutoff_top_k=[0, -1])
_GRAPH = dict(graph=[None, "V-1", ("max_depth", -1), ("max_depth", 65), ("num_ctx", 0), ("num_arcs", 10),
                     ("ctx_final", 0), ("arc_score", 0), ("ctx_begin", 0)],
              bias_weight=[NAN, INF, -INF], bias_score=[None])
_LM = dict(lm=[None, "V-1", ("order", 0), ("arc_next", 0)], lm_weight=[NAN, INF], lm_score=[None])
_RESET = dict(state=[None], V=[0, -1, 8193], ctx=[0, -1, 65], beam_size=[0, -1, 17], max_tokens=[0, -1], blank=[-1, 11])
REFUSED = {
    BIAS: dict(_BEAM, **_GRAPH, T=[0, -1], workspace=[None]),
    NGRAM_BIAS: dict(_BEAM, **_GRAPH, **_LM, T=[0, -1], workspace=[None], start_ctx=[-1, NUM_CTX]),
    BIAS_CHUNK: dict(_BEAM, **_GRAPH, T=[0, -1, 257], max_tokens=[0, -1], state=[None]),
    NGRAM_BIAS_CHUNK: dict(_BEAM, **_GRAPH, **_LM, T=[0, -1, 257], max_tokens=[0, -1], state=[None]),
    BIAS_RESET: _RESET,                                    # beam_size 0: there is no greedy form
    NGRAM_BIAS_RESET: dict(_RESET, start_ctx=[-1]),
}


def _lib():
    lib = ctypes.CDLL(_native.LIB_PATH)                    # plain handles: no launch is ever checked
    protos = _native.parse_header()
    for entry in list(ENTRIES) + [BIAS_BYTES, NGRAM_BIAS_BYTES, "s2t_rnnt_stream_state_bytes",
                                  "s2t_rnnt_ngram_stream_state_bytes"]:
        getattr(lib, entry).restype, getattr(lib, entry).argtypes = protos[entry]
    return lib, protos


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entries_refuse_before_any_launch(entry):
    lib, protos = _lib()
    assert len(protos[entry][1]) == len(ENTRIES[entry]), entry
    for arg, values in REFUSED[entry].items():
        assert arg in ENTRIES[entry], (entry, arg)
        for v in values:
            assert call(lib, entry, arg, v) == -1, (entry, arg, v)
    for b in (0, -1):                                      # nothing to do: 0, whatever else is handed over
        assert call(lib, entry, batch=b) == 0
        assert call(lib, entry, "beam_size", 17, batch=b) == 0


def test_state_queries():
    lib, _ = _lib()
    plain, ngram = lib.s2t_rnnt_stream_state_bytes, lib.s2t_rnnt_ngram_stream_state_bytes
    for B, V, ctx, beam, MT in ((2, 11, 2, 4, 16), (17, 65, 5, 4, 5), (1, 1000, 2, 16, 64), (3, 128, 5, 1, 1024)):
        for query, partner in ((lib.s2t_rnnt_bias_stream_state_bytes, plain),
                               (lib.s2t_rnnt_ngram_bias_stream_state_bytes, ngram)):
            n, m = query(B, V, ctx, beam, MT), partner(B, V, ctx, beam, MT)
            assert m > 0 and n % (256 * B) == 0 and n == m + 256 * B * (-(-8 * beam // 256)), (B, V, ctx, beam, MT)
    for query in (lib.s2t_rnnt_bias_stream_state_bytes, lib.s2t_rnnt_ngram_bias_stream_state_bytes):
        for bad in ((0, 11, 2, 4, 16), (2, 0, 2, 4, 16), (2, 8193, 2, 4, 16), (2, 11, 65, 4, 16), (2, 11, 0, 4, 16),
                    (2, 11, 2, 0, 16), (2, 11, 2, 17, 16), (2, 11, 2, -1, 16), (2, 11, 2, 4, 0)):
            assert query(*bad) == 0, bad
