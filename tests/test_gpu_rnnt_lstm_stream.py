"""GPU: the chunk-carried RNN-T search with the LSTM predictor (csrc/decode_lstm.hip
s2t_rnnt_*_lstm_chunk, model/decoding.py RnntLstmStreamingSearch), the StreamingRecognizer graph
around it and PrunedRnntTask.streaming_recognizer with `predictor.model: Lstm`.

The yardstick is exact: however [0, L) is cut into chunks, tokens, frames, out_len and score are
those of the whole-utterance device calls (rnnt_greedy_lstm_tokens_from_am /
rnnt_beam_lstm_tokens_from_am, themselves held to the float64 restatement by
tests/test_gpu_rnnt_lstm_search.py) on the concatenated am, bit for bit -- torch.equal, no
tolerance -- and the tokens are the float64 restatement's (tests/rnnt_lstm_search_cases.py: no
exclusions).  `stable_len` is held to the float64 chunked restatement of
tests/rnnt_lstm_stream_f64.py on every utterance of the two longer cases of
tests/rnnt_lstm_stream_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

import rnnt_lstm_search_cases as C
import rnnt_lstm_search_f64 as S
import rnnt_lstm_stream_cases as SC
import rnnt_lstm_stream_f64 as F
from decode_support import (_beam_modules, _feed, _fixture_free_config, _lstm_build, _lstm_case, _lstm_modules,
                            _lstm_pair, _plan, RECOGNIZER_BLANK, _regular, _same_rows, _TINY,
                            _tiny_stream_encoder, _tokenizer)
from task_support import _pruned_beam_cfg

pytestmark = pytest.mark.gpu

PARTITIONS = ("1", "7", "16", "irregular")


# ------------------------------------------------------------------------------------ helpers


_CACHE = {}


def _case(dev, name):
    """(case, modules, am and lengths on the device, the float64 results), built once per case."""
    if name in C.CASES:
        return _lstm_case(dev, name)
    if name not in _CACHE:
        c = SC.CASES[name]
        w, act, am, lens = SC.make(name)
        p, j = _lstm_modules(dev, w, c["model"])
        _CACHE[name] = (c, p, j, am.to(dev), lens.to(dev), SC.reference(name))
    return _CACHE[name]


def _lens(name):
    return np.asarray(SC.lengths(name), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _one_shot(dev, name):
    """The whole-utterance device search on a case: computed once, shared, left unchanged."""
    from speech2text_amd.model.decoding import rnnt_beam_lstm_tokens_from_am, rnnt_greedy_lstm_tokens_from_am
    c, p, j, am, lens, _ = _case(dev, name)
    if c["beam"] is None:
        out = rnnt_greedy_lstm_tokens_from_am(am, lens, p, j, c["mts"])
    else:
        out = rnnt_beam_lstm_tokens_from_am(am, lens, p, j, c["beam"], c["topk"])
    assert out is not None
    return [x.cpu() for x in out]


def _stream(dev, name, B=None, max_tokens=None, capturable=True, **kw):
    from speech2text_amd.model.decoding import RnntLstmStreamingSearch
    c, p, j = _case(dev, name)[:3]
    greedy = c["beam"] is None
    if max_tokens is None:
        max_tokens = c["T"] * (c["mts"] + 1) if greedy else c["T"]
    return RnntLstmStreamingSearch(p, j, c["B"] if B is None else B, "greedy" if greedy else "beam",
                                   max_token_step=c["mts"] or 0, beam_size=c["beam"] or 1,
                                   cutoff_top_k=c["topk"] or 1, max_tokens=max_tokens, device=dev,
                                   capturable=capturable, **kw)


# ------------------------------------------------------------------------------------ 1. greedy
@pytest.mark.parametrize("capturable", [True, False], ids=["capturable", "host_poll"])
@pytest.mark.parametrize("partition", PARTITIONS)
@pytest.mark.parametrize("name", list(SC.GREEDY_CASES))
def test_greedy_chunks_equal_the_whole_utterance_walk(dev, name, partition, capturable):
    c, p, j, am, lens, ref = _case(dev, name)
    gt, gn = _one_shot(dev, name)
    search = _stream(dev, name, capturable=capturable)
    got, off = _feed(search, am, _plan(_lens(name), partition, c["seed"]))
    assert off.tolist() == _lens(name).tolist()
    assert torch.equal(got[1], gn)
    for b, r in enumerate(ref):
        n = int(gn[b])
        assert torch.equal(got[0][b, :n], gt[b, :n]), b
        assert got[0][b, :n].tolist() == r[0], b                        # the float64 tokens
    assert int(search.overflow.sum()) == 0


# ------------------------------------------------------------------------------------ 2. beam
@pytest.mark.parametrize("partition", PARTITIONS)
@pytest.mark.parametrize("name", list(SC.BEAM_CASES))
def test_beam_chunks_equal_the_whole_utterance_search(dev, name, partition):
    """b_h64o_b33_beam4_k1 (B 33) and b_h48_b17_beam4 (B 17) cross the 16-row tile."""
    c, p, j, am, lens, ref = _case(dev, name)
    want = _one_shot(dev, name)
    search = _stream(dev, name)
    got, off = _feed(search, am, _plan(_lens(name), partition, c["seed"]))
    assert off.tolist() == _lens(name).tolist()
    _same_rows(got, want)
    for b, (tok, _, frm, _) in enumerate(ref):
        n = int(got[2][b])
        assert got[0][b, :n].tolist() == tok and got[1][b, :n].tolist() == frm, b
    assert int(search.overflow.sum()) == 0


@pytest.mark.parametrize("name", list(SC.LONG_CASES))
def test_long_chunks_cross_the_trace_blocks(dev, name):
    """90-frame rows: the whole-utterance trace-back and the chunk end both stage their records in
    blocks of 64 frames.  The whole-utterance call gives the float64 tokens and frames; the stream
    fed one 90-frame chunk, 70 + 20 frames and 7-frame chunks equals it bit for bit, with the same
    stable_len after the last chunk."""
    c, p, j, am, lens, ref = _case(dev, name)
    want = _one_shot(dev, name)
    for b, (tok, _, frm, _) in enumerate(ref):
        n = int(want[2][b])
        assert want[0][b, :n].tolist() == tok and want[1][b, :n].tolist() == frm, b
    stable = []
    for step in (90, 70, 7):
        search = _stream(dev, name)
        got, off = _feed(search, am, _regular(_lens(name), step))
        assert off.tolist() == _lens(name).tolist()
        _same_rows(got, want)
        assert int(search.overflow.sum()) == 0
        stable.append(got[4].tolist())
    assert stable[0] == stable[1] == stable[2], stable


# ------------------------------------------------------------------------------------ 3. prefix answer
@functools.lru_cache(maxsize=None)
def _run7(dev, name):
    """The 7-frame partition of a case with the outputs after every chunk."""
    snaps = []
    _feed(_stream(dev, name), _case(dev, name)[3], _regular(_lens(name), 7),
             snap=lambda off, out: snaps.append((off, out)))
    return snaps


@pytest.mark.parametrize("name", list(SC.STREAM_CASES) + ["b_yaml"])
def test_every_chunk_gives_the_prefix_answer(dev, name):
    from speech2text_amd.model.decoding import rnnt_beam_lstm_tokens_from_am
    c, p, j, am, _, _ = _case(dev, name)
    for off, out in _run7(dev, name):
        want = [x.cpu() for x in rnnt_beam_lstm_tokens_from_am(am, torch.as_tensor(off), p, j, c["beam"], c["topk"])]
        _same_rows(out, want)


# ------------------------------------------------------------------------------------ 4. stable_len
@functools.lru_cache(maxsize=None)
def _stable_f64(name, b):
    c = SC.CASES[name]
    w, act, am, _ = SC.make(name)
    n = int(_lens(name)[b])
    return F.beam_search_chunked(am[b, :n], F.cuts_of(n, "7"), S.cast(w, torch.float64), act, c["beam"],
                                 c["topk"])[4]


@pytest.mark.parametrize("name", list(SC.STREAM_CASES) + ["b_h20_beam1_k1"])
def test_stable_len(dev, name):
    """stable_len never decreases; tokens[:stable_len] is a prefix of every later result; with one
    beam it is out_len; on every utterance of the two longer cases it is the float64 chunked
    restatement's common-prefix length after every chunk."""
    snaps = _run7(dev, name)
    lens = _lens(name)
    for b in range(len(lens)):
        n = int(lens[b])
        mine = [(out[0][b], int(out[2][b]), int(out[4][b])) for _, out in snaps[:-(-n // 7)]]
        stable = [m[2] for m in mine]
        assert stable == sorted(stable) and (not mine or stable[-1] <= mine[-1][1]), b
        for k, (tok, _, st) in enumerate(mine):
            for tok2, n2, _ in mine[k:]:
                assert n2 >= st and torch.equal(tok2[:st], tok[:st]), (b, k)
        if name in SC.STREAM_CASES:
            assert stable == _stable_f64(name, b), (b, stable, _stable_f64(name, b))
    if SC.CASES[name]["beam"] == 1:
        assert all(torch.equal(out[4], out[2]) for _, out in snaps) and int(snaps[-1][1][2].sum()) > 0
    else:
        assert any(0 < int(out[4][b]) < int(out[2][b]) for _, out in snaps for b in range(len(lens)))


# ------------------------------------------------------------------------------------ 5. rows, reset
def test_rows_are_independent_and_reset_alone(dev):
    """Rows 0..3 run utterance A; row 2 is reset midway by the row mask and fed utterance B.  Rows
    0, 1, 3 are bit-identical to a run without the reset; row 2 is B's whole-utterance result with
    frames counted from its reset."""
    name = "s_h64o_t40"
    c, p, j, am_c, _, ref = _case(dev, name)
    want = _one_shot(dev, name)
    la, lb = int(_lens(name)[0]), int(_lens(name)[3])
    assert lb > 0 and int(want[2][0]) > 0 and int(want[2][3]) > 0
    am = torch.stack([am_c[0]] * 4)
    plain, _ = _feed(_stream(dev, name, B=4), am, _regular([la] * 4, 16))
    _same_rows(plain, [x[[0, 0, 0, 0]] for x in want])

    search = _stream(dev, name, B=4)
    plan = _regular([la] * 4, 16)
    half = len(plan) // 2
    _, off = _feed(search, am, plan[:half])
    assert int(search.out_len[2]) > 0
    search.reset([2])
    assert search.out_len.tolist()[2] == 0 and int(search.out_len[1]) > 0
    am2 = am.clone()
    am2[2] = am_c[3]
    off[2] = 0
    rest = [np.array([q[0], q[1], 0, q[3]]) for q in plan[half:]]
    for k, cl in enumerate(_regular([lb], 16)):                     # B rides along from its frame 0
        if k < len(rest):
            rest[k][2] = cl[0]
        else:
            rest.append(np.array([0, 0, cl[0], 0]))
    got, off = _feed(search, am2, rest, off=off)
    assert off.tolist() == [la, la, lb, la]
    for x, y in zip(got, plain):
        assert torch.equal(x[[0, 1, 3]], y[[0, 1, 3]])
    _same_rows([x[2:3] for x in got], [x[3:4] for x in want])
    assert got[0][2, :int(got[2][2])].tolist() == ref[3][0] and got[1][2, :int(got[2][2])].tolist() == ref[3][2]


# ------------------------------------------------------------------------------------ 6. idle call
@pytest.mark.parametrize("name", ["g_h64o_b3_t40", "s_h20_t40"])
def test_idle_call_changes_nothing(dev, name):
    c, p, j, am, _, _ = _case(dev, name)
    want = _one_shot(dev, name)
    search = _stream(dev, name)
    plan = _regular(_lens(name), 7)
    _, off = _feed(search, am, plan[:3])
    assert int(search.out_len.sum()) > 0
    outs = (search.state, search.tokens, search.frames, search.out_len, search.score, search.stable_len,
            search.overflow)
    for Tc in (7, 16):                                                  # an odd and an even number of rounds
        before = [x.clone() for x in outs]
        search.step(am[:, :Tc].contiguous(), torch.zeros(c["B"], dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        for x, y in zip(outs, before):
            assert torch.equal(x, y), Tc
    got, off = _feed(search, am, plan[3:], off=off)
    if c["beam"] is None:
        assert torch.equal(got[1], want[1])
        for b in range(c["B"]):
            assert torch.equal(got[0][b, :int(want[1][b])], want[0][b, :int(want[1][b])])
    else:
        _same_rows(got, want)


# ------------------------------------------------------------------------------------ 7. capacity
def test_capacity(dev):
    """max_tokens = 3 on utterances with more than 3 tokens: the first 3 tokens, out_len 3, overflow
    1; the beam search itself went on exactly -- its score is the whole-utterance score, bit for
    bit; reset clears overflow."""
    for name in ("s_h64o_t40", "g_h64o_b3_t40"):
        c, p, j, am, _, _ = _case(dev, name)
        want = _one_shot(dev, name)
        n_want = want[1] if c["beam"] is None else want[2]
        rows = [b for b in range(c["B"]) if int(n_want[b]) > 3]
        assert len(rows) >= 2, (name, n_want.tolist())
        search = _stream(dev, name, B=len(rows), max_tokens=3)
        lens = _lens(name)[rows]
        got, _ = _feed(search, am[rows].contiguous(), _regular(lens, 7))
        n_got = got[1] if c["beam"] is None else got[2]
        assert n_got.tolist() == [3] * len(rows) and search.overflow.tolist() == [1] * len(rows)
        assert torch.equal(got[0], want[0][rows, :3])
        if c["beam"] is not None:
            assert torch.equal(got[1], want[1][rows, :3])
            assert torch.equal(got[3], want[3][rows])
            assert int(got[4].max()) <= 3
        search.reset()
        torch.cuda.synchronize()
        assert search.overflow.tolist() == [0] * len(rows) and search.out_len.tolist() == [0] * len(rows)
        got, _ = _feed(search, am[rows].contiguous(), _regular(lens, 1)[:1])
        assert search.overflow.tolist() == [0] * len(rows)              # one frame: at most two tokens


# ------------------------------------------------------------------------------------ 8. refusals
def test_refusals(dev):
    """-1 before any launch, every output untouched."""
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnnt_lstm_desc
    lib = N.lib()
    V, B, MT = _TINY["V"], 2, 10
    p, j = _lstm_build(dev, **_TINY)
    desc, keep = rnnt_lstm_desc(p, j)
    bad, keep_bad = rnnt_lstm_desc(p, j)
    keep_bad[-1].H = 1028
    assert lib.s2t_rnnt_lstm_stream_state_bytes(desc, B, 16, MT) > lib.s2t_rnnt_lstm_stream_state_bytes(desc, B, 0, MT) > 0
    assert lib.s2t_rnnt_lstm_stream_state_bytes(desc, B, 16, 2 * MT) > lib.s2t_rnnt_lstm_stream_state_bytes(desc, B, 16, MT)
    for args in ((B, 17, MT), (B, -1, MT), (B, 4, 0), (0, 4, MT)):
        assert lib.s2t_rnnt_lstm_stream_state_bytes(desc, *args) == 0, args
    assert lib.s2t_rnnt_lstm_stream_state_bytes(bad, B, 4, MT) == 0
    for args in ((B, 0, 4), (B, 257, 4), (B, 4, 17), (0, 4, 4)):
        assert lib.s2t_rnnt_lstm_stream_workspace_bytes(desc, *args) == 0, args
    assert lib.s2t_rnnt_lstm_stream_workspace_bytes(bad, B, 4, 4) == 0
    state = torch.zeros(lib.s2t_rnnt_lstm_stream_state_bytes(desc, B, 16, MT), dtype=torch.uint8, device=dev)
    ws = torch.zeros(lib.s2t_rnnt_lstm_stream_workspace_bytes(desc, B, 256, 16), dtype=torch.uint8, device=dev)
    am, cl = torch.zeros(B, 257, V, device=dev), torch.ones(B, dtype=torch.int64, device=dev)
    tok, frm = (torch.full((B, MT), 7, dtype=torch.int64, device=dev) for _ in range(2))
    n_out, stable = (torch.full((B,), 7, dtype=torch.int64, device=dev) for _ in range(2))
    score = torch.full((B,), 7.0, device=dev)
    ovf = torch.full((B,), 7, dtype=torch.int32, device=dev)

    def beam(d=desc, Tc=4, beam_size=4, topk=4, mt=MT, st=state, w=ws, nb=B):
        return lib.s2t_rnnt_beam_lstm_chunk(d, N.fp(am), N.lp(cl), nb, Tc, beam_size, topk, mt, N.ptr(st), N.ptr(w),
                                            N.lp(tok), N.lp(frm), N.lp(n_out), N.fp(score), N.lp(stable),
                                            N.ip(ovf), N.stream())

    def greedy(d=desc, Tc=4, mts=1, mt=MT, st=state, w=ws, poll=0, nb=B):
        return lib.s2t_rnnt_greedy_lstm_chunk(d, N.fp(am), N.lp(cl), nb, Tc, mts, mt, poll, N.ptr(st), N.ptr(w),
                                              N.lp(tok), N.lp(n_out), N.ip(ovf), N.stream())

    def reset(d=desc, beam_size=4, mt=MT, st=state, w=ws, nb=B):
        return lib.s2t_rnnt_lstm_stream_reset(d, N.ptr(st), None, nb, beam_size, mt, N.ptr(w), N.stream())

    for kw in (dict(Tc=0), dict(Tc=257), dict(st=None), dict(w=None), dict(mt=0), dict(beam_size=0),
               dict(beam_size=17), dict(topk=0), dict(d=bad)):
        assert beam(**kw) == -1, kw
    for kw in (dict(Tc=0), dict(Tc=257), dict(st=None), dict(w=None), dict(mt=0), dict(mts=-1), dict(d=bad),
               dict(Tc=257, poll=1)):
        assert greedy(**kw) == -1, kw
    for kw in (dict(st=None), dict(w=None), dict(mt=0), dict(beam_size=17), dict(beam_size=-1), dict(d=bad)):
        assert reset(**kw) == -1, kw
    assert beam(nb=0) == 0 and greedy(nb=0) == 0 and reset(nb=0) == 0
    torch.cuda.synchronize()
    for t in (tok, frm, n_out, stable, ovf):
        assert bool((t == 7).all())
    assert bool((score == 7.0).all()) and int(state.sum()) == 0 and int(ws.sum()) == 0


def test_class_refuses_what_the_kernels_do_not_take(dev):
    from speech2text_amd.model.decoding import RnntLstmStreamingSearch, RnntStreamingSearch, rnnt_streaming_search
    p, j = _lstm_build(dev, **_TINY)
    assert isinstance(rnnt_streaming_search(p, j, 2, "beam", device=dev), RnntLstmStreamingSearch)
    assert not rnnt_streaming_search(p, j, 2, "greedy", device=dev, capturable=False).capturable
    s = _fixture_free_config(V=8, D=16, E=12, ctx=2, seed=9)
    pred, join = _beam_modules(s, dev)
    assert isinstance(rnnt_streaming_search(pred, join, 2, "beam", device=dev), RnntStreamingSearch)
    with pytest.raises(ValueError):
        RnntLstmStreamingSearch(pred, join, 2, "greedy", device=dev)
    with pytest.raises(ValueError, match="RnntLstmStreamingSearch"):     # the stateless class points here
        RnntStreamingSearch(p, join, 2, "greedy", device=dev)
    with pytest.raises(ValueError):
        RnntLstmStreamingSearch(p, j, 2, "beam", beam_size=17, device=dev)
    with pytest.raises(ValueError):
        RnntLstmStreamingSearch(p, j, 2, "viterbi", device=dev)
    with pytest.raises(ValueError):
        RnntLstmStreamingSearch(*_lstm_build(dev, **dict(_TINY, H=1028)), 2, "greedy", device=dev)
    with pytest.raises(ValueError):
        RnntLstmStreamingSearch(p, j, 2, "greedy", max_tokens=0, device=dev)
    with pytest.raises(RuntimeError):
        RnntLstmStreamingSearch(*_lstm_build("cpu", **_TINY), 2, "greedy", device=dev)
    with pytest.raises(ValueError):
        RnntLstmStreamingSearch(p, j, 2, "beam", device=dev).step(torch.zeros(2, 257, _TINY["V"], device=dev))


# ------------------------------------------------------------------------------------ 9. recogniser
# The tiny random encoder's output hardly moves from frame to frame, so on the fixture's audio a row
# emits at nearly every node (lift <= 14) or only at its first (lift >= 17); 16 sits between for both
# searches: greedy 2 and beam 22 tokens on the 48 frames.


@pytest.mark.parametrize("method", ["greedy", "beam"])
def test_recognizer_graph_equals_the_eager_composition(dev, golden_dir, method):
    """StreamingRecognizer.step (one graph replay) against streaming_step -> _enc_proj ->
    RnntLstmStreamingSearch.step issued eagerly, over the fixture's 6 chunks, twice across reset():
    am, the outputs and every encoder state bit for bit; the final tokens are the whole-utterance
    LSTM search's on the concatenation of the am chunks the recogniser returned."""
    from speech2text_amd.model.decoding import (RnntLstmStreamingSearch, rnnt_beam_lstm_tokens_from_am,
                                                rnnt_greedy_lstm_tokens_from_am)
    from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
    g, m, chunk = _tiny_stream_encoder(golden_dir, dev)
    V, D = 24, max(m.encoder_dim)
    pred, join = _lstm_pair(dev, V, D, 31, RECOGNIZER_BLANK)
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    kw = dict(method=method, max_token_step=1, beam_size=4, cutoff_top_k=4, max_tokens=64)
    rec = StreamingRecognizer(m, pred, join, _tokenizer(V), batch_size=B, device=dev, **kw)
    assert isinstance(rec.search, RnntLstmStreamingSearch) and rec.search.capturable
    eager = RnntLstmStreamingSearch(pred, join, B, device=dev, **kw)
    for rep in range(2):
        st = m.get_init_states(B, dev)
        rec.reset()
        eager.reset()
        ams = []
        for c in range(6):
            x = feats[:, 2 * chunk * c:2 * chunk * c + T]
            with torch.no_grad():
                enc, st = m.streaming_step(x, st)
                am = join._enc_proj(enc).float().contiguous()
            want = eager.step(am)
            got = rec.step(x)
            assert torch.equal(got[-1], am), (rep, c)
            for a, b in zip(got[:-1], want):
                assert torch.equal(a, b), (rep, c)
            ams.append(got[-1].clone())
        for a, b in zip(rec.states, st):
            assert torch.equal(a, b)
        am_all = torch.cat(ams, dim=1)
        n = int(rec.search.out_len.sum())
        print(f"{method} rep {rep}: {n} tokens on {B * 6 * Tc} frames")
        assert 0 < n < B * 6 * Tc
        assert int(rec.search.overflow.sum()) == 0
        lens = torch.full((B,), 6 * Tc, dtype=torch.int64)
        if method == "beam":
            want = [x.cpu() for x in rnnt_beam_lstm_tokens_from_am(am_all, lens, pred, join, 4, 4)]
            _same_rows([x.cpu() for x in rec.outputs], want)
            assert bool((rec.search.stable_len <= rec.search.out_len).all())
        else:
            gt, gn = (x.cpu() for x in rnnt_greedy_lstm_tokens_from_am(am_all, lens, pred, join, 1))
            assert torch.equal(rec.search.out_len.cpu(), gn)
            for b in range(B):
                assert torch.equal(rec.search.tokens.cpu()[b, :int(gn[b])], gt[b, :int(gn[b])])
        texts = rec.texts()
        tok = rec.search.tokens.cpu()
        assert texts == [rec.tokenizer.decode(tok[b, :int(rec.search.out_len[b])]) for b in range(B)]
        assert all(t.startswith(u) for t, u in zip(texts, rec.stable_texts()))


# ------------------------------------------------------------------------------------ 10. task
def test_task_streaming_recognizer_with_the_lstm_predictor(dev):
    """PrunedRnntTask.streaming_recognizer(batch_size=2) of a task with `predictor.model: Lstm`:
    it holds an RnntLstmStreamingSearch, and `recognize` on two utterances of different lengths
    equals feeding the chunks by hand, the shorter row idling while the longer one goes on."""
    import math
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.decoding import RnntLstmStreamingSearch
    V, chunk = 32, 8
    cfg = _pruned_beam_cfg(V)
    cfg["encoder"]["config"].update({"chunk_size": [chunk], "left_context_frames": [16]})
    cfg["predictor"] = {"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": 64, "symbol_embedding_dim": 32, "num_lstm_layers": 2,
        "lstm_hidden_dim": 48, "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}}
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(cfg).to(dev)
    task.eval()
    with torch.no_grad():
        for q in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            q.mul_(3.0)
        task._global_cmvn.global_mean.fill_(0.25)
        task._global_cmvn.global_istd.fill_(0.5)
    rec = task.streaming_recognizer(batch_size=2)
    assert isinstance(rec.search, RnntLstmStreamingSearch)
    assert (rec.search.method, rec.search.beam_size, rec.search.cutoff_top_k) == ("beam", 3, 2)
    greedy = task.streaming_recognizer(batch_size=1, method="greedy").search
    assert isinstance(greedy, RnntLstmStreamingSearch) and greedy.max_token_step == 5
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 150, 80, generator=g) * 2.0
    lens = torch.tensor([150, 71])
    texts = rec.recognize(feats.to(dev), lens)
    assert any(len(t) for t in texts)

    n_out = ((lens - 7) // 2 + 1) // 2
    assert n_out.tolist() == rec.num_output_frames(lens).tolist() == [36, 16]
    K, Tc, T = -(-36 // (chunk // 2)), chunk // 2, 2 * chunk + 13
    pad_value = math.log(1e-10) / 0.5 + 0.25                            # log(1e-10) after the CMVN
    buf = torch.full((2, 2 * chunk * (K - 1) + T, 80), pad_value)
    buf[0, :150], buf[1, :71] = feats[0], feats[1, :71]
    rec.reset()
    idle = 0
    for k in range(K):
        cl = (n_out - k * Tc).clamp(0, Tc)
        idle += int(cl[1] == 0 and cl[0] > 0)
        rec.step(buf[:, 2 * chunk * k:2 * chunk * k + T].to(dev), cl)
    assert idle > 0
    assert rec.texts() == texts
