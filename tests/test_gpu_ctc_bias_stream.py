"""GPU: the chunk-carried CTC prefix beam search with hotword biasing (csrc/decode_ctc.hip
s2t_ctc_prefix_beam_bias_chunk, s2t_ctc_prefix_beam_ngram_bias_chunk and their state-size and reset entries;
model/ctc_bias.py CtcBiasStreamingSearch, ctc_bias_streaming_search), the CtcStreamingRecognizer graph
around it and the `metric.hotwords` key of a task's YAML.

The yardstick of the bits is the one-shot device entry (ctc_prefix_beam_bias_tokens, itself held to float64
by tests/test_gpu_ctc_bias.py): however the frames of a case of tests/ctc_bias_cases.py are cut -- a frame a
call, uneven widths with idle rows in between, the whole utterance -- after EVERY call tokens[:out_len],
out_len, score, lm_score and bias_score are torch.equal to it on the frames fed so far.  A one-frame cut
stops in the middle of phrases that later frames complete: the finalisation, which takes the loan of an
unfinished match out of what is reported, must not have entered the carried state.  Every stream starts
from a state buffer filled with 0xFF bytes before its reset; frames of a chunk at and beyond chunk_len[b]
are NaN in every call.
"""
import copy

import pytest
import torch

import ctc_bias_cases as C
import ctc_bias_f64 as H
from decode_support import _tiny_ctc_encoder, _tokenizer
from task_support import _ctc_zipformer_cfg

pytestmark = pytest.mark.gpu

_CACHE, _PREFIX = {}, {}
_MAX_NODES = 1024       # above 1 + beam * T of every case: no case overflows unless a test asks for it


def _case(dev, name):
    if name not in _CACHE:
        x, lens = C.make(name)
        lm = C.model_of(name)
        _CACHE[name] = (C.CASES[name], x.to(dev), lens.to(dev), C.graph_of(name).to(dev),
                        None if lm is None else lm.to(dev))
    return _CACHE[name]


def _one_shot(dev, name, fed=None):
    """The one-shot entry on the first fed[b] frames of every row (None: the whole utterances) ->
    [tokens, out_len, score, lm_score or None, bias_score] on the host, once per (case, fed)."""
    from speech2text_amd.model.ctc_bias import ctc_prefix_beam_bias_tokens
    key = (name, None if fed is None else tuple(fed))
    if key not in _PREFIX:
        c, x, lens, graph, lm = _case(dev, name)
        if fed is not None:
            x, lens = x[:, :max(max(fed), 1)].contiguous(), torch.tensor(fed, device=dev)
        out = ctc_prefix_beam_bias_tokens(x, lens, graph, c["bias_weight"], lm, c["weight"], c["beam"], c["topk"])
        assert out is not None
        out = [t.cpu() for t in out]
        _PREFIX[key] = out[:3] + [out[3] if lm is not None else None, out[-1]]
    return _PREFIX[key]


def _search(dev, name, poison=True, **kw):
    from speech2text_amd.model.ctc_bias import CtcBiasStreamingSearch
    c, _, _, graph, lm = _case(dev, name)
    args = dict(batch_size=c["B"], beam_size=c["beam"], cutoff_top_k=c["topk"], max_tokens=c["T"],
                max_nodes=_MAX_NODES, device=dev, lm=lm, lm_weight=c["weight"], context=graph,
                context_weight=c["bias_weight"])
    args.update(kw)
    s = CtcBiasStreamingSearch(c["V"], **args)
    if poison:                                             # reset must establish all a stream reads
        s.state.fill_(0xFF)
        s.reset()
    return s


def _outputs(search):
    """[tokens, out_len, score, lm_score or None, bias_score, stable_len, overflow] on the host."""
    return [None if t is None else t.cpu().clone() for t in (
        search.tokens, search.out_len, search.score, search.lm_score, search.bias_score, search.stable_len,
        search.overflow)]


def _same_as_one_shot(got, want, what, rows=None):
    for b in (range(got[0].shape[0]) if rows is None else rows):
        n = int(want[1][b])
        assert int(got[1][b]) == n, (what, b, got[1], want[1])
        assert torch.equal(got[0][b, :n], want[0][b, :n]), (what, b)
        for k in (2, 3, 4):
            assert (got[k] is None) == (want[k] is None)
            if got[k] is not None:
                assert torch.equal(got[k][b], want[k][b]), (what, b, k, got[k], want[k])


def _state_rows(search):
    """The state's arrays by the tables in include/s2t_mi355.h: the plain layout, ctx with an n-gram, then
    bstate and bsum -> {array: (B, bytes per row) view of search.state}."""
    B, beam, M = search.batch_size, search.beam_size, search.max_nodes
    sizes = [("nodes", 16 * M), ("stage", 16 * M), ("map", 4 * M)]
    sizes += [(k, 4 * beam) for k in ("pb", "pnb", "lm_sum", "node", "last", "len")]
    sizes += [(k, 4) for k in ("nb", "kept", "depth", "ovf")] + [("eff", 8)]
    sizes += ([("ctx", 4 * beam)] if search._lm is not None else []) + [("bstate", 4 * beam), ("bsum", 4 * beam)]
    off, out = 0, {}
    for k, per in sizes:
        out[k] = search.state[off:off + B * per].view(B, per)
        off += (B * per + 255) // 256 * 256
    assert off == search.state.numel()
    return out


# ------------------------------------------------------------------ 1. every case under every cut
@pytest.mark.parametrize("cut", list(C.CUTS))
@pytest.mark.parametrize("name", list(C.CASES))
def test_any_cut_equals_the_one_shot_entry_after_every_call(dev, name, cut):
    search = _search(dev, name)
    last = None
    for i, (ch, cl, fed) in enumerate(C.chunks(name, cut)):
        out = search.step(ch.to(dev), cl.to(dev))
        assert len(out) == 4 and out[0] is search.tokens
        got = _outputs(search)
        assert int(got[6].abs().sum()) == 0, (name, cut, i, got[6])
        _same_as_one_shot(got, _one_shot(dev, name, fed), (name, cut, "after call", i))
        if last is not None:                               # what is stable stays
            assert bool((got[5] >= last[5]).all()), (name, cut, i)
            for b in range(got[0].shape[0]):
                s = int(last[5][b])
                assert torch.equal(got[0][b, :s], last[0][b, :s]), (name, cut, i, b)
        last = got
    _same_as_one_shot(last, _one_shot(dev, name), (name, cut))
    for b, r in enumerate(C.reference(name)):              # (and so the float64 restatement's tokens)
        assert last[0][b, :int(last[1][b])].tolist() == r.tokens, (name, cut, b)


@pytest.mark.parametrize("name", ["b_v6_twice", "b_v6_o3_twice"])
def test_a_cut_that_ends_mid_phrase_is_followed_by_frames_that_complete_it(dev, name):
    """The condition on the one-frame cut, stated on the restatement: some call ends with a reported
    hypothesis inside a phrase, its loan taken out of bias_score, and a later call reports that phrase
    completed.  (The equality itself is the test above.)"""
    c = C.CASES[name]
    hot = H.Hotwords(c["phrases"], c["cs"], c["scores"])
    x, _ = C.make(name)
    mid = done = None
    for t in range(1, c["T"] + 1):
        r = C.restate(c, x[0], torch.float64, frames=t)
        h = tuple(r.tokens)
        if mid is None and 0 < hot.match_len(h) and not hot.ending(h) and hot.bias_sum(h) > hot.final_bias(h):
            mid = (t, h, r.completions)
        elif mid is not None and h[:len(mid[1])] == mid[1] and r.completions > mid[2]:
            done = t
            break
    assert mid is not None and done is not None, (mid, done)
    want_mid, want_done = _one_shot(dev, name, [mid[0]] * c["B"]), _one_shot(dev, name, [done] * c["B"])
    assert float(want_mid[4][0]) == float(hot.final_bias(mid[1])) < float(want_done[4][0])


# ------------------------------------------------------------------ 2. reset, overflow, graphs
def _spelled(c, token, frames=1):
    """A chunk (B, frames, V) that says `token` in every row beyond doubt: position 0 of every beam is then
    the prefix (token,), inside the graph when a phrase starts with it."""
    ch = torch.full((c["B"], frames, c["V"]), -20.0)
    ch[:, :, token] = 20.0
    return ch


@pytest.mark.parametrize("name", ["b_v8_changes", "b_v9_o3_changes"])
def test_reset_restarts_exactly_those_rows_in_the_root(dev, name):
    c, x, lens, graph, lm = _case(dev, name)
    first = c["phrases"][0][0]
    search = _search(dev, name)
    search.step(_spelled(c, first).to(dev))
    rows = _state_rows(search)
    for b in range(c["B"]):                                # every row is inside the graph now, its loan out
        assert int(rows["bstate"].view(torch.int32)[b, 0]) == graph.states.index((first,))
        assert float(rows["bsum"].view(torch.float32)[b, 0]) == c["cs"]
    assert search.bias_score.tolist() == [0.0] * c["B"] and search.out_len.tolist() == [1] * c["B"]
    before = {k: v[2].cpu().clone() for k, v in rows.items()}
    kept = [t[2].clone() if t is not None else None for t in _outputs(search)]
    search.reset(rows=[0])
    for k, v in rows.items():                              # the other rows keep every byte
        assert torch.equal(before[k], v[2].cpu()), k
    assert int(rows["bstate"].view(torch.int32)[0, 0]) == 0 and float(rows["bsum"].view(torch.float32)[0, 0]) == 0.0
    assert int(rows["kept"].view(torch.int32)[0]) == 1 and int(rows["nb"].view(torch.int32)[0]) == 1
    if lm is not None:
        assert int(rows["ctx"].view(torch.int32)[0, 0]) == lm.start_ctx
    after = _outputs(search)
    assert int(after[1][0]) == 0 and float(after[4][0]) == 0.0
    for a, b in zip(kept, after):
        assert a is None or torch.equal(a, b[2])
    # the reset row then reads its utterance from the start; the others idle
    for ch, cl, _ in C.chunks(name, "uneven"):
        cl = cl.clone()
        cl[1:] = 0
        search.step(ch.to(dev), cl.to(dev))
    got = _outputs(search)
    _same_as_one_shot(got, _one_shot(dev, name), name, rows=[0])
    for a, b in zip(kept, got):
        assert a is None or torch.equal(a, b[2])


@pytest.mark.parametrize("name", ["b_v7_cancel", "b_v7_o2_cancel"])
def test_node_overflow_leaves_the_row_inert_with_its_bias_part_untouched(dev, name):
    c, x, lens, graph, lm = _case(dev, name)
    first = c["phrases"][0][0]
    search = _search(dev, name, max_nodes=1 + 2 * c["beam"])   # room for two frames, not for seven more
    search.step(_spelled(c, first).to(dev))
    rows = _state_rows(search)
    assert int(search.overflow[0]) == 0 and float(rows["bsum"].view(torch.float32)[0, 0]) == c["cs"]
    assert int(rows["bstate"].view(torch.int32)[0, 0]) == graph.states.index((first,))
    frozen, state = _outputs(search), {k: v.cpu().clone() for k, v in rows.items()}
    assert frozen[1].tolist() == [1] and frozen[0][0, 0] == first and float(frozen[4][0]) == 0.0
    for _ in range(2):                                     # the refused call, and a call on the inert row
        search.step(x[:, :7].contiguous())
        got = _outputs(search)
        assert int(got[6][0]) == 2
        for k, (a, b) in enumerate(zip(frozen, got)):
            assert k == 6 or a is None or torch.equal(a, b), k
        for k, v in rows.items():
            assert k == "ovf" or torch.equal(state[k], v.cpu()), k
    search.reset()
    assert int(search.overflow[0]) == 0
    search.step(x[:, :2].contiguous())
    _same_as_one_shot(_outputs(search), _one_shot(dev, name, [2]), name)


@pytest.mark.parametrize("name", ["b_v8_changes", "b_v63_o3_beam16_k16"])
def test_graph_capture_and_replays_over_a_stream(dev, name):
    """The chunk call captured once on a side stream and replayed for every chunk of a stream (the chunk
    tensors are fixed buffers) equals the eager run bit for bit, state included."""
    c = C.CASES[name]
    eager, replayed = _search(dev, name), _search(dev, name)
    Tc = 4
    ch_buf = torch.zeros(c["B"], Tc, c["V"], device=dev)
    cl_buf = torch.zeros(c["B"], dtype=torch.int64, device=dev)   # (idle for every row: the warm-up changes nothing)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        replayed.step(ch_buf, cl_buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.step(ch_buf, cl_buf)
    x, lens = C.make(name)
    for t0 in range(0, c["T"], Tc):
        ch = torch.full((c["B"], Tc, c["V"]), float("nan"))
        cl = (lens.clamp(max=c["T"]) - t0).clamp(0, Tc)
        for b in range(c["B"]):
            ch[b, :int(cl[b])] = x[b, t0:t0 + int(cl[b])]
        eager.step(ch.to(dev), cl.to(dev))
        ch_buf.copy_(ch)
        cl_buf.copy_(cl)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(_outputs(eager), _outputs(replayed)):
            assert a is None or torch.equal(a, b), t0
        assert torch.equal(eager.state, replayed.state), t0
    _same_as_one_shot(_outputs(replayed), _one_shot(dev, name), name)


def test_the_python_surface(dev):
    from speech2text_amd.model.ctc_bias import CtcBiasStreamingSearch, ctc_bias_streaming_search
    from speech2text_amd.model.decoding import CtcNgramStreamingSearch, CtcStreamingSearch
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    name = "b_v9_o3_changes"
    c = C.CASES[name]
    graph, lm = C.graph_of(name), C.model_of(name)          # CPU tables: copies follow the search
    s = ctc_bias_streaming_search(c["V"], batch_size=c["B"], beam_size=c["beam"], cutoff_top_k=c["topk"],
                                  max_tokens=c["T"], max_nodes=_MAX_NODES, device=dev, lm=lm, lm_weight=c["weight"], context=graph,
                                  context_weight=c["bias_weight"])
    assert type(s) is CtcBiasStreamingSearch and s.lm_score is not None and s.bias_score is not None
    assert graph.device.type == "cpu" and lm.device.type == "cpu" and s._context.device.type == "cuda"
    for ch, cl, _ in C.chunks(name, "whole"):
        s.step(ch.to(dev), cl.to(dev))
    _same_as_one_shot(_outputs(s), _one_shot(dev, name), name)
    t = ctc_bias_streaming_search(c["V"], device=dev, context=graph)
    assert type(t) is CtcBiasStreamingSearch and t.lm_score is None
    assert type(ctc_bias_streaming_search(c["V"], device=dev)) is CtcStreamingSearch     # no context: the factory's
    assert type(ctc_bias_streaming_search(c["V"], device=dev, lm=s._lm, lm_weight=0.3)) is CtcNgramStreamingSearch
    rnn = RnnLm(config=RnnLmConfig(num_symbols=c["V"], symbol_embedding_dim=8, num_rnn_layer=1)).to(dev).eval()
    for bad in (dict(method="greedy"), dict(lm=rnn), dict(lm=lm, lm_start_token=1), dict(context_weight=float("inf")),
                dict(beam_size=17)):
        with pytest.raises(ValueError):
            ctc_bias_streaming_search(c["V"], device=dev, **{"context": graph, **bad})
    with pytest.raises(ValueError):
        CtcBiasStreamingSearch(c["V"] + 1, device=dev, context=graph)          # graph.V != V
    with pytest.raises(ValueError):
        CtcBiasStreamingSearch(c["V"], device=dev, context=C.graph_of(name, torch.float64))


# ------------------------------------------------------------------ 3. the recogniser and the task
def test_recognizer_with_a_context_equals_the_class_on_its_one_shot_logits(dev, golden_dir):
    from speech2text_amd.model.ctc_bias import CtcBiasPrefixBeamDecoding, CtcBiasStreamingSearch
    from speech2text_amd.model.encoder.zipformer_streaming import CtcStreamingRecognizer
    from speech2text_amd.model.lm.context_graph import ContextGraph
    g, m, chunk, V = _tiny_ctc_encoder(golden_dir, dev)
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    plain = CtcStreamingRecognizer(m, _tokenizer(V), batch_size=B, device=dev, beam_size=4, cutoff_top_k=4,
                                   max_tokens=64, max_nodes=256)
    scores = []
    for k in range(6):
        scores.append(plain.step(feats[:, 2 * chunk * k:2 * chunk * k + T])[-1].clone())
    heard = plain.search.tokens[0, :int(plain.search.out_len[0])].tolist()
    assert len(heard) >= 3
    phrases = [heard[1:3], [heard[0], (heard[1] % (V - 1)) + 1], [V - 1, 1, 2]]     # one it says, two it may not
    graph = ContextGraph(phrases, V, context_score=0.8)
    rec = CtcStreamingRecognizer(m, _tokenizer(V), batch_size=B, device=dev, beam_size=4, cutoff_top_k=4,
                                 max_tokens=64, max_nodes=256, context=graph, context_weight=1.5)
    assert type(rec.search) is CtcBiasStreamingSearch
    dec = CtcBiasPrefixBeamDecoding(_tokenizer(V), beam_size=4, cutoff_top_k=4, context=graph, context_weight=1.5)
    for rep in range(2):
        rec.reset()
        for k in range(6):
            got = rec.step(feats[:, 2 * chunk * k:2 * chunk * k + T])
            assert len(got) == 5 and torch.equal(got[-1], scores[k])
        lens = torch.full((B,), 6 * Tc, dtype=torch.int64, device=dev)
        want = dec.beam_tokens(torch.cat(scores, dim=1), lens)
        s = rec.search
        assert len(want) == 4 and int(s.overflow.abs().sum()) == 0 and bool(s.bias_score.ne(0).any())
        assert torch.equal(s.out_len, want[1]) and torch.equal(s.score, want[2]) and torch.equal(s.bias_score, want[3])
        for b in range(B):
            n = int(want[1][b])
            assert torch.equal(s.tokens[b, :n], want[0][b, :n])
        assert all(t.startswith(u) for t, u in zip(rec.texts(), rec.stable_texts()))


def test_metric_hotwords_yaml_builds_the_class_and_the_recogniser(dev, tmp_path):
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.ctc_bias import CtcBiasPrefixBeamDecoding, CtcBiasStreamingSearch
    V, chunk = 32, 8
    cfg = copy.deepcopy(_ctc_zipformer_cfg(V, chunk))
    cfg["metric"].pop("lm")
    cfg["metric"].pop("lm_start_token")
    listing = tmp_path / "hotwords.txt"
    listing.write_text("abc\n\nbad\n")
    for hot in ({"phrases": ["abc", "bad"], "context_score": 0.5, "context_weight": 2.0},
                {"file": str(listing), "context_score": 0.5, "context_weight": 2.0}):
        cfg["metric"]["hotwords"] = hot
        torch.manual_seed(0)
        task = TaskFactory.get("CTC")(copy.deepcopy(cfg)).to(dev)
        task.eval()
        dec = task._metric._decode_sess
        assert type(dec) is CtcBiasPrefixBeamDecoding and dec._context_weight == 2.0
        want = [tuple(int(t) for t in task._tokenizer.encode(p)) for p in ("abc", "bad")]
        assert all(w in dec._context.states for w in want) and dec._context.context_score == 0.5
        assert "hotwords" not in task._metric_config and not any("context" in k for k in task.state_dict())
        rec = task.streaming_recognizer(batch_size=2)
        s = rec.search
        assert type(s) is CtcBiasStreamingSearch and (s.beam_size, s.cutoff_top_k, s._context_weight) == (3, 2, 2.0)
        assert torch.equal(s._context.arc_score.cpu(), dec._context.arc_score.cpu())
    feats = torch.randn(2, 150, 80, generator=torch.Generator().manual_seed(5)) * 2.0
    texts = rec.recognize(feats.to(dev), torch.tensor([150, 71]))
    assert len(texts) == 2 and int(s.overflow.abs().sum()) == 0 and bool(torch.isfinite(s.bias_score).all())
    cfg["metric"]["hotwords"] = {"phrases": ["abc"], "file": str(listing)}
    with pytest.raises(ValueError, match="either"):
        TaskFactory.get("CTC")(copy.deepcopy(cfg))
