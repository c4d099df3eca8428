"""GPU: the chunk-carried RNN-T beam search with hotword biasing, without an LM and fused with a back-off n-gram
(csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_bias_chunk, s2t_rnnt_beam_stateless_ngram_bias_chunk;
model/rnnt_bias.py RnntBiasStreamingSearch).

The yardstick is exact: however [0, L) is cut into chunks, tokens, frames, out_len, score, lm_score and bias_score
after a call are those of the one-shot entry (s2t_rnnt_beam_stateless_bias / _ngram_bias, themselves held to the
float64 restatement by tests/test_gpu_rnnt_bias.py) on the frames fed so far, bit for bit -- torch.equal, no
tolerance -- although the finalisation may report another beam after every call: nothing of its pick is carried.
`stable_len` is held to the float64 chunked restatement (tests/rnnt_bias_f64.py).
"""
import numpy as np
import pytest
import torch

import rnnt_bias_cases as C
import rnnt_bias_f64 as R
from decode_support import _feed, _regular

pytestmark = pytest.mark.gpu


def _search(dev, name, B=None, max_tokens=None, **kw):
    from speech2text_amd.model.rnnt_bias import RnntBiasStreamingSearch
    c, p, j, g, lm, am = C.device_case(dev, name)[:6]
    args = dict(lm=lm, lm_weight=c["weight"], context=g, context_weight=c["bias_weight"])
    args.update(kw)
    return RnntBiasStreamingSearch(p, j, am.shape[0] if B is None else B, c["beam"], c["topk"],
                                   am.shape[1] if max_tokens is None else max_tokens, dev, **args)


def _out_names(name):
    return ("tokens", "frames", "out_len", "score") + (("lm_score",) if C.CASES[name]["order"] else ()) + ("bias_score",)


def _outputs(search, name):
    torch.cuda.synchronize()
    return [getattr(search, k).cpu().clone() for k in _out_names(name)]


def _lens(name):
    c = C.CASES[name]
    return np.array([C.clamp(n, c["T"]) for n in C.make(name)[2].tolist()], dtype=np.int64)


def _ragged(lens, seed):
    """Per row its own cut points, pieces of 0..7 frames, and one call that idles every row."""
    g = np.random.default_rng(seed)
    rows = []
    for n in lens.tolist():
        sizes, left = [], n
        while left > 0:
            sizes.append(min(int(g.choice([0, 1, 1, 2, 3, 5, 7])), left))
            left -= sizes[-1]
        rows.append(sizes)
    K = max(len(r) for r in rows)
    plan = [np.array([r[k] if k < len(r) else 0 for r in rows], dtype=np.int64) for k in range(K)]
    plan.insert(K // 2, np.zeros(len(rows), dtype=np.int64))
    return plan


def _plan(name, cut):
    lens = _lens(name)
    return _ragged(lens, 11) if cut == "ragged" else _regular(lens, cut)


def _same(got, want, what):
    """Stream outputs against the one-shot entry's: bit for bit on the valid part of every row (a stream's arrays
    keep what an earlier, longer reported beam wrote past out_len)."""
    for b in range(len(want[2])):
        n = int(want[2][b])
        assert int(got[2][b]) == n, (what, b)
        assert torch.equal(got[0][b, :n], want[0][b, :n]) and torch.equal(got[1][b, :n], want[1][b, :n]), (what, b)
    for x, y in zip(got[3:], want[3:]):
        assert torch.equal(x, y), what


def _one_shot(dev, name, fed=None, **kw):
    case = C.device_case(dev, name)
    n = case[6] if fed is None else torch.as_tensor(fed, dtype=torch.int64)
    return [x.cpu() for x in C.fused(case, lens=n, **kw)]


def _stable_reference(name, plan):
    """Per call and row the chunked float64 restatement's common-prefix length."""
    c = C.CASES[name]
    p, am, _ = C.make(name)
    p = {k: v.numpy() for k, v in p.items()}
    rows = []
    for b in range(c["B"]):
        cuts = np.concatenate([[0], np.cumsum([int(cl[b]) for cl in plan])]).tolist()
        _, stable = R.beam_search_chunked(am[b, :cuts[-1]].numpy(), cuts, p, c["ctx"], c["act"], c["beam"], c["topk"],
                                          C.hot_of(name, np.float64), c["bias_weight"], C.dict_model(name, np.float64),
                                          c["weight"])
        rows.append(stable)
    return np.array(rows).T                                # [call][row]


def _bias_tail(search, name):
    """Per row the live beams' (bstate, bsum) bytes of the state: what the bias adds to the partner's row."""
    from speech2text_amd import _native as N
    c = C.CASES[name]
    B, beam = search.batch_size, search.beam_size
    query = N.lib().s2t_rnnt_ngram_stream_state_bytes if c["order"] else N.lib().s2t_rnnt_stream_state_bytes
    at = query(B, search.V, search.ctx, beam, search.max_tokens) // B
    torch.cuda.synchronize()
    rows = search.state.cpu().reshape(B, -1)
    out = []
    for b in range(B):
        nb = int(rows[b, :4].view(torch.int32)[0])
        tail = rows[b, at:at + 8 * beam].view(torch.int32)
        out.append((nb, tail[:nb].tolist(), tail[beam:beam + nb].tolist()))
    return out


# ------------------------------------------------------------------ 1. any cut is the one-shot search
@pytest.mark.parametrize("cut", [1, 4, 7, "ragged"], ids=str)
@pytest.mark.parametrize("name", list(C.CASES))
def test_chunks_equal_the_one_shot_search(dev, name, cut):
    c, ref = C.CASES[name], C.reference(name)
    am = C.device_case(dev, name)[5]
    plan = _plan(name, cut)
    if cut == "ragged" and c["B"] > 1:
        assert any((p == 0).any() and (p > 0).any() for p in plan)
    search = _search(dev, name)
    stable_want = _stable_reference(name, plan)
    seen, every = [], c["B"] * c["T"] <= 90                 # after every call where that is a few launches

    def snap(off, out):
        k = len(seen)
        seen.append(off)
        assert out[4].tolist() == stable_want[k].tolist(), (name, cut, k)
        if every or cut == 7:                              # the one-shot entry on the prefix fed so far
            _same(_outputs(search, name), _one_shot(dev, name, fed=off), (name, cut, k))

    _feed(search, am, plan, snap=snap)
    assert seen[-1].tolist() == _lens(name).tolist()
    got = _outputs(search, name)
    _same(got, _one_shot(dev, name), (name, cut))
    for b, r in enumerate(ref):                            # and so the float64 restatement's path
        assert got[0][b, :int(got[2][b])].tolist() == r.tokens and got[1][b, :int(got[2][b])].tolist() == r.frames
    assert search.overflow.tolist() == [0] * c["B"]
    # a second stream fed another cut ends in the same bias states and sums
    other = _search(dev, name)
    _feed(other, am, _plan(name, 4 if cut != 4 else 1))
    assert _bias_tail(other, name) == _bias_tail(search, name)
    assert torch.equal(other.bias_score, search.bias_score)


def test_a_cut_inside_a_phrase(dev):
    """An utterance that completes a phrase, cut right after each of its first tokens and right before the second:
    the reported hypothesis after such a call ends mid-phrase (the loan is taken back in the outputs only) and
    the next call goes on from the carried state: every prefix is the one-shot entry's, bit for bit."""
    for name in ("h_v11_kV", "h_long_o3"):
        refs = C.reference(name)
        b = next(i for i, r in enumerate(refs) if r.completions >= 1 and len(r.tokens) >= 4)
        r, L, hot = refs[b], int(_lens(name)[b]), C.hot_of(name, np.float64)
        am = C.device_case(dev, name)[5][b:b + 1].contiguous()
        search = _search(dev, name, B=1)
        cuts = sorted({f + 1 for f in r.frames[:6]} | {r.frames[1], L})
        mid, prev = 0, 0
        for t in cuts:
            if t == prev:
                continue
            search.step(am[:, prev:t].contiguous())
            got = _outputs(search, name)
            fed = [0] * C.CASES[name]["B"]
            fed[b] = t
            want = [x[b:b + 1] for x in _one_shot(dev, name, fed=fed)]
            _same(got, want, (name, t))
            tokens = tuple(got[0][0, :int(got[2][0])].tolist())
            mid += float(hot.bias_sum(tokens)) != float(hot.final_bias(tokens))
            prev = t
        assert mid >= 1, name


# ------------------------------------------------------------------ 2. reset, capacity
@pytest.mark.parametrize("name", ["h_v65_b17", "h_v65_b17_o3"])
def test_one_row_resets_while_its_neighbours_go_on(dev, name):
    """Row 3 is reset after two frames and fed utterance 0 from its first frame; the others go on."""
    c = C.CASES[name]
    am = C.device_case(dev, name)[5]
    lens, want = _lens(name), _one_shot(dev, name)
    assert lens[3] >= 2 and lens[0] == c["T"]
    search = _search(dev, name)
    plan = _regular(lens, 1)
    _, off = _feed(search, am, plan[:2])
    search.reset([3])
    torch.cuda.synchronize()
    assert float(search.bias_score[3]) == 0.0 and int(search.out_len[3]) == 0
    nb, bstate, bsum = _bias_tail(search, name)[3]
    assert (nb, bstate, bsum) == (1, [0], [0])             # the root, no sum
    am2 = am.clone()
    am2[3] = am[0]
    off[3] = 0
    rest = [p.copy() for p in plan[2:]]
    for k in range(c["T"]):                                # the new stream takes a frame per call
        if k < len(rest):
            rest[k][3] = 1
        else:
            rest.append(np.eye(1, c["B"], 3, dtype=np.int64)[0])
    _feed(search, am2, rest, off=off)
    got = _outputs(search, name)
    others = [b for b in range(c["B"]) if b != 3]
    _same([x[others] for x in got], [y[others] for y in want], name)
    _same([x[3:4] for x in got], [y[0:1] for y in want], name)
    assert int(want[2][0]) > 0 and float(want[-1].abs().max()) > 0


@pytest.mark.parametrize("name", C.LONG)
def test_capacity(dev, name):
    """max_tokens 3 on an utterance with more tokens: the first 3 of the reported beam, out_len 3, overflow 1, and
    the search went on exactly: the scores are the one-shot entry's, bit for bit."""
    am = C.device_case(dev, name)[5]
    want = _one_shot(dev, name)
    assert int(want[2].min()) > 3
    search = _search(dev, name, max_tokens=3)
    _feed(search, am, _plan(name, 7))
    got = _outputs(search, name)
    assert got[2].tolist() == [3] and search.overflow.tolist() == [1]
    assert torch.equal(got[0], want[0][:, :3]) and torch.equal(got[1], want[1][:, :3])
    for x, y in zip(got[3:], want[3:]):
        assert torch.equal(x, y)
    search.reset()
    torch.cuda.synchronize()
    assert search.overflow.tolist() == [0] and search.out_len.tolist() == [0] and search.bias_score.tolist() == [0.0]


def test_idle_call_changes_nothing(dev):
    name = "h_v65_b17_o3"
    am = C.device_case(dev, name)[5]
    search = _search(dev, name)
    _feed(search, am, _plan(name, 1)[:3])
    assert int(search.out_len.sum()) > 0
    outs = (search.state, search.tokens, search.frames, search.out_len, search.score, search.lm_score,
            search.bias_score, search.stable_len, search.overflow)
    before = [x.clone() for x in outs]
    search.step(am[:, :4].contiguous(), torch.zeros(am.shape[0], dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    for x, y in zip(outs, before):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 3. graph capture and replay
@pytest.mark.parametrize("name", ["h_v65_b17", "h_yaml_o3"])
def test_a_captured_step_replays_the_eager_search(dev, name):
    c = C.CASES[name]
    am = C.device_case(dev, name)[5]
    B, T, V = am.shape
    eager, graphed = _search(dev, name), _search(dev, name)
    Tc = 4
    buf = torch.zeros((B, Tc, V), device=dev)
    cl = torch.zeros((B,), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.step(buf, cl)                              # warm-up outside the capture (idle: chunk_len 0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step(buf, cl)
    lens = _lens(name)
    fed = np.zeros(B, dtype=np.int64)
    rows = torch.arange(B, device=dev).unsqueeze(1)
    for plan_cl in _regular(lens, Tc):
        idx = (torch.as_tensor(fed, device=dev).unsqueeze(1) + torch.arange(Tc, device=dev)).clamp(max=T - 1)
        chunk = am[rows, idx].contiguous()
        n = torch.as_tensor(plan_cl, dtype=torch.int64).to(dev)
        eager.step(chunk, n)
        buf.copy_(chunk)
        cl.copy_(n)
        graph.replay()
        fed += plan_cl
        torch.cuda.synchronize()
        for k in _out_names(name) + ("stable_len", "overflow"):
            assert torch.equal(getattr(graphed, k), getattr(eager, k)), (name, k, fed.tolist())
    assert torch.equal(graphed.state, eager.state)
    _same(_outputs(graphed, name), _one_shot(dev, name), name)
    assert c["beam"] > 1 and float(graphed.bias_score.abs().max()) > 0


# ------------------------------------------------------------------ 4. what the class refuses on the device
def test_class_refuses_what_the_entry_does_not_take(dev):
    import math
    from speech2text_amd.model.rnnt_bias import RnntBiasStreamingSearch, rnnt_bias_streaming_search
    name = "h_v11_kV_o2"
    c, p, j, g, lm = C.device_case(dev, name)[:5]
    s = rnnt_bias_streaming_search(p, j, 2, "beam", beam_size=4, cutoff_top_k=4, max_tokens=8, device=dev, lm=lm,
                                   lm_weight=0.3, context=C.graph_of(name), context_weight=1.0)
    assert isinstance(s, RnntBiasStreamingSearch) and s._context.device.type == "cuda"   # tables copied over
    assert s.bias_score.shape == (2,) and s.lm_score.shape == (2,)
    assert rnnt_bias_streaming_search(p, j, 2, "beam", device=dev, context=g).lm_score is None
    for kw in (dict(beam_size=17), dict(beam_size=0), dict(cutoff_top_k=0), dict(max_tokens=0),
               dict(context_weight=math.inf), dict(lm_weight=math.nan), dict(context=C.graph_of("h_v63_beam1_k1"))):
        args = dict(beam_size=4, cutoff_top_k=4, max_tokens=8, device=dev, lm=lm, lm_weight=0.3, context=g)
        args.update(kw)
        with pytest.raises(ValueError):
            RnntBiasStreamingSearch(p, j, 2, **args)
    _, jo = C.build_modules(dev, c["V"], c["E"], c["D"], c["ctx"], c["act"], inner=16)
    with pytest.raises(ValueError):
        RnntBiasStreamingSearch(p, jo, 2, device=dev, context=g)


# ------------------------------------------------------------------ 5. the recogniser and the task
def test_recognizer_with_a_context_equals_the_class_on_its_one_shot_am(dev, golden_dir):
    """StreamingRecognizer(context=).step (one graph replay a chunk) over the fixture's 6 chunks, twice across
    reset(): after the last chunk the search holds what RnntBiasBeamDecoding's fused entry gives on the
    concatenated am chunks, bit for bit, bias_score included; without an LM and with an NgramLm."""
    import ctc_ngram_cases as CN
    from decode_support import _beam_modules, _fixture_free_config, _tiny_stream_encoder, _tokenizer
    from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
    from speech2text_amd.model.lm.context_graph import ContextGraph
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    from speech2text_amd.model.rnnt_bias import RnntBiasStreamingSearch, rnnt_beam_bias_tokens_from_am
    g, m, chunk = _tiny_stream_encoder(golden_dir, dev)
    V, D = 24, max(m.encoder_dim)
    s = _fixture_free_config(V=V, D=D, E=16, ctx=3, seed=31, scale=2.0)
    s["enc_b"][0] += 4.0
    pred, join = _beam_modules(s, dev)
    pred.eval(), join.eval()
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    kw = dict(batch_size=B, device=dev, method="beam", beam_size=4, cutoff_top_k=4, max_tokens=64)
    plain = StreamingRecognizer(m, pred, join, _tokenizer(V), **kw)
    for k in range(6):
        plain.step(feats[:, 2 * chunk * k:2 * chunk * k + T])
    heard = plain.search.tokens[0, :int(plain.search.out_len[0])].tolist()
    assert len(heard) >= 3
    phrases = [heard[1:3], [heard[0], (heard[1] % (V - 1)) + 1], [V - 1, 1, 2]]     # one it says, two it may not
    graph = ContextGraph(phrases, V, context_score=0.8)
    for lm in (None, NgramLm.estimate(CN.lm_sequences(V, 200, 4), V, order=3)):
        rec = StreamingRecognizer(m, pred, join, _tokenizer(V), lm=lm, lm_weight=0.4 if lm is not None else 0.0,
                                  context=graph, context_weight=1.5, **kw)
        assert type(rec.search) is RnntBiasStreamingSearch
        for rep in range(2):
            rec.reset()
            ams = [rec.step(feats[:, 2 * chunk * k:2 * chunk * k + T])[-1].clone() for k in range(6)]
            lens = torch.full((B,), 6 * Tc, dtype=torch.int64, device=dev)
            want = rnnt_beam_bias_tokens_from_am(torch.cat(ams, dim=1), lens, pred, join, rec.search._context, 1.5,
                                                 rec.search._lm, 0.4, 4, 4)
            r = rec.search
            assert int(r.overflow.abs().sum()) == 0 and bool(r.bias_score.ne(0).any())
            assert torch.equal(r.out_len, want[2]) and torch.equal(r.score, want[3])
            assert torch.equal(r.bias_score, want[-1]) and (lm is None or torch.equal(r.lm_score, want[4]))
            for b in range(B):
                n = int(want[2][b])
                assert torch.equal(r.tokens[b, :n], want[0][b, :n]) and torch.equal(r.frames[b, :n], want[1][b, :n])
    with pytest.raises(ValueError, match="hotword"):
        StreamingRecognizer(m, pred, join, _tokenizer(V), batch_size=B, device=dev, method="greedy", context=graph)


def test_metric_hotwords_yaml_reaches_the_validation_search_and_the_recogniser(dev):
    import copy
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.rnnt_bias import RnntBiasBeamDecoding, RnntBiasStreamingSearch
    from speech2text_amd.model.utils import AsrMetric, AsrMetricConfig
    from task_support import _pruned_beam_cfg
    V, chunk = 32, 8
    cfg = _pruned_beam_cfg(V)
    cfg["encoder"]["config"].update({"chunk_size": [chunk], "left_context_frames": [16]})
    cfg["metric"] = dict(cfg["metric"], decode_method="rnnt_beam_search",
                         hotwords={"phrases": ["abc", "bad"], "context_score": 0.5, "context_weight": 2.0})
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(copy.deepcopy(cfg)).to(dev)
    task.eval()
    dec = task._metric._decode_sess
    assert type(dec) is RnntBiasBeamDecoding and dec._context_weight == 2.0 and dec._fusable()
    want = [tuple(int(t) for t in task._tokenizer.encode(p)) for p in ("abc", "bad")]
    assert all(w in dec._context.states for w in want) and dec._context.context_score == 0.5
    assert "hotwords" not in task._metric_config and not any("context" in k for k in task.state_dict())
    with torch.no_grad():
        for p in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            p.mul_(3.0)
    rec = task.streaming_recognizer(batch_size=2)
    s = rec.search
    assert type(s) is RnntBiasStreamingSearch and s._context_weight == 2.0
    assert torch.equal(s._context.arc_score.cpu(), dec._context.arc_score.cpu())
    feats = torch.randn(2, 150, 80, generator=torch.Generator().manual_seed(5)) * 2.0
    texts = rec.recognize(feats.to(dev), torch.tensor([150, 71]))
    assert len(texts) == 2 and int(s.overflow.abs().sum()) == 0 and bool(torch.isfinite(s.bias_score).all())
    enc = torch.randn(2, 9, dec._joiner._enc_proj.weight.shape[1], generator=torch.Generator().manual_seed(6)).to(dev)
    out = dec.beam_tokens(enc, torch.tensor([9, 5], device=dev))
    assert len(out) == 5 and out[-1].shape == (2,)
    cfg["metric"]["decode_method"] = "rnnt_greedy_search"                       # the greedy methods take no hotwords
    with pytest.raises(ValueError, match="hotwords"):
        TaskFactory.get("Pruned_Rnnt")(copy.deepcopy(cfg))
    with pytest.raises(ValueError, match="hotwords"):
        AsrMetric(task._tokenizer, AsrMetricConfig(decode_method="ctc_greedy_search"), context=dec._context)


@pytest.mark.parametrize("kind", ["Rnnt", "CTC_Hybrid_Rnnt"])
def test_metric_hotwords_reach_the_recogniser_of_the_other_rnnt_tasks(dev, kind):
    """RnntTask and CtcHybridRnnt (its RNN-T branch joins the encoder output beside the CTC head) inherit
    streaming_recognizer(): with metric.hotwords it builds the biased search, whose result on the recogniser's own
    am chunks is the one-shot bias entry's."""
    import copy
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.rnnt_bias import RnntBiasBeamDecoding, RnntBiasStreamingSearch, \
        rnnt_beam_bias_tokens_from_am
    from task_support import _pruned_beam_cfg
    V, chunk = 32, 8
    cfg = _pruned_beam_cfg(V)
    cfg["encoder"]["config"].update({"chunk_size": [chunk], "left_context_frames": [16]})
    cfg["task"] = dict(cfg["task"], type=kind)
    cfg["joiner"] = dict(cfg["joiner"], prune_range=-1)
    rnnt_loss = {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}}
    if kind == "Rnnt":
        cfg["loss"] = rnnt_loss
    else:
        cfg["decoder"] = {"model": "Projector", "config": {"input_dim": 64, "output_dim": V, "dropout_p": 0.1}}
        cfg["loss"] = {"rnnt_weight": 0.8, "ctc_weight": 0.2, "rnnt_loss": rnnt_loss,
                       "ctc_loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean"}}}
    cfg["metric"] = dict(cfg["metric"], decode_method="rnnt_beam_search",
                         hotwords={"phrases": ["abc", "bad"], "context_score": 0.5, "context_weight": 2.0})
    torch.manual_seed(0)
    task = TaskFactory.get(kind)(copy.deepcopy(cfg)).to(dev)
    task.eval()
    assert type(task._metric._decode_sess) is RnntBiasBeamDecoding
    with torch.no_grad():
        for p in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            p.mul_(3.0)
    rec = task.streaming_recognizer(batch_size=2)
    s = rec.search
    assert type(s) is RnntBiasStreamingSearch and (s.beam_size, s.cutoff_top_k, s._context_weight) == (3, 2, 2.0)
    feats = (torch.randn(2, 6 * 2 * chunk + 13, 80, generator=torch.Generator().manual_seed(5)) * 2.0).to(dev)
    T = 2 * chunk + 13
    ams = [rec.step(feats[:, 2 * chunk * k:2 * chunk * k + T])[-1].clone() for k in range(6)]
    lens = torch.full((2,), 6 * (chunk // 2), dtype=torch.int64, device=dev)
    want = rnnt_beam_bias_tokens_from_am(torch.cat(ams, dim=1), lens, task._predictor, task._joiner, s._context, 2.0,
                                         None, 0.0, 3, 2)
    assert int(s.overflow.abs().sum()) == 0 and torch.equal(s.out_len, want[2]) and torch.equal(s.score, want[3])
    assert torch.equal(s.bias_score, want[-1])
    for b in range(2):
        n = int(want[2][b])
        assert torch.equal(s.tokens[b, :n], want[0][b, :n]) and torch.equal(s.frames[b, :n], want[1][b, :n])
