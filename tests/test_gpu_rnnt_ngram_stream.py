"""GPU: the chunk-carried RNN-T beam search fused with a back-off n-gram (csrc/decode_rnnt.hip
s2t_rnnt_beam_stateless_ngram_chunk, model/decoding.py RnntNgramStreamingSearch), the StreamingRecognizer
graph around it and the RNN-T task's streaming_recognizer with an `lm: {arpa:}` section.

The yardstick is exact: however [0, L) is cut into chunks, tokens, frames, out_len, score and lm_score
are those of the one-shot entry (s2t_rnnt_beam_stateless_ngram, itself held to the float64 restatement
by tests/test_gpu_rnnt_ngram.py) on the frames fed so far, bit for bit -- torch.equal, no tolerance.
`stable_len` is held to the float64 chunked restatement (tests/rnnt_ngram_f64.py); the cases decide every
ranking cut by 1e-3 (tests/test_rnnt_ngram_f64.py), so the device keeps the restatement's beams.
"""
import copy
import math

import numpy as np
import pytest
import torch

import rnnt_ngram_cases as C
import rnnt_ngram_f64 as R
from decode_support import (_bad_desc, _beam_modules, _feed, _fixture_free_config, _fused, _lm_on, _ngram_case,
                            _regular, _same_rows, _tiny_stream_encoder, _tokenizer)
from task_support import _pruned_beam_cfg

pytestmark = pytest.mark.gpu

_OUT = ("tokens", "frames", "out_len", "score", "lm_score")


def _search(dev, name, B=None, max_tokens=None, lm_weight=None, **kw):
    from speech2text_amd.model.decoding import RnntNgramStreamingSearch
    c, p, j, lm, am, lens, _ = _ngram_case(dev, name)
    return RnntNgramStreamingSearch(p, j, am.shape[0] if B is None else B, c["beam"], c["topk"],
                                    am.shape[1] if max_tokens is None else max_tokens, dev, lm=lm,
                                    lm_weight=c["weight"] if lm_weight is None else lm_weight, **kw)


def _outputs(search):
    torch.cuda.synchronize()
    return [getattr(search, k).cpu().clone() for k in _OUT]


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
    """Stream outputs against the one-shot entry's: bit for bit on the valid part of every row (a stream's
    arrays keep what an earlier, longer best beam wrote past out_len)."""
    for b in range(len(want[2])):
        n = int(want[2][b])
        assert int(got[2][b]) == n, (what, b)
        assert torch.equal(got[0][b, :n], want[0][b, :n]) and torch.equal(got[1][b, :n], want[1][b, :n]), (what, b)
    assert torch.equal(got[3], want[3]), (what, "score")
    assert torch.equal(got[4], want[4]), (what, "lm_score")


def _one_shot(dev, name, fed=None, **kw):
    c, p, j, lm, am, lens, _ = _ngram_case(dev, name)
    n = lens if fed is None else torch.as_tensor(fed, dtype=torch.int64)
    return [x.cpu() for x in _fused(c, p, j, lm, am, n, **kw)]


def _stable_reference(name, plan):
    """Per call and row the chunked float64 restatement's common-prefix length."""
    c = C.CASES[name]
    p, am, _ = C.make(name)
    p = {k: v.numpy() for k, v in p.items()}
    rows = []
    for b in range(c["B"]):
        cuts = np.concatenate([[0], np.cumsum([int(cl[b]) for cl in plan])]).tolist()
        _, stable = R.beam_search_chunked(am[b, :cuts[-1]].numpy(), cuts, p, c["ctx"], c["act"], c["beam"], c["topk"],
                                          C.dict_model(name, np.float64), c["weight"])
        rows.append(stable)
    return np.array(rows).T                                # [call][row]


# ------------------------------------------------------------------ 1. any cut is the one-shot search
@pytest.mark.parametrize("cut", [1, 4, 7, "ragged"], ids=str)
@pytest.mark.parametrize("name", list(C.CASES))
def test_chunks_equal_the_one_shot_search(dev, name, cut):
    c, _, _, _, am, _, ref = _ngram_case(dev, name)
    plan = _plan(name, cut)
    if cut == "ragged" and c["B"] > 1:
        assert any((p == 0).any() and (p > 0).any() for p in plan)
    search = _search(dev, name)
    stable_want = _stable_reference(name, plan)
    seen = []

    def snap(off, out):
        k = len(seen)
        seen.append(off)
        assert out[4].tolist() == stable_want[k].tolist(), (name, cut, k)
        if cut == 7:                                       # after every chunk: the one-shot entry on the prefix
            _same(_outputs(search), _one_shot(dev, name, fed=off), (name, k))

    _feed(search, am, plan, snap=snap)
    assert seen[-1].tolist() == _lens(name).tolist()
    _same(_outputs(search), _one_shot(dev, name), (name, cut))
    got = _outputs(search)
    for b, r in enumerate(ref):                            # and so the float64 restatement's path
        assert got[0][b, :int(got[2][b])].tolist() == r.tokens and got[1][b, :int(got[2][b])].tolist() == r.frames
    assert search.overflow.tolist() == [0] * c["B"]
    assert bool((search.stable_len <= search.out_len).all())


# ------------------------------------------------------------------ 2. lm_weight 0 is the plain chunk entry
@pytest.mark.parametrize("name", ["g_v65_o3_b17", C.LARGE, "g_v520_o3"])
def test_weight_zero_is_the_plain_chunk_search(dev, name):
    from speech2text_amd.model.decoding import RnntStreamingSearch
    c, p, j, _, am, _, _ = _ngram_case(dev, name)
    plan = _plan(name, "ragged")
    ng = _search(dev, name, lm_weight=0.0)
    plain = RnntStreamingSearch(p, j, am.shape[0], "beam", beam_size=c["beam"], cutoff_top_k=c["topk"],
                                max_tokens=am.shape[1], device=dev)
    _feed(ng, am, plan)
    _feed(plain, am, plan)
    for k in ("tokens", "frames", "out_len", "score", "stable_len", "overflow"):
        assert torch.equal(getattr(ng, k), getattr(plain, k)), (name, k)
    assert int(ng.out_len.sum()) > 0 and float(ng.lm_score.abs().max()) > 0
    assert ng.state.numel() > plain.state.numel()


# ------------------------------------------------------------------ 3. idle rows, reset, capacity
def test_idle_call_changes_nothing(dev):
    name = "g_v65_o3_b17"
    _, _, _, _, am, _, _ = _ngram_case(dev, name)
    search = _search(dev, name)
    _feed(search, am, _plan(name, 1)[:3])
    assert int(search.out_len.sum()) > 0
    outs = (search.state, search.tokens, search.frames, search.out_len, search.score, search.lm_score,
            search.stable_len, search.overflow)
    before = [x.clone() for x in outs]
    search.step(am[:, :4].contiguous(), torch.zeros(am.shape[0], dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    for x, y in zip(outs, before):
        assert torch.equal(x, y)


@pytest.mark.parametrize("how", ["indices", "device mask"])
def test_one_row_resets_while_its_neighbours_go_on(dev, how):
    """Row 3 is reset after two frames and fed utterance 0 from its first frame; the others go on."""
    from speech2text_amd import _native as N
    name = "g_v65_o3_b17"
    c, _, _, lm, am, _, _ = _ngram_case(dev, name)
    lens, want = _lens(name), _one_shot(dev, name)
    assert lens[3] >= 2 and lens[0] == c["T"]
    search = _search(dev, name)
    plan = _regular(lens, 1)
    _, off = _feed(search, am, plan[:2])
    if how == "indices":
        search.reset([3])
    else:
        mask = torch.zeros(c["B"], dtype=torch.int32, device=dev)
        mask[3] = 1
        assert N.lib().s2t_rnnt_ngram_stream_reset(N.ptr(search.state), N.ip(mask), c["B"], c["V"], c["ctx"], c["beam"],
                                                   search.max_tokens, 0, int(lm.start_ctx), N.stream()) == 0
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
    got = _outputs(search)
    others = [b for b in range(c["B"]) if b != 3]
    _same([x[others] for x in got], [y[others] for y in want], how)
    _same([x[3:4] for x in got], [y[0:1] for y in want], how)   # restarted in start_ctx: utterance 0's own result
    assert int(want[2][0]) > 0 and float(want[4][0]) != 0.0


def test_capacity(dev):
    """max_tokens 3 on an utterance with more tokens: the first 3, out_len 3, overflow 1, and the search
    went on exactly: score and lm_score are the one-shot entry's, bit for bit."""
    name = C.LONG
    _, _, _, _, am, _, _ = _ngram_case(dev, name)
    want = _one_shot(dev, name)
    assert int(want[2].min()) > 3
    search = _search(dev, name, max_tokens=3)
    _feed(search, am, _plan(name, 7))
    got = _outputs(search)
    assert got[2].tolist() == [3] and search.overflow.tolist() == [1]
    assert torch.equal(got[0], want[0][:, :3]) and torch.equal(got[1], want[1][:, :3])
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
    search.reset()
    torch.cuda.synchronize()
    assert search.overflow.tolist() == [0] and search.out_len.tolist() == [0] and search.lm_score.tolist() == [0.0]


# ------------------------------------------------------------------ 4. refusals
def test_refusals_leave_state_and_outputs_untouched(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import _stateless_weights
    lib = N.lib()
    name = "g_v63_o5_beam16_k16"
    c, p, j, lm, am, _, _ = _ngram_case(dev, name)
    B, T, V = am.shape
    MT = 10
    w, E, D, ctx, act = _stateless_weights(p, j)
    need = lib.s2t_rnnt_ngram_stream_state_bytes(B, V, ctx, c["beam"], MT)
    plain = lib.s2t_rnnt_stream_state_bytes(B, V, ctx, c["beam"], MT)
    assert need % 256 == 0 and plain < need <= plain + 256 * B        # the plain row + ctx and lm_sum per beam
    for bad in ((0, V, ctx, 4, MT), (B, 0, ctx, 4, MT), (B, 8193, ctx, 4, MT), (B, V, 65, 4, MT), (B, V, ctx, 0, MT),
                (B, V, ctx, 17, MT), (B, V, ctx, 4, 0)):
        assert lib.s2t_rnnt_ngram_stream_state_bytes(*bad) == 0, bad
    state = torch.zeros(need, dtype=torch.uint8, device=dev)
    reset = dict(state=N.ptr(state), rows=None, B=B, V=V, ctx=ctx, beam=c["beam"], MT=MT, blank=0,
                 start=int(lm.start_ctx), stream=N.stream())
    assert lib.s2t_rnnt_ngram_stream_reset(*reset.values()) == 0
    outs = [torch.full((B, MT), 7, dtype=torch.int64, device=dev), torch.full((B, MT), 7, dtype=torch.int64, device=dev),
            torch.full((B,), 7, dtype=torch.int64, device=dev), torch.full((B,), 7.0, device=dev),
            torch.full((B,), 7.0, device=dev), torch.full((B,), 7, dtype=torch.int64, device=dev),
            torch.full((B,), 7, dtype=torch.int32, device=dev)]
    cl = torch.full((B,), 2, dtype=torch.int64, device=dev)
    args = dict(lm=lm.desc()[0], am=N.fp(am), cl=N.lp(cl), emb=N.fp(w[0]), conv_w=N.fp(w[1]), lin_w=N.fp(w[2]),
                lin_b=N.fp(w[3]), pre_w=N.fp(w[4]), pre_b=N.fp(w[5]), B=B, Tc=T, V=V, E=E, D=D, ctx=ctx, act=act, blank=0,
                beam=c["beam"], topk=c["topk"], weight=c["weight"], MT=MT, state=N.ptr(state), tokens=N.lp(outs[0]),
                frames=N.lp(outs[1]), out_len=N.lp(outs[2]), score=N.fp(outs[3]), lm_score=N.fp(outs[4]),
                stable=N.lp(outs[5]), overflow=N.ip(outs[6]), stream=N.stream())
    torch.cuda.synchronize()
    before = [t.clone() for t in [state] + outs]
    for change in (dict(rows=None, state=None), dict(ctx=65), dict(beam=17), dict(beam=0), dict(MT=0), dict(blank=V),
                   dict(start=-1)):
        assert lib.s2t_rnnt_ngram_stream_reset(*dict(reset, **change).values()) == -1, change
    assert lib.s2t_rnnt_ngram_stream_reset(*dict(reset, B=0).values()) == 0
    refused = [dict(lm=None), dict(desc=dict(arc_logp=None)), dict(desc=dict(V=64)), dict(desc=dict(order=9)),
               dict(desc=dict(num_ctx=0)), dict(desc=dict(num_arcs=62)), dict(weight=math.nan), dict(weight=-math.inf),
               dict(lm_score=None), dict(state=None), dict(Tc=0), dict(Tc=257), dict(V=8193), dict(E=0), dict(ctx=65),
               dict(act=2), dict(blank=63), dict(beam=0), dict(beam=17), dict(topk=0), dict(topk=17), dict(MT=0),
               dict(E=2000, D=2000)]
    for change in refused:
        a, held = dict(args), None
        for k, v in change.items():
            if k == "desc":
                a["lm"], held = _bad_desc(lm, **v)
            else:
                a[k] = v
        assert lib.s2t_rnnt_beam_stateless_ngram_chunk(*a.values()) == -1, change
        del held
    assert lib.s2t_rnnt_beam_stateless_ngram_chunk(*dict(args, B=0).values()) == 0
    torch.cuda.synchronize()
    for x, y in zip([state] + outs, before):
        assert torch.equal(x, y)
    assert lib.s2t_rnnt_beam_stateless_ngram_chunk(*args.values()) == 0                     # and the good call runs
    want = _one_shot(dev, name, fed=[2] * B)
    torch.cuda.synchronize()
    n = want[2]
    for b in range(B):
        assert int(outs[2][b]) == int(n[b]) and outs[0][b, :int(n[b])].tolist() == want[0][b, :int(n[b])].tolist()
    assert torch.equal(outs[3].cpu(), want[3]) and torch.equal(outs[4].cpu(), want[4])


def test_class_refuses_what_the_entry_does_not_take(dev):
    from speech2text_amd.model.decoding import RnntNgramStreamingSearch, rnnt_streaming_search
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    name = "g_v11_o2_kV"
    c, p, j, lm, _, _, _ = _ngram_case(dev, name)
    assert isinstance(rnnt_streaming_search(p, j, 2, "beam", beam_size=4, cutoff_top_k=4, max_tokens=8, device=dev,
                                            lm=lm, lm_weight=0.3), RnntNgramStreamingSearch)
    cpu = NgramLm.from_arpa(C.text_of(name), num_classes=c["V"])
    s = RnntNgramStreamingSearch(p, j, 2, device=dev, lm=cpu, lm_weight=0.3)               # tables copied over
    assert s._lm.device.type == "cuda" and cpu.device.type == "cpu" and s.lm_score.shape == (2,)
    for kw in (dict(beam_size=17), dict(beam_size=0), dict(cutoff_top_k=0), dict(max_tokens=0), dict(lm_weight=math.inf),
               dict(lm=None), dict(lm=_lm_on(dev, "g_v63_o1_beam1_k1"))):
        args = dict(beam_size=4, cutoff_top_k=4, max_tokens=8, device=dev, lm=lm, lm_weight=0.3)
        args.update(kw)
        with pytest.raises(ValueError):
            RnntNgramStreamingSearch(p, j, 2, **args)
    _, jo = C.build_modules(dev, c["V"], c["E"], c["D"], c["ctx"], c["act"], inner=16)
    with pytest.raises(ValueError):
        RnntNgramStreamingSearch(p, jo, 2, device=dev, lm=lm, lm_weight=0.3)
    with pytest.raises(ValueError, match="greedy"):
        rnnt_streaming_search(p, j, 2, "greedy", device=dev, lm=lm, lm_weight=0.3)


# ------------------------------------------------------------------ 5. the recogniser and the task
def test_recognizer_graph_equals_the_eager_composition(dev, golden_dir):
    """StreamingRecognizer(lm=NgramLm).step (one graph replay) against streaming_step -> _enc_proj ->
    RnntNgramStreamingSearch.step issued eagerly over the fixture's 6 chunks, twice across reset(); the
    final result is the one-shot n-gram entry's on the concatenated am chunks."""
    import ctc_ngram_cases as CN
    from speech2text_amd.model.decoding import RnntNgramStreamingSearch, rnnt_beam_ngram_tokens_from_am
    from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    g, m, chunk = _tiny_stream_encoder(golden_dir, dev)
    V, D = 24, max(m.encoder_dim)
    s = _fixture_free_config(V=V, D=D, E=16, ctx=3, seed=31, scale=2.0)
    s["enc_b"][0] += 4.0
    pred, join = _beam_modules(s, dev)
    pred.eval(), join.eval()
    lm = NgramLm.estimate(CN.lm_sequences(V, 200, 4), V, order=3)
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    rec = StreamingRecognizer(m, pred, join, _tokenizer(V), batch_size=B, device=dev, method="beam", beam_size=4,
                              cutoff_top_k=4, max_tokens=64, lm=lm, lm_weight=0.4)
    assert isinstance(rec.search, RnntNgramStreamingSearch) and lm.device.type == "cuda"
    eager = RnntNgramStreamingSearch(pred, join, B, 4, 4, 64, dev, lm=lm, lm_weight=0.4)
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
            assert torch.equal(rec.search.lm_score, eager.lm_score)
            ams.append(got[-1].clone())
        n = int(rec.search.out_len.sum())
        assert 0 < n < B * 6 * Tc
        lens = torch.full((B,), 6 * Tc, dtype=torch.int64)
        want = rnnt_beam_ngram_tokens_from_am(torch.cat(ams, dim=1), lens, pred, join, lm, 0.4, 4, 4)
        got = _outputs(rec.search)
        _same_rows(got[:4], [x.cpu() for x in want[:4]])
        assert torch.equal(got[4], want[4].cpu()) and float(got[4].abs().max()) > 0


def test_task_streaming_recognizer_builds_the_ngram_search(dev, tmp_path):
    import ctc_ngram_cases as CN
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.decoding import RnntNgramStreamingSearch
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    V, chunk = 32, 8
    cfg = _pruned_beam_cfg(V)
    cfg["encoder"]["config"].update({"chunk_size": [chunk], "left_context_frames": [16]})
    torch.manual_seed(0)
    plain = TaskFactory.get("Pruned_Rnnt")(copy.deepcopy(cfg))
    est = NgramLm.estimate(CN.lm_sequences(V, 200, 4), V, order=3)
    est.names = list(plain._tokenizer.labels)
    path = tmp_path / "pieces.arpa"
    path.write_text(est.to_arpa(), encoding="utf-8")
    cfg["metric"] = dict(cfg["metric"], decode_method="rnnt_beam_search", lm_weight=0.4, lm={"arpa": str(path)})
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(cfg).to(dev)
    task.eval()
    with torch.no_grad():
        for p in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            p.mul_(3.0)
    rec = task.streaming_recognizer(batch_size=2)
    assert isinstance(rec.search, RnntNgramStreamingSearch) and rec.search._lm_weight == 0.4
    assert rec.search._lm.num_classes == V and rec.search._lm.device.type == "cuda"
    with pytest.raises(ValueError):
        task.streaming_recognizer(batch_size=1, method="greedy", lm=rec.search._lm)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 150, 80, generator=g) * 2.0
    texts = rec.recognize(feats.to(dev), torch.tensor([150, 71]))
    assert any(len(t) for t in texts) and float(rec.search.lm_score.abs().max()) > 0
