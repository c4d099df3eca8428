"""GPU: the lockstep RNN-T beam search of the LSTM predictor fused with a back-off n-gram, whole and
chunk-carried (csrc/decode_lstm.hip s2t_rnnt_beam_lstm_ngram[_workspace_bytes], s2t_rnnt_lstm_ngram_stream_*,
s2t_rnnt_beam_lstm_ngram_chunk; model/decoding.py rnnt_beam_lstm_ngram_tokens_from_am,
RnntLstmNgramStreamingSearch, RnntBeamDecoding), and the StreamingRecognizer graph around it.

The one-shot entry is held to the float64 restatement tests/rnnt_lstm_ngram_f64.py on the cases of
tests/rnnt_lstm_ngram_cases.py (whose conditions tests/test_rnnt_lstm_ngram_f64.py asserts on the CPU):
tokens, frames and out_len exactly, score and lm_score within max(FLOOR, MARGIN x what float32 costs the
restatement); at lm_weight = 0 it is s2t_rnnt_beam_lstm bit for bit.  The chunk entry's yardstick is the
one-shot entry: for every partition, after EVERY chunk, torch.equal on the frames fed so far, lm_score
included; at lm_weight = 0 it is the plain chunk entry.  am of a chunk at and beyond chunk_len[b] is NaN.
"""
import ctypes
import functools
import math

import pytest
import torch

import rnnt_lstm_ngram_cases as C
from decode_support import _lstm_build, _lstm_pair, _ngram_lm, RECOGNIZER_BLANK, _tiny_stream_encoder, _tokenizer

pytestmark = pytest.mark.gpu


def _modules(dev, w, m):
    """The project's LstmPredictor + Joiner holding the weights `w` of the model dict m."""
    p, j = _lstm_build(dev, m["V"], m["E"], m["H"], m["D"], m["L"], m["ln"], m["inner"], m["act"])
    q = p.predictor._predictor
    with torch.no_grad():
        for dst, src in ((q.embedding.weight, "emb"), (q.input_layer_norm.weight, "in_g"),
                         (q.input_layer_norm.bias, "in_b"), (q.linear.weight, "lin_w"), (q.linear.bias, "lin_b"),
                         (q.output_layer_norm.weight, "out_g"), (q.output_layer_norm.bias, "out_b"),
                         (j._pre_proj.weight, "pre_w"), (j._pre_proj.bias, "pre_b")):
            dst.copy_(w[src])
        for lstm, lw in zip(q.lstm_layers, w["layers"]):
            lstm.x2g.weight.copy_(lw["x2g_w"])
            lstm.p2g.weight.copy_(lw["wp"])
            if m["ln"]:
                for mod, a, b in ((lstm.g_norm, "gg", "gb"), (lstm.c_norm, "cg", "cb")):
                    mod.weight.copy_(lw[a])
                    mod.bias.copy_(lw[b])
            else:
                lstm.x2g.bias.copy_(lw["x2g_b"])
        if m["inner"]:
            for lin, a, b in ((j._out_projection[0], "o1_w", "o1_b"), (j._out_projection[1], "o2_w", "o2_b")):
                lin.weight.copy_(w[a])
                lin.bias.copy_(w[b])
    return p, j


@functools.lru_cache(maxsize=None)
def _case(dev, name):
    """(case, predictor, joiner, LM, am and lengths on the device), built once per case."""
    c = C.CASES[name]
    w, _, am, lens = C.make(name)
    p, j = _modules(dev, w, c["m"])
    return c, p, j, _ngram_lm(dev, C.text_of(name), c["m"]["V"]), am.to(dev), lens.to(dev)


@functools.lru_cache(maxsize=None)
def _one_shot(dev, name, fed=None, weight=None):
    """The one-shot entry on the first fed[b] frames of every row (None: the whole utterances); shared."""
    from speech2text_amd.model.decoding import rnnt_beam_lstm_ngram_tokens_from_am
    c, p, j, lm, am, lens = _case(dev, name)
    if fed is not None:
        am, lens = am[:, :max(max(fed), 1)].contiguous(), torch.tensor(fed)
    out = rnnt_beam_lstm_ngram_tokens_from_am(am, lens, p, j, lm, c["weight"] if weight is None else weight,
                                              c["beam"], c["topk"])
    assert out is not None and len(out) == 5
    return [t.cpu() for t in out]


def _stream(dev, name, poison=True, **kw):
    from speech2text_amd.model.decoding import RnntLstmNgramStreamingSearch
    c, p, j, lm, am, _ = _case(dev, name)
    args = dict(beam_size=c["beam"], cutoff_top_k=c["topk"], max_tokens=c["T"], device=dev, lm=lm,
                lm_weight=c["weight"])
    args.update(kw)
    s = RnntLstmNgramStreamingSearch(p, j, am.shape[0], **args)
    if poison:                                             # reset must establish all a stream reads
        s.state.fill_(0xFF)
        s._ws.fill_(0xFF)
        s.reset()
    return s


def _plan(name, how):
    """-> [(Tc, [n_b])]: call i feeds row b its i-th piece of partition `how` (none left: an idle row)."""
    B = C.CASES[name]["B"]
    pieces = [[y - x for x, y in zip(c, c[1:])] for c in (C.cuts_of(name, b, how) for b in range(B))]
    out = []
    for i in range(max(len(p) for p in pieces)):
        ns = [p[i] if i < len(p) else 0 for p in pieces]
        out.append((max(1, max(ns)), ns))
    return out


def _chunks(dev, name, how):
    am = _case(dev, name)[4]
    B, _, V = am.shape
    pos = [0] * B
    for Tc, ns in _plan(name, how):
        ch = torch.full((B, Tc, V), float("nan"), device=dev)
        for b, n in enumerate(ns):
            ch[b, :n] = am[b, pos[b]:pos[b] + n]
            pos[b] += n
        yield ch, torch.tensor(ns, dtype=torch.int64, device=dev), list(pos)


def _outputs(s):
    return [t.cpu().clone() for t in (s.tokens, s.frames, s.out_len, s.score, s.lm_score, s.stable_len, s.overflow)]


def _same(got, want, what, rows=None):
    """got: _outputs of a stream; want: the one-shot entry's five."""
    for b in (range(got[2].shape[0]) if rows is None else rows):
        n = int(want[2][b])
        assert int(got[2][b]) == n, (what, b)
        assert torch.equal(got[0][b, :n], want[0][b, :n]) and torch.equal(got[1][b, :n], want[1][b, :n]), (what, b)
        assert got[3][b] == want[3][b] and got[4][b] == want[4][b], (what, b, got[3][b], want[3][b])


# ------------------------------------------------------------------ 1. the one-shot entry
@pytest.mark.parametrize("name", list(C.CASES))
def test_one_shot_entry_against_the_float64_restatement(dev, name):
    from speech2text_amd.model.decoding import rnnt_beam_lstm_tokens_from_am
    c, p, j, lm, am, lens = _case(dev, name)
    tokens, frames, out_len, score, lm_score = _one_shot(dev, name)
    ref = C.reference(name)
    for b, r in enumerate(ref):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == r.tokens and frames[b, :n].tolist() == r.frames, (name, b)
        if C.lengths(name)[b] == 0:                        # no frames: no tokens, score 0, lm_score 0
            assert n == 0 and float(score[b]) == 0.0 and float(lm_score[b]) == 0.0
    f64 = lambda i: torch.tensor([r[i] for r in ref], dtype=torch.float64)    # noqa: E731
    for what, got, i in (("score", score, 1), ("lm_score", lm_score, 2)):
        err = C.rel_err(got, f64(i))
        print(f"{name}: {what} rel_err {err:.3e} (bound {C.bound(name):.1e})")
        assert err <= C.bound(name), (name, what, err)
    plain = [t.cpu() for t in rnnt_beam_lstm_tokens_from_am(am, lens, p, j, c["beam"], c["topk"])]
    if name in C.LM_CHANGES:
        assert not torch.equal(tokens, plain[0]), "the LM changes no hypothesis"
    zero = _one_shot(dev, name, None, 0.0)                 # lm_weight = 0: the plain entry bit for bit
    for a, b in zip(plain, zero[:4]):
        assert torch.equal(a, b), name
    assert bool(torch.isfinite(zero[4]).all())


# ------------------------------------------------------------------ 2. the chunk entry
@pytest.mark.parametrize("how", C.PARTITIONS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_any_partition_equals_the_one_shot_entry_after_every_chunk(dev, name, how):
    c = C.CASES[name]
    s = _stream(dev, name)
    stable = None
    if c["B"] <= 3:                                        # stable_len: the float64 chunked restatement's
        stable = [C.chunked(name, b, how)[2] for b in range(c["B"])]
    last = None
    for i, (ch, cl, fed) in enumerate(_chunks(dev, name, how)):
        out = s.step(ch, cl)
        assert len(out) == 5
        got = _outputs(s)
        _same(got, _one_shot(dev, name, tuple(fed)), (name, how, i))
        assert int(got[6].abs().sum()) == 0
        if stable is not None:
            for b in range(c["B"]):
                if i < len(stable[b]) and fed[b] > 0:
                    assert int(got[5][b]) == stable[b][i], (name, how, i, b)
        if last is not None:
            assert bool((got[5] >= last[5]).all())
        last = got
    _same(last, _one_shot(dev, name), (name, how))


@pytest.mark.parametrize("name", ["n_v65_l1o_b17_beam4_k3", "n_v63_l2_b3_beam4_k3"])
def test_weight_zero_chunks_are_the_plain_chunk_entry(dev, name):
    from speech2text_amd.model.decoding import RnntLstmStreamingSearch
    c, p, j, _, am, _ = _case(dev, name)
    plain = RnntLstmStreamingSearch(p, j, c["B"], "beam", beam_size=c["beam"], cutoff_top_k=c["topk"],
                                    max_tokens=c["T"], device=dev)
    fused = _stream(dev, name, poison=False, lm_weight=0.0)
    for i, (ch, cl, _) in enumerate(_chunks(dev, name, "7")):
        plain.step(ch, cl)
        fused.step(ch, cl)
        for a, b in zip((plain.tokens, plain.frames, plain.out_len, plain.score, plain.stable_len, plain.overflow),
                        (fused.tokens, fused.frames, fused.out_len, fused.score, fused.stable_len, fused.overflow)):
            assert torch.equal(a, b), (name, i)
    n = plain.state.numel()                                # the plain state comes first, byte for byte
    assert torch.equal(plain.state, fused.state[:n])
    assert fused.state.numel() - n == 2 * ((4 * c["B"] * c["beam"] + 255) // 256 * 256)


def _rows_of(s, name):
    """The per-row arrays of the state by the header's layout -> {array: (outer, B, bytes per row) view}."""
    c = C.CASES[name]
    m, B, BS, MT = c["m"], c["B"], s.beam_size, s.max_tokens
    R = B * BS
    sizes = [("h", m["L"], 4 * BS * m["H"]), ("c", m["L"], 4 * BS * m["H"]), ("lm", 1, 4 * BS * m["V"]),
             ("hdr", 1, 16), ("score", 1, 4 * BS), ("blen", 1, 4 * BS), ("nb", 1, 4), ("htok", 1, 8 * BS * MT),
             ("hfrm", 1, 8 * BS * MT), ("ctx", 1, 4 * BS), ("lm_sum", 1, 4 * BS)]
    off, out = 0, {}
    for k, outer, per in sizes:
        n = outer * B * per
        out[k] = s.state[off:off + n].view(outer, B, per)
        off += (n + 255) // 256 * 256
    assert off == s.state.numel() and R > 0
    return out


def test_idle_rows_and_reset_of_some_rows(dev):
    name = "n_v63_l2_b3_beam4_k3"
    c, _, _, lm, am, lens = _case(dev, name)
    s = _stream(dev, name)
    rows = _rows_of(s, name)
    B, V = c["B"], c["m"]["V"]
    nan = torch.full((B, 5, V), float("nan"), device=dev)
    chunks = list(_chunks(dev, name, "7"))
    for i, (ch, cl, fed) in enumerate(chunks[:3]):
        if i in (0, 2):                                    # every row idle: state and outputs keep every bit
            before, state = _outputs(s), s.state.clone()
            s.step(nan, torch.zeros(B, dtype=torch.int64, device=dev))
            s.step(nan[:, :4].contiguous(), torch.full((B,), -3, dtype=torch.int64, device=dev))
            for a, b in zip(before, _outputs(s)):
                assert torch.equal(a, b), i
            assert torch.equal(state, s.state), i
        s.step(ch, cl)
    mid = _outputs(s)
    _same(mid, _one_shot(dev, name, tuple(fed)), "before the reset")
    # ---- reset row 0 alone: it restarts at <s>; the others keep every state byte
    keep = {k: v[:, 1:].cpu().clone() for k, v in rows.items()}
    s.reset(rows=[0])
    for k, v in rows.items():
        assert torch.equal(keep[k], v[:, 1:].cpu()), k
    assert int(rows["ctx"].view(torch.int32)[0, 0, 0]) == lm.start_ctx
    assert float(rows["lm_sum"].view(torch.float32)[0, 0, 0]) == 0.0
    after = _outputs(s)
    assert int(after[2][0]) == 0 and float(after[4][0]) == 0.0
    for a, b in zip(after, mid):
        assert torch.equal(a[2], b[2])
    for ch, cl, fed in chunks[:2]:                         # row 0 streams again from its first frame, row 2 idles
        cl = cl.clone()
        cl[1:] = 0
        s.step(ch, cl)
    got = _outputs(s)
    _same(got, _one_shot(dev, name, (fed[0], 0, 0)), "after the reset", rows=[0])
    for a, b in zip(got, mid):
        assert torch.equal(a[2], b[2])


def test_max_tokens_saturation_sets_bit_0(dev):
    name = "n_v63_l2_b3_beam4_k3"
    want = _one_shot(dev, name)
    cap = int(want[2].max()) // 2
    assert cap >= 2
    s = _stream(dev, name, max_tokens=cap)
    for ch, cl, _ in _chunks(dev, name, "16"):
        s.step(ch, cl)
    got = _outputs(s)
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])     # scores stay exact
    for b in range(got[2].shape[0]):
        n = int(want[2][b])
        assert int(got[2][b]) == min(n, cap) and int(got[6][b]) == (1 if n > cap else 0)
        assert torch.equal(got[0][b, :min(n, cap)], want[0][b, :min(n, cap)])
    assert int(got[6].sum()) > 0


def test_graph_capture_and_replays_over_a_stream(dev):
    name = "n_v65_l1o_b17_beam4_k3"
    c = C.CASES[name]
    eager, replayed = _stream(dev, name), _stream(dev, name)
    plan = _plan(name, "7")
    Tc = max(t for t, _ in plan)
    ch_buf = torch.zeros(c["B"], Tc, c["m"]["V"], device=dev)
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
    for i, (ch, cl, _) in enumerate(_chunks(dev, name, "7")):
        ch_buf.fill_(float("nan"))
        ch_buf[:, :ch.shape[1]] = ch
        cl_buf.copy_(cl)
        eager.step(ch_buf.clone(), cl)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(_outputs(eager), _outputs(replayed)):
            assert torch.equal(a, b), i
        assert torch.equal(eager.state, replayed.state), i
    _same(_outputs(replayed), _one_shot(dev, name), name)


# ------------------------------------------------------------------ 3. refusals
@pytest.mark.parametrize("change", [dict(Tc=0), dict(Tc=257), dict(state=None), dict(ws=None), dict(max_tokens=0),
                                    dict(beam=17), dict(beam=0), dict(topk=0), dict(topk=17), dict(lm=None),
                                    dict(lmV=64), dict(order=0), dict(order=9), dict(num_ctx=0), dict(num_arcs=62),
                                    dict(weight=math.inf), dict(weight=math.nan), dict(lm_score=None),
                                    dict(start=-1), dict(start="num_ctx"), dict(null="ctx_begin"),
                                    dict(null="arc_next"), dict(desc=None)], ids=str)
def test_entries_refuse_before_any_launch(dev, change):
    """One bad argument at a time through all six entries: -1 (the size functions 0), and the outputs,
    the state and the workspace of a stream in progress keep every bit."""
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnnt_lstm_desc
    lib = N.lib()
    name = "n_v63_l1_beam1_k1"
    c, p, j, lm, am, lens = _case(dev, name)
    B, T, V = am.shape
    s = _stream(dev, name, beam_size=4, cutoff_top_k=4)
    s.step(am[:, :4].contiguous(), torch.tensor([4, 0, 4], device=dev))
    before, state, ws = _outputs(s), s.state.clone(), s._ws.clone()
    desc, keep = rnnt_lstm_desc(p, j)
    ref, lkeep = lm.desc()
    d = type(lkeep[0]).from_buffer_copy(lkeep[0])          # a descriptor of our own to break
    if "lmV" in change:
        d.V = change["lmV"]
    for k in ("order", "num_ctx", "num_arcs"):
        if k in change:
            setattr(d, k, change[k])
    if "null" in change:
        setattr(d, change["null"], None)
    ld = None if "lm" in change else ctypes.byref(d)
    pd = None if "desc" in change else desc
    g = lambda k, dflt: change.get(k, dflt)                # noqa: E731
    beam, topk, MT = g("beam", 4), g("topk", 4), g("max_tokens", T)
    start = g("start", lm.start_ctx)
    start = lm.num_ctx if start == "num_ctx" else start
    statep = None if "state" in change else N.ptr(s.state)
    wsp = None if "ws" in change else N.ptr(s._ws)
    lmsp = None if "lm_score" in change else N.fp(s.lm_score)
    cl = torch.tensor([4, 0, 4], device=dev)
    x = am[:, :4].contiguous()
    desc_keys = {"lm", "lmV", "order", "num_ctx", "num_arcs", "null", "desc"}
    assert lib.s2t_rnnt_lstm_ngram_stream_state_bytes(desc, ref, B, 4, T) == s.state.numel()
    assert lib.s2t_rnnt_lstm_ngram_stream_workspace_bytes(desc, ref, B, 256, 4) == s._ws.numel()
    if "start" not in change:                              # (the chunk call takes no start context)
        assert lib.s2t_rnnt_beam_lstm_ngram_chunk(pd, ld, N.fp(x), N.lp(cl), B, g("Tc", 4), beam, topk, g("weight", 0.3),
                                                  MT, statep, wsp, N.lp(s.tokens), N.lp(s.frames), N.lp(s.out_len),
                                                  N.fp(s.score), lmsp, N.lp(s.stable_len), N.ip(s.overflow),
                                                  N.stream()) == -1
    if (desc_keys | {"state", "ws", "max_tokens", "beam"}) & set(change) or change.get("start") == -1:
        assert lib.s2t_rnnt_lstm_ngram_stream_reset(pd, ld, start, statep, None, B, beam, MT, wsp, N.stream()) == -1
    if (desc_keys | {"max_tokens", "beam"}) & set(change):
        assert lib.s2t_rnnt_lstm_ngram_stream_state_bytes(pd, ld, B, beam, MT) == 0
    if (desc_keys | {"beam", "Tc"}) & set(change):
        assert lib.s2t_rnnt_lstm_ngram_stream_workspace_bytes(pd, ld, B, g("Tc", 4), beam) == 0
    if (desc_keys | {"beam"}) & set(change):
        assert lib.s2t_rnnt_beam_lstm_ngram_workspace_bytes(pd, ld, B, T, beam) == 0
    if not {"Tc", "state", "max_tokens"} & set(change):    # what the one-shot entry takes
        n = lib.s2t_rnnt_beam_lstm_ngram_workspace_bytes(desc, ref, B, T, 4)
        assert n > 0
        big = torch.zeros(n, dtype=torch.uint8, device=dev)
        tok, frm = (torch.full((B, T), 7, dtype=torch.int64, device=dev) for _ in range(2))
        ol = torch.full((B,), 7, dtype=torch.int64, device=dev)
        sc, ls = torch.full((B,), 7.0, device=dev), torch.full((B,), 7.0, device=dev)
        assert lib.s2t_rnnt_beam_lstm_ngram(pd, ld, N.fp(am), N.lp(lens), B, T, beam, topk, g("weight", 0.3), start,
                                            None if "ws" in change else N.ptr(big), N.lp(tok), N.lp(frm), N.lp(ol),
                                            N.fp(sc), None if "lm_score" in change else N.fp(ls), N.stream()) == -1
        torch.cuda.synchronize()
        assert bool((tok == 7).all()) and bool((ol == 7).all()) and bool((sc == 7.0).all()) and bool((ls == 7.0).all())
    torch.cuda.synchronize()
    for a, b in zip(before, _outputs(s)):
        assert torch.equal(a, b)
    assert torch.equal(state, s.state) and torch.equal(ws, s._ws)
    del keep, lkeep


def test_empty_batch_and_the_class_surface(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import (RnntLstmNgramStreamingSearch, rnnt_beam_lstm_ngram_tokens_from_am,
                                                rnnt_lstm_desc, rnnt_streaming_search)
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    lib = N.lib()
    name = "n_v63_l1_beam1_k1"
    c, p, j, lm, am, lens = _case(dev, name)
    desc, keep = rnnt_lstm_desc(p, j)
    ref, lkeep = lm.desc()
    assert lib.s2t_rnnt_beam_lstm_ngram(desc, ref, None, None, 0, 5, 99, 99, math.nan, -1, None, None, None, None, None,
                                        None, N.stream()) == 0
    assert lib.s2t_rnnt_lstm_ngram_stream_reset(desc, ref, -1, None, None, 0, 99, 0, None, N.stream()) == 0
    assert lib.s2t_rnnt_beam_lstm_ngram_chunk(desc, ref, None, None, 0, 999, 99, 99, math.nan, 0, None, None, None,
                                              None, None, None, None, None, None, N.stream()) == 0
    del keep, lkeep
    assert rnnt_beam_lstm_ngram_tokens_from_am(am, lens, p, j, lm, 0.3, beam_size=17) is None
    with pytest.raises(RuntimeError, match="NgramLm.to"):
        rnnt_beam_lstm_ngram_tokens_from_am(am, lens, p, j, C.model(name), 0.3)
    with pytest.raises(ValueError, match="NgramLm"):       # (pinned: the factory keeps refusing the LSTM pair)
        rnnt_streaming_search(p, j, method="beam", lm=lm, lm_weight=0.5, device=dev)
    cpu = NgramLm.from_arpa(C.text_of(name), num_classes=63)
    s = RnntLstmNgramStreamingSearch(p, j, 2, device=dev, lm=cpu, lm_weight=0.3)           # tables copied over
    assert s._lm.device.type == "cuda" and cpu.device.type == "cpu" and s.lm_score.shape == (2,)
    assert s.method == "beam" and len(s.step(am[:2, :3].contiguous())) == 5
    other = _ngram_lm(dev, C.text_of("n_v65_l2_t90"), 65)
    for kw in (dict(beam_size=17), dict(beam_size=0), dict(cutoff_top_k=0), dict(max_tokens=0),
               dict(lm_weight=math.inf), dict(lm=None), dict(lm=other)):
        args = dict(beam_size=4, cutoff_top_k=4, max_tokens=8, device=dev, lm=lm, lm_weight=0.3)
        args.update(kw)
        with pytest.raises(ValueError):
            RnntLstmNgramStreamingSearch(p, j, 2, **args)


# ------------------------------------------------------------------ 4. the decoding class and the recogniser
@pytest.mark.parametrize("name", ["n_v11_l1o_beam16_kV", "n_v63_l2_b3_beam4_k3"])
def test_decoding_class_routes_the_lstm_pair_to_the_fused_entry(dev, name):
    import rnnt_ngram_cases as SN
    from speech2text_amd.model.decoding import RnntBeamDecoding
    c, p, j, lm, am, lens = _case(dev, name)
    dec = RnntBeamDecoding(SN.Ids(), p, j, beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"])
    fused = dec.beam_tokens(am, lens)                      # (the joiner's encoder projection is the identity here)
    assert len(fused) == 5
    for a, b in zip(fused, _one_shot(dev, name)):
        assert torch.equal(a.cpu(), b)
    loop = dec.beam_tokens(am, lens, fused=False)
    assert torch.equal(fused[0].cpu(), loop[0].cpu()) and torch.equal(fused[2].cpu(), loop[2].cpu())
    texts = dec.decode_batch(am, lens)
    T = am.shape[1]
    want = [dec._tokenizer.decode(dec._module_loop_lm(am[b:b + 1, :C.clamp(lens[b], T)])[0]) for b in range(am.shape[0])]
    assert texts == want and any(texts)


def test_recognizer_for_the_lstm_pair_equals_the_one_shot_call(dev, golden_dir):
    from speech2text_amd.model.decoding import RnntLstmNgramStreamingSearch, rnnt_beam_lstm_ngram_tokens_from_am
    from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
    import ctc_ngram_cases as CN
    g, m, chunk = _tiny_stream_encoder(golden_dir, dev)
    V, D = 24, max(m.encoder_dim)
    pred, join = _lstm_pair(dev, V, D, 31, RECOGNIZER_BLANK)
    lm = _ngram_lm(dev, CN.lm_text(V, 3, 200, 2), V)
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    rec = StreamingRecognizer(m, pred, join, _tokenizer(V), batch_size=B, device=dev, method="beam", beam_size=4,
                              cutoff_top_k=4, max_tokens=64, lm=lm, lm_weight=0.4)
    assert type(rec.search) is RnntLstmNgramStreamingSearch
    with pytest.raises(ValueError, match="lm_start_token"):
        StreamingRecognizer(m, pred, join, _tokenizer(V), batch_size=B, device=dev, method="beam", lm=lm,
                            lm_weight=0.4, lm_start_token=1)
    for rep in range(2):
        rec.reset()
        ams = [rec.step(feats[:, 2 * chunk * k:2 * chunk * k + T])[-1].clone() for k in range(6)]
        lens = torch.full((B,), 6 * Tc, dtype=torch.int64)
        want = [x.cpu() for x in rnnt_beam_lstm_ngram_tokens_from_am(torch.cat(ams, dim=1), lens, pred, join, lm, 0.4,
                                                                     4, 4)]
        _same(_outputs(rec.search), want, ("recogniser", rep))
        assert int(rec.search.out_len.sum()) > 0 and int(rec.search.overflow.sum()) == 0
        assert float(rec.search.lm_score.abs().max()) > 0
