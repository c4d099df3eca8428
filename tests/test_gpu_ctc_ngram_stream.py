"""GPU: the chunk-carried CTC prefix beam search fused with a back-off n-gram (csrc/decode_ctc.hip
s2t_ctc_ngram_stream_state_bytes, s2t_ctc_ngram_stream_reset, s2t_ctc_prefix_beam_ngram_chunk; model/decoding.py
CtcNgramStreamingSearch, ctc_streaming_search), the CtcStreamingRecognizer graph around it and
CtcTask.streaming_recognizer(lm=<NgramLm>).

The yardstick of the bits is the one-shot device entry (ctc_prefix_beam_ngram_tokens, itself held to
float64 by tests/test_gpu_ctc_ngram.py): however the frames of a case of tests/ctc_ngram_stream_cases.py are
cut, after EVERY call tokens[:out_len], out_len, score and lm_score are torch.equal to it on the frames fed
so far.  stable_len is held to the chunked restatement tests/ctc_ngram_stream_f64.py.  The COMPACTS cases run
with a max_nodes below the sequences they ever keep (tests/test_ctc_ngram_stream_f64.py asserts the
inequality): their equality without overflow shows the compaction at work and exact, context ids
included.  Every stream starts from a state buffer filled with 0xFF bytes (NaN floats, negative ids)
before its reset; frames of a chunk at and beyond chunk_len[b] are NaN in every call.
"""
import copy
import math

import pytest
import torch

import ctc_ngram_cases as G
import ctc_ngram_stream_cases as C
from decode_support import _lm_module, _ngram_lm, _tiny_ctc_encoder, _tokenizer
from task_support import _ctc_zipformer_cfg

pytestmark = pytest.mark.gpu

_CACHE, _PREFIX = {}, {}


def _case(dev, name):
    if name not in _CACHE:
        x, lens = G.make(name)
        _CACHE[name] = (C.CASES[name], x.to(dev), lens.to(dev), _ngram_lm(dev, G.text_of(name), C.CASES[name]["V"]))
    return _CACHE[name]


def _one_shot(dev, name, fed=None, **kw):
    """The one-shot entry on the first fed[b] frames of every row (None: the whole utterances), once per
    (case, fed, arguments)."""
    from speech2text_amd.model.decoding import ctc_prefix_beam_ngram_tokens
    key = (name, None if fed is None else tuple(fed), tuple(sorted(kw.items())))
    if key not in _PREFIX:
        c, x, lens, lm = _case(dev, name)
        if fed is not None:
            x, lens = x[:, :max(max(fed), 1)].contiguous(), torch.tensor(fed, device=dev)
        args = dict(lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"])
        args.update(kw)
        out = ctc_prefix_beam_ngram_tokens(x, lens, lm, **args)
        assert out is not None
        _PREFIX[key] = [t.cpu() for t in out]
    return _PREFIX[key]


def _search(dev, name, poison=True, **kw):
    from speech2text_amd.model.decoding import CtcNgramStreamingSearch
    c, _, _, lm = _case(dev, name)
    args = dict(batch_size=c["B"], beam_size=c["beam"], cutoff_top_k=c["topk"], max_tokens=c["T"],
                max_nodes=C.max_nodes(name), device=dev, lm=lm, lm_weight=c["weight"])
    args.update(kw)
    s = CtcNgramStreamingSearch(c["V"], **args)
    if poison:                                             # reset must establish all a stream reads
        s.state.fill_(0xFF)
        s.reset()
    return s


def _outputs(search):
    return [t.cpu().clone() for t in (search.tokens, search.out_len, search.score, search.stable_len,
                                      search.overflow, search.lm_score)]


def _same_as_one_shot(got, want, what):
    assert torch.equal(got[1], want[1]), (what, got[1], want[1])
    for b in range(got[0].shape[0]):
        n = int(want[1][b])
        assert torch.equal(got[0][b, :n], want[0][b, :n]), (what, b)
    assert torch.equal(got[2], want[2]), (what, got[2], want[2])
    assert torch.equal(got[5], want[3]), (what, got[5], want[3])


def _state_rows(search):
    """The state's arrays by the table in include/s2t_mi355.h: the plain layout, then ctx ->
    {array: (B, bytes per row) view of search.state}."""
    B, beam, M = search.batch_size, search.beam_size, search.max_nodes
    sizes = [("nodes", 16 * M), ("stage", 16 * M), ("map", 4 * M)]
    sizes += [(k, 4 * beam) for k in ("pb", "pnb", "lm_sum", "node", "last", "len")]
    sizes += [(k, 4) for k in ("nb", "kept", "depth", "ovf")] + [("eff", 8), ("ctx", 4 * beam)]
    off, out = 0, {}
    for k, per in sizes:
        out[k] = search.state[off:off + B * per].view(B, per)
        off += (B * per + 255) // 256 * 256
    assert off == search.state.numel()
    return out


# ------------------------------------------------------------------ 1. every case under every cut
@pytest.mark.parametrize("cut", C.CUTS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_any_cut_equals_the_one_shot_entry_after_every_call(dev, name, cut):
    search = _search(dev, name)
    reports = C.stream_reports(name, cut)
    last = None
    for i, (ch, cl, fed) in enumerate(C.chunks(name, cut)):
        out = search.step(ch.to(dev), cl.to(dev))
        assert len(out) == 4 and out[0] is search.tokens
        got = _outputs(search)
        assert int(got[4].abs().sum()) == 0, (name, cut, i, got[4])
        assert got[3].tolist() == [r.stable for r in reports[i]], (name, cut, i)
        _same_as_one_shot(got, _one_shot(dev, name, fed), (name, cut, "after call", i))
        if last is not None:
            assert bool((got[3] >= last[3]).all()), (name, cut, i)
            for b in range(got[0].shape[0]):
                s = int(last[3][b])
                assert torch.equal(got[0][b, :s], last[0][b, :s]), (name, cut, i, b)
        last = got
    _same_as_one_shot(last, _one_shot(dev, name), (name, cut))
    for b, r in enumerate(G.reference(name)):              # (and so the float64 restatement's tokens)
        assert last[0][b, :int(last[1][b])].tolist() == r.tokens, (name, cut, b)
    if name in C.COMPACTS:
        rows = _state_rows(search)
        kept = rows["kept"].view(torch.int32).reshape(-1).tolist()
        assert kept == [r.kept for r in reports[-1]], (name, cut, kept)
        print(f"{name} {cut}: max_nodes {C.max_nodes(name)}, sequences ever kept "
              f"{[r.ever for r in reports[-1]]}, kept at the end {kept}")


@pytest.mark.parametrize("name", list(C.CASES))
def test_weight_zero_is_the_plain_chunk_entry(dev, name):
    from speech2text_amd.model.decoding import CtcStreamingSearch
    c = C.CASES[name]
    plain = CtcStreamingSearch(c["V"], batch_size=c["B"], beam_size=c["beam"], cutoff_top_k=c["topk"],
                               max_tokens=c["T"], max_nodes=C.max_nodes(name), device=dev)
    fused = _search(dev, name, poison=False, lm_weight=0.0)
    for i, (ch, cl, _) in enumerate(C.chunks(name, "ragged")):
        plain.step(ch.to(dev), cl.to(dev))
        fused.step(ch.to(dev), cl.to(dev))
        for a, b in zip((plain.tokens, plain.out_len, plain.score, plain.stable_len, plain.overflow),
                        _outputs(fused)[:5]):
            assert torch.equal(a.cpu(), b), (name, i)
    assert bool(torch.isfinite(fused.lm_score).all())
    rows = _state_rows(fused)                              # the plain state comes first, byte for byte
    n = plain.state.numel()
    skip = rows["lm_sum"].data_ptr() - fused.state.data_ptr()
    per = rows["lm_sum"].numel()
    assert torch.equal(plain.state[:skip], fused.state[:skip])
    assert torch.equal(plain.state[skip + per:n], fused.state[skip + per:n])
    assert fused.state.numel() - n == (4 * c["B"] * c["beam"] + 255) // 256 * 256


# ------------------------------------------------------------------ 2. overflow, idle calls, reset, graphs
def test_node_overflow_makes_the_row_inert_until_reset(dev):
    name, cut = "n_v128_o3_beam4_k4", "r7"
    c, x, lens, lm = _case(dev, name)
    needs = C.row_needs(name, cut)
    assert needs[0] != needs[1], needs
    bad, good = (0, 1) if needs[0] > needs[1] else (1, 0)
    limit = max(needs) - 1                                 # one cut exceeds it, in one row
    assert limit >= needs[good]
    reports = C.stream_reports(name, cut, limit)
    first = next(i for i, row in enumerate(reports) if row[bad].overflow)
    assert first > 0 and not any(row[good].overflow for row in reports)
    search = _search(dev, name, max_nodes=limit)
    rows = _state_rows(search)
    frozen = None
    for i, (ch, cl, fed) in enumerate(C.chunks(name, cut)):
        search.step(ch.to(dev), cl.to(dev))
        got = _outputs(search)
        assert got[4].tolist() == [2 if r.overflow else 0 for r in reports[i]], (i, got[4])
        mine = {k: v[bad].cpu().clone() for k, v in rows.items()}
        if i == first - 1:
            frozen = ([t[bad].clone() for t in got], mine)
        if i >= first:                                     # outputs and state as before the refused call ...
            for k, (a, b) in enumerate(zip(frozen[0], got)):
                assert k == 4 or torch.equal(a, b[bad]), (i, k)
            for k in mine:
                assert k == "ovf" or torch.equal(frozen[1][k], mine[k]), (i, k)
            assert int(mine["ovf"].view(torch.int32)) == 2     # ... but for the bit that makes it inert
    want, got = _one_shot(dev, name), _outputs(search)
    n = int(want[1][good])
    assert int(got[1][good]) == n and torch.equal(got[0][good, :n], want[0][good, :n])
    assert got[2][good] == want[2][good] and got[5][good] == want[3][good]
    # ---- reset(rows=[bad]) restarts that row at <s>; the other row's state keeps every byte
    before = {k: v[good].cpu().clone() for k, v in rows.items()}
    search.reset(rows=[bad])
    for k, v in rows.items():
        assert torch.equal(before[k], v[good].cpu()), k
    assert int(rows["ctx"].view(torch.int32)[bad, 0]) == lm.start_ctx
    assert float(rows["lm_sum"].view(torch.float32)[bad, 0]) == 0.0 and int(rows["kept"].view(torch.int32)[bad]) == 1
    after = _outputs(search)
    assert int(after[4][bad]) == 0 and int(after[1][bad]) == 0 and float(after[5][bad]) == 0.0
    for ch, cl, fed in C.chunks(name, "r4")[:3]:
        cl = cl.clone()
        cl[good] = 0
        search.step(ch.to(dev), cl.to(dev))
    fed = [0, 0]
    fed[bad] = 12
    short, got2 = _one_shot(dev, name, fed), _outputs(search)
    n = int(short[1][bad])
    assert n > 0 and int(got2[1][bad]) == n and torch.equal(got2[0][bad, :n], short[0][bad, :n])
    assert got2[2][bad] == short[2][bad] and got2[5][bad] == short[3][bad] and int(got2[4][bad]) == 0
    for t2, t1 in zip(got2, got):
        assert torch.equal(t2[good], t1[good])


def test_token_overflow_keeps_the_first_tokens_and_exact_scores(dev):
    name = "n_v128_o3_beam4_k4"
    c = C.CASES[name]
    want = _one_shot(dev, name)
    cap = int(want[1].max()) // 2
    assert cap >= 2
    search = _search(dev, name, max_tokens=cap)
    for ch, cl, _ in C.chunks(name, "r4"):
        search.step(ch.to(dev), cl.to(dev))
    got = _outputs(search)
    assert torch.equal(got[2], want[2]) and torch.equal(got[5], want[3])
    for b in range(c["B"]):
        n = int(want[1][b])
        assert int(got[1][b]) == min(n, cap) and torch.equal(got[0][b, :min(n, cap)], want[0][b, :min(n, cap)])
        assert int(got[4][b]) == (1 if n > cap else 0) and int(got[3][b]) <= cap
    assert int(got[4].sum()) > 0


@pytest.mark.parametrize("name", ["n_v63_o5_beam16_k16", "n_v11_o2_b17_beam4_k3"])
def test_idle_calls_change_nothing(dev, name):
    c = C.CASES[name]
    search = _search(dev, name)
    nan = torch.full((c["B"], 5, c["V"]), float("nan"), device=dev)
    for i, (ch, cl, _) in enumerate(C.chunks(name, "r4")):
        if i in (0, 2):                                    # before the first frame, and between two chunks
            before, state = _outputs(search), search.state.clone()
            search.step(nan, torch.zeros(c["B"], dtype=torch.int64, device=dev))
            search.step(nan, torch.full((c["B"],), -3, dtype=torch.int64, device=dev))
            for a, b in zip(before, _outputs(search)):
                assert torch.equal(a, b), (name, i)
            assert torch.equal(state, search.state), (name, i)
        search.step(ch.to(dev), cl.to(dev))
    _same_as_one_shot(_outputs(search), _one_shot(dev, name), name)


def test_direct_entries_on_poisoned_guarded_buffers(dev):
    """The three entries called by hand: state and outputs lie between guard bytes, everything is
    poisoned before the reset, and a reset row restarts in start_ctx whatever it held."""
    from speech2text_amd import _native as N
    lib = N.lib()
    name = "n_v11_o2_b17_beam4_k3"
    c, x, lens, lm = _case(dev, name)
    B, V, beam, topk, T, M = c["B"], c["V"], c["beam"], c["topk"], c["T"], C.max_nodes(name)
    n = lib.s2t_ctc_ngram_stream_state_bytes(B, V, beam, M)
    assert n == lib.s2t_ctc_stream_state_bytes(B, V, beam, M) + (4 * B * beam + 255) // 256 * 256 and n % 256 == 0
    G_ = 512
    buf = torch.full((n + 2 * G_,), 0xFF, dtype=torch.uint8, device=dev)
    state = buf[G_:G_ + n]
    tok = torch.full((B + 2, T), -7, dtype=torch.int64, device=dev)
    ilen, stab = (torch.full((B + 2,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    score, lms = (torch.full((B + 2,), float("nan"), device=dev) for _ in range(2))
    ovf = torch.full((B + 2,), -7, dtype=torch.int32, device=dev)
    desc, keep = lm.desc()
    assert lib.s2t_ctc_ngram_stream_reset(N.ptr(state), None, B, V, beam, M, int(lm.start_ctx), N.stream()) == 0
    for ch, cl, fed in C.chunks(name, "r7"):
        ch, cl = ch.to(dev), cl.to(dev)
        assert lib.s2t_ctc_prefix_beam_ngram_chunk(desc, N.fp(ch), N.lp(cl), B, ch.shape[1], V, 0, beam, topk,
                                                   c["weight"], T, M, N.ptr(state), N.lp(tok[1:]), N.lp(ilen[1:]),
                                                   N.fp(score[1:]), N.fp(lms[1:]), N.lp(stab[1:]), N.ip(ovf[1:]),
                                                   N.stream()) == 0
    torch.cuda.synchronize()
    want = _one_shot(dev, name)
    live = [b for b in range(B) if int(lens[b]) > 0]       # (a row that never had a frame keeps its poison)
    assert len(live) < B
    for b in range(B):
        if b in live:
            k = int(want[1][b])
            assert int(ilen[1 + b]) == k and tok[1 + b, :k].cpu().tolist() == want[0][b, :k].tolist()
            assert float(score[1 + b]) == float(want[2][b]) and float(lms[1 + b]) == float(want[3][b])
            assert int(ovf[1 + b]) == 0
        else:
            assert int(ilen[1 + b]) == -7 and math.isnan(float(score[1 + b])) and int(ovf[1 + b]) == -7
    for t in (tok, ilen, stab, ovf):
        assert bool((t[0] == -7).all()) and bool((t[-1] == -7).all())
    assert bool(torch.isnan(score[[0, -1]]).all()) and bool(torch.isnan(lms[[0, -1]]).all())
    assert bool((buf[:G_] == 0xFF).all()) and bool((buf[G_ + n:] == 0xFF).all())
    # a start context beyond the table is clamped by the chunk call, not followed
    assert lib.s2t_ctc_ngram_stream_reset(N.ptr(state), None, B, V, beam, M, 1 << 30, N.stream()) == 0
    ch, cl, _ = C.chunks(name, "r4")[0]
    ch, cl = ch.to(dev), cl.to(dev)
    assert lib.s2t_ctc_prefix_beam_ngram_chunk(desc, N.fp(ch), N.lp(cl), B, 4, V, 0, beam, topk, c["weight"], T, M,
                                               N.ptr(state), N.lp(tok[1:]), N.lp(ilen[1:]), N.fp(score[1:]),
                                               N.fp(lms[1:]), N.lp(stab[1:]), N.ip(ovf[1:]), N.stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lms[1:1 + B][cl > 0]).all())
    del keep


def test_graph_capture_and_replays_over_a_stream(dev):
    """The chunk call captured once on a side stream and replayed for every chunk of a stream (the chunk
    tensors are fixed buffers) equals the eager run bit for bit, state included."""
    name = "n_v65_o3_b33_beam4_k3_norm"
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
    for i, (ch, cl, _) in enumerate(C.chunks(name, "r4")):
        eager.step(ch.to(dev), cl.to(dev))
        ch_buf.copy_(ch)
        cl_buf.copy_(cl)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(_outputs(eager), _outputs(replayed)):
            assert torch.equal(a, b), i
        assert torch.equal(eager.state, replayed.state), i
    _same_as_one_shot(_outputs(replayed), _one_shot(dev, name), name)


# ------------------------------------------------------------------ 3. refusals
_V = 32


@pytest.mark.parametrize("change", [dict(Tc=0), dict(Tc=257), dict(state=None), dict(max_nodes=0),
                                    dict(max_nodes=1048577), dict(max_tokens=0), dict(beam=17), dict(beam=0),
                                    dict(topk=0), dict(topk=17), dict(V=8193), dict(V=0), dict(blank=-1),
                                    dict(blank=_V), dict(lm=None), dict(lmV=_V + 1), dict(order=0), dict(order=9),
                                    dict(num_ctx=0), dict(num_arcs=_V - 1), dict(weight=math.inf),
                                    dict(weight=math.nan), dict(lm_score=None), dict(start=-1),
                                    dict(null="ctx_begin"), dict(null="ctx_fail"), dict(null="ctx_backoff"),
                                    dict(null="arc_token"), dict(null="arc_logp"), dict(null="arc_next")], ids=str)
def test_entries_refuse_before_any_launch(dev, change):
    """One bad argument at a time: -1 (the size function 0), and the outputs and the state of a stream in
    progress keep every bit.  No pointer is followed: logits and state are far too small for V 8193 or
    1048577 nodes."""
    import ctypes
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import CtcNgramStreamingSearch
    lib = N.lib()
    lm = _ngram_lm(dev, G.lm_text(_V, 3, 200, 2), _V)
    s = CtcNgramStreamingSearch(_V, batch_size=2, beam_size=4, cutoff_top_k=4, max_tokens=8, max_nodes=64,
                                device=dev, lm=lm, lm_weight=0.3)
    x = torch.randn(2, 4, _V, generator=torch.Generator().manual_seed(3)).to(dev)
    s.step(x)
    assert int(s.out_len.sum()) > 0
    before, state = _outputs(s), s.state.clone()
    cl = torch.full((2,), 4, dtype=torch.int64, device=dev)
    ref, keep = lm.desc()
    d = type(keep[0]).from_buffer_copy(keep[0])            # a descriptor of our own to break
    if "lmV" in change:
        d.V = change["lmV"]
    for k in ("order", "num_ctx", "num_arcs"):
        if k in change:
            setattr(d, k, change[k])
    if "null" in change:
        setattr(d, change["null"], None)
    desc = None if "lm" in change else ctypes.byref(d)
    g = lambda k, dflt: change.get(k, dflt)                # noqa: E731
    V, beam, max_nodes = g("V", _V), g("beam", 4), g("max_nodes", 64)
    statep = None if "state" in change else N.ptr(s.state)
    lmsp = None if "lm_score" in change else N.fp(s.lm_score)
    if "start" not in change:
        assert lib.s2t_ctc_prefix_beam_ngram_chunk(desc, N.fp(x), N.lp(cl), 2, g("Tc", 4), V, g("blank", 0), beam,
                                                   g("topk", 4), g("weight", 0.3), g("max_tokens", 8), max_nodes,
                                                   statep, N.lp(s.tokens), N.lp(s.out_len), N.fp(s.score), lmsp,
                                                   N.lp(s.stable_len), N.ip(s.overflow), N.stream()) == -1
    if {"state", "max_nodes", "beam", "V", "start"} & set(change):     # what the reset takes
        assert lib.s2t_ctc_ngram_stream_reset(statep, None, 2, V, beam, max_nodes, g("start", lm.start_ctx),
                                              N.stream()) == -1
    if {"max_nodes", "beam", "V"} & set(change):
        assert lib.s2t_ctc_ngram_stream_state_bytes(2, V, beam, max_nodes) == 0
    torch.cuda.synchronize()
    for a, b in zip(before, _outputs(s)):
        assert torch.equal(a, b)
    assert torch.equal(state, s.state)
    del ref, keep


def test_empty_batch_and_the_python_surface(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import CtcNgramStreamingSearch, CtcStreamingSearch, ctc_streaming_search
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    lib = N.lib()
    lm = _ngram_lm(dev, G.lm_text(_V, 3, 200, 2), _V)
    desc, keep = lm.desc()
    assert lib.s2t_ctc_ngram_stream_state_bytes(0, _V, 4, 64) == 0
    assert lib.s2t_ctc_ngram_stream_reset(None, None, 0, _V, 99, 0, -1, N.stream()) == 0
    assert lib.s2t_ctc_prefix_beam_ngram_chunk(desc, None, None, 0, 999, _V, 0, 99, 99, math.nan, 0, 0, None, None,
                                               None, None, None, None, None, N.stream()) == 0
    del keep
    s = ctc_streaming_search(_V, batch_size=2, max_tokens=8, max_nodes=64, device=dev, lm=lm, lm_weight=0.3)
    assert type(s) is CtcNgramStreamingSearch and s.method == "beam" and s.lm_score is not None
    assert type(ctc_streaming_search(_V, device=dev)) is CtcStreamingSearch
    assert type(ctc_streaming_search(_V, device=dev, lm=_lm_module(dev, V=_V, H=8, layers=1))) is CtcStreamingSearch
    assert ctc_streaming_search(_V, method="greedy", device=dev).method == "greedy"
    with pytest.raises(ValueError):                        # greedy takes no LM: CtcStreamingSearch says so
        ctc_streaming_search(_V, method="greedy", device=dev, lm=lm)
    with pytest.raises(ValueError, match="lm_start_token"):
        ctc_streaming_search(_V, device=dev, lm=lm, lm_start_token=1)
    with pytest.raises(ValueError, match="NgramLm"):
        CtcStreamingSearch(_V, lm=lm, lm_weight=0.5, device=dev)
    with pytest.raises(ValueError, match="NgramLm"):
        CtcNgramStreamingSearch(_V, device=dev, lm=_lm_module(dev, V=_V, H=8, layers=1))
    with pytest.raises(ValueError):
        CtcNgramStreamingSearch(_V + 1, device=dev, lm=lm)                      # lm.V != V
    with pytest.raises(ValueError):
        CtcNgramStreamingSearch(_V, device=dev, lm=lm, lm_weight=math.inf)
    with pytest.raises(ValueError):
        CtcNgramStreamingSearch(_V, device=dev, lm=lm, beam_size=17)
    with pytest.raises(ValueError):
        s.step(torch.zeros(2, 257, _V, device=dev))
    host = NgramLm.from_arpa(G.lm_text(_V, 3, 200, 2), num_classes=_V)         # CPU tables: a copy follows the search
    t = CtcNgramStreamingSearch(_V, batch_size=2, max_tokens=8, max_nodes=64, device=dev, lm=host, lm_weight=0.3)
    assert host.device.type == "cpu" and t._lm.device.type == "cuda"
    x = torch.randn(2, 5, _V, generator=torch.Generator().manual_seed(4)).to(dev)
    s.step(x)
    t.step(x)
    for a, b in zip(_outputs(s), _outputs(t)):
        assert torch.equal(a, b)
    # reset(rows=<device mask>) is reset(rows=[indices]) bit for bit
    s.reset(rows=[1])
    t.reset(rows=torch.tensor([0, 1], dtype=torch.int32, device=dev))
    assert torch.equal(s.state, t.state) and int(s.out_len[1]) == 0 and int(s.out_len[0]) > 0


# ------------------------------------------------------------------ 4. the recogniser and the task
def test_recognizer_with_an_ngram_equals_the_one_shot_entry_on_its_scores(dev, golden_dir):
    from speech2text_amd.model.decoding import CtcNgramStreamingSearch, ctc_prefix_beam_ngram_tokens
    from speech2text_amd.model.encoder.zipformer_streaming import CtcStreamingRecognizer
    g, m, chunk, V = _tiny_ctc_encoder(golden_dir, dev)
    lm = _ngram_lm(dev, G.lm_text(V, 3, 200, 2), V)
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    rec = CtcStreamingRecognizer(m, _tokenizer(V), batch_size=B, device=dev, beam_size=4, cutoff_top_k=4,
                                 max_tokens=64, max_nodes=256, lm=lm, lm_weight=0.5)
    assert type(rec.search) is CtcNgramStreamingSearch
    with pytest.raises(ValueError, match="lm_start_token"):
        CtcStreamingRecognizer(m, _tokenizer(V), batch_size=B, device=dev, lm=lm, lm_weight=0.5, lm_start_token=1)
    for rep in range(2):
        rec.reset()
        scores = []
        for k in range(6):
            got = rec.step(feats[:, 2 * chunk * k:2 * chunk * k + T])
            assert len(got) == 5
            scores.append(got[-1].clone())
        all_scores = torch.cat(scores, dim=1)
        lens = torch.full((B,), 6 * Tc, dtype=torch.int64, device=dev)
        want = ctc_prefix_beam_ngram_tokens(all_scores, lens, lm, 0.5, 4, 4)
        s = rec.search
        assert 0 < int(s.out_len.sum()) < B * 6 * Tc and int(s.overflow.abs().sum()) == 0
        assert torch.equal(s.out_len, want[1]) and torch.equal(s.score, want[2]) and torch.equal(s.lm_score, want[3])
        for b in range(B):
            n = int(want[1][b])
            assert torch.equal(s.tokens[b, :n], want[0][b, :n])
        assert all(t.startswith(u) for t, u in zip(rec.texts(), rec.stable_texts()))


def test_task_streaming_recognizer_takes_an_explicit_ngram(dev):
    """CtcTask.streaming_recognizer(lm=<NgramLm>, lm_weight=) builds the fused recogniser; `recognize` runs."""
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.decoding import CtcNgramStreamingSearch
    V, chunk = 32, 8
    torch.manual_seed(0)
    task = TaskFactory.get("CTC")(copy.deepcopy(_ctc_zipformer_cfg(V, chunk))).to(dev)
    task.eval()
    with torch.no_grad():
        for p in task._decoder.parameters():
            p.mul_(6.0)
    lm = _ngram_lm(dev, G.lm_text(V, 3, 200, 2), V)
    rec = task.streaming_recognizer(batch_size=2, lm=lm, lm_weight=0.4)
    s = rec.search
    assert type(s) is CtcNgramStreamingSearch and (s.beam_size, s.cutoff_top_k, s._lm_weight) == (3, 2, 0.4)
    feats = torch.randn(2, 150, 80, generator=torch.Generator().manual_seed(5)) * 2.0
    texts = rec.recognize(feats.to(dev), torch.tensor([150, 71]))
    assert any(len(t) for t in texts) and int(s.overflow.abs().sum()) == 0
    assert bool(torch.isfinite(s.lm_score).all())
