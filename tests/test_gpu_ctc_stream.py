"""GPU: the chunk-carried CTC prefix beam search (csrc/decode_ctc.hip s2t_ctc_prefix_beam_chunk,
s2t_ctc_prefix_beam_lm_chunk; model/decoding.py CtcStreamingSearch), the CtcStreamingRecognizer graph
around it and CtcTask.streaming_recognizer.

The yardstick of the bits is the one-shot device entry (ctc_prefix_beam_tokens /
ctc_prefix_beam_lm_tokens, themselves held to float64 by tests/test_gpu_ctc_prefix_beam.py): however the
frames of a case of tests/ctc_stream_cases.py are cut, tokens[:out_len], out_len, score and lm_score are
torch.equal to it.  stable_len is held to the chunked restatement tests/ctc_stream_f64.py.  The COMPACTS
cases run with a max_nodes below the sequences they ever keep (tests/test_ctc_stream_f64.py asserts the
inequality): their equality without overflow shows the compaction at work and exact.  Frames of a chunk
at and beyond chunk_len[b] are NaN in every call.
"""
import copy
import math

import pytest
import torch

import ctc_prefix_cases as C
import ctc_stream_cases as SC
import rnnt_lm_fusion_cases as L
from decode_support import _lm_module, _tiny_ctc_encoder, _tokenizer
from task_support import _ctc_zipformer_cfg

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(dev, name):
    """(case, logits and lengths on the device, the LM module or None, the one-shot entry's outputs on
    the whole utterances), once per case."""
    if name not in _CACHE:
        c = SC.CASES[name]
        x, lens, sd = SC.make(name)
        lm = _lm_module(dev, sd) if sd is not None else None
        xd, ld = x.to(dev), lens.to(dev)
        _CACHE[name] = (c, xd, ld, lm, _one_shot(c, xd, ld, lm))
    return _CACHE[name]


def _one_shot(c, x, lens, lm, **kw):
    from speech2text_amd.model.decoding import ctc_prefix_beam_lm_tokens, ctc_prefix_beam_tokens
    if lm is None:
        out = ctc_prefix_beam_tokens(x, lens, beam_size=c["beam"], cutoff_top_k=c["topk"])
    else:
        args = dict(lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"], lm_start_token=c["start"])
        args.update(kw)
        out = ctc_prefix_beam_lm_tokens(x, lens, lm, **args)
    assert out is not None
    return [t.cpu() for t in out]


def _search(dev, name, lm=None, **kw):
    from speech2text_amd.model.decoding import CtcStreamingSearch
    c = SC.CASES[name]
    args = dict(batch_size=c["B"], method="beam", beam_size=c["beam"], cutoff_top_k=c["topk"], max_tokens=c["T"],
                max_nodes=SC.max_nodes(name), device=dev)
    if lm is not None:
        args.update(lm=lm, lm_weight=c["weight"], lm_start_token=c["start"])
    args.update(kw)
    return CtcStreamingSearch(c["V"], **args)


def _outputs(search):
    outs = [search.tokens, search.out_len, search.score, search.stable_len, search.overflow]
    if search.lm_score is not None:
        outs.append(search.lm_score)
    return [t.cpu().clone() for t in outs]


def _same_as_one_shot(got, want, what):
    """got: _outputs of a stream; want: the one-shot entry's (tokens, out_len, score[, lm_score])."""
    assert torch.equal(got[1], want[1]), (what, got[1], want[1])
    for b in range(got[0].shape[0]):
        n = int(want[1][b])
        assert torch.equal(got[0][b, :n], want[0][b, :n]), (what, b)
    assert torch.equal(got[2], want[2]), (what, got[2], want[2])
    if len(want) > 3:
        assert torch.equal(got[5], want[3]), (what, got[5], want[3])


def _feed(dev, search, name, cut, reports=None, each=None):
    """Feeds the calls of a cut; after every call stable_len never decreases, tokens[:stable_len] stay,
    overflow is 0 and (reports given) stable_len is the restatement's."""
    last = None
    for i, (ch, cl, fed) in enumerate(SC.chunks(name, cut)):
        search.step(ch.to(dev), cl.to(dev))
        got = _outputs(search)
        assert int(got[4].abs().sum()) == 0, (name, cut, i, got[4])
        if reports is not None:
            assert got[3].tolist() == [r.stable for r in reports[i]], (name, cut, i)
        if last is not None:
            assert bool((got[3] >= last[3]).all()), (name, cut, i)
            for b in range(got[0].shape[0]):
                s = int(last[3][b])
                assert torch.equal(got[0][b, :s], last[0][b, :s]), (name, cut, i, b)
        if each is not None:
            each(i, fed, got)
        last = got
    return last


# ------------------------------------------------------------------ 1. every case under every cut
@pytest.mark.parametrize("cut", SC.CUTS)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_any_cut_equals_the_one_shot_entry(dev, name, cut):
    c, x, lens, lm, want = _case(dev, name)
    search = _search(dev, name, lm)
    reports = SC.stream_reports(name, cut)

    def prefix(i, fed, got):                               # after each chunk: the one-shot entry on the prefix
        T = max(max(fed), 1)
        _same_as_one_shot(got, _one_shot(c, x[:, :T].contiguous(), torch.tensor(fed, device=dev), lm),
                          (name, cut, "after call", i))

    got = _feed(dev, search, name, cut, reports, prefix if cut == "r7" else None)
    _same_as_one_shot(got, want, (name, cut))
    if name in SC.COMPACTS:
        print(f"{name} {cut}: max_nodes {SC.max_nodes(name)}, sequences ever kept "
              f"{[r.ever for r in reports[-1]]}, kept at the end {[r.kept for r in reports[-1]]}")


@pytest.mark.parametrize("name", SC.PLAIN_CASES)
def test_lm_entry_at_weight_zero_is_the_plain_chunk_entry(dev, name):
    c = SC.CASES[name]
    V = c["V"]
    model = {11: "lm20_v11", 63: "lm20", 65: "lm48", 128: "lm64"}.get(V)
    lm = _lm_module(dev, L.lm_weights(model, 3)) if model else _lm_module(dev, V=V, H=8, layers=2)
    for start in (None, V - 1):
        plain = _search(dev, name)
        fused = _search(dev, name, lm=lm, lm_weight=0.0, lm_start_token=start)
        for i, (ch, cl, _) in enumerate(SC.chunks(name, "ragged")):
            plain.step(ch.to(dev), cl.to(dev))
            fused.step(ch.to(dev), cl.to(dev))
            for a, b in zip(_outputs(plain), _outputs(fused)[:5]):
                assert torch.equal(a, b), (name, start, i)
        assert bool(torch.isfinite(fused.lm_score).all())


@pytest.mark.parametrize("name", ["p_v128_beam1_k1", "p_v65_b33_beam4_k3_norm", "s_v29_t90_b3_beam4_blank"])
def test_greedy_method_is_the_greedy_kernel(dev, name):
    from speech2text_amd.model.decoding import ctc_greedy_tokens
    c, x, lens, _, _ = _case(dev, name)
    search = _search(dev, name, method="greedy", beam_size=7, cutoff_top_k=7)
    assert (search.beam_size, search.cutoff_top_k, search.method) == (1, 1, "greedy")
    for ch, cl, _ in SC.chunks(name, "ragged"):
        search.step(ch.to(dev), cl.to(dev))
    n = lens.clamp(0, c["T"])
    tokens, out_len = ctc_greedy_tokens(torch.nan_to_num(x), n)
    assert torch.equal(search.out_len, out_len) and int(out_len.sum()) > 0
    for b in range(c["B"]):
        assert torch.equal(search.tokens[b, :int(out_len[b])], tokens[b, :int(out_len[b])]), (name, b)
    assert torch.equal(search.stable_len, search.out_len) and int(search.overflow.abs().sum()) == 0


# ------------------------------------------------------------------ 2. overflow, idle calls, reset
def _row_needs(name, cut):
    """Per row the largest kept + beam * n of its calls, by the unbounded restatement."""
    c = SC.CASES[name]
    kept, most = [1] * c["B"], [0] * c["B"]
    for (_, ns), row in zip(SC.calls(name, cut), SC.stream_reports(name, cut)):
        for b, n in enumerate(ns):
            if n:
                most[b] = max(most[b], kept[b] + c["beam"] * n)
            kept[b] = row[b].kept
    return most


def _state_rows(search):
    """The arrays both families' state begins with, by the table in include/s2t_mi355.h ->
    {array: (B, bytes per row) view of search.state}."""
    B, beam, M = search.batch_size, search.beam_size, search.max_nodes
    sizes = [("nodes", 16 * M), ("stage", 16 * M), ("map", 4 * M)]
    sizes += [(k, 4 * beam) for k in ("pb", "pnb", "lm_sum", "node", "last", "len")]
    sizes += [(k, 4) for k in ("nb", "kept", "depth", "ovf")] + [("eff", 8)]
    off, out = 0, {}
    for k, per in sizes:
        out[k] = search.state[off:off + B * per].view(B, per)
        off += (B * per + 255) // 256 * 256
    assert off == search.state.numel() if search.lm_score is None else off < search.state.numel()
    return out


@pytest.mark.parametrize("with_lm", [False, True])
def test_node_overflow_makes_the_row_inert_until_reset(dev, with_lm):
    name, cut = "s_v29_t90_b3_beam4_blank", "r7"
    c, x, lens, _, _ = _case(dev, name)
    lm = _lm_module(dev, V=c["V"], H=8, layers=2) if with_lm else None
    kw = dict(lm=lm, lm_weight=0.0, lm_start_token=None) if with_lm else {}
    needs = _row_needs(name, cut)
    assert needs[1] == 0 and needs[0] != needs[2], needs
    bad, good = (0, 2) if needs[0] > needs[2] else (2, 0)
    limit = (needs[0] + needs[2]) // 2                      # between the two rows' needs: one of them overflows
    reports = SC.stream_reports(name, cut, limit)
    first = next(i for i, row in enumerate(reports) if row[bad].overflow)
    assert first > 1 and not any(row[good].overflow for row in reports)
    print(f"needs {needs}, max_nodes {limit}: row {bad} overflows at call {first} of {len(reports)}")
    search = _search(dev, name, max_nodes=limit, **kw)
    rows = _state_rows(search)
    assert int(rows["kept"].view(torch.int32)[bad]) == 1
    frozen = None
    for i, (ch, cl, _) in enumerate(SC.chunks(name, cut)):
        search.step(ch.to(dev), cl.to(dev))
        got = _outputs(search)
        assert got[4].tolist() == [2 if row.overflow else 0 for row in reports[i]], (i, got[4])
        assert got[3].tolist() == [r.stable for r in reports[i]], i
        mine = {k: v[bad].cpu().clone() for k, v in rows.items()}       # every array of the row's state
        if i == first - 1:
            frozen = ([t[bad].clone() for t in got[:4]], mine)
        if i >= first:                                     # outputs and state as before the refused call ...
            for a, b in zip(frozen[0], got[:4]):
                assert torch.equal(a, b[bad]), i
            for k in mine:
                if k != "ovf" and not (with_lm and k == "eff"):             # (eff: per-call scratch of the LM family)
                    assert torch.equal(frozen[1][k], mine[k]), (i, k)
            assert int(mine["ovf"].view(torch.int32)) == 2     # ... but for the bit that makes it inert
    want = _one_shot(c, x, lens, None)
    got = _outputs(search)
    for b in (good, 1):                                    # the neighbours are the one-shot's
        n = int(want[1][b])
        assert int(got[1][b]) == n and torch.equal(got[0][b, :n], want[0][b, :n]) and got[2][b] == want[2][b]
    # ---- after reset(rows=[bad]) the row's next stream is the one-shot's again; the others keep theirs
    search.reset(rows=[bad])
    after = _outputs(search)
    assert int(after[4][bad]) == 0 and int(after[1][bad]) == 0 and torch.equal(after[0][good], got[0][good])
    T2 = 28
    for k in range(T2 // 7):
        ch = torch.full((c["B"], 7, c["V"]), float("nan"), device=dev)
        ch[bad] = x[bad, 7 * k:7 * k + 7]
        cl = torch.zeros(c["B"], dtype=torch.int64, device=dev)
        cl[bad] = 7
        search.step(ch, cl)
    short = _one_shot(c, x[bad:bad + 1, :T2].contiguous(), torch.tensor([T2], device=dev), None)
    got2 = _outputs(search)
    n = int(short[1][0])
    assert n > 0 and int(got2[1][bad]) == n and torch.equal(got2[0][bad, :n], short[0][0, :n])
    assert got2[2][bad] == short[2][0] and int(got2[4][bad]) == 0
    for t2, t1 in zip(got2[:4], got[:4]):
        assert torch.equal(t2[good], t1[good])


@pytest.mark.parametrize("with_lm", [False, True])
def test_token_overflow_keeps_the_first_tokens_and_exact_scores(dev, with_lm):
    name = "l_v63_lm20_beam4" if with_lm else "s_v11_t60_beam4_blank"
    c, x, lens, lm, want = _case(dev, name)
    cap = int(want[1].max()) // 2
    assert cap >= 2
    search = _search(dev, name, lm, max_tokens=cap)
    for ch, cl, _ in SC.chunks(name, "r4"):
        search.step(ch.to(dev), cl.to(dev))
    got = _outputs(search)
    assert torch.equal(got[2], want[2]) and (not with_lm or torch.equal(got[5], want[3]))
    for b in range(c["B"]):
        n = int(want[1][b])
        assert int(got[1][b]) == min(n, cap) and torch.equal(got[0][b, :min(n, cap)], want[0][b, :min(n, cap)])
        assert int(got[4][b]) == (1 if n > cap else 0) and int(got[3][b]) <= cap
    assert int(got[4].sum()) > 0


@pytest.mark.parametrize("name", ["p_v63_beam16_k16", "l_v63_lm20_beam4"])
def test_idle_calls_change_nothing(dev, name):
    c, x, lens, lm, want = _case(dev, name)
    search = _search(dev, name, lm)
    nan = torch.full((c["B"], 5, c["V"]), float("nan"), device=dev)
    for i, (ch, cl, _) in enumerate(SC.chunks(name, "r4")):
        if i in (0, 2):                                    # before the first frame, and between two chunks
            before, state = _outputs(search), search.state.clone()
            search.step(nan, torch.zeros(c["B"], dtype=torch.int64, device=dev))
            search.step(nan, torch.full((c["B"],), -3, dtype=torch.int64, device=dev))
            for a, b in zip(before, _outputs(search)):
                assert torch.equal(a, b), (name, i)
            if lm is None:                                 # (an LM round rewrites its emit / parent / token scratch)
                assert torch.equal(state, search.state), (name, i)
        search.step(ch.to(dev), cl.to(dev))
    _same_as_one_shot(_outputs(search), want, name)


def test_refused_calls_touch_nothing(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import CtcStreamingSearch
    s = CtcStreamingSearch(16, batch_size=2, beam_size=4, cutoff_top_k=4, max_tokens=8, max_nodes=64, device=dev)
    x = torch.randn(2, 4, 16, device=dev)
    s.step(x)
    before, state = _outputs(s), s.state.clone()
    cl = torch.full((2,), 4, dtype=torch.int64, device=dev)

    def chunk(Tc=4, V=16, blank=0, beam=4, topk=4, max_tokens=8, max_nodes=64, state=N.ptr(s.state)):
        return N.lib().s2t_ctc_prefix_beam_chunk(N.fp(x), N.lp(cl), 2, Tc, V, blank, beam, topk, max_tokens, max_nodes,
                                                 state, N.lp(s.tokens), N.lp(s.out_len), N.fp(s.score),
                                                 N.lp(s.stable_len), N.ip(s.overflow), N.stream())
    for kw in (dict(Tc=0), dict(Tc=257), dict(state=None), dict(max_nodes=0), dict(max_tokens=0), dict(V=0),
               dict(blank=16), dict(blank=-1), dict(beam=0), dict(beam=17), dict(topk=0), dict(topk=17, V=32)):
        assert chunk(**kw) == -1, kw
    assert N.lib().s2t_ctc_stream_reset(None, None, 2, 16, 4, 64, N.stream()) == -1
    assert N.lib().s2t_ctc_stream_reset(N.ptr(s.state), None, 2, 16, 4, 0, N.stream()) == -1
    torch.cuda.synchronize()
    for a, b in zip(before, _outputs(s)):
        assert torch.equal(a, b)
    assert torch.equal(state, s.state)
    with pytest.raises(ValueError):
        s.step(torch.zeros(2, 257, 16, device=dev))
    with pytest.raises(ValueError):
        s.step(torch.zeros(2, 0, 16, device=dev))
    with pytest.raises(ValueError):
        CtcStreamingSearch(16, lm=_lm_module(dev, V=17, H=8, layers=1), device=dev)     # lm.V != V
    with pytest.raises(ValueError):
        CtcStreamingSearch(16, lm=_lm_module(dev, V=16, H=8, layers=1), lm_start_token=16, device=dev)


_RV = 32


@pytest.mark.parametrize("change", [dict(Tc=0), dict(Tc=257), dict(state=None), dict(ws=None), dict(max_nodes=0),
                                    dict(max_nodes=1048577), dict(max_tokens=0), dict(beam=17), dict(beam=0),
                                    dict(topk=0), dict(topk=17), dict(V=8193), dict(V=0), dict(blank=-1),
                                    dict(blank=_RV), dict(H=1028), dict(H=22), dict(H=0), dict(E=1025),
                                    dict(num_layers=9), dict(num_layers=0), dict(lmV=_RV + 1), dict(start=_RV),
                                    dict(weight=math.inf), dict(weight=math.nan), dict(lm=None)], ids=str)
def test_lm_entries_refuse_before_any_launch(dev, change):
    """s2t_ctc_prefix_beam_lm_chunk and s2t_ctc_lm_stream_reset with a real descriptor and one bad
    argument at a time: -1 (the size functions 0), and the outputs, the state and the workspace of a
    stream in progress keep every bit.  No pointer is followed: logits, state and workspace are far
    too small for V 8193 or 1048577 nodes."""
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import CtcStreamingSearch, rnn_lm_desc
    lib = N.lib()
    lm = _lm_module(dev, V=_RV, H=8, layers=1)
    s = CtcStreamingSearch(_RV, batch_size=2, beam_size=4, cutoff_top_k=4, max_tokens=8, max_nodes=64, device=dev,
                           lm=lm, lm_weight=0.3, lm_start_token=3)
    x = torch.randn(2, 4, _RV, generator=torch.Generator().manual_seed(3)).to(dev)
    s.step(x)
    assert int(s.out_len.sum()) > 0
    before, state, ws = _outputs(s), s.state.clone(), s._ws.clone()
    cl = torch.full((2,), 4, dtype=torch.int64, device=dev)
    lm_desc, lm_keep = rnn_lm_desc(lm)
    assert lib.s2t_ctc_lm_stream_state_bytes(lm_desc, 2, _RV, 4, 64) == s.state.numel()
    assert lib.s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(lm_desc, 2, _RV, 4) == s._ws.numel()
    for k in ("H", "E", "num_layers"):
        if k in change:
            setattr(lm_keep[-1], k, change[k])
    if "lmV" in change:
        lm_keep[-1].V = change["lmV"]
    desc = None if "lm" in change else lm_desc
    g = lambda k, d: change.get(k, d)                      # noqa: E731
    V, beam, max_nodes = g("V", _RV), g("beam", 4), g("max_nodes", 64)
    statep = None if "state" in change else N.ptr(s.state)
    wsp = None if "ws" in change else N.ptr(s._ws)
    assert lib.s2t_ctc_prefix_beam_lm_chunk(desc, N.fp(x), N.lp(cl), 2, g("Tc", 4), V, g("blank", 0), beam, g("topk", 4),
                                            g("weight", 0.3), g("start", 3), g("max_tokens", 8), max_nodes, statep,
                                            wsp, N.lp(s.tokens), N.lp(s.out_len), N.fp(s.score), N.fp(s.lm_score),
                                            N.lp(s.stable_len), N.ip(s.overflow), N.stream()) == -1
    desc_keys = {"H", "E", "num_layers", "lmV", "lm"}
    if (desc_keys | {"state", "ws", "max_nodes", "beam", "V", "start"}) & set(change):     # what the reset takes
        assert lib.s2t_ctc_lm_stream_reset(desc, g("start", 3), statep, None, 2, V, beam, max_nodes, wsp,
                                           N.stream()) == -1
    if (desc_keys | {"max_nodes", "beam", "V"}) & set(change):
        assert lib.s2t_ctc_lm_stream_state_bytes(desc, 2, V, beam, max_nodes) == 0
    if (desc_keys | {"beam", "V"}) & set(change):
        assert lib.s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(desc, 2, V, beam) == 0
    if {"max_nodes", "beam", "V", "state"} & set(change):                                  # the plain reset too
        assert lib.s2t_ctc_stream_reset(statep, None, 2, V, beam, max_nodes, N.stream()) == -1
    torch.cuda.synchronize()
    for a, b in zip(before, _outputs(s)):
        assert torch.equal(a, b)
    assert torch.equal(state, s.state) and torch.equal(ws, s._ws)


def test_empty_batch_returns_zero_through_every_entry(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnn_lm_desc
    lib = N.lib()
    lm_desc, lm_keep = rnn_lm_desc(_lm_module(dev, V=_RV, H=8, layers=1))
    assert lib.s2t_ctc_stream_reset(None, None, 0, _RV, 99, 0, N.stream()) == 0
    assert lib.s2t_ctc_lm_stream_reset(lm_desc, 99, None, None, 0, _RV, 99, 0, None, N.stream()) == 0
    assert lib.s2t_ctc_prefix_beam_chunk(None, None, 0, 999, _RV, 0, 99, 99, 0, 0, None, None, None, None, None, None,
                                         N.stream()) == 0
    assert lib.s2t_ctc_prefix_beam_lm_chunk(lm_desc, None, None, 0, 999, _RV, 0, 99, 99, math.nan, 99, 0, 0, None,
                                            None, None, None, None, None, None, None, N.stream()) == 0


@pytest.mark.parametrize("with_lm", [False, True])
def test_reset_takes_a_device_mask(dev, with_lm):
    """reset(rows=<int32 device mask>) is reset(rows=[indices]) bit for bit, state and outputs."""
    from speech2text_amd.model.decoding import CtcStreamingSearch
    kw = dict(lm=_lm_module(dev, V=_RV, H=8, layers=1), lm_weight=0.3, lm_start_token=3) if with_lm else {}
    x = torch.randn(3, 5, _RV, generator=torch.Generator().manual_seed(4)).to(dev)
    pair = [CtcStreamingSearch(_RV, batch_size=3, max_tokens=8, max_nodes=64, device=dev, **kw) for _ in range(2)]
    for s in pair:
        s.step(x)
    pair[0].reset(rows=[0, 2])
    pair[1].reset(rows=torch.tensor([1, 0, 1], dtype=torch.int32, device=dev))
    for a, b in zip(_outputs(pair[0]), _outputs(pair[1])):
        assert torch.equal(a, b)
    assert torch.equal(pair[0].state, pair[1].state)
    assert int(pair[0].out_len[0]) == 0 and int(pair[0].out_len[1]) > 0
    with pytest.raises(ValueError):
        pair[1].reset(rows=torch.tensor([1, 0, 1], dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        pair[1].reset(rows=torch.ones(2, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------ 3. the recogniser and the task


@pytest.mark.parametrize("method", ["beam", "greedy", "beam_lm"])
def test_recognizer_graph_equals_the_eager_composition(dev, golden_dir, method):
    """CtcStreamingRecognizer.step (one graph replay) against streaming_step -> CtcStreamingSearch.step
    issued eagerly, over the fixture's 6 chunks, twice across reset(): scores, outputs and every
    encoder state bit for bit; the final tokens are the one-shot entry's on the concatenated scores."""
    from speech2text_amd.model.decoding import (CtcStreamingSearch, ctc_greedy_tokens, ctc_prefix_beam_lm_tokens,
                                                ctc_prefix_beam_tokens)
    from speech2text_amd.model.encoder.zipformer_streaming import CtcStreamingRecognizer, StreamingRecognizer
    g, m, chunk, V = _tiny_ctc_encoder(golden_dir, dev)
    assert V == 13 and m._for_ctc
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    kw = dict(method="greedy" if method == "greedy" else "beam", beam_size=4, cutoff_top_k=4, max_tokens=64,
              max_nodes=256)
    if method == "beam_lm":
        kw.update(lm=_lm_module(dev, V=V, H=8, layers=2), lm_weight=0.5, lm_start_token=V - 1)
    rec = CtcStreamingRecognizer(m, _tokenizer(V), batch_size=B, device=dev, **kw)
    eager = CtcStreamingSearch(V, batch_size=B, device=dev, **kw)
    for rep in range(2):
        st = m.get_init_states(B, dev)
        rec.reset()
        eager.reset()
        scores = []
        for c in range(6):
            x = feats[:, 2 * chunk * c:2 * chunk * c + T]
            with torch.no_grad():
                sc, st = m.streaming_step(x, st)
                sc = sc.float().contiguous()
            want = eager.step(sc)
            got = rec.step(x)
            assert len(got) == 5 and torch.equal(got[-1], sc), (rep, c)
            for a, b in zip(got[:-1], want):
                assert torch.equal(a, b), (rep, c)
            scores.append(got[-1].clone())
        for a, b in zip(rec.states, st):
            assert torch.equal(a, b)
        assert torch.equal(rec.search.overflow, eager.overflow) and int(eager.overflow.abs().sum()) == 0
        all_scores = torch.cat(scores, dim=1)
        lens = torch.full((B,), 6 * Tc, dtype=torch.int64, device=dev)
        n = int(rec.search.out_len.sum())
        print(f"{method} rep {rep}: {n} tokens on {B * 6 * Tc} frames")
        assert 0 < n < B * 6 * Tc
        if method == "greedy":
            want = ctc_greedy_tokens(all_scores, lens)
        elif method == "beam":
            want = ctc_prefix_beam_tokens(all_scores, lens, 4, 4)
            assert torch.equal(rec.search.score, want[2])
        else:
            want = ctc_prefix_beam_lm_tokens(all_scores, lens, kw["lm"], 0.5, 4, 4, lm_start_token=V - 1)
            assert torch.equal(rec.search.score, want[2]) and torch.equal(rec.search.lm_score, want[3])
        assert torch.equal(rec.search.out_len, want[1])
        for b in range(B):
            k = int(want[1][b])
            assert torch.equal(rec.search.tokens[b, :k], want[0][b, :k])
        texts = rec.texts()
        tok = rec.search.tokens.cpu()
        assert texts == [rec.tokenizer.decode(tok[b, :int(rec.search.out_len[b])]) for b in range(B)]
        assert all(t.startswith(u) for t, u in zip(texts, rec.stable_texts()))
    with pytest.raises(ValueError):
        rec.step(feats[:, :T - 1])
    # the refusals: a for_ctc encoder stays refused by the RNN-T recogniser; the CTC one wants scores
    with pytest.raises(ValueError):
        StreamingRecognizer(m, None, None, _tokenizer(V), device=dev)
    with pytest.raises(ValueError):
        CtcStreamingRecognizer(m, _tokenizer(V), head=torch.nn.Identity().eval(), device=dev)
    m.train()
    with pytest.raises(RuntimeError):
        CtcStreamingRecognizer(m, _tokenizer(V), device=dev)


def test_task_streaming_recognizer(dev):
    """CtcTask.streaming_recognizer(batch_size=2): `recognize` on two utterances of different lengths
    equals feeding the chunks by hand, the shorter row idling (chunk_len 0) while the longer one goes
    on; method, widths and the LM come from the task's metric section; the head is the Projector."""
    import math
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.lm.rnn_lm import RnnLm
    V, chunk = 32, 8
    cfg = _ctc_zipformer_cfg(V, chunk)
    torch.manual_seed(0)
    task = TaskFactory.get("CTC")(copy.deepcopy(cfg)).to(dev)
    task.eval()
    with torch.no_grad():
        for p in task._decoder.parameters():
            p.mul_(6.0)
        task._global_cmvn.global_mean.fill_(0.25)
        task._global_cmvn.global_istd.fill_(0.5)
    rec = task.streaming_recognizer(batch_size=2)
    s = rec.search
    assert (s.method, s.beam_size, s.cutoff_top_k, s._lm_weight, s._lm_start) == ("beam", 3, 2, 0.5, V - 1)
    assert isinstance(s._lm, RnnLm) and s.lm_score is not None and rec.head is task._decoder.decoder
    greedy = task.streaming_recognizer(batch_size=1, method="greedy").search
    assert (greedy.method, greedy.beam_size, greedy._lm) == ("greedy", 1, None)
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
    assert rec.texts() == texts and int(rec.search.overflow.abs().sum()) == 0
    with pytest.raises(ValueError):
        rec.recognize(feats[:1].to(dev), lens[:1])
