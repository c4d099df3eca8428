"""GPU: the back-off n-gram look-up (csrc/ngram_lookup.h, s2t_ngram_score) and the CTC prefix beam search
fused with it in one launch (csrc/decode_ctc.hip s2t_ctc_prefix_beam_ngram) against the float64 restatement
tests/ctc_ngram_f64.py on the cases of tests/ctc_ngram_cases.py, whose conditions (every decision made by at
least 1e-3 in float64, every back-off depth, merges, a re-entry, the LM changes a hypothesis)
tests/test_ctc_ngram_f64.py asserts on the CPU.  The look-up is held to the host's fp32 evaluation of
the header's statement bit for bit (the same adds in the same order); tokens and out_len must equal
the restatement's; score and lm_score are bounded by max(2e-5, 8 x what float32 costs the restatement),
relative to the largest reference value of the case.  Frames at and beyond an utterance's length are
NaN in every case: a search that read one would not return the reference's tokens.
"""
import math

import numpy as np
import pytest
import torch

import ctc_ngram_cases as C
import ctc_ngram_f64 as G
import ctc_prefix_cases as PC
from yardstick import _Ids

pytestmark = pytest.mark.gpu


_CACHE, _LMS = {}, {}


def _lm(dev, text, V):
    """A model of its own on the device per text (the shared CPU models of the cases stay where they are)."""
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    if text not in _LMS:
        _LMS[text] = NgramLm.from_arpa(text, num_classes=V).to(dev)
    return _LMS[text]


def _case(dev, name):
    if name not in _CACHE:
        x, lens = C.make(name)
        _CACHE[name] = (C.CASES[name], x.to(dev), lens.to(dev), _lm(dev, C.text_of(name), C.CASES[name]["V"]))
    return _CACHE[name]


def _fused(c, x, lens, lm, **kw):
    from speech2text_amd.model.decoding import ctc_prefix_beam_ngram_tokens
    args = dict(lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"])
    args.update(kw)
    return ctc_prefix_beam_ngram_tokens(x, lens, lm, **args)


# ------------------------------------------------------------------ 1. the look-up on its own
@pytest.mark.parametrize("name", list(C.CASES))
def test_lookup_is_the_hosts_fp32_statement_bit_for_bit(dev, name):
    """Every (context, class) pair of the case's table: logp and next."""
    _, _, _, lm = _case(dev, name)
    host = C.model(name)
    V, nc = host.num_classes, host.num_ctx
    ctx = torch.arange(nc, dtype=torch.int32, device=dev).repeat_interleave(V)
    tok = torch.arange(V, dtype=torch.int32, device=dev).repeat(nc)
    logp, nxt = lm._device_score(ctx, tok)
    want = [host._row(n) for n in range(nc)]
    assert torch.equal(logp.cpu().reshape(nc, V), torch.from_numpy(np.stack([w[0] for w in want])))
    assert torch.equal(nxt.cpu().reshape(nc, V), torch.from_numpy(np.stack([w[1] for w in want])))
    for n in range(0, nc, max(1, nc // 5)):                # (the row form is the scalar statement)
        for c in range(0, V, max(1, V // 5)):
            lp, nx = host.score(n, c)
            assert float(logp[n * V + c]) == float(lp) and int(nxt[n * V + c]) == nx
    # the protocol on the device is the same rows
    st = lm.init_states(2)
    q, new = lm.score_step(torch.tensor([V - 1, min(1, V - 1)], device=dev), st)
    hq, hnew = host.score_step(torch.tensor([V - 1, min(1, V - 1)]), host.init_states(2))
    assert torch.equal(q.cpu(), hq) and torch.equal(new.cpu(), hnew) and q.is_cuda
    assert torch.equal(lm.start_scores(st).cpu(), host.start_scores(host.init_states(2)))


# ------------------------------------------------------------------ 2. the fused entry
def _check(name, out, ref):
    tokens, out_len, score, lm_score = (t.cpu() for t in out)
    for b, r in enumerate(ref):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == r.tokens, (name, b)
        assert int(tokens[b, n:].sum()) == 0
        if not r.tokens and r.score == 0.0:                # no frames: no tokens, score 0, lm_score 0
            assert float(score[b]) == 0.0 and float(lm_score[b]) == 0.0
    f64 = lambda i: torch.tensor([r[i] for r in ref], dtype=torch.float64)    # noqa: E731
    for what, got, i in (("score", score, 1), ("lm_score", lm_score, 2)):
        err = C.rel_err(got, f64(i))
        print(f"{name}: {what} rel_err {err:.3e} (bound {C.bound(name):.1e})")
        assert err <= C.bound(name), (name, what, err)


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_entry_against_the_float64_restatement(dev, name):
    from speech2text_amd.model.decoding import ctc_prefix_beam_tokens
    c, x, lens, lm = _case(dev, name)
    out = _fused(c, x, lens, lm)
    assert out is not None and len(out) == 4
    _check(name, out, C.reference(name))
    if name in C.LM_CHANGES:
        plain = ctc_prefix_beam_tokens(x, lens, c["beam"], c["topk"])
        assert not torch.equal(out[0], plain[0]), "the LM changes no hypothesis"


@pytest.mark.parametrize("name", PC.PLAIN_CASES)
def test_weight_zero_is_the_plain_entry_bit_for_bit(dev, name):
    """On every plain case of tests/ctc_prefix_cases.py, with a sparse model of that V."""
    from speech2text_amd.model.decoding import ctc_prefix_beam_tokens
    c = PC.CASES[name]
    x, lens, _ = PC.make(name)
    x, lens = x.to(dev), lens.to(dev)
    lm = _lm(dev, C.lm_text(c["V"], 3, 200, 2), c["V"])
    plain = ctc_prefix_beam_tokens(x, lens, c["beam"], c["topk"])
    out = _fused(c, x, lens, lm, lm_weight=0.0)
    assert out is not None
    for a, b in zip(plain, out[:3]):
        assert torch.equal(a, b), name
    assert bool(torch.isfinite(out[3]).all())


@pytest.mark.parametrize("name", C.ORDER_ONE)
def test_order_one_is_a_constant_q_row(dev, name):
    """An order-1 model: the restatement with one row for every prefix, the first token included."""
    c, x, lens, lm = _case(dev, name)
    assert lm.order == 1 and lm.num_ctx == 1 and lm.num_arcs == c["V"]
    ng = C.dict_model(name, np.float64)
    out = _fused(c, x, lens, lm)
    for b, r in enumerate(C.reference(name)):
        assert out[0][b, :int(out[1][b])].tolist() == r.tokens, b
        row = sum(float(ng.probs[(t,)]) for t in r.tokens)
        assert float(out[3][b]) == pytest.approx(row, rel=1e-5, abs=1e-5)


@pytest.mark.parametrize("T,V,n,order,weight", C.BRUTE)
def test_exhaustive_cases_through_the_kernel(dev, T, V, n, order, weight):
    x = C.brute_logits(T, V, n).to(dev)
    lens = torch.full((n,), T, device=dev)
    lm = _lm(dev, C.brute_text(V, order), V)
    tokens, out_len, score, lm_score = (t.cpu() for t in _fused(dict(beam=16, topk=V, weight=weight), x, lens, lm))
    ref = C.brute_reference(T, V, n, order, weight)
    for i, (labels, logp, lms, _) in enumerate(ref):
        assert tokens[i, :int(out_len[i])].tolist() == labels, (T, V, i)
    err = C.rel_err(score, torch.tensor([r[1] for r in ref], dtype=torch.float64))
    err_lm = C.rel_err(lm_score, torch.tensor([r[2] for r in ref], dtype=torch.float64))
    print(f"exhaustive T {T} V {V}: score rel_err {err:.3e}, lm_score rel_err {err_lm:.3e}")
    assert err <= C.FLOOR and err_lm <= C.FLOOR


def test_batch_invariance(dev):
    name = "n_v11_o2_b17_beam4_k3"
    c, x, lens, lm = _case(dev, name)
    whole = _fused(c, x, lens, lm)
    for b in (0, 1, 2, 16):
        alone = _fused(c, x[b:b + 1], lens[b:b + 1], lm)
        for a, w in zip(alone, whole):
            assert torch.equal(a[0], w[b]), b


def test_graph_capture_and_two_replays(dev):
    name = "n_v65_o3_b33_beam4_k3_norm"
    c, x, lens, lm = _case(dev, name)
    eager = [t.clone() for t in _fused(c, x, lens, lm)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fused(c, x, lens, lm)                             # (warm the allocator on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _fused(c, x, lens, lm)
    for _ in range(2):
        for t in out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, out):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ 3. limits
_V = 32


@pytest.mark.parametrize("change", [dict(beam=17), dict(beam=0), dict(topk=0), dict(topk=17), dict(V=8193),
                                    dict(blank=-1), dict(blank=_V), dict(ws=None), dict(lm=None), dict(lmV=_V + 1),
                                    dict(order=0), dict(order=9), dict(num_ctx=0), dict(num_arcs=_V - 1),
                                    dict(start=-1), dict(start="num_ctx"), dict(weight=math.inf),
                                    dict(weight=math.nan), dict(null="ctx_begin"), dict(null="ctx_fail"),
                                    dict(null="ctx_backoff"), dict(null="arc_token"), dict(null="arc_logp"),
                                    dict(null="arc_next")], ids=str)
def test_limits_just_outside_return_minus_one(dev, change):
    """Outside the limits the entries answer -1 (the workspace size 0) before any launch: no pointer is
    followed (logits, workspace and outputs are far too small for V 8193) and the poisoned outputs keep
    their poison."""
    import ctypes
    from speech2text_amd import _native as N
    lib = N.lib()
    lm = _lm(dev, C.lm_text(_V, 3, 200, 2), _V)
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
    start = change.get("start", lm.start_ctx)
    start = lm.num_ctx if start == "num_ctx" else start
    beam, topk, V, blank = change.get("beam", 4), change.get("topk", 4), change.get("V", _V), change.get("blank", 0)
    need = lib.s2t_ctc_prefix_beam_ngram_workspace_bytes(1, 2, _V, 4)
    assert need == lib.s2t_ctc_prefix_beam_workspace_bytes(1, 2, _V, 4) > 0
    if {"beam", "V"} & set(change):
        assert lib.s2t_ctc_prefix_beam_ngram_workspace_bytes(1, 2, V, beam) == 0
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    wsp = None if "ws" in change else N.ptr(ws)
    x, lens = torch.zeros(1, 2, _V, device=dev), torch.tensor([2], device=dev)
    tokens = torch.full((1, 2), 7, dtype=torch.int64, device=dev)
    out_len = torch.full((1,), 7, dtype=torch.int64, device=dev)
    score, lm_score = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    assert lib.s2t_ctc_prefix_beam_ngram(desc, N.fp(x), N.lp(lens), 1, 2, V, blank, beam, topk,
                                         change.get("weight", 0.3), start, wsp, N.lp(tokens), N.lp(out_len),
                                         N.fp(score), N.fp(lm_score), N.stream()) == -1
    if {"lm", "order", "num_ctx", "num_arcs", "null"} & set(change):   # the look-up's own entry refuses them too
        ctx = torch.zeros(4, dtype=torch.int32, device=dev)
        logp, nxt = torch.full((4,), 7.0, device=dev), torch.full((4,), 7, dtype=torch.int32, device=dev)
        assert lib.s2t_ngram_score(desc, 4, N.ip(ctx), N.ip(ctx), N.fp(logp), N.ip(nxt), N.stream()) == -1
        torch.cuda.synchronize()
        assert logp.tolist() == [7.0] * 4 and nxt.tolist() == [7] * 4
    torch.cuda.synchronize()
    assert tokens.tolist() == [[7, 7]] and int(out_len[0]) == 7
    assert float(score[0]) == 7.0 and float(lm_score[0]) == 7.0
    del ref, keep


def test_empty_batch_returns_zero_and_limits_just_inside_are_taken(dev):
    from speech2text_amd import _native as N
    lib = N.lib()
    lm = _lm(dev, C.lm_text(_V, 3, 200, 2), _V)
    desc, keep = lm.desc()
    assert lib.s2t_ctc_prefix_beam_ngram(desc, None, None, 0, 2, _V, 0, 99, 99, 0.3, 0, None, None, None, None, None,
                                         N.stream()) == 0
    assert lib.s2t_ngram_score(desc, 0, None, None, None, None, N.stream()) == 0
    g = torch.Generator().manual_seed(5)
    x, lens = torch.randn(2, 3, _V, generator=g).to(dev), torch.tensor([3, 2], device=dev)
    for beam, topk in ((16, 16), (1, 16), (16, 1)):
        out = _fused(dict(beam=beam, topk=topk, weight=0.3), x, lens, lm)
        assert out is not None and bool((out[1] <= 3).all())
        assert bool(torch.isfinite(out[2]).all()) and bool(torch.isfinite(out[3]).all())
    assert _fused(dict(beam=17, topk=4, weight=0.3), x, lens, lm) is None
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    top = NgramLm.estimate(C.lm_sequences(6, 100, 0), 6, order=8).to(dev)      # S2T_NGRAM_MAX_ORDER
    small = torch.randn(1, 9, 6, generator=g).to(dev)
    out = _fused(dict(beam=4, topk=99, weight=0.3), small, torch.tensor([9], device=dev), top)
    assert out is not None and bool(torch.isfinite(out[3]).all())
    # a row the look-up is handed outside its ranges is clamped into them
    ctx = torch.tensor([-5, lm.num_ctx + 3], dtype=torch.int32, device=dev)
    tok = torch.tensor([-1, _V + 9], dtype=torch.int32, device=dev)
    logp, _ = lm._device_score(ctx, tok)
    host = C.lm_text(_V, 3, 200, 2)
    cpu = NgramLm.from_arpa(host, num_classes=_V)
    assert float(logp[0]) == float(cpu.score(0, 0)[0])
    assert float(logp[1]) == float(cpu.score(cpu.num_ctx - 1, _V - 1)[0])
    del keep


# ------------------------------------------------------------------ 4. the class
@pytest.mark.parametrize("name", ["n_v6_o3_reenter", "n_v65_o3_b33_beam4_k3_norm", "n_v63_o5_beam16_k16",
                                  "n_v128_o1_beam1_k1"])
def test_class_fused_path_is_the_module_loop(dev, name):
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    c, x, lens, _ = _case(dev, name)
    lm = NgramLm.from_arpa(C.text_of(name), num_classes=c["V"])           # on the CPU: it follows the logits
    dec = CtcPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"])
    fused = dec.beam_tokens(x, lens)
    assert lm.device == x.device
    loop = dec.beam_tokens(x, lens, fused=False)
    assert len(fused) == len(loop) == 4 and fused[0].is_cuda and loop[0].is_cuda
    assert torch.equal(fused[0], loop[0]) and torch.equal(fused[1], loop[1])
    for a, b in zip(fused[2:], loop[2:]):
        assert C.rel_err(a, b) <= 1e-4
    ref = C.reference(name)
    assert dec.decode_batch(x, lens) == [r.tokens for r in ref]
    assert dec.decode(x[:1, :C.clamp(lens[0], c["T"])]) == ref[0].tokens
    cpu = CtcPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=C.model(name),
                                lm_weight=c["weight"])
    assert cpu.decode_batch(x[:2].cpu(), lens[:2].cpu()) == [r.tokens for r in ref[:2]]     # CPU tensors: the loop
    assert C.model(name).device.type == "cpu"


def test_refused_shapes_take_the_module_loop_and_streams_refuse_the_ngram(dev):
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding, CtcStreamingSearch
    name = "n_v11_o2_b17_beam4_k3"
    c, x, lens, lm = _case(dev, name)
    dec = CtcPrefixBeamDecoding(_Ids(), beam_size=17, cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"])
    assert dec._fused(x[:2], lens[:2]) is None
    out = dec.beam_tokens(x[:2], lens[:2])
    assert len(out) == 4 and out[0].is_cuda
    ng = C.dict_model(name, np.float64)
    r = G.prefix_beam_search(x[0, :C.clamp(lens[0], c["T"])].double().cpu(), 17, c["topk"], ng, c["weight"])
    assert out[0][0, :int(out[1][0])].tolist() == r.tokens
    with pytest.raises(ValueError, match="NgramLm"):
        CtcStreamingSearch(c["V"], lm=lm, lm_weight=0.5, device=dev)
    with pytest.raises(ValueError, match="lm_start_token"):
        CtcPrefixBeamDecoding(_Ids(), lm=lm, lm_weight=0.5, lm_start_token=1)
