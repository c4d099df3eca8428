"""GPU: RNN-T greedy and beam search with the LSTM predictor on the device (csrc/decode_lstm.hip)
against the float64 restatement of tests/rnnt_lstm_search_f64.py on the seeded cases of
tests/rnnt_lstm_search_cases.py.

Tokens, counts and emission frames are compared for exact equality: tests/
test_rnnt_lstm_search_f64.py asserts that float64 decides every node of every utterance of every
case by at least 1e-3 and that float32 walks the same path.  States, lm vectors and beam scores are
held to max(2e-5, 8 x what float32 costs the restatement itself), figures recorded in the cases file.
The searches are fed `am` directly (the joiner's enc_proj replaced by the identity), so that they
see exactly the inputs the margins were established on; the validation test runs the real enc_proj.
"""
import copy

import pytest
import torch

import rnnt_lstm_search_cases as C
import rnnt_lstm_search_f64 as S
from decode_support import _lstm_build, _lstm_case, _lstm_modules, _TINY, _Tok, _weights_of
from task_support import _base_cfg, _CONF, _pcm_batch, _refs, _task, _TOK, _V

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the predictor step alone
@pytest.mark.parametrize("model", C.PRED_MODELS)
def test_pred_step_chain(dev, model):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnnt_lstm_desc
    m, R = C.MODELS[model], C.PRED_ROWS
    p, j = _lstm_modules(dev, C.weights(model, 100), model)
    desc, keep = rnnt_lstm_desc(p, j)
    nbytes = N.lib().s2t_rnnt_lstm_workspace_bytes(desc, R, 0, 0)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    new = lambda: [torch.zeros(m["L"], R, m["H"], device=dev), torch.zeros(m["L"], R, m["H"], device=dev),  # noqa: E731
                   torch.zeros(R, m["V"], device=dev)]
    cur, ref = new(), C.pred_chain(model, torch.float64)
    limit = C.bound(C.PRED_COST[model])
    for i, (tokens, emit, parent) in enumerate(C.pred_schedule(model)):
        ident = torch.equal(parent, torch.arange(R))
        before = [t.clone() for t in cur]
        out = cur if ident else new()                      # in place without a gather, else disjoint
        dt, de, dp = (x.to(device=dev, dtype=torch.int32) for x in (tokens, emit, parent))
        rc = N.lib().s2t_lstm_pred_step(desc, R, N.ip(dt), N.ip(de), None if ident else N.ip(dp),
                                        N.fp(cur[0]), N.fp(cur[1]), N.fp(cur[2]),
                                        N.fp(out[0]), N.fp(out[1]), N.fp(out[2]), N.ptr(ws), N.stream())
        assert rc == 0
        for r in (emit == 0).nonzero().flatten().tolist():  # masked: the parent's row, bit for bit
            q = int(parent[r])
            assert torch.equal(out[0][:, r], before[0][:, q]) and torch.equal(out[1][:, r], before[1][:, q])
            assert torch.equal(out[2][r], before[2][q])
        cur = out
        if i in (0, 4):
            lm, state = ref[i]
            errs = {"lm": C.rel_err(cur[2], lm)}
            for l, (h, c) in enumerate(state):
                errs[f"h{l}"], errs[f"c{l}"] = C.rel_err(cur[0][l], h), C.rel_err(cur[1][l], c)
            print(f"{model} after step {i + 1}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()),
                  f"bound {limit:.2e}")
            assert max(errs.values()) <= limit, (model, i, errs, limit)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)   # same buffers with a gather: refused
    assert N.lib().s2t_lstm_pred_step(desc, R, N.ip(dt), N.ip(de), N.ip(bad.expand(R).contiguous()),
                                      N.fp(cur[0]), N.fp(cur[1]), N.fp(cur[2]), N.fp(cur[0]), N.fp(cur[1]),
                                      N.fp(cur[2]), N.ptr(ws), N.stream()) == -1


# ------------------------------------------------------------------ 2. greedy
@pytest.mark.parametrize("name", list(C.GREEDY_CASES))
def test_greedy_exact(dev, name):
    from speech2text_amd.model.decoding import RnntGreedyDecoding, rnnt_greedy_lstm_tokens_from_am
    c, p, j, am, lens, ref = _lstm_case(dev, name)
    max_out = c["T"] * (c["mts"] + 1)
    dec = RnntGreedyDecoding(_Tok(), p, j, max_token_step=c["mts"])
    assert dec._lstm_search() and not dec._fusable() and not dec._fused()
    for how in ("abi", "class"):
        out = rnnt_greedy_lstm_tokens_from_am(am, lens, p, j, c["mts"]) if how == "abi" \
            else dec.greedy_tokens_lstm(am, lens)
        assert out is not None
        tokens, out_len = (x.cpu() for x in out)
        assert tokens.shape == (c["B"], max_out) and tokens.dtype == torch.int64
        for b, r in enumerate(ref):
            assert int(out_len[b]) == len(r[0]), (name, how, b, int(out_len[b]), len(r[0]))
            assert tokens[b, :len(r[0])].tolist() == r[0], (name, how, b)
            assert (tokens[b, len(r[0]):] == 0).all(), "the buffer beyond out_len lost the wrapper's zeros"
    texts = dec.decode_batch(am, lens)
    assert texts == [_Tok().decode(r[0]) for r in ref]
    n0 = C.clamp(lens[0], c["T"])
    assert dec.decode(am[0:1, :n0]) == texts[0]            # one utterance: the same kernels, B = 1


# ------------------------------------------------------------------ 3. beam
@pytest.mark.parametrize("name", list(C.BEAM_CASES))
def test_beam_exact(dev, name):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import RnntBeamDecoding, rnnt_beam_lstm_tokens_from_am
    c, p, j, am, lens, ref = _lstm_case(dev, name)
    dec = RnntBeamDecoding(_Tok(), p, j, beam_size=c["beam"], cutoff_top_k=c["topk"])
    assert dec._lstm_search() and not dec._fusable()
    want = torch.tensor([r[1] for r in ref])
    limit = C.bound(C.BEAM_COST[name])
    for how in ("abi", "class"):
        out = rnnt_beam_lstm_tokens_from_am(am, lens, p, j, c["beam"], c["topk"]) if how == "abi" \
            else dec.beam_tokens(am, lens)
        assert out is not None
        tokens, frames, out_len, score = (x.cpu() for x in out)
        assert tokens.shape == frames.shape == (c["B"], c["T"])
        for b, (tok, _, frm, _) in enumerate(ref):
            assert int(out_len[b]) == len(tok), (name, how, b, int(out_len[b]), len(tok))
            assert tokens[b, :len(tok)].tolist() == tok, (name, how, b)
            assert frames[b, :len(tok)].tolist() == frm, (name, how, b)
            assert (tokens[b, len(tok):] == 0).all() and (frames[b, len(tok):] == 0).all()
        err = C.rel_err(score, want)
        print(f"{name} {how}: score rel_err {err:.2e} bound {limit:.2e}")
        assert err <= limit, (name, how, err, limit)
    texts = dec.decode_batch(am, lens)
    assert texts == [_Tok().decode(r[0]) for r in ref]
    n0 = C.clamp(lens[0], c["T"])
    assert dec.decode(am[0:1, :n0]) == texts[0]
    # the module loop on the device (fp32 modules, six-product GEMMs): the same tokens
    assert N.lib().s2t_gemm_arith_set(3) == 0
    try:
        tokens, frames, out_len, _ = (x.cpu() for x in dec.beam_tokens(am, lens, fused=False))
    finally:
        N.lib().s2t_gemm_arith_set(0)
    for b, (tok, _, frm, _) in enumerate(ref):
        assert tokens[b, :int(out_len[b])].tolist() == tok and frames[b, :int(out_len[b])].tolist() == frm, (name, b)


# ------------------------------------------------------------------ 4. batch invariance
def test_batch_invariance(dev):
    """Utterance b alone, inside the first 17 and inside all 33: bit-identical tokens (and score)."""
    from speech2text_amd.model.decoding import rnnt_beam_lstm_tokens_from_am, rnnt_greedy_lstm_tokens_from_am
    c, p, j, am, lens, _ = _lstm_case(dev, "g_h64_b33_mts0")
    runs = {n: rnnt_greedy_lstm_tokens_from_am(am[:n], lens[:n], p, j, c["mts"]) for n in (17, 33)}
    for b in (0, 2, 7, 15, 16):
        alone = rnnt_greedy_lstm_tokens_from_am(am[b:b + 1], lens[b:b + 1], p, j, c["mts"])
        for n, (tokens, out_len) in runs.items():
            assert torch.equal(alone[0][0], tokens[b]) and torch.equal(alone[1][0], out_len[b]), (b, n)
    assert torch.equal(runs[17][0], runs[33][0][:17])
    c, p, j, am, lens, _ = _lstm_case(dev, "b_h64o_b33_beam4_k1")
    runs = {n: rnnt_beam_lstm_tokens_from_am(am[:n], lens[:n], p, j, c["beam"], 4) for n in (17, 33)}
    for b in (0, 2, 7, 15, 16):
        alone = rnnt_beam_lstm_tokens_from_am(am[b:b + 1], lens[b:b + 1], p, j, c["beam"], 4)
        for n, out in runs.items():
            for x, y in zip(alone, out):
                assert torch.equal(x[0], y[b]), (b, n)
    for x, y in zip(runs[17], runs[33]):
        assert torch.equal(x, y[:17])


# ------------------------------------------------------------------ 5. refusals


def _run_both(dev, p, j, V, beam=4, topk=4, T=2):
    from speech2text_amd.model.decoding import rnnt_beam_lstm_tokens_from_am, rnnt_greedy_lstm_tokens_from_am
    g = torch.Generator().manual_seed(3)
    am = torch.randn(1, T, V, generator=g).to(dev)
    lens = torch.tensor([T], device=dev)
    return (am, lens, rnnt_greedy_lstm_tokens_from_am(am, lens, p, j, 1),
            rnnt_beam_lstm_tokens_from_am(am, lens, p, j, beam, topk))


@pytest.mark.parametrize("change", [dict(E=1024, H=1024), dict(L=8), dict(V=8192), dict(inner=8192),
                                    dict(D=8192), dict(V=63, beam=16, topk=16)], ids=str)
def test_limits_just_inside_are_taken(dev, change):
    change = dict(change)
    beam, topk = change.pop("beam", 4), change.pop("topk", 4)
    dims = dict(_TINY, **change)
    p, j = _lstm_build(dev, **dims)
    _, _, greedy, beams = _run_both(dev, p, j, dims["V"], beam, topk)
    assert greedy is not None and beams is not None
    assert 0 <= int(greedy[1][0]) <= 4 and 0 <= int(beams[2][0]) <= 2
    assert bool(torch.isfinite(beams[3]).all())


@pytest.mark.parametrize("field,value", [("H", 1028), ("H", 22), ("H", 0), ("E", 1025), ("E", 0),
                                         ("num_layers", 9), ("num_layers", 0), ("V", 8193), ("V", 0),
                                         ("inner", 8193), ("inner", -1), ("D", 8193), ("D", 0), ("act", 2)])
def test_limits_just_outside_return_minus_one(dev, field, value):
    """A descriptor outside the limits: every entry point answers -1 (the workspace size 0) before
    any launch -- the pointers are never followed (the workspace here is 256 bytes)."""
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnnt_lstm_desc
    p, j = _lstm_build(dev, **_TINY)
    desc, keep = rnnt_lstm_desc(p, j)
    setattr(keep[-1], field, value)
    lib = N.lib()
    assert lib.s2t_rnnt_lstm_workspace_bytes(desc, 1, 2, 0) == 0
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    am, lens = torch.zeros(1, 2, 16, device=dev), torch.tensor([2], device=dev)
    tokens, frames = torch.zeros(1, 4, dtype=torch.int64, device=dev), torch.zeros(1, 2, dtype=torch.int64, device=dev)
    out_len, score = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, device=dev)
    i32 = torch.zeros(1, dtype=torch.int32, device=dev)
    f = torch.zeros(64, device=dev)
    assert lib.s2t_rnnt_greedy_lstm(desc, N.fp(am), N.lp(lens), 1, 2, 1, N.ptr(ws), N.lp(tokens),
                                    N.lp(out_len), N.stream()) == -1
    assert lib.s2t_rnnt_beam_lstm(desc, N.fp(am), N.lp(lens), 1, 2, 4, 4, N.ptr(ws), N.lp(tokens),
                                  N.lp(frames), N.lp(out_len), N.fp(score), N.stream()) == -1
    assert lib.s2t_lstm_pred_step(desc, 1, N.ip(i32), N.ip(i32), None, N.fp(f), N.fp(f), N.fp(f), N.fp(f),
                                  N.fp(f), N.fp(f), N.ptr(ws), N.stream()) == -1
    torch.cuda.synchronize()
    assert int(tokens.sum()) == 0 and int(out_len.sum()) == 0


def test_refused_shapes_take_the_module_loop(dev):
    """beam_size / cutoff_top_k outside 1..16 and an LSTM wider than the limit: the entry points
    refuse, the classes answer with the module loop."""
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import (RnntBeamDecoding, RnntGreedyDecoding, rnnt_beam_lstm_tokens_from_am,
                                                rnnt_lstm_desc)
    c, p, j, am, lens, ref = _lstm_case(dev, "b_h20_beam1_k1")
    desc, keep = rnnt_lstm_desc(p, j)
    ws = torch.zeros(N.lib().s2t_rnnt_lstm_workspace_bytes(desc, 1, 2, 16), dtype=torch.uint8, device=dev)
    for beam, topk, rc in ((17, 4, -1), (0, 4, -1), (4, 17, -1), (4, 0, -1)):
        z = torch.zeros(1, 2, dtype=torch.int64, device=dev)
        got = N.lib().s2t_rnnt_beam_lstm(desc, N.fp(am[:1, :2].contiguous()), N.lp(lens[:1]), 1, 2, beam, topk,
                                         N.ptr(ws), N.lp(z), N.lp(z.clone()), N.lp(z[0, :1].clone()),
                                         N.fp(torch.zeros(1, device=dev)), N.stream())
        assert got == rc, (beam, topk)
    assert rnnt_beam_lstm_tokens_from_am(am, lens, p, j, 17, 4) is None
    assert rnnt_beam_lstm_tokens_from_am(am, lens, p, j, 4, 17) is None       # V = 63: min(17, V) > 16
    wide = RnntBeamDecoding(_Tok(), p, j, beam_size=17, cutoff_top_k=1)       # (top-1: beam 1 in effect)
    texts = wide.decode_batch(am, lens)
    assert texts == [_Tok().decode(r[0]) for r in ref]
    p2, j2 = _lstm_build(dev, **dict(_TINY, H=1028))
    am2, lens2, greedy, beams = _run_both(dev, p2, j2, 16)
    assert greedy is None and beams is None
    g = RnntGreedyDecoding(_Tok(), p2, j2, max_token_step=1)
    b = RnntBeamDecoding(_Tok(), p2, j2, beam_size=2, cutoff_top_k=2)
    assert g._lstm_search() and b._lstm_search()
    with torch.no_grad():
        assert g.decode_batch(am2, lens2) == [g._module_loop(am2)]
        tok, frm, _ = b._module_loop(am2)
    assert b.decode_batch(am2, lens2) == [_Tok().decode(tok)]


# ------------------------------------------------------------------ 6. validation_step
def test_validation_steps_log_the_restatements_wer(dev):
    from oracle import decoding as OD
    cfg = _base_cfg()
    cfg.update({"task": {"type": "CTC_Hybrid_Rnnt"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Projector", "config": {"input_dim": 64, "output_dim": _V, "dropout_p": 0.1}},
                "predictor": {"model": "Lstm", "config": {"num_symbols": _V, "output_dim": 64,
                                                          "symbol_embedding_dim": 32, "num_lstm_layers": 2,
                                                          "lstm_hidden_dim": 48, "lstm_layer_norm": True,
                                                          "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.1}},
                "joiner": {"input_dim": 64, "output_dim": _V, "inner_dim": 48, "activation": "tanh",
                           "prune_range": -1},
                "metric": {"decode_method": "rnnt_greedy_search", "max_token_step": 2},
                "loss": {"rnnt_weight": 0.8, "ctc_weight": 0.2,
                         "rnnt_loss": {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}},
                         "ctc_loss": {"model": "CTC", "config": {"blank_label": 0, "reduction": "mean"}}}})
    cfg2 = copy.deepcopy(cfg)
    cfg2["task"] = {"type": "Rnnt"}
    cfg2["decoder"] = {"model": "Identity", "config": {"dummy": -1}}
    cfg2["loss"] = {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}}
    cfg2["metric"] = {"decode_method": "rnnt_beam_search", "beam_size": 3, "cutoff_top_k": 3}
    batch = _pcm_batch(dev, B=2, sec=1.0, V=_V)
    for kind, conf in (("CTC_Hybrid_Rnnt", cfg), ("Rnnt", cfg2)):
        task = _task(kind, conf, dev)
        with torch.no_grad():                              # away from the near-ties of a fresh model
            for q in list(task._predictor.parameters()) + list(task._joiner.parameters()):
                q.mul_(3.0)
        sess = task._metric._decode_sess
        assert sess._lstm_search()
        info = task.validation_step(batch, 0)
        assert "wer" in task.logged
        with torch.no_grad():
            feat, n = task.features(batch)
            enc, el = task._encoder(feat, n)
        w = _weights_of(task._predictor, task._joiner)
        hyps, margins = [], []
        for b in range(enc.shape[0]):
            with torch.no_grad():
                am = task._joiner._enc_proj(enc[b:b + 1, :int(el[b])])[0].double().cpu()
            if kind == "Rnnt":
                ids, _, _, margin = S.beam_search(am, w, "tanh", 3, 3)
            else:
                ids, margin, _ = S.greedy(am, w, "tanh", 2)
            margins.append(margin)
            hyps.append(task._tokenizer.decode(torch.tensor(ids, dtype=torch.int64)))
        print(f"{kind}: hypotheses {hyps}, smallest float64 margins {margins}")
        assert info["wer"] == pytest.approx(OD.word_error_rate(hyps, _refs(task, batch["label"])))
