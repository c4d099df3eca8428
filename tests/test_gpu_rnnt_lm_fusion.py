"""GPU: RNN-LM shallow fusion in the on-device RNN-T beam search (csrc/decode_lstm.hip:
s2t_rnn_lm_step, s2t_rnnt_beam_lstm_lm) against the float64 restatement of tests/rnnt_lm_fusion_f64.py
on the seeded cases of tests/rnnt_lm_fusion_cases.py.

Tokens, counts and emission frames are compared for exact equality: tests/test_rnnt_lm_fusion_f64.py
asserts that float64 decides every node of every utterance of every case by at least 1e-3 and that
float32 walks the same path.  LM states, q rows, score and lm_score are held to max(2e-5, 8 x what
float32 costs the restatement itself), figures recorded in the cases file.  The searches are fed `am`
directly (the joiner's enc_proj replaced by the identity); the validation test runs the real enc_proj.
"""
import copy
import math

import pytest
import torch

import rnnt_lm_fusion_cases as L
import rnnt_lm_fusion_f64 as F
import rnnt_lstm_search_cases as C
import rnnt_lstm_search_f64 as S
from decode_support import _beam_modules, _decoder, _lm_module, _lstm_build, _lstm_modules, _TINY, _Tok, _weights_of
from task_support import _pcm_batch, _refs, _rnnt_cfg, _task

pytestmark = pytest.mark.gpu


_CACHE = {}


def _case(dev, name):
    """(case, predictor, joiner, LM, am and lengths on the device, the float64 results), once per case."""
    if name not in _CACHE:
        c = L.CASES[name]
        w, act, am, lens, sd = L.make(name)
        p, j = _lstm_modules(dev, w, C.CASES[c["base"]]["model"])
        _CACHE[name] = (c, p, j, _lm_module(dev, sd), am.to(dev), lens.to(dev), L.reference(name))
    return _CACHE[name]


def _fused(c, p, j, lm, am, lens, **kw):
    from speech2text_amd.model.decoding import rnnt_beam_lstm_lm_tokens_from_am
    args = dict(lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"], lm_start_token=c["start"])
    args.update(kw)
    return rnnt_beam_lstm_lm_tokens_from_am(am, lens, p, j, lm, **args)


# ------------------------------------------------------------------ 1. the LM step alone
@pytest.mark.parametrize("model", list(L.STEP_MODELS))
def test_lm_step_chain(dev, model):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnn_lm_desc
    m, R = L.LM_MODELS[model], C.PRED_ROWS
    lm = _lm_module(dev, L.lm_weights(model, 100))
    desc, keep = rnn_lm_desc(lm)
    nbytes = N.lib().s2t_rnn_lm_step_workspace_bytes(desc, R)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    new = lambda: [torch.zeros(m["L"], R, m["H"], device=dev), torch.zeros(m["L"], R, m["H"], device=dev),  # noqa: E731
                   torch.zeros(R, m["V"], device=dev)]
    cur, ref = new(), L.step_chain(model, torch.float64)
    limit = L.bound(L.LM_STEP_COST[model])
    for i, (tokens, emit, parent) in enumerate(C.pred_schedule(L.STEP_MODELS[model])):
        ident = torch.equal(parent, torch.arange(R))
        before = [t.clone() for t in cur]
        out = cur if ident else new()                      # in place without a gather, else disjoint
        dt, de, dp = (x.to(device=dev, dtype=torch.int32) for x in (tokens, emit, parent))
        rc = N.lib().s2t_rnn_lm_step(desc, R, N.ip(dt), N.ip(de), None if ident else N.ip(dp),
                                     N.fp(cur[0]), N.fp(cur[1]), N.fp(cur[2]),
                                     N.fp(out[0]), N.fp(out[1]), N.fp(out[2]), N.ptr(ws), N.stream())
        assert rc == 0
        for r in (emit == 0).nonzero().flatten().tolist():  # masked: the parent's row, bit for bit
            q = int(parent[r])
            assert torch.equal(out[0][:, r], before[0][:, q]) and torch.equal(out[1][:, r], before[1][:, q])
            assert torch.equal(out[2][r], before[2][q])
        cur = out
        if i in (0, 4):
            q, (h, c) = ref[i]
            errs = {"q": C.rel_err(cur[2], q), "h": C.rel_err(cur[0], h), "c": C.rel_err(cur[1], c)}
            print(f"{model} after step {i + 1}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()),
                  f"bound {limit:.2e}")
            assert max(errs.values()) <= limit, (model, i, errs, limit)
            rows = (emit != 0).nonzero().flatten().to(dev)
            assert torch.allclose(cur[2][rows].exp().sum(-1), torch.ones(len(rows), device=dev), atol=1e-5)
    bad = torch.zeros(R, dtype=torch.int32, device=dev)   # same buffers with a gather: refused
    assert N.lib().s2t_rnn_lm_step(desc, R, N.ip(dt), N.ip(de), N.ip(bad), N.fp(cur[0]), N.fp(cur[1]),
                                   N.fp(cur[2]), N.fp(cur[0]), N.fp(cur[1]), N.fp(cur[2]), N.ptr(ws),
                                   N.stream()) == -1


# ------------------------------------------------------------------ 2. the fused search
@pytest.mark.parametrize("name", list(L.CASES))
def test_fused_search_exact(dev, name):
    from speech2text_amd import _native as N
    c, p, j, lm, am, lens, ref = _case(dev, name)
    B, T = am.shape[0], am.shape[1]
    dec = _decoder(c, p, j, lm)
    assert dec._lstm_search() and not dec._fusable()
    want = (torch.tensor([r[1] for r in ref], dtype=torch.float64),
            torch.tensor([r[2] for r in ref], dtype=torch.float64))
    limit = L.bound(L.FUSED_COST[name])
    for how in ("abi", "class"):
        out = _fused(c, p, j, lm, am, lens) if how == "abi" else dec.beam_tokens(am, lens)
        assert out is not None and len(out) == 5
        tokens, frames, out_len, score, lm_score = (x.cpu() for x in out)
        assert tokens.shape == frames.shape == (B, T) and tokens.dtype == torch.int64
        assert score.dtype == lm_score.dtype == torch.float32
        for b, (tok, _, _, frm, _) in enumerate(ref):
            assert int(out_len[b]) == len(tok), (name, how, b, int(out_len[b]), len(tok))
            assert tokens[b, :len(tok)].tolist() == tok, (name, how, b)
            assert frames[b, :len(tok)].tolist() == frm, (name, how, b)
            assert (tokens[b, len(tok):] == 0).all() and (frames[b, len(tok):] == 0).all()
        errs = C.rel_err(score, want[0]), C.rel_err(lm_score, want[1])
        print(f"{name} {how}: score rel_err {errs[0]:.2e} lm_score rel_err {errs[1]:.2e} bound {limit:.2e}")
        assert max(errs) <= limit, (name, how, errs, limit)
        if B > 1:                                          # no frames: no tokens, score 0, lm_score 0
            assert float(score[1]) == 0.0 and float(lm_score[1]) == 0.0 and int(out_len[1]) == 0
    texts = dec.decode_batch(am, lens)
    assert texts == [_Tok().decode(r[0]) for r in ref]
    n0 = C.clamp(lens[0], T)
    assert dec.decode(am[0:1, :n0]) == texts[0]            # one utterance: the same kernels, B = 1
    # the module loop on the device (fp32 modules, six-product GEMMs): the same tokens
    assert N.lib().s2t_gemm_arith_set(3) == 0
    try:
        tokens, frames, out_len, _, _ = (x.cpu() for x in dec.beam_tokens(am, lens, fused=False))
    finally:
        N.lib().s2t_gemm_arith_set(0)
    for b, (tok, _, _, frm, _) in enumerate(ref):
        assert tokens[b, :int(out_len[b])].tolist() == tok and frames[b, :int(out_len[b])].tolist() == frm, (name, b)


# ------------------------------------------------------------------ 3. lm_weight 0
def test_weight_zero_is_the_unfused_search_bit_for_bit(dev):
    from speech2text_amd.model.decoding import rnnt_beam_lstm_tokens_from_am
    c, p, j, lm, am, lens, _ = _case(dev, L.B33)
    assert am.shape[0] == 33
    plain = rnnt_beam_lstm_tokens_from_am(am, lens, p, j, c["beam"], c["topk"])
    for start in (None, am.shape[2] - 1):
        out = _fused(c, p, j, lm, am, lens, lm_weight=0.0, lm_start_token=start)
        for x, y in zip(out[:4], plain):
            assert torch.equal(x, y), start
        assert bool(torch.isfinite(out[4]).all()) and float(out[4].abs().max()) > 0
    assert int(plain[2].sum()) > 0
    fused = _fused(c, p, j, lm, am, lens)
    assert not torch.equal(fused[0], plain[0])             # and the LM term is not inert


# ------------------------------------------------------------------ 4. lm_score is the module's own score
@pytest.mark.parametrize("name", ["f_h48_b17_beam4", "f_h64_beam16_k4_start", "f_yaml"])
def test_lm_score_is_rnn_lm_score_of_the_tokens(dev, name):
    from speech2text_amd import _native as N
    c, p, j, lm, am, lens, ref = _case(dev, name)
    tokens, _, out_len, _, lm_score = _fused(c, p, j, lm, am, lens)
    B, T = tokens.shape
    n = out_len.cpu().tolist()
    pre = [] if c["start"] is None else [c["start"]]
    seqs = torch.zeros((B, T + 2), dtype=torch.int64)
    for b in range(B):
        seqs[b, :len(pre) + n[b]] = torch.tensor(pre + tokens[b, :n[b]].tolist(), dtype=torch.int64)
    lens2 = torch.tensor([max(2, len(pre) + k) for k in n])   # (a sequence of < 2 tokens scores 0)
    seqs = seqs[:, :int(lens2.max())].contiguous()         # (score masks up to the longest length)
    assert N.lib().s2t_gemm_arith_set(3) == 0
    try:
        got = lm.score(seqs.to(dev), lens2.to(dev)).cpu()
    finally:
        N.lib().s2t_gemm_arith_set(0)
    for b in range(B):
        if len(pre) + n[b] < 2:
            got[b] = 0.0
    err, limit = C.rel_err(lm_score, got), L.bound(L.FUSED_COST[name])
    print(f"{name}: lm_score against RnnLm.score rel_err {err:.2e} bound {limit:.2e}")
    assert float(got.abs().max()) > 0 and err <= limit, (name, err, limit)


# ------------------------------------------------------------------ 5. batch invariance
def test_batch_invariance(dev):
    """Utterance b alone, inside the first 17 and inside all 33: bit-identical, all five outputs."""
    c, p, j, lm, am, lens, _ = _case(dev, L.B33)
    runs = {n: _fused(c, p, j, lm, am[:n], lens[:n]) for n in (17, 33)}
    for b in (0, 2, 7, 15, 16):
        alone = _fused(c, p, j, lm, am[b:b + 1], lens[b:b + 1])
        assert len(alone) == 5
        for n, out in runs.items():
            for x, y in zip(alone, out):
                assert torch.equal(x[0], y[b]), (b, n)
    for x, y in zip(runs[17], runs[33]):
        assert torch.equal(x, y[:17])


# ------------------------------------------------------------------ 6. limits
_V = _TINY["V"]


def _tiny_run(dev, p, j, lm, **kw):
    from speech2text_amd.model.decoding import rnnt_beam_lstm_lm_tokens_from_am
    g = torch.Generator().manual_seed(3)
    am = torch.randn(1, 2, _V, generator=g).to(dev)
    lens = torch.tensor([2], device=dev)
    return am, lens, rnnt_beam_lstm_lm_tokens_from_am(am, lens, p, j, lm, 0.3, 4, 4, **kw)


@pytest.mark.parametrize("H,layers", [(1024, 1), (8, 8)])
def test_limits_just_inside_are_taken(dev, H, layers):
    p, j = _lstm_build(dev, **_TINY)
    lm = _lm_module(dev, V=_V, H=H, layers=layers)
    for start in (None, _V - 1):
        _, _, out = _tiny_run(dev, p, j, lm, lm_start_token=start)
        assert out is not None and 0 <= int(out[2][0]) <= 2
        assert bool(torch.isfinite(out[3]).all()) and bool(torch.isfinite(out[4]).all())


@pytest.mark.parametrize("change", [dict(H=1028), dict(H=22), dict(H=0), dict(E=1025), dict(num_layers=9),
                                    dict(num_layers=0), dict(V=_V + 1), dict(start=_V), dict(weight=math.inf),
                                    dict(weight=math.nan), dict(beam=17), dict(beam=0), dict(topk=0)], ids=str)
def test_limits_just_outside_return_minus_one(dev, change):
    """Outside the limits every entry point answers -1 (the workspace size 0) before any launch -- the
    pointers are never followed (the workspace here is 256 bytes) and no output is touched."""
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnn_lm_desc, rnnt_lstm_desc
    p, j = _lstm_build(dev, **_TINY)
    lm = _lm_module(dev, V=_V, H=8, layers=1)
    desc, keep = rnnt_lstm_desc(p, j)
    lm_desc, lm_keep = rnn_lm_desc(lm)
    lib = N.lib()
    assert lib.s2t_rnnt_beam_lstm_lm_workspace_bytes(desc, lm_desc, 1, 2, 4) > 0
    assert lib.s2t_rnn_lm_step_workspace_bytes(lm_desc, 1) > 0
    in_desc = {k: v for k, v in change.items() if k in ("H", "E", "num_layers", "V")}
    for k, v in in_desc.items():
        setattr(lm_keep[-1], k, v)
    beam, topk = change.get("beam", 4), change.get("topk", 4)
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    am, lens = torch.zeros(1, 2, _V, device=dev), torch.tensor([2], device=dev)
    tokens, frames = torch.zeros(1, 2, dtype=torch.int64, device=dev), torch.zeros(1, 2, dtype=torch.int64, device=dev)
    out_len = torch.zeros(1, dtype=torch.int64, device=dev)
    score, lm_score = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    if in_desc or "beam" in change:
        assert lib.s2t_rnnt_beam_lstm_lm_workspace_bytes(desc, lm_desc, 1, 2, beam) == 0
    assert lib.s2t_rnnt_beam_lstm_lm(desc, lm_desc, N.fp(am), N.lp(lens), 1, 2, beam, topk,
                                     change.get("weight", 0.3), change.get("start", -1), N.ptr(ws), N.lp(tokens),
                                     N.lp(frames), N.lp(out_len), N.fp(score), N.fp(lm_score), N.stream()) == -1
    if in_desc and "V" not in in_desc:                     # (the step alone has no second vocabulary)
        i32, f = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(64, device=dev)
        assert lib.s2t_rnn_lm_step_workspace_bytes(lm_desc, 1) == 0
        assert lib.s2t_rnn_lm_step(lm_desc, 1, N.ip(i32), N.ip(i32), None, N.fp(f), N.fp(f), N.fp(f), N.fp(f),
                                   N.fp(f), N.fp(f), N.ptr(ws), N.stream()) == -1
    torch.cuda.synchronize()
    assert int(tokens.sum()) == 0 and int(frames.sum()) == 0 and int(out_len.sum()) == 0
    assert float(score[0]) == 0.0 and float(lm_score[0]) == 0.0


def test_refused_shapes_take_the_module_loop(dev):
    """An LM wider than the limit, a vocabulary that is not the joiner's, a beam above 16: the wrapper
    returns None and the class answers with _module_loop_lm."""
    from speech2text_amd.model.decoding import RnntBeamDecoding
    p, j = _lstm_build(dev, **_TINY)
    wide = _lm_module(dev, V=_V, H=1028, layers=1)
    am, lens, out = _tiny_run(dev, p, j, wide)
    assert out is None
    assert _tiny_run(dev, p, j, _lm_module(dev, V=_V + 1, H=8, layers=1))[2] is None
    dec = RnntBeamDecoding(_Tok(), p, j, beam_size=2, cutoff_top_k=2, lm=wide, lm_weight=0.3)
    assert dec._lstm_search()
    with torch.no_grad():
        tok, frm, score, lm_score = dec._module_loop_lm(am)
    got = dec.beam_tokens(am, lens)
    assert len(got) == 5 and got[0].is_cuda
    assert got[0][0, :int(got[2][0])].tolist() == tok and got[1][0, :int(got[2][0])].tolist() == frm
    assert float(got[3][0]) == pytest.approx(score) and float(got[4][0]) == pytest.approx(lm_score)
    assert dec.decode_batch(am, lens) == [_Tok().decode(tok)]
    c, p2, j2, lm2, am2, lens2, ref = _case(dev, "f_h20_beam1_k1")
    assert _fused(c, p2, j2, lm2, am2, lens2, beam_size=17) is None
    loop = _decoder(c, p2, j2, lm2, beam_size=17)          # (top-1: beam 1 in effect)
    assert loop.decode_batch(am2, lens2) == [_Tok().decode(r[0]) for r in ref]


# ------------------------------------------------------------------ 7. the stateless predictor
def test_stateless_predictor_takes_the_module_loop(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import RnntBeamDecoding
    c, am, lens, sd = L.stateless_case()
    ref = L.stateless_reference()
    print("stateless: float64 margins", [r[4] for r in ref], "tokens", [r[0] for r in ref])
    assert min(r[4] for r in ref) >= S.MARGIN and sum(len(r[0]) for r in ref) > 0
    pred, join = _beam_modules(c, dev)
    join._enc_proj = torch.nn.Identity()
    lm = _lm_module(dev, sd)
    dec = RnntBeamDecoding(_Tok(), pred.eval(), join.eval(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm,
                           lm_weight=c["weight"], lm_start_token=c["start"])
    assert dec._fusable() and not dec._lstm_search()       # fusable without an LM; with one: the loop
    assert N.lib().s2t_gemm_arith_set(3) == 0
    try:
        tokens, frames, out_len, score, lm_score = (x.cpu() for x in dec.beam_tokens(am.to(dev), lens))
    finally:
        N.lib().s2t_gemm_arith_set(0)
    for b, (tok, sc, lms, frm, _) in enumerate(ref):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == tok and frames[b, :n].tolist() == frm, b
        assert float(score[b]) == pytest.approx(sc, rel=1e-4, abs=1e-4)
        assert float(lm_score[b]) == pytest.approx(lms, rel=1e-4, abs=1e-4)


# ------------------------------------------------------------------ 8. validation_step
def test_validation_step_logs_the_restatements_wer(dev):
    from oracle import decoding as OD
    cfg, V = _rnnt_cfg()
    cfg = copy.deepcopy(cfg)
    cfg["metric"].update({"lm_weight": 0.3, "lm": {"config": {"num_symbols": V, "symbol_embedding_dim": 24,
                                                               "num_rnn_layer": 2}, "checkpoint": None}})
    batch = _pcm_batch(dev, B=2, sec=1.0, V=V)
    task = _task("Rnnt", cfg, dev)
    keys = list(task.state_dict())
    sess = task._metric._decode_sess
    with torch.no_grad():                                  # away from the near-ties of fresh models
        for q in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            q.mul_(6.0)
        sess._lm._logits_layer.weight.mul_(16.0)
        for k in range(2):
            getattr(sess._lm._rnn_layer, f"weight_ih_l{k}").mul_(3.0)
    assert sess._lstm_search() and sess._lm is not None and (sess._lm_weight, sess._beam_size) == (0.3, 3)
    assert next(sess._lm.parameters()).device.type == "cpu"            # the task's .to() does not own it
    info = task.validation_step(batch, 0)
    assert "wer" in task.logged and next(sess._lm.parameters()).device.type == "cuda"
    assert list(task.state_dict()) == keys
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
    w = _weights_of(task._predictor, task._joiner)
    sd = {k: v.detach().double().cpu() for k, v in sess._lm.state_dict().items()}
    hyps, plain, margins = [], [], []
    for b in range(enc.shape[0]):
        with torch.no_grad():
            am = task._joiner._enc_proj(enc[b:b + 1, :int(el[b])])[0].double().cpu()
        ids, _, _, _, margin = F.beam_search_lm(am, w, "tanh", 3, 3, sd, 0.3)
        plain.append(S.beam_search(am, w, "tanh", 3, 3)[0])
        margins.append(margin)
        hyps.append(task._tokenizer.decode(torch.tensor(ids, dtype=torch.int64)))
    print(f"hypotheses {hyps}, un-fused token ids {plain}, smallest float64 margins {margins}")
    plain = [task._tokenizer.decode(torch.tensor(ids, dtype=torch.int64)) for ids in plain]
    assert hyps != plain, "the LM changes no hypothesis: a search that dropped its term would pass"
    assert info["wer"] == pytest.approx(OD.word_error_rate(hyps, _refs(task, batch["label"])))
