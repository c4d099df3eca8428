"""GPU: RNN-LM shallow fusion in the on-device RNN-T beam search over the stateless predictor
(csrc/decode_lstm.hip: s2t_stateless_pred_step, s2t_rnnt_beam_stateless_lm) against the float64
restatement of tests/rnnt_stateless_lm_f64.py on the seeded cases of tests/rnnt_stateless_lm_cases.py.

Tokens, counts and emission frames are compared for exact equality: tests/test_rnnt_stateless_lm_f64.py
asserts that float64 decides every node of every utterance of every case by at least 1e-3 and that
float32 walks the same path.  lm rows, score and lm_score are held to max(2e-5, 8 x what float32 costs
the restatement itself), figures recorded in the cases file.  The searches are fed `am` directly (the
joiner's enc_proj replaced by the identity); the validation test runs the real enc_proj.
"""
import copy
import math

import pytest
import torch

import rnnt_lstm_search_f64 as S
import rnnt_stateless_lm_cases as SC
import rnnt_stateless_lm_f64 as SF
from decode_support import _decoder, _lm_module, _stateless_build, _stateless_modules, _Tok
from task_support import _pcm_batch, _pruned_cfg, _refs, _task, _V

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(dev, name):
    """(case, predictor, joiner, LM, am and lengths on the device, the float64 results), once per case."""
    if name not in _CACHE:
        c = SC.CASES[name]
        p, am, lens, sd = SC.make(name)
        pred, join = _stateless_modules(dev, p, c)
        _CACHE[name] = (c, pred, join, _lm_module(dev, sd), am.to(dev), lens.to(dev), SC.reference(name))
    return _CACHE[name]


def _fused(c, p, j, lm, am, lens, **kw):
    from speech2text_amd.model.decoding import rnnt_beam_stateless_lm_tokens_from_am
    args = dict(lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"], lm_start_token=c["start"])
    args.update(kw)
    return rnnt_beam_stateless_lm_tokens_from_am(am, lens, p, j, lm, **args)


def _six_product_gemms():
    """The modules' own GEMMs in fp32 arithmetic for a module-loop run (restored by the caller)."""
    from speech2text_amd import _native as N
    assert N.lib().s2t_gemm_arith_set(3) == 0
    return N.lib()


# ------------------------------------------------------------------ 1. the predictor step alone
@pytest.mark.parametrize("name", SC.STEP_CASES)
def test_pred_step_chain(dev, name):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnnt_stateless_desc
    c, R = SC.CASES[name], SC.STEP_ROWS
    pred, join = _stateless_modules(dev, SC.make(name, 100)[0], c)
    desc, keep = rnnt_stateless_desc(pred, join)
    nbytes = N.lib().s2t_stateless_pred_step_workspace_bytes(desc, R)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    new = lambda: [torch.zeros(R, c["ctx"], dtype=torch.int32, device=dev), torch.zeros(R, c["V"], device=dev)]  # noqa: E731
    cur, ref = new(), SC.step_chain(name, torch.float64)
    limit = SC.bound(SC.STEP_COST[name])
    for i, (tokens, emit, parent) in enumerate(SC.step_schedule(name)):
        ident = torch.equal(parent, torch.arange(R))
        before = [t.clone() for t in cur]
        out = cur if ident else new()                      # in place without a gather, else disjoint
        dt, de, dp = (x.to(device=dev, dtype=torch.int32) for x in (tokens, emit, parent))
        rc = N.lib().s2t_stateless_pred_step(desc, R, N.ip(dt), N.ip(de), None if ident else N.ip(dp),
                                             N.ip(cur[0]), N.fp(cur[1]), N.ip(out[0]), N.fp(out[1]), N.ptr(ws),
                                             N.stream())
        assert rc == 0
        for r in (emit == 0).nonzero().flatten().tolist():  # masked: the parent's row, bit for bit
            q = int(parent[r])
            assert torch.equal(out[0][r], before[0][q]) and torch.equal(out[1][r], before[1][q])
        cur = out
        assert torch.equal(cur[0].cpu().long(), ref[i][0]), (name, i)          # contexts: exact
        if i in (0, 4):
            err = SC.rel_err(cur[1], ref[i][1])
            print(f"{name} after step {i + 1}: lm rel_err {err:.2e} bound {limit:.2e}")
            assert err <= limit, (name, i, err, limit)
    bad = torch.zeros(R, dtype=torch.int32, device=dev)   # same buffers with a gather: refused
    assert N.lib().s2t_stateless_pred_step(desc, R, N.ip(dt), N.ip(de), N.ip(bad), N.ip(cur[0]), N.fp(cur[1]),
                                           N.ip(cur[0]), N.fp(cur[1]), N.ptr(ws), N.stream()) == -1


# ------------------------------------------------------------------ 2. the fused search
@pytest.mark.parametrize("name", list(SC.CASES))
def test_fused_search_exact(dev, name):
    c, p, j, lm, am, lens, ref = _case(dev, name)
    B, T = am.shape[0], am.shape[1]
    dec = _decoder(c, p, j, lm)
    assert not dec._lstm_search() and dec._fusable() == (c["inner"] == 0)
    want = (torch.tensor([r[1] for r in ref], dtype=torch.float64),
            torch.tensor([r[2] for r in ref], dtype=torch.float64))
    limit = SC.bound(SC.FUSED_COST[name])
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
        errs = SC.rel_err(score, want[0]), SC.rel_err(lm_score, want[1])
        print(f"{name} {how}: score rel_err {errs[0]:.2e} lm_score rel_err {errs[1]:.2e} bound {limit:.2e}")
        assert max(errs) <= limit, (name, how, errs, limit)
        if B > 1:                                          # no frames: no tokens, score 0, lm_score 0
            assert float(score[1]) == 0.0 and float(lm_score[1]) == 0.0 and int(out_len[1]) == 0
    n0 = SC.clamp(lens[0], T)
    assert dec.decode(am[0:1, :n0]) == _Tok().decode(ref[0][0])        # one utterance: the same kernels, B = 1
    # the module loop on the device over the same modules (fp32, six-product GEMMs): the same tokens
    nl = min(B, 3)
    assert dec.decode_batch(am[:nl], lens[:nl]) == [_Tok().decode(r[0]) for r in ref[:nl]]
    lib = _six_product_gemms()
    try:
        tokens, frames, out_len, _, _ = (x.cpu() for x in dec.beam_tokens(am[:nl], lens[:nl], fused=False))
    finally:
        lib.s2t_gemm_arith_set(0)
    for b, (tok, _, _, frm, _) in enumerate(ref[:nl]):
        assert tokens[b, :int(out_len[b])].tolist() == tok and frames[b, :int(out_len[b])].tolist() == frm, (name, b)


# ------------------------------------------------------------------ 3. lm_score is the module's own score
@pytest.mark.parametrize("name", ["s_b17_ctx5_e65", "s_v128_e130_beam16_start", SC.YAML])
def test_lm_score_is_rnn_lm_score_of_the_tokens(dev, name):
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
    lib = _six_product_gemms()
    try:
        got = lm.score(seqs.to(dev), lens2.to(dev)).cpu()
    finally:
        lib.s2t_gemm_arith_set(0)
    for b in range(B):
        if len(pre) + n[b] < 2:
            got[b] = 0.0
    err, limit = SC.rel_err(lm_score, got), SC.bound(SC.FUSED_COST[name])
    print(f"{name}: lm_score against RnnLm.score rel_err {err:.2e} bound {limit:.2e}")
    assert float(got.abs().max()) > 0 and err <= limit, (name, err, limit)


# ------------------------------------------------------------------ 4. score = path score + lm_weight x lm_score
@pytest.mark.parametrize("name", ["s_b33_ctx2_v65", "s_inner_v65", SC.YAML])
def test_score_is_the_path_score_plus_the_weighted_lm_score(dev, name):
    c, p, j, lm, am, lens, ref = _case(dev, name)
    tokens, frames, out_len, score, lm_score = (x.cpu() for x in _fused(c, p, j, lm, am, lens))
    w = SF.cast(SC.make(name)[0], torch.float64)
    a, T = am.cpu(), am.shape[1]
    want = []
    for b in range(a.shape[0]):
        n = int(out_len[b])
        path = SF.path_score(a[b, :SC.clamp(lens[b], T)], w, c["ctx"], c["act"], tokens[b, :n].tolist(),
                             frames[b, :n].tolist())
        want.append(path + c["weight"] * float(lm_score[b]))
    err, limit = SC.rel_err(score, torch.tensor(want, dtype=torch.float64)), SC.bound(SC.FUSED_COST[name])
    print(f"{name}: score against float64 path score + weight x lm_score rel_err {err:.2e} bound {limit:.2e}")
    assert float(lm_score.abs().max()) > 0 and err <= limit, (name, err, limit)


# ------------------------------------------------------------------ 5. lm_weight 0
@pytest.mark.parametrize("name", [SC.B33, "s_b17_ctx5_e65"])
def test_weight_zero_walks_the_one_workgroup_search(dev, name):
    """lm_weight 0, no out-projection: tokens, frames and out_len of s2t_rnnt_beam_stateless (decided by
    1e-3 in float64 too), score within the bound of it -- not bit for bit: that kernel orders the
    predictor's sums differently."""
    from speech2text_amd.model.decoding import rnnt_beam_tokens_from_am
    c, p, j, lm, am, lens, _ = _case(dev, name)
    plain_ref = SC.unfused(name)
    assert c["inner"] == 0 and min(r[4] for r in plain_ref) >= S.MARGIN
    plain = rnnt_beam_tokens_from_am(am, lens, p, j, c["beam"], c["topk"])
    assert plain is not None and int(plain[2].sum()) > 0
    for b, r in enumerate(plain_ref):
        assert plain[0][b, :int(plain[2][b])].tolist() == r[0], b
    limit = SC.bound(SC.FUSED_COST[name])
    for start in (None, am.shape[2] - 1):
        out = _fused(c, p, j, lm, am, lens, lm_weight=0.0, lm_start_token=start)
        for x, y in zip(out[:3], plain[:3]):
            assert torch.equal(x, y), start
        err = SC.rel_err(out[3], plain[3])
        print(f"{name} start {start}: score against the one-workgroup kernel rel_err {err:.2e} bound {limit:.2e}")
        assert err <= limit
        assert bool(torch.isfinite(out[4]).all()) and float(out[4].abs().max()) > 0
    fused = _fused(c, p, j, lm, am, lens)
    assert not torch.equal(fused[0], plain[0])             # and the LM term is not inert


# ------------------------------------------------------------------ 6. batch invariance
def test_batch_invariance(dev):
    """Utterance b alone, inside the first 17 and inside all 33: bit-identical, all five outputs."""
    c, p, j, lm, am, lens, _ = _case(dev, SC.B33)
    assert am.shape[0] == 33
    runs = {n: _fused(c, p, j, lm, am[:n], lens[:n]) for n in (17, 33)}
    for b in (0, 2, 7, 15, 16):
        alone = _fused(c, p, j, lm, am[b:b + 1], lens[b:b + 1])
        assert len(alone) == 5
        for n, out in runs.items():
            for x, y in zip(alone, out):
                assert torch.equal(x[0], y[b]), (b, n)
    for x, y in zip(runs[17], runs[33]):
        assert torch.equal(x, y[:17])
    assert int(runs[33][2].sum()) > 0


# ------------------------------------------------------------------ 7. limits
def _tiny_run(dev, p, j, lm, V, beam=4, topk=4, **kw):
    from speech2text_amd.model.decoding import rnnt_beam_stateless_lm_tokens_from_am
    g = torch.Generator().manual_seed(3)
    am = torch.randn(1, 2, V, generator=g).to(dev)
    lens = torch.tensor([2], device=dev)
    return am, lens, rnnt_beam_stateless_lm_tokens_from_am(am, lens, p, j, lm, 0.3, beam, topk, **kw)


@pytest.mark.parametrize("shape", [dict(V=11, E=1024, D=20, ctx=64), dict(V=11, E=1, D=1, ctx=1),
                                   dict(V=8192, E=12, D=24, ctx=2), dict(V=11, E=12, D=20, ctx=2, inner=40),
                                   dict(V=11, E=12, D=20, ctx=2, beam=16, topk=16)], ids=str)
def test_limits_just_inside_are_taken(dev, shape):
    shape = dict(shape)
    beam, topk = shape.pop("beam", 4), shape.pop("topk", 4)
    torch.manual_seed(5)
    p, j = _stateless_build(dev, **shape)
    lm = _lm_module(dev, V=shape["V"], H=8, layers=1)
    for start in (None, shape["V"] - 1):
        _, _, out = _tiny_run(dev, p, j, lm, shape["V"], beam, topk, lm_start_token=start)
        assert out is not None and 0 <= int(out[2][0]) <= 2
        assert bool(torch.isfinite(out[3]).all()) and bool(torch.isfinite(out[4]).all())


@pytest.mark.parametrize("shape", [dict(V=11, E=1028, D=20, ctx=2), dict(V=11, E=12, D=20, ctx=65),
                                   dict(V=11, E=12, D=20, ctx=2, beam=17), dict(V=11, E=12, D=20, ctx=2, lm_V=12),
                                   dict(V=11, E=12, D=20, ctx=2, weight=math.inf)], ids=str)
def test_limits_just_outside_take_the_module_loop(dev, shape):
    """The wrapper returns None (rc -1 or size 0, before any launch) and the class answers with
    _module_loop_lm's tokens."""
    from speech2text_amd.model.decoding import RnntBeamDecoding, rnnt_beam_stateless_lm_tokens_from_am
    shape = dict(shape)
    beam, lm_V, weight = shape.pop("beam", 2), shape.pop("lm_V", shape["V"]), shape.pop("weight", 0.3)
    torch.manual_seed(5)
    p, j = _stateless_build(dev, **shape)
    lm = _lm_module(dev, V=lm_V, H=8, layers=1)
    g = torch.Generator().manual_seed(3)
    am = torch.randn(1, 2, shape["V"], generator=g).to(dev)
    lens = torch.tensor([2], device=dev)
    assert rnnt_beam_stateless_lm_tokens_from_am(am, lens, p, j, lm, weight, beam, 2) is None
    if lm_V != shape["V"] or not math.isfinite(weight) or shape["ctx"] > 64:
        return                                             # (no search is defined for these; ctx 65: the refusal alone)
    dec = RnntBeamDecoding(_Tok(), p, j, beam_size=beam, cutoff_top_k=2, lm=lm, lm_weight=weight)
    with torch.no_grad():
        tok, frm, score, lm_score = dec._module_loop_lm(am)
    got = dec.beam_tokens(am, lens)
    assert len(got) == 5 and got[0].is_cuda
    assert got[0][0, :int(got[2][0])].tolist() == tok and got[1][0, :int(got[2][0])].tolist() == frm
    assert float(got[3][0]) == pytest.approx(score) and float(got[4][0]) == pytest.approx(lm_score)
    assert dec.decode_batch(am, lens) == [_Tok().decode(tok)]


def test_a_foreign_lm_takes_the_module_loop(dev):
    """An LM that is not an RnnLm (init_states / score_step only): the class does not try the kernels."""
    c, p, j, lm, am, lens, ref = _case(dev, "s_v11_beam16_kV")

    class Wrapped:
        def init_states(self, n):
            return lm.init_states(n)

        def score_step(self, tokens, states):
            return lm.score_step(tokens, states)

    dec = _decoder(c, p, j, Wrapped())
    lib = _six_product_gemms()
    try:
        out = dec.beam_tokens(am, lens)
    finally:
        lib.s2t_gemm_arith_set(0)
    for b, r in enumerate(ref):
        assert out[0][b, :int(out[2][b])].tolist() == r[0], b


# ------------------------------------------------------------------ 8. validation_step
def test_validation_step_logs_the_restatements_wer(dev):
    from oracle import decoding as OD
    cfg = copy.deepcopy(_pruned_cfg())
    cfg["metric"] = {"decode_method": "rnnt_beam_search", "beam_size": 3, "cutoff_top_k": 3, "lm_weight": 0.5,
                     "lm": {"config": {"num_symbols": _V, "symbol_embedding_dim": 24, "num_rnn_layer": 2},
                            "checkpoint": None}}
    batch = _pcm_batch(dev, B=2, sec=1.0, V=_V)
    task = _task("Pruned_Rnnt", cfg, dev)
    keys = list(task.state_dict())
    sess = task._metric._decode_sess
    with torch.no_grad():                                  # away from the near-ties of fresh models
        for q in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            q.mul_(4.0)
        sess._lm._logits_layer.weight.mul_(32.0)
        for k in range(2):
            getattr(sess._lm._rnn_layer, f"weight_ih_l{k}").mul_(3.0)
    assert sess._fusable() and not sess._lstm_search() and sess._lm is not None
    assert (sess._lm_weight, sess._beam_size, sess._cutoff_top_k) == (0.5, 3, 3)
    assert next(sess._lm.parameters()).device.type == "cpu"            # the task's .to() does not own it
    info = task.validation_step(batch, 0)
    assert "wer" in task.logged and next(sess._lm.parameters()).device.type == "cuda"
    assert list(task.state_dict()) == keys and not any("_lm" in k or "nnlm" in k for k in keys)
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
    q, jn = task._predictor.predictor, task._joiner
    f64 = lambda t: t.detach().double().cpu()              # noqa: E731
    ctx = q._context_size
    w = dict(emb=f64(q._embedding.weight), conv_w=f64(q._conv.weight).reshape(-1, ctx), lin_w=f64(q._output_linear.weight),
             lin_b=f64(q._output_linear.bias), pre_w=f64(jn._pre_proj.weight), pre_b=f64(jn._pre_proj.bias))
    assert not jn._use_out_project
    sd = {k: f64(v) for k, v in sess._lm.state_dict().items()}
    hyps, plain, margins = [], [], []
    for b in range(enc.shape[0]):
        with torch.no_grad():
            am = f64(jn._enc_proj(enc[b:b + 1, :int(el[b])])[0])
        ids, _, _, _, margin = SF.beam_search_lm(am, w, ctx, jn._act_name, 3, 3, sd, 0.5)
        plain.append(SF.beam_search_lm(am, w, ctx, jn._act_name, 3, 3, sd, 0.0)[0])
        margins.append(margin)
        hyps.append(task._tokenizer.decode(torch.tensor(ids, dtype=torch.int64)))
    print(f"hypotheses {hyps}, lm_weight 0 token ids {plain}, smallest float64 margins {margins}")
    plain = [task._tokenizer.decode(torch.tensor(ids, dtype=torch.int64)) for ids in plain]
    assert min(margins) >= S.MARGIN
    assert hyps != plain, "the LM changes no hypothesis: a search that dropped its term would pass"
    assert info["wer"] == pytest.approx(OD.word_error_rate(hyps, _refs(task, batch["label"])))
