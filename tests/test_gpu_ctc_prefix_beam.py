"""GPU: the CTC prefix beam search on the device (csrc/decode_ctc.hip: s2t_ctc_prefix_beam in one launch,
s2t_ctc_prefix_beam_lm in lockstep rounds with s2t_rnn_lm_step) against the float64 restatement
tests/ctc_prefix_f64.py on the cases of tests/ctc_prefix_cases.py, whose conditions (every decision made by
at least 1e-3 in float64, merges, re-entries, the LM changes a hypothesis) tests/test_ctc_prefix_f64.py
asserts on the CPU.  Tokens and out_len must be equal; score and lm_score are bounded by max(2e-5, 8 x
what float32 costs the restatement), relative to the largest reference value of the case.  Frames at
and beyond an utterance's length are NaN in every case: a search that read one would not return the
reference's tokens.
"""
import copy
import math

import pytest
import torch

import ctc_prefix_cases as C
import ctc_prefix_f64 as P
import rnnt_lm_fusion_cases as L
from decode_support import _lm_module
from task_support import _ctc_cfg, _pcm_batch, _refs, _task
from yardstick import _Ids

pytestmark = pytest.mark.gpu


_CACHE = {}


def _case(dev, name):
    """(case, logits and lengths on the device, the LM module or None), once per case."""
    if name not in _CACHE:
        x, lens, sd = C.make(name)
        _CACHE[name] = (C.CASES[name], x.to(dev), lens.to(dev), _lm_module(dev, sd) if sd is not None else None)
    return _CACHE[name]


def _plain(c, x, lens, **kw):
    from speech2text_amd.model.decoding import ctc_prefix_beam_tokens
    args = dict(beam_size=c["beam"], cutoff_top_k=c["topk"])
    args.update(kw)
    return ctc_prefix_beam_tokens(x, lens, **args)


def _fused(c, x, lens, lm, **kw):
    from speech2text_amd.model.decoding import ctc_prefix_beam_lm_tokens
    args = dict(lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"], lm_start_token=c["start"])
    args.update(kw)
    return ctc_prefix_beam_lm_tokens(x, lens, lm, **args)


def _check(name, out, ref, lm):
    tokens, out_len, score = (t.cpu() for t in out[:3])
    for b, r in enumerate(ref):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == r.tokens, (name, b)
        assert int(tokens[b, n:].sum()) == 0
        if not r.tokens and r.score == 0.0:                # no frames: no tokens, score 0, lm_score 0
            assert float(score[b]) == 0.0 and (not lm or float(out[3][b]) == 0.0)
    f64 = lambda i: torch.tensor([r[i] for r in ref], dtype=torch.float64)    # noqa: E731
    err = C.rel_err(score, f64(1))
    print(f"{name}: score rel_err {err:.3e} (bound {C.bound(name):.1e})")
    assert err <= C.bound(name), (name, err)
    if lm:
        err = C.rel_err(out[3].cpu(), f64(2))
        print(f"{name}: lm_score rel_err {err:.3e} (bound {C.bound(name):.1e})")
        assert err <= C.bound(name), (name, err)


# ------------------------------------------------------------------ 1. every case, both entries
@pytest.mark.parametrize("name", list(C.CASES))
def test_plain_entry_against_the_float64_restatement(dev, name):
    c, x, lens, lm = _case(dev, name)
    out = _plain(c, x, lens)
    assert out is not None and len(out) == 3
    _check(name, out, C.reference(name) if lm is None else C.unfused(name), False)


@pytest.mark.parametrize("name", C.LM_CASES)
def test_lm_entry_against_the_float64_restatement(dev, name):
    c, x, lens, lm = _case(dev, name)
    out = _fused(c, x, lens, lm)
    assert out is not None and len(out) == 4
    _check(name, out, C.reference(name), True)
    if name in C.LM_CHANGES:
        plain = _plain(c, x, lens)
        assert not torch.equal(out[0], plain[0]), "the LM changes no hypothesis"


@pytest.mark.parametrize("name", C.PLAIN_CASES)
def test_lm_entry_at_weight_zero_is_the_plain_entry_bit_for_bit(dev, name):
    c, x, lens, _ = _case(dev, name)
    V = c["V"]
    model = {3: None, 5: None, 6: None, 300: None, 11: "lm20_v11", 63: "lm20", 65: "lm48", 128: "lm64"}[V]
    lm = _lm_module(dev, L.lm_weights(model, 3)) if model else _lm_module(dev, V=V, H=8, layers=2)
    plain = _plain(c, x, lens)
    for start in (None, V - 1):
        out = _fused(c, x, lens, lm, lm_weight=0.0, lm_start_token=start)
        assert out is not None
        for a, b in zip(plain, out[:3]):
            assert torch.equal(a, b), (name, start)
        assert bool(torch.isfinite(out[3]).all())


@pytest.mark.parametrize("name", C.LM_CASES)
def test_lm_entry_at_weight_zero_on_the_lm_cases(dev, name):
    c, x, lens, lm = _case(dev, name)
    plain, out = _plain(c, x, lens), _fused(c, x, lens, lm, lm_weight=0.0)
    for a, b in zip(plain, out[:3]):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ 2. the exhaustive cases, greedy
@pytest.mark.parametrize("T,V,n", C.BRUTE)
def test_exhaustive_cases_through_the_kernel(dev, T, V, n):
    x = C.brute_logits(T, V, n).to(dev)
    lens = torch.full((n,), T, device=dev)
    tokens, out_len, score = (t.cpu() for t in _plain(dict(beam=16, topk=V), x, lens))
    ref = C.brute_reference(T, V, n)
    for i, (labels, logp, _) in enumerate(ref):
        assert tokens[i, :int(out_len[i])].tolist() == labels, (T, V, i)
    err = C.rel_err(score, torch.tensor([r[1] for r in ref], dtype=torch.float64))
    print(f"exhaustive T {T} V {V}: score rel_err {err:.3e}")
    assert err <= C.FLOOR


@pytest.mark.parametrize("name", list(C.CASES))
def test_beam1_top1_is_ctc_greedy(dev, name):
    from speech2text_amd.model.decoding import ctc_greedy_tokens
    c, x, lens, _ = _case(dev, name)
    x = torch.nan_to_num(x, nan=0.0)                       # (s2t_ctc_greedy is not what is tested for padding)
    tokens, out_len, _ = _plain(c, x, lens, beam_size=1, cutoff_top_k=1)
    gt, gl = ctc_greedy_tokens(x, lens)
    assert torch.equal(out_len, gl)
    for b in range(x.shape[0]):
        n = int(gl[b])
        assert torch.equal(tokens[b, :n], gt[b, :n]), (name, b)


def test_batch_invariance(dev):
    """Utterance b alone and inside the batch of 17: bit-identical, both entries."""
    name = "l_v65_lm48_b17_beam4_k3"
    c, x, lens, lm = _case(dev, name)
    whole_p, whole_l = _plain(c, x, lens), _fused(c, x, lens, lm)
    for b in (0, 1, 2, 16):
        for whole, alone in ((whole_p, _plain(c, x[b:b + 1], lens[b:b + 1])),
                             (whole_l, _fused(c, x[b:b + 1], lens[b:b + 1], lm))):
            for a, w in zip(alone, whole):
                assert torch.equal(a[0], w[b]), b


# ------------------------------------------------------------------ 3. limits
_V = 32


@pytest.mark.parametrize("change", [dict(beam=17), dict(beam=0), dict(topk=0), dict(topk=17), dict(V=8193),
                                    dict(blank=-1), dict(blank=_V), dict(ws=None), dict(H=1028), dict(H=22),
                                    dict(H=0), dict(E=1025), dict(num_layers=9), dict(num_layers=0), dict(lmV=_V + 1),
                                    dict(start=_V), dict(weight=math.inf), dict(weight=math.nan), dict(lm=None)],
                         ids=str)
def test_limits_just_outside_return_minus_one(dev, change):
    """Outside the limits both entries answer -1 (the workspace size 0) before any launch: no pointer is
    followed (logits, workspace and outputs are far too small for V 8193) and the poisoned outputs keep
    their poison."""
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnn_lm_desc
    lib = N.lib()
    lm = _lm_module(dev, V=_V, H=8, layers=1)
    lm_desc, lm_keep = rnn_lm_desc(lm)
    assert lib.s2t_ctc_prefix_beam_workspace_bytes(1, 2, _V, 4) > 0
    assert lib.s2t_ctc_prefix_beam_lm_workspace_bytes(lm_desc, 1, 2, _V, 4) > 0
    lm_only = {"H", "E", "num_layers", "lmV", "start", "weight", "lm"}
    for k in ("H", "E", "num_layers"):
        if k in change:
            setattr(lm_keep[-1], k, change[k])
    if "lmV" in change:
        lm_keep[-1].V = change["lmV"]
    beam, topk, V, blank = change.get("beam", 4), change.get("topk", 4), change.get("V", _V), change.get("blank", 0)
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    wsp = None if "ws" in change else N.ptr(ws)
    x, lens = torch.zeros(1, 2, _V, device=dev), torch.tensor([2], device=dev)
    tokens = torch.full((1, 2), 7, dtype=torch.int64, device=dev)
    out_len = torch.full((1,), 7, dtype=torch.int64, device=dev)
    score, lm_score = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    if {"beam", "V"} & set(change):
        assert lib.s2t_ctc_prefix_beam_workspace_bytes(1, 2, V, beam) == 0
    if {"beam", "V", "H", "E", "num_layers", "lmV"} & set(change):
        assert lib.s2t_ctc_prefix_beam_lm_workspace_bytes(lm_desc, 1, 2, V, beam) == 0
    if "lm" in change:
        assert lib.s2t_ctc_prefix_beam_lm_workspace_bytes(None, 1, 2, V, beam) == 0
    if not lm_only & set(change):
        assert lib.s2t_ctc_prefix_beam(N.fp(x), N.lp(lens), 1, 2, V, blank, beam, topk, wsp, N.lp(tokens),
                                       N.lp(out_len), N.fp(score), N.stream()) == -1
    assert lib.s2t_ctc_prefix_beam_lm(None if "lm" in change else lm_desc, N.fp(x), N.lp(lens), 1, 2, V, blank, beam,
                                      topk, change.get("weight", 0.3), change.get("start", -1), wsp, N.lp(tokens),
                                      N.lp(out_len), N.fp(score), N.fp(lm_score), N.stream()) == -1
    torch.cuda.synchronize()
    assert tokens.tolist() == [[7, 7]] and int(out_len[0]) == 7
    assert float(score[0]) == 7.0 and float(lm_score[0]) == 7.0


def test_empty_batch_returns_zero_and_limits_just_inside_are_taken(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import rnn_lm_desc
    lib = N.lib()
    lm_desc, lm_keep = rnn_lm_desc(_lm_module(dev, V=_V, H=8, layers=1))
    assert lib.s2t_ctc_prefix_beam(None, None, 0, 2, _V, 0, 99, 99, None, None, None, None, N.stream()) == 0
    assert lib.s2t_ctc_prefix_beam_lm(lm_desc, None, None, 0, 2, _V, 0, 99, 99, 0.3, -1, None, None, None, None, None,
                                      N.stream()) == 0
    g = torch.Generator().manual_seed(5)
    x, lens = torch.randn(2, 3, _V, generator=g).to(dev), torch.tensor([3, 2], device=dev)
    for beam, topk in ((16, 16), (1, 16), (16, 1)):
        out = _plain(dict(beam=beam, topk=topk), x, lens)
        assert out is not None and bool((out[1] <= 3).all()) and bool(torch.isfinite(out[2]).all())
    for H, layers in ((1024, 1), (8, 8)):
        lm = _lm_module(dev, V=_V, H=H, layers=layers)
        for start in (None, _V - 1):
            out = _fused(dict(beam=16, topk=16, weight=0.3, start=start), x, lens, lm)
            assert out is not None and bool(torch.isfinite(out[2]).all()) and bool(torch.isfinite(out[3]).all())
    small = torch.randn(1, 2, 8, generator=g).to(dev)      # cutoff_top_k above 16 is fine where V is not
    assert _plain(dict(beam=4, topk=99), small, torch.tensor([2], device=dev)) is not None


# ------------------------------------------------------------------ 4. the class
@pytest.mark.parametrize("name", ["p_v6_reenter", "p_v65_b33_beam4_k3_norm", "l_v63_lm20_beam4",
                                  "l_v11_lm20_beam1_k1"])
def test_class_fused_path_is_the_module_loop(dev, name):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding
    c, x, lens, lm = _case(dev, name)
    dec = CtcPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"],
                                lm_start_token=c["start"])
    fused = dec.beam_tokens(x, lens)
    assert N.lib().s2t_gemm_arith_set(3) == 0              # the module's products at fp32 level
    try:
        loop = dec.beam_tokens(x, lens, fused=False)
    finally:
        N.lib().s2t_gemm_arith_set(0)
    assert len(fused) == len(loop) == (4 if lm is not None else 3) and fused[0].is_cuda and loop[0].is_cuda
    assert torch.equal(fused[0], loop[0]) and torch.equal(fused[1], loop[1])
    for a, b in zip(fused[2:], loop[2:]):
        assert C.rel_err(a, b) <= 1e-4
    ref = C.reference(name)
    assert dec.decode_batch(x, lens) == [r.tokens for r in ref]
    assert dec.decode(x[:1, :C.clamp(lens[0], c["T"])]) == ref[0].tokens


def test_refused_shapes_and_foreign_lms_take_the_module_loop(dev):
    import rnnt_lm_fusion_f64 as F
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding
    name = "l_v63_lm20_beam4"
    c, x, lens, lm = _case(dev, name)
    assert _plain(c, x, lens, beam_size=17) is None and _fused(c, x, lens, lm, beam_size=17) is None
    ref = C.reference(name)
    sd = {k: v.to(dev) for k, v in L.cast(C.make(name)[2], torch.float64).items()}
    dec = CtcPrefixBeamDecoding(_Ids(), beam_size=c["beam"], cutoff_top_k=c["topk"], lm=F.PlainLm(sd),
                                lm_weight=c["weight"])
    assert dec._fused(x, lens) is None
    out = dec.beam_tokens(x.double(), lens)
    assert out[0].is_cuda and len(out) == 4
    for b, r in enumerate(ref):
        assert out[0][b, :int(out[1][b])].tolist() == r.tokens


# ------------------------------------------------------------------ 5. validation_step


def test_validation_step_logs_the_restatements_wer(dev, golden_dir):
    from oracle import decoding as OD
    cfg, V = _ctc_cfg(golden_dir)
    cfg = copy.deepcopy(cfg)
    cfg["metric"] = {"decode_method": "ctc_prefix_beam_search", "beam_size": 3, "cutoff_top_k": 3, "lm_weight": 0.5,
                     "lm": {"config": {"num_symbols": V, "symbol_embedding_dim": 24, "num_rnn_layer": 2},
                            "checkpoint": None}}
    batch = _pcm_batch(dev, B=2, sec=1.0, V=V)
    task = _task("CTC", cfg, dev)
    keys = list(task.state_dict())
    sess = task._metric._decode_sess
    from speech2text_amd.model.decoding import CtcPrefixBeamDecoding
    from speech2text_amd.model.lm.rnn_lm import RnnLm
    assert isinstance(sess, CtcPrefixBeamDecoding) and isinstance(sess._lm, RnnLm)
    assert (sess._lm_weight, sess._beam_size, sess._cutoff_top_k) == (0.5, 3, 3)
    with torch.no_grad():                                  # away from the near-ties of fresh models
        for q in task._decoder.parameters():
            q.mul_(6.0)
        sess._lm._logits_layer.weight.mul_(16.0)
        for k in range(2):
            getattr(sess._lm._rnn_layer, f"weight_ih_l{k}").mul_(3.0)
    assert next(sess._lm.parameters()).device.type == "cpu"            # the task's .to() does not own it
    info = task.validation_step(batch, 0)
    assert "wer" in task.logged and next(sess._lm.parameters()).device.type == "cuda"
    assert list(task.state_dict()) == keys
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
        dec, dl = task._decoder(enc, el)
        lp = torch.log_softmax(dec, dim=-1)
    sd = {k: v.detach().double().cpu() for k, v in sess._lm.state_dict().items()}
    hyps, plain, margins = [], [], []
    for b in range(lp.shape[0]):
        row = lp[b, :int(dl[b])].double().cpu()
        r = P.prefix_beam_search(row, 3, 3, 0, sd, 0.5)
        plain.append(P.prefix_beam_search(row, 3, 3).tokens)
        margins.append(r.margin)
        hyps.append(task._tokenizer.decode(torch.tensor(r.tokens, dtype=torch.int64)))
    print(f"hypotheses {hyps}, un-fused token ids {plain}, smallest float64 margins {margins}")
    plain = [task._tokenizer.decode(torch.tensor(ids, dtype=torch.int64)) for ids in plain]
    assert hyps != plain, "the LM changes no hypothesis: a search that dropped its term would pass"
    assert info["wer"] == pytest.approx(OD.word_error_rate(hyps, _refs(task, batch["label"])))
