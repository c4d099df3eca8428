"""GPU: the one-launch RNN-T beam search of the stateless predictor fused with a back-off n-gram
(csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_ngram; the frame body is csrc/decode_search.h beam_walk's
n-gram mode, the look-up csrc/ngram_lookup.h) against the float64 restatement of tests/rnnt_ngram_f64.py
on the seeded cases of tests/rnnt_ngram_cases.py.

Tokens, counts and emission frames are compared for exact equality: tests/test_rnnt_ngram_f64.py asserts
that float64 decides every ranking cut of every utterance of every case by at least 1e-3 and that
float32 walks the same path.  score and lm_score are held to max(2e-5, 8 x what float32 costs the
restatement itself), figures recorded in the cases file.  The searches are fed `am` directly (the
joiner's enc_proj replaced by the identity); the task test runs the real enc_proj.
"""
import copy
import math

import numpy as np
import pytest
import torch

import rnnt_ngram_cases as C
import rnnt_ngram_f64 as R
from decode_support import _bad_desc, _fused, _ngram_case
from task_support import _pcm_batch, _pruned_cfg, _task, _V

pytestmark = pytest.mark.gpu


def _column(rows, i):
    return torch.tensor([r[i] for r in rows], dtype=torch.float64)


def _same_path(out, ref, what, zeroed=True):
    tokens, frames, out_len = (x.cpu() for x in out[:3])
    for b, r in enumerate(ref):
        n = len(r.tokens)
        assert int(out_len[b]) == n, (what, b, int(out_len[b]), n)
        assert tokens[b, :n].tolist() == r.tokens and frames[b, :n].tolist() == r.frames, (what, b)
        assert not zeroed or ((tokens[b, n:] == 0).all() and (frames[b, n:] == 0).all())


# ------------------------------------------------------------------ 1. the fused search
@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_search_exact(dev, name):
    c, p, j, lm, am, lens, ref = _ngram_case(dev, name)
    out = _fused(c, p, j, lm, am, lens)
    assert out is not None and len(out) == 5
    assert out[0].shape == out[1].shape == am.shape[:2] and out[0].dtype == torch.int64
    assert out[3].dtype == out[4].dtype == torch.float32
    _same_path(out, ref, name)
    _same_path(out, C.reference32(name), name + " float32 restatement")
    errs = C.rel_err(out[3], _column(ref, 1)), C.rel_err(out[4], _column(ref, 2))
    limit = C.bound(name)
    print(f"{name}: score rel_err {errs[0]:.2e} lm_score rel_err {errs[1]:.2e} bound {limit:.2e}")
    assert max(errs) <= limit, (name, errs, limit)
    if am.shape[0] > 1:                                    # no frames: no tokens, score 0, lm_score 0
        assert float(out[3][1]) == 0.0 and float(out[4][1]) == 0.0 and int(out[2][1]) == 0
    if c["beam"] > 1:                                      # and the LM term is not inert
        plain = _fused(c, p, j, lm, am, lens, lm_weight=0.0)
        assert not torch.equal(plain[0], out[0])


# ------------------------------------------------------------------ 2. lm_weight 0 is the plain kernel, bit for bit
@pytest.mark.parametrize("name", list(C.CASES))
def test_weight_zero_is_the_plain_entry(dev, name):
    from speech2text_amd.model.decoding import rnnt_beam_tokens_from_am
    c, p, j, lm, am, lens, _ = _ngram_case(dev, name)
    plain = rnnt_beam_tokens_from_am(am, lens, p, j, c["beam"], c["topk"])
    out = _fused(c, p, j, lm, am, lens, lm_weight=0.0)
    assert plain is not None and out is not None and int(plain[2].sum()) > 0
    for x, y, what in zip(out[:4], plain, ("tokens", "frames", "out_len", "score")):
        assert torch.equal(x, y), (name, what)
    un = C.unfused(name)
    _same_path(out, un, name)
    err, limit = C.rel_err(out[4], _column(un, 2)), C.bound(name)     # the sum of the path's look-ups
    print(f"{name}: lm_score at weight 0 rel_err {err:.2e} bound {limit:.2e}")
    assert float(out[4].abs().max()) > 0 and err <= limit


# ------------------------------------------------------------------ 3. beam 1 / top-k 1
def test_beam_one_walks_the_plain_path(dev):
    from speech2text_amd.model.decoding import rnnt_beam_tokens_from_am
    name = "g_v63_o1_beam1_k1"
    c, p, j, lm, am, lens, _ = _ngram_case(dev, name)
    assert c["beam"] == c["topk"] == 1
    plain = rnnt_beam_tokens_from_am(am, lens, p, j, 1, 1)
    out = _fused(c, p, j, lm, am, lens)
    for x, y in zip(out[:3], plain[:3]):
        assert torch.equal(x, y)
    want = plain[3].double() + c["weight"] * out[4].double()
    err = C.rel_err(out[3], want)
    print(f"{name}: score against plain score + weight x lm_score rel_err {err:.2e} bound {C.bound(name):.2e}")
    assert float(out[4].abs().max()) > 0 and err <= C.bound(name)


# ------------------------------------------------------------------ 4. refusals
def _abi_arguments(dev, name):
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import _stateless_weights
    c, p, j, lm, am, lens, _ = _ngram_case(dev, name)
    B, T, V = am.shape
    w, E, D, ctx, act = _stateless_weights(p, j)
    need = N.lib().s2t_rnnt_beam_ngram_workspace_bytes(B, T, V, c["beam"])
    assert need == N.lib().s2t_rnnt_beam_workspace_bytes(B, T, V, c["beam"]) > 0
    g = torch.Generator().manual_seed(1)
    ws = torch.randint(0, 255, (need,), dtype=torch.uint8, generator=g).to(dev)
    outs = [torch.full((B, T), 7, dtype=torch.int64, device=dev), torch.full((B, T), 7, dtype=torch.int64, device=dev),
            torch.full((B,), 7, dtype=torch.int64, device=dev), torch.full((B,), 7.0, device=dev),
            torch.full((B,), 7.0, device=dev)]
    args = dict(lm=lm.desc()[0], am=N.fp(am), lengths=N.lp(lens), emb=N.fp(w[0]), conv_w=N.fp(w[1]), lin_w=N.fp(w[2]),
                lin_b=N.fp(w[3]), pre_w=N.fp(w[4]), pre_b=N.fp(w[5]), B=B, T=T, V=V, E=E, D=D, ctx=ctx, act=act, blank=0,
                beam=c["beam"], topk=c["topk"], weight=c["weight"], start=int(lm.start_ctx), ws=N.ptr(ws),
                tokens=N.lp(outs[0]), frames=N.lp(outs[1]), out_len=N.lp(outs[2]), score=N.fp(outs[3]),
                lm_score=N.fp(outs[4]), stream=N.stream())
    return args, ws, outs, (w, lm)


_REFUSED = [dict(lm=None), dict(desc=dict(ctx_begin=None)), dict(desc=dict(arc_next=None)), dict(desc=dict(V=64)),
            dict(desc=dict(order=0)), dict(desc=dict(order=9)), dict(desc=dict(num_ctx=0)), dict(desc=dict(num_arcs=62)),
            dict(start=-1), dict(start="num_ctx"), dict(weight=math.nan), dict(weight=math.inf), dict(lm_score=None),
            dict(ws=None), dict(T=0), dict(V=8193), dict(E=0), dict(ctx=65), dict(act=2), dict(blank=63), dict(beam=0),
            dict(beam=17), dict(topk=0), dict(topk=17), dict(E=2000, D=2000)]


def test_refusals_leave_everything_untouched(dev):
    from speech2text_amd import _native as N
    lib = N.lib()
    args, ws, outs, keep = _abi_arguments(dev, "g_v63_o5_beam16_k16")
    lm = keep[1]
    order = list(args)
    assert lib.s2t_rnnt_beam_stateless_ngram(*[dict(args, B=0)[k] for k in order]) == 0     # nothing to do
    before = [t.clone() for t in [ws] + outs]
    for change in _REFUSED:
        a, held = dict(args), None
        for k, v in change.items():
            if k == "desc":
                a["lm"], held = _bad_desc(lm, **v)
            elif v == "num_ctx":
                a[k] = lm.num_ctx
            else:
                a[k] = v
        assert lib.s2t_rnnt_beam_stateless_ngram(*[a[k] for k in order]) == -1, change
        del held
    torch.cuda.synchronize()
    for x, y in zip([ws] + outs, before):
        assert torch.equal(x, y)
    B, T, V = args["B"], args["T"], args["V"]
    for bad in ((0, T, V, 4), (B, 0, V, 4), (B, T, 0, 4), (B, T, 8193, 4), (B, T, V, 0), (B, T, V, 17)):
        assert lib.s2t_rnnt_beam_ngram_workspace_bytes(*bad) == 0, bad
    assert lib.s2t_rnnt_beam_stateless_ngram(*[args[k] for k in order]) == 0                # and the good call runs
    _same_path(outs, C.reference("g_v63_o5_beam16_k16"), "after the refusals", zeroed=False)   # (the kernel writes the valid part)


def test_wrapper_refuses_tables_on_another_device(dev):
    c, p, j, lm, am, lens, _ = _ngram_case(dev, "g_v11_o2_kV")
    with pytest.raises(RuntimeError, match="NgramLm.to"):
        _fused(c, p, j, C.model("g_v11_o2_kV"), am, lens)
    assert _fused(c, p, j, lm, am, lens, beam_size=17) is None
    assert _fused(c, p, j, lm, am, lens, lm_weight=math.nan) is None


# ------------------------------------------------------------------ 5. RnntBeamDecoding end to end
def _decoder(c, p, j, lm, **kw):
    from speech2text_amd.model.decoding import RnntBeamDecoding
    args = dict(beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"])
    args.update(kw)
    return RnntBeamDecoding(C.Ids(), p, j, **args)


def _counted(monkeypatch):
    """Counts the calls of the fused wrapper the class makes."""
    from speech2text_amd.model import decoding as D
    calls, real = [], D.rnnt_beam_ngram_tokens_from_am

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(D, "rnnt_beam_ngram_tokens_from_am", spy)
    return calls


def test_class_takes_the_fused_entry_with_tables_from_the_cpu(dev, monkeypatch):
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    name = "g_v65_o3_b17"
    c, p, j, _, am, lens, ref = _ngram_case(dev, name)
    lm = NgramLm.from_arpa(C.text_of(name), num_classes=c["V"])
    assert lm.device.type == "cpu"
    calls = _counted(monkeypatch)
    dec = _decoder(c, p, j, lm)
    out = dec.beam_tokens(am, lens)
    assert calls == [True] and lm.device.type == "cuda" and len(out) == 5
    _same_path(out, ref, name)
    assert dec.decode_batch(am[:3], lens[:3]) == [C.Ids().decode(r.tokens) for r in ref[:3]]
    assert dec.decode(am[0:1, :C.clamp(lens[0], am.shape[1])]) == C.Ids().decode(ref[0].tokens)
    # a given lm_start_token is the host loop's business
    calls.clear()
    _decoder(c, p, j, lm, lm_start_token=3).beam_tokens(am[:1], lens[:1])
    assert calls == []


def _loop_reference(name, beam):
    c = C.CASES[name]
    p, am, lens = C.make(name)
    p = {k: v.numpy() for k, v in p.items()}
    return [R.beam_search(am[b, :C.clamp(lens[b], c["T"])].numpy(), p, c["ctx"], c["act"], beam, c["topk"],
                          C.dict_model(name, np.float64), c["weight"]) for b in range(c["B"])]


def test_a_refused_shape_takes_the_module_loop(dev, monkeypatch):
    """beam 17: the entry refuses, the class answers with _module_loop_lm on the device, first token scored."""
    from speech2text_amd import _native as N
    name = "g_v520_o3"
    c, p, j, lm, am, lens, _ = _ngram_case(dev, name)
    want = _loop_reference(name, 17)
    assert min(r.margin for r in want) >= C.MARGIN
    calls = _counted(monkeypatch)
    dec = _decoder(c, p, j, lm, beam_size=17)
    assert N.lib().s2t_gemm_arith_set(3) == 0              # the modules' own GEMMs in fp32 arithmetic
    try:
        out = dec.beam_tokens(am, lens)
    finally:
        N.lib().s2t_gemm_arith_set(0)
    assert calls == [False]
    _same_path(out, want, name)
    assert C.rel_err(out[4], _column(want, 2)) <= C.bound(name) and float(out[4].abs().max()) > 0


def test_an_out_projection_joiner_takes_the_module_loop(dev, monkeypatch):
    name = "g_v11_o2_kV"
    c, _, _, lm, am, lens, _ = _ngram_case(dev, name)
    torch.manual_seed(3)
    p, j = C.build_modules(dev, c["V"], c["E"], c["D"], c["ctx"], c["act"], inner=16)
    calls = _counted(monkeypatch)
    dec = _decoder(c, p, j, lm)
    assert not dec._fusable()
    out = dec.beam_tokens(am[:1], lens[:1])
    tok, frm, score, lm_score = dec._module_loop_lm(am[:1])
    assert calls == [] and len(out) == 5
    n = int(out[2][0])
    assert out[0][0, :n].tolist() == tok and out[1][0, :n].tolist() == frm
    assert float(out[4][0]) == pytest.approx(lm_score)


# ------------------------------------------------------------------ 6. a task from a YAML section
def test_task_with_an_arpa_section_decodes_through_the_fused_entry(dev, tmp_path, monkeypatch):
    import ctc_ngram_cases as CN
    from speech2text_amd.model.decoding import RnntBeamDecoding, rnnt_beam_ngram_tokens_from_am
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    cfg = copy.deepcopy(_pruned_cfg())
    plain = _task("Pruned_Rnnt", copy.deepcopy(cfg), "cpu")
    est = NgramLm.estimate(CN.lm_sequences(_V, 200, 4), _V, order=3)
    est.names = list(plain._tokenizer.labels)
    path = tmp_path / "pieces.arpa"
    path.write_text(est.to_arpa(), encoding="utf-8")
    cfg["metric"] = {"decode_method": "rnnt_beam_search", "beam_size": 3, "cutoff_top_k": 3, "lm_weight": 0.4,
                     "lm": {"arpa": str(path)}}
    task = _task("Pruned_Rnnt", cfg, dev)
    sess = task._metric._decode_sess
    assert isinstance(sess, RnntBeamDecoding) and isinstance(sess._lm, NgramLm) and sess._fusable()
    assert (sess._lm_weight, sess._beam_size, sess._cutoff_top_k) == (0.4, 3, 3)
    assert list(task.state_dict()) == list(plain.state_dict())
    batch = _pcm_batch(dev, B=2, sec=1.0, V=_V)
    with torch.no_grad():
        for q in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            q.mul_(4.0)                                    # away from the near-ties of fresh models
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
    calls = _counted(monkeypatch)
    got = sess.beam_tokens(enc, el)
    assert calls == [True] and sess._lm.device.type == "cuda"
    with torch.no_grad():
        want = rnnt_beam_ngram_tokens_from_am(task._joiner._enc_proj(enc), el, task._predictor, task._joiner, sess._lm,
                                              0.4, 3, 3)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert int(got[2].sum()) > 0 and float(got[4].abs().max()) > 0
    task.validation_step(batch, 0)
    assert "wer" in task.logged and calls == [True, True]
