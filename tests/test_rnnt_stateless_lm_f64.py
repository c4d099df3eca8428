"""CPU: the yardstick of the RNN-T beam search with RNN-LM shallow fusion over the stateless predictor
(csrc/decode_lstm.hip s2t_rnnt_beam_stateless_lm, s2t_stateless_pred_step) and the Python surface around it.

The conditions every case of tests/rnnt_stateless_lm_cases.py must meet, with no exclusions (margins,
float32 on the same path, the LM changes at least one hypothesis where beam > 1), the recorded float32
costs to a factor 4, the restatement against rnnt_lm_fusion_f64.beam_search_lm_stateless and against the
project's _module_loop_lm, rnnt_stateless_desc, and the refusals of both entry points: they precede any
launch, so the library answers them without a GPU.

The project's modules compute on the device only (no CPU fallback), so the module loop runs here over
plain-torch stand-ins with the modules' interface; tests/test_gpu_rnnt_stateless_lm.py runs it over the
real StatelessPredictor, Joiner and RnnLm.
"""
import ctypes
import math

import pytest
import torch

import rnnt_lm_fusion_cases as L
import rnnt_lm_fusion_f64 as F
import rnnt_lstm_search_f64 as S
import rnnt_stateless_lm_cases as SC
import rnnt_stateless_lm_f64 as SF
from yardstick import _Ids


class _PlainStateless:
    """init_state / streaming_step of the stateless predictor over the weights of rnnt_stateless_lm_f64."""

    def __init__(self, p, ctx):
        self.p, self.ctx = p, ctx

    def init_state(self):
        return torch.zeros(1, self.ctx - 1, dtype=torch.int64)

    def streaming_step(self, input, state):
        assert input.shape == (1, 1)
        rows = torch.cat([state, input.long()], dim=1)
        p = self.p
        e = (p["emb"][rows] * p["conv_w"].t().unsqueeze(0)).sum(dim=1)
        return (e @ p["lin_w"].t() + p["lin_b"]).reshape(1, 1, -1), rows[:, 1:]


# ------------------------------------------------------------------ 1. the cases' conditions and costs
@pytest.mark.parametrize("name", list(SC.CASES))
def test_every_utterance_of_the_case_is_decided(name):
    c = SC.CASES[name]
    ref, f32, plain = SC.reference(name), SC.evaluate(name, torch.float32), SC.unfused(name)
    _, am, lens, _ = SC.make(name)
    assert len(ref) == am.shape[0] == c["B"]
    for b, (r, s) in enumerate(zip(ref, f32)):
        print(f"{name} utterance {b}: length {SC.clamp(lens[b], c['T'])} tokens {r[0]} (lm_weight 0: {plain[b][0]}) "
              f"lm_score {r[2]:.4f} margin {r[4]:.3e}")
        assert r[4] >= S.MARGIN, f"{name} utterance {b}: float64 decides a node by {r[4]:.2e} only"
        assert s[0] == r[0] and s[3] == r[3], f"{name} utterance {b}: float32 walks another path"
    assert sum(len(r[0]) for r in ref) > 0
    changed = [b for b, (r, q) in enumerate(zip(ref, plain)) if r[0] != q[0]]
    print(f"{name}: the LM changes utterances {changed}")
    if c["beam"] > 1:
        assert changed, f"{name}: a search that dropped the LM term would pass"
    else:
        assert not changed and any(r[2] != 0.0 for r in ref)
    if c["B"] > 1:
        assert int(lens[1]) == 0 and ref[1][:4] == ([], 0.0, 0.0, [])
    if c["B"] > 2:
        assert int(lens[2]) > c["T"]
    if c["B"] > 3:
        assert 1 <= int(lens[3:].min()) and int(lens[3:].max()) <= c["T"]
    if c["B"] > 4:
        assert len(set(lens[3:].tolist())) > 1            # ragged


@pytest.mark.parametrize("name", [SC.B33, "s_b17_ctx5_e65"])
def test_the_zero_weight_search_of_these_cases_is_decided_too(name):
    """The GPU file compares the lm_weight = 0 search with the one-workgroup kernel token for token."""
    plain, f32 = SC.unfused(name), SC.evaluate(name, torch.float32, lm_weight=0.0)
    assert SC.CASES[name]["inner"] == 0 and min(r[4] for r in plain) >= S.MARGIN
    assert all(a[0] == b[0] and a[3] == b[3] for a, b in zip(plain, f32)) and sum(len(r[0]) for r in plain) > 0


def test_cases_cover_what_the_issue_names():
    cs = SC.CASES.values()
    assert {c["ctx"] for c in cs} >= {1, 2, 5}
    assert {c["E"] for c in cs} >= {12, 65, 130, 512}
    assert all(c["D"] % 16 for c in cs if c["D"] != 256)
    assert {c["V"] for c in cs} == {11, 63, 65, 128}
    assert {(c["beam"], c["topk"]) for c in cs} >= {(1, 1), (4, 4)}
    assert any(c["beam"] == 16 and c["topk"] >= c["V"] for c in cs)
    assert {c["B"] for c in cs} >= {1, 17, 33}
    assert all(c["T"] <= (4 if c["B"] >= 17 else 12) for c in cs)
    assert sum(1 for c in cs if c["inner"] > 0) == 1 and sum(1 for c in cs if c["start"] is not None) == 1
    y = SC.CASES[SC.YAML]
    assert (y["V"], y["E"], y["D"], y["ctx"], y["B"], y["lm"]) == (128, 512, 256, 5, 4, "yaml")
    assert all(SC.LM_MODELS[c["lm"]]["V"] == c["V"] for c in cs)
    assert set(SC.CASES) == set(SC.FUSED_COST) and set(SC.STEP_CASES) == set(SC.STEP_COST)
    assert {SC.CASES[n]["ctx"] for n in SC.STEP_CASES} >= {1, 5}


@pytest.mark.parametrize("name", SC.STEP_CASES)
def test_fp32_cost_of_the_predictor_step(name):
    fig = SC.step_fp32_figure(name)
    print(f"fp32 cost of five chained stateless predictor steps, {name}: {fig:.3e}")
    rec = SC.STEP_COST[name]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_fp32_cost_of_the_fused_scores(name):
    fig = SC.fused_fp32_figure(name)
    print(f"fp32 cost of score / lm_score, {name}: {fig:.3e}")
    rec = SC.FUSED_COST[name]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)


# ------------------------------------------------------------------ 2. what the restatement is
def test_restatement_is_the_sibling_search_where_both_apply():
    """inner == 0: rnnt_lm_fusion_f64.beam_search_lm_stateless walks the same path to the same scores."""
    for name in ("s_v11_beam16_kV", "s_b17_ctx5_e65"):
        c = SC.CASES[name]
        p, am, lens, sd = SC.make(name)
        p, sd = SF.cast(p, torch.float64), L.cast(sd, torch.float64)
        for b, r in enumerate(SC.reference(name)):
            got = F.beam_search_lm_stateless(am[b, :SC.clamp(lens[b], c["T"])].double(), p, c["ctx"], c["act"],
                                             c["beam"], c["topk"], sd, c["weight"], c["start"])
            assert got[0] == r[0] and got[3] == r[3], (name, b)
            assert got[1] == pytest.approx(r[1], abs=1e-9) and got[2] == pytest.approx(r[2], abs=1e-9)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_lm_score_and_score_identities(name):
    c = SC.CASES[name]
    p, am, lens, sd = SC.make(name)
    p, sd = SF.cast(p, torch.float64), L.cast(sd, torch.float64)
    for b, (tokens, score, lm_score, frames, _) in enumerate(SC.reference(name)):
        assert lm_score == pytest.approx(F.lm_score_ref(sd, tokens, c["start"]), abs=1e-9), (name, b)
        path = SF.path_score(am[b, :SC.clamp(lens[b], c["T"])], p, c["ctx"], c["act"], tokens, frames)
        assert score - c["weight"] * lm_score == pytest.approx(path, abs=1e-9), (name, b)
        assert len(tokens) == len(frames) and frames == sorted(set(frames))


def test_masked_step_keeps_and_shifts():
    name = "s_b17_ctx5_e65"
    chain = SC.step_chain(name, torch.float64)
    sched = SC.step_schedule(name)
    R, n = SC.STEP_ROWS, SC.CASES[name]["ctx"]
    ctx0, lm0 = chain[0]
    assert torch.equal(ctx0[:, -1], sched[0][0]) and int(ctx0[:, :-1].abs().sum()) == 0
    for i in range(1, 5):
        tokens, emit, parent = sched[i]
        (pc, pl), (cc, cl) = chain[i - 1], chain[i]
        for r in range(R):
            q = int(parent[r])
            if int(emit[r]):
                assert cc[r].tolist() == pc[q, 1:].tolist() + [int(tokens[r])]
            else:
                assert torch.equal(cc[r], pc[q]) and torch.equal(cl[r], pl[q])
    assert n == 5 and chain[4][0].shape == (R, 5)


@pytest.mark.parametrize("name", ["s_b1_ctx1_beam1_k1", "s_v11_beam16_kV", "s_v128_e130_beam16_start", "s_inner_v65"])
def test_module_loop_lm_on_plain_torch_stand_ins(name):
    from speech2text_amd.model.decoding import RnntBeamDecoding
    c = SC.CASES[name]
    p, am, lens, sd = SC.make(name)
    p, sd = SF.cast(p, torch.float64), L.cast(sd, torch.float64)
    dec = RnntBeamDecoding(_Ids(), _PlainStateless(p, c["ctx"]), S.PlainJoiner(p, c["act"]), beam_size=c["beam"],
                           cutoff_top_k=c["topk"], lm=F.PlainLm(sd), lm_weight=c["weight"], lm_start_token=c["start"])
    assert not dec._fusable() and not dec._lstm_search()
    ref = SC.reference(name)
    tokens, frames, out_len, score, lm_score = dec.beam_tokens(am.double(), lens)
    for b, (tok, sc, lms, frm, _) in enumerate(ref):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == tok and frames[b, :n].tolist() == frm, (name, b)
        got = dec._module_loop_lm(am[b:b + 1, :SC.clamp(lens[b], c["T"])].double())
        assert got[0] == tok and got[1] == frm
        assert got[2] == pytest.approx(sc, abs=1e-9) and got[3] == pytest.approx(lms, abs=1e-9)


# ------------------------------------------------------------------ 3. the descriptor
def _real_modules(V=11, E=12, D=20, ctx=2, inner=0, act="relu"):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D, "symbol_embedding_dim": E,
                                                       "context_size": ctx}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=max(inner, 1), activation=act, prune_range=5,
                               use_out_project=inner > 0))
    return pred, join


def test_stateless_desc_fields_and_foreign_modules():
    from speech2text_amd import _native as N
    from speech2text_amd.model.decoding import RnntBeamDecoding, rnnt_stateless_desc
    pred, join = _real_modules(V=11, E=12, D=20, ctx=3, inner=0, act="tanh")
    desc, keep = rnnt_stateless_desc(pred, join)
    d = keep[-1]
    assert desc is not None and isinstance(d, N.struct("S2tRnntStatelessDesc"))
    assert (d.V, d.E, d.D, d.ctx, d.inner, d.act) == (11, 12, 20, 3, 0, 1)
    p = pred.predictor
    assert d.emb == keep[0].data_ptr() and torch.equal(keep[0], p._embedding.weight)
    assert keep[1].shape == (12, 3) and torch.equal(keep[1], p._conv.weight.reshape(12, 3)) and d.conv_w == keep[1].data_ptr()
    assert d.lin_w == keep[2].data_ptr() and keep[2].shape == (20, 12) and keep[3].shape == (20,)
    assert d.pre_w == keep[4].data_ptr() and keep[4].shape == (11, 20) and d.pre_b == keep[5].data_ptr()
    assert not d.out1_w and not d.out1_b and not d.out2_w and not d.out2_b
    assert rnnt_stateless_desc(p, join)[0] is not None     # the bare StatelessPredictor too
    pred, join = _real_modules(V=11, inner=24)
    desc, keep = rnnt_stateless_desc(pred, join)
    d = keep[-1]
    assert (d.inner, d.act) == (24, 0) and d.out1_w and d.out2_b
    assert keep[6].shape == (24, 11) and keep[8].shape == (11, 24)
    dec = RnntBeamDecoding(_Ids(), pred, join)
    assert not dec._fusable() and not dec._lstm_search()   # (the out-projection pair without an LM: the loop)
    p0 = SF.cast(SC.make("s_v11_beam16_kV")[0], torch.float64)
    for foreign in ((_PlainStateless(p0, 2), join), (pred, S.PlainJoiner(p0, "relu")), (object(), object())):
        assert rnnt_stateless_desc(*foreign) == (None, [])
    from speech2text_amd.model.predictor.predictor import Predictor
    lstm = Predictor({"model": "Lstm", "config": {"num_symbols": 11, "output_dim": 20, "symbol_embedding_dim": 12,
                                                  "num_lstm_layers": 1, "lstm_hidden_dim": 8, "lstm_layer_norm": True,
                                                  "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}})
    assert rnnt_stateless_desc(lstm, join) == (None, [])


# ------------------------------------------------------------------ 4. the refusals precede any launch
def _descs(**change):
    """Descriptors with NULL parameters (never followed): a stateless pair and an LM, `change` applied."""
    from speech2text_amd import _native as N
    d = N.struct("S2tRnntStatelessDesc")()
    d.V, d.E, d.D, d.ctx, d.inner, d.act = 11, 12, 20, 2, 0, 0
    lm = N.struct("S2tRnnLmDesc")()
    lm.V, lm.E, lm.H, lm.num_layers = 11, 8, 8, 1
    for k, v in change.items():
        if k.startswith("lm_"):
            setattr(lm, k[3:], v)
        elif hasattr(d, k):
            setattr(d, k, v)
    return d, lm


_INSIDE = [dict(), dict(V=8192, lm_V=8192), dict(V=1, lm_V=1), dict(D=8192), dict(D=1), dict(inner=8192), dict(E=1024),
           dict(E=1), dict(ctx=64), dict(ctx=1), dict(act=1)]
_OUTSIDE = [dict(V=8193, lm_V=8193), dict(V=0, lm_V=0), dict(D=8193), dict(D=0), dict(inner=8193), dict(inner=-1),
            dict(E=1025), dict(E=0), dict(ctx=65), dict(ctx=0), dict(act=2), dict(act=-1)]


def test_size_functions_inside_the_limits():
    from speech2text_amd import _native as N
    lib = N.lib()
    assert (N.const("S2T_RNNT_LSTM_MAX_VOCAB"), N.const("S2T_RNNT_LSTM_MAX_HIDDEN"), N.const("S2T_RNNT_LSTM_MAX_BEAM"),
            N.const("S2T_RNNT_STATELESS_MAX_CONTEXT")) == (8192, 1024, 16, 64)
    for change in _INSIDE:
        d, lm = _descs(**change)
        n = lib.s2t_stateless_pred_step_workspace_bytes(ctypes.byref(d), 19)
        assert n > 0 and n % 256 == 0 and n >= 4 * 19 * (d.E + d.D), change
        for beam in (1, 16):
            m = lib.s2t_rnnt_beam_stateless_lm_workspace_bytes(ctypes.byref(d), ctypes.byref(lm), 3, 7, beam)
            R = 3 * beam
            assert m % 256 == 0 and m >= 4 * (2 * R * (d.ctx + d.V) + 3 * 7 * beam + 2 * R * (2 * lm.H + lm.V)), change
    d, lm = _descs()
    assert lib.s2t_rnnt_beam_stateless_lm_workspace_bytes(ctypes.byref(d), ctypes.byref(lm), 3, 0, 4) > 0   # (T = 0)


@pytest.mark.parametrize("change", _OUTSIDE + [dict(lm_V=12), dict(lm_H=1028), dict(lm_H=6), dict(lm_E=1025),
                                               dict(lm_num_layers=9), dict(lm_num_layers=0), dict(no_lm=1),
                                               dict(start=11), dict(weight=math.inf), dict(weight=math.nan),
                                               dict(beam=17), dict(beam=0), dict(topk=0), dict(topk=17, V=32, lm_V=32),
                                               dict(T=0), dict(no_ws=1)], ids=str)
def test_limits_just_outside_are_refused_before_any_launch(change):
    """Every refusal is made on the host from the descriptors' integers: the parameter pointers are NULL
    and the data pointers are not device memory, so a call that got past its checks would not return."""
    from speech2text_amd import _native as N
    lib = N.lib()
    d, lm = _descs(**change)
    pd, plm = ctypes.byref(d), None if "no_lm" in change else ctypes.byref(lm)
    in_desc = any(k in ("V", "E", "D", "ctx", "inner", "act") for k in change) and "topk" not in change
    in_lm = (any(k.startswith("lm_") for k in change) or "no_lm" in change) and "topk" not in change
    beam, topk = change.get("beam", 4), change.get("topk", 4)
    if in_desc:
        assert lib.s2t_stateless_pred_step_workspace_bytes(pd, 19) == 0
        assert lib.s2t_stateless_pred_step(pd, 19, 1, 1, None, 1, 1, 1, 1, 1, None) == -1
    if in_desc or in_lm or "beam" in change:
        assert lib.s2t_rnnt_beam_stateless_lm_workspace_bytes(pd, plm, 3, 7, beam) == 0
    ws = None if "no_ws" in change else 1
    assert lib.s2t_rnnt_beam_stateless_lm(pd, plm, 1, 1, 3, change.get("T", 7), beam, topk, change.get("weight", 0.3),
                                          change.get("start", -1), ws, 1, 1, 1, 1, 1, None) == -1


def test_step_refuses_mixed_buffers_and_sizes_refuse_empty_batches():
    from speech2text_amd import _native as N
    lib = N.lib()
    d, lm = _descs()
    pd, plm = ctypes.byref(d), ctypes.byref(lm)
    assert lib.s2t_stateless_pred_step_workspace_bytes(pd, 0) == 0 and lib.s2t_stateless_pred_step_workspace_bytes(None, 4) == 0
    assert lib.s2t_rnnt_beam_stateless_lm_workspace_bytes(pd, plm, 0, 7, 4) == 0
    assert lib.s2t_rnnt_beam_stateless_lm_workspace_bytes(pd, plm, 3, -1, 4) == 0
    # (tokens, emit, parent, ctx_in, lm_in, ctx_out, lm_out, workspace): stand-in addresses, never followed
    assert lib.s2t_stateless_pred_step(pd, 4, 8, 8, None, 16, 32, 16, 64, 8, None) == -1    # ctx in place, lm not
    assert lib.s2t_stateless_pred_step(pd, 4, 8, 8, None, 16, 32, 24, 32, 8, None) == -1    # lm in place, ctx not
    assert lib.s2t_stateless_pred_step(pd, 4, 8, 8, 8, 16, 32, 16, 32, 8, None) == -1       # in place with a gather
    assert lib.s2t_stateless_pred_step(pd, 4, 8, 8, None, 16, 32, 16, 32, None, None) == -1  # no workspace
    assert lib.s2t_stateless_pred_step(pd, 0, 8, 8, None, 16, 32, 16, 32, 8, None) == 0     # no rows: nothing to do
    assert lib.s2t_rnnt_beam_stateless_lm(pd, plm, 1, 1, 0, 7, 4, 4, 0.3, -1, 1, 1, 1, 1, 1, 1, None) == 0   # B = 0
