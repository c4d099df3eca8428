"""CPU: the yardsticks of the RNN-T searches over the LSTM predictor (csrc/decode_lstm.hip).

tests/rnnt_lstm_search_f64.py is pinned to the reference's own RnntGreedyDecoding / RnntBeamDecoding
loops through tests/golden/rnnt_lstm_search_ref.npz (tools/gen_golden.py::gen_rnnt_lstm_search ran
those classes over the plain-torch stand-ins) and to the project's module loops over the same
stand-ins (the real LstmPredictor's layers are HIP kernels: it does not run on the CPU).  Then the
conditions every case of tests/rnnt_lstm_search_cases.py must meet, with no exclusions: float64
decides every node of every utterance by at least 1e-3, float32 gives the same tokens, every greedy
case walks the forced frame advance; and the recorded float32 costs are checked to a factor 4, so
the GPU file's bounds (max(2e-5, 8 x figure)) cannot drift.
"""
import os

import numpy as np
import pytest
import torch

import rnnt_lstm_search_cases as C
import rnnt_lstm_search_f64 as S
from yardstick import _Ids


def _fixture(golden_dir):
    with np.load(os.path.join(golden_dir, "rnnt_lstm_search_ref.npz")) as z:
        raw = {k: z[k] for k in z.files}
    out = []
    for ci in range(int(raw["n_configs"][0])):
        pre = f"c{ci}_"
        c = {k[len(pre):]: v for k, v in raw.items() if k.startswith(pre)}
        model = str(c["model"][0])
        seed, Tmax, mts, beam, topk = (int(x) for x in c["settings"])
        w = {k[2:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("w_") and not k.startswith("w_l")}
        w["lin_w"], w["lin_b"] = torch.from_numpy(c["w_lin_w"]), torch.from_numpy(c["w_lin_b"])
        w["layers"] = []
        for l in range(C.MODELS[model]["L"]):
            w["layers"].append({k[len(f"w_l{l}_"):]: torch.from_numpy(v) for k, v in c.items()
                                if k.startswith(f"w_l{l}_")})
        w.update(eps_in=C.EPS_IN, eps_lstm=C.EPS_LSTM, eps_out=C.EPS_OUT)
        cfg = dict(model=model, act=C.MODELS[model]["act"], mts=mts, beam_size=beam, topk=topk, w=w)
        for kind in ("greedy", "beam"):
            k = kind + "_"
            lens, off, ams = c[k + "lengths"].tolist(), 0, []
            for n in lens:
                ams.append(torch.from_numpy(c[k + "am_packed"][off:off + n]))
                off += n
            cfg[kind] = dict(am=ams, tokens=[c[k + "tokens"][b, :n].tolist()
                                             for b, n in enumerate(c[k + "tok_len"].tolist())],
                             margin=c[k + "margin"])
        cfg["beam_"] = dict(frames=[c["beam_frames"][b, :n].tolist()
                                    for b, n in enumerate(c["beam_tok_len"].tolist())],
                            score=c["beam_score_f64"], score_ref=c["beam_score_ref_f32"])
        out.append(cfg)
    return out


def test_restatement_reproduces_the_reference_loops(golden_dir):
    fx = _fixture(golden_dir)
    assert len(fx) == 3
    for c in fx:
        w = S.cast(c["w"], torch.float64)
        assert len(c["greedy"]["am"]) == len(c["beam"]["am"]) == 8
        assert sum(len(t) for t in c["greedy"]["tokens"]) > 0 and sum(len(t) for t in c["beam"]["tokens"]) > 0
        for b in range(8):
            tok, margin, _ = S.greedy(c["greedy"]["am"][b], w, c["act"], c["mts"])
            assert tok == c["greedy"]["tokens"][b], (c["model"], b)
            assert margin >= S.MARGIN and margin == pytest.approx(c["greedy"]["margin"][b], rel=1e-6)
            tok, score, frames, margin = S.beam_search(c["beam"]["am"][b], w, c["act"], c["beam_size"], c["topk"])
            assert tok == c["beam"]["tokens"][b] and frames == c["beam_"]["frames"][b], (c["model"], b)
            assert score == pytest.approx(c["beam_"]["score"][b], abs=1e-9) and margin >= S.MARGIN
            assert abs(c["beam_"]["score_ref"][b] - score) <= 1e-4 * max(1.0, abs(score))


def test_module_loops_on_plain_torch_stand_ins(golden_dir):
    """The project's module loops (what every combination without a device search runs, and what
    beam_tokens(fused=False) runs) over the stand-ins give the reference classes' tokens."""
    from speech2text_amd.model.decoding import RnntBeamDecoding, RnntGreedyDecoding
    for c in _fixture(golden_dir):
        pred, join = S.PlainPredictor(c["w"]), S.PlainJoiner(c["w"], c["act"])
        g = RnntGreedyDecoding(_Ids(), pred, join, max_token_step=c["mts"])
        bs = RnntBeamDecoding(_Ids(), pred, join, beam_size=c["beam_size"], cutoff_top_k=c["topk"])
        assert not g._fused() and not g._lstm_search() and not bs._fusable() and not bs._lstm_search()
        for b in range(8):
            assert g.decode(c["greedy"]["am"][b].unsqueeze(0)) == c["greedy"]["tokens"][b], (c["model"], b)
            am = c["beam"]["am"][b].unsqueeze(0)
            tokens, frames, out_len, score = bs.beam_tokens(am, torch.tensor([am.shape[1]]))
            n = int(out_len[0])
            assert tokens[0, :n].tolist() == c["beam"]["tokens"][b], (c["model"], b)
            assert frames[0, :n].tolist() == c["beam_"]["frames"][b]
            assert float(score[0]) == pytest.approx(c["beam_"]["score"][b], rel=1e-4, abs=1e-4)


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_utterance_of_the_case_is_decided(name):
    c = C.CASES[name]
    ref, f32 = C.reference(name), C.evaluate(name, torch.float32)
    _, _, am, lens = C.make(name)
    assert len(ref) == c["B"]
    for b, (r, s) in enumerate(zip(ref, f32)):
        margin = r[1] if c["beam"] is None else r[3]
        print(f"{name} utterance {b}: length {C.clamp(lens[b], c['T'])} tokens {len(r[0])} margin {margin:.3e}")
        assert margin >= S.MARGIN, f"{name} utterance {b}: float64 decides a node by {margin:.2e} only"
        assert s[0] == r[0], f"{name} utterance {b}: float32 walks another path"
        if c["beam"] is not None:
            assert s[2] == r[2]
    assert sum(len(r[0]) for r in ref) > 0
    if c["B"] > 1:
        assert int(lens[1]) == 0 and ref[1][0] == []
    if c["B"] > 2:
        assert int(lens[2]) > c["T"]
    if c["beam"] is None:
        assert sum(r[2] for r in ref) >= 1, "max_token_step never forced a frame on"
        assert max(len(r[0]) for r in ref) <= c["T"] * (c["mts"] + 1)


def test_cases_cover_what_the_kernels_branch_on():
    ms = [C.MODELS[c["model"]] for c in C.CASES.values()]
    assert {m["H"] for m in ms} >= {20, 48, 64, 512} and {m["L"] for m in ms} == {1, 2, 3}
    assert {m["ln"] for m in ms} == {True, False} and {m["act"] for m in ms} == {"relu", "tanh"}
    assert {m["V"] for m in ms} >= {63, 65, 128} and {m["inner"] for m in ms} >= {0, 24, 256}
    assert any(m["E"] != m["H"] for m in ms)
    assert {c["B"] for c in C.GREEDY_CASES.values()} >= {1, 17, 33}
    assert {c["B"] for c in C.BEAM_CASES.values()} >= {17, 33}
    assert {c["mts"] for c in C.GREEDY_CASES.values()} == {0, 1, 10}
    assert {c["beam"] for c in C.BEAM_CASES.values()} == {1, 4, 16}
    tk = [(c["topk"], C.MODELS[c["model"]]["V"]) for c in C.BEAM_CASES.values()]
    assert {k for k, _ in tk} >= {1, 4} and any(k > V for k, V in tk)
    assert max(c["T"] for c in C.CASES.values()) == 40
    y = C.MODELS["yaml"]
    assert (y["E"], y["H"], y["L"], y["D"], y["V"], y["inner"]) == (512, 512, 3, 256, 128, 256)
    assert (C.CASES["g_yaml"]["B"], C.CASES["g_yaml"]["T"]) == (4, 24)


@pytest.mark.parametrize("model", C.PRED_MODELS)
def test_fp32_cost_of_the_predictor_step(model):
    fig = C.pred_fp32_figure(model)
    print(f"fp32 cost of five chained steps, {model}: {fig:.3e}")
    rec = C.PRED_COST[model]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)
    masks = [int(e.sum()) for _, e, _ in C.pred_schedule(model)]
    assert masks[0] == C.PRED_ROWS and masks[2] == 0 and 0 < masks[1] < C.PRED_ROWS
    assert any(not torch.equal(p, torch.arange(C.PRED_ROWS)) for _, _, p in C.pred_schedule(model))


@pytest.mark.parametrize("name", list(C.BEAM_CASES))
def test_fp32_cost_of_the_beam_score(name):
    fig = C.beam_fp32_figure(name)
    print(f"fp32 cost of the beam score, {name}: {fig:.3e}")
    rec = C.BEAM_COST[name]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)
    assert set(C.BEAM_CASES) == set(C.BEAM_COST) and set(C.PRED_MODELS) == set(C.PRED_COST)
