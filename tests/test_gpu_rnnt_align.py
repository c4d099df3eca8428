"""GPU: RNN-T forced alignment on the device (csrc/rnnt_align.hip, kernels.rnnt_align, kernels.rnnt_full_lattice,
model/alignment.py RnntForcedAligner, BaseRnntTask.align) on the cases of tests/rnnt_align_cases.py, whose
conditions tests/test_rnnt_align_f64.py asserts on the CPU.  ok, tok_frame, tok_logp and score must equal
the float32 run of the restatement tests/rnnt_align_f64.py bit for bit, ties included, on the same px / py.
Cells outside an utterance's s <= Sb, t <= Tb are NaN in every case: a kernel that read one could not
return the restatement's bits.
"""
import math

import numpy as np
import pytest
import torch

import decode_support as DS
import lattice_types_f64 as LT
import rnnt_align_cases as C
import rnnt_align_f64 as A
from task_support import _base_cfg, _CONF, _pcm_batch, _pruned_cfg, _task, _TOK, _V
from yardstick import FLOOR, MARGIN

pytestmark = pytest.mark.gpu

RNNT_RTOL = 1e-4                           # tests/test_gpu_loss_lattices.py / test_gpu_loss_types.py: losses
_CACHE = {}


def _case(dev, name):
    """(the case, its tensors on the device, the kernel's result), once per case."""
    from speech2text_amd import kernels
    if name not in _CACHE:
        m = C.make(name)
        d = dict(px=m["px"].to(dev), py=m["py"].to(dev), boundary=m["boundary"].to(dev))
        out = kernels.rnnt_align(d["px"], d["py"], d["boundary"], m["ty"])
        _CACHE[name] = (m, d, out)
    return _CACHE[name]


# ------------------------------------------------------------------ 1. every case against the restatement
@pytest.mark.parametrize("name", list(C.CASES))
def test_entry_equals_the_float32_restatement_bit_for_bit(dev, name):
    from speech2text_amd import _native as N
    from speech2text_amd import kernels
    m, d, out = _case(dev, name)
    assert N.lib().s2t_rnnt_align_form(m["S"], m["T"], kernels.RNNT_TYPES[m["ty"]]) == C.FORMS[name]   # the form this case is for
    tf, lp, score, ok = C.dense(C.restated(name), m["S"])
    got = kernels.RnntAlignment(*(t.cpu() for t in out))
    assert got.tok_frame.dtype == torch.int32 and got.ok.dtype == torch.int32
    assert got.tok_frame.shape == got.tok_logp.shape == (m["B"], m["S"]) and got.score.shape == got.ok.shape == (m["B"],)
    assert torch.equal(got.ok, ok), name
    assert torch.equal(got.tok_frame, tf), name
    assert torch.equal(got.tok_logp.double(), lp), name                     # gathered exactly
    assert torch.equal(got.score.double(), score), name                     # bit for bit (-inf included)
    bad = ~ok.bool()                                                        # the sentinels of rows without a path
    assert bool((got.tok_frame[bad] == -1).all()) and bool((got.tok_logp[bad] == 0).all())
    assert bool((got.score[bad] == -math.inf).all())
    for b in range(m["B"]):                                                 # and beyond the transcripts
        assert bool((got.tok_frame[b, m["sb"][b]:] == -1).all()) and bool((got.tok_logp[b, m["sb"][b]:] == 0).all())
    again = kernels.rnnt_align(d["px"], d["py"], d["boundary"], m["ty"], out=out)
    for a, b in zip(again, got):                                            # into the same buffers: same bits
        assert torch.equal(a.cpu(), b), name


@pytest.mark.parametrize("name", [k for k, v in C.CASES.items() if v["S"] >= 1])
def test_score_is_at_most_the_log_likelihood_of_the_same_operands(dev, name):
    """The best path's score is one term of the sum over paths that the recursion kernel forms."""
    from speech2text_amd import kernels
    m, d, out = _case(dev, name)
    clamped = LT.make_boundary(m["sb"], m["tb"]).to(dev)     # (the loss takes its lengths as they are)
    ans = kernels.mutual_information(d["px"], d["py"], clamped, want_grads=False)[0].cpu().double()
    score, ok = out.score.cpu().double(), out.ok.cpu().bool()
    assert torch.equal(torch.isfinite(ans), ok), name        # a path for one is a path for the other
    if bool(ok.any()):
        slack = RNNT_RTOL * ans[ok].abs().clamp(min=1.0)
        print(f"{name}: largest score - ans {float((score - ans)[ok].max()):.3e}")
        assert bool((score[ok] <= ans[ok] + slack).all()), name


# ------------------------------------------------------------------ 2. the fused builder at R = S + 1
@pytest.mark.parametrize("rnnt_type", LT.TYPES)
@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_full_lattice_of_the_fused_joiner_against_float64(dev, act, rnnt_type):
    """kernels.rnnt_full_lattice (s2t_rnnt_pruned_fwd with zero ranges and a band of all S + 1 rows) against
    the float64 lattice restatement: every entry of px / py is the score of a one-arc lattice and is held to
    the losses' bound (rtol 1e-4; atol 1e-5 for entries near zero: fp32 log-softmax of logits below 16 is
    good to about 1e-6), the scores of the float64 recursion over the device's px / py to the same rtol."""
    from speech2text_amd import kernels
    g = torch.Generator().manual_seed(40)
    B, T, S, Cj = 3, 9, 5, 70                                # 70 classes: a partial second lane-slot
    am, lm = 2.0 * torch.randn(B, T, Cj, generator=g), 2.0 * torch.randn(B, S + 1, Cj, generator=g)
    sym = torch.randint(1, Cj, (B, S), generator=g)
    tl, el = torch.tensor([5, 3, 0]), torch.tensor([9, 6, 4])
    bnd = LT.make_boundary(tl, el)
    px, py = kernels.rnnt_full_lattice(am.to(dev), lm.to(dev), sym.to(dev), bnd.to(dev), 0, act, rnnt_type)
    rx, ry = LT.typed_pxpy(LT.joiner_logits(am.double(), lm.double(), None, act), sym, None, bnd, 0, rnnt_type)
    assert px.shape == rx.shape and py.shape == ry.shape
    for got, ref, what in ((px, rx, "px"), (py, ry, "py")):
        got = got.cpu().double()
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), fin), what   # -inf exactly where the restatement has it
        print(f"{act} {rnnt_type} {what}: max abs dev {float((got[fin] - ref[fin]).abs().max()):.3e}")
        np.testing.assert_allclose(got[fin].numpy(), ref[fin].numpy(), rtol=RNNT_RTOL, atol=1e-5)
    sc = LT.scores(px.cpu().double(), py.cpu().double(), bnd)
    ref = LT.scores(rx, ry, bnd)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(sc), fin) and bool(fin.any())
    np.testing.assert_allclose(sc[fin].numpy(), ref[fin].numpy(), rtol=RNNT_RTOL)


# ------------------------------------------------------------------ 3. end to end
def _stateless_pair(dev, V, D, act="relu"):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    torch.manual_seed(5)
    p = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D, "symbol_embedding_dim": 16,
                                                    "context_size": 2}})
    j = Joiner(JoinerConfig(input_dim=D, output_dim=V, activation=act, use_out_project=False))
    with torch.no_grad():
        for q in list(p.parameters()) + list(j.parameters()):
            q.mul_(3.0)
    return p.to(dev).eval(), j.to(dev).eval()


def _lstm_pair(dev, V, D):
    return DS._lstm_pair(dev, V, D, 31, 2.0)


def _batch(dev, V, D, B=3, T=12, S=5):
    g = torch.Generator().manual_seed(21)
    enc = torch.randn(B, T, D, generator=g).to(dev)
    lens, tl = torch.tensor([T, T - 3, 4][:B]), torch.tensor([S, S - 2, 0][:B])
    targets = torch.randint(1, V - 1, (B, S), generator=g)
    return enc, lens.to(dev), targets.to(dev), tl.to(dev)


@pytest.mark.parametrize("rnnt_type", LT.TYPES)
@pytest.mark.parametrize("pair", ["stateless_fused", "lstm_out_projection"])
def test_aligner_end_to_end_against_the_float64_optimum(dev, pair, rnnt_type):
    """The device's path, re-scored in float64 on the device's own px / py, must lie within max(2e-5, 8 x
    what float32 costs the restatement) relative of the float64 optimum: the bound of the CTC aligner's
    tests.  What float32 costs the restatement is measured here, on the same operands: its float32 run's
    path, re-scored in float64, against the float64 run's."""
    from speech2text_amd.model.alignment import RnntForcedAligner
    V, D = 24, 32
    p, j = _stateless_pair(dev, V, D) if pair == "stateless_fused" else _lstm_pair(dev, V, D)
    enc, lens, targets, tl = _batch(dev, V, D)
    al = RnntForcedAligner(p, j, frame_seconds=0.04, rnnt_type=rnnt_type)
    with torch.no_grad():
        px, py, bnd = al._lattice(enc, lens, targets, tl)
    assert px.is_cuda and px.shape == (3, 5, 13 if rnnt_type == "regular" else 12) and py.shape == (3, 6, 12)
    out = al.align(enc, lens, targets, tl)
    px, py = px.cpu(), py.cpu()
    feasible = 0
    for b, a in enumerate(out):
        sb, tb = int(tl[b]), int(lens[b])
        ref = A.align(px[b].double(), py[b].double(), sb, tb, rnnt_type)
        f32 = A.align(px[b], py[b], sb, tb, rnnt_type)
        assert a.ok == ref.ok == f32.ok, (pair, rnnt_type, b)
        if not a.ok:
            assert a.tokens == [] and a.score == -math.inf
            continue
        feasible += 1
        scale = max(1.0, abs(ref.score))
        cost = abs(A.path_score(px[b], py[b], sb, tb, f32.tok_frame, rnnt_type) - ref.score) / scale
        frames = [t.begin for t in a.tokens]
        dev_err = abs(A.path_score(px[b], py[b], sb, tb, frames, rnnt_type) - ref.score) / scale
        print(f"{pair} {rnnt_type} row {b}: device path {dev_err:.3e}, float32 restatement {cost:.3e}")
        assert dev_err <= max(FLOOR, MARGIN * cost), (pair, rnnt_type, b)
        assert frames == f32.tok_frame and a.score == f32.score         # (and the float32 bits, as everywhere)
        assert [t.token for t in a.tokens] == targets[b, :sb].tolist()
        assert [t.logp for t in a.tokens] == f32.tok_logp
        assert all(t.end == t.begin + 1 and t.begin_s == t.begin * 0.04 for t in a.tokens)
        assert all(0 <= t.begin < tb for t in a.tokens) and frames == sorted(frames)
        if rnnt_type != "regular":
            assert len(set(frames)) == len(frames)
    assert feasible >= 2


@pytest.mark.parametrize("search", ["greedy", "beam"])
@pytest.mark.parametrize("pair", ["stateless_fused", "lstm_out_projection"])
def test_align_hypotheses_gives_every_search_ordered_times(dev, pair, search):
    from speech2text_amd.model.alignment import RnntForcedAligner
    from speech2text_amd.model.decoding import (RnntGreedyDecoding, rnnt_beam_lstm_tokens_from_am,
                                                rnnt_beam_tokens_from_am, rnnt_greedy_lstm_tokens_from_am)
    V, D = 24, 32
    p, j = _stateless_pair(dev, V, D) if pair == "stateless_fused" else _lstm_pair(dev, V, D)
    enc, lens, _, _ = _batch(dev, V, D)
    with torch.no_grad():
        am = j._enc_proj(enc).float().contiguous()
    if pair == "stateless_fused":
        if search == "greedy":
            tokens, out_len = RnntGreedyDecoding(None, p, j, max_token_step=2).greedy_tokens(enc, lens)
        else:
            tokens, _, out_len, _ = rnnt_beam_tokens_from_am(am, lens, p, j, 4, 4)
    elif search == "greedy":
        tokens, out_len = rnnt_greedy_lstm_tokens_from_am(am, lens, p, j, 2)
    else:
        tokens, _, out_len, _ = rnnt_beam_lstm_tokens_from_am(am, lens, p, j, 4, 4)
    al = RnntForcedAligner(p, j, frame_seconds=0.04)                    # regular: a frame may hold several tokens
    out = al.align_hypotheses(enc, lens, tokens, out_len)
    assert int(out_len.max()) >= 1
    for b, a in enumerate(out):
        n = int(out_len[b])
        assert a.ok and [t.token for t in a.tokens] == tokens[b, :n].tolist(), (pair, search, b)
        f = [t.begin for t in a.tokens]
        assert f == sorted(f) and all(0 <= x < int(lens[b]) for x in f), (pair, search, b)
        assert all(t.end_s == t.end * 0.04 for t in a.tokens) and math.isfinite(a.score)


# ------------------------------------------------------------------ 4. graph capture
@pytest.mark.parametrize("name", ["s7_b17_reg_ragged", "s5_mod_t5121_ws"])
def test_capture_and_replay_in_a_graph(dev, name):
    from speech2text_amd import kernels
    m, d, out = _case(dev, name)
    want = [t.clone() for t in out]
    held = kernels.RnntAlignment(*(torch.empty_like(t) for t in out))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kernels.rnnt_align(d["px"], d["py"], d["boundary"], m["ty"], out=held)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.rnnt_align(d["px"], d["py"], d["boundary"], m["ty"], out=held)
    for t in held:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(held, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 5. the Python surface
def test_surface_checks_its_inputs(dev):
    from speech2text_amd import kernels
    px, py = torch.zeros(1, 2, 5, device=dev), torch.zeros(1, 3, 4, device=dev)
    bnd = torch.tensor([[0, 0, 2, 4]], device=dev)
    with pytest.raises(ValueError, match="exceed the kernel's limit of 1024 lattice rows"):
        kernels.rnnt_align(torch.zeros(1, 1024, 3, device=dev), torch.zeros(1, 1025, 2, device=dev), bnd)
    with pytest.raises(RuntimeError, match="contiguous"):
        kernels.rnnt_align(px.transpose(1, 2), py, bnd)
    with pytest.raises(RuntimeError, match="int64"):
        kernels.rnnt_align(px, py, bnd.int())
    with pytest.raises(RuntimeError, match="float32"):
        kernels.rnnt_align(px.double(), py, bnd)
    with pytest.raises(ValueError, match="operands of the modified lattice"):
        kernels.rnnt_align(px, py, bnd, rnnt_type="modified")
    out = kernels.rnnt_align(px, py, bnd)                               # all arcs equal: every tie goes to the blank,
    assert out.ok.tolist() == [1] and out.tok_frame.tolist() == [[0, 0]] and float(out.score) == 0.0   # walking back


def test_aligner_runs_the_kernel_on_device_tensors_and_the_loop_beyond_its_limit(dev):
    from speech2text_amd import _native as N
    from speech2text_amd.model.alignment import RnntForcedAligner
    name = "ties_s6_b17_mod"
    m, d, out = _case(dev, name)
    al = RnntForcedAligner(None, None, rnnt_type=m["ty"])
    rows = al._rows(d["px"], d["py"], d["boundary"])
    for a, b in zip(rows, out):
        assert torch.equal(a, b)
    for b in range(3):                                                   # the host loop on device tensors: the same bits
        r = al._module_loop(d["px"][b], d["py"][b], m["sb"][b], m["tb"][b], m["ty"])
        assert r.ok == int(out.ok[b]) and (not r.ok or torch.equal(r.tok_frame, out.tok_frame[b, :m["sb"][b]]))
        assert not r.ok or r.score == float(out.score[b])
    g = torch.Generator().manual_seed(5)
    S, T = 1024, 3                                                       # 1025 rows: refused with -4, the loop serves it
    px, py = torch.randn(1, S, T + 1, generator=g).to(dev), torch.randn(1, S + 1, T, generator=g).to(dev)
    px[:, :, T] = -math.inf
    bnd = torch.tensor([[0, 0, S, T]], device=dev)
    buf = torch.empty(16, dtype=torch.int64, device=dev)
    rc = N.lib().s2t_rnnt_align(N.fp(px), N.fp(py), N.lp(bnd), 1, S, T, 0, None, N.ptr(buf), N.ptr(buf), N.ptr(buf),
                                N.ptr(buf), N.stream())
    assert rc == -4
    rows = RnntForcedAligner(None, None)._rows(px, py, bnd)
    want = A.align(px[0].cpu(), py[0].cpu(), S, T, "regular")
    assert rows.ok.tolist() == [1] and rows.tok_frame[0].tolist() == want.tok_frame and float(rows.score) == want.score


# ------------------------------------------------------------------ 6. the tasks
def _check_task_alignment(out, batch, lens, labels_of, one_per_frame):
    assert len(out) == batch["label"].shape[0]
    for b, a in enumerate(out):
        Tb, U = int(lens[b]), int(batch["label_length"][b])
        assert a.ok and math.isfinite(a.score) and a.score < 0.0
        assert [t.token for t in a.tokens] == batch["label"][b, :U].tolist()
        assert [t.piece for t in a.tokens] == [labels_of[i] for i in batch["label"][b, :U].tolist()]
        f = [t.begin for t in a.tokens]
        assert f == sorted(f) and all(0 <= x < Tb for x in f) and all(t.end == t.begin + 1 for t in a.tokens)
        assert not one_per_frame or len(set(f)) == len(f)
        assert all(t.begin_s == t.begin * 0.04 for t in a.tokens)
        assert a.words and a.words[0].begin == a.tokens[0].begin and a.words[-1].end == a.tokens[-1].end
        assert sum(w.logp for w in a.words) == pytest.approx(sum(t.logp for t in a.tokens), rel=1e-5)
        assert a.score <= sum(t.logp for t in a.tokens) + 1e-4          # the blanks only subtract


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
def test_pruned_rnnt_task_align(dev, rnnt_type):
    cfg = _pruned_cfg()
    cfg["loss"]["config"] = {**cfg["loss"].get("config", {}), "rnnt_type": rnnt_type, "delay_penalty": 0.01}
    task = _task("Pruned_Rnnt", cfg, dev)
    assert task._align_rnnt_type() == rnnt_type
    batch = _pcm_batch(dev, B=2, sec=1.0, V=_V)
    out = task.align(batch, frame_seconds=0.04)
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
        _, dl = task._decoder(enc, el)
    _check_task_alignment(out, batch, dl, task._tokenizer.labels, rnnt_type != "regular")


def test_rnnt_task_align_materialises_the_out_projection_joiner(dev):
    cfg = _base_cfg()
    cfg.update({"task": {"type": "Rnnt"}, "tokenizer": _TOK, "encoder": _CONF,
                "decoder": {"model": "Identity", "config": {"dummy": -1}},
                "predictor": {"model": "Lstm", "config": {"num_symbols": _V, "output_dim": 64, "symbol_embedding_dim": 32,
                                                          "num_lstm_layers": 2, "lstm_hidden_dim": 48,
                                                          "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3,
                                                          "lstm_dropout": 0.1}},
                "joiner": {"input_dim": 64, "output_dim": _V, "inner_dim": 48, "activation": "tanh", "prune_range": 0},
                "loss": {"model": "Rnnt", "config": {"blank_label": 0, "reduction": "mean"}},
                "metric": {"decode_method": "rnnt_greedy_search", "max_token_step": 1}})
    task = _task("Rnnt", cfg, dev)
    assert task._joiner._use_out_project and task._align_rnnt_type() == "regular"
    batch = _pcm_batch(dev, B=2, sec=1.0, V=_V)
    out = task.align(batch, frame_seconds=0.04)
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
        _, dl = task._decoder(enc, el)
    _check_task_alignment(out, batch, dl, task._tokenizer.labels, False)
