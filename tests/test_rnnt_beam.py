"""RNN-T beam search (reference model/decoding.py:295-435): the fused device search
(csrc/decode_rnnt.hip, s2t_rnnt_beam_stateless), RnntBeamDecoding with its module loop,
DecodingFactory and the `rnnt_beam_search` metric.

The answers come from tests/golden/rnnt_beam_ref*.npz (tools/gen_golden.py::gen_rnnt_beam): the
reference class's tokens on utterances where it agrees with the float64 restatement
(tests/rnnt_beam_restatement.py) and every decision of the search has a margin of at least 16 N,
N = the reference's own fp32 score noise of the configuration.  Bounds: tokens and frames exact;
score within 4 N."""

import numpy as np
import pytest
import torch

import rnnt_beam_restatement as R
from decode_support import _beam_modules, _fixture, _fixture_free_config, _long_input, _search, _tokenizer
from task_support import _pcm_batch, _pruned_beam_cfg


def _params(c):
    return {k: c[k] for k in R.PARAM_KEYS}


class _PlainPredictor:
    """Stateless predictor from the fixture's arrays, plain torch; only init_state / streaming_step."""

    def __init__(self, c, dev="cpu"):
        self.ctx = c["ctx"]
        self.emb, self.conv_w, self.lin_w, self.lin_b = (
            torch.from_numpy(c[k]).to(dev) for k in ("emb", "conv_w", "lin_w", "lin_b"))

    def init_state(self):
        return torch.zeros((1, self.ctx - 1), dtype=torch.int64, device=self.emb.device)

    def streaming_step(self, input, state):
        ctxed = torch.cat([state, input], dim=1)                             # (1, ctx)
        e = (self.emb[ctxed[0]].t() * self.conv_w).sum(dim=1)                # (E)
        out = torch.nn.functional.linear(e, self.lin_w, self.lin_b)
        return out.reshape(1, 1, -1), ctxed[:, 1:]


class _PlainJoiner:
    def __init__(self, c, dev="cpu"):
        self.act = torch.relu if c["act"] == "relu" else torch.tanh
        self.enc_w, self.enc_b, self.pre_w, self.pre_b = (
            torch.from_numpy(c[k]).to(dev) for k in ("enc_w", "enc_b", "pre_w", "pre_b"))

    def streaming_step(self, encoder_out, predictor_out):
        am = torch.nn.functional.linear(encoder_out, self.enc_w, self.enc_b)         # (1,1,V)
        lm = torch.nn.functional.linear(predictor_out, self.pre_w, self.pre_b)       # (beam,1,V)
        return self.act(am + lm).log_softmax(dim=-1).squeeze(1)


# ---------------------------------------------------------------------------------------- CPU

def test_restatement_reproduces_the_reference_tokens(golden_dir):
    fx = _fixture(golden_dir)
    assert len(fx) == 5
    for c in fx:
        assert len(c["tokens"]) == 8
        assert 0 < sum(len(t) for t in c["tokens"]) < int(c["lengths"].sum())   # tokens and blanks
        for b in range(8):
            n = int(c["lengths"][b])
            tok, score, frames, margin = R.beam_search(c["am"][b, :n], _params(c), c["ctx"], c["act"],
                                                       c["beam"], c["topk"])
            assert tok == c["tokens"][b] and frames == c["frames"][b], (c["V"], b)
            assert score == pytest.approx(c["score_f64"][b], abs=1e-9)
            assert margin >= 16 * c["N"]
            assert abs(c["score_ref_f32"][b] - c["score_f64"][b]) <= c["N"]
    assert int(fx[0]["lengths"].max()) >= 200


def test_module_loop_on_plain_torch_stand_ins(golden_dir):
    from speech2text_amd.model.decoding import RnntBeamDecoding
    checked = 0
    for c in _fixture(golden_dir):
        if c["V"] != 40:
            continue
        sess = RnntBeamDecoding(_tokenizer(40), _PlainPredictor(c), _PlainJoiner(c),
                                beam_size=c["beam"], cutoff_top_k=c["topk"])
        assert not sess._fusable()
        enc, lens = torch.from_numpy(c["enc"]), torch.from_numpy(c["lengths"])
        tokens, frames, out_len, score = sess.beam_tokens(enc, lens)
        for b in range(8):
            n = int(out_len[b])
            assert tokens[b, :n].tolist() == c["tokens"][b], (c["act"], c["ctx"], b)
            assert frames[b, :n].tolist() == c["frames"][b]
            assert abs(float(score[b]) - c["score_f64"][b]) <= 4 * c["N"]
        texts = sess.decode_batch(enc, lens)
        assert texts[1] == sess._tokenizer.decode(torch.tensor(c["tokens"][1]))
        assert sess.decode(enc[1:2, :int(lens[1])]) == texts[1]
        checked += 1
    assert checked == 3


def test_factory_and_metric_config():
    from speech2text_amd.model import decoding as Dm
    from speech2text_amd.model.utils import AsrMetric, AsrMetricConfig
    assert Dm.DecodingFactory["rnnt_beam_decoding"].value is Dm.RnntBeamDecoding
    assert [m.name for m in Dm.DecodingFactory] == ["ctc_greedy_decoding", "rnnt_greedy_decoding",
                                                    "rnnt_beam_decoding"]
    assert Dm.DecodingFactory["ctc_greedy_decoding"].value is Dm.CtcGreedyDecoding
    assert Dm.DecodingFactory["rnnt_greedy_decoding"].value is Dm.RnntGreedyDecoding
    assert (AsrMetricConfig().decode_method, AsrMetricConfig().beam_size,
            AsrMetricConfig().cutoff_top_k) == ("ctc_greedy_search", 4, 4)
    cfg = AsrMetricConfig(decode_method="rnnt_beam_search", beam_size=2, cutoff_top_k=3)
    c = _fixture_free_config()
    metric = AsrMetric(_tokenizer(40), cfg, predictor=_PlainPredictor(c), joiner=_PlainJoiner(c))
    sess = metric._decode_sess
    assert isinstance(sess, Dm.RnntBeamDecoding) and (sess._beam_size, sess._cutoff_top_k) == (2, 3)
    with pytest.raises(NotImplementedError):
        AsrMetric(_tokenizer(40), AsrMetricConfig(decode_method="ctc_lexicon_beam_search"))


def test_long_input_emits_on_both_sides_of_the_trace_blocks(golden_dir):
    """What tests/test_gpu_rnnt_stream_search.py::test_long_chunks_cross_the_trace_blocks relies on, by
    the float64 restatement: at beam 4 / top-k 4 the best beam of row 0 (90 frames: blocks [26, 90)
    and [0, 26)) has a token at a frame < 26 and one at a frame >= 64."""
    c = _fixture(golden_dir)[0]
    am, lens = _long_input(c)
    assert int(lens[0]) == 90
    _, _, frames, _ = R.beam_search(am[0].numpy(), _params(c), c["ctx"], c["act"], 4, 4)
    assert min(frames) < 26 and max(frames) >= 64, frames


def test_workspace_size_is_a_pure_host_function():
    from speech2text_amd import _native as N
    lib = N.lib()
    n = lib.s2t_rnnt_beam_workspace_bytes(3, 50, 500, 16)
    assert n >= 4 * 3 * 50 * 16 + 4 * 3 * 16 * 500 and n % 256 == 0     # records + spilled lm rows
    assert lib.s2t_rnnt_beam_workspace_bytes(0, 50, 500, 16) == 0


# ---------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
def test_fused_search_is_exact_on_every_stored_utterance(dev, golden_dir):
    """Checks 1 and 2: a whole configuration per launch; tokens == the reference class's, frames ==
    the float64 restatement's, |score - float64 score| <= 4 N, every utterance."""
    for ci, c in enumerate(_fixture(golden_dir)):
        tokens, frames, out_len, score = _search(c, c["am"], c["lengths"], dev)
        for b in range(8):
            n = int(out_len[b])
            err = abs(float(score[b]) - c["score_f64"][b])
            print(f"config {ci} utt {b}: T {int(c['lengths'][b])} tokens {n} |score err| {err:.2e} "
                  f"(4N = {4 * c['N']:.2e})")
            assert tokens[b, :n].tolist() == c["tokens"][b], (ci, b)
            assert frames[b, :n].tolist() == c["frames"][b], (ci, b)
            assert err <= 4 * c["N"], (ci, b)


def _greedy_from_am(c, am, lens, dev):
    """s2t_rnnt_greedy_stateless on a given am with max_token_step = 0 (one symbol per frame)."""
    from speech2text_amd import _native as N
    pred, join = _beam_modules(c, dev)
    p = pred.predictor
    am = torch.as_tensor(am).to(dev).contiguous()
    B, T, V = am.shape
    lens = torch.as_tensor(lens).to(device=dev, dtype=torch.int64)
    tokens = torch.zeros((B, T), dtype=torch.int64, device=dev)
    out_len = torch.zeros((B,), dtype=torch.int64, device=dev)
    N.check(N.lib().s2t_rnnt_greedy_stateless(
        N.fp(am), N.lp(lens), N.fp(p._embedding.weight), N.fp(p._conv.weight.reshape(c["E"], c["ctx"]).contiguous()),
        N.fp(p._output_linear.weight), N.fp(p._output_linear.bias), N.fp(join._pre_proj.weight),
        N.fp(join._pre_proj.bias), B, T, V, c["E"], c["D"], c["ctx"], 0 if c["act"] == "relu" else 1,
        0, T, 0, N.lp(tokens), N.lp(out_len), N.stream()), "s2t_rnnt_greedy_stateless")
    torch.cuda.synchronize()
    return tokens.cpu(), out_len.cpu()


@pytest.mark.gpu
def test_degenerate_beam_equals_the_greedy_kernel(dev, golden_dir):
    """Check 3: beam_size = cutoff_top_k = 1 is the greedy walk at max_token_step = 0.  Bit for bit."""
    c = _fixture(golden_dir)[0]
    g = torch.Generator().manual_seed(17)
    rand_am = torch.randn(64, 90, c["V"], generator=g) * 3.0
    rand_lens = torch.randint(1, 91, (64,), generator=g)
    rand_lens[0] = 90
    for am, lens in ((c["am"], c["lengths"]), (rand_am, rand_lens)):
        gt, gn = _greedy_from_am(c, am, lens, dev)
        tokens, frames, out_len, _ = _search(c, am, lens, dev, beam=1, topk=1)
        assert out_len.tolist() == gn.tolist()
        assert int(gn.sum()) > 0 and int(gn.sum()) < int(torch.as_tensor(lens).sum())
        for b in range(tokens.shape[0]):
            n = int(gn[b])
            assert tokens[b, :n].tolist() == gt[b, :n].tolist(), b
            assert frames[b, :n].tolist() == sorted(set(frames[b, :n].tolist()))   # one per frame


def _decidable(c, am_dev, lens):
    """Restatement in float64 on the DEVICE's am: (tokens, margin >= 16 N) per utterance."""
    rows = []
    for b in range(am_dev.shape[0]):
        tok, _, _, margin = R.beam_search(am_dev[b, :int(lens[b])].numpy(), _params(c), c["ctx"],
                                          c["act"], c["beam"], c["topk"])
        rows.append((tok, margin >= 16 * c["N"]))
    return rows


@pytest.mark.gpu
def test_through_the_class(dev, golden_dir):
    """Check 4: product Predictor / Joiner with the V = 40 relu weights; the GEMM behind
    joiner._enc_proj moves am a little, so the answer is the restatement on the device's own am,
    for the utterances that keep the fixture's 16 N margin there (at most 1 of 8 may drop out)."""
    from speech2text_amd.model.decoding import RnntBeamDecoding, batch_search
    c = _fixture(golden_dir)[1]
    assert (c["V"], c["act"], c["ctx"]) == (40, "relu", 5)
    pred, join = _beam_modules(c, dev)
    tok = _tokenizer(40)
    sess = RnntBeamDecoding(tok, pred, join, beam_size=c["beam"], cutoff_top_k=c["topk"])
    assert sess._fusable()
    enc, lens = torch.from_numpy(c["enc"]).to(dev), torch.from_numpy(c["lengths"])
    with torch.no_grad():
        am_dev = join._enc_proj(enc).float().cpu()
    texts = sess.decode_batch(enc, lens)
    rows = _decidable(c, am_dev, lens)
    left_out = [b for b, (_, ok) in enumerate(rows) if not ok]
    print("left out (margin below 16 N on the device's am):", left_out)
    assert len(left_out) <= 1
    for b, (ref, ok) in enumerate(rows):
        if ok:
            assert texts[b] == tok.decode(torch.tensor(ref, dtype=torch.int64)), b
    for b in range(8):
        assert sess.decode(enc[b:b + 1, :int(lens[b])]) == texts[b], b
    assert batch_search(enc, lens, sess) == texts


@pytest.mark.gpu
def test_ragged_and_edge_cases(dev, golden_dir):
    """Check 5, first half: lengths [T, 1, 0] with beam_size = 16 on V = 500 in one launch;
    cutoff_top_k > V behaves as V; beam_size = 0 is refused with -1."""
    from speech2text_amd import _native as N
    c = _fixture(golden_dir)[4]
    assert (c["V"], c["beam"]) == (500, 16) and int(c["lengths"][0]) == c["Tmax"]
    lens = np.array([c["Tmax"], 1, 0], dtype=np.int64)
    tokens, frames, out_len, score = _search(c, c["am"][:3], lens, dev)
    assert tokens[0, :int(out_len[0])].tolist() == c["tokens"][0]
    assert frames[0, :int(out_len[0])].tolist() == c["frames"][0]
    assert abs(float(score[0]) - c["score_f64"][0]) <= 4 * c["N"]
    tok1, score1, frames1, margin1 = R.beam_search(c["am"][1, :1], _params(c), c["ctx"], c["act"],
                                                   c["beam"], c["topk"])
    assert margin1 >= 16 * c["N"]                       # (a property of the fixture: decidable)
    assert tokens[1, :int(out_len[1])].tolist() == tok1 and frames[1, :int(out_len[1])].tolist() == frames1
    assert abs(float(score[1]) - score1) <= 4 * c["N"]
    assert int(out_len[2]) == 0 and float(score[2]) == 0.0

    # cutoff_top_k above V: a tiny vocabulary (min(cutoff_top_k, V) must stay within 16)
    s = _fixture_free_config(V=8, D=16, E=12, ctx=2, seed=9, scale=3.0)
    s.update(beam=4, topk=8)
    g = torch.Generator().manual_seed(3)
    am = torch.randn(3, 12, 8, generator=g) * 2.0
    lens = np.array([12, 1, 0], dtype=np.int64)
    at_v = _search(s, am, lens, dev, topk=8)
    above = _search(s, am, lens, dev, topk=20)
    for x, y in zip(at_v, above):
        assert torch.equal(x, y)
    assert int(at_v[2][0]) > 0
    for b in range(2):
        tok_b, score_b, frames_b, margin_b = R.beam_search(am[b, :int(lens[b])].numpy(), _params(s), 2,
                                                           "relu", 4, 20)
        if margin_b >= 1e-4:        # fp32 noise of a 12-frame score is ~1e-6: a decidable utterance
            n = int(above[2][b])
            assert above[0][b, :n].tolist() == tok_b and above[1][b, :n].tolist() == frames_b
            assert abs(float(above[3][b]) - score_b) <= 1e-4

    pred, join = _beam_modules(s, dev)
    p = pred.predictor
    amd = am.to(dev).contiguous()
    ld = torch.as_tensor(lens).to(dev)
    out = [torch.zeros((3, 12), dtype=torch.int64, device=dev) for _ in range(2)]
    n_out = torch.zeros((3,), dtype=torch.int64, device=dev)
    sc = torch.zeros((3,), dtype=torch.float32, device=dev)
    ws = torch.empty((max(256, N.lib().s2t_rnnt_beam_workspace_bytes(3, 12, 8, 4)),), dtype=torch.uint8, device=dev)
    rc = N.lib().s2t_rnnt_beam_stateless(
        N.fp(amd), N.lp(ld), N.fp(p._embedding.weight), N.fp(p._conv.weight.reshape(12, 2).contiguous()),
        N.fp(p._output_linear.weight), N.fp(p._output_linear.bias), N.fp(join._pre_proj.weight),
        N.fp(join._pre_proj.bias), 3, 12, 8, 12, 16, 2, 0, 0, 0, 4, N.ptr(ws), N.lp(out[0]),
        N.lp(out[1]), N.lp(n_out), N.fp(sc), N.stream())
    assert rc == -1


@pytest.mark.gpu
def test_large_vocabulary_keeps_lm_rows_in_the_workspace(dev):
    """V = 1024 at beam 16: lm [16][1024] does not fit the LDS next to the rest, so the rows live
    in the workspace, and the classes are re-read per selection round instead of held in registers.
    Answer: the float64 restatement on the same am.  Floor of the decision margin 1e-3 (a
    property of this seeded input, asserted): fp32 rounding of a log-probability of magnitude
    <= 10 is ~1e-6 per frame, ~2e-5 over the 24 frames; the score is held to 1e-4 likewise."""
    s = _fixture_free_config(V=1024, D=32, E=24, ctx=3, seed=21, scale=3.0)
    s.update(beam=16, topk=4)
    g = torch.Generator().manual_seed(4)
    am = torch.randn(4, 24, 1024, generator=g) * 2.0
    lens = np.array([24, 17, 5, 1], dtype=np.int64)
    tokens, frames, out_len, score = _search(s, am, lens, dev)
    for b in range(4):
        tok, sc, frm, margin = R.beam_search(am[b, :int(lens[b])].numpy(), _params(s), 3, "relu", 16, 4)
        assert margin >= 1e-3 and len(tok) > 0
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == tok and frames[b, :n].tolist() == frm, b
        assert abs(float(score[b]) - sc) <= 1e-4


@pytest.mark.gpu
def test_module_loop_on_the_device_gives_the_fused_tokens(dev, golden_dir):
    """Check 5, second half: `fused=False` runs the module loop on the device (V = 40, ctx = 2,
    beam 8 / top-k 3).  Its per-frame products need not round like the batched one, so the
    comparison holds for the utterances with the 16 N margin on the device's am (at most 1 of 8
    left out)."""
    from speech2text_amd.model.decoding import RnntBeamDecoding
    c = _fixture(golden_dir)[3]
    assert (c["V"], c["ctx"], c["beam"], c["topk"]) == (40, 2, 8, 3)
    pred, join = _beam_modules(c, dev)
    sess = RnntBeamDecoding(_tokenizer(40), pred, join, beam_size=8, cutoff_top_k=3)
    enc, lens = torch.from_numpy(c["enc"]).to(dev), torch.from_numpy(c["lengths"])
    with torch.no_grad():
        am_dev = join._enc_proj(enc).float().cpu()
    fused = [x.cpu() for x in sess.beam_tokens(enc, lens)]
    loop = [x.cpu() for x in sess.beam_tokens(enc, lens, fused=False)]
    rows = _decidable(c, am_dev, lens)
    left_out = [b for b, (_, ok) in enumerate(rows) if not ok]
    print("left out (margin below 16 N on the device's am):", left_out)
    assert len(left_out) <= 1
    for b, (ref, ok) in enumerate(rows):
        if ok:
            n = int(fused[2][b])
            assert int(loop[2][b]) == n
            assert loop[0][b, :n].tolist() == fused[0][b, :n].tolist() == ref, b
            assert loop[1][b, :n].tolist() == fused[1][b, :n].tolist(), b


@pytest.mark.gpu
def test_validation_step_reports_beam_wer(dev):
    """Check 6: AsrMetric with rnnt_beam_search inside a task's validation_step."""
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.model.decoding import RnntBeamDecoding, reference_decoder
    from speech2text_amd.model.utils import word_error_rate
    V = 32
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(_pruned_beam_cfg(V)).to(dev)
    task.eval()
    with torch.no_grad():
        for p in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            p.mul_(3.0)
    sess = task._metric._decode_sess
    assert isinstance(sess, RnntBeamDecoding) and (sess._beam_size, sess._cutoff_top_k) == (3, 2)
    assert sess._fusable()
    batch = _pcm_batch(dev, V=V)
    info = task.validation_step(batch, 0)
    assert "wer" in task.logged and np.isfinite(float(info["val_loss"]))
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
        dec, dl = task._decoder(enc, el)
    hyps = sess.decode_batch(dec, dl)
    assert any(len(h) for h in hyps)
    refs = reference_decoder(batch["label"], task._tokenizer)
    assert info["wer"] == pytest.approx(word_error_rate(hyps, refs, show_on_screen=False))
