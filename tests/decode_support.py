"""Module builders and chunk drivers shared by the decoding tests.

Test infrastructure (not a test file): what one decoding test module used to take from another.  The
LSTM, the stateless and the fixture-driven builders keep distinct names (_lstm_*, _stateless_*,
_beam_modules); the case caches are one per process, as they were through the import.  Task and
configuration builders are in tests/task_support.py.

pytest rewrites `assert` only in test_*.py, so every assertion here carries its values in its message.
"""
import ctypes
import functools
import os

import numpy as np
import torch

import rnnt_beam_restatement as R
import rnnt_lstm_search_cases as C
import rnnt_ngram_cases as NC


# ------------------------------------------------------------------ tokenizers and the library
class _Tok:
    """Token ids -> text, one word per id (the decoders only call decode)."""
    labels = []

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def _lib():
    """-> (the native module, the library), for host-side checks that need no device."""
    from speech2text_amd import _native as N
    return N, N.lib()


def _tokenizer(V):
    from speech2text_amd.dataset.utils import TokenizerSetup
    return TokenizerSetup({"type": "char", "config": {"labels": [chr(97 + i) for i in range(V - 3)]}})


# ------------------------------------------------------------------ stateless predictor, the reference's fixture
@functools.lru_cache(maxsize=None)
def _fixture(golden_dir):
    return R.load_fixture(golden_dir)


def _long_input(c):
    """Rows 0-7 of the seeded 64 x 90 input of test_degenerate_beam_equals_the_greedy_kernel (row 0 has
    90 frames): longer than one 64-frame block of the staged trace-back (csrc/decode_records.h)."""
    g = torch.Generator().manual_seed(17)
    am = torch.randn(64, 90, c["V"], generator=g) * 3.0
    lens = torch.randint(1, 91, (64,), generator=g)
    lens[0] = 90
    return am[:8].contiguous(), lens[:8].numpy()


def _fixture_free_config(V=40, D=48, E=32, ctx=3, act="relu", seed=5, scale=1.0):
    g = np.random.default_rng(seed)
    c = {"V": V, "D": D, "E": E, "ctx": ctx, "act": act}
    for k, shape in (("emb", (V, E)), ("conv_w", (E, ctx)), ("lin_w", (D, E)), ("lin_b", (D,)),
                     ("pre_w", (V, D)), ("pre_b", (V,)), ("enc_w", (V, D)), ("enc_b", (V,))):
        c[k] = (g.standard_normal(shape) * scale / np.sqrt(shape[-1])).astype(np.float32)
    return c


def _beam_modules(c, dev):
    """Product Predictor / Joiner carrying a configuration's weights."""
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    pred = Predictor({"model": "Stateless", "config": {
        "num_symbols": c["V"], "output_dim": c["D"], "symbol_embedding_dim": c["E"],
        "context_size": c["ctx"]}})
    join = Joiner(JoinerConfig(input_dim=c["D"], output_dim=c["V"], activation=c["act"],
                               prune_range=5, use_out_project=False))
    p = pred.predictor
    with torch.no_grad():
        p._embedding.weight.copy_(torch.from_numpy(c["emb"]))
        p._conv.weight.copy_(torch.from_numpy(c["conv_w"]).reshape(c["E"], 1, c["ctx"]))
        p._output_linear.weight.copy_(torch.from_numpy(c["lin_w"]))
        p._output_linear.bias.copy_(torch.from_numpy(c["lin_b"]))
        join._pre_proj.weight.copy_(torch.from_numpy(c["pre_w"]))
        join._pre_proj.bias.copy_(torch.from_numpy(c["pre_b"]))
        if "enc_w" in c:
            join._enc_proj.weight.copy_(torch.from_numpy(c["enc_w"]))
            join._enc_proj.bias.copy_(torch.from_numpy(c["enc_b"]))
    return pred.to(dev), join.to(dev)


def _search(c, am, lens, dev, beam=None, topk=None):
    from speech2text_amd.model.decoding import rnnt_beam_tokens_from_am
    pred, join = _beam_modules(c, dev)
    out = rnnt_beam_tokens_from_am(torch.as_tensor(am).to(dev), torch.as_tensor(lens), pred, join,
                                   c["beam"] if beam is None else beam,
                                   c["topk"] if topk is None else topk)
    assert out is not None, "the fused search refused a shape it must take"
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


# ------------------------------------------------------------------ LSTM predictor, rnnt_lstm_search_cases
_TINY = dict(V=16, E=8, H=8, D=8, L=1, ln=True, inner=0, act="relu")


def _lstm_build(dev, V, E, H, D, L, ln, inner, act):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    torch.manual_seed(V + H)
    p = Predictor({"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": D, "symbol_embedding_dim": E, "num_lstm_layers": L,
        "lstm_hidden_dim": H, "lstm_layer_norm": ln, "lstm_layer_norm_epsilon": C.EPS_LSTM, "lstm_dropout": 0.0}})
    j = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=inner or 8, activation=act,
                            use_out_project=bool(inner)))
    j._enc_proj = torch.nn.Identity()                     # the searches are handed am itself
    return p.to(dev).eval(), j.to(dev).eval()


def _lstm_modules(dev, w, model):
    """The project's LstmPredictor + Joiner holding the weights `w` of MODELS[model]."""
    m = C.MODELS[model]
    p, j = _lstm_build(dev, m["V"], m["E"], m["H"], m["D"], m["L"], m["ln"], m["inner"], m["act"])
    q = p.predictor._predictor
    with torch.no_grad():
        for dst, src in ((q.embedding.weight, "emb"), (q.input_layer_norm.weight, "in_g"),
                         (q.input_layer_norm.bias, "in_b"), (q.linear.weight, "lin_w"),
                         (q.linear.bias, "lin_b"), (q.output_layer_norm.weight, "out_g"),
                         (q.output_layer_norm.bias, "out_b"), (j._pre_proj.weight, "pre_w"),
                         (j._pre_proj.bias, "pre_b")):
            dst.copy_(w[src])
        for lstm, lw in zip(q.lstm_layers, w["layers"]):
            lstm.x2g.weight.copy_(lw["x2g_w"])
            lstm.p2g.weight.copy_(lw["wp"])
            if m["ln"]:
                for mod, a, b in ((lstm.g_norm, "gg", "gb"), (lstm.c_norm, "cg", "cb")):
                    mod.weight.copy_(lw[a])
                    mod.bias.copy_(lw[b])
            else:
                lstm.x2g.bias.copy_(lw["x2g_b"])
        if m["inner"]:
            for lin, a, b in ((j._out_projection[0], "o1_w", "o1_b"), (j._out_projection[1], "o2_w", "o2_b")):
                lin.weight.copy_(w[a])
                lin.bias.copy_(w[b])
    assert q.input_layer_norm.eps == C.EPS_IN and q.output_layer_norm.eps == C.EPS_OUT, \
        f"layer norm eps {q.input_layer_norm.eps} / {q.output_layer_norm.eps}, the cases' {C.EPS_IN} / {C.EPS_OUT}"
    return p, j


def _weights_of(p, j):
    """The restatement's weights (float64, CPU) of a task's modules."""
    q = p.predictor._predictor
    t = lambda x: None if x is None else x.detach().double().cpu()      # noqa: E731
    ln = isinstance(q.lstm_layers[0].g_norm, torch.nn.LayerNorm)
    w = dict(emb=t(q.embedding.weight), in_g=t(q.input_layer_norm.weight), in_b=t(q.input_layer_norm.bias),
             lin_w=t(q.linear.weight), lin_b=t(q.linear.bias), out_g=t(q.output_layer_norm.weight),
             out_b=t(q.output_layer_norm.bias), pre_w=t(j._pre_proj.weight), pre_b=t(j._pre_proj.bias),
             eps_in=q.input_layer_norm.eps, eps_out=q.output_layer_norm.eps,
             eps_lstm=q.lstm_layers[0].g_norm.eps if ln else 0.0, layers=[])
    for m in q.lstm_layers:
        lw = dict(x2g_w=t(m.x2g.weight), wp=t(m.p2g.weight))
        if ln:
            lw.update(gg=t(m.g_norm.weight), gb=t(m.g_norm.bias), cg=t(m.c_norm.weight), cb=t(m.c_norm.bias))
        else:
            lw["x2g_b"] = t(m.x2g.bias)
        w["layers"].append(lw)
    if j._use_out_project:
        w.update(o1_w=t(j._out_projection[0].weight), o1_b=t(j._out_projection[0].bias),
                 o2_w=t(j._out_projection[1].weight), o2_b=t(j._out_projection[1].bias))
    return w


_LSTM_CASES = {}


def _lstm_case(dev, name):
    """(case, modules, am and lengths on the device, the float64 results), built once per case."""
    if name not in _LSTM_CASES:
        c = C.CASES[name]
        w, act, am, lens = C.make(name)
        p, j = _lstm_modules(dev, w, c["model"])
        _LSTM_CASES[name] = (c, p, j, am.to(dev), lens.to(dev), C.reference(name))
    return _LSTM_CASES[name]


# ------------------------------------------------------------------ stateless predictor, rnnt_stateless_lm_cases
def _stateless_build(dev, V, E, D, ctx, inner=0, act="relu"):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D, "symbol_embedding_dim": E,
                                                       "context_size": ctx}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=max(inner, 1), activation=act, prune_range=5,
                               use_out_project=inner > 0))
    join._enc_proj = torch.nn.Identity()                   # the searches are handed am itself
    return pred.to(dev).eval().requires_grad_(False), join.to(dev).eval().requires_grad_(False)


def _stateless_modules(dev, p, c):
    """The project's Predictor / Joiner on the device carrying the weights `p` of a case."""
    pred, join = _stateless_build(dev, c["V"], c["E"], c["D"], c["ctx"], c["inner"], c["act"])
    q = pred.predictor
    with torch.no_grad():
        q._embedding.weight.copy_(p["emb"])
        q._conv.weight.copy_(p["conv_w"].reshape(c["E"], 1, c["ctx"]))
        q._output_linear.weight.copy_(p["lin_w"])
        q._output_linear.bias.copy_(p["lin_b"])
        join._pre_proj.weight.copy_(p["pre_w"])
        join._pre_proj.bias.copy_(p["pre_b"])
        if c["inner"]:
            o1, o2 = join._out_projection[0], join._out_projection[1]
            o1.weight.copy_(p["o1_w"])
            o1.bias.copy_(p["o1_b"])
            o2.weight.copy_(p["o2_w"])
            o2.bias.copy_(p["o2_b"])
    return pred, join


# ------------------------------------------------------------------ language models
def _lm_module(dev, sd=None, V=None, H=None, layers=None):
    """The project's RnnLm on the device, holding the state dict `sd` when given."""
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    if sd is not None:
        V, H = sd["_embedding.weight"].shape
        layers = sum(1 for k in sd if "weight_hh_l" in k)
    with torch.device(dev):
        lm = RnnLm(RnnLmConfig(num_symbols=V, symbol_embedding_dim=H, num_rnn_layer=layers))
    if sd is not None:
        lm.load_state_dict(sd, strict=True)
    return lm.to(dev).eval().requires_grad_(False)


_NGRAM_LMS, _NGRAM_CASES = {}, {}


def _ngram_lm(dev, text, V):
    """The NgramLm of an ARPA text on the device, built once per (text, V) and process."""
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    if (text, V) not in _NGRAM_LMS:
        _NGRAM_LMS[text, V] = NgramLm.from_arpa(text, num_classes=V).to(dev)
    return _NGRAM_LMS[text, V]


def _lm_on(dev, name):
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.from_arpa(NC.text_of(name), num_classes=NC.CASES[name]["V"]).to(dev)


def _ngram_case(dev, name):
    """(case, predictor, joiner, NgramLm, am and lengths on the device, the float64 results), once per case."""
    if name not in _NGRAM_CASES:
        c = NC.CASES[name]
        _, am, lens = NC.make(name)
        pred, join = NC.modules(dev, name)
        _NGRAM_CASES[name] = (c, pred, join, _lm_on(dev, name), am.to(dev), lens.to(dev), NC.reference(name))
    return _NGRAM_CASES[name]


def _fused(c, p, j, lm, am, lens, **kw):
    from speech2text_amd.model.decoding import rnnt_beam_ngram_tokens_from_am
    args = dict(lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"])
    args.update(kw)
    return rnnt_beam_ngram_tokens_from_am(am, lens, p, j, lm, **args)


def _bad_desc(lm, **change):
    from speech2text_amd import _native as N
    d = N.struct("S2tNgramLmDesc")()
    src = lm._cache["desc"]
    for f, _ in d._fields_:
        setattr(d, f, getattr(src, f))
    for k, v in change.items():
        setattr(d, k, v)
    return ctypes.byref(d), d


def _decoder(c, p, j, lm, **kw):
    """RnntBeamDecoding with the RNN-LM `lm` fused at the settings of case `c`."""
    from speech2text_amd.model.decoding import RnntBeamDecoding
    args = dict(beam_size=c["beam"], cutoff_top_k=c["topk"], lm=lm, lm_weight=c["weight"], lm_start_token=c["start"])
    args.update(kw)
    return RnntBeamDecoding(_Tok(), p, j, **args)


# ------------------------------------------------------------------ chunk plans and drivers
def _regular(lens, step):
    """Every row in `step`-frame chunks: rows that ended idle (chunk_len 0) while longer ones go on."""
    lens = np.asarray(lens, dtype=np.int64)
    K = -(-int(lens.max()) // step)
    return [np.clip(lens - k * step, 0, step) for k in range(K)]


def _irregular(lens, seed):
    """The plan of test_gpu_rnnt_stream_search._irregular (sizes 0..16 from a seeded generator, different
    per row, one call that idles every row) for any batch, one row included."""
    g = np.random.default_rng(seed)
    rows = []
    for n in np.asarray(lens).tolist():
        sizes, left = [], n
        while left > 0:
            s = min(int(g.choice([0, 0, 1, 1, 2, 3, 5, 7, 11, 16])), left)
            sizes.append(s)
            left -= s
        rows.append(sizes)
    K = max(1, max(len(r) for r in rows))
    plan = [np.array([r[k] if k < len(r) else 0 for r in rows], dtype=np.int64) for k in range(K)]
    plan.insert(K // 2, np.zeros(len(rows), dtype=np.int64))
    return plan


def _plan(lens, name, seed=0):
    return _irregular(lens, 100 + seed) if name == "irregular" else _regular(lens, int(name))


def _feed(search, am_dev, plan, snap=None, off=None):
    """am_dev (B, T, V) on the device; plan: per call the frames each row takes.  Row b's chunk is
    am[b, off[b] : off[b] + plan[k][b]] at the front of a (B, max(plan[k]), V) tensor."""
    B, T, V = am_dev.shape
    dev = am_dev.device
    off = np.zeros(B, dtype=np.int64) if off is None else off
    rows = torch.arange(B, device=dev).unsqueeze(1)
    out = None
    for cl in plan:
        Tc = max(1, int(cl.max()))
        idx = (torch.as_tensor(off, device=dev).unsqueeze(1) + torch.arange(Tc, device=dev)).clamp(max=T - 1)
        out = search.step(am_dev[rows, idx].contiguous(), torch.as_tensor(cl, dtype=torch.int64).to(dev))
        off += cl
        if snap is not None:
            snap(off.copy(), [x.cpu().clone() for x in out])
    torch.cuda.synchronize()
    return [x.cpu().clone() for x in out], off


def _same_rows(got, want, rows=None):
    """Stream outputs (tokens, frames, out_len, score[, stable_len]) against the whole-utterance
    search's (tokens, frames, out_len, score): bit for bit on the valid part of every row."""
    tokens, frames, out_len, score = got[:4]
    rows = range(len(out_len)) if rows is None else rows
    for b in rows:
        n = int(want[2][b])
        assert int(out_len[b]) == n, f"row {b}: {int(out_len[b])} tokens against {n}"
        assert torch.equal(tokens[b, :n], want[0][b, :n]), \
            f"row {b}: tokens {tokens[b, :n].tolist()} against {want[0][b, :n].tolist()}"
        assert torch.equal(frames[b, :n], want[1][b, :n]), \
            f"row {b}: frames {frames[b, :n].tolist()} against {want[1][b, :n].tolist()}"
        assert torch.equal(score[b], want[3][b]), f"row {b}: score {float(score[b])!r} against {float(want[3][b])!r}"


# ------------------------------------------------------------------ the recognisers' encoders and predictors
TINY = dict(feature_dim=80, downsampling_factor=(1, 2, 4), num_encoder_layers=(1, 1, 1),
            feedforward_dim=(64, 96, 96), encoder_dim=(32, 48, 48), encoder_unmasked_dim=(24, 32, 32),
            num_heads=(4, 4, 4), query_head_dim=(8,), value_head_dim=(4,), pos_head_dim=(4,),
            pos_dim=16, cnn_module_kernel=(7, 5, 5), causal=True)


def _tiny_stream_encoder(golden_dir, dev):
    from speech2text_amd.model.encoder.zipformer import Zipformer2, Zipformer2Config
    g = np.load(os.path.join(golden_dir, "zipformer_tiny_stream.npz"))
    chunk, left = int(g["chunk"]), int(g["left"])
    m = Zipformer2(Zipformer2Config(**TINY, chunk_size=(chunk,), left_context_frames=(left,), for_ctc=False))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and all(k.startswith("_ctc_projection") for k in unexpected), \
        f"missing {missing}, unexpected {unexpected}"
    return g, m.to(dev).eval(), chunk


def _tiny_ctc_encoder(golden_dir, dev):
    from speech2text_amd.model.encoder.zipformer import Zipformer2, Zipformer2Config
    g = np.load(os.path.join(golden_dir, "zipformer_tiny_stream.npz"))
    chunk, left = int(g["chunk"]), int(g["left"])
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    V = sd["_ctc_projection.weight"].shape[0]
    m = Zipformer2(Zipformer2Config(**TINY, chunk_size=(chunk,), left_context_frames=(left,), for_ctc=True,
                                    num_tokens=V))
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():                                  # tokens on some frames, blank on others
        m._ctc_projection.weight.mul_(4.0)
    return g, m.to(dev).eval(), chunk, V


# The tiny random encoder's output hardly moves from frame to frame, so on the fixture's audio a row
# emits at nearly every node (lift <= 14) or only at its first (lift >= 17); 16 sits between for both
# searches: greedy 2 and beam 22 tokens on the 48 frames.
RECOGNIZER_BLANK = 16.0


def _lstm_pair(dev, V, D, seed, blank):
    """An LSTM predictor and a joiner WITH output projection of fresh weights, times 3 (away from
    the near-ties of a fresh model), blank lifted behind the out-projection so that it wins on a
    share of the nodes: tokens on some frames, not on all."""
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    torch.manual_seed(seed)
    pred = Predictor({"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": D, "symbol_embedding_dim": 16, "num_lstm_layers": 2,
        "lstm_hidden_dim": 32, "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=32, activation="relu", use_out_project=True))
    with torch.no_grad():
        for q in list(pred.parameters()) + list(join.parameters()):
            q.mul_(3.0)
        join._out_projection[1].bias[0] += blank
    return pred.to(dev).eval(), join.to(dev).eval()
