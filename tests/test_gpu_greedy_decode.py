"""GPU: the validation-time greedy decoders (csrc/decode.hip) called directly, compared for exact
equality of tokens and counts.

CTC greedy (model.decoding.ctc_greedy_tokens): against a plain loop over the same float32 values
(first index on ties, collapse repeats, drop blanks), at V on either side of the 64 lanes, T off
the 4 waves, lengths 0 / T / above T, blank first and last, frequent exact ties, constant rows,
rows of -inf, repeats separated by a blank, an all-blank utterance.

RNN-T greedy (s2t_rnnt_greedy_stateless through the C ABI, so that blank != 0 and small max_out
are reachable; RnntGreedyDecoding for the wrapper): against a float64 restatement of
oracle.decoding.rnnt_greedy_stateless that takes `blank` and `max_out`.  A float32 GEMV may flip
an argmax that float64 decides by less than rounding, so the seeds below were chosen on the CPU:
at every lattice node the reference visits, the post-activation top-1 beats the runner-up by at
least 1e-3 (a relu tie at exactly 0 among entries whose pre-activations are all below -1e-3
counts as decided, for the first index).  The tests assert that margin for every utterance.
"""
import numpy as np
import pytest
import torch

from decode_support import _Tok

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ CTC
def _ctc_ref(x, length, blank):
    """x (T,V) float32 numpy; np.argmax returns the FIRST maximal index (-inf rows: 0)."""
    T = x.shape[0]
    out, prev = [], blank
    for t in range(max(0, min(int(length), T))):
        p = int(np.argmax(x[t]))
        if (p != prev or prev == blank) and p != blank:
            out.append(p)
        prev = p
    return out


def _ctc_inputs(V, T, B, blank):
    g = torch.Generator().manual_seed(V * 7919 + T * 31 + B)
    x = (torch.randn(B, T, V, generator=g) * 2).mul(10).round().div(10)     # one decimal: ties
    lens = torch.randint(0, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = T + 5                                                     # clamped to T
    sym = [v for v in range(V) if v != blank]
    a, a2 = sym[0], sym[-1]
    if T >= 3:
        x[0, 1, :] = 0.5                              # a constant row: index 0 wins
        x[0, 2, :] = float("-inf")                    # a row of -inf: index 0 wins
    if B > 3:
        x[3, :, blank] = 100.0                        # an all-blank utterance
        lens[3] = T
    if T >= 5:                                        # a a blank a a2: the blank separates repeats
        b = B - 1
        lens[b] = T
        for t, s in enumerate([a, a, blank, a, a2]):
            x[b, t, :] = -5.0
            x[b, t, s] = 5.0
    return x, lens


@pytest.mark.parametrize("blank", ["first", "last"])
@pytest.mark.parametrize("V,T,B", [(2, 1, 3), (63, 3, 4), (64, 4, 5), (65, 5, 33), (500, 127, 6),
                                   (5003, 1501, 2), (2, 1501, 5), (5003, 1, 2), (65, 127, 7),
                                   (63, 5, 5), (64, 127, 3)])
def test_ctc_greedy_tokens_exact(dev, V, T, B, blank):
    from speech2text_amd.model.decoding import ctc_greedy_tokens
    blank = 0 if blank == "first" else V - 1
    x, lens = _ctc_inputs(V, T, B, blank)
    ties = sum(int((x[b, t] == x[b, t].max()).sum() > 1) for b in range(B) for t in range(min(T, 50)))
    if V >= 63 and T >= 3:
        assert ties > 0, "the case holds no exact tie"
    tok, n = ctc_greedy_tokens(x.to(dev), lens.to(dev), blank)
    assert tok.shape == (B, T) and tok.dtype == torch.int64 and n.shape == (B,)
    tok, n = tok.cpu(), n.cpu()
    xn = x.numpy()
    for b in range(B):
        ref = _ctc_ref(xn[b], lens[b], blank)
        assert int(n[b]) == len(ref), (b, int(n[b]), len(ref))
        assert tok[b, :len(ref)].tolist() == ref, b
        assert (tok[b, len(ref):] == 0).all(), "the buffer beyond out_len lost the wrapper's zeros"
    if T >= 5:
        sym = [v for v in range(V) if v != blank]
        want = [sym[0], sym[0]] + ([sym[-1]] if len(sym) > 1 else [])     # (V = 2: a a _ a a -> a a)
        assert tok[B - 1, :len(want)].tolist() == want and int(n[B - 1]) >= len(want)
    if B > 3:
        assert int(n[3]) == 0 and int(n[1]) == 0


def test_ctc_greedy_refuses_more_frames_than_its_buffer(dev):
    """T = 16001 is above the kernel's 16000-entry shared-memory buffer: the entry point returns
    its code before any launch and the wrapper raises, naming the entry point."""
    from speech2text_amd.model.decoding import ctc_greedy_tokens
    x = torch.zeros(1, 16001, 2, device=dev)
    with pytest.raises(RuntimeError, match="s2t_ctc_greedy failed with code -1"):
        ctc_greedy_tokens(x, torch.tensor([16001], device=dev))
    tok, n = ctc_greedy_tokens(x[:, :16000], torch.tensor([16000], device=dev), blank=1)
    assert int(n[0]) == 1 and int(tok[0, 0]) == 0 and int(tok[0, 1:].sum()) == 0


# ------------------------------------------------------------------ RNN-T
MARGIN = 1e-3


def _weights(seed, V, E, D, ctx, scale, blank, act="relu", n_loop=2):
    """float32 CPU weights of a stateless predictor + projection-free joiner.  The embeddings of
    `n_loop` non-blank symbols are biased along the direction that raises their OWN logit when
    they are the newest token of the state, so that once emitted they are emitted again until
    max_token_step forces the frame on (by 6 sigma for relu; to a pre-activation of about 2 for
    tanh, below its saturation, where float64 could no longer tell the top two apart)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                               # noqa: E731
    w = dict(emb=rn(V, E), conv_w=rn(E, ctx) / ctx ** 0.5, lin_w=rn(D, E) / E ** 0.5,
             lin_b=0.1 * rn(D), pre_w=scale * rn(V, D) / D ** 0.5, pre_b=0.1 * scale * rn(V))
    loops = [v for v in range(V) if v != blank][:n_loop]
    for k in loops:
        u = (w["lin_w"].t() @ w["pre_w"][k]) * w["conv_w"][:, -1]
        boost = 6.0 * scale if act == "relu" else 2.0
        w["emb"][k] += boost * u / (u.norm() ** 2 + 1e-12)
    return w, loops


def _rnnt_ref(am, length, w, ctx, act, mts, max_out, blank):
    """float64 walk of one utterance: am (T,V).  -> (tokens, smallest margin over the visited
    nodes, number of times max_token_step forced a frame on while a symbol was winning)."""
    w = {k: v.double() for k, v in w.items()}
    am = am.double()
    T = am.shape[0]
    Tb = max(0, min(int(length), T))

    def lm_of(state):
        e = (w["conv_w"] * w["emb"][state].t()).sum(dim=1)
        return w["pre_w"] @ (w["lin_w"] @ e + w["lin_b"]) + w["pre_b"]

    state = [blank] * ctx
    lm = lm_of(state)
    out, t, nts, margin, forced = [], 0, 0, float("inf"), 0
    while t < Tb:
        pre = am[t] + lm
        if act == "relu" and float(pre.max()) < -MARGIN:
            tok = 0                                   # every entry is exactly 0: the first index
        else:
            post = torch.relu(pre) if act == "relu" else torch.tanh(pre)
            top = torch.topk(post, 2)
            margin = min(margin, float(top.values[0] - top.values[1]))
            tok = int(top.indices[0])
        if tok == blank or nts > mts:
            forced += tok != blank
            t += 1
            nts = 0
        else:
            nts += 1
            out.append(tok)
            state = state[1:] + [tok]
            lm = lm_of(state)
            if len(out) >= max_out:
                break
    return out, margin, forced


def _am(seed, B, T, V, scale, loops, blank):
    g = torch.Generator().manual_seed(seed + 77)
    am = scale * torch.randn(B, T, V, generator=g)
    am[:, :, blank] += scale * 1.3 * (2 * np.log(V)) ** 0.5     # blank wins about every other node
    for b in range(B):                                # a frame that starts a self-loop
        am[b, (b + 1) % T, loops[b % len(loops)]] += 8.0 * scale
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = T + 7
    return am, lens


# name: (seed, V, E, D, ctx, act, max_token_step, max_out or None = T (mts + 1), blank, B, T, scale)
RNNT_CASES = {
    "v2_ctx1": (0, 2, 8, 8, 1, "relu", 5, None, 0, 4, 40, 2.0),
    "v65_ctx2_tanh": (2, 65, 70, 8, 2, "tanh", 1, None, 0, 3, 12, 0.4),
    "v65_blank_last": (0, 65, 8, 70, 5, "relu", 5, None, 64, 4, 23, 2.0),
    "v500_ctx64": (0, 500, 70, 70, 64, "relu", 0, None, 0, 3, 17, 2.0),
    "v500_tanh_blank_mid": (11, 500, 70, 512, 5, "tanh", 5, None, 7, 3, 9, 0.4),
    "v5003_e512": (0, 5003, 512, 512, 2, "relu", 1, None, 0, 3, 13, 2.0),
    "v5003_blank_last": (0, 5003, 70, 512, 1, "relu", 5, None, 5002, 2, 10, 2.0),
    "v65_buffer_fills": (0, 65, 70, 70, 2, "relu", 1, 5, 0, 4, 20, 2.0),
}


def _reference_of(name):
    seed, V, E, D, ctx, act, mts, max_out, blank, B, T, scale = RNNT_CASES[name]
    w, loops = _weights(seed, V, E, D, ctx, scale, blank, act)
    am, lens = _am(seed, B, T, V, scale, loops, blank)
    max_out = T * (mts + 1) if max_out is None else max_out
    refs = [_rnnt_ref(am[b], lens[b], w, ctx, act, mts, max_out, blank) for b in range(B)]
    return w, am, lens, max_out, refs


@pytest.mark.parametrize("name", list(RNNT_CASES))
def test_rnnt_greedy_kernel_exact(dev, name):
    from speech2text_amd import _native as N
    seed, V, E, D, ctx, act, mts, _, blank, B, T, scale = RNNT_CASES[name]
    w, am, lens, max_out, refs = _reference_of(name)
    for b, (ids, margin, forced) in enumerate(refs):
        assert margin >= MARGIN, f"{name} utterance {b}: float64 decides a node by {margin:.2e} only"
    assert sum(r[2] for r in refs) >= 1, "max_token_step never forced a frame on"
    if RNNT_CASES[name][7] is not None:
        assert any(len(r[0]) == max_out for r in refs), "the buffer never fills"
    d = {k: v.to(dev).contiguous() for k, v in w.items()}
    amd, ld = am.to(dev).contiguous(), lens.to(dev)
    tokens = torch.zeros((B, max_out), dtype=torch.int64, device=dev)
    out_len = torch.zeros((B,), dtype=torch.int64, device=dev)
    N.check(N.lib().s2t_rnnt_greedy_stateless(
        N.fp(amd), N.lp(ld), N.fp(d["emb"]), N.fp(d["conv_w"]), N.fp(d["lin_w"]), N.fp(d["lin_b"]),
        N.fp(d["pre_w"]), N.fp(d["pre_b"]), B, T, V, E, D, ctx, 0 if act == "relu" else 1, mts,
        max_out, blank, N.lp(tokens), N.lp(out_len), N.stream()), "s2t_rnnt_greedy_stateless")
    tokens, out_len = tokens.cpu(), out_len.cpu()
    for b, (ids, _, _) in enumerate(refs):
        assert int(out_len[b]) == len(ids), (name, b, int(out_len[b]), len(ids))
        assert tokens[b, :len(ids)].tolist() == ids, (name, b)
        assert (tokens[b, len(ids):] == 0).all()
    assert int(out_len[1]) == 0                       # length 0


def _modules(dev, w, V, E, D, ctx, act):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    g = torch.Generator().manual_seed(V + D)
    p = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D,
                                                    "symbol_embedding_dim": E, "context_size": ctx}})
    j = Joiner(JoinerConfig(input_dim=D, output_dim=V, activation=act, use_out_project=False))
    with torch.no_grad():
        p.predictor._embedding.weight.copy_(w["emb"])
        p.predictor._conv.weight.copy_(w["conv_w"].view(E, 1, ctx))
        p.predictor._output_linear.weight.copy_(w["lin_w"])
        p.predictor._output_linear.bias.copy_(w["lin_b"])
        j._pre_proj.weight.copy_(w["pre_w"])
        j._pre_proj.bias.copy_(w["pre_b"])
        j._enc_proj.weight.copy_(torch.randn(V, D, generator=g) / D ** 0.5)
        j._enc_proj.bias.copy_(0.1 * torch.randn(V, generator=g))
    return p.to(dev).eval(), j.to(dev).eval()


@pytest.mark.parametrize("name", ["v65_ctx2_tanh", "v500_ctx64"])
def test_rnnt_greedy_wrapper_exact(dev, name):
    """RnntGreedyDecoding.greedy_tokens: blank 0, max_out = T (max_token_step + 1).  The wrapper
    forms am = enc_proj(hidden) itself (one GEMM); the reference walks the lattice of THAT am, so
    the comparison is of the search alone (the margin is asserted on it all the same)."""
    from speech2text_amd.model.decoding import RnntGreedyDecoding
    seed, V, E, D, ctx, act, mts, _, blank, B, T, scale = RNNT_CASES[name]
    assert blank == 0
    w, am, lens, max_out, _ = _reference_of(name)
    p, j = _modules(dev, w, V, E, D, ctx, act)
    dec = RnntGreedyDecoding(_Tok(), p, j, max_token_step=mts)
    assert dec._fused()
    g = torch.Generator().manual_seed(9)             # (chosen on the CPU like the case seeds)
    hidden = (scale * (3.0 if act == "relu" else 1.0) * torch.randn(B, T, D, generator=g)).to(dev)
    with torch.no_grad():
        am_dev = j._enc_proj(hidden).float().cpu()
    refs = [_rnnt_ref(am_dev[b], lens[b], w, ctx, act, mts, max_out, 0) for b in range(B)]
    for b, r in enumerate(refs):
        assert r[1] >= MARGIN, f"{name} utterance {b}: float64 decides a node by {r[1]:.2e} only"
    tokens, out_len = dec.greedy_tokens(hidden, lens.to(dev))
    assert tokens.shape == (B, max_out)
    texts = dec.decode_batch(hidden, lens.to(dev))
    for b, (ids, _, _) in enumerate(refs):
        assert int(out_len[b]) == len(ids) and tokens[b, :len(ids)].tolist() == ids, (name, b)
        assert (tokens[b, len(ids):] == 0).all()
        assert texts[b] == _Tok().decode(ids)


def test_rnnt_greedy_vocabulary_beyond_the_kernels_shared_memory(dev):
    """V = 16000: (E + D + V) 4 + ctx 4 bytes exceed the kernel's 60 KB rule.  decode_batch takes
    the base class's lattice walk (module by module) instead of raising; same tokens as float64."""
    from speech2text_amd.model.decoding import RnntGreedyDecoding
    V, E, D, ctx, act, mts, B, T, scale = 16000, 8, 8, 2, "relu", 2, 1, 3, 2.0
    w, loops = _weights(1, V, E, D, ctx, scale, 0, act)
    p, j = _modules(dev, w, V, E, D, ctx, act)
    dec = RnntGreedyDecoding(_Tok(), p, j, max_token_step=mts)
    assert dec._fusable() and not dec._fused()
    g = torch.Generator().manual_seed(9)
    hidden = scale * 3.0 * torch.randn(B, T, D, generator=g)
    am = torch.nn.functional.linear(hidden.double(), j._enc_proj.weight.detach().cpu().double(),
                                    j._enc_proj.bias.detach().cpu().double())
    ids, margin, _ = _rnnt_ref(am[0], T, w, ctx, act, mts, 10 ** 9, 0)
    assert margin >= MARGIN, margin
    assert len(ids) > 0
    texts = dec.decode_batch(hidden.to(dev), torch.tensor([T], device=dev))
    assert texts == [_Tok().decode(ids)]
    assert dec.decode(hidden.to(dev)) == texts[0]
