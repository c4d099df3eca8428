"""GPU: the chunk-carried RNN-T search (csrc/decode_rnnt.hip, model/decoding.py
RnntStreamingSearch), the StreamingRecognizer graph around it and PrunedRnntTask.streaming_recognizer.

The yardstick is exact: however [0, L) is cut into chunks, tokens, frames, out_len and score are
those of the whole-utterance kernels (s2t_rnnt_beam_stateless / s2t_rnnt_greedy_stateless, themselves
pinned to the reference class by tests/test_rnnt_beam.py and tests/test_gpu_greedy_decode.py) on the
concatenated am, bit for bit -- torch.equal, no tolerance.  `stable_len` is held to the float64
chunked restatement (tests/rnnt_stream_restatement.py) on the utterances whose stored decision
margin is at least 16 N, the project's decidability rule."""
import functools

import numpy as np
import pytest
import torch

import rnnt_beam_restatement as R
import rnnt_stream_restatement as S
from decode_support import (_beam_modules, _feed, _fixture, _fixture_free_config, _long_input, _regular,
                            _same_rows, _search, _tiny_stream_encoder, _tokenizer)
from task_support import _pruned_beam_cfg

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------ helpers


def _irregular(lens, seed):
    """Cut points from a seeded generator, different per row, sizes 0..16 with zeros interleaved,
    and one call that idles every row."""
    g = np.random.default_rng(seed)
    rows = []
    for n in np.asarray(lens).tolist():
        sizes, left = [], n
        while left > 0:
            s = int(g.choice([0, 0, 1, 1, 2, 3, 5, 7, 11, 16]))
            s = min(s, left)
            sizes.append(s)
            left -= s
        rows.append(sizes)
    K = max(len(r) for r in rows)
    plan = [np.array([r[k] if k < len(r) else 0 for r in rows], dtype=np.int64) for k in range(K)]
    plan.insert(K // 2, np.zeros(len(rows), dtype=np.int64))
    assert any((p == 0).any() and (p > 0).any() for p in plan)
    return plan


def _stream(c, dev, B, method="beam", beam=None, topk=None, max_tokens=None, mts=5, modules=None):
    from speech2text_amd.model.decoding import RnntStreamingSearch
    pred, join = modules or _beam_modules(c, dev)
    return RnntStreamingSearch(pred, join, B, method, max_token_step=mts,
                               beam_size=c.get("beam", 1) if beam is None else beam,
                               cutoff_top_k=c.get("topk", 1) if topk is None else topk,
                               max_tokens=c["Tmax"] if max_tokens is None else max_tokens, device=dev)


@functools.lru_cache(maxsize=None)
def _one_shot(golden_dir, dev, ci):
    """The whole-utterance search on a stored configuration: computed once, shared, left unchanged."""
    c = _fixture(golden_dir)[ci]
    return _search(c, c["am"], c["lengths"], dev)


def _large_v():
    """Seed and shapes of test_rnnt_beam.test_large_vocabulary_keeps_lm_rows_in_the_workspace."""
    s = _fixture_free_config(V=1024, D=32, E=24, ctx=3, seed=21, scale=3.0)
    s.update(beam=16, topk=4, Tmax=24)
    g = torch.Generator().manual_seed(4)
    return s, torch.randn(4, 24, 1024, generator=g) * 2.0, np.array([24, 17, 5, 1], dtype=np.int64)


PARTITIONS = ("1", "7", "16", "irregular")


def _plan(lens, name, seed=0):
    return _irregular(lens, 100 + seed) if name == "irregular" else _regular(lens, int(name))


# ------------------------------------------------------------------------------------ beam
@pytest.mark.parametrize("partition", PARTITIONS)
def test_beam_chunks_equal_the_whole_utterance_search(dev, golden_dir, partition):
    """Every stored utterance, 8 rows per launch; configuration 4 (V 500, beam 16) keeps its lm rows
    outside the LDS, in place in the state buffer."""
    fx = _fixture(golden_dir)
    assert (fx[4]["V"], fx[4]["beam"]) == (500, 16)
    for ci, c in enumerate(fx):
        want = _one_shot(golden_dir, dev, ci)
        search = _stream(c, dev, 8)
        got, off = _feed(search, torch.from_numpy(c["am"]).to(dev), _plan(c["lengths"], partition, ci))
        assert off.tolist() == c["lengths"].tolist()
        _same_rows(got, want)
        for b in range(8):
            n = int(got[2][b])
            assert got[0][b, :n].tolist() == c["tokens"][b], (ci, b)      # the reference class's tokens
            assert got[1][b, :n].tolist() == c["frames"][b], (ci, b)
        assert int(search.overflow.sum()) == 0


@pytest.mark.parametrize("partition", PARTITIONS)
def test_large_vocabulary_chunks(dev, partition):
    """V = 1024 at beam 16: lm rows in the state buffer, classes re-read per selection round."""
    s, am, lens = _large_v()
    want = _search(s, am, lens, dev)
    assert int(want[2].min()) > 0
    got, _ = _feed(_stream(s, dev, 4), am.to(dev), _plan(lens, partition, 9))
    _same_rows(got, want)


@functools.lru_cache(maxsize=None)
def _run7(golden_dir, dev, ci, beam=None, topk=None):
    """The 7-frame partition of a configuration with the outputs after every chunk."""
    c = _fixture(golden_dir)[ci]
    snaps = []
    _feed(_stream(c, dev, 8, beam=beam, topk=topk), torch.from_numpy(c["am"]).to(dev),
          _regular(c["lengths"], 7), snap=lambda off, out: snaps.append((off, out)))
    return snaps


def test_every_chunk_gives_the_prefix_answer(dev, golden_dir):
    """After each chunk of the 7-frame partition the outputs are the whole-utterance search's on the
    frames fed so far: the answer after every chunk, not only the last."""
    from speech2text_amd.model.decoding import rnnt_beam_tokens_from_am
    for ci, c in enumerate(_fixture(golden_dir)):
        pred, join = _beam_modules(c, dev)
        am = torch.from_numpy(c["am"]).to(dev)
        for off, out in _run7(golden_dir, dev, ci):
            want = [x.cpu() for x in rnnt_beam_tokens_from_am(am, torch.as_tensor(off), pred, join,
                                                              c["beam"], c["topk"])]
            _same_rows(out, want)


def test_stable_len(dev, golden_dir):
    """stable_len never decreases; tokens[:stable_len] is a prefix of every later result; with one
    beam it is out_len; on the utterances with the stored margin >= 16 N it is the chunked float64
    restatement's common-prefix length after every chunk (at least 3/4 of each configuration)."""
    for ci, c in enumerate(_fixture(golden_dir)):
        snaps = _run7(golden_dir, dev, ci)
        params = {k: c[k] for k in R.PARAM_KEYS}
        decidable = [b for b in range(8) if c["margin"][b] >= 16 * c["N"]]
        assert len(decidable) >= 6, ci
        for b in range(8):
            n = int(c["lengths"][b])
            mine = [(out[0][b], int(out[2][b]), int(out[4][b]))
                    for _, out in snaps[:-(-n // 7)]]                    # the calls that fed row b
            stable = [m[2] for m in mine]
            assert stable == sorted(stable) and stable[-1] <= mine[-1][1], (ci, b)
            for k, (tok, _, st) in enumerate(mine):
                for tok2, n2, _ in mine[k:]:
                    assert n2 >= st and torch.equal(tok2[:st], tok[:st]), (ci, b, k)
            if b in decidable:
                want = S.beam_search_chunked(c["am"][b, :n], list(range(0, n, 7)) + [n], params, c["ctx"],
                                             c["act"], c["beam"], c["topk"])[4]
                assert stable == want, (ci, b)
    one = _run7(golden_dir, dev, 1, 1, 1)
    assert all(torch.equal(out[4], out[2]) for _, out in one) and int(one[-1][1][2].sum()) > 0


def test_rows_are_independent_and_reset_alone(dev, golden_dir):
    """Rows 0..3 run utterance A; row 2 is reset midway by the row mask and fed utterance B.  Rows
    0, 1, 3 are bit-identical to a run without the reset; row 2 is B's whole-utterance result with
    frames counted from its reset."""
    c = _fixture(golden_dir)[1]
    want = _one_shot(golden_dir, dev, 1)
    la, lb = int(c["lengths"][0]), int(c["lengths"][1])
    A, Bu = torch.from_numpy(c["am"][0]), torch.from_numpy(c["am"][1])
    am = torch.stack([A, A, A, A]).to(dev)
    modules = _beam_modules(c, dev)
    plain, _ = _feed(_stream(c, dev, 4, modules=modules), am, _regular([la] * 4, 16))
    _same_rows(plain, [x[[0, 0, 0, 0]] for x in want])

    search = _stream(c, dev, 4, modules=modules)
    plan = _regular([la] * 4, 16)
    half = len(plan) // 2
    _, off = _feed(search, am, plan[:half])
    assert int(search.out_len[2]) > 0
    search.reset([2])
    assert search.out_len.tolist()[2] == 0 and int(search.out_len[1]) > 0
    am2 = am.clone()
    am2[2] = Bu.to(dev)
    off[2] = 0
    rest = [np.array([p[0], p[1], 0, p[3]]) for p in plan[half:]]
    for k, cl in enumerate(_regular([lb], 16)):                        # B rides along from its frame 0
        if k < len(rest):
            rest[k][2] = cl[0]
        else:
            rest.append(np.array([0, 0, cl[0], 0]))
    got, off = _feed(search, am2, rest, off=off)
    assert off.tolist() == [la, la, lb, la]
    for x, y in zip(got, plain):
        assert torch.equal(x[[0, 1, 3]], y[[0, 1, 3]])
    _same_rows([x[2:3] for x in got], [x[1:2] for x in want])
    assert got[0][2, :int(got[2][2])].tolist() == c["tokens"][1]


@pytest.mark.parametrize("method", ["greedy", "beam"])
def test_idle_call_changes_nothing(dev, golden_dir, method):
    c = _fixture(golden_dir)[2]
    search = _stream(c, dev, 8, method)
    am = torch.from_numpy(c["am"]).to(dev)
    _feed(search, am, _regular(c["lengths"], 16)[:3])
    assert int(search.out_len.sum()) > 0
    outs = (search.state, search.tokens, search.frames, search.out_len, search.score, search.stable_len,
            search.overflow)
    before = [x.clone() for x in outs]
    search.step(am[:, :16].contiguous(), torch.zeros(8, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    for x, y in zip(outs, before):
        assert torch.equal(x, y)


def test_capacity(dev, golden_dir):
    """max_tokens = 3 on utterances with more than 3 tokens: the first 3 tokens, out_len 3, overflow
    1, and the search itself went on exactly -- the score is the whole-utterance score, bit for bit."""
    c = _fixture(golden_dir)[1]
    want = _one_shot(golden_dir, dev, 1)
    assert int(want[2].min()) > 3
    search = _stream(c, dev, 8, max_tokens=3)
    got, _ = _feed(search, torch.from_numpy(c["am"]).to(dev), _regular(c["lengths"], 16))
    assert got[2].tolist() == [3] * 8 and search.overflow.tolist() == [1] * 8
    assert torch.equal(got[0], want[0][:, :3]) and torch.equal(got[1], want[1][:, :3])
    assert torch.equal(got[3], want[3])
    assert int(got[4].max()) <= 3
    search.reset()
    torch.cuda.synchronize()
    assert search.overflow.tolist() == [0] * 8 and search.out_len.tolist() == [0] * 8
    got, _ = _feed(search, torch.from_numpy(c["am"]).to(dev), _regular(c["lengths"], 1)[:2])
    assert search.overflow.tolist() == [0] * 8 and int(got[2].max()) <= 2   # (two frames: at most two tokens)

    # greedy at capacity is inert, as the whole-utterance kernel's walk ends there
    gt, gn = _greedy_one_shot(c, c["am"], c["lengths"], dev, 5, max_out=3)
    assert gn.tolist() == [3] * 8
    search = _stream(c, dev, 8, "greedy", max_tokens=3)
    got, _ = _feed(search, torch.from_numpy(c["am"]).to(dev), _regular(c["lengths"], 7))
    assert torch.equal(got[0], gt) and torch.equal(got[1], gn) and search.overflow.tolist() == [1] * 8


def test_refusals(dev):
    """-1 before any launch, outputs untouched: Tc = 257, beam_size = 17, ctx = 65, a NULL state."""
    from speech2text_amd import _native as N
    lib = N.lib()
    V, E, D, ctx, B, MT = 8, 12, 16, 2, 2, 10
    f = lambda *s: torch.zeros(*s, device=dev)                           # noqa: E731
    emb, conv_w, lin_w, lin_b, pre_w, pre_b = f(V, E), f(E, 65), f(D, E), f(D), f(V, D), f(V)
    am, cl = f(B, 257, V), torch.ones(B, dtype=torch.int64, device=dev)
    state = torch.zeros(max(lib.s2t_rnnt_stream_state_bytes(B, V, 64, 16, MT), 256), dtype=torch.uint8, device=dev)
    tok, frm = (torch.full((B, MT), 7, dtype=torch.int64, device=dev) for _ in range(2))
    n_out, stable = (torch.full((B,), 7, dtype=torch.int64, device=dev) for _ in range(2))
    score = torch.full((B,), 7.0, device=dev)
    ovf = torch.full((B,), 7, dtype=torch.int32, device=dev)
    w = [N.fp(t) for t in (emb, conv_w, lin_w, lin_b, pre_w, pre_b)]

    def beam(Tc=4, beam_size=4, ctx_=ctx, st=state, topk=4):
        return lib.s2t_rnnt_beam_stateless_chunk(
            N.fp(am), N.lp(cl), *w, B, Tc, V, E, D, ctx_, 0, 0, beam_size, topk, MT, N.ptr(st), N.lp(tok),
            N.lp(frm), N.lp(n_out), N.fp(score), N.lp(stable), N.ip(ovf), N.stream())

    def greedy(Tc=4, ctx_=ctx, st=state):
        return lib.s2t_rnnt_greedy_stateless_chunk(
            N.fp(am), N.lp(cl), *w, B, Tc, V, E, D, ctx_, 0, 5, MT, 0, N.ptr(st), N.lp(tok), N.lp(n_out),
            N.ip(ovf), N.stream())

    assert beam(Tc=257) == -1 and beam(beam_size=17) == -1 and beam(ctx_=65) == -1 and beam(st=None) == -1
    assert beam(beam_size=0) == -1 and beam(Tc=0) == -1 and beam(topk=0) == -1
    assert greedy(Tc=257) == -1 and greedy(ctx_=65) == -1 and greedy(st=None) == -1
    assert lib.s2t_rnnt_stream_reset(None, None, B, V, ctx, 4, MT, 0, N.stream()) == -1
    assert lib.s2t_rnnt_stream_reset(N.ptr(state), None, B, V, 65, 4, MT, 0, N.stream()) == -1
    assert lib.s2t_rnnt_stream_reset(N.ptr(state), None, B, V, ctx, 17, MT, 0, N.stream()) == -1
    assert lib.s2t_rnnt_stream_reset(N.ptr(state), None, 0, V, ctx, 4, MT, 0, N.stream()) == 0
    torch.cuda.synchronize()
    for t in (tok, frm, n_out, stable, ovf):
        assert bool((t == 7).all())
    assert bool((score == 7.0).all()) and int(state.sum()) == 0


def test_class_refuses_what_the_fused_search_does_not_take(dev):
    from speech2text_amd.model.decoding import RnntStreamingSearch
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    s = _fixture_free_config(V=8, D=16, E=12, ctx=2, seed=9)
    pred, join = _beam_modules(s, dev)
    RnntStreamingSearch(pred, join, 2, "beam", device=dev)
    with pytest.raises(ValueError):
        RnntStreamingSearch(pred, join, 2, "beam", beam_size=17, device=dev)
    with pytest.raises(ValueError):
        RnntStreamingSearch(pred, join, 2, "viterbi", device=dev)
    proj = Joiner(JoinerConfig(input_dim=16, output_dim=8, activation="relu", prune_range=5,
                               use_out_project=True)).to(dev)
    with pytest.raises(ValueError):
        RnntStreamingSearch(pred, proj, 2, "greedy", device=dev)
    lstm = Predictor({"model": "Lstm", "config": {"num_symbols": 8, "output_dim": 16, "symbol_embedding_dim": 12,
                                                  "num_lstm_layers": 1, "lstm_hidden_dim": 16}}).to(dev)
    with pytest.raises(ValueError):
        RnntStreamingSearch(lstm, join, 2, "greedy", device=dev)
    with pytest.raises(RuntimeError):
        RnntStreamingSearch(*_beam_modules(s, "cpu"), 2, "greedy", device=dev)
    with pytest.raises(ValueError):
        RnntStreamingSearch(pred, join, 2, "beam", device=dev).step(torch.zeros(2, 257, 8, device=dev))


# ------------------------------------------------------------------------------------ greedy
def _greedy_one_shot(c, am, lens, dev, mts, max_out=None):
    """s2t_rnnt_greedy_stateless on a given am."""
    from speech2text_amd import _native as N
    pred, join = _beam_modules(c, dev)
    p = pred.predictor
    am = torch.as_tensor(am).to(dev).contiguous()
    B, T, V = am.shape
    max_out = T * (mts + 1) if max_out is None else max_out
    lens = torch.as_tensor(lens).to(device=dev, dtype=torch.int64)
    tokens = torch.zeros((B, max_out), dtype=torch.int64, device=dev)
    out_len = torch.zeros((B,), dtype=torch.int64, device=dev)
    N.check(N.lib().s2t_rnnt_greedy_stateless(
        N.fp(am), N.lp(lens), N.fp(p._embedding.weight), N.fp(p._conv.weight.reshape(c["E"], c["ctx"]).contiguous()),
        N.fp(p._output_linear.weight), N.fp(p._output_linear.bias), N.fp(join._pre_proj.weight),
        N.fp(join._pre_proj.bias), B, T, V, c["E"], c["D"], c["ctx"], 0 if c["act"] == "relu" else 1,
        mts, max_out, 0, N.lp(tokens), N.lp(out_len), N.stream()), "s2t_rnnt_greedy_stateless")
    torch.cuda.synchronize()
    return tokens.cpu(), out_len.cpu()


def _greedy_inputs(golden_dir):
    """The stored am, and the seeded input of test_rnnt_beam.test_degenerate_beam_equals_the_greedy_
    kernel: it emits on many frames, several symbols per frame right before a chunk boundary included."""
    c = _fixture(golden_dir)[0]
    g = torch.Generator().manual_seed(17)
    rand_am = torch.randn(64, 90, c["V"], generator=g) * 3.0
    rand_lens = torch.randint(1, 91, (64,), generator=g)
    rand_lens[0] = 90
    return c, ((torch.from_numpy(c["am"]), c["lengths"]), (rand_am, rand_lens.numpy()))


@pytest.mark.parametrize("mts", [0, 1, 5])
def test_greedy_chunks_equal_the_whole_utterance_walk(dev, golden_dir, mts):
    c, inputs = _greedy_inputs(golden_dir)
    modules = _beam_modules(c, dev)
    for am, lens in inputs:
        B, T = am.shape[0], am.shape[1]
        gt, gn = _greedy_one_shot(c, am, lens, dev, mts)
        assert 0 < int(gn.sum())
        if mts == 5 and B == 64:
            assert int(gn.max()) > 90 // 2           # several symbols per frame do happen
        for partition in PARTITIONS:
            search = _stream(c, dev, B, "greedy", max_tokens=T * (mts + 1), mts=mts, modules=modules)
            got, off = _feed(search, am.to(dev), _plan(lens, partition, mts))
            assert off.tolist() == np.asarray(lens).tolist()
            assert torch.equal(got[1], gn), partition
            for b in range(B):
                assert torch.equal(got[0][b, :int(gn[b])], gt[b, :int(gn[b])]), (partition, b)
            # (overflow = the output is full and the walk stopped, as the whole-utterance walk does)
            assert search.overflow.cpu().tolist() == (gn >= T * (mts + 1)).int().tolist()


def test_degenerate_beam_chunks_equal_greedy_chunks(dev, golden_dir):
    """beam_size = cutoff_top_k = 1, chunked, is the chunked greedy walk at max_token_step = 0."""
    c, inputs = _greedy_inputs(golden_dir)
    modules = _beam_modules(c, dev)
    for am, lens in inputs:
        B, T = am.shape[0], am.shape[1]
        plan = _irregular(lens, 5)
        g, _ = _feed(_stream(c, dev, B, "greedy", max_tokens=T, mts=0, modules=modules), am.to(dev), plan)
        bm, _ = _feed(_stream(c, dev, B, "beam", beam=1, topk=1, max_tokens=T, modules=modules), am.to(dev), plan)
        assert torch.equal(bm[2], g[1]) and int(g[1].sum()) > 0
        assert torch.equal(bm[4], bm[2])                                 # one beam: everything is stable
        for b in range(B):
            assert torch.equal(bm[0][b, :int(g[1][b])], g[0][b, :int(g[1][b])]), b


def test_long_chunks_cross_the_trace_blocks(dev, golden_dir):
    """Chunks of more than 64 frames: the chunk end stages its records in 64-frame blocks, as the
    whole-utterance trace-back does.  Rows 0-7 of the seeded 64 x 90 input at beam 4 / top-k 4: a
    chunk per row, 70 + the rest, and 7-frame chunks equal the whole-utterance search bit for bit and
    end with the same stable_len.  Row 0 (90 frames: the blocks [26, 90) and [0, 26)) emits on both
    sides of both block edges; tests/test_rnnt_beam.py asserts the same of the float64 restatement."""
    c = _fixture(golden_dir)[0]
    am, lens = _long_input(c)
    assert int(lens[0]) == 90
    want = _search(c, am, lens, dev, beam=4, topk=4)
    frames0 = want[1][0, :int(want[2][0])].tolist()
    assert min(frames0) < 26 and max(frames0) >= 64, frames0
    modules = _beam_modules(c, dev)
    stable = []
    for step in (90, 70, 7):
        search = _stream(c, dev, 8, beam=4, topk=4, max_tokens=90, modules=modules)
        got, off = _feed(search, am.to(dev), _regular(lens, step))
        assert off.tolist() == lens.tolist()
        _same_rows(got, want)
        assert int(search.overflow.sum()) == 0
        stable.append(got[4].tolist())
    assert stable[0] == stable[1] == stable[2], stable


# ------------------------------------------------------------------------------------ recogniser


@pytest.mark.parametrize("method", ["greedy", "beam"])
def test_recognizer_graph_equals_the_eager_composition(dev, golden_dir, method):
    """StreamingRecognizer.step (one graph replay) against streaming_step -> _enc_proj ->
    RnntStreamingSearch.step issued eagerly, over the fixture's 6 chunks, twice across reset():
    am, tokens, frames, score and every encoder state bit for bit; the final tokens are the
    whole-utterance search's on the concatenation of the am chunks the recogniser returned."""
    from speech2text_amd.model.decoding import rnnt_beam_tokens_from_am
    from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
    g, m, chunk = _tiny_stream_encoder(golden_dir, dev)
    V, D = 24, max(m.encoder_dim)
    s = _fixture_free_config(V=V, D=D, E=16, ctx=3, seed=31, scale=2.0)
    s["enc_b"][0] += 4.0                 # blank wins on a share of the frames: tokens on some, not on all
    pred, join = _beam_modules(s, dev)
    pred.eval(), join.eval()
    feats = torch.from_numpy(g["feats"]).to(dev)
    B, T, Tc = feats.shape[0], 2 * chunk + 13, chunk // 2
    kw = dict(method=method, max_token_step=1, beam_size=4, cutoff_top_k=4, max_tokens=64)
    rec = StreamingRecognizer(m, pred, join, _tokenizer(V), batch_size=B, device=dev, **kw)
    eager = _stream(s, dev, B, method, beam=4, topk=4, max_tokens=64, mts=1, modules=(pred, join))
    for rep in range(2):
        st = m.get_init_states(B, dev)
        rec.reset()
        eager.reset()
        ams = []
        for c in range(6):
            x = feats[:, 2 * chunk * c:2 * chunk * c + T]
            with torch.no_grad():
                enc, st = m.streaming_step(x, st)
                am = join._enc_proj(enc).float().contiguous()
            want = eager.step(am)
            got = rec.step(x)
            assert torch.equal(got[-1], am), (rep, c)
            for a, b in zip(got[:-1], want):
                assert torch.equal(a, b), (rep, c)
            ams.append(got[-1].clone())
        for a, b in zip(rec.states, st):
            assert torch.equal(a, b)
        am_all = torch.cat(ams, dim=1)
        n = int(rec.search.out_len.sum())
        print(f"{method} rep {rep}: {n} tokens on {B * 6 * Tc} frames")
        assert 0 < n < B * 6 * Tc
        lens = torch.full((B,), 6 * Tc, dtype=torch.int64)
        if method == "beam":
            want = [x.cpu() for x in rnnt_beam_tokens_from_am(am_all, lens, pred, join, 4, 4)]
            _same_rows([x.cpu() for x in rec.outputs], want)
            assert bool((rec.search.stable_len <= rec.search.out_len).all())
        else:
            gt, gn = _greedy_one_shot(s, am_all, lens, dev, 1, max_out=64)
            assert torch.equal(rec.search.out_len.cpu(), gn)
            assert torch.equal(rec.search.tokens.cpu()[:, :int(gn.max())], gt[:, :int(gn.max())])
        texts = rec.texts()
        tok = rec.search.tokens.cpu()
        assert texts == [rec.tokenizer.decode(tok[b, :int(rec.search.out_len[b])]) for b in range(B)]
        stable = rec.stable_texts()
        assert all(t.startswith(u) for t, u in zip(texts, stable))
    with pytest.raises(ValueError):
        rec.step(feats[:, :T - 1])


def test_recognizer_rejects_cpu_and_training(dev, golden_dir):
    from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
    g, m, chunk = _tiny_stream_encoder(golden_dir, dev)
    s = _fixture_free_config(V=24, D=max(m.encoder_dim), E=16, ctx=3, seed=31)
    pred, join = _beam_modules(s, dev)
    pred.eval(), join.eval()
    m.train()
    with pytest.raises(RuntimeError):
        StreamingRecognizer(m, pred, join, _tokenizer(24), device=dev)
    m.eval()
    with pytest.raises(RuntimeError):
        StreamingRecognizer(m.cpu(), pred, join, _tokenizer(24), device=dev)


def test_task_streaming_recognizer(dev):
    """PrunedRnntTask.streaming_recognizer(batch_size=2): `recognize` on two utterances of different
    lengths equals feeding the chunks by hand, the shorter row idling (chunk_len 0) while the longer
    one goes on; method and widths come from the task's metric section."""
    import math
    from speech2text_amd.build_task import TaskFactory
    V, chunk = 32, 8
    cfg = _pruned_beam_cfg(V)
    cfg["encoder"]["config"].update({"chunk_size": [chunk], "left_context_frames": [16]})
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(cfg).to(dev)
    task.eval()
    with torch.no_grad():
        for p in list(task._predictor.parameters()) + list(task._joiner.parameters()):
            p.mul_(3.0)
        task._global_cmvn.global_mean.fill_(0.25)
        task._global_cmvn.global_istd.fill_(0.5)
    rec = task.streaming_recognizer(batch_size=2)
    assert (rec.search.method, rec.search.beam_size, rec.search.cutoff_top_k) == ("beam", 3, 2)
    assert task.streaming_recognizer(batch_size=1, method="greedy").search.max_token_step == 5
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 150, 80, generator=g) * 2.0
    lens = torch.tensor([150, 71])
    texts = rec.recognize(feats.to(dev), lens)
    assert any(len(t) for t in texts)

    n_out = ((lens - 7) // 2 + 1) // 2
    assert n_out.tolist() == rec.num_output_frames(lens).tolist() == [36, 16]
    K, Tc, T = -(-36 // (chunk // 2)), chunk // 2, 2 * chunk + 13
    pad_value = math.log(1e-10) / 0.5 + 0.25                            # log(1e-10) after the CMVN
    buf = torch.full((2, 2 * chunk * (K - 1) + T, 80), pad_value)
    buf[0, :150], buf[1, :71] = feats[0], feats[1, :71]
    rec.reset()
    idle = 0
    for k in range(K):
        cl = (n_out - k * Tc).clamp(0, Tc)
        idle += int(cl[1] == 0 and cl[0] > 0)
        rec.step(buf[:, 2 * chunk * k:2 * chunk * k + T].to(dev), cl)
    assert idle > 0
    assert rec.texts() == texts
    with pytest.raises(ValueError):
        rec.recognize(feats[:1].to(dev), lens[:1])
