"""GPU: CTC forced alignment on the device (csrc/ctc_align.hip, kernels.ctc_align, model/alignment.py) on
the cases of tests/ctc_align_cases.py, whose conditions tests/test_ctc_align_f64.py asserts on the CPU.
ok, path, tok_begin, tok_end and raw_score must equal the float32 run of the restatement
tests/ctc_align_f64.py bit for bit, ties included; score and tok_logp are bounded by max(2e-5, 8 x what
float32 costs the restatement) against its float64 run.  Frames at and beyond an utterance's length are
NaN in every case: a kernel that read one could not return the restatement's bits.
"""
import math

import pytest
import torch

import ctc_align_cases as C
import ctc_align_f64 as A
from task_support import _ctc_cfg, _pcm_batch, _task

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(dev, name):
    """(the case, its tensors on the device, the kernel's result), once per case."""
    from speech2text_amd import kernels
    if name not in _CACHE:
        m = C.make(name)
        d = dict(x=m["x"].to(dev), lens=m["lens"].to(dev), targets=m["targets"][:, :m["U"]].contiguous().to(dev),
                 tl=m["tl"].to(dev))
        out = kernels.ctc_align(d["x"], d["lens"], d["targets"], d["tl"], blank=m["blank"])
        _CACHE[name] = (m, d, out)
    return _CACHE[name]


# ------------------------------------------------------------------ 1. every case against the restatements
@pytest.mark.parametrize("name", list(C.CASES))
def test_entry_against_the_restatements(dev, name):
    from speech2text_amd import _native as N
    from speech2text_amd import kernels
    m, d, out = _case(dev, name)
    assert N.lib().s2t_ctc_align_form(m["T"], m["U"]) == C.FORMS[name]      # the form this case is for
    path, tb, te, lp, raw, score, ok = C.dense(C.restated(name), m["T"], m["U"])
    got = kernels.CtcAlignment(*(t.cpu() for t in out))
    assert got.path.dtype == torch.int32 and got.path.shape == (m["x"].shape[0], m["T"])
    assert got.tok_begin.shape == got.tok_end.shape == got.tok_logp.shape == (m["x"].shape[0], m["U"])
    assert torch.equal(got.ok, ok), name
    assert torch.equal(got.path, path), name
    assert torch.equal(got.tok_begin, tb) and torch.equal(got.tok_end, te), name
    assert torch.equal(got.raw_score.double(), raw), name                   # bit for bit (-inf included)
    bad = ~ok.bool()                                                        # the sentinels of infeasible rows
    assert bool((got.path[bad] == -1).all()) and bool((got.tok_begin[bad] == -1).all())
    assert bool((got.tok_end[bad] == -1).all()) and bool((got.tok_logp[bad] == 0).all())
    assert bool((got.score[bad] == -math.inf).all())
    for b in range(ok.numel()):                                             # and beyond the lengths
        n, u = C.clamp(m["lens"][b], m["T"]), min(max(int(m["tl"][b]), 0), m["U"])
        assert bool((got.path[b, n:] == -1).all()) and bool((got.tok_begin[b, u:] == -1).all())
        assert bool((got.tok_end[b, u:] == -1).all()) and bool((got.tok_logp[b, u:] == 0).all())
    es, el = C.errors(got.score, got.tok_logp, name)
    print(f"{name}: score rel_err {es:.3e}, tok_logp rel_err {el:.3e} (bound {C.bound(name):.1e})")
    assert es <= C.bound(name) and el <= C.bound(name), (name, es, el)
    again = kernels.ctc_align(d["x"], d["lens"], d["targets"], d["tl"], blank=m["blank"], out=out)
    for a, b in zip(again, got):                                            # into the same buffers: same bits
        assert torch.equal(a.cpu(), b), name


@pytest.mark.parametrize("name", list(C.CASES))
def test_score_is_at_most_the_ctc_log_likelihood(dev, name):
    """The best path's probability is one term of the sum over paths that the loss kernel forms."""
    from speech2text_amd import kernels
    m, d, out = _case(dev, name)
    x = torch.where(torch.isnan(d["x"]), 0.0, d["x"])      # (the loss's padding behaviour is not what is tested)
    loss = kernels.ctc_loss(x, d["targets"], d["lens"], d["tl"], blank=m["blank"], reduction="none",
                            zero_infinity=False).cpu().double()
    score, ok = out.score.cpu().double(), out.ok.cpu().bool()
    assert torch.equal(torch.isfinite(loss), ok), name     # feasible for one is feasible for the other
    if bool(ok.any()):
        slack = C.bound(name) * float(loss[ok].abs().max().clamp(min=1.0))
        print(f"{name}: largest score + loss {float((score + loss)[ok].max()):.3e} (slack {slack:.1e})")
        assert bool((score[ok] <= -loss[ok] + slack).all()), name


@pytest.mark.parametrize("name", [k for k, v in C.CASES.items() if v["pad"]])
def test_target_rows_with_a_stride_above_the_width(dev, name):
    from speech2text_amd import _native as N
    m, d, out = _case(dev, name)
    wide = m["targets"].to(dev)                            # (B, U + pad): the labels are its first U columns
    assert wide.stride(0) > m["U"]
    B, T, V = d["x"].shape
    U = m["U"]
    lib = N.lib()
    ws = torch.empty(lib.s2t_ctc_align_workspace_bytes(B, T, U), dtype=torch.uint8, device=dev)
    new = [torch.empty_like(t) for t in out]
    rc = lib.s2t_ctc_align(N.fp(d["x"]), N.lp(d["lens"]), N.lp(wide), wide.stride(0), N.lp(d["tl"]), B, T, V, U,
                           m["blank"], N.ptr(ws), *(t.data_ptr() for t in new), N.stream())
    assert rc == 0
    for a, b in zip(new, out):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 2. hypotheses of the searches
def _hyp_logits(dev):
    g = torch.Generator().manual_seed(77)
    x = (2.0 * torch.randn(5, 40, 11, generator=g)).to(dev)
    return x, torch.tensor([40, 1, 17, 33, 40], device=dev)


@pytest.mark.parametrize("search", ["greedy", "prefix_beam"])
def test_align_hypotheses_gives_every_search_times(dev, search):
    from speech2text_amd.model.alignment import CtcForcedAligner
    from speech2text_amd.model.decoding import ctc_greedy_tokens, ctc_prefix_beam_tokens
    x, lens = _hyp_logits(dev)
    tokens, out_len = (ctc_greedy_tokens(x, lens) if search == "greedy" else ctc_prefix_beam_tokens(x, lens, 4, 4)[:2])
    al = CtcForcedAligner(frame_seconds=0.04)
    out = al.align_hypotheses(x, lens, tokens, out_len)
    rows = al._rows(x, lens, tokens[:, :int(out_len.max())].contiguous(), out_len)
    assert int(out_len.max()) > 3
    for b, a in enumerate(out):
        hyp = tokens[b, :int(out_len[b])].tolist()
        assert a.ok and [t.token for t in a.tokens] == hyp, (search, b)
        path = rows.path[b, :int(lens[b])].tolist()
        assert A.collapse(path, hyp) == hyp, (search, b)
        assert all(0 <= t.begin < t.end <= int(lens[b]) for t in a.tokens)
        assert all(p.end <= q.begin for p, q in zip(a.tokens, a.tokens[1:]))
        assert all(t.end_s == t.end * 0.04 for t in a.tokens)
    if search == "greedy":                                 # the argmax path IS the best path of its own collapse
        am = x.argmax(dim=-1)
        for b in range(x.shape[0]):
            n, hyp = int(lens[b]), tokens[b, :int(out_len[b])].tolist()
            labels = [hyp[s >> 1] if s & 1 else 0 for s in rows.path[b, :n].tolist()]
            assert labels == am[b, :n].tolist(), b


# ------------------------------------------------------------------ 3. graph capture
def test_capture_and_replay_in_a_graph(dev):
    from speech2text_amd import kernels
    name = "u7_v65_b17_ragged"
    m, d, out = _case(dev, name)
    want = [t.clone() for t in out]
    held = kernels.CtcAlignment(*(torch.empty_like(t) for t in out))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kernels.ctc_align(d["x"], d["lens"], d["targets"], d["tl"], blank=m["blank"], out=held)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.ctc_align(d["x"], d["lens"], d["targets"], d["tl"], blank=m["blank"], out=held)
    for t in held:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(held, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 4. the Python surface
def test_surface_checks_its_inputs(dev):
    from speech2text_amd import kernels
    x, n = torch.zeros(1, 4, 5, device=dev), torch.tensor([4], device=dev)
    t, tl = torch.ones(1, 2, dtype=torch.int64, device=dev), torch.tensor([2], device=dev)
    with pytest.raises(ValueError, match="exceeds the kernel's limit of 1023 labels"):
        kernels.ctc_align(x, n, torch.ones(1, 1024, dtype=torch.int64, device=dev), tl)
    with pytest.raises(RuntimeError, match="contiguous"):
        kernels.ctc_align(x.transpose(1, 2), n, t, tl)
    with pytest.raises(RuntimeError, match="int64"):
        kernels.ctc_align(x, n.int(), t, tl)
    with pytest.raises(RuntimeError, match="float32"):
        kernels.ctc_align(x.double(), n, t, tl)
    with pytest.raises(ValueError, match="blank"):
        kernels.ctc_align(x, n, t, tl, blank=5)
    out = kernels.ctc_align(x, n, t, tl)
    assert out.ok.tolist() == [1] and A.collapse(out.path[0].tolist(), [1, 1]) == [1, 1]


def test_aligner_runs_the_kernel_on_device_tensors_and_the_loop_beyond_its_limit(dev):
    from speech2text_amd.model.alignment import CtcForcedAligner
    name = "ties_v11_b17"
    m, d, out = _case(dev, name)
    al = CtcForcedAligner(blank=m["blank"])
    rows = al._rows(d["x"], d["lens"], d["targets"], d["tl"])
    for a, b in zip(rows, out):
        assert torch.equal(a, b)
    loop = [al._module_loop(d["x"][b, :C.clamp(m["lens"][b], m["T"])], d["targets"][b, :max(int(m["tl"][b]), 0)].tolist(),
                            m["blank"]) for b in range(3)]
    for b, r in enumerate(loop):                           # the host loop on device tensors: the same path
        n = C.clamp(m["lens"][b], m["T"])
        assert r.ok == int(out.ok[b]) and (not r.ok or torch.equal(r.path, out.path[b, :n]))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 1030, 3, generator=g).to(dev)       # 1024 labels: beyond the kernel, the loop serves it
    t = (torch.arange(1024) % 2 + 1).unsqueeze(0).to(dev)
    got = al.align(x, torch.tensor([1030], device=dev), t, torch.tensor([1024], device=dev))
    assert got[0].ok and len(got[0].tokens) == 1024


# ------------------------------------------------------------------ 5. the task
def test_ctc_task_align_tiles_the_frames_in_order(dev, golden_dir):
    cfg, V = _ctc_cfg(golden_dir)
    task = _task("CTC", cfg, dev)
    batch = _pcm_batch(dev, B=2, sec=1.0, V=V)
    out = task.align(batch, frame_seconds=0.04)
    with torch.no_grad():
        feat, n = task.features(batch)
        enc, el = task._encoder(feat, n)
        _, dl = task._decoder(enc, el)
    assert len(out) == 2
    for b, a in enumerate(out):
        Tb, U = int(dl[b]), int(batch["label_length"][b])
        assert a.ok and math.isfinite(a.score) and a.score < 0.0
        assert [t.token for t in a.tokens] == batch["label"][b, :U].tolist()
        assert [t.piece for t in a.tokens] == [task._tokenizer.labels[i] for i in batch["label"][b, :U].tolist()]
        edges = [0] + [e for t in a.tokens for e in (t.begin, t.end)] + [Tb]
        assert edges == sorted(edges) and all(t.begin < t.end for t in a.tokens)      # in order inside [0, Tb)
        assert all(t.begin_s == t.begin * 0.04 for t in a.tokens)
        assert a.words and a.words[0].begin == a.tokens[0].begin and a.words[-1].end == a.tokens[-1].end
        assert sum(w.logp for w in a.words) == pytest.approx(sum(t.logp for t in a.tokens), rel=1e-5)
