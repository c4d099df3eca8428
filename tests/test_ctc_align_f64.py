"""CPU: the conditions of tests/ctc_align_cases.py on the restatement tests/ctc_align_f64.py (float32 and
float64 agree on ok, path and spans on every utterance; every TIES case has a tied decision on its best
path; the recorded cost of float32), the validity of every returned path, the host-side entries of
csrc/ctc_align.hip (sizes, forms, refusals: the library loads without a GPU), merge_words on both
tokenizers and the aligner's host loop against the restatement.
"""
import math
import os

import pytest
import torch

import ctc_align_cases as C
import ctc_align_f64 as A
from decode_support import _lib


# ------------------------------------------------------------------ 1. the conditions
@pytest.mark.parametrize("name", list(C.CASES))
def test_float32_and_float64_restatements_agree(name):
    ref, f32 = C.reference(name), C.restated(name)
    assert len(ref) == len(f32) == C.CASES[name]["B"]
    for b, (a, r) in enumerate(zip(f32, ref)):
        assert a.ok == r.ok and a.path == r.path, (name, b)
        assert a.tok_begin == r.tok_begin and a.tok_end == r.tok_end, (name, b)
        assert a.ties == r.ties, (name, b)


@pytest.mark.parametrize("name", C.TIES)
def test_ties_cases_have_a_tied_decision_on_the_best_path(name):
    ties = sum(r.ties for r in C.restated(name))
    print(f"{name}: {ties} tied decisions on the best paths")
    assert ties >= 1
    for a, r in zip(C.restated(name), C.reference(name)):                # quantised: exact in both
        assert a.raw_score == r.raw_score


def test_cases_reach_what_they_are_for():
    """Infeasible rows at T >= U, the tight alignment, the empty transcript, doubled labels."""
    m, ref = C.make("u9_v11_logp_inf"), C.reference("u9_v11_logp_inf")
    assert not ref[0].ok and int(m["lens"][0]) >= m["U"] and ref[1].ok
    m, ref = C.make("u3_tight_aab"), C.reference("u3_tight_aab")
    t = m["targets"][0, :3].tolist()
    assert t[0] == t[1] and int(m["lens"][0]) == C.need(t) and ref[0].ok
    assert int(m["lens"][1]) == C.need(m["targets"][1, :3].tolist()) - 1 and not ref[1].ok
    assert int(m["lens"][2]) < 3 and not ref[2].ok
    m, ref = C.make("u7_v65_b17_ragged"), C.reference("u7_v65_b17_ragged")
    assert int(m["tl"][1]) == 0 and int(m["tl"][2]) < 0 and m["targets"].shape[1] > m["U"]
    assert any(not r.ok for r in ref) and any(r.ok and r.path for r in ref)
    assert any(r.ok and not r.path for r in C.reference("u0_b17_ragged"))     # no frames, no labels
    assert C.make("u1023_max_tight")["U"] == 1023 and C.reference("u1023_max_tight")[0].ok
    assert {c["V"] for c in C.CASES.values()} >= {3, 65, 300} and {c["B"] for c in C.CASES.values()} >= {1, 17, 33}


@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_cost_of_score_and_tok_logp(name):
    fig = C.fp32_figure(name)
    print(f"fp32 cost of score / tok_logp, {name}: {fig:.3e}")
    rec = C.COST[name]
    assert fig <= 4 * rec and rec <= 4 * fig, (fig, rec)


# ------------------------------------------------------------------ 2. every path is a path
@pytest.mark.parametrize("name", list(C.CASES))
def test_paths_are_valid_and_collapse_to_the_targets(name):
    m = C.make(name)
    for b, r in enumerate(C.reference(name)):
        n = C.clamp(m["lens"][b], m["T"])
        t = m["targets"][b, :min(max(int(m["tl"][b]), 0), m["U"])].tolist()
        U = len(t)
        if not r.ok:
            assert r.path == [] and r.score == -math.inf and r.tok_begin == [-1] * U
            continue
        assert len(r.path) == n
        if n == 0:
            assert U == 0 and r.score == 0.0 and r.raw_score == 0.0
            continue
        assert r.path[0] in (0, 1) and r.path[-1] in ((2 * U, 2 * U - 1) if U else (0,))
        for p, q in zip(r.path, r.path[1:]):
            assert q - p in (0, 1, 2)
            if q - p == 2:
                assert p & 1 and t[q >> 1] != t[p >> 1]
        assert A.collapse(r.path, t, m["blank"]) == t, (name, b)
        for u in range(U):                                               # spans in order, inside [0, n)
            assert 0 <= r.tok_begin[u] < r.tok_end[u] <= n
            assert u == 0 or r.tok_end[u - 1] <= r.tok_begin[u]
            assert all(s == 2 * u + 1 for s in r.path[r.tok_begin[u]:r.tok_end[u]])
        assert r.score <= 1e-9 + A.ctc_log_likelihood(m["x"][b, :n], t, m["blank"]), (name, b)


def test_best_path_is_the_best_of_all_paths_on_small_lattices():
    """Against every alignment enumerated: V^T label sequences that collapse to the targets."""
    import itertools
    g = torch.Generator().manual_seed(11)
    for T, V, targets in ((4, 3, [1, 1]), (5, 3, [2, 1]), (4, 4, [3]), (3, 3, [])):
        x = torch.log_softmax(2.0 * torch.randn(T, V, generator=g, dtype=torch.float64), dim=-1)
        best = -math.inf
        for seq in itertools.product(range(V), repeat=T):
            out, prev = [], None
            for c in seq:
                if c != prev and c != 0:
                    out.append(c)
                prev = c
            if out == targets:
                best = max(best, float(sum(x[t, c] for t, c in enumerate(seq))))
        r = A.align(x, targets)
        assert r.ok and abs(r.score - best) < 1e-12 and abs(r.raw_score - best) < 1e-12


# ------------------------------------------------------------------ 3. the host side of the entry


def test_workspace_size_and_form_are_pure_host_functions():
    N, lib = _lib()
    budget, ws = N.const("S2T_CTC_ALIGN_LDS_BYTES"), N.const("S2T_CTC_ALIGN_FORM_WORKSPACE")
    assert ws == C._WS
    for name, want in C.FORMS.items():
        m = C.make(name)
        assert lib.s2t_ctc_align_form(m["T"], m["U"]) == want, name
    assert set(C.FORMS) == set(C.CASES)
    assert {f & (ws - 1) for f in C.FORMS.values()} == {1, 2, 4, 8, 16}       # every states-per-thread variant
    assert {f & (ws - 1) for f in C.FORMS.values() if f & ws} >= {1, 4, 8, 16}
    for U in (0, 5, 63, 64, 255, 256, 1023):                                 # the edge is where the header says
        S = 2 * U + 1
        fit = budget // (16 * ((S + 63) // 64) + 2)
        assert lib.s2t_ctc_align_form(fit, U) & ws == 0 and lib.s2t_ctc_align_form(fit + 1, U) & ws == ws
    pad = lambda n: (n + 15) // 16 * 16                                      # noqa: E731
    assert lib.s2t_ctc_align_workspace_bytes(2, 10, 3) == pad(4 * 20) + pad(4 * 20 * 7)
    assert lib.s2t_ctc_align_workspace_bytes(2, 316, 255) == pad(4 * 632) + pad(4 * 632 * 511) + 16 * 632 * 8
    assert lib.s2t_ctc_align_workspace_bytes(2, 10, 1024) == 0 and lib.s2t_ctc_align_workspace_bytes(2, 0, 3) == 0
    assert lib.s2t_ctc_align_form(0, 3) == -1 and lib.s2t_ctc_align_form(5, 1024) == -1
    assert lib.s2t_ctc_align_form(5, -1) == -1


@pytest.mark.parametrize("change, code", [
    (dict(B=0), 0), (dict(B=-1), 0), (dict(T=0), -1), (dict(V=0), -1), (dict(U=-1), -1), (dict(blank=-1), -1),
    (dict(blank=8), -1), (dict(stride=3), -1), (dict(null="ws"), -1), (dict(null="path"), -1),
    (dict(null="tok_begin"), -1), (dict(null="tok_end"), -1), (dict(null="tok_logp"), -1), (dict(null="raw"), -1),
    (dict(null="score"), -1), (dict(null="ok"), -1), (dict(U=1024, stride=1024), -4)], ids=str)
def test_refusals_come_before_any_launch_and_follow_no_pointer(change, code):
    """Every data pointer is NULL or an address nothing is mapped at: a refusal that followed one, or
    launched anything, would not return."""
    _, lib = _lib()
    bad = 8                                                  # never dereferenced
    a = dict(B=2, T=5, V=8, U=4, blank=0, stride=4)
    a.update({k: v for k, v in change.items() if k != "null"})
    out = {k: bad for k in ("ws", "path", "tok_begin", "tok_end", "tok_logp", "raw", "score", "ok")}
    if "null" in change:
        out[change["null"]] = None
    rc = lib.s2t_ctc_align(None, None, None, a["stride"], None, a["B"], a["T"], a["V"], a["U"], a["blank"], out["ws"],
                           out["path"], out["tok_begin"], out["tok_end"], out["tok_logp"], out["raw"], out["score"],
                           out["ok"], None)
    assert rc == code


def test_python_surface_refuses_host_tensors_and_wide_labels():
    from speech2text_amd import kernels
    x, n = torch.zeros(1, 4, 5), torch.tensor([4])
    with pytest.raises(RuntimeError, match="device tensor"):
        kernels.ctc_align(x, n, torch.ones(1, 2, dtype=torch.int64), torch.tensor([2]))


# ------------------------------------------------------------------ 4. words
class _Span:
    def __init__(self, begin, end, logp):
        self.begin, self.end, self.logp = begin, end, logp


def test_merge_words_char_tokenizer():
    from speech2text_amd.dataset.utils import CharTokenizer, CharTokenizerConfig
    from speech2text_amd.model.alignment import merge_words
    tok = CharTokenizer(CharTokenizerConfig())
    ids = tok.encode("it's a  dog ").tolist()
    pieces = [tok.labels[i] for i in ids]
    spans = [_Span(3 * i, 3 * i + 2, -0.5 * (i + 1)) for i in range(len(ids))]
    words = merge_words(pieces, spans)
    assert [w.word for w in words] == ["it's", "a", "dog"]
    assert [(w.begin, w.end) for w in words] == [(0, 11), (15, 17), (24, 32)]   # spaces belong to no word
    assert words[0].logp == pytest.approx(-0.5 * (1 + 2 + 3 + 4)) and words[1].logp == -0.5 * 6
    assert merge_words([], []) == [] and merge_words([" "], [_Span(0, 1, 0.0)]) == []


def test_merge_words_subword_tokenizer(golden_dir):
    from speech2text_amd.model.alignment import WORD_MARK, merge_words
    root = os.path.join(golden_dir, "reference_configs", "sample_data", "spm")
    text = "the quick brown fox jumps"
    try:
        import sentencepiece  # noqa: F401
        from speech2text_amd.dataset.utils import SubwordTokenizer, SubwordTokenizerConfig
        tok = SubwordTokenizer(SubwordTokenizerConfig(os.path.join(root, "tokenizer.model"),
                                                      os.path.join(root, "tokenizer.vocab")))
        pieces = tok.encode_as_tokens(text)
    except ImportError:                                      # a stub with the same marks
        pieces = [WORD_MARK + "the", WORD_MARK + "qu", "ick", WORD_MARK, "brown", WORD_MARK + "fox", WORD_MARK + "jump", "s"]
    assert len(pieces) > len(text.split()) or all(p.startswith(WORD_MARK) for p in pieces)
    spans = [_Span(2 * i, 2 * i + 1, -1.0) for i in range(len(pieces))]
    words = merge_words(pieces, spans)
    assert [w.word for w in words] == text.split()
    opens = [i for i, p in enumerate(pieces) if p.startswith(WORD_MARK)]
    assert [w.begin for w in words] == [2 * i for i in opens]
    assert [w.end for w in words] == [2 * i - 1 for i in opens[1:]] + [2 * len(pieces) - 1]
    assert sum(w.logp for w in words) == -float(len(pieces))


# ------------------------------------------------------------------ 5. the aligner's host loop
@pytest.mark.parametrize("name", ["u0_b17_ragged", "u3_tight_aab", "u7_v65_b17_ragged", "u9_v11_logp_inf",
                                  "ties_v11_b17", "u64_v65"])
def test_aligner_host_loop_is_the_restatement(name):
    from speech2text_amd.model.alignment import CtcForcedAligner
    m = C.make(name)
    al = CtcForcedAligner(blank=m["blank"], frame_seconds=0.04)
    x = m["x"]                                                           # NaN past the lengths: never read
    rows = al._rows(x, m["lens"], m["targets"][:, :m["U"]], m["tl"])
    path, tb, te, lp, raw, score, ok = C.dense(C.restated(name), m["T"], m["U"])
    assert torch.equal(rows.ok, ok) and torch.equal(rows.path, path)
    assert torch.equal(rows.tok_begin, tb) and torch.equal(rows.tok_end, te)
    assert torch.equal(rows.raw_score.double(), raw)
    es, el = C.errors(rows.score, rows.tok_logp, name)
    assert es <= C.bound(name) and el <= C.bound(name), (es, el)
    out = al.align(x, m["lens"], m["targets"][:, :m["U"]], m["tl"])
    for b, (a, r) in enumerate(zip(out, C.restated(name))):
        assert a.ok == r.ok and [t.begin for t in a.tokens] == (r.tok_begin if r.ok else [])
        assert [t.end for t in a.tokens] == (r.tok_end if r.ok else []) and a.words == []
        assert all(t.begin_s == t.begin * 0.04 and t.end_s == t.end * 0.04 for t in a.tokens)
        assert [t.token for t in a.tokens] == (m["targets"][b, :len(r.tok_begin)].tolist() if r.ok else [])


def test_align_text_gives_words_with_times():
    from speech2text_amd.dataset.utils import CharTokenizer, CharTokenizerConfig
    from speech2text_amd.model.alignment import CtcForcedAligner
    tok = CharTokenizer(CharTokenizerConfig())
    V = len(tok.labels)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 30, V, generator=g)
    al = CtcForcedAligner(tok, frame_seconds=0.04)
    out = al.align_text(x, torch.tensor([30, 4]), ["go to bed", "far too long for four frames"])
    assert out[0].ok and [w.word for w in out[0].words] == ["go", "to", "bed"]
    assert "".join(t.piece for t in out[0].tokens) == "go to bed"
    w = out[0].words
    assert all(a.end <= b.begin for a, b in zip(w, w[1:])) and w[0].begin >= 0 and w[-1].end <= 30
    assert all(x.begin_s == x.begin * 0.04 and x.end_s == x.end * 0.04 for x in w)
    assert not out[1].ok and out[1].tokens == [] and out[1].score == -math.inf
