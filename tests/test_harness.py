"""CPU: the test scaffolding itself -- tests/yardstick.py (the bound rule and its error measure),
tests/guarded.py (the guarded buffer and `hold`) and the rule that no test module is another's library.

Nothing else tests the tests: a guard that became shorter, a `hold` that stops at its first miss or a
measure that broadcasts would weaken every kernel test at once and fail none of them.  The buffers are
built on the CPU here (torch's CPU allocations are 64-byte aligned, so the alignment assertion holds).
"""
import ast
import glob
import importlib
import os
import types

import pytest
import torch

import guarded
import yardstick
from guarded import ISENT, NAN, SENT, Buf, hold

CPU = torch.device("cpu")
SHAPES = [(5,), (3, 7), (2, 3, 130)]                    # the last dimension of the third is above the 64 floor
FILLS = [(NAN, torch.float32), (SENT, torch.float32), (ISENT, torch.int64)]
FILL_IDS = ["nan", "sent", "isent"]
RULE_MODULES = ("lstm_cases", "rnn_lm_cases", "conf_cases", "zip_cases", "zipconv_cases", "zipattn_cases",
                "front_cases", "ctc_align_cases", "ctc_prefix_cases", "ctc_ngram_cases")
# these take the measure and the constants under the names their tests use (COST_MARGIN: MARGIN is their
# decision margin), or the measure alone where their bound is a neighbour's
RULE_MEASURE_ONLY = ("rnnt_lstm_search_cases", "rnnt_ngram_cases", "rnnt_lstm_ngram_cases", "rnnt_lm_fusion_cases",
                     "rnnt_stateless_lm_cases")
# the coverage checks import a GPU file in order to inspect it (COVER / RUNS / HELPERS, inspect.getsource)
COVERAGE_CHECKS = {("test_front_f64", "test_gpu_front_kernels"), ("test_zipconv_f64", "test_gpu_zip_conv_kernels"),
                   ("test_zipattn_f64", "test_gpu_zip_attn_kernels")}


def _other(fill):
    return 1 if fill != fill or fill != 1 else 2


def _cases(mis_too=True):
    return [pytest.param(shape, fill, dtype, mis, id=f"{'x'.join(map(str, shape))}-{fid}{'-mis' if mis else ''}")
            for shape in SHAPES for (fill, dtype), fid in zip(FILLS, FILL_IDS)
            for mis in ((False, True) if mis_too and dtype == torch.float32 else (False,))]


# ------------------------------------------------------------------ Buf
@pytest.mark.parametrize("shape,fill,dtype,mis", _cases())
def test_a_fresh_buffer_is_intact_untouched_and_guarded(shape, fill, dtype, mis):
    b = Buf(CPU, shape, mis=mis, fill=fill, dtype=dtype)
    b.intact("fresh")
    b.untouched("fresh")
    assert b.t.shape == shape and b.t.dtype == dtype and b.t.is_contiguous()
    assert b.t.data_ptr() % 16 == (4 if mis else 0)
    assert b.t.data_ptr() == b.full.data_ptr() + (4 if mis else 0)
    assert b.full.numel() - b.t.numel() - (1 if mis else 0) >= max(64, shape[-1])


@pytest.mark.parametrize("shape,fill,dtype,mis", _cases())
def test_intact_sees_a_write_at_either_end_of_the_guard_and_in_front(shape, fill, dtype, mis):
    for where in ("first", "last") + (("front",) if mis else ()):
        b = Buf(CPU, shape, mis=mis, fill=fill, dtype=dtype)
        n = b.t.numel()
        at = {"first": b.off + n, "last": b.full.numel() - 1, "front": 0}[where]
        b.t.fill_(_other(fill))                          # writing the buffer itself is what a kernel is for
        b.intact(f"{where}: only the buffer written")
        b.full[at] = _other(fill)
        with pytest.raises(AssertionError, match="in front of" if where == "front" else "guard behind"):
            b.intact(where)
        with pytest.raises(AssertionError, match="refused call"):
            b.untouched(where)


@pytest.mark.parametrize("shape,fill,dtype,mis", _cases())
def test_untouched_sees_a_write_of_any_interior_element(shape, fill, dtype, mis):
    n = Buf(CPU, shape, mis=mis, fill=fill, dtype=dtype).t.numel()
    for i in sorted({0, 1, n // 2, n - 1}):
        b = Buf(CPU, shape, mis=mis, fill=fill, dtype=dtype)
        b.t.view(-1)[i] = _other(fill)
        b.intact("an interior write leaves the guard alone")
        with pytest.raises(AssertionError, match="refused call"):
            b.untouched(f"element {i}")


@pytest.mark.parametrize("shape,fill,dtype,mis", _cases())
def test_src_is_copied_and_leaves_the_guard_intact(shape, fill, dtype, mis):
    src = torch.arange(1, 1 + torch.Size(shape).numel()).to(dtype)
    b = Buf(CPU, shape, src=src, mis=mis, fill=fill, dtype=dtype)
    assert torch.equal(b.t, src.reshape(shape))
    b.intact("after the copy")
    with pytest.raises(AssertionError):
        b.untouched("the copy wrote the buffer")


def test_a_scalar_shape_is_a_vector_and_ptr_takes_buffers_tensors_and_none():
    b = Buf(CPU, 9)
    assert b.t.shape == (9,) and bool(torch.isnan(b.full).all())
    t = torch.zeros(3)
    assert guarded.ptr(b) == b.t.data_ptr() and guarded.ptr(t) == t.data_ptr() and guarded.ptr(None) is None
    with pytest.raises(AssertionError, match="float32"):
        Buf(CPU, 4, mis=True, fill=ISENT, dtype=torch.int64)


# ------------------------------------------------------------------ hold
def _stub(ref, bounds, exact_ref=None, exact_tensors=()):
    """A case module in miniature: reference(name[, exact]), bound(name, key), rel_err, EXACT_TENSORS."""
    def reference(name, exact=False):
        return exact_ref if exact else ref
    return types.SimpleNamespace(reference=reference, bound=lambda name, k: bounds[k], rel_err=yardstick.rel_err,
                                 EXACT_TENSORS=exact_tensors)


REF = dict(a=torch.tensor([1.0, -2.0, 4.0], dtype=torch.float64), b=torch.ones(2, 3, dtype=torch.float64))
BOUNDS = dict(a=1e-3, b=1e-6)


def _got(da=0.0, db=0.0):
    return dict(a=(REF["a"] + da).float(), b=(REF["b"] + db).float())


def test_hold_passes_within_the_bound_and_prints_one_line_per_tensor(capsys):
    hold(_stub(REF, BOUNDS), "case", _got(da=2e-3))                       # 2e-3 / 4 = 5e-4 <= 1e-3
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("case a: err 5.000e-04 bound 1.000e-03 ratio 0.500")
    hold(_stub(REF, BOUNDS), "case", dict(a=_got()["a"].reshape(3, 1), b=_got()["b"].reshape(6)))   # reshaped


def test_hold_reports_every_tensor_over_its_bound_in_one_failure():
    with pytest.raises(AssertionError) as e:
        hold(_stub(REF, BOUNDS), "case", _got(da=1e-2, db=1e-3))
    msg = str(e.value)
    assert "case a: err 2.500e-03 > bound 1.000e-03" in msg and "case b: err 1.000e-03 > bound 1.000e-06" in msg


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_hold_fails_on_a_tensor_that_is_not_finite(bad):
    got = _got()
    got["b"][1, 2] = bad
    with pytest.raises(AssertionError, match="case b: not finite"):
        hold(_stub(REF, BOUNDS), "case", got)


def test_hold_fails_on_a_missing_or_an_extra_key_unless_partial():
    got = _got()
    with pytest.raises(AssertionError, match="against the reference's"):
        hold(_stub(REF, BOUNDS), "case", dict(a=got["a"]))
    hold(_stub(REF, BOUNDS), "case", dict(a=got["a"]), partial=True)
    with pytest.raises(AssertionError, match="against the reference's"):
        hold(_stub(REF, BOUNDS), "case", dict(got, c=got["a"]))
    with pytest.raises(AssertionError, match="case a: err"):               # partial still holds what is there
        hold(_stub(REF, BOUNDS), "case", dict(a=got["a"] + 1), partial=True)


def test_hold_honours_alias_a_given_reference_and_lists():
    got = _got()
    hold(_stub(REF, BOUNDS), "case", {"a": got["a"], "a@again": got["a"], "b": got["b"]}, alias={"a@again": "a"})
    with pytest.raises(AssertionError, match="case a@again: err"):
        hold(_stub(REF, BOUNDS), "case", {"a": got["a"], "a@again": got["a"] * 2, "b": got["b"]},
             alias={"a@again": "a"})
    other = dict(a=REF["a"] * 3, b=REF["b"])
    hold(_stub(REF, BOUNDS), "case", dict(a=got["a"] * 3, b=got["b"]), ref=other)
    lists = dict(g=[REF["a"], REF["b"]])
    hold(_stub(lists, dict(g=1e-6)), "case", dict(g=[got["a"], got["b"]]))
    with pytest.raises(AssertionError, match="case g: err"):              # each item relative to its own reference
        hold(_stub(lists, dict(g=1e-6)), "case", dict(g=[got["a"], got["b"] + 1e-3]))
    with pytest.raises(AssertionError, match="case g: not finite"):
        hold(_stub(lists, dict(g=1e-6)), "case", dict(g=[got["a"], got["b"] * float("inf")]))


def test_hold_compares_exact_tensors_for_equality_and_names_the_indices():
    exact = dict(a=torch.tensor([1.0, -2.0, 4.0], dtype=torch.float64), b=2 * torch.ones(2, 3, dtype=torch.float64))
    stub = _stub(REF, BOUNDS, exact_ref=exact, exact_tensors=("b",))
    hold(stub, "case", dict(a=exact["a"].float() + 1e-4, b=exact["b"].float()), exact=True)      # a: by its bound
    off = exact["b"].float().clone()
    off[1, 2] += 2.0 ** -22                               # far inside b's bound, and still not equal
    with pytest.raises(AssertionError, match=r"case b: differs from the reference on exact inputs at \[\[1, 2\]\]"):
        hold(stub, "case", dict(a=exact["a"].float(), b=off), exact=True)
    hold(_stub(exact, BOUNDS), "case", dict(a=exact["a"].float(), b=off))          # not exact: held by its bound


# ------------------------------------------------------------------ yardstick
def test_the_rule_and_its_constants():
    assert yardstick.FLOOR == 2e-5 and yardstick.MARGIN == 8.0 and yardstick.UNIT == 2 ** -24
    assert yardstick.bound_of(0.0) == 2e-5 and yardstick.bound_of(2.5e-6) == 2e-5
    assert yardstick.bound_of(1e-5) == 8e-5


def test_rel_err_is_relative_to_the_largest_reference_entry_and_refuses_other_shapes():
    ref = torch.tensor([[1.0, -4.0]], dtype=torch.float64)
    assert yardstick.rel_err(torch.tensor([[1.5, -4.0]]), ref) == 0.125
    assert yardstick.rel_err([ref.float(), ref.float() + 1], [ref, ref]) == 0.25
    for got in (torch.zeros(2), torch.zeros(1, 1), torch.zeros(2, 1), torch.zeros(())):
        with pytest.raises(AssertionError, match="shape"):
            yardstick.rel_err(got, ref)


@pytest.mark.parametrize("module", RULE_MODULES + RULE_MEASURE_ONLY)
def test_every_case_module_that_follows_the_rule_takes_it_from_yardstick(module):
    m = importlib.import_module(module)
    assert m.rel_err is yardstick.rel_err
    if module in RULE_MODULES:
        assert m.FLOOR == yardstick.FLOOR and m.MARGIN == yardstick.MARGIN
    for name, want in (("FLOOR", yardstick.FLOOR), ("COST_MARGIN", yardstick.MARGIN), ("UNIT", yardstick.UNIT)):
        if hasattr(m, name):
            assert getattr(m, name) == want, (module, name)


# ------------------------------------------------------------------ layout
def test_no_test_module_is_another_modules_library():
    """Helpers shared between test files live in modules whose names do not start with test_ (yardstick,
    guarded, decode_support, task_support, the *_cases and *_f64 modules).  Importing a test module runs its
    parametrisation and hides a dependency between tests; only the coverage checks may, to inspect a GPU file."""
    here = os.path.dirname(os.path.abspath(__file__))
    found = set()
    for path in sorted(glob.glob(os.path.join(here, "*.py"))):
        importer, src = os.path.basename(path)[:-3], open(path).read()
        if "import test_" not in src and "from test_" not in src:      # nothing for the parser to find
            continue
        for node in ast.walk(ast.parse(src)):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom) and node.module:
                names = [node.module] + [a.name for a in node.names]
            found |= {(importer, n.split(".")[-1]) for n in names if n.split(".")[-1].startswith("test_")}
    assert found == COVERAGE_CHECKS, sorted(found ^ COVERAGE_CHECKS)
