"""CPU: the C-ABI library loads and exports every symbol include/s2t_mi355.h declares; the structs and
constants Python takes from that header are the compiler's; the plan rule; the build's dependencies."""
import ctypes
import keyword
import os
import re
import subprocess

import pytest

from speech2text_amd import _native


def test_header_symbols_exported():
    protos = _native.parse_header()
    assert len(protos) >= 10
    assert os.path.exists(_native.LIB_PATH), "build first: python -m speech2text_amd.csrc.build"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"


def test_ctc_workspace_size_is_pure_host_function():
    lib = _native.lib()
    assert lib.s2t_ctc_workspace_floats(2, 10, 3) == 2 * 10 + 3 * 2 * 10 * 7 + 2   # lse + lp,alpha,beta + nll


def test_ctc_search_size_queries_are_pure_host_functions():
    """Every size query of the CTC prefix beam search at two shapes: the bytes the layouts took before one
    arena handed them out (literals of the library built from that commit: trie nodes of 16 bytes, every
    array rounded up to 256 bytes).  An LM desc with only V, E, H and num_layers filled is enough: no query
    reads a weight.  One refused shape per query answers 0."""
    lib = _native.lib()
    Lm = _native.parse_abi(open(_native.HEADER_PATH).read())[1]["S2tRnnLmDesc"]

    def lm(V, E, H, layers):
        d = Lm()
        d.V, d.E, d.H, d.num_layers = V, E, H, layers
        return ctypes.byref(d)

    B, T, V, beam, nodes, d = 2, 30, 50, 4, 100, lm(50, 16, 32, 2)
    assert lib.s2t_ctc_prefix_beam_workspace_bytes(B, T, V, beam) == 4096
    assert lib.s2t_ctc_prefix_beam_ngram_workspace_bytes(B, T, V, beam) == 4096
    assert lib.s2t_ctc_prefix_beam_lm_workspace_bytes(d, B, T, V, beam) == 26112
    assert lib.s2t_ctc_stream_state_bytes(B, V, beam, nodes) == 10496
    assert lib.s2t_ctc_ngram_stream_state_bytes(B, V, beam, nodes) == 10752     # + the context ids
    assert lib.s2t_ctc_bias_stream_state_bytes(B, V, beam, nodes) == 11008      # + the graph states and sums
    assert lib.s2t_ctc_ngram_bias_stream_state_bytes(B, V, beam, nodes) == 11264
    assert lib.s2t_ctc_lm_stream_state_bytes(d, B, V, beam, nodes) == 17152
    assert lib.s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(d, B, V, beam) == 13312

    B, T, V, beam, nodes, d = 1, 1, 7, 1, 1, lm(7, 8, 4, 1)
    assert lib.s2t_ctc_prefix_beam_workspace_bytes(B, T, V, beam) == 256
    assert lib.s2t_ctc_prefix_beam_ngram_workspace_bytes(B, T, V, beam) == 256
    assert lib.s2t_ctc_prefix_beam_lm_workspace_bytes(d, B, T, V, beam) == 6400
    assert lib.s2t_ctc_stream_state_bytes(B, V, beam, nodes) == 3584
    assert lib.s2t_ctc_ngram_stream_state_bytes(B, V, beam, nodes) == 3840
    assert lib.s2t_ctc_bias_stream_state_bytes(B, V, beam, nodes) == 4096
    assert lib.s2t_ctc_ngram_bias_stream_state_bytes(B, V, beam, nodes) == 4352
    assert lib.s2t_ctc_lm_stream_state_bytes(d, B, V, beam, nodes) == 5120
    assert lib.s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(d, B, V, beam) == 2560

    beam_max, nodes_max = _native.const("S2T_RNNT_LSTM_MAX_BEAM"), _native.const("S2T_CTC_STREAM_MAX_NODES")
    assert lib.s2t_ctc_prefix_beam_workspace_bytes(0, 30, 50, 4) == 0                   # no batch
    assert lib.s2t_ctc_prefix_beam_ngram_workspace_bytes(2, -1, 50, 4) == 0             # T < 0
    assert lib.s2t_ctc_prefix_beam_lm_workspace_bytes(lm(49, 16, 32, 2), 2, 30, 50, 4) == 0   # the LM's V is not V
    assert lib.s2t_ctc_stream_state_bytes(2, 50, beam_max + 1, 100) == 0
    assert lib.s2t_ctc_ngram_stream_state_bytes(2, 50, 4, 0) == 0                       # no node for the root
    assert lib.s2t_ctc_bias_stream_state_bytes(2, 50, 4, nodes_max + 1) == 0
    assert lib.s2t_ctc_ngram_bias_stream_state_bytes(2, 0, 4, 100) == 0
    assert lib.s2t_ctc_lm_stream_state_bytes(lm(50, 16, 30, 2), 2, 50, 4, 100) == 0     # H is no multiple of 4
    assert lib.s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(None, 2, 50, 4) == 0


def test_rnnt_search_size_queries_are_pure_host_functions():
    """The four size queries of the one-launch stateless RNN-T searches (csrc/decode_rnnt.hip) at two shapes:
    literals of the library built from the commit before the queries got one size function, their refusals'
    zeros, and the one place the two workspace queries have always disagreed: the plain one does not refuse a
    V or a beam past the search's limits."""
    lib = _native.lib()
    B, T, V, ctx, beam, max_tokens = 2, 30, 50, 2, 4, 16
    assert lib.s2t_rnnt_beam_workspace_bytes(B, T, V, beam) == 2816
    assert lib.s2t_rnnt_beam_ngram_workspace_bytes(B, T, V, beam) == 2816
    assert lib.s2t_rnnt_stream_state_bytes(B, V, ctx, beam, max_tokens) == 13312
    assert lib.s2t_rnnt_stream_state_bytes(B, V, ctx, 0, max_tokens) == 512              # greedy rows
    assert lib.s2t_rnnt_ngram_stream_state_bytes(B, V, ctx, beam, max_tokens) == 13824   # + contexts and LM sums

    B, T, V, ctx, beam, max_tokens = 3, 50, 500, 5, 16, 1024
    assert lib.s2t_rnnt_beam_workspace_bytes(B, T, V, beam) == 105728
    assert lib.s2t_rnnt_beam_ngram_workspace_bytes(B, T, V, beam) == 105728
    assert lib.s2t_rnnt_stream_state_bytes(B, V, ctx, beam, max_tokens) == 933888
    assert lib.s2t_rnnt_stream_state_bytes(B, V, ctx, 0, max_tokens) == 6144
    assert lib.s2t_rnnt_ngram_stream_state_bytes(B, V, ctx, beam, max_tokens) == 934656

    for q in (lib.s2t_rnnt_beam_workspace_bytes, lib.s2t_rnnt_beam_ngram_workspace_bytes):
        assert [q(0, 30, 50, 4), q(2, 0, 50, 4), q(2, 30, 0, 4), q(2, 30, 50, 0)] == [0, 0, 0, 0]
    assert lib.s2t_rnnt_beam_workspace_bytes(2, 30, 8193, 4) == 263424                   # (not refused)
    assert lib.s2t_rnnt_beam_ngram_workspace_bytes(2, 30, 8193, 4) == 0
    assert lib.s2t_rnnt_beam_workspace_bytes(2, 30, 50, 17) == 11008                     # (not refused)
    assert lib.s2t_rnnt_beam_ngram_workspace_bytes(2, 30, 50, 17) == 0
    for q in (lib.s2t_rnnt_stream_state_bytes, lib.s2t_rnnt_ngram_stream_state_bytes):
        assert [q(0, 50, 2, 4, 16), q(2, 0, 2, 4, 16), q(2, 8193, 2, 4, 16), q(2, 50, 0, 4, 16), q(2, 50, 65, 4, 16),
                q(2, 50, 2, -1, 16), q(2, 50, 2, 17, 16), q(2, 50, 2, 4, 0)] == [0] * 8
    assert lib.s2t_rnnt_ngram_stream_state_bytes(2, 50, 2, 0, 16) == 0                   # an n-gram row is a beam row


# ------------------------------------------------------------------ structs and constants from the header
def _c_name(field):
    """The header's name of a parsed field (a Python keyword got a trailing underscore)."""
    return field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field


def test_parsed_structs_match_the_compilers_layout(tmp_path):
    """A host-only program generated from the parse prints sizeof of every struct and offsetof / sizeof
    of every field as the compiler of the library lays the header out: all equal to the ctypes classes."""
    from speech2text_amd.csrc import build
    header = open(_native.HEADER_PATH).read()
    consts, structs = _native.parse_abi(header)
    assert len(structs) == len(re.findall(r"\btypedef\s+struct\b", header)) >= 17    # none skipped
    lines, want = [], []
    for sname, cls in structs.items():
        lines.append(f'  printf("{sname} %zu\\n", sizeof({sname}));')
        want.append(f"{sname} {ctypes.sizeof(cls)}")
        for fname, _ in cls._fields_:
            f = getattr(cls, fname)
            c = _c_name(fname)
            lines.append(f'  printf("{sname}.{c} %zu %zu\\n", offsetof({sname}, {c}), sizeof((({sname}*)0)->{c}));')
            want.append(f"{sname}.{c} {f.offset} {f.size}")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "s2t_mi355.h"\nint main() {\n'
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-I", os.path.dirname(_native.HEADER_PATH),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert got[:-1] == want


@pytest.mark.parametrize("body, what", [
    ("int a;\n  short b;", "unknown type 'short'"),
    ("unsigned long n;", "unknown type 'unsigned long'"),
    ("int a[S2T_NOT_DEFINED];", "undefined array dimension"),
    ("int a : 3;", "cannot parse"),
    ("S2tLater x;", "unknown type 'S2tLater'"),
])
def test_parser_refuses_what_it_does_not_know(body, what):
    txt = "#define S2T_N 4\ntypedef struct S2tBad {\n  float ok[S2T_N];\n  %s\n} S2tBad;\n" \
          "typedef struct { int z; } S2tLater;\n" % body
    with pytest.raises(ValueError, match=what) as e:
        _native.parse_abi(txt)
    assert "S2tBad" in str(e.value)                        # names the struct (and quotes the declaration)
    good = _native.parse_abi(txt.replace(body, "const float *p, *q; /* trailing */"))[1]["S2tBad"]
    assert [n for n, _ in good._fields_] == ["ok", "p", "q"] and ctypes.sizeof(good) == 32


def test_header_constants():
    header = open(_native.HEADER_PATH).read()
    found = dict(re.findall(r"#define\s+(S2T_\w+)\s+(\d+)\s*(?:/\*.*)?$", header, re.M))
    for name in ("S2T_CTC_MAX_LABELS", "S2T_BN_PARTIALS", "S2T_ADAM_MAX_GROUPS", "S2T_ZL_NDEC", "S2T_ZL_NWHITEN"):
        assert _native.const(name) == int(found[name])
    assert {k: int(v) for k, v in found.items()} == _native.parse_abi(header)[0]
    from speech2text_amd import kernels, zip_native
    assert zip_native.NDEC == len(zip_native.Call().dec) == int(found["S2T_ZL_NDEC"])
    assert zip_native.NWHITEN == int(found["S2T_ZL_NWHITEN"])
    assert kernels.CTC_MAX_LABELS == int(found["S2T_CTC_MAX_LABELS"])
    assert kernels.NLL_STATS == int(found["S2T_NLL_STATS"]) == 2


# ------------------------------------------------------------------ the plan rule
_EPI = {n: _native.const("S2T_ZL_EPI_" + n.upper())
        for n in ("act_src", "resid2", "resid_b", "act2_swoosh", "act2_add", "bal")}


def _python_rule(t_lib, t_own, R, cols, margin, act_src=False, resid2=False, resid_b=False, act2=None, bal=False):
    """The rule as zip_kernels.lt_matmul computed it before it moved into the library (act2: None |
    "swoosh_l" | "swoosh_r" | "add").  Refuses an input whose decision rests on less than 1 us."""
    fused = act_src or act2 is not None or resid_b
    rc = float(R) * cols
    pass_ms = 4.0e-3 + 12.0 * rc / 3.0e9
    n_pass = act_src + (act_src and resid2) + resid_b + (act2 in ("swoosh_l", "swoosh_r")) + bal
    n_ops = act_src + resid_b + (act2 is not None) + bal
    cost_lt = t_lib * (1.0 if fused else margin) + n_pass * pass_ms
    cost_own = t_own + n_ops * 4.0 * rc / 3.0e9
    assert abs(cost_own - cost_lt) >= 1.0e-3
    return cost_own < cost_lt


def test_plan_rule_is_the_python_rule():
    """s2t_zl_plan_choose against the arithmetic zip_kernels.lt_matmul held until the two copies became one:

        rc      = rows * cols                      (cols = N forward, K data gradient)
        pass_ms = 4.0e-3 + 12.0 * rc / 3.0e9       (one elementwise pass: 2 reads + 1 write at 3 TB/s)
        n_pass  = act_src + (act_src and resid2) + resid_b + (act2 is a Swoosh) + bal
        n_ops   = act_src + resid_b + (act2 is not None) + bal
        cost_lt = t_lib * (1.0 if (act_src or act2 or resid_b) else margin) + n_pass * pass_ms
        cost_own = t_own + n_ops * 4.0 * rc / 3.0e9
        ours iff t_own was measured and cost_own < cost_lt

    on an (N, K) no model has (the per-process table keeps every real bucket), with every decision at
    least 1 us clear of the threshold so that float rounding cannot flip it."""
    from speech2text_amd import zip_kernels as zk
    lib = _native.lib()
    Nf, Kf, R, margin = 7, 13, 64, 0.97
    ho = zk._half_octave(R)

    def choose(mode, rows, **epi):
        bits = sum(_EPI[k] for k, v in epi.items() if v)
        tile = ctypes.c_int(-7)
        return lib.s2t_zl_plan_choose(mode, rows, Nf, Kf, bits, margin, ctypes.byref(tile)), tile.value

    assert choose(0, 4096) == (-1, -7)                                 # bucket never put
    assert lib.s2t_zl_plan_put(0, zk._half_octave(4096), Nf, Kf, 0.100, -1.0, 0) == 0
    assert choose(0, 4096) == (0, -7) and choose(0, 4096, act_src=True, bal=True) == (0, -7)   # no own timing
    assert choose(1, 4096) == (-1, -7)                                 # the data-gradient bucket is another one

    assert lib.s2t_zl_plan_put(0, ho, Nf, Kf, 0.100, 0.098, 321) == 0
    assert choose(0, R) == (0, -7)                 # plain: 0.098 is not below 0.97 * 0.100
    assert choose(0, R, resid2=True) == (0, -7)    # (bias / resid2 ride in the library's product too)
    assert choose(0, R, act_src=True) == (1, 321)  # library: + one pass >= 4 us; ours: + 4 R cols / 3e9 ms
    assert choose(0, R, act_src=True, bal=True) == (1, 321)
    assert choose(0, R, resid_b=True, act2_add=True) == (1, 321)

    assert lib.s2t_zl_plan_put(0, ho, Nf, Kf, 0.100, 0.106, 222) == 0      # ours 6 us slower on the plain product
    assert choose(0, R, act_src=True) == (0, -7)                           # one pass (4 us) does not pay for it
    assert choose(0, R, act_src=True, bal=True) == (1, 222)                # two passes (8 us) do
    assert choose(0, R, act_src=True, resid2=True) == (1, 222)
    assert choose(0, R, resid_b=True, act2_add=True) == (0, -7)            # "add": one pass, the sum is the second output
    assert choose(0, R, resid_b=True, act2_swoosh=True) == (1, 222)        # a Swoosh second output is a pass of its own

    for t_own, tile in ((0.098, 321), (0.106, 222), (0.102, 411)):
        assert lib.s2t_zl_plan_put(0, ho, Nf, Kf, 0.100, t_own, tile) == 0
        assert lib.s2t_zl_plan_put(1, ho, Nf, Kf, 0.100, t_own, tile) == 0
        for act_src in (False, True):
            for resid2 in (False, True):
                for resid_b, act2 in ((False, None), (True, None), (False, "swoosh_r"), (True, "swoosh_l"), (True, "add")):
                    for bal in ((False, True) if act_src and not resid2 and act2 is None and not resid_b else (False,)):
                        for mode, cols in ((0, Nf), (1, Kf)):
                            want = _python_rule(0.100, t_own, R, cols, margin, act_src, resid2, resid_b, act2, bal)
                            got = choose(mode, R, act_src=act_src, resid2=resid2, resid_b=resid_b, bal=bal,
                                         act2_swoosh=act2 in ("swoosh_l", "swoosh_r"), act2_add=act2 == "add")
                            assert got == ((1, tile) if want else (0, -7)), (t_own, mode, act_src, resid2, resid_b, act2, bal)


# ------------------------------------------------------------------ the build
def test_public_header_makes_objects_stale():
    from speech2text_amd.csrc import build
    src = build.sources()[0]
    obj = os.path.join(build.HERE, "build", os.path.basename(src)[:-4] + ".o")
    deps = [src] + build.headers()
    assert _native.HEADER_PATH in deps
    assert os.path.exists(obj) and not build._stale(obj, deps), "build first: python -m speech2text_amd.csrc.build"
    st = os.stat(_native.HEADER_PATH)
    try:
        os.utime(_native.HEADER_PATH, ns=(st.st_atime_ns, os.stat(obj).st_mtime_ns + 10**9))
        assert build._stale(obj, deps)
    finally:
        os.utime(_native.HEADER_PATH, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not build._stale(obj, deps)
