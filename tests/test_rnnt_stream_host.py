"""CPU: the host side of the chunk-carried RNN-T search (csrc/decode_rnnt.hip) -- the size of its
state buffer -- and the test's own yardstick: the chunked float64 restatement
(tests/rnnt_stream_restatement.py) against the whole-utterance one on every stored utterance."""

import rnnt_beam_restatement as R
import rnnt_stream_restatement as S
from decode_support import _fixture


def test_state_size_is_a_pure_host_function():
    from speech2text_amd import _native as N
    f = N.lib().s2t_rnnt_stream_state_bytes          # (B, V, ctx, beam_size, max_tokens): no frame count
    for B, V, ctx, beam, mt in ((1, 128, 5, 4, 1024), (3, 500, 5, 16, 1024), (8, 40, 2, 8, 7),
                                (2, 1024, 3, 16, 100), (5, 8192, 64, 16, 3)):
        n = f(B, V, ctx, beam, mt)
        assert n > 0 and n % 256 == 0
        assert n >= 2 * B * beam * mt * (4 + 4)      # two history buffers of int32 tokens and frames
        assert n >= 4 * B * beam * V                 # the beams' lm rows
        assert f(B, V, ctx, beam, mt) == n
        assert f(B, V, ctx, beam, mt + 1) >= n and f(B, V, ctx, beam, 4 * mt) > n   # monotone in max_tokens
        assert f(2 * B, V, ctx, beam, mt) == 2 * n   # a row per stream
        g = f(B, V, ctx, 0, mt)                      # greedy: predictor state + lm vector, no histories
        assert 0 < g < n and g % 256 == 0 and g >= 4 * B * (V + ctx)
        assert f(B, V, ctx, 0, 4 * mt) == g
    assert f(0, 128, 5, 4, 1024) == 0
    assert f(-1, 128, 5, 4, 1024) == 0
    assert f(1, 128, 5, 17, 1024) == 0
    assert f(1, 128, 65, 4, 1024) == 0 and f(1, 128, 0, 4, 1024) == 0
    assert f(1, 8193, 5, 4, 1024) == 0 and f(1, 0, 5, 4, 1024) == 0
    assert f(1, 128, 5, 4, 0) == 0 and f(1, 128, 5, -1, 10) == 0


def _cuts(n, step):
    return list(range(0, n, step)) + [n]


def test_chunked_restatement_equals_the_whole_utterance_one(golden_dir):
    """Every utterance of every stored configuration, fed as 1-frame chunks, 7, 16 and one chunk:
    tokens, frames, score and margin of rnnt_beam_restatement.beam_search, exactly; the common
    prefix of the live beams never shrinks and is a prefix of every later result."""
    fx = _fixture(golden_dir)
    assert len(fx) == 5
    for ci, c in enumerate(fx):
        params = {k: c[k] for k in R.PARAM_KEYS}
        for b in range(8):
            n = int(c["lengths"][b])
            am = c["am"][b, :n]
            want = R.beam_search(am, params, c["ctx"], c["act"], c["beam"], c["topk"])
            assert want[0] == c["tokens"][b]
            for step in (1, 7, 16, n):
                tok, score, frames, margin, stable = S.beam_search_chunked(
                    am, _cuts(n, step), params, c["ctx"], c["act"], c["beam"], c["topk"])
                assert (tok, score, frames, margin) == want, (ci, b, step)
                assert stable == sorted(stable) and stable[-1] <= len(tok), (ci, b, step)
            # an idle call in the middle changes nothing
            idle = S.beam_search_chunked(am, [0, n // 2, n // 2, n], params, c["ctx"], c["act"],
                                         c["beam"], c["topk"])
            assert idle[:4] == want and idle[4][0] == idle[4][1]


def test_common_prefix():
    beams = [((3, 4, 5), (), 0.0, ()), ((3, 4), (), 0.0, ()), ((3, 4, 6, 7), (), 0.0, ())]
    assert S.common_prefix_len(beams) == 2
    assert S.common_prefix_len(beams[:1]) == 3
    assert S.common_prefix_len(beams + [((), (), 0.0, ())]) == 0
    assert S.common_prefix_len([((1, 2), (), 0.0, ()), ((2, 2), (), 0.0, ())]) == 0
    assert S.common_prefix_len(S.initial_beams(5)) == 0
