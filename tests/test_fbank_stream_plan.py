"""The integers of the chunk-carried fbank (csrc/fbank_stream.hip s2t_fbank_chunk_f32) and of the audio-in
recogniser, on the CPU: the counting rule `frames_after` and the output bound against a brute-force
framing, the header's declarations, and the ValueErrors that need no device.

The brute force knows nothing of the closed forms: frame f exists once its 400 samples from 160 f are
there, pair p leaves once frames 2p and 2p+1 both exist, a flush adds every frame that exists."""
import pytest
import torch

from speech2text_amd import _native as N
from speech2text_amd import kernels as K
from speech2text_amd.dataset.frontend.frontend import KaldiWaveFeature, LhotseKaldiFeatFbank, StreamingFbank
from speech2text_amd.model.encoder.zipformer_audio_streaming import AudioStreamingRecognizer, AudioStreamPlan

SPLIT_TOTALS = (399, 400, 401, 559, 560, 561, 719, 720, 880, 881)


def _exists(f, n):
    return 160 * f + 400 <= n


def _brute_frames(n):
    f = 0
    while _exists(f, n):
        f += 1
    return f


def _brute_after(n, ended):
    if ended:
        return _brute_frames(n)
    p = 0
    while _exists(2 * p + 1, n):
        p += 1
    return 2 * p


def test_frames_after_every_total_to_2000():
    for n in range(2001):
        assert K.fbank_frames(n) == _brute_frames(n), n
        live, done = K.fbank_frames_after(n, False), K.fbank_frames_after(n, True)
        assert live == _brute_after(n, False) and done == _brute_after(n, True), n
        assert live % 2 == 0 and done - live in (0, 1) and done == K.fbank_frames(n), n
        carry = n - 160 * live                    # samples from the first un-emitted pair's start
        assert 0 <= carry <= K.FBANK_CARRY_MAX, (n, carry)
    assert max(n - 160 * K.fbank_frames_after(n, False) for n in range(2001)) == K.FBANK_CARRY_MAX == 559


@pytest.mark.parametrize("total", SPLIT_TOTALS)
def test_every_split_into_two_calls(total):
    """Whatever the split, a call emits no more than the bound of its own sample count, the carry
    stays within 559 samples, and emitted plus flushed is the one-shot count."""
    for first in range(total + 1):
        a = K.fbank_frames_after(first, False)
        assert a <= K.fbank_chunk_max_frames(first) and first - 160 * a <= 559, (total, first)
        b = K.fbank_frames_after(total, False) - a
        assert 0 <= b <= K.fbank_chunk_max_frames(total - first) - 1, (total, first)
        assert total - 160 * (a + b) <= 559, (total, first)
        flushed = K.fbank_frames_after(total, True) - (a + b)
        assert flushed in (0, 1) and a + b + flushed == _brute_frames(total), (total, first)
        # the flush in the second call itself
        assert K.fbank_frames_after(total, True) - a <= K.fbank_chunk_max_frames(total - first), (total, first)


def test_max_frames_is_reached_and_never_passed():
    """Over every start 0..639 and every call size 0..1300: the bound holds and is no looser than one
    frame (the pairs it counts are always reachable; the flush's lone frame on top of them only from
    161 samples past a multiple of 320 on), and it is reached at 0, 161, 320 and 481 samples."""
    for n in range(1301):
        bound = K.fbank_chunk_max_frames(n)
        assert bound == (1 if n == 0 else 2 * ((n - 1) // 320 + 1) + 1)
        most = 0
        for start in range(640):
            got = K.fbank_frames_after(start + n, True) - K.fbank_frames_after(start, False)
            assert got <= bound, (start, n)
            most = max(most, got)
        assert bound - 1 <= most <= bound, n
        assert most == bound or n not in (0, 161, 320, 481), n


def test_header_declares_the_entry_and_the_carry_constant():
    protos = N.parse_header()
    assert "s2t_fbank_chunk_f32" in protos and "s2t_fbank_chunk_max_frames" in protos
    assert len(protos["s2t_fbank_chunk_f32"][1]) == 22
    assert N.const("S2T_FBANK_CARRY_MAX") == 559 and N.const("S2T_FBANK_STATE_LONGS") == 4
    assert len(protos["s2t_fbank_chunk_f32"][1]) == len(protos["s2t_fbank_f32"][1]) + 3


def test_frames_after_refuses_a_negative_total():
    with pytest.raises(ValueError):
        StreamingFbank.frames_after(-1, False)


@pytest.mark.parametrize("front", [KaldiWaveFeature(num_mel_bins=80), LhotseKaldiFeatFbank(snip_edges=True)],
                         ids=["fbank", "lhotes_fbank"])
def test_streaming_fbank_refuses_sizes_before_touching_a_device(front):
    with pytest.raises(ValueError, match="batch_size"):
        front.streaming(0, 1600)
    with pytest.raises(ValueError, match="max_chunk_samples"):
        front.streaming(2, 0)
    with pytest.raises(ValueError, match="batch_size"):
        K.FbankStreamState(0, "cpu")


def test_audio_recognizer_refuses_what_it_cannot_wrap():
    with pytest.raises(ValueError, match="StreamingRecognizer"):
        AudioStreamingRecognizer(object(), KaldiWaveFeature(num_mel_bins=80))
    for bad in (dict(batch_size=0, chunk=8, max_chunk_samples=100), dict(batch_size=1, chunk=7, max_chunk_samples=100),
                dict(batch_size=1, chunk=8, max_chunk_samples=0)):
        with pytest.raises(ValueError):
            AudioStreamPlan(**bad)


def test_lockstep_rule():
    p = AudioStreamPlan(3, 8, 4800)
    with pytest.raises(ValueError, match="0..4800"):
        p.accept(4801)
    with pytest.raises(ValueError, match="entries"):
        p.accept(100, [100, 100])
    with pytest.raises(ValueError, match="lockstep"):           # fewer samples, not marked last
        p.accept(1600, [1600, 1000, 1600])
    with pytest.raises(ValueError, match="0..1600"):
        p.accept(1600, [1600, 1601, 1600], [False, True, False])
    assert p.samples == [0, 0, 0]                                # a refused call changes nothing
    ns, last, new = p.accept(1600, [1600, 1000, 1600], [False, True, False])
    assert (ns, last, new) == ([1600, 1000, 1600], [False, True, False], [8, 4, 8])
    with pytest.raises(ValueError, match="has ended"):
        p.accept(1600, [1600, 1, 1600])
    with pytest.raises(ValueError, match="has ended"):
        p.accept(0, [0, 0, 0], [False, True, False])
    assert p.accept(1600)[0] == [1600, 0, 1600]                  # None: an ended row takes 0
    p.reset([1])
    assert p.accept(1600)[0] == [1600, 1600, 1600] and p.ended == [False] * 3


def test_plan_walks_the_issue_example_like_recognize():
    """24 300 and 11 650 samples in calls of 1 600, 4 800, 3 000: 150 and 71 frames, 36 and 16 encoder
    frames, nine steps (recognize's K), the chunk lengths recognize gives, row 1 idle in some."""
    p = AudioStreamPlan(2, 8, 4800)
    total, fed, sizes, lens, i = [24300, 11650], [0, 0], (1600, 4800, 3000), [], 0
    while any(f < t for f, t in zip(fed, total)):
        n, i = sizes[i % 3], i + 1
        ns = [0 if p.ended[b] else min(n, total[b] - fed[b]) for b in range(2)]
        last = [not p.ended[b] and fed[b] + ns[b] == total[b] for b in range(2)]
        p.accept(n, ns, last)
        fed = [f + k for f, k in zip(fed, ns)]
        while p.ready():
            lens.append(p.chunk_len())
            p.advance()
    assert p.ended == [True, True] and [p.frames(b) for b in range(2)] == [150, 71]
    while p.ready(True):
        lens.append(p.chunk_len())
        p.advance()
    assert [p.out_frames(b) for b in range(2)] == [36, 16]
    n_out = torch.tensor([36, 16])
    assert lens == [(n_out - k * 4).clamp(0, 4).tolist() for k in range(9)]
    assert any(c[1] == 0 and c[0] > 0 for c in lens)
    q = AudioStreamPlan(1, 8, 100)                               # nothing at all: recognize still steps once
    q.accept(0, [0], [True])
    assert q.ready(True) and q.chunk_len() == [0]
    q.advance()
    assert not q.ready(True)
