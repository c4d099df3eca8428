"""The chunk-carried fbank (csrc/fbank_stream.hip s2t_fbank_chunk_f32) against the one-shot kernel, bit for bit.

THE INVARIANT: however a row's samples are cut into calls, the frames it emits, in order, are the rows
of kernels.fbank_batch on the whole audio (torch.equal), their number after the flush is its frame
count, and each call's count is StreamingFbank.frames_after's difference.  The kernel packs frames 2p
and 2p+1 into one complex FFT, and a frame's float32 result depends on its partner at rounding level: a
chunk kernel that pairs by call-local index, emits a lone frame early, or gives a flushed frame an
all-zero partner differs from the one-shot kernel in the last bits, which is what torch.equal sees.

Every call's `out` and both state buffers are guarded buffers of tests/guarded.py (NaN fill: an
unwritten element of `out` fails; the guards behind must be intact).  One case is held to the float64
yardstick (front_f64.fbank_energy_ref under fbank_err and yardstick.bound_of) directly, so that the
file does not stand on the one-shot kernel alone.

Lengths (LENS): 0, 399 (no frame), 400, 401, 559 (one), 560, 561 (two), 720, 881, 5 360, 5 361 (32
frames: one workgroup of the one-shot kernel), 5 520 (33), 11 000 (66 frames: three workgroups in one
call).  Cuts: one call; 1 sample per call (on at most 1 200 samples); 159 / 160 / 161 (the hop); 319 /
320 / 321 (a pair's stride); 559 / 560 / 561 (the first pair); a seeded random cut with calls of 0
samples.  Rows of different lengths end in different calls.
"""
import functools
import random

import pytest
import torch

import front_cases as FC
import front_f64 as FF
from guarded import ISENT, Buf, env

pytestmark = pytest.mark.gpu

IBuf = functools.partial(Buf, fill=ISENT, dtype=torch.int64)
LENS = (0, 399, 400, 401, 559, 560, 561, 720, 881, 5360, 5361, 5520, 11000)
M = 80


@functools.lru_cache(maxsize=None)
def _tables(dev, hf=0.0):
    from speech2text_amd.kernels import FbankTables
    return FbankTables(M, high_freq=hf, device=dev)


@functools.lru_cache(maxsize=None)
def _audio(seed, n, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    return ((0.1 * torch.randn(n, generator=g) + 0.3 * torch.sin(2 * torch.pi * 440.0 * t / 16000.0).float()) * amp)


@functools.lru_cache(maxsize=None)
def _cmvn(dev):
    g = torch.Generator().manual_seed(11)
    return (torch.randn(M, generator=g) - 8.0).to(dev), (0.2 + torch.rand(M, generator=g)).to(dev)


def _one_shot(dev, rows, scale=1.0, cmvn=False, hf=0.0):
    """kernels.fbank_batch on the whole rows -> (feats on the CPU, frame counts)."""
    from speech2text_amd import kernels as K
    lens = [r.numel() for r in rows]
    pcm = torch.zeros(len(rows), max(max(lens), 400))
    for b, r in enumerate(rows):
        pcm[b, :lens[b]] = r
    mean, istd = _cmvn(dev) if cmvn else (None, None)
    feats, frames = K.fbank_batch(pcm.to(dev), torch.tensor(lens, device=dev), _tables(dev, hf), mean, istd, scale)
    return feats.cpu(), frames.tolist()


class _Stream:
    """B streams through s2t_fbank_chunk_f32 on guarded state; collects what each row emits."""

    def __init__(self, dev, B, scale=1.0, cmvn=False, hf=0.0):
        self.dev, self.B, self.scale, self.tab = dev, B, scale, _tables(dev, hf)
        self.mean, self.istd = _cmvn(dev) if cmvn else (None, None)
        self.carry = Buf(dev, (B, 559))
        self.counts = Buf(dev, (B, 4), src=torch.zeros(B, 4, dtype=torch.int64), fill=ISENT, dtype=torch.int64)
        self.fed, self.ended, self.got = [0] * B, [False] * B, [[] for _ in range(B)]

    def reset(self, b):
        self.counts.t[b].zero_()
        self.fed[b], self.ended[b], self.got[b] = 0, False, []

    def call(self, chunks, last=None, width=None):
        """chunks: per row the new samples (a tensor, possibly empty); last: per row.  Checks the counts
        against frames_after, the padding rows and the guards; appends the emitted frames."""
        from speech2text_amd import kernels as K
        N, lib, st = env()
        B, last = self.B, last or [False] * self.B
        n = max(max(c.numel() for c in chunks), 0) if width is None else width
        mf = K.fbank_chunk_max_frames(n)
        pcm = torch.full((B, max(n, 1)), float("nan"))
        for b, c in enumerate(chunks):
            pcm[b, :c.numel()] = c
        pcm = pcm.to(self.dev)
        ns = torch.tensor([c.numel() for c in chunks], device=self.dev)
        fl = torch.tensor([int(v) for v in last], dtype=torch.int32, device=self.dev)
        out, newf = Buf(self.dev, (B, mf, M)), IBuf(self.dev, B)
        N.check(lib.s2t_fbank_chunk_f32(N.fp(pcm), n, N.lp(ns), N.ip(fl), B, N.fp(self.carry.t), N.lp(self.counts.t),
                                        N.fp(self.tab.window), N.fp(self.tab.twiddle), N.ip(self.tab.mel_off),
                                        N.ip(self.tab.mel_k0), N.fp(self.tab.mel_w), self.tab.nnz, M, FF.EPS,
                                        float(self.scale), N.fp(self.mean), N.fp(self.istd), N.fp(out.t), mf,
                                        N.lp(newf.t), st), "s2t_fbank_chunk_f32")
        torch.cuda.synchronize()
        for buf, what in ((out, "out"), (newf, "new_frames"), (self.carry, "carry"), (self.counts, "counts")):
            buf.intact(what)
        o, want = out.t.cpu(), []
        assert bool(torch.isfinite(o).all()), "an element of out was not written"
        pad = torch.zeros(M) if self.mean is None else ((0.0 - self.mean) * self.istd).cpu()
        for b in range(B):
            before = K.fbank_frames_after(self.fed[b], self.ended[b])
            if not self.ended[b]:
                self.fed[b] += chunks[b].numel()
                self.ended[b] = bool(last[b])
            want.append(K.fbank_frames_after(self.fed[b], self.ended[b]) - before)
            self.got[b].append(o[b, :want[b]])
            assert torch.equal(o[b, want[b]:], pad.expand(mf - want[b], M)), f"row {b}: padding rows"
        assert newf.t.tolist() == want
        c = self.counts.t.cpu()
        assert c[:, 0].tolist() == self.fed and c[:, 2].tolist() == [int(e) for e in self.ended]
        assert c[:, 1].tolist() == [K.fbank_frames_after(f, e) for f, e in zip(self.fed, self.ended)]
        return want

    def emitted(self, b):
        return torch.cat(self.got[b]) if self.got[b] else torch.zeros(0, M)


def _feed(s, rows, cut):
    """Every row in calls of `cut` samples (an int, or a list of call sizes cycled); a row is marked
    last in the call that takes its final sample (rows of 0 samples: in the first call)."""
    sizes = [cut] if isinstance(cut, int) else list(cut)
    pos, i = [0] * len(rows), 0
    while not all(s.ended):
        n, i = sizes[i % len(sizes)], i + 1
        chunks, last = [], []
        for b, r in enumerate(rows):
            k = 0 if s.ended[b] else min(n, r.numel() - pos[b])
            chunks.append(r[pos[b]:pos[b] + k])
            pos[b] += k
            last.append(not s.ended[b] and pos[b] == r.numel())
        s.call(chunks, last, width=n)


def _same_as_one_shot(s, ref, frames, rows):
    for b in range(len(rows)):
        got = s.emitted(b)
        assert got.shape[0] == frames[b] == FF.fbank_frames(rows[b].numel()), f"row {b}: frame count"
        assert torch.equal(got, ref[b, :frames[b]]), \
            f"row {b} ({rows[b].numel()} samples): differs from the one-shot kernel in frames " \
            f"{(got != ref[b, :frames[b]]).any(1).nonzero().flatten()[:6].tolist()}"


ROWS3 = [LENS[i:i + 3] for i in range(0, 12, 3)] + [(11000, 5361, 0)]


@pytest.mark.parametrize("lens", ROWS3, ids=lambda v: "-".join(map(str, v)))
def test_one_call_and_hop_cuts(dev, lens):
    """B = 3 rows of different lengths: the whole audio in one call with the flush, and cut at 159 /
    160 / 161 samples; rows end in different calls."""
    rows = [_audio(100 + n, n) for n in lens]
    ref, frames = _one_shot(dev, rows)
    for cut in (max(max(lens), 1), 159, 160, 161):
        s = _Stream(dev, 3)
        _feed(s, rows, cut)
        _same_as_one_shot(s, ref, frames, rows)


@pytest.mark.parametrize("cut", [319, 320, 321, 559, 560, 561])
def test_pair_stride_and_first_pair_cuts(dev, cut):
    rows = [_audio(200 + n, n) for n in (5520, 881, 5361)]
    ref, frames = _one_shot(dev, rows)
    s = _Stream(dev, 3)
    _feed(s, rows, cut)
    _same_as_one_shot(s, ref, frames, rows)


def test_one_sample_per_call(dev):
    """1 200, 881 and 561 samples a sample at a time: every pair boundary is crossed by a call of 1."""
    rows = [_audio(300 + n, n) for n in (1200, 881, 561)]
    ref, frames = _one_shot(dev, rows)
    s = _Stream(dev, 3)
    _feed(s, rows, 1)
    _same_as_one_shot(s, ref, frames, rows)


@pytest.mark.parametrize("variant", ["plain", "cmvn", "scale", "cmvn_scale_hf"])
def test_random_cut_with_empty_calls(dev, variant):
    """A seeded random cut (calls of 0..1 500 samples, a quarter of them 0) of 11 000, 5 520 and 720
    samples; with the fused CMVN, with scale_in = 32768 on samples of +-1, and with both on the
    high_freq = -400 table of lhotes_fbank."""
    cm, sc, hf = "cmvn" in variant, 32768.0 if "scale" in variant else 1.0, -400.0 if "hf" in variant else 0.0
    rows = [_audio(400 + n, n) for n in (11000, 5520, 720)]
    ref, frames = _one_shot(dev, rows, sc, cm, hf)
    rnd = random.Random(17)
    cuts = [0 if rnd.random() < 0.25 else rnd.randrange(1, 1501) for _ in range(64)]
    assert 0 in cuts
    s = _Stream(dev, 3, sc, cm, hf)
    _feed(s, rows, cuts)
    _same_as_one_shot(s, ref, frames, rows)


def test_loud_and_silent_partners_in_different_calls(dev):
    """The signals of fb_loudsilent_i16 (noise of amplitude 0.3 * 32768 next to exact silence, so that
    an all-zero frame is packed with a loud one, as frame A, as frame B and in both positions), cut at
    700 samples: frames 2 and 3, the mixed pair, arrive in different calls (frame 2 is complete at 720
    samples, frame 3 at 880) and the lone frame of an odd count is flushed.  A kernel that pairs by
    call-local index packs them with other partners, and the float32 FFT shows it."""
    t = FC.make("fb_loudsilent_i16")
    rows = [t["pcm"][b, :n].clone() for b, n in enumerate(t["lens"])]
    rows[1] = rows[1][:400 + 160 * 8]                       # nine frames: an odd count, the flush's lone frame
    ref, frames = _one_shot(dev, rows)
    assert frames == [10, 9, 10]
    for cut in (700, 480, 1200):
        s = _Stream(dev, 3)
        _feed(s, rows, cut)
        _same_as_one_shot(s, ref, frames, rows)
    silent = float(torch.log(torch.tensor(FF.EPS)))                # the silent frames ARE there: log(eps)
    assert float((ref[0, 3:10] - silent).abs().max()) < 1e-5 and float((ref[1, :3] - silent).abs().max()) < 1e-5


def test_held_to_float64_directly(dev):
    """fb_ragged (399 ... 5 520 and more samples, noise on a sine) streamed in calls of 1 000 samples,
    each emitted frame against front_f64.fbank_energy_ref under fbank_err, within the case's own bound
    (yardstick.bound_of of the float32 cost of the restatement): not via the one-shot kernel."""
    t = FC.make("fb_ragged")
    rows = [t["pcm"][b, :n].clone() for b, n in enumerate(t["lens"])]
    ref, tol = FC.reference("fb_ragged")["energy"], FC.bound("fb_ragged", "feat")
    assert tol == FC.bound_of(FC.FP32_COST["fb_ragged"]["feat"])
    s = _Stream(dev, len(rows))
    _feed(s, rows, 1000)
    worst = 0.0
    for b in range(len(rows)):
        got = s.emitted(b)
        assert got.shape[0] == ref[b].shape[0]
        worst = max(worst, FF.fbank_err(got, ref[b]))
    print(f"streamed fb_ragged: err {worst:.3e} bound {tol:.3e}")
    assert worst <= tol


def test_reset_mid_stream_and_after_a_flush(dev):
    """Row 1 is reset after 2 000 samples and starts another utterance while rows 0 and 2 go on: all
    three equal their one-shot features.  After its flush a row emits nothing more, takes no samples,
    and neither its carry nor its counts change."""
    a, b1, b2, c = _audio(501, 4000), _audio(502, 2000), _audio(503, 1700), _audio(504, 3333)
    s = _Stream(dev, 3)
    for k in range(2):
        s.call([a[1000 * k:1000 * k + 1000], b1[1000 * k:1000 * k + 1000], c[1000 * k:1000 * k + 1000]])
    s.reset(1)
    s.call([a[2000:3000], b2[:1000], c[2000:3000]])
    s.call([a[3000:4000], b2[1000:1700], c[3000:3333]], [True, True, True])
    ref, frames = _one_shot(dev, [a, b2, c])
    _same_as_one_shot(s, ref, frames, [a, b2, c])
    carry, counts = s.carry.t.clone(), s.counts.t.clone()
    for last in (False, True):
        new = s.call([_audio(505, 900)] * 3, [last] * 3)
        assert new == [0, 0, 0]
        assert torch.equal(s.counts.t, counts)
        assert torch.equal(s.carry.t.view(torch.int32), carry.view(torch.int32))
    _same_as_one_shot(s, ref, frames, [a, b2, c])


def test_refused_sizes(dev):
    """max_new_frames below the bound of pcm_stride, 129 mel bins, a NULL state: -1, nothing written."""
    from speech2text_amd import kernels as K
    N, lib, st = env()
    tab = _tables(dev)
    pcm = torch.zeros(1, 1000, device=dev)
    ns, fl = torch.tensor([1000], device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    need = K.fbank_chunk_max_frames(1000)
    assert need == lib.s2t_fbank_chunk_max_frames(1000) == 9 and lib.s2t_fbank_chunk_max_frames(0) == 1
    for mf, mel, null_state in ((need - 1, M, False), (need, 129, False), (need, M, True)):
        carry = Buf(dev, (1, 559))
        counts = Buf(dev, (1, 4), fill=ISENT, dtype=torch.int64)
        out, newf = Buf(dev, (1, need, 129)), IBuf(dev, 1)
        rc = lib.s2t_fbank_chunk_f32(N.fp(pcm), 1000, N.lp(ns), N.ip(fl), 1, None if null_state else N.fp(carry.t),
                                     N.lp(counts.t), N.fp(tab.window), N.fp(tab.twiddle), N.ip(tab.mel_off),
                                     N.ip(tab.mel_k0), N.fp(tab.mel_w), tab.nnz, mel, FF.EPS, 1.0, None, None,
                                     N.fp(out.t), mf, N.lp(newf.t), st)
        assert rc == -1
        torch.cuda.synchronize()
        for buf in (carry, counts, out, newf):
            buf.untouched(f"s2t_fbank_chunk_f32 at max_new_frames {mf}, {mel} bins")


def test_streaming_fbank_of_both_frontends(dev):
    """_HipFbank.streaming: KaldiWaveFeature and LhotseKaldiFeatFbank (scale_in = 32768 comes along)
    give forward_batch's features through `accept`, fixed buffers and all."""
    from speech2text_amd.dataset.frontend.frontend import KaldiWaveFeature, LhotseKaldiFeatFbank
    rows = [_audio(600, 7000), _audio(601, 4100)]
    pcm = torch.zeros(2, 7000)
    pcm[0], pcm[1, :4100] = rows[0], rows[1]
    for front in (KaldiWaveFeature(num_mel_bins=80), LhotseKaldiFeatFbank(snip_edges=True)):
        ref, frames = front.forward_batch(pcm.to(dev), torch.tensor([7000, 4100]))
        sf = front.streaming(2, 1600, device=dev)
        assert sf.feats.shape == (2, 11, 80)
        with pytest.raises(ValueError, match="max_chunk_samples"):
            sf.accept(torch.zeros(2, 1601))
        with pytest.raises(ValueError, match="shape"):
            sf.accept(torch.zeros(3, 100))
        got, fed, ended = [[], []], [0, 0], [False, False]
        for k in range(5):
            ns = [min(1600, 7000 - fed[0]), min(1600, max(4100 - fed[1], 0))]
            last = [fed[0] + ns[0] == 7000, not ended[1] and fed[1] + ns[1] == 4100]
            feats, _ = sf.accept(pcm[:, 1600 * k:1600 * k + 1600].to(dev), ns, last)
            for b in range(2):
                before = sf.frames_after(fed[b], ended[b])
                fed[b], ended[b] = fed[b] + ns[b], ended[b] or last[b]
                got[b].append(feats[b, :sf.frames_after(fed[b], ended[b]) - before].clone())
        for b in range(2):
            assert torch.equal(torch.cat(got[b]), ref[b, :int(frames[b])])
        sf.reset([1])
        feats, new = sf.accept(pcm[:, :1600].to(dev), [0, 1600], [False, False])
        assert new.tolist() == [0, 8] and torch.equal(feats[1, :8], ref[1, :8])
