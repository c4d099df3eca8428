"""Audio in, text out: the streaming recognisers of zipformer_streaming.py behind the chunk-carried
fbank (dataset/frontend/frontend.py StreamingFbank, csrc/fbank_stream.hip).

The fbank call is its own launch ahead of the recogniser's replay: cuts of varying size rule out one
fixed capture.  Nothing here reads device memory back: how many frames a call emitted
follows from the sample counts the host already has (`StreamingFbank.frames_after`)."""
import math
from typing import List

import torch

from speech2text_amd import kernels as K


class AudioStreamPlan:
    """The host's integers of an AudioStreamingRecognizer: per row the samples fed, whether it has
    ended, the frames its FIFO holds and the windows it has been stepped through.  Pure Python: it
    states the lockstep rule and raises where a call breaks it.

    Lockstep: the recogniser's captured graph advances the encoder state of EVERY row, so one `accept`
    gives every row that has not ended the same n samples; a row given fewer must be marked `last`, and
    an ended row must be given 0 until its reset."""

    def __init__(self, batch_size: int, chunk: int, max_chunk_samples: int):
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if chunk < 2 or chunk % 2:
            raise ValueError(f"chunk must be even and > 0, got {chunk}")
        if max_chunk_samples < 1:
            raise ValueError(f"max_chunk_samples must be >= 1, got {max_chunk_samples}")
        self.batch_size, self.chunk, self.Tc = batch_size, chunk, chunk // 2
        self.window, self.stride = 2 * chunk + 13, 2 * chunk
        self.max_chunk_samples = max_chunk_samples
        self.samples = [0] * batch_size     # fed since the row's reset
        self.ended = [False] * batch_size
        self.held = [0] * batch_size        # frames in the row's FIFO
        self.steps = [0] * batch_size       # windows the row has been stepped through

    def reset(self, rows=None):
        for b in range(self.batch_size) if rows is None else rows:
            self.samples[b], self.ended[b], self.held[b], self.steps[b] = 0, False, 0, 0

    def frames(self, b: int) -> int:
        return K.fbank_frames_after(self.samples[b], self.ended[b])

    def accept(self, n: int, num_samples=None, last=None):
        """One call of n samples per row -> (the samples each row takes, its `last` flag, the frames
        its fbank emits in the call), three lists."""
        B = self.batch_size
        if n < 0 or n > self.max_chunk_samples:
            raise ValueError(f"a call takes 0..{self.max_chunk_samples} samples per row, got {n}")
        ns = [n if not self.ended[b] else 0 for b in range(B)] if num_samples is None \
            else [int(v) for v in num_samples]
        la = [False] * B if last is None else [bool(v) for v in last]
        if len(ns) != B or len(la) != B:
            raise ValueError(f"num_samples and last must have {B} entries")
        for b in range(B):
            if self.ended[b]:
                if ns[b] != 0 or la[b]:
                    raise ValueError(f"row {b} has ended: it takes 0 samples and no `last` until its reset "
                                     "(lockstep: the captured graph advances the encoder state of every row)")
            elif ns[b] < 0 or ns[b] > n:
                raise ValueError(f"row {b}: num_samples must lie in 0..{n}, got {ns[b]}")
            elif ns[b] != n and not la[b]:
                raise ValueError(f"row {b} is given {ns[b]} of the call's {n} samples without being marked "
                                 "`last`: every row that has not ended receives the same samples per call "
                                 "(lockstep: the captured graph advances the encoder state of every row)")
        new = []
        for b in range(B):
            before = self.frames(b)
            self.samples[b] += ns[b]
            self.ended[b] = self.ended[b] or la[b]
            new.append(self.frames(b) - before)
            self.held[b] += new[b]
        return ns, la, new

    def out_frames(self, b: int) -> int:
        """Encoder frames of an ended row (StreamingRecognizer.num_output_frames, in integers)."""
        return max(((self.frames(b) - 7) // 2 + 1) // 2, 0)

    def ready(self, finishing: bool = False) -> bool:
        """Whether a step can run: every live row holds its next window; with no live row (and
        `finishing`), while an ended row has encoder frames left -- or none has been stepped at all:
        `recognize` runs one step even on nothing."""
        live = [b for b in range(self.batch_size) if not self.ended[b]]
        if live:
            return all(self.held[b] >= self.window for b in live)
        return finishing and any(self.steps[b] * self.Tc < max(self.out_frames(b), 1)
                                 for b in range(self.batch_size))

    def chunk_len(self) -> List[int]:
        """Valid encoder frames of the next step per row: chunk//2 for a live row (one that holds
        2*chunk*(k+1)+13 frames has at least (k+1)*chunk//2 + 2 encoder frames), what is left of
        an ended one's."""
        return [min(max(self.out_frames(b) - self.steps[b] * self.Tc, 0), self.Tc) if self.ended[b]
                else self.Tc for b in range(self.batch_size)]

    def advance(self):
        for b in range(self.batch_size):
            self.held[b] = max(self.held[b] - self.stride, 0)
            self.steps[b] += 1


class AudioStreamingRecognizer:
    """Audio in, text out, in arbitrary cuts: a StreamingFbank (no fused CMVN: the recogniser applies
    its own), a per-row device FIFO of feature frames, and an existing StreamingRecognizer or
    CtcStreamingRecognizer, which does not change.

    `accept(pcm, num_samples, last)` appends the frames the cut completes and, while every row that
    has not ended holds the 2*chunk+13 frames of its next window, runs `recognizer.step(window,
    chunk_len)` and advances every row by 2*chunk frames; `finish(rows)` flushes rows and, once no row
    is live, runs the windows that remain.  An ended row is padded the way `recognize` pads (log(1e-10)
    after the CMVN) and gets chunk_len = clamp(n_out - k * chunk//2, 0, chunk//2).

    Lockstep: in one `accept` every row that has not ended receives the same n samples; a row given
    fewer must be marked `last`, an ended row must be given 0 until its reset; anything else is a
    ValueError.  The reason: the captured graph advances the encoder state of every row, so a row
    cannot sit a step out.

    The invariant: after `finish()`, tokens, out_len, scores and texts equal
    `recognizer.recognize(feats, frames)` with feats, frames = kernels.fbank_batch on the whole audio,
    bit for bit, however the audio was cut.  Nothing on this path reads device memory back: the frame
    counts are `StreamingFbank.frames_after` of the sample counts."""

    def __init__(self, recognizer, frontend, max_chunk_samples: int = 5120):
        from speech2text_amd.dataset.frontend.frontend import _HipFbank
        from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer
        if not isinstance(recognizer, StreamingRecognizer):
            raise ValueError("AudioStreamingRecognizer wraps a StreamingRecognizer or CtcStreamingRecognizer, "
                             f"got {type(recognizer).__name__}")
        if not isinstance(frontend, _HipFbank):
            raise ValueError("AudioStreamingRecognizer needs a frontend on the HIP fbank kernel (fbank / "
                             f"lhotes_fbank), got {type(frontend).__name__}")
        self.plan = AudioStreamPlan(recognizer.batch_size, recognizer.chunk, max_chunk_samples)
        self.recognizer = recognizer
        dev = recognizer.x.device
        F = recognizer.x.shape[2]
        if frontend._num_mel_bins != F:
            raise ValueError(f"the frontend gives {frontend._num_mel_bins} mel bins, the recogniser takes {F}")
        self.fbank = frontend.streaming(recognizer.batch_size, max_chunk_samples, device=dev)
        pad = torch.full((F,), math.log(1e-10), device=dev)          # as `recognize` pads
        if recognizer._cmvn is not None:
            pad = pad / recognizer._cmvn[1] + recognizer._cmvn[0]
        self._pad = pad
        # every row's frames from its next window's first onwards, then the padding: a row reset late
        # makes the others wait for its first window, hence room for two windows and two calls
        self.capacity = 2 * (self.plan.window + self.fbank.max_new_frames)
        self.fifo = pad.expand(recognizer.batch_size, self.capacity, F).clone()

    def reset(self, rows=None):
        """Rows (indices, or None for all) start a new utterance: recogniser, fbank state and FIFO."""
        rows = None if rows is None else [int(r) for r in rows]
        self.recognizer.reset(rows)
        self.fbank.reset(rows)
        self.plan.reset(rows)
        if rows is None:
            self.fifo.copy_(self._pad.expand_as(self.fifo))
        else:
            for b in rows:
                self.fifo[b].copy_(self._pad.expand_as(self.fifo[b]))

    def _run(self, finishing: bool) -> int:
        p, steps = self.plan, 0
        while p.ready(finishing):
            self.recognizer.step(self.fifo[:, :p.window], p.chunk_len())
            rest = self.fifo[:, p.stride:].clone()
            self.fifo[:, :self.capacity - p.stride].copy_(rest)
            self.fifo[:, self.capacity - p.stride:].copy_(self._pad)
            p.advance()
            steps += 1
        return steps

    @torch.no_grad()
    def accept(self, pcm, num_samples=None, last=None) -> int:
        """pcm (B, n) the new samples, num_samples (B) host integers (None: n for every row that has
        not ended), last (B) true where the row ends with this call.  -> the steps it ran."""
        if pcm.dim() != 2 or pcm.shape[0] != self.plan.batch_size:
            raise ValueError(f"expected pcm of shape ({self.plan.batch_size}, n), got {tuple(pcm.shape)}")
        p = self.plan
        held = list(p.held)
        ns, last, new = p.accept(pcm.shape[1], num_samples, last)
        if any(held[b] + new[b] > self.capacity for b in range(p.batch_size)):
            raise RuntimeError("the frame FIFO is full: a row has waited for another's first window for "
                               "more than two windows")
        feats, _ = self.fbank.accept(pcm, ns, last)
        for b in range(p.batch_size):
            if new[b]:
                self.fifo[b, held[b]:held[b] + new[b]].copy_(feats[b, :new[b]])
        return self._run(False)

    @torch.no_grad()
    def finish(self, rows=None) -> int:
        """Flushes rows (indices, None: every row that has not ended) and runs the windows that
        remain once no row is live (until then ended rows step along with the live ones).  -> steps."""
        p = self.plan
        rows = [b for b in range(p.batch_size) if not p.ended[b]] if rows is None \
            else [int(b) for b in rows if not p.ended[int(b)]]
        steps = 0
        if rows:
            last = [b in rows for b in range(p.batch_size)]
            empty = torch.zeros((p.batch_size, 0), dtype=torch.float32, device=self.fifo.device)
            steps = self.accept(empty, [0] * p.batch_size, last)
        return steps + self._run(True)

    def texts(self) -> List[str]:
        return self.recognizer.texts()

    def stable_texts(self) -> List[str]:
        return self.recognizer.stable_texts()
