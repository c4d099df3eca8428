"""Feature-pipeline factory (reference dataset/frontend/frontend.py:146-152).

Same `FeatType[feat_type].value(**feat_config)` surface, same per-utterance call
`forward(pcm[1,N]) -> feat[n,D]`; the arithmetic runs in the HIP fbank kernel.  Addition:
`forward_batch(pcm[B,Nmax], num_samples[B])` computes a whole padded batch in one launch
(optionally with the global CMVN fused), so features never leave HBM.
"""
from enum import Enum, unique

import torch
import torch.nn as nn

from speech2text_amd import kernels as K


class StreamingFbank:
    """The fbank of B audio streams, a cut at a time (kernels.fbank_chunk: the frames a row emits
    over its calls are `forward_batch`'s on the whole audio, bit for bit, however it was cut).

    Fixed buffers, so that `launch` can sit in a captured region: `pcm` (B, max_chunk_samples),
    `chunk_samples` (B) int64, `flush` (B) int32, the stream state, and the outputs `feats` (B,
    max_new_frames, M), `new_frames` (B).  `accept` is a copy-in plus `launch` and returns the two
    output buffers: consume or clone them before the next call.  Frames leave in pairs (a frame
    waits at most one hop, 10 ms, for its partner); `last` flushes a row's lone final frame and
    ends the row until its reset.  `frames_after` is the counting rule in plain integers: a caller
    that tracks its own sample counts never reads `new_frames` back."""

    def __init__(self, frontend, batch_size, max_chunk_samples, device=None, cmvn_mean=None,
                 cmvn_istd=None):
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if max_chunk_samples < 1:
            raise ValueError(f"max_chunk_samples must be >= 1, got {max_chunk_samples}")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("StreamingFbank runs on the HIP fbank kernel: device must be cuda")
        self.batch_size, self.max_chunk_samples = batch_size, max_chunk_samples
        self.max_new_frames = K.fbank_chunk_max_frames(max_chunk_samples)
        self._tables, self._scale_in = frontend.tables(device), frontend._scale_in
        self._cmvn = (cmvn_mean, cmvn_istd)
        self.state = K.FbankStreamState(batch_size, device)
        self.pcm = torch.zeros((batch_size, max_chunk_samples), dtype=torch.float32, device=device)
        self.chunk_samples = torch.zeros((batch_size,), dtype=torch.int64, device=device)
        self.flush = torch.zeros((batch_size,), dtype=torch.int32, device=device)
        self.feats = torch.zeros((batch_size, self.max_new_frames, self._tables.num_mel),
                                 dtype=torch.float32, device=device)
        self.new_frames = torch.zeros((batch_size,), dtype=torch.int64, device=device)

    frames_after = staticmethod(K.fbank_frames_after)

    def reset(self, rows=None):
        """Rows (indices, or None for all) start a new stream."""
        self.state.reset(rows)

    @torch.no_grad()
    def launch(self):
        """The chunk call on the fixed buffers as they stand."""
        return K.fbank_chunk(self.pcm, self.chunk_samples, self.flush, self.state, self._tables,
                             self._cmvn[0], self._cmvn[1], self._scale_in, out=self.feats,
                             new_frames=self.new_frames)

    @torch.no_grad()
    def accept(self, pcm, num_samples=None, last=None):
        """pcm (B, n), n <= max_chunk_samples: the new samples; num_samples (B) how many of them
        are row b's (None: n); last (B) true where the row ends with this call (None: nowhere).
        -> (feats, new_frames), the fixed output buffers."""
        if pcm.dim() != 2 or pcm.shape[0] != self.batch_size:
            raise ValueError(f"expected pcm of shape ({self.batch_size}, n), got {tuple(pcm.shape)}")
        n = pcm.shape[1]
        if n > self.max_chunk_samples:
            raise ValueError(f"a call takes at most max_chunk_samples = {self.max_chunk_samples} "
                             f"samples per row, got {n}")
        for name, v in (("num_samples", num_samples), ("last", last)):
            if v is not None and len(v) != self.batch_size:
                raise ValueError(f"{name} must have {self.batch_size} entries, got {len(v)}")
        if num_samples is not None and not torch.is_tensor(num_samples) and \
                any(int(v) < 0 or int(v) > n for v in num_samples):
            raise ValueError(f"num_samples must lie in 0..{n}, got {list(num_samples)}")
        if n:
            self.pcm[:, :n].copy_(pcm)
        if num_samples is None:
            self.chunk_samples.fill_(n)
        else:
            self.chunk_samples.copy_(torch.as_tensor(num_samples, dtype=torch.int64).clamp(0, n))
        if last is None:
            self.flush.zero_()
        else:
            self.flush.copy_(torch.as_tensor(last).to(torch.int32))
        return self.launch()


class _HipFbank(nn.Module):
    def __init__(self, num_mel_bins, high_freq=0.0, low_freq=20.0, samplerate=16000,
                 scale_in=1.0):
        super().__init__()
        self._num_mel_bins = num_mel_bins
        self._high_freq, self._low_freq, self._samplerate = high_freq, low_freq, samplerate
        self._scale_in = scale_in
        self._tables = {}

    @property
    def pcm_normalize(self):
        return True

    @property
    def feat_dim(self):
        return self._num_mel_bins

    def tables(self, device):
        key = str(device)
        if key not in self._tables:
            self._tables[key] = K.FbankTables(self._num_mel_bins, float(self._samplerate),
                                              self._low_freq, self._high_freq, device=device)
        return self._tables[key]

    @torch.no_grad()
    def forward_batch(self, pcm, num_samples, cmvn_mean=None, cmvn_istd=None):
        dev = pcm.device if pcm.is_cuda else torch.device("cuda", torch.cuda.current_device())
        pcm = pcm.to(device=dev, dtype=torch.float32).contiguous()
        num_samples = num_samples.to(device=dev, dtype=torch.int64).contiguous()
        return K.fbank_batch(pcm, num_samples, self.tables(dev), cmvn_mean, cmvn_istd,
                             self._scale_in)

    def streaming(self, batch_size, max_chunk_samples, device=None, cmvn_mean=None, cmvn_istd=None):
        """A StreamingFbank of this frontend (its tables and sample scale): audio in arbitrary
        cuts of at most max_chunk_samples samples, the frames `forward_batch` gives the whole."""
        return StreamingFbank(self, batch_size, max_chunk_samples, device, cmvn_mean, cmvn_istd)

    @torch.no_grad()
    def forward(self, pcm: torch.Tensor) -> torch.Tensor:
        assert pcm.dim() == 2 and pcm.shape[0] == 1, "expects (1, num_samples)"
        n = torch.tensor([pcm.shape[1]], dtype=torch.int64)
        feats, _ = self.forward_batch(pcm, n)
        return feats[0]


class KaldiWaveFeature(_HipFbank):
    """`fbank`: torchaudio.compliance.kaldi.fbank semantics (reference :57-94)."""

    def __init__(self, num_mel_bins=64, frame_length=25, frame_shift=10, dither=0.0,
                 samplerate=16000) -> None:
        if frame_length != 25 or frame_shift != 10 or samplerate != 16000:
            raise NotImplementedError("the HIP fbank kernel is built for 25 ms / 10 ms @ 16 kHz "
                                      "(every shipped YAML)")
        if dither != 0.0:
            raise NotImplementedError("dither != 0 is not used by any shipped YAML")
        super().__init__(num_mel_bins, high_freq=0.0, samplerate=samplerate)
        self._frame_length, self._frame_shift, self._dither = frame_length, frame_shift, dither


class LhotseKaldiFeatFbank(_HipFbank):
    """`lhotes_fbank`: lhotse KaldifeatFbank (kaldifeat defaults: 80 bins whatever
    num_mel_bins says -- the reference only stores that argument, :104 --, high_freq=-400,
    dither 0, and 16-bit-scaled samples).  PARITY UNPINNED (lhotse/kaldifeat absent)."""

    def __init__(self, num_mel_bins=80, snip_edges=False) -> None:
        if not snip_edges:
            raise NotImplementedError("snip_edges=False framing is not on the accelerated path "
                                      "(the zipformer YAML sets snip_edges: true)")
        super().__init__(80, high_freq=-400.0, scale_in=32768.0)
        self._declared_mel_bins = num_mel_bins

    @property
    def feat_dim(self):
        return self._declared_mel_bins


class DummyFrontend(nn.Module):
    def __init__(self, dummy=-1) -> None:
        super().__init__()

    @property
    def pcm_normalize(self):
        return True

    @property
    def feat_dim(self):
        return -1

    @torch.no_grad()
    def forward(self, pcm: torch.Tensor) -> torch.Tensor:
        return pcm.squeeze(0)


class TorchScriptKaldiWaveFeature(nn.Module):
    def __init__(self, torchscript: str, num_mel_bins=80) -> None:
        super().__init__()
        self._frontend_sess = torch.jit.load(torchscript)
        self._num_mel_bins = num_mel_bins

    @property
    def pcm_normalize(self):
        return True

    @property
    def feat_dim(self):
        return self._num_mel_bins

    @torch.no_grad()
    def forward(self, pcm: torch.Tensor) -> torch.Tensor:
        return self._frontend_sess(pcm)


@unique
class FeatType(Enum):
    pcm = DummyFrontend
    fbank = KaldiWaveFeature
    lhotes_fbank = LhotseKaldiFeatFbank
    torchscript_fbank = TorchScriptKaldiWaveFeature
