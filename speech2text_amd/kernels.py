"""torch.autograd wrappers around the C ABI of libs2t_mi355.so.

Everything here runs on the HIP stream torch considers current; torch is used for
device memory and autograd plumbing only.  There is no CPU path: CPU tensors raise.
"""
import collections
import math

import numpy as np
import torch

from . import _native as N

_NEG_INF = float("-inf")
CTC_MAX_LABELS = N.const("S2T_CTC_MAX_LABELS")
RNNT_MAX_ROWS = 1024      # S+1 lattice rows: one thread each in one workgroup (csrc/rnnt.hip mi_*_kernel)
RNNT_MAX_JOINER_DIM = 1024  # fused pruned joiner: 16 classes per lane of one wave (csrc/rnnt.hip)


def _dev_check(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("speech2text_amd kernels run on the GPU only (no CPU fallback)")


# =============================================================== fbank
class FbankTables:
    """Host-built constant tables of the kaldi fbank (window, FFT twiddles, mel banks).

    Formulas follow dataset/frontend/frontend.py:85-94 -> kaldi.fbank as stated by
    sample_data/model/frontend.script (povey window, mel scale 1127 ln(1+f/700),
    low 20 Hz, high = nyquist + high_freq if high_freq <= 0)."""

    def __init__(self, num_mel_bins=80, sample_frequency=16000.0, low_freq=20.0, high_freq=0.0,
                 device="cuda"):
        nfft = 512
        win = torch.hann_window(400, periodic=False, dtype=torch.float32).pow(0.85)
        m = np.arange(nfft, dtype=np.float64)
        tw = np.stack([np.cos(2 * math.pi * m / nfft), -np.sin(2 * math.pi * m / nfft)], 1)
        nyq = 0.5 * sample_frequency
        hf = high_freq + nyq if high_freq <= 0.0 else high_freq
        mel_lo = 1127.0 * math.log(1.0 + low_freq / 700.0)
        mel_hi = 1127.0 * math.log(1.0 + hf / 700.0)
        delta = (mel_hi - mel_lo) / (num_mel_bins + 1)
        b = torch.arange(num_mel_bins, dtype=torch.float32).unsqueeze(1)
        left = b * delta + mel_lo
        center = (b + 1.0) * delta + mel_lo
        right = (b + 2.0) * delta + mel_lo
        freq = torch.arange(nfft // 2, dtype=torch.float32) * (sample_frequency / nfft)
        mel = ((freq / 700.0 + 1.0).log() * 1127.0).unsqueeze(0)
        up = (mel - left) / (center - left)
        down = (right - mel) / (right - center)
        w = torch.clamp(torch.min(up, down), min=0.0).numpy()          # (M, 256)
        off, k0, vals = [0], [], []
        for r in range(num_mel_bins):
            nz = np.nonzero(w[r])[0]
            if nz.size == 0:
                k0.append(0)
            else:
                k0.append(int(nz[0]))
                vals.extend(w[r, nz[0]:nz[-1] + 1].tolist())
            off.append(len(vals))
        self.num_mel = num_mel_bins
        self.nnz = len(vals)
        self.dense = w
        self.window = win.to(device)
        self.twiddle = torch.from_numpy(tw.astype(np.float32)).contiguous().to(device)
        self.mel_off = torch.tensor(off, dtype=torch.int32, device=device)
        self.mel_k0 = torch.tensor(k0, dtype=torch.int32, device=device)
        self.mel_w = torch.tensor(vals if vals else [0.0], dtype=torch.float32, device=device)


def fbank_batch(pcm, num_samples, tables, cmvn_mean=None, cmvn_istd=None, scale_in=1.0,
                max_frames=None):
    """pcm (B,Nmax) f32 device, num_samples (B,) i64 device -> feats (B,n_max,M), n_frames (B,)."""
    _dev_check(pcm, num_samples)
    B, nmax = pcm.shape
    if max_frames is None:
        max_frames = 0 if nmax < 400 else 1 + (nmax - 400) // 160
    out = torch.empty((B, max_frames, tables.num_mel), dtype=torch.float32, device=pcm.device)
    frames = torch.empty((B,), dtype=torch.int64, device=pcm.device)
    if B == 0 or max_frames == 0:
        return out, frames.zero_()
    N.PROF[0] and N.profile_note("s2t_fbank_f32", 4.0 * (pcm.numel() + out.numel()))
    rc = N.lib().s2t_fbank_f32(N.fp(pcm), pcm.stride(0), N.lp(num_samples), B,
                               N.fp(tables.window), N.fp(tables.twiddle), N.ip(tables.mel_off),
                               N.ip(tables.mel_k0), N.fp(tables.mel_w), tables.nnz,
                               tables.num_mel, 1.1920928955078125e-07, float(scale_in),
                               N.fp(cmvn_mean), N.fp(cmvn_istd), N.fp(out), max_frames,
                               N.lp(frames), N.stream())
    N.check(rc, "s2t_fbank_f32")
    return out, frames


FBANK_CARRY_MAX = N.const("S2T_FBANK_CARRY_MAX")


def fbank_frames(num_samples):
    """Frames the one-shot fbank gives num_samples samples (snip_edges, 400 at hop 160)."""
    return 1 + (num_samples - 400) // 160 if num_samples >= 400 else 0


def fbank_chunk_max_frames(chunk_samples):
    """The most frames one fbank_chunk call of chunk_samples new samples can emit: the pairs the
    samples can complete, and the flush's lone frame (s2t_fbank_chunk_max_frames, in integers)."""
    return 2 * ((chunk_samples - 1) // 320 + 1) + 1 if chunk_samples >= 1 else 1


def fbank_frames_after(total_samples, ended):
    """Frames a stream of total_samples samples has emitted: every complete PAIR (pair p leaves once
    total_samples >= 320 p + 560); after the flush (`ended`) the one-shot count."""
    if total_samples < 0:
        raise ValueError(f"total_samples must be >= 0, got {total_samples}")
    if ended:
        return fbank_frames(total_samples)
    return 2 * ((total_samples - 560) // 320 + 1) if total_samples >= 560 else 0


class FbankStreamState:
    """The caller-owned state of fbank_chunk (include/s2t_mi355.h s2t_fbank_chunk_f32): `carry`
    (B, 559) the raw samples of the first un-emitted frame pair onwards, `counts` (B, 4) int64 the
    samples seen, the frames emitted and the ended flag.  A row whose counts are zero is a new stream."""

    def __init__(self, batch_size, device):
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        self.batch_size = batch_size
        self.carry = torch.zeros((batch_size, FBANK_CARRY_MAX), dtype=torch.float32, device=device)
        self.counts = torch.zeros((batch_size, N.const("S2T_FBANK_STATE_LONGS")), dtype=torch.int64,
                                  device=device)

    def reset(self, rows=None):
        """Rows (indices, or None for all) start a new stream."""
        if rows is None:
            self.counts.zero_()
        else:
            self.counts.index_fill_(0, torch.as_tensor(rows, dtype=torch.int64).to(self.counts.device), 0)


def fbank_chunk(pcm, chunk_samples, flush, state, tables, cmvn_mean=None, cmvn_istd=None, scale_in=1.0,
                max_new_frames=None, out=None, new_frames=None):
    """The fbank carried across chunks: pcm (B, n) f32 the NEW samples, chunk_samples (B,) i64 how
    many per row, flush (B,) i32 (!= 0 ends the row), state a FbankStreamState -> feats (B,
    max_new_frames, M), new_frames (B,).  The frames a row emits over its calls are fbank_batch's on
    the whole audio, bit for bit, however it was cut; they leave in pairs, the flush adds the lone
    last frame.  `out` / `new_frames`: fixed buffers to write instead of fresh ones."""
    _dev_check(pcm, chunk_samples, flush)
    B, n = pcm.shape
    if B != state.batch_size:
        raise ValueError(f"pcm has {B} rows, the state {state.batch_size}")
    if max_new_frames is None:
        max_new_frames = fbank_chunk_max_frames(n) if out is None else out.shape[1]
    if max_new_frames < fbank_chunk_max_frames(n):
        raise ValueError(f"a call of {n} samples can emit {fbank_chunk_max_frames(n)} frames: "
                         f"max_new_frames = {max_new_frames} is too small")
    if out is None:
        out = torch.empty((B, max_new_frames, tables.num_mel), dtype=torch.float32, device=pcm.device)
    elif tuple(out.shape) != (B, max_new_frames, tables.num_mel):
        raise ValueError(f"out must be {(B, max_new_frames, tables.num_mel)}, got {tuple(out.shape)}")
    if new_frames is None:
        new_frames = torch.empty((B,), dtype=torch.int64, device=pcm.device)
    if n == 0:                       # (a zero-width tensor has no row stride to speak of)
        pcm = pcm.new_zeros((B, 1))
    N.PROF[0] and N.profile_note("s2t_fbank_chunk_f32", 4.0 * (pcm.numel() + out.numel()))
    rc = N.lib().s2t_fbank_chunk_f32(N.fp(pcm), n, N.lp(chunk_samples), N.ip(flush), B,
                                     N.fp(state.carry), N.lp(state.counts), N.fp(tables.window),
                                     N.fp(tables.twiddle), N.ip(tables.mel_off), N.ip(tables.mel_k0),
                                     N.fp(tables.mel_w), tables.nnz, tables.num_mel,
                                     1.1920928955078125e-07, float(scale_in), N.fp(cmvn_mean),
                                     N.fp(cmvn_istd), N.fp(out), max_new_frames, N.lp(new_frames),
                                     N.stream())
    N.check(rc, "s2t_fbank_chunk_f32")
    return out, new_frames


# =============================================================== CTC
class _CtcLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, in_len, tgt_len, blank, reduction, zero_infinity):
        _dev_check(logits)
        logits = logits.contiguous().float()
        B, T, V = logits.shape
        dev = logits.device
        targets = targets.to(device=dev, dtype=torch.int64).contiguous()
        in_len = in_len.to(device=dev, dtype=torch.int64).contiguous()
        tgt_len = tgt_len.to(device=dev, dtype=torch.int64).contiguous()
        U = targets.shape[1] if targets.dim() == 2 else 0
        if U == 0:
            targets = torch.zeros((B, 1), dtype=torch.int64, device=dev)
        tl = tgt_len.clamp(min=1).float()
        if reduction == "mean":
            scale = 1.0 / (tl * B)
        else:
            scale = torch.ones(B, device=dev)
        scale = scale.contiguous()
        if U > CTC_MAX_LABELS:
            raise ValueError(f"CTC: padded label width {U} exceeds the kernel's limit of "
                             f"{CTC_MAX_LABELS} labels per utterance (2U+1 lattice states are "
                             "held in one workgroup's LDS, csrc/ctc.hip)")
        ws = torch.empty(N.lib().s2t_ctc_workspace_floats(B, T, U), dtype=torch.float32,
                         device=dev)
        per = torch.empty(B, dtype=torch.float32, device=dev)
        grad = torch.empty_like(logits)
        # 2 B T V 4 (logits in, gradient out) + 3 B T (2U+1) 4 (lattice rows)
        N.PROF[0] and N.profile_note("s2t_ctc_loss_fwd_bwd", 8.0 * B * T * V + 12.0 * B * T * (2 * U + 1))
        rc = N.lib().s2t_ctc_loss_fwd_bwd(N.fp(logits), N.lp(targets), targets.stride(0),
                                          N.lp(in_len), N.lp(tgt_len), B, T, V, U, int(blank),
                                          int(bool(zero_infinity)), N.fp(scale), N.fp(ws),
                                          N.fp(per), N.fp(grad), N.stream())
        N.check(rc, "s2t_ctc_loss_fwd_bwd")
        ctx.save_for_backward(grad)
        ctx.reduction = reduction
        if reduction == "mean":
            return (per / tl).mean()
        if reduction == "sum":
            return per.sum()
        return per

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        if ctx.reduction == "none":
            return grad * g.reshape(-1, 1, 1), None, None, None, None, None, None
        return grad * g, None, None, None, None, None, None


def ctc_loss(logits, targets, logits_length, targets_length, blank=0, reduction="mean",
             zero_infinity=True):
    """Fused log_softmax + CTC on batch-major logits (B,T,V)."""
    return _CtcLoss.apply(logits, targets, logits_length, targets_length, blank, reduction,
                          zero_infinity)


CtcAlignment = collections.namedtuple(
    "CtcAlignment", ["path", "tok_begin", "tok_end", "tok_logp", "raw_score", "score", "ok"])
CTC_ALIGN_FORM_WORKSPACE = N.const("S2T_CTC_ALIGN_FORM_WORKSPACE")


def _align_check(t, dtype, what):
    if not t.is_cuda or t.dtype is not dtype or not t.is_contiguous():
        raise RuntimeError(f"ctc_align: {what} must be a contiguous {dtype} device tensor, got "
                           f"{t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")


def ctc_align(logits, lengths, targets, target_lengths, blank=0, out=None):
    """CTC forced alignment (csrc/ctc_align.hip; the statement is in include/s2t_mi355.h): logits (B,T,V)
    fp32, raw or log-probabilities, lengths (B) int64, targets (B,U) int64, target_lengths (B) int64,
    all contiguous on the device -> CtcAlignment(path (B,T) int32, tok_begin / tok_end (B,U) int32,
    tok_logp (B,U) fp32, raw_score / score (B) fp32, ok (B) int32).  `out`: an earlier result of the same
    shapes to write into again (no allocation besides the workspace)."""
    _align_check(logits, torch.float32, "logits")
    _align_check(lengths, torch.int64, "lengths")
    _align_check(targets, torch.int64, "targets")
    _align_check(target_lengths, torch.int64, "target_lengths")
    if logits.dim() != 3 or targets.dim() != 2 or targets.shape[0] != logits.shape[0] \
            or lengths.shape != (logits.shape[0],) or target_lengths.shape != (logits.shape[0],):
        raise ValueError(f"ctc_align: logits (B,T,V), lengths (B), targets (B,U), target_lengths (B) expected, got "
                         f"{tuple(logits.shape)}, {tuple(lengths.shape)}, {tuple(targets.shape)}, "
                         f"{tuple(target_lengths.shape)}")
    B, T, V = logits.shape
    U = targets.shape[1]
    dev = logits.device
    if U > CTC_MAX_LABELS:
        raise ValueError(f"CTC: padded label width {U} exceeds the kernel's limit of "
                         f"{CTC_MAX_LABELS} labels per utterance (2U+1 lattice states are "
                         "held in one workgroup's LDS, csrc/ctc_align.hip)")
    if not 0 <= int(blank) < V:
        raise ValueError(f"ctc_align: blank {blank} is outside the {V} classes")
    if out is None:
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)      # noqa: E731
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)    # noqa: E731
        out = CtcAlignment(i32(B, T), i32(B, U), i32(B, U), f32(B, U), f32(B), f32(B), i32(B))
    if B == 0 or T == 0:
        out.path.fill_(-1), out.tok_begin.fill_(-1), out.tok_end.fill_(-1), out.tok_logp.zero_()
        empty = target_lengths <= 0                        # no frames: only the empty transcript has a path
        out.ok.copy_(empty)
        out.raw_score.copy_(torch.where(empty, 0.0, _NEG_INF))
        out.score.copy_(out.raw_score)
        return out
    ws = torch.empty(N.lib().s2t_ctc_align_workspace_bytes(B, T, U), dtype=torch.uint8, device=dev)
    # an empty tensor has no address: the entry takes none of these as NULL, and writes nothing at U = 0
    tok = [t if U else ws for t in (out.tok_begin, out.tok_end, out.tok_logp)]
    N.PROF[0] and N.profile_note("s2t_ctc_align", 4.0 * B * T * V + 12.0 * B * T * (2 * U + 1) + 4.0 * B * T)
    rc = N.lib().s2t_ctc_align(N.fp(logits), N.lp(lengths), N.lp(targets) if U else N.ptr(ws),
                               targets.stride(0) if U else 0, N.lp(target_lengths), B, T, V, U, int(blank),
                               N.ptr(ws), N.ip(out.path),
                               tok[0].data_ptr(), tok[1].data_ptr(), tok[2].data_ptr(), N.fp(out.raw_score),
                               N.fp(out.score), N.ip(out.ok), N.stream())
    N.check(rc, "s2t_ctc_align")
    return out


# =============================================================== RNN-T lattice
def _i64(t, dev):
    return t.to(device=dev, dtype=torch.int64).contiguous()


def _check_lattice_rows(S):
    if S + 1 > RNNT_MAX_ROWS:
        raise ValueError(f"RNN-T lattice: {S} symbols + 1 rows exceed the kernel's limit of "
                         f"{RNNT_MAX_ROWS} lattice rows per utterance (one thread per row in one "
                         "workgroup, csrc/rnnt.hip)")


def mutual_information(px, py, boundary, want_grads=True):
    """Raw recursion: returns (scores (B,), p, px_grad, py_grad) -- no autograd.  As in k2 the
    topology follows from the shapes: px (B,S,T+1) is the regular lattice, px (B,S,T) -- as many
    columns as py -- the modified one, in which a symbol arc advances a frame too."""
    B, S, T1 = px.shape
    _check_lattice_rows(S)
    if py.shape != (B, S + 1, T1) and py.shape != (B, S + 1, T1 - 1):
        raise ValueError(f"mutual_information: px {tuple(px.shape)} and py {tuple(py.shape)} are "
                         "neither a regular (B,S,T+1)/(B,S+1,T) nor a modified (B,S,T)/(B,S+1,T) pair")
    T = py.shape[2]
    ty = RNNT_TYPES["modified" if T1 == T else "regular"]
    dev = px.device
    p = torch.empty((B, S + 1, T + 1), dtype=torch.float32, device=dev)
    ans = torch.empty((B,), dtype=torch.float32, device=dev)
    L = N.lib()
    N.PROF[0] and N.profile_note("s2t_mutual_info_fwd", 4.0 * (px.numel() + py.numel() + p.numel()))
    N.check(L.s2t_mutual_info_fwd(N.fp(px), N.fp(py), N.lp(boundary), B, S, T, ty, N.fp(p),
                                  N.fp(ans), N.stream()), "s2t_mutual_info_fwd")
    if not want_grads:
        return ans, p, None, None
    gx = torch.empty_like(px)
    gy = torch.empty_like(py)
    N.PROF[0] and N.profile_note("s2t_mutual_info_bwd", 4.0 * (2 * px.numel() + 2 * py.numel() + p.numel()))
    N.check(L.s2t_mutual_info_bwd(N.fp(px), N.fp(py), N.lp(boundary), N.fp(p), None, B, S, T, ty,
                                  N.fp(gx), N.fp(gy), N.stream()), "s2t_mutual_info_bwd")
    return ans, p, gx, gy


RNNT_SMOOTH_MAX_C = N.const("S2T_RNNT_SMOOTH_MAX_C")
_SMOOTH_LM_SLAB = N.const("S2T_RNNT_SMOOTH_LM_SLAB")
_SMOOTH_AM_SLAB = N.const("S2T_RNNT_SMOOTH_AM_SLAB")


def check_smoothing_scales(lm_only_scale, am_only_scale):
    """k2.rnnt_loss_smoothed's weights: the joint term keeps alpha = 1 - lm_only - am_only, which
    must stay positive (with alpha <= 0 the -inf columns of px turn into NaN)."""
    lam, mu = float(lm_only_scale), float(am_only_scale)
    if not (lam >= 0.0 and mu >= 0.0 and lam + mu < 1.0):
        raise ValueError(f"smoothed RNN-T loss: lm_only_scale={lm_only_scale} and am_only_scale="
                         f"{am_only_scale} must be >= 0 with a sum below 1")
    return lam, mu


class _SimpleRnntLoss(torch.autograd.Function):
    """k2.rnnt_loss_smoothed(lm, am, symbols, blank, lm_only_scale, am_only_scale, boundary,
    reduction='none', return_grad=True) -> (neg scores (B,), px_grad, py_grad).  With both scales
    0 the launches are those of the unsmoothed path; a non-zero scale adds csrc/rnnt_smooth.hip's
    row statistics and swaps the px/py pass and the two backward row kernels for their smoothed
    forms.  With am_only_scale != 0 the utterances of a batch are coupled through the batch's
    unigram u (the mean of softmax(lm) over all B (S+1) rows, padded ones included)."""

    @staticmethod
    def forward(ctx, lm, am, symbols, boundary, blank, lam, mu):
        _dev_check(lm, am)
        lm = lm.contiguous().float()
        am = am.contiguous().float()
        B, T, C = am.shape
        S = lm.shape[1] - 1
        _check_lattice_rows(S)
        smooth = lam != 0.0 or mu != 0.0
        if smooth and C > RNNT_SMOOTH_MAX_C:
            raise ValueError(f"smoothed RNN-T loss: joiner dimension {C} exceeds the kernel's "
                             f"limit of {RNNT_SMOOTH_MAX_C} (two rows per wave are held in LDS, "
                             "csrc/rnnt_smooth.hip); there is no fallback")
        dev = am.device
        L = N.lib()
        st = N.stream()
        am_p = torch.empty_like(am)
        lm_p = torch.empty_like(lm)
        am_max = torch.empty((B, T), dtype=torch.float32, device=dev)
        lm_max = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
        N.PROF[0] and N.profile_note("s2t_rnnt_row_exp", 8.0 * (am.numel() + lm.numel()) + 4.0 * B * (T + S + 1))
        N.check(L.s2t_rnnt_row_exp(N.fp(am), B * T, C, N.fp(am_p), N.fp(am_max), st), "row_exp")
        N.check(L.s2t_rnnt_row_exp(N.fp(lm), B * (S + 1), C, N.fp(lm_p), N.fp(lm_max), st),
                "row_exp")
        # the normaliser product exp(lm) exp(am)^T (reference model/joiner/joiner.py:100-108 ->
        # k2.rnnt_loss_smoothed) and its two gradients below: our batched kernel (csrc/gemm.hip), no
        # library launch on the loss path
        from . import zip_kernels as zk
        with zk.gemm_class(zk.CLS_F):
            nrm = zk.batched_matmul(0, lm_p, am_p)                       # (B,S+1,T)
        px = torch.empty((B, S, T + 1), dtype=torch.float32, device=dev)
        py = torch.empty((B, S + 1, T), dtype=torch.float32, device=dev)
        lm_sum = u = am_dot = None
        if not smooth:
            # (two gathered operands per lattice arc -- am / lm at the arc's symbol or at blank -- the normaliser once)
            N.PROF[0] and N.profile_note("s2t_rnnt_simple_pxpy", 4.0 * (3 * px.numel() + 3 * py.numel() + nrm.numel()))
            N.check(L.s2t_rnnt_simple_pxpy(N.fp(am), N.fp(lm), N.fp(am_max), N.fp(lm_max),
                                           N.fp(nrm), N.lp(symbols), N.lp(boundary), B, S, T, C,
                                           int(blank), N.fp(px), N.fp(py), st), "simple_pxpy")
        else:
            lm_sum = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
            u_part = log_u = None
            stats_bytes = 4.0 * (lm_p.numel() + lm_sum.numel())
            if mu != 0.0:
                parts = (B * (S + 1) + _SMOOTH_LM_SLAB - 1) // _SMOOTH_LM_SLAB
                u_part = torch.empty((parts, C), dtype=torch.float32, device=dev)
                u = torch.empty((C,), dtype=torch.float32, device=dev)
                log_u = torch.empty((C,), dtype=torch.float32, device=dev)
                am_dot = torch.empty((B, T), dtype=torch.float32, device=dev)
                # lm_probs once more for the column sums, the partials out and in, am_probs once
                stats_bytes += 4.0 * (lm_p.numel() + lm_sum.numel() + 2 * u_part.numel() + 3 * C
                                      + am_p.numel() + am_dot.numel())
            N.PROF[0] and N.profile_note("s2t_rnnt_smooth_stats", stats_bytes)
            N.check(L.s2t_rnnt_smooth_stats(N.fp(am_p), N.fp(lm_p), B, S, T, C, mu, N.fp(lm_sum),
                                            N.fp(u_part), N.fp(u), N.fp(log_u), N.fp(am_dot), st),
                    "smooth_stats")
            # simple_pxpy's traffic, the row scalars and (mu) log u at the arc's class on top
            N.PROF[0] and N.profile_note("s2t_rnnt_smooth_pxpy",
                                         4.0 * ((3 + (mu != 0.0)) * (px.numel() + py.numel()) + nrm.numel()
                                                + lm_sum.numel() + (B * T if mu != 0.0 else 0)))
            N.check(L.s2t_rnnt_smooth_pxpy(N.fp(am), N.fp(lm), N.fp(am_max), N.fp(lm_max),
                                           N.fp(nrm), N.fp(lm_sum), N.fp(am_dot), N.fp(log_u),
                                           N.lp(symbols), N.lp(boundary), B, S, T, C, int(blank),
                                           lam, mu, N.fp(px), N.fp(py), st), "smooth_pxpy")
        ans, _, gx, gy = mutual_information(px, py, boundary)
        extra = () if not smooth else (lm_sum,) if mu == 0.0 else (lm_sum, u, am_dot)
        ctx.save_for_backward(am_p, lm_p, nrm, gx, gy, symbols, *extra)
        ctx.blank = int(blank)
        ctx.lam, ctx.mu = lam, mu
        ctx.mark_non_differentiable(gx, gy)
        return -ans, gx, gy

    @staticmethod
    def backward(ctx, g_loss, _gx, _gy):
        am_p, lm_p, nrm, gx, gy, symbols = ctx.saved_tensors[:6]
        B, T, C = am_p.shape
        S = lm_p.shape[1] - 1
        L = N.lib()
        st = N.stream()
        gscale = (-g_loss).contiguous().float()       # d loss / d score = -g
        W = torch.empty_like(nrm)
        N.PROF[0] and N.profile_note("s2t_rnnt_simple_w", 4.0 * (gx.numel() + gy.numel() + 2 * nrm.numel()))
        N.check(L.s2t_rnnt_simple_w(N.fp(gx), N.fp(gy), N.fp(nrm), N.fp(gscale), B, S, T,
                                    N.fp(W), st), "simple_w")
        from . import zip_kernels as zk
        with zk.gemm_class(zk.CLS_D):
            G_am = zk.batched_matmul(2, W, lm_p, own_tn=True)     # W^T @ exp(lm): (B,T,C)
            G_lm = zk.batched_matmul(1, W, am_p)                  # W @ exp(am):   (B,S+1,C)
        d_am = torch.empty_like(am_p)
        d_lm = torch.empty_like(lm_p)
        if ctx.lam == 0.0 and ctx.mu == 0.0:
            N.PROF[0] and N.profile_note("s2t_rnnt_simple_bwd", 12.0 * (am_p.numel() + lm_p.numel())
                                         + 4.0 * (gx.numel() + gy.numel()))
            N.check(L.s2t_rnnt_simple_bwd(N.fp(am_p), N.fp(lm_p), N.fp(G_am), N.fp(G_lm), N.fp(gx),
                                          N.fp(gy), N.fp(gscale), N.lp(symbols), B, S, T, C,
                                          ctx.blank, N.fp(d_am), N.fp(d_lm), 0, st), "simple_bwd")
            return d_lm, d_am, None, None, None, None, None
        lm_sum = ctx.saved_tensors[6]
        u = am_dot = dlogu_part = v = None
        extra = 0
        if ctx.mu != 0.0:
            u, am_dot = ctx.saved_tensors[7:9]
            parts = (B * T + _SMOOTH_AM_SLAB - 1) // _SMOOTH_AM_SLAB
            dlogu_part = torch.empty((parts, C), dtype=torch.float32, device=am_p.device)
            v = torch.empty((C,), dtype=torch.float32, device=am_p.device)
            # the partials out and in, lm_probs once more for q.v, the gradients once more for colsum
            extra = 2 * dlogu_part.numel() + lm_p.numel() + gx.numel() + 3 * C + B * T
        N.PROF[0] and N.profile_note("s2t_rnnt_smooth_bwd", 12.0 * (am_p.numel() + lm_p.numel())
                                     + 4.0 * (gx.numel() + gy.numel() + lm_sum.numel() + extra))
        N.check(L.s2t_rnnt_smooth_bwd(N.fp(am_p), N.fp(lm_p), N.fp(G_am), N.fp(G_lm), N.fp(gx),
                                      N.fp(gy), N.fp(gscale), N.lp(symbols), N.fp(lm_sum),
                                      N.fp(am_dot), N.fp(u), B, S, T, C, ctx.blank, ctx.lam, ctx.mu,
                                      N.fp(dlogu_part), N.fp(v), N.fp(d_am), N.fp(d_lm), st),
                "smooth_bwd")
        return d_lm, d_am, None, None, None, None, None


def rnnt_simple_loss(lm, am, symbols, boundary, blank=0, lm_only_scale=0.0, am_only_scale=0.0):
    lam, mu = check_smoothing_scales(lm_only_scale, am_only_scale)
    return _SimpleRnntLoss.apply(lm, am, symbols, boundary, blank, lam, mu)


def rnnt_prune_ranges(px_grad, py_grad, boundary, s_range):
    B, S, T1 = px_grad.shape
    T = T1 - 1
    if s_range > S:
        s_range = S + 1
    ranges = torch.empty((B, T, s_range), dtype=torch.int64, device=px_grad.device)
    N.PROF[0] and N.profile_note("s2t_rnnt_prune_ranges", 4.0 * (px_grad.numel() + py_grad.numel()) + 8.0 * ranges.numel())
    N.check(N.lib().s2t_rnnt_prune_ranges(N.fp(px_grad), N.fp(py_grad), N.lp(boundary), B, S, T,
                                          int(s_range), N.lp(ranges), N.stream()),
            "s2t_rnnt_prune_ranges")
    return ranges


_ACT = {"relu": 0, "tanh": 1}
RNNT_TYPES = {"regular": N.const("S2T_RNNT_REGULAR"), "modified": N.const("S2T_RNNT_MODIFIED"),
              "constrained": N.const("S2T_RNNT_CONSTRAINED")}


def check_rnnt_type(rnnt_type, delay_penalty):
    """k2.rnnt_loss_pruned's rnnt_type and delay_penalty -> (type constant, penalty as float)."""
    if rnnt_type not in RNNT_TYPES:
        raise ValueError(f"rnnt_type {rnnt_type!r} is not one of 'regular', 'modified', 'constrained'")
    pen = float(delay_penalty)
    if not pen >= 0.0:
        raise ValueError(f"delay_penalty {delay_penalty} is negative: k2 silently ignores such a "
                         "value (it applies the penalty only when it is > 0); it must be >= 0")
    return RNNT_TYPES[rnnt_type], pen


def _lattice_buffers(B, S, T, R, ty, dev):
    """What either lattice builder writes: px (B,S,T+1) on the regular lattice and (B,S,T) on the
    two others, py (B,S+1,T), lse (B,T,R)."""
    TX = T + 1 if ty == RNNT_TYPES["regular"] else T
    return [torch.empty(shape, dtype=torch.float32, device=dev)
            for shape in ((B, S, TX), (B, S + 1, T), (B, T, R))]


class _PrunedJoinerLoss(torch.autograd.Function):
    """Fused Joiner tail + k2.rnnt_loss_pruned(reduction='none'): per-utterance neg score
    of the lattice logits[b,t,i,:] = act(am[b,t,:] + lm[b,ranges[b,t,0]+i,:])."""

    @staticmethod
    def forward(ctx, am, lm, ranges, symbols, boundary, blank, act, ty, pen):
        _dev_check(am, lm)
        am = am.contiguous().float()
        lm = lm.contiguous().float()
        B, T, C = am.shape
        S = lm.shape[1] - 1
        R = ranges.shape[2]
        _check_lattice_rows(S)
        if C > RNNT_MAX_JOINER_DIM:
            raise ValueError(f"fused pruned joiner: joiner dimension {C} exceeds the kernel's "
                             f"limit of {RNNT_MAX_JOINER_DIM} (a row is held in one wave's "
                             "registers, csrc/rnnt.hip); there is no fallback")
        px, py, lse = _lattice_buffers(B, S, T, R, ty, am.device)
        N.PROF[0] and N.profile_note("s2t_rnnt_pruned_fwd",
                                     4.0 * (am.numel() + lm.numel() + px.numel() + py.numel() + lse.numel())
                                     + 8.0 * ranges.numel())
        N.check(N.lib().s2t_rnnt_pruned_fwd(N.fp(am), N.fp(lm), N.lp(ranges), N.lp(symbols),
                                            N.lp(boundary), B, S, T, C, R, int(blank), _ACT[act], ty,
                                            pen, N.fp(px), N.fp(py), N.fp(lse), N.stream()),
                "pruned_fwd")
        ans, _, gx, gy = mutual_information(px, py, boundary)
        ctx.save_for_backward(am, lm, ranges, symbols, lse, gx, gy)
        ctx.blank, ctx.act, ctx.ty = int(blank), _ACT[act], ty
        return -ans

    @staticmethod
    def backward(ctx, g):
        am, lm, ranges, symbols, lse, gx, gy = ctx.saved_tensors
        B, T, C = am.shape
        S = lm.shape[1] - 1
        R = ranges.shape[2]
        gscale = (-g).contiguous().float()
        d_am = torch.empty_like(am)
        d_lm = torch.empty_like(lm)
        # the (B,T,R,C) pruned logits are recomputed, never stored: the algorithmic traffic is the
        # operands and their gradients; the recomputation costs 2 B T R C flops of VALU per pass
        N.PROF[0] and N.profile_note("s2t_rnnt_pruned_bwd",
                                     4.0 * (2 * am.numel() + 2 * lm.numel() + lse.numel() + gx.numel() + gy.numel())
                                     + 8.0 * ranges.numel(), 4.0 * B * T * R * C)
        N.check(N.lib().s2t_rnnt_pruned_bwd(N.fp(am), N.fp(lm), N.lp(ranges), N.lp(symbols),
                                            N.fp(lse), N.fp(gx), N.fp(gy), N.fp(gscale), B, S, T, C,
                                            R, ctx.blank, ctx.act, ctx.ty, N.fp(d_am), N.fp(d_lm), 0,
                                            N.stream()), "pruned_bwd")
        return d_am, d_lm, None, None, None, None, None, None, None


def _full_ranges(B, T, S, dev):
    """ranges of the full lattice: every frame's band is all S+1 rows."""
    return torch.arange(S + 1, dtype=torch.int64, device=dev).expand(B, T, S + 1).contiguous()


def rnnt_pruned_joiner_loss(am, lm, ranges, symbols, boundary, blank=0, activation="relu",
                            rnnt_type="regular", delay_penalty=0.0):
    """k2.rnnt_loss_pruned(reduction='none') on the fused joiner's lattice.  rnnt_type 'modified' /
    'constrained' emit at most one symbol per frame; delay_penalty >= 0 pushes symbols to earlier
    frames.  ranges None is the full lattice: every row in every frame."""
    ty, pen = check_rnnt_type(rnnt_type, delay_penalty)
    if ranges is None:
        ranges = _full_ranges(am.shape[0], am.shape[1], lm.shape[1] - 1, am.device)
    return _PrunedJoinerLoss.apply(am, lm, ranges, symbols, boundary, blank, activation, ty, pen)


class _LatticeLoss(torch.autograd.Function):
    """Materialised lattice: logits (B,T,R,V); ranges None => full lattice (R = S+1)."""

    @staticmethod
    def forward(ctx, logits, ranges, symbols, boundary, blank, ty, pen):
        _dev_check(logits)
        logits = logits.contiguous().float()
        B, T, R, V = logits.shape
        S = symbols.shape[1]
        _check_lattice_rows(S)
        px, py, lse = _lattice_buffers(B, S, T, R, ty, logits.device)
        N.PROF[0] and N.profile_note("s2t_rnnt_lattice_fwd",
                                     4.0 * (logits.numel() + px.numel() + py.numel() + lse.numel()))
        N.check(N.lib().s2t_rnnt_lattice_fwd(N.fp(logits), N.lp(ranges), N.lp(symbols),
                                             N.lp(boundary), B, S, T, V, R, int(blank), ty, pen,
                                             N.fp(px), N.fp(py), N.fp(lse), N.stream()),
                "lattice_fwd")
        ans, _, gx, gy = mutual_information(px, py, boundary)
        ctx.save_for_backward(logits, symbols, lse, gx, gy)
        ctx.ranges = ranges
        ctx.blank, ctx.ty = int(blank), ty
        return -ans

    @staticmethod
    def backward(ctx, g):
        logits, symbols, lse, gx, gy = ctx.saved_tensors
        B, T, R, V = logits.shape
        S = symbols.shape[1]
        gscale = (-g).contiguous().float()
        d = torch.empty_like(logits)
        N.PROF[0] and N.profile_note("s2t_rnnt_lattice_bwd",
                                     4.0 * (2 * logits.numel() + lse.numel() + gx.numel() + gy.numel()))
        N.check(N.lib().s2t_rnnt_lattice_bwd(N.fp(logits), N.lp(ctx.ranges), N.lp(symbols),
                                             N.fp(lse), N.fp(gx), N.fp(gy), N.fp(gscale), B, S, T, V,
                                             R, ctx.blank, ctx.ty, N.fp(d), N.stream()),
                "lattice_bwd")
        return d, None, None, None, None, None, None


def rnnt_lattice_loss(logits, ranges, symbols, boundary, blank=0, rnnt_type="regular",
                      delay_penalty=0.0):
    """Materialised lattice under k2.rnnt_loss_pruned's rnnt_type / delay_penalty; ranges None is
    the full lattice (R = S+1) for every type."""
    ty, pen = check_rnnt_type(rnnt_type, delay_penalty)
    return _LatticeLoss.apply(logits, ranges, symbols, boundary, blank, ty, pen)


def rnnt_full_lattice(am, lm, symbols, boundary, blank=0, activation="relu", rnnt_type="regular",
                      delay_penalty=0.0):
    """(px, py) of the FULL lattice of the fused joiner act(am[b,t,:] + lm[b,s,:]), never materialised:
    s2t_rnnt_pruned_fwd with zero ranges and a band of all S+1 rows.  am (B,T,C), lm (B,S+1,C) fp32,
    symbols (B,S) and boundary (B,4) int64 on the device -> px (B,S,T+1) on the regular lattice and
    (B,S,T) on the two others, py (B,S+1,T).  No autograd: the operands of mutual_information and of
    rnnt_align."""
    ty, pen = check_rnnt_type(rnnt_type, delay_penalty)
    _dev_check(am, lm)
    am = am.contiguous().float()
    lm = lm.contiguous().float()
    B, T, C = am.shape
    S = lm.shape[1] - 1
    _check_lattice_rows(S)
    if C > RNNT_MAX_JOINER_DIM:
        raise ValueError(f"fused pruned joiner: joiner dimension {C} exceeds the kernel's limit of "
                         f"{RNNT_MAX_JOINER_DIM} (a row is held in one wave's registers, csrc/rnnt.hip); "
                         "there is no fallback")
    dev = am.device
    px, py, lse = _lattice_buffers(B, S, T, S + 1, ty, dev)
    ranges = torch.zeros((B, T, S + 1), dtype=torch.int64, device=dev)     # (only each frame's first is read)
    N.PROF[0] and N.profile_note("s2t_rnnt_pruned_fwd",
                                 4.0 * (am.numel() + lm.numel() + px.numel() + py.numel() + lse.numel())
                                 + 8.0 * ranges.numel())
    N.check(N.lib().s2t_rnnt_pruned_fwd(N.fp(am), N.fp(lm), N.lp(ranges), N.lp(_i64(symbols, dev)),
                                        N.lp(_i64(boundary, dev)), B, S, T, C, S + 1, int(blank),
                                        _ACT[activation], ty, pen, N.fp(px), N.fp(py), N.fp(lse), N.stream()),
            "pruned_fwd")
    return px, py


def rnnt_logits_lattice(logits, symbols, boundary, blank=0, rnnt_type="regular", delay_penalty=0.0):
    """(px, py) of the full lattice of materialised logits (B,T,S+1,V): s2t_rnnt_lattice_fwd with
    ranges NULL.  No autograd."""
    ty, pen = check_rnnt_type(rnnt_type, delay_penalty)
    _dev_check(logits)
    logits = logits.contiguous().float()
    B, T, R, V = logits.shape
    S = symbols.shape[1]
    if R != S + 1:
        raise ValueError(f"rnnt_logits_lattice: logits {tuple(logits.shape)} are not the full lattice of "
                         f"{S} symbols (B,T,S+1,V)")
    _check_lattice_rows(S)
    dev = logits.device
    px, py, lse = _lattice_buffers(B, S, T, R, ty, dev)
    N.PROF[0] and N.profile_note("s2t_rnnt_lattice_fwd",
                                 4.0 * (logits.numel() + px.numel() + py.numel() + lse.numel()))
    N.check(N.lib().s2t_rnnt_lattice_fwd(N.fp(logits), None, N.lp(_i64(symbols, dev)),
                                         N.lp(_i64(boundary, dev)), B, S, T, V, R, int(blank), ty, pen,
                                         N.fp(px), N.fp(py), N.fp(lse), N.stream()), "lattice_fwd")
    return px, py


RnntAlignment = collections.namedtuple("RnntAlignment", ["tok_frame", "tok_logp", "score", "ok"])


def rnnt_align(px, py, boundary, rnnt_type="regular", out=None):
    """RNN-T forced alignment (csrc/rnnt_align.hip; the statement is in include/s2t_mi355.h): the
    operands of mutual_information -- px (B,S,T+1) for the regular lattice, (B,S,T) for 'modified' /
    'constrained', py (B,S+1,T) fp32, boundary (B,4) int64, contiguous on the device ->
    RnntAlignment(tok_frame (B,S) int32: the frame each symbol is emitted at, tok_logp (B,S) fp32: the
    log-probability on that arc, score (B) fp32: the best path's, ok (B) int32).  `out`: an earlier result
    of the same shapes to write into again (no allocation besides the workspace, where one is needed)."""
    if rnnt_type not in RNNT_TYPES:
        raise ValueError(f"rnnt_type {rnnt_type!r} is not one of 'regular', 'modified', 'constrained'")
    ty = RNNT_TYPES[rnnt_type]
    for t, dtype, what in ((px, torch.float32, "px"), (py, torch.float32, "py"), (boundary, torch.int64, "boundary")):
        if not t.is_cuda or t.dtype is not dtype or not t.is_contiguous():
            raise RuntimeError(f"rnnt_align: {what} must be a contiguous {dtype} device tensor, got "
                               f"{t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")
    if px.dim() != 3 or py.dim() != 3:
        raise ValueError(f"rnnt_align: px (B,S,T+1 or T) and py (B,S+1,T) expected, got {tuple(px.shape)}, "
                         f"{tuple(py.shape)}")
    B, S, TX = px.shape
    T = py.shape[2]
    if py.shape != (B, S + 1, T) or TX != (T + 1 if rnnt_type == "regular" else T) or boundary.shape != (B, 4):
        raise ValueError(f"rnnt_align: px {tuple(px.shape)}, py {tuple(py.shape)} and boundary "
                         f"{tuple(boundary.shape)} are not the (B,S,{'T+1' if rnnt_type == 'regular' else 'T'}), "
                         f"(B,S+1,T), (B,4) operands of the {rnnt_type} lattice")
    _check_lattice_rows(S)
    dev = px.device
    if out is None:
        out = RnntAlignment(torch.empty((B, S), dtype=torch.int32, device=dev),
                            torch.empty((B, S), dtype=torch.float32, device=dev),
                            torch.empty((B,), dtype=torch.float32, device=dev),
                            torch.empty((B,), dtype=torch.int32, device=dev))
    if B == 0:
        return out
    if T == 0:
        raise ValueError("rnnt_align: py has no frames; the lattice needs at least one (s2t_rnnt_align refuses T <= 0)")
    nbytes = N.lib().s2t_rnnt_align_workspace_bytes(B, S, T, ty)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    # an empty tensor has no address: the entry takes no output as NULL, and writes nothing there at S = 0
    tok = [t if S else ws for t in (out.tok_frame, out.tok_logp)]
    N.PROF[0] and N.profile_note("s2t_rnnt_align", 4.0 * (px.numel() + py.numel()) + 8.0 * B * S)
    rc = N.lib().s2t_rnnt_align(px.data_ptr(), N.fp(py), N.lp(boundary), B, S, T, ty, N.ptr(ws),
                                tok[0].data_ptr(), tok[1].data_ptr(), N.fp(out.score), N.ip(out.ok), N.stream())
    N.check(rc, "s2t_rnnt_align")
    return out


def make_boundary(target_lengths, frame_lengths, device):
    B = target_lengths.shape[0]
    b = torch.zeros((B, 4), dtype=torch.int64, device=device)
    b[:, 2] = target_lengths.to(device)
    b[:, 3] = frame_lengths.to(device)
    return b


# =============================================================== BEST-RQ SSL heads
NLL_STATS = N.const("S2T_NLL_STATS")     # floats per row the forward saves for the backward (csrc/ssl_loss.hip)


class _SmoothedNll(torch.autograd.Function):
    """Per-row  C0 - sum_c t_c log_softmax(scale * logits)_c  (csrc/ssl_loss.hip)."""

    @staticmethod
    def forward(ctx, logits, labels, scale, t_other, t_label, c0):
        _dev_check(logits)
        logits = logits.contiguous().float()
        rows, K = logits.shape
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        row = torch.empty(rows, dtype=torch.float32, device=logits.device)
        stats = torch.empty((rows, NLL_STATS), dtype=torch.float32, device=logits.device)
        N.PROF[0] and N.profile_note("s2t_smoothed_nll_fwd", 4.0 * logits.numel())
        N.check(N.lib().s2t_smoothed_nll_fwd(N.fp(logits), N.lp(labels), rows, K, float(scale),
                                             float(t_other), float(t_label), float(c0),
                                             N.fp(row), N.fp(stats), N.stream()), "smoothed_nll_fwd")
        ctx.save_for_backward(logits, labels, stats)
        ctx.cfg = (float(scale), float(t_other), float(t_label))
        return row

    @staticmethod
    def backward(ctx, g):
        logits, labels, stats = ctx.saved_tensors
        scale, t_other, t_label = ctx.cfg
        rows, K = logits.shape
        grad = torch.empty_like(logits)
        N.PROF[0] and N.profile_note("s2t_smoothed_nll_bwd", 8.0 * logits.numel())
        N.check(N.lib().s2t_smoothed_nll_bwd(N.fp(logits), N.lp(labels), N.fp(stats),
                                             N.fp(g.contiguous().float()), rows, K, scale, t_other,
                                             t_label, N.fp(grad), N.stream()), "smoothed_nll_bwd")
        return grad, None, None, None, None, None


def smoothed_nll_rows(logits2d, labels, scale, t_other, t_label, c0):
    return _SmoothedNll.apply(logits2d, labels, scale, t_other, t_label, c0)


# =============================================================== StatelessPredictor context
PRED_MAX_CONTEXT = 8      # == PRED_MAXK (csrc/predictor.hip)


class _PredictorContext(torch.autograd.Function):
    """out[b,u,:] = sum_k w[:,k] * emb[tokens[b,u+k]]: nn.Embedding + depthwise nn.Conv1d of
    reference stateless_predictor.py:27-105 as one gather pass (csrc/predictor.hip)."""

    @staticmethod
    def forward(ctx, tokens, emb, w):
        _dev_check(tokens, emb, w)
        B, L = tokens.shape
        V, D = emb.shape
        K = w.shape[-1]
        tok = tokens.to(torch.int32).contiguous()
        e, wk = emb.contiguous().float(), w.reshape(D, K).contiguous().float()
        out = torch.empty((B, L - K + 1, D), dtype=torch.float32, device=emb.device)
        N.PROF[0] and N.profile_note("s2t_predictor_ctx_fwd", 4.0 * (K + 1) * out.numel() + 4.0 * tok.numel())
        N.check(N.lib().s2t_predictor_ctx_fwd(N.ip(tok), N.fp(e), N.fp(wk), B, L, K, D, V, N.fp(out),
                                              N.stream()), "s2t_predictor_ctx_fwd")
        ctx.save_for_backward(tok, e, wk)
        ctx.wshape = w.shape
        return out

    @staticmethod
    def backward(ctx, g):
        tok, e, wk = ctx.saved_tensors
        B, L = tok.shape
        V, D = e.shape
        K = wk.shape[1]
        g = g.contiguous().float()
        de = torch.zeros_like(e) if ctx.needs_input_grad[1] else None
        dw = torch.zeros_like(wk) if ctx.needs_input_grad[2] else None
        N.PROF[0] and N.profile_note("s2t_predictor_ctx_bwd", 4.0 * (2 * K + 1) * g.numel() + 4.0 * tok.numel())
        N.check(N.lib().s2t_predictor_ctx_bwd(N.ip(tok), N.fp(e), N.fp(wk), N.fp(g), B, L, K, D, V,
                                              N.fp(de), N.fp(dw), N.stream()), "s2t_predictor_ctx_bwd")
        return None, de, (None if dw is None else dw.view(ctx.wshape))


def predictor_context(tokens, emb_weight, conv_weight):
    """tokens (B, L) integer, emb_weight (V, D), conv_weight (D, 1, K) -> (B, L-K+1, D)."""
    return _PredictorContext.apply(tokens, emb_weight, conv_weight)

