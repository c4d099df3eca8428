// Batched kaldi-style log-mel filterbank ("fbank") for gfx950.
//
// Replaces, for a whole padded batch of utterances in one launch, the
// per-utterance CPU call  dataset/frontend/frontend.py:85-94
// (torchaudio.compliance.kaldi.fbank, whose op graph is stated in
// sample_data/model/frontend.script) and optionally the following
// GlobalCmvnLayer (model/layer/global_cmvn.py:30-38).
//
// Algorithm per frame (snip_edges): 400 samples at hop 160 -> subtract frame
// mean -> pre-emphasis 0.97 (replicate first sample) -> Povey window ->
// zero-pad to 512 -> |rFFT|^2 -> triangular mel filterbank -> log(max(.,eps)).
// A frame whose 400 samples are all exactly zero gives log(eps) in every bin.
//
// Mapping to CDNA4: one 256-thread workgroup stages the samples of 32
// consecutive frames of one utterance in LDS with coalesced 4-byte loads
// (HBM is read once: 160 new samples per frame).  Each 64-lane wave packs TWO
// real frames into one complex 512-point FFT (re = frame A, im = frame B);
// the FFT is 8x8x8: three register-resident radix-8 butterflies with two LDS
// transposes, twiddles from a host-computed (double precision) table held in
// LDS.  The mel filterbank is stored compactly (each FFT bin touches <= 2
// filters) and applied from LDS; the log/CMVN epilogue is fused and frames
// are written as contiguous rows.
//
// The kernel text is csrc/fbank_kernel.h: this file instantiates it for whole utterances,
// csrc/fbank_stream.hip for audio that arrives in cuts (s2t_fbank_chunk_f32).
#include "fbank_kernel.h"

// C ABI -- see include/s2t_mi355.h
extern "C" int s2t_fbank_f32(const float* pcm, long pcm_stride, const long* num_samples,
                             int batch, const float* window400, const float* twiddle512,
                             const int* mel_off, const int* mel_k0, const float* mel_w, int nnz,
                             int num_mel, float eps, float scale_in, const float* cmvn_mean,
                             const float* cmvn_istd, float* out, int max_frames,
                             long* out_frames, void* stream) {
  if (batch <= 0 || max_frames <= 0) return 0;
  if (nnz > 1024 || num_mel > 128 || num_mel <= 0) return -1;
  dim3 grid((max_frames + kFramesPerBlock - 1) / kFramesPerBlock, batch);
  hipLaunchKernelGGL(fbank_kernel<false>, grid, dim3(256), kSmemBytes, (hipStream_t)stream, pcm,
                     pcm_stride, num_samples, nullptr, nullptr, nullptr, window400, twiddle512, mel_off, mel_k0, mel_w, nnz, num_mel,
                     eps, scale_in, cmvn_mean, cmvn_istd, out, max_frames, out_frames);
  S2T_CHECK_LAUNCH();
  return 0;
}
