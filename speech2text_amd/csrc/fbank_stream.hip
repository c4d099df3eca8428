// The fbank carried across chunks: s2t_fbank_chunk_f32 (the statement: include/s2t_mi355.h).
// Audio arrives in arbitrary cuts; the frames leave as s2t_fbank_f32 would have computed them on the whole
// audio, bit for bit.  The frame kernel is the chunk instantiation of csrc/fbank_kernel.h's one kernel text
// (the one-shot entry of csrc/fbank.hip is the other); the state update is a second small launch behind it.
#include "fbank_kernel.h"

namespace {

// The state update, a launch of its own behind the frame kernel: one workgroup per row moves the new
// tail to the front of carry (through registers, the ranges overlap) and writes the counts.
__global__ __launch_bounds__(256) void fbank_carry_kernel(
    const float* __restrict__ pcm, long pcm_stride, const long* __restrict__ chunk_samples,
    const int* __restrict__ flush, float* carry, long* counts) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const ChunkPlan p = chunk_plan(counts, chunk_samples, flush, pcm_stride, b);
  if (p.ended) return;
  float* carry_b = carry + (long)b * kCarryMax;
  const float* pcm_b = pcm + (long)b * pcm_stride;
  const long shift = (p.emitted - counts[(long)b * S2T_FBANK_STATE_LONGS + 1]) * kHop;
  // an ended row's tail is dead; a live one keeps N - 160 * emitted <= 559 samples
  const int keep = p.flush ? 0 : (int)min(max(p.carried + p.n - shift, 0L), (long)kCarryMax);
  constexpr int kPer = (kCarryMax + 255) / 256;
  float v[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int j = tid + 256 * k;
    v[k] = j < keep ? chunk_sample(carry_b, pcm_b, p.carried, shift + j) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int j = tid + 256 * k;
    if (j < keep) carry_b[j] = v[k];
  }
  if (tid == 0) {
    long* st = counts + (long)b * S2T_FBANK_STATE_LONGS;
    st[0] = p.total;
    st[1] = p.emitted;
    st[2] = p.flush ? 1 : 0;
  }
}

}  // namespace

// C ABI -- see include/s2t_mi355.h
extern "C" int s2t_fbank_chunk_max_frames(long chunk_samples) {
  if (chunk_samples < 1) return 1;  // nothing new completes a pair; a flush may emit the lone frame
  const long f = 2 * ((chunk_samples - 1) / (2 * kHop) + 1) + 1;
  return f > 0x7fffffffL ? 0x7fffffff : (int)f;
}

extern "C" int s2t_fbank_chunk_f32(const float* pcm, long pcm_stride, const long* chunk_samples,
                                   const int* flush, int batch, float* carry, long* counts,
                                   const float* window400, const float* twiddle512,
                                   const int* mel_off, const int* mel_k0, const float* mel_w, int nnz,
                                   int num_mel, float eps, float scale_in, const float* cmvn_mean,
                                   const float* cmvn_istd, float* out, int max_new_frames,
                                   long* new_frames, void* stream) {
  if (batch <= 0) return 0;
  if (nnz > 1024 || num_mel > 128 || num_mel <= 0) return -1;
  if (pcm_stride < 0 || !carry || !counts || !chunk_samples || !flush || !out) return -1;
  if (max_new_frames < s2t_fbank_chunk_max_frames(pcm_stride)) return -1;
  dim3 grid((max_new_frames + kFramesPerBlock - 1) / kFramesPerBlock, batch);
  hipLaunchKernelGGL(fbank_kernel<true>, grid, dim3(256), kSmemBytes, (hipStream_t)stream, pcm,
                     pcm_stride, chunk_samples, flush, carry, counts, window400, twiddle512,
                     mel_off, mel_k0, mel_w, nnz, num_mel, eps, scale_in, cmvn_mean, cmvn_istd, out,
                     max_new_frames, new_frames);
  S2T_CHECK_LAUNCH();
  hipLaunchKernelGGL(fbank_carry_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, pcm,
                     pcm_stride, chunk_samples, flush, carry, counts);
  S2T_CHECK_LAUNCH();
  return 0;
}
