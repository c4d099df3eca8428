// The fbank kernels of csrc/fbank.hip (one-shot entry) and csrc/fbank_stream.hip (chunk-carried entry):
// ONE kernel text, instantiated once in each of the two sources, so that the entries cannot drift apart.
// The algorithm and its mapping to CDNA4 are described at the top of csrc/fbank.hip.
#pragma once
#include "../../include/s2t_mi355.h"
#include "common.h"

namespace {

constexpr int kFrameLen = 400;
constexpr int kHop = 160;
constexpr int kNfft = 512;
constexpr int kBins = 257;
constexpr int kFramesPerBlock = 32;
constexpr int kWaves = 4;
constexpr int kStage = (kFramesPerBlock - 1) * kHop + kFrameLen;  // 5360 samples
// The LDS image of a workgroup, about 41 KB: 32 frames' samples, the tables, and per wave a FFT buffer
// and two power spectra.
constexpr size_t kSmemBytes =
    sizeof(float) * (kStage + 2 * kNfft + kFrameLen + 1024 + 2 * kWaves * kNfft + kWaves * 2 * 260);

struct c32 {
  float x, y;
};
__device__ __forceinline__ c32 cadd(c32 a, c32 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ c32 csub(c32 a, c32 b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ c32 cmul(c32 a, c32 b) {
  return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
__device__ __forceinline__ c32 mul_negi(c32 a) { return {a.y, -a.x}; }  // a * (-i)

// In-register forward 8-point DFT (decimation in frequency), natural order out.
__device__ __forceinline__ void dft8(c32 v[8]) {
  const float c = 0.70710678118654752440f;
  c32 a0 = cadd(v[0], v[4]), a4 = csub(v[0], v[4]);
  c32 a1 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]);
  c32 a2 = cadd(v[2], v[6]), a6 = csub(v[2], v[6]);
  c32 a3 = cadd(v[3], v[7]), a7 = csub(v[3], v[7]);
  a5 = {c * (a5.x + a5.y), c * (a5.y - a5.x)};   // * w8^1
  a6 = mul_negi(a6);                             // * w8^2
  a7 = {c * (a7.y - a7.x), -c * (a7.x + a7.y)};  // * w8^3
  // even outputs: DFT4(a0..a3)
  c32 c0 = cadd(a0, a2), c2 = csub(a0, a2), c1 = cadd(a1, a3), c3 = mul_negi(csub(a1, a3));
  v[0] = cadd(c0, c1);
  v[4] = csub(c0, c1);
  v[2] = cadd(c2, c3);
  v[6] = csub(c2, c3);
  // odd outputs: DFT4(a4..a7)
  c32 d0 = cadd(a4, a6), d2 = csub(a4, a6), d1 = cadd(a5, a7), d3 = mul_negi(csub(a5, a7));
  v[1] = cadd(d0, d1);
  v[5] = csub(d0, d1);
  v[3] = cadd(d2, d3);
  v[7] = csub(d2, d3);
}

__device__ __forceinline__ long fbank_frames(long n) {
  return n >= kFrameLen ? 1 + (n - kFrameLen) / kHop : 0;
}

// ---- the fbank carried across chunks (the statement: include/s2t_mi355.h): what a call does ----
constexpr int kPairLen = kHop + kFrameLen;  // 560: pair P is complete when N >= 320 P + 560
constexpr int kCarryMax = S2T_FBANK_CARRY_MAX;
static_assert(kCarryMax == kPairLen - 1, "an un-emitted pair holds fewer than 560 samples");

// What a call does to row b, from its counts and the call's arguments: the same integers in every
// workgroup of the frame kernel and in the carry kernel that follows it.
struct ChunkPlan {
  long n;       // new samples taken (0 for an ended row)
  long total;   // N after the call
  long emitted; // frames emitted after the call
  int carried;  // live samples in carry before the call: N - 160 * emitted, 0..559
  int emit;     // frames this call emits
  bool ended, flush;
};

__device__ __forceinline__ ChunkPlan chunk_plan(const long* counts,
                                                const long* __restrict__ chunk_samples,
                                                const int* __restrict__ flush, long pcm_stride, int b) {
  const long* st = counts + (long)b * S2T_FBANK_STATE_LONGS;
  const long N = st[0], E = st[1];
  ChunkPlan p;
  p.ended = st[2] != 0;
  p.flush = !p.ended && flush[b] != 0;
  p.n = p.ended ? 0 : min(max(chunk_samples[b], 0L), pcm_stride);
  p.carried = (int)min(max(N - E * kHop, 0L), (long)kCarryMax);
  p.total = N + p.n;
  // pair p is complete when N >= 320 p + 560; a flush adds the lone frame of an odd count
  const long pairs = p.total >= kPairLen ? (p.total - kPairLen) / (2 * kHop) + 1 : 0;
  p.emitted = p.ended ? E : (p.flush ? fbank_frames(p.total) : 2 * pairs);
  p.emit = (int)max(p.emitted - E, 0L);
  return p;
}

// sample j of the row's un-emitted stream: the carried tail, then the chunk (the caller bounds j)
__device__ __forceinline__ float chunk_sample(const float* carry_b,
                                              const float* __restrict__ pcm_b, int carried, long j) {
  return j < carried ? carry_b[j] : pcm_b[j - carried];
}

// THE kernel body, instantiated twice: kChunk = false is the one-shot kernel (fbank_kernel), true the
// chunk kernel.  Mean, pre-emphasis, window, the three FFT passes, the un-packing, the silent-frame
// rule, mel, log and CMVN are this one text; the instantiations differ only in where a staged sample
// comes from (the utterance | the carried tail, then the chunk, then zero) and in which frames they
// store (frame f0 + i of the utterance, nframes of them | frame i counted from the row's first
// un-emitted frame, which is even, so that frames pair by ABSOLUTE index; nframes = those the call
// emits).  num_samples is chunk_samples for the chunk kernel; flush, carry, counts are its alone.
template <bool kChunk>
__global__ __launch_bounds__(256) void fbank_kernel(
    const float* __restrict__ pcm, long pcm_stride, const long* __restrict__ num_samples,
    const int* __restrict__ flush, const float* __restrict__ carry, const long* __restrict__ counts,
    const float* __restrict__ window,   // [400]
    const float* __restrict__ twiddle,  // [512][2]  exp(-2 pi i m / 512)
    const int* __restrict__ mel_off,    // [M+1] offsets into mel_w
    const int* __restrict__ mel_k0,     // [M] first FFT bin of each filter
    const float* __restrict__ mel_w,    // [nnz]
    int nnz, int num_mel, float eps, float scale_in, const float* __restrict__ cmvn_mean,
    const float* __restrict__ cmvn_istd, float* __restrict__ out, int max_frames,
    long* __restrict__ out_frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* s_pcm = reinterpret_cast<float*>(smem_raw);      // kStage
  c32* s_tw = reinterpret_cast<c32*>(s_pcm + kStage);     // 512
  float* s_win = reinterpret_cast<float*>(s_tw + kNfft);  // 400
  float* s_melw = s_win + kFrameLen;                      // nnz (<= 1024)
  c32* s_fft = reinterpret_cast<c32*>(s_melw + 1024);     // kWaves * 512
  float* s_pow = reinterpret_cast<float*>(s_fft + kWaves * kNfft);  // kWaves * 2 * 260

  const int b = blockIdx.y;
  const int f0 = blockIdx.x * kFramesPerBlock;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nframes;
  // ---- stage samples + constant tables (coalesced) ----
  if constexpr (kChunk) {
    const ChunkPlan p = chunk_plan(counts, num_samples, flush, pcm_stride, b);
    nframes = min(p.emit, max_frames);
    if (blockIdx.x == 0 && tid == 0 && out_frames) out_frames[b] = nframes;
    const float* carry_b = carry + (long)b * kCarryMax;
    const float* pcm_b = pcm + (long)b * pcm_stride;
    const long have = p.carried + p.n;
    for (int i = tid; i < kStage; i += 256) {
      const long j = (long)f0 * kHop + i;
      s_pcm[i] = (j < have) ? chunk_sample(carry_b, pcm_b, p.carried, j) * scale_in : 0.f;
    }
  } else {
    const long ns = num_samples[b];
    nframes = ns >= kFrameLen ? (int)(1 + (ns - kFrameLen) / kHop) : 0;
    if (blockIdx.x == 0 && tid == 0 && out_frames) out_frames[b] = nframes;
    const float* src = pcm + (long)b * pcm_stride + (long)f0 * kHop;
    const long remain = ns - (long)f0 * kHop;
    for (int i = tid; i < kStage; i += 256) s_pcm[i] = (i < remain) ? src[i] * scale_in : 0.f;
  }
  for (int i = tid; i < kNfft; i += 256) s_tw[i] = {twiddle[2 * i], twiddle[2 * i + 1]};
  for (int i = tid; i < kFrameLen; i += 256) s_win[i] = window[i];
  for (int i = tid; i < nnz; i += 256) s_melw[i] = mel_w[i];
  __syncthreads();

  c32* fbuf = s_fft + wave * kNfft;
  float* pA = s_pow + wave * 2 * 260;
  float* pB = pA + 260;

  for (int it = 0; it < kFramesPerBlock / (2 * kWaves); ++it) {
    const int fa = it * 2 * kWaves + wave * 2;  // local frame index of frame A
    const float* xa = s_pcm + fa * kHop;
    const float* xb = xa + kHop;
    // frame means (reference: torch.mean over the 400 raw samples)
    float sa = 0.f, sb = 0.f;
    int nza = 0, nzb = 0;
    for (int i = lane; i < kFrameLen; i += 64) {
      sa += xa[i];
      sb += xb[i];
      nza |= xa[i] != 0.f;
      nzb |= xb[i] != 0.f;
    }
    const float ma = wave_sum(sa) * (1.0f / kFrameLen);
    const float mb = wave_sum(sb) * (1.0f / kFrameLen);
    // A frame of exact zeros has no power, but packed with a loud partner it would receive what the
    // float32 FFT loses of Hermitian symmetry (measured 6.7e-4 at int16 sample scale, where the
    // partner's energies reach 1e11: 5600 x eps, where the reference gives log(eps)).
    const bool silent_a = __ballot(nza) == 0, silent_b = __ballot(nzb) == 0;

    // ---- pass A: lane = n2, element j = n1, sample index n = 64*j + lane ----
    c32 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n = 64 * j + lane;
      float ra = 0.f, rb = 0.f;
      if (n < kFrameLen) {
        const int np = n > 0 ? n - 1 : 0;
        const float w = s_win[n];
        const float a0 = __fsub_rn(xa[n], ma), a1 = __fsub_rn(xa[np], ma);
        const float b0 = __fsub_rn(xb[n], mb), b1 = __fsub_rn(xb[np], mb);
        ra = __fmul_rn(__fsub_rn(a0, __fmul_rn(a1, 0.97f)), w);
        rb = __fmul_rn(__fsub_rn(b0, __fmul_rn(b1, 0.97f)), w);
      }
      v[j] = {ra, rb};
    }
    dft8(v);
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) {
      c32 t = cmul(v[k1], s_tw[(lane * k1) & 511]);
      fbuf[k1 * 64 + lane] = t;
    }
    __syncthreads();
    // ---- pass B: lane = (k1, m2), element m1 ----
    {
      const int k1 = lane >> 3, m2 = lane & 7;
#pragma unroll
      for (int m1 = 0; m1 < 8; ++m1) v[m1] = fbuf[k1 * 64 + 8 * m1 + m2];
      dft8(v);
      __syncthreads();
#pragma unroll
      for (int q1 = 0; q1 < 8; ++q1) {
        c32 t = cmul(v[q1], s_tw[(8 * m2 * q1) & 511]);
        fbuf[k1 * 64 + q1 * 8 + m2] = t;
      }
    }
    __syncthreads();
    // ---- pass C: lane = (k1, q1), element m2 -> X[k1 + 8 q1 + 64 q2] ----
    {
      const int k1 = lane >> 3, q1 = lane & 7;
#pragma unroll
      for (int m2 = 0; m2 < 8; ++m2) v[m2] = fbuf[k1 * 64 + q1 * 8 + m2];
      dft8(v);
      __syncthreads();
#pragma unroll
      for (int q2 = 0; q2 < 8; ++q2) fbuf[k1 + 8 * q1 + 64 * q2] = v[q2];
    }
    __syncthreads();
    // ---- un-pack the two real spectra, power ----
    for (int k = lane; k < kBins; k += 64) {
      const c32 z = fbuf[k], zc = fbuf[(kNfft - k) & 511];
      const float ar = z.x + zc.x, ai = z.y - zc.y;
      const float br = z.x - zc.x, bi = z.y + zc.y;
      pA[k] = 0.25f * (ar * ar + ai * ai);
      pB[k] = 0.25f * (br * br + bi * bi);
    }
    __syncthreads();
    // ---- mel filterbank + log + optional CMVN, coalesced row stores ----
    const int ga = f0 + fa, gb = ga + 1;
    for (int m = lane; m < num_mel; m += 64) {
      const int o0 = mel_off[m], o1 = mel_off[m + 1], k0 = mel_k0[m];
      float ea = 0.f, eb = 0.f;
      for (int i = o0; i < o1; ++i) {
        const float w = s_melw[i];
        ea = fmaf(pA[k0 + i - o0], w, ea);
        eb = fmaf(pB[k0 + i - o0], w, eb);
      }
      if (silent_a) ea = 0.f;
      if (silent_b) eb = 0.f;
      float la = logf(fmaxf(ea, eps)), lb = logf(fmaxf(eb, eps));
      float mean = 0.f, istd = 1.f;
      if (cmvn_mean) {
        mean = cmvn_mean[m];
        istd = cmvn_istd[m];
      }
      if (ga < max_frames) {
        const float val = ga < nframes ? la : 0.f;
        out[((long)b * max_frames + ga) * num_mel + m] = cmvn_mean ? (val - mean) * istd : val;
      }
      if (gb < max_frames) {
        const float val = gb < nframes ? lb : 0.f;
        out[((long)b * max_frames + gb) * num_mel + m] = cmvn_mean ? (val - mean) * istd : val;
      }
    }
    __syncthreads();
  }
}

}  // namespace
