// Validation-time greedy decoders for gfx950.
//
// CTC greedy search (reference model/decoding.py:51-82 CtcGreedyDecoding.decode, called per
// utterance by batch_search :27-48): per-frame argmax, collapse repeats, drop blanks -- the
// whole batch in ONE launch, one workgroup per utterance.
// RNN-T greedy search (reference model/decoding.py:196-271 RnntGreedyDecoding.decode) for the
// stateless predictor (model/predictor/stateless_predictor.py:109-125 streaming_step) and a
// joiner without output projection (model/joiner/joiner.py:186-207 streaming_step): the
// reference runs a Python loop of predictor / joiner module calls per lattice move; here one
// workgroup per utterance walks its lattice on the device.  The predictor state is the last
// `ctx` tokens, so the language-side vector lm = pre_proj(linear(conv(embed(state)))) is
// recomputed (two wave-per-row GEMVs) only when a symbol is emitted.  The walk is decode_search.h's
// greedy_walk (decode_rnnt.hip runs it a chunk at a time, and holds the beam searches).  This kernel stays in
// this code object: next to the ten kernels of decode_rnnt.hip, instruction for instruction the same, it
// measured 1 % slower.
#include "common.h"
#include "decode_search.h"

namespace {

struct ArgMax {
  float v;
  int i;
};
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {   // first index wins ties
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
__device__ __forceinline__ ArgMax wave_argmax(ArgMax a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ArgMax b;
    b.v = __shfl_xor(a.v, o, 64);
    b.i = __shfl_xor(a.i, o, 64);
    a = better(a, b);
  }
  return a;
}

__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* __restrict__ logits,
                                                         const long* __restrict__ lengths, int T,
                                                         int V, int blank,
                                                         long* __restrict__ tokens,
                                                         long* __restrict__ out_len) {
  extern __shared__ int ids[];                       // [T] per-frame argmax
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long Tb = lengths[b];
  if (Tb > T) Tb = T;
  if (Tb < 0) Tb = 0;
  const float* x = logits + (long)b * T * V;
  for (int t = wave; t < Tb; t += 4) {
    ArgMax a{S2T_NEG_INF, V};
    for (int c = lane; c < V; c += 64) a = better(a, ArgMax{x[(long)t * V + c], c});
    a = wave_argmax(a);
    if (lane == 0) ids[t] = a.i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long n = 0;
    int prev = blank;
    long* out = tokens + (long)b * T;
    for (int t = 0; t < Tb; ++t) {
      const int p = ids[t];
      if ((p != prev || prev == blank) && p != blank) out[n++] = p;
      prev = p;
    }
    out_len[b] = n;
  }
}

struct RnntGreedyArgs {
  const float* am;        // [B][T][V]  = enc_proj(encoder_out), bias included
  const long* lengths;    // [B]
  s2t_dec::StatelessPointers p;
  int T;
  s2t_dec::StatelessDims d;
  int max_token_step, max_out, blank;
  long* tokens;           // [B][max_out]
  long* out_len;          // [B]
};

__global__ __launch_bounds__(s2t_dec::kGreedyThreads) void rnnt_greedy_kernel(RnntGreedyArgs a) {
  extern __shared__ float sm[];
  float* e = sm;                       // [E]   conv(embed(state))
  float* hvec = e + a.d.E;             // [D]
  float* lm = hvec + a.d.D;            // [V]
  int* state = reinterpret_cast<int*>(lm + a.d.V);   // [ctx] most recent last
  __shared__ s2t_dec::GreedyShared s_walk;
  const int b = blockIdx.x, tid = threadIdx.x;
  long Tb = a.lengths[b];
  if (Tb > a.T) Tb = a.T;
  for (int k = tid; k < a.d.ctx; k += s2t_dec::kGreedyThreads) state[k] = a.blank;   // init_state + blank start token
  __syncthreads();
  long n = 0;
  bool need_lm = true;
  // the walk itself is shared with the chunk-carried kernel (decode_search.h)
  s2t_dec::greedy_walk(a.p, a.d, a.max_token_step, a.blank, s_walk, a.am + (long)b * a.T * a.d.V, Tb, state, e, hvec, lm,
                       need_lm, n, a.tokens + (long)b * a.max_out, a.max_out);
  if (tid == 0) a.out_len[b] = n < a.max_out ? n : a.max_out;
}

}  // namespace

extern "C" int s2t_ctc_greedy(const float* logits, const long* lengths, int B, int T, int V,
                              int blank, long* tokens, long* out_len, void* stream) {
  if (B <= 0) return 0;
  if (T <= 0 || V <= 0 || blank < 0 || blank >= V || T > 16000) return -1;
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), sizeof(int) * T, (hipStream_t)stream,
                     logits, lengths, T, V, blank, tokens, out_len);
  S2T_CHECK_LAUNCH();
  return 0;
}

// (this entry alone has never tested its blank, and holds V to its LDS only: tests/test_rnnt_refusals.py)
extern "C" int s2t_rnnt_greedy_stateless(const float* am, const long* lengths, const float* emb,
                                         const float* conv_w, const float* lin_w,
                                         const float* lin_b, const float* pre_w, const float* pre_b,
                                         int B, int T, int V, int E, int D, int ctx, int act,
                                         int max_token_step, int max_out, int blank, long* tokens,
                                         long* out_len, void* stream) {
  if (B <= 0) return 0;
  const s2t_dec::StatelessWeights w = s2t_dec::stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act);
  if (!s2t_dec::greedy_ok(T, w, max_out)) return -1;
  RnntGreedyArgs a{am, lengths, w, T, w, max_token_step, max_out, blank, tokens, out_len};
  hipLaunchKernelGGL(rnnt_greedy_kernel, dim3(B), dim3(s2t_dec::kGreedyThreads), s2t_dec::greedy_lds(w),
                     (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}
