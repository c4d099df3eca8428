// RNN-T beam search (reference model/decoding.py:295-425 RnntBeamDecoding.decode) for the
// stateless predictor and a joiner without output projection, for gfx950.
//
// The reference is a Python loop per utterance, per frame, per beam, with a predictor module call
// per surviving beam per frame.  Here the whole batch is ONE launch, one workgroup (8 waves) per
// utterance, walking its frames on the device:
//   A  a wave per live beam (8 at a time): z = act(am[t] + lm[beam]), the cutoff_top_k best classes by
//      (z descending, class ascending) in cutoff_top_k rounds of wave arg-max, lse = log sum exp z;
//      one candidate (beam score + z - lse, class) per selected class.  log-softmax is monotone in
//      z, so the order is taken on z itself (no ties created by the subtraction).
//   B  a thread per candidate ranks it by counting the candidates that beat it
//      (score descending, then parent position, then rank in the parent's top-k: the candidate
//      index); the beam_size best become the new beams.  Equal hypotheses are NOT merged.
//   C  wave 0 builds the new beams: a blank candidate keeps its parent's predictor state and lm
//      row, any other class shifts the token in and takes a free lm row; one (parent, class)
//      record per kept beam goes to the workspace -- token histories are never copied.
//   D  lm = pre_proj(linear(conv(embed(state)))) is recomputed for the beams that emitted only,
//      up to 4 beams per pass over the weights (the arithmetic per beam is the greedy kernel's:
//      with beam_size = cutoff_top_k = 1 the walk is s2t_rnnt_greedy_stateless at
//      max_token_step = 0, bit for bit).
// After the last frame the best beam (position 0) is traced back through the records
// (decode_records.h trace_best, which also holds the record, the ranking of B and the limits).
// lm [beam_size][V] lives in LDS when it fits and in the workspace (L2 resident) when it does not.
// s2t_rnnt_beam_stateless_ngram is the same walk in beam_walk's n-gram mode (decode_search.h): between A
// and B a thread per candidate adds lm_weight x the back-off n-gram's look-up, C carries the context id.
#include "common.h"
#include "decode_search.h"

namespace {

using namespace s2t_dec;           // Top, better, wave_top, after, activate (decode_common.h); the
                                   // constants, BeamShared, recompute_lm, beam_walk (decode_search.h);
                                   // clamped_len, trace_best, align256 (decode_records.h)

struct BeamArgs {
  const float* am;        // [B][T][V]  = enc_proj(encoder_out), bias included
  const long* lengths;    // [B]
  const float* emb;       // [num_symbols][E]
  const float* conv_w;    // [E][ctx]   depthwise, no bias
  const float* lin_w;     // [D][E]
  const float* lin_b;     // [D]
  const float* pre_w;     // [V][D]
  const float* pre_b;     // [V]
  int T, V, E, D, ctx, act, blank, beam, topk, lm_in_lds;
  int* records;           // [B][T][beam]  pack_record(parent, class)
  float* lm_spill;        // [B][beam][V]  (used when lm does not fit the LDS)
  long* tokens;           // [B][T]
  long* frames;           // [B][T]
  long* out_len;          // [B]
  float* score;           // [B]
};

template <bool CACHE>
__global__ __launch_bounds__(kThreads) void rnnt_beam_kernel(BeamArgs a) {
  extern __shared__ float sm[];
  __shared__ BeamShared s;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = a.V, BS = a.beam;
  float* e = sm;                                           // [kGroup][E]
  float* h = e + kGroup * a.E;                             // [kGroup][D]
  int* state = reinterpret_cast<int*>(h + kGroup * a.D);   // [2][kMaxBeam][ctx], most recent last
  float* lm = a.lm_in_lds ? reinterpret_cast<float*>(state + 2 * kMaxBeam * a.ctx)
                          : a.lm_spill + (long)b * BS * V;  // [beam][V]
  const int Tb = (int)clamped_len(a.lengths, b, a.T);
  if (Tb == 0) {                                           // no frames: no tokens, score 0
    if (tid == 0) {
      a.out_len[b] = 0;
      a.score[b] = 0.f;
    }
    return;
  }
  const float* amb = a.am + (long)b * a.T * V;
  int* rec = a.records + (long)b * a.T * BS;

  // one beam: no tokens, score 0, state = init state + the blank start token
  for (int k = tid; k < a.ctx; k += kThreads) state[k] = a.blank;
  if (tid == 0) {
    s.score[0][0] = 0.f;
    s.slot[0][0] = 0;
    s.len[0][0] = 0;
    s.emit[0] = 0;
  }
  __syncthreads();
  recompute_lm(a, s.emit, 1, state, s.slot[0], e, h, lm);
  int nb = 1, cur = 0;
  // phases A-D per frame: shared with the chunk-carried kernel (decode_search.h)
  beam_walk<CACHE>(a, s, amb, Tb, nb, cur, e, h, state, lm,
                   [&](int t, int pos, int r) { rec[(long)t * BS + pos] = r; });

  // ---- the best beam is position 0: trace its (parent, class) records back
  const int n = s.len[cur][0];
  if (tid == 0) {
    a.out_len[b] = n;
    a.score[b] = s.score[cur][0];
  }
  trace_best<kThreads>(rec, Tb, BS, a.blank, n, s.trace, &s.nemit, a.tokens + (long)b * a.T,
                       a.frames + (long)b * a.T);
}

// ---- the same search fused with a back-off n-gram (ngram_lookup.h): beam_walk's n-gram mode.  A beam
// also carries a context id and the unweighted sum of its look-ups; nothing runs between frames.
struct BeamNgramArgs {
  BeamArgs c;
  NgramTables g;
  float lm_weight;
  int start_ctx;
  float* lm_score;        // [B]
};

template <bool CACHE>
__global__ __launch_bounds__(kThreads) void rnnt_beam_ngram_kernel(BeamNgramArgs a) {
  extern __shared__ float sm[];
  __shared__ BeamShared s;
  __shared__ RnntNgramShared ng;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = a.c.V, BS = a.c.beam;
  float* e = sm;                                           // [kGroup][E]
  float* h = e + kGroup * a.c.E;                           // [kGroup][D]
  int* state = reinterpret_cast<int*>(h + kGroup * a.c.D); // [2][kMaxBeam][ctx], most recent last
  float* lm = a.c.lm_in_lds ? reinterpret_cast<float*>(state + 2 * kMaxBeam * a.c.ctx)
                            : a.c.lm_spill + (long)b * BS * V;
  const int Tb = (int)clamped_len(a.c.lengths, b, a.c.T);
  if (Tb == 0) {                                           // no frames: no tokens, score 0, lm_score 0
    if (tid == 0) {
      a.c.out_len[b] = 0;
      a.c.score[b] = 0.f;
      a.lm_score[b] = 0.f;
    }
    return;
  }
  const float* amb = a.c.am + (long)b * a.c.T * V;
  int* rec = a.c.records + (long)b * a.c.T * BS;

  // one beam: no tokens, score 0, ctx blanks, the LM's start context, no LM sum
  for (int k = tid; k < a.c.ctx; k += kThreads) state[k] = a.c.blank;
  if (tid == 0) {
    s.score[0][0] = 0.f;
    s.slot[0][0] = 0;
    s.len[0][0] = 0;
    s.emit[0] = 0;
    ng.g = a.g;
    ng.ctx[0][0] = a.start_ctx;
    ng.lm_sum[0][0] = 0.f;
  }
  __syncthreads();
  recompute_lm(a.c, s.emit, 1, state, s.slot[0], e, h, lm);
  int nb = 1, cur = 0;
  beam_walk<CACHE, kLmNgram>(a.c, s, amb, Tb, nb, cur, e, h, state, lm,
                             [&](int t, int pos, int r) { rec[(long)t * BS + pos] = r; }, &ng, a.lm_weight);

  const int n = s.len[cur][0];
  if (tid == 0) {
    a.c.out_len[b] = n;
    a.c.score[b] = s.score[cur][0];
    a.lm_score[b] = ng.lm_sum[cur][0];
  }
  trace_best<kThreads>(rec, Tb, BS, a.c.blank, n, s.trace, &s.nemit, a.c.tokens + (long)b * a.c.T,
                       a.c.frames + (long)b * a.c.T);
}

size_t records_bytes(int B, int T, int beam) { return align256(sizeof(int) * (size_t)B * T * beam); }

// what s2t_rnnt_beam_stateless refuses of its shape
bool beam_shape_ok(int T, int V, int E, int D, int ctx, int act, int blank, int beam_size, int cutoff_top_k) {
  return T > 0 && V > 0 && V <= 8192 && E > 0 && D > 0 && ctx >= 1 && ctx <= 64 && act >= 0 && act <= 1 &&
         blank >= 0 && blank < V && beam_size >= 1 && beam_size <= kMaxBeam && cutoff_top_k >= 1 &&
         (cutoff_top_k < V ? cutoff_top_k : V) <= kMaxBeam && beam_fixed_lds(E, D, ctx) <= kLdsBudget;
}

}  // namespace

extern "C" long s2t_rnnt_beam_workspace_bytes(int B, int T, int V, int beam_size) {
  if (B <= 0 || T <= 0 || V <= 0 || beam_size <= 0) return 0;
  return (long)(records_bytes(B, T, beam_size) + align256(sizeof(float) * (size_t)B * beam_size * V));
}

extern "C" int s2t_rnnt_beam_stateless(const float* am, const long* lengths, const float* emb,
                                       const float* conv_w, const float* lin_w, const float* lin_b,
                                       const float* pre_w, const float* pre_b, int B, int T, int V,
                                       int E, int D, int ctx, int act, int blank, int beam_size,
                                       int cutoff_top_k, void* workspace, long* tokens, long* frames,
                                       long* out_len, float* score, void* stream) {
  if (B <= 0) return 0;
  if (!beam_shape_ok(T, V, E, D, ctx, act, blank, beam_size, cutoff_top_k) || !workspace) return -1;
  const size_t fixed = beam_fixed_lds(E, D, ctx);
  const size_t lm_bytes = sizeof(float) * (size_t)beam_size * V;
  const int lm_in_lds = fixed + lm_bytes <= kLdsBudget;
  char* ws = static_cast<char*>(workspace);
  BeamArgs a{am, lengths, emb, conv_w, lin_w, lin_b, pre_w, pre_b, T, V, E, D, ctx, act, blank,
             beam_size, cutoff_top_k, lm_in_lds, reinterpret_cast<int*>(ws),
             reinterpret_cast<float*>(ws + records_bytes(B, T, beam_size)), tokens, frames, out_len,
             score};
  const size_t smem = fixed + (lm_in_lds ? lm_bytes : 0);
  if (V <= 64 * kRegs)
    hipLaunchKernelGGL(rnnt_beam_kernel<true>, dim3(B), dim3(kThreads), smem, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(rnnt_beam_kernel<false>, dim3(B), dim3(kThreads), smem, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

extern "C" long s2t_rnnt_beam_ngram_workspace_bytes(int B, int T, int V, int beam_size) {
  if (V > 8192 || beam_size > kMaxBeam) return 0;
  return s2t_rnnt_beam_workspace_bytes(B, T, V, beam_size);
}

extern "C" int s2t_rnnt_beam_stateless_ngram(const S2tNgramLmDesc* lm, const float* am, const long* lengths,
                                             const float* emb, const float* conv_w, const float* lin_w,
                                             const float* lin_b, const float* pre_w, const float* pre_b, int B,
                                             int T, int V, int E, int D, int ctx, int act, int blank,
                                             int beam_size, int cutoff_top_k, float lm_weight, int start_ctx,
                                             void* workspace, long* tokens, long* frames, long* out_len,
                                             float* score, float* lm_score, void* stream) {
  if (B <= 0) return 0;
  if (!beam_shape_ok(T, V, E, D, ctx, act, blank, beam_size, cutoff_top_k) || !ngram_desc_ok(lm) || lm->V != V ||
      start_ctx < 0 || start_ctx >= lm->num_ctx || !__builtin_isfinite(lm_weight) || !workspace || !lm_score)
    return -1;
  const size_t fixed = beam_fixed_lds(E, D, ctx);
  const size_t lm_bytes = sizeof(float) * (size_t)beam_size * V;
  const int lm_in_lds = fixed + lm_bytes <= kLdsBudget;
  char* ws = static_cast<char*>(workspace);
  BeamNgramArgs a{{am, lengths, emb, conv_w, lin_w, lin_b, pre_w, pre_b, T, V, E, D, ctx, act, blank, beam_size,
                   cutoff_top_k, lm_in_lds, reinterpret_cast<int*>(ws),
                   reinterpret_cast<float*>(ws + records_bytes(B, T, beam_size)), tokens, frames, out_len, score},
                  ngram_tables(*lm), lm_weight, start_ctx, lm_score};
  const size_t smem = fixed + (lm_in_lds ? lm_bytes : 0);
  if (V <= 64 * kRegs)
    hipLaunchKernelGGL(rnnt_beam_ngram_kernel<true>, dim3(B), dim3(kThreads), smem, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(rnnt_beam_ngram_kernel<false>, dim3(B), dim3(kThreads), smem, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}
