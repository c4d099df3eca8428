// The one-launch RNN-T beam searches for the stateless predictor (model/predictor/stateless_predictor.py:109-125
// streaming_step) and a joiner without output projection (reference model/decoding.py:295-425
// RnntBeamDecoding.decode), whole utterances and chunk-carried streams, plain or fused with a back-off n-gram;
// and the chunk-carried form of the greedy search (the whole-utterance one: decode.hip).  The reference is a
// Python loop per utterance, frame and beam; here the whole batch is ONE launch, one workgroup (8 waves) per
// utterance, walking its frames on the device (decode_search.h beam_walk):
//   A  a wave per live beam (8 at a time): z = act(am[t] + lm[beam]), the cutoff_top_k best classes by
//      (z descending, class ascending) in cutoff_top_k rounds of wave arg-max, lse = log sum exp z;
//      one candidate (beam score + z - lse, class) per selected class.  log-softmax is monotone in
//      z, so the order is taken on z itself (no ties created by the subtraction).
//   B  a thread per candidate ranks it by counting the candidates that beat it
//      (score descending, then parent position, then rank in the parent's top-k: the candidate
//      index); the beam_size best become the new beams.  Equal hypotheses are NOT merged.
//   C  wave 0 builds the new beams: a blank candidate keeps its parent's predictor state and lm
//      row, any other class shifts the token in and takes a free lm row; one (parent, class)
//      record per kept beam is written -- token histories are never copied per frame.
//   D  lm = pre_proj(linear(conv(embed(state)))) is recomputed for the beams that emitted only, up to 4 beams
//      per pass over the weights (per beam the greedy kernel's arithmetic: with beam_size = cutoff_top_k = 1
//      the walk is s2t_rnnt_greedy_stateless at max_token_step = 0, bit for bit).
// In the n-gram mode a thread per candidate adds lm_weight x the n-gram's look-up between A and B, and C
// carries the context id and the unweighted sum of the look-ups.  lm [beam_size][V] lives in LDS when it fits
// and in the workspace / the state row (L2 resident) when not.  Whole utterance: after the last frame the best
// beam (position 0) is traced back through the records (decode_records.h trace_best).
// In the hotword mode (BIAS; without an LM or with the n-gram) the same thread adds bias_weight x the context
// graph's look-up behind the LM term, C carries the graph state and the unweighted sum, and when an entry writes
// its outputs it reports the live beam that is best once the loan of an unfinished match is taken back
// (decode_search.h bias_pick): outputs only, nothing of the pick is stored or carried.
//
// Chunk-carried: the same walks fed their frames in pieces, so for any cut of [0, L) into chunks the result
// is the whole-utterance search's on the concatenated am, bit for bit; what is added is what is carried.
// One caller-owned device buffer holds a row of state per stream (s2t_rnnt_stream_state_bytes):
//   greedy  hdr {tokens so far, frames so far, inert, lm valid} | predictor state [ctx] | lm [V]
//   beam    hdr {beams, frames so far, overflow, lm valid, history buffer in use, stable_len}
//           | score [16] | len [16] | lm row of each beam [16] | predictor states [16][ctx]
//           | lm [beam][V] | records [256][beam] | token histories [2][beam][max_tokens]
//           | frame histories [2][beam][max_tokens]
//   n-gram  the beam row, every offset unchanged | ctx [beam] int32 | lm_sum [beam] fp32
//   bias    the beam or the n-gram row, byte for byte | bstate [beam] int32 | bsum [beam] fp32
// The lm rows are PERSISTED, not recomputed on entry: a chunk then starts with beam V floats from
// HBM instead of up to four passes over the predictor's weights, and when the rows do not fit the LDS the
// search works on them in place.  Only a reset row has no lm yet (reset takes no weights): its first chunk
// computes it, as the whole-utterance kernels do.
//
// The chunk beam search keeps (parent, class) records for the frames of THIS chunk only (hence Tc <= 256:
// they have a fixed home in the state row).  At chunk end a lane per surviving beam walks them back
// to the beam's ancestor position at chunk start, writing the chunk's emissions to the tail of the
// beam's new history on the way; a wave per beam then copies the ancestor's history in front of
// them.  The two history buffers swap roles per chunk, so a history is never copied onto itself.
// This is the text of decode_records.h chunk_histories (the LSTM chunk end calls that), kept written
// out here, with the chunk length clamped by hand: through the shared function, in every form tried,
// the chunk search measured 1.6-2.4 % slower (profiles/decode_records_resources.txt).
#include <type_traits>

#include "common.h"
#include "decode_search.h"

namespace {

using namespace s2t_dec;           // Top, better, wave_top, after, activate (decode_common.h); StatelessWeights,
                                   // the constants, BeamShared, the walks (decode_search.h); clamped_len,
                                   // trace_best, align256 (decode_records.h)

constexpr int kHdr = 64;           // bytes of a row's header, and of each [16] array after it
constexpr int kMaxV = 8192;

// ------------------------------------------------------------------------------------ a row of state
struct Layout {                    // byte offsets inside a row of state
  long pstate, lm, rec, htok, hfrm, stride;
};

bool row_ok(int V, int ctx, int beam, int max_tokens) {
  return V > 0 && V <= kMaxV && ctx >= 1 && ctx <= 64 && beam >= 0 && beam <= kMaxBeam && max_tokens > 0;
}

// o_ng given: the n-gram beam row, which is the plain beam row, every offset unchanged, followed by ctx [beam]
// int32, the beams' n-gram context ids, and lm_sum [beam] fp32.  o_bias given: that row (plain or n-gram),
// byte for byte, followed by bstate [beam] int32, the beams' hotword graph states, and bsum [beam] fp32
Layout layout(int V, int ctx, int beam, int max_tokens, long* o_ng = nullptr, long* o_bias = nullptr) {
  Layout l{};
  if (beam == 0) {                 // greedy
    l.pstate = 16;
    l.lm = l.pstate + (long)sizeof(int) * ctx;
    l.stride = (long)align256(l.lm + sizeof(float) * (size_t)V);
    return l;
  }
  l.pstate = 4 * kHdr;
  l.lm = (long)align256(l.pstate + sizeof(int) * (size_t)kMaxBeam * ctx);
  l.rec = (long)align256(l.lm + sizeof(float) * (size_t)beam * V);
  l.htok = (long)align256(l.rec + sizeof(int) * (size_t)kMaxChunk * beam);
  l.hfrm = l.htok + (long)(sizeof(int) * 2 * (size_t)beam * max_tokens);
  l.stride = (long)align256(l.hfrm + sizeof(int) * 2 * (size_t)beam * max_tokens);
  if (o_ng) {
    *o_ng = l.stride;
    l.stride = (long)align256(l.stride + (sizeof(int) + sizeof(float)) * (size_t)beam);
  }
  if (o_bias) {
    *o_bias = l.stride;
    l.stride = (long)align256(l.stride + (sizeof(int) + sizeof(float)) * (size_t)beam);
  }
  return l;
}

// B rows of state: behind the four s2t_rnnt_*stream_state_bytes
long state_bytes(int B, int V, int ctx, int beam, int max_tokens, bool ngram, bool bias = false) {
  if (B <= 0 || !row_ok(V, ctx, beam, max_tokens) || ((ngram || bias) && beam < 1)) return 0;
  long o_ng, o_bias;
  return (long)B * layout(V, ctx, beam, max_tokens, ngram ? &o_ng : nullptr, bias ? &o_bias : nullptr).stride;
}

// the whole-utterance beam search's workspace: records [B][T][beam] | lm_spill [B][beam][V]
size_t records_bytes(int B, int T, int beam) { return align256(sizeof(int) * (size_t)B * T * beam); }

// ------------------------------------------------------------------------------------ reset
// o_ng != 0: an n-gram beam row, whose one beam starts in the context start_ctx with no LM sum.  One text for
// both kernels: without a tail the plain / n-gram reset with the arguments it has always had, with o_bias as
// its tail the reset of a hotword row (beam >= 1), whose one beam also starts in the graph's root with bias_sum 0.
template <typename... Tail>
__global__ __launch_bounds__(64) void rnnt_stream_reset_kernel(char* state, const int* __restrict__ rows,
                                                               long stride, long pstate, int beam,
                                                               int ctx, int blank, long o_ng, int start_ctx,
                                                               Tail... o_bias) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (rows && rows[b] == 0) return;
  char* row = state + (long)b * stride;
  int* hdr = reinterpret_cast<int*>(row);
  if (beam == 0) {
    if (tid < 4) hdr[tid] = 0;                             // no tokens, frame 0, live, lm to compute
  } else {
    if (tid < kHdr / 4) hdr[tid] = tid == 0 ? 1 : 0;       // one beam, frame 0, no overflow, lm to compute
    if (tid == 0) {
      reinterpret_cast<float*>(row + kHdr)[0] = 0.f;       // its score, length, lm row
      reinterpret_cast<int*>(row + 2 * kHdr)[0] = 0;
      reinterpret_cast<int*>(row + 3 * kHdr)[0] = 0;
      if (o_ng) {
        reinterpret_cast<int*>(row + o_ng)[0] = start_ctx;
        reinterpret_cast<float*>(row + o_ng)[beam] = 0.f;
      }
      if constexpr (sizeof...(Tail) == 1) {
        const long at = (o_bias, ...);
        reinterpret_cast<int*>(row + at)[0] = 0;
        reinterpret_cast<float*>(row + at)[beam] = 0.f;
      }
    }
  }
  int* ps = reinterpret_cast<int*>(row + pstate);          // init state + the blank start token
  if (tid < ctx) ps[tid] = blank;
}

// All four resets.  ngram: an n-gram row, which is a beam row; its start_ctx is tested from below alone, because a
// reset sees no tables (the chunk kernel clamps what it loads).  bias: a hotword row, which is a beam row too.
int rnnt_reset(void* state, const int* rows, int B, int V, int ctx, int beam, int max_tokens, int blank, bool ngram,
               int start_ctx, void* stream, bool bias = false) {
  if (B <= 0) return 0;
  if (!state || !row_ok(V, ctx, beam, max_tokens) || blank < 0 || blank >= V ||
      (ngram && (beam < 1 || start_ctx < 0)) || (bias && beam < 1))
    return -1;
  long o_ng = 0, o_bias = 0;
  const Layout l = layout(V, ctx, beam, max_tokens, ngram ? &o_ng : nullptr, bias ? &o_bias : nullptr);
  if (bias)
    hipLaunchKernelGGL(rnnt_stream_reset_kernel<long>, dim3(B), dim3(64), 0, (hipStream_t)stream,
                       static_cast<char*>(state), rows, l.stride, l.pstate, beam, ctx, blank, o_ng, start_ctx, o_bias);
  else
    hipLaunchKernelGGL(rnnt_stream_reset_kernel<>, dim3(B), dim3(64), 0, (hipStream_t)stream, static_cast<char*>(state),
                       rows, l.stride, l.pstate, beam, ctx, blank, o_ng, start_ctx);
  S2T_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------ greedy
struct GreedyChunkArgs {
  const float* am;        // [B][Tc][V]
  const long* lengths;    // [B]  chunk_len
  StatelessPointers p;
  int T;                  // Tc
  StatelessDims d;
  int max_token_step, max_out, blank;   // max_out: max_tokens
  char* state;
  long stride, o_pstate, o_lm;
  long* tokens;           // [B][max_tokens]
  long* out_len;          // [B]
  int* overflow;          // [B]
};

__global__ __launch_bounds__(kGreedyThreads) void rnnt_greedy_chunk_kernel(GreedyChunkArgs a) {
  extern __shared__ float sm[];
  const StatelessDims& w = a.d;
  float* e = sm;                       // [E]
  float* hvec = e + w.E;             // [D]
  float* lm = hvec + w.D;            // [V]
  int* state = reinterpret_cast<int*>(lm + w.V);   // [ctx] most recent last
  __shared__ GreedyShared s_walk;
  const int b = blockIdx.x, tid = threadIdx.x;
  char* row = a.state + (long)b * a.stride;
  int* hdr = reinterpret_cast<int*>(row);
  int* g_state = reinterpret_cast<int*>(row + a.o_pstate);
  float* g_lm = reinterpret_cast<float*>(row + a.o_lm);
  const long Tb = clamped_len(a.lengths, b, a.T);
  const int n0 = hdr[0], f0 = hdr[1], inert = hdr[2], lm_valid = hdr[3];
  if (Tb == 0 || inert) return;        // an idle stream, or a full one: state and outputs stay
  for (int k = tid; k < w.ctx; k += kGreedyThreads) state[k] = g_state[k];
  if (lm_valid)
    for (int c = tid; c < w.V; c += kGreedyThreads) lm[c] = g_lm[c];
  __syncthreads();
  // A chunk ends right after a frame advance, where the walk's symbols-on-this-frame counter is 0
  // and its lm is current (decode_search.h greedy_walk): neither is carried.  Only a reset row
  // enters without an lm.
  long n = n0;
  bool need_lm = !lm_valid;
  const bool full = greedy_walk(a.p, a.d, a.max_token_step, a.blank, s_walk, a.am + (long)b * a.T * w.V, Tb, state,
                                e, hvec, lm, need_lm, n, a.tokens + (long)b * a.max_out, a.max_out);
  __syncthreads();
  for (int k = tid; k < w.ctx; k += kGreedyThreads) g_state[k] = state[k];
  for (int c = tid; c < w.V; c += kGreedyThreads) g_lm[c] = lm[c];
  if (tid == 0) {
    hdr[0] = (int)n;
    hdr[1] = f0 + (int)Tb;
    hdr[2] = full ? 1 : 0;
    hdr[3] = 1;
    a.out_len[b] = n < a.max_out ? n : a.max_out;
    a.overflow[b] = full ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------ beam
// One argument type composed from parts, in the order the kernels have always had them: an instantiation
// carries its own modes' fields only.
template <int>
struct NoPart {};

struct BeamHead {
  const float* am;        // [B][T][V]  = enc_proj(encoder_out), bias included; chunk: T is Tc
  const long* lengths;    // [B]        chunk: chunk_len
  StatelessPointers p;
  int T;
  StatelessDims d;
  int blank, beam, topk, lm_in_lds;
};
struct BeamWholePart {
  int* records;           // [B][T][beam]  pack_record(parent, class)
  float* lm_spill;        // [B][beam][V]  (used when lm does not fit the LDS)
};
struct BeamChunkPart {
  int max_tokens;
  char* state;
  Layout l;
};
struct BeamOutputs {
  long* tokens;           // [B][T]     chunk: [B][max_tokens]
  long* frames;           // [B][T]     chunk: [B][max_tokens]
  long* out_len;          // [B]
  float* score;           // [B]
};
struct BeamChunkOutputs {
  long* stable_len;       // [B]
  int* overflow;          // [B]
};
struct BeamNgramWholePart {        // the n-gram mode's (decode_search.h beam_walk)
  NgramTables g;
  float lm_weight;
  int start_ctx;          // the one fresh beam's context
  float* lm_score;        // [B]
};
struct BeamNgramChunkPart {
  NgramTables g;
  float lm_weight;
  long o_ng;              // ctx [beam] int32 | lm_sum [beam] fp32 inside a row of state
  float* lm_score;        // [B]
};

struct BeamBiasPart {              // the hotword mode's (decode_search.h beam_walk), behind every other part
  NgramTables graph;
  const float* ctx_final; // [num_ctx]
  float bias_weight;
  float* bias_score;      // [B]
};
struct BeamBiasChunkPart {
  long o_bias;            // bstate [beam] int32 | bsum [beam] fp32 inside a row of state
};

template <int LM, bool CHUNK, bool BIAS = false>
struct BeamArgs : BeamHead,
                  std::conditional_t<CHUNK, BeamChunkPart, BeamWholePart>,
                  BeamOutputs,
                  std::conditional_t<CHUNK, BeamChunkOutputs, NoPart<0>>,
                  std::conditional_t<LM == kLmNgram, std::conditional_t<CHUNK, BeamNgramChunkPart, BeamNgramWholePart>,
                                     NoPart<1>>,
                  std::conditional_t<BIAS, BeamBiasPart, NoPart<2>>,
                  std::conditional_t<BIAS && CHUNK, BeamBiasChunkPart, NoPart<3>> {};

template <bool CACHE, int LM, bool BIAS = false>
__global__ __launch_bounds__(kThreads) void rnnt_beam_kernel(BeamArgs<LM, false, BIAS> a) {
  extern __shared__ float sm[];
  __shared__ BeamShared s;
  RnntNgramShared* ng = nullptr;
  if constexpr (LM == kLmNgram) {
    __shared__ RnntNgramShared s_ng;
    ng = &s_ng;
  }
  RnntBiasShared* bs = nullptr;
  if constexpr (BIAS) {
    __shared__ RnntBiasShared s_bias;
    bs = &s_bias;
  }

  const int b = blockIdx.x, tid = threadIdx.x;
  const StatelessDims& w = a.d;
  const int V = w.V, BS = a.beam;
  float* e = sm;                                           // [kGroup][E]
  float* h = e + kGroup * w.E;                             // [kGroup][D]
  int* state = reinterpret_cast<int*>(h + kGroup * w.D);   // [2][kMaxBeam][ctx], most recent last
  float* lm = a.lm_in_lds ? reinterpret_cast<float*>(state + 2 * kMaxBeam * w.ctx)
                          : a.lm_spill + (long)b * BS * V;  // [beam][V]
  const int Tb = (int)clamped_len(a.lengths, b, a.T);
  if (Tb == 0) {                                           // no frames: no tokens, score 0, lm_score 0
    if (tid == 0) {
      a.out_len[b] = 0;
      a.score[b] = 0.f;
      if constexpr (LM == kLmNgram) a.lm_score[b] = 0.f;
      if constexpr (BIAS) a.bias_score[b] = 0.f;
    }
    return;
  }
  const float* amb = a.am + (long)b * a.T * V;
  int* rec = a.records + (long)b * a.T * BS;

  // one beam: no tokens, score 0, state = init state + the blank start token, the LM's start context, no LM sum
  for (int k = tid; k < w.ctx; k += kThreads) state[k] = a.blank;
  if (tid == 0) {
    s.score[0][0] = 0.f;
    s.slot[0][0] = 0;
    s.len[0][0] = 0;
    s.emit[0] = 0;
    if constexpr (LM == kLmNgram) {
      ng->g = a.g;
      ng->ctx[0][0] = a.start_ctx;
      ng->lm_sum[0][0] = 0.f;
    }
    if constexpr (BIAS) {                                  // the graph's root, no bias sum
      bs->g = a.graph;
      bs->final = a.ctx_final;
      bs->bstate[0][0] = 0;
      bs->bsum[0][0] = 0.f;
    }
  }
  __syncthreads();
  recompute_lm(a.p, a.d, s.emit, 1, state, s.slot[0], e, h, lm);
  int nb = 1, cur = 0;
  float lm_weight = 0.f;
  if constexpr (LM == kLmNgram) lm_weight = a.lm_weight;
  // phases A-D per frame: shared with the chunk-carried kernel (decode_search.h)
  if constexpr (BIAS)
    beam_walk<CACHE, LM, true>(a.p, a.d, a, s, amb, Tb, nb, cur, e, h, state, lm,
                               [&](int t, int pos, int r) { rec[(long)t * BS + pos] = r; }, ng, lm_weight, bs,
                               a.bias_weight);
  else
    beam_walk<CACHE, LM>(a.p, a.d, a, s, amb, Tb, nb, cur, e, h, state, lm,
                         [&](int t, int pos, int r) { rec[(long)t * BS + pos] = r; }, ng, lm_weight);

  // ---- the best beam is position 0: trace its (parent, class) records back
  if constexpr (BIAS) {            // ... the finalisation's pick with hotwords: outputs only, nothing is stored
    float top;
    const int pos = bias_pick(*bs, s.score[cur], cur, nb, a.bias_weight, &top);
    const int n = s.len[cur][pos];
    if (tid == 0) {
      a.out_len[b] = n;
      a.score[b] = top;
      if constexpr (LM == kLmNgram) a.lm_score[b] = ng->lm_sum[cur][pos];
      a.bias_score[b] = bs->bsum[cur][pos] + bs->final[bs->bstate[cur][pos]];
    }
    trace_best<kThreads>(rec, Tb, BS, a.blank, n, s.trace, &s.nemit, a.tokens + (long)b * a.T,
                         a.frames + (long)b * a.T, pos);
    return;
  }
  const int n = s.len[cur][0];
  if (tid == 0) {
    a.out_len[b] = n;
    a.score[b] = s.score[cur][0];
    if constexpr (LM == kLmNgram) a.lm_score[b] = ng->lm_sum[cur][0];
  }
  trace_best<kThreads>(rec, Tb, BS, a.blank, n, s.trace, &s.nemit, a.tokens + (long)b * a.T,
                       a.frames + (long)b * a.T);
}

// The chunk-carried form: it loads the carried beams where the kernel above starts one, and ends as the file
// header says.  A text of its own: folded into the kernel above behind `if constexpr`, in every order of
// statements tried, its instantiations lost the unrolled copies of lm and two registers.
template <bool CACHE, int LM, bool BIAS = false>
__global__ __launch_bounds__(kThreads) void rnnt_beam_chunk_kernel(BeamArgs<LM, true, BIAS> a) {
  extern __shared__ float sm[];
  __shared__ BeamShared s;
  __shared__ int s_anc[kMaxBeam], s_base[kMaxBeam];
  RnntNgramShared* ng = nullptr;
  if constexpr (LM == kLmNgram) {
    __shared__ RnntNgramShared s_ng;
    ng = &s_ng;
  }
  RnntBiasShared* bs = nullptr;
  if constexpr (BIAS) {
    __shared__ RnntBiasShared s_bias;
    bs = &s_bias;
  }

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.d.V, BS = a.beam, MT = a.max_tokens;
  long Tl = a.lengths[b];
  if (Tl > a.T) Tl = a.T;
  if (Tl <= 0) return;                                     // an idle stream: state and outputs stay
  const int Tb = (int)Tl;
  char* row = a.state + (long)b * a.l.stride;
  int* hdr = reinterpret_cast<int*>(row);
  float* g_score = reinterpret_cast<float*>(row + kHdr);
  int* g_len = reinterpret_cast<int*>(row + 2 * kHdr);
  int* g_slot = reinterpret_cast<int*>(row + 3 * kHdr);
  int* g_state = reinterpret_cast<int*>(row + a.l.pstate);
  float* g_lm = reinterpret_cast<float*>(row + a.l.lm);
  int* rec = reinterpret_cast<int*>(row + a.l.rec);        // [Tc][beam]  pack_record(parent, class)
  int* htok = reinterpret_cast<int*>(row + a.l.htok);      // [2][beam][max_tokens]
  int* hfrm = reinterpret_cast<int*>(row + a.l.hfrm);

  float* e = sm;                                           // [kGroup][E]
  float* h = e + kGroup * a.d.E;                             // [kGroup][D]
  int* state = reinterpret_cast<int*>(h + kGroup * a.d.D);   // [2][kMaxBeam][ctx], most recent last
  float* lm = a.lm_in_lds ? reinterpret_cast<float*>(state + 2 * kMaxBeam * a.d.ctx) : g_lm;

  // ---- the carried beams become buffer 0
  const int nb0 = hdr[0], f0 = hdr[1], ovf0 = hdr[2], lm_valid = hdr[3], hcur = hdr[4];
  if (tid < nb0) {
    s.score[0][tid] = g_score[tid];
    s.len[0][tid] = g_len[tid];
    s.slot[0][tid] = g_slot[tid];
  }
  for (int x = tid; x < nb0 * a.d.ctx; x += kThreads) state[x] = g_state[x];
  if (a.lm_in_lds && lm_valid)
    for (int x = tid; x < BS * V; x += kThreads) lm[x] = g_lm[x];
  if (tid == 0) s.emit[0] = 0;
  if constexpr (LM == kLmNgram) {
    const int* g_ctx = reinterpret_cast<const int*>(row + a.o_ng);
    if (tid < nb0) {                                       // (clamped: the look-up indexes with it)
      ng->ctx[0][tid] = ngram_clamp(g_ctx[tid], a.g.num_ctx);
      ng->lm_sum[0][tid] = reinterpret_cast<const float*>(g_ctx + BS)[tid];
    }
    if (tid == 0) ng->g = a.g;
  }
  if constexpr (BIAS) {
    const int* g_bstate = reinterpret_cast<const int*>(row + a.o_bias);
    if (tid < nb0) {                                       // (clamped: the look-up and ctx_final index with it)
      bs->bstate[0][tid] = ngram_clamp(g_bstate[tid], a.graph.num_ctx);
      bs->bsum[0][tid] = reinterpret_cast<const float*>(g_bstate + BS)[tid];
    }
    if (tid == 0) {
      bs->g = a.graph;
      bs->final = a.ctx_final;
    }
  }
  __syncthreads();
  if (!lm_valid) recompute_lm(a.p, a.d, s.emit, 1, state, s.slot[0], e, h, lm);   // (a reset row: one beam)
  int nb = nb0, cur = 0;
  if constexpr (BIAS) {
    float lm_weight = 0.f;
    if constexpr (LM == kLmNgram) lm_weight = a.lm_weight;
    beam_walk<CACHE, LM, true>(a.p, a.d, a, s, a.am + (long)b * a.T * V, Tb, nb, cur, e, h, state, lm,
                               [&](int t, int pos, int r) { rec[t * BS + pos] = r; }, ng, lm_weight, bs,
                               a.bias_weight);
  } else if constexpr (LM == kLmNgram)
    beam_walk<CACHE, kLmNgram>(a.p, a.d, a, s, a.am + (long)b * a.T * V, Tb, nb, cur, e, h, state, lm,
                               [&](int t, int pos, int r) { rec[t * BS + pos] = r; }, ng, a.lm_weight);
  else
    beam_walk<CACHE>(a.p, a.d, a, s, a.am + (long)b * a.T * V, Tb, nb, cur, e, h, state, lm,
                     [&](int t, int pos, int r) { rec[t * BS + pos] = r; });

  // ---- the beams go back
  if (tid < nb) {
    g_score[tid] = s.score[cur][tid];
    g_len[tid] = s.len[cur][tid];
    g_slot[tid] = s.slot[cur][tid];
    if constexpr (LM == kLmNgram) {
      int* g_ctx = reinterpret_cast<int*>(row + a.o_ng);
      g_ctx[tid] = ng->ctx[cur][tid];
      reinterpret_cast<float*>(g_ctx + BS)[tid] = ng->lm_sum[cur][tid];
    }
    if constexpr (BIAS) {
      int* g_bstate = reinterpret_cast<int*>(row + a.o_bias);
      g_bstate[tid] = bs->bstate[cur][tid];
      reinterpret_cast<float*>(g_bstate + BS)[tid] = bs->bsum[cur][tid];
    }
  }
  for (int x = tid; x < nb * a.d.ctx; x += kThreads) g_state[x] = state[cur * kMaxBeam * a.d.ctx + x];
  if (a.lm_in_lds)
    for (int x = tid; x < BS * V; x += kThreads) g_lm[x] = lm[x];

  // ---- histories: new = ancestor's old + this chunk's emissions (kept up to max_tokens)
  const int* otok = htok + (long)hcur * BS * MT;
  const int* ofrm = hfrm + (long)hcur * BS * MT;
  int* ntok = htok + (long)(hcur ^ 1) * BS * MT;
  int* nfrm = hfrm + (long)(hcur ^ 1) * BS * MT;
  const bool tracer = wave == 0 && lane < nb;              // a lane per surviving beam
  int pos = lane, left = tracer ? s.len[cur][lane] : 0;
  for (int tend = Tb; tend > 0; tend -= kTraceFrames) {
    const int t0 = max(0, tend - kTraceFrames);
    for (int x = tid; x < (tend - t0) * BS; x += kThreads) s.trace[x] = rec[t0 * BS + x];
    __syncthreads();
    if (tracer) {
      for (int t = tend - 1; t >= t0; --t) {
        const int r = s.trace[(t - t0) * BS + pos];
        const int cls = record_class(r);
        pos = record_parent(r);
        if (cls != a.blank) {
          --left;
          if (left < MT) {
            ntok[(long)lane * MT + left] = cls;
            nfrm[(long)lane * MT + left] = f0 + t;
          }
        }
      }
    }
    __syncthreads();
  }
  if (tracer) {
    s_anc[lane] = pos;                                     // position at chunk start
    s_base[lane] = left;                                   // = that beam's length there
  }
  __syncthreads();
  for (int i = wave; i < nb; i += kWaves) {
    const int anc = s_anc[i], m = min(s_base[i], MT);
    for (int p = lane; p < m; p += 64) {
      ntok[(long)i * MT + p] = otok[(long)anc * MT + p];
      nfrm[(long)i * MT + p] = ofrm[(long)anc * MT + p];
    }
  }
  __syncthreads();

  // ---- outputs: the best beam (position 0), and the prefix all live beams share
  const int n0 = s.len[cur][0], m0 = min(n0, MT);
  int rpos = 0, rlen = m0;         // with hotwords the finalisation's pick is reported: outputs only, the
  float rtop = 0.f;                // header, stable_len, overflow and what is carried stay position 0's
  if constexpr (BIAS) {
    rpos = bias_pick(*bs, s.score[cur], cur, nb, a.bias_weight, &rtop);
    rlen = min(s.len[cur][rpos], MT);
    for (int p = tid; p < rlen; p += kThreads) {
      a.tokens[(long)b * MT + p] = ntok[(long)rpos * MT + p];
      a.frames[(long)b * MT + p] = nfrm[(long)rpos * MT + p];
    }
  } else {
    for (int p = tid; p < m0; p += kThreads) {
      a.tokens[(long)b * MT + p] = ntok[p];
      a.frames[(long)b * MT + p] = nfrm[p];
    }
  }
  if (wave == 0) {
    int shortest = m0, longest = n0;
    for (int i = 1; i < nb; ++i) {
      shortest = min(shortest, s.len[cur][i]);
      longest = max(longest, s.len[cur][i]);
    }
    int stable = shortest;                                 // first position where two beams differ
    for (int p = lane; p < shortest; p += 64) {
      const int t0 = ntok[p];
      bool same = true;
      for (int i = 1; i < nb; ++i) same = same && ntok[(long)i * MT + p] == t0;
      if (!same) {
        stable = p;
        break;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) stable = min(stable, __shfl_xor(stable, o, 64));
    if (lane == 0) {
      const int ovf = (ovf0 || longest > MT) ? 1 : 0;
      if constexpr (BIAS) {
        a.out_len[b] = rlen;
        a.score[b] = rtop;
        if constexpr (LM == kLmNgram) a.lm_score[b] = ng->lm_sum[cur][rpos];
        a.bias_score[b] = bs->bsum[cur][rpos] + bs->final[bs->bstate[cur][rpos]];
      } else {
        a.out_len[b] = m0;
        a.score[b] = s.score[cur][0];
        if constexpr (LM == kLmNgram) a.lm_score[b] = ng->lm_sum[cur][0];
      }
      a.stable_len[b] = stable;
      a.overflow[b] = ovf;
      hdr[0] = nb;
      hdr[1] = f0 + Tb;
      hdr[2] = ovf;
      hdr[3] = 1;
      hdr[4] = hcur ^ 1;
      hdr[5] = stable;
    }
  }
}

// One host path for the eight beam entries: an entry fills the arguments it was handed, this states the refusals,
// the LDS rule and the choice of instantiation.  memory: the workspace; chunk: the state.
template <int LM, bool CHUNK, bool BIAS>
int rnnt_beam_search(BeamArgs<LM, CHUNK, BIAS>& a, const StatelessWeights& w, int B, void* memory,
                     const S2tNgramLmDesc* lm, void* stream, const S2tContextGraphDesc* graph = nullptr) {
  if (B <= 0) return 0;
  bool ok = a.T > 0 && dims_ok(w) && w.V <= kMaxV && a.blank >= 0 && a.blank < w.V && a.beam >= 1 &&
            a.beam <= kMaxBeam && a.topk >= 1 && (a.topk < w.V ? a.topk : w.V) <= kMaxBeam &&
            beam_fixed_lds(w.E, w.D, w.ctx) <= kLdsBudget && memory;
  if constexpr (CHUNK) ok = ok && a.T <= kMaxChunk && a.max_tokens > 0;
  if constexpr (LM == kLmNgram) {
    ok = ok && ngram_desc_ok(lm) && lm->V == w.V && __builtin_isfinite(a.lm_weight) && a.lm_score;
    if constexpr (!CHUNK) ok = ok && a.start_ctx >= 0 && a.start_ctx < lm->num_ctx;
  }
  if constexpr (BIAS)
    ok = ok && context_desc_ok(graph) && graph->V == w.V && __builtin_isfinite(a.bias_weight) && a.bias_score;
  if (!ok) return -1;
  a.p = w, a.d = w;
  const size_t fixed = beam_fixed_lds(w.E, w.D, w.ctx), lm_bytes = sizeof(float) * (size_t)a.beam * w.V;
  a.lm_in_lds = fixed + lm_bytes <= kLdsBudget;
  long* o_ng = nullptr;
  if constexpr (LM == kLmNgram) {
    a.g = ngram_tables(*lm);
    if constexpr (CHUNK) o_ng = &a.o_ng;
  }
  long* o_bias = nullptr;
  if constexpr (BIAS) {
    a.graph = context_tables(*graph), a.ctx_final = graph->ctx_final;
    if constexpr (CHUNK) o_bias = &a.o_bias;
  }
  if constexpr (CHUNK) {
    a.state = static_cast<char*>(memory);
    a.l = layout(w.V, w.ctx, a.beam, a.max_tokens, o_ng, o_bias);
  } else {
    a.records = static_cast<int*>(memory);
    a.lm_spill = reinterpret_cast<float*>(static_cast<char*>(memory) + records_bytes(B, a.T, a.beam));
  }
  // CACHE: V <= 64 kRegs, a frame's am is held in registers (decode_search.h beam_walk)
  const size_t smem = fixed + (a.lm_in_lds ? lm_bytes : 0);
  const bool cache = w.V <= 64 * kRegs;
  if constexpr (CHUNK)
    hipLaunchKernelGGL((cache ? rnnt_beam_chunk_kernel<true, LM, BIAS> : rnnt_beam_chunk_kernel<false, LM, BIAS>),
                       dim3(B), dim3(kThreads), smem, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((cache ? rnnt_beam_kernel<true, LM, BIAS> : rnnt_beam_kernel<false, LM, BIAS>), dim3(B),
                       dim3(kThreads), smem, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

// the arguments every beam entry has
template <typename A>
void beam_head(A& a, const float* am, const long* lengths, int T, int blank, int beam, int topk, long* tokens,
               long* frames, long* out_len, float* score) {
  a.am = am, a.lengths = lengths, a.T = T, a.blank = blank, a.beam = beam, a.topk = topk;
  a.tokens = tokens, a.frames = frames, a.out_len = out_len, a.score = score;
}

}  // namespace

// ------------------------------------------------------------------------------------ sizes and resets
extern "C" long s2t_rnnt_beam_workspace_bytes(int B, int T, int V, int beam_size) {
  if (B <= 0 || T <= 0 || V <= 0 || beam_size <= 0) return 0;
  return (long)(records_bytes(B, T, beam_size) + align256(sizeof(float) * (size_t)B * beam_size * V));
}

// (the plain query above has never refused a V or a beam past the search's limits; this one has)
extern "C" long s2t_rnnt_beam_ngram_workspace_bytes(int B, int T, int V, int beam_size) {
  if (V > kMaxV || beam_size > kMaxBeam) return 0;
  return s2t_rnnt_beam_workspace_bytes(B, T, V, beam_size);
}

extern "C" long s2t_rnnt_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens) {
  return state_bytes(B, V, ctx, beam_size, max_tokens, false);
}

extern "C" long s2t_rnnt_ngram_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens) {
  return state_bytes(B, V, ctx, beam_size, max_tokens, true);
}

extern "C" int s2t_rnnt_stream_reset(void* state, const int* rows, int B, int V, int ctx,
                                     int beam_size, int max_tokens, int blank, void* stream) {
  return rnnt_reset(state, rows, B, V, ctx, beam_size, max_tokens, blank, false, 0, stream);
}

extern "C" int s2t_rnnt_ngram_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                                           int max_tokens, int blank, int start_ctx, void* stream) {
  return rnnt_reset(state, rows, B, V, ctx, beam_size, max_tokens, blank, true, start_ctx, stream);
}

extern "C" long s2t_rnnt_bias_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens) {
  return state_bytes(B, V, ctx, beam_size, max_tokens, false, true);
}

extern "C" long s2t_rnnt_ngram_bias_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens) {
  return state_bytes(B, V, ctx, beam_size, max_tokens, true, true);
}

extern "C" int s2t_rnnt_bias_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                                          int max_tokens, int blank, void* stream) {
  return rnnt_reset(state, rows, B, V, ctx, beam_size, max_tokens, blank, false, 0, stream, true);
}

extern "C" int s2t_rnnt_ngram_bias_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                                                int max_tokens, int blank, int start_ctx, void* stream) {
  return rnnt_reset(state, rows, B, V, ctx, beam_size, max_tokens, blank, true, start_ctx, stream, true);
}

// ------------------------------------------------------------------------------------ the searches
// (s2t_rnnt_greedy_stateless in decode.hip tests neither its blank nor V <= 8192; this one does)
extern "C" int s2t_rnnt_greedy_stateless_chunk(const float* am, const long* chunk_len, const float* emb,
                                               const float* conv_w, const float* lin_w,
                                               const float* lin_b, const float* pre_w,
                                               const float* pre_b, int B, int Tc, int V, int E, int D,
                                               int ctx, int act, int max_token_step, int max_tokens,
                                               int blank, void* state, long* tokens, long* out_len,
                                               int* overflow, void* stream) {
  if (B <= 0) return 0;
  const StatelessWeights w = stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act);
  if (Tc > kMaxChunk || blank < 0 || blank >= V || V > kMaxV || !state || !greedy_ok(Tc, w, max_tokens)) return -1;
  const Layout l = layout(V, ctx, 0, max_tokens);
  GreedyChunkArgs a{am, chunk_len, w, Tc, w, max_token_step, max_tokens, blank, static_cast<char*>(state),
                    l.stride, l.pstate, l.lm, tokens, out_len, overflow};
  hipLaunchKernelGGL(rnnt_greedy_chunk_kernel, dim3(B), dim3(kGreedyThreads), greedy_lds(w), (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

extern "C" int s2t_rnnt_beam_stateless(const float* am, const long* lengths, const float* emb,
                                       const float* conv_w, const float* lin_w, const float* lin_b,
                                       const float* pre_w, const float* pre_b, int B, int T, int V,
                                       int E, int D, int ctx, int act, int blank, int beam_size,
                                       int cutoff_top_k, void* workspace, long* tokens, long* frames,
                                       long* out_len, float* score, void* stream) {
  BeamArgs<kLmNone, false> a{};
  beam_head(a, am, lengths, T, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          workspace, nullptr, stream);
}

extern "C" int s2t_rnnt_beam_stateless_ngram(const S2tNgramLmDesc* lm, const float* am, const long* lengths,
                                             const float* emb, const float* conv_w, const float* lin_w,
                                             const float* lin_b, const float* pre_w, const float* pre_b, int B,
                                             int T, int V, int E, int D, int ctx, int act, int blank,
                                             int beam_size, int cutoff_top_k, float lm_weight, int start_ctx,
                                             void* workspace, long* tokens, long* frames, long* out_len,
                                             float* score, float* lm_score, void* stream) {
  BeamArgs<kLmNgram, false> a{};
  beam_head(a, am, lengths, T, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  a.lm_weight = lm_weight, a.start_ctx = start_ctx, a.lm_score = lm_score;
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          workspace, lm, stream);
}

extern "C" int s2t_rnnt_beam_stateless_chunk(const float* am, const long* chunk_len, const float* emb,
                                             const float* conv_w, const float* lin_w,
                                             const float* lin_b, const float* pre_w, const float* pre_b,
                                             int B, int Tc, int V, int E, int D, int ctx, int act,
                                             int blank, int beam_size, int cutoff_top_k, int max_tokens,
                                             void* state, long* tokens, long* frames, long* out_len,
                                             float* score, long* stable_len, int* overflow,
                                             void* stream) {
  BeamArgs<kLmNone, true> a{};
  beam_head(a, am, chunk_len, Tc, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  a.max_tokens = max_tokens, a.stable_len = stable_len, a.overflow = overflow;
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          state, nullptr, stream);
}

extern "C" int s2t_rnnt_beam_stateless_ngram_chunk(const S2tNgramLmDesc* lm, const float* am, const long* chunk_len,
                                                   const float* emb, const float* conv_w, const float* lin_w,
                                                   const float* lin_b, const float* pre_w, const float* pre_b,
                                                   int B, int Tc, int V, int E, int D, int ctx, int act, int blank,
                                                   int beam_size, int cutoff_top_k, float lm_weight,
                                                   int max_tokens, void* state, long* tokens, long* frames,
                                                   long* out_len, float* score, float* lm_score, long* stable_len,
                                                   int* overflow, void* stream) {
  BeamArgs<kLmNgram, true> a{};
  beam_head(a, am, chunk_len, Tc, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  a.max_tokens = max_tokens, a.stable_len = stable_len, a.overflow = overflow;
  a.lm_weight = lm_weight, a.lm_score = lm_score;
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          state, lm, stream);
}

// ------------------------------------------------------------------------------------ with hotwords
extern "C" int s2t_rnnt_beam_stateless_bias(const S2tContextGraphDesc* graph, const float* am, const long* lengths,
                                            const float* emb, const float* conv_w, const float* lin_w,
                                            const float* lin_b, const float* pre_w, const float* pre_b, int B, int T,
                                            int V, int E, int D, int ctx, int act, int blank, int beam_size,
                                            int cutoff_top_k, float bias_weight, void* workspace, long* tokens,
                                            long* frames, long* out_len, float* score, float* bias_score,
                                            void* stream) {
  BeamArgs<kLmNone, false, true> a{};
  beam_head(a, am, lengths, T, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  a.bias_weight = bias_weight, a.bias_score = bias_score;
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          workspace, nullptr, stream, graph);
}

extern "C" int s2t_rnnt_beam_stateless_ngram_bias(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                                  const float* am, const long* lengths, const float* emb,
                                                  const float* conv_w, const float* lin_w, const float* lin_b,
                                                  const float* pre_w, const float* pre_b, int B, int T, int V, int E,
                                                  int D, int ctx, int act, int blank, int beam_size, int cutoff_top_k,
                                                  float lm_weight, int start_ctx, float bias_weight, void* workspace,
                                                  long* tokens, long* frames, long* out_len, float* score,
                                                  float* lm_score, float* bias_score, void* stream) {
  BeamArgs<kLmNgram, false, true> a{};
  beam_head(a, am, lengths, T, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  a.lm_weight = lm_weight, a.start_ctx = start_ctx, a.lm_score = lm_score;
  a.bias_weight = bias_weight, a.bias_score = bias_score;
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          workspace, lm, stream, graph);
}

extern "C" int s2t_rnnt_beam_stateless_bias_chunk(const S2tContextGraphDesc* graph, const float* am,
                                                  const long* chunk_len, const float* emb, const float* conv_w,
                                                  const float* lin_w, const float* lin_b, const float* pre_w,
                                                  const float* pre_b, int B, int Tc, int V, int E, int D, int ctx,
                                                  int act, int blank, int beam_size, int cutoff_top_k,
                                                  float bias_weight, int max_tokens, void* state, long* tokens,
                                                  long* frames, long* out_len, float* score, float* bias_score,
                                                  long* stable_len, int* overflow, void* stream) {
  BeamArgs<kLmNone, true, true> a{};
  beam_head(a, am, chunk_len, Tc, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  a.max_tokens = max_tokens, a.stable_len = stable_len, a.overflow = overflow;
  a.bias_weight = bias_weight, a.bias_score = bias_score;
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          state, nullptr, stream, graph);
}

extern "C" int s2t_rnnt_beam_stateless_ngram_bias_chunk(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                                        const float* am, const long* chunk_len, const float* emb,
                                                        const float* conv_w, const float* lin_w, const float* lin_b,
                                                        const float* pre_w, const float* pre_b, int B, int Tc, int V,
                                                        int E, int D, int ctx, int act, int blank, int beam_size,
                                                        int cutoff_top_k, float lm_weight, float bias_weight,
                                                        int max_tokens, void* state, long* tokens, long* frames,
                                                        long* out_len, float* score, float* lm_score,
                                                        float* bias_score, long* stable_len, int* overflow,
                                                        void* stream) {
  BeamArgs<kLmNgram, true, true> a{};
  beam_head(a, am, chunk_len, Tc, blank, beam_size, cutoff_top_k, tokens, frames, out_len, score);
  a.max_tokens = max_tokens, a.stable_len = stable_len, a.overflow = overflow;
  a.lm_weight = lm_weight, a.lm_score = lm_score;
  a.bias_weight = bias_weight, a.bias_score = bias_score;
  return rnnt_beam_search(a, stateless_weights(emb, conv_w, lin_w, lin_b, pre_w, pre_b, V, E, D, ctx, act), B,
                          state, lm, stream, graph);
}
