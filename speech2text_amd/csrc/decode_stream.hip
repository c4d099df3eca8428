// Chunk-carried (streaming) RNN-T search for the stateless predictor and a joiner without output
// projection, for gfx950: s2t_rnnt_greedy_stateless and s2t_rnnt_beam_stateless fed their frames in
// pieces.  The walks are the device functions of decode_search.h that the whole-utterance kernels
// instantiate too, so for any cut of [0, L) into chunks the result is the whole-utterance kernel's
// on the concatenated am, bit for bit; what is new here is only what is carried between calls.
//
// One caller-owned device buffer holds a row of state per stream (s2t_rnnt_stream_state_bytes):
//   greedy  hdr {tokens so far, frames so far, inert, lm valid} | predictor state [ctx] | lm [V]
//   beam    hdr {beams, frames so far, overflow, lm valid, history buffer in use, stable_len}
//           | score [16] | len [16] | lm row of each beam [16] | predictor states [16][ctx]
//           | lm [beam][V] | records [256][beam] | token histories [2][beam][max_tokens]
//           | frame histories [2][beam][max_tokens]
//   n-gram  the beam row, every offset unchanged | ctx [beam] int32 | lm_sum [beam] fp32
//           (s2t_rnnt_ngram_stream_state_bytes; the beam kernel's kLmNgram instantiation)
// The lm rows are PERSISTED, not recomputed on entry: a chunk then starts with beam V floats from
// HBM instead of up to four passes over the predictor's weights (decode_search.h recompute_lm), and
// when the rows do not fit the LDS the search simply works on them in place.  Only a reset row has
// no lm yet (reset takes no weights): its first chunk computes it, as the whole-utterance kernels do.
//
// The beam kernel keeps (parent, class) records for the frames of THIS chunk only (hence Tc <= 256:
// they have a fixed home in the state row).  At chunk end a lane per surviving beam walks them back
// to the beam's ancestor position at chunk start, writing the chunk's emissions to the tail of the
// beam's new history on the way; a wave per beam then copies the ancestor's history in front of
// them.  The two history buffers swap roles per chunk, so a history is never copied onto itself.
// This is the text of decode_records.h chunk_histories (the LSTM chunk end calls that), kept written
// out here, with the chunk length clamped by hand: through the shared function, in every form tried,
// the chunk search measured 1.6-2.4 % slower (profiles/decode_records_resources.txt).
#include "common.h"
#include "decode_search.h"

namespace {

using namespace s2t_dec;

constexpr int kHdr = 64;           // bytes of a row's header, and of each [16] array after it

struct Layout {                    // byte offsets inside a row of state
  long pstate, lm, rec, htok, hfrm, stride;
};

bool shape_ok(int V, int ctx, int beam, int max_tokens) {
  return V > 0 && V <= 8192 && ctx >= 1 && ctx <= 64 && beam >= 0 && beam <= kMaxBeam && max_tokens > 0;
}

Layout layout(int V, int ctx, int beam, int max_tokens) {
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
  return l;
}

// The n-gram beam row (s2t_rnnt_ngram_stream_state_bytes) is the plain beam row, every offset as above,
// followed by ctx [beam] int32, the beams' n-gram context ids, and lm_sum [beam] fp32.
Layout ngram_layout(int V, int ctx, int beam, int max_tokens, long* o_ng) {
  Layout l = layout(V, ctx, beam, max_tokens);
  *o_ng = l.stride;
  l.stride = (long)align256(l.stride + (sizeof(int) + sizeof(float)) * (size_t)beam);
  return l;
}

// ------------------------------------------------------------------------------------ reset
// o_ng != 0: an n-gram beam row, whose one beam starts in the context start_ctx with no LM sum
__global__ __launch_bounds__(64) void rnnt_stream_reset_kernel(char* state, const int* __restrict__ rows,
                                                               long stride, long pstate, int beam,
                                                               int ctx, int blank, long o_ng, int start_ctx) {
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
    }
  }
  int* ps = reinterpret_cast<int*>(row + pstate);          // init state + the blank start token
  if (tid < ctx) ps[tid] = blank;
}

// ------------------------------------------------------------------------------------ greedy
struct GreedyChunkArgs {
  const float* am;        // [B][Tc][V]
  const long* chunk_len;  // [B]
  const float* emb;
  const float* conv_w;
  const float* lin_w;
  const float* lin_b;
  const float* pre_w;
  const float* pre_b;
  int Tc, V, E, D, ctx, act, max_token_step, max_tokens, blank;
  char* state;
  long stride, o_pstate, o_lm;
  long* tokens;           // [B][max_tokens]
  long* out_len;          // [B]
  int* overflow;          // [B]
};

__global__ __launch_bounds__(kGreedyThreads) void rnnt_greedy_chunk_kernel(GreedyChunkArgs a) {
  extern __shared__ float sm[];
  float* e = sm;                       // [E]
  float* hvec = e + a.E;               // [D]
  float* lm = hvec + a.D;              // [V]
  int* state = reinterpret_cast<int*>(lm + a.V);   // [ctx] most recent last
  __shared__ GreedyShared s_walk;
  const int b = blockIdx.x, tid = threadIdx.x;
  char* row = a.state + (long)b * a.stride;
  int* hdr = reinterpret_cast<int*>(row);
  int* g_state = reinterpret_cast<int*>(row + a.o_pstate);
  float* g_lm = reinterpret_cast<float*>(row + a.o_lm);
  const long Tb = clamped_len(a.chunk_len, b, a.Tc);
  const int n0 = hdr[0], f0 = hdr[1], inert = hdr[2], lm_valid = hdr[3];
  if (Tb == 0 || inert) return;        // an idle stream, or a full one: state and outputs stay
  for (int k = tid; k < a.ctx; k += kGreedyThreads) state[k] = g_state[k];
  if (lm_valid)
    for (int c = tid; c < a.V; c += kGreedyThreads) lm[c] = g_lm[c];
  __syncthreads();
  // A chunk ends right after a frame advance, where the walk's symbols-on-this-frame counter is 0
  // and its lm is current (decode_search.h greedy_walk): neither is carried.  Only a reset row
  // enters without an lm.
  long n = n0;
  bool need_lm = !lm_valid;
  const bool full = greedy_walk(a, s_walk, a.am + (long)b * a.Tc * a.V, Tb, state, e, hvec, lm, need_lm,
                                n, a.tokens + (long)b * a.max_tokens, a.max_tokens);
  __syncthreads();
  for (int k = tid; k < a.ctx; k += kGreedyThreads) g_state[k] = state[k];
  for (int c = tid; c < a.V; c += kGreedyThreads) g_lm[c] = lm[c];
  if (tid == 0) {
    hdr[0] = (int)n;
    hdr[1] = f0 + (int)Tb;
    hdr[2] = full ? 1 : 0;
    hdr[3] = 1;
    a.out_len[b] = n < a.max_tokens ? n : a.max_tokens;
    a.overflow[b] = full ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------ beam
struct BeamChunkArgs {
  const float* am;        // [B][Tc][V]
  const long* chunk_len;  // [B]
  const float* emb;
  const float* conv_w;
  const float* lin_w;
  const float* lin_b;
  const float* pre_w;
  const float* pre_b;
  int Tc, V, E, D, ctx, act, blank, beam, topk, lm_in_lds, max_tokens;
  char* state;
  Layout l;
  long* tokens;           // [B][max_tokens]
  long* frames;           // [B][max_tokens]
  long* out_len;          // [B]
  float* score;           // [B]
  long* stable_len;       // [B]
  int* overflow;          // [B]
};

struct BeamNgramChunkArgs : BeamChunkArgs {    // the n-gram mode's (decode_search.h beam_walk)
  NgramTables g;
  float lm_weight;
  long o_ng;              // ctx [beam] int32 | lm_sum [beam] fp32 inside a row of state
  float* lm_score;        // [B]
};

template <bool CACHE, int LM = kLmNone, typename Args = BeamChunkArgs>
__global__ __launch_bounds__(kThreads) void rnnt_beam_chunk_kernel(Args a) {
  extern __shared__ float sm[];
  __shared__ BeamShared s;
  __shared__ int s_anc[kMaxBeam], s_base[kMaxBeam];
  RnntNgramShared* ng = nullptr;
  if constexpr (LM == kLmNgram) {
    __shared__ RnntNgramShared s_ng;
    ng = &s_ng;
  }

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V, BS = a.beam, MT = a.max_tokens;
  long Tl = a.chunk_len[b];
  if (Tl > a.Tc) Tl = a.Tc;
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
  float* h = e + kGroup * a.E;                             // [kGroup][D]
  int* state = reinterpret_cast<int*>(h + kGroup * a.D);   // [2][kMaxBeam][ctx], most recent last
  float* lm = a.lm_in_lds ? reinterpret_cast<float*>(state + 2 * kMaxBeam * a.ctx) : g_lm;

  // ---- the carried beams become buffer 0
  const int nb0 = hdr[0], f0 = hdr[1], ovf0 = hdr[2], lm_valid = hdr[3], hcur = hdr[4];
  if (tid < nb0) {
    s.score[0][tid] = g_score[tid];
    s.len[0][tid] = g_len[tid];
    s.slot[0][tid] = g_slot[tid];
  }
  for (int x = tid; x < nb0 * a.ctx; x += kThreads) state[x] = g_state[x];
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
  __syncthreads();
  if (!lm_valid) recompute_lm(a, s.emit, 1, state, s.slot[0], e, h, lm);   // (a reset row: one beam)
  int nb = nb0, cur = 0;
  if constexpr (LM == kLmNgram)
    beam_walk<CACHE, kLmNgram>(a, s, a.am + (long)b * a.Tc * V, Tb, nb, cur, e, h, state, lm,
                               [&](int t, int pos, int r) { rec[t * BS + pos] = r; }, ng, a.lm_weight);
  else
    beam_walk<CACHE>(a, s, a.am + (long)b * a.Tc * V, Tb, nb, cur, e, h, state, lm,
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
  }
  for (int x = tid; x < nb * a.ctx; x += kThreads) g_state[x] = state[cur * kMaxBeam * a.ctx + x];
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
  for (int p = tid; p < m0; p += kThreads) {
    a.tokens[(long)b * MT + p] = ntok[p];
    a.frames[(long)b * MT + p] = nfrm[p];
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
      a.out_len[b] = m0;
      a.score[b] = s.score[cur][0];
      if constexpr (LM == kLmNgram) a.lm_score[b] = ng->lm_sum[cur][0];
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

}  // namespace

extern "C" long s2t_rnnt_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens) {
  if (B <= 0 || !shape_ok(V, ctx, beam_size, max_tokens)) return 0;
  return (long)B * layout(V, ctx, beam_size, max_tokens).stride;
}

extern "C" int s2t_rnnt_stream_reset(void* state, const int* rows, int B, int V, int ctx,
                                     int beam_size, int max_tokens, int blank, void* stream) {
  if (B <= 0) return 0;
  if (!state || !shape_ok(V, ctx, beam_size, max_tokens) || blank < 0 || blank >= V) return -1;
  const Layout l = layout(V, ctx, beam_size, max_tokens);
  hipLaunchKernelGGL(rnnt_stream_reset_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream,
                     static_cast<char*>(state), rows, l.stride, l.pstate, beam_size, ctx, blank, 0L, 0);
  S2T_CHECK_LAUNCH();
  return 0;
}

extern "C" int s2t_rnnt_greedy_stateless_chunk(const float* am, const long* chunk_len, const float* emb,
                                               const float* conv_w, const float* lin_w,
                                               const float* lin_b, const float* pre_w,
                                               const float* pre_b, int B, int Tc, int V, int E, int D,
                                               int ctx, int act, int max_token_step, int max_tokens,
                                               int blank, void* state, long* tokens, long* out_len,
                                               int* overflow, void* stream) {
  if (B <= 0) return 0;
  if (Tc <= 0 || Tc > kMaxChunk || E <= 0 || D <= 0 || act < 0 || act > 1 || blank < 0 ||
      !shape_ok(V, ctx, 0, max_tokens) || blank >= V || !state)
    return -1;
  const size_t smem = sizeof(float) * ((size_t)E + D + V) + sizeof(int) * ctx;
  if (smem > 60 * 1024) return -1;
  const Layout l = layout(V, ctx, 0, max_tokens);
  GreedyChunkArgs a{am, chunk_len, emb, conv_w, lin_w, lin_b, pre_w, pre_b, Tc, V, E, D, ctx, act,
                    max_token_step, max_tokens, blank, static_cast<char*>(state), l.stride, l.pstate,
                    l.lm, tokens, out_len, overflow};
  hipLaunchKernelGGL(rnnt_greedy_chunk_kernel, dim3(B), dim3(kGreedyThreads), smem, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

extern "C" int s2t_rnnt_beam_stateless_chunk(const float* am, const long* chunk_len, const float* emb,
                                             const float* conv_w, const float* lin_w,
                                             const float* lin_b, const float* pre_w, const float* pre_b,
                                             int B, int Tc, int V, int E, int D, int ctx, int act,
                                             int blank, int beam_size, int cutoff_top_k, int max_tokens,
                                             void* state, long* tokens, long* frames, long* out_len,
                                             float* score, long* stable_len, int* overflow,
                                             void* stream) {
  if (B <= 0) return 0;
  if (Tc <= 0 || Tc > kMaxChunk || E <= 0 || D <= 0 || act < 0 || act > 1 || blank < 0 ||
      beam_size < 1 || !shape_ok(V, ctx, beam_size, max_tokens) || blank >= V || cutoff_top_k < 1 ||
      (cutoff_top_k < V ? cutoff_top_k : V) > kMaxBeam || !state)
    return -1;
  const size_t fixed = beam_fixed_lds(E, D, ctx);
  if (fixed > kLdsBudget) return -1;
  const size_t lm_bytes = sizeof(float) * (size_t)beam_size * V;
  const int lm_in_lds = fixed + lm_bytes <= kLdsBudget;
  BeamChunkArgs a{am, chunk_len, emb, conv_w, lin_w, lin_b, pre_w, pre_b, Tc, V, E, D, ctx, act, blank,
                  beam_size, cutoff_top_k, lm_in_lds, max_tokens, static_cast<char*>(state),
                  layout(V, ctx, beam_size, max_tokens), tokens, frames, out_len, score, stable_len,
                  overflow};
  const size_t smem = fixed + (lm_in_lds ? lm_bytes : 0);
  if (V <= 64 * kRegs)
    hipLaunchKernelGGL(rnnt_beam_chunk_kernel<true>, dim3(B), dim3(kThreads), smem, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(rnnt_beam_chunk_kernel<false>, dim3(B), dim3(kThreads), smem, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

// ---- the beam search above fused with a back-off n-gram (decode_search.h beam_walk's n-gram mode)
extern "C" long s2t_rnnt_ngram_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens) {
  if (B <= 0 || beam_size < 1 || !shape_ok(V, ctx, beam_size, max_tokens)) return 0;
  long o_ng;
  return (long)B * ngram_layout(V, ctx, beam_size, max_tokens, &o_ng).stride;
}

extern "C" int s2t_rnnt_ngram_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                                           int max_tokens, int blank, int start_ctx, void* stream) {
  if (B <= 0) return 0;
  if (!state || beam_size < 1 || !shape_ok(V, ctx, beam_size, max_tokens) || blank < 0 || blank >= V || start_ctx < 0)
    return -1;
  long o_ng;
  const Layout l = ngram_layout(V, ctx, beam_size, max_tokens, &o_ng);
  hipLaunchKernelGGL(rnnt_stream_reset_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream,
                     static_cast<char*>(state), rows, l.stride, l.pstate, beam_size, ctx, blank, o_ng, start_ctx);
  S2T_CHECK_LAUNCH();
  return 0;
}

extern "C" int s2t_rnnt_beam_stateless_ngram_chunk(const S2tNgramLmDesc* lm, const float* am, const long* chunk_len,
                                                   const float* emb, const float* conv_w, const float* lin_w,
                                                   const float* lin_b, const float* pre_w, const float* pre_b,
                                                   int B, int Tc, int V, int E, int D, int ctx, int act, int blank,
                                                   int beam_size, int cutoff_top_k, float lm_weight,
                                                   int max_tokens, void* state, long* tokens, long* frames,
                                                   long* out_len, float* score, float* lm_score, long* stable_len,
                                                   int* overflow, void* stream) {
  if (B <= 0) return 0;
  if (Tc <= 0 || Tc > kMaxChunk || E <= 0 || D <= 0 || act < 0 || act > 1 || blank < 0 ||
      beam_size < 1 || !shape_ok(V, ctx, beam_size, max_tokens) || blank >= V || cutoff_top_k < 1 ||
      (cutoff_top_k < V ? cutoff_top_k : V) > kMaxBeam || !state || !ngram_desc_ok(lm) || lm->V != V ||
      !__builtin_isfinite(lm_weight) || !lm_score)
    return -1;
  const size_t fixed = beam_fixed_lds(E, D, ctx);
  if (fixed > kLdsBudget) return -1;
  const size_t lm_bytes = sizeof(float) * (size_t)beam_size * V;
  const int lm_in_lds = fixed + lm_bytes <= kLdsBudget;
  long o_ng;
  const Layout l = ngram_layout(V, ctx, beam_size, max_tokens, &o_ng);
  BeamNgramChunkArgs a{{am, chunk_len, emb, conv_w, lin_w, lin_b, pre_w, pre_b, Tc, V, E, D, ctx, act, blank,
                        beam_size, cutoff_top_k, lm_in_lds, max_tokens, static_cast<char*>(state), l, tokens,
                        frames, out_len, score, stable_len, overflow},
                       ngram_tables(*lm), lm_weight, o_ng, lm_score};
  const size_t smem = fixed + (lm_in_lds ? lm_bytes : 0);
  if (V <= 64 * kRegs)
    hipLaunchKernelGGL((rnnt_beam_chunk_kernel<true, kLmNgram, BeamNgramChunkArgs>), dim3(B), dim3(kThreads), smem,
                       (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((rnnt_beam_chunk_kernel<false, kLmNgram, BeamNgramChunkArgs>), dim3(B), dim3(kThreads), smem,
                       (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}
