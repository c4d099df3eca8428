// The walks of the two stateless-predictor RNN-T searches as device functions, so that the
// whole-utterance kernels (csrc/decode.hip, csrc/decode_rnnt.hip) and the chunk-carried kernels
// (csrc/decode_rnnt.hip) instantiate ONE body each: a
// search fed its frames in pieces then makes the arithmetic of the search fed them at once, in the
// same order, and gives the same bits.
//   greedy_walk  the lattice walk of s2t_rnnt_greedy_stateless over frames [0, Tb) of one row
//                (256 threads): lm recompute after an emission, arg-max, emit or advance.
//   beam_walk    phases A-D of s2t_rnnt_beam_stateless (see decode_rnnt.hip) over frames [0, Tb) of
//                one row (8 waves); the (parent, class) record of every kept beam goes to a functor.
//                Its LM mode kLmNgram adds the back-off n-gram term of ngram_lookup.h to the candidates
//                (s2t_rnnt_beam_stateless_ngram and its chunk form); kLmNone is the search as it was.
//                Its switch BIAS adds the hotword graph's term behind that, in either LM mode
//                (s2t_rnnt_beam_stateless_bias, s2t_rnnt_beam_stateless_ngram_bias and their chunk forms).
// Both take the search state by reference and leave it as the next frame needs it, and read the
// predictor from the two parts of StatelessWeights, the one place that names its fields.  The limits, the record and
// candidate ranking are decode_records.h's.
#pragma once
#include "common.h"
#include "decode_common.h"
#include "decode_records.h"
#include "ngram_lookup.h"

namespace s2t_dec {

// The stateless predictor and the joiner's activation: the one place that names these fields.  In two parts,
// because the kernels' argument blocks have always kept them apart (a search's T sits between the pointers and
// the dimensions, and moving it moves the compiler's scalar loads and, at these kernels' register limits, their
// schedule); the walks read both parts where they lie, the host holds them as one.
struct StatelessPointers {
  const float* emb;                // [num_symbols][E]
  const float* conv_w;             // [E][ctx]   depthwise, no bias
  const float* lin_w;              // [D][E]
  const float* lin_b;              // [D]
  const float* pre_w;              // [V][D]
  const float* pre_b;              // [V]
};
struct StatelessDims {
  int V, E, D, ctx, act;
};
struct StatelessWeights : StatelessPointers, StatelessDims {};

// the predictor's arguments every search entry has, in the order of its prototype
inline StatelessWeights stateless_weights(const float* emb, const float* conv_w, const float* lin_w,
                                          const float* lin_b, const float* pre_w, const float* pre_b, int V, int E,
                                          int D, int ctx, int act) {
  StatelessWeights w;
  w.emb = emb, w.conv_w = conv_w, w.lin_w = lin_w, w.lin_b = lin_b, w.pre_w = pre_w, w.pre_b = pre_b;
  w.V = V, w.E = E, w.D = D, w.ctx = ctx, w.act = act;
  return w;
}

inline bool dims_ok(const StatelessDims& d) {              // (V's upper limit is the caller's)
  return d.V > 0 && d.E > 0 && d.D > 0 && d.ctx >= 1 && d.ctx <= 64 && d.act >= 0 && d.act <= 1;
}

// ------------------------------------------------------------------------------------ greedy
constexpr int kGreedyThreads = 256;

// LDS of a greedy workgroup: e [E], h [D], lm [V], state [ctx]
inline size_t greedy_lds(const StatelessDims& d) {
  return sizeof(float) * ((size_t)d.E + d.D + d.V) + sizeof(int) * d.ctx;
}

// what both greedy entries refuse of their shape (the chunk entry refuses more: decode_rnnt.hip)
inline bool greedy_ok(int T, const StatelessDims& d, int max_out) {
  return T > 0 && dims_ok(d) && max_out > 0 && greedy_lds(d) <= 60 * 1024;
}

// y[r] = w[r] . x + b[r], one wave per row, x in LDS
__device__ __forceinline__ void gemv_rows(const float* __restrict__ w, const float* __restrict__ bias,
                                          const float* __restrict__ x, int rows, int cols,
                                          float* __restrict__ y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < rows; r += 4) {
    const float* wr = w + (long)r * cols;
    float acc = 0.f;
    for (int c = lane; c < cols; c += 64) acc = fmaf(wr[c], x[c], acc);
    acc = wave_sum(acc);
    if (lane == 0) y[r] = acc + (bias ? bias[r] : 0.f);
  }
}

struct GreedyShared {
  Top red[4];
  int tok;
};

// Frames [0, Tb) of amb [Tb][V] from (state, lm, need_lm, n); tokens_row holds max_out tokens.
// Returns true when the output filled up and the walk stopped inside a frame (the
// whole-utterance kernel ends there; a stream is inert from there on).  Every frame advance
// leaves need_lm false and the symbols-on-this-frame counter at 0, so neither is part of what a
// chunk hands to the next: a walk that starts at a frame boundary starts them as this does.
__device__ __forceinline__ bool greedy_walk(const StatelessPointers& p, const StatelessDims& d, int max_token_step, int blank,
                                            GreedyShared& s, const float* __restrict__ amb, long Tb,
                                            int* state, float* e, float* hvec, float* lm, bool& need_lm,
                                            long& n, long* __restrict__ tokens_row, int max_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int t = 0, nts = 0;
  while (t < Tb) {
    if (need_lm) {
      for (int c = tid; c < d.E; c += kGreedyThreads) {
        float acc = 0.f;
        for (int k = 0; k < d.ctx; ++k) acc = fmaf(p.conv_w[c * d.ctx + k], p.emb[(long)state[k] * d.E + c], acc);
        e[c] = acc;
      }
      __syncthreads();
      gemv_rows(p.lin_w, p.lin_b, e, d.D, d.E, hvec);
      __syncthreads();
      gemv_rows(p.pre_w, p.pre_b, hvec, d.V, d.D, lm);
      __syncthreads();
      need_lm = false;
    }
    Top best{S2T_NEG_INF, d.V};
    for (int c = tid; c < d.V; c += kGreedyThreads) {
      float v = amb[(long)t * d.V + c] + lm[c];
      v = d.act == 0 ? fmaxf(v, 0.f) : tanhf(v);
      best = better(best, Top{v, c});
    }
    best = wave_top(best);
    if (lane == 0) s.red[wave] = best;
    __syncthreads();
    if (tid == 0) s.tok = better(better(s.red[0], s.red[1]), better(s.red[2], s.red[3])).i;
    __syncthreads();
    const int tok = s.tok;
    if (tok == blank || nts > max_token_step) {
      ++t;
      nts = 0;
    } else {
      ++nts;
      if (tid == 0 && n < max_out) tokens_row[n] = tok;
      ++n;
      __syncthreads();
      if (tid == 0) {
        for (int k = 0; k + 1 < d.ctx; ++k) state[k] = state[k + 1];
        state[d.ctx - 1] = tok;
      }
      need_lm = true;
      if (n >= max_out) return true;                 // output buffer full (uniform exit)
    }
    __syncthreads();
  }
  return false;
}

// ------------------------------------------------------------------------------------ beam
constexpr int kGroup = 4;          // beams per pass over the predictor weights
constexpr int kRows = 4;           // weight rows in flight per wave in that pass ...
constexpr int kCols = 4;           // ... and 64-column steps of each row loaded before they are used
constexpr int kWaves = 8;          // waves per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kRegs = 8;           // classes per lane held in registers (V <= 512)
constexpr size_t kLdsBudget = 60 * 1024;

struct BeamShared {
  float cscore[kMaxCand];          // candidates of this frame: score, class
  int ccls[kMaxCand];
  int pick[kMaxBeam];              // candidate index of each new beam
  float score[2][kMaxBeam];        // beams, double-buffered over frames
  int slot[2][kMaxBeam];           // lm row of each beam
  int len[2][kMaxBeam];            // tokens emitted so far
  int emit[kMaxBeam];              // beams whose lm is to be recomputed
  int nemit;
  int trace[kTraceFrames * kMaxBeam];
};

constexpr int kLmNone = 0, kLmNgram = 1;   // the LM modes of beam_walk

struct RnntNgramShared {           // the n-gram mode's part of the beams and of the candidates
  NgramTables g;                   // (in LDS, as in CtcNgramShared: ten scalar registers less across the frame)
  int ctx[2][kMaxBeam];            // context id of each beam, double-buffered like score
  float lm_sum[2][kMaxBeam];       // unweighted sum of the look-ups a beam was extended by
  int cnext[kMaxCand];             // per candidate: the context its look-up returned (blank: the parent's)
  float cq[kMaxCand];              // ... and the look-up's value (blank: 0)
};

struct RnntBiasShared {            // the hotword mode's part of the beams and of the candidates
  NgramTables g;                   // the graph in the n-gram's table form (ngram_lookup.h context_tables)
  const float* final;              // ctx_final [num_ctx]
  int bstate[2][kMaxBeam];         // graph state of each beam, double-buffered like score
  float bsum[2][kMaxBeam];         // unweighted sum of the look-ups a beam was extended by (bias_sum)
  int cnext[kMaxCand];             // per candidate: the state its look-up returned (blank: the parent's)
  float cd[kMaxCand];              // ... and the look-up's value (blank: 0)
};

// The bias term of candidate q of the beam at `parent`, by the thread that ran the n-gram's look-up for it
// (after that): look = a class other than blank in a round that is not empty.  The candidate's score takes
// bias_weight * d as one more fp32 add behind what it holds.
__device__ __forceinline__ void bias_candidate(RnntBiasShared& bs, float* cscore, int cur, int q, int parent, int cls,
                                               bool look, float bias_weight) {
  const int pst = bs.bstate[cur][parent];
  NgramHit hit{0.f, pst};                                  // blank, or an empty round: no term, no look-up
  if (look) {
    hit = ngram_score(bs.g, pst, cls);
    cscore[q] = __fadd_rn(cscore[q], __fmul_rn(bias_weight, hit.logp));
  }
  bs.cd[q] = hit.logp;
  bs.cnext[q] = hit.next;
}

// The finalisation's pick among the nb live beams of buffer cur: the largest score + bias_weight *
// ctx_final[bstate], ties to the lower position; *top is that value.  Every thread may call it (LDS and
// table reads only); nothing of it is stored in the beams.
__device__ __forceinline__ int bias_pick(const RnntBiasShared& bs, const float* score, int cur, int nb,
                                         float bias_weight, float* top) {
  int pos = 0;
  float best = 0.f;
  for (int i = 0; i < nb; ++i) {
    const float v = __fadd_rn(score[i], __fmul_rn(bias_weight, bs.final[bs.bstate[cur][i]]));
    if (i == 0 || v > best) {
      best = v;
      pos = i;
    }
  }
  *top = best;
  return pos;
}

// LDS of a beam workgroup besides BeamShared: e [kGroup][E], h [kGroup][D], state [2][kMaxBeam][ctx]
// (most recent token last), then lm [beam][V] when it fits next to them.
__host__ __device__ inline size_t beam_fixed_lds(int E, int D, int ctx) {
  return sizeof(float) * kGroup * ((size_t)E + D) + sizeof(int) * 2 * kMaxBeam * ctx;
}

// y[g][r] = w[r] . x[g] + bias[r] for the ng <= kGroup vectors x[g] (LDS, [g][cols]): a wave per
// row, kRows rows in flight per wave so that their loads overlap (the walk is latency-bound: one
// workgroup reads the weights from L2 once per frame).  Per (g, r) the products are summed in the
// order of the greedy kernel's gemv_rows: per lane over c = lane, lane + 64, ..., then wave_sum.
template <typename Store>
__device__ __forceinline__ void gemv_group(const float* __restrict__ w, const float* __restrict__ bias,
                                           const float* __restrict__ x, int rows, int cols, int ng,
                                           Store store) {
  constexpr int kVals = kRows * kGroup;                    // sums per wave and step: v[j * kGroup + g]
  static_assert(kVals == 16, "the reduction below folds 16 sums over lane bits 5..2");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // after the reduction lane l holds the sum of index mine (lane bits 5,4,3,2 -> index bits 3..0)
  const int mine = ((lane >> 5) & 1) << 3 | ((lane >> 4) & 1) << 2 | ((lane >> 3) & 1) << 1 | ((lane >> 2) & 1);
  const int full = cols - cols % (64 * kCols);
  for (int r0 = wave * kRows; r0 < rows; r0 += kWaves * kRows) {
    float v[kVals];
#pragma unroll
    for (int i = 0; i < kVals; ++i) v[i] = 0.f;
    const int myrow = r0 + mine / kGroup;
    const float mybias = bias[min(myrow, rows - 1)];
    const float* wr[kRows];                                // clamped: loads are never conditional (a
#pragma unroll                                             // load under a condition is a branch of its
    for (int j = 0; j < kRows; ++j)                        // own, waited for where the branch ends)
      wr[j] = w + (long)min(r0 + j, rows - 1) * cols;
    for (int c0 = 0; c0 < full; c0 += 64 * kCols) {        // whole chunks: all loads first
      float wv[kRows][kCols];
#pragma unroll
      for (int j = 0; j < kRows; ++j)
#pragma unroll
        for (int q = 0; q < kCols; ++q) wv[j][q] = wr[j][c0 + 64 * q + lane];
#pragma unroll
      for (int q = 0; q < kCols; ++q)
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {                 // (rows g >= ng of x: stale, never stored)
          const float xv = x[g * cols + c0 + 64 * q + lane];
#pragma unroll
          for (int j = 0; j < kRows; ++j) v[j * kGroup + g] = fmaf(wv[j][q], xv, v[j * kGroup + g]);
        }
    }
    if (full < cols) {                                     // the ragged rest, same order
      float wv[kRows][kCols];
#pragma unroll
      for (int j = 0; j < kRows; ++j)
#pragma unroll
        for (int q = 0; q < kCols; ++q) wv[j][q] = wr[j][min(full + 64 * q + lane, cols - 1)];
#pragma unroll
      for (int q = 0; q < kCols; ++q) {
        const int c = full + 64 * q + lane;
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
          const float xv = x[g * cols + min(c, cols - 1)];
#pragma unroll
          for (int j = 0; j < kRows; ++j)
            v[j * kGroup + g] = c < cols ? fmaf(wv[j][q], xv, v[j * kGroup + g]) : v[j * kGroup + g];
        }
      }
    }
    // wave_sum of the 16 sums at once.  A butterfly step o adds lane l ^ o's value to lane l's, for
    // every sum; here the two lanes split the sums between them (the upper lane keeps the upper
    // half), so each step halves the sums a lane carries: 8 + 4 + 2 + 1 shuffles instead of 4 x 16.
    // The pairs added are the butterfly's (fp32 addition commutes), so every sum has wave_sum's bits.
    {
      const bool up32 = lane & 32, up16 = lane & 16, up8 = lane & 8, up4 = lane & 4;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float keep = up32 ? v[i + 8] : v[i], send = up32 ? v[i] : v[i + 8];
        v[i] = keep + __shfl_xor(send, 32, 64);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float keep = up16 ? v[i + 4] : v[i], send = up16 ? v[i] : v[i + 4];
        v[i] = keep + __shfl_xor(send, 16, 64);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float keep = up8 ? v[i + 2] : v[i], send = up8 ? v[i] : v[i + 2];
        v[i] = keep + __shfl_xor(send, 8, 64);
      }
      const float keep = up4 ? v[1] : v[0], send = up4 ? v[0] : v[1];
      float s = keep + __shfl_xor(send, 4, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 1, 64);
      if ((lane & 3) == 0 && mine % kGroup < ng && myrow < rows) store(mine % kGroup, myrow, s + mybias);
    }
  }
}

// lm rows of the beams list[0..n) from their predictor states; per beam the arithmetic (and its
// order) of the greedy kernel's gemv_rows.  Ends with a barrier.
__device__ inline void recompute_lm(const StatelessPointers& p, const StatelessDims& d, const int* __restrict__ list, int n,
                             const int* __restrict__ state, const int* __restrict__ slot,
                             float* __restrict__ e, float* __restrict__ h, float* lm) {
  const int tid = threadIdx.x;
  for (int g0 = 0; g0 < n; g0 += kGroup) {
    const int ng = min(kGroup, n - g0);
    for (int x = tid; x < ng * d.E; x += kThreads) {
      const int g = x / d.E, c = x - g * d.E;
      const int* st = state + list[g0 + g] * d.ctx;
      float acc = 0.f;
      for (int k0 = 0; k0 < d.ctx; k0 += kCols) {          // (loads first, clamped, as in gemv_group)
        float cw[kCols], ev[kCols];
#pragma unroll
        for (int q = 0; q < kCols; ++q) {
          const int k = min(k0 + q, d.ctx - 1);
          cw[q] = p.conv_w[c * d.ctx + k];
          ev[q] = p.emb[(long)st[k] * d.E + c];
        }
#pragma unroll
        for (int q = 0; q < kCols; ++q) acc = k0 + q < d.ctx ? fmaf(cw[q], ev[q], acc) : acc;
      }
      e[g * d.E + c] = acc;
    }
    __syncthreads();
    gemv_group(p.lin_w, p.lin_b, e, d.D, d.E, ng, [&](int g, int r, float y) { h[g * d.D + r] = y; });
    __syncthreads();
    gemv_group(p.pre_w, p.pre_b, h, d.V, d.D, ng,
               [&](int g, int r, float y) { lm[(long)slot[list[g0 + g]] * d.V + r] = y; });
    __syncthreads();
  }
}

// Frames [0, Tb) of amb [Tb][V], Tb >= 1, from the nb beams of buffer `cur` (s.score / s.slot / s.len
// [cur], state [cur], their lm rows): phases A-D per frame.  rec(t, position, pack_record(parent,
// class)) is called by the lane of every kept beam.  On return nb and cur name the beams after the
// last frame, best first.  CACHE: V <= 64 kRegs, the frame's am is held in registers and the next
// frame's is fetched a frame ahead.  c: the search's blank, beam and topk (decode_rnnt.hip BeamHead).
// LM = kLmNgram (ng, lm_weight given; ng->g and ng->ctx / lm_sum [cur] filled): between A and B a thread
// per candidate of a class other than blank adds lm_weight * ngram_score(parent's context, class) to
// the candidate's score, as (beam score + log-probability) + lm_weight * q in fp32, and C hands the
// kept beams the look-up's context and lm_sum + q; a blank candidate keeps its parent's context and
// sum.  The cut to top-k, the ranking, the records and D are the same code in both modes.
// BIAS (bs, bias_weight given; bs->g, bs->final and bs->bstate / bsum [cur] filled): the same thread then adds
// bias_weight * d, (d, next) = the graph's look-up from the parent's state, behind the LM term, and C hands
// the kept beams next and bsum + d; blank keeps the parent's.  Without an LM the candidate phase and its
// barrier exist for the bias alone; with the n-gram every bias LDS write stands beside the n-gram's write of
// the same kind, under the barriers that were there.
template <bool CACHE, int LM = kLmNone, bool BIAS = false, typename C, typename Rec>
__device__ __forceinline__ void beam_walk(const StatelessPointers& p, const StatelessDims& d, const C& c, BeamShared& s,
                                          const float* __restrict__ amb, int Tb, int& nb, int& cur, float* e,
                                          float* h, int* state, float* lm, Rec rec,
                                          RnntNgramShared* ng = nullptr, float lm_weight = 0.f,
                                          RnntBiasShared* bs = nullptr, float bias_weight = 0.f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = d.V, K = min(c.topk, V), BS = c.beam;
  float am_cur[kRegs] = {}, am_next[kRegs] = {};
  if (CACHE) {
#pragma unroll
    for (int j = 0; j < kRegs; ++j) {
      am_cur[j] = amb[min(lane + 64 * j, V - 1)];
    }
  }
  for (int t = 0; t < Tb; ++t) {
    const float* amt = amb + (long)t * V;
    if (CACHE && t + 1 < Tb) {                             // next frame's am: off the critical path
#pragma unroll
      for (int j = 0; j < kRegs; ++j) {
        am_next[j] = amt[V + min(lane + 64 * j, V - 1)];
      }
    }
    // ---- A: a wave per live beam
    for (int i = wave; i < nb; i += kWaves) {
      const float* lmi = lm + (long)s.slot[cur][i] * V;
      const float base = s.score[cur][i];
      float zr[kRegs];
      if (CACHE) {
#pragma unroll
        for (int j = 0; j < kRegs; ++j) {
          const int c = lane + 64 * j;
          zr[j] = c < V ? activate(am_cur[j] + lmi[min(c, V - 1)], d.act) : S2T_NEG_INF;
        }
      }
      float pv = 0.f, lse = 0.f, zmax = 0.f;
      int pi = -1;
      for (int r = 0; r < K; ++r) {
        Top best{S2T_NEG_INF, V};
        if (CACHE) {
#pragma unroll
          for (int j = 0; j < kRegs; ++j) {
            const int c = lane + 64 * j;
            if (c < V && (r == 0 || after(zr[j], c, pv, pi))) best = better(best, Top{zr[j], c});
          }
        } else {
          for (int c = lane; c < V; c += 64) {
            const float z = activate(amt[c] + lmi[c], d.act);
            if (r == 0 || after(z, c, pv, pi)) best = better(best, Top{z, c});
          }
        }
        best = wave_top(best);
        pv = best.v;
        pi = best.i;
        if (r == 0) {                                      // log-softmax as max, then log sum exp
          zmax = pv;
          float sum = 0.f;
          if (CACHE) {
#pragma unroll
            for (int j = 0; j < kRegs; ++j)
              if (lane + 64 * j < V) sum += expf(zr[j] - zmax);
          } else {
            for (int c = lane; c < V; c += 64) sum += expf(activate(amt[c] + lmi[c], d.act) - zmax);
          }
          lse = logf(wave_sum(sum));
        }
        if (lane == 0) {
          const bool ok = pi < V;                          // (only a NaN input leaves a round empty)
          s.cscore[i * K + r] = ok ? base + ((pv - zmax) - lse) : S2T_NEG_INF;
          s.ccls[i * K + r] = ok ? pi : c.blank;
        }
      }
    }
    __syncthreads();
    if constexpr (LM == kLmNgram) {                        // ---- the LM term: a thread per candidate
      for (int q = tid; q < nb * K; q += kThreads) {
        const int cls = s.ccls[q], pctx = ng->ctx[cur][q / K];
        const float sc = s.cscore[q];
        NgramHit hit{0.f, pctx};                           // blank, or an empty round: no term, no look-up
        if (cls != c.blank && sc != S2T_NEG_INF) {
          hit = ngram_score(ng->g, pctx, cls);
          s.cscore[q] = __fadd_rn(sc, __fmul_rn(lm_weight, hit.logp));
        }
        ng->cq[q] = hit.logp;
        ng->cnext[q] = hit.next;
        if constexpr (BIAS)
          bias_candidate(*bs, s.cscore, cur, q, q / K, cls, cls != c.blank && sc != S2T_NEG_INF, bias_weight);
      }
      __syncthreads();
    } else if constexpr (BIAS) {                           // ---- the bias term alone: a thread per candidate
      for (int q = tid; q < nb * K; q += kThreads) {
        const int cls = s.ccls[q];
        bias_candidate(*bs, s.cscore, cur, q, q / K, cls, cls != c.blank && s.cscore[q] != S2T_NEG_INF,
                       bias_weight);
      }
      __syncthreads();
    }
    // ---- B: rank the candidates, keep the beam_size best
    const int nc = nb * K, nnb = min(nc, BS), nxt = cur ^ 1;
    rank_candidates(s.cscore, nc, nnb, s.pick);
    __syncthreads();
    // ---- C: the new beams (wave 0, a lane per beam)
    if (wave == 0) {
      const bool live = lane < nnb;
      int parent = 0, cls = c.blank;
      if (live) {
        const int q = s.pick[lane];
        parent = q / K;
        cls = s.ccls[q];
        s.score[nxt][lane] = s.cscore[q];
        s.len[nxt][lane] = s.len[cur][parent] + (cls != c.blank ? 1 : 0);
        if constexpr (LM == kLmNgram) {
          ng->ctx[nxt][lane] = ng->cnext[q];
          ng->lm_sum[nxt][lane] = ng->lm_sum[cur][parent] + ng->cq[q];
        }
        if constexpr (BIAS) {
          bs->bstate[nxt][lane] = bs->cnext[q];
          bs->bsum[nxt][lane] = bs->bsum[cur][parent] + bs->cd[q];
        }
        rec(t, lane, pack_record(parent, cls));
        const int* so = state + (cur * kMaxBeam + parent) * d.ctx;
        int* sn = state + (nxt * kMaxBeam + lane) * d.ctx;
        if (cls == c.blank) {
          for (int k = 0; k < d.ctx; ++k) sn[k] = so[k];
        } else {
          for (int k = 0; k + 1 < d.ctx; ++k) sn[k] = so[k + 1];
          sn[d.ctx - 1] = cls;
        }
      }
      const bool emits = live && cls != c.blank;
      // lm rows: a blank child keeps its parent's row (a parent has at most one); the emitting
      // beams take the rows that are left, in beam order
      unsigned used = (live && !emits) ? 1u << s.slot[cur][parent] : 0u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) used |= __shfl_xor(used, o, 64);
      const unsigned long long em = __ballot(emits);
      int myslot = live ? s.slot[cur][parent] : 0;
      if (emits) {
        int order = __popcll(em & ((1ull << lane) - 1ull));
        s.emit[order] = lane;
        for (int sl = 0; sl < kMaxBeam; ++sl)
          if (!((used >> sl) & 1u)) {
            if (order == 0) {
              myslot = sl;
              break;
            }
            --order;
          }
      }
      if (live) s.slot[nxt][lane] = myslot;
      if (lane == 0) s.nemit = __popcll(em);
    }
    __syncthreads();
    // ---- D: lm of the beams that emitted (at most one symbol per frame per beam)
    const int ne = s.nemit;
    if (ne > 0) recompute_lm(p, d, s.emit, ne, state + nxt * kMaxBeam * d.ctx, s.slot[nxt], e, h, lm);
    nb = nnb;
    cur = nxt;
    if (CACHE) {
#pragma unroll
      for (int j = 0; j < kRegs; ++j) am_cur[j] = am_next[j];
    }
  }
}

}  // namespace s2t_dec
