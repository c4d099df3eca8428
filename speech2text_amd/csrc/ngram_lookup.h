// The back-off n-gram look-up as ONE device function: s2t_ngram_score's kernel (csrc/ngram.hip) and the
// n-gram mode of the CTC frame body (csrc/decode_ctc.h) share it.  It is the scoring statement of
// include/s2t_mi355.h: acc = 0.f, n = ctx; while n != 0, binary-search c among the arcs of n (found:
// acc + arc_logp, arc_next), else acc += ctx_backoff[n], n = ctx_fail[n]; at the dense root acc +
// arc_logp[c], arc_next[c].  fp32 adds in exactly this order.
//
// The tables are validated on the host and trusted here, with two cheap guards so that no table can
// hang a kernel or make it read outside its arrays: the loop over hops is bounded by `order` (then the
// root answers), and every index taken from a table is clamped into its array before it is used.
#pragma once
#include "../../include/s2t_mi355.h"
#include "common.h"

namespace s2t_dec {

struct NgramTables {
  int V, order, num_ctx, num_arcs;
  const int *ctx_begin, *ctx_fail;
  const float* ctx_backoff;
  const int* arc_token;
  const float* arc_logp;
  const int* arc_next;
};

struct NgramHit {
  float logp;
  int next;
};

__device__ __forceinline__ int ngram_clamp(int v, int n) { return min(max(v, 0), n - 1); }

// c in [0, V), ctx in [0, num_ctx): the callers clamp what they were handed
__device__ __forceinline__ NgramHit ngram_score(const NgramTables& g, int ctx, int c) {
  float acc = 0.f;
  int n = ctx, arc = c;                                    // the root's arc of c, unless a context lists c
  for (int hop = 0; hop < g.order && n != 0; ++hop) {
    const int end = min(max(g.ctx_begin[n + 1], 0), g.num_arcs);
    int lo = min(max(g.ctx_begin[n], 0), end), hi = end;
    while (lo < hi) {                                      // the first arc whose token is not below c
      const int mid = (lo + hi) >> 1;
      if (g.arc_token[mid] < c) lo = mid + 1;
      else hi = mid;
    }
    if (lo < end && g.arc_token[lo] == c) {
      arc = lo;
      break;
    }
    acc += g.ctx_backoff[n];
    n = ngram_clamp(g.ctx_fail[n], g.num_ctx);
  }
  return NgramHit{acc + g.arc_logp[arc], ngram_clamp(g.arc_next[arc], g.num_ctx)};
}

// the descriptor's limits, checked on the host before any launch; no device pointer is followed
inline bool ngram_desc_ok(const S2tNgramLmDesc* d) {
  return d && d->V >= 1 && d->V <= S2T_RNNT_LSTM_MAX_VOCAB && d->order >= 1 && d->order <= S2T_NGRAM_MAX_ORDER &&
         d->num_ctx >= 1 && d->num_arcs >= d->V && d->ctx_begin && d->ctx_fail && d->ctx_backoff && d->arc_token &&
         d->arc_logp && d->arc_next;
}

inline NgramTables ngram_tables(const S2tNgramLmDesc& d) {
  return NgramTables{d.V, d.order, d.num_ctx, d.num_arcs, d.ctx_begin, d.ctx_fail, d.ctx_backoff, d.arc_token,
                     d.arc_logp, d.arc_next};
}

// A hotword graph (S2tContextGraphDesc, THE BIAS STATEMENT) is the same kind of table: ngram_score reads
// its hop bound from the tables it is handed, so the graph rides the same device function with order =
// max_depth + 1 (a state of depth d fails at most d times) and arc_logp = arc_score.  Its limits have a
// host check of their own.
inline bool context_desc_ok(const S2tContextGraphDesc* d) {
  return d && d->V >= 1 && d->V <= S2T_RNNT_LSTM_MAX_VOCAB && d->max_depth >= 0 &&
         d->max_depth <= S2T_CONTEXT_MAX_DEPTH && d->num_ctx >= 1 && d->num_arcs >= d->V && d->ctx_begin &&
         d->ctx_fail && d->ctx_backoff && d->ctx_final && d->arc_token && d->arc_score && d->arc_next;
}

inline NgramTables context_tables(const S2tContextGraphDesc& d) {
  return NgramTables{d.V, d.max_depth + 1, d.num_ctx, d.num_arcs, d.ctx_begin, d.ctx_fail, d.ctx_backoff,
                     d.arc_token, d.arc_score, d.arc_next};
}

}  // namespace s2t_dec
