// One frame of the CTC prefix beam search as a device function, so that the one-launch kernel and the
// lockstep round kernel of csrc/decode_ctc.hip instantiate ONE body: with lm_weight = 0 the fused
// entry then makes the arithmetic of the plain one, in the same order, and gives the same bits.
//
// A live prefix carries pb / pnb (log-probabilities of its alignments ending in blank / non-blank),
// its trie node, its last token, its length and (with an LM) lm_sum.  Prefix identity is EXACT: every
// token sequence that was ever kept has one node (parent, token, first_child, next_sibling) of a
// per-utterance trie in the workspace, and a new node is created only after the children of its
// parent were searched for its token.  A sequence therefore has one node id for ever, also when it
// leaves the beam and enters it again, and "is p + c live" is a compare of node ids.
//
// Candidates of a frame are slots: slot i (K + 1) is prefix i staying, slot i (K + 1) + 1 + r its
// extension by the class of rank r.  Two slots spell the same sequence only when an extension lands
// on a live prefix (p + c = p' + c' implies p = p'), so a merged candidate has at most two pnb terms and
// the two-operand logaddexp (symmetric in its operands) leaves no summation order to choose.  Its
// rank key is the smallest contributing slot: first contributing parent, staying before
// extensions, class rank.
//
// The body stands once for three LM modes: none; RNN rows (q [beam][V] of the live prefixes, and emit /
// parent / token for the LM step that follows the frame); n-gram (a live prefix also carries its
// context id, the slot thread that would add q[i * V + c] runs the look-up of csrc/ngram_lookup.h instead
// and records the `next` it returns beside clm, and a kept prefix that was not live takes that next:
// nothing has to run between frames).  The n-gram mode's extra LDS is a struct of its own, so the
// other modes' kernels keep the LDS and the arithmetic they had.
//
// Beside the LM mode stands a compile-time bias switch (hotwords: THE BIAS STATEMENT of
// include/s2t_mi355.h).  A live prefix then also carries a graph state and bias_sum, in a struct of their
// own (CtcBiasShared); the slot thread that runs the n-gram's look-up runs the graph's after it, through
// the same device function; the ranking total gains bias_weight * bias_sum as its last add.  Every LDS
// write of the bias part stands next to the n-gram part's write of the same kind (the candidates'
// before the barrier that ends the slot phase, the beam's after the barrier that follows the picks'
// reads), so the body needs no barrier it did not have.  With the switch off the body's text is what
// it was.
#pragma once
#include "common.h"
#include "decode_common.h"
#include "decode_records.h"
#include "ngram_lookup.h"

namespace s2t_dec {

constexpr int kCtcThreads = 256;
constexpr int kCtcWaves = kCtcThreads / 64;
constexpr int kCtcSlots = kMaxBeam * (kMaxBeam + 1);
constexpr int kCtcNoKey = 0x7fffffff;
constexpr int kCtcPlain = 0, kCtcRnn = 1, kCtcNgram = 2;   // the LM modes of ctc_frame

struct alignas(16) CtcNode {
  int parent, token, first_child, next_sibling;
};

struct CtcShared {
  Top red[2][kCtcWaves];
  float scratch[kCtcWaves];
  int cls[kMaxBeam];               // the frame's classes in rank order and their log-probabilities
  float lp[kMaxBeam];
  float pb[kMaxBeam], pnb[kMaxBeam], lm_sum[kMaxBeam];   // the beam
  int node[kMaxBeam], last[kMaxBeam], len[kMaxBeam];
  int nb, nnodes;
  float cpb[kCtcSlots], cpnb[kCtcSlots], ctot[kCtcSlots], clm[kCtcSlots];   // the candidates
  int cnode[kCtcSlots], ckey[kCtcSlots];
  float ext_in[kMaxBeam];          // what an extension adds to the live prefix it lands on ...
  int ext_key[kMaxBeam];           // ... and the slot it came from
  int pick[kMaxBeam];
  int par_node[kMaxBeam];          // node of a new prefix' parent
};

struct CtcNgramShared {            // the n-gram mode's part of the beam and of the candidates
  NgramTables g;                   // (in LDS: ten scalar registers less to hold across the frame)
  int state[kMaxBeam];             // a live prefix' context id
  int cnext[kCtcSlots];            // the context a candidate is in when it is kept
};

struct CtcBiasShared {             // the bias switch's part of the beam and of the candidates
  NgramTables g;                   // the graph in the look-up's table form (order = max_depth + 1)
  const float* final;              // ctx_final [num_ctx]
  int state[kMaxBeam];             // a live prefix' graph state ...
  float sum[kMaxBeam];             // ... and its bias_sum
  int cnext[kCtcSlots];            // the state a candidate is in when it is kept ...
  float csum[kCtcSlots];           // ... and its bias_sum
};

// the empty prefix: pb = 0, pnb = -inf, the root node
__device__ __forceinline__ void ctc_start(CtcShared& s, CtcNode* nodes) {
  if (threadIdx.x == 0) {
    s.pb[0] = 0.f;
    s.pnb[0] = S2T_NEG_INF;
    s.lm_sum[0] = 0.f;
    s.node[0] = 0;
    s.last[0] = -1;
    s.len[0] = 0;
    s.nb = 1;
    s.nnodes = 1;
    nodes[0] = CtcNode{-1, -1, -1, -1};
  }
}

// One frame x [V] (global) of one utterance; row: LDS [V].  kCtcRnn: q [beam][V] are the rows of the live
// prefixes (beam order); emit / parent / token [beam] receive what s2t_rnn_lm_step needs, parent as a
// row of the whole batch (row0 + position).  kCtcNgram: ng holds the tables and the context ids (else
// NULL).  All kCtcThreads threads call it; it begins and ends with the beam in s (and ng) consistent
// for every thread.  BIAS: bs holds the graph, the states and the sums (else NULL).
template <int MODE, bool BIAS = false>
__device__ __forceinline__ void ctc_frame(CtcShared& s, float* row, const float* __restrict__ x, int V, int K,
                                          int BS, int blank, CtcNode* nodes, int max_nodes, float lm_weight,
                                          const float* __restrict__ q, int* emit, int* parent, int* token,
                                          int row0, CtcNgramShared* ng = nullptr, CtcBiasShared* bs = nullptr,
                                          float bias_weight = 0.f) {
  constexpr bool LM = MODE != kCtcPlain;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = s.nb, K1 = K + 1, nc = nb * K1;
  // ---- the frame's log-softmax and its K classes, once for all prefixes
  float m = S2T_NEG_INF;
  for (int c = tid; c < V; c += kCtcThreads) {
    const float v = x[c];
    row[c] = v;                                            // (a thread only ever reads its own columns)
    m = fmaxf(m, v);
  }
  if (tid < kMaxBeam) {
    s.ext_in[tid] = S2T_NEG_INF;
    s.ext_key[tid] = kCtcNoKey;
    s.pick[tid] = -1;
  }
  const float zmax = block_max(m, s.scratch);
  float sum = 0.f;
  for (int c = tid; c < V; c += kCtcThreads) sum += expf(row[c] - zmax);
  const float lse = logf(block_sum(sum, s.scratch));
  float pv = 0.f;
  int pi = -1;
  for (int r = 0; r < K; ++r) {
    Top best{S2T_NEG_INF, V};
    for (int c = tid; c < V; c += kCtcThreads) {
      const float z = row[c];
      if (r == 0 || after(z, c, pv, pi)) best = better(best, Top{z, c});
    }
    best = wave_top(best);
    if (lane == 0) s.red[r & 1][wave] = best;
    __syncthreads();                                       // (one barrier a round: red is double-buffered)
    best = better(better(s.red[r & 1][0], s.red[r & 1][1]), better(s.red[r & 1][2], s.red[r & 1][3]));
    pv = best.v;
    pi = best.i;
    if (tid == 0) {
      const bool ok = pi < V;                              // (only a NaN input leaves a round empty)
      s.cls[r] = ok ? pi : blank;
      s.lp[r] = ok ? (pv - zmax) - lse : S2T_NEG_INF;
    }
  }
  __syncthreads();
  // ---- a thread per (prefix, staying or class) contribution
  for (int xs = tid; xs < nc; xs += kCtcThreads) {
    const int i = xs / K1, j = xs - i * K1;
    const float pb = s.pb[i], pnb = s.pnb[i], sc = log_add_precise(pb, pnb);
    const int last = s.last[i];
    float cpb = S2T_NEG_INF, cpnb = S2T_NEG_INF, clm = s.lm_sum[i];
    int cnode = s.node[i], key = kCtcNoKey, cnext = 0;
    if (MODE == kCtcNgram) cnext = ng->state[i];
    float cbsum = 0.f;
    int cbnext = 0;
    if (BIAS) {
      cbsum = bs->sum[i];
      cbnext = bs->state[i];
    }
    if (j == 0) {
      for (int r = 0; r < K; ++r) {
        const int c = s.cls[r];
        if (c == blank) cpb = sc + s.lp[r];
        else if (c == last) cpnb = pnb + s.lp[r];
      }
      if (cpb > S2T_NEG_INF || cpnb > S2T_NEG_INF) key = xs;
    } else {
      const int c = s.cls[j - 1];
      const float v = c == blank ? S2T_NEG_INF : (c == last ? pb : sc) + s.lp[j - 1];
      if (v > S2T_NEG_INF) {
        int id = nodes[cnode].first_child;                 // the one node of p + c, if it was ever kept
        for (int hop = 0; id >= 0; ++hop) {
          const CtcNode n = nodes[id];
          if (n.token == c) break;
          id = hop < max_nodes ? n.next_sibling : -1;      // (a list is shorter than the trie: never a hang)
        }
        int landed = -1;
        if (id >= 0)
          for (int mm = 0; mm < nb; ++mm)
            if (s.node[mm] == id) landed = mm;
        if (landed >= 0) {                                 // p + c is live: one writer (its only parent)
          s.ext_in[landed] = v;
          s.ext_key[landed] = xs;
        } else {
          cpnb = v;
          key = xs;
          if (MODE == kCtcRnn) clm += q[(long)i * V + c];
          if (MODE == kCtcNgram) {
            const NgramHit h = ngram_score(ng->g, cnext, c);
            clm += h.logp;
            cnext = h.next;
          }
          if (BIAS) {
            const NgramHit h = ngram_score(bs->g, cbnext, c);
            cbsum += h.logp;
            cbnext = h.next;
          }
        }
        cnode = id;
      }
    }
    s.cpb[xs] = cpb;
    s.cpnb[xs] = cpnb;
    s.clm[xs] = clm;
    s.cnode[xs] = cnode;
    s.ckey[xs] = key;
    if (MODE == kCtcNgram) ng->cnext[xs] = cnext;
    float ctot = LM ? cpnb + lm_weight * clm : cpnb;       // (an extension: pb = -inf; staying: below)
    if (BIAS) {
      bs->cnext[xs] = cbnext;
      bs->csum[xs] = cbsum;
      ctot = ctot + bias_weight * cbsum;
    }
    s.ctot[xs] = ctot;
  }
  __syncthreads();
  if (tid < nb) {                                          // the staying candidates take what landed on them
    const int xs = tid * K1;
    const float pnb = log_add_precise(s.cpnb[xs], s.ext_in[tid]);
    const float tot = log_add_precise(s.cpb[xs], pnb);
    s.cpnb[xs] = pnb;
    s.ckey[xs] = min(s.ckey[xs], s.ext_key[tid]);
    float ctot = LM ? tot + lm_weight * s.clm[xs] : tot;
    if (BIAS) ctot = ctot + bias_weight * bs->csum[xs];
    s.ctot[xs] = ctot;
  }
  __syncthreads();
  // ---- rank by counting: total descending, then key ascending
  for (int xs = tid; xs < nc; xs += kCtcThreads) {
    const int key = s.ckey[xs];
    if (key == kCtcNoKey) continue;
    const float mine = s.ctot[xs];
    int rank = 0;
    for (int o = 0; o < nc; ++o) {
      const int ok = s.ckey[o];
      const float ot = s.ctot[o];
      rank += (ok != kCtcNoKey && (ot > mine || (ot == mine && ok < key))) ? 1 : 0;
    }
    if (rank < BS) s.pick[rank] = xs;
  }
  __syncthreads();
  // ---- the new beam
  const int xs = tid < BS ? s.pick[tid] : -1;
  const bool kept = xs >= 0;
  float npb = 0.f, npnb = 0.f, nlm = 0.f, nbsum = 0.f;
  int nnode = 0, nlast = 0, nlen = 0, npar = 0, src = tid, ext = 0, nstate = 0, nbstate = 0;
  if (kept) {
    src = xs / K1;
    const int j = xs - src * K1;
    ext = j > 0;
    npb = s.cpb[xs];
    npnb = s.cpnb[xs];
    nlm = s.clm[xs];
    nnode = s.cnode[xs];
    nlast = ext ? s.cls[j - 1] : s.last[src];
    nlen = s.len[src] + ext;
    npar = s.node[src];
    if (MODE == kCtcNgram) nstate = ng->cnext[xs];
    if (BIAS) {
      nbstate = bs->cnext[xs];
      nbsum = bs->csum[xs];
    }
  }
  __syncthreads();
  if (s.pick[0] < 0) {                                     // no candidate at all (NaN input): the beam stays
    if (MODE == kCtcRnn && tid < BS) {
      emit[tid] = 0;
      parent[tid] = row0 + tid;
      token[tid] = 0;
    }
    return;
  }
  if (kept) {
    s.pb[tid] = npb;
    s.pnb[tid] = npnb;
    s.lm_sum[tid] = nlm;
    s.node[tid] = nnode;
    s.last[tid] = nlast;
    s.len[tid] = nlen;
    s.par_node[tid] = npar;
    if (MODE == kCtcNgram) ng->state[tid] = nstate;
    if (BIAS) {
      bs->state[tid] = nbstate;
      bs->sum[tid] = nbsum;
    }
  }
  if (MODE == kCtcRnn && tid < BS) {                       // a prefix that was not live steps the LM
    emit[tid] = kept && ext;
    parent[tid] = row0 + src;
    token[tid] = kept && ext ? nlast : 0;
  }
  const unsigned long long keep_mask = __ballot(kept);     // (BS <= 16: all in wave 0)
  __syncthreads();
  if (tid == 0) {                                          // nodes of the sequences kept for the first time
    const int nnb = __popcll(keep_mask);
    int nn = s.nnodes;
    for (int r = 0; r < nnb; ++r) {
      if (s.node[r] >= 0) continue;
      const int pn = s.par_node[r];
      const int id = nn < max_nodes ? nn++ : max_nodes - 1;    // (cannot exceed: beam new nodes a frame)
      nodes[id] = CtcNode{pn, s.last[r], -1, nodes[pn].first_child};
      nodes[pn].first_child = id;
      s.node[r] = id;
    }
    s.nnodes = nn;
    s.nb = nnb;
  }
  __syncthreads();
}

// the best prefix (position 0): its tokens by a walk to the root, its acoustic score.  tokens holds
// max_tokens positions: a longer prefix keeps its first max_tokens tokens and out_len saturates there
// (the whole-utterance entries pass T: a prefix has at most a token a frame).  The walk ends at the
// root, whatever its depth (a chunk-carried trie's root is the committed prefix), after at most
// max_hops nodes.  pos: the beam position reported (the bias entries' finalisation picks it).
__device__ __forceinline__ void ctc_finish(const CtcShared& s, const CtcNode* nodes, long* __restrict__ tokens,
                                           long* out_len, float* score, float* lm_score, int max_tokens,
                                           int max_hops, int pos = 0) {
  if (threadIdx.x == 0) {
    const int n = s.len[pos];
    *out_len = min(n, max_tokens);
    *score = log_add_precise(s.pb[pos], s.pnb[pos]);
    if (lm_score) *lm_score = s.lm_sum[pos];
    int id = s.node[pos];
    for (int p = n - 1, hop = 0; p >= 0 && id > 0 && hop < max_hops; --p, ++hop) {
      const CtcNode nd = nodes[id];
      if (p < max_tokens) tokens[p] = nd.token;
      id = nd.parent;
    }
  }
}

// The bias entries' finalisation: the live prefix with the largest (logaddexp(pb, pnb) + lm_weight *
// lm_sum) + bias_weight * (bias_sum + ctx_final[state]), ties to the lower position; *bias_score is its
// bias_sum + ctx_final[state].  It reads the beam and writes an output: nothing of it is carried.
// Thread 0 calls it, after the barrier that ends a frame (or the load of the beam).
template <bool LM>
__device__ __forceinline__ int ctc_bias_pick(const CtcShared& s, const CtcBiasShared& bs, float lm_weight,
                                             float bias_weight, float* bias_score) {
  int pos = 0;
  float best = 0.f, best_bias = 0.f;
  for (int i = 0; i < s.nb; ++i) {
    float tot = log_add_precise(s.pb[i], s.pnb[i]);
    if (LM) tot = tot + lm_weight * s.lm_sum[i];
    const float fb = bs.sum[i] + bs.final[ngram_clamp(bs.state[i], bs.g.num_ctx)];
    tot = tot + bias_weight * fb;
    if (i == 0 || tot > best) {
      pos = i;
      best = tot;
      best_bias = fb;
    }
  }
  *bias_score = best_bias;
  return pos;
}

}  // namespace s2t_dec
