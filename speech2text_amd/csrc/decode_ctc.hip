// CTC prefix beam search, lexicon-free, with equal prefixes merged exactly and optional RNN-LM
// shallow fusion, for gfx950.  (The reference's CTC beam decoder wraps a lexicon decoder of a library;
// this is the textbook prefix search over the model's own classes.)  The per-frame body, the trie that
// gives a token sequence one node id for ever and the candidate slots are csrc/decode_ctc.h.
//
//   s2t_ctc_prefix_beam      ONE launch per batch, one workgroup (4 waves) per utterance walking its
//                            frames on the device; the beam lives in LDS, the trie in the workspace.
//   s2t_ctc_prefix_beam_lm   lockstep rounds over the batch, exactly T of them and no host
//                            synchronisation: per round one search kernel (the same frame body; it
//                            gathers the q[c] it needs from the live prefixes' LM rows and writes emit /
//                            parent / token), then s2t_rnn_lm_step on B * beam_size rows through two
//                            alternating state buffers.  The beam lives in the workspace between
//                            rounds.  A row past its length passes its state through.
//   s2t_ctc_prefix_beam_ngram
//                            the plain entry's one launch with a back-off n-gram LM: the frame body's
//                            n-gram mode scores an extension by the look-up of csrc/ngram_lookup.h and a
//                            kept prefix takes the context that look-up returned, so nothing runs
//                            between frames.  The beam gains one int per prefix, in LDS.
//   s2t_ctc_prefix_beam_chunk, s2t_ctc_prefix_beam_lm_chunk
//                            the two above fed their frames in pieces: beam and trie in a caller-owned
//                            state, the same frame body and round kernel, and at the end of every call
//                            a compaction of the trie to what the live prefixes can still reach.
//   s2t_ctc_prefix_beam_bias, s2t_ctc_prefix_beam_ngram_bias, and their _chunk partners
//                            the plain and n-gram launches with the frame body's bias switch on: a live
//                            prefix also carries a hotword-graph state and bias_sum (two more arrays behind
//                            the state's layout), and the outputs report the live prefix that is best
//                            once every unfinished match has been paid back (the finalisation).
//   s2t_ctc_prefix_beam_ngram_chunk
//                            the n-gram form fed its frames in pieces: the plain chunk kernel's shape in
//                            the frame body's n-gram mode, still ONE launch; the state gains the live
//                            prefixes' context ids behind the plain layout.
#include <hip/hip_runtime.h>

#include "../../include/s2t_mi355.h"
#include "common.h"
#include "decode_ctc.h"

namespace {

using namespace s2t_dec;

static_assert(S2T_RNNT_LSTM_MAX_BEAM == kMaxBeam, "the header's limit is the kernels'");
struct CtcCompact {
  int anc, depth;                  // the live nodes' lowest common ancestor and its absolute depth
  int part[kCtcWaves];
};

static_assert(sizeof(float) * S2T_RNNT_LSTM_MAX_VOCAB + sizeof(CtcShared) + sizeof(CtcNgramShared) +
                      sizeof(CtcBiasShared) + sizeof(CtcCompact) <= 60 * 1024,
              "a frame's logits are staged in LDS whole, beside the beam, the n-gram part, the bias part and the "
              "compaction's");

struct CtcArgs {
  const float* logits;    // [B][T][V]
  const long* lengths;    // [B]
  int T, V, blank, beam, topk, max_nodes;
  CtcNode* nodes;         // [B][max_nodes]
  long* tokens;           // [B][T]
  long* out_len;          // [B]
  float* score;           // [B]
};

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_kernel(CtcArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  const int b = blockIdx.x;
  const int Tb = (int)clamped_len(a.lengths, b, a.T);
  CtcNode* nodes = a.nodes + (long)b * a.max_nodes;
  const float* x = a.logits + (long)b * a.T * a.V;
  ctc_start(s, nodes);
  __syncthreads();
  const int K = min(a.topk, a.V);
  for (int t = 0; t < Tb; ++t)
    ctc_frame<kCtcPlain>(s, row, x + (long)t * a.V, a.V, K, a.beam, a.blank, nodes, a.max_nodes, 0.f, nullptr,
                         nullptr, nullptr, nullptr, 0);
  ctc_finish(s, nodes, a.tokens + (long)b * a.T, a.out_len + b, a.score + b, nullptr, a.T, a.max_nodes);
}

// ------------------------------------------------------------------ the n-gram form: one launch
struct CtcNgramArgs {
  CtcArgs c;
  NgramTables g;
  float lm_weight;
  int start_ctx;
  float* lm_score;        // [B]
};

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_ngram_kernel(CtcNgramArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  __shared__ CtcNgramShared ng;
  const int b = blockIdx.x;
  const int Tb = (int)clamped_len(a.c.lengths, b, a.c.T);
  CtcNode* nodes = a.c.nodes + (long)b * a.c.max_nodes;
  const float* x = a.c.logits + (long)b * a.c.T * a.c.V;
  ctc_start(s, nodes);
  if (threadIdx.x == 0) {
    ng.g = a.g;
    ng.state[0] = a.start_ctx;
  }
  __syncthreads();
  const int K = min(a.c.topk, a.c.V);
  for (int t = 0; t < Tb; ++t)
    ctc_frame<kCtcNgram>(s, row, x + (long)t * a.c.V, a.c.V, K, a.c.beam, a.c.blank, nodes, a.c.max_nodes,
                         a.lm_weight, nullptr, nullptr, nullptr, nullptr, 0, &ng);
  ctc_finish(s, nodes, a.c.tokens + (long)b * a.c.T, a.c.out_len + b, a.c.score + b, a.lm_score + b, a.c.T,
             a.c.max_nodes);
}

// ------------------------------------------------------------------ the bias forms: one launch
struct CtcBiasArgs {
  CtcNgramArgs n;         // (g, lm_weight, start_ctx, lm_score: the n-gram form only)
  NgramTables graph;
  const float* ctx_final;
  float bias_weight;
  float* bias_score;      // [B]
};

// the graph and the empty prefix' bias part: the root, nothing lent
__device__ __forceinline__ void ctc_bias_start(CtcBiasShared& bs, const NgramTables& graph, const float* ctx_final) {
  if (threadIdx.x == 0) {
    bs.g = graph;
    bs.final = ctx_final;
    bs.state[0] = 0;
    bs.sum[0] = 0.f;
  }
}

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_bias_kernel(CtcBiasArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  __shared__ CtcBiasShared bs;
  const CtcArgs& c = a.n.c;
  const int b = blockIdx.x;
  const int Tb = (int)clamped_len(c.lengths, b, c.T);
  CtcNode* nodes = c.nodes + (long)b * c.max_nodes;
  const float* x = c.logits + (long)b * c.T * c.V;
  ctc_start(s, nodes);
  ctc_bias_start(bs, a.graph, a.ctx_final);
  __syncthreads();
  const int K = min(c.topk, c.V);
  for (int t = 0; t < Tb; ++t)
    ctc_frame<kCtcPlain, true>(s, row, x + (long)t * c.V, c.V, K, c.beam, c.blank, nodes, c.max_nodes, 0.f, nullptr,
                               nullptr, nullptr, nullptr, 0, nullptr, &bs, a.bias_weight);
  int pos = 0;
  if (threadIdx.x == 0) pos = ctc_bias_pick<false>(s, bs, 0.f, a.bias_weight, a.bias_score + b);
  ctc_finish(s, nodes, c.tokens + (long)b * c.T, c.out_len + b, c.score + b, nullptr, c.T, c.max_nodes, pos);
}

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_ngram_bias_kernel(CtcBiasArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  __shared__ CtcNgramShared ng;
  __shared__ CtcBiasShared bs;
  const CtcArgs& c = a.n.c;
  const int b = blockIdx.x;
  const int Tb = (int)clamped_len(c.lengths, b, c.T);
  CtcNode* nodes = c.nodes + (long)b * c.max_nodes;
  const float* x = c.logits + (long)b * c.T * c.V;
  ctc_start(s, nodes);
  if (threadIdx.x == 0) {
    ng.g = a.n.g;
    ng.state[0] = a.n.start_ctx;
  }
  ctc_bias_start(bs, a.graph, a.ctx_final);
  __syncthreads();
  const int K = min(c.topk, c.V);
  for (int t = 0; t < Tb; ++t)
    ctc_frame<kCtcNgram, true>(s, row, x + (long)t * c.V, c.V, K, c.beam, c.blank, nodes, c.max_nodes, a.n.lm_weight,
                               nullptr, nullptr, nullptr, nullptr, 0, &ng, &bs, a.bias_weight);
  int pos = 0;
  if (threadIdx.x == 0) pos = ctc_bias_pick<true>(s, bs, a.n.lm_weight, a.bias_weight, a.bias_score + b);
  ctc_finish(s, nodes, c.tokens + (long)b * c.T, c.out_len + b, c.score + b, a.n.lm_score + b, c.T, c.max_nodes,
             pos);
}

// ------------------------------------------------------------------ the lockstep form
struct CtcState {                  // the beams between rounds, R = B * beam rows
  float *pb, *pnb, *lm_sum;        // [R]
  int *node, *last, *len;          // [R]
  int *nb, *nnodes;                // [B]
  int *emit, *parent, *token;      // [R]
};

struct CtcLmArgs {
  CtcArgs c;
  CtcState st;
  const float* q;                  // [R][V] rows of the live prefixes
  float lm_weight;
  int t, lm_start_token;
  float* lm_score;
};

__device__ __forceinline__ void load_beam(CtcShared& s, const CtcState& st, int b, int BS) {
  const int tid = threadIdx.x, r = b * BS + tid;
  if (tid < BS) {
    s.pb[tid] = st.pb[r];
    s.pnb[tid] = st.pnb[r];
    s.lm_sum[tid] = st.lm_sum[r];
    s.node[tid] = st.node[r];
    s.last[tid] = st.last[r];
    s.len[tid] = st.len[r];
  }
  if (tid == 0) {
    s.nb = st.nb[b];
    s.nnodes = st.nnodes[b];
  }
}

// grid B: the empty prefix of every utterance; the LM's first step is asked for on row 0 of each
__global__ __launch_bounds__(64) void ctc_lm_init_kernel(CtcLmArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.c.beam, r = b * BS + tid;
  if (tid < BS) {
    a.st.pb[r] = tid == 0 ? 0.f : S2T_NEG_INF;
    a.st.pnb[r] = S2T_NEG_INF;
    a.st.lm_sum[r] = 0.f;
    a.st.node[r] = 0;
    a.st.last[r] = -1;
    a.st.len[r] = 0;
    a.st.emit[r] = tid == 0;
    a.st.parent[r] = r;
    a.st.token[r] = a.lm_start_token < 0 ? 0 : a.lm_start_token;
  }
  if (tid == 0) {
    a.st.nb[b] = 1;
    a.st.nnodes[b] = 1;
    a.c.nodes[(long)b * a.c.max_nodes] = CtcNode{-1, -1, -1, -1};
  }
}

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_round_kernel(CtcLmArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.c.beam, r = b * BS + tid;
  const int Tb = (int)clamped_len(a.c.lengths, b, a.c.T);
  if (a.t >= Tb) {                                         // no frame: every row keeps its LM state
    if (tid < BS) {
      a.st.emit[r] = 0;
      a.st.parent[r] = r;
      a.st.token[r] = 0;
    }
    return;
  }
  CtcNode* nodes = a.c.nodes + (long)b * a.c.max_nodes;
  load_beam(s, a.st, b, BS);
  __syncthreads();
  ctc_frame<kCtcRnn>(s, row, a.c.logits + ((long)b * a.c.T + a.t) * a.c.V, a.c.V, min(a.c.topk, a.c.V), BS,
                     a.c.blank, nodes, a.c.max_nodes, a.lm_weight, a.q + (long)b * BS * a.c.V, a.st.emit + b * BS,
                     a.st.parent + b * BS, a.st.token + b * BS, b * BS);
  if (tid < s.nb) {
    a.st.pb[r] = s.pb[tid];
    a.st.pnb[r] = s.pnb[tid];
    a.st.lm_sum[r] = s.lm_sum[tid];
    a.st.node[r] = s.node[tid];
    a.st.last[r] = s.last[tid];
    a.st.len[r] = s.len[tid];
  }
  if (tid == 0) {
    a.st.nb[b] = s.nb;
    a.st.nnodes[b] = s.nnodes;
  }
}

__global__ __launch_bounds__(64) void ctc_lm_finish_kernel(CtcLmArgs a) {
  __shared__ CtcShared s;
  const int b = blockIdx.x;
  load_beam(s, a.st, b, a.c.beam);
  __syncthreads();
  ctc_finish(s, a.c.nodes + (long)b * a.c.max_nodes, a.c.tokens + (long)b * a.c.T, a.c.out_len + b,
             a.c.score + b, a.lm_score + b, a.c.T, a.c.max_nodes);
}

bool ctc_ok(int T, int V, int blank, int beam_size, int cutoff_top_k) {
  return T >= 0 && V >= 1 && V <= S2T_RNNT_LSTM_MAX_VOCAB && blank >= 0 && blank < V && beam_size >= 1 &&
         beam_size <= kMaxBeam && cutoff_top_k >= 1 && (cutoff_top_k < V ? cutoff_top_k : V) <= kMaxBeam;
}

bool lm_desc_ok(const S2tRnnLmDesc* d, int V) {
  return d && d->V == V && d->E >= 1 && d->E <= S2T_RNNT_LSTM_MAX_HIDDEN && d->H >= 4 &&
         d->H <= S2T_RNNT_LSTM_MAX_HIDDEN && d->H % 4 == 0 && d->num_layers >= 1 &&
         d->num_layers <= S2T_RNNT_LSTM_MAX_LAYERS;
}

int max_nodes_of(int T, int beam) { return 1 + T * beam; }   // the root, at most beam new nodes a frame

size_t nodes_bytes(int B, int T, int beam) {
  return align256(sizeof(CtcNode) * (size_t)B * max_nodes_of(T, beam));
}

struct CtcLmWorkspace {
  CtcNode* nodes;
  CtcState st;
  float *h[2], *c[2], *q[2];
  void* step;
  size_t bytes;
};

CtcLmWorkspace carve_ctc_lm(const S2tRnnLmDesc& d, int B, int T, int beam, void* base) {
  const size_t R = (size_t)B * beam, L = d.num_layers;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t n) {
    char* q = p + off;
    off += align256(n);
    return q;
  };
  auto f = [&](size_t n) { return reinterpret_cast<float*>(take(4 * n)); };
  auto i = [&](size_t n) { return reinterpret_cast<int*>(take(4 * n)); };
  CtcLmWorkspace w;
  w.nodes = reinterpret_cast<CtcNode*>(take(nodes_bytes(B, T, beam)));
  w.st = CtcState{f(R), f(R), f(R), i(R), i(R), i(R), i(B), i(B), i(R), i(R), i(R)};
  for (int s = 0; s < 2; ++s) {
    w.h[s] = f(L * R * d.H);
    w.c[s] = f(L * R * d.H);
    w.q[s] = f(R * d.V);
  }
  w.step = take((size_t)s2t_rnn_lm_step_workspace_bytes(&d, (int)R));
  w.bytes = off;
  return w;
}

// ------------------------------------------------------------------ the chunk-carried form
// A stream's beam and trie live in a caller-owned state buffer between calls.  A call that consumes
// frames ends by compacting the trie: the lowest common ancestor of the live nodes becomes the root,
// only the union of the paths from it to the live nodes survives (renumbered in ascending order of
// the old ids, so that parent id < child id still holds; the child lists filtered in their order),
// and the ancestor's depth is kept as the committed depth.  Nothing outside that subtree can be live
// again, and a sequence off those paths gets from a fresh node what it got from its old one: node
// ids enter results only through "is p + c live".  st.nnodes is then `kept`, and a row consumes its n
// frames only when kept + beam * n <= max_nodes: no node is ever written outside the array.
struct CtcStream {
  CtcNode *nodes, *stage;          // [B][max_nodes] the trie; where a compaction builds its successor
  int* map;                        // [B][max_nodes] old node id -> new id, -1: dropped
  CtcState st;                     // the beams; emit / parent / token with an LM only
  int *depth, *ovf;                // [B] the committed depth; the overflow bits
  long* eff;                       // [B] frames the current call consumes (the LM family's rounds read it)
  float *h, *c, *q;                // the LM's live copy (LM family)
  int* ctx;                        // [R] the live prefixes' context ids (n-gram family)
  int* bstate;                     // [R] the live prefixes' graph states and bias sums (bias families)
  float* bsum;
  size_t bytes;
};

CtcStream carve_ctc_stream(const S2tRnnLmDesc* lm, int B, int V, int beam, int max_nodes, void* base,
                           bool ngram = false, bool bias = false) {
  const size_t R = (size_t)B * beam, M = (size_t)B * max_nodes;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t n) {
    char* q = p + off;
    off += align256(n);
    return q;
  };
  auto f = [&](size_t n) { return reinterpret_cast<float*>(take(4 * n)); };
  auto i = [&](size_t n) { return reinterpret_cast<int*>(take(4 * n)); };
  CtcStream s{};
  s.nodes = reinterpret_cast<CtcNode*>(take(sizeof(CtcNode) * M));
  s.stage = reinterpret_cast<CtcNode*>(take(sizeof(CtcNode) * M));
  s.map = i(M);
  s.st = CtcState{f(R), f(R), f(R), i(R), i(R), i(R), i(B), i(B), nullptr, nullptr, nullptr};
  s.depth = i(B);
  s.ovf = i(B);
  s.eff = reinterpret_cast<long*>(take(sizeof(long) * (size_t)B));
  if (lm) {
    s.st.emit = i(R);
    s.st.parent = i(R);
    s.st.token = i(R);
    s.h = f((size_t)lm->num_layers * R * lm->H);
    s.c = f((size_t)lm->num_layers * R * lm->H);
    s.q = f(R * V);
  }
  if (ngram) s.ctx = i(R);                                 // (behind the plain layout, which it leaves as it is)
  if (bias) {                                              // (behind either, likewise)
    s.bstate = i(R);
    s.bsum = f(R);
  }
  s.bytes = off;
  return s;
}

struct CtcLmStreamWorkspace {      // the second copy of the LM's state, the LM step's scratch
  float *h, *c, *q;
  void* step;
  size_t bytes;
};

CtcLmStreamWorkspace carve_ctc_lm_stream_ws(const S2tRnnLmDesc& d, int B, int beam, void* base) {
  const size_t R = (size_t)B * beam;
  char* p = static_cast<char*>(base);
  CtcLmStreamWorkspace w;
  size_t off = 0;
  auto f = [&](size_t n) {
    char* q = p + off;
    off += align256(4 * n);
    return reinterpret_cast<float*>(q);
  };
  w.h = f((size_t)d.num_layers * R * d.H);
  w.c = f((size_t)d.num_layers * R * d.H);
  w.q = f(R * d.V);
  w.step = p + off;
  off += align256((size_t)s2t_rnn_lm_step_workspace_bytes(&d, (int)R));
  w.bytes = off;
  return w;
}

struct CtcStreamArgs {
  CtcArgs c;                       // lengths: chunk_len, T: Tc, nodes: the state's, tokens [B][max_tokens]
  CtcState st;
  CtcNode* stage;
  int *map, *depth, *ovf;
  long* eff;
  int max_tokens;
  float* lm_score;                 // NULL: the plain family
  long* stable_len;
  int* overflow;
};

// frames row b consumes in this call: 0 for an idle row, an inert one, and one whose nodes do not fit
// (which then becomes inert: bit 1)
__device__ __forceinline__ int ctc_stream_admit(const CtcStreamArgs& a, int b) {
  const int n = (int)clamped_len(a.c.lengths, b, a.c.T);
  const int ovf = a.ovf[b];
  const long need = (long)a.st.nnodes[b] + (long)a.c.beam * n;
  __syncthreads();                                         // (every thread has read what thread 0 may write)
  if (n <= 0 || (ovf & 2)) return 0;
  if (need <= a.c.max_nodes) return n;
  if (threadIdx.x == 0) {
    a.ovf[b] = ovf | 2;
    a.overflow[b] = ovf | 2;
  }
  return 0;
}

// After the last frame of a call, beam in s: the outputs, then the compaction.  All kCtcThreads
// threads call it.  Every walk is bounded by the node count: a corrupt state ends in a wrong answer.
// pos: the beam position the outputs report (the bias families' finalisation; it enters nothing else).
struct CtcBiasHome {               // where the bias part of the beam goes home
  const CtcBiasShared* bs;
  int* bstate;
  float* bsum;
};

__device__ __forceinline__ void ctc_stream_close(CtcShared& s, CtcCompact& k, const CtcStreamArgs& a, int b,
                                                 const CtcNgramShared* ng = nullptr, int* ctx = nullptr,
                                                 CtcBiasHome bh = CtcBiasHome{nullptr, nullptr, nullptr},
                                                 int pos = 0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.c.max_nodes, nb = s.nb, nn = s.nnodes, BS = a.c.beam;
  CtcNode* nodes = a.c.nodes + (long)b * M;
  CtcNode* stage = a.stage + (long)b * M;
  int* map = a.map + (long)b * M;
  const int root_depth = a.depth[b];
  // ---- the best prefix: positions from the committed depth up (below it earlier calls wrote them)
  ctc_finish(s, nodes, a.c.tokens + (long)b * a.max_tokens, a.c.out_len + b, a.c.score + b,
             a.lm_score ? a.lm_score + b : nullptr, a.max_tokens, nn, pos);
  for (int id = tid; id < nn; id += kCtcThreads) map[id] = -1;
  // ---- the lowest common ancestor: a lane per live node, levelled to the shallowest, then up together
  if (wave == 0) {
    const int i = lane < nb ? lane : 0;
    int id = s.node[i], d = s.len[i], dmin = d;
    for (int o = 32; o; o >>= 1) dmin = min(dmin, __shfl_xor(dmin, o));
    for (int hop = 0; d > dmin && id > 0 && hop < nn; ++hop, --d) id = nodes[id].parent;
    bool same = false;
    for (int hop = 0; hop <= nn; ++hop) {
      same = __all(id == __shfl(id, 0)) != 0;
      if (same) break;
      if (id > 0) {
        id = nodes[id].parent;
        --d;
      }
    }
    if (lane == 0) {
      const bool ok = same && id >= 0 && id < nn;
      k.anc = ok ? id : 0;
      k.depth = ok ? d : root_depth;
    }
  }
  __syncthreads();
  const int anc = k.anc;
  // ---- mark the paths from the live nodes to it
  if (tid < nb) {
    int id = s.node[tid];
    for (int hop = 0; id > 0 && id < nn && id != anc && hop < nn; ++hop) {
      map[id] = 1;
      id = nodes[id].parent;
    }
  }
  __syncthreads();
  if (tid == 0) map[anc] = 1;
  __syncthreads();
  // ---- new ids: the marked nodes counted in ascending order of the old ones
  int kept = 0;
  for (int base = 0; base < nn; base += kCtcThreads) {
    const int id = base + tid;
    const bool on = id < nn && map[id] == 1;
    const unsigned long long m = __ballot(on);
    if (lane == 0) k.part[wave] = __popcll(m);
    __syncthreads();
    int mine = kept + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < kCtcWaves; ++w) {
      if (w < wave) mine += k.part[w];
      kept += k.part[w];
    }
    if (id < nn) map[id] = on ? mine : -1;
    __syncthreads();
  }
  // ---- the surviving nodes, their child lists filtered in order, into the staging copy
  for (int id = tid; id < nn; id += kCtcThreads) {
    const int nid = map[id];
    if (nid < 0) continue;
    const CtcNode o = nodes[id];
    CtcNode nw{-1, -1, -1, -1};
    int ch = o.first_child;
    for (int hop = 0; ch >= 0 && ch < nn && map[ch] < 0; ++hop) ch = hop < nn ? nodes[ch].next_sibling : -1;
    nw.first_child = ch >= 0 && ch < nn ? map[ch] : -1;
    if (id != anc) {
      nw.parent = o.parent >= 0 && o.parent < nn ? map[o.parent] : -1;
      nw.token = o.token;
      int sb = o.next_sibling;
      for (int hop = 0; sb >= 0 && sb < nn && map[sb] < 0; ++hop) sb = hop < nn ? nodes[sb].next_sibling : -1;
      nw.next_sibling = sb >= 0 && sb < nn ? map[sb] : -1;
    }
    stage[nid] = nw;
  }
  __syncthreads();
  for (int id = tid; id < kept; id += kCtcThreads) nodes[id] = stage[id];
  // ---- the beam goes home under its new node ids
  if (tid < nb) {
    const int r = b * BS + tid, id = s.node[tid];
    const int nid = id >= 0 && id < nn ? map[id] : -1;
    a.st.pb[r] = s.pb[tid];
    a.st.pnb[r] = s.pnb[tid];
    a.st.lm_sum[r] = s.lm_sum[tid];
    a.st.node[r] = nid < 0 ? 0 : nid;
    a.st.last[r] = s.last[tid];
    a.st.len[r] = s.len[tid];
    if (ng) ctx[r] = ng->state[tid];                       // (a context id belongs to a beam position, not to a node)
    if (bh.bs) {
      bh.bstate[r] = bh.bs->state[tid];
      bh.bsum[r] = bh.bs->sum[tid];
    }
  }
  if (tid == 0) {
    const int ovf = a.ovf[b] | (s.len[0] > a.max_tokens || s.len[pos] > a.max_tokens ? 1 : 0);
    a.st.nb[b] = nb;
    a.st.nnodes[b] = kept;
    a.depth[b] = k.depth;
    a.ovf[b] = ovf;
    a.overflow[b] = ovf;
    a.stable_len[b] = min(k.depth, a.max_tokens);
  }
}

// grid B: rows[b] != 0 (NULL: every row) becomes the empty prefix; with an LM its state is zeroed and
// the first LM step is asked for on row 0 of exactly those utterances; with an n-gram (ctx) the one live
// prefix starts in start_ctx; with a graph (bstate) in its root with nothing lent
__global__ __launch_bounds__(kCtcThreads) void ctc_stream_reset_kernel(CtcStreamArgs a, const int* rows,
                                                                       int lm_start_token, int layers, int H,
                                                                       float* h, float* c, float* q, int* ctx,
                                                                       int start_ctx, int* bstate = nullptr,
                                                                       float* bsum = nullptr) {
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.c.beam, r = b * BS + tid;
  const long R = (long)gridDim.x * BS;
  const bool on = !rows || rows[b] != 0;
  if (a.st.emit && tid < BS) {
    a.st.emit[r] = on && tid == 0;
    a.st.parent[r] = r;
    a.st.token[r] = lm_start_token < 0 ? 0 : lm_start_token;
  }
  if (!on) return;
  if (tid < BS) {
    a.st.pb[r] = tid == 0 ? 0.f : S2T_NEG_INF;
    a.st.pnb[r] = S2T_NEG_INF;
    a.st.lm_sum[r] = 0.f;
    a.st.node[r] = 0;
    a.st.last[r] = -1;
    a.st.len[r] = 0;
    if (ctx) ctx[r] = start_ctx;
    if (bstate) {
      bstate[r] = 0;
      bsum[r] = 0.f;
    }
  }
  if (tid == 0) {
    a.st.nb[b] = 1;
    a.st.nnodes[b] = 1;
    a.depth[b] = 0;
    a.ovf[b] = 0;
    a.eff[b] = 0;
    a.c.nodes[(long)b * a.c.max_nodes] = CtcNode{-1, -1, -1, -1};
  }
  if (!h) return;
  for (int l = 0; l < layers; ++l)
    for (int x = tid; x < BS * H; x += kCtcThreads) {
      h[(l * R + (long)b * BS) * H + x] = 0.f;
      c[(l * R + (long)b * BS) * H + x] = 0.f;
    }
  for (long x = tid; x < (long)BS * a.c.V; x += kCtcThreads) q[(long)b * BS * a.c.V + x] = 0.f;
}

// the plain family: ONE launch, a workgroup per utterance, like ctc_prefix_kernel
__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_chunk_kernel(CtcStreamArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  __shared__ CtcCompact k;
  const int b = blockIdx.x;
  const int n = ctc_stream_admit(a, b);
  if (n == 0) return;
  CtcNode* nodes = a.c.nodes + (long)b * a.c.max_nodes;
  const float* x = a.c.logits + (long)b * a.c.T * a.c.V;
  load_beam(s, a.st, b, a.c.beam);
  __syncthreads();
  const int K = min(a.c.topk, a.c.V);
  for (int t = 0; t < n; ++t)
    ctc_frame<kCtcPlain>(s, row, x + (long)t * a.c.V, a.c.V, K, a.c.beam, a.c.blank, nodes, a.c.max_nodes, 0.f,
                         nullptr, nullptr, nullptr, nullptr, 0);
  ctc_stream_close(s, k, a, b);
}

// the n-gram family: the same launch in the frame body's n-gram mode; the context ids are loaded with the
// beam (clamped: the reset that wrote them saw no tables) and go home with it
struct CtcNgramStreamArgs {
  CtcStreamArgs s;
  NgramTables g;
  float lm_weight;
  int* ctx;                        // [B][beam]
};

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_ngram_chunk_kernel(CtcNgramStreamArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  __shared__ CtcNgramShared ng;
  __shared__ CtcCompact k;
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.s.c.beam;
  const int n = ctc_stream_admit(a.s, b);
  if (n == 0) return;
  CtcNode* nodes = a.s.c.nodes + (long)b * a.s.c.max_nodes;
  const float* x = a.s.c.logits + (long)b * a.s.c.T * a.s.c.V;
  load_beam(s, a.s.st, b, BS);
  if (tid < BS) ng.state[tid] = ngram_clamp(a.ctx[b * BS + tid], a.g.num_ctx);
  if (tid == 0) ng.g = a.g;
  __syncthreads();
  const int K = min(a.s.c.topk, a.s.c.V);
  for (int t = 0; t < n; ++t)
    ctc_frame<kCtcNgram>(s, row, x + (long)t * a.s.c.V, a.s.c.V, K, BS, a.s.c.blank, nodes, a.s.c.max_nodes,
                         a.lm_weight, nullptr, nullptr, nullptr, nullptr, 0, &ng);
  ctc_stream_close(s, k, a.s, b, &ng, a.ctx);
}

// the bias families: the two launches above with the frame body's bias switch on; the graph states and sums
// are loaded with the beam (clamped, like the context ids) and go home with it.  pos is thread 0's: it
// alone writes outputs.
struct CtcBiasStreamArgs {
  CtcNgramStreamArgs n;            // (g, lm_weight, ctx: the n-gram family only)
  NgramTables graph;
  const float* ctx_final;
  float bias_weight;
  int* bstate;                     // [B][beam]
  float* bsum;                     // [B][beam]
  float* bias_score;               // [B]
};

__device__ __forceinline__ void ctc_bias_load(CtcBiasShared& bs, const CtcBiasStreamArgs& a, int b, int BS) {
  const int tid = threadIdx.x;
  if (tid < BS) {
    bs.state[tid] = ngram_clamp(a.bstate[b * BS + tid], a.graph.num_ctx);
    bs.sum[tid] = a.bsum[b * BS + tid];
  }
  if (tid == 0) {
    bs.g = a.graph;
    bs.final = a.ctx_final;
  }
}

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_bias_chunk_kernel(CtcBiasStreamArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  __shared__ CtcBiasShared bs;
  __shared__ CtcCompact k;
  const CtcStreamArgs& sa = a.n.s;
  const int b = blockIdx.x, BS = sa.c.beam;
  const int n = ctc_stream_admit(sa, b);
  if (n == 0) return;
  CtcNode* nodes = sa.c.nodes + (long)b * sa.c.max_nodes;
  const float* x = sa.c.logits + (long)b * sa.c.T * sa.c.V;
  load_beam(s, sa.st, b, BS);
  ctc_bias_load(bs, a, b, BS);
  __syncthreads();
  const int K = min(sa.c.topk, sa.c.V);
  for (int t = 0; t < n; ++t)
    ctc_frame<kCtcPlain, true>(s, row, x + (long)t * sa.c.V, sa.c.V, K, BS, sa.c.blank, nodes, sa.c.max_nodes, 0.f,
                               nullptr, nullptr, nullptr, nullptr, 0, nullptr, &bs, a.bias_weight);
  int pos = 0;
  if (threadIdx.x == 0) pos = ctc_bias_pick<false>(s, bs, 0.f, a.bias_weight, a.bias_score + b);
  ctc_stream_close(s, k, sa, b, nullptr, nullptr, CtcBiasHome{&bs, a.bstate, a.bsum}, pos);
}

__global__ __launch_bounds__(kCtcThreads) void ctc_prefix_ngram_bias_chunk_kernel(CtcBiasStreamArgs a) {
  extern __shared__ float row[];
  __shared__ CtcShared s;
  __shared__ CtcNgramShared ng;
  __shared__ CtcBiasShared bs;
  __shared__ CtcCompact k;
  const CtcStreamArgs& sa = a.n.s;
  const int b = blockIdx.x, tid = threadIdx.x, BS = sa.c.beam;
  const int n = ctc_stream_admit(sa, b);
  if (n == 0) return;
  CtcNode* nodes = sa.c.nodes + (long)b * sa.c.max_nodes;
  const float* x = sa.c.logits + (long)b * sa.c.T * sa.c.V;
  load_beam(s, sa.st, b, BS);
  if (tid < BS) ng.state[tid] = ngram_clamp(a.n.ctx[b * BS + tid], a.n.g.num_ctx);
  if (tid == 0) ng.g = a.n.g;
  ctc_bias_load(bs, a, b, BS);
  __syncthreads();
  const int K = min(sa.c.topk, sa.c.V);
  for (int t = 0; t < n; ++t)
    ctc_frame<kCtcNgram, true>(s, row, x + (long)t * sa.c.V, sa.c.V, K, BS, sa.c.blank, nodes, sa.c.max_nodes,
                               a.n.lm_weight, nullptr, nullptr, nullptr, nullptr, 0, &ng, &bs, a.bias_weight);
  int pos = 0;
  if (tid == 0) pos = ctc_bias_pick<true>(s, bs, a.n.lm_weight, a.bias_weight, a.bias_score + b);
  ctc_stream_close(s, k, sa, b, &ng, a.n.ctx, CtcBiasHome{&bs, a.bstate, a.bsum}, pos);
}

// the LM family: what the rounds read as lengths, before them ...
__global__ __launch_bounds__(64) void ctc_stream_begin_kernel(CtcStreamArgs a) {
  const int b = blockIdx.x;
  const int n = ctc_stream_admit(a, b);
  if (threadIdx.x == 0) a.eff[b] = n;
}

// ... and outputs and compaction after them
__global__ __launch_bounds__(kCtcThreads) void ctc_stream_end_kernel(CtcStreamArgs a) {
  __shared__ CtcShared s;
  __shared__ CtcCompact k;
  const int b = blockIdx.x;
  if (a.eff[b] <= 0) return;
  load_beam(s, a.st, b, a.c.beam);
  __syncthreads();
  ctc_stream_close(s, k, a, b);
}

// after an odd Tc the survivors' LM state is in the workspace's copy: one launch takes it home
struct CtcCopyHomeArgs {
  const float* src[3];
  float* dst[3];
  long n[3];
};

__global__ __launch_bounds__(kCtcThreads) void ctc_lm_copy_home_kernel(CtcCopyHomeArgs a) {
  const long step = (long)gridDim.x * kCtcThreads, i0 = (long)blockIdx.x * kCtcThreads + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (long i = i0; i < a.n[k]; i += step) a.dst[k][i] = a.src[k][i];
}

bool ctc_stream_ok(int V, int beam_size, int max_nodes) {
  return V >= 1 && V <= S2T_RNNT_LSTM_MAX_VOCAB && beam_size >= 1 && beam_size <= kMaxBeam && max_nodes >= 1 &&
         max_nodes <= S2T_CTC_STREAM_MAX_NODES;
}

CtcStreamArgs stream_args(const CtcStream& s, const float* logits, const long* chunk_len, int Tc, int V, int blank,
                          int beam_size, int cutoff_top_k, int max_tokens, int max_nodes, long* tokens,
                          long* out_len, float* score, float* lm_score, long* stable_len, int* overflow) {
  return CtcStreamArgs{{logits, chunk_len, Tc, V, blank, beam_size, cutoff_top_k, max_nodes, s.nodes, tokens, out_len,
                        score},
                       s.st, s.stage, s.map, s.depth, s.ovf, s.eff, max_tokens, lm_score, stable_len, overflow};
}

}  // namespace

extern "C" {

long s2t_ctc_prefix_beam_workspace_bytes(int B, int T, int V, int beam_size) {
  if (B <= 0 || T < 0 || V < 1 || V > S2T_RNNT_LSTM_MAX_VOCAB || beam_size < 1 || beam_size > kMaxBeam) return 0;
  return (long)nodes_bytes(B, T, beam_size);
}

int s2t_ctc_prefix_beam(const float* logits, const long* lengths, int B, int T, int V, int blank,
                        int beam_size, int cutoff_top_k, void* workspace, long* tokens, long* out_len,
                        float* score, void* stream) {
  if (B <= 0) return 0;
  if (T <= 0 || !ctc_ok(T, V, blank, beam_size, cutoff_top_k) || !workspace) return -1;
  CtcArgs a{logits, lengths, T, V, blank, beam_size, cutoff_top_k, max_nodes_of(T, beam_size),
            static_cast<CtcNode*>(workspace), tokens, out_len, score};
  hipLaunchKernelGGL(ctc_prefix_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

long s2t_ctc_prefix_beam_ngram_workspace_bytes(int B, int T, int V, int beam_size) {
  return s2t_ctc_prefix_beam_workspace_bytes(B, T, V, beam_size);
}

int s2t_ctc_prefix_beam_ngram(const S2tNgramLmDesc* lm, const float* logits, const long* lengths, int B, int T,
                              int V, int blank, int beam_size, int cutoff_top_k, float lm_weight, int start_ctx,
                              void* workspace, long* tokens, long* out_len, float* score, float* lm_score,
                              void* stream) {
  if (B <= 0) return 0;
  if (T <= 0 || !ctc_ok(T, V, blank, beam_size, cutoff_top_k) || !ngram_desc_ok(lm) || lm->V != V || start_ctx < 0 ||
      start_ctx >= lm->num_ctx || !__builtin_isfinite(lm_weight) || !workspace)
    return -1;
  CtcNgramArgs a{{logits, lengths, T, V, blank, beam_size, cutoff_top_k, max_nodes_of(T, beam_size),
                  static_cast<CtcNode*>(workspace), tokens, out_len, score},
                 ngram_tables(*lm), lm_weight, start_ctx, lm_score};
  hipLaunchKernelGGL(ctc_prefix_ngram_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_prefix_beam_bias(const S2tContextGraphDesc* graph, const float* logits, const long* lengths, int B,
                             int T, int V, int blank, int beam_size, int cutoff_top_k, float bias_weight,
                             void* workspace, long* tokens, long* out_len, float* score, float* bias_score,
                             void* stream) {
  if (B <= 0) return 0;
  if (T <= 0 || !ctc_ok(T, V, blank, beam_size, cutoff_top_k) || !context_desc_ok(graph) || graph->V != V ||
      !__builtin_isfinite(bias_weight) || !bias_score || !workspace)
    return -1;
  CtcBiasArgs a{{{logits, lengths, T, V, blank, beam_size, cutoff_top_k, max_nodes_of(T, beam_size),
                  static_cast<CtcNode*>(workspace), tokens, out_len, score},
                 NgramTables{}, 0.f, 0, nullptr},
                context_tables(*graph), graph->ctx_final, bias_weight, bias_score};
  hipLaunchKernelGGL(ctc_prefix_bias_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_prefix_beam_ngram_bias(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph, const float* logits,
                                   const long* lengths, int B, int T, int V, int blank, int beam_size,
                                   int cutoff_top_k, float lm_weight, int start_ctx, float bias_weight,
                                   void* workspace, long* tokens, long* out_len, float* score, float* lm_score,
                                   float* bias_score, void* stream) {
  if (B <= 0) return 0;
  if (T <= 0 || !ctc_ok(T, V, blank, beam_size, cutoff_top_k) || !ngram_desc_ok(lm) || lm->V != V || start_ctx < 0 ||
      start_ctx >= lm->num_ctx || !__builtin_isfinite(lm_weight) || !context_desc_ok(graph) || graph->V != V ||
      !__builtin_isfinite(bias_weight) || !lm_score || !bias_score || !workspace)
    return -1;
  CtcBiasArgs a{{{logits, lengths, T, V, blank, beam_size, cutoff_top_k, max_nodes_of(T, beam_size),
                  static_cast<CtcNode*>(workspace), tokens, out_len, score},
                 ngram_tables(*lm), lm_weight, start_ctx, lm_score},
                context_tables(*graph), graph->ctx_final, bias_weight, bias_score};
  hipLaunchKernelGGL(ctc_prefix_ngram_bias_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V,
                     (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

long s2t_ctc_prefix_beam_lm_workspace_bytes(const S2tRnnLmDesc* lm, int B, int T, int V, int beam_size) {
  if (B <= 0 || T < 0 || V < 1 || V > S2T_RNNT_LSTM_MAX_VOCAB || beam_size < 1 || beam_size > kMaxBeam ||
      !lm_desc_ok(lm, V))
    return 0;
  return (long)carve_ctc_lm(*lm, B, T, beam_size, nullptr).bytes;
}

int s2t_ctc_prefix_beam_lm(const S2tRnnLmDesc* lm, const float* logits, const long* lengths, int B, int T,
                           int V, int blank, int beam_size, int cutoff_top_k, float lm_weight,
                           int lm_start_token, void* workspace, long* tokens, long* out_len, float* score,
                           float* lm_score, void* stream) {
  if (B <= 0) return 0;
  if (T <= 0 || !ctc_ok(T, V, blank, beam_size, cutoff_top_k) || !lm_desc_ok(lm, V) || lm_start_token >= V ||
      !__builtin_isfinite(lm_weight) || !workspace)
    return -1;
  hipStream_t st = (hipStream_t)stream;
  const int R = B * beam_size;
  const CtcLmWorkspace w = carve_ctc_lm(*lm, B, T, beam_size, workspace);
  const size_t lm_state = sizeof(float) * (size_t)lm->num_layers * R * lm->H;
  hipError_t e = hipMemsetAsync(w.h[0], 0, lm_state, st);
  if (e == hipSuccess) e = hipMemsetAsync(w.c[0], 0, lm_state, st);
  if (e == hipSuccess) e = hipMemsetAsync(w.q[0], 0, sizeof(float) * (size_t)R * V, st);
  if (e != hipSuccess) return (int)e;
  CtcLmArgs a{{logits, lengths, T, V, blank, beam_size, cutoff_top_k, max_nodes_of(T, beam_size), w.nodes, tokens,
               out_len, score},
              w.st, w.q[0], lm_weight, 0, lm_start_token, lm_score};
  hipLaunchKernelGGL(ctc_lm_init_kernel, dim3(B), dim3(64), 0, st, a);
  if (lm_start_token >= 0) {                               // the LM's first step, on the start token
    const int rc = s2t_rnn_lm_step(lm, R, w.st.token, w.st.emit, nullptr, w.h[0], w.c[0], w.q[0], w.h[0], w.c[0],
                                   w.q[0], w.step, stream);
    if (rc != 0) return rc;
  }
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    a.t = t;
    a.q = w.q[cur];
    hipLaunchKernelGGL(ctc_prefix_round_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V, st, a);
    if (t + 1 == T) break;                                 // (nothing reads the LM after the last frame)
    const int rc = s2t_rnn_lm_step(lm, R, w.st.token, w.st.emit, w.st.parent, w.h[cur], w.c[cur], w.q[cur],
                                   w.h[cur ^ 1], w.c[cur ^ 1], w.q[cur ^ 1], w.step, stream);
    if (rc != 0) return rc;
    cur ^= 1;
  }
  hipLaunchKernelGGL(ctc_lm_finish_kernel, dim3(B), dim3(64), 0, st, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ the chunk-carried entries
long s2t_ctc_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  if (B <= 0 || !ctc_stream_ok(V, beam_size, max_nodes)) return 0;
  return (long)carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, nullptr).bytes;
}

int s2t_ctc_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes, void* stream) {
  if (B <= 0) return 0;
  if (!ctc_stream_ok(V, beam_size, max_nodes) || !state) return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state);
  const CtcStreamArgs a = stream_args(s, nullptr, nullptr, 0, V, 0, beam_size, 1, 1, max_nodes, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3(B), dim3(kCtcThreads), 0, (hipStream_t)stream, a, rows, -1, 0, 0,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, (int*)nullptr, 0);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_prefix_beam_chunk(const float* logits, const long* chunk_len, int B, int Tc, int V, int blank,
                              int beam_size, int cutoff_top_k, int max_tokens, int max_nodes, void* state,
                              long* tokens, long* out_len, float* score, long* stable_len, int* overflow,
                              void* stream) {
  if (B <= 0) return 0;
  if (Tc < 1 || Tc > 256 || !ctc_ok(Tc, V, blank, beam_size, cutoff_top_k) || max_tokens < 1 ||
      !ctc_stream_ok(V, beam_size, max_nodes) || !state)
    return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state);
  const CtcStreamArgs a = stream_args(s, logits, chunk_len, Tc, V, blank, beam_size, cutoff_top_k, max_tokens,
                                      max_nodes, tokens, out_len, score, nullptr, stable_len, overflow);
  hipLaunchKernelGGL(ctc_prefix_chunk_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V, (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

long s2t_ctc_ngram_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  if (B <= 0 || !ctc_stream_ok(V, beam_size, max_nodes)) return 0;
  return (long)carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, nullptr, true).bytes;
}

int s2t_ctc_ngram_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                               int start_ctx, void* stream) {
  if (B <= 0) return 0;
  if (!ctc_stream_ok(V, beam_size, max_nodes) || start_ctx < 0 || !state) return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state, true);
  const CtcStreamArgs a = stream_args(s, nullptr, nullptr, 0, V, 0, beam_size, 1, 1, max_nodes, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3(B), dim3(kCtcThreads), 0, (hipStream_t)stream, a, rows, -1, 0, 0,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, s.ctx, start_ctx);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_prefix_beam_ngram_chunk(const S2tNgramLmDesc* lm, const float* logits, const long* chunk_len, int B,
                                    int Tc, int V, int blank, int beam_size, int cutoff_top_k, float lm_weight,
                                    int max_tokens, int max_nodes, void* state, long* tokens, long* out_len,
                                    float* score, float* lm_score, long* stable_len, int* overflow, void* stream) {
  if (B <= 0) return 0;
  if (Tc < 1 || Tc > 256 || !ctc_ok(Tc, V, blank, beam_size, cutoff_top_k) || max_tokens < 1 ||
      !ctc_stream_ok(V, beam_size, max_nodes) || !ngram_desc_ok(lm) || lm->V != V ||
      !__builtin_isfinite(lm_weight) || !lm_score || !state)
    return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state, true);
  const CtcNgramStreamArgs a{stream_args(s, logits, chunk_len, Tc, V, blank, beam_size, cutoff_top_k, max_tokens,
                                         max_nodes, tokens, out_len, score, lm_score, stable_len, overflow),
                             ngram_tables(*lm), lm_weight, s.ctx};
  hipLaunchKernelGGL(ctc_prefix_ngram_chunk_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V,
                     (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

long s2t_ctc_bias_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  if (B <= 0 || !ctc_stream_ok(V, beam_size, max_nodes)) return 0;
  return (long)carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, nullptr, false, true).bytes;
}

long s2t_ctc_ngram_bias_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  if (B <= 0 || !ctc_stream_ok(V, beam_size, max_nodes)) return 0;
  return (long)carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, nullptr, true, true).bytes;
}

int s2t_ctc_bias_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                              void* stream) {
  if (B <= 0) return 0;
  if (!ctc_stream_ok(V, beam_size, max_nodes) || !state) return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state, false, true);
  const CtcStreamArgs a = stream_args(s, nullptr, nullptr, 0, V, 0, beam_size, 1, 1, max_nodes, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3(B), dim3(kCtcThreads), 0, (hipStream_t)stream, a, rows, -1, 0, 0,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, (int*)nullptr, 0, s.bstate, s.bsum);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_ngram_bias_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                                    int start_ctx, void* stream) {
  if (B <= 0) return 0;
  if (!ctc_stream_ok(V, beam_size, max_nodes) || start_ctx < 0 || !state) return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state, true, true);
  const CtcStreamArgs a = stream_args(s, nullptr, nullptr, 0, V, 0, beam_size, 1, 1, max_nodes, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3(B), dim3(kCtcThreads), 0, (hipStream_t)stream, a, rows, -1, 0, 0,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, s.ctx, start_ctx, s.bstate, s.bsum);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_prefix_beam_bias_chunk(const S2tContextGraphDesc* graph, const float* logits, const long* chunk_len,
                                   int B, int Tc, int V, int blank, int beam_size, int cutoff_top_k,
                                   float bias_weight, int max_tokens, int max_nodes, void* state, long* tokens,
                                   long* out_len, float* score, float* bias_score, long* stable_len, int* overflow,
                                   void* stream) {
  if (B <= 0) return 0;
  if (Tc < 1 || Tc > 256 || !ctc_ok(Tc, V, blank, beam_size, cutoff_top_k) || max_tokens < 1 ||
      !ctc_stream_ok(V, beam_size, max_nodes) || !context_desc_ok(graph) || graph->V != V ||
      !__builtin_isfinite(bias_weight) || !bias_score || !state)
    return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state, false, true);
  const CtcBiasStreamArgs a{{stream_args(s, logits, chunk_len, Tc, V, blank, beam_size, cutoff_top_k, max_tokens,
                                         max_nodes, tokens, out_len, score, nullptr, stable_len, overflow),
                             NgramTables{}, 0.f, nullptr},
                            context_tables(*graph), graph->ctx_final, bias_weight, s.bstate, s.bsum, bias_score};
  hipLaunchKernelGGL(ctc_prefix_bias_chunk_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V,
                     (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_prefix_beam_ngram_bias_chunk(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                         const float* logits, const long* chunk_len, int B, int Tc, int V, int blank,
                                         int beam_size, int cutoff_top_k, float lm_weight, float bias_weight,
                                         int max_tokens, int max_nodes, void* state, long* tokens, long* out_len,
                                         float* score, float* lm_score, float* bias_score, long* stable_len,
                                         int* overflow, void* stream) {
  if (B <= 0) return 0;
  if (Tc < 1 || Tc > 256 || !ctc_ok(Tc, V, blank, beam_size, cutoff_top_k) || max_tokens < 1 ||
      !ctc_stream_ok(V, beam_size, max_nodes) || !ngram_desc_ok(lm) || lm->V != V ||
      !__builtin_isfinite(lm_weight) || !lm_score || !context_desc_ok(graph) || graph->V != V ||
      !__builtin_isfinite(bias_weight) || !bias_score || !state)
    return -1;
  const CtcStream s = carve_ctc_stream(nullptr, B, V, beam_size, max_nodes, state, true, true);
  const CtcBiasStreamArgs a{{stream_args(s, logits, chunk_len, Tc, V, blank, beam_size, cutoff_top_k, max_tokens,
                                         max_nodes, tokens, out_len, score, lm_score, stable_len, overflow),
                             ngram_tables(*lm), lm_weight, s.ctx},
                            context_tables(*graph), graph->ctx_final, bias_weight, s.bstate, s.bsum, bias_score};
  hipLaunchKernelGGL(ctc_prefix_ngram_bias_chunk_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V,
                     (hipStream_t)stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

long s2t_ctc_lm_stream_state_bytes(const S2tRnnLmDesc* lm, int B, int V, int beam_size, int max_nodes) {
  if (B <= 0 || !ctc_stream_ok(V, beam_size, max_nodes) || !lm_desc_ok(lm, V)) return 0;
  return (long)carve_ctc_stream(lm, B, V, beam_size, max_nodes, nullptr).bytes;
}

long s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(const S2tRnnLmDesc* lm, int B, int V, int beam_size) {
  if (B <= 0 || !ctc_stream_ok(V, beam_size, 1) || !lm_desc_ok(lm, V)) return 0;
  return (long)carve_ctc_lm_stream_ws(*lm, B, beam_size, nullptr).bytes;
}

int s2t_ctc_lm_stream_reset(const S2tRnnLmDesc* lm, int lm_start_token, void* state, const int* rows, int B, int V,
                            int beam_size, int max_nodes, void* workspace, void* stream) {
  if (B <= 0) return 0;
  if (!ctc_stream_ok(V, beam_size, max_nodes) || !lm_desc_ok(lm, V) || lm_start_token >= V || !state || !workspace)
    return -1;
  const CtcStream s = carve_ctc_stream(lm, B, V, beam_size, max_nodes, state);
  const CtcLmStreamWorkspace w = carve_ctc_lm_stream_ws(*lm, B, beam_size, workspace);
  const CtcStreamArgs a = stream_args(s, nullptr, nullptr, 0, V, 0, beam_size, 1, 1, max_nodes, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3(B), dim3(kCtcThreads), 0, (hipStream_t)stream, a, rows,
                     lm_start_token, lm->num_layers, lm->H, s.h, s.c, s.q, (int*)nullptr, 0);
  if (lm_start_token >= 0) {                               // the one-shot entry's own first step, masked by rows
    const int rc = s2t_rnn_lm_step(lm, B * beam_size, s.st.token, s.st.emit, nullptr, s.h, s.c, s.q, s.h, s.c, s.q,
                                   w.step, stream);
    if (rc != 0) return rc;
  }
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_ctc_prefix_beam_lm_chunk(const S2tRnnLmDesc* lm, const float* logits, const long* chunk_len, int B, int Tc,
                                 int V, int blank, int beam_size, int cutoff_top_k, float lm_weight,
                                 int lm_start_token, int max_tokens, int max_nodes, void* state, void* workspace,
                                 long* tokens, long* out_len, float* score, float* lm_score, long* stable_len,
                                 int* overflow, void* stream) {
  if (B <= 0) return 0;
  if (Tc < 1 || Tc > 256 || !ctc_ok(Tc, V, blank, beam_size, cutoff_top_k) || max_tokens < 1 ||
      !ctc_stream_ok(V, beam_size, max_nodes) || !lm_desc_ok(lm, V) || lm_start_token >= V ||
      !__builtin_isfinite(lm_weight) || !state || !workspace)
    return -1;
  hipStream_t st = (hipStream_t)stream;
  const int R = B * beam_size;
  const CtcStream s = carve_ctc_stream(lm, B, V, beam_size, max_nodes, state);
  const CtcLmStreamWorkspace w = carve_ctc_lm_stream_ws(*lm, B, beam_size, workspace);
  const CtcStreamArgs sa = stream_args(s, logits, chunk_len, Tc, V, blank, beam_size, cutoff_top_k, max_tokens,
                                       max_nodes, tokens, out_len, score, lm_score, stable_len, overflow);
  hipLaunchKernelGGL(ctc_stream_begin_kernel, dim3(B), dim3(64), 0, st, sa);
  CtcLmArgs a{sa.c, s.st, s.q, lm_weight, 0, lm_start_token, lm_score};
  a.c.lengths = s.eff;                                     // the rounds walk the frames this call consumes
  float *h[2] = {s.h, w.h}, *c[2] = {s.c, w.c}, *q[2] = {s.q, w.q};
  int cur = 0;
  for (int t = 0; t < Tc; ++t) {
    a.t = t;
    a.q = q[cur];
    hipLaunchKernelGGL(ctc_prefix_round_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * V, st, a);
    const int rc = s2t_rnn_lm_step(lm, R, s.st.token, s.st.emit, s.st.parent, h[cur], c[cur], q[cur], h[cur ^ 1],
                                   c[cur ^ 1], q[cur ^ 1], w.step, stream);   // (also after the last frame: the
    if (rc != 0) return rc;                                                   // next chunk's frame 0 reads it)
    cur ^= 1;
  }
  if (cur) {
    const long ns = (long)lm->num_layers * R * lm->H, nq = (long)R * V;
    const CtcCopyHomeArgs cp{{w.h, w.c, w.q}, {s.h, s.c, s.q}, {ns, ns, nq}};
    const long most = ns > nq ? ns : nq, need = (most + kCtcThreads - 1) / kCtcThreads;
    hipLaunchKernelGGL(ctc_lm_copy_home_kernel, dim3((int)(need < 1024 ? need : 1024)), dim3(kCtcThreads), 0, st, cp);
  }
  hipLaunchKernelGGL(ctc_stream_end_kernel, dim3(B), dim3(kCtcThreads), 0, st, sa);
  S2T_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
