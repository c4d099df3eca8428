// CTC prefix beam search, lexicon-free, with equal prefixes merged exactly, for gfx950.  (The reference's
// CTC beam decoder wraps a lexicon decoder of a library; this is the textbook prefix search over the
// model's own classes.)  The per-frame body, the trie that gives a token sequence one node id for ever
// and the candidate slots are csrc/decode_ctc.h.  Around that body this file states each thing once:
//
//   ctc_search_kernel<MODE, BIAS, CHUNK>
//                  the ONE-launch searches: a workgroup (4 waves) per utterance walks its frames on the
//                  device, the beam in LDS, the trie in the workspace or the caller's state.  MODE: plain
//                  or back-off n-gram; BIAS: the hotword graph; CHUNK: the beam is loaded from a
//                  caller-owned state and goes home through ctc_stream_close (outputs, then the trie's
//                  compaction) instead of starting empty and ending in ctc_finish.  Eight instantiations
//                  behind s2t_ctc_prefix_beam[_ngram][_bias][_chunk]; one that has no n-gram, graph or
//                  state has no LDS, load or store of theirs.  All take one CtcSearchArgs.
//   ctc_search     the host path of those eight entries: the refusals, the argument struct filled by
//                  name, the instantiation, the launch.  An entry only describes its call (CtcSearch).
//   ctc_reset      likewise for the five s2t_ctc_*_stream_reset entries and ctc_stream_reset_kernel.
//   ctc_lm_rounds  the RNN-LM family (s2t_ctc_prefix_beam_lm, _lm_chunk): lockstep rounds over the batch
//                  and no host synchronisation; per round ctc_prefix_round_kernel (the same frame body; it
//                  gathers the q[c] it needs from the live prefixes' LM rows and writes emit / parent /
//                  token), then s2t_rnn_lm_step on B * beam_size rows from one copy of the LM's state
//                  into the other, then the flip.  A row past its length passes its state through.
//   carve_*        every workspace and state layout, handed out by the Arena of decode_records.h, which
//                  also answers the *_bytes queries.
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

struct CtcLmCopies {               // the two copies of the LM's state the rounds alternate between
  float *h[2], *c[2], *q[2];
  void* step;                      // s2t_rnn_lm_step's scratch
};

struct CtcLmWorkspace {
  CtcNode* nodes;
  CtcState st;
  CtcLmCopies lm;
};

CtcLmWorkspace carve_ctc_lm(const S2tRnnLmDesc& d, int B, int T, int beam, Arena& m) {
  const size_t R = (size_t)B * beam, L = d.num_layers;
  auto f = [&](size_t n) { return m.take<float>(n); };
  auto i = [&](size_t n) { return m.take<int>(n); };
  CtcLmWorkspace w;
  w.nodes = m.take<CtcNode>((size_t)B * max_nodes_of(T, beam));
  w.st = CtcState{f(R), f(R), f(R), i(R), i(R), i(R), i(B), i(B), i(R), i(R), i(R)};
  for (int s = 0; s < 2; ++s) {
    w.lm.h[s] = f(L * R * d.H);
    w.lm.c[s] = f(L * R * d.H);
    w.lm.q[s] = f(R * d.V);
  }
  w.lm.step = m.take<char>((size_t)s2t_rnn_lm_step_workspace_bytes(&d, (int)R));
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
};

CtcStream carve_ctc_stream(const S2tRnnLmDesc* lm, int B, int V, int beam, int max_nodes, Arena& m,
                           bool ngram = false, bool bias = false) {
  const size_t R = (size_t)B * beam, M = (size_t)B * max_nodes;
  auto f = [&](size_t n) { return m.take<float>(n); };
  auto i = [&](size_t n) { return m.take<int>(n); };
  CtcStream s{};
  s.nodes = m.take<CtcNode>(M);
  s.stage = m.take<CtcNode>(M);
  s.map = i(M);
  s.st = CtcState{f(R), f(R), f(R), i(R), i(R), i(R), i(B), i(B), nullptr, nullptr, nullptr};
  s.depth = i(B);
  s.ovf = i(B);
  s.eff = m.take<long>(B);
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
  return s;
}

struct CtcLmStreamWorkspace {      // the second copy of the LM's state, the LM step's scratch
  float *h, *c, *q;
  void* step;
};

CtcLmStreamWorkspace carve_ctc_lm_stream_ws(const S2tRnnLmDesc& d, int B, int beam, Arena& m) {
  const size_t R = (size_t)B * beam;
  CtcLmStreamWorkspace w;
  w.h = m.take<float>((size_t)d.num_layers * R * d.H);
  w.c = m.take<float>((size_t)d.num_layers * R * d.H);
  w.q = m.take<float>(R * d.V);
  w.step = m.take<char>((size_t)s2t_rnn_lm_step_workspace_bytes(&d, (int)R));
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

// grid B: rows[b] != 0 (NULL: every row) becomes the empty prefix; with an LM (s.h) its state is zeroed and
// the first LM step is asked for on row 0 of exactly those utterances; with an n-gram (s.ctx) the one live
// prefix starts in start_ctx; with a graph (s.bstate) in its root with nothing lent
struct CtcResetArgs {
  CtcStream s;                     // the state's arrays
  const int* rows;                 // [B] or NULL
  int V, beam, max_nodes;
  int lm_start_token, layers, H;   // (-1, 0, 0 without an LM)
  int start_ctx;
};

__global__ __launch_bounds__(kCtcThreads) void ctc_stream_reset_kernel(CtcResetArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.beam, r = b * BS + tid;
  const long R = (long)gridDim.x * BS;
  const CtcState& st = a.s.st;
  const bool on = !a.rows || a.rows[b] != 0;
  if (st.emit && tid < BS) {
    st.emit[r] = on && tid == 0;
    st.parent[r] = r;
    st.token[r] = a.lm_start_token < 0 ? 0 : a.lm_start_token;
  }
  if (!on) return;
  if (tid < BS) {
    st.pb[r] = tid == 0 ? 0.f : S2T_NEG_INF;
    st.pnb[r] = S2T_NEG_INF;
    st.lm_sum[r] = 0.f;
    st.node[r] = 0;
    st.last[r] = -1;
    st.len[r] = 0;
    if (a.s.ctx) a.s.ctx[r] = a.start_ctx;
    if (a.s.bstate) {
      a.s.bstate[r] = 0;
      a.s.bsum[r] = 0.f;
    }
  }
  if (tid == 0) {
    st.nb[b] = 1;
    st.nnodes[b] = 1;
    a.s.depth[b] = 0;
    a.s.ovf[b] = 0;
    a.s.eff[b] = 0;
    a.s.nodes[(long)b * a.max_nodes] = CtcNode{-1, -1, -1, -1};
  }
  if (!a.s.h) return;
  for (int l = 0; l < a.layers; ++l)
    for (int x = tid; x < BS * a.H; x += kCtcThreads) {
      a.s.h[(l * R + (long)b * BS) * a.H + x] = 0.f;
      a.s.c[(l * R + (long)b * BS) * a.H + x] = 0.f;
    }
  for (long x = tid; x < (long)BS * a.V; x += kCtcThreads) a.s.q[(long)b * BS * a.V + x] = 0.f;
}

// ------------------------------------------------------------------ the one-launch searches
// One struct for the eight instantiations; a part is read only by the instantiations that have it.
struct CtcSearchArgs {
  CtcStreamArgs s;                 // whole utterance: s.c and s.lm_score alone (c.lengths, c.T: the utterance's)
  // MODE == kCtcNgram
  NgramTables g;
  float lm_weight;
  int start_ctx;                   // whole utterance: the empty prefix' context
  int* ctx;                        // chunk: [B][beam] the live prefixes' contexts, in the state
  // BIAS
  NgramTables graph;
  const float* ctx_final;
  float bias_weight;
  int* bstate;                     // chunk: [B][beam] the live prefixes' graph states and sums, in the state
  float* bsum;
  float* bias_score;               // [B]
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

// the graph states and sums are loaded with the beam (clamped: the reset that wrote them saw no tables)
__device__ __forceinline__ void ctc_bias_load(CtcBiasShared& bs, const CtcSearchArgs& a, int b, int BS) {
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

// ONE launch, a workgroup per utterance.  The n-gram part, the bias part and the compaction's are LDS objects
// of the branches that use them: an instantiation without one reserves nothing for it.  The context ids,
// graph states and sums of a chunk call are loaded with the beam and go home with it; the bias
// instantiations report the position their finalisation picks (thread 0's: it alone writes outputs).
template <int MODE, bool BIAS, bool CHUNK>
__global__ __launch_bounds__(kCtcThreads) void ctc_search_kernel(CtcSearchArgs a) {
  constexpr bool NGRAM = MODE == kCtcNgram;
  extern __shared__ float row[];
  __shared__ CtcShared s;
  CtcNgramShared* ng = nullptr;
  CtcBiasShared* bs = nullptr;
  if constexpr (NGRAM) {
    __shared__ CtcNgramShared ngram_part;
    ng = &ngram_part;
  }
  if constexpr (BIAS) {
    __shared__ CtcBiasShared bias_part;
    bs = &bias_part;
  }
  const CtcArgs& c = a.s.c;
  const int b = blockIdx.x, tid = threadIdx.x, BS = c.beam;
  int n;
  if constexpr (CHUNK) {
    n = ctc_stream_admit(a.s, b);
    if (n == 0) return;
  } else {
    n = (int)clamped_len(c.lengths, b, c.T);
  }
  CtcNode* nodes = c.nodes + (long)b * c.max_nodes;
  const float* x = c.logits + (long)b * c.T * c.V;
  if constexpr (CHUNK) load_beam(s, a.s.st, b, BS);
  else ctc_start(s, nodes);
  if constexpr (NGRAM && CHUNK) {
    if (tid < BS) ng->state[tid] = ngram_clamp(a.ctx[b * BS + tid], a.g.num_ctx);
    if (tid == 0) ng->g = a.g;
  }
  if constexpr (NGRAM && !CHUNK) {
    if (tid == 0) {
      ng->g = a.g;
      ng->state[0] = a.start_ctx;
    }
  }
  if constexpr (BIAS && CHUNK) ctc_bias_load(*bs, a, b, BS);
  if constexpr (BIAS && !CHUNK) ctc_bias_start(*bs, a.graph, a.ctx_final);
  __syncthreads();
  const float lm_weight = NGRAM ? a.lm_weight : 0.f, bias_weight = BIAS ? a.bias_weight : 0.f;
  const int K = min(c.topk, c.V);
  for (int t = 0; t < n; ++t)
    ctc_frame<MODE, BIAS>(s, row, x + (long)t * c.V, c.V, K, BS, c.blank, nodes, c.max_nodes, lm_weight, nullptr,
                          nullptr, nullptr, nullptr, 0, ng, bs, bias_weight);
  int pos = 0;
  if constexpr (BIAS) {
    if (tid == 0) pos = ctc_bias_pick<NGRAM>(s, *bs, lm_weight, bias_weight, a.bias_score + b);
  }
  if constexpr (CHUNK) {
    __shared__ CtcCompact k;
    CtcBiasHome home{nullptr, nullptr, nullptr};
    if constexpr (BIAS) home = CtcBiasHome{bs, a.bstate, a.bsum};
    ctc_stream_close(s, k, a.s, b, ng, NGRAM ? a.ctx : nullptr, home, pos);
  } else {
    ctc_finish(s, nodes, c.tokens + (long)b * c.T, c.out_len + b, c.score + b, NGRAM ? a.s.lm_score + b : nullptr,
               c.T, c.max_nodes, pos);
  }
}

using CtcSearchKernel = void (*)(CtcSearchArgs);
const CtcSearchKernel kCtcSearchKernels[2][2][2] = {   // [CHUNK][n-gram][BIAS]
    {{ctc_search_kernel<kCtcPlain, false, false>, ctc_search_kernel<kCtcPlain, true, false>},
     {ctc_search_kernel<kCtcNgram, false, false>, ctc_search_kernel<kCtcNgram, true, false>}},
    {{ctc_search_kernel<kCtcPlain, false, true>, ctc_search_kernel<kCtcPlain, true, true>},
     {ctc_search_kernel<kCtcNgram, false, true>, ctc_search_kernel<kCtcNgram, true, true>}}};

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

// the state's arrays a chunk call works on
void stream_part(CtcStreamArgs& a, const CtcStream& s) {
  a.c.nodes = s.nodes;
  a.st = s.st;
  a.stage = s.stage;
  a.map = s.map;
  a.depth = s.depth;
  a.ovf = s.ovf;
  a.eff = s.eff;
}

long stream_state_bytes(const S2tRnnLmDesc* lm, int B, int V, int beam, int max_nodes, bool ngram, bool bias) {
  if (B <= 0 || !ctc_stream_ok(V, beam, max_nodes)) return 0;
  return bytes_of([&](Arena& m) { carve_ctc_stream(lm, B, V, beam, max_nodes, m, ngram, bias); });
}

// ------------------------------------------------------------------ one host path for the one-launch searches
struct CtcSearch {                 // what an extern "C" search entry asks for
  const float* logits;
  const long* lengths;             // chunk: chunk_len
  int B, T, V, blank, beam, topk;  // chunk: T is Tc
  void* memory;                    // the workspace; chunk: the state
  long *tokens, *out_len;
  float* score;
  void* stream;
  bool chunk = false;
  int max_tokens = 0, max_nodes = 0;
  long* stable_len = nullptr;
  int* overflow = nullptr;
  bool ngram = false;
  const S2tNgramLmDesc* lm = nullptr;
  float lm_weight = 0.f;
  int start_ctx = 0;               // whole utterance only: a stream's is its reset's
  float* lm_score = nullptr;
  bool lm_score_may_be_null = false;   // s2t_ctc_prefix_beam_ngram alone has never refused a NULL lm_score
  bool bias = false;
  const S2tContextGraphDesc* graph = nullptr;
  float bias_weight = 0.f;
  float* bias_score = nullptr;
};

// the arguments every search entry has, in the order of its prototype
CtcSearch ctc_call(const float* logits, const long* lengths, int B, int T, int V, int blank, int beam, int topk,
                   void* memory, long* tokens, long* out_len, float* score, void* stream) {
  CtcSearch q;
  q.logits = logits, q.lengths = lengths;
  q.B = B, q.T = T, q.V = V, q.blank = blank, q.beam = beam, q.topk = topk;
  q.memory = memory, q.tokens = tokens, q.out_len = out_len, q.score = score, q.stream = stream;
  return q;
}

void chunk_part(CtcSearch& q, int max_tokens, int max_nodes, long* stable_len, int* overflow) {
  q.chunk = true;
  q.max_tokens = max_tokens, q.max_nodes = max_nodes, q.stable_len = stable_len, q.overflow = overflow;
}

void ngram_part(CtcSearch& q, const S2tNgramLmDesc* lm, float lm_weight, float* lm_score) {
  q.ngram = true;
  q.lm = lm, q.lm_weight = lm_weight, q.lm_score = lm_score;
}

void bias_part(CtcSearch& q, const S2tContextGraphDesc* graph, float bias_weight, float* bias_score) {
  q.bias = true;
  q.graph = graph, q.bias_weight = bias_weight, q.bias_score = bias_score;
}

int ctc_search(const CtcSearch& q) {
  if (q.B <= 0) return 0;
  bool ok = q.T >= 1 && ctc_ok(q.T, q.V, q.blank, q.beam, q.topk) && q.memory;
  if (q.chunk) ok = ok && q.T <= 256 && q.max_tokens >= 1 && ctc_stream_ok(q.V, q.beam, q.max_nodes);
  if (q.ngram) {
    ok = ok && ngram_desc_ok(q.lm) && q.lm->V == q.V && __builtin_isfinite(q.lm_weight) &&
         (q.lm_score || q.lm_score_may_be_null);
    if (!q.chunk) ok = ok && q.start_ctx >= 0 && q.start_ctx < q.lm->num_ctx;
  }
  if (q.bias)
    ok = ok && context_desc_ok(q.graph) && q.graph->V == q.V && __builtin_isfinite(q.bias_weight) && q.bias_score;
  if (!ok) return -1;
  CtcSearchArgs a{};
  CtcArgs& c = a.s.c;
  c.logits = q.logits;
  c.lengths = q.lengths;
  c.T = q.T;
  c.V = q.V;
  c.blank = q.blank;
  c.beam = q.beam;
  c.topk = q.topk;
  c.tokens = q.tokens;
  c.out_len = q.out_len;
  c.score = q.score;
  a.s.lm_score = q.lm_score;
  if (q.chunk) {
    Arena m(q.memory);
    const CtcStream s = carve_ctc_stream(nullptr, q.B, q.V, q.beam, q.max_nodes, m, q.ngram, q.bias);
    stream_part(a.s, s);
    c.max_nodes = q.max_nodes;
    a.s.max_tokens = q.max_tokens;
    a.s.stable_len = q.stable_len;
    a.s.overflow = q.overflow;
    a.ctx = s.ctx;
    a.bstate = s.bstate;
    a.bsum = s.bsum;
  } else {
    c.nodes = static_cast<CtcNode*>(q.memory);
    c.max_nodes = max_nodes_of(q.T, q.beam);
  }
  if (q.ngram) {
    a.g = ngram_tables(*q.lm);
    a.lm_weight = q.lm_weight;
    a.start_ctx = q.start_ctx;
  }
  if (q.bias) {
    a.graph = context_tables(*q.graph);
    a.ctx_final = q.graph->ctx_final;
    a.bias_weight = q.bias_weight;
    a.bias_score = q.bias_score;
  }
  hipLaunchKernelGGL(kCtcSearchKernels[q.chunk][q.ngram][q.bias], dim3(q.B), dim3(kCtcThreads), sizeof(float) * q.V,
                     (hipStream_t)q.stream, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ one host path for the resets
struct CtcReset {                  // what an extern "C" reset entry asks for
  void* state;
  const int* rows;
  int B, V, beam, max_nodes;
  void* stream;
  bool ngram = false, bias = false, rnn = false;
  int start_ctx = 0;
  const S2tRnnLmDesc* lm = nullptr;   // rnn: the LM, its start token, the chunk entry's workspace
  int lm_start_token = -1;
  void* workspace = nullptr;
};

CtcReset reset_call(void* state, const int* rows, int B, int V, int beam, int max_nodes, void* stream) {
  CtcReset q;
  q.state = state, q.rows = rows, q.B = B, q.V = V, q.beam = beam, q.max_nodes = max_nodes, q.stream = stream;
  return q;
}

int ctc_reset(const CtcReset& q) {
  if (q.B <= 0) return 0;
  bool ok = ctc_stream_ok(q.V, q.beam, q.max_nodes) && q.state && q.start_ctx >= 0;
  if (q.rnn) ok = ok && lm_desc_ok(q.lm, q.V) && q.lm_start_token < q.V && q.workspace;
  if (!ok) return -1;
  Arena m(q.state);
  CtcResetArgs a{};
  a.s = carve_ctc_stream(q.lm, q.B, q.V, q.beam, q.max_nodes, m, q.ngram, q.bias);
  a.rows = q.rows;
  a.V = q.V;
  a.beam = q.beam;
  a.max_nodes = q.max_nodes;
  a.lm_start_token = q.lm_start_token;
  a.layers = q.rnn ? q.lm->num_layers : 0;
  a.H = q.rnn ? q.lm->H : 0;
  a.start_ctx = q.start_ctx;
  hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3(q.B), dim3(kCtcThreads), 0, (hipStream_t)q.stream, a);
  if (q.rnn && q.lm_start_token >= 0) {                    // the one-shot entry's own first step, masked by rows
    Arena wm(q.workspace);
    const CtcLmStreamWorkspace w = carve_ctc_lm_stream_ws(*q.lm, q.B, q.beam, wm);
    const int rc = s2t_rnn_lm_step(q.lm, q.B * q.beam, a.s.st.token, a.s.st.emit, nullptr, a.s.h, a.s.c, a.s.q, a.s.h,
                                   a.s.c, a.s.q, w.step, q.stream);
    if (rc != 0) return rc;
  }
  S2T_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ the LM family's rounds
// Frames 0 .. T - 1 in lockstep over the batch: the round kernel reads the q rows of the live copy, then
// s2t_rnn_lm_step takes the state from it into the other copy, then the two flip.  step_after_last: the
// step also follows the last frame (a chunk call: the next chunk's frame 0 reads it; a whole utterance:
// nothing does).  *live: the copy the state is in afterwards.
int ctc_lm_rounds(const S2tRnnLmDesc* lm, CtcLmArgs& a, int B, int T, const CtcLmCopies& w, bool step_after_last,
                  void* stream, int* live) {
  const int R = B * a.c.beam;
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    a.t = t;
    a.q = w.q[cur];
    hipLaunchKernelGGL(ctc_prefix_round_kernel, dim3(B), dim3(kCtcThreads), sizeof(float) * a.c.V,
                       (hipStream_t)stream, a);
    if (t + 1 == T && !step_after_last) break;
    const int rc = s2t_rnn_lm_step(lm, R, a.st.token, a.st.emit, a.st.parent, w.h[cur], w.c[cur], w.q[cur],
                                   w.h[cur ^ 1], w.c[cur ^ 1], w.q[cur ^ 1], w.step, stream);
    if (rc != 0) return rc;
    cur ^= 1;
  }
  *live = cur;
  return 0;
}

}  // namespace

extern "C" {

long s2t_ctc_prefix_beam_workspace_bytes(int B, int T, int V, int beam_size) {
  if (B <= 0 || T < 0 || V < 1 || V > S2T_RNNT_LSTM_MAX_VOCAB || beam_size < 1 || beam_size > kMaxBeam) return 0;
  return (long)nodes_bytes(B, T, beam_size);
}

long s2t_ctc_prefix_beam_ngram_workspace_bytes(int B, int T, int V, int beam_size) {
  return s2t_ctc_prefix_beam_workspace_bytes(B, T, V, beam_size);
}

int s2t_ctc_prefix_beam(const float* logits, const long* lengths, int B, int T, int V, int blank,
                        int beam_size, int cutoff_top_k, void* workspace, long* tokens, long* out_len,
                        float* score, void* stream) {
  return ctc_search(ctc_call(logits, lengths, B, T, V, blank, beam_size, cutoff_top_k, workspace, tokens, out_len,
                             score, stream));
}

int s2t_ctc_prefix_beam_ngram(const S2tNgramLmDesc* lm, const float* logits, const long* lengths, int B, int T,
                              int V, int blank, int beam_size, int cutoff_top_k, float lm_weight, int start_ctx,
                              void* workspace, long* tokens, long* out_len, float* score, float* lm_score,
                              void* stream) {
  CtcSearch q = ctc_call(logits, lengths, B, T, V, blank, beam_size, cutoff_top_k, workspace, tokens, out_len, score,
                         stream);
  ngram_part(q, lm, lm_weight, lm_score);
  q.start_ctx = start_ctx;
  q.lm_score_may_be_null = true;
  return ctc_search(q);
}

int s2t_ctc_prefix_beam_bias(const S2tContextGraphDesc* graph, const float* logits, const long* lengths, int B,
                             int T, int V, int blank, int beam_size, int cutoff_top_k, float bias_weight,
                             void* workspace, long* tokens, long* out_len, float* score, float* bias_score,
                             void* stream) {
  CtcSearch q = ctc_call(logits, lengths, B, T, V, blank, beam_size, cutoff_top_k, workspace, tokens, out_len, score,
                         stream);
  bias_part(q, graph, bias_weight, bias_score);
  return ctc_search(q);
}

int s2t_ctc_prefix_beam_ngram_bias(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph, const float* logits,
                                   const long* lengths, int B, int T, int V, int blank, int beam_size,
                                   int cutoff_top_k, float lm_weight, int start_ctx, float bias_weight,
                                   void* workspace, long* tokens, long* out_len, float* score, float* lm_score,
                                   float* bias_score, void* stream) {
  CtcSearch q = ctc_call(logits, lengths, B, T, V, blank, beam_size, cutoff_top_k, workspace, tokens, out_len, score,
                         stream);
  ngram_part(q, lm, lm_weight, lm_score);
  q.start_ctx = start_ctx;
  bias_part(q, graph, bias_weight, bias_score);
  return ctc_search(q);
}

long s2t_ctc_prefix_beam_lm_workspace_bytes(const S2tRnnLmDesc* lm, int B, int T, int V, int beam_size) {
  if (B <= 0 || T < 0 || V < 1 || V > S2T_RNNT_LSTM_MAX_VOCAB || beam_size < 1 || beam_size > kMaxBeam ||
      !lm_desc_ok(lm, V))
    return 0;
  return bytes_of([&](Arena& m) { carve_ctc_lm(*lm, B, T, beam_size, m); });
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
  Arena m(workspace);
  const CtcLmWorkspace w = carve_ctc_lm(*lm, B, T, beam_size, m);
  const size_t lm_state = sizeof(float) * (size_t)lm->num_layers * R * lm->H;
  hipError_t e = hipMemsetAsync(w.lm.h[0], 0, lm_state, st);
  if (e == hipSuccess) e = hipMemsetAsync(w.lm.c[0], 0, lm_state, st);
  if (e == hipSuccess) e = hipMemsetAsync(w.lm.q[0], 0, sizeof(float) * (size_t)R * V, st);
  if (e != hipSuccess) return (int)e;
  CtcLmArgs a{{logits, lengths, T, V, blank, beam_size, cutoff_top_k, max_nodes_of(T, beam_size), w.nodes, tokens,
               out_len, score},
              w.st, w.lm.q[0], lm_weight, 0, lm_start_token, lm_score};
  hipLaunchKernelGGL(ctc_lm_init_kernel, dim3(B), dim3(64), 0, st, a);
  if (lm_start_token >= 0) {                               // the LM's first step, on the start token
    const int rc = s2t_rnn_lm_step(lm, R, w.st.token, w.st.emit, nullptr, w.lm.h[0], w.lm.c[0], w.lm.q[0], w.lm.h[0],
                                   w.lm.c[0], w.lm.q[0], w.lm.step, stream);
    if (rc != 0) return rc;
  }
  int live;
  const int rc = ctc_lm_rounds(lm, a, B, T, w.lm, false, stream, &live);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ctc_lm_finish_kernel, dim3(B), dim3(64), 0, st, a);
  S2T_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ the chunk-carried entries
long s2t_ctc_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  return stream_state_bytes(nullptr, B, V, beam_size, max_nodes, false, false);
}

long s2t_ctc_ngram_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  return stream_state_bytes(nullptr, B, V, beam_size, max_nodes, true, false);
}

long s2t_ctc_bias_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  return stream_state_bytes(nullptr, B, V, beam_size, max_nodes, false, true);
}

long s2t_ctc_ngram_bias_stream_state_bytes(int B, int V, int beam_size, int max_nodes) {
  return stream_state_bytes(nullptr, B, V, beam_size, max_nodes, true, true);
}

long s2t_ctc_lm_stream_state_bytes(const S2tRnnLmDesc* lm, int B, int V, int beam_size, int max_nodes) {
  return lm_desc_ok(lm, V) ? stream_state_bytes(lm, B, V, beam_size, max_nodes, false, false) : 0;
}

long s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(const S2tRnnLmDesc* lm, int B, int V, int beam_size) {
  if (B <= 0 || !ctc_stream_ok(V, beam_size, 1) || !lm_desc_ok(lm, V)) return 0;
  return bytes_of([&](Arena& m) { carve_ctc_lm_stream_ws(*lm, B, beam_size, m); });
}

int s2t_ctc_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes, void* stream) {
  return ctc_reset(reset_call(state, rows, B, V, beam_size, max_nodes, stream));
}

int s2t_ctc_ngram_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                               int start_ctx, void* stream) {
  CtcReset q = reset_call(state, rows, B, V, beam_size, max_nodes, stream);
  q.ngram = true;
  q.start_ctx = start_ctx;
  return ctc_reset(q);
}

int s2t_ctc_bias_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                              void* stream) {
  CtcReset q = reset_call(state, rows, B, V, beam_size, max_nodes, stream);
  q.bias = true;
  return ctc_reset(q);
}

int s2t_ctc_ngram_bias_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                                    int start_ctx, void* stream) {
  CtcReset q = reset_call(state, rows, B, V, beam_size, max_nodes, stream);
  q.ngram = q.bias = true;
  q.start_ctx = start_ctx;
  return ctc_reset(q);
}

int s2t_ctc_lm_stream_reset(const S2tRnnLmDesc* lm, int lm_start_token, void* state, const int* rows, int B, int V,
                            int beam_size, int max_nodes, void* workspace, void* stream) {
  CtcReset q = reset_call(state, rows, B, V, beam_size, max_nodes, stream);
  q.rnn = true;
  q.lm = lm;
  q.lm_start_token = lm_start_token;
  q.workspace = workspace;
  return ctc_reset(q);
}

int s2t_ctc_prefix_beam_chunk(const float* logits, const long* chunk_len, int B, int Tc, int V, int blank,
                              int beam_size, int cutoff_top_k, int max_tokens, int max_nodes, void* state,
                              long* tokens, long* out_len, float* score, long* stable_len, int* overflow,
                              void* stream) {
  CtcSearch q = ctc_call(logits, chunk_len, B, Tc, V, blank, beam_size, cutoff_top_k, state, tokens, out_len, score,
                         stream);
  chunk_part(q, max_tokens, max_nodes, stable_len, overflow);
  return ctc_search(q);
}

int s2t_ctc_prefix_beam_ngram_chunk(const S2tNgramLmDesc* lm, const float* logits, const long* chunk_len, int B,
                                    int Tc, int V, int blank, int beam_size, int cutoff_top_k, float lm_weight,
                                    int max_tokens, int max_nodes, void* state, long* tokens, long* out_len,
                                    float* score, float* lm_score, long* stable_len, int* overflow, void* stream) {
  CtcSearch q = ctc_call(logits, chunk_len, B, Tc, V, blank, beam_size, cutoff_top_k, state, tokens, out_len, score,
                         stream);
  chunk_part(q, max_tokens, max_nodes, stable_len, overflow);
  ngram_part(q, lm, lm_weight, lm_score);
  return ctc_search(q);
}

int s2t_ctc_prefix_beam_bias_chunk(const S2tContextGraphDesc* graph, const float* logits, const long* chunk_len,
                                   int B, int Tc, int V, int blank, int beam_size, int cutoff_top_k,
                                   float bias_weight, int max_tokens, int max_nodes, void* state, long* tokens,
                                   long* out_len, float* score, float* bias_score, long* stable_len, int* overflow,
                                   void* stream) {
  CtcSearch q = ctc_call(logits, chunk_len, B, Tc, V, blank, beam_size, cutoff_top_k, state, tokens, out_len, score,
                         stream);
  chunk_part(q, max_tokens, max_nodes, stable_len, overflow);
  bias_part(q, graph, bias_weight, bias_score);
  return ctc_search(q);
}

int s2t_ctc_prefix_beam_ngram_bias_chunk(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                         const float* logits, const long* chunk_len, int B, int Tc, int V, int blank,
                                         int beam_size, int cutoff_top_k, float lm_weight, float bias_weight,
                                         int max_tokens, int max_nodes, void* state, long* tokens, long* out_len,
                                         float* score, float* lm_score, float* bias_score, long* stable_len,
                                         int* overflow, void* stream) {
  CtcSearch q = ctc_call(logits, chunk_len, B, Tc, V, blank, beam_size, cutoff_top_k, state, tokens, out_len, score,
                         stream);
  chunk_part(q, max_tokens, max_nodes, stable_len, overflow);
  ngram_part(q, lm, lm_weight, lm_score);
  bias_part(q, graph, bias_weight, bias_score);
  return ctc_search(q);
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
  Arena sm(state), wm(workspace);
  const CtcStream s = carve_ctc_stream(lm, B, V, beam_size, max_nodes, sm);
  const CtcLmStreamWorkspace w = carve_ctc_lm_stream_ws(*lm, B, beam_size, wm);
  CtcStreamArgs sa{};
  sa.c = CtcArgs{logits, chunk_len, Tc, V, blank, beam_size, cutoff_top_k, max_nodes, s.nodes, tokens, out_len, score};
  stream_part(sa, s);
  sa.max_tokens = max_tokens;
  sa.lm_score = lm_score;
  sa.stable_len = stable_len;
  sa.overflow = overflow;
  hipLaunchKernelGGL(ctc_stream_begin_kernel, dim3(B), dim3(64), 0, st, sa);
  CtcLmArgs a{sa.c, s.st, s.q, lm_weight, 0, lm_start_token, lm_score};
  a.c.lengths = s.eff;                                     // the rounds walk the frames this call consumes
  const CtcLmCopies copies{{s.h, w.h}, {s.c, w.c}, {s.q, w.q}, w.step};
  int live;
  const int rc = ctc_lm_rounds(lm, a, B, Tc, copies, true, stream, &live);
  if (rc != 0) return rc;
  if (live) {                                              // (an odd Tc: the survivors' LM state is in the workspace)
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
