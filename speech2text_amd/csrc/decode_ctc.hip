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
#include <hip/hip_runtime.h>

#include "../../include/s2t_mi355.h"
#include "common.h"
#include "decode_ctc.h"

namespace {

using namespace s2t_dec;

static_assert(S2T_RNNT_LSTM_MAX_BEAM == kMaxBeam, "the header's limit is the kernels'");
static_assert(sizeof(float) * S2T_RNNT_LSTM_MAX_VOCAB + sizeof(CtcShared) <= 60 * 1024,
              "a frame's logits are staged in LDS whole");

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
    ctc_frame<false>(s, row, x + (long)t * a.V, a.V, K, a.beam, a.blank, nodes, a.max_nodes, 0.f, nullptr,
                     nullptr, nullptr, nullptr, 0);
  ctc_finish(s, nodes, a.tokens + (long)b * a.T, a.out_len + b, a.score + b, nullptr);
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
  ctc_frame<true>(s, row, a.c.logits + ((long)b * a.c.T + a.t) * a.c.V, a.c.V, min(a.c.topk, a.c.V), BS,
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
             a.c.score + b, a.lm_score + b);
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

}  // extern "C"
