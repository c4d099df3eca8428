// RNN-T greedy and beam search (reference model/decoding.py:196-271 RnntGreedyDecoding, :295-425
// RnntBeamDecoding) with the layer-norm LSTM predictor (model/predictor/lstm_predictor.py:28-109 ->
// torchaudio _Predictor / _CustomLSTM) and the joiner with or without output projection
// (model/joiner/joiner.py:186-207), for gfx950, float32 throughout.
//
// The reference walks one utterance and one lattice move at a time, a few dozen launches per move.
// Here the search runs in LOCKSTEP over the batch.  A "round" is one lattice move of every live row
// (greedy: a row per utterance; beam: beam_size rows per utterance):
//   joint     a workgroup per row: z = act(am[b, t_b] + lm[row]) (through the two out-projection
//             Linears when there are any) and the row's decision -- greedy: arg-max, first index on
//             ties, and the reference's bookkeeping; beam: log-softmax, the cutoff_top_k best classes,
//             then (a workgroup per utterance) candidate ranking, selection and trace-back records
//             in the orders of csrc/decode_rnnt.hip, by the functions both share
//             (csrc/decode_records.h).  Rows that emitted are counted on the device.
//   predictor for the rows that emitted: LN(embedding[token]); per layer the raw gates
//             x . x2g^T (+ bias) + h . p2g^T as (16 rows x 16 gate rows) tiles -- a weight matrix is
//             read once per round and row tile, not once per row -- then g_norm, i / f / cell / o,
//             c_norm, h per row; LN(linear(h_last)); pre_proj -> the row's lm vector.
// Launches are ordered by the stream alone (csrc/lstm_step.hip): no grid-wide barrier, no cooperative
// launch, no flag.  Every predictor launch reads the round's count first and returns on zero, so a
// round in which no row emitted costs its launches and nothing else.  Greedy rounds are enqueued in
// blocks of 32 with one host read of the "rows still live" counter per block; a beam search is
// exactly T rounds (at most one symbol per frame per beam) and never synchronises.
//
// The same rounds also run a chunk at a time on caller-owned state (s2t_rnnt_*_lstm_chunk, at the
// end of this file): the whole-utterance calls and the chunk calls enqueue them through the same
// host functions.  A beam chunk's records become histories and outputs by decode_records.h
// chunk_histories, the scheme csrc/decode_rnnt.hip keeps written out.
//
// RNN-LM shallow fusion (s2t_rnnt_beam_lstm_lm): a second recurrent model rides the beam rounds.  Every
// row also carries the LM's (h, c), q = log_softmax(logits(h_last)) [V] and the sum of the q it was
// extended by; a candidate of class c != blank scores lm_weight * q[c] more; the rows that emitted
// step the LM after the predictor, on the same emit / parent / token / count, by the same tiled
// products and cell kernel (no layer norm) and a log-softmax row kernel.
//
// The same fused search over the stateless predictor (s2t_rnnt_beam_stateless_lm): the rounds, the joint,
// the LM step and the records are the ones above; a row's predictor state is its last ctx tokens and
// its step is one row kernel (gather, shift, depthwise window sum) and two tiled products.
//
// Both fused searches also run a chunk at a time (s2t_rnnt_beam_lstm_lm_chunk,
// s2t_rnnt_beam_stateless_lm_chunk): the same rounds through the same host functions, the LM's (h, c), q
// and lm_sum carried in the caller's state buffer behind the predictor's.
//
// Back-off n-gram shallow fusion (s2t_rnnt_beam_lstm_ngram, s2t_rnnt_beam_lstm_ngram_chunk): the LM's state
// is one context id per row, so nothing rides the rounds: beam_expand_kernel and beam_select_kernel have a
// compile-time n-gram mode in which the K candidates of a row take their look-ups (csrc/ngram_lookup.h) on K
// threads after the top-k loop and a kept row takes the context its look-up returned.  A round stays
// expand, select, predictor step; context ids and lm_sum are per-row arrays updated in place by select.
//
// On the host every beam entry point is ONE function, beam_search: a predictor (LstmPredictor or
// StatelessPredictor, which say how their workspace and state are carved, blanked, stepped and copied
// home), with an LM or not, the whole utterance or a chunk.  It checks the shapes, fills BeamArgs by name
// and enqueues the launches; stream_reset does the same for the three resets.  Buffers are handed out
// by one Arena, which also answers the *_bytes queries.
//
// A row's arithmetic does not depend on the rows that share its launch: tiles sit at fixed row
// positions, every (row, output) sum is taken per lane over k = lane, lane + 64, ... and folded by the
// same butterfly, and rows beyond R read clamped addresses and are never stored.
#include <type_traits>

#include "common.h"
#include "decode_common.h"
#include "decode_records.h"
#include "ngram_lookup.h"
#include "../../include/s2t_mi355.h"

namespace {

using namespace s2t_dec;           // decode_common.h: Top, better, wave_top, after, activate; decode_records.h:
                                   // the limits, the record, rank_candidates, trace_best, chunk_histories

constexpr int kTileRows = 16;      // rows of a tile
constexpr int kTileOuts = 4;       // outputs of a wave: 4 x 16 sums, one per lane after the fold
constexpr int kTileWaves = 4;      // waves of a tile workgroup: 16 outputs
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRoundBlock = 32;    // greedy rounds between two host reads of the live counter
static_assert(kMaxCand <= kThreads, "a thread per candidate");
static_assert(S2T_RNNT_LSTM_MAX_BEAM == s2t_dec::kMaxBeam, "the header's limit is the kernels'");

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------------------ tiled products
// One butterfly step over lane bit HALF: the two lanes split the sums between them (the upper lane
// keeps the upper half), so after the steps 32, 16, ..., 1 lane l holds the complete sum number l.
// The pairs added are wave_sum's, whatever the number of the sum.
template <int HALF>
__device__ __forceinline__ void fold_step(float (&v)[64]) {
  const bool up = (threadIdx.x & HALF) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float keep = up ? v[i + HALF] : v[i], send = up ? v[i] : v[i + HALF];
    v[i] = keep + __shfl_xor(send, HALF, 64);
  }
}

// acc[j * 16 + r] += sum_k w[n0 + j][k] x[rows[r]][k]: a lane takes k = lane, lane + 64, ...; loads
// are unconditional on clamped addresses, a k beyond K multiplies by a zeroed weight.
__device__ __forceinline__ void tile_accumulate(float (&acc)[64], const float* __restrict__ x, long ld,
                                                const int* rows, const float* __restrict__ w, int K,
                                                int n0, int N) {
  const int lane = threadIdx.x & 63;
  const float* wr[kTileOuts];
#pragma unroll
  for (int j = 0; j < kTileOuts; ++j) wr[j] = w + (long)min(n0 + j, N - 1) * K;
  const float* xr[kTileRows];
#pragma unroll
  for (int r = 0; r < kTileRows; ++r) xr[r] = x + (long)rows[r] * ld;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane, kk = min(k, K - 1);
    float wv[kTileOuts], xv[kTileRows];
#pragma unroll
    for (int j = 0; j < kTileOuts; ++j) wv[j] = wr[j][kk];
#pragma unroll
    for (int r = 0; r < kTileRows; ++r) xv[r] = xr[r][kk];
#pragma unroll
    for (int j = 0; j < kTileOuts; ++j) {
      const float wj = k < K ? wv[j] : 0.f;
#pragma unroll
      for (int r = 0; r < kTileRows; ++r) acc[j * kTileRows + r] = fmaf(wj, xv[r], acc[j * kTileRows + r]);
    }
  }
}

struct TileArgs {
  const float* x1;      // [R][ld1], row r
  long ld1;
  const float* w1;      // [N][K1]
  int K1;
  const float* x2;      // [R][ld2], row parent[r] (parent NULL: r), or NULL
  long ld2;
  const float* w2;      // [N][K2]
  int K2;
  const float* bias;    // [N] or NULL
  int N, R;
  const int* emit;      // [R]
  const int* parent;    // [R] or NULL
  const int* count;     // rows that emit this round
  float* y;             // [R][ldy], written for emitting rows
  long ldy;
};

// grid (ceil(N / 16), ceil(R / 16)): y[r][n] = x1[r] . w1[n] + x2[parent r] . w2[n] + bias[n]
__global__ __launch_bounds__(64 * kTileWaves) void tile_linear_kernel(TileArgs a) {
  if (*a.count == 0) return;
  __shared__ int s_rows[2][kTileRows];
  __shared__ int s_any;
  const int tid = threadIdx.x, row0 = blockIdx.y * kTileRows;
  if (tid < kTileRows) {
    const int r = min(row0 + tid, a.R - 1);
    s_rows[0][tid] = r;
    s_rows[1][tid] = a.parent ? a.parent[r] : r;
  }
  if (tid == 64) {
    int any = 0;
    for (int r = row0; r < min(row0 + kTileRows, a.R); ++r) any |= a.emit[r];
    s_any = any;
  }
  __syncthreads();
  if (!s_any) return;
  const int n0 = (blockIdx.x * kTileWaves + (tid >> 6)) * kTileOuts;
  if (n0 >= a.N) return;                                   // (no barrier below)
  float acc[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) acc[i] = 0.f;
  tile_accumulate(acc, a.x1, a.ld1, s_rows[0], a.w1, a.K1, n0, a.N);
  if (a.x2) tile_accumulate(acc, a.x2, a.ld2, s_rows[1], a.w2, a.K2, n0, a.N);
  fold_step<32>(acc);
  fold_step<16>(acc);
  fold_step<8>(acc);
  fold_step<4>(acc);
  fold_step<2>(acc);
  fold_step<1>(acc);
  const int lane = tid & 63, n = n0 + (lane >> 4), row = row0 + (lane & 15);
  if (n < a.N && row < a.R && a.emit[row]) a.y[row * a.ldy + n] = acc[0] + (a.bias ? a.bias[n] : 0.f);
}

// ------------------------------------------------------------------ per-row kernels of a predictor step
// LayerNorm of the n values v[0..n) (LDS) in place, two passes; ends with a barrier.
__device__ __forceinline__ void layer_norm_lds(float* v, int n, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, float eps, float* scratch) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) s += v[i];
  const float mean = block_sum(s, scratch) / n;
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const float d = v[i] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.f / sqrtf(block_sum(q, scratch) / n + eps);
  for (int i = threadIdx.x; i < n; i += kThreads) v[i] = (v[i] - mean) * rstd * gamma[i] + beta[i];
  __syncthreads();
}

struct RowLnArgs {
  const float* in;      // rows of ld floats: row index[r] (index NULL: r)
  long ld;
  const int* index;
  const float *gamma, *beta;
  float eps;
  int n, R;
  const int* emit;
  const int* count;
  int inplace;          // the state buffers are updated in place: nothing to do without an emission
  float* out;           // [R][n]
  // rows that do not emit receive copy_src[parent r] (n_copy floats) in copy_dst[r] (not inplace)
  const float* copy_src;
  float* copy_dst;
  int n_copy;
  const int* parent;
};

// grid R: out[r] = LN(in[index r]) for the rows that emit
__global__ __launch_bounds__(kThreads) void row_ln_kernel(RowLnArgs a) {
  extern __shared__ float sm[];
  __shared__ float scratch[kWaves];
  if (a.inplace && *a.count == 0) return;
  const int row = blockIdx.x, tid = threadIdx.x;
  if (!a.emit[row]) {
    if (!a.inplace && a.copy_src) {
      const float* s = a.copy_src + (long)(a.parent ? a.parent[row] : row) * a.n_copy;
      float* d = a.copy_dst + (long)row * a.n_copy;
      for (int i = tid; i < a.n_copy; i += kThreads) d[i] = s[i];
    }
    return;
  }
  const float* x = a.in + (long)(a.index ? a.index[row] : row) * a.ld;
  for (int i = tid; i < a.n; i += kThreads) sm[i] = x[i];
  __syncthreads();
  layer_norm_lds(sm, a.n, a.gamma, a.beta, a.eps, scratch);
  for (int i = tid; i < a.n; i += kThreads) a.out[(long)row * a.n + i] = sm[i];
}

struct CellArgs {
  const float* raw;     // [R][4H] raw gates of the rows that emit
  const float *g_gamma, *g_beta, *c_gamma, *c_beta;   // NULL: no layer norm
  float eps;
  int H, R;
  const int* emit;
  const int* parent;
  const int* count;
  int inplace;
  const float *h_src, *c_src;   // [R][H] of this layer
  float *h_dst, *c_dst;
};

// grid R: g_norm, i / f / cell / o, c_norm, h of one layer; a row that does not emit takes its
// parent's state as it is
__global__ __launch_bounds__(kThreads) void cell_kernel(CellArgs a) {
  extern __shared__ float sm[];                            // [4H] gates, [H] cell
  __shared__ float scratch[kWaves];
  if (a.inplace && *a.count == 0) return;
  const int row = blockIdx.x, tid = threadIdx.x, H = a.H;
  const long src = a.parent ? a.parent[row] : row;
  if (!a.emit[row]) {
    if (!a.inplace)
      for (int i = tid; i < H; i += kThreads) {
        a.h_dst[(long)row * H + i] = a.h_src[src * H + i];
        a.c_dst[(long)row * H + i] = a.c_src[src * H + i];
      }
    return;
  }
  float* g = sm;
  float* c = sm + 4 * H;
  for (int i = tid; i < 4 * H; i += kThreads) g[i] = a.raw[(long)row * 4 * H + i];
  __syncthreads();
  if (a.g_gamma) layer_norm_lds(g, 4 * H, a.g_gamma, a.g_beta, a.eps, scratch);
  for (int j = tid; j < H; j += kThreads)
    c[j] = sigm(g[H + j]) * a.c_src[src * H + j] + sigm(g[j]) * tanhf(g[2 * H + j]);
  __syncthreads();
  if (a.c_gamma) layer_norm_lds(c, H, a.c_gamma, a.c_beta, a.eps, scratch);
  for (int j = tid; j < H; j += kThreads) {
    a.c_dst[(long)row * H + j] = c[j];
    a.h_dst[(long)row * H + j] = sigm(g[3 * H + j]) * tanhf(c[j]);
  }
}

// ------------------------------------------------------------------ workspace (Arena: decode_records.h)
// What a search works on whatever its predictor: R = B * max(1, beam) rows.
struct SearchArrays {
  float *z, *mid, *logit;       // joint: act(am + lm) [R][V], [R][inner], out-projection [R][V]
  float* cscore;                // beam: candidates [B][kMaxCand]
  float* score;                 // beam: [R]
  int *ccls, *blen, *nb, *rec;  // beam: candidate classes, tokens per beam [R], live beams [B], records [B][T][beam]
  int *emit, *token, *parent;   // [R]
  int* counts;                  // [0], [1]: rows that emit, by round parity; [2]: R; [3]: rows still live
};

// joint: the caller runs the joint (a search); a predictor step on its own keeps one-element placeholders.
// n_mid: the elements of `mid`, which the two predictors' workspaces have sized differently without an
// out-projection (R or 1) and the size queries' answers keep.
SearchArrays carve_search(Arena& m, int B, int T, int beam, int V, size_t n_mid, bool joint) {
  const size_t R = (size_t)B * (beam > 0 ? beam : 1);
  SearchArrays a;
  a.z = m.take<float>(joint ? R * V : 1);
  a.mid = m.take<float>(n_mid);
  a.logit = m.take<float>(joint ? R * V : 1);
  a.cscore = m.take<float>(joint ? (size_t)B * kMaxCand : 1);
  a.score = m.take<float>(R);
  a.ccls = m.take<int>(joint ? (size_t)B * kMaxCand : 1);
  a.blen = m.take<int>(R);
  a.nb = m.take<int>(B);
  a.rec = m.take<int>(beam > 0 ? (size_t)B * T * beam : 1);
  a.emit = m.take<int>(R);
  a.token = m.take<int>(R);
  a.parent = m.take<int>(R);
  a.counts = m.take<int>(4);
  return a;
}

struct StateBuf {
  float *h, *c, *lm;            // [layers][R][H], [layers][R][H], [R][V]
};

struct Workspace {
  StateBuf buf[2];              // state and lm twice
  float *x, *raw, *lin, *dvec;  // LN(embedding) [R][E], raw gates [R][4H], linear(h) [R][D], its LN
  SearchArrays s;
  int *t, *nts, *done;          // greedy: [R]
};

// n_state: how many copies of (h, c, lm) the workspace holds -- two for a whole-utterance search; a
// chunk call keeps the live copy in the caller's state buffer (beam: one here, greedy: none)
Workspace carve(const S2tRnntLstmDesc& d, int B, int T, int beam, Arena& m, int n_state = 2) {
  const size_t R = (size_t)B * (beam > 0 ? beam : 1), L = d.num_layers;
  Workspace w;
  for (int s = 0; s < 2; ++s) {
    w.buf[s].h = s < n_state ? m.take<float>(L * R * d.H) : nullptr;
    w.buf[s].c = s < n_state ? m.take<float>(L * R * d.H) : nullptr;
    w.buf[s].lm = s < n_state ? m.take<float>(R * d.V) : nullptr;
  }
  w.x = m.take<float>(R * d.E);
  w.raw = m.take<float>(R * 4 * d.H);
  w.lin = m.take<float>(R * d.D);
  w.dvec = m.take<float>(R * d.D);
  w.s = carve_search(m, B, T, beam, d.V, R * (d.inner > 0 ? d.inner : 1), true);
  w.t = m.take<int>(R);
  w.nts = m.take<int>(R);
  w.done = m.take<int>(R);
  return w;
}

bool desc_ok(const S2tRnntLstmDesc* d) {
  return d && d->V >= 1 && d->V <= S2T_RNNT_LSTM_MAX_VOCAB && d->D >= 1 && d->D <= S2T_RNNT_LSTM_MAX_VOCAB &&
         d->inner >= 0 && d->inner <= S2T_RNNT_LSTM_MAX_VOCAB && d->E >= 1 &&
         d->E <= S2T_RNNT_LSTM_MAX_HIDDEN && d->H >= 4 && d->H <= S2T_RNNT_LSTM_MAX_HIDDEN && d->H % 4 == 0 &&
         d->num_layers >= 1 && d->num_layers <= S2T_RNNT_LSTM_MAX_LAYERS && d->act >= 0 && d->act <= 1;
}

// ------------------------------------------------------------------ one predictor step, enqueued
// In place (src == dst, parent NULL) or from buffer `src` to buffer `dst`.
void enqueue_pred_step(const S2tRnntLstmDesc& d, int R, const int* tokens, const int* emit,
                       const int* parent, const int* count, const float* h_src, const float* c_src,
                       const float* lm_src, float* h_dst, float* c_dst, float* lm_dst,
                       const Workspace& w, hipStream_t st) {
  const int inplace = h_src == h_dst;
  const int row_tiles = (R + kTileRows - 1) / kTileRows;
  constexpr int kOuts = kTileWaves * kTileOuts;
  const size_t LRH = (size_t)R * d.H;
  {
    RowLnArgs a{d.emb, d.E, tokens, d.in_gamma, d.in_beta, d.in_eps, d.E, R, emit, count, inplace, w.x,
                nullptr, nullptr, 0, parent};
    hipLaunchKernelGGL(row_ln_kernel, dim3(R), dim3(kThreads), sizeof(float) * d.E, st, a);
  }
  for (int l = 0; l < d.num_layers; ++l) {
    const S2tLstmLayer& p = d.layers[l];
    const float* x = l ? h_dst + (l - 1) * LRH : w.x;
    const int K = l ? d.H : d.E;
    TileArgs t{x, K, p.x2g_w, K, h_src + l * LRH, d.H, p.p2g_w, d.H, p.x2g_b, 4 * d.H, R, emit, parent,
               count, w.raw, 4L * d.H};
    hipLaunchKernelGGL(tile_linear_kernel, dim3((4 * d.H + kOuts - 1) / kOuts, row_tiles),
                       dim3(64 * kTileWaves), 0, st, t);
    CellArgs c{w.raw, p.g_gamma, p.g_beta, p.c_gamma, p.c_beta, d.lstm_eps, d.H, R, emit, parent, count,
               inplace, h_src + l * LRH, c_src + l * LRH, h_dst + l * LRH, c_dst + l * LRH};
    hipLaunchKernelGGL(cell_kernel, dim3(R), dim3(kThreads), sizeof(float) * 5 * d.H, st, c);
  }
  {
    TileArgs t{h_dst + (d.num_layers - 1) * LRH, d.H, d.lin_w, d.H, nullptr, 0, nullptr, 0, d.lin_b, d.D, R,
               emit, nullptr, count, w.lin, d.D};
    hipLaunchKernelGGL(tile_linear_kernel, dim3((d.D + kOuts - 1) / kOuts, row_tiles),
                       dim3(64 * kTileWaves), 0, st, t);
    RowLnArgs a{w.lin, d.D, nullptr, d.out_gamma, d.out_beta, d.out_eps, d.D, R, emit, count, inplace,
                w.dvec, lm_src, lm_dst, d.V, parent};
    hipLaunchKernelGGL(row_ln_kernel, dim3(R), dim3(kThreads), sizeof(float) * d.D, st, a);
    TileArgs u{w.dvec, d.D, d.pre_w, d.D, nullptr, 0, nullptr, 0, d.pre_b, d.V, R, emit, nullptr, count,
               lm_dst, d.V};
    hipLaunchKernelGGL(tile_linear_kernel, dim3((d.V + kOuts - 1) / kOuts, row_tiles),
                       dim3(64 * kTileWaves), 0, st, u);
  }
}

__global__ void count_kernel(const int* emit, int R, int* count) {
  __shared__ int s;
  if (threadIdx.x == 0) s = 0;
  __syncthreads();
  int n = 0;
  for (int r = threadIdx.x; r < R; r += blockDim.x) n += emit[r] != 0;
  if (n) atomicAdd(&s, n);
  __syncthreads();
  if (threadIdx.x == 0) *count = s;
}

// ------------------------------------------------------------------ one RNN-LM step, enqueued
// The language model of model/lm/rnn_lm.py: Embedding -> LSTM stack (no layer norm, bias b_ih + b_hh
// on the raw gates) -> Linear -> log-softmax.  Masked and gathered like the predictor's step, on the
// same tiled products and cell kernel.
struct LmWorkspace {
  float *h[2], *c[2], *q[2];    // state [layers][R][H] twice, log-probabilities [R][V] twice
  float *x, *raw, *logit;       // embedding rows [R][E], raw gates [R][4H], logits [R][V]
  float *cq, *lm_sum;           // beam: the candidates' q [B][kMaxCand], the rows' sums [R]
  int *tok, *counts;            // the start token [R]; the step on its own: its count
};

// n_state copies of (h, c, q): two for a search, none for the step on its own (the caller's buffers)
LmWorkspace carve_lm(const S2tRnnLmDesc& d, int B, int beam, Arena& m, int n_state) {
  const size_t R = (size_t)B * (beam > 0 ? beam : 1), L = d.num_layers;
  LmWorkspace w;
  for (int s = 0; s < 2; ++s) {
    w.h[s] = s < n_state ? m.take<float>(L * R * d.H) : nullptr;
    w.c[s] = s < n_state ? m.take<float>(L * R * d.H) : nullptr;
    w.q[s] = s < n_state ? m.take<float>(R * d.V) : nullptr;
  }
  w.x = m.take<float>(R * d.E);
  w.raw = m.take<float>(R * 4 * d.H);
  w.logit = m.take<float>(R * d.V);
  w.cq = m.take<float>(beam > 0 ? (size_t)B * kMaxCand : 1);
  w.lm_sum = m.take<float>(R);
  w.tok = m.take<int>(R);
  w.counts = m.take<int>(4);
  return w;
}

bool lm_ok(const S2tRnnLmDesc* d) {
  return d && d->V >= 1 && d->V <= S2T_RNNT_LSTM_MAX_VOCAB && d->E >= 1 && d->E <= S2T_RNNT_LSTM_MAX_HIDDEN &&
         d->H >= 4 && d->H <= S2T_RNNT_LSTM_MAX_HIDDEN && d->H % 4 == 0 && d->num_layers >= 1 &&
         d->num_layers <= S2T_RNNT_LSTM_MAX_LAYERS;
}

// grid R: x[r] = emb[tokens[r]] for the rows that emit
__global__ __launch_bounds__(kThreads) void lm_embed_kernel(const float* __restrict__ emb, int V, int E,
                                                            const int* tokens, const int* emit,
                                                            const int* count, float* x) {
  if (*count == 0) return;
  const int row = blockIdx.x;
  if (!emit[row]) return;
  const float* e = emb + (long)min(max(tokens[row], 0), V - 1) * E;
  for (int i = threadIdx.x; i < E; i += kThreads) x[(long)row * E + i] = e[i];
}

struct LogSoftmaxArgs {
  const float* logit;   // [R][V] of the rows that emit
  int V;
  const int* emit;
  const int* parent;
  const int* count;
  int inplace;
  const float* q_src;   // [R][V]
  float* q_dst;
};

// grid R: q[r] = log_softmax(logit[r]) as max, then log sum exp (beam_expand_kernel's form); a row that
// does not emit takes its parent's q as it is
__global__ __launch_bounds__(kThreads) void lm_log_softmax_kernel(LogSoftmaxArgs a) {
  __shared__ float scratch[kWaves];
  if (a.inplace && *a.count == 0) return;
  const int row = blockIdx.x, tid = threadIdx.x, V = a.V;
  float* q = a.q_dst + (long)row * V;
  if (!a.emit[row]) {
    if (!a.inplace) {
      const float* s = a.q_src + (long)(a.parent ? a.parent[row] : row) * V;
      for (int i = tid; i < V; i += kThreads) q[i] = s[i];
    }
    return;
  }
  const float* lg = a.logit + (long)row * V;
  float m = S2T_NEG_INF;
  for (int c = tid; c < V; c += kThreads) m = fmaxf(m, lg[c]);
  const float zmax = block_max(m, scratch);
  float s = 0.f;
  for (int c = tid; c < V; c += kThreads) s += expf(lg[c] - zmax);
  const float lse = logf(block_sum(s, scratch));
  for (int c = tid; c < V; c += kThreads) q[c] = (lg[c] - zmax) - lse;
}

// In place (src == dst, parent NULL) or from buffer `src` to buffer `dst`.
void enqueue_lm_step(const S2tRnnLmDesc& d, int R, const int* tokens, const int* emit, const int* parent,
                     const int* count, const float* h_src, const float* c_src, const float* q_src,
                     float* h_dst, float* c_dst, float* q_dst, const LmWorkspace& w, hipStream_t st) {
  const int inplace = h_src == h_dst;
  const int row_tiles = (R + kTileRows - 1) / kTileRows;
  constexpr int kOuts = kTileWaves * kTileOuts;
  const size_t LRH = (size_t)R * d.H;
  hipLaunchKernelGGL(lm_embed_kernel, dim3(R), dim3(kThreads), 0, st, d.emb, d.V, d.E, tokens, emit, count, w.x);
  for (int l = 0; l < d.num_layers; ++l) {
    const S2tLstmLayer& p = d.layers[l];
    const float* x = l ? h_dst + (l - 1) * LRH : w.x;
    const int K = l ? d.H : d.E;
    TileArgs t{x, K, p.x2g_w, K, h_src + l * LRH, d.H, p.p2g_w, d.H, p.x2g_b, 4 * d.H, R, emit, parent,
               count, w.raw, 4L * d.H};
    hipLaunchKernelGGL(tile_linear_kernel, dim3((4 * d.H + kOuts - 1) / kOuts, row_tiles),
                       dim3(64 * kTileWaves), 0, st, t);
    CellArgs c{w.raw, nullptr, nullptr, nullptr, nullptr, 0.f, d.H, R, emit, parent, count,
               inplace, h_src + l * LRH, c_src + l * LRH, h_dst + l * LRH, c_dst + l * LRH};
    hipLaunchKernelGGL(cell_kernel, dim3(R), dim3(kThreads), sizeof(float) * 5 * d.H, st, c);
  }
  TileArgs t{h_dst + (d.num_layers - 1) * LRH, d.H, d.out_w, d.H, nullptr, 0, nullptr, 0, d.out_b, d.V, R,
             emit, nullptr, count, w.logit, d.V};
  hipLaunchKernelGGL(tile_linear_kernel, dim3((d.V + kOuts - 1) / kOuts, row_tiles), dim3(64 * kTileWaves), 0,
                     st, t);
  LogSoftmaxArgs a{w.logit, d.V, emit, parent, count, inplace, q_src, q_dst};
  hipLaunchKernelGGL(lm_log_softmax_kernel, dim3(R), dim3(kThreads), 0, st, a);
}

__global__ void lm_start_kernel(int R, int token, int* tok, float* lm_sum) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
    tok[r] = token;
    lm_sum[r] = 0.f;
  }
}

// ------------------------------------------------------------------ joint
struct JointArgs {
  const float* am;      // [B][T][V]
  int T, V, inner, act;
  const float *out1_w, *out1_b, *out2_w, *out2_b;
  float *z, *mid, *logit;   // [R][V], [R][inner], [R][V]
};

// The joiner's output for one row, before the log-softmax: returns the row's V logits (global
// memory, visible to the whole workgroup).  y[r] = w[r] . x + b[r] by a wave per r, a lane over
// c = lane, lane + 64, ..., then wave_sum.
__device__ __forceinline__ void gemv_wave(const float* __restrict__ w, const float* __restrict__ b,
                                          const float* x, int rows, int cols, float* y) {
  const int lane = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < rows; r += kWaves) {
    const float* wr = w + (long)r * cols;
    float s = 0.f;
    for (int c = lane; c < cols; c += 64) s = fmaf(wr[c], x[c], s);
    s = wave_sum(s);
    if (lane == 0) y[r] = s + b[r];
  }
}

__device__ const float* joint_logits(const JointArgs& a, int row, int b, int t, const float* lm_row) {
  const float* amt = a.am + ((long)b * a.T + t) * a.V;
  float* z = a.z + (long)row * a.V;
  for (int c = threadIdx.x; c < a.V; c += kThreads) z[c] = activate(amt[c] + lm_row[c], a.act);
  __syncthreads();
  if (a.inner <= 0) return z;
  float* mid = a.mid + (long)row * a.inner;
  float* out = a.logit + (long)row * a.V;
  gemv_wave(a.out1_w, a.out1_b, z, a.inner, a.V, mid);
  __syncthreads();
  gemv_wave(a.out2_w, a.out2_b, mid, a.V, a.inner, out);
  __syncthreads();
  return out;
}

// the best (value descending, class ascending) of the classes this thread is given, over the
// workgroup; every thread gets it.  Ends with a barrier.
__device__ __forceinline__ Top block_top(Top mine, Top* s_top) {
  mine = wave_top(mine);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_top[threadIdx.x >> 6] = mine;
  __syncthreads();
  Top best = s_top[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) best = better(best, s_top[w]);
  return best;
}

// ------------------------------------------------------------------ greedy
struct GreedyArgs {
  JointArgs j;
  const long* lengths;
  const float* lm;      // [B][V]
  int max_token_step, max_out, parity;
  int *t, *nts, *done, *emit, *token, *counts;
  long* tokens;         // [B][max_out]
  long* out_len;        // [B]
};

__global__ void greedy_init_kernel(const long* lengths, int B, int T, int* t, int* nts, int* done, int* emit,
                                   int* token, int* counts, long* out_len) {
  __shared__ int live;
  if (threadIdx.x == 0) live = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const long n = lengths[b];
    t[b] = 0;
    nts[b] = 0;
    done[b] = n <= 0;
    emit[b] = 1;                                           // the first predictor step: blank, from zero state
    token[b] = 0;
    out_len[b] = 0;
    if (n > 0) atomicAdd(&live, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[0] = 0;
    counts[1] = 0;
    counts[2] = B;
    counts[3] = live;
  }
}

// grid B: one lattice move of every live utterance (reference model/decoding.py:244-268)
__global__ __launch_bounds__(kThreads) void greedy_joint_kernel(GreedyArgs a) {
  __shared__ Top s_top[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b == 0 && tid == 0) a.counts[a.parity ^ 1] = 0;      // the next round's count
  if (a.done[b]) {
    if (tid == 0) a.emit[b] = 0;
    return;
  }
  const int t = a.t[b], V = a.j.V;
  const float* lg = joint_logits(a.j, b, b, t, a.lm + (long)b * V);
  Top best{S2T_NEG_INF, V};
  for (int c = tid; c < V; c += kThreads) best = better(best, Top{lg[c], c});
  best = block_top(best, s_top);
  if (tid == 0) {
    const int tok = best.i < V ? best.i : 0;               // (only a NaN row leaves no class)
    const int nts = a.nts[b];
    if (tok == 0 || nts > a.max_token_step) {
      long Tb = a.lengths[b];
      if (Tb > a.j.T) Tb = a.j.T;
      a.t[b] = t + 1;
      a.nts[b] = 0;
      a.emit[b] = 0;
      if (t + 1 >= Tb) {
        a.done[b] = 1;
        atomicSub(&a.counts[3], 1);
      }
    } else {
      const long n = a.out_len[b];
      if (n < a.max_out) a.tokens[(long)b * a.max_out + n] = tok;
      a.out_len[b] = n + 1;
      a.nts[b] = nts + 1;
      a.emit[b] = 1;
      a.token[b] = tok;
      atomicAdd(&a.counts[a.parity], 1);
    }
  }
}

// ------------------------------------------------------------------ beam
struct BeamArgs {
  JointArgs j;
  const long* lengths;
  const float* lm;      // [R][V], the buffer the round reads
  int t, B, beam, topk, parity;
  float *cscore, *score;
  int *ccls, *blen, *nb, *rec, *emit, *token, *parent, *counts;
  // shallow fusion (q NULL: none): the LM's log-probabilities [R][V] of the buffer the round reads,
  // the weight, the candidates' own q [B][kMaxCand] and the rows' unweighted sums [R]
  const float* q;
  float lm_weight;
  float *cq, *lm_sum;
};

__global__ void beam_init_kernel(int B, int beam, float* score, int* blen, int* nb, int* emit, int* token,
                                 int* counts) {
  const int R = B * beam;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    score[r] = 0.f;
    blen[r] = 0;
    emit[r] = 1;
    token[r] = 0;
  }
  for (int b = threadIdx.x; b < B; b += blockDim.x) nb[b] = 1;
  if (threadIdx.x == 0) {
    counts[0] = 0;
    counts[1] = 0;
    counts[2] = R;
    counts[3] = 0;
  }
}

// grid B * beam: the cutoff_top_k best classes of a live beam by (logit descending, class ascending)
// -- log-softmax is monotone, the order is taken on the logits -- as candidates (beam score +
// log-probability, class)
// n-gram mode: the tables, the rows' context ids [R] (updated in place by select) and the context a
// candidate is in when it is kept [B][kMaxCand]; the weight, the candidates' q and the rows' sums are
// BeamArgs' lm_weight, cq and lm_sum (q stays NULL: there are no LM rows)
struct BeamNgram {
  NgramTables g;
  int *ctx, *cnext;
};

// The two beam kernels are instantiated on their argument struct: BeamArgs (no LM, or the RNN-LM's q
// rows), or BeamNgramArgs, the compile-time n-gram mode.  The plain instantiations keep their kernel
// arguments and their code.
struct BeamNgramArgs : BeamArgs {
  BeamNgram ng;
};

template <class Args>
__global__ __launch_bounds__(kThreads) void beam_expand_kernel(Args a) {
  constexpr bool NG = std::is_same_v<Args, BeamNgramArgs>;
  __shared__ Top s_top[kWaves];
  __shared__ float scratch[kWaves];
  __shared__ float s_sc[NG ? kMaxBeam : 1];                // n-gram mode: the row's candidates before the LM term
  __shared__ int s_cls[NG ? kMaxBeam : 1];
  const int row = blockIdx.x, b = row / a.beam, i = row - b * a.beam, tid = threadIdx.x;
  if (a.t >= clamped_len(a.lengths, b, a.j.T) || i >= a.nb[b]) return;
  const int V = a.j.V, K = min(a.topk, V);
  const float* lg = joint_logits(a.j, row, b, a.t, a.lm + (long)row * V);
  const float base = a.score[row];
  const float* q = a.q ? a.q + (long)row * V : nullptr;
  float pv = 0.f, zmax = 0.f, lse = 0.f;
  int pi = -1;
  for (int r = 0; r < K; ++r) {
    Top best{S2T_NEG_INF, V};
    for (int c = tid; c < V; c += kThreads)
      if (r == 0 || after(lg[c], c, pv, pi)) best = better(best, Top{lg[c], c});
    best = block_top(best, s_top);
    pv = best.v;
    pi = best.i;
    if (r == 0) {                                          // log-softmax as max, then log sum exp
      zmax = pv;
      float s = 0.f;
      for (int c = tid; c < V; c += kThreads) s += expf(lg[c] - zmax);
      lse = logf(block_sum(s, scratch));
    }
    if (tid == 0) {
      const bool ok = pi < V;                              // (only a NaN input leaves a round empty)
      float sc = base + ((pv - zmax) - lse);
      if (q) {                                             // blank carries no LM term
        const float qv = ok && pi != 0 ? q[pi] : 0.f;
        sc = __fadd_rn(sc, __fmul_rn(a.lm_weight, qv));
        a.cq[b * kMaxCand + i * K + r] = qv;
      }
      if constexpr (NG) {                                  // the LM term follows the loop, a thread per candidate
        s_sc[r] = sc;
        s_cls[r] = ok ? pi : -1;
      } else {
        a.cscore[b * kMaxCand + i * K + r] = ok ? sc : S2T_NEG_INF;
        a.ccls[b * kMaxCand + i * K + r] = ok ? pi : 0;
      }
    }
  }
  if constexpr (NG) {
    __syncthreads();
    if (tid < K) {                                         // blank: no look-up, the parent's context
      const int at = b * kMaxCand + i * K + tid;
      const bool ok = s_cls[tid] >= 0;                     // (only a NaN input leaves a round empty)
      const int cls = ok ? s_cls[tid] : 0;
      const int ctx = ngram_clamp(a.ng.ctx[row], a.ng.g.num_ctx);
      NgramHit h{0.f, ctx};
      if (cls != 0) h = ngram_score(a.ng.g, ctx, cls);
      a.cscore[at] = ok ? __fadd_rn(s_sc[tid], __fmul_rn(a.lm_weight, h.logp)) : S2T_NEG_INF;
      a.ccls[at] = cls;
      a.cq[at] = h.logp;
      a.ng.cnext[at] = h.next;
    }
  }
}


// grid B: rank the candidates of an utterance (score descending, then parent position, then rank
// in the parent's top-k: the candidate index), keep the beam_size best as the new beams, one
// (parent, class) record each; the rows' parent / emit / token for the predictor step.
template <class Args>
__global__ __launch_bounds__(kThreads) void beam_select_kernel(Args a) {
  constexpr bool NG = std::is_same_v<Args, BeamNgramArgs>;
  __shared__ float s_cscore[kMaxCand], s_lmsum[kMaxBeam];
  __shared__ int s_ccls[kMaxCand], s_pick[kMaxBeam], s_len[kMaxBeam];
  __shared__ int s_ctx[NG ? kMaxBeam : 1];                 // n-gram mode: the parents' context ids
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.beam, row0 = b * BS;
  if (b == 0 && tid == 0) a.counts[a.parity ^ 1] = 0;
  if (a.t >= clamped_len(a.lengths, b, a.j.T)) {           // finished: the rows keep what they have
    if (tid < BS) {
      a.emit[row0 + tid] = 0;
      a.parent[row0 + tid] = row0 + tid;
    }
    return;
  }
  const int nb = a.nb[b], K = min(a.topk, a.j.V), nc = nb * K, nnb = min(nc, BS);
  if (tid < nc) {
    s_cscore[tid] = a.cscore[b * kMaxCand + tid];
    s_ccls[tid] = a.ccls[b * kMaxCand + tid];
  }
  if (tid < nb) {                                          // the rows of an utterance read each other's
    s_len[tid] = a.blen[row0 + tid];
    if (NG || a.q) s_lmsum[tid] = a.lm_sum[row0 + tid];
    if constexpr (NG) s_ctx[tid] = a.ng.ctx[row0 + tid];
  }
  __syncthreads();
  rank_candidates(s_cscore, nc, nnb, s_pick);
  __syncthreads();
  if (tid < BS) {
    const int row = row0 + tid;
    if (tid < nnb) {
      const int q = s_pick[tid], parent = q / K, cls = s_ccls[q];
      a.score[row] = s_cscore[q];
      a.blen[row] = s_len[parent] + (cls != 0 ? 1 : 0);
      if (NG || a.q) a.lm_sum[row] = cls != 0 ? s_lmsum[parent] + a.cq[b * kMaxCand + q] : s_lmsum[parent];
      if constexpr (NG) a.ng.ctx[row] = cls != 0 ? a.ng.cnext[b * kMaxCand + q] : s_ctx[parent];
      a.rec[((long)b * a.j.T + a.t) * BS + tid] = pack_record(parent, cls);
      a.parent[row] = row0 + parent;
      a.emit[row] = cls != 0;
      a.token[row] = cls;
      if (cls != 0) atomicAdd(&a.counts[a.parity], 1);
    } else {
      a.parent[row] = row;
      a.emit[row] = 0;
    }
  }
  if (tid == 0) a.nb[b] = nnb;
}

// grid B: the best beam is position 0; its (parent, class) records traced back
__global__ __launch_bounds__(64) void beam_trace_kernel(const long* lengths, int T, int beam, const int* rec,
                                                        const int* blen, const float* score, long* tokens,
                                                        long* frames, long* out_len, float* out_score,
                                                        const float* lm_sum, float* out_lm) {
  __shared__ int s_trace[kTraceFrames * kMaxBeam], s_left;
  const int b = blockIdx.x;
  const int Tb = (int)clamped_len(lengths, b, T), n = Tb ? blen[b * beam] : 0;
  if (threadIdx.x == 0) {                                  // no frames: no tokens, score 0
    out_len[b] = n;
    out_score[b] = Tb ? score[b * beam] : 0.f;
    if (out_lm) out_lm[b] = Tb ? lm_sum[b * beam] : 0.f;
  }
  trace_best<64>(rec + (long)b * T * beam, Tb, beam, 0, n, s_trace, &s_left, tokens + (long)b * T,
                 frames + (long)b * T);
}

// Desc: S2tRnntLstmDesc or S2tRnntStatelessDesc (the joiner's fields carry the same names)
template <class Desc>
JointArgs joint_args(const Desc& d, const float* am, int T, const SearchArrays& s) {
  return JointArgs{am, T, d.V, d.inner, d.act, d.out1_w, d.out1_b, d.out2_w, d.out2_b, s.z, s.mid, s.logit};
}

// The rounds of a greedy search on the state (h, c, lm), in place: a joint launch and a predictor
// step each.  host_poll: blocks of kRoundBlock rounds with one host read of the "rows still live"
// counter per block; else every round is enqueued (finished rows are inert: the same bits).
int greedy_rounds(const S2tRnntLstmDesc& d, int B, GreedyArgs g, float* h, float* c, float* lm,
                  const Workspace& w, long max_rounds, int host_poll, hipStream_t st) {
  for (long r = 0; r < max_rounds;) {
    for (int q = 0; (q < kRoundBlock || !host_poll) && r < max_rounds; ++q, ++r) {
      g.parity = (int)(r & 1);
      hipLaunchKernelGGL(greedy_joint_kernel, dim3(B), dim3(kThreads), 0, st, g);
      enqueue_pred_step(d, B, w.s.token, w.s.emit, nullptr, w.s.counts + g.parity, h, c, lm, h, c, lm, w, st);
    }
    S2T_CHECK_LAUNCH();
    if (!host_poll) continue;
    int live = 0;                                          // the one host read of the block
    hipError_t e = hipMemcpyAsync(&live, w.s.counts + 3, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (live <= 0) break;
  }
  return 0;
}

// ------------------------------------------------------------------ the stateless predictor in the row layout
// model/predictor/predictor.py StatelessPredictor: Embedding -> depthwise Conv1d over the last ctx tokens
// (no bias) -> Linear.  A row's state is its ctx tokens, most recent last.  A step is the row kernel
// below and two tiled products (lin, pre_proj).
struct StatelessRowArgs {
  const float* emb;     // [V][E]
  const float* conv_w;  // [E][ctx]
  int V, E, ctx;
  const int *tokens, *emit, *parent, *count;
  int inplace;
  const int* ctx_src;   // [R][ctx]
  int* ctx_dst;
  const float* lm_src;  // [R][V]
  float* lm_dst;
  float* x;             // [R][E], written for emitting rows
};

// grid R: a row that emits takes its parent's context, shifts its token in and sums the depthwise
// window, x[e] = sum_k conv_w[e][k] emb[ctx[k]][e] over k = 0, 1, ... (csrc/decode_search.h's order); a row
// that does not takes its parent's context and lm row as they are
__global__ __launch_bounds__(kThreads) void stateless_row_kernel(StatelessRowArgs a) {
  __shared__ int s_ctx[S2T_RNNT_STATELESS_MAX_CONTEXT];
  if (a.inplace && *a.count == 0) return;
  const int row = blockIdx.x, tid = threadIdx.x, n = a.ctx;
  const long src = a.parent ? a.parent[row] : row;
  if (!a.emit[row]) {
    if (!a.inplace) {
      for (int k = tid; k < n; k += kThreads) a.ctx_dst[(long)row * n + k] = a.ctx_src[src * n + k];
      for (int i = tid; i < a.V; i += kThreads) a.lm_dst[(long)row * a.V + i] = a.lm_src[src * a.V + i];
    }
    return;
  }
  if (tid < n) s_ctx[tid] = tid + 1 < n ? a.ctx_src[src * n + tid + 1] : a.tokens[row];
  __syncthreads();                                         // (in place: the row is read before it is written)
  if (tid < n) {
    s_ctx[tid] = min(max(s_ctx[tid], 0), a.V - 1);
    a.ctx_dst[(long)row * n + tid] = s_ctx[tid];
  }
  __syncthreads();
  for (int e = tid; e < a.E; e += kThreads) {
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc = fmaf(a.conv_w[e * n + k], a.emb[(long)s_ctx[k] * a.E + e], acc);
    a.x[(long)row * a.E + e] = acc;
  }
}

struct StatelessBuf {
  int* ctx;                     // [R][ctx]
  float* lm;                    // [R][V]
};

struct StatelessWorkspace {
  StatelessBuf buf[2];          // state and lm twice
  float *x, *lin;               // the depthwise sums [R][E], linear(x) [R][D]
  SearchArrays s;
};

// n_state copies of (ctx, lm): two for a search, none for the step on its own (the caller's buffers)
StatelessWorkspace carve_stateless(const S2tRnntStatelessDesc& d, int B, int T, int beam, Arena& m, int n_state) {
  const size_t R = (size_t)B * (beam > 0 ? beam : 1);
  StatelessWorkspace w;
  for (int s = 0; s < 2; ++s) {
    w.buf[s].ctx = s < n_state ? m.take<int>(R * d.ctx) : nullptr;
    w.buf[s].lm = s < n_state ? m.take<float>(R * d.V) : nullptr;
  }
  w.x = m.take<float>(R * d.E);
  w.lin = m.take<float>(R * d.D);
  w.s = carve_search(m, B, T, beam, d.V, beam > 0 && d.inner > 0 ? R * d.inner : 1, beam > 0);
  return w;
}

bool stateless_ok(const S2tRnntStatelessDesc* d) {
  return d && d->V >= 1 && d->V <= S2T_RNNT_LSTM_MAX_VOCAB && d->D >= 1 && d->D <= S2T_RNNT_LSTM_MAX_VOCAB &&
         d->inner >= 0 && d->inner <= S2T_RNNT_LSTM_MAX_VOCAB && d->E >= 1 && d->E <= S2T_RNNT_LSTM_MAX_HIDDEN &&
         d->ctx >= 1 && d->ctx <= S2T_RNNT_STATELESS_MAX_CONTEXT && d->act >= 0 && d->act <= 1;
}

// In place (src == dst, parent NULL) or from buffer `src` to buffer `dst`.
void enqueue_stateless_step(const S2tRnntStatelessDesc& d, int R, const int* tokens, const int* emit,
                            const int* parent, const int* count, const int* ctx_src, const float* lm_src,
                            int* ctx_dst, float* lm_dst, const StatelessWorkspace& w, hipStream_t st) {
  const int row_tiles = (R + kTileRows - 1) / kTileRows;
  constexpr int kOuts = kTileWaves * kTileOuts;
  StatelessRowArgs a{d.emb, d.conv_w, d.V, d.E, d.ctx, tokens, emit, parent, count, ctx_src == ctx_dst,
                     ctx_src, ctx_dst, lm_src, lm_dst, w.x};
  hipLaunchKernelGGL(stateless_row_kernel, dim3(R), dim3(kThreads), 0, st, a);
  TileArgs t{w.x, d.E, d.lin_w, d.E, nullptr, 0, nullptr, 0, d.lin_b, d.D, R, emit, nullptr, count, w.lin, d.D};
  hipLaunchKernelGGL(tile_linear_kernel, dim3((d.D + kOuts - 1) / kOuts, row_tiles), dim3(64 * kTileWaves), 0,
                     st, t);
  TileArgs u{w.lin, d.D, d.pre_w, d.D, nullptr, 0, nullptr, 0, d.pre_b, d.V, R, emit, nullptr, count, lm_dst,
             d.V};
  hipLaunchKernelGGL(tile_linear_kernel, dim3((d.V + kOuts - 1) / kOuts, row_tiles), dim3(64 * kTileWaves), 0,
                     st, u);
}

// ------------------------------------------------------------------ chunk-carried search
// The searches above fed their frames in pieces.  A round's launches are the ones above, on the
// same arguments; what follows only says where the state lives between two calls and turns a
// chunk's records into histories.  The caller's state buffer holds (h, c, lm) in the layout the
// round kernels work on ([layers][R][H], [R][V] over all rows of the batch), so a greedy chunk steps
// it in place and nothing is loaded or stored.  A beam chunk alternates between the state buffer
// (frame 0 reads it) and one copy in the workspace; after an odd number of rounds the live copy is
// the workspace's and one launch copies it home, so the launches of a call depend on Tc alone and
// nothing between two calls depends on host memory.
constexpr int kStreamHdr = 4;      // ints per row: frames since reset, overflow, history buffer in use, stable_len

struct StreamState {
  StateBuf live;                   // (h, c, lm)
  float* score;                    // beam: [R]
  int *blen, *nb;                  // beam: tokens per beam [R] (not clamped), live beams [B]
  long* n;                         // greedy: symbols since the reset [B] (not clamped)
  int* hdr;                        // [B][kStreamHdr]
  int *htok, *hfrm;                // beam: [B][2][beam][max_tokens]
};

// (the order is the header's documented layout)
StreamState carve_state(const S2tRnntLstmDesc& d, int B, int beam, int max_tokens, Arena& m) {
  const size_t R = (size_t)B * (beam > 0 ? beam : 1), L = d.num_layers;
  StreamState s{};
  s.live.h = m.take<float>(L * R * d.H);
  s.live.c = m.take<float>(L * R * d.H);
  s.live.lm = m.take<float>(R * d.V);
  s.hdr = m.take<int>((size_t)B * kStreamHdr);
  if (beam > 0) {
    s.score = m.take<float>(R);
    s.blen = m.take<int>(R);
    s.nb = m.take<int>(B);
    s.htok = m.take<int>(2 * R * max_tokens);
    s.hfrm = m.take<int>(2 * R * max_tokens);
  } else {
    s.n = m.take<long>(B);
  }
  return s;
}

struct ResetArgs {
  const int* rows;      // [B] or NULL
  int beam, BS, layers, H;   // BS = max(1, beam) rows per utterance
  float *h, *c, *score;
  int *blen, *nb, *hdr;
  long* n;
  int *emit, *token;    // [R]: the rows that take the first predictor step, on blank
};

// grid B: a row the mask names becomes the empty hypothesis -- zero (h, c), one live beam of score
// 0, no tokens, frame 0, no overflow -- and is marked for the predictor step on blank that follows;
// the other rows are marked idle and keep every bit.
__global__ __launch_bounds__(kThreads) void stream_reset_kernel(ResetArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.BS, row0 = b * BS;
  const long R = (long)gridDim.x * BS;
  const int on = !a.rows || a.rows[b] != 0;
  if (tid < BS) {
    a.emit[row0 + tid] = on;
    a.token[row0 + tid] = 0;
  }
  if (!on) return;
  for (int l = 0; l < a.layers; ++l)
    for (int x = tid; x < BS * a.H; x += kThreads) {
      a.h[(l * R + row0) * a.H + x] = 0.f;
      a.c[(l * R + row0) * a.H + x] = 0.f;
    }
  if (a.beam > 0 && tid < BS) {
    a.score[row0 + tid] = 0.f;
    a.blen[row0 + tid] = 0;
  }
  if (tid < kStreamHdr) a.hdr[b * kStreamHdr + tid] = 0;
  if (tid == 0) {
    if (a.beam > 0) a.nb[b] = 1;
    else a.n[b] = 0;
  }
}

// greedy_init_kernel for a chunk: every row with frames in this chunk is live at its frame 0; no
// row emits (the carried lm is current: a chunk ends right after a frame advance)
__global__ void greedy_chunk_init_kernel(const long* chunk_len, int B, int* t, int* nts, int* done, int* emit,
                                         int* token, int* counts) {
  __shared__ int live;
  if (threadIdx.x == 0) live = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const long n = chunk_len[b];
    t[b] = 0;
    nts[b] = 0;
    done[b] = n <= 0;
    emit[b] = 0;
    token[b] = 0;
    if (n > 0) atomicAdd(&live, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[0] = 0;
    counts[1] = 0;
    counts[2] = B;
    counts[3] = live;
  }
}

__global__ void greedy_chunk_end_kernel(const long* chunk_len, int B, int Tc, int max_tokens, const long* n,
                                        int* hdr, long* out_len, int* overflow) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    const long Tb = clamped_len(chunk_len, b, Tc);
    if (Tb <= 0) continue;                                 // an idle stream: state and outputs stay
    const long nn = n[b];
    const int ovf = nn > max_tokens ? 1 : 0;               // a symbol was dropped
    hdr[b * kStreamHdr] += (int)Tb;
    hdr[b * kStreamHdr + 1] = ovf;
    out_len[b] = ovf ? max_tokens : nn;
    overflow[b] = ovf;
  }
}

__global__ void beam_chunk_init_kernel(int* counts, int R) {
  if (threadIdx.x < 4) counts[threadIdx.x] = threadIdx.x == 2 ? R : 0;
}

struct BeamEndArgs {
  const long* chunk_len;
  int Tc, beam, max_tokens;
  const int *rec, *blen, *nb;   // records [B][Tc][beam] of this chunk; lengths and live beams after it
  const float* score;
  int *hdr, *htok, *hfrm;
  long *tokens, *frames, *out_len;   // [B][max_tokens] twice, [B]
  float* out_score;
  long* stable_len;
  int* overflow;
  const float* lm_sum;  // shallow fusion: the rows' unweighted LM sums [R] after the chunk, or NULL
  float* out_lm;        // [B]
};

// grid B: the chunk's records become the beams' new histories and the row's outputs
// (decode_records.h chunk_histories, the scheme of csrc/decode_rnnt.hip).  The two history
// buffers swap roles per chunk (the index is the row's, on the device).
__global__ __launch_bounds__(kThreads) void beam_chunk_end_kernel(BeamEndArgs a) {
  __shared__ int s_trace[kTraceFrames * kMaxBeam], s_anc[kMaxBeam], s_base[kMaxBeam], s_len[kMaxBeam];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = (int)clamped_len(a.chunk_len, b, a.Tc);
  if (Tb == 0) return;                                     // an idle stream: state and outputs stay
  const int BS = a.beam, MT = a.max_tokens, row0 = b * BS, nb = a.nb[b];
  int* hdr = a.hdr + b * kStreamHdr;
  const int f0 = hdr[0], ovf0 = hdr[1], hcur = hdr[2];
  int* htok = a.htok + (long)b * 2 * BS * MT;
  int* hfrm = a.hfrm + (long)b * 2 * BS * MT;
  if (tid < nb) s_len[tid] = a.blen[row0 + tid];           // (read first by the thread that wrote it)
  chunk_histories<kThreads>(
      tid, tid & 63, tid >> 6,
      ChunkHistoryArgs{Tb, nb, BS, MT, 0, f0, ovf0, a.rec + (long)b * a.Tc * BS, s_len, htok + (long)hcur * BS * MT,
                       hfrm + (long)hcur * BS * MT, htok + (long)(hcur ^ 1) * BS * MT,
                       hfrm + (long)(hcur ^ 1) * BS * MT, a.tokens + (long)b * MT, a.frames + (long)b * MT,
                       s_trace, s_anc, s_base},
      [&](int out_len, int stable, int ovf) {
        a.out_len[b] = out_len;
        a.out_score[b] = a.score[row0];
        if (a.out_lm) a.out_lm[b] = a.lm_sum[row0];
        a.stable_len[b] = stable;
        a.overflow[b] = ovf;
        hdr[0] = f0 + Tb;
        hdr[1] = ovf;
        hdr[2] = hcur ^ 1;
        hdr[3] = stable;
      });
}

// ------------------------------------------------------------------ chunk-carried search with the RNN-LM
// The fused searches (s2t_rnnt_beam_lstm_lm, s2t_rnnt_beam_stateless_lm) fed their frames in pieces: the
// rounds are beam_rounds with the LM, on carried buffers.  Behind the predictor's stream state the
// caller's buffer holds the LM's live (h, c, q) and lm_sum; the workspace holds the second copy of (h, c,
// q), and after an odd Tc ONE launch copies every survivor home, the predictor's and the LM's.
struct LmStreamState {
  float *h, *c, *q;                // [layers][R][H] twice, [R][V]
  float* lm_sum;                   // [R]
};

LmStreamState carve_lm_state(const S2tRnnLmDesc& d, int B, int beam, Arena& m) {
  const size_t R = (size_t)B * beam, L = d.num_layers;
  LmStreamState s{};
  s.h = m.take<float>(L * R * d.H);
  s.c = m.take<float>(L * R * d.H);
  s.q = m.take<float>(R * d.V);
  s.lm_sum = m.take<float>(R);
  return s;
}

// the stateless predictor's stream state: StreamState with the context in place of (h, c)
struct StatelessStreamState {
  StatelessBuf live;               // (ctx, lm)
  float* score;                    // [R]
  int *blen, *nb, *hdr;            // [R], [B], [B][kStreamHdr]
  int *htok, *hfrm;                // [B][2][beam][max_tokens]
};

// (the order is the header's documented layout)
StatelessStreamState carve_stateless_state(const S2tRnntStatelessDesc& d, int B, int beam, int max_tokens,
                                           Arena& m) {
  const size_t R = (size_t)B * beam;
  StatelessStreamState s{};
  s.live.ctx = m.take<int>(R * d.ctx);
  s.live.lm = m.take<float>(R * d.V);
  s.hdr = m.take<int>((size_t)B * kStreamHdr);
  s.score = m.take<float>(R);
  s.blen = m.take<int>(R);
  s.nb = m.take<int>(B);
  s.htok = m.take<int>(2 * R * max_tokens);
  s.hfrm = m.take<int>(2 * R * max_tokens);
  return s;
}

// The LM workspace a chunk's rounds work on: buffer 0 is the state's (the live copy, frame 0 reads it),
// buffer 1 the workspace's one copy; lm_sum is the state's, updated in place.
LmWorkspace live_lm(LmWorkspace w, const LmStreamState& s) {
  w.h[1] = w.h[0];
  w.c[1] = w.c[0];
  w.q[1] = w.q[0];
  w.h[0] = s.h;
  w.c[0] = s.c;
  w.q[0] = s.q;
  w.lm_sum = s.lm_sum;
  return w;
}

struct LmResetArgs {
  const int* rows;      // [B] or NULL
  int BS, layers, H, V, nctx, start;   // nctx: the stateless predictor's context (0: none)
  float *h, *c, *q, *lm_sum;
  int* tok;             // [R]: the token of the LM's first step
  int* ctx;             // [R][nctx] or NULL
};

// grid B, after stream_reset_kernel: a row the mask names gets zero LM (h, c), q = 0, lm_sum = 0 and
// (stateless predictor) a context of blanks; the other rows keep every bit.  Every row's start token
// is written (lm_start_kernel's tok), the step that follows is masked by emit.
__global__ __launch_bounds__(kThreads) void lm_stream_reset_kernel(LmResetArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, BS = a.BS, row0 = b * BS;
  const long R = (long)gridDim.x * BS;
  if (tid < BS) a.tok[row0 + tid] = a.start;
  if (a.rows && a.rows[b] == 0) return;
  for (int l = 0; l < a.layers; ++l)
    for (int x = tid; x < BS * a.H; x += kThreads) {
      a.h[(l * R + row0) * a.H + x] = 0.f;
      a.c[(l * R + row0) * a.H + x] = 0.f;
    }
  for (long x = tid; x < (long)BS * a.V; x += kThreads) a.q[(long)row0 * a.V + x] = 0.f;
  if (tid < BS) a.lm_sum[row0 + tid] = 0.f;
  if (a.ctx)
    for (int x = tid; x < BS * a.nctx; x += kThreads) a.ctx[(long)row0 * a.nctx + x] = 0;
}

constexpr int kCopyParts = 6;

struct CopyHomeArgs {
  const void* src[kCopyParts];
  void* dst[kCopyParts];
  long n[kCopyParts];              // 4-byte words (float or int); 0: unused
};

// a chunk's copy-home: the predictor's survivors and the LM's in one launch
__global__ __launch_bounds__(kThreads) void state_copy_parts_kernel(CopyHomeArgs a) {
  const long step = (long)gridDim.x * kThreads, i0 = (long)blockIdx.x * kThreads + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kCopyParts; ++k) {
    const unsigned* __restrict__ s = static_cast<const unsigned*>(a.src[k]);
    unsigned* d = static_cast<unsigned*>(a.dst[k]);
    for (long i = i0; i < a.n[k]; i += step) d[i] = s[i];
  }
}

void enqueue_copy_home(const CopyHomeArgs& c, hipStream_t st) {
  long most = 1;
  for (int k = 0; k < kCopyParts; ++k) most = c.n[k] > most ? c.n[k] : most;
  const long need = (most + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(state_copy_parts_kernel, dim3((int)(need < 1024 ? need : 1024)), dim3(kThreads), 0, st, c);
}

struct HomeList {
  CopyHomeArgs c{};
  int parts = 0;
  void add(const void* src, void* dst, long n) {
    c.src[parts] = src;
    c.dst[parts] = dst;
    c.n[parts++] = n;
  }
};

// ------------------------------------------------------------------ the two predictors, as the beam search sees them
// What beam_search and stream_reset below ask of a predictor: whether the descriptor is valid and its V;
// the joint's arguments; its workspace (Work: two buffers `buf`, scratch, the search's arrays `s`) and its
// stream state (State: the live buffer `live`, then score / blen / nb / hdr / htok / hfrm); how a buffer is
// blanked for a whole-utterance search; its step from one buffer to another on the workspace's emit /
// token; which arrays go home after an odd number of rounds; what the reset kernels are told.
struct LstmPredictor {
  using Work = Workspace;
  using State = StreamState;
  using Buf = StateBuf;
  const S2tRnntLstmDesc* d;

  bool ok() const { return desc_ok(d); }
  int V() const { return d->V; }
  JointArgs joint(const float* am, int T, const Work& w) const { return joint_args(*d, am, T, w.s); }
  Work work(int B, int T, int beam, Arena& m, int n_state) const { return carve(*d, B, T, beam, m, n_state); }
  State state(int B, int beam, int max_tokens, Arena& m) const { return carve_state(*d, B, beam, max_tokens, m); }
  hipError_t blank(const Buf& b, int R, hipStream_t st) const {   // zero (h, c)
    const size_t bytes = sizeof(float) * (size_t)d->num_layers * R * d->H;
    const hipError_t e = hipMemsetAsync(b.h, 0, bytes, st);
    return e == hipSuccess ? hipMemsetAsync(b.c, 0, bytes, st) : e;
  }
  // parent NULL: in place (src is dst)
  void step(int R, const Work& w, const int* parent, const int* count, const Buf& src, const Buf& dst,
            hipStream_t st) const {
    enqueue_pred_step(*d, R, w.s.token, w.s.emit, parent, count, src.h, src.c, src.lm, dst.h, dst.c, dst.lm, w, st);
  }
  void home(HomeList& l, int R, const Buf& src, const Buf& dst) const {
    const long n_state = (long)d->num_layers * R * d->H;
    l.add(src.h, dst.h, n_state);
    l.add(src.c, dst.c, n_state);
    l.add(src.lm, dst.lm, (long)R * d->V);
  }
  void reset_args(const State& s, ResetArgs& a, LmResetArgs&) const {   // (h, c) to zero, greedy's counter
    a.layers = d->num_layers;
    a.H = d->H;
    a.h = s.live.h;
    a.c = s.live.c;
    a.n = s.n;
  }
};

struct StatelessPredictor {
  using Work = StatelessWorkspace;
  using State = StatelessStreamState;
  using Buf = StatelessBuf;
  const S2tRnntStatelessDesc* d;

  bool ok() const { return stateless_ok(d); }
  int V() const { return d->V; }
  JointArgs joint(const float* am, int T, const Work& w) const { return joint_args(*d, am, T, w.s); }
  Work work(int B, int T, int beam, Arena& m, int n_state) const {
    return carve_stateless(*d, B, T, beam, m, n_state);
  }
  State state(int B, int beam, int max_tokens, Arena& m) const {
    return carve_stateless_state(*d, B, beam, max_tokens, m);
  }
  hipError_t blank(const Buf& b, int R, hipStream_t st) const {   // a context of blanks
    return hipMemsetAsync(b.ctx, 0, sizeof(int) * (size_t)R * d->ctx, st);
  }
  void step(int R, const Work& w, const int* parent, const int* count, const Buf& src, const Buf& dst,
            hipStream_t st) const {
    enqueue_stateless_step(*d, R, w.s.token, w.s.emit, parent, count, src.ctx, src.lm, dst.ctx, dst.lm, w, st);
  }
  void home(HomeList& l, int R, const Buf& src, const Buf& dst) const {
    l.add(src.ctx, dst.ctx, (long)R * d->ctx);
    l.add(src.lm, dst.lm, (long)R * d->V);
  }
  // (no LSTM layers: the predictor's state is the context, which the LM's reset blanks)
  void reset_args(const State& s, ResetArgs&, LmResetArgs& la) const {
    la.nctx = d->ctx;
    la.ctx = s.live.ctx;
  }
};

// ------------------------------------------------------------------ the beam search, whole or a chunk of it
struct Fusion {                    // shallow fusion: with an RNN-LM (lm), or with a back-off n-gram (ngram)
  const S2tRnnLmDesc* lm;
  float weight;
  int start_token;                 // the LM's first input, < 0: none (a chunk call: the reset has taken it)
  float* lm_score;                 // [B]
  const S2tNgramLmDesc* ngram = nullptr;
  int start_ctx = 0;               // n-gram: the empty hypothesis' context (a chunk call: the reset has set it)
};

// What the n-gram adds to a search's buffers: in the workspace the candidates' q and next contexts, and for
// a whole-utterance search the rows' context ids and sums; a chunk call keeps those two in the caller's
// state, behind the predictor's.
struct NgramWork {
  float *cq, *lm_sum;              // [B][kMaxCand], [R]
  int *cnext, *ctx;                // [B][kMaxCand], [R]
};

NgramWork carve_ngram(int B, int beam, Arena& m, bool rows) {
  NgramWork w{};
  w.cq = m.take<float>((size_t)B * kMaxCand);
  w.cnext = m.take<int>((size_t)B * kMaxCand);
  if (rows) {
    w.ctx = m.take<int>((size_t)B * beam);
    w.lm_sum = m.take<float>((size_t)B * beam);
  }
  return w;
}

struct NgramStreamState {
  int* ctx;                        // [R]
  float* lm_sum;                   // [R]
};

// (the order is the header's documented layout)
NgramStreamState carve_ngram_state(int B, int beam, Arena& m) {
  NgramStreamState s{};
  s.ctx = m.take<int>((size_t)B * beam);
  s.lm_sum = m.take<float>((size_t)B * beam);
  return s;
}

// grid B, after stream_reset_kernel: the one live beam of a row the mask names starts in start_ctx with
// lm_sum 0; the other rows keep every bit
__global__ __launch_bounds__(64) void ngram_stream_reset_kernel(const int* rows, int BS, int start_ctx, int* ctx,
                                                                float* lm_sum) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (rows && rows[b] == 0) return;
  if (tid < BS) {
    ctx[b * BS + tid] = start_ctx;
    lm_sum[b * BS + tid] = 0.f;
  }
}

struct Chunk {                     // a chunk call: the caller's state, and what it answers beside the search's outputs
  void* state;
  int max_tokens;
  long* stable_len;
  int* overflow;
};

bool beam_ok(int beam, int least) { return beam >= least && beam <= kMaxBeam; }
bool chunk_ok(int Tc) { return Tc >= 1 && Tc <= kMaxChunk; }
bool fusion_ok(const S2tRnnLmDesc* lm, int V) { return lm_ok(lm) && lm->V == V; }
bool fusion_ok(const Fusion& f, int V) {
  return f.ngram ? !f.lm && ngram_desc_ok(f.ngram) && f.ngram->V == V : fusion_ok(f.lm, V);
}

// The T rounds of a beam search: frame t reads buf[t & 1] and leaves the survivors in buf[~t & 1], by the
// predictor's step on a.token / a.emit / a.parent / a.counts + cur.  With an LM (shallow fusion) its step
// follows the predictor's on the same four, from its buffer cur to nxt; with an n-gram (ng) the two
// kernels run in their n-gram mode and nothing follows.
template <class P>
void beam_rounds(const P& p, BeamArgs a, const typename P::Buf (&buf)[2], const typename P::Work& w,
                 const S2tRnnLmDesc* lm, const LmWorkspace& lw, const BeamNgram* ng, int T, hipStream_t st) {
  const int R = a.B * a.beam;
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    a.t = t;
    a.parity = cur;
    a.lm = buf[cur].lm;
    if (lm) a.q = lw.q[cur];
    if (ng) {                                              // (no LM step: a kept row took its context in select)
      const BeamNgramArgs na{a, *ng};
      hipLaunchKernelGGL(beam_expand_kernel<BeamNgramArgs>, dim3(R), dim3(kThreads), 0, st, na);
      hipLaunchKernelGGL(beam_select_kernel<BeamNgramArgs>, dim3(a.B), dim3(kThreads), 0, st, na);
    } else {
      hipLaunchKernelGGL(beam_expand_kernel<BeamArgs>, dim3(R), dim3(kThreads), 0, st, a);
      hipLaunchKernelGGL(beam_select_kernel<BeamArgs>, dim3(a.B), dim3(kThreads), 0, st, a);
    }
    p.step(R, w, a.parent, a.counts + cur, buf[cur], buf[nxt], st);
    if (lm)
      enqueue_lm_step(*lm, R, a.token, a.emit, a.parent, a.counts + cur, lw.h[cur], lw.c[cur], lw.q[cur],
                      lw.h[nxt], lw.c[nxt], lw.q[nxt], lw, st);
  }
}

// Every lockstep beam entry point: predictor p, with an LM or not (f NULL), the whole utterance (ch NULL:
// state in the workspace, blanked here, the best beam traced back at the end) or one chunk of it (the live
// state is the caller's: frame 0 reads it, an odd T copies the survivors home, the records become histories).
template <class P>
int beam_search(const P& p, const Fusion* f, const Chunk* ch, const float* am, const long* lengths, int B, int T,
                int beam, int topk, void* workspace, long* tokens, long* frames, long* out_len, float* score,
                hipStream_t st) {
  if (B <= 0) return 0;
  if (!p.ok() || (f && !fusion_ok(*f, p.V())) || !beam_ok(beam, 1) || topk < 1 ||
      (topk < p.V() ? topk : p.V()) > kMaxBeam || (f && f->start_token >= p.V()) ||
      (f && !__builtin_isfinite(f->weight)) || (ch ? !chunk_ok(T) || ch->max_tokens < 1 || !ch->state : T <= 0) ||
      !workspace)
    return -1;
  const S2tNgramLmDesc* ngram = f ? f->ngram : nullptr;
  if (ngram && (!f->lm_score || (!ch && (f->start_ctx < 0 || f->start_ctx >= ngram->num_ctx)))) return -1;
  const S2tRnnLmDesc* lm = f ? f->lm : nullptr;
  const int R = B * beam, n_state = ch ? 1 : 2;
  Arena wm(workspace);
  const typename P::Work w = p.work(B, T, beam, wm, n_state);
  const SearchArrays& s = w.s;
  LmWorkspace lw{};
  if (lm) lw = carve_lm(*lm, B, beam, wm, n_state);
  NgramWork nw{};
  if (ngram) nw = carve_ngram(B, beam, wm, !ch);
  typename P::State carried{};     // a chunk: the caller's state; buf[0] is its live copy
  typename P::Buf buf[2] = {w.buf[0], w.buf[1]};
  if (ch) {
    Arena sm(ch->state);
    carried = p.state(B, beam, ch->max_tokens, sm);
    buf[1] = buf[0];
    buf[0] = carried.live;
    if (lm) lw = live_lm(lw, carve_lm_state(*lm, B, beam, sm));
    if (ngram) {
      const NgramStreamState ns = carve_ngram_state(B, beam, sm);
      nw.ctx = ns.ctx;
      nw.lm_sum = ns.lm_sum;
    }
    hipLaunchKernelGGL(beam_chunk_init_kernel, dim3(1), dim3(64), 0, st, s.counts, R);
  } else {
    hipError_t e = p.blank(buf[0], R, st);
    if (lm) {
      const size_t lm_state = sizeof(float) * (size_t)lm->num_layers * R * lm->H;
      if (e == hipSuccess) e = hipMemsetAsync(lw.h[0], 0, lm_state, st);
      if (e == hipSuccess) e = hipMemsetAsync(lw.c[0], 0, lm_state, st);
      if (e == hipSuccess) e = hipMemsetAsync(lw.q[0], 0, sizeof(float) * (size_t)R * p.V(), st);
    }
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(beam_init_kernel, dim3(1), dim3(kThreads), 0, st, B, beam, s.score, s.blen, s.nb, s.emit,
                       s.token, s.counts);
    if (lm)
      hipLaunchKernelGGL(lm_start_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, R,
                         f->start_token, lw.tok, lw.lm_sum);
    if (ngram)                                             // every row in start_ctx, lm_sum 0
      hipLaunchKernelGGL(lm_start_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, R,
                         f->start_ctx, nw.ctx, nw.lm_sum);
    p.step(R, w, nullptr, s.counts + 2, buf[0], buf[0], st);   // the first step: blank, from the blanked state
    if (lm && f->start_token >= 0)                          // the LM's first step, as the predictor's on blank
      enqueue_lm_step(*lm, R, lw.tok, s.emit, nullptr, s.counts + 2, lw.h[0], lw.c[0], lw.q[0], lw.h[0], lw.c[0],
                      lw.q[0], lw, st);
  }
  BeamArgs a{};                    // (t, parity, lm and q are the round's)
  a.j = p.joint(am, T, w);
  a.lengths = lengths;
  a.B = B;
  a.beam = beam;
  a.topk = topk;
  a.cscore = s.cscore;
  a.ccls = s.ccls;
  a.score = ch ? carried.score : s.score;
  a.blen = ch ? carried.blen : s.blen;
  a.nb = ch ? carried.nb : s.nb;
  a.rec = s.rec;
  a.emit = s.emit;
  a.token = s.token;
  a.parent = s.parent;
  a.counts = s.counts;
  if (f) {                         // else q stays NULL: no fusion (an n-gram: q stays NULL too, no LM rows)
    a.lm_weight = f->weight;
    a.cq = ngram ? nw.cq : lw.cq;
    a.lm_sum = ngram ? nw.lm_sum : lw.lm_sum;
  }
  BeamNgram bn{};
  if (ngram) bn = BeamNgram{ngram_tables(*ngram), nw.ctx, nw.cnext};
  beam_rounds(p, a, buf, w, lm, lw, ngram ? &bn : nullptr, T, st);
  const float* lm_sum = f ? a.lm_sum : nullptr;
  float* lm_score = f ? f->lm_score : nullptr;
  if (ch) {
    if (T & 1) {                                           // the live copies go home
      HomeList l;
      p.home(l, R, buf[1], buf[0]);
      if (lm) {
        const long n_lstate = (long)lm->num_layers * R * lm->H;
        l.add(lw.h[1], lw.h[0], n_lstate);
        l.add(lw.c[1], lw.c[0], n_lstate);
        l.add(lw.q[1], lw.q[0], (long)R * p.V());
      }
      enqueue_copy_home(l.c, st);
    }
    BeamEndArgs e{lengths, T, beam, ch->max_tokens, s.rec, carried.blen, carried.nb, carried.score, carried.hdr,
                  carried.htok, carried.hfrm, tokens, frames, out_len, score, ch->stable_len, ch->overflow, lm_sum, lm_score};
    hipLaunchKernelGGL(beam_chunk_end_kernel, dim3(B), dim3(kThreads), 0, st, e);
  } else {
    hipLaunchKernelGGL(beam_trace_kernel, dim3(B), dim3(64), 0, st, lengths, T, beam, s.rec, s.blen, s.score,
                       tokens, frames, out_len, score, lm_sum, lm_score);
  }
  S2T_CHECK_LAUNCH();
  return 0;
}

// Every stream reset: the rows the mask names become the empty hypothesis (with an LM: its state too), then
// the one-shot call's own first step(s) with emit = the mask.
template <class P>
int stream_reset(const P& p, const Fusion* f, void* state, const int* rows, int B, int beam, int max_tokens,
                 void* workspace, hipStream_t st) {
  if (B <= 0) return 0;
  if (!p.ok() || (f && !fusion_ok(*f, p.V())) || !beam_ok(beam, f ? 1 : 0) || max_tokens < 1 ||
      (f && f->start_token >= p.V()) || (f && f->ngram && f->start_ctx < 0) || !state || !workspace)
    return -1;
  const S2tRnnLmDesc* lm = f ? f->lm : nullptr;
  const int BS = beam > 0 ? beam : 1, R = B * BS;
  Arena sm(state), wm(workspace);
  const typename P::State s = p.state(B, beam, max_tokens, sm);
  const typename P::Work w = p.work(B, 1, beam, wm, beam > 0 ? 1 : 0);
  LmStreamState ls{};
  LmWorkspace lw{};
  if (lm) {
    ls = carve_lm_state(*lm, B, beam, sm);
    lw = carve_lm(*lm, B, beam, wm, 1);
  }
  NgramStreamState ns{};
  if (f && f->ngram) ns = carve_ngram_state(B, beam, sm);
  // as for a predictor without LSTM layers or context; the predictor fills in its own
  ResetArgs a{rows, beam, BS, 0, 0, nullptr, nullptr, s.score, s.blen, s.nb, s.hdr, nullptr, w.s.emit, w.s.token};
  LmResetArgs la{rows, BS, lm ? lm->num_layers : 0, lm ? lm->H : 0, p.V(), 0, lm ? f->start_token : -1,
                 ls.h, ls.c, ls.q, ls.lm_sum, lw.tok, nullptr};
  p.reset_args(s, a, la);
  hipLaunchKernelGGL(stream_reset_kernel, dim3(B), dim3(kThreads), 0, st, a);
  if (lm) hipLaunchKernelGGL(lm_stream_reset_kernel, dim3(B), dim3(kThreads), 0, st, la);
  if (ns.ctx)
    hipLaunchKernelGGL(ngram_stream_reset_kernel, dim3(B), dim3(64), 0, st, rows, BS, f->start_ctx, ns.ctx, ns.lm_sum);
  hipLaunchKernelGGL(count_kernel, dim3(1), dim3(kThreads), 0, st, w.s.emit, R, w.s.counts + 2);
  p.step(R, w, nullptr, w.s.counts + 2, s.live, s.live, st);
  if (lm && f->start_token >= 0)                           // the LM's first step, as the predictor's on blank
    enqueue_lm_step(*lm, R, lw.tok, w.s.emit, nullptr, w.s.counts + 2, ls.h, ls.c, ls.q, ls.h, ls.c, ls.q, lw,
                    st);
  S2T_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ sizes, on the host (bytes_of: decode_records.h)
// a fused search's workspace: the predictor's, then the LM's
template <class P>
long fused_workspace_bytes(const P& p, const Fusion& f, int B, int T, int beam, int n_state) {
  if (!p.ok() || !fusion_ok(f, p.V()) || B <= 0 || T < 0 || !beam_ok(beam, 1)) return 0;
  return bytes_of([&](Arena& m) {
    p.work(B, T, beam, m, n_state);
    if (f.ngram) carve_ngram(B, beam, m, n_state == 2);
    else carve_lm(*f.lm, B, beam, m, n_state);
  });
}

// a fused search's stream state: the predictor's, then the LM's
template <class P>
long fused_state_bytes(const P& p, const Fusion& f, int B, int beam, int max_tokens) {
  if (B <= 0 || !p.ok() || !fusion_ok(f, p.V()) || !beam_ok(beam, 1) || max_tokens < 1) return 0;
  return bytes_of([&](Arena& m) {
    p.state(B, beam, max_tokens, m);
    if (f.ngram) carve_ngram_state(B, beam, m);
    else carve_lm_state(*f.lm, B, beam, m);
  });
}

Fusion rnn_fusion(const S2tRnnLmDesc* lm, float weight = 0.f, int start_token = -1, float* lm_score = nullptr) {
  return Fusion{lm, weight, start_token, lm_score};
}

Fusion ngram_fusion(const S2tNgramLmDesc* lm, float weight = 0.f, int start_ctx = 0, float* lm_score = nullptr) {
  Fusion f{nullptr, weight, -1, lm_score};
  f.ngram = lm;
  f.start_ctx = start_ctx;
  return f;
}

}  // namespace

extern "C" {

long s2t_rnnt_lstm_workspace_bytes(const S2tRnntLstmDesc* desc, int B, int T, int beam_size) {
  if (!desc_ok(desc) || B <= 0 || T < 0 || !beam_ok(beam_size, 0)) return 0;
  return bytes_of([&](Arena& m) { carve(*desc, B, T, beam_size, m); });
}

int s2t_lstm_pred_step(const S2tRnntLstmDesc* desc, int R, const int* tokens, const int* emit,
                       const int* parent, const float* h_in, const float* c_in, const float* lm_in,
                       float* h_out, float* c_out, float* lm_out, void* workspace, void* stream) {
  if (R <= 0) return 0;
  if (!desc_ok(desc) || !workspace) return -1;
  const bool same = h_in == h_out;
  if (same != (c_in == c_out) || same != (lm_in == lm_out) || (same && parent)) return -1;
  Arena m(workspace);
  const Workspace w = carve(*desc, R, 0, 0, m);
  hipLaunchKernelGGL(count_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, emit, R, w.s.counts);
  enqueue_pred_step(*desc, R, tokens, emit, parent, w.s.counts, h_in, c_in, lm_in, h_out, c_out, lm_out, w,
                    (hipStream_t)stream);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_rnnt_greedy_lstm(const S2tRnntLstmDesc* desc, const float* am, const long* lengths, int B,
                         int T, int max_token_step, void* workspace, long* tokens, long* out_len,
                         void* stream) {
  if (B <= 0) return 0;
  if (!desc_ok(desc) || T <= 0 || max_token_step < 0 || !workspace) return -1;
  const LstmPredictor p{desc};
  hipStream_t st = (hipStream_t)stream;
  Arena m(workspace);
  const Workspace w = p.work(B, T, 0, m, 2);
  const SearchArrays& s = w.s;
  const StateBuf& b = w.buf[0];
  const hipError_t e = p.blank(b, B, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(greedy_init_kernel, dim3(1), dim3(kThreads), 0, st, lengths, B, T, w.t, w.nts, w.done,
                     s.emit, s.token, s.counts, out_len);
  p.step(B, w, nullptr, s.counts + 2, b, b, st);
  GreedyArgs g{p.joint(am, T, w), lengths, b.lm, max_token_step, T * (max_token_step + 1), 0,
               w.t, w.nts, w.done, s.emit, s.token, s.counts, tokens, out_len};
  return greedy_rounds(*desc, B, g, b.h, b.c, b.lm, w, (long)T * (max_token_step + 2), 1, st);
}

int s2t_rnnt_beam_lstm(const S2tRnntLstmDesc* desc, const float* am, const long* lengths, int B,
                       int T, int beam_size, int cutoff_top_k, void* workspace, long* tokens,
                       long* frames, long* out_len, float* score, void* stream) {
  return beam_search(LstmPredictor{desc}, nullptr, nullptr, am, lengths, B, T, beam_size, cutoff_top_k, workspace,
                     tokens, frames, out_len, score, (hipStream_t)stream);
}

long s2t_rnn_lm_step_workspace_bytes(const S2tRnnLmDesc* lm, int R) {
  if (!lm_ok(lm) || R <= 0) return 0;
  return bytes_of([&](Arena& m) { carve_lm(*lm, R, 0, m, 0); });
}

int s2t_rnn_lm_step(const S2tRnnLmDesc* lm, int R, const int* tokens, const int* emit, const int* parent,
                    const float* h_in, const float* c_in, const float* q_in, float* h_out, float* c_out,
                    float* q_out, void* workspace, void* stream) {
  if (R <= 0) return 0;
  if (!lm_ok(lm) || !workspace) return -1;
  const bool same = h_in == h_out;
  if (same != (c_in == c_out) || same != (q_in == q_out) || (same && parent)) return -1;
  Arena m(workspace);
  const LmWorkspace w = carve_lm(*lm, R, 0, m, 0);
  hipLaunchKernelGGL(count_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, emit, R, w.counts);
  enqueue_lm_step(*lm, R, tokens, emit, parent, w.counts, h_in, c_in, q_in, h_out, c_out, q_out, w,
                  (hipStream_t)stream);
  S2T_CHECK_LAUNCH();
  return 0;
}

long s2t_rnnt_beam_lstm_lm_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int B, int T,
                                           int beam_size) {
  return fused_workspace_bytes(LstmPredictor{desc}, rnn_fusion(lm), B, T, beam_size, 2);
}

int s2t_rnnt_beam_lstm_lm(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, const float* am,
                          const long* lengths, int B, int T, int beam_size, int cutoff_top_k, float lm_weight,
                          int lm_start_token, void* workspace, long* tokens, long* frames, long* out_len,
                          float* score, float* lm_score, void* stream) {
  const Fusion f{lm, lm_weight, lm_start_token, lm_score};
  return beam_search(LstmPredictor{desc}, &f, nullptr, am, lengths, B, T, beam_size, cutoff_top_k, workspace,
                     tokens, frames, out_len, score, (hipStream_t)stream);
}

long s2t_stateless_pred_step_workspace_bytes(const S2tRnntStatelessDesc* desc, int R) {
  if (!stateless_ok(desc) || R <= 0) return 0;
  return bytes_of([&](Arena& m) { carve_stateless(*desc, R, 0, 0, m, 0); });
}

int s2t_stateless_pred_step(const S2tRnntStatelessDesc* desc, int R, const int* tokens, const int* emit,
                            const int* parent, const int* ctx_in, const float* lm_in, int* ctx_out,
                            float* lm_out, void* workspace, void* stream) {
  if (R <= 0) return 0;
  if (!stateless_ok(desc) || !workspace) return -1;
  const bool same = ctx_in == ctx_out;
  if (same != (lm_in == lm_out) || (same && parent)) return -1;
  Arena m(workspace);
  const StatelessWorkspace w = carve_stateless(*desc, R, 0, 0, m, 0);
  hipLaunchKernelGGL(count_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, emit, R, w.s.counts);
  enqueue_stateless_step(*desc, R, tokens, emit, parent, w.s.counts, ctx_in, lm_in, ctx_out, lm_out, w,
                         (hipStream_t)stream);
  S2T_CHECK_LAUNCH();
  return 0;
}

long s2t_rnnt_beam_stateless_lm_workspace_bytes(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm, int B,
                                                int T, int beam_size) {
  return fused_workspace_bytes(StatelessPredictor{desc}, rnn_fusion(lm), B, T, beam_size, 2);
}

int s2t_rnnt_beam_stateless_lm(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm, const float* am,
                               const long* lengths, int B, int T, int beam_size, int cutoff_top_k,
                               float lm_weight, int lm_start_token, void* workspace, long* tokens,
                               long* frames, long* out_len, float* score, float* lm_score, void* stream) {
  const Fusion f{lm, lm_weight, lm_start_token, lm_score};
  return beam_search(StatelessPredictor{desc}, &f, nullptr, am, lengths, B, T, beam_size, cutoff_top_k, workspace,
                     tokens, frames, out_len, score, (hipStream_t)stream);
}

long s2t_rnnt_lstm_stream_state_bytes(const S2tRnntLstmDesc* desc, int B, int beam_size, int max_tokens) {
  if (B <= 0 || !desc_ok(desc) || !beam_ok(beam_size, 0) || max_tokens < 1) return 0;
  return bytes_of([&](Arena& m) { carve_state(*desc, B, beam_size, max_tokens, m); });
}

long s2t_rnnt_lstm_stream_workspace_bytes(const S2tRnntLstmDesc* desc, int B, int Tc, int beam_size) {
  if (!desc_ok(desc) || B <= 0 || !chunk_ok(Tc) || !beam_ok(beam_size, 0)) return 0;
  return bytes_of([&](Arena& m) { carve(*desc, B, Tc, beam_size, m, beam_size > 0 ? 1 : 0); });
}

int s2t_rnnt_lstm_stream_reset(const S2tRnntLstmDesc* desc, void* state, const int* rows, int B,
                               int beam_size, int max_tokens, void* workspace, void* stream) {
  return stream_reset(LstmPredictor{desc}, nullptr, state, rows, B, beam_size, max_tokens, workspace,
                      (hipStream_t)stream);
}

int s2t_rnnt_greedy_lstm_chunk(const S2tRnntLstmDesc* desc, const float* am, const long* chunk_len, int B,
                               int Tc, int max_token_step, int max_tokens, int host_poll, void* state,
                               void* workspace, long* tokens, long* out_len, int* overflow, void* stream) {
  if (B <= 0) return 0;
  if (!desc_ok(desc) || max_tokens < 1 || !chunk_ok(Tc) || max_token_step < 0 || !state || !workspace) return -1;
  const S2tRnntLstmDesc& d = *desc;
  hipStream_t st = (hipStream_t)stream;
  Arena sm(state), wm(workspace);
  const StreamState s = carve_state(d, B, 0, max_tokens, sm);
  const Workspace w = carve(d, B, Tc, 0, wm, 0);
  hipLaunchKernelGGL(greedy_chunk_init_kernel, dim3(1), dim3(kThreads), 0, st, chunk_len, B, w.t, w.nts, w.done,
                     w.s.emit, w.s.token, w.s.counts);
  // the walk's own counter of symbols is the state's: it appends to the caller's tokens at the
  // stream's length and goes on counting past max_tokens
  GreedyArgs g{joint_args(d, am, Tc, w.s), chunk_len, s.live.lm, max_token_step, max_tokens, 0,
               w.t, w.nts, w.done, w.s.emit, w.s.token, w.s.counts, tokens, s.n};
  const int rc = greedy_rounds(d, B, g, s.live.h, s.live.c, s.live.lm, w, (long)Tc * (max_token_step + 2), host_poll,
                               st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(greedy_chunk_end_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                     chunk_len, B, Tc, max_tokens, s.n, s.hdr, out_len, overflow);
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_rnnt_beam_lstm_chunk(const S2tRnntLstmDesc* desc, const float* am, const long* chunk_len, int B,
                             int Tc, int beam_size, int cutoff_top_k, int max_tokens, void* state,
                             void* workspace, long* tokens, long* frames, long* out_len, float* score,
                             long* stable_len, int* overflow, void* stream) {
  const Chunk ch{state, max_tokens, stable_len, overflow};
  return beam_search(LstmPredictor{desc}, nullptr, &ch, am, chunk_len, B, Tc, beam_size, cutoff_top_k, workspace,
                     tokens, frames, out_len, score, (hipStream_t)stream);
}

long s2t_rnnt_lstm_lm_stream_state_bytes(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int B,
                                         int beam_size, int max_tokens) {
  return fused_state_bytes(LstmPredictor{desc}, rnn_fusion(lm), B, beam_size, max_tokens);
}

long s2t_rnnt_lstm_lm_stream_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int B, int Tc,
                                             int beam_size) {
  return chunk_ok(Tc) ? fused_workspace_bytes(LstmPredictor{desc}, rnn_fusion(lm), B, Tc, beam_size, 1) : 0;
}

int s2t_rnnt_lstm_lm_stream_reset(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int lm_start_token,
                                  void* state, const int* rows, int B, int beam_size, int max_tokens,
                                  void* workspace, void* stream) {
  const Fusion f{lm, 0.f, lm_start_token, nullptr};
  return stream_reset(LstmPredictor{desc}, &f, state, rows, B, beam_size, max_tokens, workspace,
                      (hipStream_t)stream);
}

int s2t_rnnt_beam_lstm_lm_chunk(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, const float* am,
                                const long* chunk_len, int B, int Tc, int beam_size, int cutoff_top_k,
                                float lm_weight, int max_tokens, void* state, void* workspace, long* tokens,
                                long* frames, long* out_len, float* score, float* lm_score, long* stable_len,
                                int* overflow, void* stream) {
  const Fusion f{lm, lm_weight, -1, lm_score};
  const Chunk ch{state, max_tokens, stable_len, overflow};
  return beam_search(LstmPredictor{desc}, &f, &ch, am, chunk_len, B, Tc, beam_size, cutoff_top_k, workspace, tokens,
                     frames, out_len, score, (hipStream_t)stream);
}

// ---- the LSTM predictor's beam search with a back-off n-gram: the RNN-LM family's siblings
long s2t_rnnt_beam_lstm_ngram_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int B, int T,
                                              int beam_size) {
  return fused_workspace_bytes(LstmPredictor{desc}, ngram_fusion(lm), B, T, beam_size, 2);
}

int s2t_rnnt_beam_lstm_ngram(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, const float* am,
                             const long* lengths, int B, int T, int beam_size, int cutoff_top_k, float lm_weight,
                             int start_ctx, void* workspace, long* tokens, long* frames, long* out_len,
                             float* score, float* lm_score, void* stream) {
  const Fusion f = ngram_fusion(lm, lm_weight, start_ctx, lm_score);
  return beam_search(LstmPredictor{desc}, &f, nullptr, am, lengths, B, T, beam_size, cutoff_top_k, workspace,
                     tokens, frames, out_len, score, (hipStream_t)stream);
}

long s2t_rnnt_lstm_ngram_stream_state_bytes(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int B,
                                            int beam_size, int max_tokens) {
  return fused_state_bytes(LstmPredictor{desc}, ngram_fusion(lm), B, beam_size, max_tokens);
}

long s2t_rnnt_lstm_ngram_stream_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int B,
                                                int Tc, int beam_size) {
  return chunk_ok(Tc) ? fused_workspace_bytes(LstmPredictor{desc}, ngram_fusion(lm), B, Tc, beam_size, 1) : 0;
}

int s2t_rnnt_lstm_ngram_stream_reset(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int start_ctx,
                                     void* state, const int* rows, int B, int beam_size, int max_tokens,
                                     void* workspace, void* stream) {
  const Fusion f = ngram_fusion(lm, 0.f, start_ctx, nullptr);
  return stream_reset(LstmPredictor{desc}, &f, state, rows, B, beam_size, max_tokens, workspace,
                      (hipStream_t)stream);
}

int s2t_rnnt_beam_lstm_ngram_chunk(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, const float* am,
                                   const long* chunk_len, int B, int Tc, int beam_size, int cutoff_top_k,
                                   float lm_weight, int max_tokens, void* state, void* workspace, long* tokens,
                                   long* frames, long* out_len, float* score, float* lm_score, long* stable_len,
                                   int* overflow, void* stream) {
  const Fusion f = ngram_fusion(lm, lm_weight, 0, lm_score);
  const Chunk ch{state, max_tokens, stable_len, overflow};
  return beam_search(LstmPredictor{desc}, &f, &ch, am, chunk_len, B, Tc, beam_size, cutoff_top_k, workspace, tokens,
                     frames, out_len, score, (hipStream_t)stream);
}

long s2t_rnnt_stateless_lm_stream_state_bytes(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm, int B,
                                              int beam_size, int max_tokens) {
  return fused_state_bytes(StatelessPredictor{desc}, rnn_fusion(lm), B, beam_size, max_tokens);
}

long s2t_rnnt_stateless_lm_stream_workspace_bytes(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm, int B,
                                                  int Tc, int beam_size) {
  return chunk_ok(Tc) ? fused_workspace_bytes(StatelessPredictor{desc}, rnn_fusion(lm), B, Tc, beam_size, 1) : 0;
}

int s2t_rnnt_stateless_lm_stream_reset(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm,
                                       int lm_start_token, void* state, const int* rows, int B, int beam_size,
                                       int max_tokens, void* workspace, void* stream) {
  const Fusion f{lm, 0.f, lm_start_token, nullptr};
  return stream_reset(StatelessPredictor{desc}, &f, state, rows, B, beam_size, max_tokens, workspace,
                      (hipStream_t)stream);
}

int s2t_rnnt_beam_stateless_lm_chunk(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm, const float* am,
                                     const long* chunk_len, int B, int Tc, int beam_size, int cutoff_top_k,
                                     float lm_weight, int max_tokens, void* state, void* workspace,
                                     long* tokens, long* frames, long* out_len, float* score, float* lm_score,
                                     long* stable_len, int* overflow, void* stream) {
  const Fusion f{lm, lm_weight, -1, lm_score};
  const Chunk ch{state, max_tokens, stable_len, overflow};
  return beam_search(StatelessPredictor{desc}, &f, &ch, am, chunk_len, B, Tc, beam_size, cutoff_top_k, workspace,
                     tokens, frames, out_len, score, (hipStream_t)stream);
}

}  // extern "C"

