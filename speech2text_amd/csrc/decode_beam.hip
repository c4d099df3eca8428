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
// After the last frame the best beam (position 0) is traced back through the records.
// lm [beam_size][V] lives in LDS when it fits and in the workspace (L2 resident) when it does not.
#include "common.h"
#include "decode_common.h"

namespace {

constexpr int kMaxBeam = 16;       // beams, and classes kept per beam
constexpr int kMaxCand = kMaxBeam * kMaxBeam;
constexpr int kGroup = 4;          // beams per pass over the predictor weights
constexpr int kRows = 4;           // weight rows in flight per wave in that pass ...
constexpr int kCols = 4;           // ... and 64-column steps of each row loaded before they are used
constexpr int kWaves = 8;          // waves per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kRegs = 8;           // classes per lane held in registers (V <= 512)
constexpr int kTraceFrames = 64;   // frames of records staged in LDS per trace-back step
constexpr size_t kLdsBudget = 60 * 1024;

using namespace s2t_dec;           // Top, better, wave_top, after, activate (decode_common.h)

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
  int* records;           // [B][T][beam]  parent position | class << 4
  float* lm_spill;        // [B][beam][V]  (used when lm does not fit the LDS)
  long* tokens;           // [B][T]
  long* frames;           // [B][T]
  long* out_len;          // [B]
  float* score;           // [B]
};

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
__device__ void recompute_lm(const BeamArgs& a, const int* __restrict__ list, int n,
                             const int* __restrict__ state, const int* __restrict__ slot,
                             float* __restrict__ e, float* __restrict__ h, float* lm) {
  const int tid = threadIdx.x;
  for (int g0 = 0; g0 < n; g0 += kGroup) {
    const int ng = min(kGroup, n - g0);
    for (int x = tid; x < ng * a.E; x += kThreads) {
      const int g = x / a.E, c = x - g * a.E;
      const int* st = state + list[g0 + g] * a.ctx;
      float acc = 0.f;
      for (int k0 = 0; k0 < a.ctx; k0 += kCols) {          // (loads first, clamped, as in gemv_group)
        float cw[kCols], ev[kCols];
#pragma unroll
        for (int q = 0; q < kCols; ++q) {
          const int k = min(k0 + q, a.ctx - 1);
          cw[q] = a.conv_w[c * a.ctx + k];
          ev[q] = a.emb[(long)st[k] * a.E + c];
        }
#pragma unroll
        for (int q = 0; q < kCols; ++q) acc = k0 + q < a.ctx ? fmaf(cw[q], ev[q], acc) : acc;
      }
      e[g * a.E + c] = acc;
    }
    __syncthreads();
    gemv_group(a.lin_w, a.lin_b, e, a.D, a.E, ng, [&](int g, int r, float y) { h[g * a.D + r] = y; });
    __syncthreads();
    gemv_group(a.pre_w, a.pre_b, h, a.V, a.D, ng,
               [&](int g, int r, float y) { lm[(long)slot[list[g0 + g]] * a.V + r] = y; });
    __syncthreads();
  }
}

template <bool CACHE>
__global__ __launch_bounds__(kThreads) void rnnt_beam_kernel(BeamArgs a) {
  extern __shared__ float sm[];
  __shared__ float s_cscore[kMaxCand];          // candidates of this frame: score, class
  __shared__ int s_ccls[kMaxCand];
  __shared__ int s_pick[kMaxBeam];              // candidate index of each new beam
  __shared__ float s_score[2][kMaxBeam];        // beams, double-buffered over frames
  __shared__ int s_slot[2][kMaxBeam];           // lm row of each beam
  __shared__ int s_len[2][kMaxBeam];            // tokens emitted so far
  __shared__ int s_emit[kMaxBeam];              // beams whose lm is to be recomputed
  __shared__ int s_nemit;
  __shared__ int s_trace[kTraceFrames * kMaxBeam];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V, K = min(a.topk, V), BS = a.beam;
  float* e = sm;                                           // [kGroup][E]
  float* h = e + kGroup * a.E;                             // [kGroup][D]
  int* state = reinterpret_cast<int*>(h + kGroup * a.D);   // [2][kMaxBeam][ctx], most recent last
  float* lm = a.lm_in_lds ? reinterpret_cast<float*>(state + 2 * kMaxBeam * a.ctx)
                          : a.lm_spill + (long)b * BS * V;  // [beam][V]
  long Tb = a.lengths[b];
  if (Tb > a.T) Tb = a.T;
  if (Tb < 0) Tb = 0;
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
    s_score[0][0] = 0.f;
    s_slot[0][0] = 0;
    s_len[0][0] = 0;
    s_emit[0] = 0;
  }
  __syncthreads();
  recompute_lm(a, s_emit, 1, state, s_slot[0], e, h, lm);
  int nb = 1, cur = 0;

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
      const float* lmi = lm + (long)s_slot[cur][i] * V;
      const float base = s_score[cur][i];
      float zr[kRegs];
      if (CACHE) {
#pragma unroll
        for (int j = 0; j < kRegs; ++j) {
          const int c = lane + 64 * j;
          zr[j] = c < V ? activate(am_cur[j] + lmi[min(c, V - 1)], a.act) : S2T_NEG_INF;
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
            const float z = activate(amt[c] + lmi[c], a.act);
            if (r == 0 || after(z, c, pv, pi)) best = better(best, Top{z, c});
          }
        }
        best = wave_top(best);
        pv = best.v;
        pi = best.i;
        if (r == 0) {                                      // log-softmax as max, then log sum exp
          zmax = pv;
          float s = 0.f;
          if (CACHE) {
#pragma unroll
            for (int j = 0; j < kRegs; ++j)
              if (lane + 64 * j < V) s += expf(zr[j] - zmax);
          } else {
            for (int c = lane; c < V; c += 64) s += expf(activate(amt[c] + lmi[c], a.act) - zmax);
          }
          lse = logf(wave_sum(s));
        }
        if (lane == 0) {
          const bool ok = pi < V;                          // (only a NaN input leaves a round empty)
          s_cscore[i * K + r] = ok ? base + ((pv - zmax) - lse) : S2T_NEG_INF;
          s_ccls[i * K + r] = ok ? pi : a.blank;
        }
      }
    }
    __syncthreads();
    // ---- B: rank the candidates, keep the beam_size best
    const int nc = nb * K, nnb = min(nc, BS), nxt = cur ^ 1;
    if (tid < nc) {
      const float mine = s_cscore[tid];
      int rank = 0;
      for (int q = 0; q < nc; ++q) {
        const float o = s_cscore[q];
        rank += (o > mine || (o == mine && q < tid)) ? 1 : 0;
      }
      if (rank < nnb) s_pick[rank] = tid;
    }
    __syncthreads();
    // ---- C: the new beams (wave 0, a lane per beam)
    if (wave == 0) {
      const bool live = lane < nnb;
      int parent = 0, cls = a.blank;
      if (live) {
        const int q = s_pick[lane];
        parent = q / K;
        cls = s_ccls[q];
        s_score[nxt][lane] = s_cscore[q];
        s_len[nxt][lane] = s_len[cur][parent] + (cls != a.blank ? 1 : 0);
        rec[(long)t * BS + lane] = parent | (cls << 4);
        const int* so = state + (cur * kMaxBeam + parent) * a.ctx;
        int* sn = state + (nxt * kMaxBeam + lane) * a.ctx;
        if (cls == a.blank) {
          for (int k = 0; k < a.ctx; ++k) sn[k] = so[k];
        } else {
          for (int k = 0; k + 1 < a.ctx; ++k) sn[k] = so[k + 1];
          sn[a.ctx - 1] = cls;
        }
      }
      const bool emits = live && cls != a.blank;
      // lm rows: a blank child keeps its parent's row (a parent has at most one); the emitting
      // beams take the rows that are left, in beam order
      unsigned used = (live && !emits) ? 1u << s_slot[cur][parent] : 0u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) used |= __shfl_xor(used, o, 64);
      const unsigned long long em = __ballot(emits);
      int myslot = live ? s_slot[cur][parent] : 0;
      if (emits) {
        int order = __popcll(em & ((1ull << lane) - 1ull));
        s_emit[order] = lane;
        for (int s = 0; s < kMaxBeam; ++s)
          if (!((used >> s) & 1u)) {
            if (order == 0) {
              myslot = s;
              break;
            }
            --order;
          }
      }
      if (live) s_slot[nxt][lane] = myslot;
      if (lane == 0) s_nemit = __popcll(em);
    }
    __syncthreads();
    // ---- D: lm of the beams that emitted (at most one symbol per frame per beam)
    const int ne = s_nemit;
    if (ne > 0) recompute_lm(a, s_emit, ne, state + nxt * kMaxBeam * a.ctx, s_slot[nxt], e, h, lm);
    nb = nnb;
    cur = nxt;
    if (CACHE) {
#pragma unroll
      for (int j = 0; j < kRegs; ++j) am_cur[j] = am_next[j];
    }
  }

  // ---- the best beam is position 0: trace its (parent, class) records back
  const int n = s_len[cur][0];
  if (tid == 0) {
    a.out_len[b] = n;
    a.score[b] = s_score[cur][0];
  }
  int pos = 0, left = n;                                   // tokens still to be found
  for (int tend = (int)Tb; tend > 0 && left > 0; tend -= kTraceFrames) {
    const int t0 = max(0, tend - kTraceFrames);
    for (int x = tid; x < (tend - t0) * BS; x += kThreads) s_trace[x] = rec[(long)t0 * BS + x];
    __syncthreads();
    if (tid == 0) {
      for (int t = tend - 1; t >= t0; --t) {
        const int r = s_trace[(t - t0) * BS + pos];
        const int cls = r >> 4;
        pos = r & 15;
        if (cls != a.blank) {
          --left;
          a.tokens[(long)b * a.T + left] = cls;
          a.frames[(long)b * a.T + left] = t;
        }
      }
      s_nemit = left;
    }
    __syncthreads();
    left = s_nemit;                                        // every thread leaves with thread 0
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t records_bytes(int B, int T, int beam) { return align256(sizeof(int) * (size_t)B * T * beam); }

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
  if (T <= 0 || V <= 0 || V > 8192 || E <= 0 || D <= 0 || ctx < 1 || ctx > 64 || act < 0 ||
      act > 1 || blank < 0 || blank >= V || beam_size < 1 || beam_size > kMaxBeam ||
      cutoff_top_k < 1 || (cutoff_top_k < V ? cutoff_top_k : V) > kMaxBeam || !workspace)
    return -1;
  const size_t fixed = sizeof(float) * kGroup * ((size_t)E + D) + sizeof(int) * 2 * kMaxBeam * ctx;
  if (fixed > kLdsBudget) return -1;
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
