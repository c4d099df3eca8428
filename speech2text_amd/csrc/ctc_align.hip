// CTC forced alignment for gfx950: the max-product (Viterbi) twin of csrc/ctc.hip's alpha recursion over
// the same 2U+1 lattice, with backpointers, a backtrace and per-token times (the statement is in
// include/s2t_mi355.h above s2t_ctc_align).  Three launches, no atomics, no memset, no host
// synchronisation:
//   1. per (t,b) row with t < Tb: log-sum-exp of the V logits + the lattice's 2U+1 RAW emissions
//      x[label(s)] gathered into a dense row (ctc_lse_gather_kernel's shape; raw, not x - lse: the best
//      path does not move under a per-frame constant, and max + one fp32 add is exact arithmetic to
//      restate, ties included)
//   2. one workgroup (2 waves) per utterance: the recursion with states in LDS ping-pong rows, one barrier
//      per frame, the emission rows prefetched several frames ahead; each wave's 64 two-bit backpointers of a frame are
//      two __ballot masks (16 bytes per 64 states per frame) held in LDS.  Where a whole utterance's
//      masks do not fit next to the rows (S2T_CTC_ALIGN_LDS_BYTES) they are kept a BLOCK of frames at a
//      time: a full block is flushed coalesced to the workspace and the backtrace stages the blocks back
//      in reverse; the last block never leaves LDS.  With T frames in one block nothing is flushed: the
//      two forms are one body.  One lane walks a block in LDS (the masks of the next 4 frames are
//      fetched for the chunk of states it stands in before the dependent steps), the path of the block
//      goes to LDS and then coalesced to `path`.
//   3. one workgroup per utterance: frame-parallel token boundaries (a frame whose state differs from
//      its neighbour's writes that token's begin / end: one writer each), then one thread per token sums
//      its own span's log-probabilities in frame order; score = raw_score - sum of lse.
#include "common.h"
#include "../../include/s2t_mi355.h"

namespace {

constexpr int kThreads = 128;            // recursion workgroup: states s = tid + 128 r, r < MAXR
constexpr int kMaskBytes = 16;           // per frame and chunk of 64 states: low-bit mask, high-bit mask

struct AlignPlan {
  int maxr;      // lattice states per thread
  int chunks;    // 64-state chunks of a frame's backpointers
  int fb;        // frames per LDS block
  int ws;        // 1: the blocks of an utterance do not all fit, the workspace form
};

// Pure host arithmetic: what serves (T, Umax).  A frame costs 16 bytes per chunk of backpointers and 2
// bytes of path in LDS; T frames in one block is the LDS form.
inline AlignPlan align_plan(int T, int Umax) {
  AlignPlan p;
  const int Smax = 2 * Umax + 1;
  p.maxr = Smax <= 128 ? 1 : Smax <= 256 ? 2 : Smax <= 512 ? 4 : Smax <= 1024 ? 8 : 16;
  p.chunks = (Smax + 63) / 64;
  const int per_frame = kMaskBytes * p.chunks + 2;
  const int fit = S2T_CTC_ALIGN_LDS_BYTES / per_frame;
  p.ws = T > fit;
  p.fb = p.ws ? fit : T;
  return p;
}

inline long align_up16(long n) { return (n + 15) & ~15L; }

__device__ __forceinline__ int clamp_labels(long u, int Umax) {
  return u < 0 ? 0 : (u > Umax ? Umax : (int)u);
}

// One wave per (t, b) row with t < Tb; rows at and beyond Tb are not read and nothing is written for them.
__global__ __launch_bounds__(64) void align_rows_kernel(
    const float* __restrict__ x, const long* __restrict__ lengths, const long* __restrict__ targets,
    long tgt_stride, const long* __restrict__ tgt_len, int T, int V, int Umax, int blank,
    float* __restrict__ lse, float* __restrict__ em) {
  const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (t >= lengths[b]) return;
  const long row = (long)b * T + t;
  const float* p = x + row * V;
  float m = S2T_NEG_INF;
  for (int c = lane; c < V; c += 64) m = fmaxf(m, p[c]);
  m = wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < V; c += 64) sum += expf(p[c] - m);
  sum = wave_sum(sum);
  if (lane == 0) lse[row] = m + logf(sum);
  const int Smax = 2 * Umax + 1;
  const int S = 2 * clamp_labels(tgt_len[b], Umax) + 1;
  float* o = em + row * Smax;
  const long* tg = targets + (long)b * tgt_stride;
  for (int s = lane; s < S; s += 64) {
    const long c = (s & 1) ? tg[s >> 1] : (long)blank;
    o[s] = (c >= 0 && c < V) ? p[c] : S2T_NEG_INF;       // a label outside the classes has no path
  }
}

__device__ __forceinline__ int mask_step(ulonglong2 m, int s) {
  const int l = s & 63;
  return (int)((m.x >> l) & 1ull) | ((int)((m.y >> l) & 1ull) << 1);
}

template <int MAXR>
__global__ __launch_bounds__(kThreads) void align_viterbi_kernel(
    const float* __restrict__ em, const long* __restrict__ lengths, const long* __restrict__ targets,
    long tgt_stride, const long* __restrict__ tgt_len, int T, int Umax, int FB,
    ulonglong2* __restrict__ bp_ws, int* __restrict__ path, float* __restrict__ raw_score,
    int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int Smax = 2 * Umax + 1;
  const int C = (Smax + 63) >> 6;
  const int LD = (Smax + 2 + 3) & ~3;                    // 2 leading pads of -inf: s-1, s-2 always exist
  float* v0 = reinterpret_cast<float*>(smem_raw);
  float* v1 = v0 + LD;
  ulonglong2* bp = reinterpret_cast<ulonglong2*>(v1 + LD);           // [FB][C]
  unsigned short* pth = reinterpret_cast<unsigned short*>(bp + (long)FB * C);   // [FB]
  __shared__ int sh_state;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long Tl = lengths[b];
  const int Tb = Tl < 0 ? 0 : (Tl > T ? T : (int)Tl);
  const int U = clamp_labels(tgt_len[b], Umax);
  const int S = 2 * U + 1;
  int* prow = path + (long)b * T;
  if (Tb == 0) {
    for (int t = tid; t < T; t += kThreads) prow[t] = -1;
    if (tid == 0) {
      raw_score[b] = U == 0 ? 0.f : S2T_NEG_INF;
      ok[b] = U == 0;
    }
    return;
  }
  const long* tg = targets + (long)b * tgt_stride;
  const float* eb = em + (long)b * T * Smax;
  ulonglong2* bw = bp_ws + (long)b * T * C;
  for (int s = tid; s < 2 * LD; s += kThreads) v0[s] = S2T_NEG_INF;
  unsigned skip = 0;                                     // bit r: state tid + 128 r may come from s - 2
  // The emission rows are read D frames ahead of their use: a frame of the recursion is far shorter
  // than a trip to L2, one frame of prefetch would make every frame wait for its row.
  constexpr int D = MAXR <= 2 ? 8 : (MAXR == 4 ? 4 : 2);
  float pre[D][MAXR];
#pragma unroll
  for (int r = 0; r < MAXR; ++r) {
    const int s = tid + kThreads * r;
    if ((s & 1) && s >= 3 && s < S && tg[s >> 1] != tg[(s >> 1) - 1]) skip |= 1u << r;
#pragma unroll
    for (int d = 0; d < D; ++d) pre[d][r] = (s < S && 1 + d < Tb) ? eb[(long)(1 + d) * Smax + s] : 0.f;
  }
  __syncthreads();
  if (tid < 2 && tid < S) v0[2 + tid] = eb[tid];
  __syncthreads();
  float* vp = v0 + 2;
  float* vc = v1 + 2;
  int slot = 1;                                          // frame t of block t / FB sits in slot t % FB
  for (int t0 = 1; t0 < Tb; t0 += D) {
    float cur[D][MAXR];
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
      for (int r = 0; r < MAXR; ++r) {
        const int s = tid + kThreads * r;
        cur[d][r] = pre[d][r];
        pre[d][r] = (s < S && t0 + D + d < Tb) ? eb[(long)(t0 + D + d) * Smax + s] : 0.f;
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = t0 + d;
      if (t < Tb) {
        if (slot == FB) slot = 0;
#pragma unroll
        for (int r = 0; r < MAXR; ++r) {
          const int s = tid + kThreads * r;
          int k = 0;
          if (s < S) {
            float m = vp[s];
            const float c1 = vp[s - 1];
            const float c2 = ((skip >> r) & 1u) ? vp[s - 2] : S2T_NEG_INF;
            if (c1 > m) { m = c1; k = 1; }
            if (c2 > m) { m = c2; k = 2; }
            vc[s] = m + cur[d][r];
          }
          const unsigned long long m0 = __ballot(k & 1);
          const unsigned long long m1 = __ballot(k >> 1);
          const int chunk = 2 * r + wave;
          if (lane == 0 && chunk < C) bp[(long)slot * C + chunk] = make_ulonglong2(m0, m1);
        }
        ++slot;
        __syncthreads();
        float* tmp = vp; vp = vc; vc = tmp;
        if (slot == FB && t + 1 < Tb) {                  // a full block that is not the last: to the workspace
          const long n = (long)FB * C;
          ulonglong2* dst = bw + (long)(t + 1 - FB) * C;
          for (long i = tid; i < n; i += kThreads) dst[i] = bp[i];
          __syncthreads();
        }
      }
    }
  }
  if (tid == 0) {
    float e = vp[S - 1];
    int s = S - 1;
    if (U > 0 && !(e > vp[S - 2])) { s = S - 2; e = vp[S - 2]; }
    const bool good = e > S2T_NEG_INF;
    raw_score[b] = e;
    ok[b] = good;
    sh_state = good ? s : -1;
  }
  __syncthreads();
  int s_cur = sh_state;
  __syncthreads();                                       // (lane 0 writes sh_state again below)
  if (s_cur < 0) {
    for (int t = tid; t < T; t += kThreads) prow[t] = -1;
    return;
  }
  for (int t = Tb + tid; t < T; t += kThreads) prow[t] = -1;
  for (int lo = ((Tb - 1) / FB) * FB; lo >= 0; lo -= FB) {
    const int hi = lo + FB < Tb ? lo + FB : Tb;          // the block's frames [lo, hi); state at hi - 1 known
    if (hi < Tb) {                                       // (the last block is still in LDS)
      const long n = (long)FB * C;
      const ulonglong2* src = bw + (long)lo * C;
      for (long i = tid; i < n; i += kThreads) bp[i] = src[i];
      __syncthreads();
    }
    if (tid == 0) {
      int s = s_cur;
      pth[hi - 1 - lo] = (unsigned short)s;
      const int stop = lo > 0 ? lo : 1;                  // frame t's mask leads to frame t - 1; frame 0 has none
      for (int t = hi - 1; t >= stop; t -= 4) {
        const int c0 = s >> 6;
        unsigned long long wx[4], wy[4];                 // four independent loads, then the dependent steps
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = t - j >= stop ? t - j : stop;
          const ulonglong2 m = bp[(long)(f - lo) * C + c0];
          wx[j] = m.x;
          wy[j] = m.y;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (t - j >= stop) {
            const int c = s >> 6;
            ulonglong2 m = make_ulonglong2(wx[j], wy[j]);
            if (c != c0) m = bp[(long)(t - j - lo) * C + c];
            s -= mask_step(m, s);
            s = s < 0 ? 0 : s;
            if (t - j - 1 >= lo) pth[t - j - 1 - lo] = (unsigned short)s;
          }
        }
      }
      sh_state = s;                                      // the state at frame lo - 1 (unused when lo == 0)
    }
    __syncthreads();
    for (int i = tid; i < hi - lo; i += kThreads) prow[lo + i] = pth[i];
    s_cur = sh_state;
    __syncthreads();
  }
}

// One workgroup per utterance, after `path` is complete.
__global__ __launch_bounds__(256) void align_tokens_kernel(
    const float* __restrict__ em, const float* __restrict__ lse, const long* __restrict__ lengths,
    const long* __restrict__ tgt_len, const int* __restrict__ path, const int* __restrict__ ok,
    const float* __restrict__ raw_score, int T, int Umax, int* __restrict__ tok_begin,
    int* __restrict__ tok_end, float* __restrict__ tok_logp, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  int* tb = reinterpret_cast<int*>(smem_raw);            // [Umax] begin, [Umax] end
  int* te = tb + Umax;
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Smax = 2 * Umax + 1;
  long Tl = lengths[b];
  const int Tb = Tl < 0 ? 0 : (Tl > T ? T : (int)Tl);
  const int U = clamp_labels(tgt_len[b], Umax);
  const bool good = ok[b] != 0;
  const int* prow = path + (long)b * T;
  const float* lb = lse + (long)b * T;
  for (int u = tid; u < Umax; u += 256) tb[u] = te[u] = -1;
  __syncthreads();
  float part = 0.f;
  if (good) {
    for (int t = tid; t < Tb; t += 256) {
      part += lb[t];
      const int s = prow[t];
      if ((s & 1) && (s >> 1) < U) {                     // a feasible path visits every token
        if (t == 0 || prow[t - 1] != s) tb[s >> 1] = t;
        if (t + 1 == Tb || prow[t + 1] != s) te[s >> 1] = t + 1;
      }
    }
  }
  const float total = block_sum(part, red);              // (its barriers also publish tb / te)
  if (tid == 0) score[b] = good ? raw_score[b] - total : S2T_NEG_INF;
  const float* eb = em + (long)b * T * Smax;
  for (int u = tid; u < Umax; u += 256) {
    const int t0 = u < U ? tb[u] : -1, t1 = (u < U && t0 >= 0) ? te[u] : -1;
    float acc = 0.f;
    for (int t = t0; t < t1; ++t) acc += eb[(long)t * Smax + 2 * u + 1] - lb[t];
    const long o = (long)b * Umax + u;
    tok_begin[o] = t0;
    tok_end[o] = t1;
    tok_logp[o] = acc;
  }
}

}  // namespace

extern "C" int s2t_ctc_align_form(int T, int Umax) {
  if (T <= 0 || Umax < 0 || Umax > S2T_CTC_MAX_LABELS) return -1;
  const AlignPlan p = align_plan(T, Umax);
  return p.maxr | (p.ws ? S2T_CTC_ALIGN_FORM_WORKSPACE : 0);
}

// bytes: lse B*T floats, emissions B*T*(2Umax+1) floats, and in the workspace form B*T*chunks masks
extern "C" long s2t_ctc_align_workspace_bytes(int B, int T, int Umax) {
  if (B <= 0 || T <= 0 || Umax < 0 || Umax > S2T_CTC_MAX_LABELS) return 0;
  const AlignPlan p = align_plan(T, Umax);
  long n = align_up16(4L * B * T) + align_up16(4L * B * T * (2L * Umax + 1));
  if (p.ws) n += (long)kMaskBytes * B * T * p.chunks;
  return n;
}

extern "C" int s2t_ctc_align(const float* logits, const long* lengths, const long* targets,
                             long tgt_stride, const long* tgt_len, int B, int T, int V, int Umax,
                             int blank, void* workspace, int* path, int* tok_begin, int* tok_end,
                             float* tok_logp, float* raw_score, float* score, int* ok, void* stream) {
  if (B <= 0) return 0;
  if (T <= 0 || V <= 0 || Umax < 0 || blank < 0 || blank >= V || tgt_stride < Umax) return -1;
  if (!workspace || !path || !tok_begin || !tok_end || !tok_logp || !raw_score || !score || !ok)
    return -1;
  if (Umax > S2T_CTC_MAX_LABELS) return -4;
  hipStream_t st = (hipStream_t)stream;
  const AlignPlan p = align_plan(T, Umax);
  const int Smax = 2 * Umax + 1;
  unsigned char* w = static_cast<unsigned char*>(workspace);
  float* lse = reinterpret_cast<float*>(w);
  float* em = reinterpret_cast<float*>(w + align_up16(4L * B * T));
  ulonglong2* bp_ws = reinterpret_cast<ulonglong2*>(w + align_up16(4L * B * T) +
                                                    align_up16(4L * B * T * (long)Smax));
  hipLaunchKernelGGL(align_rows_kernel, dim3(T, B), dim3(64), 0, st, logits, lengths, targets,
                     tgt_stride, tgt_len, T, V, Umax, blank, lse, em);
  S2T_CHECK_LAUNCH();
  const int LD = (Smax + 2 + 3) & ~3;
  const size_t smem = sizeof(float) * 2 * LD + (size_t)p.fb * (kMaskBytes * p.chunks + 2) + 16;
#define S2T_CTC_ALIGN(R)                                                                            \
  hipLaunchKernelGGL(align_viterbi_kernel<R>, dim3(B), dim3(kThreads), smem, st, em, lengths, targets, \
                     tgt_stride, tgt_len, T, Umax, p.fb, bp_ws, path, raw_score, ok)
  switch (p.maxr) {
    case 1: S2T_CTC_ALIGN(1); break;
    case 2: S2T_CTC_ALIGN(2); break;
    case 4: S2T_CTC_ALIGN(4); break;
    case 8: S2T_CTC_ALIGN(8); break;
    default: S2T_CTC_ALIGN(16); break;
  }
#undef S2T_CTC_ALIGN
  S2T_CHECK_LAUNCH();
  hipLaunchKernelGGL(align_tokens_kernel, dim3(B), dim3(256), sizeof(int) * 2 * (Umax + 1), st, em, lse,
                     lengths, tgt_len, path, ok, raw_score, T, Umax, tok_begin, tok_end, tok_logp, score);
  S2T_CHECK_LAUNCH();
  return 0;
}
