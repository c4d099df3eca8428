// RNN-T forced alignment for gfx950: the max-product (Viterbi) twin of csrc/rnnt.hip's mutual-information
// recursion over the same (S+1) x (T+1) lattice, with backpointers, a backtrace and per-token frames (the
// statement is in include/s2t_mi355.h above s2t_rnnt_align).  One launch, no atomics, no memset, no host
// synchronisation.
//   One workgroup per utterance, one thread per lattice row s (S + 1 rounded up to whole waves).  REGULAR
//   walks the Sb + Tb + 1 anti-diagonals, MODIFIED / CONSTRAINED the Tb frames: the thread's own previous
//   value stays in a register, the row below's comes through a double-buffered LDS row, one barrier per
//   step.  Operands are requested a group of RA_PD steps ahead through raw buffer loads on straight-line
//   code (a lane outside the lattice passes an out-of-range offset and gets 0), as mi_fwd_kernel does and
//   for its reason.  A step's backpointers ("symbol" exactly when cu > cl) are one __ballot word per wave, 8 bytes
//   per 64 rows and step, which lane 0 writes to an LDS block of FB steps.  Where all the steps fit in one
//   block nothing leaves LDS; otherwise a full block that is not the last is flushed coalesced to the
//   workspace and the backtrace stages the blocks back in reverse: the two forms are one body, as in
//   csrc/ctc_align.hip.  One lane walks a block's masks in LDS (the words of the next 4 steps are fetched
//   for the chunk of rows it stands in before the dependent steps) and writes the frames to LDS; the
//   workgroup then stores tok_frame and gathers tok_logp, one row per thread.
#include "common.h"
#include "../../include/s2t_mi355.h"

namespace {

constexpr int RA_PD = 8;                  // steps in a group: the operand look-ahead
constexpr unsigned RA_OOB = 0xFFFFFFF0u;  // beyond every descriptor: the load returns 0

__device__ __forceinline__ __amdgpu_buffer_rsrc_t ra_rsrc(const float* p, long floats) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)(floats * 4), 0x00020000);
}
__device__ __forceinline__ float ra_load(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
}

struct RnntAlignPlan {
  int waves;     // per workgroup: 64-row chunks of a step's backpointers
  long steps;    // of the widest utterance: S + T + 1 anti-diagonals, or T frames
  int fb;        // steps per LDS block, a multiple of 8
  int ws;        // 1: the steps do not fit in one block, the workspace form
};

// Pure host arithmetic: what serves (S, T, rnnt_type).
inline RnntAlignPlan rnnt_align_plan(int S, int T, int rnnt_type) {
  RnntAlignPlan p;
  p.waves = (S + 1 + 63) / 64;
  p.steps = rnnt_type == S2T_RNNT_REGULAR ? (long)S + T + 1 : (long)T;
  const int fit = S2T_RNNT_ALIGN_LDS_BYTES / (8 * p.waves);
  p.ws = p.steps > fit;
  // the recursion closes a block only between its groups of 8 steps
  p.fb = p.ws ? (fit & ~7) : (int)((p.steps + 7) & ~7L);
  return p;
}

inline bool ra_known_type(int rnnt_type) {
  return rnnt_type == S2T_RNNT_REGULAR || rnnt_type == S2T_RNNT_MODIFIED ||
         rnnt_type == S2T_RNNT_CONSTRAINED;
}

// 0: a shape the entry serves; else its return value.  The raw buffer accesses address an utterance's px
// and py through 32-bit byte offsets.
inline int rnnt_align_refuse(int S, int T, int rnnt_type) {
  if (T <= 0 || S < 0 || !ra_known_type(rnnt_type)) return -1;
  if (S + 1 > 1024) return -4;
  if (((long)S + 1) * ((long)T + 1) * 4 > 0x7fffffffL) return -1;
  return 0;
}

inline size_t align_up16(size_t n) { return (n + 15) & ~(size_t)15; }

__device__ __forceinline__ int clamp_len(long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

template <bool REG>
__global__ __launch_bounds__(1024) void rnnt_align_kernel(
    const float* __restrict__ px, const float* __restrict__ py, const long* __restrict__ boundary, int S,
    int T, int FB, unsigned long long* __restrict__ bp_ws, long ws_stride,
    int* __restrict__ tok_frame, float* __restrict__ tok_logp, float* __restrict__ score,
    int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int b = blockIdx.x, s = threadIdx.x, nt = blockDim.x, W = nt >> 6;
  const int lane = s & 63, wave = s >> 6;
  unsigned long long* bp = reinterpret_cast<unsigned long long*>(smem_raw);          // [FB][W]
  float* ex = reinterpret_cast<float*>(smem_raw + (((size_t)FB * W * 8 + 15) & ~(size_t)15));  // [2][nt + 1]
  int* tokf = reinterpret_cast<int*>(ex + ((2 * (nt + 1) + 3) & ~3));                 // [S]
  float* shf = reinterpret_cast<float*>(tokf + ((S + 1 + 3) & ~3));                   // the end value
  const int TX = REG ? T + 1 : T;
  const int Sb = clamp_len(boundary[b * 4 + 2], S), Tb = clamp_len(boundary[b * 4 + 3], T);
  const float* pxb = px + (long)b * S * TX;
  const __amdgpu_buffer_rsrc_t rpx = ra_rsrc(pxb, (long)S * TX);
  const __amdgpu_buffer_rsrc_t rpy = ra_rsrc(py + (long)b * (S + 1) * T, (long)(S + 1) * T);
  unsigned long long* bw = bp_ws + (long)b * ws_stride;
  const bool act = s <= Sb;
  // REGULAR starts before diagonal 0, the others after column 0, which holds the start state only
  float own = (!REG && s == 0) ? 0.f : S2T_NEG_INF;      // v[s][t-1]
  ex[s] = (!REG && act) ? own : S2T_NEG_INF;
  ex[nt + 1 + s] = S2T_NEG_INF;
  if (s == 0) {
    ex[nt] = S2T_NEG_INF;
    ex[2 * nt + 1] = S2T_NEG_INF;
  }
  if (s < S) tokf[s] = -1;
  __syncthreads();
  // step i is diagonal d = i (cells (s, i - s); operands px[s-1][t], py[s][t-1]) or frame t = i + 1
  // (operands px[s-1][t-1], py[s][t-1])
  const int nsteps = REG ? Sb + Tb + 1 : Tb;
  float rx[RA_PD], ry[RA_PD];
#define RA_FETCH(II, X, Y)                                                                   \
  {                                                                                          \
    const int t1_ = REG ? (II) - s : (II) + 1;                                               \
    const bool in_ = act && t1_ >= 0 && t1_ <= Tb;                                           \
    X = ra_load(rpx, (in_ && s > 0) ? (unsigned)((s - 1) * TX + (REG ? t1_ : t1_ - 1)) * 4u : RA_OOB); \
    Y = ra_load(rpy, (in_ && t1_ > 0) ? (unsigned)(s * T + t1_ - 1) * 4u : RA_OOB);          \
  }
  int cur = REG ? 0 : 1;
  // Block by block (FB is a whole number of groups; step i sits in slot i % FB).  Inside a block: whole
  // groups of RA_PD steps on straight-line code; the ones past the last step have no cell in the lattice
  // and fall through as no-ops whose (empty) masks land in the block's unused tail -- no exit test and
  // no flush inside the loop that carries the look-ahead, which starts again with every block.
  for (int lo = 0; lo < nsteps; lo += FB) {
    const int hi = lo + FB < nsteps ? lo + FB : nsteps;
#pragma unroll
    for (int u = 0; u < RA_PD; ++u) RA_FETCH(lo + u, rx[u], ry[u])
    for (int i0 = lo; i0 < hi; i0 += RA_PD) {
      // the next group's operands, all requested before this group's first step: the compiler closes the
      // loop with a full wait for whatever the body requested, and by then these have had a group's time
      float nx[RA_PD], ny[RA_PD];
#pragma unroll
      for (int u = 0; u < RA_PD; ++u) RA_FETCH(i0 + RA_PD + u, nx[u], ny[u])
#pragma unroll
      for (int u = 0; u < RA_PD; ++u) {
        const int i = i0 + u;
        const int t = REG ? i - s : i + 1;
        const float vx = rx[u], vy = ry[u];
        const bool in = act && t >= 0 && t <= Tb;
        const float cu = (s > 0) ? ex[(cur ^ 1) * (nt + 1) + (s > 0 ? s - 1 : 0)] + vx : S2T_NEG_INF;
        const float cl = (t > 0) ? own + vy : S2T_NEG_INF;
        const bool sym = cu > cl;                        // the first maximum in the order blank, symbol
        const float step = (REG && i == 0) ? 0.f : (sym ? cu : cl);
        const float val = in ? step : S2T_NEG_INF;
        const unsigned long long mask = __ballot(in && sym);
        own = in ? val : own;
        ex[cur * (nt + 1) + s] = val;
        if (lane == 0) bp[(i - lo) * W + wave] = mask;
        __syncthreads();
        cur ^= 1;
      }
#pragma unroll
      for (int u = 0; u < RA_PD; ++u) {
        rx[u] = nx[u];
        ry[u] = ny[u];
      }
    }
    if (hi < nsteps) {                                  // a full block that is not the last: to the workspace
      const int n = FB * W;
      unsigned long long* dst = bw + (long)lo * W;
      for (int k = s; k < n; k += nt) dst[k] = bp[k];
      __syncthreads();
    }
  }
#undef RA_FETCH
  if (s == Sb) shf[0] = own;
  __syncthreads();
  const float end = shf[0];
  const bool good = end > S2T_NEG_INF;
  if (s == 0) {
    score[b] = good ? end : S2T_NEG_INF;
    ok[b] = good;
  }
  if (good) {
    const int first = REG ? 1 : 0;                       // diagonal 0 is the start cell: no backpointer
    int s_cur = Sb;                                      // (lane 0's: the row it stands in)
    for (int lo = ((nsteps - 1) / FB) * FB; lo >= 0; lo -= FB) {
      const int hi = lo + FB < nsteps ? lo + FB : nsteps;  // the block's steps [lo, hi)
      if (hi < nsteps) {                                 // (the last block is still in LDS)
        const int n = FB * W;
        const unsigned long long* src = bw + (long)lo * W;
        for (int k = s; k < n; k += nt) bp[k] = src[k];
        __syncthreads();
      }
      if (s == 0) {
        int r = s_cur;
        const int stop = lo > first ? lo : first;
        for (int i = hi - 1; i >= stop; i -= 4) {
          const int c0 = r >> 6;
          unsigned long long w[4];                       // four independent loads, then the dependent steps
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = i - j >= stop ? i - j : stop;
            w[j] = bp[(long)(f - lo) * W + c0];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (i - j >= stop) {
              const int c = r >> 6;
              unsigned long long m = w[j];
              if (c != c0) m = bp[(long)(i - j - lo) * W + c];
              if (((m >> (r & 63)) & 1ull) && r > 0) {   // the symbol arc into row r leaves row r - 1
                tokf[r - 1] = REG ? i - j - r : i - j;
                --r;
              }
            }
          }
        }
        s_cur = r;
      }
      __syncthreads();
    }
  }
  if (s < S) {
    const int f = (good && s < Sb) ? tokf[s] : -1;
    tok_frame[(long)b * S + s] = f;
    tok_logp[(long)b * S + s] = (f >= 0 && f < TX) ? pxb[(long)s * TX + f] : 0.f;
  }
}

}  // namespace

extern "C" int s2t_rnnt_align_form(int S, int T, int rnnt_type) {
  if (rnnt_align_refuse(S, T, rnnt_type)) return -1;
  const RnntAlignPlan p = rnnt_align_plan(S, T, rnnt_type);
  return p.waves | (p.ws ? S2T_RNNT_ALIGN_FORM_WORKSPACE : 0);
}

// bytes: in the workspace form one 8-byte word per utterance, step and wave; 0 otherwise
extern "C" long s2t_rnnt_align_workspace_bytes(int B, int S, int T, int rnnt_type) {
  if (B <= 0 || rnnt_align_refuse(S, T, rnnt_type)) return 0;
  const RnntAlignPlan p = rnnt_align_plan(S, T, rnnt_type);
  return p.ws ? 8L * B * p.steps * p.waves : 0;
}

extern "C" int s2t_rnnt_align(const float* px, const float* py, const long* boundary, int B, int S,
                              int T, int rnnt_type, void* workspace, int* tok_frame, float* tok_logp,
                              float* score, int* ok, void* stream) {
  if (B <= 0) return 0;
  const int rc = rnnt_align_refuse(S, T, rnnt_type);
  if (rc) return rc;
  if (!tok_frame || !tok_logp || !score || !ok) return -1;
  const RnntAlignPlan p = rnnt_align_plan(S, T, rnnt_type);
  if (p.ws && !workspace) return -1;
  const int nt = 64 * p.waves;
  const size_t smem = align_up16((size_t)p.fb * p.waves * 8) + sizeof(float) * ((2 * (nt + 1) + 3) & ~3) +
                      sizeof(int) * ((S + 1 + 3) & ~3) + 16;
  unsigned long long* ws = static_cast<unsigned long long*>(workspace);
  const long ws_stride = p.ws ? p.steps * p.waves : 0;
  hipLaunchKernelGGL(rnnt_type == S2T_RNNT_REGULAR ? rnnt_align_kernel<true> : rnnt_align_kernel<false>,
                     dim3(B), dim3(nt), smem, (hipStream_t)stream, px, py, boundary, S, T, p.fb, ws,
                     ws_stride, tok_frame, tok_logp, score, ok);
  S2T_CHECK_LAUNCH();
  return 0;
}
