// The lm-only / am-only smoothing of k2.rnnt_loss_smoothed (reference model/joiner/joiner.py:24-25,
// 100-106: the YAML keys `joiner: lm_scale` = lam and `joiner: am_scale` = mu) for gfx950.  With both
// scales 0 nothing here is launched: csrc/rnnt.hip's simple_pxpy / simple_w / simple_bwd are the path.
//
// alpha = 1 - lam - mu, Z the joint normaliser of csrc/rnnt.hip, y the arc's symbol or the blank:
//   q[b,s,:] = softmax(lm[b,s,:]),  Ll[b,s] = logsumexp_c lm[b,s,:]
//   u[c]     = mean over ALL B (S+1) rows of q[b,s,c] (rows past S_b included, as k2's torch.mean
//              of the padded tensor) + the smallest normal float
//   La[b,t]  = log sum_c exp(am[b,t,c]) u[c]
//   px/py    = alpha (am_y + lm_y - Z) + lam (lm_y - Ll) + mu (am_y + log u_y - La)
// A scale that is exactly 0 drops its term (k2 keeps it times 1e-20, below fp32 resolution).
//
// Backward, with d = gscale (gy + gx), P the joint posterior (the two GEMMs on W of csrc/rnnt.hip):
//   d_am = -alpha sum_s d P + (alpha+mu) hot_am - mu colsum r,       r = softmax_c(am + log u)
//   d_lm = -alpha sum_t d P + (alpha+lam) hot_lm - lam rowsum q + q (v - sum_c q v)
//   dlogu[c] = sum_{b,t} (the mu part of d_am)[b,t,c],  v[c] = dlogu[c] / (u[c] B (S+1))
// The last term of d_lm couples every utterance's am-only term to every lm row of the batch.
//
// Nothing of size (B,S+1,T,C) or (B,S+1,T) is formed here; the C-vectors u and dlogu are reduced
// column-parallel over slabs of rows into partials, then summed by one final pass: no atomics on
// global memory, so both are deterministic.
#include "common.h"
#include "../../include/s2t_mi355.h"

namespace {

constexpr int LM_SLAB = S2T_RNNT_SMOOTH_LM_SLAB;
constexpr int AM_SLAB = S2T_RNNT_SMOOTH_AM_SLAB;
constexpr int AM_RPW = AM_SLAB / 4;   // am rows per wave of a 4-wave workgroup
constexpr float TINY = 1.17549435e-38f;

// ---------------------------------------------------------------- row statistics
// out[r] = sum_c x[r][c] * (w ? w[c] : 1); one wave per row.
__global__ __launch_bounds__(256) void row_dot_kernel(const float* __restrict__ x, long rows, int C,
                                                      const float* __restrict__ w,
                                                      float* __restrict__ out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* p = x + row * C;
  float a = 0.f;
  if (w)
    for (int c = lane; c < C; c += 64) a += p[c] * w[c];
  else
    for (int c = lane; c < C; c += 64) a += p[c];
  a = wave_sum(a);
  if (lane == 0) out[row] = a;
}

// Column sums of a row-major [rows][C] matrix, column-parallel: a workgroup is COLS columns x
// 256 / COLS row groups, group g adds rows r0 + g, r0 + g + groups, ... of its slab (four loads in
// flight per thread), the groups meet in LDS.  MODE 0 (a slab of S2T_RNNT_SMOOTH_LM_SLAB lm rows per
// blockIdx.y): out[slab][c] = sum_r x[r][c] / row_div[r], the partial unigram.  MODE 1 (one slab =
// all partials): u[c] = sum / n + tiny -> out, log u -> out2.  MODE 2 (all partials of dlogu):
// v[c] = sum / (col_div[c] n) -> out.
template <int MODE, int COLS>
__global__ __launch_bounds__(256) void col_sum_kernel(const float* __restrict__ x, long rows,
                                                      int slab, int C,
                                                      const float* __restrict__ row_div,
                                                      const float* __restrict__ col_div, float n,
                                                      float* __restrict__ out,
                                                      float* __restrict__ out2) {
  constexpr int GROUPS = 256 / COLS;
  __shared__ float sm[256];
  const int col = threadIdx.x % COLS, grp = threadIdx.x / COLS;
  const int c = blockIdx.x * COLS + col;
  const long r0 = (long)blockIdx.y * slab;
  const long r1 = r0 + slab < rows ? r0 + slab : rows;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < C) {
    long r = r0 + grp;
    for (; r + 3 * GROUPS < r1; r += 4 * GROUPS) {
      float x0 = x[r * C + c], x1 = x[(r + GROUPS) * C + c];
      float x2 = x[(r + 2 * GROUPS) * C + c], x3 = x[(r + 3 * GROUPS) * C + c];
      if (MODE == 0) {
        x0 /= row_div[r];
        x1 /= row_div[r + GROUPS];
        x2 /= row_div[r + 2 * GROUPS];
        x3 /= row_div[r + 3 * GROUPS];
      }
      a0 += x0;
      a1 += x1;
      a2 += x2;
      a3 += x3;
    }
    for (; r < r1; r += GROUPS) a0 += MODE == 0 ? x[r * C + c] / row_div[r] : x[r * C + c];
  }
  sm[threadIdx.x] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (grp != 0 || c >= C) return;
  float a = 0.f;
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) a += sm[g * COLS + col];
  if (MODE == 0) {
    out[(long)blockIdx.y * C + c] = a;
  } else if (MODE == 1) {
    a = a / n + TINY;
    out[c] = a;
    out2[c] = logf(a);
  } else {
    out[c] = a / (col_div[c] * n);
  }
}

// ------------------------------------------------------- smoothed px / py, one pass
__global__ __launch_bounds__(256) void smooth_pxpy_kernel(
    const float* __restrict__ am, const float* __restrict__ lm, const float* __restrict__ am_max,
    const float* __restrict__ lm_max, const float* __restrict__ nrm,
    const float* __restrict__ lm_sum, const float* __restrict__ am_dot,
    const float* __restrict__ log_u, const long* __restrict__ symbols,
    const long* __restrict__ boundary, int S, int T, int C, int blank, float alpha, float lam,
    float mu, float* __restrict__ px, float* __restrict__ py) {
  const int b = blockIdx.z, s = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int S1 = S + 1;
  if (t > T) return;
  const long Tb = boundary[b * 4 + 3];
  if (t == T) {
    if (s < S) px[((long)b * S + s) * (T + 1) + T] = S2T_NEG_INF;
    return;
  }
  const float n = nrm[((long)b * S1 + s) * T + t];
  const float lmx = lm_max[b * S1 + s], amx = am_max[b * T + t];
  const float z = logf(n + TINY) + lmx + amx;
  const float ll = lam != 0.f ? logf(lm_sum[b * S1 + s]) + lmx : 0.f;
  const float la = mu != 0.f ? logf(am_dot[b * T + t]) + amx : 0.f;
  const float* amr = am + ((long)b * T + t) * C;
  const float* lmr = lm + ((long)b * S1 + s) * C;
  {
    const float a = amr[blank], l = lmr[blank];
    float v = alpha * (a + l - z);
    if (lam != 0.f) v += lam * (l - ll);
    if (mu != 0.f) v += mu * (a + log_u[blank] - la);
    py[((long)b * S1 + s) * T + t] = v;
  }
  if (s < S) {
    const long y = symbols[(long)b * S + s];
    const float a = amr[y], l = lmr[y];
    float v = alpha * (a + l - z);
    if (lam != 0.f) v += lam * (l - ll);
    if (mu != 0.f) v += mu * (a + log_u[y] - la);
    if (t == Tb) v = S2T_NEG_INF;  // fix_for_boundary
    px[((long)b * S + s) * (T + 1) + t] = v;
  }
}

// ---------------------------------------------------------------- backward rows
// d_am: simple_dam_kernel's form (one wave per (b,t) row, the row assembled in LDS so that the
// gather terms can be added there), each of the four waves walking RPW rows.  MU (RPW = AM_RPW, a
// workgroup per slab of AM_SLAB rows): the row's am-only part -mu colsum r + mu hot_am is also summed
// per wave over its rows (acc, LDS) and the four waves' sums leave as dlogu_part[workgroup][:].
// Without MU nothing is carried from row to row: RPW = 1, simple_dam_kernel's grid.
template <bool MU, int RPW>
__global__ __launch_bounds__(256) void smooth_dam_kernel(
    const float* __restrict__ am_probs, const float* __restrict__ G, const float* __restrict__ dpx,
    const float* __restrict__ dpy, const float* __restrict__ gscale,
    const long* __restrict__ symbols, const float* __restrict__ am_dot,
    const float* __restrict__ u, int B, int S, int T, int C, int blank, float alpha, float mu,
    float* __restrict__ d_am, float* __restrict__ dlogu_part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* rowbuf = reinterpret_cast<float*>(smem_raw) + wave * C;
  float* acc = reinterpret_cast<float*>(smem_raw) + (4 + wave) * C;   // MU only
  const int S1 = S + 1;
  const long rows = (long)B * T;
  if (MU)
    for (int c = lane; c < C; c += 64) acc[c] = 0.f;
  for (int i = 0; i < RPW; ++i) {
    const long row = (long)blockIdx.x * (4 * RPW) + i * 4 + wave;
    const bool ok = row < rows;
    const int b = ok ? (int)(row / T) : 0, t = ok ? (int)(row % T) : 0;
    const float g = gscale[b];
    float sy = 0.f, sx = 0.f;
    if (ok) {
      for (int s = lane; s < S1; s += 64) sy += dpy[((long)b * S1 + s) * T + t];
      if (MU)
        for (int s = lane; s < S; s += 64) sx += dpx[((long)b * S + s) * (T + 1) + t];
    }
    sy = wave_sum(sy) * g;
    if (MU) sx = wave_sum(sx) * g;
    if (ok) {
      float k = 0.f;
      if (MU) k = -mu * (sy + sx) / am_dot[row];
      for (int c = lane; c < C; c += 64) {
        const float p = am_probs[row * C + c];
        float v = alpha * p * G[row * C + c];
        if (MU) {
          const float m = k * p * u[c];
          acc[c] += m;
          v += m;
        }
        rowbuf[c] = v;
      }
    }
    __syncthreads();
    if (ok) {
      if (lane == 0) {
        atomicAdd(&rowbuf[blank], (alpha + mu) * sy);
        if (MU) atomicAdd(&acc[blank], mu * sy);
      }
      for (int s = lane; s < S; s += 64) {
        const float v = dpx[((long)b * S + s) * (T + 1) + t] * g;
        if (v != 0.f) {
          const long y = symbols[(long)b * S + s];
          atomicAdd(&rowbuf[y], (alpha + mu) * v);
          if (MU) atomicAdd(&acc[y], mu * v);
        }
      }
    }
    __syncthreads();
    if (ok) {
      float* o = d_am + row * C;
      for (int c = lane; c < C; c += 64) o[c] = rowbuf[c];
    }
  }
  if (MU) {
    __syncthreads();
    const float* a0 = reinterpret_cast<float*>(smem_raw) + 4 * C;
    float* o = dlogu_part + (long)blockIdx.x * C;
    for (int c = threadIdx.x; c < C; c += 256)
      o[c] = (a0[c] + a0[C + c]) + (a0[2 * C + c] + a0[3 * C + c]);
  }
}

// d_lm: simple_dlm_kernel's form (one wave per (b,s) row) with the lm-only softmax term and, MU,
// the unigram's q (v - q.v), which reaches padded rows too.
template <bool MU>
__global__ __launch_bounds__(256) void smooth_dlm_kernel(
    const float* __restrict__ lm_probs, const float* __restrict__ G, const float* __restrict__ dpx,
    const float* __restrict__ dpy, const float* __restrict__ gscale,
    const long* __restrict__ symbols, const float* __restrict__ lm_sum,
    const float* __restrict__ v, int B, int S, int T, int C, int blank, float alpha, float lam,
    float* __restrict__ d_lm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* rowbuf = reinterpret_cast<float*>(smem_raw) + (threadIdx.x >> 6) * C;
  const int S1 = S + 1;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const bool ok = row < (long)B * S1;
  const int b = ok ? (int)(row / S1) : 0, s = ok ? (int)(row % S1) : 0;
  const float g = gscale[b];
  float sy = 0.f, sx = 0.f, qv = 0.f;
  if (ok) {
    for (int t = lane; t < T; t += 64) sy += dpy[((long)b * S1 + s) * T + t];
    if (s < S)
      for (int t = lane; t <= T; t += 64) sx += dpx[((long)b * S + s) * (T + 1) + t];
    if (MU)
      for (int c = lane; c < C; c += 64) qv += lm_probs[row * C + c] * v[c];
  }
  sy = wave_sum(sy) * g;
  sx = wave_sum(sx) * g;
  if (MU) qv = wave_sum(qv);
  if (ok) {
    const float inv = 1.f / lm_sum[row];
    const float k = -lam * (sx + sy);
    if (MU) qv *= inv;
    for (int c = lane; c < C; c += 64) {
      const float p = lm_probs[row * C + c];
      const float q = p * inv;
      float o = alpha * p * G[row * C + c] + k * q;
      if (MU) o += q * (v[c] - qv);
      rowbuf[c] = o;
    }
  }
  __syncthreads();
  if (ok && lane == 0) {
    rowbuf[blank] += (alpha + lam) * sy;
    if (s < S) rowbuf[symbols[(long)b * S + s]] += (alpha + lam) * sx;
  }
  __syncthreads();
  if (ok) {
    float* o = d_lm + row * C;
    for (int c = lane; c < C; c += 64) o[c] = rowbuf[c];
  }
}

bool scales_ok(float lam, float mu) {
  return lam >= 0.f && mu >= 0.f && lam + mu < 1.f && (lam != 0.f || mu != 0.f);
}

}  // namespace

extern "C" int s2t_rnnt_smooth_stats(const float* am_probs, const float* lm_probs, int B, int S,
                                     int T, int C, float mu, float* lm_sum, float* u_part,
                                     float* u, float* log_u, float* am_dot, void* stream) {
  if (B <= 0) return 0;
  if (S < 0 || T <= 0 || C <= 0 || mu < 0.f) return -1;
  hipStream_t st = (hipStream_t)stream;
  const long lm_rows = (long)B * (S + 1), am_rows = (long)B * T;
  hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)((lm_rows + 3) / 4)), dim3(256), 0, st,
                     lm_probs, lm_rows, C, (const float*)nullptr, lm_sum);
  S2T_CHECK_LAUNCH();
  if (mu == 0.f) return 0;
  const int parts = (int)((lm_rows + LM_SLAB - 1) / LM_SLAB);
  hipLaunchKernelGGL((col_sum_kernel<0, 64>), dim3((C + 63) / 64, parts), dim3(256), 0, st, lm_probs,
                     lm_rows, LM_SLAB, C, (const float*)lm_sum, (const float*)nullptr, 0.f, u_part,
                     (float*)nullptr);
  S2T_CHECK_LAUNCH();
  hipLaunchKernelGGL((col_sum_kernel<1, 16>), dim3((C + 15) / 16, 1), dim3(256), 0, st,
                     (const float*)u_part, (long)parts, parts, C, (const float*)nullptr,
                     (const float*)nullptr, (float)lm_rows, u, log_u);
  S2T_CHECK_LAUNCH();
  hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)((am_rows + 3) / 4)), dim3(256), 0, st,
                     am_probs, am_rows, C, (const float*)u, am_dot);
  S2T_CHECK_LAUNCH();
  return 0;
}

extern "C" int s2t_rnnt_smooth_pxpy(const float* am, const float* lm, const float* am_max,
                                    const float* lm_max, const float* nrm, const float* lm_sum,
                                    const float* am_dot, const float* log_u, const long* symbols,
                                    const long* boundary, int B, int S, int T, int C, int blank,
                                    float lam, float mu, float* px, float* py, void* stream) {
  if (B <= 0) return 0;
  if (S < 0 || T <= 0 || C <= 0 || !scales_ok(lam, mu)) return -1;
  dim3 grid((T + 1 + 255) / 256, S + 1, B);
  hipLaunchKernelGGL(smooth_pxpy_kernel, grid, dim3(256), 0, (hipStream_t)stream, am, lm, am_max,
                     lm_max, nrm, lm_sum, am_dot, log_u, symbols, boundary, S, T, C, blank,
                     1.f - lam - mu, lam, mu, px, py);
  S2T_CHECK_LAUNCH();
  return 0;
}

extern "C" int s2t_rnnt_smooth_bwd(const float* am_probs, const float* lm_probs, const float* G_am,
                                   const float* G_lm, const float* dpx, const float* dpy,
                                   const float* gscale, const long* symbols, const float* lm_sum,
                                   const float* am_dot, const float* u, int B, int S, int T, int C,
                                   int blank, float lam, float mu, float* dlogu_part, float* v,
                                   float* d_am, float* d_lm, void* stream) {
  if (B <= 0) return 0;
  if (S < 0 || T <= 0 || C <= 0 || C > S2T_RNNT_SMOOTH_MAX_C || !scales_ok(lam, mu)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const float alpha = 1.f - lam - mu;
  const long am_rows = (long)B * T, lm_rows = (long)B * (S + 1);
  const int parts = (int)((am_rows + AM_SLAB - 1) / AM_SLAB);
  if (mu != 0.f) {
    hipLaunchKernelGGL((smooth_dam_kernel<true, AM_RPW>), dim3(parts), dim3(256), sizeof(float) * 8 * C, st,
                       am_probs, G_am, dpx, dpy, gscale, symbols, am_dot, u, B, S, T, C, blank,
                       alpha, mu, d_am, dlogu_part);
    S2T_CHECK_LAUNCH();
    hipLaunchKernelGGL((col_sum_kernel<2, 16>), dim3((C + 15) / 16, 1), dim3(256), 0, st,
                       (const float*)dlogu_part, (long)parts, parts, C, (const float*)nullptr, u,
                       (float)lm_rows, v, (float*)nullptr);
    S2T_CHECK_LAUNCH();
    hipLaunchKernelGGL(smooth_dlm_kernel<true>, dim3((unsigned)((lm_rows + 3) / 4)), dim3(256),
                       sizeof(float) * 4 * C, st, lm_probs, G_lm, dpx, dpy, gscale, symbols,
                       lm_sum, v, B, S, T, C, blank, alpha, lam, d_lm);
  } else {
    hipLaunchKernelGGL((smooth_dam_kernel<false, 1>), dim3((unsigned)((am_rows + 3) / 4)), dim3(256),
                       sizeof(float) * 4 * C, st,
                       am_probs, G_am, dpx, dpy, gscale, symbols, am_dot, u, B, S, T, C, blank,
                       alpha, mu, d_am, dlogu_part);
    S2T_CHECK_LAUNCH();
    hipLaunchKernelGGL(smooth_dlm_kernel<false>, dim3((unsigned)((lm_rows + 3) / 4)), dim3(256),
                       sizeof(float) * 4 * C, st, lm_probs, G_lm, dpx, dpy, gscale, symbols,
                       lm_sum, v, B, S, T, C, blank, alpha, lam, d_lm);
  }
  S2T_CHECK_LAUNCH();
  return 0;
}
