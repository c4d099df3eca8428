// LSTM layer of the RNN language model, one launch per time step, the recurrent matrix shared
// across the batch, for gfx950.
//
// Reference: model/lm/rnn_lm.py:40-45 (torch.nn.LSTM, no layer norm), gate order i, f, g, o in rows
// [0,H) [H,2H) [2H,3H) [3H,4H) of weight_hh:
//     a_t = gx_t + h_{t-1} W_hh^T               gx = x W_ih^T + b_ih + b_hh, one GEMM outside
//     c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g)
//     h_t = sigmoid(o) tanh(c_t)
// csrc/lstm.hip gives one workgroup to each utterance and streams all of W_hh per workgroup and
// step: right for the predictor (B a few dozen), wrong for the language model (B = 256: 256 reads
// of the same 4 MB per step).  Here a workgroup owns HS hidden units and BT utterances: its sixteen
// waves form the (BT x HS) tiles of the four gates, h_{t-1}[tile, :] . W_hh[g H + slice, :]^T over
// K = H, wave (g, p) the p-th quarter of K for gate g (a step is latency bound: sixteen short
// chains of loads instead of four long ones), on the f32-input matrix instruction (exact f32: the
// recurrence compounds rounding over T); the sixteen partial tiles meet in LDS and the cell update
// is the epilogue, so one launch finishes a step and W_hh is read once per step and batch tile.  Steps are ordered by the stream alone: no grid-wide
// barrier, no cooperative launch, no flag.  The backward walks t in reverse the same way: the
// workgroup of slice j forms dh_t[:, j] = dhs_t[:, j] + dgates_{t+1} . W_hh[:, j] (K = 4H, wave
// (g, p) takes a quarter of the rows of gate g, against the TRANSPOSED matrix so that both operands are k-contiguous)
// and then dc and the four dgates_t of its slice, all of it slice-local.
//
// Rule: H % 4 == 0 (16-byte operand loads) and H <= 1024 (the rule of csrc/lstm.hip, so that the
// wrapper's small-batch dispatch between the two kernels needs no second rule); B and T are free.
// H need not be a multiple of HS nor B of BT: rows beyond either produce tile entries nobody reads.
#include "common.h"
#include "../../include/s2t_mi355.h"

namespace {

constexpr int HS = 16;         // hidden units per workgroup
constexpr int BT = 16;         // utterances per workgroup
constexpr int NW = 16;         // waves: (gate, or that gate's rows of K in the backward) x (quarter of K)
constexpr int NT = 64 * NW;

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float sigm(float x) { return __fdividef(1.f, 1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
  const float e = __expf(-2.f * fabsf(x));
  const float t = __fdividef(1.f - e, 1.f + e);
  return x < 0.f ? -t : t;
}

// One wave: D[m][n] = sum_{k0 <= k < k1} A[m][k] Bm[n][k] for m, n < 16, both row-major with k
// contiguous and 16-byte aligned rows, k0 % 64 == 0, k1 % 4 == 0.  Rows m >= na of A and n >= nb
// of Bm do not exist: their loads are redirected to the last row that does, and the rows / columns
// of D they produce are never read.
// v_mfma_f32_16x16x4_f32 takes A[lane & 15][k = lane >> 4] and B[k = lane >> 4][lane & 15]; a lane
// loads the float4 at k = 16 c + 4 (lane >> 4) of its row and feeds component i to the i-th of four
// instructions, so instruction i of sub-chunk c sums k = 16 c + 4 q + i over q -- the same k on both
// operands.  Four sub-chunks run on four accumulators (40 cycles of dependent latency against 32
// of issue).  Every load is unconditional (whole 64-chunks; the tail reads a clamped address and
// zeroes what lies at or beyond k1), so the eight of a chunk are in flight together.
// Result: lane holds D[4 (lane >> 4) + r][lane & 15] in component r.
__device__ __forceinline__ void mfma_chunk(f32x4 (&acc)[4], const float4 (&a)[4], const float4 (&b)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u].x, acc[u], 0, 0, 0);
    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u].y, acc[u], 0, 0, 0);
    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u].z, acc[u], 0, 0, 0);
    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u].w, acc[u], 0, 0, 0);
  }
}

__device__ __forceinline__ f32x4 tile_product(const float* __restrict__ A, long lda, int na,
                                              const float* __restrict__ Bm, long ldb, int nb,
                                              int k0, int k1) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const float4* ap = reinterpret_cast<const float4*>(A + min(r, na - 1) * lda);
  const float4* bp = reinterpret_cast<const float4*>(Bm + min(r, nb - 1) * ldb);
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  int kc = k0;
  for (; kc + 64 <= k1; kc += 64) {
    float4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = ap[(kc >> 2) + 4 * u + q];
      b[u] = bp[(kc >> 2) + 4 * u + q];
    }
    mfma_chunk(acc, a, b);
  }
  if (kc < k1) {
    float4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kc + 16 * u + 4 * q;             // this lane's float4 of sub-chunk u
      const int i4 = min(k, k1 - 4) >> 2;
      const bool in = k < k1;
      const float4 av = ap[i4], bv = bp[i4];
      a[u] = make_float4(in ? av.x : 0.f, in ? av.y : 0.f, in ? av.z : 0.f, in ? av.w : 0.f);
      b[u] = make_float4(in ? bv.x : 0.f, in ? bv.y : 0.f, in ? bv.z : 0.f, in ? bv.w : 0.f);
    }
    mfma_chunk(acc, a, b);
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// wave w of the sixteen: gate (w & 3), quarter (w >> 2) of that gate's K range, in whole 64-chunks
__device__ __forceinline__ void k_range(int H, int& k0, int& k1) {
  const int kq = ((H + 255) >> 8) << 6, part = threadIdx.x >> 8;
  k0 = min(H, part * kq);
  k1 = min(H, k0 + kq);
}

// the sixteen waves' tiles -> LDS [wave][utterance][unit] (row padded against bank conflicts)
__device__ __forceinline__ void park_tile(float (*tile)[BT][HS + 1], f32x4 acc) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[w][4 * (lane >> 4) + r][lane & 15] = acc[r];
}

// sum over the four K quarters of gate g
__device__ __forceinline__ float gate_sum(float (*tile)[BT][HS + 1], int g, int b, int j) {
  return (tile[g][b][j] + tile[4 + g][b][j]) + (tile[8 + g][b][j] + tile[12 + g][b][j]);
}

// grid (ceil(H / HS), ceil(B / BT)).  hprev / cprev: the state before this step, (B,H), or NULL =
// zeros; hT / cT: non-NULL on the last step.
__global__ __launch_bounds__(NT) void lstm_step_fwd_kernel(
    const float* __restrict__ gx_t, const float* __restrict__ whh, const float* __restrict__ hprev,
    const float* __restrict__ cprev, int B, int H, float* __restrict__ hs_t,
    float* __restrict__ gates_t, float* __restrict__ cells_t, float* __restrict__ hT,
    float* __restrict__ cT) {
  __shared__ float tile[NW][BT][HS + 1];
  const int j0 = blockIdx.x * HS, b0 = blockIdx.y * BT, g4 = (threadIdx.x >> 6) & 3;
  const int nb = min(HS, H - j0), na = min(BT, B - b0);
  int k0, k1;
  k_range(H, k0, k1);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (hprev)
    acc = tile_product(hprev + (long)b0 * H, H, na, whh + ((long)g4 * H + j0) * H, H, nb, k0, k1);
  park_tile(tile, acc);
  __syncthreads();
  const int j = threadIdx.x & 15, b = threadIdx.x >> 4;
  if (j < nb && b < na) {
    const long row = b0 + b, G = 4L * H;
    const int jj = j0 + j;
    const float* g = gx_t + row * G + jj;
    const float ig = sigm(g[0] + gate_sum(tile, 0, b, j)), fg = sigm(g[H] + gate_sum(tile, 1, b, j));
    const float zg = tanh_f(g[2 * H] + gate_sum(tile, 2, b, j));
    const float og = sigm(g[3 * H] + gate_sum(tile, 3, b, j));
    const float cp = cprev ? cprev[row * H + jj] : 0.f;
    const float c = fg * cp + ig * zg;
    const float h = og * tanh_f(c);
    float* ga = gates_t + row * G + jj;
    ga[0] = ig;
    ga[H] = fg;
    ga[2 * H] = zg;
    ga[3 * H] = og;
    cells_t[row * H + jj] = c;
    hs_t[row * H + jj] = h;
    if (hT) {
      hT[row * H + jj] = h;
      cT[row * H + jj] = c;
    }
  }
}

// dg_next: dgx of step t + 1, (B,4H), or NULL on the last step (then the carried dc is zero too and
// `dc` is only written); cprev: the cell before this step or NULL = zeros.
__global__ __launch_bounds__(NT) void lstm_step_bwd_kernel(
    const float* __restrict__ whh_t, const float* __restrict__ dg_next,
    const float* __restrict__ dhs_t, const float* __restrict__ gates_t,
    const float* __restrict__ cells_t, const float* __restrict__ cprev, int B, int H,
    float* __restrict__ dgx_t, float* __restrict__ dc) {
  __shared__ float tile[NW][BT][HS + 1];
  const int j0 = blockIdx.x * HS, b0 = blockIdx.y * BT, g4 = (threadIdx.x >> 6) & 3;
  const int nb = min(HS, H - j0), na = min(BT, B - b0);
  const long G = 4L * H;
  int k0, k1;
  k_range(H, k0, k1);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (dg_next)
    acc = tile_product(dg_next + (long)b0 * G + (long)g4 * H, G, na,
                       whh_t + (long)j0 * G + (long)g4 * H, G, nb, k0, k1);
  park_tile(tile, acc);
  __syncthreads();
  const int j = threadIdx.x & 15, b = threadIdx.x >> 4;
  if (j < nb && b < na) {
    const long row = b0 + b;
    const int jj = j0 + j;
    const float dh = dhs_t[row * H + jj] +
                     ((gate_sum(tile, 0, b, j) + gate_sum(tile, 1, b, j)) +
                      (gate_sum(tile, 2, b, j) + gate_sum(tile, 3, b, j)));
    const float* ga = gates_t + row * G + jj;
    const float ig = ga[0], fg = ga[H], zg = ga[2 * H], og = ga[3 * H];
    const float tc = tanh_f(cells_t[row * H + jj]);
    const float cp = cprev ? cprev[row * H + jj] : 0.f;
    const float dcv = dh * og * (1.f - tc * tc) + (dg_next ? dc[row * H + jj] : 0.f);
    float* d = dgx_t + row * G + jj;
    d[0] = dcv * zg * ig * (1.f - ig);
    d[H] = dcv * cp * fg * (1.f - fg);
    d[2 * H] = dcv * ig * (1.f - zg * zg);
    d[3 * H] = dh * tc * og * (1.f - og);
    dc[row * H + jj] = dcv * fg;
  }
}

bool width_ok(int H) { return H > 0 && (H & 3) == 0 && H <= 1024; }

}  // namespace

extern "C" {

int s2t_lstm_seq_fwd(const float* gx, const float* whh, const float* h0, const float* c0, int T,
                     int B, int H, float* hs, float* gates, float* cells, float* hT, float* cT,
                     void* stream) {
  if (T <= 0 || B <= 0) return 0;
  if (!width_ok(H)) return -2;
  const dim3 grid((H + HS - 1) / HS, (B + BT - 1) / BT);
  const long BH = (long)B * H;
  for (int t = 0; t < T; ++t) {
    const bool last = t == T - 1;
    hipLaunchKernelGGL(lstm_step_fwd_kernel, grid, dim3(NT), 0, (hipStream_t)stream,
                       gx + t * 4 * BH, whh, t ? hs + (t - 1) * BH : h0,
                       t ? cells + (t - 1) * BH : c0, B, H, hs + t * BH, gates + t * 4 * BH,
                       cells + t * BH, last ? hT : nullptr, last ? cT : nullptr);
  }
  S2T_CHECK_LAUNCH();
  return 0;
}

int s2t_lstm_seq_bwd(const float* whh_t, const float* c0, int T, int B, int H, const float* gates,
                     const float* cells, const float* dhs, float* dgx, float* dc_ws, void* stream) {
  if (T <= 0 || B <= 0) return 0;
  if (!width_ok(H)) return -2;
  const dim3 grid((H + HS - 1) / HS, (B + BT - 1) / BT);
  const long BH = (long)B * H;
  for (int t = T - 1; t >= 0; --t) {
    hipLaunchKernelGGL(lstm_step_bwd_kernel, grid, dim3(NT), 0, (hipStream_t)stream, whh_t,
                       t == T - 1 ? nullptr : dgx + (t + 1) * 4 * BH, dhs + t * BH,
                       gates + t * 4 * BH, cells + t * BH, t ? cells + (t - 1) * BH : c0, B, H,
                       dgx + t * 4 * BH, dc_ws);
  }
  S2T_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
