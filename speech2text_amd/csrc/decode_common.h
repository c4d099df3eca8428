// Device functions shared by the RNN-T search kernels (csrc/decode_search.h, csrc/decode_lstm.hip):
// the (value descending, index ascending) order every arg-max / top-k of the searches is taken in,
// and the joiner's activation.  The searches' bookkeeping -- limits, (parent, class) records, candidate
// ranking, trace-back, chunk histories -- is csrc/decode_records.h.
#pragma once
#include "common.h"

namespace s2t_dec {

struct Top {
  float v;
  int i;
};
__device__ __forceinline__ Top better(Top a, Top b) {   // first index wins ties
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
__device__ __forceinline__ Top wave_top(Top a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Top b;
    b.v = __shfl_xor(a.v, o, 64);
    b.i = __shfl_xor(a.i, o, 64);
    a = better(a, b);
  }
  return a;
}
// (v, i) comes strictly after (pv, pi) in the order (value descending, index ascending)
__device__ __forceinline__ bool after(float v, int i, float pv, int pi) {
  return v < pv || (v == pv && i > pi);
}

__device__ __forceinline__ float activate(float v, int act) {
  return act == 0 ? fmaxf(v, 0.f) : tanhf(v);
}

}  // namespace s2t_dec
