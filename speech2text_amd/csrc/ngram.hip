// s2t_ngram_score: the back-off n-gram look-up (csrc/ngram_lookup.h, the scoring statement of
// include/s2t_mi355.h) for R independent rows in one launch, for gfx950.  It is the device side of
// NgramLm.score_step and what lets the look-up be held to the host's fp32 evaluation on its own; the
// CTC prefix beam search runs the same device function inside its frame body (csrc/decode_ctc.h).
// s2t_context_score is the same kernel on a hotword graph's tables (THE BIAS STATEMENT of the header).
#include <hip/hip_runtime.h>

#include "../../include/s2t_mi355.h"
#include "common.h"
#include "ngram_lookup.h"

namespace {

using namespace s2t_dec;

constexpr int kNgramThreads = 256;

__global__ __launch_bounds__(kNgramThreads) void ngram_score_kernel(NgramTables g, int R, const int* __restrict__ ctx,
                                                                    const int* __restrict__ token,
                                                                    float* __restrict__ logp, int* __restrict__ next) {
  const int r = blockIdx.x * kNgramThreads + threadIdx.x;
  if (r >= R) return;
  const NgramHit h = ngram_score(g, ngram_clamp(ctx[r], g.num_ctx), ngram_clamp(token[r], g.V));
  logp[r] = h.logp;
  next[r] = h.next;
}

}  // namespace

extern "C" {

int s2t_ngram_score(const S2tNgramLmDesc* lm, int R, const int* ctx, const int* token, float* logp, int* next,
                    void* stream) {
  if (R <= 0) return 0;
  if (!ngram_desc_ok(lm) || !ctx || !token || !logp || !next) return -1;
  hipLaunchKernelGGL(ngram_score_kernel, dim3((R + kNgramThreads - 1) / kNgramThreads), dim3(kNgramThreads), 0,
                     (hipStream_t)stream, ngram_tables(*lm), R, ctx, token, logp, next);
  S2T_CHECK_LAUNCH();
  return 0;
}

// THE BIAS STATEMENT of a hotword graph: the same kernel handed the graph's tables
int s2t_context_score(const S2tContextGraphDesc* graph, int R, const int* state, const int* token, float* score,
                      int* next, void* stream) {
  if (R <= 0) return 0;
  if (!context_desc_ok(graph) || !state || !token || !score || !next) return -1;
  hipLaunchKernelGGL(ngram_score_kernel, dim3((R + kNgramThreads - 1) / kNgramThreads), dim3(kNgramThreads), 0,
                     (hipStream_t)stream, context_tables(*graph), R, state, token, score, next);
  S2T_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
