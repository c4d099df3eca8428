// A stand-alone host program for an undefined-behaviour check of the host paths of the stateless one-launch
// RNN-T searches (csrc/decode_rnnt.hip, csrc/decode.hip): it calls the four size queries and, for each of the
// six search entries and the two resets, the calls of tests/test_rnnt_refusals.py -- a valid tuple with one
// argument broken.  The four hotword entries and their two resets get the same calls, and the breaks of the
// graph's descriptor, bias_weight and bias_score (tests/test_rnnt_bias_f64.py).  Every call returns before any
// launch: a refused one as it stands (-1), one the entry does not test with B = 0 (0).
// tools/run_rnnt_refusals_ubsan.sh builds it with the host side instrumented, next to the sources it links
// against, and runs it; it needs no device.  Exit code 0: every code was the expected one and the sanitizer saw
// nothing.
#include <cmath>
#include <cstdio>
#include <functional>
#include <vector>

#include "s2t_mi355.h"

namespace {

void* const kFake = reinterpret_cast<void*>(0x1000);       // a non-null address no entry follows on the host

struct Args {
  S2tNgramLmDesc desc{};
  const S2tNgramLmDesc* lm = &desc;
  int B = 2, T = 9, V = 11, E = 12, D = 24, ctx = 2, act = 0, blank = 0, beam = 4, topk = 4, mts = 1, max_tokens = 16,
      start_ctx = 0;
  float lm_weight = 0.5f, bias_weight = 1.f;
  void *memory = kFake, *lm_score = kFake, *bias_score = kFake;
  S2tContextGraphDesc gdesc{};
  const S2tContextGraphDesc* graph = &gdesc;
  bool graph_v_broken = false;     // set by the break that puts the graph's V off the call's
  Args() {
    gdesc.V = V, gdesc.max_depth = 6, gdesc.num_ctx = 12, gdesc.num_arcs = 64;
    gdesc.ctx_begin = gdesc.ctx_fail = gdesc.arc_token = gdesc.arc_next = static_cast<const int*>(kFake);
    gdesc.ctx_backoff = gdesc.ctx_final = gdesc.arc_score = static_cast<const float*>(kFake);
    desc.V = V, desc.order = 2, desc.num_ctx = 12, desc.num_arcs = 64;
    desc.ctx_begin = desc.ctx_fail = desc.arc_token = desc.arc_next = static_cast<const int*>(kFake);
    desc.ctx_backoff = desc.arc_logp = static_cast<const float*>(kFake);
  }
};

enum {
  G = 1, GC = 2, B = 4, BN = 8, BC = 16, BNC = 32, R = 64, NR = 128,
  XB = 256, XBN = 512, XBC = 1024, XBNC = 2048, XR = 4096, XNR = 8192,       // the hotword entries and their resets
  BIAS = XB | XBN | XBC | XBNC, SEARCH = 63 | BIAS, BEAMS = 60 | BIAS, NGRAM = 40 | XBN | XBNC, ALL = 16383
};

const float* f(void* p) { return static_cast<const float*>(p); }
const long* l(void* p) { return static_cast<const long*>(p); }
long* lo(void* p) { return static_cast<long*>(p); }

int call(int entry, const Args& a) {
  void* k = kFake;
  float *lms = static_cast<float*>(a.lm_score), *bs = static_cast<float*>(a.bias_score);
  switch (entry) {
    case XB:
      return s2t_rnnt_beam_stateless_bias(a.graph, f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V, a.E,
                                          a.D, a.ctx, a.act, a.blank, a.beam, a.topk, a.bias_weight, a.memory, lo(k),
                                          lo(k), lo(k), static_cast<float*>(k), bs, nullptr);
    case XBN:
      return s2t_rnnt_beam_stateless_ngram_bias(a.lm, a.graph, f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T,
                                                a.V, a.E, a.D, a.ctx, a.act, a.blank, a.beam, a.topk, a.lm_weight,
                                                a.start_ctx, a.bias_weight, a.memory, lo(k), lo(k), lo(k),
                                                static_cast<float*>(k), lms, bs, nullptr);
    case XBC:
      return s2t_rnnt_beam_stateless_bias_chunk(a.graph, f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V,
                                                a.E, a.D, a.ctx, a.act, a.blank, a.beam, a.topk, a.bias_weight,
                                                a.max_tokens, a.memory, lo(k), lo(k), lo(k), static_cast<float*>(k), bs,
                                                lo(k), static_cast<int*>(k), nullptr);
    case XBNC:
      return s2t_rnnt_beam_stateless_ngram_bias_chunk(a.lm, a.graph, f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k),
                                                      a.B, a.T, a.V, a.E, a.D, a.ctx, a.act, a.blank, a.beam, a.topk,
                                                      a.lm_weight, a.bias_weight, a.max_tokens, a.memory, lo(k), lo(k),
                                                      lo(k), static_cast<float*>(k), lms, bs, lo(k),
                                                      static_cast<int*>(k), nullptr);
    case XR:
      return s2t_rnnt_bias_stream_reset(a.memory, nullptr, a.B, a.V, a.ctx, a.beam, a.max_tokens, a.blank, nullptr);
    case XNR:
      return s2t_rnnt_ngram_bias_stream_reset(a.memory, nullptr, a.B, a.V, a.ctx, a.beam, a.max_tokens, a.blank,
                                              a.start_ctx, nullptr);
    case G:
      return s2t_rnnt_greedy_stateless(f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V, a.E, a.D, a.ctx,
                                       a.act, a.mts, a.max_tokens, a.blank, lo(k), lo(k), nullptr);
    case GC:
      return s2t_rnnt_greedy_stateless_chunk(f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V, a.E, a.D,
                                             a.ctx, a.act, a.mts, a.max_tokens, a.blank, a.memory, lo(k), lo(k),
                                             static_cast<int*>(k), nullptr);
    case B:
      return s2t_rnnt_beam_stateless(f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V, a.E, a.D, a.ctx,
                                     a.act, a.blank, a.beam, a.topk, a.memory, lo(k), lo(k), lo(k),
                                     static_cast<float*>(k), nullptr);
    case BN:
      return s2t_rnnt_beam_stateless_ngram(a.lm, f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V, a.E,
                                           a.D, a.ctx, a.act, a.blank, a.beam, a.topk, a.lm_weight, a.start_ctx,
                                           a.memory, lo(k), lo(k), lo(k), static_cast<float*>(k), lms, nullptr);
    case BC:
      return s2t_rnnt_beam_stateless_chunk(f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V, a.E, a.D,
                                           a.ctx, a.act, a.blank, a.beam, a.topk, a.max_tokens, a.memory, lo(k), lo(k),
                                           lo(k), static_cast<float*>(k), lo(k), static_cast<int*>(k), nullptr);
    case BNC:
      return s2t_rnnt_beam_stateless_ngram_chunk(a.lm, f(k), l(k), f(k), f(k), f(k), f(k), f(k), f(k), a.B, a.T, a.V,
                                                 a.E, a.D, a.ctx, a.act, a.blank, a.beam, a.topk, a.lm_weight,
                                                 a.max_tokens, a.memory, lo(k), lo(k), lo(k), static_cast<float*>(k),
                                                 lms, lo(k), static_cast<int*>(k), nullptr);
    case R:
      return s2t_rnnt_stream_reset(a.memory, nullptr, a.B, a.V, a.ctx, a.beam, a.max_tokens, a.blank, nullptr);
    default:
      return s2t_rnnt_ngram_stream_reset(a.memory, nullptr, a.B, a.V, a.ctx, a.beam, a.max_tokens, a.blank,
                                         a.start_ctx, nullptr);
  }
}

struct Break {
  const char* what;
  std::function<void(Args&)> apply;
  int refused_by;                  // the entries that answer -1; the others are called with B = 0
};

}  // namespace

int main() {
  const std::vector<Break> breaks = {
      {"B=0", [](Args& a) { a.B = 0; }, 0},
      {"B=-1", [](Args& a) { a.B = -1; }, 0},
      {"T=0", [](Args& a) { a.T = 0; }, SEARCH},
      {"T=-1", [](Args& a) { a.T = -1; }, SEARCH},
      {"Tc=257", [](Args& a) { a.T = 257; }, GC | BC | BNC | XBC | XBNC},
      {"V=0", [](Args& a) { a.V = a.desc.V = 0; }, ALL},
      {"V=-1", [](Args& a) { a.V = a.desc.V = -1; }, ALL},
      {"V=8193", [](Args& a) { a.V = a.desc.V = 8193; }, ALL & ~G},
      {"V=15323", [](Args& a) { a.V = a.desc.V = 15323; }, ALL},          // one past the greedy LDS rule
      {"E=0", [](Args& a) { a.E = 0; }, SEARCH},
      {"E=-1", [](Args& a) { a.E = -1; }, SEARCH},
      {"E=3801", [](Args& a) { a.E = 3801; }, BEAMS},
      {"E=15324", [](Args& a) { a.E = 15324; }, SEARCH},
      {"D=0", [](Args& a) { a.D = 0; }, SEARCH},
      {"D=-1", [](Args& a) { a.D = -1; }, SEARCH},
      {"D=3813", [](Args& a) { a.D = 3813; }, BEAMS},
      {"D=15336", [](Args& a) { a.D = 15336; }, SEARCH},
      {"ctx=0", [](Args& a) { a.ctx = 0; }, ALL},
      {"ctx=-1", [](Args& a) { a.ctx = -1; }, ALL},
      {"ctx=65", [](Args& a) { a.ctx = 65; }, ALL},
      {"act=-1", [](Args& a) { a.act = -1; }, SEARCH},
      {"act=2", [](Args& a) { a.act = 2; }, SEARCH},
      {"blank=-1", [](Args& a) { a.blank = -1; }, ALL & ~G},
      {"blank=V", [](Args& a) { a.blank = a.V; }, ALL & ~G},
      {"beam=0", [](Args& a) { a.beam = 0; }, BEAMS | NR | XR | XNR},
      {"beam=-1", [](Args& a) { a.beam = -1; }, BEAMS | R | NR | XR | XNR},
      {"beam=17", [](Args& a) { a.beam = 17; }, BEAMS | R | NR | XR | XNR},
      {"topk=0", [](Args& a) { a.topk = 0; }, BEAMS},
      {"topk=-1", [](Args& a) { a.topk = -1; }, BEAMS},
      {"topk=17", [](Args& a) { a.topk = 17; }, 0},
      {"max_token_step=-1", [](Args& a) { a.mts = -1; }, 0},
      {"max_tokens=0", [](Args& a) { a.max_tokens = 0; }, G | GC | BC | BNC | R | NR | XBC | XBNC | XR | XNR},
      {"max_tokens=-1", [](Args& a) { a.max_tokens = -1; }, G | GC | BC | BNC | R | NR | XBC | XBNC | XR | XNR},
      {"lm_weight=nan", [](Args& a) { a.lm_weight = NAN; }, NGRAM},
      {"lm_weight=inf", [](Args& a) { a.lm_weight = INFINITY; }, NGRAM},
      {"start_ctx=-1", [](Args& a) { a.start_ctx = -1; }, BN | NR | XBN | XNR},
      {"start_ctx=num_ctx", [](Args& a) { a.start_ctx = a.desc.num_ctx; }, BN | XBN},
      {"lm=NULL", [](Args& a) { a.lm = nullptr; }, NGRAM},
      {"lm.V=V-1", [](Args& a) { a.desc.V = a.V - 1; }, NGRAM},
      {"lm.order=0", [](Args& a) { a.desc.order = 0; }, NGRAM},
      {"lm.arc_next=NULL", [](Args& a) { a.desc.arc_next = nullptr; }, NGRAM},
      {"memory=NULL", [](Args& a) { a.memory = nullptr; }, ALL & ~G},
      {"lm_score=NULL", [](Args& a) { a.lm_score = nullptr; }, NGRAM},
      {"graph=NULL", [](Args& a) { a.graph = nullptr; }, BIAS},
      {"graph.V=V-1", [](Args& a) { a.gdesc.V = a.V - 1, a.graph_v_broken = true; }, BIAS},
      {"graph.max_depth=65", [](Args& a) { a.gdesc.max_depth = 65; }, BIAS},
      {"graph.ctx_final=NULL", [](Args& a) { a.gdesc.ctx_final = nullptr; }, BIAS},
      {"bias_weight=nan", [](Args& a) { a.bias_weight = NAN; }, BIAS},
      {"bias_weight=-inf", [](Args& a) { a.bias_weight = -INFINITY; }, BIAS},
      {"bias_score=NULL", [](Args& a) { a.bias_score = nullptr; }, BIAS},
  };
  int bad = 0, calls = 0;
  for (const Break& b : breaks)
    for (int entry = G; entry <= XNR; entry <<= 1) {
      Args a;
      b.apply(a);
      a.lm = a.lm ? &a.desc : nullptr;                     // (the copy's own descriptors)
      a.graph = a.graph ? &a.gdesc : nullptr;
      if (!a.graph_v_broken) a.gdesc.V = a.V;              // (the graph's V follows the call's, unless the break set it)
      const bool refused = b.refused_by & entry;
      if (!refused) a.B = a.B > 0 ? 0 : a.B;
      const int want = refused ? -1 : 0, got = call(entry, a);
      ++calls;
      if (got != want) {
        std::printf("entry %d, %s: %d, expected %d\n", entry, b.what, got, want);
        ++bad;
      }
    }
  const long sizes[] = {s2t_rnnt_beam_workspace_bytes(2, 30, 50, 4),         s2t_rnnt_beam_ngram_workspace_bytes(2, 30, 50, 4),
                        s2t_rnnt_stream_state_bytes(2, 50, 2, 4, 16),        s2t_rnnt_stream_state_bytes(2, 50, 2, 0, 16),
                        s2t_rnnt_ngram_stream_state_bytes(2, 50, 2, 4, 16),  s2t_rnnt_beam_workspace_bytes(3, 50, 500, 16),
                        s2t_rnnt_stream_state_bytes(3, 500, 5, 16, 1024),    s2t_rnnt_ngram_stream_state_bytes(3, 500, 5, 16, 1024),
                        s2t_rnnt_beam_workspace_bytes(2, 30, 8193, 4),       s2t_rnnt_beam_ngram_workspace_bytes(2, 30, 8193, 4),
                        s2t_rnnt_stream_state_bytes(2, 50, 2, 17, 16),       s2t_rnnt_ngram_stream_state_bytes(2, 50, 2, 0, 16),
                        s2t_rnnt_bias_stream_state_bytes(2, 50, 2, 4, 16),   s2t_rnnt_ngram_bias_stream_state_bytes(2, 50, 2, 4, 16),
                        s2t_rnnt_bias_stream_state_bytes(2, 50, 2, 0, 16),   s2t_rnnt_ngram_bias_stream_state_bytes(3, 500, 5, 16, 1024)};
  const long want[] = {2816, 2816, 13312, 512, 13824, 105728, 933888, 934656, 263424, 0, 0, 0, 13824, 14336, 0, 935424};
  for (int i = 0; i < 16; ++i)
    if (sizes[i] != want[i]) {
      std::printf("size query %d: %ld, expected %ld\n", i, sizes[i], want[i]);
      ++bad;
    }
  std::printf("%d calls, %d unexpected codes\n", calls, bad);
  return bad ? 1 : 0;
}
