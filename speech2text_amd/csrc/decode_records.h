// What the RNN-T beam searches keep besides a predictor, once for the stateless kernels
// (decode_search.h, decode_rnnt.hip) and the lockstep LSTM ones (decode_lstm.hip):
// the limits, the (parent, class) record, candidate ranking, the trace-back of the best beam, and a
// chunk's records turned into histories and outputs.  THREADS is a template parameter: the two
// families launch 512 and 256 (or 64) threads.  Also the Arena that hands out the workspaces and states
// of decode_lstm.hip and decode_ctc.hip and answers their size queries.
#pragma once
#include "common.h"

namespace s2t_dec {

constexpr int kMaxBeam = 16;       // beams, and classes kept per beam
constexpr int kMaxCand = kMaxBeam * kMaxBeam;
constexpr int kTraceFrames = 64;   // frames of records staged in LDS per trace-back step
constexpr int kMaxChunk = 256;     // frames per chunk call

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// A caller's buffer handed out array by array, each on a 256-byte boundary.  Without a base (the
// *_bytes queries) it only adds the sizes up and hands out NULL.
struct Arena {
  char* base;
  size_t bytes = 0;
  explicit Arena(void* b) : base(static_cast<char*>(b)) {}
  template <class T>
  T* take(size_t n) {
    const size_t at = bytes;
    bytes += align256(sizeof(T) * n);
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

// the size a layout takes: its carve function run on an Arena without a base
template <class Carve>
long bytes_of(Carve carve) {
  Arena m(nullptr);
  carve(m);
  return (long)m.bytes;
}

// frames of row b, held to [0, T]
__host__ __device__ __forceinline__ long clamped_len(const long* lengths, int b, int T) {
  const long n = lengths[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

// ------------------------------------------------------------------------------------ the record
// One int per kept beam and frame: its parent's position among the previous frame's beams, its class.
static_assert(kMaxBeam <= 16, "a record keeps the parent position in 4 bits");
__device__ __forceinline__ int pack_record(int parent, int cls) { return parent | (cls << 4); }
__device__ __forceinline__ int record_parent(int r) { return r & 15; }
__device__ __forceinline__ int record_class(int r) { return r >> 4; }

// ------------------------------------------------------------------------------------ ranking
// Thread tid < nc counts the candidates that beat its own (score descending, then candidate index);
// the nnb best write pick[rank] = tid.  cscore, pick: LDS; the barriers around it are the caller's.
__device__ __forceinline__ void rank_candidates(const float* cscore, int nc, int nnb, int* pick) {
  const int tid = threadIdx.x;
  if (tid < nc) {
    const float mine = cscore[tid];
    int rank = 0;
    for (int q = 0; q < nc; ++q) {
      const float o = cscore[q];
      rank += (o > mine || (o == mine && q < tid)) ? 1 : 0;
    }
    if (rank < nnb) pick[rank] = tid;
  }
}

// ------------------------------------------------------------------------------------ trace-back
// The best beam is position 0 after the last frame: its n tokens and the frames they were emitted
// at, from the records rec [Tb][beam].  They are staged in blocks of kTraceFrames through trace (LDS,
// kTraceFrames * kMaxBeam ints); thread 0 walks them and hands the count of tokens still to be found
// to every thread through *left_slot (LDS): the walk ends at the block of the first token.  pos0: the
// position the walk starts at, for a search that reports another beam (the hotword finalisation).
template <int THREADS>
__device__ __forceinline__ void trace_best(const int* __restrict__ rec, int Tb, int beam, int blank, int n,
                                           int* trace, int* left_slot, long* __restrict__ tokens,
                                           long* __restrict__ frames, int pos0 = 0) {
  const int tid = threadIdx.x;
  int pos = pos0, left = n;                                // tokens still to be found
  for (int tend = Tb; tend > 0 && left > 0; tend -= kTraceFrames) {
    const int t0 = max(0, tend - kTraceFrames);
    for (int x = tid; x < (tend - t0) * beam; x += THREADS) trace[x] = rec[(long)t0 * beam + x];
    __syncthreads();
    if (tid == 0) {
      for (int t = tend - 1; t >= t0; --t) {
        const int r = trace[(t - t0) * beam + pos], cls = record_class(r);
        pos = record_parent(r);
        if (cls != blank) {
          --left;
          tokens[left] = cls;
          frames[left] = t;
        }
      }
      *left_slot = left;
    }
    __syncthreads();
    left = *left_slot;                                     // every thread leaves with thread 0
  }
}

// ------------------------------------------------------------------------------------ chunk end
struct ChunkHistoryArgs {
  int Tb, nb, beam, max_tokens, blank;   // frames of this chunk, beams that survive it
  int f0, ovf0;                    // frames before this chunk, overflow so far
  const int* rec;                  // [Tb][beam] records of this chunk
  const int* len;                  // LDS [nb]: tokens of each surviving beam (not clamped)
  const int *otok, *ofrm;          // [beam][max_tokens] histories before this chunk ...
  int *ntok, *nfrm;                // ... and after it: the other buffer, never the same
  long *tokens, *frames;           // [max_tokens] the row's outputs
  int *trace, *anc, *base;         // LDS: kTraceFrames * kMaxBeam, kMaxBeam, kMaxBeam ints
};

// new history = ancestor's old history + this chunk's emissions, kept up to max_tokens: a lane per
// surviving beam walks the chunk's records (staged as in trace_best) back to the beam's ancestor
// position at chunk start, writing the chunk's emissions to the tail of the beam's new history on
// the way; a wave per beam then copies the ancestor's old history in front of them.  Then the best
// beam's (position 0) tokens and frames, and the prefix all live beams share.  All threads call it,
// with the indices the kernel holds; ONE thread then calls done(out_len, stable_len, overflow), where
// the caller writes its own header and scalar outputs.  (decode_rnnt.hip keeps this text written
// out: the call cost its 512-thread kernel, which runs at the limit of its scalar registers, time.)
template <int THREADS, typename Done>
__device__ __forceinline__ void chunk_histories(int tid, int lane, int wave, const ChunkHistoryArgs& a,
                                                Done done) {
  const int BS = a.beam, MT = a.max_tokens, nb = a.nb;
  const bool tracer = wave == 0 && lane < nb;              // a lane per surviving beam
  int pos = lane, left = tracer ? a.len[lane] : 0;
  for (int tend = a.Tb; tend > 0; tend -= kTraceFrames) {
    const int t0 = max(0, tend - kTraceFrames);
    for (int x = tid; x < (tend - t0) * BS; x += THREADS) a.trace[x] = a.rec[t0 * BS + x];
    __syncthreads();
    if (tracer) {
      for (int t = tend - 1; t >= t0; --t) {
        const int r = a.trace[(t - t0) * BS + pos], cls = record_class(r);
        pos = record_parent(r);
        if (cls != a.blank) {
          --left;
          if (left < MT) {
            a.ntok[(long)lane * MT + left] = cls;
            a.nfrm[(long)lane * MT + left] = a.f0 + t;
          }
        }
      }
    }
    __syncthreads();
  }
  if (tracer) {
    a.anc[lane] = pos;                                     // position at chunk start
    a.base[lane] = left;                                   // = that beam's length there
  }
  __syncthreads();
  for (int i = wave; i < nb; i += THREADS / 64) {
    const int anc = a.anc[i], m = min(a.base[i], MT);
    for (int p = lane; p < m; p += 64) {
      a.ntok[(long)i * MT + p] = a.otok[(long)anc * MT + p];
      a.nfrm[(long)i * MT + p] = a.ofrm[(long)anc * MT + p];
    }
  }
  __syncthreads();

  const int n0 = a.len[0], m0 = min(n0, MT);
  for (int p = tid; p < m0; p += THREADS) {
    a.tokens[p] = a.ntok[p];
    a.frames[p] = a.nfrm[p];
  }
  if (wave == 0) {
    int shortest = m0, longest = n0;
    for (int i = 1; i < nb; ++i) {
      shortest = min(shortest, a.len[i]);
      longest = max(longest, a.len[i]);
    }
    int stable = shortest;                                 // first position where two beams differ
    for (int p = lane; p < shortest; p += 64) {
      const int t0 = a.ntok[p];
      bool same = true;
      for (int i = 1; i < nb; ++i) same = same && a.ntok[(long)i * MT + p] == t0;
      if (!same) {
        stable = p;
        break;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) stable = min(stable, __shfl_xor(stable, o, 64));
    if (lane == 0) done(m0, stable, (a.ovf0 || longest > MT) ? 1 : 0);
  }
}

}  // namespace s2t_dec
