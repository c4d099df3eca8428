/* libs2t_mi355.so -- C ABI of the MI355X (gfx950) ASR-training hot path.
 *
 * The reference (guangkun0818/speech2text) has no native layer: its hot path is
 * Python calling torch / torchaudio / k2 ops.  Every entry point below replaces
 * one of those call sites (cited per function, paths relative to the reference
 * tree) and is what a maintainer would bind with ctypes from the same Python
 * module.
 *
 * Conventions: all pointers are DEVICE pointers owned by the caller; fp32 data,
 * int64 ("long") lengths / labels / ranges exactly as the reference's tensors;
 * `stream` is a hipStream_t; nothing allocates or synchronises; the return value
 * is 0 on success, a hipError_t (>0) from the launch, or -1 for invalid sizes.
 */
#ifndef S2T_MI355_H_
#define S2T_MI355_H_

#ifdef __cplusplus
extern "C" {
#endif

/* ---- frontend: dataset/frontend/frontend.py:85-94 (kaldi fbank), + optional
 * model/layer/global_cmvn.py:30-38 fused.  pcm [batch][pcm_stride], num_samples
 * [batch]; out [batch][max_frames][num_mel] (frames past an utterance's own
 * count are the batch padding value 0, CMVN'd if CMVN is fused); out_frames
 * [batch] (may be NULL).  Host-built tables: window400 = povey window,
 * twiddle512 = exp(-2*pi*i*m/512) as (re,im), compact mel filterbank. */
int s2t_fbank_f32(const float* pcm, long pcm_stride, const long* num_samples, int batch,
                  const float* window400, const float* twiddle512, const int* mel_off,
                  const int* mel_k0, const float* mel_w, int nnz, int num_mel, float eps,
                  float scale_in, const float* cmvn_mean, const float* cmvn_istd, float* out,
                  int max_frames, long* out_frames, void* stream);

/* ---- the fbank carried across chunks (csrc/fbank_stream.hip, csrc/fbank_kernel.h): audio arrives in arbitrary cuts, the frames
 * leave as the one-shot kernel would have computed them.  pcm [batch][pcm_stride] holds each row's NEW
 * samples, chunk_samples [batch] how many (clamped to 0..pcm_stride), flush [batch] != 0 ends the row;
 * tables, eps, scale_in and the optional fused CMVN as s2t_fbank_f32; out [batch][max_new_frames]
 * [num_mel], new_frames [batch] (may be NULL).  THE STATEMENT, for row b: the stream so far is the
 * concatenation of every chunk fed since the row's reset, N samples in total; one_shot is
 * s2t_fbank_f32 on those N samples; frames(N) = N >= 400 ? 1 + (N - 400) / 160 : 0.
 *   Frames leave in pairs: pair p (frames 2p and 2p+1) is emitted by the first call after which
 *   N >= 320 p + 560, all newly completed pairs in frame order.  The kernel packs frames 2p and 2p+1
 *   into one complex FFT and a frame's fp32 result depends on its partner at rounding level, so the
 *   pairing is by ABSOLUTE frame index, whatever the cuts.
 *   Flush: with flush[b] != 0 the call also emits the one remaining complete frame, if frames(N) is
 *   odd, packed with the partner the one-shot kernel stages for it: the samples that exist, then
 *   zeros.  After a flush the row is ended: until its reset it accepts no samples (chunk_samples[b] is
 *   read as 0), emits nothing, and its state keeps every bit.
 *   The invariant: the frames a row has emitted up to any call, in order, equal the corresponding rows
 *   of one_shot's output on the N samples the stream holds in the end, bit for bit -- with and
 *   without the fused CMVN, for any scale_in, however the samples were cut, calls of 0 samples
 *   included; after the flush their number is one_shot's out_frames.
 *   Output rows: new_frames[b] = the frames this call emitted for row b; rows of out at or past it
 *   hold the one-shot kernel's padding (0, CMVN'd when CMVN is fused); every element of out is written.
 * State, caller-owned, two buffers:
 *   carry  [batch][S2T_FBANK_CARRY_MAX] fp32   the RAW samples (scale_in is applied where the one-shot
 *          kernel applies it, at staging) from the start of the first un-emitted pair: pair P is
 *          un-emitted exactly when N < 320 P + 560, so at most 559 samples, N - 160 * emitted of them;
 *   counts [batch][S2T_FBANK_STATE_LONGS] int64   N, the frames emitted, the ended flag, 0.
 *   A row is reset by zeroing its counts (its carry need not be cleared: none of it is live).
 * A call of n >= 1 samples emits at most 2 * ((n - 1) / 320 + 1) + 1 frames, one of 0 samples at most
 * 1 (the flush): s2t_fbank_chunk_max_frames(n), a pure host function.  max_new_frames must be at least
 * s2t_fbank_chunk_max_frames(pcm_stride), so that no emitted frame is ever without a row; the grid is
 * sized from max_new_frames, 32 frames to a workgroup.
 * Two launches on `stream`: the frame kernel reads carry and counts in every workgroup and writes
 * neither; a second launch of one workgroup per row then moves the new tail into carry (through
 * registers: the ranges overlap) and writes counts.  Stream order is what keeps a workgroup from
 * overwriting what another still reads.  No host synchronisation, no memset: capturable.
 * Return 0; -1 before any launch for pcm_stride < 0, max_new_frames below the bound, carry or counts
 * NULL, and what s2t_fbank_f32 refuses; batch <= 0 returns 0. */
#define S2T_FBANK_CARRY_MAX 559
#define S2T_FBANK_STATE_LONGS 4
int s2t_fbank_chunk_max_frames(long chunk_samples);
int s2t_fbank_chunk_f32(const float* pcm, long pcm_stride, const long* chunk_samples, const int* flush,
                        int batch, float* carry, long* counts, const float* window400,
                        const float* twiddle512, const int* mel_off, const int* mel_k0,
                        const float* mel_w, int nnz, int num_mel, float eps, float scale_in,
                        const float* cmvn_mean, const float* cmvn_istd, float* out, int max_new_frames,
                        long* new_frames, void* stream);

/* ---- CTC: model/loss/ctc_loss.py:35-41 (log_softmax + nn.CTCLoss).
 * logits [B][T][V] batch-major; targets [B][tgt_stride]; loss_per_utt [B] (nll,
 * or 0 where infinite and zero_infinity); grad_logits [B][T][V] =
 * grad_scale[b] * d nll_b / d logits (NULL to skip).  Umax (padded label width) may be at most
 * S2T_CTC_MAX_LABELS: the 2U+1 lattice states of an utterance live in one workgroup's LDS
 * (128 threads x up to 16 states each); a wider batch returns -4. */
#define S2T_CTC_MAX_LABELS 1023
long s2t_ctc_workspace_floats(int B, int T, int Umax);
int s2t_ctc_loss_fwd_bwd(const float* logits, const long* targets, long tgt_stride,
                         const long* in_len, const long* tgt_len, int B, int T, int V, int Umax,
                         int blank, int zero_infinity, const float* grad_scale, float* workspace,
                         float* loss_per_utt, float* grad_logits, void* stream);

/* ---- CTC forced alignment: the best path of a known transcript over the frames, and from it token
 * times (csrc/ctc_align.hip).  logits [B][T][V] batch-major, raw or already log-probabilities; targets
 * [B][tgt_stride].  THE STATEMENT, for utterance b:
 *   Tb = clamp(lengths[b], 0, T), U = max(tgt_len[b], 0) (and at most Umax); states s = 0..2U;
 *   label(s) = blank for even s, targets[b][s>>1] for odd s;
 *   e[t][s] = logits[b][t][label(s)], gathered exactly (a label outside [0, V) gives -inf); frames at or
 *   beyond Tb are never read;
 *   v[0][0] = e[0][0], v[0][1] = e[0][1], -inf elsewhere; for t >= 1  v[t][s] = m + e[t][s] (one fp32
 *   add), m = max(c0, c1, c2) with c0 = v[t-1][s], c1 = v[t-1][s-1] (s >= 1), c2 = v[t-1][s-2] (only odd
 *   s >= 3 with label(s) != label(s-2)); the backpointer is the FIRST maximum in the order stay, step,
 *   skip: k = 0, then k = 1 if c1 > c0, then k = 2 if c2 > max(c0, c1);
 *   end state 2U, unless U > 0 and !(v[Tb-1][2U] > v[Tb-1][2U-1]): then 2U-1;
 *   feasible (ok = 1) when Tb > 0 and the end value is above -inf, or when Tb == 0 and U == 0 (the empty
 *   path, raw_score = score = 0); the path follows the backpointers from the end state.
 * A per-frame constant does not move the best path, so the recursion runs on the raw logits: a max and
 * one fp32 add per step, which a float32 restatement on the host repeats bit for bit, ties included.
 * Outputs (the caller's buffers; every element is written, none needs zeroing):
 *   path [B][T] int: the lattice state of every frame, -1 at t >= Tb and on infeasible rows;
 *   tok_begin, tok_end [B][Umax] int: the first frame at state 2u+1 and one past the last, -1 for u >= U
 *   and on infeasible rows;
 *   tok_logp [B][Umax]: sum of e[t][2u+1] - lse[t] over the token's frames in frame order in fp32, lse[t]
 *   the row's log-sum-exp; 0 where there is no token;
 *   raw_score [B]: the end value v (-inf on infeasible rows); score [B] = raw_score - sum_t lse[t], the
 *   path's log-probability, -inf on infeasible rows; ok [B] int.
 * Three launches on `stream` (rows, recursion + backtrace, token outputs), no host synchronisation, no
 * memset, no atomics, no cooperative launch: the call can be captured in a graph.
 * s2t_ctc_align_form(T, Umax) names the kernel form that serves a shape: the lattice states per thread
 * of the recursion (1, 2, 4, 8, 16: 128 threads x that many cover 2 Umax + 1), plus
 * S2T_CTC_ALIGN_FORM_WORKSPACE when the 2-bit backpointers of T frames (16 bytes per 64 states and
 * frame, and 2 bytes of path per frame) exceed S2T_CTC_ALIGN_LDS_BYTES of LDS: then they are kept a
 * block of frames at a time, full blocks go to the workspace and are staged back for the backtrace;
 * otherwise they never leave LDS.  -1 for T <= 0 or Umax outside 0..S2T_CTC_MAX_LABELS.
 * s2t_ctc_align_workspace_bytes: 0 for a shape the entry refuses.  Both are pure host functions.
 * Returns as s2t_ctc_loss_fwd_bwd: B <= 0 returns 0; -1 for T <= 0, V <= 0, Umax < 0, blank outside
 * [0, V), tgt_stride < Umax, a NULL workspace or output; -4 for Umax > S2T_CTC_MAX_LABELS; every refusal
 * before any launch and without following a pointer. */
#define S2T_CTC_ALIGN_LDS_BYTES 40960
#define S2T_CTC_ALIGN_FORM_WORKSPACE 256
long s2t_ctc_align_workspace_bytes(int B, int T, int Umax);
int s2t_ctc_align_form(int T, int Umax);
int s2t_ctc_align(const float* logits, const long* lengths, const long* targets, long tgt_stride,
                  const long* tgt_len, int B, int T, int V, int Umax, int blank, void* workspace,
                  int* path, int* tok_begin, int* tok_end, float* tok_logp, float* raw_score,
                  float* score, int* ok, void* stream);

/* ---- RNN-T lattice.  k2 call sites: model/joiner/joiner.py:100-123,
 * model/loss/pruned_rnnt_loss.py:39-48; torchaudio: model/loss/rnnt_loss.py:42-44.
 * am [B][T][C], lm [B][S+1][C], symbols [B][S], boundary [B][4]=(0,0,S_b,T_b),
 * px [B][S][T+1], py [B][S+1][T], p [B][S+1][T+1], ranges [B][T][R]. */
int s2t_fill_f32(float* p, long n, float v, void* stream);
int s2t_rnnt_row_exp(const float* x, long rows, int C, float* probs, float* rowmax, void* stream);
int s2t_rnnt_simple_pxpy(const float* am, const float* lm, const float* am_max,
                         const float* lm_max, const float* nrm, const long* symbols,
                         const long* boundary, int B, int S, int T, int C, int blank, float* px,
                         float* py, void* stream);
int s2t_rnnt_simple_w(const float* dpx, const float* dpy, const float* nrm, const float* gscale,
                      int B, int S, int T, float* W, void* stream);
int s2t_rnnt_simple_bwd(const float* am_probs, const float* lm_probs, const float* G_am,
                        const float* G_lm, const float* dpx, const float* dpy,
                        const float* gscale, const long* symbols, int B, int S, int T, int C,
                        int blank, float* d_am, float* d_lm, int accumulate, void* stream);
/* k2.rnnt_loss_smoothed with lm_only_scale = lam and/or am_only_scale = mu non-zero (both >= 0,
 * lam + mu < 1; alpha = 1 - lam - mu).  With both 0 the three entry points above are the whole
 * path and none of these is called.  am_probs / lm_probs / am_max / lm_max are s2t_rnnt_row_exp's,
 * nrm their product, as above.
 *   stats: lm_sum [B][S+1] = sum_c lm_probs (so Ll = log lm_sum + lm_max, q = lm_probs / lm_sum).
 *     With mu != 0 also the unigram u [C] = mean of q over ALL B (S+1) rows, padded ones included
 *     (+ the smallest normal float, as k2), log_u [C], and am_dot [B][T] = sum_c am_probs u (so
 *     La = log am_dot + am_max); u is reduced column-parallel over slabs of
 *     S2T_RNNT_SMOOTH_LM_SLAB rows into u_part [ceil(B (S+1) / slab)][C], then in one final pass.
 *     With mu == 0 u, log_u, am_dot and u_part are not touched and may be NULL.
 *   pxpy: px / py = alpha (joint) + lam (lm only) + mu (am only) log-probs at the symbol / at the
 *     blank, written in one pass (column T of px and column T_b stay -inf); a scale that is exactly
 *     0 drops its term.
 *   bwd: what s2t_rnnt_simple_bwd does, from the same G_am / G_lm (products of s2t_rnnt_simple_w's
 *     W, which the row kernels scale by alpha), with the lm-only / am-only softmax terms and, for
 *     mu != 0, the gradient through u: the am rows' share of d loss / d log u is reduced over
 *     slabs of S2T_RNNT_SMOOTH_AM_SLAB rows into dlogu_part [ceil(B T / slab)][C], summed into
 *     v [C] = dlogu / (u B (S+1)), and fed to every lm row.  With mu == 0 dlogu_part and v may be
 *     NULL.  C may be at most S2T_RNNT_SMOOTH_MAX_C (two rows per wave in LDS); wider returns -1. */
#define S2T_RNNT_SMOOTH_LM_SLAB 64
#define S2T_RNNT_SMOOTH_AM_SLAB 32
#define S2T_RNNT_SMOOTH_MAX_C 2048
int s2t_rnnt_smooth_stats(const float* am_probs, const float* lm_probs, int B, int S, int T, int C,
                          float mu, float* lm_sum, float* u_part, float* u, float* log_u,
                          float* am_dot, void* stream);
int s2t_rnnt_smooth_pxpy(const float* am, const float* lm, const float* am_max,
                         const float* lm_max, const float* nrm, const float* lm_sum,
                         const float* am_dot, const float* log_u, const long* symbols,
                         const long* boundary, int B, int S, int T, int C, int blank, float lam,
                         float mu, float* px, float* py, void* stream);
int s2t_rnnt_smooth_bwd(const float* am_probs, const float* lm_probs, const float* G_am,
                        const float* G_lm, const float* dpx, const float* dpy,
                        const float* gscale, const long* symbols, const float* lm_sum,
                        const float* am_dot, const float* u, int B, int S, int T, int C, int blank,
                        float lam, float mu, float* dlogu_part, float* v, float* d_am, float* d_lm,
                        void* stream);
/* k2.rnnt_loss_pruned's rnnt_type: an argument of the recursion and of both lattice builders.
 * REGULAR: px [B][S][T+1], columns T and T_b -inf.  MODIFIED: px [B][S][T], no such fix.  CONSTRAINED:
 * MODIFIED, then px[b][s][t] += py[b][s+1][t] (-inf where row s+1 is outside frame t's band).
 * delay_penalty >= 0 (any type): px[b][s][t] += delay_penalty * ((T_b - 1) / 2 - t), a constant without
 * a gradient, so the _bwd entry points take the type only; their dpx is [B][S][T+1] or [B][S][T] as px.
 * An unknown type or a negative penalty returns -1 before anything is launched. */
#define S2T_RNNT_REGULAR 0
#define S2T_RNNT_MODIFIED 1
#define S2T_RNNT_CONSTRAINED 2
/* The recursion.  REGULAR walks the anti-diagonals of px [B][S][T+1]; MODIFIED and CONSTRAINED (k2
 * selects it by px.shape[2] == T) walk the frames, as the symbol arc advances a frame too: p[s][t] =
 * logadd(p[s-1][t-1] + px[s-1][t-1], p[s][t-1] + py[s][t-1]), px and px_grad [B][S][T].  Either way
 * py [B][S+1][T], p [B][S+1][T+1], at most 1024 lattice rows.  An utterance without a path (modified:
 * S_b > T_b, or a band that one symbol per frame cannot follow) scores -inf and has zero gradients. */
int s2t_mutual_info_fwd(const float* px, const float* py, const long* boundary, int B, int S,
                        int T, int rnnt_type, float* p, float* ans, void* stream);
int s2t_mutual_info_bwd(const float* px, const float* py, const long* boundary, const float* p,
                        const float* ans_grad, int B, int S, int T, int rnnt_type, float* px_grad,
                        float* py_grad, void* stream);
int s2t_rnnt_prune_ranges(const float* px_grad, const float* py_grad, const long* boundary, int B,
                          int S, int T, int s_range, long* ranges, void* stream);
/* fused joiner: logits[b,t,i,:] = act(am[b,t,:] + lm[b,ranges[b,t,0]+i,:]) is
 * never materialised; act: 0 = relu, 1 = tanh.  lse [B][T][R]. */
int s2t_rnnt_pruned_fwd(const float* am, const float* lm, const long* ranges,
                        const long* symbols, const long* boundary, int B, int S, int T, int C,
                        int R, int blank, int act, int rnnt_type, float delay_penalty, float* px,
                        float* py, float* lse, void* stream);
int s2t_rnnt_pruned_bwd(const float* am, const float* lm, const long* ranges,
                        const long* symbols, const float* lse, const float* dpx, const float* dpy,
                        const float* gscale, int B, int S, int T, int C, int R, int blank, int act,
                        int rnnt_type, float* d_am, float* d_lm, int accumulate, void* stream);
/* materialised lattice: logits [B][T][R][V]; ranges NULL => full lattice, R = S+1 */
int s2t_rnnt_lattice_fwd(const float* logits, const long* ranges, const long* symbols,
                         const long* boundary, int B, int S, int T, int V, int R, int blank,
                         int rnnt_type, float delay_penalty, float* px, float* py, float* lse,
                         void* stream);
int s2t_rnnt_lattice_bwd(const float* logits, const long* ranges, const long* symbols,
                         const float* lse, const float* dpx, const float* dpy,
                         const float* gscale, int B, int S, int T, int V, int R, int blank,
                         int rnnt_type, float* d_logits, void* stream);

/* ---- RNN-T forced alignment: the best path of a known transcript over the lattice, and from it the
 * frame each token is emitted at (csrc/rnnt_align.hip).  px, py and boundary are exactly the operands of
 * s2t_mutual_info_fwd: px [B][S][T+1] for REGULAR and [B][S][T] for MODIFIED / CONSTRAINED, py
 * [B][S+1][T], boundary [B][4] of which only entries 2 and 3 are read.  THE STATEMENT, for utterance b:
 *   Sb = clamp(boundary[b][2], 0, S), Tb = clamp(boundary[b][3], 0, T); cells (s, t) with 0 <= s <= Sb,
 *   0 <= t <= Tb; v[0][0] = 0; a candidate with no predecessor is -inf;
 *   REGULAR: cl = v[s][t-1] + py[s][t-1] (t >= 1), cu = v[s-1][t] + px[s-1][t] (s >= 1);
 *   MODIFIED and CONSTRAINED (one recursion, as in the loss: the constrained px already carries its
 *   blank): the same cl, cu = v[s-1][t-1] + px[s-1][t-1] (s >= 1 and t >= 1);
 *   each candidate is one fp32 add; v[s][t] = max(cl, cu); the backpointer is the FIRST maximum in the
 *   order blank, symbol: "symbol" exactly when cu > cl;
 *   score[b] = v[Sb][Tb], ok[b] = score > -inf: Sb == Tb == 0 is the empty path with score 0, MODIFIED
 *   with Sb > Tb has no path;
 *   following the backpointers from (Sb, Tb), the symbol arc into row s + 1 gives tok_frame[b][s]: the
 *   frame t it is on for REGULAR, t - 1 otherwise; tok_logp[b][s] is the px value on that arc, gathered
 *   exactly.
 * There is no multiply and no normaliser in the recursion, so a float32 restatement on the host repeats
 * every output bit for bit, ties included.  A cell outside s <= Sb, t <= Tb is never read.
 * Outputs (the caller's buffers; every element is written, none needs zeroing): tok_frame [B][S] int and
 * tok_logp [B][S]: -1 and 0 for s >= Sb and on rows without a path; score [B]: -inf on such rows; ok [B]
 * int.
 * One launch on `stream`: one workgroup per utterance and one thread per lattice row (at most 1024
 * rows, the recursion's limit); no host synchronisation, no memset, no atomics, no cooperative launch:
 * the call can be captured in a graph.
 * s2t_rnnt_align_form(S, T, rnnt_type) names the kernel form that serves a shape: the waves per
 * workgroup, ceil((S + 1) / 64), plus S2T_RNNT_ALIGN_FORM_WORKSPACE when the backpointers of all the
 * steps (S + T + 1 anti-diagonals for REGULAR, T frames otherwise; 8 bytes per step and wave) exceed
 * S2T_RNNT_ALIGN_LDS_BYTES of LDS: then they are kept a block of
 * S2T_RNNT_ALIGN_LDS_BYTES / (8 ceil((S + 1) / 64)) steps at a time (rounded down to whole groups of 8
 * steps, the recursion's look-ahead), full blocks go to the workspace and are staged back for the backtrace; otherwise they never leave LDS and the workspace may be NULL.  -1
 * for a shape the entry refuses.  s2t_rnnt_align_workspace_bytes: 0 for the LDS form and for a shape the
 * entry refuses.  Both are pure host functions.
 * Returns: B <= 0 returns 0; -1 for T <= 0, S < 0, an unknown rnnt_type, (S + 1) (T + 1) floats beyond
 * 2 GiB (an utterance's operands are addressed by 32-bit offsets), a NULL output, a NULL workspace in
 * the workspace form; -4 for S + 1 > 1024; every refusal before any launch and without following a
 * pointer. */
#define S2T_RNNT_ALIGN_LDS_BYTES 40960
#define S2T_RNNT_ALIGN_FORM_WORKSPACE 256
long s2t_rnnt_align_workspace_bytes(int B, int S, int T, int rnnt_type);
int s2t_rnnt_align_form(int S, int T, int rnnt_type);
int s2t_rnnt_align(const float* px, const float* py, const long* boundary, int B, int S, int T,
                   int rnnt_type, void* workspace, int* tok_frame, float* tok_logp, float* score,
                   int* ok, void* stream);


/* ---- zipformer streaming ops (model/layer/scaling.py: Swoosh :1340-1509, BiasNorm
 * :347-476, Balancer backward :741-789 in closed form). */
int s2t_swoosh_fwd(const float* x, float* y, long n, float offset, float constant, void* stream);
int s2t_swoosh_bwd(const float* x, const float* g, float* d, long n, float offset, void* stream);
int s2t_biasnorm_fwd(const float* x, const float* bias, const float* log_scale, long rows, int D,
                     float* y, float* scales, void* stream);
/* s2t_biasnorm_fwd / _bwd with the (B,T,D) -> (T,B,D) transposition of the zipformer frontend's output
 * (model/encoder/zipformer.py:183 `x.transpose(0, 1)` on the output of Conv2dSubsampling.out_norm,
 * model/layer/subsampling.py:262) riding in the pass: x, dx are batch-major (row b T + t), y and g
 * time-major (row t B + b); scales stay in x's row order. */
int s2t_biasnorm_fwd_tb(const float* x, const float* bias, const float* log_scale, int T, int B, int D,
                        float* y, float* scales, void* stream);
int s2t_biasnorm_bwd_tb(const float* x, const float* bias, const float* scales, const float* g, int T,
                        int B, int D, float* dx, float* dbias, float* dls, void* stream);
/* BiasNorm + the layer's bypass as ONE pass each way (the end of Zipformer2EncoderLayer.forward,
 * model/encoder/zipformer.py:1330-1337): out = orig + (x * scales[row] - orig) * bypass_scale[c]
 * (* fm[row % B, c] when fm is given: the stack's feature mask); scales[row] = exp(log_scale) /
 * rms(x - bias) is written for backward, the normalised tensor itself is not.  bwd: g' = g * fm;
 * d_orig = g' (1 - bypass_scale); dx = BiasNorm's backward of g' bypass_scale; d_bypass_scale, dbias,
 * dls are ADDED to.  Equals s2t_biasnorm_fwd + s2t_bypass_fwd[_mask] and s2t_bypass_bwd[_mask] +
 * s2t_biasnorm_bwd. */
int s2t_norm_bypass_fwd(const float* x, const float* bias, const float* log_scale, const float* orig,
                        const float* bypass_scale, const float* fm, int B, long rows, int D, float* out,
                        float* scales, void* stream);
int s2t_norm_bypass_bwd(const float* x, const float* bias, const float* scales, const float* orig,
                        const float* bypass_scale, const float* g, const float* fm, int B, long rows, int D,
                        float* dx, float* d_orig, float* d_bypass_scale, float* dbias, float* dls,
                        void* stream);
int s2t_biasnorm_bwd(const float* x, const float* bias, const float* scales, const float* g,
                     long rows, int D, float* dx, float* dbias, float* dls, void* stream);
/* The whole Balancer backward (model/layer/scaling.py:741-789) in two launches and no fills:
 * out = g + |g| * (a'[c] + b'[c] x); the column statistics of x are accumulated by the first
 * launch, every workgroup of the second derives the per-channel coefficients from them itself.
 * x / g / out are row-strided (ldx / ldg / ldo floats; out == g allowed).  `workspace`:
 * s2t_balancer_bwd_workspace_floats() floats holding two alternating accumulators, zeroed ONCE
 * when allocated; the caller passes parity = 0, 1, 0, 1, ... on successive calls (each call
 * clears the accumulator of the next) and keeps all calls on one stream.  C <= 1024.
 * act_off >= 0: g is the gradient w.r.t. Swoosh(x) (offset act_off: 4 = SwooshL, 1 = SwooshR) and
 * is taken through the activation first -- the hidden Balancer of FeedforwardModule
 * (zipformer.py:1573-1593) and the Swoosh backward in one pass; act_off < 0: plain Balancer. */
long s2t_balancer_bwd_workspace_floats(void);
int s2t_balancer_bwd(const float* x, long ldx, const float* g, long ldg, long rows, int C,
                     float min_mean, float max_mean, float min_rms, float max_rms,
                     float grad_scale, float* out, long ldo, float* workspace, int parity,
                     float act_off, void* stream);
/* the two passes of s2t_balancer_bwd as separate calls: the column statistics (stats: 2 * 1024
 * floats, zeroed by the caller) may be taken where x is produced -- forward pass, side stream --
 * and only the update runs on the data-gradient chain */
int s2t_balancer_stats(const float* x, long ldx, long rows, int C, float* stats, void* stream);
int s2t_balancer_apply(const float* x, long ldx, const float* g, long ldg, long rows, int C,
                       float min_mean, float max_mean, float min_rms, float max_rms,
                       float grad_scale, float* out, long ldo, const float* stats, float act_off,
                       void* stream);


/* ---- zipformer convolution module core (model/encoder/zipformer.py:2672-2690 +
 * model/layer/scaling.py:622-681), time-major.  u (T,B,ld): x = u[..., 0:C], gate
 * pre-activation = u[..., gate_off:gate_off+C] (gate_off < 0: no gate); mask (B,T) bytes,
 * 1 = padded frame (may be NULL); wc (C,(K+1)/2), bc (C): causal taps (NULL for a plain
 * depthwise conv); wk (C,K), bk (C): chunkwise/plain taps; scale (2,C,K) edge scales or NULL;
 * chunk = chunk size in frames (>= T: one chunk).  y (T,B,C).  Backward: du (T,B,2C) (or
 * (T,B,C) without gate) is written; the parameter gradients are ACCUMULATED (zero them). */
int s2t_zipconv_fwd(const float* u, long ld, int gate_off, const unsigned char* mask, int T, int B,
                    int C, int K, int chunk, const float* wc, const float* bc, const float* wk,
                    const float* bk, const float* scale, float* y, void* stream);
/* s2t_zipconv_fwd that also writes y_act = Swoosh(y) (act_kind 1 = SwooshL, 2 = SwooshR): the
 * activation between the depthwise conv and out_proj (model/encoder/zipformer.py:2700-2703) leaves
 * with the conv's output tile instead of re-reading y. */
int s2t_zipconv_fwd_act(const float* u, long ld, int gate_off, const unsigned char* mask, int T, int B,
                        int C, int K, int chunk, const float* wc, const float* bc, const float* wk,
                        const float* bk, const float* scale, float* y, float* y_act, int act_kind,
                        void* stream);
int s2t_zipconv_bwd(const float* u, long ld, int gate_off, const unsigned char* mask, int T, int B,
                    int C, int K, int chunk, const float* wc, const float* wk, const float* bk,
                    const float* scale, const float* dy, float* du, float* dwc, float* dbc,
                    float* dwk, float* dbk, float* dscale, float* workspace, void* stream);
/* the two halves of s2t_zipconv_bwd as separate calls: the parameter gradients only feed the
 * optimizer, so a caller may run them on another stream (ordered after the producers of u / dy;
 * u, dy and workspace alive until that stream is joined) while du stays on the chain */
int s2t_zipconv_bwd_data(const float* u, long ld, int gate_off, const unsigned char* mask, int T,
                         int B, int C, int K, int chunk, const float* wc, const float* wk,
                         const float* bk, const float* scale, const float* dy, float* du,
                         void* stream);
int s2t_zipconv_bwd_params(const float* u, long ld, int gate_off, const unsigned char* mask, int T,
                           int B, int C, int K, int chunk, const float* wc, const float* wk,
                           const float* bk, const float* scale, const float* dy, float* dwc,
                           float* dbc, float* dwk, float* dbk, float* dscale, float* workspace,
                           void* stream);
long s2t_zipconv_bwd_workspace_floats(int T, int B, int C, int K);


/* ---- relative-position attention weights (model/encoder/zipformer.py:1966-2066).
 * qkp (T,B,H*(2*qd+pd)) = in_proj output [q | k | p]; pos (2T-1, H*pd) = linear_pos(pos_emb)
 * or NULL (position term skipped); kpm (B,T) bytes, 1 = padded key; amask (T,T) bytes,
 * 1 = masked (either may be NULL); W (H,B,T,T) softmax weights.  Backward: the gradient
 * of W is passed materialised (dW) and/or factored -- dW0 (B,T,T) for head 0 and up to two
 * (dO_c, V_c) pairs (T,B,H*dv_c) whose outer products are contracted on the fly, so the
 * consumers' (H,B,T,T) gradients are never written; with factors, delta_ws (H,B,T) must hold
 * sum_j W*dW on entry (delta_given=1).  dqkp (T,B,Dp) and dpos fully written (dpos is cleared
 * by the entry point before the partial sums are added; the caller need not zero it).
 * pd == 0 means "no position term" in forward and backward alike: `pos` is then ignored even when
 * it is not NULL (the forward treats it as NULL, the backward writes neither dpos nor workspace). */
int s2t_relpos_attn_fwd(const float* qkp, const float* pos, const unsigned char* kpm,
                        const unsigned char* amask, int T, int B, int H, int qd, int pd, float* W,
                        void* stream);
/* As s2t_relpos_attn_fwd, and *pen_flag (device-visible, e.g. pinned host memory; the caller zeroes
 * it) is set to 1.0f when any raw score -- q.k + p.pos, before masking -- exceeds pen_limit in
 * absolute value: whether the reference's penalize_abs_values_gt(scores, limit=25, penalty=1e-4)
 * (zipformer.py:2010-2026, scaling.py:905-935) contributes a gradient on this call.  Returns -3
 * when the shape is outside the MFMA kernel's range (the only one that reports the limit). */
int s2t_relpos_attn_fwd_flag(const float* qkp, const float* pos, const unsigned char* kpm,
                             const unsigned char* amask, int T, int B, int H, int qd, int pd,
                             float* W, float pen_limit, float* pen_flag, void* stream);
int s2t_relpos_attn_bwd(const float* qkp, const float* pos, const unsigned char* kpm,
                        const unsigned char* amask, int T, int B, int H, int qd, int pd,
                        const float* W, const float* dW, const float* dW0, const float* dO1,
                        const float* V1, int dv1, const float* dO2, const float* V2, int dv2,
                        int delta_given, float* delta_ws, float* dqkp, float* dpos,
                        float* workspace, void* stream);
/* floats of `workspace` (per-(b,h,query block) partial sums of dpos, reduced in a second pass
 * instead of contended atomics); may be NULL when pos is NULL. */
long s2t_relpos_attn_bwd_workspace_floats(int T, int B, int H, int pd);
/* attention apply (model/encoder/zipformer.py:2269): transpose=0: out[i] = sum_j W[i,j] v[j];
 * transpose=1: out[j] = sum_i W[i,j] v[i] (gradient w.r.t. the values).  v,out (T,B,H*dv). */
int s2t_attn_apply(const float* W, const float* v, int T, int B, int H, int dv, int transpose,
                   float* out, void* stream);


/* ---- weight / bias gradient of the linear layers (torch.nn.Linear under loss.backward();
 * model/encoder/zipformer.py:1573-1593 FeedforwardModule, 1966-1992 in_proj, scaling.py
 * ScaledLinear): dW (N,M) = g^T a, db (N) = column sums of g (db may be NULL), for g (R,N) and
 * a (R,M) with row strides ldg/lda (floats), R >> N,M.  The rows are split over the chip and
 * the partial sums land in `workspace` (s2t_linear_wgrad_workspace_floats) before a reduce
 * pass; accumulate=1 adds to dW/db instead of overwriting.  N, M, ldg, lda must be even and
 * the bases 8-byte aligned (-1 otherwise). */
long s2t_linear_wgrad_workspace_floats(int R, int N, int M);
int s2t_linear_wgrad(const float* g, long ldg, const float* a, long lda, int R, int N, int M,
                     float* dW, float* db, int accumulate, float* workspace, void* stream);

/* ---- Whiten gradient shaping (model/layer/scaling.py:949-1095).  Forward, when the module
 * fires: xtx (C,C) = x^T x and colsum (C) (both accumulated by the TN mode of s2t_gemm_f32 over
 * (x, x)) -> per-group centred covariance cov (G,cg,cg), mean (C), scal = [mean diag,
 * sum cov^2 / C, denom, metric]; the metric is also stored to host_metric (pinned host memory,
 * may be NULL) so the host can read it after an event without draining the stream.  xtx and
 * colsum are CONSUMED: the kernel leaves them zeroed, ready for the next accumulating GEMM (no
 * fill launch per call); `workspace` = 4 + 2*C floats, zeroed once when allocated (a
 * self-resetting ticket + per-row partial sums).  Backward: dcov (C,C, block diagonal) =
 * d metric / d cov, bias (C) = -mean . dcov, sums[2] zeroed; the caller forms pg = x dcov + bias
 * with a plain GEMM; s2t_whiten_apply writes out = g + pg * grad_scale * |g| / (|pg| + 1e-20). */
int s2t_whiten_metric(float* xtx, float* colsum, long n, int G, int cg, float* cov, float* mean,
                      float* scal, float* host_metric, float* workspace, void* stream);
/* The fused form of the backward (shapes the pre-split-weight kernel takes): s2t_whiten_prep = s2t_whiten_dcov's dcov / bias, and sums64 = the
 * [2][64] partial-sum slots of the two norms zeroed -- everything that depends on x only, so it runs in
 * FORWARD on the statistics' stream, followed there by s2t_x3p_split of dcov into a per-site piece
 * buffer.  Backward is then s2t_gemm_x3p_sq (pg = x dcov + bias from dcov's pieces, with ||g||^2 and
 * ||pg||^2 taken in its epilogue: the norms are those of the pg actually computed, as the reference
 * takes them) and s2t_whiten_combine64 (out = g + pg * grad_scale ||g|| / (||pg|| + 1e-20)).
 * s2t_gemm_x3p_sq: `other` (= g) and `sums` are required (-1).  Where the pre-split kernel refuses the
 * shape: s2t_whiten_dcov + s2t_gemm_f32_sq + s2t_whiten_combine (sums[2]); where that product's 16-byte
 * rules refuse as well: a plain product + s2t_whiten_apply, which takes the two norms in a pass of its own. */
int s2t_whiten_prep(const float* cov, const float* mean, const float* scal, int G, int cg, float* dcov,
                    float* bias, float* sums64, void* stream);
int s2t_gemm_x3p_sq(const float* A, long lda, const unsigned short* Bp, int N, int K, float* C, long ldc,
                    int M, const float* bias, const float* other, long ld_other, float* sums, int tile,
                    void* stream);
int s2t_whiten_combine64(const float* g, const float* pg, long numel, float grad_scale,
                         const float* sums64, float* out, void* stream);
int s2t_whiten_dcov(const float* cov, const float* mean, const float* scal, int G, int cg,
                    float* dcov, float* bias, float* sums, void* stream);
int s2t_whiten_apply(const float* g, const float* pg, long numel, float grad_scale, float* sums,
                     float* out, void* stream);
/* limit_param_value backward (model/layer/scaling.py:1153-1190): out = g with the sign flipped
 * where (g > 0 and x < lo), then where (g < 0 and x > hi). */
int s2t_limit_param_grad(const float* x, const float* g, float lo, float hi, long n, float* out,
                         void* stream);

/* ---- BEST-RQ labels (model/ssl/best_rq.py:168-217,259-294): stack 9 taps (kernel (3,3),
 * stride (2,2)) -> projection (F*9 -> D) -> nearest code (cosine == euclidean on normalised
 * vectors), label = index + 1, first index on ties.  fp64 internally; bit-exact integer output. */
int s2t_bestrq_labels(const float* feats, int B, int T, int F, const float* proj, int D,
                      const float* codebooks, int ncb, int K, int T2, long* labels, void* stream);


/* col2im of the 3x3 convolutions of Conv2dSubsampling (model/layer/subsampling.py:184-229, the
 * data gradient of nn.Conv2d under loss.backward()) on channel-last data, as one gather pass:
 * dc (B,Ho,Wo,3,3,C) = dy . W^T per patch -> dx (B,H,W,C), Ho = (H-3)/sh+1, Wo = (W-3)/sw+1. */
int s2t_col2im3x3_nhwc(const float* dc, int B, int H, int W, int C, int Ho, int Wo, int sh, int sw,
                       float* dx, void* stream);

/* First subsampling convolution as a direct stencil: Conv2d(1, CO, 3, padding=(0, pw)) of
 * Conv2dSubsampling (model/layer/subsampling.py:184-229) on x (B,H,W) -> y (B,H-2,W+2pw-2,CO),
 * weights in nn.Conv2d's (CO,1,3,3) layout.  mode 0: y = conv(x) + bias; mode 1: dw (CO*9) and
 * db (CO) ACCUMULATED from (x, g) (caller zeroes them); mode 2: dx (B,H,W) from (g, w).  Returns -2
 * for channel counts other than the reference's 8 (the caller then uses im2col + GEMM). */
int s2t_conv3x3_c1(int mode, const float* x, const float* w, const float* bias, const float* g, int B,
                   int H, int W, int pw, int CO, float* y, float* dw, float* db, float* dx,
                   void* stream);

/* Second subsampling convolution as direct kernels: Conv2d(8, 32, 3, stride 2) of
 * Conv2dSubsampling (model/layer/subsampling.py:184-229) on x (B,H,W,8) -> y (B,(H-3)/2+1,
 * (W-3)/2+1,32), weights in nn.Conv2d's (CO,CI,3,3) layout.  mode 0: y = conv(x) + bias; mode 2:
 * dx (B,H,W,8) from (g, w) (the weight gradient stays a TN GEMM over the patch matrix).  Returns -2
 * for other channel counts (the caller then uses im2col + GEMM). */
int s2t_conv3x3_s2(int mode, const float* x, const float* w, const float* bias, const float* g, int B,
                   int H, int W, int CI, int CO, float* y, float* dx, void* stream);

/* ---- 3x3 convolution products with the patch matrix read in place (no im2col copy in HBM):
 * the third subsampling conv and the weight gradients of the second and third
 * (model/layer/subsampling.py:226-243 nn.Conv2d(8,32,3,stride=2), nn.Conv2d(32,128,3,stride=(1,2))).
 * x (B,H,W,C) channel-last, R = B*Ho*Wo output positions, C % 4 == 0 and CO % 4 == 0 (-2 otherwise).
 *   mode 0: out[R,CO] = patches(x)[R,9C] . w2[CO,9C]^T (+ bias[CO]);  w2_or_g = w2 in (cout,kh,kw,cin) order
 *   mode 2: out[CO,9C] += g[R,CO]^T . patches(x)[R,9C],  db[CO] += column sums of g (db may be NULL);
 *           w2_or_g = g; out / db zeroed (or holding the running gradient) by the caller.
 * bf16x3 matrix-core arithmetic: fp32-level error. */
int s2t_conv3x3_gemm(int mode, const float* x, int B, int H, int W, int C, int sh, int sw, int CO,
                     const float* w2_or_g, const float* bias, float* out, float* db, void* stream);

/* ---- channel-last depthwise conv2d of the zipformer frontend (ConvNeXt 7x7,
 * model/layer/subsampling.py:47-53,121).  x,y (N,H,W,C); wgt (C,KH,KW); "same" zero padding.
 * flip=1 applies the flipped taps (= backward data).  wgrad writes dw (C,KH,KW) and db (C). */
int s2t_dwconv2d_nhwc_fwd(const float* x, const float* wgt, const float* bias, int N, int H, int W,
                          int C, int KH, int KW, int flip, float* y, void* stream);
/* same with y = conv(x) + add (add has y's layout; 7x7 only, -2 otherwise): ConvNeXt's residual
 * gradient (subsampling.py:57 `bypass + x`) added inside the backward-data pass. */
int s2t_dwconv2d_nhwc_fwd_add(const float* x, const float* wgt, const float* bias, const float* add,
                              int N, int H, int W, int C, int KH, int KW, int flip, float* y,
                              void* stream);
long s2t_dwconv2d_wgrad_workspace_floats(int N, int H, int C, int KH, int KW);
int s2t_dwconv2d_nhwc_wgrad(const float* x, const float* dy, int N, int H, int W, int C, int KH,
                            int KW, float* workspace, float* dw, float* db, void* stream);

/* ---- fused multi-tensor ScaledAdam + grad-norm clip + zero_grad over one flat fp32 buffer
 * (optimizer/scaled_adam.py:408-527 _get_clipping_scale, :563-736 _step_one_batch / _size_update
 * / _step / _step_scalar; the trainer's gradient_clip_val of config/training/<task>.yaml `trainer:`).
 * The flat buffer holds every tensor padded to 16 bytes; a host-built chunk table cuts each
 * tensor into chunks of s2t_optim_chunk_elems() elements: chunk_off/len/seg [nchunks],
 * seg_chunk_begin [nseg+1], seg_len [nseg].  s2t_seg_stats writes partial [nchunks][3] =
 * (sum g^2, sum p g, sum p^2); s2t_scaled_adam_coef (one workgroup, one param group = tensors
 * [seg_lo,seg_hi)) turns them into per-tensor coefficients segc [nseg][s2t_optim_segc_floats()]
 * and advances the group state (param_rms, scale_exp_avg_sq [nseg_g], scale_grads [P][nseg_g],
 * model_norms [period], fstate [3] = threshold / last norm / last clip factor, istate [3] =
 * has_threshold / num_clipped / non-finite-median flag); s2t_scaled_adam_apply updates
 * p, delta, exp_avg_sq in place and stores the clipped gradient (or zeros if zero_grad).
 * skip (s2t_scaled_adam_coef, s2t_adam_apply): NULL, or a DEVICE flag: != 0 makes the step a no-op
 * on parameters and optimizer state (the gradient is still cleared) -- the data-parallel reducer's
 * "this step's gradient was dropped on every rank" flag (speech2text_amd/ddp.py), no host sync. */
int s2t_optim_chunk_elems(void);
int s2t_optim_segc_floats(void);
int s2t_seg_stats(const float* p, const float* g, const int* chunk_off, const int* chunk_len,
                  int nchunks, float* partial, void* stream);
int s2t_scaled_adam_coef(const float* partial, const int* seg_chunk_begin, const int* seg_len,
                         int nchunks_all, int seg_lo, int seg_hi, float lr, float beta1,
                         float beta2, float eps, float scalar_lr_scale, float param_min_rms,
                         float param_max_rms, float scalar_max, float clip_val,
                         float clipping_scale, int step, int size_update_period,
                         int clipping_update_period, float bc2, float bc2_size, float beta2c,
                         float* param_rms, float* scale_exp_avg_sq, float* scale_grads,
                         float* model_norms, float* fstate, int* istate, float* segstat,
                         float* segc, const float* skip, void* stream);
int s2t_scaled_adam_apply(float* p, float* g, float* delta, float* exp_avg_sq,
                          const int* chunk_off, const int* chunk_len, const int* chunk_seg,
                          int nchunks, const float* segc, int zero_grad, void* stream);

/* ---- fp32 MFMA GEMM family with fused prologue / epilogue (csrc/gemm.hip) for the dense layers:
 * nn.Linear / ScaledLinear / ActivationDropoutAndLinear of model/encoder/zipformer.py:1924-2695,
 * model/layer/scaling.py:1512-1583 and their backward passes.
 *   mode 0 (NT): C[M,N]  = pro_a(A[M,K]) B[N,K]^T  (+ bias[N]) (* act'(act_src)) (+ resid) (+ C)
 *   mode 1 (NN): C[M,N]  = A[M,K] B[K,N]            same epilogue
 *   mode 2 (TN): C[M,N] += A[K,M]^T pro_b(B[K,N])   atomically (split over K); colsum[M] += sum_k A
 * act kinds: 0 none, 1 SwooshL, 2 SwooshR.  Leading dimensions in floats; A and B 16-byte
 * aligned with lda, ldb % 4 == 0 (and K % 4 == 0 for modes 0/1), else -2 (caller falls back to
 * a library GEMM). */
int s2t_gemm_f32(int mode, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                 int M, int N, int K, const float* bias, const float* resid, long ldr,
                 const float* act_src, long lds, int act_kind, int pro_a, int pro_b, float* colsum,
                 int accumulate, void* stream);

/* `batch` independent fp32 products in one launch (bf16x3 matrix cores), X_b = X + b * sX floats:
 * mode 0: C_b[M,N] = A_b[M,K] . B_b[N,K]^T; mode 1: C_b = A_b[M,K] . B_b[K,N];
 * mode 2: C_b[M,N] += A_b[K,M]^T . B_b[K,N] (fp32 atomics: zero C first).  Replaces torch.bmm in
 * the nonlinear attention (reference model/encoder/zipformer.py:2438-2483: attn_weights[0] @ x and
 * its two gradients).  -2 = alignment rules of s2t_gemm_f32 not met (keep the library). */
int s2t_gemm_f32_batched(int mode, const float* A, long lda, long sA, const float* B, long ldb, long sB,
                         float* C, long ldc, long sC, int M, int N, int K, int batch, void* stream);

/* s2t_gemm_f32 modes 0 / 1 (bias only) that also ADDS sums[0] += ||other||_F^2 and sums[1] += ||C||_F^2,
 * other = an (M, N) matrix with rows ld_other apart: the two norms Whiten's backward combines
 * (reference model/layer/scaling.py:1024-1027: x_grad + |x_grad| / |penalty_grad| * grad_scale *
 * penalty_grad), taken while C = x dcov + bias leaves the accumulators instead of by a pass over both
 * tensors.  s2t_whiten_combine is the update that follows (s2t_whiten_apply without its own sums
 * pass).  -2: operands outside the 16-byte epilogue's rules (run s2t_gemm_f32 + s2t_whiten_apply). */
int s2t_gemm_f32_sq(int mode, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                    int M, int N, int K, const float* bias, const float* other, long ld_other,
                    float* sums, void* stream);
int s2t_whiten_combine(const float* g, const float* pg, long numel, float grad_scale, const float* sums,
                       float* out, void* stream);

/* s2t_gemm_f32 modes 0 (NT) / 1 (NN) with the block tile chosen by the caller: tile = "tm tn"
 * digits for a (64 tm) x (64 tn) tile, one of 11 12 21 22 23; 0 = the dispatcher's choice. */
int s2t_gemm_f32_tiled(int mode, const float* A, long lda, const float* B, long ldb, float* C,
                       long ldc, int M, int N, int K, const float* bias, const float* resid,
                       long ldr, int tile, void* stream);

/* Arithmetic of the TN (weight-gradient) products, s2t_gemm_f32 mode 2 / s2t_gemm_tn_grouped /
 * s2t_gemm_xtx: 1 (default) = both fp32 operands split exactly into three bf16
 * pieces, six v_mfma_f32_32x32x16_bf16 products per 16-deep step, fp32 accumulation (fp32-level
 * error); 0 = v_mfma_f32_32x32x2_f32.  set >= 0 selects, set < 0 queries; returns the mode. */
int s2t_tn_x3(int set);
/* Kernel form of the bf16-split TN products (round 5): 1 = wave-specialised
 * 128x128 / 128x192 / 192x128 tiles (producer waves load 16-byte runs and split, consumer waves run
 * the MFMAs; aligned non-symmetric problems: s2t_gemm_f32 mode 2, s2t_gemm_tn_grouped, and
 * s2t_conv3x3_gemm mode 2 with its implicit patch operand); 0 = the all-waves form (every wave splits
 * what it staged and multiplies it: 64x64 tiles under six products, 128x128 under three).  Same
 * arithmetic, different summation order.  With no setting (or set == 2) the form
 * follows the weight-gradient class's arithmetic (s2t_gemm_arith_of(2)): six products -> 1, three -> 0
 * (round 6: measured per step; the implicit-patch product stays on the W form).  set = 0 / 1
 * forces, set = 2 returns to automatic, set < 0 queries; returns the form now in effect. */
int s2t_tn_w(int set);
/* the same switch for the NT / NN products of s2t_gemm_f32 (default 1) */
int s2t_nn_x3(int set);

/* x^T x for the Whiten statistics (model/layer/scaling.py:949-1012): xtx (C,C, ldc) += x^T x and
 * colsum (C) += column sums of x (R,C, ldx), restricted to what the per-group covariance needs:
 * the 64x64 tiles on or above the diagonal that contain a pair of channels of the same group of
 * cg channels.  Tiles below the diagonal are NOT written (s2t_whiten_metric mirrors them). */
int s2t_gemm_xtx(const float* x, long ldx, int R, int C, int cg, float* xtx, long ldc,
                 float* colsum, void* stream);

/* The weight-gradient GEMMs of one layer in ONE launch (mode TN of s2t_gemm_f32, 64x64 tiles):
 * for each problem  C[M,N] += A[K,M]^T . B[K,N]  and  colsum[m] += sum_k A[k][m]  (colsum may be
 * NULL), both scaled by `alpha` (the conformer's 0.5 feed-forward residual weight rides here
 * instead of in a scaling pass over the gradient).  A = the gradient of a Linear's output (rows x out_features), B = its input
 * (rows x in_features), C / colsum = the weight / bias gradient views of the flat gradient buffer
 * (what loss.backward() leaves in .grad for every nn.Linear of
 * model/encoder/zipformer.py:1095-1221).  `probs` is a HOST array of n entries. */
typedef struct S2tTnProblem {
  const float* A;
  long lda;
  const float* B;
  long ldb;
  float* C;
  long ldc;
  int M, N, K;
  float* colsum;
  float alpha;
} S2tTnProblem;
int s2t_gemm_tn_grouped(int n, const S2tTnProblem* probs, void* stream);

/* ---- BEST-RQ SSL heads: fused log-softmax + smoothed-target loss (model/loss/kl_divergence.py:
 * 36-76, model/loss/cross_entropy.py:38-69; call site task_factory/ssl_task.py:140-158).
 * logits [rows][K]; labels [rows]; target t_c = t_other (c != label) / t_label; row_loss[r] =
 * c0 - sum_c t_c log_softmax(scale x)_c; backward grad[r][c] = row_weight[r] * scale *
 * (softmax_c - t_c)  (row_weight = upstream gradient * mask / mask.sum()).  stats
 * [rows][S2T_NLL_STATS] is what the forward saves for the backward: the row maximum of scale x and
 * the log of sum_c exp(scale x_c - maximum), kept apart so that an offset row loses nothing.  A
 * label outside [0, K) matches no class: no label term in the loss, t_c = t_other in the gradient. */
#define S2T_NLL_STATS 2
int s2t_smoothed_nll_fwd(const float* logits, const long* labels, long rows, int K, float scale,
                         float t_other, float t_label, float c0, float* row_loss, float* stats,
                         void* stream);
int s2t_smoothed_nll_bwd(const float* logits, const long* labels, const float* stats,
                         const float* row_weight, long rows, int K, float scale, float t_other,
                         float t_label, float* grad, void* stream);

/* ---- validation-time greedy decoders (model/decoding.py:51-82 CtcGreedyDecoding, :196-271
 * RnntGreedyDecoding; batch_search :27-48 calls them per utterance).  One launch per batch.
 * s2t_ctc_greedy: logits [B][T][V] -> tokens [B][T] (first out_len[b] valid), argmax ties take
 * the first index.  s2t_rnnt_greedy_stateless: am [B][T][V] = joiner enc_proj(encoder_out);
 * stateless predictor parameters (embedding [S][E], depthwise conv [E][ctx], linear [D][E]+[D]),
 * joiner pre_proj [V][D]+[V]; act 0 relu / 1 tanh; at most max_token_step+1 symbols per frame
 * as the reference loop; tokens [B][max_out]. */
int s2t_ctc_greedy(const float* logits, const long* lengths, int B, int T, int V, int blank,
                   long* tokens, long* out_len, void* stream);
int s2t_rnnt_greedy_stateless(const float* am, const long* lengths, const float* emb,
                              const float* conv_w, const float* lin_w, const float* lin_b,
                              const float* pre_w, const float* pre_b, int B, int T, int V, int E,
                              int D, int ctx, int act, int max_token_step, int max_out, int blank,
                              long* tokens, long* out_len, void* stream);

/* ---- RNN-T beam search (model/decoding.py:295-425 RnntBeamDecoding), stateless predictor and a
 * joiner without output projection; inputs as s2t_rnnt_greedy_stateless.  One launch per batch,
 * one workgroup per utterance.  Per frame t < lengths[b] and live beam: lp = log_softmax(act(am[b,t]
 * + lm[beam])); the cutoff_top_k best classes by (value descending, class ascending; a
 * cutoff_top_k above V behaves as V) give one candidate each -- blank keeps the beam's tokens and
 * predictor state, any other class appends it (at most one symbol per frame per beam) -- with
 * score = beam score + lp in fp32; the beam_size best candidates by (score descending, parent beam
 * position ascending, rank in the parent's top-k ascending) are kept, equal hypotheses are not
 * merged.  Outputs are the best beam's after the last frame: tokens [B][T] and frames [B][T]
 * (the frame at which each token was emitted), first out_len[b] valid; score [B].  A zero-length
 * utterance gives no tokens and score 0.  workspace: s2t_rnnt_beam_workspace_bytes(B, T, V,
 * beam_size) bytes of device memory (a pure host function), 256-byte aligned: the (parent, class)
 * records the best beam is traced back through, and the beams' lm rows when they do not fit the
 * LDS.  Returns -1 for shapes the fused search does not take: beam_size or min(cutoff_top_k, V)
 * outside 1..16, V > 8192, ctx > 64, or 16 (E + D) + 128 ctx bytes above 60 KiB. */
long s2t_rnnt_beam_workspace_bytes(int B, int T, int V, int beam_size);
int s2t_rnnt_beam_stateless(const float* am, const long* lengths, const float* emb,
                            const float* conv_w, const float* lin_w, const float* lin_b,
                            const float* pre_w, const float* pre_b, int B, int T, int V, int E,
                            int D, int ctx, int act, int blank, int beam_size, int cutoff_top_k,
                            void* workspace, long* tokens, long* frames, long* out_len,
                            float* score, void* stream);

/* ---- chunk-carried (streaming) RNN-T search: the two searches above fed their frames in pieces
 * (csrc/decode_stream.hip).  Same predictor / joiner parameters, same orders, same limits; the walks
 * are the device functions the whole-utterance kernels run (csrc/decode_search.h), so for ANY cut of
 * [0, L) into chunks -- one frame each, different per row -- tokens, frames, out_len and score after
 * the last chunk are those of the whole-utterance call on the concatenated am with lengths = L, bit
 * for bit, and after every chunk those of the prefix fed so far.  No call synchronises with the
 * host: all of them can be captured into a graph.
 * state: ONE caller-owned device buffer of s2t_rnnt_stream_state_bytes(B, V, ctx, beam_size,
 * max_tokens) bytes (a pure host function; beam_size 0 = the greedy state; a multiple of 256; 0 for
 * B <= 0 or a shape outside the limits: V in 1..8192, ctx in 1..64, beam_size in 0..16, max_tokens
 * >= 1), a row per stream.  Its size does not depend on how many chunks or frames a stream sees.
 * A greedy row holds the predictor state and its lm vector; a beam row holds per beam the score,
 * length, predictor state and lm vector (persisted: a chunk starts without a pass over the
 * predictor's weights), the (parent, class) records of the current chunk's frames only, and two
 * alternating buffers [beam_size][max_tokens] of token and frame histories (int32).
 * s2t_rnnt_stream_reset: a kernel on `stream` that makes every row b with rows[b] != 0 (rows NULL:
 * every row) the empty hypothesis: one beam, score 0, no tokens, predictor state = ctx blanks, frame
 * counter 0, overflow 0.  Other rows are not touched: a slot can end one stream and start another
 * while its neighbours go on.  The caller's output arrays are not reset's to write: they show the
 * new stream from its first chunk with chunk_len > 0 on.
 * A chunk call advances row b over the first min(chunk_len[b], Tc) frames of am [B][Tc][V] from the
 * carried state and stores the state back; Tc <= 256.  chunk_len[b] <= 0 leaves row b's state AND
 * outputs exactly as they were (an idle stream is not a zero-length utterance).  Outputs are the
 * result for the whole stream since its reset:
 * s2t_rnnt_greedy_stateless_chunk: tokens [B][max_tokens] is appended to, so a stream must be given
 *   the same array on every call; out_len [B].  When max_tokens tokens are out the row is inert
 *   until reset (the whole-utterance kernel ends its walk there too) and overflow[b] = 1: later
 *   symbols, if any, are lost.
 * s2t_rnnt_beam_stateless_chunk: the best beam's tokens [B][max_tokens], the frames [B][max_tokens]
 *   at which they were emitted counted from the reset (not from the chunk's start), out_len [B],
 *   score [B], all rewritten by every call with chunk_len > 0.  stable_len [B]: the length of the
 *   longest common prefix of all live beams' token sequences; every later result starts with these
 *   tokens, so it never decreases and a client may print them; with one live beam it is out_len.
 *   A beam that would pass max_tokens keeps its first max_tokens tokens while the search goes on
 *   with exact scores and predictor states: out_len saturates, and overflow[b] = 1 from the first
 *   chunk after which a live beam is longer than max_tokens until reset.
 * Return 0; -1 before any launch (outputs untouched) for Tc outside 1..256, state NULL, max_tokens
 * < 1, or what the whole-utterance call refuses; B <= 0 returns 0. */
long s2t_rnnt_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens);
int s2t_rnnt_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                          int max_tokens, int blank, void* stream);
int s2t_rnnt_greedy_stateless_chunk(const float* am, const long* chunk_len, const float* emb,
                                    const float* conv_w, const float* lin_w, const float* lin_b,
                                    const float* pre_w, const float* pre_b, int B, int Tc, int V,
                                    int E, int D, int ctx, int act, int max_token_step,
                                    int max_tokens, int blank, void* state, long* tokens,
                                    long* out_len, int* overflow, void* stream);
int s2t_rnnt_beam_stateless_chunk(const float* am, const long* chunk_len, const float* emb,
                                  const float* conv_w, const float* lin_w, const float* lin_b,
                                  const float* pre_w, const float* pre_b, int B, int Tc, int V, int E,
                                  int D, int ctx, int act, int blank, int beam_size,
                                  int cutoff_top_k, int max_tokens, void* state, long* tokens,
                                  long* frames, long* out_len, float* score, long* stable_len,
                                  int* overflow, void* stream);

/* ---- RNN-T greedy and beam search with the layer-norm LSTM predictor (model/decoding.py:196-425 over
 * model/predictor/lstm_predictor.py:28-109 and model/joiner/joiner.py:186-207), joiner with or
 * without output projection (csrc/decode_lstm.hip).  The search runs in LOCKSTEP over the batch: a
 * "round" makes one lattice move for every live row (greedy: one row per utterance; beam: beam_size
 * rows per utterance), as a handful of launches ordered by the stream alone.  Per round the rows
 * that emitted a symbol take one predictor step -- LN(embedding[token]); per layer the raw gates
 * x . x2g^T (+ bias) + h . p2g^T tiled over 16 rows x 16 gate rows, so that a weight matrix is read
 * once per round and row tile, then g_norm, i / f / cell / o, c_norm and h per row; LN(linear(h)) and
 * pre_proj give the row's lm vector (V) -- and every live row takes z = act(am[b, t_b] + lm[row]),
 * through the two out-projection Linears when inner > 0, and decides on it.  A device-side count of
 * the rows that emitted lets every launch of a round without one return at once.  A row's result
 * does not depend on the rows that share its launch.  Blank is class 0; the initial state is zero
 * state + one predictor step on blank.
 * S2tRnntLstmDesc: the modules' shapes and parameter addresses.  layer_norm = 0: x2g has a bias and
 * the four norm pointers of a layer are NULL; layer_norm = 1: x2g_b is NULL.  inner = 0: no
 * output projection (out1_* / out2_* unused).  act: 0 relu, 1 tanh.
 * Limits (else -1, before any launch): E, H <= S2T_RNNT_LSTM_MAX_HIDDEN and H % 4 == 0; layers <=
 * S2T_RNNT_LSTM_MAX_LAYERS; V, D, inner <= S2T_RNNT_LSTM_MAX_VOCAB; beam_size and min(cutoff_top_k,
 * V) in 1..S2T_RNNT_LSTM_MAX_BEAM. */
#define S2T_RNNT_LSTM_MAX_HIDDEN 1024
#define S2T_RNNT_LSTM_MAX_LAYERS 8
#define S2T_RNNT_LSTM_MAX_VOCAB 8192
#define S2T_RNNT_LSTM_MAX_BEAM 16
typedef struct S2tLstmLayer {
  const float* x2g_w;              /* (4H, E or H) */
  const float* x2g_b;              /* (4H) or NULL */
  const float* p2g_w;              /* (4H, H) */
  const float *g_gamma, *g_beta;   /* (4H) or NULL */
  const float *c_gamma, *c_beta;   /* (H) or NULL */
} S2tLstmLayer;
typedef struct S2tRnntLstmDesc {
  int V, E, H, D, inner, num_layers, layer_norm, act;
  float in_eps, lstm_eps, out_eps; /* input_layer_norm, g_norm / c_norm, output_layer_norm */
  int pad_;
  const float* emb;                /* (num_symbols, E) */
  const float *in_gamma, *in_beta; /* (E) */
  S2tLstmLayer layers[S2T_RNNT_LSTM_MAX_LAYERS];
  const float *lin_w, *lin_b;      /* predictor linear (D, H), (D) */
  const float *out_gamma, *out_beta;   /* (D) */
  const float *pre_w, *pre_b;      /* joiner pre_proj (V, D), (V) */
  const float *out1_w, *out1_b;    /* out-projection (inner, V), (inner) */
  const float *out2_w, *out2_b;    /* (V, inner), (V) */
} S2tRnntLstmDesc;
/* bytes of device `workspace` (256-byte aligned) of the three calls below for R = B * max(1,
 * beam_size) rows; a pure host function, 0 for a shape outside the limits. */
long s2t_rnnt_lstm_workspace_bytes(const S2tRnntLstmDesc* desc, int B, int T, int beam_size);
/* One predictor step for R rows.  Row r with emit[r] != 0 steps from the state of row parent[r]
 * (parent NULL: r itself) of h_in / c_in [layers][R][H] on tokens[r] and writes its new state to
 * h_out / c_out and its lm vector to lm_out [R][V]; a row with emit[r] == 0 receives the state and
 * the lm_in row of parent[r] unchanged, bit for bit.  In and out buffers are either the same (then
 * parent must be NULL) or disjoint. */
int s2t_lstm_pred_step(const S2tRnntLstmDesc* desc, int R, const int* tokens, const int* emit,
                       const int* parent, const float* h_in, const float* c_in, const float* lm_in,
                       float* h_out, float* c_out, float* lm_out, void* workspace, void* stream);
/* am [B][T][V] = enc_proj(encoder_out); tokens [B][max_out] with max_out = T (max_token_step + 1),
 * zeroed by the caller; out_len [B].  Per row the reference's walk: blank, or more than
 * max_token_step symbols on this frame, moves to the next frame; anything else is emitted and fed
 * to the predictor.  Rounds are enqueued in blocks of 32 with ONE host read (a stream
 * synchronisation) of the device's count of unfinished rows per block, at most T (max_token_step +
 * 2) rounds; finished rows are inert. */
int s2t_rnnt_greedy_lstm(const S2tRnntLstmDesc* desc, const float* am, const long* lengths, int B,
                         int T, int max_token_step, void* workspace, long* tokens, long* out_len,
                         void* stream);
/* The search of s2t_rnnt_beam_stateless (same orders, same outputs) over this predictor and joiner:
 * exactly T rounds, the survivors gather their LSTM state and lm row from their parent's row through
 * two alternating state buffers; no host synchronisation. */
int s2t_rnnt_beam_lstm(const S2tRnntLstmDesc* desc, const float* am, const long* lengths, int B,
                       int T, int beam_size, int cutoff_top_k, void* workspace, long* tokens,
                       long* frames, long* out_len, float* score, void* stream);

/* ---- RNN-LM shallow fusion in the beam search above (csrc/decode_lstm.hip).  Every live beam also
 * carries the state (h, c) of an RNN language model (model/lm/rnn_lm.py: Embedding -> LSTM stack
 * without layer norm -> Linear), the row q[V] = log_softmax(logits(h_last)) of the next token given
 * the beam's tokens, and the running sum lm_sum of the q it was extended by.  The cutoff_top_k classes
 * of a beam are chosen as above (the LM does not enter the cut); the candidate of class c scores
 * score + lp + (c != blank ? lm_weight * q[c] : 0) and sums lm_sum + (c != blank ? q[c] : 0); ranking,
 * selection and records are unchanged.  A kept beam that emitted c steps the LM on c from its
 * parent's LM state in the same round as the predictor, by the same tiled products; a beam that took
 * blank copies its parent's LM state, q and lm_sum bit for bit.  lm_start_token < 0: zero LM state,
 * q = 0 (the first token of a hypothesis carries no LM term, as RnnLm.score scores a sequence);
 * lm_start_token = s in [0, V): the LM is first stepped on s from zero state.  With lm_weight = 0
 * tokens, frames, out_len and score are s2t_rnnt_beam_lstm's bit for bit.
 * S2tRnnLmDesc: layers[l].x2g_w = weight_ih_l (4H, E or H), x2g_b = bias_ih_l + bias_hh_l (4H),
 * p2g_w = weight_hh_l (4H, H), the four norm pointers NULL; gate order i, f, g, o.
 * Limits (else -1 / size 0, before any launch and without following a pointer): lm.V == desc.V; E, H
 * <= S2T_RNNT_LSTM_MAX_HIDDEN and H % 4 == 0; 1 <= num_layers <= S2T_RNNT_LSTM_MAX_LAYERS;
 * lm_start_token < V; lm_weight finite; and the limits of s2t_rnnt_beam_lstm. */
typedef struct S2tRnnLmDesc {
  int V, E, H, num_layers;
  const float* emb;                /* (V, E) */
  S2tLstmLayer layers[S2T_RNNT_LSTM_MAX_LAYERS];
  const float *out_w, *out_b;      /* logits layer (V, H), (V) */
} S2tRnnLmDesc;
/* bytes of device `workspace` of s2t_rnn_lm_step for R rows; 0 outside the limits. */
long s2t_rnn_lm_step_workspace_bytes(const S2tRnnLmDesc* lm, int R);
/* One LM step for R rows, masked and gathered as s2t_lstm_pred_step: row r with emit[r] != 0 steps
 * from the state of row parent[r] (NULL: r) of h_in / c_in [layers][R][H] on tokens[r] and writes its
 * new state and q_out[r] = log_softmax(logits) [R][V]; a row with emit[r] == 0 receives the state and
 * the q_in row of parent[r] bit for bit.  In and out buffers are either the same (then parent must be
 * NULL) or disjoint. */
int s2t_rnn_lm_step(const S2tRnnLmDesc* lm, int R, const int* tokens, const int* emit,
                    const int* parent, const float* h_in, const float* c_in, const float* q_in,
                    float* h_out, float* c_out, float* q_out, void* workspace, void* stream);
long s2t_rnnt_beam_lstm_lm_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int B,
                                           int T, int beam_size);
/* s2t_rnnt_beam_lstm with the LM term; lm_score [B]: the best beam's unweighted lm_sum, so that
 * score = (RNN-T path score) + lm_weight * lm_score.  An utterance without frames: no tokens, score 0,
 * lm_score 0.  Exactly T rounds, no host synchronisation. */
int s2t_rnnt_beam_lstm_lm(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, const float* am,
                          const long* lengths, int B, int T, int beam_size, int cutoff_top_k,
                          float lm_weight, int lm_start_token, void* workspace, long* tokens,
                          long* frames, long* out_len, float* score, float* lm_score, void* stream);

/* ---- The fused search above over the STATELESS predictor (model/predictor/predictor.py: Embedding ->
 * depthwise Conv1d over the last ctx tokens, no bias -> Linear) and the joiner with or without output
 * projection (csrc/decode_lstm.hip).  Same lockstep rounds, same joint, candidates, ranking, records
 * and LM step; a row's predictor state is int ctx[ctx], its last ctx tokens, most recent last, ctx
 * blanks at the start.  A predictor step is three launches: one row kernel (gather of the parent's
 * context, shift, x[r][e] = sum_k conv_w[e][k] emb[ctx[k]][e] in the order k = 0, 1, ..., and the
 * masked copy of context and lm row), then the tiled products lin and pre_proj.
 * S2tRnntStatelessDesc: emb (V, E), conv_w (E, ctx), lin_w (D, E), lin_b (D), pre_w (V, D), pre_b (V),
 * out1_w (inner, V), out1_b, out2_w (V, inner), out2_b (unused when inner == 0); act: 0 relu, 1 tanh;
 * blank is class 0.
 * Limits (else -1 / size 0, before any launch and without following a pointer): 1 <= V, D <=
 * S2T_RNNT_LSTM_MAX_VOCAB; 0 <= inner <= S2T_RNNT_LSTM_MAX_VOCAB; 1 <= E <= S2T_RNNT_LSTM_MAX_HIDDEN;
 * 1 <= ctx <= S2T_RNNT_STATELESS_MAX_CONTEXT (the limit of s2t_rnnt_beam_stateless); act in {0, 1}. */
#define S2T_RNNT_STATELESS_MAX_CONTEXT 64
typedef struct S2tRnntStatelessDesc {
  int V, E, D, ctx, inner, act;
  const float* emb;                /* (V, E) */
  const float* conv_w;             /* (E, ctx) */
  const float *lin_w, *lin_b;      /* predictor linear (D, E), (D) */
  const float *pre_w, *pre_b;      /* joiner pre_proj (V, D), (V) */
  const float *out1_w, *out1_b;    /* out-projection (inner, V), (inner) */
  const float *out2_w, *out2_b;    /* (V, inner), (V) */
} S2tRnntStatelessDesc;
/* bytes of device `workspace` of s2t_stateless_pred_step for R rows; 0 outside the limits. */
long s2t_stateless_pred_step_workspace_bytes(const S2tRnntStatelessDesc* desc, int R);
/* One predictor step for R rows, masked and gathered as s2t_lstm_pred_step: row r with emit[r] != 0
 * takes the context of row parent[r] (parent NULL: r itself) of ctx_in [R][ctx], shifts tokens[r] in
 * (clamped to [0, V)), writes it to ctx_out and lm_out[r] = pre_proj(linear(x[r])) [R][V]; a row with
 * emit[r] == 0 receives the context and the lm_in row of parent[r] bit for bit.  In and out buffers
 * are either the same (then parent must be NULL) or disjoint. */
int s2t_stateless_pred_step(const S2tRnntStatelessDesc* desc, int R, const int* tokens, const int* emit,
                            const int* parent, const int* ctx_in, const float* lm_in, int* ctx_out,
                            float* lm_out, void* workspace, void* stream);
long s2t_rnnt_beam_stateless_lm_workspace_bytes(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm,
                                                int B, int T, int beam_size);
/* s2t_rnnt_beam_lstm_lm over this predictor: same arguments, same outputs, same refusals (lm required,
 * lm.V == desc.V, lm_weight finite, lm_start_token < V, beam_size and min(cutoff_top_k, V) in
 * 1..S2T_RNNT_LSTM_MAX_BEAM).  Exactly T rounds, no host synchronisation.  With lm_weight = 0 and inner
 * == 0 tokens and frames are s2t_rnnt_beam_stateless's and score is within rounding of it (that
 * kernel orders the predictor's sums differently). */
int s2t_rnnt_beam_stateless_lm(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm, const float* am,
                               const long* lengths, int B, int T, int beam_size, int cutoff_top_k,
                               float lm_weight, int lm_start_token, void* workspace, long* tokens,
                               long* frames, long* out_len, float* score, float* lm_score, void* stream);

/* ---- CTC prefix beam search, lexicon-free, equal prefixes merged exactly, with optional RNN-LM shallow
 * fusion (csrc/decode_ctc.hip, csrc/decode_ctc.h).  logits [B][T][V], raw or already normalised; per
 * utterance the frames t < min(lengths[b], T) are searched and no later frame is read.  A live prefix
 * carries pb / pnb, the log-probabilities of its alignments that end in blank / in a non-blank; the
 * search starts from the empty prefix (pb 0, pnb -inf).  Per frame: lp = log_softmax(logits[b][t]) in
 * fp32; the k = min(cutoff_top_k, V) classes by (logit descending, class ascending) are chosen once
 * for all prefixes (the LM does not enter this cut).  With s = logaddexp(pb, pnb) of prefix p, in beam
 * order, class c in rank order: blank adds s + lp[c] to pb of p; c == last(p) adds pnb + lp[c] to pnb of
 * p and pb + lp[c] to pnb of p + c; any other c adds s + lp[c] to pnb of p + c ("adds" is logaddexp; a term
 * of -inf is skipped and makes no candidate).  Candidates with equal token sequences are ONE candidate
 * whatever parents they came from: a per-utterance trie in the workspace gives every sequence ever
 * kept one node id.  Candidates rank by total = logaddexp(pb, pnb) + lm_weight * lm_sum, descending,
 * then first contributing parent, staying before extensions, class rank; the beam_size best survive.
 * tokens [B][T] (zeroed by the caller; at most one token a frame), out_len [B], score [B] = logaddexp(pb,
 * pnb) of the best prefix, the acoustic part alone.  No frames: no tokens, score 0.  beam_size =
 * cutoff_top_k = 1 gives s2t_ctc_greedy's tokens.  s2t_ctc_prefix_beam is one launch, a workgroup per
 * utterance.
 * Limits (else -1 / size 0, before any launch and without following a pointer): beam_size and
 * min(cutoff_top_k, V) in 1..S2T_RNNT_LSTM_MAX_BEAM; 1 <= V <= S2T_RNNT_LSTM_MAX_VOCAB; blank in [0, V);
 * workspace not NULL.  B <= 0 returns 0. */
long s2t_ctc_prefix_beam_workspace_bytes(int B, int T, int V, int beam_size);
int s2t_ctc_prefix_beam(const float* logits, const long* lengths, int B, int T, int V, int blank,
                        int beam_size, int cutoff_top_k, void* workspace, long* tokens, long* out_len,
                        float* score, void* stream);
/* The same search with the LM term: a live prefix also carries the LM state, q[V] = log_softmax(LM
 * logits) of its next token and lm_sum; an extension p + c has lm_sum(p) + q_p[c], a candidate that is a
 * live prefix keeps its own lm_sum, q and state bit for bit; a kept prefix that was not live steps the
 * LM on its last token from its parent's state.  The LM starts as in s2t_rnnt_beam_lstm_lm
 * (lm_start_token < 0: zero state, q = 0).  Exactly T lockstep rounds over the batch, each one search
 * kernel and s2t_rnn_lm_step on B * beam_size rows, no host synchronisation.  lm_score [B] = the best
 * prefix' lm_sum, so that its total is score + lm_weight * lm_score.  With lm_weight = 0 tokens, out_len
 * and score are s2t_ctc_prefix_beam's bit for bit.  Refused as well: lm NULL or outside S2tRnnLmDesc's
 * limits, lm.V != V, lm_start_token >= V, lm_weight not finite. */
long s2t_ctc_prefix_beam_lm_workspace_bytes(const S2tRnnLmDesc* lm, int B, int T, int V, int beam_size);
int s2t_ctc_prefix_beam_lm(const S2tRnnLmDesc* lm, const float* logits, const long* lengths, int B, int T,
                           int V, int blank, int beam_size, int cutoff_top_k, float lm_weight,
                           int lm_start_token, void* workspace, long* tokens, long* out_len, float* score,
                           float* lm_score, void* stream);

/* ---- Back-off n-gram language model over the model's own classes, and the CTC prefix beam search
 * fused with it in ONE launch (csrc/ngram_lookup.h, csrc/ngram.hip, csrc/decode_ctc.hip; the host side
 * and the ARPA reader are model/lm/ngram_lm.py).  The LM's state is one integer, a context node.
 * Tables: ctx_begin [num_ctx + 1] (the arcs of context n are [ctx_begin[n], ctx_begin[n + 1])), ctx_fail
 * [num_ctx] (the context with its oldest token dropped), ctx_backoff [num_ctx] (natural log), arc_token /
 * arc_logp (natural log) / arc_next [num_arcs] (the longest suffix of context + token that is itself a
 * context, precomputed on the host).  Context 0 is the root and is dense: exactly V arcs, arc c is class
 * c.  The arcs of every other context are sorted by token, without duplicates.  The host validates the
 * tables (NgramLm); the kernels trust them, and only clamp what they index with so that no table
 * makes them read outside the arrays.
 * THE SCORING STATEMENT, score(ctx, c) -> (logp, next):  acc = 0.f, n = ctx.  While n != 0: binary-search
 * c among the arcs of n; found at arc a: return (acc + arc_logp[a], arc_next[a]); else acc += ctx_backoff[n],
 * n = ctx_fail[n].  At the root return (acc + arc_logp[c], arc_next[c]).  fp32 adds in exactly this order;
 * at most `order` hops (the loop is bounded by order whatever the tables hold, then the root answers).
 * Limits (else -1 / size 0, before any launch and without following a device pointer): lm and each of
 * its six pointers not NULL; 1 <= V <= S2T_RNNT_LSTM_MAX_VOCAB; order in 1..S2T_NGRAM_MAX_ORDER; num_ctx
 * >= 1; num_arcs >= V. */
#define S2T_NGRAM_MAX_ORDER 8
typedef struct S2tNgramLmDesc {
  int V, order, num_ctx, num_arcs;
  const int *ctx_begin, *ctx_fail;
  const float* ctx_backoff;
  const int* arc_token;
  const float* arc_logp;
  const int* arc_next;
} S2tNgramLmDesc;
/* The statement for R independent rows in one launch: (logp[r], next[r]) = score(ctx[r], token[r]); a ctx
 * outside [0, num_ctx) or a token outside [0, V) is clamped into it.  R <= 0 returns 0. */
int s2t_ngram_score(const S2tNgramLmDesc* lm, int R, const int* ctx, const int* token, float* logp,
                    int* next, void* stream);
/* s2t_ctc_prefix_beam_lm's statement with two changes: q_p[c] is score(state_p, c).logp, and instead of an
 * LM step a kept prefix that was not live takes the `next` its look-up returned.  A live prefix carries
 * its context id; the empty prefix starts in start_ctx, so the first token is scored too; a candidate
 * that lands on a live prefix keeps that prefix' lm_sum and state.  The look-up runs only for an
 * extension that does not land on a live prefix.  There is no end-of-sentence term.  ONE launch, a
 * workgroup per utterance, no host synchronisation (it can be captured in a graph); the workspace is
 * the plain entry's (the tries).  lm_score [B] = the best prefix' lm_sum.  With lm_weight = 0 tokens,
 * out_len and score are s2t_ctc_prefix_beam's bit for bit.  Refused (-1 / size 0): the plain entry's
 * limits, the descriptor's limits above, lm.V != V, start_ctx outside [0, num_ctx), lm_weight not finite. */
long s2t_ctc_prefix_beam_ngram_workspace_bytes(int B, int T, int V, int beam_size);
int s2t_ctc_prefix_beam_ngram(const S2tNgramLmDesc* lm, const float* logits, const long* lengths, int B,
                              int T, int V, int blank, int beam_size, int cutoff_top_k, float lm_weight,
                              int start_ctx, void* workspace, long* tokens, long* out_len, float* score,
                              float* lm_score, void* stream);

/* ---- The n-gram above fused into the one-workgroup RNN-T beam search (csrc/decode_search.h beam_walk's
 * n-gram mode; csrc/decode_beam.hip, csrc/decode_stream.hip).  s2t_rnnt_beam_stateless's statement with
 * the LM term of s2t_rnnt_beam_lstm_lm: a live beam also carries a context id and lm_sum; the cutoff_top_k
 * classes of a beam are chosen as there (the LM does not enter the cut); the candidate of class c !=
 * blank of a beam in context n takes (q, next) = score(n, c) of THE SCORING STATEMENT above, scores
 * (beam score + lp) + lm_weight * q in fp32, in this order, sums lm_sum + q, and a kept beam takes next;
 * a blank candidate carries no LM term and no look-up and keeps its parent's context and lm_sum.  The
 * look-ups of a frame run a thread per candidate, at most beam_size * cutoff_top_k <= 256.  Ranking,
 * selection, records, predictor states and lm rows are unchanged.  The empty hypothesis starts in
 * start_ctx, so the first token is scored too; there is no end-of-sentence term.  ONE launch, a workgroup
 * per utterance, no host synchronisation (it can be captured in a graph); the workspace is the plain
 * entry's.  lm_score [B] = the best beam's lm_sum, so that score = (RNN-T path score) + lm_weight *
 * lm_score up to the order of the adds; a zero-length utterance gives no tokens, score 0 and lm_score 0.
 * With lm_weight = 0 tokens, frames, out_len and score are s2t_rnnt_beam_stateless's bit for bit.
 * Refused (-1 / size 0, before any launch and without following a pointer): what s2t_rnnt_beam_stateless
 * refuses, the descriptor's limits above, lm.V != V, start_ctx outside [0, num_ctx), lm_weight not
 * finite, lm_score NULL. */
long s2t_rnnt_beam_ngram_workspace_bytes(int B, int T, int V, int beam_size);
int s2t_rnnt_beam_stateless_ngram(const S2tNgramLmDesc* lm, const float* am, const long* lengths,
                                  const float* emb, const float* conv_w, const float* lin_w,
                                  const float* lin_b, const float* pre_w, const float* pre_b, int B, int T,
                                  int V, int E, int D, int ctx, int act, int blank, int beam_size,
                                  int cutoff_top_k, float lm_weight, int start_ctx, void* workspace,
                                  long* tokens, long* frames, long* out_len, float* score, float* lm_score,
                                  void* stream);
/* The search above fed its frames in pieces: s2t_rnnt_beam_stateless_chunk's contract word for word
 * (idle rows keep state and outputs, stable_len, the max_tokens saturation and overflow, Tc in 1..256,
 * reset of chosen rows only), with lm_score [B] beside score.  The frame body is the one-shot kernel's
 * own, so for ANY cut tokens, frames, out_len, score and lm_score after a chunk are
 * s2t_rnnt_beam_stateless_ngram's on the frames fed so far, bit for bit.
 * state: s2t_rnnt_ngram_stream_state_bytes(B, V, ctx, beam_size, max_tokens) bytes, beam_size in 1..16 (0
 * for what s2t_rnnt_stream_state_bytes refuses, and for beam_size 0: there is no greedy form).  A row is
 * the plain beam row of s2t_rnnt_stream_state_bytes, unchanged, followed by ctx [beam_size] int32, the
 * beams' context ids, and lm_sum [beam_size] fp32, padded to a multiple of 256.
 * s2t_rnnt_ngram_stream_reset: s2t_rnnt_stream_reset, and the one beam of a reset row starts in start_ctx
 * with lm_sum 0; -1 as well for start_ctx < 0 (reset sees no tables: a chunk call clamps the context ids
 * it loads into [0, num_ctx)).  The chunk call refuses what s2t_rnnt_beam_stateless_chunk and, of the LM
 * arguments, s2t_rnnt_beam_stateless_ngram refuse. */
long s2t_rnnt_ngram_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens);
int s2t_rnnt_ngram_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                                int max_tokens, int blank, int start_ctx, void* stream);
int s2t_rnnt_beam_stateless_ngram_chunk(const S2tNgramLmDesc* lm, const float* am, const long* chunk_len,
                                        const float* emb, const float* conv_w, const float* lin_w,
                                        const float* lin_b, const float* pre_w, const float* pre_b, int B,
                                        int Tc, int V, int E, int D, int ctx, int act, int blank,
                                        int beam_size, int cutoff_top_k, float lm_weight, int max_tokens,
                                        void* state, long* tokens, long* frames, long* out_len, float* score,
                                        float* lm_score, long* stable_len, int* overflow, void* stream);

/* ---- chunk-carried (streaming) CTC prefix beam search: the two searches above fed their frames in
 * pieces (csrc/decode_ctc.hip).  logits [B][Tc][V], Tc in 1..256; row b advances over the first n =
 * min(chunk_len[b], Tc) frames of the chunk and reads no later frame.  A frame is the one-shot entries'
 * own device function (csrc/decode_ctc.h ctc_frame, ctc_finish; the LM family's round is their round
 * kernel plus s2t_rnn_lm_step), no frame body is forked or restated, so:
 * EQUALITY.  For ANY cut of [0, L) into chunks -- one frame each, different per row, idle calls in
 * between -- while overflow[b] == 0, tokens[b][:out_len[b]], out_len, score and lm_score after the last
 * chunk are those of the one-shot entry on the concatenated logits with lengths = L, bit for bit, and
 * after every chunk those of the prefix fed so far.  Through the LM entry with lm_weight = 0 tokens,
 * out_len, score, stable_len and overflow are the plain chunk entry's bit for bit.  beam_size =
 * cutoff_top_k = 1 gives s2t_ctc_greedy's tokens of the frames fed so far.
 * IDLE ROWS.  chunk_len[b] <= 0 leaves row b's state and all its outputs exactly as they were (in the LM
 * family with one exception, the per-call arrays eff and emit / parent / token: they are scratch,
 * rewritten for every row by every call -- eff by its begin kernel, the others by every round and every
 * reset -- before anything reads them, and carry nothing from call to call).
 * THE TRIE DOES NOT GROW WITH THE STREAM.  stable_len[b] is the length of the longest common prefix of
 * all live prefixes, the depth of the lowest common ancestor of the live nodes.  Every later live
 * prefix descends from a live one, so stable_len never decreases and tokens[b][:stable_len[b]] never
 * change again; no sequence outside that ancestor's subtree can be live again; and a sequence that is
 * not on a path from the ancestor to a live node gets from a fresh node what it got from its old one
 * (node ids enter results only through "is p + c live"; rank keys are slots).  Hence every call that
 * consumes frames ends by compacting the row's trie -- always, not when room is short: one code path,
 * the same launches every replay: the ancestor becomes the root, only the union of the root-to-live
 * paths survives, renumbered in ascending order of the old ids (parent id < child id still holds), the
 * child lists filtered in their order; the ancestor's depth is kept per row as the committed depth;
 * prefix lengths stay absolute.  The trace-back of a call walks from the best node to the root only and
 * writes tokens[b][p] for p from the committed depth up; positions below it were written by earlier
 * calls, so a stream must pass the SAME tokens array [B][max_tokens] on every call (as
 * s2t_rnnt_greedy_stateless_chunk requires).  A call's cost follows the unstable region, not the
 * stream.  Every walk (sibling list, path to the root, ancestor) carries a hop bound: a corrupt state
 * ends in a wrong answer, never in a hang.
 * OVERFLOW, bits of overflow[b].  Bit 1 (value 2), nodes: row b consumes its n frames if and only if
 * kept + beam_size * n <= max_nodes, kept = the row's node count after its last compaction (1 after a
 * reset); otherwise the call consumes none of them, sets bit 1 and the row is inert until reset, its
 * state and outputs as they were: no write lands outside the node array.  Bit 0 (value 1), tokens: a
 * best prefix longer than max_tokens keeps its first max_tokens tokens in the array, out_len and
 * stable_len saturate there, the search goes on with exact scores.
 * state: ONE caller-owned buffer of s2t_ctc_stream_state_bytes / s2t_ctc_lm_stream_state_bytes bytes (a
 * multiple of 256, independent of the frames seen), every array 256-byte aligned, in this order, R = B *
 * beam_size, M = B * max_nodes:
 *   nodes   [M] x 16 B   the trie (int32 parent, token, first_child, next_sibling), a row's at b * max_nodes
 *   stage   [M] x 16 B   where a compaction builds the surviving nodes before they are copied back
 *   map     [M] int32    old node id -> new id, -1 dropped (scratch of a compaction)
 *   pb, pnb, lm_sum [R] fp32;  node, last, len [R] int32     the live prefixes in beam order
 *   nb, kept [B] int32   live prefixes; nodes after the last compaction
 *   depth, ovf [B] int32 the committed depth; the overflow bits
 *   eff     [B] int64    frames the current call consumes (scratch; the LM rounds' lengths)
 *   LM family only: emit, parent, token [R] int32 (what s2t_rnn_lm_step is asked: scratch), h, c
 *   [lm.layers][R][lm.H], q [R][V] fp32: the LIVE copy of the LM's state.
 * workspace (LM family): s2t_ctc_prefix_beam_lm_chunk_workspace_bytes bytes of scratch, independent of
 * Tc, serving every call and the reset: the second copy of h, c, q and s2t_rnn_lm_step's workspace.  The
 * rounds alternate between the copies; the LM step after the chunk's last frame IS enqueued (the next
 * chunk's first frame reads it; outputs do not depend on it), and after an odd Tc ONE launch copies the
 * survivors home, so the launches of a call depend on its arguments alone.
 * *_stream_reset: every row b with rows[b] != 0 (rows NULL: every row) becomes the empty prefix: root
 * node only, pb 0, pnb -inf, committed depth 0, overflow 0; the LM family also zeroes the row's LM
 * state and q and, with lm_start_token >= 0, makes the one-shot entry's own first LM step on that
 * token, masked by rows.  Other rows keep every bit (but the scratch arrays named above).  The
 * caller's outputs are not reset's to write.
 * s2t_ctc_prefix_beam_chunk is ONE launch, a workgroup per utterance; s2t_ctc_prefix_beam_lm_chunk is a
 * begin kernel (admission, the effective lengths), exactly Tc lockstep rounds, the copy home after an odd
 * Tc and an end kernel (outputs, compaction).  No host synchronisation, no cooperative launch, no memset:
 * reset and chunk calls can be captured into a graph and replayed.
 * Return 0; -1 / size 0 before any launch (outputs untouched, no pointer followed) for Tc outside
 * 1..256, state (or workspace, lm) NULL, max_tokens < 1, max_nodes outside 1..S2T_CTC_STREAM_MAX_NODES, and
 * what the one-shot entries refuse; B <= 0 returns 0.  The size functions are pure host functions. */
#define S2T_CTC_STREAM_MAX_NODES 1048576
long s2t_ctc_stream_state_bytes(int B, int V, int beam_size, int max_nodes);
int s2t_ctc_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                         void* stream);
int s2t_ctc_prefix_beam_chunk(const float* logits, const long* chunk_len, int B, int Tc, int V, int blank,
                              int beam_size, int cutoff_top_k, int max_tokens, int max_nodes, void* state,
                              long* tokens, long* out_len, float* score, long* stable_len, int* overflow,
                              void* stream);
long s2t_ctc_lm_stream_state_bytes(const S2tRnnLmDesc* lm, int B, int V, int beam_size, int max_nodes);
long s2t_ctc_prefix_beam_lm_chunk_workspace_bytes(const S2tRnnLmDesc* lm, int B, int V, int beam_size);
int s2t_ctc_lm_stream_reset(const S2tRnnLmDesc* lm, int lm_start_token, void* state, const int* rows, int B,
                            int V, int beam_size, int max_nodes, void* workspace, void* stream);
int s2t_ctc_prefix_beam_lm_chunk(const S2tRnnLmDesc* lm, const float* logits, const long* chunk_len, int B,
                                 int Tc, int V, int blank, int beam_size, int cutoff_top_k, float lm_weight,
                                 int lm_start_token, int max_tokens, int max_nodes, void* state,
                                 void* workspace, long* tokens, long* out_len, float* score, float* lm_score,
                                 long* stable_len, int* overflow, void* stream);
/* The n-gram search (s2t_ctc_prefix_beam_ngram) fed its frames in pieces: the chunk-carried block's
 * contract above word for word -- EQUALITY, IDLE ROWS, the compaction, both OVERFLOW bits, the refusals --
 * with s2t_ctc_prefix_beam_ngram as the one-shot partner: for ANY cut, while overflow[b] == 0,
 * tokens[b][:out_len[b]], out_len, score and lm_score after a chunk are the one-shot entry's on the frames
 * fed so far, bit for bit.  With lm_weight = 0 tokens, out_len, score, stable_len and overflow are
 * s2t_ctc_prefix_beam_chunk's bit for bit.  ONE launch per call, a workgroup per utterance: the plain
 * chunk kernel's shape in the frame body's n-gram mode (admission, the beam and its context ids, the
 * frames, outputs and compaction); no workspace, no host synchronisation; it can be captured in a graph.
 * state: s2t_ctc_ngram_stream_state_bytes(B, V, beam_size, max_nodes) bytes: the plain state of
 * s2t_ctc_stream_state_bytes first, byte for byte in the same order (lm_sum is part of it), followed by
 *   ctx     [R] int32    the live prefixes' context ids, in beam order
 * 256-byte aligned like every other array.  A context id belongs to a beam position, not to a trie node:
 * the compaction leaves it alone.
 * s2t_ctc_ngram_stream_reset: s2t_ctc_stream_reset, and the one live prefix of a reset row starts in
 * start_ctx with lm_sum 0; -1 as well for start_ctx < 0 (reset sees no tables: a chunk call clamps every
 * context id it loads into [0, num_ctx)).
 * The chunk call refuses (-1, before any launch and without following a device pointer) what
 * s2t_ctc_prefix_beam_chunk refuses and, of the LM arguments, what s2t_ctc_prefix_beam_ngram refuses (the
 * descriptor's limits, lm.V != V, lm_weight not finite), and a NULL lm_score. */
long s2t_ctc_ngram_stream_state_bytes(int B, int V, int beam_size, int max_nodes);
int s2t_ctc_ngram_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                               int start_ctx, void* stream);
int s2t_ctc_prefix_beam_ngram_chunk(const S2tNgramLmDesc* lm, const float* logits, const long* chunk_len,
                                    int B, int Tc, int V, int blank, int beam_size, int cutoff_top_k,
                                    float lm_weight, int max_tokens, int max_nodes, void* state, long* tokens,
                                    long* out_len, float* score, float* lm_score, long* stable_len,
                                    int* overflow, void* stream);

/* ---- Hotword (contextual) biasing of the CTC prefix beam search (csrc/ngram_lookup.h, csrc/ngram.hip,
 * csrc/decode_ctc.h, csrc/decode_ctc.hip; the host side is model/lm/context_graph.py).  The caller's
 * phrases (token-id lists) are compiled to an Aho-Corasick automaton in the n-gram's table form: a state
 * is the longest suffix of a hypothesis that begins a phrase.  On a whole history h:
 *   match(h)      the longest suffix of h that is a prefix (proper or whole) of some phrase
 *   bias_sum(h) = context_score * len(match(h)) + sum over k in 1..len(h), over every phrase p that h[:k]
 *                 ends with, of bonus(p)          (the first term is a loan, paid back when the match is lost)
 *   final_bias(h) = bias_sum(h) without the first term
 * Tables: ctx_begin [num_ctx + 1], ctx_fail [num_ctx] (the longest proper suffix of the state that is a
 * state), ctx_backoff [num_ctx] = context_score * (depth(fail[n]) - depth(n)), ctx_final [num_ctx] =
 * -context_score * depth(n), arc_token / arc_score / arc_next [num_arcs]; arc_score = context_score + the
 * bonuses of every phrase ending at the arc's target.  State 0 is the root and is dense: exactly V arcs,
 * arc c is class c (score 0 and next 0 for a class no phrase starts with).  The arcs of every other state
 * are sorted by token, without duplicates.  The host validates the tables (ContextGraph).
 * THE BIAS STATEMENT, bias(state, c) -> (score, next):  acc = 0.f, n = state.  While n != 0: binary-search c
 * among the arcs of n; found at arc a: return (acc + arc_score[a], arc_next[a]); else acc += ctx_backoff[n],
 * n = ctx_fail[n].  At the root return (acc + arc_score[c], arc_next[c]).  fp32 adds in exactly this
 * order; the loop is bounded by max_depth + 1 whatever the tables hold (then the root answers), and every
 * index taken from a table is clamped into its array.  It is THE SCORING STATEMENT's device function,
 * handed these tables.
 * Limits (else -1 / size 0, before any launch and without following a device pointer): graph and each of
 * its seven pointers not NULL; 1 <= V <= S2T_RNNT_LSTM_MAX_VOCAB; max_depth in 0..S2T_CONTEXT_MAX_DEPTH;
 * num_ctx >= 1; num_arcs >= V. */
#define S2T_CONTEXT_MAX_DEPTH 64
typedef struct S2tContextGraphDesc {
  int V, max_depth, num_ctx, num_arcs;
  const int *ctx_begin, *ctx_fail;
  const float *ctx_backoff, *ctx_final;
  const int* arc_token;
  const float* arc_score;
  const int* arc_next;
} S2tContextGraphDesc;
/* The statement for R independent rows in one launch: (score[r], next[r]) = bias(state[r], token[r]); a
 * state outside [0, num_ctx) or a token outside [0, V) is clamped into it.  R <= 0 returns 0. */
int s2t_context_score(const S2tContextGraphDesc* graph, int R, const int* state, const int* token,
                      float* score, int* next, void* stream);
/* s2t_ctc_prefix_beam / s2t_ctc_prefix_beam_ngram with the bias term, still ONE launch and the plain
 * entry's workspace.  A live prefix also carries a graph state and bias_sum; the empty prefix starts in
 * the root with bias_sum 0.  An extension that does not land on a live prefix runs the look-up (after the
 * n-gram's, in the same thread), has bias_sum(p) + hit and, when kept, takes the `next` it returned; a
 * candidate that lands on a live prefix keeps that prefix' sum and state.  Candidates rank by
 *   (logaddexp(pb, pnb) + lm_weight * lm_sum) + bias_weight * bias_sum      (fp32, in this order; no LM: no
 * LM term).  FINALISATION: when an entry writes its outputs, the reported hypothesis is the live prefix
 * with the largest (logaddexp(pb, pnb) + lm_weight * lm_sum) + bias_weight * (bias_sum + ctx_final[state]),
 * ties to the lower beam position: an utterance that ends mid-phrase keeps nothing for the unfinished
 * part.  bias_score [B] is that prefix' bias_sum + ctx_final[state]; score and lm_score are that prefix'
 * own.  The finalisation touches the outputs only.  A zero-length utterance: no tokens, all scores 0.
 * With bias_weight = 0, and with a graph of no phrases at any weight, tokens, out_len, score and lm_score
 * are the plain / n-gram entry's bit for bit.
 * Refused (-1): what the partner entry refuses, the graph's limits above, graph.V != V, bias_weight not
 * finite, bias_score NULL. */
int s2t_ctc_prefix_beam_bias(const S2tContextGraphDesc* graph, const float* logits, const long* lengths,
                             int B, int T, int V, int blank, int beam_size, int cutoff_top_k,
                             float bias_weight, void* workspace, long* tokens, long* out_len, float* score,
                             float* bias_score, void* stream);
int s2t_ctc_prefix_beam_ngram_bias(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                   const float* logits, const long* lengths, int B, int T, int V, int blank,
                                   int beam_size, int cutoff_top_k, float lm_weight, int start_ctx,
                                   float bias_weight, void* workspace, long* tokens, long* out_len,
                                   float* score, float* lm_score, float* bias_score, void* stream);
/* The two entries above fed their frames in pieces: s2t_ctc_prefix_beam_chunk's /
 * s2t_ctc_prefix_beam_ngram_chunk's contract word for word, ONE launch per call, with the entries above as
 * the one-shot partners: for ANY cut, while overflow[b] == 0, a chunk call's outputs are the one-shot
 * entry's on the frames fed so far bit for bit, bias_score included (the finalisation enters no state:
 * the carried beam, its order, its states and the compaction are what they would be without it).
 * Overflow bit 0 is set when the reported prefix or the one at beam position 0 is longer than max_tokens.
 * state: the plain (s2t_ctc_stream_state_bytes) or n-gram (s2t_ctc_ngram_stream_state_bytes) layout
 * first, byte for byte, followed by
 *   bstate  [R] int32    the live prefixes' graph states, in beam order
 *   bsum    [R] fp32     their bias_sum
 * 256-byte aligned like every other array.  The resets are their partners'; a reset row starts in the
 * root with bias_sum 0.  The graph must not change between the chunks of a live stream. */
long s2t_ctc_bias_stream_state_bytes(int B, int V, int beam_size, int max_nodes);
int s2t_ctc_bias_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                              void* stream);
int s2t_ctc_prefix_beam_bias_chunk(const S2tContextGraphDesc* graph, const float* logits,
                                   const long* chunk_len, int B, int Tc, int V, int blank, int beam_size,
                                   int cutoff_top_k, float bias_weight, int max_tokens, int max_nodes,
                                   void* state, long* tokens, long* out_len, float* score, float* bias_score,
                                   long* stable_len, int* overflow, void* stream);
long s2t_ctc_ngram_bias_stream_state_bytes(int B, int V, int beam_size, int max_nodes);
int s2t_ctc_ngram_bias_stream_reset(void* state, const int* rows, int B, int V, int beam_size, int max_nodes,
                                    int start_ctx, void* stream);
int s2t_ctc_prefix_beam_ngram_bias_chunk(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                         const float* logits, const long* chunk_len, int B, int Tc, int V,
                                         int blank, int beam_size, int cutoff_top_k, float lm_weight,
                                         float bias_weight, int max_tokens, int max_nodes, void* state,
                                         long* tokens, long* out_len, float* score, float* lm_score,
                                         float* bias_score, long* stable_len, int* overflow, void* stream);

/* ---- Hotword biasing of the one-workgroup RNN-T beam search (csrc/decode_search.h beam_walk's bias mode;
 * csrc/decode_rnnt.hip).  s2t_rnnt_beam_stateless / s2t_rnnt_beam_stateless_ngram with the bias term of the
 * block above (its bias_sum, final_bias, tables and THE BIAS STATEMENT, not restated here), still ONE launch
 * and the partner's workspace (s2t_rnnt_beam_workspace_bytes / s2t_rnnt_beam_ngram_workspace_bytes).  A live
 * beam also carries a graph state and an unweighted bias_sum; the fresh beam starts in the root with 0.  The
 * candidate of class c != blank whose round is not empty takes (d, next) = bias(parent's state, c), looked up
 * by the thread that ran the n-gram's look-up, after it, and scores
 *   ((beam score + lp) + lm_weight * q) + bias_weight * d        (fp32, in this order; no LM: no LM term);
 * a kept beam takes next and bias_sum + d.  A blank candidate and an empty round run no look-up and keep the
 * parent's state and sum.  The cut to cutoff_top_k, the ranking, the records and the predictor are the
 * partner's; equal hypotheses are not merged, so no candidate lands on a live beam.
 * FINALISATION: when an entry writes its outputs it reports the live beam with the largest
 * score + bias_weight * ctx_final[state] (fp32), ties to the lower position.  score [B] is that value,
 * bias_score [B] that beam's bias_sum + ctx_final[state], lm_score [B] that beam's own lm_sum, tokens, frames
 * and out_len that beam's.  It touches the outputs only.  A zero-length utterance: no tokens, all scores 0.
 * With bias_weight = 0, and with a graph of no phrases at any weight, tokens, frames, out_len, score and
 * lm_score are the partner entry's bit for bit.
 * Refused (-1, before any launch and without following a device pointer): what the partner entry refuses, the
 * graph's limits above, graph.V != V, bias_weight not finite, bias_score NULL. */
int s2t_rnnt_beam_stateless_bias(const S2tContextGraphDesc* graph, const float* am, const long* lengths,
                                 const float* emb, const float* conv_w, const float* lin_w, const float* lin_b,
                                 const float* pre_w, const float* pre_b, int B, int T, int V, int E, int D,
                                 int ctx, int act, int blank, int beam_size, int cutoff_top_k, float bias_weight,
                                 void* workspace, long* tokens, long* frames, long* out_len, float* score,
                                 float* bias_score, void* stream);
int s2t_rnnt_beam_stateless_ngram_bias(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                       const float* am, const long* lengths, const float* emb,
                                       const float* conv_w, const float* lin_w, const float* lin_b,
                                       const float* pre_w, const float* pre_b, int B, int T, int V, int E, int D,
                                       int ctx, int act, int blank, int beam_size, int cutoff_top_k,
                                       float lm_weight, int start_ctx, float bias_weight, void* workspace,
                                       long* tokens, long* frames, long* out_len, float* score, float* lm_score,
                                       float* bias_score, void* stream);
/* The two entries above fed their frames in pieces: s2t_rnnt_beam_stateless_chunk's /
 * s2t_rnnt_beam_stateless_ngram_chunk's contract word for word, ONE launch per call.  Nothing of the
 * finalisation is stored: stable_len, overflow, the header, the histories and the carried beams with their order
 * are what the partner computes, so for ANY cut, while overflow[b] == 0, a chunk call's outputs are the
 * one-shot entry's on the frames fed so far bit for bit, bias_score included.
 * state: the plain (s2t_rnnt_stream_state_bytes) or n-gram (s2t_rnnt_ngram_stream_state_bytes) beam row
 * first, byte for byte, followed, 256-byte aligned, by bstate [beam_size] int32, the beams' graph states, and
 * bsum [beam_size] fp32, padded to a multiple of 256; size 0 for what the partner's query refuses and for
 * beam_size 0 (there is no greedy form).  The resets are their partners', -1 as well for beam_size 0; a reset
 * row starts in the root with bias_sum 0.  A chunk call clamps the graph states it loads into [0, num_ctx).
 * The graph must not change between the chunks of a live stream. */
long s2t_rnnt_bias_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens);
int s2t_rnnt_bias_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                               int max_tokens, int blank, void* stream);
int s2t_rnnt_beam_stateless_bias_chunk(const S2tContextGraphDesc* graph, const float* am, const long* chunk_len,
                                       const float* emb, const float* conv_w, const float* lin_w,
                                       const float* lin_b, const float* pre_w, const float* pre_b, int B, int Tc,
                                       int V, int E, int D, int ctx, int act, int blank, int beam_size,
                                       int cutoff_top_k, float bias_weight, int max_tokens, void* state,
                                       long* tokens, long* frames, long* out_len, float* score, float* bias_score,
                                       long* stable_len, int* overflow, void* stream);
long s2t_rnnt_ngram_bias_stream_state_bytes(int B, int V, int ctx, int beam_size, int max_tokens);
int s2t_rnnt_ngram_bias_stream_reset(void* state, const int* rows, int B, int V, int ctx, int beam_size,
                                     int max_tokens, int blank, int start_ctx, void* stream);
int s2t_rnnt_beam_stateless_ngram_bias_chunk(const S2tNgramLmDesc* lm, const S2tContextGraphDesc* graph,
                                             const float* am, const long* chunk_len, const float* emb,
                                             const float* conv_w, const float* lin_w, const float* lin_b,
                                             const float* pre_w, const float* pre_b, int B, int Tc, int V, int E,
                                             int D, int ctx, int act, int blank, int beam_size, int cutoff_top_k,
                                             float lm_weight, float bias_weight, int max_tokens, void* state,
                                             long* tokens, long* frames, long* out_len, float* score,
                                             float* lm_score, float* bias_score, long* stable_len, int* overflow,
                                             void* stream);

/* ---- chunk-carried (streaming) RNN-T search with the LSTM predictor: the two searches above fed
 * their frames in pieces (csrc/decode_lstm.hip).  A round's launches ARE the whole-utterance calls'
 * (one text, the same arguments), and a row's arithmetic does not depend on the rows that share its
 * launch, so for ANY cut of [0, L) into chunks -- one frame each, different per row, idle calls in
 * between -- tokens, frames, out_len and score after the last chunk are those of the whole-utterance
 * call on the concatenated am with lengths = L, bit for bit, and after every chunk those of the
 * prefix fed so far.  Descriptor and limits as above; Tc in 1..256; max_tokens >= 1.
 * state: ONE caller-owned device buffer of s2t_rnnt_lstm_stream_state_bytes(desc, B, beam_size,
 * max_tokens) bytes (beam_size 0 = the greedy state; a multiple of 256), whose size does not depend
 * on how many chunks or frames a stream sees.  It holds, for R = B * max(1, beam_size) rows, the
 * LSTM state [layers][R][H] (h and c), the lm vectors [R][V] and per utterance the frames seen since
 * the reset; greedy adds the count of symbols since the reset; beam adds score and length per beam,
 * the live-beam count, overflow, stable_len, and two alternating buffers [beam_size][max_tokens] of
 * token and frame histories (int32) with the index of the one in use.
 * workspace: s2t_rnnt_lstm_stream_workspace_bytes(desc, B, Tc, beam_size) bytes of scratch, 256-byte
 * aligned, which calls on one stream may share (one sized for Tc = 256 serves every call): the
 * per-round vectors, the candidates, the emit / token / parent rows and the counters, the (parent,
 * class) records [B][Tc][beam_size] of the current chunk only, and for beam the second of the two
 * alternating state copies.  The LIVE copy is always the state buffer's: frame 0 of a chunk reads
 * it, and after an odd Tc one launch copies the survivors home, so the launches of a call depend on
 * its arguments alone.  Both size functions are pure host functions and return 0 for a shape
 * outside the limits.
 * s2t_rnnt_lstm_stream_reset: makes every row b with rows[b] != 0 (rows NULL: every row) the empty
 * hypothesis by the launches the whole-utterance calls start with -- zero (h, c), one predictor step
 * on blank giving lm, one live beam of score 0, frame counter 0, overflow 0.  Other rows keep their
 * state bit for bit.  The caller's output arrays are not reset's to write.
 * A chunk call advances row b over the first min(chunk_len[b], Tc) frames of am [B][Tc][V].
 * chunk_len[b] <= 0 leaves row b's hypothesis AND the caller's outputs for it as they were; a
 * finished or idle row never reads am.  Outputs are the result for the whole stream since its reset:
 * s2t_rnnt_greedy_lstm_chunk: tokens [B][max_tokens] is appended to, so a stream must be given the
 *   same array on every call; out_len [B].  A symbol past max_tokens is dropped, out_len saturates
 *   and overflow[b] = 1 -- and the walk GOES ON (the predictor takes the dropped symbol, later
 *   frames are walked), as s2t_rnnt_greedy_lstm never ends a walk early either.  This differs from
 *   s2t_rnnt_greedy_stateless_chunk, whose full row is inert until reset.  host_poll = 0 enqueues
 *   all Tc (max_token_step + 2) rounds and never synchronises; host_poll = 1 enqueues blocks of 32
 *   rounds with one host read of the live counter each, as s2t_rnnt_greedy_lstm does.  Finished rows
 *   are inert, so both give the same bits.
 * s2t_rnnt_beam_lstm_chunk: the best beam's tokens and frames [B][max_tokens] (frames counted from
 *   the reset), out_len, score, stable_len (the longest common prefix of the live beams' token
 *   sequences; it never decreases) and overflow, as s2t_rnnt_beam_stateless_chunk: a beam past
 *   max_tokens keeps its first max_tokens tokens, scores and states stay exact.
 * s2t_rnnt_beam_lstm_chunk, the reset, and the greedy call with host_poll = 0 make no host
 * synchronisation and no cooperative launch, and leave nothing behind that depends on host memory:
 * they can be captured into a graph and replayed.
 * Return 0; -1 before any launch (outputs untouched) for Tc outside 1..256, state or workspace NULL,
 * max_tokens < 1, or what the whole-utterance call refuses; B <= 0 returns 0. */
long s2t_rnnt_lstm_stream_state_bytes(const S2tRnntLstmDesc* desc, int B, int beam_size,
                                      int max_tokens);
long s2t_rnnt_lstm_stream_workspace_bytes(const S2tRnntLstmDesc* desc, int B, int Tc, int beam_size);
int s2t_rnnt_lstm_stream_reset(const S2tRnntLstmDesc* desc, void* state, const int* rows, int B,
                               int beam_size, int max_tokens, void* workspace, void* stream);
int s2t_rnnt_greedy_lstm_chunk(const S2tRnntLstmDesc* desc, const float* am, const long* chunk_len,
                               int B, int Tc, int max_token_step, int max_tokens, int host_poll,
                               void* state, void* workspace, long* tokens, long* out_len,
                               int* overflow, void* stream);
int s2t_rnnt_beam_lstm_chunk(const S2tRnntLstmDesc* desc, const float* am, const long* chunk_len,
                             int B, int Tc, int beam_size, int cutoff_top_k, int max_tokens,
                             void* state, void* workspace, long* tokens, long* frames,
                             long* out_len, float* score, long* stable_len, int* overflow,
                             void* stream);

/* ---- chunk-carried (streaming) RNN-T beam search with RNN-LM shallow fusion: s2t_rnnt_beam_lstm_lm and
 * s2t_rnnt_beam_stateless_lm fed their frames in pieces (csrc/decode_lstm.hip).  The contract of the block
 * above, word for word, extended by the LM: a round's launches ARE the fused whole-utterance calls'
 * (chunk_len where those take lengths, Tc where they take T, the carried buffers where they take their
 * workspace's), so for ANY cut of [0, L) into chunks tokens, frames, out_len, score and lm_score after
 * the last chunk are those of the fused call on the concatenated am with lengths = L, bit for bit, and
 * after every chunk those of the prefix fed so far.  lm_score [B]: the best beam's unweighted lm_sum.
 * Beam only (the greedy searches take no LM); lm is required.  The stateless family takes inner == 0
 * and inner > 0: it is the only chunk-carried search of the out-projection joiner with that predictor.
 * state: ONE caller-owned buffer of *_lm_stream_state_bytes(desc, lm, B, beam_size, max_tokens) bytes (a
 * multiple of 256, independent of the chunks or frames seen), every array 256-byte aligned.  LSTM
 * family: the state of s2t_rnnt_lstm_stream_state_bytes (same layout), then the LM's h, c
 * [lm.layers][R][lm.H], q [R][V] and lm_sum [R], R = B * beam_size.  Stateless family: ctx [R][ctx]
 * (int32) and lm [R][V] in place of the LSTM (h, c, lm), the same per-utterance and per-beam records,
 * then the same LM arrays.  lm_sum is updated in place by the rounds' select launch.
 * workspace: *_lm_stream_workspace_bytes(desc, lm, B, Tc, beam_size) bytes of scratch (one sized for Tc =
 * 256 serves every call and the reset), holding the second copy of the predictor's and the LM's
 * state.  The LIVE copy is always the state buffer's: frame 0 of a chunk reads it, and after an odd Tc
 * ONE launch copies every survivor home (predictor state and lm rows, the LM's h, c, q, the stateless
 * ctx), so the launches of a call depend on its arguments alone.
 * *_lm_stream_reset: for every row b with rows[b] != 0 (rows NULL: every row): zero predictor state (LSTM
 * (h, c); ctx blanks), zero LM (h, c), q = 0, lm_sum = 0, one live beam of score 0, frame counter 0,
 * overflow 0, then the fused call's own first predictor step on blank and, with lm_start_token >= 0, its
 * own first LM step on that token, both masked by rows.  Other rows keep every bit, LM state included.
 * The caller's output arrays are not reset's to write.  The same lm_start_token convention as
 * s2t_rnnt_beam_lstm_lm (< 0: none).
 * *_lm_chunk: outputs as s2t_rnnt_beam_lstm_chunk plus lm_score.  chunk_len[b] <= 0 leaves row b's
 * hypothesis, its LM state and the caller's outputs for it as they were; a finished or idle row never
 * reads am.  Past max_tokens a beam keeps its first max_tokens tokens and overflow[b] = 1; score,
 * lm_score and all states stay exact.  With lm_weight = 0 the LSTM family's tokens, frames, out_len,
 * score, stable_len and overflow are s2t_rnnt_beam_lstm_chunk's bit for bit.
 * No host synchronisation, no cooperative launch, no memset, nothing left behind that depends on host
 * memory: reset and chunk call can be captured into a graph and replayed.
 * Return 0; -1 before any launch (outputs untouched, no pointer followed) for Tc outside 1..256, state,
 * workspace or lm NULL, max_tokens < 1, lm_start_token >= V, lm_weight not finite, lm.V != desc.V, or
 * what the fused whole-utterance call refuses; B <= 0 returns 0.  The size functions are pure host
 * functions and return 0 outside the limits. */
long s2t_rnnt_lstm_lm_stream_state_bytes(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int B,
                                         int beam_size, int max_tokens);
long s2t_rnnt_lstm_lm_stream_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int B,
                                             int Tc, int beam_size);
int s2t_rnnt_lstm_lm_stream_reset(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, int lm_start_token,
                                  void* state, const int* rows, int B, int beam_size, int max_tokens,
                                  void* workspace, void* stream);
int s2t_rnnt_beam_lstm_lm_chunk(const S2tRnntLstmDesc* desc, const S2tRnnLmDesc* lm, const float* am,
                                const long* chunk_len, int B, int Tc, int beam_size, int cutoff_top_k,
                                float lm_weight, int max_tokens, void* state, void* workspace,
                                long* tokens, long* frames, long* out_len, float* score, float* lm_score,
                                long* stable_len, int* overflow, void* stream);
long s2t_rnnt_stateless_lm_stream_state_bytes(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm,
                                              int B, int beam_size, int max_tokens);
long s2t_rnnt_stateless_lm_stream_workspace_bytes(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm,
                                                  int B, int Tc, int beam_size);
int s2t_rnnt_stateless_lm_stream_reset(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm,
                                       int lm_start_token, void* state, const int* rows, int B,
                                       int beam_size, int max_tokens, void* workspace, void* stream);
int s2t_rnnt_beam_stateless_lm_chunk(const S2tRnntStatelessDesc* desc, const S2tRnnLmDesc* lm,
                                     const float* am, const long* chunk_len, int B, int Tc, int beam_size,
                                     int cutoff_top_k, float lm_weight, int max_tokens, void* state,
                                     void* workspace, long* tokens, long* frames, long* out_len,
                                     float* score, float* lm_score, long* stable_len, int* overflow,
                                     void* stream);

/* ---- The back-off n-gram (S2tNgramLmDesc, THE SCORING STATEMENT above) fused into the lockstep RNN-T beam
 * search of the LSTM predictor, whole and chunk-carried (csrc/decode_lstm.hip): the siblings of the RNN-LM
 * family (s2t_rnnt_beam_lstm_lm*, s2t_rnnt_lstm_lm_stream_*), with the n-gram's descriptor where those take
 * the RNN LM's and start_ctx where those take lm_start_token.
 * STATEMENT.  s2t_rnnt_beam_lstm's statement with the LM term of s2t_rnnt_beam_stateless_ngram: a live row
 * also carries a context id and lm_sum; the cutoff_top_k classes of a row are chosen on the logits, as there
 * (the LM does not enter the cut); the candidate of class c != blank of a row in context n takes (q, next) =
 * score(n, c), scores (row score + lp) + lm_weight * q in fp32, in this order (an fp32 multiply, then an
 * fp32 add, not contracted), sums lm_sum + q, and a kept row takes next; a blank candidate makes no
 * look-up and keeps its parent's context and lm_sum.  The empty hypothesis starts in start_ctx, so the
 * first token is scored too; there is no end-of-sentence term.  lm_score [B] = the best beam's lm_sum; a
 * zero-length utterance gives no tokens, score 0 and lm_score 0.  With lm_weight = 0 tokens, frames, out_len
 * and score are s2t_rnnt_beam_lstm's bit for bit.
 * LAUNCHES.  A round stays expand, select, predictor step: the look-ups of a row's K candidates run on K
 * threads of the expand launch after its top-k loop, select hands the kept rows their contexts and sums in
 * place; no LM step is launched, and the two-buffer alternation and the copy home after an odd Tc concern
 * the predictor's state only.  No host synchronisation; reset and chunk call can be captured in a graph.
 * workspace: the plain search's (s2t_rnnt_lstm_workspace_bytes / s2t_rnnt_lstm_stream_workspace_bytes),
 * then the candidates' q and next contexts [B][256] and, for the whole-utterance call, ctx and lm_sum [R].
 * state (chunk-carried): the state of s2t_rnnt_lstm_stream_state_bytes (same layout), then ctx [R] int32,
 * the rows' context ids, and lm_sum [R] fp32, R = B * beam_size, each 256-byte aligned.
 * s2t_rnnt_lstm_ngram_stream_reset: s2t_rnnt_lstm_stream_reset, and every beam of a reset row starts in
 * start_ctx with lm_sum 0; other rows keep every bit.  Reset follows no table: the chunk call clamps every
 * context id it loads into [0, num_ctx).
 * s2t_rnnt_beam_lstm_ngram_chunk: s2t_rnnt_beam_lstm_lm_chunk's contract word for word (idle rows keep
 * state and outputs, stable_len, the max_tokens saturation and overflow, Tc in 1..256, reset of chosen rows
 * only): for ANY cut, tokens, frames, out_len, score and lm_score after a chunk are
 * s2t_rnnt_beam_lstm_ngram's on the frames fed so far, bit for bit.
 * Refused (-1 / size 0, before any launch and without following a device pointer): what the RNN-LM siblings
 * refuse, with the n-gram descriptor's limits in place of the RNN LM's: lm NULL or outside its limits,
 * lm.V != desc.V, start_ctx outside [0, num_ctx) (reset: < 0), lm_weight not finite, lm_score NULL. */
long s2t_rnnt_beam_lstm_ngram_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int B,
                                              int T, int beam_size);
int s2t_rnnt_beam_lstm_ngram(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, const float* am,
                             const long* lengths, int B, int T, int beam_size, int cutoff_top_k,
                             float lm_weight, int start_ctx, void* workspace, long* tokens, long* frames,
                             long* out_len, float* score, float* lm_score, void* stream);
long s2t_rnnt_lstm_ngram_stream_state_bytes(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int B,
                                            int beam_size, int max_tokens);
long s2t_rnnt_lstm_ngram_stream_workspace_bytes(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int B,
                                                int Tc, int beam_size);
int s2t_rnnt_lstm_ngram_stream_reset(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, int start_ctx,
                                     void* state, const int* rows, int B, int beam_size, int max_tokens,
                                     void* workspace, void* stream);
int s2t_rnnt_beam_lstm_ngram_chunk(const S2tRnntLstmDesc* desc, const S2tNgramLmDesc* lm, const float* am,
                                   const long* chunk_len, int B, int Tc, int beam_size, int cutoff_top_k,
                                   float lm_weight, int max_tokens, void* state, void* workspace,
                                   long* tokens, long* frames, long* out_len, float* score, float* lm_score,
                                   long* stable_len, int* overflow, void* stream);

/* ---- batched on-device augmentation + collate next to the fbank kernel
 * (dataset/frontend/data_augmentation.py:13-56 AddNoise, :59-118 MixFeats, :150-196 SpecAugment;
 * dataset/utils.py:182-202 batch()).  Random decisions are made on the host as the reference
 * does; each op is one launch over the padded batch.
 * s2t_row_energy: out[b] = sum over the len[b]*D valid elements of exp(x) (mode 0) or x^2 (mode 1).
 * s2t_mix: mode 0 MixFeats on log-mel (T,D) rows, mode 1 AddNoise on PCM (D = 1); the noise is
 *   indexed (start[b] + t) mod nlen[b] (= the reference's repeat + slice).
 * s2t_specaug: zero the nt time spans and nf frequency spans (start, end) of each utterance.
 * s2t_pad_rows: packed rows + element offsets [B+1] -> zero-padded (B, Lmax, D). */
int s2t_row_energy(const float* x, long stride, const long* len, int B, int D, int mode, float* out,
                   void* stream);
int s2t_mix(const float* src, long sstride, const long* slen, const float* noise, long nstride,
            const long* nlen, const long* start, const float* snr, const float* src_e,
            const float* noise_e, int B, long rows_max, int D, int mode, float max_gain_db,
            float* out, void* stream);
int s2t_specaug(float* feats, int B, int T, int F, const int* tspan, int nt, const int* fspan,
                int nf, void* stream);
int s2t_pad_rows(const float* packed, const long* offsets, int B, long Lmax, int D, float* out,
                 void* stream);

/* ---- plain dense GEMMs of the Linear layers through hipBLASLt's C API (csrc/gemm_lib.hip), with
 * bias and residual / accumulation in the epilogue (model/encoder/zipformer.py:1095-1221
 * `src = src + module(src)`, and the data gradients under loss.backward()).
 * mode 0: D[M,N] = X[M,K] W[N,K]^T (+ bias[N]) (+ beta C[M,N]);  mode 1: D[M,K] = X[M,N] W[N,K] (+ beta C).
 * Row-major, leading dimensions in floats; C may be NULL (beta ignored) or alias D.  Returns -2 when
 * the library offers no algorithm for the shape (the caller then uses torch.matmul). */
int s2t_linear_lt(int mode, const float* X, long ldx, const float* W, long ldw, const float* bias,
                  const float* C, long ldc, float beta, float* D, long ldd, int M, int N, int K,
                  void* workspace, long ws_bytes, void* stream);
/* plans made (one per exact shape, table capped) and buckets {mode, half-octave of M, N, K,
 * bias} whose candidates were timed (capped at 192) so far. */
int s2t_linear_lt_stats(int* plans, int* timed);
/* s2t_linear_lt times OUR NT / NN kernel (s2t_gemm_f32, bf16x3 form, bias + residual epilogue) as one
 * more candidate of a bucket and keeps it where it beats the library's best by > 8 % twice;
 * launches it has served so far: */
long s2t_linear_lt_own_calls(void);

/* ---- fused glue of the zipformer layer (csrc/zip_glue.hip), rows of C channels, time-major.
 * bypass (model/encoder/zipformer.py:1523-1555): out = orig + (src - orig) * scale[c]; backward
 * writes d_orig, d_src and ACCUMULATES d_scale[c] (caller zeroes it).
 * nonlinear attention (zipformer.py:2438-2483): u (T,B,3C) = in_proj(x) = [s | x | y];
 * gate_fwd: xs (B,T,C) = x * tanh(s) (batch-major for the head-0 weights @ x bmm);
 * out_fwd: o (T,B,C) = z (B,T,C) * y;  out_bwd: dz (B,T,C) = g * y, du[..,2C:3C] = g * z;
 * gate_bwd: du[..,0:C] = dxs * x * (1 - tanh(s)^2), du[..,C:2C] = dxs * tanh(s). */
int s2t_bypass_fwd(const float* orig, const float* src, const float* scale, long rows, int C,
                   float* out, void* stream);
int s2t_bypass_bwd(const float* orig, const float* src, const float* scale, const float* g,
                   long rows, int C, float* d_orig, float* d_src, float* d_scale, void* stream);
/* layer-executor helpers (speech2text_amd/zip_layer.py): bypass backward whose d_orig also takes
 * the gradient already collected for orig (acc_in); grad += d with limit_param_value's sign flip
 * (model/layer/scaling.py:1153-1190) applied to d when `limit`; the softmax-backward row constants
 * delta[h,b,i] of the attention weights from its deferred consumers (pairs (dO,O) of the two
 * SelfAttention modules, dW0 (B,T,T) of the head-0 consumer), one launch. */
int s2t_bypass_bwd_acc(const float* orig, const float* src, const float* scale, const float* g,
                       const float* acc_in, long rows, int C, float* d_orig, float* d_src,
                       float* d_scale, void* stream);
int s2t_attn_delta_pairs(const float* W, const float* dW0, const float* dO1, const float* O1,
                         int dv1, const float* dO2, const float* O2, int dv2, int T, int B, int H,
                         float* delta, void* stream);
/* bypass with the stack's per-utterance feature mask (zipformer.py:1095-1113, `output * feature_mask`
 * after every layer) folded in: out = (orig + (src - orig) * scale[c]) * fm[b, c], rows ordered
 * (t, b); the backward multiplies the incoming gradient by fm on the fly. */
int s2t_bypass_fwd_mask(const float* orig, const float* src, const float* scale, const float* fm,
                        int B, long rows, int C, float* out, void* stream);
int s2t_bypass_bwd_mask(const float* orig, const float* src, const float* scale, const float* g,
                        const float* fm, int B, long rows, int C, float* d_orig, float* d_src,
                        float* d_scale, void* stream);
/* SimpleDownsample (zipformer.py:1653-1695): out (ceil(T/ds),B,C) = sum_k w[k] src[min(tt*ds+k, T-1)]
 * with w = softmax(bias) supplied by the caller (ds <= 8); the backward writes d_src (T,B,C) and
 * ACCUMULATES dw[ds] (caller zeroes it; the softmax backward stays with the caller).
 * SimpleUpsample + the out_combiner BypassModule of a downsampled stack (zipformer.py:1253-1283,
 * 1698-1719): out[t] = orig[t] + (src[t / up] - orig[t]) * scale[c] with src (ceil(T/up),B,C) --
 * the upsampled tensor is never materialised; the backward writes d_orig, d_src and ACCUMULATES
 * d_scale[C] (caller zeroes it). */
int s2t_downsample_fwd(const float* src, const float* w, int ds, int T, int B, int C, float* out,
                       void* stream);
int s2t_downsample_bwd(const float* src, const float* w, const float* g, int ds, int T, int B, int C,
                       float* d_src, float* dw, void* stream);
/* the same pair with the OUTPUT (and its gradient g) batch-major, (B, ceil(T/ds), C): the encoder's
 * final x.transpose(0, 1) (model/encoder/zipformer.py:199) rides in the pass that writes / reads it. */
int s2t_downsample_fwd_bt(const float* src, const float* w, int ds, int T, int B, int C, float* out,
                          void* stream);
int s2t_downsample_bwd_bt(const float* src, const float* w, const float* g, int ds, int T, int B, int C,
                          float* d_src, float* dw, void* stream);
int s2t_bypass_up_fwd(const float* orig, const float* src, const float* scale, int up, int T, int B,
                      int C, float* out, void* stream);
int s2t_bypass_up_bwd(const float* orig, const float* src, const float* scale, const float* g, int up,
                      int T, int B, int C, float* d_orig, float* d_src, float* d_scale, void* stream);
/* Up to 8 small parameters in one launch: grad[e] += d[e] (limit_param_value's sign flip,
 * scaling.py:1153-1190, applied to d first where `limit`), then d[e] = 0 -- the accumulators the
 * layer's backward kernels add into are handed back clean.  `items` is a HOST array. */
typedef struct S2tCommit {
  const float* x;
  float* d;
  float* grad;
  float lo, hi;
  int limit;
  long n;
} S2tCommit;
int s2t_param_grad_commit_n(int n, const S2tCommit* items, void* stream);
int s2t_nonlin_gate_fwd(const float* u, int T, int B, int C, float* xs, void* stream);
int s2t_nonlin_out_fwd(const float* z, const float* u, int T, int B, int C, float* o, void* stream);
int s2t_nonlin_out_bwd(const float* g, const float* z, const float* u, int T, int B, int C, float* dz,
                       float* du, void* stream);
int s2t_nonlin_gate_bwd(const float* dxs, const float* u, int T, int B, int C, float* du,
                        void* stream);

/* ---- conformer block (torchaudio.models.Conformer as called at model/encoder/conformer.py:
 * 170-178,193; block structure in csrc/conf_elem.hip).  All (rows, C) tensors row-major fp32,
 * rows ordered (t, b), C % 4 == 0, C <= 1024, 16-byte aligned.
 * s2t_layernorm_fwd: nn.LayerNorm.  y != NULL: the input is x + alpha * y (the layer's residual
 * sums "0.5 * ffn(x) + x" / "x + module(x)"), written to xsum as well.  stats [rows][2] = (mean,
 * rstd) for the backward.
 * s2t_layernorm_bwd: dx = LayerNorm'(dy) (+ resid, the residual branch's gradient); the
 * per-workgroup sums of d gamma / d beta go to `partial` (s2t_layernorm_bwd_partial_floats(rows, C)
 * floats).  s2t_layernorm_param_grad folds the partials of n LayerNorms of width C in one launch:
 * dgamma[C] += ..., dbeta[C] += ... (the parameters' views of the flat gradient buffer); `items`
 * is a HOST array. */
int s2t_layernorm_fwd(const float* x, const float* y, float alpha, const float* gamma,
                      const float* beta, long rows, int C, float eps, float* xsum, float* out,
                      float* stats, void* stream);
typedef struct S2tLnFold {
  const float* partial;
  long rows;
  float* dgamma;
  float* dbeta;
} S2tLnFold;
long s2t_layernorm_bwd_partial_floats(long rows, int C);
int s2t_layernorm_bwd(const float* x, const float* stats, const float* gamma, const float* dy,
                      const float* resid, long rows, int C, float* dx, float* partial,
                      void* stream);
int s2t_layernorm_param_grad(int n, const S2tLnFold* items, int C, void* stream);
/* nn.SiLU of the feed-forward modules: a = h * sigmoid(h); dh = scale * da * silu'(h) (dh may
 * alias da; scale carries the layer's 0.5 feed-forward residual weight). */
int s2t_silu_fwd(const float* h, long n, float* a, void* stream);
int s2t_silu_bwd(const float* h, const float* da, long n, float scale, float* dh, void* stream);
/* nn.Dropout sites of the conformer block (torchaudio.models.Conformer: after the feed-forward
 * SiLU, after each module's last Linear / pointwise conv, model/encoder/conformer.py:170-178).  The
 * keep decision of element i is a stateless hash of (seed, i) -- the one s2t_mhsa_* uses for the
 * attention probabilities -- so backward regenerates the forward's mask; kept values are scaled by
 * 1 / (1 - p).  s2t_dropout_add: out = x + alpha * drop(y) (x may be NULL: the masked gradient);
 * s2t_silu_drop_fwd: a = drop(silu(h)); s2t_silu_drop_bwd: dh = scale * da * mask * silu'(h). */
int s2t_dropout_add(const float* x, const float* y, long n, float alpha, float p,
                    unsigned long long seed, float* out, void* stream);
int s2t_silu_drop_fwd(const float* h, long n, float p, unsigned long long seed, float* a,
                      void* stream);
int s2t_silu_drop_bwd(const float* h, const float* da, long n, float scale, float p,
                      unsigned long long seed, float* dh, void* stream);
/* nn.BatchNorm1d (training mode: statistics over all rows, biased variance for the normalisation,
 * running_mean / running_var (unbiased) / num_batches_tracked updated; running_* may be NULL)
 * followed by nn.SiLU, conv module of the conformer block.  save_mean / save_rstd [C] feed the
 * backward, which ACCUMULATES dgamma / dbeta.  workspace: s2t_bn_workspace_floats(C) floats. */
#define S2T_BN_PARTIALS 128
long s2t_bn_workspace_floats(int C);
int s2t_bn_silu_fwd(const float* x, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, long* num_batches,
                    long rows, int C, float* y, float* save_mean, float* save_rstd,
                    float* workspace, void* stream);
/* evaluation mode (running statistics): y = silu((x - mean) * rstd * gamma + beta) */
int s2t_bn_silu_apply(const float* x, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, long rows, int C, float* y, void* stream);
int s2t_bn_silu_bwd(const float* x, const float* ds, const float* save_mean,
                    const float* save_rstd, const float* gamma, const float* beta, long rows, int C,
                    float* dx, float* dgamma, float* dbeta, float* workspace, void* stream);
/* nn.MultiheadAttention core (no positional term): o = softmax(q k^T * scale, keys >= lens[b]
 * masked) v per (b, head).  q / k / v are the column blocks [qoff | koff | voff] + h * dh of the
 * in-projection output qkv (T*B rows (t, b), row stride ld); o (T*B, ldo) column h * dh;
 * lse [B][H][T] row log-sum-exp kept for the backward.  dh in {16, 32, 64}.
 * dropout_p > 0: dropout on the attention probabilities (nn.MultiheadAttention(dropout=p),
 * training); the mask is a hash of (seed, b, h, q, k) that the backward regenerates from the
 * same seed -- it is never stored.
 * s2t_mhsa_bwd: dqkv (same layout as qkv) from d_o; delta [B][H][T] is scratch. */
int s2t_mhsa_fwd(const float* qkv, long ld, int qoff, int koff, int voff, const long* lens, int T,
                 int B, int H, int dh, float scale, float dropout_p, unsigned long seed, float* o,
                 long ldo, float* lse, void* stream);
int s2t_mhsa_bwd(const float* qkv, long ld, int qoff, int koff, int voff, const long* lens, int T,
                 int B, int H, int dh, float scale, float dropout_p, unsigned long seed,
                 const float* o, const float* d_o, long ldo, const float* lse, float* delta,
                 float* dqkv, void* stream);

/* ---- first convolution of the conformer Subsampling (model/encoder/conformer.py:47-60,114-126):
 * Conv2d(1, C, 3, stride 2) + ReLU on x (B, T, F) -> out (B, T1, F1, C) channel-last, T1 =
 * (T-3)/2+1, F1 = (F-3)/2+1; w (C, 9), bias (C).  s2t_conv1_relu_wgrad: dw (C, 9) and db (C) are
 * ACCUMULATED from d_out (gradient w.r.t. out, same layout); the ReLU mask is recomputed from x.
 * C % 4 == 0, 256 % (C/4) == 0.  workspace: s2t_conv1_relu_workspace_floats(C) floats. */
long s2t_conv1_relu_workspace_floats(int C);
int s2t_conv1_relu_fwd(const float* x, const float* w, const float* bias, int B, int T, int F,
                       int C, float* out, void* stream);
int s2t_conv1_relu_wgrad(const float* x, const float* w, const float* bias, const float* d_out,
                         int B, int T, int F, int C, float* dw, float* db, float* workspace,
                         void* stream);

/* ---- Adam / AdamW on the flat parameter / gradient buffers (torch.optim.Adam / AdamW, amsgrad
 * off: the conformer YAMLs' `optimizer: type: "AdamW"`, optimizer/optim_setup.py:364-385) with the
 * trainer's grad-norm clip and zero_grad folded in: s2t_seg_stats -> s2t_clip_coef (out[0] =
 * min(1, clip / (||g|| + 1e-6)), out[1] = ||g||; clip <= 0: 1) -> s2t_adam_apply.  Chunk tables as
 * for ScaledAdam; group q owns the chunks below groups[q].chunk_hi that no earlier group owns;
 * chunks past the last group are only zeroed.  `groups` is a HOST array. */
#define S2T_ADAM_MAX_GROUPS 8
typedef struct S2tAdamGroup {
  int chunk_hi;
  float lr, beta1, beta2, eps, weight_decay;
  float bias_correction1;         /* 1 - beta1^step */
  float sqrt_bias_correction2;    /* sqrt(1 - beta2^step) */
  int decoupled;                  /* 1: AdamW, 0: Adam (L2 added to the gradient) */
} S2tAdamGroup;
int s2t_clip_coef(const float* partial, int nchunks, float clip_val, float* out, void* stream);
int s2t_adam_apply(float* p, float* g, float* exp_avg, float* exp_avg_sq, const int* chunk_off,
                   const int* chunk_len, int nchunks, int ngroups, const S2tAdamGroup* groups,
                   const float* coef, int zero_grad, const float* skip, void* stream);

/* ---- layer-norm LSTM layer of the RNN-T predictor (model/predictor/lstm_predictor.py:28-109 ->
 * torchaudio 0.13.1 _Predictor / _CustomLSTM), whole sequence per launch, one workgroup per
 * utterance (csrc/lstm.hip).  gx (T,B,4H) = x2g(x); wp_t = p2g.weight transposed (H,4H) for the
 * forward, wp = p2g.weight (4H,H) for the backward; g_* / c_* = g_norm / c_norm weight and bias
 * (all four NULL: no layer norm); h0 / c0 (B,H) or NULL = zeros.  The forward writes hs (T,B,H),
 * the final state hT / cT (B,H) and keeps ghat (T,B,4H), chat (T,B,H), rstd (T,B,2) for the
 * backward, which writes dgx (T,B,4H) (gradient w.r.t. the raw gates: the weight gradients of
 * x2g / p2g are TN GEMMs over its rows) and ACCUMULATES the four LayerNorm parameter gradients.
 * H <= 1024. */
int s2t_lnlstm_fwd(const float* gx, const float* wp_t, const float* g_gamma, const float* g_beta,
                   const float* c_gamma, const float* c_beta, const float* h0, const float* c0,
                   int T, int B, int H, float eps, float* hs, float* ghat, float* chat,
                   float* rstd, float* hT, float* cT, void* stream);
int s2t_lnlstm_bwd(const float* wp, const float* g_gamma, const float* g_beta,
                   const float* c_gamma, const float* c_beta, const float* c0, int T, int B, int H,
                   const float* ghat, const float* chat, const float* rstd, const float* dhs,
                   float* dgx, float* d_g_gamma, float* d_g_beta, float* d_c_gamma,
                   float* d_c_beta, void* stream);

/* ---- LSTM layer of the RNN language model (reference model/lm/rnn_lm.py:40-45: torch.nn.LSTM, gate
 * order i, f, g, o, no layer norm), ONE LAUNCH PER TIME STEP, ordered by the stream alone
 * (csrc/lstm_step.hip): a workgroup owns 16 hidden units and 16 utterances, so the recurrent matrix
 * is read once per step and batch tile, not once per utterance.  gx (T,B,4H) = x W_ih^T + b_ih +
 * b_hh; whh = weight_hh (4H,H) for the forward, whh_t = its transpose (H,4H) for the backward;
 * h0 / c0 (B,H) or NULL = zeros.  The forward writes hs (T,B,H), the final state hT / cT (B,H) and
 * keeps the ACTIVATED gates (T,B,4H) and the cells (T,B,H); the backward takes dhs (T,B,H) and
 * writes dgx (T,B,4H), the gradient w.r.t. the raw gates (weight gradients: TN GEMMs over its
 * rows; bias gradients: its column sums); dc_ws (B,H) is scratch for the carried cell gradient.
 * H % 4 == 0, H <= 1024 (else -2); all pointers 16-byte aligned. */
int s2t_lstm_seq_fwd(const float* gx, const float* whh, const float* h0, const float* c0, int T,
                     int B, int H, float* hs, float* gates, float* cells, float* hT, float* cT,
                     void* stream);
int s2t_lstm_seq_bwd(const float* whh_t, const float* c0, int T, int B, int H, const float* gates,
                     const float* cells, const float* dhs, float* dgx, float* dc_ws, void* stream);

/* ---- StatelessPredictor: embedding + depthwise context convolution in one pass
 * (reference model/predictor/stateless_predictor.py:27-105: nn.Embedding -> nn.Conv1d(D, D, K,
 * groups=D, bias=False) on the blank-left-padded labels).  tokens (B,L) int32 (values clamped to
 * [0,V)), emb (V,D), w (D,K) = the conv weight (D,1,K), K <= 8:
 *   out[b,u,d] = sum_k w[d,k] emb[tokens[b,u+k], d],  out (B, L-K+1, D).
 * bwd: g (B, L-K+1, D); d_emb (V,D) and d_w (D,K) are ADDED to (fp32 atomics; the caller
 * zeroes them); either may be NULL. */
int s2t_predictor_ctx_fwd(const int* tokens, const float* emb, const float* w, int B, int L, int K,
                          int D, int V, float* out, void* stream);
int s2t_predictor_ctx_bwd(const int* tokens, const float* emb, const float* w, const float* g, int B,
                          int L, int K, int D, int V, float* d_emb, float* d_w, void* stream);

/* ---- fp32 GEMM on the bf16 matrix cores with the weight operand split ahead of time
 * (csrc/gemm_x3p.hip): the forward (y = x W^T + b) and data-gradient (dx = g W) products of the
 * layers' Linears (reference model/encoder/zipformer.py:1924-1975,2372-2378,2643-2695,
 * model/layer/scaling.py:1512-1583).  The three bf16 pieces of a logical matrix Bm[n][k]
 * (= src[n*ld + k], or src[k*ld + n] when transposed) are stored fragment-major
 * [ceil(N/32)][2 ceil(K/32)][3][64 lanes][8], zero-padded: s2t_x3p_plane_elems(N,K) bf16.
 * s2t_x3p_split: every matrix of a model in ONE launch -- tab = DEVICE array of n S2tPlaneDesc
 *   (src_off: floats from base; dst_off: bf16 from dst; blk_begin: first block of the descriptor,
 *   ascending, descriptor d owns s2t_x3p_split_blocks(N,K) blocks), total_blocks = their sum.
 * s2t_gemm_x3p: C[M,N] = A[M,K] . Bm^T (+ bias[N]) (* act'(act_src[M,N])) (+ resid[M,N])
 *   (+ resid_b[M,N]) and optionally C2 = act2(C); act kinds 1 = SwooshL, 2 = SwooshR; act2 = 3:
 *   C2 = C + resid_b instead (C itself without resid_b: a module's output and the residual
 *   stream after it from one launch).  K % 8 == 0, N % 4 == 0, rows
 *   16-byte aligned (else -2).  tile = 0 (from the shape) | 11 | 12 | 21 | 22: block tile
 *   (64 tm) x (64 tn); + 100 w: w persistent workgroups per CU;
 *   2000 + tm tn: the form that moves the weight pieces global -> LDS directly, + 200 (two-piece
 *   arithmetic only): 32-deep barrier intervals.  Any other code: -1.  -2: a tile code the current
 *   arithmetic has not. */
/* ---- the arithmetic of every bf16 matrix-core GEMM of the library (s2t_gemm_x3p*, the weight-gradient /
 * NT / NN / batched kernels of csrc/gemm.hip): pieces per fp32 operand.
 *   3 ("bf16x3/6"): x = p0 + p1 + p2 exactly, six piece products per term: fp32-level error
 *       (<= 2e-6 of the result's max against fp64);
 *   2 ("bf16x2/3"): x ~ p0 + p1 (2^-18 relative), the products a0 b0 + a0 b1 + a1 b0: ~ 2^-17 per
 *       term -- torch's float32 matmul precision "high"; the reference trains under the looser
 *       "medium" (reference build_task.py:79, inference.py:58).
 * The arithmetic is a POLICY over four classes of product -- 0 F forward (y = x W^T, conv forward,
 * W0 @ x), 1 D data gradient (dx = g W and the batched products of backward), 2 W weight gradient
 * (dW += g^T x: every TN launch), 3 S statistics (Whiten's x^T x and its penalty product x dcov) --
 * consulted PER CALL: s2t_gemm_arith_set's value (2 | 3) for every class if one is pinned (0 =
 * unpinned); else the environment's S2T_GEMM_ARITH_F / _D / _W / _S for that class, else
 * S2T_GEMM_ARITH for all ("2" | "3" | "bf16x2" | "bf16x3" | "bf16x2/3" | "bf16x3/6"), else the
 * built-in default of the class.  s2t_gemm_arith_of(cls) = that value (cls outside 0..3: the base
 * value).  Entry points whose class is implied take it (TN launches: W; s2t_gemm_xtx: S; the 3x3
 * conv forward: F); s2t_gemm_x3p*, s2t_gemm_f32 (NT / NN) and s2t_gemm_f32_batched run in the class
 * the calling THREAD declared last with s2t_gemm_class_set(cls) (returns the previous one; -1 = none:
 * the base value) -- s2t_gemm_arith() is that class's value.  The weights' piece image (s2t_x3p_split)
 * is the same for both arithmetics: two-piece launches read its first two pieces. */
int s2t_gemm_arith(void);
int s2t_gemm_arith_of(int cls);
int s2t_gemm_class_set(int cls);
int s2t_gemm_arith_set(int arith);
typedef struct {
  long src_off;
  long dst_off;
  int N, K, ld, transposed;
  unsigned blk_begin;
  int pad_;
} S2tPlaneDesc;
long s2t_x3p_plane_elems(int N, int K);
long s2t_x3p_split_blocks(int N, int K);
int s2t_x3p_split(const float* base, const void* tab, int n, int total_blocks, unsigned short* dst,
                  void* stream);
int s2t_gemm_x3p(const float* A, long lda, const unsigned short* Bp, int N, int K, float* C, long ldc,
                 int M, const float* bias, const float* resid, long ldr, const float* act_src,
                 long ld_act, int act_kind, float* C2, long ldc2, int act2, const float* resid_b,
                 long ldrb, int tile, void* stream);
/* s2t_gemm_x3p for a data gradient through an activation with the Balancer on the activation's input
 * in the epilogue (the hidden Balancer of FeedforwardModule / ConvolutionModule / ConvNeXt,
 * model/encoder/zipformer.py:2372-2378, 2643-2695, model/layer/subsampling.py:106-132; update rule
 * model/layer/scaling.py:741-789): C = act'(act_src) (A Bm^T) (+ resid), then C += |C| (a[c] + b[c]
 * act_src) with a, b derived from bal_stats = 4096 floats: column sums [0..N) and sums of squares
 * [1024..1024+N) of act_src over its M rows (s2t_balancer_stats into a zeroed buffer); the call writes
 * the per-column a, b into [2048..) and [3072..) with one small launch before the product (N <= 1024).
 * s2t_balancer_coef is that small launch as its own call, for a caller that takes the statistics early
 * (forward pass, side stream): it then passes tile | S2T_X3P_BAL_COEF_READY.
 * Replaces the separate s2t_balancer_apply pass over the (M, N) gradient.  -2: shape / tile outside the
 * kernel's rules. */
#define S2T_X3P_BAL_COEF_READY (1 << 20)   /* or-ed into `tile`: s2t_balancer_coef already filled [2048..4096) */
int s2t_balancer_coef(float* bal_stats, int N, long rows, float min_mean, float max_mean, float min_rms,
                      float max_rms, float grad_scale, void* stream);
int s2t_gemm_x3p_bal(const float* A, long lda, const unsigned short* Bp, int N, int K, float* C, long ldc,
                     int M, const float* resid, long ldr, const float* act_src, long ld_act, int act_kind,
                     int tile, float* bal_stats, float min_mean, float max_mean, float min_rms,
                     float max_rms, float grad_scale, void* stream);

/* s2t_gemm_x3p with IMPLICIT operands: C = A' Bm^T (+ bias[N]) where row r of A' is `nseg` (<= 4) segments
 * of `seg` (multiple of 16) contiguous floats of the buffer A, segment s at amap(r) + segoff[s], and row
 * r of C lies at cmap(r) (cmap NULL: plain rows of ldc floats); K = seg * nseg; Bp = pieces of Bm (N, K).
 * map(r) = base + b sb + i sh + j sw for r = (b, i, j), b = r / hw, i = (r % hw) / w, j = r % w (all
 * offsets in floats, multiples of 4).  c_elems: elements of the mapped C buffer.  Serves the 3x3 /
 * stride-2 convolution of the conformer's Subsampling (model/encoder/conformer.py:47-57, 114-126)
 * without a patch matrix: forward (3 segments of 3 C floats per output position of the channel-last
 * map) and the data gradient (one launch per input-pixel parity class gathering 1 / 2 / 2 / 4 taps of
 * the zero-bordered output gradient and writing every second pixel), and the zipformer frontend's 32 -> 128
 * stride-(1, 2) convolution (model/layer/subsampling.py:277-319): forward and the data gradient by column
 * parity (even columns: one run of 2 Cout floats per kh, odd: Cout).  tile: 22 (default) 21 12 11; + 200:
 * 32-deep barrier intervals (two-piece arithmetic, seg a multiple of 32: else -2) -- a row's 128 bytes per
 * interval are one cache line fetched once. */
typedef struct S2tRowMap {
  int hw, w;
  long sb, sh, sw, base;
} S2tRowMap;
int s2t_gemm_x3p_map(const float* A, const S2tRowMap* amap, int seg, int nseg, const long* segoff,
                     const unsigned short* Bp, int N, float* C, long ldc, const S2tRowMap* cmap,
                     long c_elems, int M, const float* bias, int tile, void* stream);

/* ---- side stream for work off the critical path (csrc/streams.hip): the weight-gradient GEMMs
 * of backward overlap the data-gradient chain.  s2t_side_stream returns the library-owned stream;
 * s2t_stream_order(from, to) makes later work on `to` wait for the work enqueued so far on `from`. */
void* s2t_side_stream(void);
int s2t_stream_order(void* from, void* to);

/* ---- kernel-attached timing (bench.py's roofline figure).  s2t_prof_pair_arm hands a created
 * (start, stop) HIP event pair to the NEXT s2t_gemm_x3p launch of the calling thread, which is then
 * issued with hipExtLaunchKernelGGL: the pair holds the kernel's own begin / end times (what rocprof
 * reports), not the times of marker packets recorded around it.  s2t_prof_pair_consumed: 1 if a
 * launch took the armed pair, 0 if it was still armed (either way it is disarmed afterwards).
 * s2t_prof_pair_ms waits for the stop event and returns the elapsed milliseconds in *ms. */
/* the same for a SAMPLE of launches, counted inside s2t_gemm_x3p itself (so the launches the native
 * layer executor issues are sampled like the Python call sites'): every `every`-th launch between
 * begin and end carries its own event pair; end waits for them and reports how many were timed, their
 * total milliseconds and the algorithmic bytes / flops of exactly those launches
 * (4 M (N + K + operands N) + 2 P N K bytes for P pieces, 2 M N K flops).  s2t_gemm_x3p_calls: launches so far. */
int s2t_x3p_sample_begin(int every);
int s2t_x3p_sample_end(long* launches, double* total_ms, double* bytes, double* flops);
/* of the sample closed last: 4 M (N + K) + 2 P N K summed -- A, C and the weight pieces only, without the
 * epilogue operands and second outputs the figure above includes */
int s2t_x3p_sample_min_bytes(double* bytes_min);
long s2t_gemm_x3p_calls(void);
long s2t_linear_lt_calls(void);
int s2t_prof_pair_create(void** start, void** stop);
int s2t_prof_pair_arm(void* start, void* stop);
int s2t_prof_pair_consumed(void);
int s2t_prof_pair_ms(void* start, void* stop, float* ms);
int s2t_prof_pair_destroy(void* start, void* stop);


/* ---- element-wise helpers of the layer executor's library-GEMM path (csrc/zip_elem.hip):
 * out = a + b (out may alias an operand; 16-byte aligned); the parity sequence 0, 1, 0, ... of
 * s2t_balancer_bwd's two alternating accumulators, shared by every caller of the process. */
int s2t_add_f32(const float* a, const float* b, float* out, long n, void* stream);
int s2t_balancer_next_parity(void);

/* ---- batch of dense row-major fp32 products through hipBLASLt's strided-batch API (csrc/gemm_lib.hip):
 * the shapes of the nonlinear attention's products (model/encoder/zipformer.py:2468-2473 and their
 * gradients) that s2t_gemm_f32_batched refuses (rows that are not 16-byte multiples: T = 495, 62)
 * and the a^T b form.  mode 0: C_b[M,N] = A_b[M,K] B_b[N,K]^T; 1: C_b = A_b[M,K] B_b[K,N];
 * 2: C_b[M,N] = A_b[K,M]^T B_b[K,N].  Batch strides = rows * cols.  -2: no library algorithm. */
int s2t_bmm_lt(int mode, const float* A, const float* B, float* C, int batch, int M, int N, int K,
               void* workspace, long ws_bytes, void* stream);

/* ---- native per-layer executor (csrc/zip_layer.hip): ONE call per Zipformer2EncoderLayer forward and
 * one per backward issues every launch of the layer (model/encoder/zipformer.py:909-1338 under
 * loss.backward(); gradient shaping model/layer/scaling.py:741-789, 994-1028, 1153-1190).  The Python
 * side (speech2text_amd/zip_native.py) draws the layer's random decisions where the reference draws
 * them and passes them as `dec`; C++ only reads them.
 *   desc  : the layer's shapes, parameter / gradient addresses (views of the FlatStore), bf16 piece
 *           addresses of its weights (planes.py; NULL = library path) and module constants;
 *   call  : this call's shapes, inputs, masks, decisions, persistent scratch, and the switches the
 *           caller still varies (Whiten forms, the plan's tile / margin, what runs on the side stream):
 *           every field is read;
 *   state : s2t_zip_layer_state_bytes() bytes of HOST memory, written by fwd, read by bwd;
 *   ws    : device workspace, >= s2t_zip_layer_ws_floats(desc, call, backward) floats; the forward's
 *           must stay alive (and untouched) until the backward has been enqueued.
 * Decision indices (dec[]): 0 balance_keys, 1 whiten_keys, 2 use positional scores, 3 score penalty
 * drawn; feed-forward i (hidden balancer, out whiten, post balancer): 4-6, 15-17, 23-25; nonlinear
 * attention (balancer, whiten1, whiten2, post balancer) 7-10; self_attn whiten 11, 19; conv module
 * (balancer1, balancer2, whiten) 12-14, 20-22; limit_param_value of bypass_mid 18, norm.log_scale 27,
 * bypass 28; layer balancer1 26, balancer2 29, whiten 30.
 * Whiten sites (s2t_zip_layer_info(state, 0, site) after bwd: 1 penalty applied, 0 below the limit,
 * -1 did not fire): 0 keys, 1 ff1, 2 nonlin whiten1, 3 nonlin whiten2, 4 self_attn1, 5 conv1, 6 ff2,
 * 7 self_attn2, 8 conv2, 9 ff3, 10 layer output.
 * Returns 0; -4 workspace too small; -5 a product's shape bucket has no plan entry yet (nothing was
 * launched: run the Python executor for this call, it times the shapes); bwd returns 1 when the
 * score penalty of this call is non-zero (it stopped before the attention-weights backward: write
 * dqkp / dpos -- addresses from s2t_zip_layer_info -- and call again with phase 2). */
#define S2T_ZL_NDEC 32
#define S2T_ZL_NWHITEN 11
typedef struct S2tZlLin {          /* nn.Linear, weight (N,K) row-major */
  const float* w;
  const float* b;                  /* NULL: no bias */
  float* gw;
  float* gb;
  const unsigned short* pf;        /* pieces for x W^T, or NULL */
  const unsigned short* pb;        /* pieces for g W, or NULL */
  int N, K;
} S2tZlLin;
typedef struct S2tZlBal {          /* Balancer.cfg(): scaling.py:792-902 */
  float min_mean, max_mean, min_rms, max_rms, grad_scale;
} S2tZlBal;
typedef struct S2tZlWh {           /* Whiten: scaling.py:1031-1095 */
  int groups;
  float limit, grad_scale;
} S2tZlWh;
typedef struct S2tZlFf {
  S2tZlLin in, out;
  S2tZlBal hidden;
  S2tZlWh out_wh;
  S2tZlBal post;                   /* balancer_ff2 / balancer_ff3 of the layer (unused for ff1) */
} S2tZlFf;
typedef struct S2tZlSa {
  S2tZlLin in, out;
  S2tZlWh wh;
} S2tZlSa;
typedef struct S2tZlConv {
  S2tZlLin in, out;
  S2tZlBal bal1, bal2;
  S2tZlWh wh;
  int K, causal;
  const float *wc, *bc, *wk, *bk, *scale;
  float *gwc, *gbc, *gwk, *gbk, *gscale;
} S2tZlConv;
typedef struct S2tZlNa {
  S2tZlLin in, out;
  S2tZlBal bal;
  S2tZlWh wh1, wh2;
  S2tZlBal post;                   /* balancer_na of the layer */
} S2tZlNa;
typedef struct S2tZlParam {
  const float* x;
  float* grad;
  float lo, hi;
} S2tZlParam;
typedef struct S2tZipLayerDesc {
  int D, H, qd, pd, pos_dim;
  S2tZlLin attn_in, attn_pos;
  S2tZlBal bal_keys;
  S2tZlWh wh_keys;
  S2tZlFf ff[3];
  S2tZlNa na;
  S2tZlSa sa[2];
  S2tZlConv cv[2];
  S2tZlParam byp_mid, byp, norm_bias, norm_ls;
  S2tZlBal bal1, bal2;
  S2tZlWh wh_out;
} S2tZipLayerDesc;
typedef struct S2tZlWhScratch {    /* persistent scratch of the Whiten statistics, per channel count */
  int C;
  float* acc;                      /* (C+1, C), zeroed once */
  float* ws;                       /* 4 + 2 C floats, zeroed once */
  const void* tab;                 /* S2tPlaneDesc of a (C,C) matrix for mode 1, or NULL */
  unsigned short* buf;             /* its piece buffer, or NULL */
  int blocks;
} S2tZlWhScratch;
typedef struct S2tZipLayerCall {
  int T, B, chunk_size;
  const float* x0;                 /* (T*B, D) layer input */
  const float* pos;                /* (2T-1, pos_dim) positional embedding */
  const unsigned char* k8;         /* (B,T) key padding mask or NULL */
  const unsigned char* a8;         /* (T,T) attention mask or NULL */
  const float* fm;                 /* (B,D) feature mask or NULL */
  float* out;                      /* forward: (T*B, D) layer output */
  const float* g;                  /* backward: gradient w.r.t. out */
  float* gx;                       /* backward: gradient w.r.t. x0 */
  int dec[S2T_ZL_NDEC];
  float* bal_ws;                   /* s2t_balancer_bwd_workspace_floats(), zeroed once */
  float* layer_acc;                /* 3 D + 4 floats, zeroed once (per D) */
  S2tZlWhScratch wh[8];
  int nwh;
  void* lt_ws;
  long lt_ws_bytes;
  float x3p_margin;                /* s2t_zl_plan_choose's margin */
  int use_side;                    /* the caller passes a side stream to fwd / bwd: Whiten and firing Balancers' statistics,
                                      conv parameter gradients and weight gradients run there (the sizing pass has no
                                      streams and sizes by this) */
} S2tZipLayerCall;
long s2t_zip_layer_state_bytes(void);
long s2t_zip_layer_ws_floats(const S2tZipLayerDesc* desc, const S2tZipLayerCall* call, int backward);
int s2t_zip_layer_plans_missing(const S2tZipLayerDesc* desc, int T, int B);
int s2t_zip_layer_fwd(const S2tZipLayerDesc* desc, const S2tZipLayerCall* call, void* state, float* ws,
                      long ws_floats, void* stream, void* side);
int s2t_zip_layer_bwd(const S2tZipLayerDesc* desc, const S2tZipLayerCall* call, void* state, float* ws,
                      long ws_floats, int phase, void* stream, void* side);
long s2t_zip_layer_info(const void* state, int what, int idx);
void* s2t_zip_layer_error(void);
/* the timings zip_kernels.lt_matmul took for a shape bucket {mode, half-octave of the rows, N, K} of a
 * Linear: library ms, own-kernel ms (< 0: none) and its tile -- what the executor's plan is made of.
 * mode = (0 forward | 1 data gradient) | (the arithmetic the bucket was timed under, s2t_gemm_arith()) << 4 */
int s2t_zl_plan_put(int mode, int half_oct, int N, int K, double t_lib_ms, double t_own_ms, int tile);
int s2t_zl_plan_clear(void);
long s2t_zl_plan_count(void);
/* THE plan rule: which kernel serves a product of `rows` rows in the bucket {mode as given to
 * s2t_zl_plan_put, half-octave of rows, N, K} with the epilogue `epilogue_bits` (S2T_ZL_EPI_*).  1: our
 * kernel, *tile = the bucket's tile; 0: the library; -1: the bucket has no timings yet.  With one
 * elementwise pass over the (rows, cols) result costed at 4 us + 12 rows cols bytes at 3 TB/s:
 *   library = t_lib (* margin when the epilogue is plain: bias / resid2 only)
 *             + one pass per {act_src, act_src with resid2, resid_b, Swoosh act2, bal};
 *   ours    = t_own + 4 rows cols bytes at 3 TB/s per {act_src, resid_b, any act2, bal};
 * ours where it is strictly cheaper.  Launches nothing. */
#define S2T_ZL_EPI_ACT_SRC 1
#define S2T_ZL_EPI_RESID2 2
#define S2T_ZL_EPI_RESID_B 4
#define S2T_ZL_EPI_ACT2_SWOOSH 8
#define S2T_ZL_EPI_ACT2_ADD 16
#define S2T_ZL_EPI_BAL 32
int s2t_zl_plan_choose(int mode, long rows, int N, int K, int epilogue_bits, float margin, int* tile);

#ifdef __cplusplus
}
#endif
#endif /* S2T_MI355_H_ */
