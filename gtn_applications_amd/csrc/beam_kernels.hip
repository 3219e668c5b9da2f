// CTC prefix beam search on the device (wfl_ctc_beam_search; the rules are in include/wfl.h and DESIGN.md section 17).
// The greedy decode of decode_kernels.hip maximises over frame paths; this one over label sequences, whose score is the
// log-sum over all their alignments.  Three launch families:
//   candidates (a wave per row (b, t), t < T_b; the only pass over x): the K best classes of the row, ties to the lower
//              class, in that order, by K rounds of a wave argmax over keys that order (score, class) -- the row in
//              registers up to 256 classes, re-read (from cache) beyond; slot K holds the blank if it is not among them
//              (class -1 otherwise).  Also the row's log-sum-exp by wfl_row_lse's rule.
//   beam       (a workgroup per utterance: the dependent part): the ranked beam {pb, pnb, tot, two prefix hashes, last label,
//              length, arena node} lives in LDS, double-buffered.  Per frame: where does each hypothesis' last label sit
//              among the candidates; which hypothesis is the one-label extension of which (hashes, length, last label);
//              the stay entries with the merged extensions added; the W-th best stay as a lower bound of the W-th best
//              entry; every entry at or above it into a compact list; rank of each by counting -- the order is (tot
//              descending, entry index ascending), entry index = stays by rank, then extensions by (parent rank,
//              candidate position), which is the tie rule; the entries of rank < W are the next beam, a new prefix
//              appends its (parent node, label) record to the utterance's arena.  All hypothesis arithmetic is float64.
//   write      (a wave per (b, rank < nbest)): base = the lengths before it summed in a fixed order, then lane 0 walks
//              the arena back from the final node and stores the labels -- plain vector stores, `out` / `out_offsets` /
//              `scores` may be pinned host memory.
// wfl_ctc_beam_search_lm is the same three launches with a token-level n-gram LM and a length bonus fused into the beam
// launch: the beam kernel takes the LM as a parameter pack, the instantiation without one is the
// code it was; with it a hypothesis carries an LM state, an extension costs one back-off lookup (bounded binary searches
// in the LM's arrays, which stay in global memory) where its key is formed -- unless it cannot reach the W-th best stay
// entry even with the LM's largest term --, its next state waits in LDS beside the entry for place(), and the final
// beam is ranked again with </s>.
// wfl_ctc_beam_search_lexicon is the same three launches again with a lexicon and an optional word-level n-gram LM
// (DESIGN.md section 20): a third parameter pack, BeamLex, carries the lexicon's trie and a BeamLm over word ids; a
// hypothesis carries a trie node beside its LM state, an extension costs one bounded binary search among the arcs of
// its node and, where the arc completes a word, one LM step; the final beam drops the ranks inside a word.
// wfl_asg_beam_search is the search of the ASG criterion on the same launches: a fourth pack,
// BeamAsg, carries the transition matrix -- no blank (the candidates launch leaves slot K empty), one mass per
// hypothesis, the transition weight of an entry gathered where its key is formed; a hypothesis whose last label is no
// candidate of the frame has no stay entry.  Its write launch can map a result on the way out (garbage dropped, replabels
// unpacked: what ASG.viterbi does to a path), behind a launch that counts the mapped lengths.
// wfl_transducer_beam_search is the search of the Transducer criterion on the same launches: a
// fifth pack, BeamTok, carries the frame-level transitions over tokens + blank (or none) and the token graph's topology
// -- CTC's two masses per hypothesis and a transition weight on every frame-to-frame step: three gathers in a stay, two
// gathers and a log-add in an extension; the forced topology leaves the blank state only and ranks the result by pb.
// wfl_transducer_beam_search_merged is that search with hypotheses identified by the graphemes they spell and their last
// token: a sixth pack, BeamSpell, adds the spelling table of the classes; the token sequences
// that spell the same graphemes share one hypothesis, their masses summed inside the beam launch.
// wfl_asg_beam_search_lexicon is the ASG search with the lexicon and word LM of the CTC one: a
// seventh pack, BeamAsgLex, holds a BeamAsg, a BeamLex over raw class sequences and the garbage class, which the trie
// does not see -- ASG's one mass and transition gather per entry, the lexicon's node and state per hypothesis.
// wfl_transducer_beam_search_lexicon is the Transducer search with that lexicon and word LM: an
// eighth pack, BeamTokLex, holds a BeamTok and a BeamLex -- the Transducer's two masses and transition gathers per
// entry, the lexicon's node and state per hypothesis.
// wfl_ctc_beam_search_lexicon_marked and wfl_transducer_beam_search_lexicon_marked are the two lexicon searches with a
// start-marked lexicon (word pieces that carry the word boundary at the start of a word; a word
// ends where the next begins or with the utterance): the packs BeamLexMarked and BeamTokLexMarked add node_word and
// start_node to their siblings' fields, selected at compile time -- another step function, the node behind a word in
// place(), the pending word's term in the final block; the siblings' kernels are the code they were.
// The four *_lookahead entries are the lexicon searches of CTC and the Transducer, end- and start-marked, with unigram max
// look-ahead of the word LM inside words: BeamLook<sibling's pack> adds node_look, the best word
// score below every trie node; a hypothesis pays lm_weight node_look[node] provisionally on the way down a word and
// settles it where the word ends, so the totals are the siblings' and a narrow beam ranks by the word the LM wants.
// wfl_transducer_beam_search_lm is the Transducer search with the token-level n-gram LM and length bonus of the CTC one
// (DESIGN.md section 28): a pack BeamTokLm holds a BeamTok and a BeamLm -- the Transducer's two masses and transition
// gathers per entry, the LM's state per hypothesis, one back-off lookup per extension behind the same skip test, and
// the forced topology's drop-and-rank-by-pb ahead of </s> in the final block.
// wfl_asg_beam_search_lm is the ASG search with that token-level LM and length bonus: a pack BeamAsgLm
// holds a BeamAsg, a BeamLm over the criterion's tokens and the raw alphabet (replabels, garbage) the LM reads through --
// the LM reads what the mapped write launch emits: a token steps it once, a replabel right behind a token steps it by
// that token again (k + 1 times), the garbage and any other replabel step it not at all; a hypothesis carries the
// token a replabel would repeat beside its LM state.
// All sixteen issue these launches through one host path, beam_run (behind the kernels): an entry makes the checks that are
// its own, describes the call in a BeamCall and hands over its pack, by which beam_run picks the beam kernel.
// No atomics on global memory and no cross-workgroup waits; the one LDS counter only decides where an entry sits in the
// compact list, never its rank: the result is deterministic.
#include "device_common.h"

namespace wfl {

constexpr int kBeamMax = 64;                                    // beam width and classes per frame
constexpr int kBeamCand = kBeamMax + 1;                         // + the appended blank
constexpr int kBeamEntries = kBeamMax + kBeamMax * kBeamCand;   // stays + extensions: 4224
constexpr int kBeamMaxClasses = 16384;
constexpr unsigned long long kBeamHashMul = 0x9E3779B97F4A7C15ull;  // odd: h' = h * mul + label + 1 (mod 2^64)
constexpr unsigned long long kBeamHashMul2 = 0xC2B2AE3D27D4EB4Full;  // a second, independent hash of the same form
constexpr long long kKeyDropped = (long long)0x8000000000000000ull;  // below the key of every finite score
constexpr unsigned long long kKeySign = 0x8000000000000000ull;       // key ^ sign: the same order, unsigned
constexpr int kBeamRankAll = 512;  // entries above the bound up to which every one of them is ranked against every other

// workspace: [candidate classes: B T (K+1) int32 | candidate scores: B T (K+1) float | row lse: B T float |
//             arena: B T W int2 | final node: B nbest int32 | final length: B nbest int32]
// asg (wfl_asg_beam_search): no row lse, and behind the rest [mapped length: B nbest int32]
// (beam_workspace reports its size and beam_run turns it into pointers: nothing else reads it)
struct BeamWs {
  int64_t cls, sc, lse, arena, fin_node, fin_len, out_len, bytes;
};
inline int64_t beam_align16(int64_t n) { return (n + 15) & ~(int64_t)15; }
inline BeamWs beam_ws_layout(int64_t B, int64_t T, int64_t W, int64_t K, int64_t nbest, bool asg = false) {
  BeamWs w;
  w.cls = 0;
  w.sc = w.cls + beam_align16(B * T * (K + 1) * 4);
  w.lse = w.sc + beam_align16(B * T * (K + 1) * 4);
  w.arena = w.lse + (asg ? 0 : beam_align16(B * T * 4));
  w.fin_node = w.arena + beam_align16(B * T * W * 8);
  w.fin_len = w.fin_node + beam_align16(B * nbest * 4);
  w.out_len = w.fin_len + beam_align16(B * nbest * 4);
  w.bytes = w.out_len + (asg ? beam_align16(B * nbest * 4) : 0);
  return w;
}

// a score as an int whose signed order is the order of the scores: -0 = +0, NaN = -inf (wfl_row_argmax's rule)
__device__ __forceinline__ int beam_score_key(float v) {
  if (v != v) return (int)0x807fffff;  // the key of -inf
  int b = __float_as_int(v);
  if (b == (int)0x80000000) b = 0;
  return b >= 0 ? b : b ^ 0x7fffffff;
}

constexpr int kBeamNoIndex = 0x3fffffff;
constexpr int kBeamNoKey = -2147483647 - 1;

// NV > 0: the row in NV registers per lane (C <= 64 NV); NV == 0: any C, the row re-read in every round
template <int NV>
__global__ void __launch_bounds__(256) beam_candidates_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                               int B, int T, int C, int blank, int K,
                                                               int32_t* __restrict__ cls_out, float* __restrict__ sc_out,
                                                               float* __restrict__ lse_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)B * T) return;  // (a whole wave)
  const int b = (int)(row / T), t = (int)(row % T);
  const int Tb = lengths ? min(max(lengths[b], 0), T) : T;
  if (t >= Tb) return;  // (wave-uniform: the frames behind the utterance are not read)
  const float* r = x + row * C;
  int key[NV > 0 ? NV : 1];
  float m = WFL_NEG_INF;
  if constexpr (NV > 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      const float v = c < C ? nan_to_neg(r[c]) : WFL_NEG_INF;
      key[i] = beam_score_key(v);
      m = fmaxf(m, v);
    }
  } else {
    for (int c = lane; c < C; c += 64) m = fmaxf(m, nan_to_neg(r[c]));
  }
  // the row's log-sum-exp (wfl_row_lse's rule: float32, relative to the maximum, -inf for a row without a finite score)
  // (lse_out NULL -- the ASG search, which normalises by its own denominator: no log-sum-exp)
  if (lse_out) {  // (uniform)
    m = wave_all_max(m);
    float sum = 0.f;
    if (m > WFL_NEG_INF)
      for (int c = lane; c < C; c += 64) sum += fast_exp(nan_to_neg(r[c]) - m);
    sum = wave_all_sum(sum);
    if (lane == 0) lse_out[row] = m > WFL_NEG_INF ? m + fast_log(sum) : WFL_NEG_INF;
  }
  // K rounds: the best (score, lowest class) behind the previous round's pick; lane k keeps the pick of round k
  int pk = 0x7fffffff, pi = -1, mine = -1;
  for (int k = 0; k < K; ++k) {
    int bk = kBeamNoKey, bi = kBeamNoIndex;
    if constexpr (NV > 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        const bool behind = key[i] < pk || (key[i] == pk && c > pi);
        if (c < C && behind && key[i] > bk) bk = key[i], bi = c;  // (ascending c: the first of equals stays)
      }
    } else {
#pragma unroll 4
      for (int c = lane; c < C; c += 64) {
        const int kc = beam_score_key(r[c]);
        const bool behind = kc < pk || (kc == pk && c > pi);
        if (behind && kc > bk) bk = kc, bi = c;
      }
    }
    pk = wave_all_max_int(bk);
    pi = -wave_all_max_int(-(bk == pk ? bi : kBeamNoIndex));
    if (lane == k) mine = pi;
  }
  const int64_t o = row * (K + 1);
  if (lane < K) cls_out[o + lane] = mine, sc_out[o + lane] = nan_to_neg(r[min(max(mine, 0), C - 1)]);
  // (blank < 0 -- the ASG search, which has none: slot K holds class -1 and nothing is read at index -1)
  const bool found = blank < 0 || __ballot(lane < K && mine == blank) != 0ull;
  if (lane == 0) cls_out[o + K] = found ? -1 : blank, sc_out[o + K] = found ? WFL_NEG_INF : nan_to_neg(r[blank]);
}

__device__ __forceinline__ int wave_inclusive_scan_int(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// log(exp(a) + exp(b)) in float64, -inf the identity
__device__ __forceinline__ double beam_lae(double a, double b) {
  const double ninf = -__builtin_inf();
  if (a == ninf) return b;
  if (b == ninf) return a;
  return fmax(a, b) + log1p(exp(-fabs(a - b)));
}
// a total as an int64 whose signed order is the order of the totals; -inf (and NaN): dropped
__device__ __forceinline__ long long beam_key(double d) {
  if (!(d > -__builtin_inf())) return kKeyDropped;
  if (d == 0.0) return 0;
  const long long b = __double_as_longlong(d);
  return b >= 0 ? b : b ^ 0x7fffffffffffffffLL;
}

// the LM of a launch: wfl_ngram_lm's device arrays (a pack that passed wfl_ngram_lm_check) and the scalars of the call
struct BeamLm {
  const int32_t *arc_ptr, *arc_label, *arc_next, *bo_next;
  const double *arc_w, *bo_w;
  int start, eos;  // eos: the label of </s> = C
  double alpha, beta;
  double bound;  // no extension's alpha step + beta is above it (+inf: unknown)
  int score_eos;
};
constexpr int kLmMaxBackoff = WFL_NGRAM_LM_MAX_BACKOFF;

// step(s, c) of include/wfl.h: the log weight of label c from state s, backing off while s has no such arc; -inf if the
// chain ends without one.  Both loops are bounded: at most kLmMaxBackoff back-offs, 31 halvings of a range of < 2^31 arcs.
__device__ __forceinline__ double beam_lm_step(const BeamLm& lm, int s, int c, int& next) {
  double acc = 0.0;
  for (int d = 0; d <= kLmMaxBackoff; ++d) {
    const int end = lm.arc_ptr[s + 1];
    int lo = lm.arc_ptr[s], hi = end;
    for (int it = 0; it < 31 && lo < hi; ++it) {  // the first arc whose label is not below c
      const int mid = lo + ((hi - lo) >> 1);
      if (lm.arc_label[mid] < c)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < end && lm.arc_label[lo] == c) {
      next = lm.arc_next[lo];
      return acc + lm.arc_w[lo];
    }
    const int bo = lm.bo_next[s];
    if (bo < 0) break;
    acc += lm.bo_w[s], s = bo;
  }
  next = lm.start;  // (never used: the entry does not exist)
  return -__builtin_inf();
}
// The total a key was made of: beam_key's inverse.  beam_key maps +0 and -0 to the key 0 before it folds the sign, so
// the key of a zero comes back as +0 -- the one total whose bits may differ, and equal to it.  (Not for kKeyDropped.)
__device__ __forceinline__ double beam_key_total(long long k) {
  return __longlong_as_double(k >= 0 ? k : k ^ 0x7fffffffffffffffLL);
}

struct BeamHyp {  // (struct of arrays, one per buffer)
  double pb[kBeamMax], pnb[kBeamMax], tot[kBeamMax];
  unsigned long long hash[kBeamMax], hash2[kBeamMax];
  int last[kBeamMax], len[kBeamMax], node[kBeamMax];
};

__device__ __forceinline__ const BeamLm& beam_lm_of(const BeamLm& lm) { return lm; }

// the lexicon of a launch: wfl_lexicon's device arrays (a pack that passed wfl_lexicon_check), the word LM or none, and
// the scalars of the call.  lm.alpha, lm.beta, lm.score_eos are the call's; lm.eos is the word LM's </s> label V + 1;
// without a word LM (has_lm == 0) lm's pointers are not read and every word's step is 0.
struct BeamLex {
  const int32_t *arc_ptr, *arc_label, *arc_next;
  BeamLm lm;
  int has_lm;
  double omega;  // the word bonus
  double bound;  // no extension's term is above it (+inf: unknown)
};
__device__ __forceinline__ const BeamLex& beam_lex_of(const BeamLex& lx) { return lx; }

// The term of an extension that completes a word whose LM step is l: (alpha l + omega) + beta, each operation rounded
// on its own -- on the host, where beam_lex_bound forms the largest such term, and on the device alike, so that the
// bound holds by the monotonicity of the rounded operations (a fused multiply-add would round once and may land above).
__host__ __device__ inline double beam_lex_word_term(double alpha, double l, double omega, double beta) {
#pragma clang fp contract(off)
  const double al = alpha * l;
  const double t = al + omega;
  return t + beta;
}
// The largest term of an extension: beta inside a word (= 0 + beta), beam_lex_word_term at a word's end with
// l in [step_min, step_max].  alpha l <= max(alpha step_min, alpha step_max) =: m, so (alpha l + omega) + beta <=
// (m + omega) + beta <= max(0, m + omega) + beta, and 0 + beta is below the last as well; 0 * inf: no bound.
inline double beam_lex_bound(double alpha, double step_min, double step_max, double omega, double beta) {
#pragma clang fp contract(off)
  const double t0 = alpha * step_min, t1 = alpha * step_max;
  if (t0 != t0 || t1 != t1) return __builtin_inf();
  const double m = fmax(t0, t1) + omega;
  return fmax(0.0, m) + beta;
}

constexpr int kLexAbsent = -2147483647 - 1;  // no arc_next: word ids are below 2^31 - 1

// Word-LM look-ahead (wfl_lexicon_lookahead): look[n] is the best word score below trie node n, 0 at
// the root; a hypothesis at node n has paid alpha look[n] provisionally.  The three terms that move it, every operation
// rounded on its own, on the host (wfl_lexicon_lookahead_check, beam_look_bound) and on the device alike:
// an inner arc n -> m costs (alpha (look[m] - look[n])) + beta (rule 1);
__host__ __device__ inline double beam_look_arc_diff(double look_to, double look_from) {
#pragma clang fp contract(off)
  return look_to - look_from;  // (the check records the range of exactly this value)
}
__host__ __device__ inline double beam_look_inner_term(double alpha, double look_to, double look_from, double beta) {
#pragma clang fp contract(off)
  const double d = beam_look_arc_diff(look_to, look_from);
  const double ad = alpha * d;
  return ad + beta;
}
// the LM step of a word that completes at node n is settled against what was paid: l - look[n] (rules 2 and 4);
__host__ __device__ inline double beam_look_settled(double l, double look_at) {
#pragma clang fp contract(off)
  return l - look_at;
}
// a start-marked word's first label behind a word pays the first node's share on top of the word's term (rule 3)
__host__ __device__ inline double beam_look_start_term(double alpha, double term, double look_start) {
#pragma clang fp contract(off)
  const double al = alpha * look_start;
  return term + al;
}

// The extension of a hypothesis at trie node `node` with LM state `state` by class c: its term, -inf if it does not
// exist (no such arc, or a word the LM cannot follow the history with).  enc: where the new hypothesis stands -- an
// inner node n as n >= 0 (the LM state stays), the root behind a word as -(next LM state + 1).  The search among the
// node's arcs is bounded like the LM's: 31 halvings.  LOOK: the terms of section 27 (look: node_look), one 8-byte load
// per end of the arc; without it `look` is not read and the function is the one it was.
template <bool LOOK>
__device__ __forceinline__ double beam_lex_step_at(const BeamLex& lx, const double* __restrict__ look, int node, int state,
                                                   int c, int& enc) {
  const int end = lx.arc_ptr[node + 1];
  int lo = lx.arc_ptr[node], hi = end;
  for (int it = 0; it < 31 && lo < hi; ++it) {  // the first arc whose label is not below c
    const int mid = lo + ((hi - lo) >> 1);
    if (lx.arc_label[mid] < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  enc = 0;
  const int nx = (lo < end && lx.arc_label[lo] == c) ? lx.arc_next[lo] : kLexAbsent;
  if (nx == kLexAbsent) return -__builtin_inf();
  if (nx >= 0) {
    enc = nx;
    if constexpr (LOOK) return beam_look_inner_term(lx.lm.alpha, look[nx], look[node], lx.lm.beta);
    return lx.lm.beta;
  }
  double l = 0.0;
  int ns = 0;
  if (lx.has_lm) {
    l = beam_lm_step(lx.lm, state, -(nx + 1), ns);
    if (!(l > -__builtin_inf())) return -__builtin_inf();
  }
  enc = -(ns + 1);
  if constexpr (LOOK) l = beam_look_settled(l, look[node]);
  return beam_lex_word_term(lx.lm.alpha, l, lx.omega, lx.lm.beta);
}
__device__ __forceinline__ double beam_lex_step(const BeamLex& lx, int node, int state, int c, int& enc) {
  return beam_lex_step_at<false>(lx, nullptr, node, state, c, enc);
}

// A start-marked lexicon (wfl_lexicon_marked): BeamLex's trie with stored leaves and all arc targets
// inner nodes, node_word[n] the word whose spelling ends at node n (-1: none), start_node[c] the root's child by class c
// (-1: c starts no word).  A word ends where the next begins, or with the utterance.
struct BeamLexMarked {
  BeamLex lex;
  const int32_t *node_word, *start_node;
};
__device__ __forceinline__ const BeamLex& beam_lex_of(const BeamLexMarked& m) { return m.lex; }
__device__ __forceinline__ const BeamLexMarked& beam_lex_marked_of(const BeamLexMarked& m) { return m; }

// The term of a word that ends with the utterance (section 26 rule 5): alpha l + omega, each operation rounded on its own
__device__ __forceinline__ double beam_lex_pending_term(double alpha, double l, double omega) {
#pragma clang fp contract(off)
  const double al = alpha * l;
  return al + omega;
}

// beam_lex_step for a start-marked lexicon (section 26 rule 3).  One load of start_node[c] decides the case: c starts no
// word -- the bounded search among the node's arcs (none at the root, whose arcs all start words), the state stays; c
// starts a word from the root -- its child, the state stays; from a terminal node -- the LM step of the word that ends
// there, enc = -(next LM state + 1) and place() takes the node from start_node[c]; from any other node -- nothing.
// LOOK: section 27's terms, as in beam_lex_step_at (the root's look is 0 by wfl_lexicon_marked_lookahead_check).
template <bool LOOK>
__device__ __forceinline__ double beam_lex_step_marked_at(const BeamLexMarked& m, const double* __restrict__ look, int node,
                                                          int state, int c, int& enc) {
  const BeamLex& lx = m.lex;
  enc = 0;
  const int sn = m.start_node[c];
  if (sn < 0) {
    if (node == 0) return -__builtin_inf();
    const int end = lx.arc_ptr[node + 1];
    int lo = lx.arc_ptr[node], hi = end;
    for (int it = 0; it < 31 && lo < hi; ++it) {  // the first arc whose label is not below c
      const int mid = lo + ((hi - lo) >> 1);
      if (lx.arc_label[mid] < c)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (!(lo < end && lx.arc_label[lo] == c)) return -__builtin_inf();
    enc = lx.arc_next[lo];
    if constexpr (LOOK) return beam_look_inner_term(lx.lm.alpha, look[enc], look[node], lx.lm.beta);
    return lx.lm.beta;
  }
  if (node == 0) {
    enc = sn;
    if constexpr (LOOK) return beam_look_inner_term(lx.lm.alpha, look[sn], 0.0, lx.lm.beta);
    return lx.lm.beta;
  }
  const int v = m.node_word[node];
  if (v < 0) return -__builtin_inf();
  double l = 0.0;
  int ns = 0;
  if (lx.has_lm) {
    l = beam_lm_step(lx.lm, state, v, ns);
    if (!(l > -__builtin_inf())) return -__builtin_inf();
  }
  enc = -(ns + 1);
  if constexpr (LOOK) {
    const double term = beam_lex_word_term(lx.lm.alpha, beam_look_settled(l, look[node]), lx.omega, lx.lm.beta);
    return beam_look_start_term(lx.lm.alpha, term, look[sn]);
  }
  return beam_lex_word_term(lx.lm.alpha, l, lx.omega, lx.lm.beta);
}
__device__ __forceinline__ double beam_lex_step_marked(const BeamLexMarked& m, int node, int state, int c, int& enc) {
  return beam_lex_step_marked_at<false>(m, nullptr, node, state, c, enc);
}

// the transitions of an ASG launch (wfl_asg_beam_search): Wt [(C+1), C] float32 in the criterion's layout (asg.py:54-69:
// row 0 start -> c, row 1 + i: j -> i), and the denominator to subtract from the scores or NULL
struct BeamAsg {
  const float* Wt;
  const float* logz;  // [B] float32 (wfl_dense_forward's), or NULL: raw scores
  int C;
};
__device__ __forceinline__ const BeamAsg& beam_asg_of(const BeamAsg& a) { return a; }
// the transition weight into class c behind last label l (l < 0: from the start), widened exactly, a NaN = -inf: one
// gather from a matrix that the frames of every utterance share (it stays in L2)
__device__ __forceinline__ double beam_asg_w(const BeamAsg& a, int l, int c) {
  const float w = l < 0 ? a.Wt[c] : a.Wt[(int64_t)(1 + c) * a.C + l];
  return w != w ? -__builtin_inf() : (double)w;
}

// the ASG launch with a lexicon (wfl_asg_beam_search_lexicon): BeamAsg's transitions and BeamLex's
// trie, word LM and bonuses -- the trie over RAW class sequences (replabels included) --, and the garbage class, which
// no spelling contains: an extension by it keeps node and state and costs no lookup (-1: the criterion has none)
struct BeamAsgLex {
  BeamAsg asg;
  BeamLex lex;
  int garbage;
};
__device__ __forceinline__ const BeamAsgLex& beam_asg_lex_of(const BeamAsgLex& a) { return a; }
__device__ __forceinline__ const BeamAsg& beam_asg_of(const BeamAsgLex& a) { return a.asg; }
__device__ __forceinline__ const BeamLex& beam_lex_of(const BeamAsgLex& a) { return a.lex; }

// the transitions of a Transducer launch (wfl_transducer_beam_search): Wt [(C+1), C] float32 in the dense engine's layout
// (row 0 start -> c, row 1 + i: j -> i) or NULL (every weight 0), the denominator to subtract or NULL (the row
// log-sum-exps, as in the plain search), and the topology of the token graph
struct BeamTok {
  const float* Wt;
  const float* logz;  // [B] float32 (wfl_dense_forward's), or NULL
  int C;
  int forced;  // 1: a token is entered from the blank state only, and a path ends in the blank
};
__device__ __forceinline__ const BeamTok& beam_tok_of(const BeamTok& a) { return a; }
// w(p, c): the weight into class c behind frame label p (p < 0: from the start), widened exactly, a NaN = -inf
__device__ __forceinline__ double beam_tok_w(const BeamTok& a, int p, int c) {
  if (!a.Wt) return 0.0;
  const float w = p < 0 ? a.Wt[c] : a.Wt[(int64_t)(1 + c) * a.C + p];
  return w != w ? -__builtin_inf() : (double)w;
}
// rule 4: the extension by candidate c (score s) of a hypothesis (pb, pnb, last label l) whose blank-side state is
// `brow` (the start in frame 0, the blank behind it)
__device__ __forceinline__ double beam_tok_ext(const BeamTok& a, double pb, double pnb, int l, int brow, int c, double s) {
  double m = pb + beam_tok_w(a, brow, c);
  if (!a.forced && l >= 0 && c != l && pnb > -__builtin_inf()) m = beam_lae(m, pnb + beam_tok_w(a, l, c));
  return s + m;
}

// the Transducer launch with a token-level LM (wfl_transducer_beam_search_lm): BeamTok's
// transitions and topology, BeamLm's acceptor over the tokens, the two scalars and the bound of an extension's term
struct BeamTokLm {
  BeamTok tok;
  BeamLm lm;
};
__device__ __forceinline__ const BeamTok& beam_tok_of(const BeamTokLm& a) { return a.tok; }
__device__ __forceinline__ const BeamLm& beam_lm_of(const BeamTokLm& a) { return a.lm; }
// The LM term of such an extension whose step is l: alpha l + beta, each operation rounded on its own -- on the device
// as where the entry forms the largest such term, so that the bound holds by the monotonicity of the rounded
// operations (a fused multiply-add would round once and may land above).
__device__ __forceinline__ double beam_tok_lm_term(double alpha, double l, double beta) {
#pragma clang fp contract(off)
  const double al = alpha * l;
  return al + beta;
}
// the largest such term, l in [step_min, step_max], by the same operations (0 * inf: no bound)
inline double beam_tok_lm_bound(double alpha, double step_min, double step_max, double beta) {
#pragma clang fp contract(off)
  const double t0 = alpha * step_min, t1 = alpha * step_max;
  if (t0 != t0 || t1 != t1) return __builtin_inf();
  return fmax(t0, t1) + beta;
}

// the ASG launch with a token-level LM (wfl_asg_beam_search_lm): BeamAsg's transitions, BeamLm's
// acceptor over the N = C - replabels - (garbage >= 0) tokens (lm.eos = N + 1), and the raw alphabet the LM reads
// through: replabel k is raw class k < replabels, token i is raw class i + replabels, `garbage` the garbage class (-1:
// none).  lm.bound: the largest term of an extension (beam_asg_lm_bound).
struct BeamAsgLm {
  BeamAsg asg;
  BeamLm lm;
  int replabels;
  int garbage;
};
__device__ __forceinline__ const BeamAsgLm& beam_asg_lm_of(const BeamAsgLm& a) { return a; }
__device__ __forceinline__ const BeamAsg& beam_asg_of(const BeamAsgLm& a) { return a.asg; }
__device__ __forceinline__ const BeamLm& beam_lm_of(const BeamAsgLm& a) { return a.lm; }
// rep': the token a replabel right behind the prefix + c would repeat (-1: none), from the prefix' own `rep` -- the
// write launch's rule (beam_map_walk, read forwards): the garbage is not seen, a token is the next to repeat, a
// replabel uses the token up
__device__ __forceinline__ int beam_asg_lm_rep(const BeamAsgLm& a, int rep, int c) {
  if (c == a.garbage) return rep;
  return c >= a.replabels ? c - a.replabels : -1;
}
// The LM term of the extension by raw class c of a hypothesis with LM state `state` and `rep` (section 29 rules 1 and
// 2): the labels c emits -- none for the garbage and for a replabel with nothing to repeat, the token c - R once, the
// token `rep` c + 1 times for a replabel behind it -- stepped in order, term = term + (alpha l + beta) per label, each
// operation rounded on its own (as where beam_asg_lm_bound forms the largest such sum); -inf where a step is: the
// extension does not exist.  next: the state behind the labels (`state` where nothing is emitted).  At most max(1, R)
// lookups; the loop is bounded by R.
__device__ __forceinline__ double beam_asg_lm_term(const BeamAsgLm& a, int state, int rep, int c, int& next) {
#pragma clang fp contract(off)
  next = state;
  if (c == a.garbage) return 0.0;
  const bool token = c >= a.replabels;
  if (!token && rep < 0) return 0.0;
  const int u = token ? c - a.replabels : rep, n = token ? 1 : c + 1;
  double term = 0.0;
  for (int q = n; q > 0 && term > -__builtin_inf(); --q) {  // (n <= max(1, R): a replabel is a class below R)
    int nx;
    const double l = beam_lm_step(a.lm, next, u, nx);
    const double al = a.lm.alpha * l;
    const double t = al + a.lm.beta;
    term = l > -__builtin_inf() ? term + t : -__builtin_inf();
    next = nx;
  }
  return term;
}
// the largest such term: n = 0 .. max(1, R) accumulations of max(alpha step_min, alpha step_max) + beta, by the same
// rounded operations -- every partial sum of a term is below the partial sum here by their monotonicity (0 * inf: no bound)
inline double beam_asg_lm_bound(double alpha, double step_min, double step_max, double beta, int R) {
#pragma clang fp contract(off)
  const double t0 = alpha * step_min, t1 = alpha * step_max;
  if (t0 != t0 || t1 != t1) return __builtin_inf();
  const double m = fmax(t0, t1) + beta;
  double acc = 0.0, bound = 0.0;
  for (int n = 0; n < (R > 1 ? R : 1); ++n) {
    acc = acc + m;
    bound = fmax(bound, acc);
  }
  return bound;
}

// the Transducer launch with a lexicon (wfl_transducer_beam_search_lexicon): BeamTok's transitions
// and topology, BeamLex's trie over token sequences, word LM and bonuses
struct BeamTokLex {
  BeamTok tok;
  BeamLex lex;
};
__device__ __forceinline__ const BeamTok& beam_tok_of(const BeamTokLex& a) { return a.tok; }
__device__ __forceinline__ const BeamLex& beam_lex_of(const BeamTokLex& a) { return a.lex; }

// the same launch with a start-marked lexicon (wfl_transducer_beam_search_lexicon_marked)
struct BeamTokLexMarked {
  BeamTok tok;
  BeamLexMarked lex;
};
__device__ __forceinline__ const BeamTok& beam_tok_of(const BeamTokLexMarked& a) { return a.tok; }
__device__ __forceinline__ const BeamLex& beam_lex_of(const BeamTokLexMarked& a) { return a.lex.lex; }
__device__ __forceinline__ const BeamLexMarked& beam_lex_marked_of(const BeamTokLexMarked& a) { return a.lex; }

// the lexicon's term of an extension by the convention of the launch's pack: beam_lex_step, or beam_lex_step_marked
__device__ __forceinline__ double beam_lex_ext(const BeamLex& a, int node, int state, int c, int& enc) {
  return beam_lex_step(a, node, state, c, enc);
}
__device__ __forceinline__ double beam_lex_ext(const BeamAsgLex& a, int node, int state, int c, int& enc) {
  return beam_lex_step(a.lex, node, state, c, enc);
}
__device__ __forceinline__ double beam_lex_ext(const BeamTokLex& a, int node, int state, int c, int& enc) {
  return beam_lex_step(a.lex, node, state, c, enc);
}
__device__ __forceinline__ double beam_lex_ext(const BeamLexMarked& a, int node, int state, int c, int& enc) {
  return beam_lex_step_marked(a, node, state, c, enc);
}
__device__ __forceinline__ double beam_lex_ext(const BeamTokLexMarked& a, int node, int state, int c, int& enc) {
  return beam_lex_step_marked(a.lex, node, state, c, enc);
}

// The four lexicon searches of CTC and the Transducer with word-LM look-ahead (the wfl_*_beam_search_lexicon*_lookahead
// entries): the sibling's pack and node_look [num_nodes] behind it, selected at compile time -- the
// step functions' LOOK terms and the pending word's settled step in the final block; the siblings' kernels are the code
// they were.  The lexicon's `bound` is beam_look_bound's there.
template <typename P>
struct BeamLook {
  P pack;
  const double* node_look;
};
using BeamLexLook = BeamLook<BeamLex>;
using BeamLexMarkedLook = BeamLook<BeamLexMarked>;
using BeamTokLexLook = BeamLook<BeamTokLex>;
using BeamTokLexMarkedLook = BeamLook<BeamTokLexMarked>;
template <typename P>
__device__ __forceinline__ const BeamLex& beam_lex_of(const BeamLook<P>& a) {
  return beam_lex_of(a.pack);
}
template <typename P>
__device__ __forceinline__ const BeamLexMarked& beam_lex_marked_of(const BeamLook<P>& a) {
  return beam_lex_marked_of(a.pack);
}
template <typename P>
__device__ __forceinline__ const BeamTok& beam_tok_of(const BeamLook<P>& a) {
  return beam_tok_of(a.pack);
}
template <typename P>
__device__ __forceinline__ const double* beam_look_of(const BeamLook<P>& a) {
  return a.node_look;
}
__device__ __forceinline__ double beam_lex_ext(const BeamLexLook& a, int node, int state, int c, int& enc) {
  return beam_lex_step_at<true>(a.pack, a.node_look, node, state, c, enc);
}
__device__ __forceinline__ double beam_lex_ext(const BeamTokLexLook& a, int node, int state, int c, int& enc) {
  return beam_lex_step_at<true>(a.pack.lex, a.node_look, node, state, c, enc);
}
__device__ __forceinline__ double beam_lex_ext(const BeamLexMarkedLook& a, int node, int state, int c, int& enc) {
  return beam_lex_step_marked_at<true>(a.pack, a.node_look, node, state, c, enc);
}
__device__ __forceinline__ double beam_lex_ext(const BeamTokLexMarkedLook& a, int node, int state, int c, int& enc) {
  return beam_lex_step_marked_at<true>(a.pack.lex, a.node_look, node, state, c, enc);
}

// the Transducer launch that merges by spelling (wfl_transducer_beam_search_merged): BeamTok's
// fields and the spelling table over the C classes -- class c spells the graphemes spell_sym[spell_ptr[c] ..
// spell_ptr[c + 1]), none for the blank, 1 .. WFL_SPELL_MAX for every other class (wfl_spelling_check)
struct BeamSpell {
  BeamTok tok;
  const int32_t *spell_ptr, *spell_sym;
};
__device__ __forceinline__ const BeamSpell& beam_spell_of(const BeamSpell& a) { return a; }
__device__ __forceinline__ const BeamTok& beam_tok_of(const BeamSpell& a) { return a.tok; }
constexpr int kSpellMax = WFL_SPELL_MAX;
// the inverse of an odd multiplier mod 2^64 (Newton: every round doubles the correct low bits, a itself has three)
constexpr unsigned long long beam_inverse(unsigned long long a) {
  unsigned long long v = a;
  for (int i = 0; i < 6; ++i) v *= 2ull - a * v;
  return v;
}
constexpr unsigned long long kBeamHashInv = beam_inverse(kBeamHashMul), kBeamHashInv2 = beam_inverse(kBeamHashMul2);
static_assert(kBeamHashInv * kBeamHashMul == 1ull && kBeamHashInv2 * kBeamHashMul2 == 1ull, "the hash multipliers' inverses");

template <typename... Lm>
struct BeamPack {
  static constexpr bool lm = false, lex = false, asg = false, tok = false, spell = false;
};
template <>
struct BeamPack<BeamLm> {
  static constexpr bool lm = true, lex = false, asg = false, tok = false, spell = false;
};
template <>
struct BeamPack<BeamLex> {
  static constexpr bool lm = false, lex = true, asg = false, tok = false, spell = false;
};
template <>
struct BeamPack<BeamAsg> {
  static constexpr bool lm = false, lex = false, asg = true, tok = false, spell = false;
};
// (asg and lex: ASG's single mass and transition gather, the lexicon's node / state arrays and final drop-and-rerank)
template <>
struct BeamPack<BeamAsgLex> {
  static constexpr bool lm = false, lex = true, asg = true, tok = false, spell = false;
};
// (asg and lm: ASG's single mass and transition gather, the LM's state arrays and </s> ranking, and `rep` per hypothesis)
template <>
struct BeamPack<BeamAsgLm> {
  static constexpr bool lm = true, lex = false, asg = true, tok = false, spell = false;
};
template <>
struct BeamPack<BeamTok> {
  static constexpr bool lm = false, lex = false, asg = false, tok = true, spell = false;
};
// (tok and lex: the Transducer's two masses and transition gathers, the lexicon's node / state arrays, term per
// extension and final drop, ahead of the ranking the Transducer's result shares with it)
template <>
struct BeamPack<BeamTokLex> {
  static constexpr bool lm = false, lex = true, asg = false, tok = true, spell = false;
};
// (tok and lm: the Transducer's two masses and transition gathers, the LM's state arrays, term per extension and </s>
// behind the topology's score in the ranking the Transducer's result shares with it)
template <>
struct BeamPack<BeamTokLm> {
  static constexpr bool lm = true, lex = false, asg = false, tok = true, spell = false;
};
// (the two lexicon packs with a start-marked lexicon: the traits of their end-marked siblings, and BeamMarked below)
template <>
struct BeamPack<BeamLexMarked> : BeamPack<BeamLex> {};
template <>
struct BeamPack<BeamTokLexMarked> : BeamPack<BeamTokLex> {};
// whether the pack's lexicon is start-marked (section 26): the step of an extension, the node behind a word in place(),
// and the pending word after the last frame
template <typename... Lm>
struct BeamMarked {
  static constexpr bool value = false;
};
template <>
struct BeamMarked<BeamLexMarked> {
  static constexpr bool value = true;
};
template <>
struct BeamMarked<BeamTokLexMarked> {
  static constexpr bool value = true;
};
// (the four packs with look-ahead: the traits of their siblings, and BeamLooks below)
template <typename P>
struct BeamPack<BeamLook<P>> : BeamPack<P> {};
template <typename P>
struct BeamMarked<BeamLook<P>> : BeamMarked<P> {};
// whether the pack's lexicon search has word-LM look-ahead (section 27): the step of an extension (by beam_lex_ext's
// overload) and the pending word after the last frame
template <typename... Lm>
struct BeamLooks {
  static constexpr bool value = false;
};
template <typename P>
struct BeamLooks<BeamLook<P>> {
  static constexpr bool value = true;
};
// (tok: what the three Transducer searches share -- the normaliser, the frame's log-sum-exp, the forced topology's result)
template <>
struct BeamPack<BeamSpell> {
  static constexpr bool lm = false, lex = false, asg = false, tok = true, spell = true;
};

// NT threads: 256 where a frame has at most 1024 entries, 1024 beyond (the ranking is the work that scales).
// Lm: nothing -- the search of wfl_ctc_beam_search, its parameters and its code what they were --, or one BeamLm: the
// n-gram LM and length bonus of wfl_ctc_beam_search_lm, or one BeamLex: the lexicon, word LM and bonuses of
// wfl_ctc_beam_search_lexicon, or one BeamAsg: the search of wfl_asg_beam_search -- no blank
// (blank = -1, slot K of the candidates empty), one mass per hypothesis (tot; pb = -inf, pnb = tot), a transition weight
// in every stay and every extension, a hypothesis whose last label is no candidate has no stay entry; lengths and
// row_lse NULL, normalize != 0: the pack's logz[b] is subtracted; or one BeamTok: the search of
// wfl_transducer_beam_search -- the plain search's two masses with a transition weight on every
// step (w = 0 without a matrix), the blank-side state the start row in frame 0, the forced topology's extensions from pb
// alone and none in frame 0, the final beam ranked again by pb there; lengths NULL, row_lse NULL where logz normalises;
// or one BeamSpell: the search of wfl_transducer_beam_search_merged -- BeamTok's arithmetic per
// hypothesis, but a hypothesis is identified by (the graphemes it spells, its last token): the hashes run over
// graphemes, len counts them and a token count rides along for the write launch; per frame the hypotheses of one
// spelling form a class (a member mask, the leader its lowest rank), an extension entry exists for leaders only and
// sums the extensions of the members in rank order, and the parent class of a hypothesis is found by un-appending
// the spelling of its last token from its hashes (the multipliers are odd: one multiplication by the inverse per
// grapheme, once per hypothesis -- cheaper than extending every class by it); the result merges the ranks of one
// spelling before it is ranked; or one BeamAsgLex: the search of wfl_asg_beam_search_lexicon --
// BeamAsg's arithmetic with BeamLex's node and state per hypothesis, term per extension and final drop-and-rerank; an
// extension by the garbage class keeps node and state; or one BeamTokLex: the search of
// wfl_transducer_beam_search_lexicon -- BeamTok's arithmetic with BeamLex's node and state per
// hypothesis, term per extension (the merged one inside a stay included) and final drop ahead of the ranking; or a
// start-marked sibling of a lexicon pack (section 26), or BeamLook<a lexicon pack of CTC or the Transducer>: that pack's
// search with the terms of word-LM look-ahead (section 27) -- beam_lex_ext's overload and the pending word's settled step;
// or one BeamTokLm: the search of wfl_transducer_beam_search_lm -- BeamTok's arithmetic with
// BeamLm's state per hypothesis, LM term per extension (the merged one inside a stay included) behind the skip test, and
// </s> on top of the topology's score in the final ranking; or one BeamAsgLm: the search of wfl_asg_beam_search_lm
//  -- BeamAsg's arithmetic with BeamLm's state and `rep` per hypothesis, beam_asg_lm_term per
// extension (the merged one inside a stay and the one that stands in for a missing stay in the bound included) behind
// the skip test, and the LM search's </s> ranking.
template <int NT, typename... Lm>
__global__ void __launch_bounds__(NT) beam_search_kernel(const int32_t* __restrict__ lengths, int T, int blank, int W, int K,
                                                           int nbest, int normalize, const int32_t* __restrict__ cand_cls,
                                                           const float* __restrict__ cand_sc, const float* __restrict__ row_lse,
                                                           int2* __restrict__ arena, int32_t* __restrict__ fin_node,
                                                           int32_t* __restrict__ fin_len, double* __restrict__ scores,
                                                           Lm... lm_arg) {
  constexpr bool LM = BeamPack<Lm...>::lm, LEX = BeamPack<Lm...>::lex, ASG = BeamPack<Lm...>::asg, TOK = BeamPack<Lm...>::tok;
  constexpr bool SPELL = BeamPack<Lm...>::spell;  // (TOK as well)
  constexpr bool MARK = BeamMarked<Lm...>::value;  // (LEX as well)
  constexpr bool LOOK = BeamLooks<Lm...>::value;  // (LEX as well)
  __shared__ BeamHyp beam[2];
  __shared__ long long ckey[kBeamEntries];
  __shared__ int cidx[kBeamEntries];
  __shared__ double s_sc[2][kBeamCand];
  __shared__ int s_cls[2][kBeamCand];
  __shared__ int s_bpos[2];
  __shared__ double spb[kBeamMax], spnb[kBeamMax], stot[kBeamMax];
  __shared__ long long skey[kBeamMax];
  __shared__ unsigned long long mmask[kBeamMax];
  __shared__ int lpos[kBeamMax], par[kBeamMax];
  __shared__ long long s_tau;
  __shared__ int s_count;
  __shared__ int hist[256];
  __shared__ long long wkey[kBeamMax];
  __shared__ int widx[kBeamMax];
  __shared__ int s_bin, s_need, s_ties, s_wcount;
  __shared__ double s_norm;
  // LM only: the state of every hypothesis (double-buffered like the beam) and the next state of every extension, by
  // entry index, from where its key is formed to place()
  int(*lmst)[kBeamMax] = nullptr;
  int* enext = nullptr;
  if constexpr (LM) {
    __shared__ int s_lmst[2][kBeamMax];
    __shared__ int s_enext[kBeamEntries];
    lmst = s_lmst, enext = s_enext;
  }
  // lexicon only: the same two, enext holding beam_lex_step's `enc` (node and state of an extension in one int), and
  // the trie node of every hypothesis
  int(*tnode)[kBeamMax] = nullptr;
  if constexpr (LEX) {
    __shared__ int s_xlmst[2][kBeamMax];
    __shared__ int s_xtnode[2][kBeamMax];
    __shared__ int s_xenext[kBeamEntries];
    lmst = s_xlmst, tnode = s_xtnode, enext = s_xenext;
  }
  // merging by spelling only: the token count of every hypothesis (len counts graphemes there), and per frame the
  // member mask of every hypothesis' spelling class
  // ASG with a token-level LM only: the token a replabel behind every hypothesis would repeat (double-buffered like
  // the beam); an entry's own follows from its parent's and its class in place(): nothing is kept per entry
  int(*hrep)[kBeamMax] = nullptr;
  if constexpr (ASG && LM) {
    __shared__ int s_hrep[2][kBeamMax];
    hrep = s_hrep;
  }
  int(*ntok)[kBeamMax] = nullptr;
  unsigned long long* cmask = nullptr;
  if constexpr (SPELL) {
    __shared__ int s_ntok[2][kBeamMax];
    __shared__ unsigned long long s_cmask[kBeamMax];
    ntok = s_ntok, cmask = s_cmask;
  }

  const int tid = threadIdx.x, b = blockIdx.x;
  const int KC = K + 1;
  const int Tb = lengths ? min(max(lengths[b], 0), T) : T;
  const double ninf = -__builtin_inf();
  const int32_t* ccls = cand_cls + (int64_t)b * T * KC;
  const float* csc = cand_sc + (int64_t)b * T * KC;
  const float* lse = row_lse + (int64_t)b * T;
  int2* nodes = arena + (int64_t)b * T * W;

  if (tid == 0) {
    s_bpos[0] = s_bpos[1] = 0;
    beam[0].pb[0] = 0.0, beam[0].pnb[0] = ninf, beam[0].tot[0] = 0.0;
    beam[0].hash[0] = 0ull, beam[0].hash2[0] = 0ull, beam[0].last[0] = -1, beam[0].len[0] = 0, beam[0].node[0] = -1;
    if constexpr (LM) lmst[0][0] = beam_lm_of(lm_arg...).start;
    if constexpr (ASG && LM) hrep[0][0] = -1;
    if constexpr (LEX) lmst[0][0] = beam_lex_of(lm_arg...).has_lm ? beam_lex_of(lm_arg...).lm.start : 0, tnode[0][0] = 0;
    if constexpr (SPELL) ntok[0][0] = 0;
  }
  __syncthreads();
  // the candidates of frame 0 into buffer 0
  if (tid < KC && Tb > 0) {
    const int c = ccls[tid];
    s_cls[0][tid] = c, s_sc[0][tid] = (double)csc[tid];
    if (c == blank) s_bpos[0] = tid;
  }
  int nbeam = 1;
  double norm = 0.0;
  __syncthreads();

  for (int t = 0; t < Tb; ++t) {
    const int cur = t & 1;
    const BeamHyp& h = beam[cur];
    BeamHyp& g = beam[cur ^ 1];
    const int* cls = s_cls[cur];
    const double* sc = s_sc[cur];
    // the next frame's candidates: loads in flight across this frame's work
    int ncls = -1;
    float nsc = 0.f, flse = 0.f;
    if (tid < KC && t + 1 < Tb) ncls = ccls[(int64_t)(t + 1) * KC + tid], nsc = csc[(int64_t)(t + 1) * KC + tid];
    if constexpr (TOK) {
      if (tid == 0 && row_lse) flse = lse[t];
    } else if constexpr (!ASG)
      if (tid == 0) flse = lse[t];
    const int ncand = K + (cls[K] >= 0 ? 1 : 0);
    const int bpos = s_bpos[cur];

    // where each hypothesis' last label sits among the candidates
    if (tid < nbeam) {
      int p = -1;
      const int l = h.last[tid];
      if (l >= 0)
        for (int q = 0; q < ncand; ++q)
          if (cls[q] == l) p = q;
      lpos[tid] = p, par[tid] = -1;
    }
    __syncthreads();
    if constexpr (SPELL) {
      // the spelling class of every hypothesis (its members' ranks as a mask; the leader is the lowest), and the leader
      // of its parent class: the class that spells what it spells without its last token
      const BeamSpell& sp = beam_spell_of(lm_arg...);
      if (tid < nbeam) {
        const unsigned long long hh = h.hash[tid], hh2 = h.hash2[tid];
        const int ln = h.len[tid], l = h.last[tid];
        unsigned long long m = 0ull;
        for (int j = 0; j < nbeam; ++j)
          if (h.len[j] == ln && h.hash[j] == hh && h.hash2[j] == hh2) m |= 1ull << j;
        cmask[tid] = m;
        int pl = -1;
        if (lpos[tid] >= 0 && !(sp.tok.forced && t == 0)) {  // (only a candidate extends anything; lpos >= 0: l >= 0)
          const int s0 = sp.spell_ptr[l], n = min(sp.spell_ptr[l + 1] - s0, kSpellMax);
          unsigned long long ph = hh, ph2 = hh2;
          for (int q = n - 1; q >= 0; --q) {  // h = h_parent mul^n + ...: taken off from the end
            const unsigned long long gq = (unsigned long long)(sp.spell_sym[s0 + q] + 1);
            ph = (ph - gq) * kBeamHashInv, ph2 = (ph2 - gq) * kBeamHashInv2;
          }
          const int plen = ln - n;
          for (int j = nbeam - 1; j >= 0; --j)
            if (h.len[j] == plen && h.hash[j] == ph && h.hash2[j] == ph2) pl = j;
        }
        par[tid] = pl;
      }
      __syncthreads();
      // every member's extension by the last token of a hypothesis whose parent class it is in merges into that stay
      if (tid < nbeam) {
        const int lead = __ffsll(cmask[tid]) - 1;
        unsigned long long mask = 0ull;
        for (int j = 0; j < nbeam; ++j)
          if (par[j] == lead) mask |= 1ull << lpos[j];  // (par[j] >= 0 only where lpos[j] >= 0)
        mmask[tid] = mask;
      }
    } else if (tid < nbeam) {
      // which hypothesis j is hypothesis i plus one label: that extension merges into j's stay entry
      unsigned long long mask = 0ull;
      const unsigned long long hm = h.hash[tid] * kBeamHashMul, hm2 = h.hash2[tid] * kBeamHashMul2;
      const int l1 = h.len[tid] + 1;
      for (int j = 0; j < nbeam; ++j)
        if (lpos[j] >= 0 && h.len[j] == l1 && h.hash[j] == hm + (unsigned long long)(h.last[j] + 1) &&
            h.hash2[j] == hm2 + (unsigned long long)(h.last[j] + 1))
          mask |= 1ull << lpos[j], par[j] = tid;
      mmask[tid] = mask;
    }
    __syncthreads();
    // the stay entries
    if constexpr (ASG) {
      // ASG: a stay repeats the last label l over its self transition l -> l, and exists only where l is a candidate;
      // the merged extension comes over the transition from its parent's last label into l
      if (tid < nbeam) {
        const BeamAsg& a = beam_asg_of(lm_arg...);
        const int p = lpos[tid], l = h.last[tid], i = par[tid];
        double m = ninf;
        if constexpr (LEX || !LM) m = p >= 0 ? (sc[p] + beam_asg_w(a, l, l)) + h.tot[tid] : ninf;
        long long rk;
        if constexpr (LEX) {
          // With a lexicon one extension per hypothesis is looked up here: the one merged into this stay (p >= 0, i >= 0),
          // which carries the term of the prefix it makes (node and state: functions of it), or -- where there is no
          // stay (p < 0, and then i < 0: par is set only where lpos is) -- the own extension that stands in for the
          // bound below.  The garbage is transparent to the trie: term 0, no lookup.
          // The bound wants one entry per hypothesis that EXISTS (arc present, LM step finite): the garbage extension
          // where the garbage is a candidate (no lookup), else the first own extension, looked up; absent, the
          // hypothesis contributes kKeyDropped and the frame's bound prunes nothing.
          const int garbage = beam_asg_lex_of(lm_arg...).garbage;
          int src = i, c = l, q = p;
          if (p < 0) {
            const unsigned long long own = ~mmask[tid];
            q = own ? __ffsll(own) - 1 : ncand;
            for (int j = 0; j < ncand; ++j)
              if (cls[j] == garbage && ((own >> j) & 1ull)) q = j;
            if (q < ncand) src = tid, c = cls[q];
          }
          double e = ninf;
          if (src >= 0) {
            const double ac = (sc[q] + beam_asg_w(a, h.last[src], c)) + h.tot[src];
            double term = 0.0;
            int enc;
            if (c != garbage)
              term = ac > ninf ? beam_lex_ext(lm_arg..., tnode[cur][src], lmst[cur][src], c, enc) : ninf;
            if (term > ninf) e = ac + term;
          }
          if (p >= 0) m = beam_lae(m, e);
          rk = beam_key(p >= 0 ? m : e);
          spb[tid] = ninf, spnb[tid] = m, stot[tid] = m, skey[tid] = beam_key(m);
        } else if constexpr (LM) {
          // (ahead of the plain branch below.)  With a token-level LM one extension per hypothesis gets its term here: the
          // one merged into this stay (p >= 0, i >= 0), which carries the term of the prefix it makes (state and rep:
          // functions of it), or -- where there is no stay (p < 0, and then i < 0) -- the first own extension, which
          // stands in for the bound below with its real term, lookups included: it may serve only if it EXISTS; where
          // a step is -inf the hypothesis contributes kKeyDropped and the frame's bound prunes nothing.
          const BeamAsgLm& al = beam_asg_lm_of(lm_arg...);
          int src = i, c = l, q = p;
          if (p < 0) {
            const unsigned long long own = ~mmask[tid];
            q = own ? __ffsll(own) - 1 : ncand;
            if (q < ncand) src = tid, c = cls[q];
          }
          double e = ninf;
          if (src >= 0) {
            const double ac = (sc[q] + beam_asg_w(a, h.last[src], c)) + h.tot[src];
            int nx;
            const double term = ac > ninf ? beam_asg_lm_term(al, lmst[cur][src], hrep[cur][src], c, nx) : ninf;
            if (term > ninf) e = ac + term;
          }
          // (the stay's own term behind the lookup: nothing of it is live across the LM's loops)
          if (p >= 0) m = beam_lae((sc[p] + beam_asg_w(a, l, l)) + h.tot[tid], e);
          rk = beam_key(p >= 0 ? m : e);
          spb[tid] = ninf, spnb[tid] = m, stot[tid] = m, skey[tid] = beam_key(m);
        } else {
          if (i >= 0) m = beam_lae(m, (sc[p] + beam_asg_w(a, h.last[i], l)) + h.tot[i]);  // (par[j] is set only where lpos[j] >= 0)
          rk = beam_key(m);
          spb[tid] = ninf, spnb[tid] = m, stot[tid] = m, skey[tid] = rk;
          // The bound below wants one entry per hypothesis.  CTC's blank gives every hypothesis a stay; here a hypothesis
          // whose last label is no candidate has none, and its first extension that is an entry of its own stands in
          // (l is no candidate, so no candidate is l; a merged extension is part of another hypothesis' stay).
          if (p < 0) {
            const unsigned long long own = ~mmask[tid];
            const int q = own ? __ffsll(own) - 1 : ncand;
            if (q < ncand) rk = beam_key((sc[q] + beam_asg_w(a, l, cls[q])) + h.tot[tid]);
          }
        }
        wkey[tid] = rk;  // (wkey: free until the selection)
      }
    } else if constexpr (SPELL) {
      // section 22's stay; behind its own term the extensions of every member of the parent class, in rank order
      if (tid < nbeam) {
        const BeamTok& a = beam_tok_of(lm_arg...);
        const int p = lpos[tid], l = h.last[tid], pl = par[tid], brow = t == 0 ? -1 : blank;
        double m = h.pb[tid] + beam_tok_w(a, brow, blank);
        if (l >= 0 && h.pnb[tid] > ninf) m = beam_lae(m, h.pnb[tid] + beam_tok_w(a, l, blank));
        const double pb = sc[bpos] + m;
        double pnb = p >= 0 && h.pnb[tid] > ninf ? (sc[p] + h.pnb[tid]) + beam_tok_w(a, l, l) : ninf;
        if (pl >= 0) {  // (par: only where p >= 0, and never in the forced topology's frame 0)
          unsigned long long mm = cmask[pl];
          for (int it = 0; it < kBeamMax && mm; ++it) {
            const int i = __ffsll(mm) - 1;
            mm &= mm - 1ull;
            pnb = beam_lae(pnb, beam_tok_ext(a, h.pb[i], h.pnb[i], h.last[i], brow, l, sc[p]));
          }
        }
        const double tot = beam_lae(pb, pnb);
        spb[tid] = pb, spnb[tid] = pnb, stot[tid] = tot, skey[tid] = beam_key(tot);
      }
    } else if constexpr (TOK) {
      // rule 3: the blank is entered from the blank-side state and from the last label, the last label repeats over its
      // self transition; the merged extension is rule 4's
      if (tid < nbeam) {
        const BeamTok& a = beam_tok_of(lm_arg...);
        const int p = lpos[tid], l = h.last[tid], i = par[tid], brow = t == 0 ? -1 : blank;
        double m = h.pb[tid] + beam_tok_w(a, brow, blank);
        if (l >= 0 && h.pnb[tid] > ninf) m = beam_lae(m, h.pnb[tid] + beam_tok_w(a, l, blank));
        const double pb = sc[bpos] + m;
        double pnb = p >= 0 && h.pnb[tid] > ninf ? (sc[p] + h.pnb[tid]) + beam_tok_w(a, l, l) : ninf;
        if constexpr (LEX) {
          // (section 25 rule 3: the merged extension carries the term of the prefix it makes -- node and state are
          // functions of it --, and does not exist where the trie or the LM has none)
          if (i >= 0 && !(a.forced && t == 0)) {
            const double ac = beam_tok_ext(a, h.pb[i], h.pnb[i], h.last[i], brow, l, sc[p]);
            int enc;
            const double term = ac > ninf ? beam_lex_ext(lm_arg..., tnode[cur][i], lmst[cur][i], l, enc) : ninf;
            if (term > ninf) pnb = beam_lae(pnb, ac + term);
          }
        } else if constexpr (LM) {
          // (section 28: the merged extension carries the LM term of the prefix it makes -- the state is a function of
          // it --, and does not exist where the LM has no step)
          if (i >= 0 && !(a.forced && t == 0)) {
            const BeamLm& lm = beam_lm_of(lm_arg...);
            const double ac = beam_tok_ext(a, h.pb[i], h.pnb[i], h.last[i], brow, l, sc[p]);
            int nx;
            const double st = ac > ninf ? beam_lm_step(lm, lmst[cur][i], l, nx) : ninf;
            if (st > ninf) pnb = beam_lae(pnb, ac + beam_tok_lm_term(lm.alpha, st, lm.beta));
          }
        } else if (i >= 0 && !(a.forced && t == 0))
          pnb = beam_lae(pnb, beam_tok_ext(a, h.pb[i], h.pnb[i], h.last[i], brow, l, sc[p]));  // (par: only where p >= 0)
        const double tot = beam_lae(pb, pnb);
        spb[tid] = pb, spnb[tid] = pnb, stot[tid] = tot, skey[tid] = beam_key(tot);
      }
    } else if (tid < nbeam) {
      const int p = lpos[tid];
      const double pb = sc[bpos] + h.tot[tid];
      double pnb = p >= 0 ? sc[p] + h.pnb[tid] : ninf;
      const int i = par[tid];
      if constexpr (LM) {
        if (i >= 0) {  // the merged extension carries the LM term of the prefix it makes
          const BeamLm& lm = beam_lm_of(lm_arg...);
          const double e = sc[p] + (h.last[i] == h.last[tid] ? h.pb[i] : h.tot[i]);
          int nx;
          const double l = e > ninf ? beam_lm_step(lm, lmst[cur][i], h.last[tid], nx) : ninf;
          if (l > ninf) pnb = beam_lae(pnb, e + (lm.alpha * l + lm.beta));
        }
      } else if constexpr (LEX) {
        if (i >= 0) {  // the merged extension carries the term of the prefix it makes (node and state: functions of it)
          const double e = sc[p] + (h.last[i] == h.last[tid] ? h.pb[i] : h.tot[i]);
          int enc;
          const double term = e > ninf ? beam_lex_ext(lm_arg..., tnode[cur][i], lmst[cur][i], h.last[tid], enc) : ninf;
          if (term > ninf) pnb = beam_lae(pnb, e + term);
        }
      } else {
        if (i >= 0) pnb = beam_lae(pnb, sc[p] + (h.last[i] == h.last[tid] ? h.pb[i] : h.tot[i]));
      }
      const double tot = beam_lae(pb, pnb);
      spb[tid] = pb, spnb[tid] = pnb, stot[tid] = tot, skey[tid] = beam_key(tot);
    }
    if (tid == 0) s_tau = kKeyDropped, s_count = 0, norm += (double)flse;
    __syncthreads();
    // a full beam: the W-th best stay bounds the W-th best entry from below (ASG: of the one entry per hypothesis above)
    const long long* bkey = skey;
    if constexpr (ASG) bkey = wkey;
    if (tid < nbeam && nbeam == W) {
      const long long k = bkey[tid];
      int n = 0;
      for (int j = 0; j < W; ++j) n += (bkey[j] > k || (bkey[j] == k && j < tid)) ? 1 : 0;
      if (n == W - 1) s_tau = k;
    }
    __syncthreads();
    // every entry at or above the bound into the compact list
    const long long tau = s_tau;
    for (int e = tid; e < nbeam * (1 + ncand); e += NT) {
      long long k;
      int idx;
      if (e < nbeam) {
        k = skey[e], idx = e;
      } else {
        const int q = e - nbeam, i = q / ncand, p = q - i * ncand;
        const int c = cls[p];
        idx = kBeamMax + i * kBeamCand + p;
        if (c == blank || ((mmask[i] >> p) & 1ull))
          k = kKeyDropped;
        else if constexpr (ASG && LEX) {
          // ASG's extension (one mass, the transition gathered here) with the lexicon's term: the garbage keeps node and
          // state (enc = the node: >= 0, the state stays) and is not looked up; a trie extension is the lexicon
          // search's, its skip test included (the garbage has term 0: nothing to skip)
          const BeamLex& lx = beam_lex_of(lm_arg...);
          const int l = h.last[i];
          int enc = 0;
          if (c == l)
            k = kKeyDropped;  // (i's stay, not an extension)
          else {
            const double ac = (sc[p] + beam_asg_w(beam_asg_of(lm_arg...), l, c)) + h.tot[i];
            if (c == beam_asg_lex_of(lm_arg...).garbage) {
              k = beam_key(ac), enc = tnode[cur][i];
            } else {
              const bool reach = ac > ninf && beam_key(ac + lx.bound) >= tau;
              const double term = reach ? beam_lex_ext(lm_arg..., tnode[cur][i], lmst[cur][i], c, enc) : ninf;
              k = term > ninf ? beam_key(ac + term) : kKeyDropped;
            }
          }
          enext[idx] = enc;
        } else if constexpr (ASG && LM) {
          // ASG's extension (one mass, the transition gathered here) with the token-level LM's term (section 29): what
          // c emits through the raw alphabet stepped from i's state; (ahead of the LM and ASG branches, which each take
          // the other for unset.)  The skip test is the LM search's with the largest term of up to max(1, R) steps; an
          // extension that emits nothing has term 0 <= that bound and is not looked up either way.
          const BeamAsgLm& al = beam_asg_lm_of(lm_arg...);
          const int l = h.last[i];
          int nx = lmst[cur][i];
          if (c == l)
            k = kKeyDropped;  // (i's stay, not an extension)
          else {
            const double ac = (sc[p] + beam_asg_w(al.asg, l, c)) + h.tot[i];
            const bool reach = ac > ninf && beam_key(ac + al.lm.bound) >= tau;
            const double term = reach ? beam_asg_lm_term(al, lmst[cur][i], hrep[cur][i], c, nx) : ninf;
            k = term > ninf ? beam_key(ac + term) : kKeyDropped;
          }
          enext[idx] = nx;
        } else if constexpr (TOK && LEX) {
          // the Transducer's extension (section 22 rule 4: both masses, the transitions gathered here; none in the forced
          // topology's frame 0) with the lexicon's term and skip test; (ahead of the LEX and TOK branches, which each
          // take the other for unset)
          const BeamLex& lx = beam_lex_of(lm_arg...);
          const BeamTok& a = beam_tok_of(lm_arg...);
          const double ac = beam_tok_ext(a, h.pb[i], h.pnb[i], h.last[i], t == 0 ? -1 : blank, c, sc[p]);
          int enc = 0;
          const bool reach = !(a.forced && t == 0) && ac > ninf && beam_key(ac + lx.bound) >= tau;
          const double term = reach ? beam_lex_ext(lm_arg..., tnode[cur][i], lmst[cur][i], c, enc) : ninf;
          k = term > ninf ? beam_key(ac + term) : kKeyDropped;
          enext[idx] = enc;
        } else if constexpr (TOK && LM) {
          // the Transducer's extension (section 22 rule 4: both masses, the transitions gathered here; none in the forced
          // topology's frame 0) with the LM's term and skip test; (ahead of the LM and TOK branches, which each take
          // the other for unset)
          const BeamLm& lm = beam_lm_of(lm_arg...);
          const BeamTok& a = beam_tok_of(lm_arg...);
          const double ac = beam_tok_ext(a, h.pb[i], h.pnb[i], h.last[i], t == 0 ? -1 : blank, c, sc[p]);
          int nx = 0;
          const bool reach = !(a.forced && t == 0) && ac > ninf && beam_key(ac + lm.bound) >= tau;
          const double l = reach ? beam_lm_step(lm, lmst[cur][i], c, nx) : ninf;
          k = l > ninf ? beam_key(ac + beam_tok_lm_term(lm.alpha, l, lm.beta)) : kKeyDropped;
          enext[idx] = nx;
        } else if constexpr (LM) {
          const BeamLm& lm = beam_lm_of(lm_arg...);
          const double ac = sc[p] + (c == h.last[i] ? h.pb[i] : h.tot[i]);  // the extension without its LM term
          int nx = 0;
          // (an entry below the bound even with the LM's largest term is outside the beam: no lookup; + is monotone)
          const bool reach = ac > ninf && beam_key(ac + lm.bound) >= tau;
          const double l = reach ? beam_lm_step(lm, lmst[cur][i], c, nx) : ninf;
          k = l > ninf ? beam_key(ac + (lm.alpha * l + lm.beta)) : kKeyDropped;
          enext[idx] = nx;
        } else if constexpr (LEX) {
          const BeamLex& lx = beam_lex_of(lm_arg...);
          const double ac = sc[p] + (c == h.last[i] ? h.pb[i] : h.tot[i]);  // the extension without its term
          int enc = 0;
          // (an entry below the bound even with the largest term is outside the beam: no lookup; + is monotone)
          const bool reach = ac > ninf && beam_key(ac + lx.bound) >= tau;
          const double term = reach ? beam_lex_ext(lm_arg..., tnode[cur][i], lmst[cur][i], c, enc) : ninf;
          k = term > ninf ? beam_key(ac + term) : kKeyDropped;
          enext[idx] = enc;
        } else if constexpr (ASG) {
          // (c the last label of i: that is i's stay, not an extension; the start row of Wt for the empty prefix)
          const int l = h.last[i];
          k = c == l ? kKeyDropped : beam_key((sc[p] + beam_asg_w(beam_asg_of(lm_arg...), l, c)) + h.tot[i]);
        } else if constexpr (SPELL) {
          // one entry per spelling class and candidate, at the leader: the members' extensions summed in rank order
          const BeamTok& a = beam_tok_of(lm_arg...);
          unsigned long long mm = cmask[i];
          if ((a.forced && t == 0) || __ffsll(mm) - 1 != i)
            k = kKeyDropped;
          else {
            double m = ninf;
            for (int it = 0; it < kBeamMax && mm; ++it) {
              const int j = __ffsll(mm) - 1;
              mm &= mm - 1ull;
              m = beam_lae(m, beam_tok_ext(a, h.pb[j], h.pnb[j], h.last[j], t == 0 ? -1 : blank, c, sc[p]));
            }
            k = beam_key(m);
          }
        } else if constexpr (TOK) {
          const BeamTok& a = beam_tok_of(lm_arg...);
          k = a.forced && t == 0 ? kKeyDropped
                                 : beam_key(beam_tok_ext(a, h.pb[i], h.pnb[i], h.last[i], t == 0 ? -1 : blank, c, sc[p]));
        } else
          k = beam_key(sc[p] + (c == h.last[i] ? h.pb[i] : h.tot[i]));
      }
      if (k != kKeyDropped && k >= tau) {
        const int slot = atomicAdd(&s_count, 1);
        ckey[slot] = k, cidx[slot] = idx;
      }
    }
    __syncthreads();
    const int M = s_count;
    // entry idx (of key k) is the hypothesis of rank r of the next beam
    auto place = [&](int idx, int r, long long k) {
      if (idx < kBeamMax) {
        g.pb[r] = spb[idx], g.pnb[r] = spnb[idx], g.tot[r] = stot[idx];
        g.hash[r] = h.hash[idx], g.hash2[r] = h.hash2[idx], g.last[r] = h.last[idx], g.len[r] = h.len[idx], g.node[r] = h.node[idx];
        if constexpr (LM) lmst[cur ^ 1][r] = lmst[cur][idx];
        if constexpr (ASG && LM) hrep[cur ^ 1][r] = hrep[cur][idx];
        if constexpr (LEX) lmst[cur ^ 1][r] = lmst[cur][idx], tnode[cur ^ 1][r] = tnode[cur][idx];
        if constexpr (SPELL) ntok[cur ^ 1][r] = ntok[cur][idx];
      } else if constexpr (SPELL) {
        // a new (spelling, last token): the class' sum is in the key; the representative token sequence is that of
        // the lowest-ranked member whose own extension is finite (there is one: the sum is), with c behind it
        const BeamSpell& sp = beam_spell_of(lm_arg...);
        const int i = (idx - kBeamMax) / kBeamCand, p = (idx - kBeamMax) - i * kBeamCand;
        const int c = cls[p];
        const double e = beam_key_total(k);
        unsigned long long mm = cmask[i];
        int rep = i;
        for (int it = 0; it < kBeamMax && mm; ++it) {
          const int j = __ffsll(mm) - 1;
          mm &= mm - 1ull;
          if (beam_tok_ext(sp.tok, h.pb[j], h.pnb[j], h.last[j], t == 0 ? -1 : blank, c, sc[p]) > ninf) {
            rep = j;
            break;
          }
        }
        const int s0 = sp.spell_ptr[c], n = min(sp.spell_ptr[c + 1] - s0, kSpellMax);
        unsigned long long nh = h.hash[i], nh2 = h.hash2[i];
        for (int q = 0; q < n; ++q) {
          const unsigned long long gq = (unsigned long long)(sp.spell_sym[s0 + q] + 1);
          nh = nh * kBeamHashMul + gq, nh2 = nh2 * kBeamHashMul2 + gq;
        }
        const int node = t * W + r;
        g.pb[r] = ninf, g.pnb[r] = e, g.tot[r] = e;
        g.hash[r] = nh, g.hash2[r] = nh2;
        g.last[r] = c, g.len[r] = h.len[i] + n, g.node[r] = node;
        ntok[cur ^ 1][r] = ntok[cur][rep] + 1;
        nodes[node] = make_int2(h.node[rep], c);
      } else {
        const int i = (idx - kBeamMax) / kBeamCand, p = (idx - kBeamMax) - i * kBeamCand;
        const int c = cls[p];
        double e;
        if constexpr (ASG && LM)  // (ahead of the LM branch: the parent's rep and c give the entry's)
          hrep[cur ^ 1][r] = beam_asg_lm_rep(beam_asg_lm_of(lm_arg...), hrep[cur][i], c);
        if constexpr (LM)
          e = beam_key_total(k), lmst[cur ^ 1][r] = enext[idx];  // (the total with its LM term: the key holds it)
        else if constexpr (LEX) {
          // (inside a word: the node, the parent's state; behind one: the root, a new state; ASG's garbage: the
          // parent's node as enc, so both stay -- and the total with its transition weight is in the key there too,
          // as with the Transducer's transitions)
          const int enc = enext[idx];
          e = beam_key_total(k);
          // (a start-marked lexicon: behind a word stands the first node of the next, the root's child by c)
          int behind = 0;
          if constexpr (MARK)
            if (enc < 0) behind = beam_lex_marked_of(lm_arg...).start_node[c];
          tnode[cur ^ 1][r] = enc >= 0 ? enc : behind, lmst[cur ^ 1][r] = enc >= 0 ? lmst[cur][i] : -(enc + 1);
        } else if constexpr (ASG || TOK)
          e = beam_key_total(k);  // (the total with its transition weight: the key holds it, no second gather)
        else
          e = sc[p] + (c == h.last[i] ? h.pb[i] : h.tot[i]);
        const int node = t * W + r;
        g.pb[r] = ninf, g.pnb[r] = e, g.tot[r] = e;
        g.hash[r] = h.hash[i] * kBeamHashMul + (unsigned long long)(c + 1);
        g.hash2[r] = h.hash2[i] * kBeamHashMul2 + (unsigned long long)(c + 1);
        g.last[r] = c, g.len[r] = h.len[i] + 1, g.node[r] = node;
        nodes[node] = make_int2(h.node[i], c);
      }
    };
    // A long list: the W-th largest key by a radix select over the keys' bytes, most significant first (a histogram
    // of the byte among the keys that share the bytes above it, then the bin the W-th largest falls into) -- O(M) per
    // byte where ranking every entry is O(M^2).  The entries at or above that key are the survivors, unless more keys
    // tie with it than the beam has room for: then the order among the ties decides, and the full ranking below does it.
    bool selected = false;
    if (M > kBeamRankAll) {
      unsigned long long prefix = 0ull;
      int need = W;
      for (int pass = 7; pass >= 0; --pass) {
        const int shift = 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int m = tid; m < M; m += NT) {
          const unsigned long long u = (unsigned long long)ckey[m] ^ kKeySign;
          if (pass == 7 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)(u >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid < 64) {  // lane l: the bins 255 - 4 l down to 252 - 4 l; the first lane whose running count reaches `need`
          const int top = 255 - 4 * tid;
          const int h0 = hist[top], h1 = hist[top - 1], h2 = hist[top - 2], h3 = hist[top - 3];
          const int incl = wave_inclusive_scan_int(h0 + h1 + h2 + h3, tid);
          const unsigned long long reach = __ballot(incl >= need);
          if (reach && tid == __ffsll(reach) - 1) {
            int left = need - (incl - (h0 + h1 + h2 + h3)), bin = top, n = h0;  // (left >= 1: the lanes above fell short)
            if (left > n) left -= n, bin = top - 1, n = h1;
            if (bin == top - 1 && left > n) left -= n, bin = top - 2, n = h2;
            if (bin == top - 2 && left > n) left -= n, bin = top - 3, n = h3;
            s_bin = bin, s_need = left, s_ties = n;
          }
          if (tid == 0) s_wcount = 0;
        }
        __syncthreads();
        prefix |= (unsigned long long)s_bin << shift;
        need = s_need;
      }
      selected = s_ties == need;  // (uniform: exactly the W best are at or above the key)
      if (selected) {
        for (int m = tid; m < M; m += NT)
          if (((unsigned long long)ckey[m] ^ kKeySign) >= prefix) {
            const int slot = atomicAdd(&s_wcount, 1);
            wkey[slot] = ckey[m], widx[slot] = cidx[m];
          }
        __syncthreads();
        if (tid < W) {
          const long long k = wkey[tid];
          const int idx = widx[tid];
          int r = 0;
          for (int q = 0; q < W; ++q) r += (wkey[q] > k || (wkey[q] == k && widx[q] < idx)) ? 1 : 0;
          place(idx, r, k);
        }
      }
    }
    // rank by counting; the entries of rank < W are the next beam
    if (!selected)
      for (int m = tid; m < M; m += NT) {
        const long long k = ckey[m];
        const int idx = cidx[m];
        int r = 0;
#pragma unroll 8
        for (int q = 0; q < M; ++q) {  // (unrolled: the LDS reads of a batch in flight together)
          const long long kq = ckey[q];
          r += (kq > k || (kq == k && cidx[q] < idx)) ? 1 : 0;
        }
        if (r < W) place(idx, r, k);
      }
    // the next frame's candidates into the other buffer (last read a frame ago)
    if (tid < KC && t + 1 < Tb) {
      s_cls[cur ^ 1][tid] = ncls, s_sc[cur ^ 1][tid] = (double)nsc;
      if (ncls == blank) s_bpos[cur ^ 1] = tid;
    }
    nbeam = min(W, M);
    __syncthreads();
    if (nbeam == 0) break;  // (uniform: nothing survives, the utterance decodes to nothing)
  }

  if (tid == 0) s_norm = norm;
  if constexpr (ASG)
    if (tid == 0) s_norm = beam_asg_of(lm_arg...).logz ? (double)beam_asg_of(lm_arg...).logz[b] : 0.0;
  if constexpr (TOK)
    if (tid == 0 && beam_tok_of(lm_arg...).logz) s_norm = (double)beam_tok_of(lm_arg...).logz[b];
  __syncthreads();
  const BeamHyp& f = beam[Tb & 1];
  if constexpr (LM || LEX || TOK) {
    // </s>: every rank's total with the LM's end weight, a rank without one dropped, then the ranks again by counting
    // (descending, ties to the earlier rank; dropped keys are below every other and come out behind them, empty).
    // With a lexicon a rank inside a word is dropped first, and </s> needs a word LM.
    // The Transducer's rules 5 and 6 by the same ranking: the optional topology's beam as it stands (ranked by tot); the
    // forced one by pb alone, a rank whose paths all end in a token dropped.
    // Merging by spelling (section 23 rule 4): the ranks of one spelling are one result -- their scores added in rank
    // order, at the place (and with the token sequence) of the first of them whose score is finite.
    // The Transducer with a lexicon (section 25 rule 5): the lexicon's drop of a rank inside a word, the topology's
    // score, </s> on top of it.  The Transducer with a token-level LM (section 28): the topology's score, </s> on top.
    // ASG with a token-level LM (section 29): the LM search's branch as it stands -- the one mass in tot, </s> = N + 1
    // from the pack's BeamLm, then logz where the call normalises.
    if constexpr (SPELL) {
      if (tid < nbeam) spb[tid] = beam_tok_of(lm_arg...).forced ? f.pb[tid] : f.tot[tid];  // (spb: free behind the frames)
      __syncthreads();
    }
    if (tid < nbeam) {
      double s = f.tot[tid];
      if constexpr (SPELL) {
        bool owner = spb[tid] > ninf;
        s = ninf;
        for (int j = 0; j < nbeam; ++j)
          if (f.len[j] == f.len[tid] && f.hash[j] == f.hash[tid] && f.hash2[j] == f.hash2[tid]) {
            const double sj = spb[j];
            if (j < tid && sj > ninf) owner = false;
            s = beam_lae(s, sj);
          }
        if (!owner) s = ninf;
      } else if constexpr (TOK && !LEX) {
        if (beam_tok_of(lm_arg...).forced) s = f.pb[tid];
        // (section 28: </s> on top of the topology's score; a rank the forced topology drops is not looked up)
        if constexpr (LM) {
          const BeamLm& lm = beam_lm_of(lm_arg...);
          if (s > ninf && lm.score_eos) {
            int nx;
            const double l = beam_lm_step(lm, lmst[Tb & 1][tid], lm.eos, nx);
            s = l > ninf ? s + lm.alpha * l : ninf;
          }
        }
      } else if constexpr (LEX) {
        const BeamLex& lx = beam_lex_of(lm_arg...);
        if constexpr (TOK)
          if (beam_tok_of(lm_arg...).forced) s = f.pb[tid];  // (-inf: dropped below, with or without </s>)
        if constexpr (MARK) {
          // section 26 rule 5: the root (the empty sequence) as it is; a terminal node: the pending word's term and the
          // state behind it, dropped where the LM cannot follow; any other node: inside a word, dropped
          const int nd = tnode[Tb & 1][tid];
          int st = lmst[Tb & 1][tid];
          if (nd != 0) {
            const int v = beam_lex_marked_of(lm_arg...).node_word[nd];
            double l = v >= 0 ? 0.0 : ninf;
            if (v >= 0 && lx.has_lm) {
              int ns;
              l = beam_lm_step(lx.lm, st, v, ns);
              st = ns;
            }
            // (section 27 rule 4: the pending word's step settled against what its node has paid)
            if constexpr (LOOK)
              if (l > ninf) l = beam_look_settled(l, beam_look_of(lm_arg...)[nd]);
            s = l > ninf ? s + beam_lex_pending_term(lx.lm.alpha, l, lx.omega) : ninf;
          }
          if (s > ninf && lx.has_lm && lx.lm.score_eos) {
            int nx;
            const double l = beam_lm_step(lx.lm, st, lx.lm.eos, nx);
            s = l > ninf ? s + lx.lm.alpha * l : ninf;
          }
        } else if (tnode[Tb & 1][tid] != 0)
          s = ninf;
        else if (lx.has_lm && lx.lm.score_eos) {
          int nx;
          const double l = beam_lm_step(lx.lm, lmst[Tb & 1][tid], lx.lm.eos, nx);
          s = l > ninf ? s + lx.lm.alpha * l : ninf;
        }
      } else {
        const BeamLm& lm = beam_lm_of(lm_arg...);
        if (lm.score_eos) {
          int nx;
          const double l = beam_lm_step(lm, lmst[Tb & 1][tid], lm.eos, nx);
          s = l > ninf ? s + lm.alpha * l : ninf;
        }
      }
      stot[tid] = s, skey[tid] = beam_key(s);
    }
    __syncthreads();
    if (tid < max(nbeam, nbest)) {
      int r = tid;
      bool have = false;
      if (tid < nbeam) {
        const long long k = skey[tid];
        r = 0;
        for (int j = 0; j < nbeam; ++j) r += (skey[j] > k || (skey[j] == k && j < tid)) ? 1 : 0;
        have = k != kKeyDropped;
      }
      if (r < nbest) {
        const int64_t o = (int64_t)b * nbest + r;
        fin_node[o] = have ? f.node[tid] : -1;
        if constexpr (SPELL)
          fin_len[o] = have ? ntok[Tb & 1][tid] : 0;  // (the write launch walks tokens; len counts graphemes)
        else
          fin_len[o] = have ? f.len[tid] : 0;
        scores[o] = have ? (normalize ? stot[tid] - s_norm : stot[tid]) : ninf;
      }
    }
  } else if (tid < nbest) {
    const int64_t o = (int64_t)b * nbest + tid;
    const bool have = tid < nbeam;
    fin_node[o] = have ? f.node[tid] : -1;
    fin_len[o] = have ? f.len[tid] : 0;
    scores[o] = have ? (normalize ? f.tot[tid] - s_norm : f.tot[tid]) : ninf;
  }
}

// The mapping of a result on its way out (wfl_asg_beam_search; the meaning of `drop` and R = num_replabels is
// wfl_decode_paths'): labels equal to `drop` are removed, then a label v >= R becomes v - R and a replabel r < R right
// behind a label repeats that label r + 1 times, any other replabel is dropped (asg.py:35-49).  A result is walked from
// its end, so a replabel waits (`pending`) for the value before it: a label takes it, another replabel replaces it.
// Returns the mapped length; dst: NULL, or the END of the room mapped labels (stored downwards, never below it).
__device__ __forceinline__ int beam_map_walk(const int2* __restrict__ nodes, int node, int len, int TW, int drop, int R,
                                             int32_t* dst, int room) {
  int pending = -1, n = 0;
  for (int k = len - 1; k >= 0 && node >= 0 && node < TW; --k) {
    const int2 rec = nodes[node];
    const int v = rec.y;
    node = rec.x;
    if (v == drop) continue;
    if (v >= R) {
      const int copies = 1 + (pending >= 0 ? pending + 1 : 0);
      if (dst)
        for (int q = 0; q < copies && n + q < room; ++q) *--dst = v - R;
      n += copies, pending = -1;
    } else
      pending = v;
  }
  return n;
}

// a thread per (b, rank): the mapped length of the result (the write launch needs those before it for its offset)
__global__ void __launch_bounds__(256) beam_map_count_kernel(int n, int T, int W, int nbest, int drop, int R,
                                                              const int2* __restrict__ arena, const int32_t* __restrict__ fin_node,
                                                              const int32_t* __restrict__ fin_len, int32_t* __restrict__ out_len) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n) return;
  const int2* nodes = arena + (w / nbest) * (int64_t)T * W;
  out_len[w] = beam_map_walk(nodes, fin_node[w], min(max(fin_len[w], 0), T), T * W, drop, R, nullptr, 0);
}

// one wave per (b, rank): the sequences back to back in (b, rank) order.  MAP: mapped on the way (beam_map_walk), out_len
// their mapped lengths (beam_map_count_kernel's); without it the kernel is the one it was.
template <bool MAP>
__global__ void __launch_bounds__(256) beam_write_kernel(int n, int T, int W, int nbest, const int2* __restrict__ arena,
                                                          const int32_t* __restrict__ fin_node, const int32_t* __restrict__ fin_len,
                                                          int32_t* __restrict__ out, int64_t* __restrict__ out_offsets,
                                                          const int32_t* __restrict__ out_len, int drop, int R) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n) return;
  const int32_t* lens = MAP ? out_len : fin_len;
  long long base = 0;
  for (int r = lane; r < (int)w; r += 64) base += lens[r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o, 64);
  if (lane != 0) return;
  const int len = min(max(fin_len[w], 0), T);
  const int2* nodes = arena + (w / nbest) * (int64_t)T * W;
  int node = fin_node[w];
  if constexpr (MAP) {
    const int mapped = max(out_len[w], 0);
    out_offsets[w] = base;
    if (w == n - 1) out_offsets[n] = base + mapped;
    beam_map_walk(nodes, node, len, T * W, drop, R, out + base + mapped, mapped);
  } else {
    out_offsets[w] = base;
    if (w == n - 1) out_offsets[n] = base + len;
    for (int k = len - 1; k >= 0 && node >= 0 && node < T * W; --k) {
      const int2 rec = nodes[node];
      out[base + k] = rec.y;
      node = rec.x;
    }
  }
}

}  // namespace wfl

using namespace wfl;

// ------------------------------------------------------------------------------------------------------------
// The host side: one launch path (beam_run) and one set of checks (beam_check, beam_call_check) for all five
// searches.  An entry makes the checks that are its own, builds its pack and calls beam_run; a new search is a new
// pack (a struct by value, its BeamPack traits, its branches in the kernel) and such an entry.
// ------------------------------------------------------------------------------------------------------------

// the sizes of a search; R: the replabels of the mapping on the way out, by wfl_decode_workspace's rule (0: none)
static int beam_check(const char* what, int B, int T, int C, int beam, int K, int nbest, int R = 0) {
  if (B < 1 || T < 1 || C < 1 || beam < 1 || beam > kBeamMax || K < 1 || K > std::min(C, kBeamMax) || nbest < 1 || nbest > beam) {
    set_error("%s: bad arguments (B %d, T %d, C %d, beam %d, classes_per_frame %d, nbest %d)", what, B, T, C, beam, K, nbest);
    return WFL_ERR_INVALID;
  }
  if (C > kBeamMaxClasses || (int64_t)T * kBeamMax > 0x7fffffffLL || (int64_t)B * nbest > 0x7fffffffLL ||
      (int64_t)B * T > 0x7fffffffLL * 4) {
    set_error("%s: B %d, T %d, C %d is more than the beam search takes (C <= %d)", what, B, T, C, kBeamMaxClasses);
    return WFL_ERR_UNSUPPORTED;
  }
  if (R < 0) {
    set_error("%s: num_replabels %d is negative", what, R);
    return WFL_ERR_INVALID;
  }
  if ((int64_t)T * std::max(1, R) > 0x7fffffffLL) {
    set_error("%s: T %d, num_replabels %d is more than the index width of the unpacking takes", what, T, R);
    return WFL_ERR_UNSUPPORTED;
  }
  return WFL_OK;
}

// the three workspace queries (asg: its layout; R: per rank wfl_decode_workspace's T max(1, R) labels)
static int beam_workspace(const char* what, int B, int T, int C, int beam, int K, int nbest, int R, bool asg,
                          int64_t* out_capacity, int64_t* ws_bytes) {
  if (!out_capacity || !ws_bytes) {
    set_error("%s: a NULL pointer", what);
    return WFL_ERR_INVALID;
  }
  if (const int rc = beam_check(what, B, T, C, beam, K, nbest, R)) return rc;
  *out_capacity = (int64_t)B * nbest * T * std::max(1, R);
  *ws_bytes = beam_ws_layout(B, T, beam, K, nbest, asg).bytes;
  return WFL_OK;
}

// what the five entries vary in, apart from the pack; the last four as the three CTC entries have them
struct BeamCall {
  const float* x;
  const int32_t* lengths;  // or NULL
  int B, T, C;
  int blank;  // -1 with `asg`: none
  int beam, K, nbest;
  int normalize;  // as the beam kernel receives it
  void* ws;
  int32_t* out;
  int64_t out_capacity;
  int64_t* out_offsets;
  double* scores;
  void* stream;
  bool lse = true;       // the candidates launch computes the rows' log-sum-exps and the beam launch reads them
  bool asg = false;      // the ASG search: no blank; its layout of the workspace, which alone has room for a mapping
  int drop = -1, R = 0;  // the mapping on the way out; -1, 0: none, beam_write_kernel<false>
};

// what every entry refuses first, in this order; the room in `out` comes behind it, in beam_run
static int beam_call_check(const char* what, const BeamCall& c) {
  if (!c.x || !c.ws || !c.out || !c.out_offsets || !c.scores) {
    set_error("%s: a NULL pointer", what);
    return WFL_ERR_INVALID;
  }
  if (const int rc = beam_check(what, c.B, c.T, c.C, c.beam, c.K, c.nbest, c.R)) return rc;
  if (!c.asg && (c.blank < 0 || c.blank >= c.C)) {
    set_error("%s: blank %d is outside [0, %d)", what, c.blank, c.C);
    return WFL_ERR_INVALID;
  }
  if (c.drop < -1 || c.drop >= c.C) {
    set_error("%s: drop %d is outside [-1, %d)", what, c.drop, c.C);
    return WFL_ERR_INVALID;
  }
  return WFL_OK;
}

// the candidates launch (blank < 0: none, slot K stays empty; lse NULL: no row log-sum-exp)
static void beam_candidates(const float* x, const int32_t* lengths, int B, int T, int C, int blank, int K, int32_t* cls, float* sc,
                            float* lse, hipStream_t s) {
  const unsigned rows = (unsigned)(((int64_t)B * T + 3) / 4);
  auto candidates = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(rows), dim3(256), 0, s, x, lengths, B, T, C, blank, K, cls, sc, lse);
  };
  if (C <= 64)
    candidates(beam_candidates_kernel<1>);
  else if (C <= 128)
    candidates(beam_candidates_kernel<2>);
  else if (C <= 256)
    candidates(beam_candidates_kernel<4>);
  else
    candidates(beam_candidates_kernel<0>);
}

template <typename T>
static T* beam_ws_at(void* ws, int64_t offset) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + offset);
}

// A whole search: the checks every entry shares, then the launches -- candidates, beam, write (behind a count, where
// the results are mapped).  pack: nothing (the plain search), or the one struct the beam kernel takes behind its
// arguments, already checked by its entry.
template <typename... Pack>
static int beam_run(const char* what, const BeamCall& c, Pack... pack) {
  if (const int rc = beam_call_check(what, c)) return rc;
  const int B = c.B, T = c.T, W = c.beam, K = c.K, nbest = c.nbest, n = B * nbest;
  const int64_t need = (int64_t)n * T * std::max(1, c.R);
  if (c.out_capacity < need) {
    set_error("%s: out holds %lld labels, B nbest T%s = %lld are needed", what, (long long)c.out_capacity,
              c.asg ? " max(1, num_replabels)" : "", (long long)need);
    return WFL_ERR_INVALID;
  }
  const BeamWs w = beam_ws_layout(B, T, W, K, nbest, c.asg);
  int32_t* cls = beam_ws_at<int32_t>(c.ws, w.cls);
  float* sc = beam_ws_at<float>(c.ws, w.sc);
  float* lse = c.lse ? beam_ws_at<float>(c.ws, w.lse) : nullptr;
  int2* arena = beam_ws_at<int2>(c.ws, w.arena);
  int32_t* fin_node = beam_ws_at<int32_t>(c.ws, w.fin_node);
  int32_t* fin_len = beam_ws_at<int32_t>(c.ws, w.fin_len);
  int32_t* out_len = c.asg ? beam_ws_at<int32_t>(c.ws, w.out_len) : nullptr;
  hipStream_t s = (hipStream_t)c.stream;
  beam_candidates(c.x, c.lengths, B, T, c.C, c.blank, K, cls, sc, lse, s);
  WFL_LAUNCH_CHECK();
  if (W * (K + 2) <= 1024)
    hipLaunchKernelGGL((beam_search_kernel<256, Pack...>), dim3(B), dim3(256), 0, s, c.lengths, T, c.blank, W, K, nbest, c.normalize,
                       cls, sc, lse, arena, fin_node, fin_len, c.scores, pack...);
  else
    hipLaunchKernelGGL((beam_search_kernel<1024, Pack...>), dim3(B), dim3(1024), 0, s, c.lengths, T, c.blank, W, K, nbest, c.normalize,
                       cls, sc, lse, arena, fin_node, fin_len, c.scores, pack...);
  WFL_LAUNCH_CHECK();
  const dim3 waves((unsigned)((n + 3) / 4));
  if (c.drop < 0 && c.R == 0) {  // the raw class sequences: the write launch as it is
    hipLaunchKernelGGL(beam_write_kernel<false>, waves, dim3(256), 0, s, n, T, W, nbest, arena, fin_node, fin_len, c.out,
                       c.out_offsets, (const int32_t*)nullptr, -1, 0);
  } else {  // count first, then store: a result is walked from its end
    hipLaunchKernelGGL(beam_map_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, T, W, nbest, c.drop, c.R, arena,
                       fin_node, fin_len, out_len);
    WFL_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_write_kernel<true>, waves, dim3(256), 0, s, n, T, W, nbest, arena, fin_node, fin_len, c.out,
                       c.out_offsets, (const int32_t*)out_len, c.drop, c.R);
  }
  WFL_LAUNCH_CHECK();
  return WFL_OK;
}

// What the seven Transducer entries do first, in this order: the call (no lengths; with transitions logz normalises,
// not the rows), beam_call_check, the topology's flag -- beam_tok_call --, then the denominator's rule and the
// transitions of the launch -- beam_tok_terms.  Two halves, since wfl_transducer_beam_search_merged refuses a NULL
// spelling table between them.
struct BeamTokCall {
  BeamCall c;
  BeamTok tok;
};
static int beam_tok_call(const char* what, const float* x, const float* Wt, int B, int T, int C, int blank, int forced, int beam, int K,
                         int nbest, int normalize, void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets, double* scores,
                         void* stream, BeamTokCall* p) {
  p->c = BeamCall{x, nullptr, B, T, C, blank, beam, K, nbest, normalize, ws, out, out_capacity, out_offsets, scores, stream, !Wt};
  // (beam_run makes this check again: an entry's own have always come behind it and ahead of the room in `out`)
  if (const int rc = beam_call_check(what, p->c)) return rc;
  if (forced != 0 && forced != 1) {
    set_error("%s: forced %d is neither 0 nor 1", what, forced);
    return WFL_ERR_INVALID;
  }
  return WFL_OK;
}
static int beam_tok_terms(const char* what, const float* Wt, const float* logz, int forced, BeamTokCall* p) {
  if ((Wt != nullptr) != (logz != nullptr) && (p->c.normalize || logz)) {
    set_error("%s: normalised scores need logz with transitions, and logz belongs to transitions only", what);
    return WFL_ERR_INVALID;
  }
  p->tok = BeamTok{Wt, p->c.normalize ? logz : nullptr, p->c.C, forced};
  return WFL_OK;
}
static int beam_tok_prelude(const char* what, const float* x, const float* Wt, const float* logz, int B, int T, int C, int blank,
                            int forced, int beam, int K, int nbest, int normalize, void* ws, int32_t* out, int64_t out_capacity,
                            int64_t* out_offsets, double* scores, void* stream, BeamTokCall* p) {
  if (const int rc = beam_tok_call(what, x, Wt, B, T, C, blank, forced, beam, K, nbest, normalize, ws, out, out_capacity, out_offsets,
                                   scores, stream, p))
    return rc;
  return beam_tok_terms(what, Wt, logz, forced, p);
}

// CTC's topology runs CTC's search: without transitions and with the optional blank a Transducer entry's rules are its
// CTC sibling's without lengths, and that sibling's kernel is the one that runs -- with the sibling's pack `ctc` (none:
// the plain search); otherwise the entry's own, with `tok`
template <typename Tok, typename... Ctc>
static int beam_run_tok(const char* what, const BeamTokCall& p, const Tok& tok, const Ctc&... ctc) {
  if (!p.tok.Wt && !p.tok.forced) return beam_run(what, p.c, ctc...);
  return beam_run(what, p.c, tok);
}

extern "C" {

// The beam search of the ASG criterion (asg.py:54-69: the transitions; asg.py:72-115: the score of a label sequence, the
// force-align numerator, and the denominator logz; asg.py:35-49, 225-234: what viterbi() does to a result).  The
// reference has no such search: it is an addition, like wfl_ctc_beam_search.
int wfl_asg_beam_workspace(int B, int T, int C, int beam, int classes_per_frame, int nbest, int num_replabels,
                           int64_t* out_capacity, int64_t* ws_bytes) {
  return beam_workspace("asg_beam_workspace", B, T, C, beam, classes_per_frame, nbest, num_replabels, true, out_capacity, ws_bytes);
}

int wfl_asg_beam_search(const float* x, const float* Wt, const float* logz, int B, int T, int C, int beam, int classes_per_frame,
                        int nbest, int drop, int num_replabels, void* ws, int32_t* out, int64_t out_capacity,
                        int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "asg_beam_search";
  if (!Wt) {
    set_error("%s: a NULL pointer", what);
    return WFL_ERR_INVALID;
  }
  // no blank, no lengths, no row log-sum-exp: ASG has none of them, and normalises by the pack's logz
  const BeamCall c{x, nullptr, B, T, C, -1, beam, classes_per_frame, nbest, logz ? 1 : 0, ws, out, out_capacity, out_offsets,
                   scores, stream, false, true, drop, num_replabels};
  return beam_run(what, c, BeamAsg{Wt, logz, C});
}

// The beam search of the Transducer criterion.  The reference has no such search: an addition.
int wfl_transducer_beam_workspace(int B, int T, int C, int beam, int classes_per_frame, int nbest, int64_t* out_capacity,
                                  int64_t* ws_bytes) {
  // (the plain search's layout: it may be the one that runs)
  return beam_workspace("transducer_beam_workspace", B, T, C, beam, classes_per_frame, nbest, 0, false, out_capacity, ws_bytes);
}

int wfl_transducer_beam_search(const float* x, const float* Wt, const float* logz, int B, int T, int C, int blank, int forced,
                               int beam, int classes_per_frame, int nbest, int normalize, void* ws, int32_t* out,
                               int64_t out_capacity, int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "transducer_beam_search";
  BeamTokCall p;
  if (const int rc = beam_tok_prelude(what, x, Wt, logz, B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize, ws, out,
                                      out_capacity, out_offsets, scores, stream, &p))
    return rc;
  return beam_run_tok(what, p, p.tok);  // (CTC's side: section 17's rules, the plain search)
}

int wfl_spelling_check(const int32_t* spell_ptr, const int32_t* spell_sym, int C, int blank) {
  const char* what = "spelling_check";
  if (!spell_ptr || !spell_sym) {
    set_error("%s: a NULL pointer", what);
    return WFL_ERR_INVALID;
  }
  if (C < 1 || blank < 0 || blank >= C) {
    set_error("%s: %d classes, blank %d", what, C, blank);
    return WFL_ERR_INVALID;
  }
  if (spell_ptr[0] != 0) {
    set_error("%s: spell_ptr starts at %d, not at 0", what, spell_ptr[0]);
    return WFL_ERR_INVALID;
  }
  for (int c = 0; c < C; ++c) {  // (every range before any symbol: nothing is read outside [0, spell_ptr[C]))
    const int64_t n = (int64_t)spell_ptr[c + 1] - spell_ptr[c];
    if (n < 0) {
      set_error("%s: spell_ptr descends at class %d", what, c);
      return WFL_ERR_INVALID;
    }
    if (c == blank ? n != 0 : (n < 1 || n > WFL_SPELL_MAX)) {
      if (c == blank)
        set_error("%s: the blank %d spells %lld graphemes, not none", what, c, (long long)n);
      else
        set_error("%s: class %d spells %lld graphemes, not 1 .. %d", what, c, (long long)n, WFL_SPELL_MAX);
      return WFL_ERR_INVALID;
    }
  }
  for (int c = 0; c < C; ++c)
    for (int q = spell_ptr[c]; q < spell_ptr[c + 1]; ++q)
      if (spell_sym[q] < 0) {
        set_error("%s: grapheme %d of class %d is %d (graphemes are >= 0)", what, q - spell_ptr[c], c, spell_sym[q]);
        return WFL_ERR_INVALID;
      }
  return WFL_OK;
}

// The Transducer search with hypotheses merged by spelling: wfl_transducer_beam_search's checks
// in its order, then this entry's own; always the BeamSpell kernel, also where the plain search would do.
int wfl_transducer_beam_search_merged(const float* x, const float* Wt, const float* logz, const int32_t* spell_ptr,
                                      const int32_t* spell_sym, int B, int T, int C, int blank, int forced, int beam,
                                      int classes_per_frame, int nbest, int normalize, void* ws, int32_t* out,
                                      int64_t out_capacity, int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "transducer_beam_search_merged";
  BeamTokCall p;
  if (const int rc = beam_tok_call(what, x, Wt, B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize, ws, out,
                                   out_capacity, out_offsets, scores, stream, &p))
    return rc;
  if (!spell_ptr || !spell_sym) {
    set_error("%s: a NULL spelling table", what);
    return WFL_ERR_INVALID;
  }
  if (const int rc = beam_tok_terms(what, Wt, logz, forced, &p)) return rc;
  return beam_run(what, p.c, BeamSpell{p.tok, spell_ptr, spell_sym});
}

int wfl_ctc_beam_workspace(int B, int T, int C, int beam, int classes_per_frame, int nbest, int64_t* out_capacity,
                           int64_t* ws_bytes) {
  return beam_workspace("ctc_beam_workspace", B, T, C, beam, classes_per_frame, nbest, 0, false, out_capacity, ws_bytes);
}

int wfl_ctc_beam_search(const float* x, const int32_t* lengths, int B, int T, int C, int blank, int beam, int classes_per_frame,
                        int nbest, int normalize, void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets,
                        double* scores, void* stream) {
  return beam_run("ctc_beam_search", {x, lengths, B, T, C, blank, beam, classes_per_frame, nbest, normalize, ws, out, out_capacity,
                                      out_offsets, scores, stream});
}

static int ngram_lm_shape(const char* what, const wfl_ngram_lm* lm) {
  if (!lm || !lm->arc_ptr || !lm->arc_label || !lm->arc_next || !lm->arc_w || !lm->bo_next || !lm->bo_w) {
    set_error("%s: a NULL language model or array of it", what);
    return WFL_ERR_INVALID;
  }
  if (lm->num_states < 1 || lm->num_arcs < 0 || lm->start < 0 || lm->start >= lm->num_states) {
    set_error("%s: a language model of %d states, %d arcs, start %d", what, lm->num_states, lm->num_arcs, lm->start);
    return WFL_ERR_INVALID;
  }
  return WFL_OK;
}

int wfl_ngram_lm_check(wfl_ngram_lm* lm, int C, int blank) {
  const char* what = "ngram_lm_check";
  if (const int rc = ngram_lm_shape(what, lm)) return rc;
  if (C < 1 || blank < 0 || blank >= C) {
    set_error("%s: %d classes, blank %d", what, C, blank);
    return WFL_ERR_INVALID;
  }
  const int S = lm->num_states, A = lm->num_arcs;
  if (lm->arc_ptr[0] != 0 || lm->arc_ptr[S] != A) {
    set_error("%s: arc_ptr runs from %d to %d, not from 0 to %d", what, lm->arc_ptr[0], lm->arc_ptr[S], A);
    return WFL_ERR_INVALID;
  }
  for (int s = 0; s < S; ++s)
    if (lm->arc_ptr[s] > lm->arc_ptr[s + 1] || lm->arc_ptr[s] < 0 || lm->arc_ptr[s + 1] > A) {
      set_error("%s: arc_ptr descends or leaves [0, %d] at state %d", what, A, s);
      return WFL_ERR_INVALID;
    }
  for (int s = 0; s < S; ++s) {
    for (int a = lm->arc_ptr[s]; a < lm->arc_ptr[s + 1]; ++a) {
      const int l = lm->arc_label[a];
      if (l < 0 || l > C || l == blank) {
        set_error("%s: arc %d of state %d has label %d (classes [0, %d), %d for </s>, never the blank %d)", what, a, s, l, C, C,
                  blank);
        return WFL_ERR_INVALID;
      }
      if (a > lm->arc_ptr[s] && lm->arc_label[a - 1] >= l) {
        set_error("%s: the labels of state %d are not strictly ascending at arc %d", what, s, a);
        return WFL_ERR_INVALID;
      }
      if (lm->arc_next[a] < 0 || lm->arc_next[a] >= S) {
        set_error("%s: arc %d of state %d leads to state %d of %d", what, a, s, lm->arc_next[a], S);
        return WFL_ERR_INVALID;
      }
      if (!(lm->arc_w[a] < __builtin_inf())) {  // (NaN or +inf)
        set_error("%s: arc %d of state %d has a weight that is NaN or +inf", what, a, s);
        return WFL_ERR_INVALID;
      }
    }
    if (lm->bo_next[s] < -1 || lm->bo_next[s] >= S) {
      set_error("%s: state %d backs off to state %d of %d", what, s, lm->bo_next[s], S);
      return WFL_ERR_INVALID;
    }
    if (lm->bo_next[s] >= 0 && !(lm->bo_w[s] < __builtin_inf())) {
      set_error("%s: state %d has a back-off weight that is NaN or +inf", what, s);
      return WFL_ERR_INVALID;
    }
  }
  for (int s = 0; s < S; ++s) {  // a chain longer than the cap: too deep or a cycle, refused alike
    int t = s, depth = 0;
    while (lm->bo_next[t] >= 0 && depth <= WFL_NGRAM_LM_MAX_BACKOFF) t = lm->bo_next[t], ++depth;
    if (depth > WFL_NGRAM_LM_MAX_BACKOFF) {
      set_error("%s: the back-off chain of state %d is cyclic or deeper than %d", what, s, WFL_NGRAM_LM_MAX_BACKOFF);
      return WFL_ERR_INVALID;
    }
  }
  {  // the bounds of step(), written into the struct: an arc weight and at most the cap's number of back-off weights
    double lo = __builtin_inf(), hi = -__builtin_inf(), blo = 0.0, bhi = 0.0;
    for (int a = 0; a < A; ++a) lo = fmin(lo, lm->arc_w[a]), hi = fmax(hi, lm->arc_w[a]);
    for (int s = 0; s < S; ++s)
      if (lm->bo_next[s] >= 0) blo = fmin(blo, lm->bo_w[s]), bhi = fmax(bhi, lm->bo_w[s]);
    lo += WFL_NGRAM_LM_MAX_BACKOFF * blo, hi += WFL_NGRAM_LM_MAX_BACKOFF * bhi;
    lm->step_min = A > 0 ? lo : 0.0, lm->step_max = A > 0 ? hi : 0.0;
  }
  return WFL_OK;
}

// The LM terms of a launch, for the two entries below: the shape of `lm` and its step bounds checked (none, where the
// entry allows that: the lexicon search without a word LM, whose step is 0 and whose arrays are not read), and `d`
// filled from it and the call's scalars -- all but d->bound, which each entry forms by its own expression.
static int beam_lm_terms(const char* what, const wfl_ngram_lm* lm, bool optional, int eos, double alpha, double beta,
                         int score_eos, BeamLm* d) {
  if (lm || !optional) {
    if (const int rc = ngram_lm_shape(what, lm)) return rc;
    if (lm->step_min != lm->step_min || lm->step_max != lm->step_max) {
      set_error("%s: the language model's step_min or step_max is NaN", what);
      return WFL_ERR_INVALID;
    }
  }
  const wfl_ngram_lm none = {}, &m = lm ? *lm : none;  // (none: null arrays, start 0)
  d->arc_ptr = m.arc_ptr, d->arc_label = m.arc_label, d->arc_next = m.arc_next, d->bo_next = m.bo_next;
  d->arc_w = m.arc_w, d->bo_w = m.bo_w;
  d->start = m.start, d->eos = eos, d->alpha = alpha, d->beta = beta, d->score_eos = score_eos ? 1 : 0;
  return WFL_OK;
}

int wfl_ctc_beam_search_lm(const float* x, const int32_t* lengths, int B, int T, int C, int blank, int beam,
                           int classes_per_frame, int nbest, int normalize, const wfl_ngram_lm* lm, double lm_weight,
                           double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                           int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "ctc_beam_search_lm";
  BeamLm d;
  if (const int rc = beam_lm_terms(what, lm, false, C, lm_weight, length_bonus, score_eos, &d)) return rc;
  if (!(fabs(lm_weight) < __builtin_inf()) || !(fabs(length_bonus) < __builtin_inf())) {
    set_error("%s: lm_weight %g and length_bonus %g must be finite", what, lm_weight, length_bonus);
    return WFL_ERR_INVALID;
  }
  // the largest LM term of an extension, by the operations the kernel forms a term with (0 * inf: no bound)
  const double t0 = lm_weight * lm->step_min, t1 = lm_weight * lm->step_max;
  d.bound = (t0 != t0 || t1 != t1) ? __builtin_inf() : fmax(t0, t1) + length_bonus;
  return beam_run(what, {x, lengths, B, T, C, blank, beam, classes_per_frame, nbest, normalize, ws, out, out_capacity, out_offsets,
                         scores, stream}, d);
}

// The Transducer search with a token-level n-gram LM: wfl_transducer_beam_search's call and checks
// in its order, then wfl_ctc_beam_search_lm's checks of the LM and the two scalars.
int wfl_transducer_beam_search_lm(const float* x, const float* Wt, const float* logz, int B, int T, int C, int blank, int forced,
                                  int beam, int classes_per_frame, int nbest, int normalize, const wfl_ngram_lm* lm,
                                  double lm_weight, double length_bonus, int score_eos, void* ws, int32_t* out,
                                  int64_t out_capacity, int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "transducer_beam_search_lm";
  BeamTokCall p;
  if (const int rc = beam_tok_prelude(what, x, Wt, logz, B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize, ws, out,
                                      out_capacity, out_offsets, scores, stream, &p))
    return rc;
  BeamTokLm d;
  if (const int rc = beam_lm_terms(what, lm, false, C, lm_weight, length_bonus, score_eos, &d.lm)) return rc;
  if (!(fabs(lm_weight) < __builtin_inf()) || !(fabs(length_bonus) < __builtin_inf())) {
    set_error("%s: lm_weight %g and length_bonus %g must be finite", what, lm_weight, length_bonus);
    return WFL_ERR_INVALID;
  }
  d.lm.bound = beam_tok_lm_bound(lm_weight, lm->step_min, lm->step_max, length_bonus);
  d.tok = p.tok;
  return beam_run_tok(what, p, d, d.lm);  // (CTC's side: section 18's rules without lengths)
}

static int lexicon_shape(const char* what, const wfl_lexicon* lex) {
  if (!lex || !lex->arc_ptr || !lex->arc_label || !lex->arc_next) {
    set_error("%s: a NULL lexicon or array of it", what);
    return WFL_ERR_INVALID;
  }
  if (lex->num_nodes < 1 || lex->num_arcs < 1 || lex->num_words < 1 || lex->num_words == 0x7fffffff) {  // (</s> is V + 1)
    set_error("%s: a lexicon of %d nodes, %d arcs, %d words", what, lex->num_nodes, lex->num_arcs, lex->num_words);
    return WFL_ERR_INVALID;
  }
  return WFL_OK;
}

int wfl_lexicon_check(const wfl_lexicon* lex, int C, int blank) {
  const char* what = "lexicon_check";
  if (const int rc = lexicon_shape(what, lex)) return rc;
  if (C < 1 || blank < 0 || blank >= C) {
    set_error("%s: %d classes, blank %d", what, C, blank);
    return WFL_ERR_INVALID;
  }
  const int N = lex->num_nodes, A = lex->num_arcs, V = lex->num_words;
  if (lex->arc_ptr[0] != 0 || lex->arc_ptr[N] != A) {
    set_error("%s: arc_ptr runs from %d to %d, not from 0 to %d", what, lex->arc_ptr[0], lex->arc_ptr[N], A);
    return WFL_ERR_INVALID;
  }
  for (int n = 0; n < N; ++n) {
    if (lex->arc_ptr[n] > lex->arc_ptr[n + 1] || lex->arc_ptr[n] < 0 || lex->arc_ptr[n + 1] > A) {
      set_error("%s: arc_ptr descends or leaves [0, %d] at node %d", what, A, n);
      return WFL_ERR_INVALID;
    }
    if (lex->arc_ptr[n] == lex->arc_ptr[n + 1]) {
      set_error("%s: node %d has no arc (a dead end)", what, n);
      return WFL_ERR_INVALID;
    }
  }
  std::vector<char> entered((size_t)N, 0), spelled((size_t)V, 0);
  for (int n = 0; n < N; ++n)
    for (int a = lex->arc_ptr[n]; a < lex->arc_ptr[n + 1]; ++a) {
      const int l = lex->arc_label[a], nx = lex->arc_next[a];
      if (l < 0 || l >= C || l == blank) {
        set_error("%s: arc %d of node %d has label %d (classes [0, %d), never the blank %d)", what, a, n, l, C, blank);
        return WFL_ERR_INVALID;
      }
      if (a > lex->arc_ptr[n] && lex->arc_label[a - 1] >= l) {
        set_error("%s: the labels of node %d are not strictly ascending at arc %d", what, n, a);
        return WFL_ERR_INVALID;
      }
      if (nx >= 0) {
        if (nx < 1 || nx >= N) {
          set_error("%s: arc %d of node %d leads to node %d (inner nodes are 1 .. %d)", what, a, n, nx, N - 1);
          return WFL_ERR_INVALID;
        }
        if (entered[(size_t)nx]) {
          set_error("%s: node %d is the target of more than one arc (arc %d is the second)", what, nx, a);
          return WFL_ERR_INVALID;
        }
        entered[(size_t)nx] = 1;
      } else {
        const int64_t v = -((int64_t)nx + 1);
        if (v >= V) {
          set_error("%s: arc %d of node %d completes word %lld of %d", what, a, n, (long long)v, V);
          return WFL_ERR_INVALID;
        }
        if (spelled[(size_t)v]) {
          set_error("%s: word %lld is completed by more than one arc (arc %d is the second)", what, (long long)v, a);
          return WFL_ERR_INVALID;
        }
        spelled[(size_t)v] = 1;
      }
    }
  for (int n = 1; n < N; ++n)
    if (!entered[(size_t)n]) {
      set_error("%s: node %d is the target of no arc", what, n);
      return WFL_ERR_INVALID;
    }
  for (int v = 0; v < V; ++v)
    if (!spelled[(size_t)v]) {
      set_error("%s: word %d is completed by no arc", what, v);
      return WFL_ERR_INVALID;
    }
  {  // one arc into every inner node still allows a cycle apart from the root: every node must be reached from it
    std::vector<int> stack(1, 0);
    int reached = 0;
    while (!stack.empty()) {
      const int n = stack.back();
      stack.pop_back();
      ++reached;
      for (int a = lex->arc_ptr[n]; a < lex->arc_ptr[n + 1]; ++a)
        if (lex->arc_next[a] >= 0) stack.push_back(lex->arc_next[a]);
    }
    if (reached != N) {
      set_error("%s: %d of %d nodes are reached from the root: the rest form a cycle", what, reached, N);
      return WFL_ERR_INVALID;
    }
  }
  return WFL_OK;
}

// The lexicon of a launch, for the entries below: the shape of `lex`, the word LM's terms (beam_lm_terms) and the three
// constants checked, in that order, and `d` filled from them -- the bound of an extension's term included.
static int beam_lex_fill(const char* what, const wfl_lexicon* lex, const wfl_ngram_lm* word_lm, double lm_weight,
                         double word_bonus, double length_bonus, int score_eos, BeamLex* d) {
  if (const int rc = lexicon_shape(what, lex)) return rc;
  // word v is LM label v, the LM's unused blank is V and </s> is V + 1
  if (const int rc = beam_lm_terms(what, word_lm, true, lex->num_words + 1, lm_weight, length_bonus, score_eos, &d->lm)) return rc;
  if (!(fabs(lm_weight) < __builtin_inf()) || !(fabs(word_bonus) < __builtin_inf()) || !(fabs(length_bonus) < __builtin_inf())) {
    set_error("%s: lm_weight %g, word_bonus %g and length_bonus %g must be finite", what, lm_weight, word_bonus, length_bonus);
    return WFL_ERR_INVALID;
  }
  d->arc_ptr = lex->arc_ptr, d->arc_label = lex->arc_label, d->arc_next = lex->arc_next;
  d->has_lm = word_lm ? 1 : 0;
  d->omega = word_bonus;
  // (without a word LM every word's step is 0: the bounds of step are [0, 0])
  d->bound = beam_lex_bound(lm_weight, word_lm ? word_lm->step_min : 0.0, word_lm ? word_lm->step_max : 0.0, word_bonus, length_bonus);
  d->lm.bound = d->bound;
  return WFL_OK;
}

static int lexicon_marked_shape(const char* what, const wfl_lexicon_marked* lex) {
  if (!lex) {
    set_error("%s: a NULL lexicon or array of it", what);
    return WFL_ERR_INVALID;
  }
  if (const int rc = lexicon_shape(what, &lex->trie)) return rc;
  if (!lex->node_word || !lex->start_node) {
    set_error("%s: a NULL lexicon or array of it", what);
    return WFL_ERR_INVALID;
  }
  return WFL_OK;
}

// Every clause of rule 1 of DESIGN.md section 26, on host arrays: arc_ptr is read first, then nothing outside
// [0, num_arcs), [0, num_nodes) and [0, C).
int wfl_lexicon_marked_check(const wfl_lexicon_marked* lex, int C, int blank) {
  const char* what = "lexicon_marked_check";
  if (const int rc = lexicon_marked_shape(what, lex)) return rc;
  if (C < 1 || blank < 0 || blank >= C) {
    set_error("%s: %d classes, blank %d", what, C, blank);
    return WFL_ERR_INVALID;
  }
  const wfl_lexicon& t = lex->trie;
  const int N = t.num_nodes, A = t.num_arcs, V = t.num_words;
  if (t.arc_ptr[0] != 0 || t.arc_ptr[N] != A) {
    set_error("%s: arc_ptr runs from %d to %d, not from 0 to %d", what, t.arc_ptr[0], t.arc_ptr[N], A);
    return WFL_ERR_INVALID;
  }
  for (int n = 0; n < N; ++n)
    if (t.arc_ptr[n] > t.arc_ptr[n + 1] || t.arc_ptr[n] < 0 || t.arc_ptr[n + 1] > A) {
      set_error("%s: arc_ptr descends or leaves [0, %d] at node %d", what, A, n);
      return WFL_ERR_INVALID;
    }
  std::vector<char> entered((size_t)N, 0), spelled((size_t)V, 0), starts((size_t)C, 0);
  for (int n = 0; n < N; ++n)
    for (int a = t.arc_ptr[n]; a < t.arc_ptr[n + 1]; ++a) {
      const int l = t.arc_label[a], nx = t.arc_next[a];
      if (l < 0 || l >= C || l == blank) {
        set_error("%s: arc %d of node %d has label %d (classes [0, %d), never the blank %d)", what, a, n, l, C, blank);
        return WFL_ERR_INVALID;
      }
      if (a > t.arc_ptr[n] && t.arc_label[a - 1] >= l) {
        set_error("%s: the labels of node %d are not strictly ascending at arc %d", what, n, a);
        return WFL_ERR_INVALID;
      }
      if (nx < 1 || nx >= N) {
        set_error("%s: arc %d of node %d leads to node %d (targets are 1 .. %d)", what, a, n, nx, N - 1);
        return WFL_ERR_INVALID;
      }
      if (entered[(size_t)nx]) {
        set_error("%s: node %d is the target of more than one arc (arc %d is the second)", what, nx, a);
        return WFL_ERR_INVALID;
      }
      entered[(size_t)nx] = 1;
      if (n == 0) starts[(size_t)l] = 1;
    }
  for (int n = 1; n < N; ++n)
    if (!entered[(size_t)n]) {
      set_error("%s: node %d is the target of no arc", what, n);
      return WFL_ERR_INVALID;
    }
  {  // one arc into every other node still allows a cycle apart from the root: every node must be reached from it
    std::vector<int> stack(1, 0);
    int reached = 0;
    while (!stack.empty()) {
      const int n = stack.back();
      stack.pop_back();
      ++reached;
      for (int a = t.arc_ptr[n]; a < t.arc_ptr[n + 1]; ++a) stack.push_back(t.arc_next[a]);
    }
    if (reached != N) {
      set_error("%s: %d of %d nodes are reached from the root: the rest form a cycle", what, reached, N);
      return WFL_ERR_INVALID;
    }
  }
  for (int n = 0; n < N; ++n) {
    const int v = lex->node_word[n];
    if (v < -1 || v >= V) {
      set_error("%s: node %d ends word %d of %d", what, n, v, V);
      return WFL_ERR_INVALID;
    }
    if (n == 0 && v >= 0) {
      set_error("%s: the root ends word %d (no word has an empty spelling)", what, v);
      return WFL_ERR_INVALID;
    }
    if (v < 0 && t.arc_ptr[n] == t.arc_ptr[n + 1]) {
      set_error("%s: node %d has no arc and ends no word (a dead end)", what, n);
      return WFL_ERR_INVALID;
    }
    if (v >= 0) spelled[(size_t)v] = 1;
  }
  for (int v = 0; v < V; ++v)
    if (!spelled[(size_t)v]) {
      set_error("%s: word %d ends at no node", what, v);
      return WFL_ERR_INVALID;
    }
  for (int c = 0; c < C; ++c) {  // start_node against the root's arcs (labels ascending: the one arc by c, if any)
    int child = -1;
    for (int a = t.arc_ptr[0]; a < t.arc_ptr[1]; ++a)
      if (t.arc_label[a] == c) child = t.arc_next[a];
    if (lex->start_node[c] != child) {
      set_error("%s: start_node[%d] is %d, the root's child by class %d is %d", what, c, lex->start_node[c], c, child);
      return WFL_ERR_INVALID;
    }
  }
  for (int n = 1; n < N; ++n)
    for (int a = t.arc_ptr[n]; a < t.arc_ptr[n + 1]; ++a)
      if (starts[(size_t)t.arc_label[a]]) {
        set_error("%s: class %d starts a word and is the label of arc %d of node %d inside one", what, t.arc_label[a], a, n);
        return WFL_ERR_INVALID;
      }
  return WFL_OK;
}

// What both look-ahead checks share (DESIGN.md section 27 rule 6): the lexicon's CSR inside its arrays -- so that nothing
// is read outside [0, num_arcs) and [0, num_nodes) --, node_look finite with 0 at the root, then the three ranges.
// node_word: a start-marked lexicon's (every arc inner, a word completes at a terminal node), or NULL.
static int lexicon_lookahead_check(const char* what, const wfl_lexicon* lex, const int32_t* node_word, wfl_lexicon_lookahead* look) {
  if (!look || !look->node_look) {
    set_error("%s: a NULL look-ahead or node_look", what);
    return WFL_ERR_INVALID;
  }
  const int N = lex->num_nodes, A = lex->num_arcs;
  if (lex->arc_ptr[0] != 0 || lex->arc_ptr[N] != A) {
    set_error("%s: arc_ptr runs from %d to %d, not from 0 to %d", what, lex->arc_ptr[0], lex->arc_ptr[N], A);
    return WFL_ERR_INVALID;
  }
  for (int n = 0; n < N; ++n)
    if (lex->arc_ptr[n] > lex->arc_ptr[n + 1] || lex->arc_ptr[n] < 0 || lex->arc_ptr[n + 1] > A) {
      set_error("%s: arc_ptr descends or leaves [0, %d] at node %d", what, A, n);
      return WFL_ERR_INVALID;
    }
  for (int a = 0; a < A; ++a)
    if (lex->arc_next[a] >= N || (node_word && lex->arc_next[a] < 1)) {
      set_error("%s: arc %d leads to node %d of %d", what, a, lex->arc_next[a], N);
      return WFL_ERR_INVALID;
    }
  const double* L = look->node_look;
  for (int n = 0; n < N; ++n)
    if (!(fabs(L[n]) < __builtin_inf())) {
      set_error("%s: node_look[%d] is not finite", what, n);
      return WFL_ERR_INVALID;
    }
  if (L[0] != 0.0) {
    set_error("%s: node_look[0] is %g, the root's look-ahead is 0", what, L[0]);
    return WFL_ERR_INVALID;
  }
  const double inf = __builtin_inf();
  double arc_min = inf, arc_max = -inf, end_min = inf, end_max = -inf, start_min = inf, start_max = -inf;
  for (int n = 0; n < N; ++n) {
    bool ends = node_word && node_word[n] >= 0;
    for (int a = lex->arc_ptr[n]; a < lex->arc_ptr[n + 1]; ++a) {
      const int m = lex->arc_next[a];
      if (m < 0) {
        ends = true;
        continue;
      }
      // (the difference as the kernel forms it: beam_look_inner_term's first operation; a marked root arc: L[m] - 0)
      const double d = beam_look_arc_diff(L[m], (node_word && n == 0) ? 0.0 : L[n]);
      arc_min = fmin(arc_min, d), arc_max = fmax(arc_max, d);
      if (node_word && n == 0) start_min = fmin(start_min, L[m]), start_max = fmax(start_max, L[m]);
    }
    if (ends) end_min = fmin(end_min, L[n]), end_max = fmax(end_max, L[n]);
  }
  // (a range nothing fell into -- a lexicon of one-label words has no inner arc --: [0, 0], which bounds nothing away)
  if (arc_min > arc_max) arc_min = arc_max = 0.0;
  if (end_min > end_max) end_min = end_max = 0.0;
  if (start_min > start_max) start_min = start_max = 0.0;
  look->arc_min = arc_min, look->arc_max = arc_max, look->end_min = end_min, look->end_max = end_max;
  look->start_min = start_min, look->start_max = start_max;
  return WFL_OK;
}

int wfl_lexicon_lookahead_check(const wfl_lexicon* lex, wfl_lexicon_lookahead* look) {
  const char* what = "lexicon_lookahead_check";
  if (const int rc = lexicon_shape(what, lex)) return rc;
  return lexicon_lookahead_check(what, lex, nullptr, look);
}

int wfl_lexicon_marked_lookahead_check(const wfl_lexicon_marked* lex, wfl_lexicon_lookahead* look) {
  const char* what = "lexicon_marked_lookahead_check";
  if (const int rc = lexicon_marked_shape(what, lex)) return rc;
  return lexicon_lookahead_check(what, &lex->trie, lex->node_word, look);
}

// The largest term of an extension with look-ahead (section 27 rule 6), by the operations the kernel forms a term with:
// an inner arc's (alpha d) + beta with d in [arc_min, arc_max]; a completed word's ((alpha (l - L) + omega) + beta) + alpha S
// with l in [step_min, step_max], L in [end_min, end_max], S in [start_min, start_max] (0, 0 end-marked: + 0 changes
// nothing).  Every rounded operation is monotone in each argument, a product with a constant in one direction or the
// other: its largest value is at an end of the range.  A NaN on the way (0 inf, inf - inf): no bound.
static double beam_look_bound(double alpha, double step_min, double step_max, double omega, double beta,
                              const wfl_lexicon_lookahead& k) {
#pragma clang fp contract(off)
  const double i0 = alpha * k.arc_min, i1 = alpha * k.arc_max;
  const double lo = step_min - k.end_max, hi = step_max - k.end_min;
  const double w0 = alpha * lo, w1 = alpha * hi;
  const double s0 = alpha * k.start_min, s1 = alpha * k.start_max;
  const double inner = fmax(i0, i1) + beta;
  const double mo = fmax(w0, w1) + omega;
  const double mb = mo + beta;
  const double word = mb + fmax(s0, s1);
  // (fmax drops a NaN operand: every product and difference is tested itself)
  if (i0 != i0 || i1 != i1 || lo != lo || hi != hi || w0 != w0 || w1 != w1 || s0 != s0 || s1 != s1 || inner != inner ||
      word != word)
    return __builtin_inf();
  return fmax(inner, word);
}

// What the four look-ahead entries check behind their sibling's checks and beam_lex_fill, and the bound they replace
static int beam_look_fill(const char* what, const wfl_lexicon_lookahead* look, const wfl_ngram_lm* word_lm, BeamLex* d) {
  if (!look || !look->node_look) {
    set_error("%s: a NULL look-ahead or node_look", what);
    return WFL_ERR_INVALID;
  }
  if (!(look->arc_min <= look->arc_max) || !(look->end_min <= look->end_max) || !(look->start_min <= look->start_max)) {
    set_error("%s: a range of the look-ahead is NaN or has min > max (wfl_lexicon_lookahead_check writes them)", what);
    return WFL_ERR_INVALID;
  }
  if (!word_lm) {
    set_error("%s: look-ahead needs a word LM", what);
    return WFL_ERR_INVALID;
  }
  d->bound = beam_look_bound(d->lm.alpha, word_lm->step_min, word_lm->step_max, d->omega, d->lm.beta, *look);
  d->lm.bound = d->bound;
  return WFL_OK;
}


}  // extern "C"

// The lexicon's pack of a launch, for the nine entries below -- P: BeamLex, BeamLexMarked or the BeamLook of either, by
// the lexicon's convention (`lex`: a wfl_lexicon or a wfl_lexicon_marked) and whether there is a look-ahead (`look`, not
// read otherwise).  The checks in the order the entries have always had them: the start-marked lexicon's shape,
// beam_lex_fill, beam_look_fill.
template <typename P, typename Lexicon>
static int beam_lex_pack(const char* what, const Lexicon* lex, const wfl_lexicon_lookahead* look, const wfl_ngram_lm* word_lm,
                         double lm_weight, double word_bonus, double length_bonus, int score_eos, P* d) {
  constexpr bool marked = BeamMarked<P>::value, looks = BeamLooks<P>::value;
  auto* base = [d] {
    if constexpr (looks)
      return &d->pack;
    else
      return d;
  }();
  const wfl_lexicon* trie;
  BeamLex* lx;
  if constexpr (marked) {
    if (const int rc = lexicon_marked_shape(what, lex)) return rc;
    trie = &lex->trie, lx = &base->lex;
    base->node_word = lex->node_word, base->start_node = lex->start_node;
  } else {
    trie = lex, lx = base;
  }
  if (const int rc = beam_lex_fill(what, trie, word_lm, lm_weight, word_bonus, length_bonus, score_eos, lx)) return rc;
  if constexpr (looks) {
    if (const int rc = beam_look_fill(what, look, word_lm, lx)) return rc;
    d->node_look = look->node_look;
  }
  return WFL_OK;
}

extern "C" {

int wfl_ctc_beam_search_lexicon(const float* x, const int32_t* lengths, int B, int T, int C, int blank, int beam,
                                int classes_per_frame, int nbest, int normalize, const wfl_lexicon* lex,
                                const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus, double length_bonus,
                                int score_eos, void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets,
                                double* scores, void* stream) {
  const char* what = "ctc_beam_search_lexicon";
  BeamLex d;
  if (const int rc = beam_lex_pack(what, lex, nullptr, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  return beam_run(what, {x, lengths, B, T, C, blank, beam, classes_per_frame, nbest, normalize, ws, out, out_capacity, out_offsets,
                         scores, stream}, d);
}

// wfl_ctc_beam_search_lexicon with a start-marked lexicon: its checks in its order
int wfl_ctc_beam_search_lexicon_marked(const float* x, const int32_t* lengths, int B, int T, int C, int blank, int beam,
                                       int classes_per_frame, int nbest, int normalize, const wfl_lexicon_marked* lex,
                                       const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus, double length_bonus,
                                       int score_eos, void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets,
                                       double* scores, void* stream) {
  const char* what = "ctc_beam_search_lexicon_marked";
  BeamLexMarked d;
  if (const int rc = beam_lex_pack(what, lex, nullptr, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  return beam_run(what, {x, lengths, B, T, C, blank, beam, classes_per_frame, nbest, normalize, ws, out, out_capacity, out_offsets,
                         scores, stream}, d);
}

// wfl_ctc_beam_search_lexicon with look-ahead: its checks in its order, then the look-ahead's
int wfl_ctc_beam_search_lexicon_lookahead(const float* x, const int32_t* lengths, int B, int T, int C, int blank, int beam,
                                          int classes_per_frame, int nbest, int normalize, const wfl_lexicon* lex,
                                          const wfl_lexicon_lookahead* look, const wfl_ngram_lm* word_lm, double lm_weight,
                                          double word_bonus, double length_bonus, int score_eos, void* ws, int32_t* out,
                                          int64_t out_capacity, int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "ctc_beam_search_lexicon_lookahead";
  BeamLexLook d;
  if (const int rc = beam_lex_pack(what, lex, look, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  return beam_run(what, {x, lengths, B, T, C, blank, beam, classes_per_frame, nbest, normalize, ws, out, out_capacity, out_offsets,
                         scores, stream}, d);
}

// wfl_ctc_beam_search_lexicon_marked with look-ahead: its checks in its order, then the look-ahead's
int wfl_ctc_beam_search_lexicon_marked_lookahead(const float* x, const int32_t* lengths, int B, int T, int C, int blank, int beam,
                                                 int classes_per_frame, int nbest, int normalize, const wfl_lexicon_marked* lex,
                                                 const wfl_lexicon_lookahead* look, const wfl_ngram_lm* word_lm, double lm_weight,
                                                 double word_bonus, double length_bonus, int score_eos, void* ws, int32_t* out,
                                                 int64_t out_capacity, int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "ctc_beam_search_lexicon_marked_lookahead";
  BeamLexMarkedLook d;
  if (const int rc = beam_lex_pack(what, lex, look, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  return beam_run(what, {x, lengths, B, T, C, blank, beam, classes_per_frame, nbest, normalize, ws, out, out_capacity, out_offsets,
                         scores, stream}, d);
}

// The Transducer search with a lexicon and an optional word LM: wfl_transducer_beam_search's call
// and checks in its order, then wfl_ctc_beam_search_lexicon's checks of the lexicon, the LM and the three constants.
int wfl_transducer_beam_search_lexicon(const float* x, const float* Wt, const float* logz, int B, int T, int C, int blank,
                                       int forced, int beam, int classes_per_frame, int nbest, int normalize,
                                       const wfl_lexicon* lex, const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus,
                                       double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                                       int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "transducer_beam_search_lexicon";
  BeamTokCall p;
  if (const int rc = beam_tok_prelude(what, x, Wt, logz, B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize, ws, out,
                                      out_capacity, out_offsets, scores, stream, &p))
    return rc;
  BeamLex d;
  if (const int rc = beam_lex_pack(what, lex, nullptr, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  return beam_run_tok(what, p, BeamTokLex{p.tok, d}, d);  // (CTC's side: section 20's rules without lengths)
}

// wfl_transducer_beam_search_lexicon with a start-marked lexicon: its checks in its order
int wfl_transducer_beam_search_lexicon_marked(const float* x, const float* Wt, const float* logz, int B, int T, int C, int blank,
                                              int forced, int beam, int classes_per_frame, int nbest, int normalize,
                                              const wfl_lexicon_marked* lex, const wfl_ngram_lm* word_lm, double lm_weight,
                                              double word_bonus, double length_bonus, int score_eos, void* ws, int32_t* out,
                                              int64_t out_capacity, int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "transducer_beam_search_lexicon_marked";
  BeamTokCall p;
  if (const int rc = beam_tok_prelude(what, x, Wt, logz, B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize, ws, out,
                                      out_capacity, out_offsets, scores, stream, &p))
    return rc;
  BeamLexMarked d;
  if (const int rc = beam_lex_pack(what, lex, nullptr, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  return beam_run_tok(what, p, BeamTokLexMarked{p.tok, d}, d);  // (CTC's side: wfl_ctc_beam_search_lexicon_marked's rules)
}

// wfl_transducer_beam_search_lexicon with look-ahead: its checks in its order, then the look-ahead's
int wfl_transducer_beam_search_lexicon_lookahead(const float* x, const float* Wt, const float* logz, int B, int T, int C, int blank,
                                                 int forced, int beam, int classes_per_frame, int nbest, int normalize,
                                                 const wfl_lexicon* lex, const wfl_lexicon_lookahead* look,
                                                 const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus,
                                                 double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                                                 int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "transducer_beam_search_lexicon_lookahead";
  BeamTokCall p;
  if (const int rc = beam_tok_prelude(what, x, Wt, logz, B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize, ws, out,
                                      out_capacity, out_offsets, scores, stream, &p))
    return rc;
  BeamLexLook d;
  if (const int rc = beam_lex_pack(what, lex, look, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  // (CTC's side: wfl_ctc_beam_search_lexicon_lookahead's rules without lengths)
  return beam_run_tok(what, p, BeamTokLexLook{{p.tok, d.pack}, d.node_look}, d);
}

// wfl_transducer_beam_search_lexicon_marked with look-ahead: its checks in its order, then the
// look-ahead's
int wfl_transducer_beam_search_lexicon_marked_lookahead(const float* x, const float* Wt, const float* logz, int B, int T, int C,
                                                        int blank, int forced, int beam, int classes_per_frame, int nbest,
                                                        int normalize, const wfl_lexicon_marked* lex,
                                                        const wfl_lexicon_lookahead* look, const wfl_ngram_lm* word_lm,
                                                        double lm_weight, double word_bonus, double length_bonus, int score_eos,
                                                        void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets,
                                                        double* scores, void* stream) {
  const char* what = "transducer_beam_search_lexicon_marked_lookahead";
  BeamTokCall p;
  if (const int rc = beam_tok_prelude(what, x, Wt, logz, B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize, ws, out,
                                      out_capacity, out_offsets, scores, stream, &p))
    return rc;
  BeamLexMarkedLook d;
  if (const int rc = beam_lex_pack(what, lex, look, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d)) return rc;
  // (CTC's side: wfl_ctc_beam_search_lexicon_marked_lookahead's rules without lengths)
  return beam_run_tok(what, p, BeamTokLexMarkedLook{{p.tok, d.pack}, d.node_look}, d);
}

// The ASG search with a lexicon and an optional word LM: wfl_asg_beam_search's call and checks,
// wfl_ctc_beam_search_lexicon's checks of the lexicon, the LM and the three constants, and the garbage class.
int wfl_asg_beam_search_lexicon(const float* x, const float* Wt, const float* logz, int B, int T, int C, int beam,
                                int classes_per_frame, int nbest, int drop, int num_replabels, int garbage, const wfl_lexicon* lex,
                                const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus, double length_bonus,
                                int score_eos, void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets, double* scores,
                                void* stream) {
  const char* what = "asg_beam_search_lexicon";
  if (!Wt) {
    set_error("%s: a NULL pointer", what);
    return WFL_ERR_INVALID;
  }
  const BeamCall c{x, nullptr, B, T, C, -1, beam, classes_per_frame, nbest, logz ? 1 : 0, ws, out, out_capacity, out_offsets,
                   scores, stream, false, true, drop, num_replabels};
  // (beam_run makes this check again: this entry's own come behind it and ahead of the room in `out`)
  if (const int rc = beam_call_check(what, c)) return rc;
  if (garbage < -1 || garbage >= C) {
    set_error("%s: garbage %d is outside [-1, %d)", what, garbage, C);
    return WFL_ERR_INVALID;
  }
  BeamAsgLex d;
  if (const int rc = beam_lex_pack(what, lex, nullptr, word_lm, lm_weight, word_bonus, length_bonus, score_eos, &d.lex)) return rc;
  d.asg = BeamAsg{Wt, logz, C};
  d.garbage = garbage;
  return beam_run(what, c, d);
}

// The ASG search with a token-level n-gram LM: wfl_asg_beam_search's call and checks, the raw
// alphabet the LM reads through (garbage, replabels), then wfl_ctc_beam_search_lm's checks of the LM and the two scalars.
int wfl_asg_beam_search_lm(const float* x, const float* Wt, const float* logz, int B, int T, int C, int beam, int classes_per_frame,
                           int nbest, int drop, int num_replabels, int garbage, int replabels, const wfl_ngram_lm* lm,
                           double lm_weight, double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                           int64_t* out_offsets, double* scores, void* stream) {
  const char* what = "asg_beam_search_lm";
  if (!Wt) {
    set_error("%s: a NULL pointer", what);
    return WFL_ERR_INVALID;
  }
  const BeamCall c{x, nullptr, B, T, C, -1, beam, classes_per_frame, nbest, logz ? 1 : 0, ws, out, out_capacity, out_offsets,
                   scores, stream, false, true, drop, num_replabels};
  // (beam_run makes this check again: this entry's own come behind it and ahead of the room in `out`)
  if (const int rc = beam_call_check(what, c)) return rc;
  if (garbage < -1 || garbage >= C) {
    set_error("%s: garbage %d is outside [-1, %d)", what, garbage, C);
    return WFL_ERR_INVALID;
  }
  const int64_t tokens = (int64_t)C - replabels - (garbage >= 0 ? 1 : 0);
  if (replabels < 0 || tokens < 1) {
    set_error("%s: replabels %d is negative or, with garbage %d, leaves no token among %d classes", what, replabels, garbage, C);
    return WFL_ERR_INVALID;
  }
  BeamAsgLm d;
  // token i is LM label i, the LM's unused blank is N and </s> is N + 1
  if (const int rc = beam_lm_terms(what, lm, false, (int)tokens + 1, lm_weight, length_bonus, score_eos, &d.lm)) return rc;
  if (!(fabs(lm_weight) < __builtin_inf()) || !(fabs(length_bonus) < __builtin_inf())) {
    set_error("%s: lm_weight %g and length_bonus %g must be finite", what, lm_weight, length_bonus);
    return WFL_ERR_INVALID;
  }
  d.lm.bound = beam_asg_lm_bound(lm_weight, lm->step_min, lm->step_max, length_bonus, replabels);
  d.asg = BeamAsg{Wt, logz, C};
  d.replabels = replabels;
  d.garbage = garbage;
  return beam_run(what, c, d);
}

}  // extern "C"
