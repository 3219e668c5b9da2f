// Token and word error counts behind viterbi() (the reference's compute_edit_distance, train.py:74-87, as test.py:94-109
// uses it), on the device: per utterance the symbol strings of the hypothesis labels (what wfl_decode_emissions /
// wfl_decode_paths left) and of the reference labels (the CtcTargets layout), separators stripped at both ends, their
// Levenshtein distance, and the Levenshtein distance of their word sequences -- B x 4 int32 out, nothing else.
//
// Three launches, a wave per (utterance, side) or (utterance, distance); every position is a prefix sum, no atomics:
//   measure   (utterance, side): L = the number of symbols the labels expand to;
//   prepare   (utterance, side): the block's base in the workspace = the sum of the block sizes before it (fixed order,
//             as the decode's write launch finds an utterance's base), the symbols, the stripped range [lo, hi) and the
//             words (start, end) by ballot + prefix popcount over "not a separator, behind a separator or first";
//   distance  (utterance, symbols | words): anti-diagonal wavefront.  Lane l owns reference column j0 + 1 + l of a strip
//             of 64 columns and computes row s - l + 1 at step s: `up` is its own value of step s - 1, `left` lane l - 1's
//             (a DPP wave_shr:1, taken unconditionally, selected afterwards), `diag` the previous `left`.  Lane 0 takes
//             left / diag from the column the strip before left in the workspace, the strip's last lane writes that
//             column for the next strip.  Hypothesis rows and that column pass through LDS in chunks of kErrChunk steps:
//             the LDS use does not depend on the string lengths.  The word distance is the same code with another
//             equality: lengths, then symbols (exact, no hashing).
// The workspace is laid out on the device, block after block: the layout does not depend on the tables' longest
// expansion, only its bound (wfl_errors_workspace) does.
#include "device_common.h"

#include <type_traits>

namespace wfl {

constexpr int kErrChunk = 512;  // steps of a strip per LDS fill
constexpr int kErrUnroll = 8;   // steps whose operands are read from LDS together (divides kErrChunk)

// per (side, utterance): what the launches hand to each other
struct ErrMeta {
  int32_t L, lo, hi, nwords;  // symbols; the stripped range; words
  int32_t n, pad;             // labels
  int64_t base;               // of the block, in int32 words behind the meta table
  int64_t first;              // of the labels, in the side's label buffer
};

struct ErrSide {
  const int32_t* lab;
  const int64_t* off;
  const int32_t* exp_ptr;
  const int32_t* exp_sym;
  int V;
  int64_t capacity;
};
struct ErrArgs {
  ErrSide side[2];  // 0: hypothesis, 1: reference
  int B, sep;
};

// block of an utterance, in int32 words.  hypothesis: symbols L | word starts + ends L + 1 | the two boundary columns
// 2 (L + 1); reference: symbols L | word starts + ends L + 1.  (words <= (L + 1) / 2.)
__host__ __device__ inline int64_t err_block_words(int side, int64_t L) { return side == 0 ? 4 * L + 3 : 2 * L + 1; }
inline int64_t err_align16(int64_t n) { return (n + 15) & ~(int64_t)15; }
inline int64_t err_meta_bytes(int64_t B) { return err_align16(2 * B * (int64_t)sizeof(ErrMeta)); }

__device__ __forceinline__ int err_wave_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
__device__ __forceinline__ int64_t err_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the labels of utterance b on a side: [first, first + n), inside the side's buffer and apart from every other
// utterance's whatever the offsets say (the running maximum of the clamped offsets: theirs, where they ascend) -- so
// the labels of a side never number more than its capacity, which is what the workspace bound rests on
__device__ __forceinline__ void err_row(const ErrSide& s, int b, int lane, int64_t* first, int* n) {
  long long lo = 0;
  for (int r = lane; r <= b; r += 64) lo = max(lo, (long long)err_clamp64(s.off[r], 0, s.capacity));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lo = max(lo, __shfl_xor(lo, o, 64));
  const int64_t hi = err_clamp64(s.off[b + 1], lo, s.capacity);
  *first = lo;
  *n = (int)min(hi - lo, (int64_t)0x3fffffff);
}
// the expansion of label v: [*start, *start + return) of exp_sym, inside the table whatever its entries say
__device__ __forceinline__ int err_expansion(const ErrSide& s, int v, int* start) {
  *start = 0;
  if (!s.exp_ptr) return 1;  // a label is its own symbol
  if (v < 0 || v >= s.V) return 0;
  const int total = max(s.exp_ptr[s.V], 0);
  const int lo = min(max(s.exp_ptr[v], 0), total);
  const int hi = min(max(s.exp_ptr[v + 1], lo), total);
  *start = lo;
  return hi - lo;
}

__global__ void __launch_bounds__(64) errors_measure_kernel(ErrArgs a, ErrMeta* __restrict__ meta) {
  const int lane = threadIdx.x, b = blockIdx.x, sd = blockIdx.y;
  const ErrSide& s = a.side[sd];
  int64_t first;
  int n;
  err_row(s, b, lane, &first, &n);
  int total = 0;
  for (int k = lane; k < n; k += 64) {
    int st;
    total += err_expansion(s, s.lab[first + k], &st);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  if (lane == 0) {
    ErrMeta* me = meta + (int64_t)sd * a.B + b;
    me->L = total, me->n = n, me->first = first;
  }
}

__global__ void __launch_bounds__(64) errors_prepare_kernel(ErrArgs a, ErrMeta* __restrict__ meta, int32_t* __restrict__ arena) {
  const int lane = threadIdx.x, b = blockIdx.x, sd = blockIdx.y;
  const ErrSide& s = a.side[sd];
  // base: the blocks before this one, the hypotheses' first
  long long base = 0;
  const int before = sd * a.B + b;
  for (int r = lane; r < before; r += 64) base += err_block_words(r >= a.B, meta[r].L);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o, 64);
  ErrMeta* me = meta + before;
  const int L = me->L;
  int32_t* sym = arena + base;
  int32_t* wstart = sym + L;
  int32_t* wend = wstart + (L + 1) / 2;
  const int64_t first = me->first;
  const int n = me->n;
  // 1. the symbols
  int running = 0;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    int st = 0, len = 0, v = 0;
    if (k < n) v = s.lab[first + k], len = err_expansion(s, v, &st);
    const int incl = err_wave_scan(len, lane);
    const int pos = running + incl - len;
    if (pos + len <= L) {  // (always: the measure launch counted the same expansions)
      if (s.exp_ptr)
        for (int i = 0; i < len; ++i) sym[pos + i] = s.exp_sym[st + i];
      else if (len)
        sym[pos] = v;
    }
    running += __shfl(incl, 63, 64);
  }
  __syncthreads();  // (the symbols, written by other lanes, are read below)
  // 2. the stripped range and the words
  int lo = 0x7fffffff, hi = 0, nwords = 0;
  if (a.sep < 0) {
    lo = 0, hi = L;
  } else {
    int ends = 0;
    for (int k0 = 0; k0 < L; k0 += 64) {
      const int k = k0 + lane;
      const bool in = k < L;
      const bool is = in && sym[k] != a.sep;
      const bool opens = is && (k == 0 || sym[k - 1] == a.sep);
      const bool closes = is && (k == L - 1 || sym[k + 1] == a.sep);
      const unsigned long long mo = __ballot(opens), mc = __ballot(closes), below = (1ull << lane) - 1ull;
      if (opens) wstart[nwords + __popcll(mo & below)] = k;
      if (closes) wend[ends + __popcll(mc & below)] = k + 1;
      nwords += __popcll(mo), ends += __popcll(mc);
      if (is) lo = min(lo, k), hi = max(hi, k + 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, 64)), hi = max(hi, __shfl_xor(hi, o, 64));
    if (hi == 0) lo = 0;  // nothing but separators
  }
  if (lane == 0) me->lo = lo, me->hi = hi, me->nwords = nwords, me->base = base;
}

struct ErrWord {
  int start, len;
};
// are word h of the hypothesis and word r of the reference the same symbols in the same order?
__device__ __forceinline__ bool err_same_word(const int32_t* __restrict__ hsym, ErrWord h, const int32_t* __restrict__ rsym, ErrWord r) {
  if (h.len != r.len) return false;
  for (int k = 0; k < h.len; ++k)
    if (hsym[h.start + k] != rsym[r.start + k]) return false;
  return true;
}

// One wave per (utterance, distance): blockIdx.y = 0 symbols (counts[b][0..1]), 1 words (counts[b][2..3]).
template <bool WORDS>
__device__ __forceinline__ void errors_distance(const ErrMeta& mh, const ErrMeta& mr, int32_t* __restrict__ arena,
                                                int32_t* __restrict__ out2, ErrWord* rows_lds, int32_t* edge) {
  using Row = typename std::conditional<WORDS, ErrWord, int32_t>::type;  // a hypothesis row: a word, or a symbol
  Row* rows = reinterpret_cast<Row*>(rows_lds);
  const int lane = threadIdx.x;
  const int32_t* hsym = arena + mh.base;
  const int32_t* rsym = arena + mr.base;
  const int Lh = mh.L, Lr = mr.L;
  const int32_t* hws = hsym + Lh;
  const int32_t* hwe = hws + (Lh + 1) / 2;
  const int32_t* rws = rsym + Lr;
  const int32_t* rwe = rws + (Lr + 1) / 2;
  // the column left of a strip, D[0..n][j0]: one per distance
  int32_t* column = arena + mh.base + 2 * (int64_t)Lh + 1 + (WORDS ? Lh + 1 : 0);
  const int n = WORDS ? min(mh.nwords, (Lh + 1) / 2) : max(min(mh.hi, Lh) - max(mh.lo, 0), 0);  // rows: the hypothesis
  const int m = WORDS ? min(mr.nwords, (Lr + 1) / 2) : max(min(mr.hi, Lr) - max(mr.lo, 0), 0);  // columns: the reference
  const int hlo = max(mh.lo, 0), rlo = max(mr.lo, 0);
  auto word = [](const int32_t* ws, const int32_t* we, int k, int L) {
    const int st = min(max(ws[k], 0), L);
    return ErrWord{st, min(max(we[k] - st, 0), L - st)};
  };
  int result = n;  // (no reference: every row is a deletion)
  for (int j0 = 0; j0 < m; j0 += 64) {
    const int W = min(64, m - j0), j = j0 + 1 + lane;
    const bool first = j0 == 0, last = j0 + 64 >= m;
    ErrWord mine{0, 0};  // this lane's column: a symbol (in .start) or a word
    if (lane < W) mine = WORDS ? word(rws, rwe, j - 1, Lr) : ErrWord{rsym[rlo + j - 1], 0};
    int cur = j, diag = j - 1;  // row 0
    const int steps = n + W - 1;
    for (int s0 = 0; s0 < steps; s0 += kErrChunk) {
      __syncthreads();  // the chunk before has been read; the column the strip before wrote is visible
      // rows[k]: row s0 - 62 + k (k <= kErrChunk + 62);  edge[k]: D[s0 + 1 + k][j0]
#pragma unroll  // (every load of the fill in flight together)
      for (int k = lane; k < kErrChunk + 63; k += 64) {
        const int i = s0 - 62 + k;
        if constexpr (WORDS)
          rows[k] = i >= 1 && i <= n ? word(hws, hwe, i - 1, Lh) : ErrWord{0, 0};
        else
          rows[k] = i >= 1 && i <= n ? hsym[hlo + i - 1] : 0;
      }
#pragma unroll
      for (int k = lane; k < kErrChunk; k += 64) {
        const int i = s0 + 1 + k;
        edge[k] = first ? i : (i <= n ? column[i] : 0);
      }
      __syncthreads();
      // kErrUnroll steps at a time, their LDS reads issued before the first cell: what is left on the chain from cell
      // to cell is the shift and three VALU operations.  (Steps past the last one find no active lane.)
      const int send = min(s0 + kErrChunk, steps);
      for (int s = s0; s < send; s += kErrUnroll) {
        Row r[kErrUnroll];
        int e[kErrUnroll];
#pragma unroll
        for (int u = 0; u < kErrUnroll; ++u) r[u] = rows[s - s0 + u + 63 - lane], e[u] = edge[s - s0 + u];
#pragma unroll
        for (int u = 0; u < kErrUnroll; ++u) {
          const int i = s + u - lane + 1;
          const int shifted = dpp_i32<0x138, 0xf>(0, cur);  // wave_shr:1, every lane takes part; selected below
          const int left = lane == 0 ? e[u] : shifted;
          const bool active = i >= 1 && i <= n && lane < W;
          bool same = false;
          if constexpr (WORDS) {
            if (active) same = err_same_word(hsym, r[u], rsym, mine);
          } else {
            same = r[u] == mine.start;
          }
          const int cell = min(min(cur, left) + 1, diag + (same ? 0 : 1));
          if (active) cur = cell;
          diag = left;
          if (!last && active && lane == W - 1) column[i] = cur;
        }
      }
    }
    if (last) result = __shfl(cur, W - 1, 64);
  }
  if (lane == 0) out2[0] = result, out2[1] = m;
}

__global__ void __launch_bounds__(64) errors_distance_kernel(int B, int sep, const ErrMeta* __restrict__ meta,
                                                              int32_t* __restrict__ arena, int32_t* __restrict__ counts) {
  __shared__ ErrWord rows[kErrChunk + 63];
  __shared__ int32_t edge[kErrChunk];
  const int b = blockIdx.x;
  const ErrMeta mh = meta[b], mr = meta[B + b];
  int32_t* out = counts + (int64_t)b * 4;
  if (blockIdx.y == 0)
    errors_distance<false>(mh, mr, arena, out, rows, edge);
  else if (sep >= 0)
    errors_distance<true>(mh, mr, arena, out + 2, rows, edge);
  else if (threadIdx.x == 0)
    out[2] = 0, out[3] = 0;
}

}  // namespace wfl

using namespace wfl;

extern "C" {

int wfl_errors_chunk_steps(void) { return kErrChunk; }

int wfl_errors_workspace(int B, int64_t hyp_capacity, int64_t ref_labels, int hyp_max_expansion, int ref_max_expansion,
                         int64_t* ws_bytes) {
  if (B < 1 || hyp_capacity < 0 || ref_labels < 0 || hyp_max_expansion < 0 || ref_max_expansion < 0 || !ws_bytes) {
    set_error("errors_workspace: bad arguments (B %d, hyp_capacity %lld, ref_labels %lld, max expansions %d, %d)", B,
              (long long)hyp_capacity, (long long)ref_labels, hyp_max_expansion, ref_max_expansion);
    return WFL_ERR_INVALID;
  }
  const int64_t lim = 0x3fffffff;  // symbols of a side: the index width of the kernels
  if ((hyp_max_expansion && hyp_capacity > lim / hyp_max_expansion) || (ref_max_expansion && ref_labels > lim / ref_max_expansion)) {
    set_error("errors_workspace: %lld x %d or %lld x %d symbols is more than the index width of the count takes",
              (long long)hyp_capacity, hyp_max_expansion, (long long)ref_labels, ref_max_expansion);
    return WFL_ERR_UNSUPPORTED;
  }
  const int64_t words = err_block_words(0, hyp_capacity * hyp_max_expansion) + 3 * ((int64_t)B - 1) +
                        err_block_words(1, ref_labels * ref_max_expansion) + ((int64_t)B - 1);
  *ws_bytes = err_meta_bytes(B) + err_align16(words * (int64_t)sizeof(int32_t));
  return WFL_OK;
}

int wfl_errors_count(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref, const int64_t* ref_off, int B,
                     const int32_t* hyp_exp_ptr, const int32_t* hyp_exp_sym, int hyp_V, const int32_t* ref_exp_ptr,
                     const int32_t* ref_exp_sym, int ref_V, int sep, int64_t hyp_capacity, int64_t ref_labels, void* ws,
                     int32_t* counts, void* stream) {
  if (B < 1 || !hyp || !hyp_off || !ref || !ref_off || !ws || !counts || hyp_capacity < 0 || ref_labels < 0 ||
      (hyp_exp_ptr != nullptr) != (hyp_exp_sym != nullptr) || (ref_exp_ptr != nullptr) != (ref_exp_sym != nullptr) ||
      (hyp_exp_ptr && hyp_V < 1) || (ref_exp_ptr && ref_V < 1)) {
    set_error("errors_count: bad arguments (B %d, hyp_capacity %lld, ref_labels %lld, table sizes %d, %d)", B,
              (long long)hyp_capacity, (long long)ref_labels, hyp_V, ref_V);
    return WFL_ERR_INVALID;
  }
  ErrArgs a;
  a.side[0] = ErrSide{hyp, hyp_off, hyp_exp_ptr, hyp_exp_sym, hyp_V, hyp_capacity};
  a.side[1] = ErrSide{ref, ref_off, ref_exp_ptr, ref_exp_sym, ref_V, ref_labels};
  a.B = B, a.sep = sep < 0 ? -1 : sep;
  ErrMeta* meta = static_cast<ErrMeta*>(ws);
  int32_t* arena = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + err_meta_bytes(B));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(errors_measure_kernel, dim3(B, 2), dim3(64), 0, st, a, meta);
  WFL_LAUNCH_CHECK();
  hipLaunchKernelGGL(errors_prepare_kernel, dim3(B, 2), dim3(64), 0, st, a, meta, arena);
  WFL_LAUNCH_CHECK();
  hipLaunchKernelGGL(errors_distance_kernel, dim3(B, 2), dim3(64), 0, st, B, a.sep, meta, arena, counts);
  WFL_LAUNCH_CHECK();
  return WFL_OK;
}

}  // extern "C"
