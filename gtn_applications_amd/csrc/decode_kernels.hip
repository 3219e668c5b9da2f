// The decode every criterion's viterbi() ends with (ctc.py:126-135, asg.py:225-234, transducer.py:216-232), on the
// device: per utterance, in frame order, collapse runs of equal frame labels, drop one label (blank / garbage),
// optionally expand replabels (asg.py:35-49) or reject rows the blank="forced" token graph does not accept
// (csrc/graph.cpp::token_decode), and deliver the utterances back to back with their offsets.
//
// Two front ends produce the frame labels of a chunk of kDecodeChunk frames, one wave per chunk, lane i = frame t0 + i:
//   emissions: the first maximal class of x[b, t, :] (+ bias), a wave per row, rows batched for loads in flight -- the
//              [B,T] label array never exists in memory; the wave also takes the label of frame t0 - 1 (one more row);
//   paths:     a load from the [B, path_stride] label paths of wfl_dense_viterbi.
// One back end, three launches:
//   count  (a wave per chunk):  keep flags, ballot + prefix popcount compaction of the kept values into the chunk's
//          slot of the workspace, and the chunk's summary {kept, first kept, last kept, outputs it emits when no label
//          precedes it, accepted};
//   scan   (a wave per utterance): walks the utterance's summaries 64 at a time; carries the last kept value (does a
//          replabel that opens a chunk follow a label?) and the running output count from chunk to chunk, and decides
//          whether the row is accepted;
//   write  (a wave per chunk):  the utterance's base = sum of the totals of the utterances before it (fixed order),
//          then the chunk's kept values, replabels expanded, to out -- plain vector stores, so `out` / `out_offsets`
//          may be pinned host memory.
// No atomics anywhere: every position is a prefix sum, the result is deterministic.
// Per-utterance lengths (wfl_decode_emissions_lengths: a padded batch, criterions/ctc.py): the frames t >= lengths[b] are
// no candidates in the count step -- they are neither read nor kept, and everything behind the count step sees a row
// that ends at lengths[b].
#include <type_traits>

#include "device_common.h"

namespace wfl {

constexpr int kDecodeChunk = 64;   // frames per chunk = lanes per wave
constexpr int kDecodeSummary = 8;  // int32 words per chunk summary
enum { kSumKept = 0, kSumFirst = 1, kSumLast = 2, kSumEmit = 3, kSumOk = 4, kSumOffset = 5, kSumCarry = 6 };

struct DecodeArgs {
  int B, T, nch;  // nch: chunks per utterance
  int drop, R, flags;
};

// workspace: [summaries: B nch x 8 int32 | row totals: B int64 | row accepted: B int32 | kept values: B nch x 64 int32]
struct DecodeWs {
  int64_t summaries, totals, accepted, values, bytes;
};
inline int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }
inline DecodeWs decode_ws_layout(int64_t B, int64_t T) {
  const int64_t chunks = B * ((T + kDecodeChunk - 1) / kDecodeChunk);
  DecodeWs w;
  w.summaries = 0;
  w.totals = align16(chunks * kDecodeSummary * (int64_t)sizeof(int32_t));
  w.accepted = w.totals + align16(B * (int64_t)sizeof(int64_t));
  w.values = w.accepted + align16(B * (int64_t)sizeof(int32_t));
  w.bytes = w.values + chunks * kDecodeChunk * (int64_t)sizeof(int32_t);
  return w;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// A score as an int whose signed order is the order the argmax wants: -0 = +0, and a NaN either below everything
// (= -inf: wfl_row_argmax's rule) or above everything, all NaNs equal (torch.argmax's rule: the first NaN wins).
__device__ __forceinline__ int score_key(float v, bool nan_is_max) {
  if (v != v) return nan_is_max ? 0x7fffffff : (int)0x807fffff;  // (0x807fffff: the key of -inf)
  int b = __float_as_int(v);
  if (b == (int)0x80000000) b = 0;
  return b >= 0 ? b : b ^ 0x7fffffff;
}

constexpr int kNoIndex = 0x3fffffff;
constexpr int kNoKey = -2147483647 - 1;  // below the key of every score

// first[u] = the first maximal class of frame min(t + u, T - 1) for u < N, the same in every lane.  NV > 0: the row in
// NV registers per lane (C <= 64 NV), every load of the N rows issued before the first reduction.  NV == 0: any C.
template <int NV, int N>
__device__ __forceinline__ void first_max_rows(const float* __restrict__ xb, int T, int C, int t, int lane,
                                               const float* bv, const float* __restrict__ bias, bool nan_is_max,
                                               int* first) {
  int key[N], idx[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const float* row = xb + (int64_t)min(t + u, T - 1) * C;
    key[u] = kNoKey, idx[u] = kNoIndex;
    if constexpr (NV > 0) {
      float v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? row[c] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        const int k = score_key(v[i] + bv[i], nan_is_max);
        if (c < C && k > key[u]) key[u] = k, idx[u] = c;  // (ascending c: the first of equals stays)
      }
    } else {
#pragma unroll 4
      for (int c = lane; c < C; c += 64) {
        const int k = score_key(bias ? row[c] + bias[c] : row[c], nan_is_max);
        if (k > key[u]) key[u] = k, idx[u] = c;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int m = wave_all_max_int(key[u]);
    first[u] = -wave_all_max_int(-(key[u] == m ? idx[u] : kNoIndex));
  }
}

// The count step of one chunk, from its frame labels (lane i: frame t0 + i; prev0: the label of frame t0 - 1).  Tb <= a.T:
// the frames of the utterance (wfl_decode_emissions_lengths) -- a frame t >= Tb is no candidate, so a chunk's kept
// values, its first / last kept value and what the scan carries across the boundaries are those of a row that ends at Tb.
__device__ __forceinline__ void decode_count_chunk(int lab, int prev0, int t0, int lane, const DecodeArgs& a, int Tb,
                                                   int32_t* __restrict__ summary, int32_t* __restrict__ values) {
  const int t = t0 + lane;
  const bool valid = t < Tb;
  int prev = __shfl_up(lab, 1, 64);
  if (lane == 0) prev = prev0;
  const bool keep = valid && (t == 0 || lab != prev) && lab != a.drop;
  const unsigned long long mask = __ballot(keep);
  const unsigned long long below = mask & ((1ull << lane) - 1ull);
  const int kept = __popcll(mask);
  if (keep) values[__popcll(below)] = lab;
  // outputs this chunk emits if no label precedes its first kept value (the scan adds that case)
  const int before = __shfl(lab, below ? 63 - __clzll(below) : lane, 64);  // the kept value before this lane's
  int emit = 0;
  if (keep) emit = (a.R == 0 || lab >= a.R) ? 1 : (below != 0 && before >= a.R ? lab + 1 : 0);
  emit = wave_sum_int(emit);
  const int first = __shfl(lab, mask ? __ffsll(mask) - 1 : 0, 64);
  const int last = __shfl(lab, mask ? 63 - __clzll(mask) : 0, 64);
  // blank="forced" token graph (graph.cpp::token_decode): starts and ends with the blank, tokens separated by blanks
  bool bad = false;
  if (valid && (a.flags & WFL_DECODE_BLANK_SEPARATED)) {
    if (t == 0) bad = lab != a.drop;
    else bad = !(lab == a.drop || prev == a.drop || lab == prev);
    if (t == Tb - 1) bad = bad || lab != a.drop;
  }
  const int ok = __ballot(bad) == 0ull;
  if (lane == 0) {
    summary[kSumKept] = kept;
    summary[kSumFirst] = kept ? first : -1;
    summary[kSumLast] = kept ? last : -1;
    summary[kSumEmit] = emit;
    summary[kSumOk] = ok;
  }
}

// LEN: per-utterance lengths (wfl_decode_emissions_lengths); without them the kernel is the one it was
template <int NV, int RU, bool LEN>
__global__ void __launch_bounds__(256) decode_count_emissions_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                                      const int32_t* __restrict__ lengths, int C, DecodeArgs a,
                                                                      int32_t* __restrict__ summaries, int32_t* __restrict__ values) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= (int64_t)a.B * a.nch) return;  // (a whole wave)
  const int b = (int)(chunk / a.nch), t0 = (int)(chunk % a.nch) * kDecodeChunk;
  const float* xb = x + (int64_t)b * a.T * C;
  const int Tb = LEN ? min(max(lengths[b], 0), a.T) : a.T;  // (wave-uniform; the rows read stay those of [0, T))
  const bool nan_is_max = (a.flags & WFL_DECODE_NAN_IS_MAX) != 0;
  float bv[NV > 0 ? NV : 1];
#pragma unroll
  for (int i = 0; i < (NV > 0 ? NV : 1); ++i) {
    const int c = lane + 64 * i;
    bv[i] = (bias && c < C) ? bias[c] : 0.f;
  }
  int prev0 = -1;
  if (t0 > 0 && t0 < Tb) first_max_rows<NV, 1>(xb, a.T, C, t0 - 1, lane, bv, bias, nan_is_max, &prev0);
  int lab = 0;
  for (int u0 = 0; u0 < kDecodeChunk && t0 + u0 < Tb; u0 += RU) {
    int first[RU];
    first_max_rows<NV, RU>(xb, a.T, C, t0 + u0, lane, bv, bias, nan_is_max, first);
#pragma unroll
    for (int u = 0; u < RU; ++u)
      if (lane == u0 + u) lab = first[u];
  }
  decode_count_chunk(lab, prev0, t0, lane, a, Tb, summaries + chunk * kDecodeSummary, values + chunk * kDecodeChunk);
}

__global__ void __launch_bounds__(256) decode_count_paths_kernel(const int32_t* __restrict__ paths, int64_t path_stride,
                                                                  DecodeArgs a, int32_t* __restrict__ summaries,
                                                                  int32_t* __restrict__ values) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= (int64_t)a.B * a.nch) return;
  const int b = (int)(chunk / a.nch), t0 = (int)(chunk % a.nch) * kDecodeChunk;
  const int32_t* row = paths + (int64_t)b * path_stride;
  const int lab = t0 + lane < a.T ? row[t0 + lane] : 0;
  const int prev0 = t0 > 0 ? row[t0 - 1] : -1;
  decode_count_chunk(lab, prev0, t0, lane, a, a.T, summaries + chunk * kDecodeSummary, values + chunk * kDecodeChunk);
}

// One wave per utterance: what crosses the chunk boundaries.  carry = the last kept value before the chunk (-1: none;
// labels are >= 0), running = the outputs before the chunk.
__global__ void __launch_bounds__(64) decode_scan_kernel(DecodeArgs a, int32_t* __restrict__ summaries,
                                                          int64_t* __restrict__ totals, int32_t* __restrict__ accepted) {
  const int lane = threadIdx.x, b = blockIdx.x;
  int32_t* rows = summaries + (int64_t)b * a.nch * kDecodeSummary;
  int carry = -1, running = 0;
  bool ok = true;
  for (int j0 = 0; j0 < a.nch; j0 += 64) {
    const int j = j0 + lane;
    const bool in = j < a.nch;
    int32_t* s = rows + (int64_t)(in ? j : 0) * kDecodeSummary;
    const int kept = in ? s[kSumKept] : 0, first = s[kSumFirst], last = s[kSumLast];
    int emit = in ? s[kSumEmit] : 0;
    ok = ok && (!in || s[kSumOk] != 0);
    const unsigned long long mask = __ballot(kept > 0);
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int near = __shfl(last, below ? 63 - __clzll(below) : lane, 64);
    const int cin = below ? near : carry;
    if (a.R > 0 && kept > 0 && first < a.R && cin >= a.R) emit += first + 1;  // a replabel that opens the chunk, behind a label
    const int incl = wave_inclusive_scan(emit, lane);
    if (in) s[kSumOffset] = running + incl - emit, s[kSumCarry] = cin;
    const int top = __shfl(last, mask ? 63 - __clzll(mask) : 0, 64);
    if (mask) carry = top;
    running += __shfl(incl, 63, 64);
  }
  ok = __ballot(!ok) == 0ull;
  if (lane == 0) {
    const bool take = ok || !(a.flags & WFL_DECODE_BLANK_SEPARATED);
    totals[b] = take ? running : 0;
    accepted[b] = take;
  }
}

__global__ void __launch_bounds__(256) decode_write_kernel(DecodeArgs a, const int32_t* __restrict__ summaries,
                                                            const int64_t* __restrict__ totals, const int32_t* __restrict__ accepted,
                                                            const int32_t* __restrict__ values, int32_t* __restrict__ out,
                                                            int64_t* __restrict__ out_offsets) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= (int64_t)a.B * a.nch) return;
  const int b = (int)(chunk / a.nch), ch = (int)(chunk % a.nch);
  long long base = 0;
  for (int r = lane; r < b; r += 64) base += totals[r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o, 64);
  if (ch == 0 && lane == 0) {
    out_offsets[b] = base;
    if (b == a.B - 1) out_offsets[a.B] = base + totals[b];
  }
  const int32_t* s = summaries + chunk * kDecodeSummary;
  const int kept = s[kSumKept];
  if (!accepted[b] || kept == 0) return;
  const int32_t* vals = values + chunk * kDecodeChunk;
  const bool have = lane < kept;
  const int v = have ? vals[lane] : 0;
  const int before = have ? (lane > 0 ? vals[lane - 1] : s[kSumCarry]) : -1;
  int emit = 0;
  if (have) emit = (a.R == 0 || v >= a.R) ? 1 : (before >= a.R ? v + 1 : 0);
  const int incl = wave_inclusive_scan(emit, lane);
  int32_t* dst = out + base + s[kSumOffset] + (incl - emit);
  const int value = (v >= a.R ? v : before) - a.R;
  for (int k = 0; k < emit; ++k) dst[k] = value;
}

}  // namespace wfl

using namespace wfl;

static int decode_check(const char* what, int B, int T, int drop, int R, int flags, const void* ws, const void* out,
                        int64_t out_capacity, const void* out_offsets, DecodeArgs* a) {
  if (B < 1 || T < 1 || R < 0 || drop < -1 || !ws || !out || !out_offsets ||
      (flags & ~(WFL_DECODE_NAN_IS_MAX | WFL_DECODE_BLANK_SEPARATED)) || ((flags & WFL_DECODE_BLANK_SEPARATED) && drop < 0)) {
    set_error("%s: bad arguments (B %d, T %d, drop %d, num_replabels %d, flags %d)", what, B, T, drop, R, flags);
    return WFL_ERR_INVALID;
  }
  const int64_t nch = ((int64_t)T + kDecodeChunk - 1) / kDecodeChunk;
  if ((int64_t)T * std::max(1, R) > 0x7fffffffLL || (int64_t)B * nch > 0x7fffffffLL) {
    set_error("%s: B %d, T %d, num_replabels %d is more than the index width of the decode takes", what, B, T, R);
    return WFL_ERR_UNSUPPORTED;
  }
  if (out_capacity < (int64_t)B * T * std::max(1, R)) {
    set_error("%s: out holds %lld labels, B T max(1, num_replabels) = %lld are needed", what, (long long)out_capacity,
              (long long)B * T * std::max(1, R));
    return WFL_ERR_INVALID;
  }
  *a = DecodeArgs{B, T, (int)nch, drop, R, flags};
  return WFL_OK;
}

// the scan and write launches behind a count launch
static int decode_finish(const DecodeArgs& a, void* ws, int32_t* out, int64_t* out_offsets, hipStream_t stream) {
  const DecodeWs w = decode_ws_layout(a.B, a.T);
  char* base = static_cast<char*>(ws);
  int32_t* summaries = reinterpret_cast<int32_t*>(base + w.summaries);
  int64_t* totals = reinterpret_cast<int64_t*>(base + w.totals);
  int32_t* accepted = reinterpret_cast<int32_t*>(base + w.accepted);
  const int32_t* values = reinterpret_cast<const int32_t*>(base + w.values);
  hipLaunchKernelGGL(decode_scan_kernel, dim3(a.B), dim3(64), 0, stream, a, summaries, totals, accepted);
  WFL_LAUNCH_CHECK();
  const unsigned grid = (unsigned)(((int64_t)a.B * a.nch + 3) / 4);
  hipLaunchKernelGGL(decode_write_kernel, dim3(grid), dim3(256), 0, stream, a, summaries, totals, accepted, values, out,
                     out_offsets);
  WFL_LAUNCH_CHECK();
  return WFL_OK;
}

extern "C" {

int wfl_decode_chunk_frames(void) { return kDecodeChunk; }

int wfl_decode_workspace(int B, int T, int num_replabels, int64_t* out_capacity, int64_t* ws_bytes) {
  if (B < 1 || T < 1 || num_replabels < 0 || !out_capacity || !ws_bytes) {
    set_error("decode_workspace: bad arguments (B %d, T %d, num_replabels %d)", B, T, num_replabels);
    return WFL_ERR_INVALID;
  }
  *out_capacity = (int64_t)B * T * std::max(1, num_replabels);
  *ws_bytes = decode_ws_layout(B, T).bytes;
  return WFL_OK;
}

static int decode_emissions_impl(const float* x, const float* bias, const int32_t* lengths, int B, int T, int C, int drop,
                                 int num_replabels, int flags, void* ws, int32_t* out, int64_t out_capacity,
                                 int64_t* out_offsets, void* stream) {
  DecodeArgs a;
  if (!x || C < 1 || drop >= C) {
    set_error("decode_emissions: bad arguments (C %d, drop %d)", C, drop);
    return WFL_ERR_INVALID;
  }
  if (const int rc = decode_check("decode_emissions", B, T, drop, num_replabels, flags, ws, out, out_capacity, out_offsets, &a)) return rc;
  const DecodeWs w = decode_ws_layout(B, T);
  int32_t* summaries = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + w.summaries);
  int32_t* values = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + w.values);
  const unsigned grid = (unsigned)(((int64_t)B * a.nch + 3) / 4);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, bias, lengths, C, a, summaries, values);
  };
  auto pick = [&](auto len) {
    constexpr bool LEN = decltype(len)::value;
    if (C <= 64)
      launch(decode_count_emissions_kernel<1, 16, LEN>);
    else if (C <= 128)
      launch(decode_count_emissions_kernel<2, 8, LEN>);
    else if (C <= 256)
      launch(decode_count_emissions_kernel<4, 4, LEN>);
    else if (C <= 512)
      launch(decode_count_emissions_kernel<8, 2, LEN>);
    else if (C <= 1024)
      launch(decode_count_emissions_kernel<16, 1, LEN>);
    else
      launch(decode_count_emissions_kernel<0, 1, LEN>);
  };
  if (lengths)
    pick(std::true_type{});
  else
    pick(std::false_type{});
  WFL_LAUNCH_CHECK();
  return decode_finish(a, ws, out, out_offsets, (hipStream_t)stream);
}

int wfl_decode_emissions(const float* x, const float* bias, int B, int T, int C, int drop, int num_replabels, int flags,
                         void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets, void* stream) {
  return decode_emissions_impl(x, bias, nullptr, B, T, C, drop, num_replabels, flags, ws, out, out_capacity, out_offsets, stream);
}

int wfl_decode_emissions_lengths(const float* x, const float* bias, const int32_t* lengths, int B, int T, int C, int drop,
                                 int num_replabels, int flags, void* ws, int32_t* out, int64_t out_capacity,
                                 int64_t* out_offsets, void* stream) {
  if (!lengths) {
    set_error("decode_emissions_lengths: lengths is NULL (wfl_decode_emissions decodes every frame)");
    return WFL_ERR_INVALID;
  }
  return decode_emissions_impl(x, bias, lengths, B, T, C, drop, num_replabels, flags, ws, out, out_capacity, out_offsets,
                               stream);
}

int wfl_decode_paths(const int32_t* paths, int64_t path_stride, int B, int T, int drop, int num_replabels, int flags,
                     void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets, void* stream) {
  DecodeArgs a;
  if (!paths || path_stride < T || (flags & WFL_DECODE_NAN_IS_MAX)) {
    set_error("decode_paths: bad arguments (path_stride %lld, T %d, flags %d)", (long long)path_stride, T, flags);
    return WFL_ERR_INVALID;
  }
  if (const int rc = decode_check("decode_paths", B, T, drop, num_replabels, flags, ws, out, out_capacity, out_offsets, &a)) return rc;
  const DecodeWs w = decode_ws_layout(B, T);
  int32_t* summaries = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + w.summaries);
  int32_t* values = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + w.values);
  const unsigned grid = (unsigned)(((int64_t)B * a.nch + 3) / 4);
  hipLaunchKernelGGL(decode_count_paths_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, paths, path_stride, a, summaries,
                     values);
  WFL_LAUNCH_CHECK();
  return decode_finish(a, ws, out, out_offsets, (hipStream_t)stream);
}

}  // extern "C"
