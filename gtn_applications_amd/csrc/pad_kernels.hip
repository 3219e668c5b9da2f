// Per-utterance input lengths of a padded CTC batch (criterions/ctc.py, `input_lengths`): the two bandwidth kernels
// around a criterion launch that itself sweeps all T frames of every utterance.
//
// The rule ("Input lengths as certain-blank frames"): for the CTC label graph a frame whose emissions are 0
// for the blank and -inf for every other class is the identity -- the only finite arcs are the blank's self loop on the
// last blank and the blank arc from the last label into it, so the T-frame score with such frames at t >= T_b is the
// T_b-frame score, the posteriors of the frames before T_b are unchanged and those of the pad frames sit on the blank.
//   ctc_pad_frames: out = x with the rows t >= lengths[b] replaced by those constants (the criterion runs on `out`);
//   zero_pad_rows:  dx[b, t, :] = 0 for t >= lengths[b], nothing else touched (the constants do not depend on x).
// One wave per row, lanes along the classes; the test on lengths[b] is wave-uniform.
#include <algorithm>

#include "device_common.h"

namespace wfl {

constexpr int kPadRowsPerBlock = 4;  // waves of a workgroup = rows it takes

__global__ void __launch_bounds__(64 * kPadRowsPerBlock)
    ctc_pad_frames_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths, int64_t rows, int T, int C,
                          int blank, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kPadRowsPerBlock + (threadIdx.x >> 6);
  if (row >= rows) return;  // (a whole wave)
  const int b = (int)(row / T), t = (int)(row % T);
  const bool pad = t >= lengths[b];
  const float* src = x + row * C;
  float* dst = out + row * C;
  const float ninf = -__builtin_inff();
  if (pad) {
    for (int c = lane; c < C; c += 64) dst[c] = c == blank ? 0.f : ninf;
  } else {
    for (int c = lane; c < C; c += 64) dst[c] = src[c];
  }
}

__global__ void __launch_bounds__(64 * kPadRowsPerBlock)
    zero_pad_rows_kernel(float* __restrict__ dx, const int32_t* __restrict__ lengths, int64_t rows, int T, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kPadRowsPerBlock + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = (int)(row / T), t = (int)(row % T);
  if (t < lengths[b]) return;
  float* dst = dx + row * C;
  for (int c = lane; c < C; c += 64) dst[c] = 0.f;
}

}  // namespace wfl

using namespace wfl;

static int pad_check(const char* what, const void* p, const int32_t* lengths, int B, int T, int C, int64_t* rows) {
  if (!p || !lengths || B < 1 || T < 1 || C < 1) {
    set_error("%s: bad arguments (B %d, T %d, C %d)", what, B, T, C);
    return WFL_ERR_INVALID;
  }
  *rows = (int64_t)B * T;
  if ((*rows + kPadRowsPerBlock - 1) / kPadRowsPerBlock > 0x7fffffffLL) {
    set_error("%s: B %d x T %d rows are more than one grid takes", what, B, T);
    return WFL_ERR_UNSUPPORTED;
  }
  return WFL_OK;
}

extern "C" {

int wfl_ctc_pad_frames(const float* x, const int32_t* lengths, int B, int T, int C, int blank, float* out, void* stream) {
  int64_t rows = 0;
  if (const int rc = pad_check("ctc_pad_frames", x, lengths, B, T, C, &rows)) return rc;
  if (!out || out == x || blank < 0 || blank >= C) {
    set_error("ctc_pad_frames: bad arguments (blank %d of %d classes; out must be a buffer of its own)", blank, C);
    return WFL_ERR_INVALID;
  }
  const unsigned grid = (unsigned)((rows + kPadRowsPerBlock - 1) / kPadRowsPerBlock);
  hipLaunchKernelGGL(ctc_pad_frames_kernel, dim3(grid), dim3(64 * kPadRowsPerBlock), 0, (hipStream_t)stream, x, lengths, rows,
                     T, C, blank, out);
  WFL_LAUNCH_CHECK();
  return WFL_OK;
}

int wfl_zero_pad_rows(float* dx, const int32_t* lengths, int B, int T, int C, void* stream) {
  int64_t rows = 0;
  if (const int rc = pad_check("zero_pad_rows", dx, lengths, B, T, C, &rows)) return rc;
  const unsigned grid = (unsigned)((rows + kPadRowsPerBlock - 1) / kPadRowsPerBlock);
  hipLaunchKernelGGL(zero_pad_rows_kernel, dim3(grid), dim3(64 * kPadRowsPerBlock), 0, (hipStream_t)stream, dx, lengths, rows,
                     T, C);
  WFL_LAUNCH_CHECK();
  return WFL_OK;
}

}  // extern "C"
