// Where the lattice engine keeps its bookkeeping in the alpha and beta buffers (lattice_kernels.hip, lattice_streamed.h).
// Plain C++ outside hipcc: lattice_layout_check.cpp prints the layout on the host.
#pragma once
#include <cstdint>
#include "../../include/wfl.h"
#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace wfl {
constexpr int kDumpDoubles = 1024;  // where lanes without a state of the unrolled sweeps "store" (run_chain_prob)
constexpr int kLiveTile = 32;  // frames per job of the gradient beside the sweeps (at least: T / tiles, rounded up)
                               // (40 / 48 / 56 / 64 with the gradient in two phases, same box, three runs each: 0.324-0.326 / 0.307-0.317 /
                               //  0.307-0.310 / 0.335-0.337 against 0.309-0.335 -- inside the runs' own spread)
// xg: log-domain rows | probability-domain factors of the same rows | one reference per row; floats of each of the first two
__host__ __device__ inline int64_t xg_main(const wfl_lattice_desc& d, int T) { return (((int64_t)d.B * T * d.max_labels) + 3) & ~(int64_t)3; }
// floats of the score arrays in front of the tail (float | double: room for doubles)
__host__ __device__ inline int64_t ab_main_elems(const wfl_lattice_desc& d, int T) {
  return 2 * (d.shared ? (int64_t)d.B * (T + 1) * d.max_states : (int64_t)(T + 1) * d.total_states);
}
// header of the gradient beside the sweeps (AbTail::occ_header): uint32 words of the alpha buffer
struct OccHeader {
  uint32_t* bad;    // [B]
  int32_t* nx;      // [8]  utterances whose sweeps run on XCD x
  uint32_t* next;   // [8]  next job of XCD x
  int32_t* list;    // [8][B]
  uint32_t* busy;   // [8][256]  == token while a sweep runs on CU (xcc, HW_ID[15:8])
  uint32_t* meta;   // [2]       the launch's token and its tiles per utterance (for served_beside_the_sweeps)
  uint32_t* next_base;  // [8]   next base-row job of XCD x (occ_live_kernel, first phase)
  uint32_t* based;  // [B][tiles] == token once the tile's base rows are written
};

// The tail: what the sweeps leave behind the score arrays, `tail` floats (even: 8-byte aligned) into the alpha and the
// beta buffer.  Both buffers have this layout and wfl_lattice_workspace's size; B = d.B, nch1 = T + 1:
//   field    type                  alpha buffer                                   beta buffer
//   offs     double [B][nch1]      log offsets of the stored scores, per slot     the same, of the backward sweep
//   z        double [B]            ln Z (log2 Z: probability-domain utterances)   Z as the backward sweep sees it
//   fmt      int32  [B]            the sweep format: kFmtLog / kFmtProb / kFmtOcc \ verdict double [B] of prob_certify_kernel:
//   wref     float  [B]            reference of the arc weight factors            / 0 certified, 1 re-run in the log domain
//   dump     double [kDumpDoubles] nobody reads it; one unused double follows     the same
//   prog     uint64 [B]            progress word of the forward sweep             of the backward sweep
//   bad      uint32 [B, even]      token: the gradient workgroups gave up on b    1: the backward sweep stored occupancies
//   nx .. based  (OccHeader)       lists and counters of the gradient workgroups  unused
//   spare    2 B - (B & 1) + 26 floats of unused reserve in both, kept so that no size and no offset behind the tail moves
// An accessor without a buffer gives the field's offset from the tail's start in the field's own unit, one with a buffer
// the pointer; end_floats() and total_floats() count from the buffer's start.
struct AbTail {
  int64_t tail, B;
  int nch1;
  __host__ __device__ AbTail(const wfl_lattice_desc& d, int64_t tail_, int nch1_) : tail(tail_), B(d.B), nch1(nch1_) {}
  __host__ __device__ int64_t offs(int b) const { return (int64_t)b * nch1; }
  __host__ __device__ int64_t z(int b) const { return B * nch1 + b; }
  __host__ __device__ int64_t fmt(int b) const { return 2 * (z(0) + B) + b; }
  __host__ __device__ int64_t wref(int b) const { return fmt(0) + B + b; }
  __host__ __device__ int64_t verdict(int b) const { return z(0) + B + b; }
  __host__ __device__ int64_t dump() const { return z(0) + 2 * B; }
  __host__ __device__ int64_t prog(int b) const { return dump() + kDumpDoubles + 1 + b; }
  __host__ __device__ int64_t bad(int b) const { return 2 * prog(0) + 2 * B + b; }
  __host__ __device__ int64_t nx() const { return bad(0) + ((B + 1) & ~(int64_t)1); }
  __host__ __device__ int64_t next() const { return nx() + 8; }
  __host__ __device__ int64_t list() const { return next() + 8; }
  __host__ __device__ int64_t busy() const { return list() + 8 * B; }
  __host__ __device__ int64_t meta() const { return busy() + 8 * 256; }
  __host__ __device__ int64_t next_base() const { return meta() + 2; }
  __host__ __device__ int64_t based() const { return next_base() + 8; }
  __host__ __device__ int live_tiles() const { return (nch1 - 1) / kLiveTile + 1; }  // the most a launch cuts T frames into
  __host__ __device__ int64_t end_floats() const { return tail + based() + B * live_tiles(); }
  __host__ __device__ int64_t spare_floats() const { return 2 * B - (B & 1) + 26; }
  __host__ __device__ int64_t total_floats() const { return end_floats() + spare_floats(); }
  __host__ __device__ double* offs(float* ab, int b) const { return reinterpret_cast<double*>(ab + tail) + offs(b); }
  __host__ __device__ const double* offs(const float* ab, int b) const { return offs(const_cast<float*>(ab), b); }
  __host__ __device__ double* z(float* ab, int b) const { return reinterpret_cast<double*>(ab + tail) + z(b); }
  __host__ __device__ const double* z(const float* ab, int b) const { return z(const_cast<float*>(ab), b); }
  __host__ __device__ int32_t* fmt(float* alpha, int b) const { return reinterpret_cast<int32_t*>(alpha + tail) + fmt(b); }
  __host__ __device__ const int32_t* fmt(const float* alpha, int b) const { return fmt(const_cast<float*>(alpha), b); }
  __host__ __device__ float* wref(float* alpha, int b) const { return alpha + tail + wref(b); }
  __host__ __device__ const float* wref(const float* alpha, int b) const { return alpha + tail + wref(b); }
  __host__ __device__ double* verdict(float* beta, int b) const { return reinterpret_cast<double*>(beta + tail) + verdict(b); }
  __host__ __device__ double* dump(float* ab) const { return reinterpret_cast<double*>(ab + tail) + dump(); }
  __host__ __device__ uint64_t* prog(float* ab, int b) const { return reinterpret_cast<uint64_t*>(ab + tail) + prog(b); }
  __host__ __device__ OccHeader occ_header(float* ab) const {  // (of the beta buffer: `bad` only)
    uint32_t* w = reinterpret_cast<uint32_t*>(ab + tail);
    int32_t* i = reinterpret_cast<int32_t*>(w);
    return OccHeader{w + bad(0), i + nx(), w + next(), i + list(), w + busy(), w + meta(), w + next_base(), w + based()};
  }
};
// one offset per time slot (probability domain; the log domain uses one per chunk) behind the score arrays
__host__ __device__ inline AbTail ab_tail(const wfl_lattice_desc& d, int T) { return AbTail(d, ab_main_elems(d, T), T + 1); }
}  // namespace wfl
