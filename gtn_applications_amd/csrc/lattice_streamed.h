// Streamed sweeps of the generic lattice engine: acceptors whose arcs do not fit one CU's LDS (included by
// lattice_kernels.hip inside namespace wfl; the host side is there too, next to the tuned launches).
//
// run_chain stages the whole acceptor in LDS.  Beyond 160 KiB (a pruned back-off bigram over 1 000 word pieces: 55 K
// arcs, ~485 KB; CTC targets of ~1 650 labels and more) these kernels sweep it instead:
//   stream_stage_kernel   once per call: every arc as {other state | slot << 16, weight} in both CSR orders (by
//                         destination for alpha, by source for beta), epsilon arcs likewise, a by-slot copy for the
//                         gradient, and per direction the lists of states with more than kStreamHeavy in-arcs
//                         (labelled, epsilon).  The learnable weights are added here, NaN -> -inf as run_chain does.
//                         A shared graph has ONE copy for the whole batch (0.9 MB at 55 K arcs: resident in L2).
//   stream_chain_kernel   one 1 024-thread workgroup per (utterance, direction), as chain_kernel.  Arcs are read from
//                         global memory every frame; state vectors double-buffered in LDS where 2 Q doubles fit
//                         (LDSST), otherwise the alpha / beta output rows themselves (the frame just written is read
//                         back after a barrier: everything stays inside the workgroup).  Emission rows are staged a
//                         chunk of R frames ahead, the epsilon closure runs by levels, and the per-chunk double
//                         offsets of run_chain keep alpha / beta in the layout grad_kernel and backtrace_kernel read.
//   stream_grad_kernel    dense emission gradient rows: one workgroup per (utterance, tile of frames), threads own
//                         16 consecutive by-slot arcs of one frame and add their posteriors to a compact
//                         [frames][labels] tile in LDS; rows streamed out as grad_kernel does (stream_grad_rows).
//   stream_dw_kernel      learnable-weight gradient, arc-major: a thread owns an arc of one utterance and loops over
//                         the frames in registers -- one global atomic per arc and workgroup.
// Relaxation semantics are run_chain's: arcs in CSR order, strict '>' (tropical ties keep the lowest arc index; an
// epsilon arc replaces the labelled back-pointer only if strictly better), double state values in the log semiring.

constexpr int kStreamThreads = 1024;  // threads of a sweep workgroup
constexpr int kStreamHeavy = 32;      // in-degree (labelled or epsilon) from which a whole wave relaxes a state
constexpr int kStreamChunk = 16;      // by-slot arcs per work item of the emission gradient

struct StreamArea {
  int2* arcs[2];  // [total_arcs] per direction, that direction's CSR order: {other | slot << 16, weight bits}
  int2* sarc;     // [total_arcs] by slot (slot_arc order): {src | dst << 16, weight bits}
  int2* eps[2];   // [total_eps] per direction: {other, weight bits}
  int* heavy[2];  // [2 (total_states + B)] per direction; graph g at 2 (s0_g + g): {n_lab, n_eps, lab[Q], eps[Q]}
};
// int32 words of the area (behind the tuned layout of the alpha buffer: wfl_lattice_workspace)
__host__ __device__ inline int64_t stream_area_words(const wfl_lattice_desc& d) {
  return 6 * d.total_arcs + 4 * d.total_eps + 4 * (d.total_states + d.B) + 4;
}
__host__ __device__ inline StreamArea stream_area(const wfl_lattice_desc& d, int32_t* base) {
  StreamArea s;
  int2* p = reinterpret_cast<int2*>(base);
  s.arcs[0] = p, p += d.total_arcs;
  s.arcs[1] = p, p += d.total_arcs;
  s.sarc = p, p += d.total_arcs;
  s.eps[0] = p, p += d.total_eps;
  s.eps[1] = p, p += d.total_eps;
  int* h = reinterpret_cast<int*>(p);
  s.heavy[0] = h, h += 2 * (d.total_states + d.B);
  s.heavy[1] = h;
  return s;
}

template <typename V>
__device__ __forceinline__ V wave_max64(V v) {  // every lane receives the wave's maximum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const V w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_min64(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

// grid (blocks, graphs): graph g = utterance, or 0 for a shared descriptor
__global__ void __launch_bounds__(256) stream_stage_kernel(wfl_lattice_desc d, const int32_t* __restrict__ ints,
                                                            const float* __restrict__ floats,
                                                            const float* __restrict__ weights, int32_t* __restrict__ base) {
  const int g = blockIdx.y;
  const UttView u = make_view(d, ints, floats, g, 0);
  const StreamArea S = stream_area(d, base);
  const int A = u.A, E = u.E, Q = u.Q;
  auto wt = [&](float w, int wid) {
    if (weights && wid >= 0) w += nan_to_neg(weights[wid]);
    return __float_as_int(w);
  };
  const int n = 3 * A + 2 * E;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    if (i < 2 * A) {
      const int dir = i >= A, k = i - dir * A;
      const int a = dir == 0 ? k : u.out_arc[k];
      const int other = dir == 0 ? u.arc_src[a] : u.arc_dst[a];
      S.arcs[dir][u.a0 + k] = make_int2(other | (u.arc_slot[a] << 16), wt(u.arc_w[a], u.arc_wid[a]));
    } else if (i < 3 * A) {
      const int j = i - 2 * A, a = u.slot_arc[j];
      S.sarc[u.a0 + j] = make_int2(u.arc_src[a] | (u.arc_dst[a] << 16), wt(u.arc_w[a], u.arc_wid[a]));
    } else {
      const int i2 = i - 3 * A, dir = i2 >= E, k = i2 - dir * E;
      const int e = dir == 0 ? k : u.eout_arc[k];
      const int other = dir == 0 ? u.eps_src[e] : u.eps_dst[e];
      S.eps[dir][u.e0 + k] = make_int2(other, wt(u.eps_w[e], u.eps_wid[e]));
    }
  }
  if (blockIdx.x != 0) return;
  __shared__ int cnt[4];
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int s0 = ints[d.state_off + g];
  int* h0 = S.heavy[0] + 2 * ((int64_t)s0 + g);
  int* h1 = S.heavy[1] + 2 * ((int64_t)s0 + g);
  for (int q = threadIdx.x; q < Q; q += 256) {  // (list order does not matter: every state is relaxed on its own)
    if (u.in_ptr[q + 1] - u.in_ptr[q] > kStreamHeavy) h0[2 + atomicAdd(&cnt[0], 1)] = q;
    if (u.ein_ptr[q + 1] - u.ein_ptr[q] > kStreamHeavy) h0[2 + Q + atomicAdd(&cnt[1], 1)] = q;
    if (u.out_ptr[q + 1] - u.out_ptr[q] > kStreamHeavy) h1[2 + atomicAdd(&cnt[2], 1)] = q;
    if (u.eout_ptr[q + 1] - u.eout_ptr[q] > kStreamHeavy) h1[2 + Q + atomicAdd(&cnt[3], 1)] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) h0[0] = cnt[0], h0[1] = cnt[1], h1[0] = cnt[2], h1[1] = cnt[3];
}

template <int SR, int DIR, bool LDSST>
__device__ void run_stream(const wfl_lattice_desc& d, const UttView& u, const StreamArea& S, int g, int s0, char* smem,
                           int T, int R, const float* __restrict__ xg, float* __restrict__ out_f, int32_t* __restrict__ bptr,
                           float* __restrict__ logz, int b, double* __restrict__ offs, double* __restrict__ z64) {
  using VT = typename ChainVal<SR>::type;
  constexpr bool TROP = SR == WFL_SEMIRING_TROPICAL;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
  const int Q = u.Q, A = u.A, nlev = u.nlev, Kmax = d.max_labels;
  VT* const out = reinterpret_cast<VT*>(out_f);
  const int2* __restrict__ arcs = S.arcs[DIR] + u.a0;
  const int2* __restrict__ eps = S.eps[DIR] + u.e0;
  const int* __restrict__ ptr = DIR == 0 ? u.in_ptr : u.out_ptr;
  const int* __restrict__ eptr = DIR == 0 ? u.ein_ptr : u.eout_ptr;
  const int* __restrict__ hv = S.heavy[DIR] + 2 * ((int64_t)s0 + g);
  const int n_heavy = hv[0], n_heavy_e = hv[1];
  const int* __restrict__ heavy = hv + 2;
  const int* __restrict__ heavy_e = hv + 2 + Q;
  float* rows = reinterpret_cast<float*>(smem);  // [2][R][Kmax] (R even: 8-byte aligned behind it)
  float* red = rows + (size_t)2 * R * Kmax;      // [64]
  VT* buf0 = reinterpret_cast<VT*>(red + 64);    // LDSST: [Qmax] each
  VT* buf1 = buf0 + d.max_states;
  auto vec = [&](int slot) -> VT* {
    if (LDSST) return (slot & 1) ? buf1 : buf0;
    return out + u.ab_base + (int64_t)slot * Q;
  };
  const int2 pad = make_int2(0, __float_as_int(WFL_NEG_INF));
  auto accum = [&](VT v, VT& m, VT& s) {  // streaming log-add (m = -inf: s is 0 and exp(-inf) = 0)
    if (v > m) {
      s = s * (VT)lse_exp((float)(m - v)) + 1;
      m = v;
    } else if (v > WFL_NEG_INF) {
      s += (VT)lse_exp((float)(v - m));
    }
  };
  // one state's labelled in-arcs [k0, k1), by one thread; `sub` is subtracted from every `from` value (the chunk's
  // renormalisation when the vectors live in global memory)
  auto relax_light = [&](const VT* from, VT sub, const float* row, int k0, int k1, VT& val, int& arg) {
    VT m = WFL_NEG_INF, s = 0;
    int am = -1;
    for (int k = k0; k < k1; k += 4) {
      int2 a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = k + j < k1 ? arcs[k + j] : pad;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const VT v = (from[a[j].x & 0xffff] - sub) + (VT)row[(unsigned)a[j].x >> 16] + (VT)__int_as_float(a[j].y);
        if (TROP) {
          if (v > m) m = v, am = k + j;
        } else {
          accum(v, m, s);
        }
      }
    }
    if (!TROP && m > WFL_NEG_INF) m += (VT)lse_log((double)s);
    val = m, arg = am;
  };
  // the same by a whole wave (uniform k0, k1): lanes stride over the list, ascending within a lane
  auto relax_wave = [&](const VT* from, VT sub, const float* row, int k0, int k1, VT& val, int& arg) {
    VT m = WFL_NEG_INF, s = 0;
    int am = 0x7fffffff;
    for (int k = k0 + lane; k < k1; k += 256) {
      int2 a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = k + 64 * j < k1 ? arcs[k + 64 * j] : pad;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const VT v = (from[a[j].x & 0xffff] - sub) + (VT)row[(unsigned)a[j].x >> 16] + (VT)__int_as_float(a[j].y);
        if (TROP) {
          if (v > m) m = v, am = k + 64 * j;
        } else {
          accum(v, m, s);
        }
      }
    }
    const VT mt = wave_max64(m);
    if (TROP) {
      const int cand = wave_min64((m == mt && mt > WFL_NEG_INF) ? am : 0x7fffffff);
      val = mt, arg = cand == 0x7fffffff ? -1 : cand;
    } else {
      const double st = wave_sum64(m > WFL_NEG_INF ? (double)s * (double)lse_exp((float)(m - mt)) : 0.0);
      val = mt > WFL_NEG_INF ? mt + (VT)lse_log(st) : (VT)WFL_NEG_INF, arg = -1;
    }
  };
  // epsilon in-arcs of a state whose labelled result is `val` (the other endpoints are final)
  auto relax_eps_light = [&](const VT* vals, int k0, int k1, VT& val, int& arg) {
    VT m = val, s = val > WFL_NEG_INF ? 1 : 0;
    int am = arg;
    for (int k = k0; k < k1; k += 4) {
      int2 a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = k + j < k1 ? eps[k + j] : pad;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const VT v = vals[a[j].x] + (VT)__int_as_float(a[j].y);
        if (TROP) {
          if (v > m) m = v, am = A + k + j;
        } else {
          accum(v, m, s);
        }
      }
    }
    if (!TROP && m > WFL_NEG_INF) m += (VT)lse_log((double)s);
    val = m, arg = am;
  };
  auto relax_eps_wave = [&](const VT* vals, int k0, int k1, VT& val, int& arg) {
    VT m = WFL_NEG_INF, s = 0;
    int am = 0x7fffffff;
    for (int k = k0 + lane; k < k1; k += 256) {
      int2 a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = k + 64 * j < k1 ? eps[k + 64 * j] : pad;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const VT v = vals[a[j].x] + (VT)__int_as_float(a[j].y);
        if (TROP) {
          if (v > m) m = v, am = A + k + 64 * j;
        } else {
          accum(v, m, s);
        }
      }
    }
    const VT mt = wave_max64(m);
    if (TROP) {
      if (mt > val) {  // (uniform) an epsilon arc replaces the labelled back-pointer only if strictly better
        arg = wave_min64(m == mt ? am : 0x7fffffff);
        val = mt;
      }
    } else {
      const VT top = mt > val ? mt : val;
      if (top > WFL_NEG_INF) {
        double st = wave_sum64(m > WFL_NEG_INF ? (double)s * (double)lse_exp((float)(m - top)) : 0.0);
        if (val > WFL_NEG_INF) st += (double)lse_exp((float)(val - top));
        val = top + (VT)lse_log(st);
      }
    }
  };
  auto closure = [&](VT* vals, int tslot) {
    if (nlev <= 1) return;
    int32_t* bp = TROP && DIR == 0 ? bptr + u.ab_base + (int64_t)tslot * Q : nullptr;
    for (int step = 1; step < nlev; ++step) {
      const int lev = DIR == 0 ? step : nlev - 1 - step;
      __syncthreads();
      const int q0 = u.lvl_ptr[lev], q1 = u.lvl_ptr[lev + 1];
      for (int q = q0 + tid; q < q1; q += NT) {
        const int k0 = eptr[q], k1 = eptr[q + 1];
        if (k1 == k0 || k1 - k0 > kStreamHeavy) continue;
        VT v = vals[q];
        int arg = -2;
        relax_eps_light(vals, k0, k1, v, arg);
        vals[q] = v;
        if (bp && arg != -2) bp[q] = arg;
      }
      for (int h = wave; h < n_heavy_e; h += nw) {
        const int q = heavy_e[h];
        if (q < q0 || q >= q1) continue;  // (uniform within the wave)
        VT v = vals[q];
        int arg = -2;
        relax_eps_wave(vals, eptr[q], eptr[q + 1], v, arg);
        if (lane == 0) {
          vals[q] = v;
          if (bp && arg != -2) bp[q] = arg;
        }
      }
    }
  };

  double cum = 0.0;
  if (!TROP && tid == 0) offs[0] = 0.0;
  const int t_first = DIR == 0 ? 0 : T;
  {
    VT* cur = vec(t_first);
    for (int q = tid; q < Q; q += NT) {
      cur[q] = (VT)(DIR == 0 ? u.start_w[q] : u.accept_w[q]);
      if (TROP && DIR == 0) bptr[u.ab_base + q] = -1;
    }
    closure(cur, t_first);
    __syncthreads();
    if (LDSST)
      for (int q = tid; q < Q; q += NT) out[u.ab_base + (int64_t)t_first * Q + q] = cur[q];
  }
  const int nchunks = (T + R - 1) / R;
  auto chunk_frames = [&](int c, int& f0, int& n) {  // frames [f0, f0+n) in ascending order
    const int c0 = c * R;
    n = min(R, T - c0);
    f0 = DIR == 0 ? c0 : T - c0 - n;
  };
  if (T > 0) {
    int f0, n;
    chunk_frames(0, f0, n);
    const float* src = xg + u.xg_base + (int64_t)f0 * Kmax;
    for (int e = tid; e < n * Kmax; e += NT) rows[e] = src[e];
  }
  __syncthreads();
  const int kq0 = tid < Q ? ptr[tid] : 0, kq1 = tid < Q ? ptr[tid + 1] : 0;
  const bool direct = nlev <= 1;  // no epsilon closure: the relaxed value is final
  VT shift = 0;
  for (int c = 0; c < nchunks; ++c) {
    int f0, n;
    chunk_frames(c, f0, n);
    const float* tile = rows + (size_t)(c & 1) * R * Kmax;
    float pre[kPre];
    int pn = 0;
    if (c + 1 < nchunks) {
      int pf0;
      chunk_frames(c + 1, pf0, pn);
      const float* src = xg + u.xg_base + (int64_t)pf0 * Kmax;
#pragma unroll
      for (int j = 0; j < kPre; ++j) {
        const int e = tid + j * NT;
        if (e < pn * Kmax) pre[j] = src[e];
      }
    }
    if (!TROP) {
      if (c > 0) {
        VT* fromb = vec(DIR == 0 ? f0 : f0 + n);  // slot the first frame of the chunk reads
        float v = WFL_NEG_INF;
        for (int q = tid; q < Q; q += NT) v = fmaxf(v, (float)fromb[q]);
        float m = block_reduce_max(v, red);
        if (!(m > WFL_NEG_INF && m < __builtin_inff())) m = 0.f;
        if (LDSST) {
          if (m != 0.f)
            for (int q = tid; q < Q; q += NT) fromb[q] -= (VT)m;
        } else {
          shift = (VT)m;  // (the stored slot keeps its own chunk's offset: subtracted as it is read)
        }
        __syncthreads();
        cum += (double)m;
      }
      if (tid == 0) offs[1 + c] = cum;
    }
    for (int i = 0; i < n; ++i) {
      // forward: consume frame t, produce slot t+1.  backward: consume frame t, produce slot t.
      const int t = DIR == 0 ? f0 + i : f0 + n - 1 - i;
      const int slot_from = DIR == 0 ? t : t + 1, slot_to = DIR == 0 ? t + 1 : t;
      const VT* from = vec(slot_from);
      VT* to = vec(slot_to);
      const VT sub = (!LDSST && i == 0) ? shift : (VT)0;
      const float* row = tile + (size_t)(t - f0) * Kmax;
      VT* orow = out + u.ab_base + (int64_t)slot_to * Q;
      int32_t* bp = TROP && DIR == 0 ? bptr + u.ab_base + (int64_t)slot_to * Q : nullptr;
      for (int q = tid; q < Q; q += NT) {
        const int k0 = q == tid ? kq0 : ptr[q], k1 = q == tid ? kq1 : ptr[q + 1];
        if (k1 - k0 > kStreamHeavy) continue;
        VT v;
        int arg;
        relax_light(from, sub, row, k0, k1, v, arg);
        to[q] = v;
        if (LDSST && direct) orow[q] = v;
        if (bp) bp[q] = arg;
      }
      for (int h = wave; h < n_heavy; h += nw) {
        const int q = heavy[h];
        VT v;
        int arg;
        relax_wave(from, sub, row, ptr[q], ptr[q + 1], v, arg);
        if (lane == 0) {
          to[q] = v;
          if (LDSST && direct) orow[q] = v;
          if (bp) bp[q] = arg;
        }
      }
      closure(to, slot_to);
      __syncthreads();
      if (LDSST && !direct)
        for (int q = tid; q < Q; q += NT) orow[q] = to[q];
    }
    if (c + 1 < nchunks) {
      float* dst = rows + (size_t)((c + 1) & 1) * R * Kmax;
#pragma unroll
      for (int j = 0; j < kPre; ++j) {
        const int e = tid + j * NT;
        if (e < pn * Kmax) dst[e] = pre[j];
      }
      __syncthreads();
    }
  }
  if (DIR == 0 && logz) {
    const VT* fin = vec(T);
    float m = WFL_NEG_INF;
    for (int q = tid; q < Q; q += NT) m = fmaxf(m, (float)(fin[q] + (VT)u.accept_w[q]));
    m = block_reduce_max(m, red);
    double z = m;
    if (!TROP && m > WFL_NEG_INF) {
      float s = 0.f;
      for (int q = tid; q < Q; q += NT) s += fast_exp((float)(fin[q] + (VT)u.accept_w[q] - (VT)m));
      s = block_reduce_sum(s, red);
      z = (double)m + lse_log((double)s);
    }
    if (tid == 0) {
      const double zd = z + cum;  // (-inf + cum = -inf: no accepting path)
      logz[b] = (float)zd;
      if (!TROP) z64[b] = zd;
    }
  }
}

// grid (B, directions).  Behind the score arrays the tuned layout (AbTail), stream_stage_kernel's area at alpha + area_off.
template <int SR, bool LDSST>
__global__ void __launch_bounds__(kStreamThreads)
    stream_chain_kernel(wfl_lattice_desc d, const int32_t* __restrict__ ints, const float* __restrict__ floats,
                        const float* __restrict__ xg, int T, int R, float* __restrict__ alpha, float* __restrict__ beta,
                        int32_t* __restrict__ bptr, float* __restrict__ logz, int64_t tail, int nch1, int64_t area_off) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x, dir = blockIdx.y;
  const UttView u = make_view(d, ints, floats, b, T);
  const int g = d.shared ? 0 : b;
  const int s0 = ints[d.state_off + g];
  const StreamArea S = stream_area(d, reinterpret_cast<int32_t*>(alpha + area_off));
  const AbTail lay(d, tail, nch1);
  if (SR == WFL_SEMIRING_LOG && dir == 0 && threadIdx.x == 0) *lay.fmt(alpha, b) = kFmtLog;
  if (dir == 0)
    run_stream<SR, 0, LDSST>(d, u, S, g, s0, smem, T, R, xg, alpha, bptr, logz, b, lay.offs(alpha, b), lay.z(alpha, 0));
  else
    run_stream<SR, 1, LDSST>(d, u, S, g, s0, smem, T, R, xg, beta, nullptr, nullptr, b, lay.offs(beta, b), nullptr);
}

// offset index of a slot: alpha slot s belongs to chunk (s-1)/R of the forward sweep, beta slot s to chunk (T-1-s)/R of
// the backward sweep, the boundary slots to offset 0 (run_chain, run_stream)
__device__ __forceinline__ int offs_index_a(int s, int R) { return s == 0 ? 0 : 1 + (s - 1) / R; }
__device__ __forceinline__ int offs_index_b(int s, int T, int R) { return s == T ? 0 : 1 + (T - 1 - s) / R; }

// grid (tiles of TS frames, B), 256 threads.  LDS: acc [TS][Kmax] | corr [TS] | slot pointers [Kmax + 2] | colmap [C]
__global__ void __launch_bounds__(256)
    stream_grad_kernel(wfl_lattice_desc d, const int32_t* __restrict__ ints, const float* __restrict__ floats,
                       const float* __restrict__ xg, int T, int C, int R, const float* __restrict__ alpha,
                       const float* __restrict__ beta, const float* __restrict__ logz, const float* __restrict__ coef,
                       const float* __restrict__ gout, int accumulate, const float* __restrict__ x,
                       const float* __restrict__ row_lse, float* __restrict__ dx, int TS, int64_t tail, int nch1,
                       int64_t area_off) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.y, tid = threadIdx.x, NT = blockDim.x;
  const UttView u = make_view(d, ints, floats, b, T);
  const int Q = u.Q, K = u.K, A = u.A, Kmax = d.max_labels;
  const StreamArea S = stream_area(d, const_cast<int32_t*>(reinterpret_cast<const int32_t*>(alpha + area_off)));
  const int2* __restrict__ sarc = S.sarc + u.a0;
  const AbTail lay(d, tail, nch1);
  const double *offs_a = lay.offs(alpha, b), *offs_b = lay.offs(beta, b);
  const double zd = *lay.z(alpha, b);
  float* acc = reinterpret_cast<float*>(smem);
  double* corr = reinterpret_cast<double*>(acc + (((size_t)TS * Kmax + 1) & ~(size_t)1));
  int* sptr = reinterpret_cast<int*>(corr + TS);
  int16_t* colmap = reinterpret_cast<int16_t*>(sptr + Kmax + 2);
  const float g0 = gout ? gout[0] : 1.f;
  const float cf = coef ? coef[b] * g0 : g0;
  const float z = logz[b];
  const bool dead = !(z > WFL_NEG_INF) || !(z < __builtin_inff());  // no accepting path: zero gradient
  const int t_begin = blockIdx.x * TS, nr = min(TS, T - t_begin);
  for (int c = tid; c < C; c += NT) colmap[c] = -1;
  for (int i = tid; i < nr * Kmax; i += NT) acc[i] = 0.f;
  for (int k = tid; k <= K; k += NT) sptr[k] = u.slot_ptr[k];
  if (tid < nr) {
    const int t = t_begin + tid;
    corr[tid] = offs_a[offs_index_a(t, R)] + offs_b[offs_index_b(t + 1, T, R)] - zd;
  }
  __syncthreads();
  for (int k = tid; k < K; k += NT) colmap[u.labels[k]] = (int16_t)k;
  if (!dead && A > 0) {
    const double* alpha_d = reinterpret_cast<const double*>(alpha) + u.ab_base;
    const double* beta_d = reinterpret_cast<const double*>(beta) + u.ab_base;
    const int nch = (A + kStreamChunk - 1) / kStreamChunk;
    for (int i = tid; i < nr * nch; i += NT) {
      const int r = i / nch, j0 = (i - r * nch) * kStreamChunk, j1 = min(A, j0 + kStreamChunk);
      const int t = t_begin + r;
      const double* pa = alpha_d + (int64_t)t * Q;
      const double* pb = beta_d + (int64_t)(t + 1) * Q;
      const float* xrow = xg + u.xg_base + (int64_t)t * Kmax;
      int lo = 0, hi = K - 1;  // the slot of arc j0: the largest k with sptr[k] <= j0
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sptr[mid] <= j0) lo = mid; else hi = mid - 1;
      }
      int k = lo, kend = sptr[k + 1];
      double xv = (double)xrow[k] + corr[r];
      float sum = 0.f;
      for (int j = j0; j < j1; ++j) {
        while (j >= kend) {  // (next non-empty slot)
          if (sum != 0.f) atomicAdd(&acc[r * Kmax + k], sum);
          sum = 0.f;
          ++k;
          kend = sptr[k + 1];
          xv = (double)xrow[k] + corr[r];
        }
        const int2 a = sarc[j];
        const double v = pa[a.x & 0xffff] + pb[(unsigned)a.x >> 16] + (xv + (double)__int_as_float(a.y));
        sum += fast_exp((float)v);  // exp(-inf) = 0
      }
      if (sum != 0.f) atomicAdd(&acc[r * Kmax + k], sum);
    }
  }
  __syncthreads();
  stream_grad_rows(b, t_begin, nr, T, C, Kmax, tid, NT, dx, x, row_lse, accumulate, dead, cf, acc, colmap);
}

// grid (arc blocks + epsilon blocks, B), 256 threads: thread = one arc of utterance b, frames in registers
__global__ void __launch_bounds__(256)
    stream_dw_kernel(wfl_lattice_desc d, const int32_t* __restrict__ ints, const float* __restrict__ floats,
                     const float* __restrict__ xg, int T, int R, const float* __restrict__ weights,
                     const float* __restrict__ alpha, const float* __restrict__ beta, const float* __restrict__ logz,
                     const float* __restrict__ coef_w, const float* __restrict__ gout, float* __restrict__ dW, int nb_arcs,
                     int64_t tail, int nch1) {
  const int b = blockIdx.y;
  const float z = logz[b];
  if (!(z > WFL_NEG_INF) || !(z < __builtin_inff())) return;  // no accepting path: zero gradient
  const UttView u = make_view(d, ints, floats, b, T);
  const int Q = u.Q, Kmax = d.max_labels;
  const AbTail lay(d, tail, nch1);
  const double *offs_a = lay.offs(alpha, b), *offs_b = lay.offs(beta, b);
  const double zd = *lay.z(alpha, b);
  const double* alpha_d = reinterpret_cast<const double*>(alpha) + u.ab_base;
  const double* beta_d = reinterpret_cast<const double*>(beta) + u.ab_base;
  const float cw = (coef_w ? coef_w[b] : 1.f) * (gout ? gout[0] : 1.f);
  float sum = 0.f;
  int wid;
  if ((int)blockIdx.x < nb_arcs) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= u.A) return;
    wid = u.arc_wid[a];
    if (wid < 0) return;
    const double w = (double)(u.arc_w[a] + (weights ? nan_to_neg(weights[wid]) : 0.f));
    const int src = u.arc_src[a], dst = u.arc_dst[a];
    const float* px = xg + u.xg_base + u.arc_slot[a];
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      const double cr = offs_a[offs_index_a(t, R)] + offs_b[offs_index_b(t + 1, T, R)] - zd;
      const double v = alpha_d[(int64_t)t * Q + src] + beta_d[(int64_t)(t + 1) * Q + dst] + ((double)px[(int64_t)t * Kmax] + cr + w);
      sum += fast_exp((float)v);
    }
  } else {
    const int e = (blockIdx.x - nb_arcs) * 256 + threadIdx.x;
    if (e >= u.E) return;
    wid = u.eps_wid[e];
    if (wid < 0) return;
    const double w = (double)(u.eps_w[e] + (weights ? nan_to_neg(weights[wid]) : 0.f));
    const int src = u.eps_src[e], dst = u.eps_dst[e];
#pragma unroll 4
    for (int t = 0; t <= T; ++t) {  // the T + 1 closures
      const double cr = offs_a[offs_index_a(t, R)] + offs_b[offs_index_b(t, T, R)] - zd;
      const float v = (float)(alpha_d[(int64_t)t * Q + src] + beta_d[(int64_t)t * Q + dst] + (cr + w));
      if (v > WFL_NEG_INF) sum += fast_exp(v);
    }
  }
  if (sum != 0.f) atomicAdd(&dW[wid], sum * cw);
}
