// Autograd nodes of the criteria's hot operator paths, in C++ (module gtn_applications_amd._wfl_torch).
//
// The kernels of the CTC step take ~60 us at the reference's benchmark shape; a Python torch.autograd.Function
// around them costs more than that in interpreter time alone (apply() bookkeeping, the engine's call back into
// Python for backward, tensor wrapping of the saved state).  This file is the same operator -- counterpart of
// CTCLossFunction.forward / backward, /root/reference/criterions/ctc.py:31-93 -- as a torch::autograd::Function that
// calls the C ABI of libwfl.so (include/wfl.h) directly.  Host-side plumbing only: no arithmetic happens here.
#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/csrc/autograd/engine.h>
#include <torch/csrc/autograd/functions/accumulate_grad.h>
#include <torch/csrc/autograd/python_variable.h>
#include <torch/extension.h>
#include <pybind11/numpy.h>

#include <cstdlib>
#include <cstring>
#include <functional>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>

#include "../../include/wfl.h"

namespace {
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

void* current_stream(const at::Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check(int rc, const char* what) { TORCH_CHECK(rc == WFL_OK, what, ": ", wfl_last_error()); }

// Loss and gradient of a CTC batch in ONE pipelined launch (wfl_ctc_forward_backward); backward only applies the
// upstream scalar to the gradient computed here (like torch's own CTC the gradient is produced eagerly).
//   staged: the uint8 device buffer of StagedTargets (offsets | flat labels | per-utterance factors), addressed
//   by the byte offsets that follow; ws / nll: the per-stream scratch of ctc_workspace (below); lse: optional row
//   log-sum-exps of x (fused log_softmax, ctc.py:107).
struct CtcStep : public torch::autograd::Function<CtcStep> {
  static at::Tensor forward(AutogradContext* ctx, const at::Tensor& x, const at::Tensor& staged, int64_t off_offsets,
                            int64_t off_flat, int64_t off_scale, int64_t off_coef, int64_t max_len, int64_t blank,
                            const at::Tensor& ws, const at::Tensor& nll, const c10::optional<at::Tensor>& lse,
                            int64_t n_labels, int64_t host_state) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous() && x.dim() == 3,
                "ctc_step: x must be a contiguous float32 [B,T,C] device tensor");
    const auto B = x.size(0), T = x.size(1), C = x.size(2);
    at::Tensor dx = at::empty_like(x);
    at::Tensor loss = at::empty({}, x.options());
    const char* base = static_cast<const char*>(staged.data_ptr());
    const float* lse_p = lse.has_value() && lse->defined() ? lse->data_ptr<float>() : nullptr;
    // (what the step remembers between calls is the caller's: wfl_ctc_call in include/wfl.h)
    const wfl_ctc_call call{n_labels, reinterpret_cast<int32_t*>(host_state)};
    check(wfl_ctc_forward_backward_call(x.data_ptr<float>(), (int)B, (int)T, (int)C,
                                        reinterpret_cast<const int32_t*>(base + off_flat),
                                        reinterpret_cast<const int64_t*>(base + off_offsets), (int)max_len, (int)blank,
                                        ws.data_ptr<float>(), nll.data_ptr<float>(),
                                        reinterpret_cast<const float*>(base + off_coef), nullptr, dx.data_ptr<float>(),
                                        reinterpret_cast<const float*>(base + off_scale), loss.data_ptr<float>(), lse_p,
                                        &call, current_stream(x)),
          "ctc_step");
    ctx->saved_data["x"] = x.detach();
    ctx->saved_data["staged"] = staged;
    ctx->saved_data["ws"] = ws;
    ctx->saved_data["nll"] = nll;
    ctx->saved_data["dx"] = dx;
    if (lse_p) ctx->saved_data["lse"] = *lse;
    ctx->saved_data["ints"] = std::vector<int64_t>{off_offsets, off_flat, off_coef, max_len, blank, n_labels};
    return loss;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    TORCH_CHECK(ctx->saved_data.find("freed") == ctx->saved_data.end(),
                "Trying to backward through the graph a second time (or directly access saved tensors after they have "
                "already been freed). Saved intermediate values of the graph are freed when you call .backward() or "
                "autograd.grad(). Specify retain_graph=True if you need to backward through the graph a second time.");
    at::Tensor x = ctx->saved_data["x"].toTensor();
    if (!grads[0].defined())  // (the loss did not take part in what is being differentiated)
      return {at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(),
              at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    at::Tensor g = grads[0].detach().reshape({1});
    if (!g.is_cuda() || g.scalar_type() != at::kFloat) g = g.to(x.device(), at::kFloat);
    auto it = ctx->saved_data.find("dx");
    at::Tensor dx;
    if (it != ctx->saved_data.end() && it->second.isTensor() && it->second.toTensor().defined()) {
      dx = it->second.toTensor();
      ctx->saved_data.erase(it);  // handed out (and scaled in place) once
      check(wfl_scale(dx.data_ptr<float>(), dx.numel(), g.data_ptr<float>(), current_stream(x)), "ctc_step backward");
    } else {
      // a second backward through a retained graph: the same launch again into a fresh buffer, the upstream scalar
      // applied by the kernel (with the same row log-sum-exps when the log_softmax is fused)
      const auto v = ctx->saved_data["ints"].toIntVector();
      at::Tensor staged = ctx->saved_data["staged"].toTensor(), ws = ctx->saved_data["ws"].toTensor(),
                 nll = ctx->saved_data["nll"].toTensor();
      const char* base = static_cast<const char*>(staged.data_ptr());
      auto l = ctx->saved_data.find("lse");
      const float* lse_p = l != ctx->saved_data.end() ? l->second.toTensor().data_ptr<float>() : nullptr;
      dx = at::empty_like(x);
      const wfl_ctc_call call{v[5], nullptr};  // (a recomputation: not a step whose outcome is to be remembered)
      check(wfl_ctc_forward_backward_call(x.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)x.size(2),
                                          reinterpret_cast<const int32_t*>(base + v[1]),
                                          reinterpret_cast<const int64_t*>(base + v[0]), (int)v[3], (int)v[4],
                                          ws.data_ptr<float>(), nll.data_ptr<float>(),
                                          reinterpret_cast<const float*>(base + v[2]), g.data_ptr<float>(),
                                          dx.data_ptr<float>(), nullptr, nullptr, lse_p, &call, current_stream(x)),
            "ctc_step backward");
    }
    return {dx, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(),
            at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
  }
};

// ------------------------------------------------------------------------------------------------------------
// Targets of a batch, staged and uploaded without passing through Python objects: list-of-int-lists (or 1-D int
// tensors) -> [int64 offsets | int32 labels | six per-utterance factor arrays] in a pinned ring -> one wfl_upload ->
// small content-keyed cache.  The one stager of the package: engine.CtcTargets is a thin wrapper around its handle.
// ------------------------------------------------------------------------------------------------------------
// the per-utterance factor arrays behind the labels, in this order: scale_b (1/len_b for "mean", 1 for "none"), then
// both times +1/B and -1/B (ctc.py:53-58,87, asg.py:116-121,171-179)
enum Factor { kScaleNone, kScaleMean, kCposNone, kCposMean, kCnegNone, kCnegMean, kFactors };
const char* const kFactorNames[kFactors] = {"scale_none", "scale_mean", "cpos_none", "cpos_mean", "cneg_none", "cneg_mean"};

struct StagedTargets {
  at::Tensor dev_buf;  // uint8 on the batch's device (CPU: the unpinned host buffer it was staged in)
  std::string key_bytes;  // [offsets | labels] as staged (confirms a cache hit byte for byte; the host copies)
  int64_t B = 0, n = 0, max_len = 0, off_flat = 0, off_fac = 0;
  long label_min = 0, label_max = -1;
  py::object owner = py::none();  // the Python wrapper (engine.CtcTargets) handed out for this batch while it is in the cache
  hipStream_t up_stream = nullptr;  // the stream the upload was queued on ...
  hipEvent_t up_event = nullptr;    // ... and this batch's OWN event behind it (the staging slot's event is re-recorded
                                    // by later uploads, possibly on another stream)
  int dev_index = 0;  // (an event belongs to the device it was created on)
  StagedTargets() = default;
  StagedTargets(const StagedTargets&) = delete;
  StagedTargets& operator=(const StagedTargets&) = delete;
  ~StagedTargets() {
    if (up_event) free_events(dev_index).push_back(up_event);  // (creating an event costs more than recording one: kept for the next batch)
  }
  static std::vector<hipEvent_t>& free_events(int dev) {
    static auto* pools = new std::unordered_map<int, std::vector<hipEvent_t>>();  // (never destroyed: see g_targets)
    return (*pools)[dev];
  }
  // every hand-out: a use on another stream than the one that uploaded the batch is ordered behind the upload
  void wait_upload() const {
    if (!up_event) return;
    const hipStream_t now = c10::hip::getCurrentHIPStream(dev_index).stream();
    if (now != up_stream) (void)hipStreamWaitEvent(now, up_event, 0);
  }
};

struct PinnedRing {  // reusable pinned staging buffers; a slot is reused after the upload that read it has completed
  static constexpr int kSlots = 8;
  at::Tensor buf[kSlots];
  hipEvent_t ev[kSlots] = {};
  int i = 0;
  uint8_t* next(int64_t need, int& slot) {
    slot = i = (i + 1) % kSlots;
    if (ev[slot]) (void)hipEventSynchronize(ev[slot]);
    if (!buf[slot].defined() || buf[slot].numel() < need) {
      int64_t cap = 1 << 18;
      while (cap < need) cap <<= 1;
      // every slot at once: a pinned allocation costs hundreds of microseconds, and allocating slot by slot would
      // spread eight of them over the first eight steps of a run instead of paying them in the first one
      for (int k = 0; k < kSlots; ++k)
        if (!buf[k].defined() || buf[k].numel() < cap) {
          if (ev[k]) (void)hipEventSynchronize(ev[k]);
          buf[k] = at::empty({cap}, at::TensorOptions().dtype(at::kByte).pinned_memory(true));
        }
    }
    return buf[slot].data_ptr<uint8_t>();
  }
  void unused() { i = (i + kSlots - 1) % kSlots; }  // (the slot next() gave out was not uploaded from)
  void uploaded(int slot, hipStream_t stream) {
    if (!ev[slot]) (void)hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming);
    (void)hipEventRecord(ev[slot], stream);
  }
};

inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t fmix64(uint64_t k) {
  k ^= k >> 33, k *= 0xff51afd7ed558ccdULL, k ^= k >> 33, k *= 0xc4ceb9fe1a85ec53ULL, k ^= k >> 33;
  return k;
}
std::pair<uint64_t, uint64_t> hash128(const uint8_t* p, int64_t n) {  // MurmurHash3 x64_128 mixing steps
  const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
  uint64_t h1 = 0x9e3779b97f4a7c15ULL, h2 = 0xd1b54a32d192ed03ULL;
  const int64_t nb = n / 16;
  for (int64_t i = 0; i < nb; ++i) {
    uint64_t k1, k2;
    memcpy(&k1, p + 16 * i, 8), memcpy(&k2, p + 16 * i + 8, 8);
    k1 *= c1, k1 = rotl64(k1, 31), k1 *= c2, h1 ^= k1, h1 = rotl64(h1, 27), h1 += h2, h1 = h1 * 5 + 0x52dce729;
    k2 *= c2, k2 = rotl64(k2, 33), k2 *= c1, h2 ^= k2, h2 = rotl64(h2, 31), h2 += h1, h2 = h2 * 5 + 0x38495ab5;
  }
  uint64_t t1 = 0, t2 = 0;
  const int64_t rem = n - 16 * nb;
  if (rem > 8) memcpy(&t2, p + 16 * nb + 8, (size_t)(rem - 8));
  if (rem > 0) memcpy(&t1, p + 16 * nb, (size_t)(rem > 8 ? 8 : rem));
  t2 *= c2, t2 = rotl64(t2, 33), t2 *= c1, h2 ^= t2;
  t1 *= c1, t1 = rotl64(t1, 31), t1 *= c2, h1 ^= t1;
  h1 ^= (uint64_t)n, h2 ^= (uint64_t)n, h1 += h2, h2 += h1, h1 = fmix64(h1), h2 = fmix64(h2), h1 += h2, h2 += h1;
  return {h1, h2};
}

// The batch a device saw last, recognised by OBJECT IDENTITY: the reference's benchmarks (ctc_benchmark.py:26-31) hand the
// same list of int lists to every iteration, and flattening + hashing its 5 632 labels is 10 of the ~20 us the forward
// spends on the host -- on a step whose kernels take 45.  Python ints are immutable, so "the same int OBJECTS in the same
// places" means the same labels: one pointer comparison per label against the batch remembered here.  The entry holds a
// reference to every label object (an address it compares against cannot be recycled for another int) and is only
// filled when the content-keyed cache below HITS -- a run whose targets are new every step never pays for it.
struct LastBatch {
  std::vector<PyObject*> elems;  // owned references, row after row
  std::vector<Py_ssize_t> lens;
  std::shared_ptr<StagedTargets> st;
  void clear() {
    for (PyObject* o : elems) Py_DECREF(o);
    elems.clear(), lens.clear(), st.reset();
  }
  // the rows of `t` (lists / tuples only) hold exactly the remembered objects?
  bool matches(PyObject** rows, Py_ssize_t B) const {
    if (!st || (Py_ssize_t)lens.size() != B) return false;
    size_t k = 0;
    for (Py_ssize_t b = 0; b < B; ++b) {
      PyObject* r = rows[b];
      if (!PyList_Check(r) && !PyTuple_Check(r)) return false;
      const Py_ssize_t n = PySequence_Fast_GET_SIZE(r);
      if (n != lens[b]) return false;
      if (n && memcmp(PySequence_Fast_ITEMS(r), elems.data() + k, (size_t)n * sizeof(PyObject*)) != 0) return false;
      k += (size_t)n;
    }
    return true;
  }
  void remember(PyObject** rows, Py_ssize_t B, const std::shared_ptr<StagedTargets>& staged) {
    clear();
    for (Py_ssize_t b = 0; b < B; ++b) {
      PyObject* r = rows[b];
      if (!PyList_Check(r) && !PyTuple_Check(r)) {  // (tensor rows: their storage is mutable, identity proves nothing)
        clear();
        return;
      }
      const Py_ssize_t n = PySequence_Fast_GET_SIZE(r);
      PyObject** it = PySequence_Fast_ITEMS(r);
      lens.push_back(n);
      for (Py_ssize_t i = 0; i < n; ++i) {
        if (!PyLong_CheckExact(it[i])) {  // (an int subclass could answer differently next time)
          clear();
          return;
        }
        Py_INCREF(it[i]);
        elems.push_back(it[i]);
      }
    }
    st = staged;
  }
};

struct TargetCache {  // per device: ring + LRU of the last 64 distinct batches
  PinnedRing ring;
  LastBatch last;
  using Key = std::tuple<uint64_t, uint64_t, int64_t>;
  using Lru = std::list<std::pair<Key, std::shared_ptr<StagedTargets>>>;
  Lru lru;
  std::map<Key, Lru::iterator> index;
  void evict(Lru::iterator it) {
    // the entry lets go of its wrapper (which holds the entry: the cycle ends here) and is no longer recognised
    it->second->owner = py::none();
    if (last.st == it->second) last.clear();
    index.erase(it->first);
    lru.erase(it);
  }
};
// (never destroyed: its entries hold Python objects, which static destructors would release after the interpreter)
std::unordered_map<int, TargetCache>& g_targets = *new std::unordered_map<int, TargetCache>();

// -> staged targets of `dev` (CPU: an unpinned host buffer, nothing uploaded), or nullptr if `targets` is not a list /
// tuple of lists / tuples of ints or 1-D CPU int64 / int32 tensors (the caller normalises the rows and calls again)
std::shared_ptr<StagedTargets> stage_targets(const py::handle& targets, const at::Device& device) {
  TORCH_CHECK(device.is_cuda() || device.is_cpu(), "stage_targets: a CUDA or CPU device, not ", device);
  const at::Device dev = device.is_cuda() && !device.has_index()
                             ? at::Device(at::kCUDA, c10::hip::getCurrentHIPStream().device_index())
                             : device;
  PyObject* t = targets.ptr();
  if (!PyList_Check(t) && !PyTuple_Check(t)) return nullptr;
  const Py_ssize_t B = PySequence_Fast_GET_SIZE(t);
  PyObject** rows = PySequence_Fast_ITEMS(t);
  // rows: lists / tuples of ints (the benchmarks, `[t.tolist() for t in targets]`) or 1-D CPU int tensors (train.py)
  auto tensor_row = [](PyObject* r) -> const at::Tensor* {
    if (!THPVariable_Check(r)) return nullptr;
    const at::Tensor& v = THPVariable_Unpack(r);
    const bool ok = v.dim() == 1 && v.device().is_cpu() && (v.scalar_type() == at::kLong || v.scalar_type() == at::kInt);
    return ok ? &v : nullptr;
  };
  int64_t total = 0, max_len = 0;
  for (Py_ssize_t b = 0; b < B; ++b) {
    int64_t n;
    if (PyList_Check(rows[b]) || PyTuple_Check(rows[b]))
      n = PySequence_Fast_GET_SIZE(rows[b]);
    else if (const at::Tensor* v = tensor_row(rows[b]))
      n = v->numel();
    else
      return nullptr;
    total += n, max_len = std::max<int64_t>(max_len, n);
  }
  TargetCache& tc = g_targets[dev.is_cuda() ? dev.index() : -1];
  auto hand_out = [](const std::shared_ptr<StagedTargets>& e) {
    e->wait_upload();
    return e;
  };
  if (tc.last.matches(rows, B)) return hand_out(tc.last.st);  // the same label objects as last time: nothing to stage
  const bool cuda = dev.is_cuda();
  const int64_t off_flat = 8 * (B + 1), off_fac = (off_flat + 4 * std::max<int64_t>(total, 1) + 7) & ~(int64_t)7;
  const int64_t nbytes = off_fac + 4 * B * kFactors;
  int slot = 0;
  at::Tensor host;  // (CPU: staged where it stays)
  if (!cuda) host = at::empty({nbytes}, at::TensorOptions().dtype(at::kByte));
  uint8_t* base = cuda ? tc.ring.next(nbytes + 16, slot) : host.data_ptr<uint8_t>();
  int64_t* off = reinterpret_cast<int64_t*>(base);
  int32_t* flat = reinterpret_cast<int32_t*>(base + off_flat);
  long lo = 0, hi = -1;
  bool first = true;
  int64_t k = 0;
  auto put = [&](long v) {
    if (v > INT32_MAX || v < INT32_MIN) throw py::value_error("target label does not fit int32");
    if (first || v < lo) lo = v;
    if (first || v > hi) hi = v;
    first = false;
    flat[k++] = (int32_t)v;
  };
  for (Py_ssize_t b = 0; b < B; ++b) {
    off[b] = k;
    if (const at::Tensor* v = tensor_row(rows[b])) {
      const int64_t n = v->numel(), st = n ? v->stride(0) : 1;
      if (v->scalar_type() == at::kLong) {
        const int64_t* p = v->data_ptr<int64_t>();
        for (int64_t i = 0; i < n; ++i) put((long)p[i * st]);
      } else {
        const int32_t* p = v->data_ptr<int32_t>();
        for (int64_t i = 0; i < n; ++i) put((long)p[i * st]);
      }
      continue;
    }
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(rows[b]);
    PyObject** it = PySequence_Fast_ITEMS(rows[b]);
    for (Py_ssize_t i = 0; i < n; ++i) {
      long v;
      PyObject* o = it[i];
#if PY_VERSION_HEX < 0x030C0000
      // (exact ints of one 30-bit digit -- every label there is -- without the call: the long layout of CPython <= 3.11;
      // from 3.12 on the digits live under long_value and Py_SIZE is not defined for ints: PyLong_AsLong below)
      if (PyLong_CheckExact(o) && (Py_SIZE(o) == 1 || Py_SIZE(o) == 0)) {
        v = Py_SIZE(o) ? (long)reinterpret_cast<PyLongObject*>(o)->ob_digit[0] : 0;
        put(v);
        continue;
      }
#endif
      v = PyLong_AsLong(o);
      if (v == -1 && PyErr_Occurred()) {
        const bool overflow = PyErr_ExceptionMatches(PyExc_OverflowError);
        PyErr_Clear();
        if (overflow) throw py::value_error("target label does not fit int32");
        if (cuda) tc.ring.unused();
        return nullptr;  // not ints: the Python side normalises (numpy ints, ranges, ...)
      }
      put(v);
    }
  }
  off[B] = k;
  const int64_t nkey = off_flat + 4 * total;
  const auto h = hash128(base, nkey);
  const TargetCache::Key key{h.first, h.second, nkey};
  auto hit = tc.index.find(key);
  if (hit != tc.index.end() && (int64_t)hit->second->second->key_bytes.size() == nkey &&
      memcmp(hit->second->second->key_bytes.data(), base, (size_t)nkey) == 0) {
    tc.lru.splice(tc.lru.begin(), tc.lru, hit->second);
    if (cuda) tc.ring.unused();  // nothing was uploaded from the slot
    auto& e = hit->second->second;
    tc.last.remember(rows, B, e);  // (seen before, by content: next time its objects are recognised without the staging)
    return hand_out(e);
  }
  memset(base + nkey, 0, (size_t)(off_fac - nkey));  // (the alignment gap: the same batch is the same bytes)
  float* fac = reinterpret_cast<float*>(base + off_fac);
  const float inv_b = 1.0f / (float)(B > 0 ? B : 1);
  for (Py_ssize_t b = 0; b < B; ++b) {
    const float ln = (float)(off[b + 1] - off[b]);
    const float mean = ln > 0.f ? 1.0f / ln : 1.0f;
    fac[kScaleNone * B + b] = 1.0f, fac[kScaleMean * B + b] = mean;
    fac[kCposNone * B + b] = inv_b, fac[kCposMean * B + b] = mean * inv_b;
    fac[kCnegNone * B + b] = -inv_b, fac[kCnegMean * B + b] = mean * -inv_b;
  }
  auto st = std::make_shared<StagedTargets>();
  st->B = B, st->n = total, st->max_len = max_len, st->off_flat = off_flat, st->off_fac = off_fac;
  st->label_min = lo, st->label_max = hi;
  st->key_bytes.assign(reinterpret_cast<const char*>(base), (size_t)nkey);
  st->dev_index = dev.index();
  if (cuda) {
    st->dev_buf = at::empty({nbytes}, at::TensorOptions().dtype(at::kByte).device(dev));
    const hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    check(wfl_upload(st->dev_buf.data_ptr(), base, nbytes, (void*)stream), "stage_targets");
    tc.ring.uploaded(slot, stream);
    st->up_stream = stream;
    auto& pool = StagedTargets::free_events(st->dev_index);
    if (!pool.empty())
      st->up_event = pool.back(), pool.pop_back();
    else if (hipEventCreateWithFlags(&st->up_event, hipEventDisableTiming) != hipSuccess)
      st->up_event = nullptr;
    if (st->up_event) (void)hipEventRecord(st->up_event, stream);
  } else {
    st->dev_buf = host;
  }
  if (hit != tc.index.end()) tc.evict(hit->second);  // (same hash, different bytes: replace)
  tc.lru.emplace_front(key, st);
  tc.index[key] = tc.lru.begin();
  if (tc.lru.size() > 64) tc.evict(std::prev(tc.lru.end()));
  return st;
}

// ------------------------------------------------------------------------------------------------------------
// What the CTC step keeps between calls, per (device, stream, shape): its workspace and its host-state words.
// ------------------------------------------------------------------------------------------------------------
struct WsKey {
  int dev;
  void* stream;
  int64_t B, T, C, L;
  bool operator<(const WsKey& o) const { return std::tie(dev, stream, B, T, C, L) < std::tie(o.dev, o.stream, o.B, o.T, o.C, o.L); }
};
WsKey ws_key(const at::Tensor& x, int64_t max_len) {
  return {x.device().index(), current_stream(x), x.size(0), x.size(1), x.size(2), max_len};
}

// scratch + per-utterance nll of the pipelined step: consecutive steps on a stream are ordered, so they can share it
// (the nll is overwritten by the next step of the same shape on the same stream)
std::map<WsKey, std::pair<at::Tensor, at::Tensor>> g_ws;
const std::pair<at::Tensor, at::Tensor>& ctc_workspace(const at::Tensor& x, int64_t max_len) {
  const WsKey wk = ws_key(x, max_len);
  auto w = g_ws.find(wk);
  if (w == g_ws.end()) {
    int64_t n = 0;
    check(wfl_ctc_workspace((int)wk.B, (int)wk.T, (int)wk.C, (int)max_len, &n), "ctc_workspace");
    if (g_ws.size() >= 16) g_ws.clear();
    const auto f32 = x.options().dtype(at::kFloat);
    w = g_ws.emplace(wk, std::make_pair(at::empty({n}, f32), at::empty({wk.B}, f32))).first;
  }
  return w->second;
}

// The step's memory between calls (wfl_ctc_call::host_state: two pinned int32 per stream and shape, written by the
// repair launch without anybody waiting).  At most kShapes shapes at once (variable-length training sees thousands),
// least recently used first out: its pair goes to the next new shape -- a late write of the evicted shape's launch can
// then only mislead that shape's FIRST choice of launch, never a result.  The pairs are cut from pinned pages that are
// never freed: a launch still in flight may write its words whatever happens to the workspace above.
struct HostStatePool {
  static constexpr size_t kWords = 1024, kShapes = 256;
  std::mutex mu;
  std::list<std::pair<WsKey, int32_t*>> lru;  // most recently used first
  std::map<WsKey, decltype(lru)::iterator> index;
  std::vector<int32_t*> pages;
  size_t used = kWords;
};
HostStatePool& host_state_pool() {
  static auto* p = new HostStatePool();  // (never destroyed: see above)
  return *p;
}
int32_t* ctc_host_state(const WsKey& k) {
  HostStatePool& P = host_state_pool();
  std::lock_guard<std::mutex> lock(P.mu);
  auto it = P.index.find(k);
  if (it != P.index.end()) {
    P.lru.splice(P.lru.begin(), P.lru, it->second);
    return it->second->second;
  }
  // (a stream that is being captured into a graph: no allocation, no memory -- the captured step replays one choice)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)k.stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
  int32_t* w;
  if (P.lru.size() >= HostStatePool::kShapes) {
    w = P.lru.back().second;
    P.index.erase(P.lru.back().first);
    P.lru.pop_back();
  } else {
    if (P.used + 2 > HostStatePool::kWords) {
      void* p = nullptr;
      if (hipHostMalloc(&p, HostStatePool::kWords * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) return nullptr;
      P.pages.push_back(static_cast<int32_t*>(p));
      P.used = 0;
    }
    w = P.pages.back() + P.used;
    P.used += 2;
  }
  w[0] = w[1] = 0;
  P.lru.emplace_front(k, w);
  P.index[k] = P.lru.begin();
  return w;
}
// forget what the steps remembered: the next call of every shape starts with the lane-exponent step (tests that run
// unrelated data through one shape)
void ctc_reset_host_state() {
  HostStatePool& P = host_state_pool();
  std::lock_guard<std::mutex> lock(P.mu);
  for (int32_t* page : P.pages) memset(page, 0, HostStatePool::kWords * sizeof(int32_t));
}

// CTCLoss(log_probs, targets, blank, reduction) for the hot case, from staged targets to the launch in this one
// function.  Returns None when the case is not the hot one (the caller takes the Python path).
py::object ctc_loss_staged(const at::Tensor& x, const std::shared_ptr<StagedTargets>& st, int64_t blank, bool mean,
                           bool fused_lse, int64_t lim_len, int64_t lim_c, int64_t lim_c_long) {
  const auto B = x.size(0), T = x.size(1), C = x.size(2);
  if (!st) return py::none();
  if (!(st->max_len <= lim_len && C <= (st->max_len <= 63 ? lim_c : lim_c_long))) return py::none();
  TORCH_CHECK(st->dev_buf.device() == x.device(), "ctc_loss_staged: targets staged for another device");
  if (st->B != B) throw py::value_error("got " + std::to_string(st->B) + " targets for a batch of " + std::to_string(B));
  if (st->label_min < 0 || st->label_max >= C) {
    const long bad = st->label_min < 0 ? st->label_min : st->label_max;
    throw py::value_error("CTCLoss: target label " + std::to_string(bad) + " is outside [0, " + std::to_string(C) +
                          ") (emissions have " + std::to_string(C) + " classes)");
  }
  if (blank < 0 || blank >= C)
    throw py::value_error("CTCLoss: blank index " + std::to_string(blank) + " is outside [0, " + std::to_string(C) + ")");
  const auto& w = ctc_workspace(x, st->max_len);
  c10::optional<at::Tensor> lse;
  if (fused_lse) {
    lse = at::empty({B, T}, x.options());
    check(wfl_row_lse(x.data_ptr<float>(), B * T, (int)C, lse->data_ptr<float>(), current_stream(x)), "row_lse");
  }
  const int64_t scale = st->off_fac + 4 * B * (mean ? kScaleMean : kScaleNone);
  const int64_t coef = st->off_fac + 4 * B * (mean ? kCnegMean : kCnegNone);
  return py::cast(CtcStep::apply(x, st->dev_buf, 0, st->off_flat, scale, coef, st->max_len, blank, w.first, w.second, lse,
                                 st->n, reinterpret_cast<int64_t>(ctc_host_state(ws_key(x, st->max_len)))));
}

// CTCLoss(log_probs, targets, blank, reduction) for the hot case, everything between the Python call and the launch
// in this one function.  Returns None when the case is not the hot one (the caller takes the Python path).
py::object ctc_loss_lists(const at::Tensor& x, const py::handle& targets, int64_t blank, bool mean, bool fused_lse,
                          int64_t lim_len, int64_t lim_c, int64_t lim_c_long) {
  return ctc_loss_staged(x, stage_targets(targets, x.device()), blank, mean, fused_lse, lim_len, lim_c, lim_c_long);
}

// `loss.backward()` for the loss a CtcStep node returned, without running THIS node on the autograd engine: the gradient
// was computed by the forward launch (for an upstream gradient of one, which is what a bare .backward() on a scalar
// means), so what is left is to hand dx on.
//   * Leaf emissions (ctc_benchmark.py's protocol on device-resident inputs): what AccumulateGrad would do -- dx becomes
//     the leaf's .grad (or is added to it).  No engine at all.
//   * Emissions that are some producer's OUTPUT (a model's, train.py:262-266; `.cuda()` of a host leaf,
//     ctc_benchmark.py:22): the engine is started AT the emissions' edge with dx as its root gradient
//     (x.backward(dx) without needing x): same graph below, same hooks on x and on everything under it -- but no
//     ones_like fill, no trip through this node and no scale launch.
// The engine's version of the first costs two thread hand-overs (device nodes run on the engine's device thread), a
// ones_like fill and the scale launch: 40-60 us of host time per step where the step's kernels take 45.  Returns false --
// the caller then takes the ordinary torch.Tensor.backward -- whenever anything is not exactly the plain case: the loss
// is not a fresh CtcStep output, hooks are registered on the loss or its node (or, for a leaf, on the emissions: the
// engine runs those), the gradient buffer has been handed out already.  Same results, same .grad semantics (first
// gradient: the buffer itself; later ones: added in place), same error on a second backward.
// Only what torch's public headers declare is read here: Node::{pre,post,tensor_pre,retains_grad}_hooks(),
// next_edge(), AccumulateGrad::variable / tensor_post_acc_grad_hooks(), Engine::execute (built_for_torch() below lets
// the Python side refuse this path under another torch than the one these headers came from).
bool ctc_fast_backward(const at::Tensor& loss) {
  auto fn = loss.grad_fn();
  auto* node = dynamic_cast<torch::autograd::CppNode<CtcStep>*>(fn.get());
  if (!node || loss.dim() != 0) return false;
  if (!fn->pre_hooks().empty() || !fn->post_hooks().empty() || !fn->tensor_pre_hooks().empty() ||
      !fn->retains_grad_hooks().empty())
    return false;
  const torch::autograd::Edge edge = fn->next_edge(0);
  if (!edge.function) return false;
  auto* acc = dynamic_cast<torch::autograd::AccumulateGrad*>(edge.function.get());
  at::Tensor x;
  if (acc) {
    if (!acc->pre_hooks().empty() || !acc->post_hooks().empty() || !acc->tensor_pre_hooks().empty() ||
        acc->tensor_post_acc_grad_hooks())
      return false;
    x = acc->variable;
    if (!x.defined() || !x.requires_grad()) return false;
  }
  auto& saved = node->ctx_.saved_data;
  if (saved.find("freed") != saved.end()) return false;  // (the ordinary path raises torch's error)
  auto it = saved.find("dx");
  if (it == saved.end() || !it->second.isTensor() || !it->second.toTensor().defined()) return false;
  at::Tensor dx = it->second.toTensor();
  saved.clear();  // what the engine's release of the graph does
  saved["freed"] = true;
  if (acc) {
    at::NoGradGuard no_grad;
    at::Tensor& grad = x.mutable_grad();
    if (!grad.defined())
      grad = std::move(dx);
    else
      grad.add_(dx);
    return true;
  }
  py::gil_scoped_release no_gil;  // (the engine takes the GIL itself where it runs Python nodes and hooks)
  torch::autograd::Engine::get_default_engine().execute({edge}, {std::move(dx)}, /*keep_graph=*/false,
                                                        /*create_graph=*/false, /*accumulate_grad=*/true, {});
  return true;
}

// the torch these nodes were compiled against (criterions/ctc.py compares it with the running one)
std::string built_for_torch() { return TORCH_VERSION; }


// ------------------------------------------------------------------------------------------------------------
// Every launch of an ASG step's forward in ONE native call: counterpart of ASGLossFunction.forward,
// /root/reference/criterions/asg.py:84-139 (the per-sample graph loop under gtn.parallel_for and the reduction), after
// the targets have been packed (engine.PackedLattice.asg_force_align, cached per batch).  Spelled in Python, one engine
// call after the other, the same sequence took 180-205 us of interpreter time per step, against 450 us of kernels at the
// benchmark shape and ~100 us at a training batch of 8.  Host-side plumbing only.
//   numerator (force-aligned lattice, lattice engine) on `side_stream`, forked from the current stream; its gradient
//   for grad_output = 1 right behind its sweeps; denominator (dense engine) on the current stream; the loss reduction
//   after the numerator's sweeps; `early`: the denominator's gradient (+ the numerator's, as its addend) for
//   grad_output = 1 as well.
//   `phases`: timing events for bench.py (engine.phase_events), a start / end handle per launch group -- lattice_gather,
//   lattice_chain, lattice_grad (the numerator's stream), dense_chain, dense_grad (this one) --, 0: not timed.
// Returns {loss, den_alpha, den_beta, den_logz, den_ws, dx_num, dw_num, dx, dW} (undefined where not asked for).
// ------------------------------------------------------------------------------------------------------------
struct EventRing {  // fork / join events of the native steps, per device (created on first use, never destroyed)
  static constexpr int kN = 32;
  hipEvent_t ev[kN] = {};
  unsigned next = 0;
  std::mutex mu;  // concurrent steps on one device (DataParallel threads, several streams): one event per take
  hipEvent_t take() {
    std::lock_guard<std::mutex> lock(mu);
    hipEvent_t& e = ev[next++ % kN];
    if (!e) TORCH_CHECK(hipEventCreateWithFlags(&e, wfl_order_event_flags()) == hipSuccess, "hipEventCreate");
    return e;
  }
};
EventRing& event_ring(int dev) {
  static std::mutex mu;
  static auto* rings = new std::map<int, EventRing>();
  std::lock_guard<std::mutex> lock(mu);
  return (*rings)[dev];
}
void order_after(hipStream_t waiter, hipStream_t signaller, int dev) {  // waiter's later work after signaller's earlier work
  hipEvent_t e = event_ring(dev).take();
  TORCH_CHECK(hipEventRecord(e, signaller) == hipSuccess && hipStreamWaitEvent(waiter, e, 0) == hipSuccess, "stream ordering");
}
void used_on(const at::Tensor& t, const c10::hip::HIPStream& s) {
  if (t.defined()) c10::hip::HIPCachingAllocator::recordStream(t.storage().data_ptr(), s);
}
float* fptr(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

// The timing events of launch group i of a native step (engine.phase_events): handles ev[2 i] and ev[2 i + 1], recorded
// on the stream the group runs on right before and right after its launches; 0 (or no pair at all): not timed.
struct Phase {
  const std::vector<int64_t>& ev;
  size_t i;
  void mark(size_t k, hipStream_t s) const {
    if (2 * i + k < ev.size() && ev[2 * i + k])
      TORCH_CHECK(hipEventRecord(reinterpret_cast<hipEvent_t>(ev[2 * i + k]), s) == hipSuccess, "hipEventRecord");
  }
  void start(hipStream_t s) const { mark(0, s); }
  void end(hipStream_t s) const { mark(1, s); }
};

c10::hip::HIPStream& fill_stream(int dev) {  // a third stream per device: the step's one fill, off both critical paths
  static std::mutex mu;
  static auto* streams = new std::map<int, c10::hip::HIPStream>();
  std::lock_guard<std::mutex> lock(mu);
  auto it = streams->find(dev);
  if (it == streams->end()) it = streams->emplace(dev, c10::hip::getStreamFromPool(false, (c10::DeviceIndex)dev)).first;
  return it->second;
}

std::vector<at::Tensor> asg_forward(const at::Tensor& x, const at::Tensor& W, int64_t desc_ptr, const at::Tensor& ints,
                                    const at::Tensor& floats, const at::Tensor& scale, const at::Tensor& cpos,
                                    const at::Tensor& cneg, bool need_dx, bool need_dw, bool early, int64_t side_stream,
                                    const std::vector<int64_t>& phases) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous() && x.dim() == 3,
              "asg_forward: x must be a contiguous float32 [B,T,C] device tensor");
  TORCH_CHECK(W.is_cuda() && W.scalar_type() == at::kFloat && W.is_contiguous(), "asg_forward: W must be contiguous float32");
  const int dev = x.device().index();
  const int B = (int)x.size(0), T = (int)x.size(1), C = (int)x.size(2);
  const auto* d = reinterpret_cast<const wfl_lattice_desc*>(desc_ptr);
  const c10::hip::HIPStream main_s = c10::hip::getCurrentHIPStream(dev);
  const c10::hip::HIPStream side_s = c10::hip::getStreamFromExternal(reinterpret_cast<hipStream_t>(side_stream), dev);
  hipStream_t ms = main_s.stream(), ss = side_s.stream();
  const bool need_grad = need_dx || need_dw;
  early = early && need_grad;
  const auto f32 = x.options();
  EventRing& ring = event_ring(dev);
  // What sits on the caller's stream is what the step's time is made of: the denominator's sweeps, its gradient, the
  // reduction of the transition-gradient partials, the loss reduction.  The numerator and the zero fill of its
  // transition gradient run beside it.
  at::Tensor dx_num = need_dx ? at::empty_like(x) : at::Tensor();
  used_on(dx_num, side_s);
  at::Tensor dw_num;
  hipEvent_t filled = nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  TORCH_CHECK(hipStreamIsCapturing(ms, &cap) == hipSuccess, "hipStreamIsCapturing");
  if (need_dw && cap != hipStreamCaptureStatusNone) {
    dw_num = at::zeros_like(W);  // (under capture: on this stream, before the fork -- the fill stream is not in the graph)
    used_on(dw_num, side_s);
  } else if (need_dw) {
    const c10::hip::HIPStream& fs = fill_stream(dev);
    c10::hip::HIPStreamGuard guard(fs);  // (the buffer belongs to that stream: nothing of an earlier step can still be using it)
    dw_num = at::zeros_like(W);
    filled = ring.take();
    TORCH_CHECK(hipEventRecord(filled, fs.stream()) == hipSuccess, "hipEventRecord");
    used_on(dw_num, side_s), used_on(dw_num, main_s);
  }
  const int32_t* ip = ints.data_ptr<int32_t>();
  at::Tensor xg, al, be, lz;
  order_after(ss, ms, dev);
  {
    c10::hip::HIPStreamGuard guard(side_s);  // (the numerator's buffers belong to its stream: freed when this call returns)
    int64_t n_xg = 0, n_ab = 0;
    check(wfl_lattice_workspace(d, T, &n_xg, &n_ab), "asg_forward");
    xg = at::empty({std::max<int64_t>(n_xg, 1)}, f32);
    al = at::empty({std::max<int64_t>(n_ab, 1)}, f32);
    if (need_grad) be = at::empty({std::max<int64_t>(n_ab, 1)}, f32);
    lz = at::empty({B}, f32);
    const Phase gather{phases, 0}, chain{phases, 1}, grad{phases, 2};
    gather.start(ss);
    check(wfl_lattice_gather(d, ip, x.data_ptr<float>(), T, C, xg.data_ptr<float>(), nullptr, ss), "asg_forward");
    gather.end(ss), chain.start(ss);
    check(wfl_lattice_forward(d, ip, floats.data_ptr<float>(), xg.data_ptr<float>(), T, W.data_ptr<float>(), WFL_SEMIRING_LOG,
                              al.data_ptr<float>(), fptr(be), nullptr, lz.data_ptr<float>(), ss),
          "asg_forward");
    chain.end(ss);
    if (filled) TORCH_CHECK(hipStreamWaitEvent(ss, filled, 0) == hipSuccess, "hipStreamWaitEvent");
    if (need_grad) {
      grad.start(ss);
      check(wfl_lattice_grad(d, ip, floats.data_ptr<float>(), xg.data_ptr<float>(), T, C, W.data_ptr<float>(),
                             al.data_ptr<float>(), be.data_ptr<float>(), lz.data_ptr<float>(), cneg.data_ptr<float>(),
                             cneg.data_ptr<float>(), nullptr, 0, nullptr, nullptr, fptr(dx_num), fptr(dw_num), ss),
            "asg_forward");
      grad.end(ss);
    }
  }
  hipEvent_t num_done = ring.take();
  TORCH_CHECK(hipEventRecord(num_done, ss) == hipSuccess, "hipEventRecord");
  int64_t n_part = 0, n_ws = 0;
  check(wfl_dense_workspace(B, T, C, &n_part, &n_ws), "asg_forward");
  at::Tensor da = at::empty({B, T, C}, f32), db = need_grad ? at::empty({B, T, C}, f32) : at::Tensor();
  at::Tensor dz = at::empty({B}, f32), ws = at::empty({n_ws}, f32.dtype(at::kByte));
  at::Tensor loss = at::empty({}, f32);
  at::Tensor dx, dW, part;
  if (early) {
    if (need_dx) dx = at::empty_like(x);
    if (need_dw) dW = at::empty_like(W), part = at::empty({n_part}, f32);
  }
  auto dense_forward = [&](int parts, hipStream_t st) {
    check(wfl_dense_forward_parts(x.data_ptr<float>(), W.data_ptr<float>(), B, T, C, WFL_SEMIRING_LOG, da.data_ptr<float>(),
                                  fptr(db), nullptr, dz.data_ptr<float>(), ws.data_ptr(), parts, st),
          "asg_forward");
  };
  auto dense_grad = [&](int parts, hipStream_t st) {
    check(wfl_dense_grad_parts(x.data_ptr<float>(), W.data_ptr<float>(), B, T, C, da.data_ptr<float>(), db.data_ptr<float>(),
                               dz.data_ptr<float>(), cpos.data_ptr<float>(), cpos.data_ptr<float>(), nullptr, 0, fptr(dx_num),
                               fptr(dw_num), fptr(dx), fptr(dW), fptr(part), ws.data_ptr(), parts, st),
          "asg_forward");
  };
  // One wait on this stream (for the numerator's launches) and nothing else between its kernels: a wait or an event
  // record between two launches keeps the second from being dispatched under the first one's tail -- ~6 us each,
  // measured (scripts/step_timeline.sh) -- so the loss reduction comes last, back to back with the gradient's
  // launches, rather than on the numerator's stream with an event each way.  (The log-domain launches stay here too:
  // beside the gradient kernel, which fills every SIMD's registers, an "empty" launch of 2 B workgroups only gets
  // through as that kernel's workgroups retire: measured 86 us.)
  const Phase chain{phases, 3}, grad{phases, 4};
  chain.start(ms);
  dense_forward(WFL_DENSE_ALL, ms);
  chain.end(ms);
  TORCH_CHECK(hipStreamWaitEvent(ms, num_done, 0) == hipSuccess, "hipStreamWaitEvent");
  used_on(lz, main_s);
  if (early) {
    grad.start(ms);
    dense_grad(WFL_DENSE_ALL, ms);
    grad.end(ms);
  }
  check(wfl_reduce_loss(dz.data_ptr<float>(), lz.data_ptr<float>(), scale.data_ptr<float>(), B, 1.0f, 0, loss.data_ptr<float>(), ms),
        "asg_forward");
  return {loss, da, db, dz, ws, dx_num, dw_num, dx, dW};
}

// ------------------------------------------------------------------------------------------------------------
// The launches of a Transducer step WITHOUT a transition model in one native call: counterpart of
// TransducerLossFunction.forward, /root/reference/criterions/transducer.py:239-315, after the batch of alignment
// acceptors has been packed (wfl_transducer_pack_batch, cached per batch): gather (+ row log-sum-exps when the
// log_softmax of transducer.py:186-187 is fused), the sweeps -- with the emission gradient beside them when asked for and
// possible --, the loss reduction, the join.  (A Transducer WITH a transition model issues its launches from
// criterions/transducer.py.)  `phases`: as asg_forward's, for lattice_gather and lattice_chain.
// Returns ({loss, xg, alpha, beta, logz, row_lse, dx}, in_launch); dx undefined unless in_launch.
// ------------------------------------------------------------------------------------------------------------
std::pair<std::vector<at::Tensor>, bool> lattice_loss_forward(const at::Tensor& x, int64_t desc_ptr, const at::Tensor& ints,
                                                              const at::Tensor& floats, const at::Tensor& scale,
                                                              const at::Tensor& cneg, bool log_softmax, bool want_dx,
                                                              bool need_beta, const std::vector<int64_t>& phases) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous() && x.dim() == 3,
              "lattice_loss_forward: x must be a contiguous float32 [B,T,C] device tensor");
  const int B = (int)x.size(0), T = (int)x.size(1), C = (int)x.size(2);
  const auto* d = reinterpret_cast<const wfl_lattice_desc*>(desc_ptr);
  void* st = current_stream(x);
  const auto f32 = x.options();
  int64_t n_xg = 0, n_ab = 0;
  check(wfl_lattice_workspace(d, T, &n_xg, &n_ab), "lattice_loss_forward");
  at::Tensor xg = at::empty({std::max<int64_t>(n_xg, 1)}, f32), al = at::empty({std::max<int64_t>(n_ab, 1)}, f32);
  at::Tensor be = need_beta ? at::empty({std::max<int64_t>(n_ab, 1)}, f32) : at::Tensor();
  at::Tensor lz = at::empty({B}, f32), loss = at::empty({}, f32);
  at::Tensor lse = log_softmax ? at::empty({B, T}, f32) : at::Tensor();
  at::Tensor dx = (want_dx && need_beta) ? at::empty_like(x) : at::Tensor();
  const int32_t* ip = ints.data_ptr<int32_t>();
  const Phase gather{phases, 0}, chain{phases, 1};
  const hipStream_t hs = reinterpret_cast<hipStream_t>(st);
  gather.start(hs);
  check(wfl_lattice_gather(d, ip, x.data_ptr<float>(), T, C, xg.data_ptr<float>(), fptr(lse), st), "lattice_loss_forward");
  gather.end(hs), chain.start(hs);
  int flag = 0;
  if (dx.defined()) {
    flag = 2;  // (the join comes behind the loss reduction, which then runs under the gradient's tail)
    check(wfl_lattice_forward_grad(d, ip, floats.data_ptr<float>(), xg.data_ptr<float>(), T, C, nullptr, al.data_ptr<float>(),
                                   be.data_ptr<float>(), lz.data_ptr<float>(), cneg.data_ptr<float>(),
                                   log_softmax ? x.data_ptr<float>() : nullptr, fptr(lse), dx.data_ptr<float>(), &flag, st),
          "lattice_loss_forward");
  } else {
    check(wfl_lattice_forward(d, ip, floats.data_ptr<float>(), xg.data_ptr<float>(), T, nullptr, WFL_SEMIRING_LOG,
                              al.data_ptr<float>(), fptr(be), nullptr, lz.data_ptr<float>(), st),
          "lattice_loss_forward");
  }
  chain.end(hs);
  check(wfl_reduce_loss(lz.data_ptr<float>(), nullptr, scale.data_ptr<float>(), B, -1.0f, 0, loss.data_ptr<float>(), st),
        "lattice_loss_forward");
  const bool in_launch = flag != 0 && dx.defined();
  if (in_launch) check(wfl_lattice_side_join(st), "lattice_loss_forward");
  if (!in_launch) dx = at::Tensor();
  return {{loss, xg, al, be, lz, lse, dx}, in_launch};
}

// ------------------------------------------------------------------------------------------------------------
// Landing results on the host.  The kernels behind viterbi(), beam_search() and errors() store
// what the host needs straight into pinned host memory; the host waits on one event and copies it out: no
// hipMemcpyAsync, nothing of size B T crosses the link.  THE INVARIANT: a landing buffer is held under its lock from
// the launch until the result has been copied out of it, and what is returned never aliases it.  land() is the one
// place that keeps it.
// ------------------------------------------------------------------------------------------------------------
struct Landing {
  std::mutex mu;
  at::Tensor pinned;  // uint8, a power of two bytes; laid out by the caller of land()
  hipEvent_t done = nullptr;
};
// Two per device, so that a count does not wait behind another thread's decode:
//   kLandHypotheses: offsets, scores and labels of the greedy decode and of the beam search; kLandCounts: the [B][4] counts
enum LandingKind { kLandHypotheses, kLandCounts };
Landing& landing(int dev, LandingKind kind) {
  static std::mutex mu;
  static auto* all = new std::map<std::pair<int, int>, Landing>();  // (never destroyed: see g_targets)
  std::lock_guard<std::mutex> lock(mu);
  return (*all)[{dev, (int)kind}];
}
struct DeviceScope {  // the input's device current for the launches (viterbi() may be called with another one current)
  int prev = -1;
  explicit DeviceScope(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// launch(base, stream) issues kernels that store `need` bytes at base; read(base) copies them out once they are there.
// Without the GIL; `what` prefixes the error of a launch that failed on the device.
template <class Launch, class Read>
void land(int dev, LandingKind kind, int64_t need, const char* what, const Launch& launch, const Read& read) {
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev).stream();
  Landing& buf = landing(dev, kind);
  py::gil_scoped_release nogil;
  std::lock_guard<std::mutex> lock(buf.mu);
  if (!buf.pinned.defined() || buf.pinned.numel() < need) {
    int64_t cap = kind == kLandCounts ? 1 << 14 : 1 << 16;
    while (cap < need) cap <<= 1;
    buf.pinned = at::empty({cap}, at::TensorOptions().dtype(at::kByte).pinned_memory(true));
  }
  if (!buf.done) TORCH_CHECK(hipEventCreateWithFlags(&buf.done, hipEventDisableTiming) == hipSuccess, "hipEventCreate");
  uint8_t* base = buf.pinned.data_ptr<uint8_t>();
  launch(base, (void*)stream);
  TORCH_CHECK(hipEventRecord(buf.done, stream) == hipSuccess && hipEventSynchronize(buf.done) == hipSuccess, what, ": ",
              hipGetErrorString(hipGetLastError()));
  read(base);
}

// ------------------------------------------------------------------------------------------------------------
// A source of hypotheses: the greedy decode behind viterbi() (wfl_decode_emissions / wfl_decode_paths,
// csrc/decode_kernels.hip: counterpart of the reference's criterions/ctc.py:126-135, asg.py:225-234,
// transducer.py:216-232) or the CTC prefix beam search (wfl_ctc_beam_search, csrc/beam_kernels.hip: the decode the
// reference does not have) or the ASG one (wfl_asg_beam_search).  What an op checks once and then issues, shared by the op that collects the labels on the
// host and the one that counts errors behind the same launch.
// ------------------------------------------------------------------------------------------------------------
struct Hypotheses {
  at::Tensor on;  // the input: its device is the launches'
  int B = 0;
  int64_t rows = 0;     // label sequences the launch writes: B, B nbest of a beam search
  bool scored = false;  // a beam search: a float64 score per row as well (the greedy decode is handed no scores)
  const char* what = "";
  std::function<void(int64_t* capacity, int64_t* ws_bytes)> workspace;  // of this shape
  std::function<void(void* ws, int32_t* out, int64_t capacity, int64_t* offsets, double* scores, void* stream)> launch;
};

// x: the emissions of a decode or a search; their sizes
struct Emissions {
  int B, T, C;
};
Emissions checked_emissions(const at::Tensor& x, const char* what) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous() && x.dim() == 3, what,
              ": x must be a contiguous float32 [B,T,C] device tensor");
  return {(int)x.size(0), (int)x.size(1), (int)x.size(2)};
}

// lengths: int32 [B] on x's device (a padded batch), or none
at::Tensor checked_lengths(const c10::optional<at::Tensor>& lengths, const at::Tensor& x, const char* what) {
  if (!lengths.has_value() || !lengths->defined()) return at::Tensor();
  TORCH_CHECK(lengths->device() == x.device() && lengths->scalar_type() == at::kInt && lengths->is_contiguous() &&
                  lengths->dim() == 1 && lengths->numel() == x.size(0),
              what, ": lengths must be a contiguous int32 [B] tensor on x's device");
  return *lengths;
}

// transitions: float32 [C + 1, C] on x's device (the dense engine's layout), or none
at::Tensor checked_transitions(const c10::optional<at::Tensor>& Wt, const at::Tensor& x, const char* what) {
  if (!Wt.has_value() || !Wt->defined()) return at::Tensor();
  TORCH_CHECK(Wt->device() == x.device() && Wt->scalar_type() == at::kFloat && Wt->is_contiguous() && Wt->dim() == 2 &&
                  Wt->size(0) == x.size(2) + 1 && Wt->size(1) == x.size(2),
              what, ": transitions must be a contiguous float32 [C + 1, C] tensor on x's device");
  return *Wt;
}

// logz: float32 [B] on x's device (wfl_dense_forward's denominator), or none
at::Tensor checked_logz(const c10::optional<at::Tensor>& logz, const at::Tensor& x, const char* what) {
  if (!logz.has_value() || !logz->defined()) return at::Tensor();
  TORCH_CHECK(logz->device() == x.device() && logz->scalar_type() == at::kFloat && logz->is_contiguous() && logz->dim() == 1 &&
                  logz->numel() == x.size(0),
              what, ": logz must be a contiguous float32 [B] tensor on x's device");
  return *logz;
}

// lengths given: wfl_decode_emissions_lengths, frames t >= lengths[b] are not decoded; none: every frame is
Hypotheses emissions_source(const at::Tensor& x, const c10::optional<at::Tensor>& bias, int64_t drop, int64_t num_replabels,
                            int64_t flags, const c10::optional<at::Tensor>& lengths) {
  const Emissions e = checked_emissions(x, "decode_emissions");
  const int B = e.B, T = e.T, C = e.C, R = (int)num_replabels;
  at::Tensor bt;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->device() == x.device() && bias->scalar_type() == at::kFloat && bias->is_contiguous() && bias->numel() == C,
                "decode_emissions: bias must be a contiguous float32 [C] tensor on x's device");
    bt = *bias;
  }
  const at::Tensor lt = checked_lengths(lengths, x, "decode_emissions");
  return {x, B, B, false, "decode",
          [=](int64_t* capacity, int64_t* ws_bytes) { check(wfl_decode_workspace(B, T, R, capacity, ws_bytes), "decode"); },
          [=](void* ws, int32_t* out, int64_t cap, int64_t* offs, double*, void* s) {
            const float* bp = bt.defined() ? bt.data_ptr<float>() : nullptr;
            if (lt.defined())
              check(wfl_decode_emissions_lengths(x.data_ptr<float>(), bp, lt.data_ptr<int32_t>(), B, T, C, (int)drop, R,
                                                 (int)flags, ws, out, cap, offs, s),
                    "decode_emissions_lengths");
            else
              check(wfl_decode_emissions(x.data_ptr<float>(), bp, B, T, C, (int)drop, R, (int)flags, ws, out, cap, offs, s),
                    "decode_emissions");
          }};
}

Hypotheses paths_source(const at::Tensor& paths, int64_t T, int64_t drop, int64_t num_replabels, int64_t flags) {
  TORCH_CHECK(paths.is_cuda() && paths.scalar_type() == at::kInt && paths.dim() == 2 && (paths.size(1) == 0 || paths.stride(1) == 1) &&
                  paths.size(1) >= T,
              "decode_paths: paths must be an int32 [B, >= T] device tensor with unit stride along the frames");
  const int B = (int)paths.size(0), R = (int)num_replabels;
  const int64_t stride = B > 1 ? paths.stride(0) : paths.size(1);
  return {paths, B, B, false, "decode",
          [=](int64_t* capacity, int64_t* ws_bytes) { check(wfl_decode_workspace(B, (int)T, R, capacity, ws_bytes), "decode"); },
          [=](void* ws, int32_t* out, int64_t cap, int64_t* offs, double*, void* s) {
            check(wfl_decode_paths(paths.data_ptr<int32_t>(), stride, B, (int)T, (int)drop, R, (int)flags, ws, out, cap, offs, s),
                  "decode_paths");
          }};
}

// An n-gram LM on the device (wfl_ngram_lm; lm.py's NGramLM.on_device builds one per device): ints = [arc_ptr (S+1) |
// arc_label (A) | arc_next (A) | bo_next (S)] int32, weights = [arc_w (A) | bo_w (S)] float64, both contiguous on one
// GPU, from a pack that passed wfl_ngram_lm_check on the host (step_min, step_max: what that check wrote).
struct DeviceLm {
  at::Tensor ints, weights;  // (kept alive: lm points into them)
  wfl_ngram_lm lm;
  DeviceLm(const at::Tensor& ints_, const at::Tensor& weights_, int64_t S, int64_t A, int64_t start, double step_min,
           double step_max)
      : ints(ints_), weights(weights_) {
    TORCH_CHECK(S >= 1 && A >= 0 && S < (1LL << 31) && A < (1LL << 31) && start >= 0 && start < S,
                "ctc_beam_search_lm: a language model of ", S, " states, ", A, " arcs, start ", start);
    TORCH_CHECK(ints.is_cuda() && ints.scalar_type() == at::kInt && ints.is_contiguous() && ints.dim() == 1 &&
                    ints.numel() == 2 * S + 1 + 2 * A,
                "ctc_beam_search_lm: the LM's int32 arrays must be one contiguous [2 S + 1 + 2 A] tensor on a GPU");
    TORCH_CHECK(weights.device() == ints.device() && weights.scalar_type() == at::kDouble && weights.is_contiguous() &&
                    weights.dim() == 1 && weights.numel() == A + S,
                "ctc_beam_search_lm: the LM's float64 weights must be one contiguous [A + S] tensor on the device of its "
                "int32 arrays");
    const int32_t* ip = ints.data_ptr<int32_t>();
    const double* wp = weights.data_ptr<double>();
    lm.num_states = (int32_t)S, lm.num_arcs = (int32_t)A, lm.start = (int32_t)start, lm.reserved = 0;
    lm.arc_ptr = ip, lm.arc_label = ip + S + 1, lm.arc_next = ip + S + 1 + A, lm.bo_next = ip + S + 1 + 2 * A;
    lm.arc_w = wp, lm.bo_w = wp + A, lm.step_min = step_min, lm.step_max = step_max;
  }
};

// A lexicon on the device (wfl_lexicon; lexicon.py's Lexicon.on_device builds one per device): ints = [arc_ptr (N+1) |
// arc_label (A) | arc_next (A)] int32, contiguous on one GPU, from a pack that passed wfl_lexicon_check on the host.
// A start-marked lexicon (wfl_lexicon_marked; marked_classes = its C > 0) has [node_word (N) |
// start_node (C)] behind them, from a pack that passed wfl_lexicon_marked_check; `marked` then, and its trie is `lex`.
struct DeviceLexicon {
  at::Tensor ints;  // (kept alive: lex and marked point into it)
  wfl_lexicon lex;
  wfl_lexicon_marked marked;
  bool is_marked;
  DeviceLexicon(const at::Tensor& ints_, int64_t N, int64_t A, int64_t V, int64_t marked_classes) : ints(ints_) {
    TORCH_CHECK(N >= 1 && A >= 1 && V >= 1 && N < (1LL << 31) && A < (1LL << 31) && V < (1LL << 31) - 1,
                "ctc_beam_search_lexicon: a lexicon of ", N, " nodes, ", A, " arcs, ", V, " words");
    TORCH_CHECK(marked_classes >= 0 && marked_classes < (1LL << 31), "ctc_beam_search_lexicon: a start-marked lexicon of ",
                marked_classes, " classes");
    is_marked = marked_classes > 0;
    const int64_t extra = is_marked ? N + marked_classes : 0;
    TORCH_CHECK(ints.is_cuda() && ints.scalar_type() == at::kInt && ints.is_contiguous() && ints.dim() == 1 &&
                    ints.numel() == N + 1 + 2 * A + extra,
                "ctc_beam_search_lexicon: the lexicon's int32 arrays must be one contiguous [N + 1 + 2 A] tensor on a GPU"
                " ([N + 1 + 2 A + N + C] for a start-marked one)");
    const int32_t* ip = ints.data_ptr<int32_t>();
    lex.num_nodes = (int32_t)N, lex.num_arcs = (int32_t)A, lex.num_words = (int32_t)V, lex.reserved = 0;
    lex.arc_ptr = ip, lex.arc_label = ip + N + 1, lex.arc_next = ip + N + 1 + A;
    marked.trie = lex;
    marked.node_word = is_marked ? ip + N + 1 + 2 * A : nullptr;
    marked.start_node = is_marked ? ip + N + 1 + 2 * A + N : nullptr;
  }
};

// A lexicon's word-LM look-ahead on the device (wfl_lexicon_lookahead; lexicon.py's
// LexiconLookahead.on_device builds one per device): node_look float64 [N], contiguous on one GPU, from an array that
// wfl_lexicon_lookahead_check (or its start-marked sibling) accepted on the host, and the six ranges that check wrote.
struct DeviceLookahead {
  at::Tensor node_look;  // (kept alive: look points into it)
  wfl_lexicon_lookahead look;
  DeviceLookahead(const at::Tensor& node_look_, double arc_min, double arc_max, double end_min, double end_max, double start_min,
                  double start_max)
      : node_look(node_look_) {
    TORCH_CHECK(node_look.is_cuda() && node_look.scalar_type() == at::kDouble && node_look.is_contiguous() &&
                    node_look.dim() == 1 && node_look.numel() >= 1,
                "beam_search_lookahead: node_look must be one contiguous float64 [num_nodes] tensor on a GPU");
    look.node_look = node_look.data_ptr<double>();
    look.arc_min = arc_min, look.arc_max = arc_max, look.end_min = end_min, look.end_max = end_max;
    look.start_min = start_min, look.start_max = start_max;
  }
  // (what a plan checks where the look-ahead meets its lexicon and word LM)
  void check_for(const std::shared_ptr<DeviceLexicon>& lexicon, const std::shared_ptr<DeviceLm>& lm, const char* what) const {
    TORCH_CHECK(lexicon && lm, what, ": lookahead needs a lexicon and its word LM");
    TORCH_CHECK(node_look.numel() == lexicon->lex.num_nodes, what, ": the look-ahead has ", node_look.numel(),
                " nodes, the lexicon ", lexicon->lex.num_nodes);
    TORCH_CHECK(node_look.device() == lexicon->ints.device(), what, ": the look-ahead must be on the lexicon's device");
  }
};

enum BeamFamily { kBeamCtc, kBeamAsg, kBeamTransducer };
// the names errors carry, [family][kind]: the C entries' (a lexicon's kinds: + 1 start-marked, + 2 with look-ahead)
enum BeamKind { kBeamPlain, kBeamLm, kBeamLexicon, kBeamLexiconMarked, kBeamLexiconLookahead, kBeamLexiconMarkedLookahead, kBeamMerged };
#define WFL_BEAM_NAMES(f) {f, f "_lm", f "_lexicon", f "_lexicon_marked", f "_lexicon_lookahead", f "_lexicon_marked_lookahead", f "_merged"}
const char* const kBeamNames[3][7] = {WFL_BEAM_NAMES("ctc_beam_search"), WFL_BEAM_NAMES("asg_beam_search"),
                                      WFL_BEAM_NAMES("transducer_beam_search")};
// The options of one bound beam search, whichever criterion's it is: what the module's four plan classes (below)
// construct and every beam op takes.  blank: -1 for ASG, which has none; forced: the Transducer's topology; garbage:
// ASG's with a lexicon or a token-level LM (-1: none); replabels: the raw alphabet's, ASG's with a token-level LM.  lm
// none: lm_weight, score_eos and -- without a lexicon -- length_bonus are not read; lexicon: lm is its word LM;
// lookahead none: the lexicon search as it was.
struct BeamOptions {
  BeamFamily family;
  int blank;
  bool forced;
  int beam, K, nbest, garbage;
  std::shared_ptr<DeviceLm> lm;
  std::shared_ptr<DeviceLexicon> lexicon;
  std::shared_ptr<DeviceLookahead> lookahead;
  double lm_weight, word_bonus, length_bonus;
  bool score_eos;
  int replabels;
  BeamOptions(BeamFamily family_, int blank_, bool forced_, int beam_, int K_, int nbest_, int garbage_ = -1,
              const std::shared_ptr<DeviceLm>& lm_ = nullptr, const std::shared_ptr<DeviceLexicon>& lexicon_ = nullptr,
              const std::shared_ptr<DeviceLookahead>& lookahead_ = nullptr, double lm_weight_ = 1.0, double word_bonus_ = 0.0,
              double length_bonus_ = 0.0, bool score_eos_ = true, int replabels_ = 0)
      : family(family_), blank(blank_), forced(forced_), beam(beam_), K(K_), nbest(nbest_), garbage(garbage_), lm(lm_),
        lexicon(lexicon_), lookahead(lookahead_), lm_weight(lm_weight_), word_bonus(word_bonus_), length_bonus(length_bonus_),
        score_eos(score_eos_), replabels(replabels_) {
    const char* what = kBeamNames[family][kBeamLexicon];
    TORCH_CHECK(family != kBeamAsg || !lexicon || !lexicon->is_marked, what, ": a start-marked lexicon is not for ASG");
    TORCH_CHECK(!lm || !lexicon || lm->ints.device() == lexicon->ints.device(), what,
                ": the word LM's arrays must be on the lexicon's device");
    if (lookahead) lookahead->check_for(lexicon, lm, kBeamNames[family][kBeamLexiconLookahead]);
  }
};

// The five plan classes of the module, each the constructor of a BeamOptions by the keywords of its engine.*.on_device
struct BeamPlan : BeamOptions {  // CTC's: an lm, a lexicon and its look-ahead are all optional
  BeamPlan(int blank_, int beam_, int K_, int nbest_, const std::shared_ptr<DeviceLm>& lm_, double lm_weight_,
           double length_bonus_, bool score_eos_, const std::shared_ptr<DeviceLexicon>& lexicon_, double word_bonus_,
           const std::shared_ptr<DeviceLookahead>& lookahead_)
      : BeamOptions(kBeamCtc, blank_, false, beam_, K_, nbest_, -1, lm_, lexicon_, lookahead_, lm_weight_, word_bonus_,
                    length_bonus_, score_eos_) {}
};
struct AsgLexiconPlan : BeamOptions {
  AsgLexiconPlan(int beam_, int K_, int nbest_, int garbage_, const std::shared_ptr<DeviceLexicon>& lexicon_,
                 const std::shared_ptr<DeviceLm>& lm_, double lm_weight_, double word_bonus_, double length_bonus_,
                 bool score_eos_)
      : BeamOptions(kBeamAsg, -1, false, beam_, K_, nbest_, garbage_, lm_, lexicon_, nullptr, lm_weight_, word_bonus_,
                    length_bonus_, score_eos_) {
    TORCH_CHECK(lexicon, "asg_beam_search_lexicon: a lexicon is needed");
  }
};
struct AsgLmPlan : BeamOptions {
  AsgLmPlan(int beam_, int K_, int nbest_, int garbage_, int replabels_, const std::shared_ptr<DeviceLm>& lm_, double lm_weight_,
            double length_bonus_, bool score_eos_)
      : BeamOptions(kBeamAsg, -1, false, beam_, K_, nbest_, garbage_, lm_, nullptr, nullptr, lm_weight_, 0.0, length_bonus_,
                    score_eos_, replabels_) {
    TORCH_CHECK(lm, "asg_beam_search_lm: a language model is needed");
  }
};
struct TransducerLexiconPlan : BeamOptions {
  TransducerLexiconPlan(int blank_, bool forced_, int beam_, int K_, int nbest_, const std::shared_ptr<DeviceLexicon>& lexicon_,
                        const std::shared_ptr<DeviceLm>& lm_, double lm_weight_, double word_bonus_, double length_bonus_,
                        bool score_eos_, const std::shared_ptr<DeviceLookahead>& lookahead_)
      : BeamOptions(kBeamTransducer, blank_, forced_, beam_, K_, nbest_, -1, lm_, lexicon_, lookahead_, lm_weight_, word_bonus_,
                    length_bonus_, score_eos_) {
    TORCH_CHECK(lexicon, "transducer_beam_search_lexicon: a lexicon is needed");
  }
};
struct TransducerLmPlan : BeamOptions {
  TransducerLmPlan(int blank_, bool forced_, int beam_, int K_, int nbest_, const std::shared_ptr<DeviceLm>& lm_, double lm_weight_,
                   double length_bonus_, bool score_eos_)
      : BeamOptions(kBeamTransducer, blank_, forced_, beam_, K_, nbest_, -1, lm_, nullptr, nullptr, lm_weight_, 0.0, length_bonus_,
                    score_eos_) {
    TORCH_CHECK(lm, "transducer_beam_search_lm: a language model is needed");
  }
};

// Every beam search as a source of hypotheses: the options `o` (already checked), rank count and normalisation of this
// call, and what the families take besides -- lengths: CTC's padded batches; Wt: float32 [C + 1, C] on x's device, ASG's
// (needed) and the Transducer's (or none: every weight 0); logz: float32 [B] on x's device (wfl_dense_forward's
// denominator: normalised scores) or none; drop, num_replabels: ASG's mapping of the results on their way out (-1, 0:
// the raw class sequences); spelling: the Transducer search that merges by spelling (wfl_transducer_beam_search_merged,
// DESIGN.md section 23) -- int32 [spell_ptr: C + 1 | spell_sym: num_symbols] on x's device, one contiguous tensor, a
// table that wfl_spelling_check passed on the host (engine.Spelling.on_device) --, or null.  The C entry is chosen
// here and nowhere else: family x {plain, lm, lexicon} x start-marked x look-ahead, or merged.
Hypotheses beam_source(const at::Tensor& x, const c10::optional<at::Tensor>& lengths, const c10::optional<at::Tensor>& Wt,
                       const c10::optional<at::Tensor>& logz, const BeamOptions& o, int nbest, bool normalize, int64_t drop = -1,
                       int64_t num_replabels = 0, const at::Tensor* spelling = nullptr, int64_t num_symbols = 0) {
  const bool ctc = o.family == kBeamCtc, asg = o.family == kBeamAsg, merged = spelling != nullptr;
  // the names errors carry: the search's (the CTC ops have always said ctc_beam_search) and the C entry's
  const char* const* names = kBeamNames[o.family];
  const int kind = merged ? kBeamMerged : o.lexicon ? kBeamLexicon : o.lm ? kBeamLm : kBeamPlain;
  const char* what = names[ctc ? kBeamPlain : kind];
  const char* entry = names[o.lexicon ? kind + (o.lexicon->is_marked ? 1 : 0) + (o.lookahead ? 2 : 0) : kind];
  const Emissions e = checked_emissions(x, what);
  const at::Tensor lt = checked_lengths(lengths, x, what);
  const at::Tensor W = checked_transitions(Wt, x, what), lz = checked_logz(logz, x, what);
  TORCH_CHECK(!asg || W.defined(), what, ": transitions must be a contiguous float32 [C + 1, C] tensor on x's device");
  // (a word LM is on its lexicon's device by the options' check; CTC alone names the LM first, as it always has)
  TORCH_CHECK(!o.lm || (o.lexicon && !ctc) || o.lm->ints.device() == x.device(), names[kBeamLm], ": the LM's arrays must be on x's device");
  TORCH_CHECK(!o.lexicon || o.lexicon->ints.device() == x.device(), names[kBeamLexicon], ": the lexicon's arrays must be on x's device");
  TORCH_CHECK(!merged || (spelling->device() == x.device() && spelling->scalar_type() == at::kInt && spelling->is_contiguous() &&
                          spelling->dim() == 1 && num_symbols >= 0 && spelling->numel() == (int64_t)e.C + 1 + num_symbols),
              what, ": the spelling table must be one contiguous int32 [C + 1 + symbols] tensor on x's device");
  const at::Tensor table = merged ? *spelling : at::Tensor();
  const int B = e.B, T = e.T, C = e.C, R = (int)num_replabels, beam = o.beam, K = o.K;
  return {x, B, (int64_t)B * nbest, true, what,
          [=](int64_t* cap, int64_t* bytes) {
            check(ctc   ? wfl_ctc_beam_workspace(B, T, C, beam, K, nbest, cap, bytes)
                  : asg ? wfl_asg_beam_workspace(B, T, C, beam, K, nbest, R, cap, bytes)
                        : wfl_transducer_beam_workspace(B, T, C, beam, K, nbest, cap, bytes),
                  what);
          },
          [=](void* ws, int32_t* out, int64_t cap, int64_t* offs, double* scores, void* s) {
            const float* xp = x.data_ptr<float>();
            const int norm = normalize ? 1 : 0, eos = o.score_eos ? 1 : 0;
            const wfl_ngram_lm* lm = o.lm ? &o.lm->lm : nullptr;
            // a family's entries: its leading arguments, an entry's own (`mid`), the results
            auto ctc_call = [&](auto fn, auto... mid) {
              return fn(xp, lt.defined() ? lt.data_ptr<int32_t>() : nullptr, B, T, C, o.blank, o.beam, o.K, nbest, norm, mid..., ws, out,
                        cap, offs, scores, s);
            };
            auto asg_call = [&](auto fn, auto... mid) {
              return fn(xp, fptr(W), fptr(lz), B, T, C, o.beam, o.K, nbest, (int)drop, R, mid..., ws, out, cap, offs, scores, s);
            };
            auto transducer_call = [&](auto fn, auto... mid) {
              return fn(xp, fptr(W), fptr(lz), B, T, C, o.blank, o.forced ? 1 : 0, o.beam, o.K, nbest, norm, mid..., ws, out, cap, offs,
                        scores, s);
            };
            // the one choice of start-marked x look-ahead, for the two families that have it
            auto lexicon_call = [&](auto call, auto plain, auto marked, auto look, auto marked_look) {
              const DeviceLexicon& dl = *o.lexicon;
              if (o.lookahead && dl.is_marked)
                return call(marked_look, &dl.marked, &o.lookahead->look, lm, o.lm_weight, o.word_bonus, o.length_bonus, eos);
              if (o.lookahead) return call(look, &dl.lex, &o.lookahead->look, lm, o.lm_weight, o.word_bonus, o.length_bonus, eos);
              if (dl.is_marked) return call(marked, &dl.marked, lm, o.lm_weight, o.word_bonus, o.length_bonus, eos);
              return call(plain, &dl.lex, lm, o.lm_weight, o.word_bonus, o.length_bonus, eos);
            };
            int rc;
            if (merged) {
              const int32_t* sp = table.data_ptr<int32_t>();
              rc = wfl_transducer_beam_search_merged(xp, fptr(W), fptr(lz), sp, sp + C + 1, B, T, C, o.blank, o.forced ? 1 : 0, o.beam,
                                                     o.K, nbest, norm, ws, out, cap, offs, scores, s);
            } else if (ctc) {
              rc = o.lexicon ? lexicon_call(ctc_call, wfl_ctc_beam_search_lexicon, wfl_ctc_beam_search_lexicon_marked,
                                            wfl_ctc_beam_search_lexicon_lookahead, wfl_ctc_beam_search_lexicon_marked_lookahead)
                   : o.lm    ? ctc_call(wfl_ctc_beam_search_lm, lm, o.lm_weight, o.length_bonus, eos)
                             : ctc_call(wfl_ctc_beam_search);
            } else if (asg) {
              rc = o.lexicon ? asg_call(wfl_asg_beam_search_lexicon, o.garbage, &o.lexicon->lex, lm, o.lm_weight, o.word_bonus,
                                        o.length_bonus, eos)
                   : o.lm    ? asg_call(wfl_asg_beam_search_lm, o.garbage, o.replabels, lm, o.lm_weight, o.length_bonus, eos)
                             : asg_call(wfl_asg_beam_search);
            } else {
              rc = o.lexicon ? lexicon_call(transducer_call, wfl_transducer_beam_search_lexicon,
                                            wfl_transducer_beam_search_lexicon_marked, wfl_transducer_beam_search_lexicon_lookahead,
                                            wfl_transducer_beam_search_lexicon_marked_lookahead)
                   : o.lm    ? transducer_call(wfl_transducer_beam_search_lm, lm, o.lm_weight, o.length_bonus, eos)
                             : transducer_call(wfl_transducer_beam_search);
            }
            check(rc, entry);
          }};
}

// The launch of `h` into the device's landing buffer -- [offsets: (rows + 1) int64 | scores: rows float64, a scored
// source | labels: capacity int32], each part padded to 16 bytes -- and from there into fresh CPU tensors: only the
// labels that survived leave the device.
struct Collected {
  at::Tensor labels, offsets, scores;  // [total] int32 or (as_int64) int64; int64 [rows + 1]; float64 [rows] or undefined
};
Collected hypotheses_collect(const Hypotheses& h, bool as_int64) {
  const int dev = h.on.device().index();
  DeviceScope scope(dev);
  int64_t capacity = 0, ws_bytes = 0;
  h.workspace(&capacity, &ws_bytes);
  const int64_t n = h.rows, off_bytes = ((n + 1) * 8 + 15) & ~(int64_t)15, sc_bytes = h.scored ? (n * 8 + 15) & ~(int64_t)15 : 0;
  at::Tensor ws = at::empty({ws_bytes}, h.on.options().dtype(at::kByte));
  Collected r;
  land(
      dev, kLandHypotheses, off_bytes + sc_bytes + capacity * 4, h.what,
      [&](uint8_t* base, void* stream) {
        h.launch(ws.data_ptr(), reinterpret_cast<int32_t*>(base + off_bytes + sc_bytes), capacity, reinterpret_cast<int64_t*>(base),
                 h.scored ? reinterpret_cast<double*>(base + off_bytes) : nullptr, stream);
      },
      [&](const uint8_t* base) {
        const int64_t* offsets = reinterpret_cast<const int64_t*>(base);
        const int32_t* labels = reinterpret_cast<const int32_t*>(base + off_bytes + sc_bytes);
        const int64_t total = offsets[n];
        TORCH_CHECK(offsets[0] == 0 && total >= 0 && total <= capacity, h.what, ": the kernels left inconsistent offsets");
        r.labels = at::empty({total}, at::TensorOptions().dtype(as_int64 ? at::kLong : at::kInt));
        if (as_int64) {
          int64_t* dst = r.labels.data_ptr<int64_t>();
          for (int64_t i = 0; i < total; ++i) dst[i] = labels[i];
        } else if (total) {
          memcpy(r.labels.data_ptr<int32_t>(), labels, (size_t)total * sizeof(int32_t));
        }
        r.offsets = at::empty({n + 1}, at::TensorOptions().dtype(at::kLong));
        memcpy(r.offsets.data_ptr<int64_t>(), offsets, (size_t)(n + 1) * 8);
        if (h.scored) {
          r.scores = at::empty({n}, at::TensorOptions().dtype(at::kDouble));
          memcpy(r.scores.data_ptr<double>(), base + off_bytes, (size_t)n * 8);
        }
      });
  return r;
}

// the B label sequences of a greedy decode as views of one CPU tensor
std::vector<at::Tensor> decode_rows(const Hypotheses& h, bool as_int64) {
  if (h.B == 0) return {};
  const Collected r = hypotheses_collect(h, as_int64);
  const int64_t* offsets = r.offsets.data_ptr<int64_t>();
  std::vector<int64_t> lens((size_t)h.B);
  for (int b = 0; b < h.B; ++b) lens[(size_t)b] = offsets[b + 1] - offsets[b];
  return r.labels.split_with_sizes(lens);
}

std::vector<at::Tensor> decode_emissions(const at::Tensor& x, const c10::optional<at::Tensor>& bias, int64_t drop,
                                         int64_t num_replabels, int64_t flags, bool as_int64,
                                         const c10::optional<at::Tensor>& lengths) {
  return decode_rows(emissions_source(x, bias, drop, num_replabels, flags, lengths), as_int64);
}

std::vector<at::Tensor> decode_paths(const at::Tensor& paths, int64_t T, int64_t drop, int64_t num_replabels, int64_t flags,
                                     bool as_int64) {
  return decode_rows(paths_source(paths, T, drop, num_replabels, flags), as_int64);
}

// ------------------------------------------------------------------------------------------------------------
// Token and word error counts behind the hypotheses (wfl_errors_count, csrc/error_kernels.hip): counterpart of the
// reference's compute_edit_distance (train.py:74-87).  Hypotheses and references stay on the device; the B x 4 counts
// land in the device's second landing buffer.
// ------------------------------------------------------------------------------------------------------------
struct ErrorSide {  // a side's expansion table: int32 [exp_ptr: V + 1 | exp_sym], or undefined (a label is its own symbol)
  at::Tensor table;
  int V = 0, longest = 1;
  const int32_t* ptr() const { return table.defined() ? table.data_ptr<int32_t>() : nullptr; }
  const int32_t* sym() const { return table.defined() ? table.data_ptr<int32_t>() + V + 1 : nullptr; }
};
using ErrorSideSpec = c10::optional<std::tuple<at::Tensor, int64_t, int64_t>>;  // (table, V, longest expansion), or none

// Both tables and the separator of a metrics.ErrorCounter, uploaded (ErrorCounter.tables builds one per device)
struct ErrorTables {
  ErrorSide hyp, ref;
  int sep = -1;
  ErrorTables(const ErrorSideSpec& h, const ErrorSideSpec& r, int64_t sep_)
      : hyp(side(h, "hypothesis")), ref(side(r, "reference")), sep(sep_ < 0 ? -1 : (int)sep_) {}

  static ErrorSide side(const ErrorSideSpec& spec, const char* what) {
    ErrorSide e;
    if (!spec.has_value()) return e;
    const at::Tensor& t = std::get<0>(*spec);
    const int64_t V = std::get<1>(*spec), longest = std::get<2>(*spec);
    TORCH_CHECK(t.defined() && t.scalar_type() == at::kInt && t.is_contiguous() && V >= 1 && V < INT32_MAX && t.numel() > V &&
                    longest >= 0 && longest <= INT32_MAX,
                "errors: the ", what, " table must be a contiguous int32 [V + 1 + symbols] tensor");
    e.table = t, e.V = (int)V, e.longest = (int)longest;
    return e;
  }
  // per call: the launches read the tables on device `dev`
  void check_device(int dev) const {
    for (const ErrorSide* e : {&hyp, &ref})
      TORCH_CHECK(!e->table.defined() || (e->table.is_cuda() && e->table.device().index() == dev),
                  "errors: the ", e == &hyp ? "hypothesis" : "reference", " table must be on the batch's device");
  }
  // ValueError for a staged label a table has no entry for (h: null for hypotheses a decode wrote).  Needs no device:
  // metrics.ErrorCounter calls it on a machine without a GPU, ahead of reporting that.
  void check_labels(const StagedTargets* h, const StagedTargets* r) const {
    if (h && hyp.table.defined() && h->n > 0 && (h->label_min < 0 || h->label_max >= hyp.V))
      throw py::value_error("errors: predicted label " + std::to_string(h->label_min < 0 ? h->label_min : h->label_max) +
                            " is outside the hypothesis table [0, " + std::to_string(hyp.V) + ")");
    if (r && ref.table.defined() && r->n > 0 && (r->label_min < 0 || r->label_max >= ref.V))
      throw py::value_error("errors: target label " + std::to_string(r->label_min < 0 ? r->label_min : r->label_max) +
                            " is outside the reference table [0, " + std::to_string(ref.V) + ")");
  }
};

// the count behind B hypotheses that are on device `dev` already (staged_hyp: where they were staged on the host, or
// null), every check before the launch; -> int64 CPU tensor [B, 4]
at::Tensor errors_collect(int dev, int B, const int32_t* hyp, const int64_t* hyp_off, int64_t hyp_capacity,
                          const StagedTargets* staged_hyp, const std::shared_ptr<StagedTargets>& ref, const ErrorTables& t) {
  TORCH_CHECK(ref && ref->dev_buf.is_cuda() && ref->dev_buf.device().index() == dev,
              "errors: the targets must be staged on the device of the hypotheses");
  if (ref->B != B) throw py::value_error("errors: " + std::to_string(B) + " predictions for " + std::to_string(ref->B) + " targets");
  t.check_labels(staged_hyp, ref.get());
  t.check_device(dev);
  int64_t ws_bytes = 0;
  check(wfl_errors_workspace(B, hyp_capacity, ref->n, t.hyp.longest, t.ref.longest, &ws_bytes), "errors");
  at::Tensor ws = at::empty({ws_bytes}, at::TensorOptions().dtype(at::kByte).device(at::Device(at::kCUDA, (c10::DeviceIndex)dev)));
  ref->wait_upload();
  const char* rbase = static_cast<const char*>(ref->dev_buf.data_ptr());
  at::Tensor counts = at::empty({B, 4}, at::TensorOptions().dtype(at::kLong));
  land(
      dev, kLandCounts, (int64_t)B * 4 * sizeof(int32_t), "errors",
      [&](uint8_t* base, void* stream) {
        check(wfl_errors_count(hyp, hyp_off, reinterpret_cast<const int32_t*>(rbase + ref->off_flat),
                               reinterpret_cast<const int64_t*>(rbase), B, t.hyp.ptr(), t.hyp.sym(), t.hyp.V, t.ref.ptr(),
                               t.ref.sym(), t.ref.V, t.sep, hyp_capacity, ref->n, ws.data_ptr(), reinterpret_cast<int32_t*>(base),
                               stream),
              "errors_count");
      },
      [&](const uint8_t* base) {
        const int32_t* landed = reinterpret_cast<const int32_t*>(base);
        int64_t* dst = counts.data_ptr<int64_t>();
        for (int64_t i = 0; i < (int64_t)B * 4; ++i) dst[i] = landed[i];
      });
  return counts;
}

// hypotheses that are on the host: staged like targets (the one stager), then counted on the device
at::Tensor errors_count(const std::shared_ptr<StagedTargets>& hyp, const std::shared_ptr<StagedTargets>& ref,
                        const ErrorTables& tables) {
  TORCH_CHECK(hyp && hyp->dev_buf.is_cuda(), "errors_count: the predictions must be staged on a GPU");
  const int dev = hyp->dev_buf.device().index();
  if (hyp->B == 0 && ref && ref->B == 0) return at::empty({0, 4}, at::TensorOptions().dtype(at::kLong));
  DeviceScope scope(dev);
  hyp->wait_upload();
  const char* hbase = static_cast<const char*>(hyp->dev_buf.data_ptr());
  return errors_collect(dev, (int)hyp->B, reinterpret_cast<const int32_t*>(hbase + hyp->off_flat),
                        reinterpret_cast<const int64_t*>(hbase), hyp->n, hyp.get(), ref, tables);
}

// a source's launch into device buffers (one hypothesis per utterance), the count behind it: the predictions never
// reach the host
at::Tensor hypotheses_errors(const Hypotheses& h, const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  const int dev = h.on.device().index();
  if (h.B == 0 && ref && ref->B == 0) return at::empty({0, 4}, at::TensorOptions().dtype(at::kLong));
  TORCH_CHECK(h.B > 0 && h.rows == h.B, "errors: an empty batch of emissions for ", ref ? ref->B : 0, " targets");
  DeviceScope scope(dev);
  int64_t capacity = 0, ws_bytes = 0;
  h.workspace(&capacity, &ws_bytes);
  const auto bytes = h.on.options().dtype(at::kByte);
  at::Tensor ws = at::empty({ws_bytes}, bytes);
  at::Tensor out = at::empty({capacity}, bytes.dtype(at::kInt));
  at::Tensor offs = at::empty({h.rows + 1}, bytes.dtype(at::kLong));
  at::Tensor scores = h.scored ? at::empty({h.rows}, bytes.dtype(at::kDouble)) : at::Tensor();
  hipStream_t stream = c10::hip::getCurrentHIPStream(dev).stream();
  h.launch(ws.data_ptr(), out.data_ptr<int32_t>(), capacity, offs.data_ptr<int64_t>(),
           h.scored ? scores.data_ptr<double>() : nullptr, (void*)stream);
  return errors_collect(dev, h.B, out.data_ptr<int32_t>(), offs.data_ptr<int64_t>(), capacity, nullptr, ref, tables);
}

at::Tensor decode_emissions_errors(const at::Tensor& x, const c10::optional<at::Tensor>& bias, int64_t drop, int64_t num_replabels,
                                   int64_t flags, const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables,
                                   const c10::optional<at::Tensor>& lengths) {
  return hypotheses_errors(emissions_source(x, bias, drop, num_replabels, flags, lengths), ref, tables);
}

at::Tensor decode_paths_errors(const at::Tensor& paths, int64_t T, int64_t drop, int64_t num_replabels, int64_t flags,
                               const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  return hypotheses_errors(paths_source(paths, T, drop, num_replabels, flags), ref, tables);
}

// The fourteen beam ops: seven searches, each as the op that collects its hypotheses on the host and the op that counts
// errors behind the same launches.
// -> (labels int64 CPU [total], offsets int64 CPU [B nbest + 1], scores float64 CPU [B, nbest])
py::tuple beam_results(const Hypotheses& h) {
  const Collected r = hypotheses_collect(h, true);
  return py::make_tuple(r.labels, r.offsets, r.scores.view({(int64_t)h.B, -1}));
}
// the first rank, unnormalised (nothing reads the scores), and the counts behind it
at::Tensor beam_errors(const at::Tensor& x, const c10::optional<at::Tensor>& lengths, const c10::optional<at::Tensor>& Wt,
                       const BeamOptions& o, const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables, int64_t drop = -1,
                       int64_t num_replabels = 0, const at::Tensor* spelling = nullptr, int64_t num_symbols = 0) {
  return hypotheses_errors(beam_source(x, lengths, Wt, c10::nullopt, o, 1, false, drop, num_replabels, spelling, num_symbols), ref,
                           tables);
}

py::tuple ctc_beam_search(const at::Tensor& x, const c10::optional<at::Tensor>& lengths, const BeamPlan& plan, bool normalize) {
  return beam_results(beam_source(x, lengths, c10::nullopt, c10::nullopt, plan, plan.nbest, normalize));
}
at::Tensor ctc_beam_search_errors(const at::Tensor& x, const c10::optional<at::Tensor>& lengths, const BeamPlan& plan,
                                  const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  return beam_errors(x, lengths, c10::nullopt, plan, ref, tables);
}

py::tuple asg_beam_search(const at::Tensor& x, const at::Tensor& Wt, const c10::optional<at::Tensor>& logz, int beam, int K,
                          int nbest, int64_t drop, int64_t num_replabels) {
  return beam_results(beam_source(x, c10::nullopt, Wt, logz, {kBeamAsg, -1, false, beam, K, nbest}, nbest, false, drop, num_replabels));
}
at::Tensor asg_beam_search_errors(const at::Tensor& x, const at::Tensor& Wt, int beam, int K, int64_t drop, int64_t num_replabels,
                                  const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  return beam_errors(x, c10::nullopt, Wt, {kBeamAsg, -1, false, beam, K, 1}, ref, tables, drop, num_replabels);
}

py::tuple asg_beam_search_lexicon(const at::Tensor& x, const at::Tensor& Wt, const c10::optional<at::Tensor>& logz,
                                  const AsgLexiconPlan& plan, int64_t drop, int64_t num_replabels) {
  return beam_results(beam_source(x, c10::nullopt, Wt, logz, plan, plan.nbest, false, drop, num_replabels));
}
at::Tensor asg_beam_search_lexicon_errors(const at::Tensor& x, const at::Tensor& Wt, const AsgLexiconPlan& plan, int64_t drop,
                                          int64_t num_replabels, const std::shared_ptr<StagedTargets>& ref,
                                          const ErrorTables& tables) {
  return beam_errors(x, c10::nullopt, Wt, plan, ref, tables, drop, num_replabels);
}

py::tuple asg_beam_search_lm(const at::Tensor& x, const at::Tensor& Wt, const c10::optional<at::Tensor>& logz, const AsgLmPlan& plan,
                             int64_t drop, int64_t num_replabels) {
  return beam_results(beam_source(x, c10::nullopt, Wt, logz, plan, plan.nbest, false, drop, num_replabels));
}
at::Tensor asg_beam_search_lm_errors(const at::Tensor& x, const at::Tensor& Wt, const AsgLmPlan& plan, int64_t drop,
                                     int64_t num_replabels, const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  return beam_errors(x, c10::nullopt, Wt, plan, ref, tables, drop, num_replabels);
}

py::tuple transducer_beam_search(const at::Tensor& x, const c10::optional<at::Tensor>& Wt, const c10::optional<at::Tensor>& logz,
                                 int blank, bool forced, int beam, int K, int nbest, bool normalize) {
  return beam_results(beam_source(x, c10::nullopt, Wt, logz, {kBeamTransducer, blank, forced, beam, K, nbest}, nbest, normalize));
}
at::Tensor transducer_beam_search_errors(const at::Tensor& x, const c10::optional<at::Tensor>& Wt, int blank, bool forced, int beam,
                                         int K, const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  return beam_errors(x, c10::nullopt, Wt, {kBeamTransducer, blank, forced, beam, K, 1}, ref, tables);
}

py::tuple transducer_beam_search_lexicon(const at::Tensor& x, const c10::optional<at::Tensor>& Wt,
                                         const c10::optional<at::Tensor>& logz, const TransducerLexiconPlan& plan, bool normalize) {
  return beam_results(beam_source(x, c10::nullopt, Wt, logz, plan, plan.nbest, normalize));
}
at::Tensor transducer_beam_search_lexicon_errors(const at::Tensor& x, const c10::optional<at::Tensor>& Wt,
                                                 const TransducerLexiconPlan& plan, const std::shared_ptr<StagedTargets>& ref,
                                                 const ErrorTables& tables) {
  return beam_errors(x, c10::nullopt, Wt, plan, ref, tables);
}

py::tuple transducer_beam_search_lm(const at::Tensor& x, const c10::optional<at::Tensor>& Wt, const c10::optional<at::Tensor>& logz,
                                    const TransducerLmPlan& plan, bool normalize) {
  return beam_results(beam_source(x, c10::nullopt, Wt, logz, plan, plan.nbest, normalize));
}
at::Tensor transducer_beam_search_lm_errors(const at::Tensor& x, const c10::optional<at::Tensor>& Wt, const TransducerLmPlan& plan,
                                            const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  return beam_errors(x, c10::nullopt, Wt, plan, ref, tables);
}

py::tuple transducer_beam_search_merged(const at::Tensor& x, const c10::optional<at::Tensor>& Wt,
                                        const c10::optional<at::Tensor>& logz, const at::Tensor& spelling, int64_t num_symbols,
                                        int blank, bool forced, int beam, int K, int nbest, bool normalize) {
  return beam_results(beam_source(x, c10::nullopt, Wt, logz, {kBeamTransducer, blank, forced, beam, K, nbest}, nbest, normalize, -1, 0,
                                  &spelling, num_symbols));
}
at::Tensor transducer_beam_search_merged_errors(const at::Tensor& x, const c10::optional<at::Tensor>& Wt, const at::Tensor& spelling,
                                                int64_t num_symbols, int blank, bool forced, int beam, int K,
                                                const std::shared_ptr<StagedTargets>& ref, const ErrorTables& tables) {
  return beam_errors(x, c10::nullopt, Wt, {kBeamTransducer, blank, forced, beam, K, 1}, ref, tables, -1, 0, &spelling, num_symbols);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  py::class_<DeviceLm, std::shared_ptr<DeviceLm>>(m, "DeviceLm", "an n-gram LM's pack on a GPU (lm.NGramLM.on_device)")
      .def(py::init<const at::Tensor&, const at::Tensor&, int64_t, int64_t, int64_t, double, double>(), py::arg("ints"),
           py::arg("weights"), py::arg("num_states"), py::arg("num_arcs"), py::arg("start"), py::arg("step_min"),
           py::arg("step_max"))
      .def_readonly("ints", &DeviceLm::ints)
      .def_readonly("weights", &DeviceLm::weights);
  py::class_<DeviceLexicon, std::shared_ptr<DeviceLexicon>>(m, "DeviceLexicon",
                                                            "a lexicon's pack on a GPU (lexicon.Lexicon.on_device)")
      .def(py::init<const at::Tensor&, int64_t, int64_t, int64_t, int64_t>(), py::arg("ints"), py::arg("num_nodes"),
           py::arg("num_arcs"), py::arg("num_words"), py::arg("marked_classes") = 0)
      .def_readonly("ints", &DeviceLexicon::ints);
  py::class_<DeviceLookahead, std::shared_ptr<DeviceLookahead>>(
      m, "DeviceLookahead", "a lexicon's word-LM look-ahead on a GPU (lexicon.LexiconLookahead.on_device)")
      .def(py::init<const at::Tensor&, double, double, double, double, double, double>(), py::arg("node_look"),
           py::arg("arc_min"), py::arg("arc_max"), py::arg("end_min"), py::arg("end_max"), py::arg("start_min"),
           py::arg("start_max"))
      .def_readonly("node_look", &DeviceLookahead::node_look);
  py::class_<ErrorTables, std::shared_ptr<ErrorTables>>(m, "ErrorTables",
                                                        "both tables of a metrics.ErrorCounter, uploaded, and its separator")
      .def(py::init<const ErrorSideSpec&, const ErrorSideSpec&, int64_t>(), py::arg("hyp"), py::arg("ref"), py::arg("sep"),
           "hyp, ref: (int32 [exp_ptr: V + 1 | exp_sym] tensor, V, longest expansion) or None: a label is its own symbol")
      .def("check_labels", &ErrorTables::check_labels, py::arg("hyp"), py::arg("ref"),
           "ValueError for a staged label (StagedTargets or None) outside its table; needs no device");
  py::class_<BeamPlan>(m, "BeamPlan", "the options of one CTC beam search, bound (engine.BeamPlan.on_device)")
      .def(py::init<int, int, int, int, const std::shared_ptr<DeviceLm>&, double, double, bool,
                    const std::shared_ptr<DeviceLexicon>&, double, const std::shared_ptr<DeviceLookahead>&>(),
           py::arg("blank"), py::arg("beam"), py::arg("classes_per_frame"), py::arg("nbest"), py::arg("lm"), py::arg("lm_weight"),
           py::arg("length_bonus"), py::arg("score_eos"), py::arg("lexicon"), py::arg("word_bonus"),
           py::arg("lookahead") = std::shared_ptr<DeviceLookahead>(),
           "an n-gram LM (DeviceLm; its weight, a length bonus, whether </s> is scored) or None, a lexicon "
           "(DeviceLexicon; lm is then its word LM; a word bonus) or None, and the lexicon's look-ahead (DeviceLookahead) or None");
  m.def("ctc_beam_search", &ctc_beam_search, py::arg("x"), py::arg("lengths"), py::arg("plan"), py::arg("normalize"),
        "CTC prefix beam search on the device by a BeamPlan: (labels int64 CPU, offsets int64 CPU [B nbest + 1], scores "
        "float64 CPU [B, nbest])");
  m.def("ctc_beam_search_errors", &ctc_beam_search_errors, py::arg("x"), py::arg("lengths"), py::arg("plan"), py::arg("ref"),
        py::arg("tables"),
        "ctc_beam_search's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  m.def("asg_beam_search", &asg_beam_search, py::arg("x"), py::arg("transitions"), py::arg("logz"), py::arg("beam"),
        py::arg("classes_per_frame"), py::arg("nbest"), py::arg("drop"), py::arg("num_replabels"),
        "ASG prefix beam search on the device (engine.AsgBeamPlan's options): (labels int64 CPU, offsets int64 CPU "
        "[B nbest + 1], scores float64 CPU [B, nbest]); logz float32 [B] (normalised scores) or None");
  m.def("asg_beam_search_errors", &asg_beam_search_errors, py::arg("x"), py::arg("transitions"), py::arg("beam"),
        py::arg("classes_per_frame"), py::arg("drop"), py::arg("num_replabels"), py::arg("ref"), py::arg("tables"),
        "asg_beam_search's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  py::class_<AsgLexiconPlan>(m, "AsgLexiconPlan",
                             "the options of one ASG beam search with a lexicon, bound (engine.AsgLexiconBeamPlan.on_device)")
      .def(py::init<int, int, int, int, const std::shared_ptr<DeviceLexicon>&, const std::shared_ptr<DeviceLm>&, double, double,
                    double, bool>(),
           py::arg("beam"), py::arg("classes_per_frame"), py::arg("nbest"), py::arg("garbage"), py::arg("lexicon"), py::arg("lm"),
           py::arg("lm_weight"), py::arg("word_bonus"), py::arg("length_bonus"), py::arg("score_eos"),
           "the garbage class (-1: none), a lexicon over raw class sequences (DeviceLexicon), its word LM (DeviceLm) or None, "
           "and the constants of the CTC lexicon search");
  m.def("asg_beam_search_lexicon", &asg_beam_search_lexicon, py::arg("x"), py::arg("transitions"), py::arg("logz"),
        py::arg("plan"), py::arg("drop"), py::arg("num_replabels"),
        "ASG prefix beam search with a lexicon on the device by an AsgLexiconPlan: (labels int64 CPU, offsets int64 CPU "
        "[B nbest + 1], scores float64 CPU [B, nbest]); logz float32 [B] (normalised scores) or None");
  m.def("asg_beam_search_lexicon_errors", &asg_beam_search_lexicon_errors, py::arg("x"), py::arg("transitions"), py::arg("plan"),
        py::arg("drop"), py::arg("num_replabels"), py::arg("ref"), py::arg("tables"),
        "asg_beam_search_lexicon's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  py::class_<AsgLmPlan>(m, "AsgLmPlan",
                        "the options of one ASG beam search with a token-level LM, bound (engine.AsgLmBeamPlan.on_device)")
      .def(py::init<int, int, int, int, int, const std::shared_ptr<DeviceLm>&, double, double, bool>(), py::arg("beam"),
           py::arg("classes_per_frame"), py::arg("nbest"), py::arg("garbage"), py::arg("replabels"), py::arg("lm"),
           py::arg("lm_weight"), py::arg("length_bonus"), py::arg("score_eos"),
           "the raw alphabet the LM reads through (the garbage class, -1: none; the replabels), an LM over the tokens "
           "(DeviceLm) and the scalars of the CTC search with an LM");
  m.def("asg_beam_search_lm", &asg_beam_search_lm, py::arg("x"), py::arg("transitions"), py::arg("logz"), py::arg("plan"),
        py::arg("drop"), py::arg("num_replabels"),
        "ASG prefix beam search with a token-level LM on the device by an AsgLmPlan: (labels int64 CPU, offsets int64 CPU "
        "[B nbest + 1], scores float64 CPU [B, nbest]); logz float32 [B] (normalised scores) or None");
  m.def("asg_beam_search_lm_errors", &asg_beam_search_lm_errors, py::arg("x"), py::arg("transitions"), py::arg("plan"),
        py::arg("drop"), py::arg("num_replabels"), py::arg("ref"), py::arg("tables"),
        "asg_beam_search_lm's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  m.def("transducer_beam_search", &transducer_beam_search, py::arg("x"), py::arg("transitions"), py::arg("logz"),
        py::arg("blank"), py::arg("forced"), py::arg("beam"), py::arg("classes_per_frame"), py::arg("nbest"), py::arg("normalize"),
        "Transducer prefix beam search on the device (engine.TransducerBeamPlan's options): (labels int64 CPU, offsets int64 "
        "CPU [B nbest + 1], scores float64 CPU [B, nbest]); transitions float32 [C + 1, C] or None, logz float32 [B] or None");
  m.def("transducer_beam_search_errors", &transducer_beam_search_errors, py::arg("x"), py::arg("transitions"), py::arg("blank"),
        py::arg("forced"), py::arg("beam"), py::arg("classes_per_frame"), py::arg("ref"), py::arg("tables"),
        "transducer_beam_search's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  py::class_<TransducerLexiconPlan>(
      m, "TransducerLexiconPlan",
      "the options of one Transducer beam search with a lexicon, bound (engine.TransducerLexiconBeamPlan.on_device)")
      .def(py::init<int, bool, int, int, int, const std::shared_ptr<DeviceLexicon>&, const std::shared_ptr<DeviceLm>&, double,
                    double, double, bool, const std::shared_ptr<DeviceLookahead>&>(),
           py::arg("blank"), py::arg("forced"), py::arg("beam"), py::arg("classes_per_frame"), py::arg("nbest"),
           py::arg("lexicon"), py::arg("lm"), py::arg("lm_weight"), py::arg("word_bonus"), py::arg("length_bonus"),
           py::arg("score_eos"), py::arg("lookahead") = std::shared_ptr<DeviceLookahead>(),
           "the blank and topology, a lexicon over token sequences (DeviceLexicon), its word LM (DeviceLm) or None, the "
           "constants of the CTC lexicon search, and the lexicon's look-ahead (DeviceLookahead) or None");
  m.def("transducer_beam_search_lexicon", &transducer_beam_search_lexicon, py::arg("x"), py::arg("transitions"), py::arg("logz"),
        py::arg("plan"), py::arg("normalize"),
        "Transducer prefix beam search with a lexicon on the device by a TransducerLexiconPlan: (labels int64 CPU, offsets "
        "int64 CPU [B nbest + 1], scores float64 CPU [B, nbest]); transitions float32 [C + 1, C] or None; logz float32 [B] "
        "(with transitions and normalize) or None");
  m.def("transducer_beam_search_lexicon_errors", &transducer_beam_search_lexicon_errors, py::arg("x"), py::arg("transitions"),
        py::arg("plan"), py::arg("ref"), py::arg("tables"),
        "transducer_beam_search_lexicon's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  py::class_<TransducerLmPlan>(
      m, "TransducerLmPlan",
      "the options of one Transducer beam search with a token-level LM, bound (engine.TransducerLmBeamPlan.on_device)")
      .def(py::init<int, bool, int, int, int, const std::shared_ptr<DeviceLm>&, double, double, bool>(), py::arg("blank"),
           py::arg("forced"), py::arg("beam"), py::arg("classes_per_frame"), py::arg("nbest"), py::arg("lm"), py::arg("lm_weight"),
           py::arg("length_bonus"), py::arg("score_eos"),
           "the blank and topology, an LM over the tokens (DeviceLm) and the scalars of the CTC search with an LM");
  m.def("transducer_beam_search_lm", &transducer_beam_search_lm, py::arg("x"), py::arg("transitions"), py::arg("logz"),
        py::arg("plan"), py::arg("normalize"),
        "Transducer prefix beam search with a token-level LM on the device by a TransducerLmPlan: (labels int64 CPU, offsets "
        "int64 CPU [B nbest + 1], scores float64 CPU [B, nbest]); transitions float32 [C + 1, C] or None; logz float32 [B] "
        "(with transitions and normalize) or None");
  m.def("transducer_beam_search_lm_errors", &transducer_beam_search_lm_errors, py::arg("x"), py::arg("transitions"),
        py::arg("plan"), py::arg("ref"), py::arg("tables"),
        "transducer_beam_search_lm's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  m.def("transducer_beam_search_merged", &transducer_beam_search_merged, py::arg("x"), py::arg("transitions"), py::arg("logz"),
        py::arg("spelling"), py::arg("num_symbols"), py::arg("blank"), py::arg("forced"), py::arg("beam"),
        py::arg("classes_per_frame"), py::arg("nbest"), py::arg("normalize"),
        "transducer_beam_search with hypotheses merged by spelling (DESIGN.md section 23); spelling: int32 [spell_ptr: C + 1 | "
        "spell_sym: num_symbols] on x's device (engine.Spelling.on_device)");
  m.def("transducer_beam_search_merged_errors", &transducer_beam_search_merged_errors, py::arg("x"), py::arg("transitions"),
        py::arg("spelling"), py::arg("num_symbols"), py::arg("blank"), py::arg("forced"), py::arg("beam"),
        py::arg("classes_per_frame"), py::arg("ref"), py::arg("tables"),
        "transducer_beam_search_merged's best hypotheses into device memory and the error counts behind them: int64 CPU [B, 4]");
  m.def("decode_emissions", &decode_emissions, py::arg("x"), py::arg("bias"), py::arg("drop"), py::arg("num_replabels"),
        py::arg("flags"), py::arg("as_int64"), py::arg("lengths"),
        "viterbi()'s decode from emissions (argmax, collapse, drop, unpack) on the device: B CPU tensors; lengths int32 [B] "
        "on x's device (a padded batch: frames t >= lengths[b] are not decoded) or None");
  m.def("decode_paths", &decode_paths, py::arg("paths"), py::arg("T"), py::arg("drop"), py::arg("num_replabels"),
        py::arg("flags"), py::arg("as_int64"), "viterbi()'s decode from [B, >= T] int32 device label paths: B CPU tensors");
  m.def("errors_count", &errors_count,
        "token and word error counts (train.py:74-87) of staged predictions against staged targets: int64 CPU [B, 4]");
  m.def("decode_emissions_errors", &decode_emissions_errors, py::arg("x"), py::arg("bias"), py::arg("drop"),
        py::arg("num_replabels"), py::arg("flags"), py::arg("ref"), py::arg("tables"), py::arg("lengths"),
        "decode_emissions' launch into device memory and the error counts behind it: int64 CPU [B, 4]");
  m.def("decode_paths_errors", &decode_paths_errors,
        "decode_paths' launch into device memory and the error counts behind it: int64 CPU [B, 4]");
  m.def("ctc_fast_backward", &ctc_fast_backward,
        "loss.backward() of a CtcStep loss without the autograd engine (false: not the plain case, use the engine)");
  m.def(
      "order_after",
      [](int64_t waiter, int64_t signaller, int dev) {
        order_after(reinterpret_cast<hipStream_t>(waiter), reinterpret_cast<hipStream_t>(signaller), dev);
      },
      "waiter's later work after signaller's earlier work (raw stream handles): a pooled device-scope event");
  m.def("built_for_torch", &built_for_torch, "torch version whose headers this module was compiled against");
  m.def("asg_forward", &asg_forward, "every launch of an ASG step's forward in one native call (criterions/asg.py)");
  m.def("lattice_loss_forward", &lattice_loss_forward,
        "gather, sweeps (+ the gradient beside them), loss reduction and join of a Transducer step without transitions");
  py::tuple factors((size_t)kFactors);
  for (int f = 0; f < kFactors; ++f) factors[f] = kFactorNames[f];
  m.attr("FACTORS") = factors;
  py::class_<StagedTargets, std::shared_ptr<StagedTargets>>(m, "StagedTargets")
      .def_readonly("B", &StagedTargets::B)
      .def_readonly("n", &StagedTargets::n)
      .def_readonly("max_len", &StagedTargets::max_len)
      .def_readonly("label_min", &StagedTargets::label_min)
      .def_readonly("label_max", &StagedTargets::label_max)
      .def_readonly("off_flat", &StagedTargets::off_flat)
      .def_readonly("off_fac", &StagedTargets::off_fac)
      .def_readonly("dev_buf", &StagedTargets::dev_buf)
      .def_property_readonly("offsets",
                             [](const StagedTargets& s) {
                               return py::array_t<int64_t>(s.B + 1, reinterpret_cast<const int64_t*>(s.key_bytes.data()));
                             })
      .def_property_readonly("flat",
                             [](const StagedTargets& s) {
                               return py::array_t<int32_t>(s.n, reinterpret_cast<const int32_t*>(s.key_bytes.data() + s.off_flat));
                             })
      .def_readwrite("owner", &StagedTargets::owner, "the Python wrapper handed out for this batch (engine.CtcTargets)")
      .def("wait_upload", &StagedTargets::wait_upload, "order the current stream behind this batch's upload");
  m.def("stage_targets", &stage_targets,
        "stage + upload a batch's targets through the content-keyed cache (None if the rows are not lists / tuples of "
        "ints or 1-D CPU int64 / int32 tensors)");
  m.def("ctc_loss_staged", &ctc_loss_staged, "the CTC step for staged targets (None: not the hot case)");
  m.def("ctc_loss_lists", &ctc_loss_lists,
        "CTCLoss for list-of-int-list targets: staging, upload, checks and the pipelined launch in one native call");
  m.def("ctc_workspace", &ctc_workspace, "(scratch, nll) of the CTC step per (device, current stream, shape)");
  m.def(
      "ctc_host_state", [](const at::Tensor& x, int64_t max_len) { return reinterpret_cast<int64_t>(ctc_host_state(ws_key(x, max_len))); },
      "address of the CTC step's two pinned host-state words per (device, current stream, shape); 0 while capturing");
  m.def("ctc_reset_host_state", &ctc_reset_host_state, "zero the steps' memory of which launch to start with");
}
