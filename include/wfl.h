/*
 * wfl.h -- C ABI of libwfl.so, the MI355X-native differentiable-WFST loss engine.
 *
 * This is the drop-in boundary for the hot path of facebookresearch/gtn_applications:
 * the criterion layer (criterions/{ctc,asg,stc,transducer}.py) reaches its arithmetic through the
 * pybind11 bindings of the external `gtn` C++ library.  Every entry point below names the gtn call
 * sites (file:line under /root/reference) whose work it replaces.  There is no reference header to
 * mirror (gtn is not vendored), so the ABI is designed for the path:
 *
 *   - plain C symbols, plain pointers and sizes, no C++/torch types, no exceptions;
 *   - every function returns an int status (WFL_OK == 0); wfl_last_error() gives a thread-local
 *     message for the last failure on the calling thread;
 *   - device entry points take caller-owned DEVICE buffers and a hipStream_t (passed as void*),
 *     enqueue work asynchronously and never synchronise, allocate or free device memory;
 *   - host graph entry points (wfl_graph_*) work on opaque handles and never touch the GPU;
 *   - no hidden global state: re-entrant from several host threads (autograd worker threads).  What a step remembers
 *     between calls (the CTC step's choice of launch) lives in memory the caller hands in (wfl_ctc_call); the gradient
 *     beside the lattice sweeps keeps per-device COUNTERS of whether kernels of two streams overlap on this stack
 *     (wfl_lattice_diagnostics) -- they pick between two launch plans with identical results.
 *
 * Emissions are always float32 [B, T, C] row-major ("the emissions graph": gtn.linear_graph +
 * set_weights, ctc.py:40-44, asg.py:96-100, stc.py:74-78, transducer.py:262-264 -- here the
 * tensor IS the graph, nothing is materialised).
 */
#ifndef WFL_H_
#define WFL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFL_OK 0
#define WFL_ERR_INVALID 1     /* bad argument (shape, null pointer, label out of range ...) */
#define WFL_ERR_UNSUPPORTED 2 /* valid request this build cannot serve (e.g. more than 65535 states) */
#define WFL_ERR_RUNTIME 3     /* HIP runtime error (message has the hipError string) */

#define WFL_EPSILON (-1) /* gtn.epsilon; pinned by tests/trans_backoff_test.txt:3 */

#define WFL_SEMIRING_LOG 0      /* forward_score  */
#define WFL_SEMIRING_TROPICAL 1 /* viterbi_score / viterbi_path */

const char* wfl_last_error(void);
int wfl_version(void);
/* hipEventCreateWithFlags flags of the library's stream-ordering events (fork / join of its side streams), as chosen
 * by WFL_ORDER_EVENTS (csrc/device_common.h): for callers that order their own streams the same way. */
unsigned wfl_order_event_flags(void);

/* ------------------------------------------------------------------------------------------------
 * Host WFST library (replaces gtn.Graph and the graph functions the criteria call)
 * ------------------------------------------------------------------------------------------------ */
typedef struct wfl_graph wfl_graph; /* opaque */

/* gtn.Graph(calc_grad) -- ctc.py:16, asg.py:57,73, stc.py:34, transducer.py:16,24,33,65,87,352 */
wfl_graph* wfl_graph_new(void);
void wfl_graph_free(wfl_graph* g);
wfl_graph* wfl_graph_clone(const wfl_graph* g);
/* Graph.add_node(start, accept) -> node id */
int wfl_graph_add_node(wfl_graph* g, int start, int accept);
/* Graph.add_arc(src, dst, ilabel, olabel, weight) -> arc id (insertion order), <0 on error */
int wfl_graph_add_arc(wfl_graph* g, int src, int dst, int ilabel, int olabel, float weight);
/* bulk forms of the two calls above (same ordering semantics) */
int wfl_graph_add_nodes(wfl_graph* g, int n, const uint8_t* start, const uint8_t* accept);
int wfl_graph_add_arcs(wfl_graph* g, int64_t n, const int32_t* src, const int32_t* dst,
                       const int32_t* ilabel, const int32_t* olabel, const float* weight);
int wfl_graph_num_nodes(const wfl_graph* g);
int64_t wfl_graph_num_arcs(const wfl_graph* g);
/* copy out: any pointer may be NULL.  start/accept: [num_nodes] bytes; arcs: [num_arcs] each */
int wfl_graph_get(const wfl_graph* g, uint8_t* start, uint8_t* accept, int32_t* src, int32_t* dst,
                  int32_t* ilabel, int32_t* olabel, float* weight);
/* Graph.set_weights(ptr): num_arcs float32 in arc-id order (ctc.py:44, asg.py:66, transducer.py:256) */
int wfl_graph_set_weights(wfl_graph* g, const float* w);
/* Graph.arc_sort(olabel): orders each node's in/out arc lists by label; arc ids are unchanged */
int wfl_graph_arc_sort(wfl_graph* g, int olabel);
/* gtn.compose / gtn.intersect (ctc.py:50, asg.py:112-114, stc.py:86, transducer.py:216-287):
 * first.olabel is matched with second.ilabel, epsilons advance alone, weights add, result trimmed.
 * If prov_first / prov_second are non-NULL they receive malloc'ed arrays [num_arcs(result)] with
 * the arc id each result arc came from (or -1); release them with wfl_free(). */
wfl_graph* wfl_graph_compose(const wfl_graph* first, const wfl_graph* second, int32_t** prov_first,
                             int32_t** prov_second);
/* gtn.remove(g, label) (transducer.py:221,229,269,274); prov as above (arc id in g) */
wfl_graph* wfl_graph_remove(const wfl_graph* g, int ilabel, int olabel, int32_t** prov);
/* gtn.project_input / project_output (transducer.py:229,269,273) */
wfl_graph* wfl_graph_project(const wfl_graph* g, int output);
/* gtn.viterbi_path on a host graph (transducer.py:228: tiny path (x) token-graph compositions).
 * Ties: maximum weight, then fewest non-epsilon output labels ("we take the shortest",
 * transducer.py:226-227), then first found.  Result is a chain graph. */
wfl_graph* wfl_graph_viterbi_path(const wfl_graph* g);
/* project_input(remove(compose(tokens, tokens_target))) (transducer.py:273-276) without the composition, for
 * tokens = make_token_graph(N, blank="optional", allow_repeats=False) (transducer.py:78-123) and a
 * single-start acceptor over the tokens: isomorphic to what the three calls give.  NULL (and no
 * error) if `tokens` does not have that shape -- use the three calls. */
wfl_graph* wfl_graph_token_alignments(const wfl_graph* tokens, const wfl_graph* tokens_target);
/* gtn.equal / gtn.isomorphic (tests/transducer_test.py:47-55,376-418) */
int wfl_graph_equal(const wfl_graph* a, const wfl_graph* b);
int wfl_graph_isomorphic(const wfl_graph* a, const wfl_graph* b);
/* gtn.loadtxt / savetxt text format (utils.py:261, build_transitions.py:221; format pinned by
 * tests/trans_backoff_test.txt) */
wfl_graph* wfl_graph_loadtxt(const char* path);
int wfl_graph_savetxt(const wfl_graph* g, const char* path);
/* gtn.load / gtn.save (utils.py:261 reads config["transitions"] with gtn.load; scripts/build_transitions.py:221
 * writes it with gtn.save).  load sniffs the file: gtn text (as above) or gtn's binary layout -- int32 counts
 * {nodes, start, accept, arcs}, start ids, accept ids, then {src, dst, ilabel, olabel, float weight} per arc --
 * restated from gtn's published utils.cpp and UNPINNED (gtn is not vendored): the reader cross-checks the counts
 * against the file size and id ranges (both plausible count orders) and fails loudly on anything else. */
wfl_graph* wfl_graph_load(const char* path);
int wfl_graph_save(const wfl_graph* g, const char* path);
void wfl_free(void* p);

/* ------------------------------------------------------------------------------------------------
 * Packed lattice batch: B acceptors A_b ready for the device kernels.
 *
 * Per utterance b (all indices local to b): Q_b states renumbered by epsilon level, A_b labelled
 * arcs sorted by destination, E_b epsilon arcs sorted by destination.  One int32 blob and one
 * float blob hold everything; `wfl_lattice_desc` says where each array starts (element offsets).
 * wfl_lattice_pack*() build the blobs on the host; the caller uploads them (one H2D each) and
 * passes device pointers + the descriptor (by value, host memory) to the kernels.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t B, max_states, max_arcs, max_eps, max_labels, max_levels;
  int64_t total_states, total_arcs, total_eps, total_labels;
  int32_t shared; /* 1: one graph shared by every utterance (transition graphs) */
  /* element offsets into the int32 blob */
  int64_t state_off; /* [B+1] first state of b in the per-state arrays                         */
  int64_t arc_off;   /* [B+1] first labelled arc of b                                         */
  int64_t eps_off;   /* [B+1] first epsilon arc of b                                          */
  int64_t lab_off;   /* [B+1] first entry of b in `labels`                                    */
  int64_t lvl_off;   /* [B+1] first entry of b in `lvl_ptr` (n_levels_b + 1 entries each)      */
  int64_t in_ptr;    /* [total_states + B] CSR by destination over labelled arcs (local ids)   */
  int64_t out_ptr;   /* [total_states + B] CSR by source                                      */
  int64_t out_arc;   /* [total_arcs] labelled-arc ids in by-source order                      */
  int64_t ein_ptr;   /* [total_states + B] CSR by destination over epsilon arcs               */
  int64_t eout_ptr;  /* [total_states + B]                                                    */
  int64_t eout_arc;  /* [total_eps]                                                           */
  int64_t arc_src, arc_dst, arc_slot, arc_lab, arc_wid; /* [total_arcs] each                   */
  int64_t eps_src, eps_dst, eps_wid;                    /* [total_eps] each                    */
  int64_t labels;    /* [total_labels] distinct emission columns used by b (slot -> column)    */
  int64_t lvl_ptr;   /* level boundaries (state ranges) for the epsilon closure                */
  int64_t arc_orig;  /* [total_arcs] caller's arc id of each labelled arc (for Viterbi paths)  */
  int64_t eps_orig;  /* [total_eps]                                                           */
  int64_t slot_ptr;  /* [total_labels + B] CSR by emission slot over labelled arcs (gradient rows) */
  int64_t slot_arc;  /* [total_arcs] labelled-arc ids in by-slot order                         */
  int64_t int_words; /* size of the int32 blob                                                 */
  /* element offsets into the float blob */
  int64_t arc_w;     /* [total_arcs] constant weight (NaN is stored as -inf)    */
  int64_t eps_w;     /* [total_eps]                                                           */
  int64_t start_w;   /* [total_states] 0 for start states else -inf                           */
  int64_t accept_w;  /* [total_states] 0 for accept states else -inf                          */
  int64_t float_words;
} wfl_lattice_desc;

typedef struct wfl_lattice_host wfl_lattice_host; /* opaque: descriptor + host blobs */

/* Generic packer: one graph per utterance (or a single shared graph, shared=1, n_graphs=1).
 * graphs[b] must be an acceptor over emission columns: arc ilabel in [0,C) or WFL_EPSILON.
 * wid[b] (may be NULL) gives, per arc of graphs[b], the index of the learnable weight it adds
 * (-1: none).  Replaces what gtn.intersect(emissions, A_b) needs to know about A_b. */
wfl_lattice_host* wfl_lattice_pack(const wfl_graph* const* graphs, const int32_t* const* wid,
                                   int n_graphs, int B, int shared, int C);
/* Hint that a batch is about to be packed: wakes the host pool's sleeping workers so that the job
 * submitted a few tens of microseconds later finds them polling (no-op when the pool does not
 * spin, WFL_HOST_SPIN_US=0). */
void wfl_host_pool_wake(void);

/* TransducerLossFunction.forward's per-sample host work for a whole batch (transducer.py:262-281 under
 * gtn.parallel_for, :296): for every target b (flat int32 graphemes + offsets[B+1])
 *     tokens_target = remove(project_output(compose(chain(target_b), lexicon)))
 *     alignments_b  = project_input(remove(compose(tokens, tokens_target)))
 *     [alignments_b = compose(transitions, alignments_b); wid = arc of `transitions` behind each arc]
 * on a persistent pool of host threads (nthreads: 1 = serial in the caller, otherwise the pool: one thread per
 * host core up to 64), packed like wfl_lattice_pack.  With `transitions` the arcs' constant weights are 0 (the
 * learnable weights are added on the device through wid), as the reference overwrites them (transducer.py:255). */
wfl_lattice_host* wfl_transducer_pack_batch(const wfl_graph* tokens, const wfl_graph* lexicon,
                                            const wfl_graph* transitions, const int32_t* targets,
                                            const int64_t* offsets, int B, int C, int nthreads);
/* The same, with the blobs written to the CALLER's buffer (typically pinned staging memory that is then uploaded:
 * saves the copy out of the handle) if they fit: `dst` (16-byte aligned, dst_bytes) receives
 * [float blob | reserve_floats floats left for the caller | pad to 16 bytes | int32 blob].
 * wfl_lattice_host_external(h) then returns the byte offset of the int blob in dst (and the handle holds only the
 * descriptor); -1 means the blobs did not fit (or dst was NULL) and are in the handle as usual. */
wfl_lattice_host* wfl_transducer_pack_batch_into(const wfl_graph* tokens, const wfl_graph* lexicon,
                                                 const wfl_graph* transitions, const int32_t* targets,
                                                 const int64_t* offsets, int B, int C, int nthreads, void* dst,
                                                 int64_t dst_bytes, int64_t reserve_floats);
int64_t wfl_lattice_host_external(const wfl_lattice_host* h);
/* Transducer.viterbi's decode stage for a whole batch -- transducer.py:221-232, the part of process(b) behind the best
 * frame path, run under gtn.parallel_for (transducer.py:232) and called in every training step (train.py:278-279):
 *     out_b = labels_to_list(remove(project_output(viterbi_path(compose(chain(labels_b), tokens)))))
 * labels: the frame-level label paths, flat, utterance b = labels[offsets[b] .. offsets[b+1]) (back-off epsilons already
 * removed).  out (caller's buffer, out_capacity int32; offsets[B] - offsets[0] always suffices for make_token_graph
 * graphs) receives the token sequences back to back, out_offsets[B+1] their boundaries; an utterance without an
 * accepting path decodes to nothing.  Ties (allow_repeats) go to the path with the fewest output labels, as
 * wfl_graph_viterbi_path breaks them.  The graphs make_token_graph builds (transducer.py:78-123) are recognised arc
 * for arc and decoded directly -- collapse repeated labels, drop blanks, within what the graph accepts --; any other
 * `tokens` goes through the graph algebra per utterance on the host pool (nthreads: 1 = serial in the caller). */
int wfl_transducer_decode_batch(const wfl_graph* tokens, const int32_t* labels, const int64_t* offsets, int B,
                                int32_t* out, int64_t out_capacity, int64_t* out_offsets, int nthreads);
/* Which make_token_graph(N tokens, blank, allow_repeats) (transducer.py:78-123) `tokens` is, arc for arc (all weights
 * zero): 0 blank "none", 1 blank "optional", 2 blank "forced" (each with repeats allowed), 3 blank "optional" without
 * repeats; *n_tokens = N (the blank, where there is one, is label N).  -1: none of them.  All four transduce a
 * frame-label sequence the same way wherever they accept it -- collapse repeats, drop the blank -- and only the
 * "forced" graph rejects sequences over its alphabet (WFL_DECODE_BLANK_SEPARATED below): what picks `drop` and the
 * flags of the device decode. */
int wfl_graph_token_kind(const wfl_graph* tokens, int* n_tokens);
/* Bulk builders for the three fixed-topology label graphs (no per-arc host calls):
 *   CTC  create_ctc_graph          ctc.py:15-29     targets flat + offsets[B+1], blank
 *   ASG  create_force_align_graph  asg.py:72-81 composed with the transitions graph asg.py:54-69:
 *        arcs carry wid into W[(C+1),C] row-major
 *   STC  create_stc_graph          stc.py:23-64     star_idx, log(prob) on star arcs */
wfl_lattice_host* wfl_lattice_pack_ctc(const int32_t* targets, const int64_t* offsets, int B, int blank, int C);
wfl_lattice_host* wfl_lattice_pack_asg_fal(const int32_t* targets, const int64_t* offsets, int B, int C);
wfl_lattice_host* wfl_lattice_pack_stc(const int32_t* targets, const int64_t* offsets, int B, int star_idx,
                                       float log_prob, int C);
void wfl_lattice_host_free(wfl_lattice_host* h);
const wfl_lattice_desc* wfl_lattice_host_desc(const wfl_lattice_host* h);
const int32_t* wfl_lattice_host_ints(const wfl_lattice_host* h);
const float* wfl_lattice_host_floats(const wfl_lattice_host* h);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: generic lattice engine
 *   loss_b-related quantity logZ_b = forward_score(intersect(emissions_b, A_b))
 * ------------------------------------------------------------------------------------------------ */
/* Bytes of scratch the calls below need: xg [B,T,max_labels], alpha/beta [sum_b (T+1) Q_b].
 * Returned through the out pointers (element counts of float32). */
int wfl_lattice_workspace(const wfl_lattice_desc* d, int T, int64_t* xg_elems, int64_t* ab_elems);
/* Diagnostics: offset (float32 elements) in the alpha buffer of the int32 [B] array that says how each
 * utterance of a log-semiring wfl_lattice_forward was swept (1: fp64 probability domain, 0: fp32 log
 * domain -- acceptor shape, or the certificate's repair). */
int wfl_lattice_formats_offset(const wfl_lattice_desc* d, int T, int64_t* offset);

/* Stage 1 (all CUs, coalesced): xg[b,t,k] = x[b,t,labels_b[k]].
 * If row_lse != NULL it also receives logsumexp_c x[b,t,c] and xg is written log-softmaxed
 * (fused torch.nn.functional.log_softmax of ctc.py:107 / transducer.py:186-187). */
int wfl_lattice_gather(const wfl_lattice_desc* d, const int32_t* ints, const float* x, int T, int C,
                       float* xg, float* row_lse, void* stream);

/* Stage 2 (one workgroup per utterance and direction): time-synchronous forward (alpha) and, if
 * beta != NULL, backward (beta) sweeps of gtn.forward_score (ctc.py:50, asg.py:111, stc.py:86,
 * transducer.py:283,287) / viterbi_score.  weights = learnable weight vector indexed by arc_wid
 * (may be NULL).  logz[B] receives the total score.  For WFL_SEMIRING_TROPICAL back-pointers are
 * written to bptr [sum_b T*Q_b] (int32) instead of beta. */
int wfl_lattice_forward(const wfl_lattice_desc* d, const int32_t* ints, const float* floats,
                        const float* xg, int T, const float* weights, int semiring, float* alpha,
                        float* beta, int32_t* bptr, float* logz, void* stream);

/* Stage 3 (all CUs): arc posteriors -> dense emission gradient rows and learnable-weight grads.
 *   dx[b,t,c] (+)= coef[b] * gout * sum_{arcs with label c} gamma_t(arc)
 *   dW[wid]    += coef_w[b] * gout * sum_t gamma_t(arc)           (atomic)
 * (gtn.backward + emissions.grad(): ctc.py:78-81, asg.py:158-168, stc.py:113-116,
 * transducer.py:321-325,333-336).  gout: device scalar (grad_output) or NULL for 1.
 * accumulate != 0 adds into dx instead of overwriting.  If row_lse != NULL the gradient is taken
 * through the fused log-softmax: dx = coef*(post - softmax(x) * sum_c post). */
int wfl_lattice_grad(const wfl_lattice_desc* d, const int32_t* ints, const float* floats,
                     const float* xg, int T, int C, const float* weights, const float* alpha,
                     const float* beta, const float* logz, const float* coef, const float* coef_w,
                     const float* gout, int accumulate, const float* x, const float* row_lse,
                     float* dx, float* dW, void* stream);

/* Stage 2 + the emission gradient in ONE launch (log semiring).  Same sweeps and outputs as
 * wfl_lattice_forward; when the batch allows it (uniform-label acceptors without epsilon arcs:
 * the Transducer's alignment graphs of transducer.py:262-281, CTC-like chains) the launch also
 * holds gradient workgroups that follow the two sweeps outwards from the middle of each utterance
 * and write   dx[b,t,c] = coef[b] * sum_{arcs with label c} gamma_t(arc)      (grad_output = 1)
 * (through the fused log-softmax if row_lse != NULL, as wfl_lattice_grad), and *in_launch is set to 1.
 * Otherwise *in_launch = 0, nothing is written to dx and wfl_lattice_grad does the whole job.
 * After in_launch = 1: scale dx by grad_output if it is not 1 (wfl_scale), then call
 * wfl_lattice_grad_rest, which overwrites the rows of the utterances the launch did not serve
 * (other acceptors; utterances the certificate sent to the log-domain sweeps). */
/* *in_launch on ENTRY: 2 = do not wait for the gradient workgroups before returning to the stream --
 * the caller queues more of its own launches first (the loss reduction) and then calls
 * wfl_lattice_side_join(stream), without which nothing may touch dx, alpha or beta afterwards;
 * any other value: the call joins before it returns. */
int wfl_lattice_side_join(void* stream);
int wfl_lattice_forward_grad(const wfl_lattice_desc* d, const int32_t* ints, const float* floats,
                             const float* xg, int T, int C, const float* weights, float* alpha,
                             float* beta, float* logz, const float* coef, const float* x,
                             const float* row_lse, float* dx, int* in_launch, void* stream);
/* What became of the gradient workgroups beside the sweeps (wfl_lattice_forward_grad), counters of the calling thread's
 * CURRENT DEVICE (a give-up on one GPU does not back off the others):
 *   out[0] calls that launched them            out[1] of those, gates that GAVE UP waiting for the sweeps (kernels of
 *   out[2] gates that went through                     two streams did not run at the same time: a serialising
 *   out[3] calls that took the plain path              profiler, a debugger) -- the call fell back to
 *          during the back-off after a give-up         wfl_lattice_grad_rest for every row, results unaffected
 *   out[4] calls left in the current back-off   out[5] 1 = the environment announces serialised launches
 *   out[6] the gate's bound (polls of ~2 us)           (AMD_SERIALIZE_KERNEL / HIP_LAUNCH_BLOCKING): never tried
 *   out[7] 1 = the side stream forks from the caller's stream (default)
 *   out[8] launches of the streamed sweeps and their gradient (process-wide host counter: one per wfl_lattice_forward /
 *          wfl_lattice_grad call that took them).  Acceptors whose sweeps do not fit one CU's LDS (more than 160 KiB
 *          of arcs, states and emission rows) are swept with their arcs streamed from L2 -- decided from the
 *          descriptor's maxima, the same way by every call (and by wfl_lattice_workspace, which then asks for room
 *          for the streamed arc copies behind the alpha layout); WFL_LATTICE_STREAMED=1 / 2 forces that path (tests).
 *   out[9] of the sweep launches in out[8], those whose state vectors lived in global memory (the alpha / beta arrays
 *          themselves: 2 * max_states doubles did not fit LDS beside the emission rows, or WFL_LATTICE_STREAMED=2);
 *          the others kept them in LDS.  The gradient of either is the same launch and is not counted here.
 * The device counters behind out[1..2] are read without synchronisation: they lag the stream. n <= 10 words; a caller
 * that asks for fewer gets the first n. */
int wfl_lattice_diagnostics(uint64_t* out, int n);
int wfl_lattice_grad_rest(const wfl_lattice_desc* d, const int32_t* ints, const float* floats,
                          const float* xg, int T, int C, const float* weights, const float* alpha,
                          const float* beta, const float* logz, const float* coef, const float* gout,
                          const float* x, const float* row_lse, float* dx, void* stream);

/* Tropical back-trace (gtn.viterbi_path, transducer.py:221): path[b, 0..len_b) = caller's arc
 * ids along the best path, in order, including epsilon arcs; path_len[b] its length
 * (<= T + max_levels*(T+1)); path stride = path_stride. */
int wfl_lattice_backtrace(const wfl_lattice_desc* d, const int32_t* ints, const float* floats,
                          const float* alpha, const int32_t* bptr, int T, int32_t* path,
                          int32_t* path_len, int path_stride, void* stream);

/* diagnostic: resident workgroups per CU of the lattice gradient kernel for a dynamic LDS size */
int wfl_debug_grad_occupancy(int lds_bytes);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: dense (fully connected) transitions -- ASG denominator / ASG Viterbi
 *   W [(C+1), C] row-major: W[0,i] start->i, W[1+i, j] = score(prev j -> cur i)  (asg.py:54-69)
 * ------------------------------------------------------------------------------------------------ */
/* Sizes of the scratch buffers: dW_partial [partial_elems] floats (per-workgroup partial sums of the
 * transition gradient) and the opaque workspace `ws` [ws_bytes] shared by forward and grad
 * (per-frame scale bookkeeping of the probability-domain sweeps, per-utterance range flags). */
int wfl_dense_workspace(int B, int T, int C, int64_t* partial_elems, int64_t* ws_bytes);
/* Largest C the dense-transition entry points accept (asg.py:191-209 has no limit: 16384 is an index-width bound).  Up
 * to wfl_dense_on_chip_classes() (192) the (C+1) x C matrix is private to a workgroup -- registers for the
 * probability-domain sweeps, LDS for the log-domain launches behind them; beyond, the frame update of the whole batch
 * runs as one tiled matrix product per frame on the matrix cores, the matrix streamed from L2 (csrc/dense_wide.h): same
 * entry points, same buffers (sizes from wfl_dense_workspace).  wfl_dense_viterbi keeps the matrix in registers up
 * to 256 classes (the max-plus frame has no matrix-core form) and takes a tiled per-frame launch beyond. */
int wfl_dense_max_classes(void);
int wfl_dense_on_chip_classes(void);
/* Byte offset / length of a field of the opaque dense workspace (diagnostics and tests, like wfl_ctc_workspace_field):
 * WFL_DENSE_WS_FLAGS = int32 [B][2], non-zero where a probability-domain sweep (forward, backward) handed the
 * utterance to the log-domain kernels. */
#define WFL_DENSE_WS_FLAGS 0
int wfl_dense_workspace_field(int B, int T, int field, int64_t* offset_bytes, int64_t* length_bytes);
/* The same for any class count C.  Beyond wfl_dense_on_chip_classes() the flags are the batch's range verdict on W
 * (an entry of W[1:] that is -inf, NaN, +inf or more than 2^-60 below its row maximum), the same for every utterance:
 * such a batch is recomputed by the log-domain launches behind the probability-domain product. */
int wfl_dense_workspace_field_c(int B, int T, int C, int field, int64_t* offset_bytes, int64_t* length_bytes);
/* forward_score(intersect(emissions, transitions)) (asg.py:114): logz [B]; alpha, beta [B,T,C] are
 * opaque inputs of wfl_dense_grad in the log semiring (scaled probabilities for utterances served
 * by the probability-domain sweep, log scores for utterances it had to hand to the log-domain
 * sweep; ws records which), max-plus scores in the tropical semiring (ws may be NULL there). */
int wfl_dense_forward(const float* x, const float* W, int B, int T, int C, int semiring,
                      float* alpha, float* beta, int32_t* bptr, float* logz, void* ws, void* stream);
/* dx[b,t,i] = (accumulate ? dx : 0) + gout*addend[b,t,i] + coef[b]*gout*post_t(i);
 * dW       = (accumulate ? dW : 0) + gout*dW_addend    + sum_b coef_w[b]*gout*transition posteriors.
 * `addend` [B,T,C] and `dW_addend` [(C+1),C] (either may be NULL): terms computed for gout = 1 before gout was
 * known -- the ASG numerator's posteriors, which the criterion computes during forward on a second stream under the
 * (longer) denominator sweeps (asg.py:158-168 adds the two gradients in backward). */
int wfl_dense_grad(const float* x, const float* W, int B, int T, int C, const float* alpha,
                   const float* beta, const float* logz, const float* coef, const float* coef_w,
                   const float* gout, int accumulate, const float* addend, const float* dW_addend,
                   float* dx, float* dW, float* dW_partial, const void* ws, void* stream);
/* The same two calls in parts, for a caller that runs them on two streams (criterions/asg.py through
 * csrc/torch_ops.cpp::asg_forward): the probability-domain launches serve every utterance whose transition matrix has a
 * bounded dynamic range, the log-domain launches behind them only what those flagged (normally nothing: they return at
 * once) -- different utterances, disjoint rows of every output.  A caller may put WFL_DENSE_REPAIR on a second stream,
 * ordered after the WFL_DENSE_MAIN part of wfl_dense_forward_parts (it reads the flags that part writes), and run
 * WFL_DENSE_REDUCE (the sum of the per-workgroup transition-gradient partials into dW) once both gradient parts are done.
 * WFL_DENSE_ALL on one stream is wfl_dense_forward / wfl_dense_grad.  Beyond wfl_dense_on_chip_classes() and in the
 * tropical semiring the work is one piece: it goes with WFL_DENSE_MAIN, the other parts do nothing. */
#define WFL_DENSE_MAIN 1
#define WFL_DENSE_REPAIR 2
#define WFL_DENSE_REDUCE 4
#define WFL_DENSE_ALL 7
int wfl_dense_forward_parts(const float* x, const float* W, int B, int T, int C, int semiring,
                            float* alpha, float* beta, int32_t* bptr, float* logz, void* ws, int parts, void* stream);
int wfl_dense_grad_parts(const float* x, const float* W, int B, int T, int C, const float* alpha,
                         const float* beta, const float* logz, const float* coef, const float* coef_w,
                         const float* gout, int accumulate, const float* addend, const float* dW_addend,
                         float* dx, float* dW, float* dW_partial, const void* ws, int parts, void* stream);
/* viterbi_path(intersect(emissions, transitions)).labels_to_list() (asg.py:225-226):
 * path [B,T] int32 emission labels.  Ties: lowest previous label, then lowest final label.
 * alpha [B,T,C]: the max-plus vectors (an output).  bptr: unused since round 5 (neither read nor written, may be NULL):
 * the back-trace re-derives the one back-pointer per frame it follows from the stored vectors; wfl_dense_forward in the
 * tropical semiring still fills a back-pointer buffer. */
int wfl_dense_viterbi(const float* x, const float* W, int B, int T, int C, float* alpha,
                      int32_t* bptr, int32_t* path, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: ConvTransduce1D (transducer.py:351-556)
 *   out[b, w, k] = forward_score | viterbi_score (intersect(x[b, w*stride : w*stride+ks, :],
 *                  make_kernel_graph(lexicon[k])))                       transducer.py:485-500
 *   x [B,T,C] already padded by the caller (T >= ks, transducer.py:468-470), Tout = (T-ks)/stride+1.
 *   ktab [K][36] int32 describes the lexicon: {L, skip mask (bit i: arc 2i-1 -> 2i+1 exists),
 *   tok[16], base[16] (index in kernel_params of entry k's arc 2i -> 2i+1), index of its arc 0->0,
 *   pad}; arc ids follow the insertion order of make_kernel_graph (transducer.py:351-364).
 *   params: kernel_params (NULL: all arc weights 0).  L <= 15, ks <= 16.
 * ------------------------------------------------------------------------------------------------ */
#define WFL_CONV_SPIKE 1          /* flags: no self loops on sub-token states */
#define WFL_CONV_BLANK_OPTIONAL 2 /* flags: state 2L-1 accepts, skip arcs between different sub-tokens */
/* Bytes of LDS a launch may use: the forward stages ks*C*4 of them, the backward twice that, and either returns
 * WFL_ERR_UNSUPPORTED beyond it (a caller that will need the gradient can ask before it runs the forward). */
int wfl_conv_lds_limit(void);
int wfl_conv_forward(const float* x, int B, int T, int C, const int32_t* ktab, int K, int ks,
                     int stride, int blank, int flags, const float* params, int semiring, float* out,
                     void* stream);
/* dx [B,T,C] = sum_{w,k} delta[b,w,k] * d out[b,w,k] / d x (overwritten); dparams [num_arcs]
 * (accumulated, may be NULL) likewise for kernel_params (transducer.py:514-552). */
int wfl_conv_grad(const float* x, int B, int T, int C, const int32_t* ktab, int K, int ks, int stride,
                  int blank, int flags, const float* params, int semiring, const float* delta,
                  float* dx, float* dparams, void* stream);

/* STC's alphabet augmentation (stc.py:199-220) in one launch each way.  x: log-probabilities [T, B, C] (the module's
 * input layout); select[K]: the classes of the batch, the blank (0) first, each once; inv[C]: select's inverse (-1 for a
 * class that is not selected).  out [B, T, 2K] = (selected columns | <star> = logsumexp over c >= 1 | <star>\token for
 * select[1..]), lse [T * B] the rows' <star> (kept for the backward); dx [T, B, C] is OVERWRITTEN with the gradient for
 * the upstream g [B, T, 2K]. */
int wfl_stc_augment(const float* x, int T, int B, int C, const int32_t* select, int K, float* out, float* lse, void* stream);
int wfl_stc_augment_grad(const float* x, int T, int B, int C, const int32_t* select, const int32_t* inv, int K,
                         const float* lse, const float* g, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: CTC fast path (create_ctc_graph + intersect + forward_score + backward of
 * ctc.py:15-94; banded recursion with register-resident state, no lattice arrays).
 *   targets: device int32 flat, offsets: device int64 [B+1]; requires max target length <= 255 and
 *   C <= 16384 (targets of more than 63 labels: C <= 602) -- the gradient tiles live in LDS
 *   (up to 63: one position per lane; longer: two to four positions per lane)
 *   (longer targets: WFL_ERR_UNSUPPORTED -> use wfl_lattice_pack_ctc + the lattice engine).
 *   loss_b = -logZ_b is written to nll[B]; dx = coef[b]*gout*posteriors (dense rows).
 *   Base-2 log-domain arithmetic, block-renormalised; the chain stores one checkpoint per 16
 *   frames and the gradient kernel recomputes inside the blocks (csrc/ctc_kernels.hip).
 * ------------------------------------------------------------------------------------------------ */
int wfl_ctc_workspace(int B, int T, int C, int max_len, int64_t* ws_elems);
/* Diagnostics: offset (in floats) and length of a bookkeeping field inside the CTC workspace.
 *   WFL_CTC_WS_REJECTED  int32[B]    (unused since round 4: the three-launch lane-exponent step is retired; zeros)
 *   WFL_CTC_WS_STATUS    int32[2]    pipelined step: [0] a gradient wave gave up waiting, [1] utterances repaired
 *   WFL_CTC_WS_LOG2Z     double[B]   log2 Z per utterance
 *   WFL_CTC_WS_ZRANGE    int64[B][2] pipelined lane-exponent step: min / max over the blocks of log2 Z * 2^16
 *   WFL_CTC_WS_DEBUG     per-wave cycle counters of a -DWFL_MITM_STATS=1 build (length 0 in a normal build)
 *   WFL_CTC_WS_CLOCK     int64[B][2][2] meet-in-the-middle step: the device's constant 100 MHz clock at the entry of every sweep's
 *                        workgroup and at the exit of its last wave (the launch's own duration, measured on the device) */
#define WFL_CTC_WS_REJECTED 0
#define WFL_CTC_WS_STATUS 1
#define WFL_CTC_WS_LOG2Z 2
#define WFL_CTC_WS_ZRANGE 3
#define WFL_CTC_WS_DEBUG 4
#define WFL_CTC_WS_CLOCK 5
int wfl_ctc_workspace_field(int B, int T, int max_len, int field, int64_t* offset_elems, int64_t* length_elems);
/* alpha and beta chains: writes nll[B] = -log Z_b and the 16-frame checkpoints into ws.
 * flags must be 0 (the log-domain chain; the lane-exponent variant of this call was retired in round 4 --
 * wfl_ctc_forward_backward is the training step). */
int wfl_ctc_forward(const float* x, int B, int T, int C, const int32_t* targets,
                    const int64_t* offsets, int max_len, int blank, int flags, float* ws, float* nll,
                    void* stream);
/* wfl_ctc_forward for a padded batch: input_lengths int32 [B] on the device (see wfl_ctc_call.input_lengths); targets of up
 * to 63 labels (WFL_ERR_UNSUPPORTED beyond), WFL_ERR_INVALID for NULL lengths. */
int wfl_ctc_forward_lengths(const float* x, int B, int T, int C, const int32_t* targets,
                            const int64_t* offsets, int max_len, int blank, int flags, float* ws, float* nll,
                            const int32_t* input_lengths, void* stream);
/* Per-call extras of wfl_ctc_forward_backward_call -- everything the step remembers or assumes beyond its arguments
 * is the CALLER's:
 *   n_labels    the number of labels behind `targets` the caller vouches for (= offsets[B] as the host knows it; 0:
 *               unknown).  With it a workgroup asks for its labels together with its offsets (one memory round trip at
 *               kernel entry instead of two) under the guess that every target has max_len labels -- true for bucketed
 *               batches and the benchmark's; a ragged batch asks again, results are the same.
 *   host_state  2 x int32 of PINNED host memory (hipHostMalloc / a pin_memory tensor), zeroed by the caller once, one per
 *               criterion / workspace and never shared between concurrent calls -- or NULL.  [0] is written by the
 *               repair launch (how many utterances of the last lane-exponent step it recomputed; system scope, nobody
 *               waits for it), [1] is the step's own counter.  When the LAST lane-exponent step recomputed more than an
 *               eighth of its utterances the call goes straight to the log-domain step, and every 16th such call tries
 *               the lane-exponent step again.  NULL: every call starts with the lane-exponent step.  Results are within
 *               the parity bar on either path (bit-identical only on the same path); zero the words to forget.
 *   input_lengths  per-utterance input lengths of a padded batch, int32 [B] on the DEVICE, 1 <= T_b <= T (the caller's
 *               to check), or NULL: every utterance has T frames.  A frame t >= T_b is read as a certain-blank frame
 *               (0 for the blank, -inf for every other class, nothing subtracted from it under row_lse): the identity
 *               of the CTC label graph, so nll[b] and the gradient rows t < T_b are those of x[b, :T_b] alone.  The
 *               launch still sweeps T frames; the rows t >= T_b of dx hold no gradient -- call wfl_zero_pad_rows behind
 *               it.  Targets of up to 63 labels only (WFL_ERR_UNSUPPORTED beyond: pad a copy, wfl_ctc_pad_frames). */
typedef struct wfl_ctc_call {
  int64_t n_labels;
  int32_t* host_state;
  const int32_t* input_lengths;
} wfl_ctc_call;

/* wfl_ctc_forward and wfl_ctc_grad as ONE pipelined launch: gradient waves wait for the checkpoints
 * they need and run while the chains are still sweeping.  Same outputs (nll, dx); posteriors are
 * normalised per 16-frame block by the Z the block reproduces.
 * Targets of up to 63 labels: chains and gradient blocks run in lane-exponent
 * (probability-domain) arithmetic; every block certifies its result (log2 Z reproduced to 1.5e-4, the
 * posteriors of its frames sum to one to 2e-4) and a second, normally empty launch recomputes rejected
 * utterances in the log domain -- the caller always receives certified or log-domain results.
 * WFL_CTC_PIPELINE=log in the environment selects the log-domain launch throughout.  If loss_out is
 * not NULL it also receives mean_b(loss_scale[b] * nll[b]) (ctc.py:68-69; loss_scale NULL = 1),
 * reduced in a fixed order by the last chain to finish -- no separate wfl_reduce_loss launch.
 * If row_lse is not NULL, x holds RAW scores and row_lse[b*T + t] their log-sum-exp over the classes
 * (wfl_row_lse): the log_softmax of the CTC module (ctc.py:107) is fused into the launch, forward
 * and backward (dx is then the gradient w.r.t. the raw scores). */
int wfl_ctc_forward_backward(const float* x, int B, int T, int C, const int32_t* targets,
                             const int64_t* offsets, int max_len, int blank, float* ws, float* nll,
                             const float* coef, const float* gout, float* dx, const float* loss_scale,
                             float* loss_out, const float* row_lse, void* stream);
/* wfl_ctc_forward_backward with the per-call extras above (call may be NULL: the same as the function above, which
 * keeps no memory between calls) */
int wfl_ctc_forward_backward_call(const float* x, int B, int T, int C, const int32_t* targets,
                                  const int64_t* offsets, int max_len, int blank, float* ws, float* nll,
                                  const float* coef, const float* gout, float* dx, const float* loss_scale,
                                  float* loss_out, const float* row_lse, const wfl_ctc_call* call, void* stream);
/* out[r] = logsumexp_c x[r*C + c] for r < rows (NaN counts as -inf) */
int wfl_row_lse(const float* x, int64_t rows, int C, float* out, void* stream);
/* out[r] = the first c with x[r*C + c] == max_c x[r*C + c] (NaN counts as -inf; a row without a finite score: 0) --
 * viterbi_path of the bare emissions graph (transducer.py:205-216 without transitions), one frame per row */
int wfl_row_argmax(const float* x, int64_t rows, int C, int32_t* out, void* stream);
/* dense gradient rows, recomputed block by block from the checkpoints of wfl_ctc_forward */
int wfl_ctc_grad(const float* x, int B, int T, int C, const int32_t* targets, const int64_t* offsets,
                 int max_len, int blank, const float* ws, const float* nll, const float* coef,
                 const float* gout, float* dx, void* stream);
/* wfl_ctc_grad behind wfl_ctc_forward_lengths (same lengths); the rows t >= T_b of dx hold no gradient: wfl_zero_pad_rows */
int wfl_ctc_grad_lengths(const float* x, int B, int T, int C, const int32_t* targets, const int64_t* offsets,
                         int max_len, int blank, const float* ws, const float* nll, const float* coef,
                         const float* gout, float* dx, const int32_t* input_lengths, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: the decode behind a best path (csrc/decode_kernels.hip)
 *   what every criterion's viterbi() ends with -- ctc.py:126-135, asg.py:225-234, transducer.py:216-232 -- per
 *   utterance and in frame order:
 *     frame t is kept iff lab[t] != lab[t-1] (t = 0: always a candidate) and lab[t] != drop   (drop = -1: nothing);
 *     num_replabels = R > 0: unpack_replabels (asg.py:35-49) on the kept values -- v >= R emits v - R; v < R emits
 *       u - R another v + 1 times if the kept value right before it in the row is a label u >= R, else nothing;
 *     WFL_DECODE_BLANK_SEPARATED (needs drop >= 0): the row decodes to nothing unless it starts and ends with `drop`
 *       and no two different non-drop labels are adjacent (make_token_graph(blank="forced"), transducer.py:78-123).
 *   Labels are >= 0.  out: the utterances back to back in batch order (capacity B T max(1, R) int32),
 *   out_offsets [B+1] int64.  Both are written by plain stores of a kernel, in a fixed order (no atomics: the result
 *   is deterministic), so they may be any device-accessible memory -- pinned host memory delivers the few labels that
 *   survive the collapse to the host without a copy call (wfl_upload's trick in the other direction).  ws: device
 *   scratch of wfl_decode_workspace's size, 16-byte aligned, contents irrelevant before and after.  Three launches on
 *   `stream`, no allocation, no synchronisation.  WFL_ERR_INVALID: B < 1, T < 1, C < 1, R < 0, drop outside [-1, C)
 *   (paths: < -1), path_stride < T, out_capacity too small, an unknown flag.
 * ------------------------------------------------------------------------------------------------ */
#define WFL_DECODE_NAN_IS_MAX 1       /* emissions: a NaN is the maximum, the first NaN wins (torch.argmax, ctc.py:128) */
#define WFL_DECODE_BLANK_SEPARATED 2  /* reject rows the blank="forced" token graph does not accept */
/* frames per chunk: the frames are split into chunks over the grid, and the previous label, the last kept value and
 * the output count are carried across the chunk boundaries (tests straddle them) */
int wfl_decode_chunk_frames(void);
/* wavefront steps per LDS fill of wfl_errors_count's distance launch (compute_edit_distance, train.py:74-87; test.py:94-109):
 * a strip of W <= 64 reference columns against n hypothesis rows takes n + W - 1 steps, and the cell values and the
 * boundary column are carried from one fill to the next (tests cross it) */
int wfl_errors_chunk_steps(void);
/* out_capacity = B T max(1, num_replabels) (int32 elements of `out`), ws_bytes = the device scratch of a call */
int wfl_decode_workspace(int B, int T, int num_replabels, int64_t* out_capacity, int64_t* ws_bytes);
/* lab[b][t] = the first maximal class of x[b,t,:] + bias (x [B,T,C] float32; bias [C] or NULL: the unigram transition
 * model's x + params, transducer.py:205-216, added in float32), never written to memory.  Ties: the lowest class.
 * Default: NaN counts as -inf, a row without a finite score gives class 0 (wfl_row_argmax's rule);
 * WFL_DECODE_NAN_IS_MAX: torch.argmax's (ctc.py:128).  Replaces ctc.py:126-135 and transducer.py:216-232. */
int wfl_decode_emissions(const float* x, const float* bias, int B, int T, int C, int drop, int num_replabels, int flags,
                         void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets, void* stream);
/* wfl_decode_emissions for a padded batch: lengths [B] int32 on the device, utterance b has the frames [0, lengths[b])
 * (values are clamped to [0, T]).  A frame t >= lengths[b] is no candidate: it is not read, not kept, and the previous
 * label / last kept value carried across the chunk boundaries are those of a row that ends at lengths[b] -- the result
 * for utterance b is wfl_decode_emissions' of x[b, :lengths[b]] alone (WFL_DECODE_BLANK_SEPARATED: its last frame is
 * lengths[b] - 1).  Same launches, workspace and capacities.  WFL_ERR_INVALID also for lengths == NULL. */
int wfl_decode_emissions_lengths(const float* x, const float* bias, const int32_t* lengths, int B, int T, int C, int drop,
                                 int num_replabels, int flags, void* ws, int32_t* out, int64_t out_capacity,
                                 int64_t* out_offsets, void* stream);
/* lab[b][t] = paths[b * path_stride + t]: the label paths of wfl_dense_viterbi.  Replaces asg.py:225-234 and
 * transducer.py:216-232 under the bigram transition model. */
int wfl_decode_paths(const int32_t* paths, int64_t path_stride, int B, int T, int drop, int num_replabels, int flags,
                     void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: CTC prefix beam search (csrc/beam_kernels.hip)
 *   wfl_decode_emissions gives the best FRAME PATH (argmax per frame, collapse, drop the blank).  CTC scores a LABEL
 *   SEQUENCE by the sum over all its alignments; this search maximises that.  Per utterance b, over the frames
 *   t < T_b of x [B,T,C] float32 (a NaN counts as -inf), with beam width W = beam, K = classes_per_frame:
 *     - all hypothesis arithmetic is float64 in the log domain, lae(a, b) = max(a, b) + log1p(exp(-|a - b|)), -inf the
 *       identity;
 *     - candidates of a frame: its K classes of highest score, ties to the lower class, in that order; the blank is
 *       appended if it is not among them;
 *     - a hypothesis is (prefix, pb, pnb): the log mass of the prefix' alignments that end in the blank / do not; the
 *       search starts from the empty prefix with pb = 0, pnb = -inf; the beam is ranked by tot = lae(pb, pnb), descending;
 *     - frame t, hypothesis of rank i, candidate c with s = (double)x[b,t,c]: c the blank -- i's stay entry gets
 *       pb' = s + tot_i; c the last label of i -- the stay entry gets pnb' = s + pnb_i and the extension i + c gets
 *       e = s + pb_i; any other c -- the extension i + c gets e = s + tot_i;
 *     - an extension whose prefix is that of a hypothesis j in the beam is merged into j's stay entry,
 *       pnb'_j = lae(pnb'_j, e) (there is at most one per j); every other extension is a new entry (pb' = -inf, pnb' = e);
 *     - entries with tot' = -inf are dropped, the W entries of largest tot' survive, in the order: larger tot'; stay
 *       entries before new ones; the lower parent rank; the lower position of c among the candidates.  Nothing survives:
 *       the utterance decodes to the empty sequence with score -inf.
 *   Prefixes are identified by (two 64-bit rolling hashes h' = h * P + c + 1 mod 2^64 with different odd P, length, last
 *   label).
 *   Result: the first nbest ranks of the final beam.  out: their labels back to back in (b, rank) order (capacity
 *   B nbest T int32), out_offsets [B nbest + 1] int64, scores [B nbest] float64 = tot, minus the sum over t < T_b of the
 *   rows' log-sum-exps over all C classes (wfl_row_lse's rule, added up in float64 in frame order) if normalize != 0.
 *   Ranks beyond the final beam's size are empty sequences with score -inf.  With nbest == 1, out / out_offsets are what
 *   wfl_errors_count reads as hyp / hyp_off.  lengths: int32 [B] on the device or NULL (every utterance has T frames);
 *   values are clamped to [0, T], frames t >= T_b are not read, T_b = 0 gives the empty sequence with score 0.
 *   out, out_offsets and scores are written by plain stores of a kernel in a fixed order: any device-accessible memory,
 *   pinned host memory included; the result is deterministic.  ws: device scratch of wfl_ctc_beam_workspace's size,
 *   16-byte aligned, contents irrelevant before and after.  Three launches on `stream` (candidates: a wave per frame, the
 *   only pass over x; beam: a workgroup per utterance; write), no allocation, no synchronisation.
 *   WFL_ERR_INVALID: a NULL required pointer, B, T or C < 1, blank outside [0, C), beam outside [1, 64],
 *   classes_per_frame outside [1, min(C, 64)], nbest outside [1, beam], out_capacity too small.
 *   WFL_ERR_UNSUPPORTED: C > 16384.  CTC only.  A token-level n-gram LM and a length bonus: wfl_ctc_beam_search_lm
 *   below; a lexicon and a word-level LM: wfl_ctc_beam_search_lexicon below that.
 * ------------------------------------------------------------------------------------------------ */
/* out_capacity = B nbest T (int32 elements of `out`), ws_bytes = the device scratch of a call */
int wfl_ctc_beam_workspace(int B, int T, int C, int beam, int classes_per_frame, int nbest, int64_t* out_capacity,
                           int64_t* ws_bytes);
int wfl_ctc_beam_search(const float* x, const int32_t* lengths /* or NULL */, int B, int T, int C, int blank, int beam,
                        int classes_per_frame, int nbest, int normalize, void* ws, int32_t* out, int64_t out_capacity,
                        int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same search with a token-level n-gram LM and a length bonus fused in (csrc/beam_kernels.hip).
 *   Every rule of wfl_ctc_beam_search stands; the additions:
 *     - LM form: a deterministic back-off acceptor over the emission classes.  State s has the arcs
 *       [arc_ptr[s], arc_ptr[s+1]) =(arc_label, arc_next, arc_w), labels strictly ascending, w float64 natural log, and
 *       an optional back-off (bo_next[s], bo_w[s]), bo_next[s] = -1 for none.  Labels are CTC class indices 0 .. C-1,
 *       never the blank; label C stands for </s> (the next state of such an arc is not used).  `start` is the <s> history.
 *     - step(s, c): acc = 0; search c among the arcs of s (a binary search, at most 31 steps); found: (acc + w, next);
 *       s without a back-off: (-inf, none); otherwise acc += bo_w[s], s = bo_next[s], search again.  A chain has at
 *       most WFL_NGRAM_LM_MAX_BACKOFF = 8 back-offs; the kernel's loop is bounded by the same constant.
 *     - every hypothesis carries an LM state, the empty prefix has `start`;
 *     - the extension i + c: (l, nxt) = step(state_i, c); l = -inf: the extension does not exist; otherwise
 *       e = (s + base) + (lm_weight l + length_bonus), base as above (pb_i if c is i's last label, else tot_i), and the
 *       new entry has the state nxt.  An extension with s + base = -inf does not exist either (no lookup).  The kernel also
 *       skips the lookup of an extension that cannot reach the W-th best stay entry even with the LM's largest term,
 *       max(lm_weight step_min, lm_weight step_max) + length_bonus: such an entry is outside the beam whatever its step.
 *     - stays add nothing and keep their state; a merged extension carries the same term as a new one (state and LM
 *       score are functions of the prefix), so unpruned tot(l) = mass(l) + lm_weight LM(l) + length_bonus |l| exactly;
 *     - candidates (by acoustic score alone), the order of entries, the tie rule and the -inf drop rule do not change;
 *     - score_eos != 0: after the last frame rank r gets tot_r + lm_weight step(state_r, C); a rank whose step is -inf is
 *       dropped, the rest are ranked again by the new score, descending, ties to the earlier rank; nbest is taken after
 *       that.  T_b = 0 gives the empty sequence with score lm_weight step(start, C) (0 without score_eos);
 *     - normalize still subtracts the rows' log-sum-exps and nothing else.
 *   lm: a struct in HOST memory of DEVICE pointers to a pack that wfl_ngram_lm_check accepted (with host pointers, for
 *   the same C and blank), with the step_min / step_max that check wrote -- the kernels trust it: they check no index.
 *   lm_weight, length_bonus: finite.  The same workspace (wfl_ctc_beam_workspace), outputs, three launches and
 *   guarantees as wfl_ctc_beam_search; no global atomics, no cross-workgroup waits, every loop bounded by T_b, W, K,
 *   the back-off cap or 31 search steps.
 *   WFL_ERR_INVALID: what wfl_ctc_beam_search refuses; lm or one of its arrays NULL, num_states < 1, num_arcs < 0,
 *   start outside [0, num_states), step_min or step_max NaN, a weight or bonus that is not finite.
 * ------------------------------------------------------------------------------------------------ */
#define WFL_NGRAM_LM_MAX_BACKOFF 8
typedef struct wfl_ngram_lm {
  int32_t num_states, num_arcs, start, reserved;
  double step_min, step_max; /* written by wfl_ngram_lm_check: every step(s, c) that is not -inf lies in between */
  const int32_t* arc_ptr;   /* [num_states + 1], arc_ptr[0] = 0, arc_ptr[num_states] = num_arcs */
  const int32_t* arc_label; /* [num_arcs] */
  const int32_t* arc_next;  /* [num_arcs] */
  const double* arc_w;      /* [num_arcs] */
  const int32_t* bo_next;   /* [num_states], -1: no back-off */
  const double* bo_w;       /* [num_states] */
} wfl_ngram_lm;
/* The pack check (host arrays, no device): sizes and `start` in range, arc_ptr ascending from 0 to num_arcs, labels
 * strictly ascending within a state, in [0, C], never the blank; arc_next and bo_next in range (bo_next may be -1); the
 * back-off chains acyclic and at most WFL_NGRAM_LM_MAX_BACKOFF deep; no weight NaN or +inf.  WFL_ERR_INVALID names the first offence in
 * wfl_last_error().  On success it WRITES lm->step_min and lm->step_max, the bounds the search prunes lookups with:
 * [min arc weight + 8 min(0, least back-off weight), max arc weight + 8 max(0, largest back-off weight)], [0, 0]
 * without arcs; whatever they held before is not read.  A caller copies them into the struct of device pointers it
 * hands to wfl_ctc_beam_search_lm. */
int wfl_ngram_lm_check(wfl_ngram_lm* lm, int C, int blank);
int wfl_ctc_beam_search_lm(const float* x, const int32_t* lengths /* or NULL */, int B, int T, int C, int blank, int beam,
                           int classes_per_frame, int nbest, int normalize, const wfl_ngram_lm* lm, double lm_weight,
                           double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                           int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same search with a lexicon and an optional word-level n-gram LM (csrc/beam_kernels.hip).
 *   Every rule of wfl_ctc_beam_search stands; with a = lm_weight, o = word_bonus, b = length_bonus the additions:
 *     - lexicon form: a trie over the words' spellings (sequences of emission classes, never the blank), packed as a CSR
 *       of nodes with the root at node 0.  Node n has the arcs [arc_ptr[n], arc_ptr[n+1]) = (arc_label, arc_next), labels
 *       strictly ascending; arc_next >= 0: an inner node; arc_next = -(v+1): the arc completes word v and leads back to
 *       the root.  No leaves are stored.  The lexicon is prefix-free (no spelling is a prefix of another): a label
 *       sequence has at most one segmentation into words, so trie node and LM state are functions of the prefix;
 *     - word LM form: a wfl_ngram_lm over word ids -- word v is label v, V = num_words is its unused blank and V + 1 its
 *       </s> -- checked by wfl_ngram_lm_check with C = V + 1, blank = V; NULL: every word's step is 0;
 *     - every hypothesis carries a trie node and an LM state, the empty prefix has the root and the LM's `start`;
 *     - the extension i + c, base as in wfl_ctc_beam_search (pb_i if c is i's last label, else tot_i): c is searched
 *       among the arcs of node_i (a binary search, at most 31 steps).  Absent: the extension does not exist.  An inner
 *       arc: e = (s + base) + b, the new node is the arc's target, the LM state stays.  An arc that completes word v:
 *       (l, nxt) = step(state_i, v), (0, -) without an LM; l = -inf: the extension does not exist; otherwise
 *       e = (s + base) + ((a l + o) + b), the new node is the root and the new LM state nxt.  An extension with
 *       s + base = -inf does not exist and is not looked up.  The kernel also skips the lookup of an extension that
 *       cannot reach the W-th best stay entry even with the largest term, max(0, max(a step_min, a step_max) + o) + b
 *       (step_min = step_max = 0 without an LM): such an entry is outside the beam whatever its arc;
 *     - stays add nothing and keep node and state; a merged extension carries the same term as a new one, so unpruned
 *       tot(l) = mass(l) + a LM(words(l)) + o #words + b |l| exactly;
 *     - candidates (by acoustic score alone), the order of entries, the tie rule and the -inf drop rule do not change;
 *     - after the last frame a rank whose node is not the root is dropped (it ends inside a word); with score_eos != 0
 *       and an LM a remaining rank gets + a step(state, V + 1) and is dropped if that step is -inf; the remaining ranks
 *       are ranked again by score, descending, ties to the earlier rank; nbest is taken after that; nothing left: the
 *       empty sequence with score -inf.  T_b = 0 gives the empty sequence with score a step(start, V + 1), 0 without
 *       score_eos or without an LM;
 *     - normalize still subtracts the rows' log-sum-exps and nothing else; out holds the token labels as before.
 *   lex, word_lm: structs in HOST memory of DEVICE pointers to packs that wfl_lexicon_check (for the same C and blank)
 *   and wfl_ngram_lm_check (for V + 1 and V) accepted with host pointers -- the kernels trust them: they check no
 *   index.  The same workspace (wfl_ctc_beam_workspace), outputs, three launches and guarantees as wfl_ctc_beam_search;
 *   no global atomics, no cross-workgroup waits, every loop bounded by T_b, W, K, the back-off cap or 31 search steps.
 *   WFL_ERR_INVALID: what wfl_ctc_beam_search refuses; lex or one of its arrays NULL, num_nodes, num_arcs or num_words
 *   < 1 (or num_words = 2^31 - 1: </s> is V + 1); a weight or bonus that is not finite; for a non-NULL word_lm what wfl_ctc_beam_search_lm refuses.
 *   Not here: a token-level LM together with a lexicon, out-of-vocabulary arcs (LM look-ahead inside words:
 *   wfl_ctc_beam_search_lexicon_lookahead, below the Transducer's lexicon search).  Several
 *   spellings of one word and vocabularies that are not prefix-free: wfl_ctc_beam_search_lexicon_marked below.
 * ------------------------------------------------------------------------------------------------ */
typedef struct wfl_lexicon {
  int32_t num_nodes, num_arcs, num_words, reserved;
  const int32_t* arc_ptr;   /* [num_nodes + 1], arc_ptr[0] = 0, arc_ptr[num_nodes] = num_arcs */
  const int32_t* arc_label; /* [num_arcs] */
  const int32_t* arc_next;  /* [num_arcs], >= 0 inner node, -(v+1) completes word v */
} wfl_lexicon;
/* The pack check (host arrays, no device): sizes >= 1, arc_ptr ascending from 0 to num_arcs; labels strictly ascending
 * within a node, in [0, C), never the blank; every inner target in [1, num_nodes) and the target of exactly one arc,
 * every node reached from the root (a tree rooted at node 0); every node, the root included, has at least one arc (no
 * dead ends); every word id in [0, num_words) is completed by exactly one arc.  WFL_ERR_INVALID names the first offence
 * in wfl_last_error(). */
int wfl_lexicon_check(const wfl_lexicon* lex, int C, int blank);
int wfl_ctc_beam_search_lexicon(const float* x, const int32_t* lengths /* or NULL */, int B, int T, int C, int blank, int beam,
                                int classes_per_frame, int nbest, int normalize, const wfl_lexicon* lex,
                                const wfl_ngram_lm* word_lm /* or NULL */, double lm_weight, double word_bonus,
                                double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                                int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The lexicon searches with a START-MARKED lexicon (csrc/beam_kernels.hip): word pieces as they are,
 * the word boundary carried by the class that BEGINS a word.  Such a vocabulary is not prefix-free (a word may be a
 * proper prefix of another, a word may have several spellings), yet a label sequence still has one segmentation: a
 * word has ended where the next one begins, or where the utterance ends.  Every rule of wfl_ctc_beam_search_lexicon
 * (and of wfl_transducer_beam_search_lexicon) stands unless replaced here; a = lm_weight, o = word_bonus, b = length_bonus.
 *     1. the lexicon: a trie with root 0 in wfl_lexicon's CSR whose nodes may be terminal: node_word[n] = v >= 0 where a
 *        spelling of word v ends, -1 otherwise.  Leaves are stored: every arc_next is a node >= 1.  A node without arcs
 *        is terminal; the root is not.  Several terminal nodes may carry one word id (several spellings of a word); a
 *        spelling is that of one word.  Spellings may be proper prefixes of one another.  The one structural condition:
 *        the set R of labels on the root's arcs is disjoint from the labels of all deeper arcs.  start_node[c], c in
 *        [0, C), is the root's child by c, -1 if c is not in R;
 *     2. every hypothesis carries a trie node and, with a word LM, an LM state: the history of the COMPLETED words.
 *        Only the empty prefix is at the root.  Both are functions of the prefix;
 *     3. the extension i + c, s + base as in the end-marked search, -inf: it does not exist and is not looked up.
 *        c not in R: c is searched among the arcs of node_i (the bounded binary search); absent, or node_i the root: the
 *        extension does not exist; present: e = (s + base) + b, the node is the arc's target, the state stays.
 *        c in R from the root: e = (s + base) + b, the node is start_node[c], the state stays.
 *        c in R from a node with v = node_word[node_i] >= 0: (l, nxt) = step(state_i, v), (0, -) without an LM; l = -inf:
 *        the extension does not exist; otherwise e = (s + base) + ((a l + o) + b), each operation rounded on its own,
 *        the node is start_node[c] and the state nxt.  c in R from a non-terminal node: the extension does not exist;
 *     4. stays, merging by prefix, candidates, entry order, the tie rule, the -inf drop rule and the prune bound do not
 *        change: every term is b or (a l + o) + b, so max(0, max(a step_min, a step_max) + o) + b still bounds it;
 *     5. after the last frame: a rank at the root (the empty sequence) keeps its score; a rank at a terminal node gets
 *        + (a l + o) for its pending word, (l, nxt) = step(state, node_word[node]), moves to nxt, and is dropped if
 *        l = -inf; a rank at any other node is dropped.  Then the </s> term, the re-ranking and nbest as in the
 *        end-marked search, T_b = 0 included (the Transducer: the topology's score first, as in its rule 5);
 *     6. unpruned, tot(l) = mass(l) + a LM(words(l)) + o #words + b |l| plus the </s> term for every l that ends at a
 *        terminal node.  Two spellings of the same words are different label sequences and separate hypotheses;
 *     7. during the search a hypothesis is ranked WITHOUT the LM term of its pending (last, unfinished) word: that term
 *        arrives with the next word's first label or at the end.  A property, not a defect.
 *   The same workspace functions, outputs, three launches, refusals and guarantees as the end-marked siblings: no
 *   allocation, no synchronisation, no global atomics, no cross-workgroup waits, every loop bounded.  lex: a struct in HOST
 *   memory of DEVICE pointers to a pack that wfl_lexicon_marked_check accepted with host pointers; the kernels trust it.
 *   WFL_ERR_INVALID besides the siblings': node_word or start_node NULL.  The Transducer entry with Wt == NULL and
 *   forced == 0 runs the CTC entry's search: bit-identical results.
 *   Not here: ASG, a token-level LM together with a lexicon, merging by spelling together with a lexicon,
 *   out-of-vocabulary arcs.  (LM look-ahead, which lifts rule 7: the *_lexicon_marked_lookahead entries below.)
 * ------------------------------------------------------------------------------------------------ */
typedef struct wfl_lexicon_marked {
  wfl_lexicon trie;          /* arc_next: every target a node in [1, num_nodes) */
  const int32_t* node_word;  /* [num_nodes], the word whose spelling ends at the node, -1: none */
  const int32_t* start_node; /* [C], the root's child by the class, -1: the class starts no word */
} wfl_lexicon_marked;
/* The pack check (host arrays, no device), every clause of rule 1: sizes >= 1, arc_ptr ascending from 0 to num_arcs;
 * labels strictly ascending within a node, in [0, C), never the blank; every target in [1, num_nodes) and the target of
 * exactly one arc, every node reached from the root (a tree rooted at node 0); node_word in [-1, num_words), -1 at the
 * root, >= 0 at a node without arcs; every word id on at least one node; start_node[c] the root's child by c or -1; no
 * label of a root arc on a deeper arc.  WFL_ERR_INVALID names the first offence in wfl_last_error(). */
int wfl_lexicon_marked_check(const wfl_lexicon_marked* lex, int C, int blank);
int wfl_ctc_beam_search_lexicon_marked(const float* x, const int32_t* lengths /* or NULL */, int B, int T, int C, int blank,
                                       int beam, int classes_per_frame, int nbest, int normalize, const wfl_lexicon_marked* lex,
                                       const wfl_ngram_lm* word_lm /* or NULL */, double lm_weight, double word_bonus,
                                       double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                                       int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);
int wfl_transducer_beam_search_lexicon_marked(const float* x, const float* Wt /* [(C+1), C] or NULL */,
                                              const float* logz /* [B] or NULL */, int B, int T, int C, int blank, int forced,
                                              int beam, int classes_per_frame, int nbest, int normalize,
                                              const wfl_lexicon_marked* lex, const wfl_ngram_lm* word_lm /* or NULL */,
                                              double lm_weight, double word_bonus, double length_bonus, int score_eos, void* ws,
                                              int32_t* out, int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */,
                                              double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: ASG prefix beam search (csrc/beam_kernels.hip)
 *   wfl_dense_viterbi gives the best FRAME PATH under emissions + transitions (asg.py:211-224).  The ASG criterion scores a
 *   LABEL SEQUENCE by the sum over all its alignments -- the force-align numerator, asg.py:72-115 --; this search
 *   maximises that, on the launches of wfl_ctc_beam_search.  The reference has no such decoder.  Per utterance b, over
 *   all T frames of x [B,T,C] float32 (a NaN counts as -inf), with the transitions Wt [(C+1), C] float32 in the
 *   criterion's layout (asg.py:54-69: Wt[0][c] is start -> c, Wt[1+i][j] is j -> i; a NaN counts as -inf, +inf is not a
 *   weight), beam width W = beam, K = classes_per_frame.  There is no blank and there are no input lengths: ASG has neither.
 *     1. all hypothesis arithmetic is float64 in the log domain with wfl_ctc_beam_search's lae; scores and transition
 *        weights are widened from float32 exactly;
 *     2. candidates of a frame: its K classes of highest EMISSION score, ties to the lower class, in that order;
 *        transitions do not enter the choice and no class is appended;
 *     3. a hypothesis is (prefix, p): a class sequence without two equal neighbours and the log mass of all its
 *        alignments over the frames so far, emissions plus transitions; the search starts from the empty prefix with
 *        p = 0; the beam is ranked by p, descending;
 *     4. frame t, hypothesis of rank i with last label l, candidate c with s = (double)x[b,t,c]: c == l -- i's stay entry
 *        gets p' = (s + Wt[1+l][l]) + p_i; c != l -- the extension i + c gets e = (s + Wt[1+c][l]) + p_i; from the empty
 *        prefix (only at t = 0) e = (s + Wt[0][c]) + 0.  The empty prefix has no stay entry, and neither has a hypothesis
 *        whose last label is not among the candidates: it lives on only through its extensions (CTC's blank keeps every
 *        hypothesis alive; ASG has none);
 *     5. an extension whose prefix is that of a hypothesis j in the beam is merged into j's stay entry by lae (there is
 *        at most one per j, and j's last label is then a candidate, so the stay entry exists, possibly at -inf); every
 *        other extension is a new entry;
 *     6. selection and order are wfl_ctc_beam_search's: entries at -inf are dropped (an extension over a -inf transition
 *        among them), the W entries of largest p' survive, in the order: larger p'; stay entries before new ones; the
 *        lower parent rank; the lower position of c among the candidates.  Nothing survives: the empty sequence, -inf;
 *     7. result: the first nbest ranks with their p, minus (double)logz[b] if logz is not NULL -- logz [B] float32 on the
 *        device, the denominator wfl_dense_forward computes (asg.py:114): the normalised score of a sequence is then minus
 *        its ASG loss where none of its alignments was pruned, a lower bound of that otherwise.  Ranks beyond the final
 *        beam's size are empty sequences with score -inf.
 *   Prefixes are identified as in wfl_ctc_beam_search.  drop, num_replabels: the mapping of a result on its way out, with
 *   the meaning they have in wfl_decode_paths (what ASG.viterbi does to a path, asg.py:225-234): labels equal to drop
 *   (the garbage class; -1: none) are removed, then a label v >= num_replabels becomes v - num_replabels and a replabel
 *   right behind a label repeats it (asg.py:35-49).  drop = -1, num_replabels = 0: the raw class sequences.  The search
 *   and the scores are over raw sequences whatever the mapping.  out: the (mapped) labels back to back in (b, rank) order,
 *   capacity B nbest T max(1, num_replabels) int32 (wfl_decode_workspace's rule per rank); out_offsets [B nbest + 1] int64;
 *   scores [B nbest] float64; with nbest == 1, out / out_offsets are what wfl_errors_count reads as hyp / hyp_off.  All
 *   three are written by plain stores of a kernel in a fixed order: any device-accessible memory, pinned host memory
 *   included; the result is deterministic.  ws: device scratch of wfl_asg_beam_workspace's size, 16-byte aligned.  Three
 *   launches on `stream` (candidates; beam: a workgroup per utterance, one gather from Wt per entry; write), four with a
 *   mapping (the mapped lengths are counted before they are stored: a result is walked from its end); no allocation, no
 *   synchronisation, no atomics on global memory, no cross-workgroup waits, every loop bounded by T, W, K.
 *   WFL_ERR_INVALID: a NULL required pointer (logz may be NULL), B, T or C < 1, beam outside [1, 64], classes_per_frame
 *   outside [1, min(C, 64)], nbest outside [1, beam], drop outside [-1, C), num_replabels < 0, out_capacity too small.
 *   WFL_ERR_UNSUPPORTED: C > 16384, T max(1, num_replabels) >= 2^31.  Not here: input lengths.  A lexicon:
 *   wfl_asg_beam_search_lexicon; a token-level LM: wfl_asg_beam_search_lm.
 * ------------------------------------------------------------------------------------------------ */
/* out_capacity = B nbest T max(1, num_replabels) (int32 elements of `out`), ws_bytes = the device scratch of a call */
int wfl_asg_beam_workspace(int B, int T, int C, int beam, int classes_per_frame, int nbest, int num_replabels,
                           int64_t* out_capacity, int64_t* ws_bytes);
int wfl_asg_beam_search(const float* x, const float* Wt /* [(C+1), C] */, const float* logz /* [B] or NULL */, int B, int T,
                        int C, int beam, int classes_per_frame, int nbest, int drop, int num_replabels, void* ws, int32_t* out,
                        int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * The ASG search with a lexicon and an optional word-level n-gram LM (csrc/beam_kernels.hip).
 *   Every rule of wfl_asg_beam_search stands.  a = lm_weight, o = word_bonus, b = length_bonus, all finite float64 (the
 *   names of wfl_ctc_beam_search_lexicon); R = num_replabels; C = the classes of x (tokens + R + the garbage, if any).
 *     1. raw classes: replabel k is class k (k < R), token i is class i + R, the garbage class -- if the criterion has
 *        one -- is `garbage` = tokens + R (-1: none).  The lexicon is a wfl_lexicon over RAW class sequences: a word's
 *        spelling is its token sequence (separator token included, if there is one) packed as the criterion packs its
 *        targets (asg.py:13-32), so "aa|" with R = 1 is [a + R, 0, sep + R].  A spelling never contains the garbage;
 *     2. every hypothesis carries a trie node and, with a word LM, an LM state; the empty prefix has the root and the
 *        LM's `start`.  Both are functions of the raw prefix, so merging by prefix identity (rule 5 of the ASG search)
 *        stays exact, and a merged extension carries the same term as a new one;
 *     3. the extension of hypothesis i (last label l, the start for the empty prefix) by candidate c != l, with
 *        ac = (s + Wt[1+c][l]) + p_i as in rule 4 of the ASG search: c == garbage -- the garbage is transparent: e = ac,
 *        node and state stay, nothing is looked up and nothing is added.  Otherwise c is searched among the arcs of
 *        node_i (a binary search, at most 31 steps).  Absent: the extension does not exist.  An inner arc: e = ac + b,
 *        the node becomes the arc's target, the state stays.  An arc that completes word v: (l, nxt) = step(state_i, v),
 *        (0, -) without an LM; l = -inf: the extension does not exist; otherwise e = ac + ((a l + o) + b), each
 *        operation rounded on its own, the new node is the root and the new state nxt.  An extension with ac = -inf does
 *        not exist and is not looked up;
 *     4. stays add nothing and keep node and state, for the garbage as for any other class; candidates (by emission
 *        score alone), the order of entries, the tie rule and the -inf drop rule are the ASG search's;
 *     5. after the last frame (rule 5 of wfl_ctc_beam_search_lexicon) a rank whose node is not the root is dropped; with
 *        score_eos != 0 and an LM a remaining rank gets + a step(state, V + 1) and is dropped if that step is -inf; the
 *        remaining ranks are ranked again by score, descending, ties to the earlier rank; nbest is taken after that;
 *        nothing left: the empty sequence with score -inf;
 *     6. where nothing is pruned, score(l) = mass_ASG(l) + a LM(words(l)) + o #words + b #(classes of l other than the
 *        garbage), plus the </s> term; logz[b] is subtracted if logz is given;
 *     7. the labels are mapped on the way out as in wfl_asg_beam_search (drop, num_replabels).  The search and the
 *        n-best list are over raw sequences: a word spelled `a a` is found as raw `a, r0` only -- raw `a, garbage, a`
 *        unpacks to the same tokens but does not walk the trie, which holds the packed form the criterion trains on.
 *   The bound.  The kernel ranks only the entries at or above a lower bound of the W-th best entry, formed from one entry
 *   per hypothesis of a full beam: its stay, or -- where its last label is no candidate -- an extension of its own, which
 *   may serve only if it EXISTS (arc present, LM step finite): the garbage extension where the garbage is a candidate,
 *   else the first own extension, looked up; if that is absent the hypothesis contributes nothing and the frame's bound
 *   is -inf.  The lookup of a trie extension that cannot reach the bound even with the largest term (that of
 *   wfl_ctc_beam_search_lexicon) is skipped; garbage extensions have term 0.  The bound decides what is ranked, never
 *   the result.
 *   lex, word_lm: structs in HOST memory of DEVICE pointers, as for wfl_ctc_beam_search_lexicon; lex passed
 *   wfl_lexicon_check for (C, garbage) with a garbage class, for (C + 1, C) without one (a phantom blank that is never a
 *   label); word_lm passed wfl_ngram_lm_check for V + 1 and V.  The kernels trust them.  The same workspace
 *   (wfl_asg_beam_workspace), outputs, launches (three, four with a mapping) and guarantees as wfl_asg_beam_search: no
 *   allocation, no synchronisation, no global atomics, no cross-workgroup waits, every loop bounded by T, W, K, the
 *   back-off cap or 31 search steps.
 *   WFL_ERR_INVALID: what wfl_asg_beam_search refuses; garbage outside [-1, C); lex or one of its arrays NULL, num_nodes,
 *   num_arcs or num_words < 1 (or num_words = 2^31 - 1); a weight or bonus that is not finite; for a non-NULL word_lm
 *   what wfl_ctc_beam_search_lm refuses.  Not here: a token-level LM together with the lexicon (alone:
 *   wfl_asg_beam_search_lm), LM look-ahead inside words, several spellings of one word, out-of-vocabulary arcs, input
 *   lengths.
 * ------------------------------------------------------------------------------------------------ */
int wfl_asg_beam_search_lexicon(const float* x, const float* Wt /* [(C+1), C] */, const float* logz /* [B] or NULL */, int B,
                                int T, int C, int beam, int classes_per_frame, int nbest, int drop, int num_replabels,
                                int garbage /* -1: none */, const wfl_lexicon* lex, const wfl_ngram_lm* word_lm /* or NULL */,
                                double lm_weight, double word_bonus, double length_bonus, int score_eos, void* ws,
                                int32_t* out, int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */,
                                double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The ASG search with a token-level n-gram LM and a length bonus (csrc/beam_kernels.hip): the letter
 * criterion decoded lexicon-free with a letter n-gram.
 *   THE LM READS EXACTLY WHAT THE MAPPED WRITE LAUNCH EMITS: the raw class sequence with the garbage dropped and the
 *   replabels unpacked by wfl_decode_paths' rule.  R = `replabels`, G = `garbage` (-1: none), N = C - R - (G >= 0 ? 1 : 0)
 *   the number of tokens; replabel k is raw class k < R, token i is raw class i + R.  The LM is a wfl_ngram_lm over the N
 *   tokens: LM label i is token i, built for (num_classes = N + 1, blank = N) -- the phantom blank N is never a label --,
 *   LM label N + 1 is </s>.  Every rule of wfl_asg_beam_search stands; step, wfl_ngram_lm and wfl_ngram_lm_check are
 *   wfl_ctc_beam_search_lm's; a = lm_weight, b = length_bonus, both finite float64.  A hypothesis carries, beside its
 *   mass, an LM state (lm->start for the empty prefix) and rep: the token a replabel right behind the prefix would
 *   repeat, or -1 (the empty prefix: -1).  Both are functions of the raw prefix, so merging by prefix identity (rule 5 of
 *   the ASG search) stays exact, and a merged extension carries the same term as a new one.
 *     1. extension: hypothesis i with last label l (or the start), candidate c != l, ac = (s + Wt[1+c][l]) + p_i as in
 *        rule 4 of the ASG search.  ac = -inf: the extension does not exist and nothing is looked up.  Otherwise c emits
 *        a list of LM labels and moves rep: c == G emits nothing, state and rep stay; c >= R (and c != G) emits [c - R],
 *        rep' = c - R; c < R with rep >= 0 emits rep another c + 1 times, rep' = -1; c < R with rep = -1 (a replabel at
 *        the start or behind another replabel) emits nothing, rep' = -1 -- the write launch emits nothing for it either;
 *     2. term = 0; for each emitted label u in order: (lw, state) = step(state, u); lw = -inf: the extension does not
 *        exist; otherwise term = term + (a lw + b), each operation rounded on its own.  Then e = ac + term.  An extension
 *        that emits nothing has e = ac and costs no lookup; at most max(1, R) lookups per extension;
 *     3. stays add nothing and keep the LM state and rep.  Candidates (by emission score alone), entry order, the tie
 *        rule and the -inf drop rule are the ASG search's;
 *     4. after the last frame: with score_eos != 0 rank r gets + a step(state_r, N + 1) and is dropped if that step is
 *        -inf; one re-ranking by score, descending, ties to the earlier rank; nbest is taken after it; missing ranks are
 *        empty sequences with score -inf; logz[b] is subtracted if given, and nothing else;
 *     5. where nothing is pruned, score(l) = mass_ASG(l) + a LM(map(l)) + b |map(l)|, plus the </s> term; map is the
 *        write launch's mapping with (drop = G, num_replabels = R);
 *     6. the search and the n-best list stay over RAW sequences: two raw sequences with the same mapped output (a, G, a
 *        and a, r0) are separate hypotheses with the same LM term, as in wfl_asg_beam_search;
 *     7. the bound.  The ASG search bounds the W-th best entry by one entry per hypothesis of a full beam: its stay or,
 *        where its last label is no candidate, its first own extension.  Such an entry may serve only if it EXISTS: the
 *        stand-in extension is scored with its real term, lookups included, and where a step is -inf the hypothesis
 *        contributes nothing and the frame's bound is -inf.  The lookup of any other extension may be skipped when
 *        ac + bound is below that bound of the frame, `bound` the largest term an extension can have: the maximum over
 *        n = 0 .. max(1, R) of n accumulations of max(a step_min, a step_max) + b, formed on the host by the kernel's
 *        rounded operations.  The bound decides what is ranked, never the result.
 *   drop, num_replabels: the mapping of the results on the way out, as in wfl_asg_beam_search -- kept apart from garbage,
 *   replabels, so that raw results can be asked for under the same LM.  lm: a struct in HOST memory of DEVICE pointers to
 *   a pack that wfl_ngram_lm_check accepted for (N + 1, N), with the step_min / step_max it wrote; the kernels trust it.
 *   The workspace is wfl_asg_beam_workspace's; outputs, launches (three, four with a mapping) and guarantees as
 *   wfl_asg_beam_search: no allocation, no synchronisation, no atomics on global memory, no cross-workgroup waits, every
 *   loop bounded by T, W, K, R, the back-off cap or 31 search steps; deterministic.
 *   WFL_ERR_INVALID, in this order: what wfl_asg_beam_search refuses; garbage outside [-1, C); replabels < 0 or
 *   C - replabels - (garbage >= 0) < 1; what wfl_ctc_beam_search_lm refuses about the LM and the two scalars; then
 *   out_capacity too small.  Not here: merging raw hypotheses by mapped output, a token LM together with a lexicon, input
 *   lengths (ASG has none anywhere).
 * ------------------------------------------------------------------------------------------------ */
int wfl_asg_beam_search_lm(const float* x, const float* Wt /* [(C+1), C] */, const float* logz /* [B] or NULL */, int B, int T,
                           int C, int beam, int classes_per_frame, int nbest, int drop, int num_replabels,
                           int garbage /* -1: none */, int replabels, const wfl_ngram_lm* lm, double lm_weight,
                           double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                           int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: Transducer prefix beam search (csrc/beam_kernels.hip)
 *   wfl_dense_viterbi gives the best FRAME PATH of the Transducer criterion; the criterion scores a TOKEN SEQUENCE by the
 *   sum over all its alignments under a token graph with a blank and a frame-level transition model over tokens + blank.
 *   This search maximises that, on the launches of wfl_ctc_beam_search, for the two token graphs in which a frame path
 *   spells exactly one token sequence: the optional blank without repeats (CTC's topology, forced = 0) and the forced
 *   blank (forced = 1: every token is entered from the blank state, repeats itself, and returns to the blank; a path
 *   starts and ends in the blank).  The reference has no such decoder.
 *   Input, per utterance b over all T frames: x [B,T,C] float32; the blank class; optionally the transitions Wt
 *   [(C+1), C] float32 in the dense engine's layout (Wt[0][c] is start -> c, Wt[1+i][j] is j -> i) over the same C
 *   classes, the blank among them.  A NaN counts as -inf in x and Wt; +inf is not a weight.  W = beam in [1, 64],
 *   K = classes_per_frame in [1, min(C, 64)], nbest in [1, W], C <= 16384.  No input lengths: the Transducer has none.
 *   w(p, c) is the weight into class c behind frame label p: Wt[1+c][p], Wt[0][c] from the start, 0 if Wt is NULL.
 *     1. arithmetic (float64, lae), candidates (the K best EMISSION scores, ties to the lower class, the blank appended
 *        if it is not among them), prefix identity, merging, selection and tie order are wfl_ctc_beam_search's;
 *     2. a hypothesis is (prefix, pb, pnb): the log mass of its alignments whose last frame is the blank / is the
 *        prefix' last label l.  The search starts from the empty prefix with pb = 0, pnb = -inf; the state behind pb is
 *        the START in frame 0 (row 0 of Wt) and the blank from frame 1 on: call it beta;
 *     3. the stay entry of hypothesis i in frame t, s_c = (double)x[b,t,c]:
 *          pb'  = s_blank + lae(pb_i + w(beta, blank), pnb_i + w(l, blank)),
 *          pnb' = (s_l + pnb_i) + w(l, l) if l is a candidate, else -inf;
 *     4. the extension of i by a candidate c != blank:
 *          forced = 0, c != l:  e = s_c + lae(pb_i + w(beta, c), pnb_i + w(l, c)),
 *          forced = 0, c == l:  e = s_c + (pb_i + w(beta, c)),
 *          forced = 1:          e = s_c + (pb_i + w(beta, c)) for every c, and NO extension in frame 0;
 *        merged into the stay entry of the hypothesis with that prefix (pnb' = lae(pnb', e)) or a new entry
 *        (pb' = -inf, pnb' = e); entries are ranked by tot' = lae(pb', pnb') in both topologies;
 *     5. result, forced = 0: the first nbest ranks of the final beam with tot;
 *     6. result, forced = 1: a path ends in the blank, so only pb counts: ranks with pb = -inf are dropped, the rest are
 *        ranked by pb, descending, ties to the earlier rank; ranks beyond those are empty sequences with score -inf;
 *     7. normalize != 0: minus the normaliser -- with Wt (double)logz[b], logz [B] float32 on the device, the denominator
 *        wfl_dense_forward computes for x and Wt; without Wt the sum of the rows' log-sum-exps by wfl_ctc_beam_search's
 *        rule.  The normalised score of a sequence is then minus the criterion's loss of it where nothing was pruned, a
 *        lower bound otherwise.
 *   Wt == NULL and forced == 0 are wfl_ctc_beam_search's rules, and its search is what runs: bit-identical results.
 *   out (capacity B nbest T int32), out_offsets [B nbest + 1] int64, scores [B nbest] float64 as in wfl_ctc_beam_search
 *   (the blank is never a label of a result); plain stores in a fixed order, any device-accessible memory; deterministic.
 *   ws: device scratch of wfl_transducer_beam_workspace's size, 16-byte aligned.  Three launches on `stream` (candidates;
 *   beam: a workgroup per utterance, up to three gathers from Wt per stay and two per extension; write), no allocation,
 *   no synchronisation, no atomics on global memory, no cross-workgroup waits, every loop bounded by T, W, K.
 *   WFL_ERR_INVALID: a NULL required pointer (Wt and logz may be NULL), B, T or C < 1, blank outside [0, C), forced not
 *   0 or 1, beam outside [1, 64], classes_per_frame outside [1, min(C, 64)], nbest outside [1, beam], out_capacity too
 *   small, normalize != 0 with Wt but without logz, logz without Wt.  WFL_ERR_UNSUPPORTED: C > 16384.
 *   Not here: the ambiguous token graphs (no blank; the optional blank with repeats), input lengths.  A token-level LM:
 *   wfl_transducer_beam_search_lm; a lexicon: wfl_transducer_beam_search_lexicon.
 * ------------------------------------------------------------------------------------------------ */
/* out_capacity = B nbest T (int32 elements of `out`), ws_bytes = the device scratch of a call */
int wfl_transducer_beam_workspace(int B, int T, int C, int beam, int classes_per_frame, int nbest, int64_t* out_capacity,
                                  int64_t* ws_bytes);
int wfl_transducer_beam_search(const float* x, const float* Wt /* [(C+1), C] or NULL */, const float* logz /* [B] or NULL */,
                               int B, int T, int C, int blank, int forced, int beam, int classes_per_frame, int nbest,
                               int normalize, void* ws, int32_t* out, int64_t out_capacity,
                               int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: Transducer prefix beam search, hypotheses merged by spelling (csrc/beam_kernels.hip)
 *   With word pieces the criterion's targets are GRAPHEME sequences and its loss sums over every alignment of every
 *   decomposition of the graphemes into tokens.  wfl_transducer_beam_search stops at the token sequence: two sequences
 *   that spell the same graphemes compete.  This search identifies a hypothesis by what it spells and sums the mass of
 *   the decompositions inside the beam launch.  The rules extend those above and keep their symbols.
 *   Additional input, the spelling table over the C classes: spell_ptr int32 [C+1], spell_sym int32 [spell_ptr[C]];
 *   class c spells the graphemes spell_sym[spell_ptr[c] .. spell_ptr[c+1]); the blank's range is empty, every other
 *   class has 1 .. WFL_SPELL_MAX graphemes, each >= 0.
 *     1. arithmetic, candidates, stay entries (rule 3), the mass of an extension (rule 4), the frame-0 start row, the
 *        forced topology's "no extension in frame 0", selection and tie order are unchanged, per hypothesis;
 *     2. a hypothesis is (S, l, pb, pnb, rho): S the grapheme sequence spelt so far, l the last token, rho a
 *        REPRESENTATIVE token sequence with spelling S and last token l.  Its identity is the pair (S, l) -- what its
 *        future depends on: the stay, "c = l extends from pb only" and every w(l, .) need l, the blank-side state is the
 *        blank whatever l was.  The search starts from ((), none) with pb = 0, pnb = -inf;
 *     3. the extension of hypothesis i by a candidate c != blank has the key (S_i ++ spell(c), c).  All extensions of a
 *        frame with the same key are ONE entry (their parents share S and differ in l); their masses are added with lae
 *        in the order of the parents' ranks.  If the key is the identity of a beam hypothesis j (then l_j = c is a
 *        candidate and j has a stay) the sum goes into j's pnb' by lae, behind j's own stay term, and j keeps rho_j.
 *        Otherwise the sum is a new entry: its place in the tie order is (rank of its lowest-ranked parent, candidate
 *        position), whether or not that parent's own contribution is finite; rho = rho_p ++ c, p the lowest-ranked
 *        parent whose contribution is finite; an entry at -inf is dropped, as always;
 *     4. result: each hypothesis of the final beam scores lae(pb, pnb) (forced = 0) or pb (forced = 1; -inf dropped);
 *        hypotheses with the same S are merged -- scores added with lae in rank order, at the place and with the rho of
 *        the best-ranked member with a finite score --, the merged ones ranked by score descending, ties to the earlier
 *        place; the first nbest are returned as rho (token indices, never the blank) with their score, minus the
 *        normaliser of rule 7 above if normalize != 0.  No two ranks spell the same graphemes; ranks beyond the result
 *        are empty with score -inf;
 *     5. the beam is ranked per (S, l), not per S: a stated pruning choice.
 *   A score is the mass, kept by the beam, of all alignments of all decompositions of S, minus the normaliser: minus the
 *   criterion's loss of target S where nothing is pruned, a lower bound of it otherwise.  Where every token is a single
 *   grapheme and the graphemes are distinct, (S, l) and the token sequence determine each other and the results are
 *   those of wfl_transducer_beam_search's rules (lae is applied in the same order).
 *   wfl_spelling_check (HOST arrays, once per table): WFL_ERR_INVALID for a NULL pointer, C < 1, blank outside [0, C),
 *   spell_ptr[0] != 0, descending pointers, a blank that spells something, another class with no grapheme or more than
 *   WFL_SPELL_MAX, a negative grapheme; the message names the first offence.
 *   wfl_transducer_beam_search_merged: wfl_transducer_beam_search's arguments with the table's two DEVICE pointers behind
 *   logz; the workspace is wfl_transducer_beam_workspace's; the same refusals in the same order, a NULL table refused
 *   behind `forced`; the same three launches -- always with the merging beam kernel, also for Wt == NULL, forced == 0 --,
 *   the beam launch reading the table from global memory; every loop bounded by T, W, K, WFL_SPELL_MAX.
 *   Not here: a lexicon, an LM, input lengths, graphemes in the place of tokens as the result.
 * ------------------------------------------------------------------------------------------------ */
#define WFL_SPELL_MAX 64
int wfl_spelling_check(const int32_t* spell_ptr /* [C+1] */, const int32_t* spell_sym /* [spell_ptr[C]] */, int C, int blank);
int wfl_transducer_beam_search_merged(const float* x, const float* Wt /* [(C+1), C] or NULL */,
                                      const float* logz /* [B] or NULL */, const int32_t* spell_ptr, const int32_t* spell_sym,
                                      int B, int T, int C, int blank, int forced, int beam, int classes_per_frame, int nbest,
                                      int normalize, void* ws, int32_t* out, int64_t out_capacity,
                                      int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The Transducer search with a lexicon and an optional word-level n-gram LM (csrc/beam_kernels.hip).
 *   Every rule of wfl_transducer_beam_search stands: candidates, the two masses pb / pnb, the blank-side state, prefix
 *   identity, merging, selection and tie order.  a = lm_weight, o = word_bonus, b = length_bonus, all finite float64 (the
 *   names of wfl_ctc_beam_search_lexicon).  The lexicon is a wfl_lexicon over TOKEN sequences for (C, blank).
 *     1. every hypothesis carries a trie node and, with a word LM, an LM state; the empty prefix has the root and the
 *        LM's `start`.  Both are functions of the token prefix, so merging by prefix identity stays exact, and a merged
 *        extension carries the same term as a new one;
 *     2. the extension of hypothesis i by a candidate c != blank, ac the value of rule 4 of wfl_transducer_beam_search
 *        (forced = 0: both masses, pb alone for c == l; forced = 1: pb alone, and no extension in frame 0).  ac = -inf:
 *        the extension does not exist and nothing is looked up.  Otherwise c is searched among the arcs of node_i (a
 *        binary search, at most 31 steps).  Absent: the extension does not exist.  An inner arc: e = ac + b, the node
 *        becomes the arc's target, the state stays.  An arc that completes word v: (l, nxt) = step(state_i, v), (0, -)
 *        without an LM; l = -inf: the extension does not exist; otherwise e = ac + ((a l + o) + b), each operation
 *        rounded on its own, the new node is the root and the new state nxt;
 *     3. stays are rule 3 of wfl_transducer_beam_search: they add no term and keep node and state; the merged extension
 *        inside a stay carries rule 2's term;
 *     4. the bound is wfl_ctc_beam_search's: the blank gives every hypothesis a stay, so the W-th best stay of a full
 *        beam bounds the W-th best entry from below.  The lookup of an extension with ac + (the largest term, that of
 *        wfl_ctc_beam_search_lexicon) below the bound is skipped.  The bound decides what is ranked, never the result;
 *     5. after the last frame, in this order: a rank whose node is not the root is dropped; forced = 1: the score is pb,
 *        a rank with pb = -inf is dropped; forced = 0: the score is lae(pb, pnb); with score_eos != 0 and an LM a
 *        remaining rank gets + a step(state, V + 1) and is dropped if that step is -inf; the remaining ranks are ranked
 *        again by score, descending, ties to the earlier rank; nbest is taken after that; nothing left: the empty
 *        sequence with score -inf;
 *     6. where nothing is pruned, score(l) = mass_Transducer(l) + a LM(words(l)) + o #words + b |l|, plus the </s> term;
 *        mass_Transducer(l) is the log-sum over l's alignments under the token graph and Wt; normalize != 0: minus the
 *        normaliser of rule 7 of wfl_transducer_beam_search (logz[b] with Wt, the rows' log-sum-exps without);
 *     7. Wt == NULL and forced == 0 are wfl_ctc_beam_search_lexicon's rules without lengths, and its search is what
 *        runs: bit-identical results.
 *   lex, word_lm: structs in HOST memory of DEVICE pointers, as for wfl_ctc_beam_search_lexicon; lex passed
 *   wfl_lexicon_check for (C, blank), word_lm wfl_ngram_lm_check for V + 1 and V.  The kernels trust them.  The workspace
 *   (wfl_transducer_beam_workspace), outputs, three launches and guarantees of wfl_transducer_beam_search: no allocation,
 *   no synchronisation, no global atomics, no cross-workgroup waits, every loop bounded by T, W, K, the back-off cap or
 *   31 search steps.
 *   WFL_ERR_INVALID: what wfl_transducer_beam_search refuses, in its order; then lex or one of its arrays NULL,
 *   num_nodes, num_arcs or num_words < 1 (or num_words = 2^31 - 1); for a non-NULL word_lm what wfl_ctc_beam_search_lm
 *   refuses; a weight or bonus that is not finite.  Not here: a token-level LM, merging by spelling, input lengths, the
 *   ambiguous token graphs (LM look-ahead inside words: wfl_transducer_beam_search_lexicon_lookahead below).  Several
 *   spellings of one word and vocabularies that are not prefix-free: wfl_transducer_beam_search_lexicon_marked.
 * ------------------------------------------------------------------------------------------------ */
int wfl_transducer_beam_search_lexicon(const float* x, const float* Wt /* [(C+1), C] or NULL */,
                                       const float* logz /* [B] or NULL */, int B, int T, int C, int blank, int forced, int beam,
                                       int classes_per_frame, int nbest, int normalize, const wfl_lexicon* lex,
                                       const wfl_ngram_lm* word_lm /* or NULL */, double lm_weight, double word_bonus,
                                       double length_bonus, int score_eos, void* ws, int32_t* out, int64_t out_capacity,
                                       int64_t* out_offsets /* [B*nbest+1] */, double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The Transducer search with a token-level n-gram LM and a length bonus (csrc/beam_kernels.hip):
 * shallow fusion with an LM over the tokens themselves -- no vocabulary, and words that no lexicon lists.
 *   Every rule of wfl_transducer_beam_search (rules 1-7) stands.  The LM form, step(s, c), wfl_ngram_lm and
 *   wfl_ngram_lm_check are those of wfl_ctc_beam_search_lm: labels are the classes 0 .. C-1, never the blank (which is
 *   one of the C classes), and label C stands for </s>.  a = lm_weight, b = length_bonus, both finite float64.
 *     1. every hypothesis carries an LM state, the empty prefix has lm->start;
 *     2. a stay entry (rule 3) adds nothing and keeps its state;
 *     3. the extension of hypothesis i by a candidate c != blank (rule 4, both topologies), m the mass term rule 4 gives
 *        for the topology (forced = 0: lae of both masses, pb alone for c == l; forced = 1: pb alone, and no extension
 *        in frame 0): s_c + m = -inf: the extension does not exist and nothing is looked up.  Otherwise
 *        (l, nxt) = step(state_i, c); l = -inf: the extension does not exist; otherwise e = (s_c + m) + (a l + b), each
 *        operation rounded on its own, and the entry gets the state nxt.  A merged extension carries the same term as a
 *        new one (state and LM score are functions of the prefix), so unpruned tot(l) = mass(l) + a LM(l) + b |l|;
 *     4. the kernel may skip the lookup of an extension that cannot reach the W-th best stay entry even with the largest
 *        possible term, max(a step_min, a step_max) + b.  The bound decides what is ranked, never the result;
 *     5. after the last frame: q_r = tot_r for forced = 0; for forced = 1 q_r = pb_r, and the ranks with pb_r = -inf are
 *        dropped first (rule 6).  With score_eos != 0 the score is q_r + a step(state_r, C) and a rank whose step is -inf
 *        is dropped; without it the score is q_r.  One re-ranking by that score, descending, ties to the earlier rank;
 *        nbest is taken after it; missing ranks are empty sequences with score -inf;
 *     6. normalize subtracts what rule 7 subtracts and nothing else;
 *     7. Wt == NULL and forced == 0 are wfl_ctc_beam_search_lm's rules without lengths, and its search is what runs:
 *        bit-identical results;
 *     8. candidates, prefix identity, entry order, the tie rule and the -inf drop rule do not change.
 *   lm: a struct in HOST memory of DEVICE pointers to a pack that wfl_ngram_lm_check accepted for (C, blank), with the
 *   step_min / step_max it wrote; the kernels trust it.  The workspace is wfl_transducer_beam_workspace's; outputs as in
 *   wfl_transducer_beam_search.  Three launches, no allocation, no synchronisation, no atomics on global memory, no
 *   cross-workgroup waits, every loop bounded by T, W, K, the back-off cap or 31 search steps; deterministic.
 *   WFL_ERR_INVALID: what wfl_transducer_beam_search refuses, in its order; then what wfl_ctc_beam_search_lm refuses
 *   about the LM (lm or one of its arrays NULL, num_states < 1, num_arcs < 0, start outside [0, num_states), step_min
 *   or step_max NaN) and a weight or bonus that is not finite.  Not here: a token-level LM together with a lexicon or
 *   with merging by spelling, input lengths, the ambiguous token graphs.  ASG with a letter LM: wfl_asg_beam_search_lm.
 * ------------------------------------------------------------------------------------------------ */
int wfl_transducer_beam_search_lm(const float* x, const float* Wt /* [(C+1), C] or NULL */, const float* logz /* [B] or NULL */,
                                  int B, int T, int C, int blank, int forced, int beam, int classes_per_frame, int nbest,
                                  int normalize, const wfl_ngram_lm* lm, double lm_weight, double length_bonus, int score_eos,
                                  void* ws, int32_t* out, int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */,
                                  double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The four lexicon searches of CTC and the Transducer with word-LM LOOK-AHEAD inside words (csrc/beam_kernels.hip; DESIGN
 * section 27).  Without it a hypothesis is ranked with no LM information about the word it is spelling: the word's term
 * arrives with its last label (one label later still with a start-marked lexicon), and a narrow beam loses the word the
 * LM wants before the LM has had a say.  Unigram max look-ahead ("smearing"): every word v has a score u[v] (finite,
 * natural log; by default the word LM's unigram score) and every trie node n the best of them below it,
 *     L[0] = 0 at the root; otherwise L[n] = max u[v] over the words that can still be completed from n -- end-marked: the
 *     completing arcs in the subtree of n; start-marked: the terminal nodes in the subtree, n included.
 * A hypothesis at node n has paid a L[n] provisionally; the payment moves down the trie with it and is settled where the
 * word ends.  Every rule of the sibling entry stands unless replaced here; a = lm_weight, o = word_bonus, b = length_bonus,
 * every operation rounded on its own (no fused multiply-add), by the same functions on the host and on the device:
 *     1. an inner arc n -> m: the term is (a (L[m] - L[n])) + b, in place of b.  A start-marked word's first label from the
 *        root is such an arc, with L[root] = 0;
 *     2. an arc that completes a word at node n (end-marked), (l, nxt) = step(state, v): l = -inf: the extension does not
 *        exist, as before; otherwise the term is (a (l - L[n]) + o) + b;
 *     3. start-marked, a word-starting class c from a terminal node n: rule 2's term, + a L[start_node[c]];
 *     4. after the last frame -- end-marked: unchanged, a rank inside a word is dropped with what it has paid;
 *        start-marked: the pending word at a terminal node n gets (a (l - L[n]) + o), every other non-root rank is
 *        dropped.  The </s> term, the re-ranking, nbest, T_b = 0 and the normalisation are unchanged;
 *     5. the mass of a hypothesis at node n includes a L[n], a function of the prefix because the node is: merging by
 *        prefix stays exact, stays add nothing.  Along a word the payments telescope, so unpruned the total of a sequence
 *        of whole words is the sibling's up to rounding (the sums are associated differently), and the set of sequences
 *        is the sibling's.  With every u[v] = 0, or with a = 0, every term is the sibling's bit for bit;
 *     6. the prune bound is still a proof.  wfl_lexicon_lookahead_check records [arc_min, arc_max], the range of
 *        L[m] - L[n] over the inner arcs (the rounded differences the kernel forms; a start-marked root arc counts
 *        L[m] - 0), [end_min, end_max], the range of L[n] over the nodes where a word can complete (end-marked: a node
 *        with a completing arc; start-marked: a terminal node), and [start_min, start_max], the range of L over the
 *        root's children (start-marked; [0, 0] end-marked).  Per call the largest term of an extension is
 *        max( max(a arc_min, a arc_max) + b,
 *             ((max(a (step_min - end_max), a (step_max - end_min)) + o) + b) + max(a start_min, a start_max) ),
 *        by the monotonicity of each rounded operation (DESIGN section 27 has the argument); a NaN on the way (0 inf,
 *        inf - inf): no bound, every extension is looked up.
 *   look: a struct in HOST memory; for the searches node_look is a DEVICE pointer to the array that
 *   wfl_lexicon_lookahead_check (or wfl_lexicon_marked_lookahead_check) accepted with a host pointer, for the same
 *   lexicon, and the six scalars are what that check wrote.  The kernels trust it: they check no index.  word_lm is
 *   required (look-ahead of no LM is nothing).  One or two 8-byte loads per looked-up extension; no workspace of its own:
 *   the sibling's workspace function, outputs, three launches and guarantees -- no allocation, no synchronisation, no
 *   global atomics, no cross-workgroup waits, every loop bounded.  The Transducer entries with Wt == NULL and forced == 0
 *   run the CTC entries' search: bit-identical results.
 *   WFL_ERR_INVALID: what the sibling entry refuses, in its order; then look or look->node_look NULL, one of the six
 *   scalars NaN or a range with min > max, word_lm NULL.
 *   Not here: ASG, look-ahead that depends on the LM state, log-add smearing, a token-level LM together with a lexicon,
 *   out-of-vocabulary arcs, back-off transition graphs, input lengths for the Transducer.
 * ------------------------------------------------------------------------------------------------ */
typedef struct wfl_lexicon_lookahead {
  const double* node_look; /* [num_nodes] of the lexicon: finite, node_look[0] = 0 */
  double arc_min, arc_max;     /* written by the check: node_look[m] - node_look[n] over the inner arcs n -> m lies between */
  double end_min, end_max;     /* written by the check: node_look[n] over the nodes where a word can complete */
  double start_min, start_max; /* written by the check: node_look over the root's children (start-marked), else 0, 0 */
} wfl_lexicon_lookahead;
/* The look-ahead's check (host arrays, no device) for a lexicon that wfl_lexicon_check accepted: lex and look and their
 * arrays not NULL, the lexicon's sizes >= 1 and its arc_ptr / arc_next inside their arrays (read before node_look is
 * indexed by them); every node_look[n] finite; node_look[0] == 0.  WFL_ERR_INVALID names the first offence in
 * wfl_last_error().  On success it WRITES the six scalars of rule 6; whatever they held before is not read.  It does not
 * ask that node_look is the maximum of any word scores: the totals telescope for every finite array (rule 5). */
int wfl_lexicon_lookahead_check(const wfl_lexicon* lex, wfl_lexicon_lookahead* look);
/* The same for a start-marked lexicon that wfl_lexicon_marked_check accepted (node_word is read, start_node is not). */
int wfl_lexicon_marked_lookahead_check(const wfl_lexicon_marked* lex, wfl_lexicon_lookahead* look);
int wfl_ctc_beam_search_lexicon_lookahead(const float* x, const int32_t* lengths /* or NULL */, int B, int T, int C, int blank,
                                          int beam, int classes_per_frame, int nbest, int normalize, const wfl_lexicon* lex,
                                          const wfl_lexicon_lookahead* look, const wfl_ngram_lm* word_lm, double lm_weight,
                                          double word_bonus, double length_bonus, int score_eos, void* ws, int32_t* out,
                                          int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */,
                                          double* scores /* [B*nbest] */, void* stream);
int wfl_ctc_beam_search_lexicon_marked_lookahead(const float* x, const int32_t* lengths /* or NULL */, int B, int T, int C,
                                                 int blank, int beam, int classes_per_frame, int nbest, int normalize,
                                                 const wfl_lexicon_marked* lex, const wfl_lexicon_lookahead* look,
                                                 const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus,
                                                 double length_bonus, int score_eos, void* ws, int32_t* out,
                                                 int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */,
                                                 double* scores /* [B*nbest] */, void* stream);
int wfl_transducer_beam_search_lexicon_lookahead(const float* x, const float* Wt /* [(C+1), C] or NULL */,
                                                 const float* logz /* [B] or NULL */, int B, int T, int C, int blank, int forced,
                                                 int beam, int classes_per_frame, int nbest, int normalize,
                                                 const wfl_lexicon* lex, const wfl_lexicon_lookahead* look,
                                                 const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus,
                                                 double length_bonus, int score_eos, void* ws, int32_t* out,
                                                 int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */,
                                                 double* scores /* [B*nbest] */, void* stream);
int wfl_transducer_beam_search_lexicon_marked_lookahead(const float* x, const float* Wt /* [(C+1), C] or NULL */,
                                                        const float* logz /* [B] or NULL */, int B, int T, int C, int blank,
                                                        int forced, int beam, int classes_per_frame, int nbest, int normalize,
                                                        const wfl_lexicon_marked* lex, const wfl_lexicon_lookahead* look,
                                                        const wfl_ngram_lm* word_lm, double lm_weight, double word_bonus,
                                                        double length_bonus, int score_eos, void* ws, int32_t* out,
                                                        int64_t out_capacity, int64_t* out_offsets /* [B*nbest+1] */,
                                                        double* scores /* [B*nbest] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: token and word error counts behind a best path (csrc/error_kernels.hip)
 *   what the training loop does with viterbi()'s result -- compute_edit_distance, train.py:74-87, called per batch at
 *   train.py:278-284 and test.py:94-109 -- per utterance b:
 *     1. s_hyp = the labels hyp[hyp_off[b] .. hyp_off[b+1]) with each label replaced by its expansion, s_ref the same
 *        over ref.  Each side has its own optional table (exp_ptr int32 [V+1], exp_sym int32 [exp_ptr[V]]): label v
 *        stands for the symbols exp_sym[exp_ptr[v] .. exp_ptr[v+1]), possibly none (tokens_to_text for word pieces,
 *        to_text for graphemes, train.py:80).  NULL tables: a label is its own symbol.  A label outside [0, V)
 *        expands to nothing.
 *     2. sep >= 0: leading and trailing `sep` symbols are removed from both strings (str.strip(wordsep)).
 *     3. counts[b][0] = the Levenshtein distance of the two strings (unit costs), counts[b][1] = |s_ref|.
 *     4. sep >= 0: the words of a string are its maximal runs of symbols other than `sep` (no empty words:
 *        filter(None, split(wordsep)), train.py:81-82); counts[b][2] = the Levenshtein distance of the two word
 *        sequences -- two words are equal iff they are the same symbols in the same order, compared exactly --,
 *        counts[b][3] = the number of reference words.  sep < 0: both 0.
 *   hyp / hyp_off are what wfl_decode_emissions / wfl_decode_paths left (hyp_capacity: their out_capacity; the lengths
 *   are known only on the device, the kernels read the offsets themselves), ref / ref_off the targets of the batch
 *   (int64 offsets [B+1], int32 labels, ref_labels of them).  Every index read from device memory is clamped to its
 *   buffer.  counts [B][4] int32 is written by plain stores of a kernel: any device-accessible memory, pinned host
 *   memory included.  ws: device scratch of wfl_errors_workspace's size, 16-byte aligned, contents irrelevant before
 *   and after.  Three launches on `stream`, no allocation, no synchronisation, no atomics.
 *   WFL_ERR_INVALID: B < 1, a NULL required pointer, a negative capacity, a table pointer without its partner, V < 1
 *   with a table, a negative max_expansion.  Any string length is served, 0 on either or both sides included.
 * ------------------------------------------------------------------------------------------------ */
/* ws_bytes = the device scratch of a wfl_errors_count call (compute_edit_distance, train.py:74-87, test.py:94-109) whose tables' longest expansions are
 * hyp_max_expansion / ref_max_expansion symbols (1 without a table): derived from the capacities and these maxima, never
 * from data on the device.  WFL_ERR_UNSUPPORTED: a side's capacity x max_expansion beyond 2^30 - 1 symbols. */
int wfl_errors_workspace(int B, int64_t hyp_capacity, int64_t ref_labels, int hyp_max_expansion, int ref_max_expansion,
                         int64_t* ws_bytes);
/* counts[b] = {token distance, reference tokens, word distance, reference words} of utterance b: compute_edit_distance
 * (train.py:74-87; test.py:94-109) for the whole batch */
int wfl_errors_count(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref, const int64_t* ref_off, int B,
                     const int32_t* hyp_exp_ptr, const int32_t* hyp_exp_sym, int hyp_V, const int32_t* ref_exp_ptr,
                     const int32_t* ref_exp_sym, int ref_V, int sep, int64_t hyp_capacity, int64_t ref_labels, void* ws,
                     int32_t* counts /* [B][4] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device kernels: per-utterance input lengths of a padded CTC batch (csrc/pad_kernels.hip)
 *   For the CTC label graph (ctc.py:15-29) a frame whose emissions are 0 for the blank and -inf for every other class
 *   is the identity: from the accepting states only the blank arc into / on the last blank is finite, so the T-frame
 *   score of x with such frames at t >= T_b is the T_b-frame score of x[:T_b], the posteriors of the frames < T_b are
 *   unchanged, those of the pad frames sit on the blank, and an utterance that cannot be aligned in T_b frames keeps
 *   Z = 0.  The constants do not depend on x: the gradient of the pad rows is 0.  The criterion (criterions/ctc.py,
 *   `input_lengths`) runs the launches that do not read lengths themselves (wfl_ctc_call.input_lengths does, for targets
 *   of up to 63 labels) on the padded copy, and zeroes the pad rows behind every gradient.  lengths: int32 [B] on the device,
 *   1 <= lengths[b] <= T is the caller's to check (any value only moves the comparison, nothing is indexed with it).
 *   One launch each on `stream`, no allocation, no synchronisation.  WFL_ERR_INVALID: a NULL pointer, B, T or C < 1,
 *   blank outside [0, C), out == x.
 * ------------------------------------------------------------------------------------------------ */
/* out [B,T,C] = x [B,T,C] with every row t >= lengths[b] replaced by {0 at blank, -inf elsewhere} */
int wfl_ctc_pad_frames(const float* x, const int32_t* lengths, int B, int T, int C, int blank, float* out, void* stream);
/* dx[b, t, :] = 0 for t >= lengths[b]; the rows before are not touched.  Runs behind every CTC gradient taken with
 * lengths, before the gradient is handed out. */
int wfl_zero_pad_rows(float* dx, const int32_t* lengths, int B, int T, int C, void* stream);

/* small device utilities used by the Python layer (kept here so the product never needs a
 * torch op inside the timed path) */
/* dst[0..nbytes) (device) = src_pinned[0..nbytes) (PINNED host memory, e.g. hipHostMalloc / a pin_memory tensor), by
 * a kernel that reads the host buffer through its device-visible address; both 16-byte aligned.  For the small
 * per-batch uploads of the criteria (targets, packed lattices): unlike hipMemcpyAsync, which on this stack sometimes
 * blocks the calling thread until the stream has drained (measured: 7 us .. 5 ms for 23 KB behind queued kernels),
 * a launch is always asynchronous.  The host buffer must stay untouched until the stream has passed the launch. */
int wfl_upload(void* dst, const void* src_pinned, int64_t nbytes, void* stream);
/* v[0..n) *= s[0] on the device; a no-op pass when s[0] == 1 (upstream gradient of a scalar loss) */
int wfl_scale(float* v, int64_t n, const float* s, void* stream);
/* out[0] = (1/B) * sum_b sign * scale[b] * (vals[b] - minus[b])  (+ out[0] if accumulate); minus may be NULL (0).
 * With `minus` the two-term criteria (ASG: denominator - numerator, asg.py:116-121; Transducer) reduce in one launch. */
int wfl_reduce_loss(const float* vals, const float* minus, const float* scale, int B, float sign,
                    int accumulate, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WFL_H_ */
