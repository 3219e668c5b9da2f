"""ConvTransduce1D and the STC augmentation at the limits their kernels are built around (-m gpu): csrc/conv_kernels.hip.

  conv_forward_kernel / conv_grad_kernel   a row of 16 lanes per dynamic program (lane i owns states 2i, 2i+1), register
      histories of 16 frames, Viterbi codes packed 2 bits per frame into one int, the lexicon walked 16 entries per pass with
      a clamped tail, the opt-in launch above 48 KB of dynamic LDS: entries of 0..15 sub-tokens, kernel sizes 1, 15 and 16,
      K around 16 and 32, every stride case, -inf / NaN emissions and a -inf arc weight -- against the float64 graph oracle
      (oracle/criteria.py::conv_transduce_1d_grad), at the tolerance of tests/test_gpu_configs.py
  Viterbi on exactly tying scores   the kernel's path is read bit by bit from the gradients and checked to be A best path of
      the kernel graph ("Viterbi ties": the oracle's tie rule differs, so paths are not compared with its own)
  host-side validation   sub-tokens / blank outside the input's classes, the backward's LDS limit known before the forward
  stc_augment_kernel / stc_augment_grad_kernel   more selected classes than one wave, a single row, fewer classes than a
      wave -- against a float64 torch autograd of the torch spelling (criterions/stc.py, the host-input branch of
      STC.forward)

The worst ratios land in the parity_r06.json that tests/test_gpu_configs.py writes, beside those of the at-size tests.
Nothing here reads the reference project."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import criteria as OC  # noqa: E402
# _gpu_and_stats: the module-level fixture of test_gpu_configs, registered for this module too by the import -- skips
# without a GPU, and writes STATS (shared, so with every module's records so far) when this module's tests are over:
# this module runs after test_gpu_configs, whose own write would miss the records made here
from test_gpu_configs import _gpu_and_stats, check  # noqa: E402,F401

NEG = float("-inf")


# =================================================================================================
# A. log and tropical sweeps against the oracle
# =================================================================================================
def _table(lexicon, blank, bo, spike):
    from gtn_applications_amd.criterions import transducer as tr

    tab = tr._KernelTable(lexicon, bo, spike)
    tab.blank_idx = blank
    return tab


def _min_frames(entry, bo):
    """The shortest window entry can align in: a blank between repeats, and without the optional blank one after every
    sub-token (the first one may start the window: make_kernel_graph has the arc 0 -> 1)."""
    if not entry:
        return 1
    return len(entry) + sum(a == b for a, b in zip(entry[:-1], entry[1:])) if bo else 2 * len(entry)


def _arc_slices(lexicon, blank, bo, spike):
    n, res = 0, []
    for l in lexicon:
        na = OC.make_kernel_graph(l, blank, bo, spike).num_arcs()
        res.append(slice(n, n + na))
        n += na
    return res


# Seeds of the random cases, by case id (1 where none is named): the first at which the oracle's own result meets
# _conv_reference's conditions (found on the host, by the oracle alone -- no kernel result enters the choice).
SEEDS = {"ks1_log": 4, "ks1_trop": 4, "len_bo0_sp0_trop": 2, "len_bo0_sp1_trop": 3, "len_bo1_sp1_log": 3,
         "stride3_T18_log": 2, "stride3_T18_trop": 2}


def _conv_reference(case, lexicon, C, blank, ks, stride, B, T, bo, spike, viterbi, neg_param_entry, seed=None):
    """Inputs of one configuration and the oracle's result for them: random emissions with one -inf and one NaN in single
    elements of token columns (the kernels read NaN as -inf: nan_to_neg -- the oracle is fed -inf there), random kernel
    parameters with one -inf (the blank self-loop on state 0 of one entry), a random upstream gradient."""
    rs = np.random.RandomState(SEEDS.get(case, 1) if seed is None else seed)
    K = len(lexicon)
    x = rs.randn(B, T, C).astype(np.float32)
    starts = list(range(0, T - ks + 1, stride))
    tokens = sorted(set(c for l in lexicon for c in l if c != blank))
    t0, t1 = starts[0] + min(1, ks - 1), starts[-1] + ks - 1
    x[0, t0, tokens[0]] = NEG
    x[B - 1, t1, tokens[-1]] = np.nan
    x_ref = x.astype(np.float64)
    x_ref[B - 1, t1, tokens[-1]] = NEG
    tab = _table(lexicon, blank, bo, spike)
    params = (0.5 * rs.randn(tab.num_arcs)).astype(np.float32)
    if neg_param_entry is not None:
        params[tab.table[neg_param_entry, 34]] = NEG
    delta = rs.randn(B, len(starts), K).astype(np.float32)
    want = OC.conv_transduce_1d_grad(x_ref, lexicon, blank, ks, stride, delta.astype(np.float64), bo, spike,
                                     params.astype(np.float64), viterbi)
    # The case does not hide behind -inf: most outputs are finite and every entry that can align does so somewhere.  No
    # finite score is close to zero either: outputs are held to 1e-4 RELATIVE, and an fp32 sum of up to 16 emissions and
    # arc weights whose partial sums reach 16 carries some 1e-6 per addition (half an ulp of 16), so below 0.05 the bound
    # would ask for more than the number format has.
    fin = np.isfinite(want[0])
    assert fin.mean() >= 0.6, (case, fin.mean())
    for k, l in enumerate(lexicon):
        assert fin[:, :, k].any() == (_min_frames(l, bo) <= ks), (case, k, l)
    assert np.abs(want[0][fin]).min() >= 0.05, (case, np.abs(want[0][fin]).min())
    assert np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    return x, tab, params, delta, starts, want


def _conv_case(stat, case, lexicon, C, blank, ks, stride, B, T, bo, spike, viterbi, neg_param_entry):
    """One configuration through ConvTransduce1DFunction (the module's odd-kernel assertion is not in the way) against the
    oracle: outputs (-inf exactly where the oracle has it, relative elsewhere), dx and dparams at 2e-5 of the |delta| mass
    that reaches the element, exact zeros where nothing reaches.  Returns the kernels' outputs."""
    from gtn_applications_amd.criterions import transducer as tr

    x, tab, params, delta, starts, (want_out, want_dx, want_dp) = _conv_reference(
        case, lexicon, C, blank, ks, stride, B, T, bo, spike, viterbi, neg_param_entry)
    K, Tout, name = len(lexicon), len(starts), stat
    fin = np.isfinite(want_out)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    pd = torch.from_numpy(params).cuda().requires_grad_(True)
    out = tr.ConvTransduce1DFunction.apply(xd, tab, ks, stride, pd, viterbi)
    assert tuple(out.shape) == (B, Tout, K)
    out.backward(torch.from_numpy(delta).cuda())
    got_out, got_dx, got_dp = out.detach().cpu().numpy(), xd.grad.cpu().numpy(), pd.grad.cpu().numpy()

    assert ((got_out == NEG) == ~fin).all(), name
    check(name + "_out", got_out[fin], want_out[fin], 0.0)
    # |delta| mass per frame: the windows that touch it, all their entries
    mass = np.zeros((B, T))
    for w, t in enumerate(starts):
        mass[:, t:t + ks] += np.abs(delta[:, w]).sum(axis=1)[:, None]
    check(name + "_dx", got_dx, want_dx, float(mass.max()))
    assert (got_dx[mass == 0] == 0).all(), name  # frames between / behind the windows
    assert (got_dx[want_dx == 0] == 0).all(), name  # classes no entry names, entries that cannot align
    check(name + "_dparams", got_dp, want_dp, float(np.abs(delta).sum(axis=(0, 1)).max()))
    for k, sl in enumerate(_arc_slices(lexicon, blank, bo, spike)):
        if not fin[:, :, k].any():
            assert (got_dp[sl] == 0).all(), (name, k)
    return got_out


def _lengths_lexicon(ks, blank):
    """Entries of 0, 1, 2, 3, 7, 14 and 15 sub-tokens, repeats that fill the kernel exactly (size_with_rep == ks), the
    blank as an entry's only sub-token and between two sub-tokens."""
    seven = (0, 1, 2, 3, 4, 5, 6)
    fourteen = tuple((3 * i + 1) % 17 for i in range(14))
    fifteen = tuple((5 * i + 2) % 17 for i in range(15))
    reps = (3,) * ((ks + 1) // 2) if ks % 2 else (3,) * (ks // 2) + (4,)
    assert _min_frames(reps, True) == ks
    return [(), (1,), (6, 2), (4, 5, 4), seven, fourteen, fifteen, reps, (blank,), (2, blank, 5), (7,), (8, 9)]


@pytest.mark.parametrize("viterbi", [False, True])
@pytest.mark.parametrize("spike", [False, True])
@pytest.mark.parametrize("bo", [True, False])
def test_entries_of_every_length_up_to_fifteen(bo, spike, viterbi):
    """ks = 15, overlapping windows, two trailing frames no window reaches.  With the optional blank every entry aligns
    (lane 15 idles only for the 15-token entry's accept state 30 = lane 15's blank); without it the entries of 8, 14 and 15
    sub-tokens need more than 15 frames: -inf and a zero gradient, as the oracle says."""
    C, blank, ks, stride, B, T = 20, 19, 15, 5, 2, 27
    lexicon = _lengths_lexicon(ks, blank)
    sr = "trop" if viterbi else "log"
    got_out = _conv_case(f"conv_edges_len_{sr}", f"len_bo{int(bo)}_sp{int(spike)}_{sr}", lexicon, C, blank, ks, stride, B, T,
                         bo, spike, viterbi, 2)
    if not bo:
        for k in (5, 6, 7):
            assert (got_out[:, :, k] == NEG).all()


@pytest.mark.parametrize("viterbi", [False, True])
@pytest.mark.parametrize("ks", [1, 16])
def test_kernel_sizes_one_and_sixteen(ks, viterbi):
    """ks = 16: every register history slot and, with the 15-token entry, a skip code in bits 30-31 of the packed codes;
    ks = 1: one frame, only the entries of at most one sub-token align."""
    C, blank = 20, 19
    if ks == 16:
        lexicon, B, T, stride, neg = _lengths_lexicon(16, blank), 2, 35, 9, 2
    else:
        lexicon, B, T, stride, neg = [(), (1,), (blank,), (2,), (5,), (3, 3), (2, blank, 5)], 2, 9, 2, 3
    sr = "trop" if viterbi else "log"
    _conv_case(f"conv_edges_ks{ks}_{sr}", f"ks{ks}_{sr}", lexicon, C, blank, ks, stride, B, T, True, False, viterbi, neg)


@pytest.mark.parametrize("viterbi", [False, True])
@pytest.mark.parametrize("stride,T", [(2, 12), (5, 15), (7, 19), (7, 22), (3, 18)])
def test_strides_below_at_and_above_the_kernel_size(stride, T, viterbi):
    """ks = 5: overlapping windows (gradient rows of several windows add up), touching windows, windows with frames between
    them and frames behind the last one ((T - ks) % stride != 0): frames no window reaches get a gradient of exactly 0."""
    C, blank, ks = 9, 8, 5
    lexicon = [(0, 1), (2,), (1, 1), (0, 1, 2), (), (blank,), (3, blank, 4), (5, 6, 7, 5, 6), (2, 2, 2)]
    sr = "trop" if viterbi else "log"
    _conv_case(f"conv_edges_stride_{sr}", f"stride{stride}_T{T}_{sr}", lexicon, C, blank, ks, stride, 2, T, True, False,
               viterbi, 1)


@pytest.mark.parametrize("viterbi", [False, True])
@pytest.mark.parametrize("K", [1, 16, 17, 32, 33])
def test_lexicon_sizes_around_the_sixteen_entry_pass(K, viterbi):
    """The lexicon is walked 16 entries per pass and the tail rows of the last pass are clamped to the last entry: distinct
    short entries, then a 15-token one, so a tail row that leaked into the output or the gradient would show."""
    C, blank, ks, stride, B, T = 20, 19, 15, 5, 1, 20
    short = [(a,) for a in range(17)] + [(a, (a + 5) % 17) for a in range(17)]
    lexicon = short[:K - 1] + [tuple((5 * i + 2) % 17 for i in range(15))]
    assert len(lexicon) == K and len(set(lexicon)) == K
    sr = "trop" if viterbi else "log"
    _conv_case(f"conv_edges_K_{sr}", f"K{K}_{sr}", lexicon, C, blank, ks, stride, B, T, True, False, viterbi,
               K // 2 if K > 1 else None)


@pytest.mark.parametrize("viterbi", [False, True])
def test_windows_above_48_kb_of_lds(viterbi):
    """ks = 15, C = 830: 49800 B for the forward's window, 99600 B for the backward's window + gradient rows -- both
    launches opt in to more than 48 KB of dynamic LDS.  The lexicon names classes at both ends of a row."""
    C, ks, stride, B, T = 830, 15, 5, 1, 20
    blank = C - 1
    assert ks * C * 4 > 48 * 1024
    long = (0, C - 2) + tuple(50 * i + 7 for i in range(12)) + (C - 2,)
    lexicon = [(0,), (C - 2,), (0, C - 2), (C - 2, 400, 0), (), (blank,), (0, 0, C - 2, C - 2), long]
    assert len(long) == 15
    sr = "trop" if viterbi else "log"
    _conv_case(f"conv_edges_lds_{sr}", f"lds_{sr}", lexicon, C, blank, ks, stride, B, T, True, False, viterbi, 3)


# =================================================================================================
# B. Viterbi on exactly tying scores
# =================================================================================================
def _accepting_paths(g, labels, allowed=None):
    """Every arc sequence of g from a start node to an accept node that reads `labels` (over `allowed` arcs only)."""
    paths = [(n, ()) for n in g.start_nodes()]
    for l in labels:
        paths = [(g.dst[a], p + (a,)) for n, p in paths for a in g.out_arcs[n]
                 if g.ilab[a] == l and (allowed is None or a in allowed)]
    accept = set(g.accept_nodes())
    return [p for n, p in paths if n in accept]


TIE_KS, TIE_C, TIE_BLANK = 7, 4, 3
TIE_LEXICON = [(0, 1), (2,), (1, 1), (0, 1, 2), (), (TIE_BLANK,), (0, TIE_BLANK, 1), (2, 2, 2), (0, 1, 2, 0, 1, 2, 0),
               (1, 0), (2, 1, 0, 1)]


def _tie_windows():
    rs = np.random.RandomState(7)
    two = np.full((2, TIE_KS, TIE_C), -1.0, np.float32)
    # two alignments of (0, 1, 2) at score 0, everything else lower: with the optional blank ...
    for labels in ([0, 0, 1, 1, 2, 2, 2], [0, 0, 0, 1, 1, 2, 2]):
        two[0, np.arange(TIE_KS), labels] = 0.0
    # ... and without it
    for labels in ([0, 3, 1, 3, 2, 3, 3], [0, 0, 3, 1, 3, 2, 3]):
        two[1, np.arange(TIE_KS), labels] = 0.0
    return [np.zeros((TIE_KS, TIE_C), np.float32), rs.randint(-1, 2, size=(TIE_KS, TIE_C)).astype(np.float32),
            rs.randint(-1, 2, size=(TIE_KS, TIE_C)).astype(np.float32), two[0], two[1]]


@pytest.mark.parametrize("learn", [False, True])
@pytest.mark.parametrize("spike", [False, True])
@pytest.mark.parametrize("bo", [True, False])
def test_viterbi_ties_give_a_valid_best_path(bo, spike, learn):
    """Small-integer emissions and arc weights: every sum is exact in fp32, and many alignments tie.  One window per
    launch with delta[k] = 2**k, so entry k's path is bit k of dx (the class it reads per frame) and of dparams (the arcs it
    takes).  The score is the oracle's, exactly; the path is accepted by the entry's kernel graph, its emissions and arc
    weights sum to the score, and it spends exactly ks arcs.  Which of the tying paths it is, is the kernel's own rule."""
    from gtn_applications_amd.criterions import transducer as tr

    ks, C, blank, lexicon = TIE_KS, TIE_C, TIE_BLANK, TIE_LEXICON
    K = len(lexicon)
    tab = _table(lexicon, blank, bo, spike)
    graphs = [OC.make_kernel_graph(l, blank, bo, spike) for l in lexicon]
    slices = _arc_slices(lexicon, blank, bo, spike)
    params = None
    if learn:
        params = np.random.RandomState(11 + 2 * bo + spike).randint(-2, 3, size=tab.num_arcs).astype(np.float32)
    delta = (2.0 ** np.arange(K)).astype(np.float32).reshape(1, 1, K)
    finite = 0
    for win in _tie_windows():
        x = win[None]
        want_out, _, _ = OC.conv_transduce_1d_grad(x, lexicon, blank, ks, ks, 0.0 * delta, bo, spike,
                                                   None if params is None else params.astype(np.float64), True)
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        pd = torch.from_numpy(params).cuda().requires_grad_(True) if learn else None
        out = tr.ConvTransduce1DFunction.apply(xd, tab, ks, ks, pd, True)
        out.backward(torch.from_numpy(delta).cuda())
        got_out, got_dx = out.detach().cpu().numpy()[0, 0].astype(np.float64), xd.grad.cpu().numpy()[0].astype(np.float64)
        assert (got_out == want_out[0, 0]).all(), (got_out, want_out[0, 0])  # 1. exactly the oracle's score
        assert (got_dx == np.round(got_dx)).all() and (got_dx >= 0).all()
        bits = got_dx.astype(np.int64)
        assert (bits >> K == 0).all()
        got_dp = None
        if learn:
            got_dp = pd.grad.cpu().numpy().astype(np.float64)
            assert (got_dp == np.round(got_dp)).all() and (got_dp >= 0).all()
        for k, g in enumerate(graphs):
            reads = (bits >> k) & 1  # [ks, C]
            counts = None if got_dp is None else got_dp[slices[k]] / 2.0 ** k
            if got_out[k] == NEG:  # no path: bit k nowhere
                assert not reads.any() and (counts is None or not counts.any()), (k, lexicon[k])
                continue
            finite += 1
            assert (reads.sum(axis=1) == 1).all(), (k, lexicon[k], reads)  # 2. one class per frame
            labels = reads.argmax(axis=1).tolist()
            emitted = float(win[np.arange(ks), labels].astype(np.float64).sum())
            if counts is None:
                # 3. some accepting arc sequence reads these labels, 4. and the emissions alone sum to the score
                assert _accepting_paths(g, labels), (k, lexicon[k], labels)
                assert emitted == got_out[k], (k, lexicon[k], labels)
                continue
            assert (counts == np.round(counts)).all() and counts.sum() == ks, (k, lexicon[k], counts)  # 5.
            marked = set(np.nonzero(counts)[0].tolist())
            mine = [p for p in _accepting_paths(g, labels, marked)
                    if (np.bincount(p, minlength=len(counts)) == counts).all()]
            assert mine, (k, lexicon[k], labels, counts)  # 3. the marked arcs are an accepting path with these labels
            weight = float((counts * params[slices[k]].astype(np.float64)).sum())
            assert emitted + weight == got_out[k], (k, lexicon[k], labels, counts)  # 4.
    assert finite >= (30 if bo else 15)


# =================================================================================================
# C. host-side validation
# =================================================================================================
def test_sub_tokens_outside_the_classes_are_refused_and_the_last_class_works():
    from gtn_applications_amd.criterions import transducer as tr

    C, ks = 6, 5
    x = torch.randn(1, 8, C, device="cuda")
    for lexicon, bad in (([(0, 1), (2, C)], 1), ([(0, -1), (2,)], 0)):
        with pytest.raises(ValueError, match=f"entry {bad} "):
            tr.ConvTransduce1DFunction.apply(x, _table(lexicon, C - 1, True, False), ks, 1)
        with pytest.raises(ValueError, match=f"entry {bad} "):
            tr.ConvTransduce1D(lexicon, ks, 1, C - 1)(x)
    for blank in (C, -1):
        with pytest.raises(ValueError, match="blank_idx"):
            tr.ConvTransduce1DFunction.apply(x, _table([(0, 1)], blank, True, False), ks, 1)
    # the largest class as a sub-token (and the second largest as the blank)
    lexicon = [(C - 1,), (0, C - 1), (C - 1, C - 1, 3)]
    xd = x.clone().requires_grad_(True)
    out = tr.ConvTransduce1DFunction.apply(xd, _table(lexicon, C - 2, True, False), ks, 3)
    delta = np.random.RandomState(3).randn(1, 2, 3)
    out.backward(torch.from_numpy(delta.astype(np.float32)).cuda())
    want_out, want_dx, _ = OC.conv_transduce_1d_grad(x.cpu().numpy(), lexicon, C - 2, ks, 3, delta)
    check("conv_edges_last_class_out", out.detach().cpu().numpy(), want_out, 0.0)
    check("conv_edges_last_class_dx", xd.grad.cpu().numpy(), want_dx, float(np.abs(delta).sum()))


def test_backward_lds_limit_is_known_before_the_forward():
    """ks = 15: the forward has room for C <= 2730, the backward (window + gradient rows) for C <= 1365.  In between, a
    call that will need the gradient is refused at once, with the backward's own message; without one it runs."""
    from gtn_applications_amd import _native as N
    from gtn_applications_amd.criterions import transducer as tr

    ks, C = 15, 1400
    assert ks * C * 4 <= N.lib.wfl_conv_lds_limit() < 2 * ks * C * 4
    lexicon = [(0,), (C - 2, 0), (700, 701, 700), ()]
    tab = _table(lexicon, C - 1, True, False)
    x = torch.from_numpy(np.random.RandomState(5).randn(1, ks, C).astype(np.float32)).cuda().requires_grad_(True)
    with pytest.raises(N.WflUnsupported, match="conv_grad: window of 15 frames x 1400 classes does not fit LDS"):
        tr.ConvTransduce1DFunction.apply(x, tab, ks, 1)
    with pytest.raises(N.WflUnsupported, match="conv_grad"):  # (the parameters alone ask for the backward too)
        tr.ConvTransduce1DFunction.apply(x.detach(), tab, ks, 1, torch.zeros(tab.num_arcs, device="cuda", requires_grad=True))
    with torch.no_grad():
        out = tr.ConvTransduce1DFunction.apply(x, tab, ks, 1)
    want = OC.conv_transduce_1d(x.detach().cpu().numpy(), [OC.make_kernel_graph(l, C - 1, True) for l in lexicon], ks, 1)
    check("conv_edges_forward_only_out", out.cpu().numpy(), want, 0.0)
    C = 2731
    tab = _table(lexicon, C - 1, True, False)
    for grad in (True, False):
        x = torch.zeros(1, ks, C, device="cuda", requires_grad=grad)
        with pytest.raises(N.WflUnsupported, match="does not fit LDS"):
            tr.ConvTransduce1DFunction.apply(x, tab, ks, 1)
    with torch.no_grad(), pytest.raises(N.WflUnsupported, match="conv_forward"):
        tr.ConvTransduce1DFunction.apply(torch.zeros(1, ks, C, device="cuda"), tab, ks, 1)


# =================================================================================================
# D. STC augmentation beyond one wave of selected classes
# =================================================================================================
def _stc_augment_ref(x, select):
    """criterions/stc.py, the torch spelling in STC.forward (stc.py:199-220), in float64 on the host: x [T, B, C]."""
    lp = x.permute(1, 0, 2)
    lse = torch.logsumexp(lp[:, :, 1:], 2, keepdim=True)
    sel = lp.index_select(2, select)
    neglse = lse + torch.log1p(1e-7 - torch.exp(sel[:, :, 1:] - lse))
    return torch.cat([sel, lse, neglse], dim=2), torch.exp(sel[:, :, 1:] - lse)


@pytest.mark.parametrize("T,B,C,K", [(5, 3, 200, 151), (1, 1, 70, 66), (6, 2, 3, 3)])
def test_stc_augmentation_beyond_one_wave_of_selected_classes(T, B, C, K):
    """_StcAugment with K - 1 distinct labels in a shuffled order: three trips of the kernels' `k += 64` loops and a wave
    sum over more than 64 selected classes at K = 151 (T * B = 15 rows: the last workgroup is not full), one row, and
    every class selected with fewer classes than a wave has lanes.  Inputs are sub-normalised log-probabilities well
    below zero, so that no output is near 0 (rtol alone bounds the outputs) and u = exp(x[select] - lse) <= 0.9: near
    u = 1 the 1 + 1e-7 - u term is ill-conditioned in fp32 for kernel and torch alike, which is not this test's matter."""
    from gtn_applications_amd.criterions import stc

    rs = np.random.RandomState(31 + K)
    x = ((0.5 if C < 64 else 1.0) * rs.randn(T, B, C) - 8.0).astype(np.float32)
    select = [0] + (1 + rs.permutation(C - 1)[:K - 1]).tolist()
    rest = sorted(set(range(C)) - set(select))
    if rest:
        x[T // 2, B - 1, rest[len(rest) // 2]] = NEG  # a class the batch does not name
    inv = np.full(C, -1, np.int32)
    inv[select] = np.arange(K, dtype=np.int32)
    g = rs.randn(B, T, 2 * K).astype(np.float32)

    x64 = torch.from_numpy(x).double().requires_grad_(True)
    want, u = _stc_augment_ref(x64, torch.tensor(select))
    assert float(u.detach().max()) <= 0.9
    (want * torch.from_numpy(g).double()).sum().backward()

    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    got = stc._StcAugment.apply(xd, torch.tensor(select, dtype=torch.int32).cuda(), torch.from_numpy(inv).cuda())
    assert tuple(got.shape) == (B, T, 2 * K)
    got.backward(torch.from_numpy(g).cuda())
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=2e-5, atol=0)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x64.grad.numpy(), rtol=2e-4, atol=2e-6)
