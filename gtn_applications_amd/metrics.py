"""Token and word error counts of a batch, on the device: the reference's compute_edit_distance (train.py:74-87, called
per batch at train.py:278-284 and test.py:94-109) behind wfl_errors_count (csrc/error_kernels.hip).

Per utterance: the labels of the prediction and of the target are replaced by the symbols they stand for (each side has
its own table: tokens_to_text for predictions, to_text for targets, train.py:80), the word separator is stripped at both
ends, and four integers come out -- the Levenshtein distance of the two symbol strings, the length of the target string,
the Levenshtein distance of the two word sequences (maximal runs of symbols other than the separator; words are equal iff
they are the same symbols in the same order) and the number of target words.  There is no host implementation:
predictions that are on the host are uploaded like targets are (the stager of csrc/torch_ops.cpp); the criteria's
errors() count behind their device decode without the predictions ever reaching the host."""
import numpy as np
import torch

from . import _native as N
from . import engine as E


def _table(symbols, number):
    """(exp_ptr int32 [V+1], exp_sym int32 [exp_ptr[V]], longest expansion) of a sequence of symbol sequences"""
    ptr = np.zeros(len(symbols) + 1, np.int32)
    sym = []
    for v, s in enumerate(symbols):
        sym.extend(number(c) for c in s)
        ptr[v + 1] = len(sym)
    longest = int(np.diff(ptr).max()) if len(symbols) else 0
    return ptr, np.asarray(sym, np.int32).reshape(-1), longest


class ErrorCounter:
    """ErrorCounter(hyp_symbols=None, ref_symbols=None, wordsep=None)

    `hyp_symbols` / `ref_symbols`: a sequence, indexed by label, of the symbol sequences the labels of predictions /
    targets stand for (a string per label: each character is a symbol; an entry may be empty).  None: a label is its own
    symbol.  With both tables given the symbols are any hashables; the counter numbers them once, `wordsep` included.
    With a table on one side only, that table's symbols and `wordsep` are the other side's labels: non-negative ints,
    taken as they are.  `wordsep` None: no stripping, no words (both word counts are 0)."""

    def __init__(self, hyp_symbols=None, ref_symbols=None, wordsep=None):
        numbered = hyp_symbols is not None and ref_symbols is not None
        ids = {}

        def number(c):
            if numbered:
                return ids.setdefault(c, len(ids))
            if isinstance(c, (bool, str)) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) <= 0x7FFFFFFF:
                raise ValueError(f"ErrorCounter: with a table on one side only its symbols and the separator are the other "
                                 f"side's labels (non-negative ints), not {c!r}")
            return int(c)

        self.hyp_table = None if hyp_symbols is None else _table(hyp_symbols, number)
        self.ref_table = None if ref_symbols is None else _table(ref_symbols, number)
        for name, t in (("hyp_symbols", self.hyp_table), ("ref_symbols", self.ref_table)):
            if t is not None and len(t[0]) < 2:
                raise ValueError(f"ErrorCounter: {name} is empty")
        self.sep = -1 if wordsep is None else number(wordsep)
        self.symbol_ids = ids if numbered else None
        self._device_tables = {}

    @classmethod
    def for_preprocessor(cls, pre):
        """The tables tokens_to_text / to_text use (datasets/*.py): predictions spell `pre.tokens`, targets `pre.tokens`
        under a lexicon and `pre.graphemes` without one; every entry is a string, every character a symbol."""
        ref = pre.tokens if getattr(pre, "lexicon", None) is not None else pre.graphemes
        return cls(list(pre.tokens), list(ref), pre.wordsep)

    @property
    def hyp_size(self):
        """labels the hypothesis table covers (None: identity, any label)"""
        return None if self.hyp_table is None else len(self.hyp_table[0]) - 1

    @property
    def ref_size(self):
        return None if self.ref_table is None else len(self.ref_table[0]) - 1

    def tables(self, device):
        """the operators' ErrorTables (csrc/torch_ops.cpp) of this counter on `device`: both tables ([exp_ptr | exp_sym]
        int32, uploaded once per device) and the separator"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        held = self._device_tables.get(device)
        if held is None:
            sides = [None if t is None else (torch.from_numpy(np.concatenate(t[:2])).to(device), len(t[0]) - 1, t[2])
                     for t in (self.hyp_table, self.ref_table)]
            held = self._device_tables[device] = N.ops.ErrorTables(*sides, self.sep)
        return held

    def check_hypothesis_labels(self, n_labels, what):
        """ValueError unless the hypothesis table covers the labels [0, n_labels) a decode can emit"""
        if self.hyp_table is not None and self.hyp_size < n_labels:
            raise ValueError(f"{what}: the decode can emit {n_labels} labels, the counter's hypothesis table has "
                             f"{self.hyp_size} entries")

    def counts(self, predictions, targets):
        """int64 CPU tensor [B, 4]: per utterance (token distance, target tokens, word distance, target words).
        `predictions`: what viterbi() returns (1-D int tensors or int lists); `targets`: what the criterion takes."""
        predictions = list(predictions)
        if len(predictions) != len(targets):
            raise ValueError(f"ErrorCounter: {len(predictions)} predictions for {len(targets)} targets")
        dev = E.require_gpu() if torch.cuda.is_available() else torch.device("cpu")
        if not predictions:
            return torch.zeros((0, 4), dtype=torch.int64)
        ref = E.targets_on_device(targets, dev)
        hyp = E.CtcTargets([p.cpu() if isinstance(p, torch.Tensor) and p.is_cuda else p for p in predictions], dev)
        tables = self.tables(dev)
        if dev.type != "cuda":  # (a label outside its table is the caller's error: reported before a missing GPU is)
            tables.check_labels(hyp._st, ref._st)
            E.require_gpu()
        return N.ops.errors_count(hyp._st, ref._st, tables)

    @staticmethod
    def totals(counts):
        """(tokens_dist, words_dist, n_tokens, n_words) of a [B, 4] counts tensor: the tuple of train.py:87"""
        s = counts.sum(dim=0).tolist() if counts.numel() else [0, 0, 0, 0]
        return s[0], s[2], s[1], s[3]

    def __call__(self, predictions, targets):
        return self.totals(self.counts(predictions, targets))


def _staged(counter, targets, batch, drop=None):
    """(the targets staged on the batch's device, the counter's tables there, `drop` as the operators take it) of a batch
    of B utterances; the operators check the targets' labels against the reference table before they launch"""
    if len(targets) != batch.shape[0]:
        raise ValueError(f"errors: {batch.shape[0]} utterances for {len(targets)} targets")
    return E.targets_on_device(targets, batch.device)._st, counter.tables(batch.device), -1 if drop is None else int(drop)


def decode_emissions_errors(counter, targets, x, drop, bias=None, num_replabels=0, flags=0, lengths=None):
    """engine.decode_emissions' launch and the counts behind it, on x's device: [B, 4] int64 on the host and nothing else
    (lengths: int32 [B] on x's device, the frames of each utterance of a padded batch)"""
    ref, tables, drop = _staged(counter, targets, x, drop)
    return N.ops.decode_emissions_errors(x, bias, drop, num_replabels, flags, ref, tables, lengths)


def beam_search_errors(counter, targets, x, plan, lengths=None):
    """The launches of engine.BeamPlan.search (`plan`: checked; its best hypothesis only) and the counts behind them, on
    x's device: [B, 4] int64 on the host and nothing else"""
    ref, tables, _ = _staged(counter, targets, x)
    return N.ops.ctc_beam_search_errors(x, lengths, plan.on_device(x.device), ref, tables)


def asg_beam_search_errors(counter, targets, x, W, plan, drop, num_replabels):
    """The launches of engine.AsgBeamPlan.search (`plan`: checked; its best hypothesis only, garbage dropped and
    replabels unpacked on the way out) and the counts behind them, on x's device: [B, 4] int64 on the host and nothing else"""
    ref, tables, drop = _staged(counter, targets, x, drop)
    return N.ops.asg_beam_search_errors(x, W, plan.beam, plan.classes_per_frame, drop, num_replabels, ref, tables)


def asg_beam_search_lexicon_errors(counter, targets, x, W, plan, drop, num_replabels):
    """asg_beam_search_errors for the search with a lexicon (`plan`: a checked engine.AsgLexiconBeamPlan): the launches
    of its search() and the counts behind them"""
    ref, tables, drop = _staged(counter, targets, x, drop)
    return N.ops.asg_beam_search_lexicon_errors(x, W, plan.on_device(x.device), drop, num_replabels, ref, tables)


def asg_beam_search_lm_errors(counter, targets, x, W, plan, drop, num_replabels):
    """asg_beam_search_errors for the search with a token-level LM (`plan`: a checked engine.AsgLmBeamPlan): the launches
    of its search() and the counts behind them"""
    ref, tables, drop = _staged(counter, targets, x, drop)
    return N.ops.asg_beam_search_lm_errors(x, W, plan.on_device(x.device), drop, num_replabels, ref, tables)


def transducer_beam_search_errors(counter, targets, x, Wt, plan):
    """The launches of engine.TransducerBeamPlan.search (`plan`: checked; its best hypothesis only; Wt: the transitions
    or None) and the counts behind them, on x's device: [B, 4] int64 on the host and nothing else"""
    ref, tables, _ = _staged(counter, targets, x)
    return N.ops.transducer_beam_search_errors(x, Wt, plan.blank, plan.forced, plan.beam, plan.classes_per_frame, ref, tables)


def transducer_beam_search_lexicon_errors(counter, targets, x, Wt, plan):
    """transducer_beam_search_errors for the search with a lexicon (`plan`: a checked engine.TransducerLexiconBeamPlan):
    the launches of its search() and the counts behind them"""
    ref, tables, _ = _staged(counter, targets, x)
    return N.ops.transducer_beam_search_lexicon_errors(x, Wt, plan.on_device(x.device), ref, tables)


def transducer_beam_search_lm_errors(counter, targets, x, Wt, plan):
    """transducer_beam_search_errors for the search with a token-level LM (`plan`: a checked engine.TransducerLmBeamPlan):
    the launches of its search() and the counts behind them"""
    ref, tables, _ = _staged(counter, targets, x)
    return N.ops.transducer_beam_search_lm_errors(x, Wt, plan.on_device(x.device), ref, tables)


def transducer_merged_beam_search_errors(counter, targets, x, Wt, plan, spelling):
    """transducer_beam_search_errors with hypotheses merged by spelling (`spelling`: the engine.Spelling of the plan's
    classes and blank): the launches of engine.transducer_merged_search and the counts behind them"""
    ref, tables, _ = _staged(counter, targets, x)
    return N.ops.transducer_beam_search_merged_errors(x, Wt, spelling.on_device(x.device), spelling.num_symbols, plan.blank,
                                                      plan.forced, plan.beam, plan.classes_per_frame, ref, tables)


def plan_errors(counter, targets, x, plan, *args, spelling=None):
    """The counts behind the best hypotheses of `plan`'s search: the plan knows which -- a checked plan of any of engine's
    classes; args: what its search() takes behind x, without normalize and dtype (CTC: lengths; ASG: W, drop,
    num_replabels; the Transducer: Wt).  spelling: as TransducerBeamPlan.search's, the merged search"""
    if spelling is not None:
        return transducer_merged_beam_search_errors(counter, targets, x, args[0], plan, spelling)
    if isinstance(plan, E.BeamPlan):
        return beam_search_errors(counter, targets, x, plan, *args)
    count = next(count for cls, count in ((E.AsgBeamPlan, asg_beam_search_errors),
                                          (E.AsgLexiconBeamPlan, asg_beam_search_lexicon_errors),
                                          (E.AsgLmBeamPlan, asg_beam_search_lm_errors),
                                          (E.TransducerBeamPlan, transducer_beam_search_errors),
                                          (E.TransducerLexiconBeamPlan, transducer_beam_search_lexicon_errors),
                                          (E.TransducerLmBeamPlan, transducer_beam_search_lm_errors)) if isinstance(plan, cls))
    return count(counter, targets, x, args[0], plan, *args[1:])


def decode_paths_errors(counter, targets, paths, drop, num_replabels=0, flags=0, T=None):
    """engine.decode_paths' launch and the counts behind it"""
    ref, tables, drop = _staged(counter, targets, paths, drop)
    return N.ops.decode_paths_errors(paths, paths.shape[1] if T is None else T, drop, num_replabels, flags, ref, tables)
