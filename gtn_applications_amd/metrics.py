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
        """(hyp table, V, longest, ref table, V, longest, sep) as the operators take them; the tables ([exp_ptr | exp_sym]
        int32) are uploaded once per device"""
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        args = self._device_tables.get(device)
        if args is None:
            args = ()
            for t in (self.hyp_table, self.ref_table):
                if t is None:
                    args += (None, 0, 1)
                else:
                    args += (torch.from_numpy(np.concatenate([t[0], t[1]])).to(device), len(t[0]) - 1, t[2])
            args = self._device_tables[device] = args + (self.sep,)
        return args

    def check_hypothesis_labels(self, n_labels, what):
        """ValueError unless the hypothesis table covers the labels [0, n_labels) a decode can emit"""
        if self.hyp_table is not None and self.hyp_size < n_labels:
            raise ValueError(f"{what}: the decode can emit {n_labels} labels, the counter's hypothesis table has "
                             f"{self.hyp_size} entries")

    def staged_targets(self, targets, device):
        """the batch's targets on `device` (the stager's cache: free for a batch the criterion has just seen), checked
        against the reference table"""
        tg = E.targets_on_device(targets, device)
        if self.ref_table is not None and tg.n and (tg.label_min < 0 or tg.label_max >= self.ref_size):
            bad = tg.label_min if tg.label_min < 0 else tg.label_max
            raise ValueError(f"ErrorCounter: target label {bad} is outside the reference table [0, {self.ref_size})")
        return tg

    def counts(self, predictions, targets):
        """int64 CPU tensor [B, 4]: per utterance (token distance, target tokens, word distance, target words).
        `predictions`: what viterbi() returns (1-D int tensors or int lists); `targets`: what the criterion takes."""
        predictions = list(predictions)
        if len(predictions) != len(targets):
            raise ValueError(f"ErrorCounter: {len(predictions)} predictions for {len(targets)} targets")
        # (the labels are checked where they are staged, before anything is launched -- and before a missing GPU is reported)
        dev = E.require_gpu() if torch.cuda.is_available() else torch.device("cpu")
        if not predictions:
            return torch.zeros((0, 4), dtype=torch.int64)
        ref = self.staged_targets(targets, dev)
        hyp = E.CtcTargets([p.cpu() if isinstance(p, torch.Tensor) and p.is_cuda else p for p in predictions], dev)
        if self.hyp_table is not None and hyp.n and (hyp.label_min < 0 or hyp.label_max >= self.hyp_size):
            bad = hyp.label_min if hyp.label_min < 0 else hyp.label_max
            raise ValueError(f"ErrorCounter: predicted label {bad} is outside the hypothesis table [0, {self.hyp_size})")
        if dev.type != "cuda":
            E.require_gpu()
        return N.ops.errors_count(hyp._st, ref._st, *self.tables(dev))

    @staticmethod
    def totals(counts):
        """(tokens_dist, words_dist, n_tokens, n_words) of a [B, 4] counts tensor: the tuple of train.py:87"""
        s = counts.sum(dim=0).tolist() if counts.numel() else [0, 0, 0, 0]
        return s[0], s[2], s[1], s[3]

    def __call__(self, predictions, targets):
        return self.totals(self.counts(predictions, targets))


def decode_emissions_errors(counter, targets, x, drop, bias=None, num_replabels=0, flags=0, lengths=None):
    """engine.decode_emissions' launch and the counts behind it, on x's device: [B, 4] int64 on the host and nothing else
    (lengths: int32 [B] on x's device, the frames of each utterance of a padded batch)"""
    if len(targets) != x.shape[0]:
        raise ValueError(f"errors: {x.shape[0]} utterances for {len(targets)} targets")
    ref = counter.staged_targets(targets, x.device)
    drop = -1 if drop is None else int(drop)
    if lengths is not None:
        return N.ops.decode_emissions_lengths_errors(x, bias, lengths, drop, num_replabels, flags, ref._st,
                                                     *counter.tables(x.device))
    return N.ops.decode_emissions_errors(x, bias, drop, num_replabels, flags, ref._st, *counter.tables(x.device))


def beam_search_errors(counter, targets, x, blank, beam_size, classes_per_frame, lengths=None, lm=None, lm_weight=1.0,
                       length_bonus=0.0, lm_eos=True):
    """engine.ctc_beam_search's launches (best hypothesis only) and the counts behind them, on x's device: [B, 4] int64
    on the host and nothing else (beam_size, classes_per_frame: already checked, engine.check_beam_arguments).  lm,
    lm_weight, length_bonus, lm_eos: as in engine.ctc_beam_search."""
    if len(targets) != x.shape[0]:
        raise ValueError(f"errors: {x.shape[0]} utterances for {len(targets)} targets")
    lm, weight, bonus, eos = E.check_lm_arguments(lm, x.shape[2], int(blank), lm_weight, length_bonus, lm_eos, "errors")
    ref = counter.staged_targets(targets, x.device)
    if lm is not None:
        return N.ops.ctc_beam_search_lm_errors(x, lengths, int(blank), int(beam_size), int(classes_per_frame),
                                               *lm.device_arguments(x.device), weight, bonus, eos, ref._st,
                                               *counter.tables(x.device))
    return N.ops.ctc_beam_search_errors(x, lengths, int(blank), int(beam_size), int(classes_per_frame), ref._st,
                                        *counter.tables(x.device))


def decode_paths_errors(counter, targets, paths, drop, num_replabels=0, flags=0, T=None):
    """engine.decode_paths' launch and the counts behind it"""
    if len(targets) != paths.shape[0]:
        raise ValueError(f"errors: {paths.shape[0]} utterances for {len(targets)} targets")
    ref = counter.staged_targets(targets, paths.device)
    T = paths.shape[1] if T is None else T
    return N.ops.decode_paths_errors(paths, T, -1 if drop is None else int(drop), num_replabels, flags, ref._st,
                                     *counter.tables(paths.device))
