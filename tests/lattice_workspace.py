"""wfl_lattice_workspace of the tuned sweeps, restated independently of csrc/lattice_layout.h (shared by
test_gpu_lattice_streamed.py and test_lattice_layout_host.py)."""


def tuned_workspace(d, T):
    """wfl_lattice_workspace of the tuned sweeps, restated: xg rows | factors | references, and the alpha / beta
    scores followed by offsets, Z, formats and the bookkeeping of the probability-domain launches"""
    xg_main = (d.B * T * d.max_labels + 3) & ~3
    nch1 = T + 1
    tail = 2 * (d.B * (T + 1) * d.max_states if d.shared else (T + 1) * d.total_states)
    ab = tail + 2 * (d.B * nch1 + d.B) + 2 * d.B + 2 + 2 * 1024 + 12 * d.B + 32 + 2048 + 4 + 16 + d.B * (T // 32 + 2)
    return 2 * xg_main + d.B * T, ab
