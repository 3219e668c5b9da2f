"""Host time of the pieces of the CTC operator's C++ path (GPU box): staging, node forward, backward."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtn_applications_amd import engine as E
from gtn_applications_amd.criterions import ctc
from gtn_applications_amd._native import ops as node

B, T, C, L, N = 128, 1000, 100, 44, 1000
g = torch.Generator().manual_seed(0)
x = torch.randn(B, T, C, generator=g).cuda().requires_grad_(True)
tg = torch.randint(C - 2, (B, L), generator=g).tolist()
lim = (C - 1, False, False, E.CTC_FAST_MAX_LEN, E.CTC_FAST_MAX_CLASSES, E.CTC_FAST_MAX_CLASSES_LONG)


def timed(fn, n=N, skip=50):
    for i in range(skip):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn()
    host = (time.perf_counter() - t0) / n * 1e6
    torch.cuda.synchronize()
    return host


st = node.stage_targets(tg, x.device)
print("stage_targets (same targets) %.1f us" % timed(lambda: node.stage_targets(tg, x.device)))
print("ctc_loss_staged (forward)    %.1f us" % timed(lambda: node.ctc_loss_staged(x, st, *lim)))
print("ctc_loss_lists (forward)     %.1f us" % timed(lambda: node.ctc_loss_lists(x, tg, *lim)))
print("CTCLoss() (forward)          %.1f us" % timed(lambda: ctc.CTCLoss(x, tg, C - 1)))
def fb():
    x.grad = None
    ctc.CTCLoss(x, tg, C - 1).backward()
print("CTCLoss().backward()         %.1f us" % timed(fb))
loss = [None]
def f2():
    loss[0] = node.ctc_loss_lists(x, tg, *lim)
def b2():
    f2()
    loss[0].backward()
print("lists fwd + backward         %.1f us" % timed(b2))
xd = x.detach()
print("empty_like                   %.1f us" % timed(lambda: torch.empty_like(xd)))
with torch.no_grad():
    print("CTCLoss() no_grad (py path)  %.1f us" % timed(lambda: ctc.CTCLoss(xd, tg, C - 1)))
