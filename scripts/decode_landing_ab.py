"""Where the device decode's result lands (csrc/decode_kernels.hip): the kernels' stores straight into pinned host memory
and one event wait -- what the operator does (csrc/torch_ops.cpp::hypotheses_collect) -- against a device buffer plus one
copy of the offsets and one of the compact region.  CTC's call at the benchmark shape, through the C ABI, alternating."""
import ctypes, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from gtn_applications_amd import _native as N
from gtn_applications_amd import engine as E

torch.manual_seed(0)
B, T, C = 128, 1000, 100
x = torch.randn(B, T, C).cuda()
cap, wsb = ctypes.c_int64(), ctypes.c_int64()
N.check(N.lib.wfl_decode_workspace(B, T, 0, ctypes.byref(cap), ctypes.byref(wsb)))
ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
bufs = {"pinned": (torch.empty(cap.value, dtype=torch.int32).pin_memory(), torch.empty(B + 1, dtype=torch.int64).pin_memory()),
        "device": (torch.empty(cap.value, dtype=torch.int32, device="cuda"), torch.empty(B + 1, dtype=torch.int64, device="cuda"))}
done = torch.cuda.Event()


def call(kind):
    out, offs = bufs[kind]
    N.check(N.lib.wfl_decode_emissions(E.ptr(x), None, B, T, C, C - 1, 0, N.DECODE_NAN_IS_MAX, E.ptr(ws), E.ptr(out), cap.value,
                                       E.ptr(offs), E.stream_ptr()))
    if kind == "pinned":
        done.record()
        done.synchronize()
        return out[:int(offs[B])].clone()
    total = int(offs.cpu()[B])
    return out[:total].cpu()


def timed(kind, n=50):
    for _ in range(5):
        call(kind)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call(kind)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


assert torch.equal(call("pinned"), call("device"))
for rep in range(3):
    for kind in ("pinned", "device"):
        print(f"decode_emissions B={B} T={T} C={C}, result to {kind} memory: {timed(kind):.4f} ms per call")
