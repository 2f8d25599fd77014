"""What K6's other kinds and the per-sample evaluation kernel cost, BASELINE batch (B=4096, T=1001, xd=8), time-major pred, mask widths 1
and D, on one GPU.  Output: --out, by default profiles/loss_kinds_cost.txt.

    python profiles/scripts/loss_kinds_cost.py [--parent-lib PATH/libpsnode_hip.so] [--out FILE]

 (a) psnode_masked_mse_f32 (loss + grad, the kernel call) of a build of the PARENT commit (--parent-lib, loaded next to this build through
     ctypes) and of this build, same arguments.  The listing of every kernel of psnode_loss.o is identical (profiles/loss_kinds_listing_diff.txt),
     so this is a confirmation, not a finding.
 (b) every kind through masked_loss: the kernel call (loss + grad) and forward + backward through autograd.
 (c) the same objective in torch ops with the same Loss_func: the route before.
 (d) per_sample_loss for MSE and Huber against the torch evaluation line.
Method: every variant of a group is timed in turn, ROUNDS times round-robin (so that a drift of the machine hits all of them), each timing a
device-event window of N calls after a warm-up; reported: the median over rounds and the range [min, max].
Algorithmic bytes per (b,t) row, D=8: pred 32 + target 32 + mask 4*mw read, grad 32 written (training); no grad, + 32*B/(B*T) out (per-sample).
HBM fraction: of the 8.0 TB/s spec peak, as profiles/scripts/loss_bench.py reports it."""
import argparse
import ctypes
import functools
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from py_psnode_amd import _lib  # noqa: E402
from py_psnode_amd import loss as L  # noqa: E402
from py_psnode_amd.fused import _workspace_of  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "loss_kinds_cost.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--T", type=int, default=1001)
args = ap.parse_args()

assert torch.cuda.is_available(), "a measurement needs the GPU"
dev = torch.device("cuda", 0)
B, T, D = args.B, args.T, 8
KNEE = 0.05
KINDS = {"mse": F.mse_loss, "l1": F.l1_loss, "smooth_l1": functools.partial(F.smooth_l1_loss, beta=KNEE),
         "huber": functools.partial(F.huber_loss, delta=KNEE)}
g = torch.Generator().manual_seed(0)
x = (0.3 * torch.randn(B, T, D, generator=g)).to(dev)
xs = (x.permute(1, 0, 2) + 0.05 * torch.randn(T, B, D, device=dev)).contiguous()      # time-major integrator output
pred = xs.permute(1, 0, 2)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def group(title, variants, nbytes=None):
    """variants: [(name, fn)]; round-robin, median and range of ms per call"""
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            ms[name].append(window(fn, args.calls))
    say(title)
    out = {}
    for name, _ in variants:
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        extra = ""
        if nbytes and name in nbytes:
            extra = f"   {nbytes[name] / med / 1e6:7.0f} GB/s = {nbytes[name] / med / 1e6 / 8000:.3f} of 8.0 TB/s"
        say(f"  {name:<44s} {med:8.4f} ms  [{lo:.4f}, {hi:.4f}]{extra}")
        out[name] = (med, lo, hi)
    return out


def raw_call(lib, mask, inv):
    """psnode_masked_mse_f32 of `lib` on (pred, x, mask): loss + grad"""
    a, keep, _ = L._loss_args(pred, x, mask, None, inv, 1.0, 0.0, "cost")
    out = torch.empty(D + 2, device=dev)
    grad = torch.empty(T, B, D, device=dev)
    a.out, a.grad_pred = out.data_ptr(), grad.data_ptr()
    lib.psnode_masked_mse_workspace_bytes.restype = ctypes.c_size_t
    lib.psnode_masked_mse_workspace_bytes.argtypes = [ctypes.POINTER(_lib.LossArgsF32)]
    lib.psnode_masked_mse_f32.restype = ctypes.c_int32
    lib.psnode_masked_mse_f32.argtypes = [ctypes.POINTER(_lib.LossArgsF32), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    nbytes = lib.psnode_masked_mse_workspace_bytes(ctypes.byref(a))
    ws, p, _ = _workspace_of(nbytes, dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call():
        assert lib.psnode_masked_mse_f32(ctypes.byref(a), ctypes.c_void_p(p), ctypes.c_size_t(nbytes), ctypes.c_void_p(st)) == 0
    call.keep = (keep, out, grad, ws)
    call.out, call.grad = out, grad
    return call


say(f"loss_kinds_cost: B={B} T={T} D={D}, time-major pred, beta = delta = {KNEE}; {args.rounds} rounds x {args.calls} calls, "
    f"median [min, max] per call; {torch.cuda.get_device_name(0)}")
this = _lib.load()
parent = ctypes.CDLL(args.parent_lib) if args.parent_lib else None
for mw in (1, D):
    mask = (torch.rand(B, T, mw, generator=g) > 0.1).float().to(dev)
    inv = L.inv_mask_sum(mask)
    algo = B * T * (3 * 4 * D + 4 * mw)
    say()
    say(f"==== mask width {mw}")
    # (a)
    if parent is not None:
        ca, cb = raw_call(parent, mask, inv), raw_call(this, mask, inv)
        r = group("(a) psnode_masked_mse_f32, loss + grad, kernel call", [("parent build", ca), ("this build", cb)],
                  {"parent build": algo, "this build": algo})
        same = torch.equal(ca.out, cb.out) and torch.equal(ca.grad, cb.grad)
        say(f"  outputs of the two builds bitwise equal: {same};  this / parent = {r['this build'][0] / r['parent build'][0]:.4f}")
    else:
        say("(a) not measured: no --parent-lib")

    # (b) kernel call and autograd round trip
    def kernel_call(lf):
        return lambda: L.masked_loss_terms(pred, x, mask, lf, inv_norm=inv, want_grad=True)

    def fused_fwd_bwd(lf):
        def f():
            p = xs.permute(1, 0, 2).requires_grad_(True)
            L.masked_loss(p, x, mask, lf, inv_norm=inv)[0].backward()
        return f

    def torch_fwd_bwd(lf):
        def f():
            p = xs.permute(1, 0, 2).requires_grad_(True)
            torch.sum(torch.sum(torch.sum(lf(p, x, reduction="none") * mask, dim=1), dim=0) / torch.sum(mask)).backward()
        return f

    r = group("(b) masked_loss_terms, loss + grad, kernel call (python call included)", [(k, kernel_call(lf)) for k, lf in KINDS.items()],
              {k: algo for k in KINDS})
    lo, hi = r["mse"][1], r["mse"][2]
    for k in ("l1", "smooth_l1", "huber"):
        inside = lo <= r[k][0] <= hi
        say(f"  {k}: median / mse median = {r[k][0] / r['mse'][0]:.4f}; inside mse's own range [{lo:.4f}, {hi:.4f}]: {inside}")
    group("(b) masked_loss via autograd, forward + backward", [(k, fused_fwd_bwd(lf)) for k, lf in KINDS.items()])
    # (c)
    group("(c) the same objective in torch ops, forward + backward", [(k, torch_fwd_bwd(lf)) for k, lf in KINDS.items()])

    # (d)
    def torch_eval(lf):
        return lambda: torch.sum(lf(pred * mask, x * mask, reduction="none"), dim=1)

    ps_bytes = B * T * (2 * 4 * D + 4 * mw) + B * D * 4
    with torch.no_grad():
        r = group("(d) per-sample evaluation table [B, D]",
                  [("per_sample_loss mse", lambda: L.per_sample_loss(pred, x, mask, "mse")),
                   ("per_sample_loss huber", lambda: L.per_sample_loss(pred, x, mask, KINDS["huber"])),
                   ("torch evaluation line mse", torch_eval(KINDS["mse"])), ("torch evaluation line huber", torch_eval(KINDS["huber"]))],
                  {"per_sample_loss mse": ps_bytes, "per_sample_loss huber": ps_bytes})
    say(f"  ({(B + 31) // 32} workgroups of 256 threads: one per strip of 32 trajectories, each walking its {(T + 15) // 16} time tiles in order)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write("\n".join(lines) + "\n")
