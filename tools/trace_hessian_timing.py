#!/usr/bin/env python3
"""termTraceHessian (hessianFunc = hessianSecond) on device tensors: ONE launch of curv_kernel's HJ_CURV_TRACE mode
(hj_term_trace_hessian) against the composed path on the same tensors (hessianSecond, then cellMatrixMultiply /
cellMatrixTrace and the step bound as array ops -- what termTraceHessian does with any other hessianFunc).

    python tools/trace_hessian_timing.py [case ...]        cases: 201^3 513^3 4096^2 129^4 (default: all)

Per case and matrix form (every entry of L and R a scalar / dense per-node L and R): microseconds per call from HIP events
around 20 back-to-back calls after 3 warm-up calls, the fraction of 8 TB/s on the algorithmic bytes (read phi, write ydot;
per-node forms also read the 2 n^2 entry arrays), and the speed-up over the composed path.  The per-node call reads
max |trace(L D R)| back to the host (one synchronisation per call), which the all-scalar call does not."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                        # noqa: E402
import levelsetpy_amd as L          # noqa: E402

PEAK = 8e12
CASES = {"201^3": (201, 3, torch.float64), "513^3": (513, 3, torch.float64), "4096^2": (4096, 2, torch.float64),
         "129^4": (129, 4, torch.float32)}


def _composed(grid, data):          # a hessianFunc that is not hessianSecond itself: termTraceHessian's array path
    return L.hessianSecond(grid, data)


def _time(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def run(name):
    n, nd, dt = CASES[name]
    g = L.createGrid(-np.ones((nd, 1)), np.ones((nd, 1)), n * np.ones((nd, 1), dtype=np.int64), low_mem=True)
    x = torch.linspace(-1, 1, n, device="cuda", dtype=dt)
    r2 = torch.zeros((n,) * nd, device="cuda", dtype=dt)
    for d in range(nd):
        r2 = r2 + (x.reshape([n if k == d else 1 for k in range(nd)]) - 0.05 * (d + 1)) ** 2
    phi = r2.sqrt() - 0.5
    del r2
    y = phi.reshape(-1, 1)
    cells = phi.numel()
    esz = phi.element_size()
    sig = np.eye(nd) + 0.1 * np.arange(nd * nd).reshape(nd, nd) / (nd * nd)
    for kind in ("scalar", "per-node"):
        if kind == "scalar":
            Lm, Rm = sig, sig.T
        else:
            w = 1 + 0.1 * torch.cos(phi)
            Lm = [[w * float(sig[i, j]) for j in range(nd)] for i in range(nd)]
            Rm = [[w * float(sig[j, i]) for j in range(nd)] for i in range(nd)]
            del w
        sd = L.Bundle(dict(grid=g, hessianFunc=L.hessianSecond, L=Lm, R=Rm))
        us = _time(lambda: L.termTraceHessian(0.0, y, sd))
        nbytes = cells * esz * (2 if kind == "scalar" else 2 + 2 * nd * nd)
        sdc = L.Bundle(dict(grid=g, hessianFunc=_composed, L=Lm, R=Rm))
        try:
            uc = _time(lambda: L.termTraceHessian(0.0, y, sdc), reps=3)
            ref = "composed %10.1f us  x%5.1f" % (uc, uc / us)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            ref = "composed: out of device memory"
        print("%-7s %-7s %-8s L, R: termTraceHessian %9.1f us/call  %5.3f of 8 TB/s (%d B/cell)  %s"
              % (name, str(dt).replace("torch.", ""), kind, us, nbytes / (us * 1e-6) / PEAK, nbytes // cells, ref), flush=True)
        del Lm, Rm, sd, sdc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    for c in (sys.argv[1:] or list(CASES)):
        run(c)
