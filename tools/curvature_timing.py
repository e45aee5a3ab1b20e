#!/usr/bin/env python3
"""termCurvature (curvatureFunc = curvatureSecond) on device tensors: ONE launch of curv_kernel (hj_term_curvature) against
the same formula as torch array ops on the device (ghost padding, centred differences, O&F eq. 1.8).

    python tools/curvature_timing.py [case ...]        cases: 201^3 513^3 4096^2 129^4 (default: all)

Per case and multiplier kind (scalar b / array b): microseconds per call from HIP events around 20 back-to-back calls
after 3 warm-up calls, the fraction of 8 TB/s on the algorithmic bytes (read phi, write ydot, read b when it is an
array: 16 / 24 B per cell in fp64, half in fp32), and the speed-up over the torch formulation.  The array-b call reads
max b back to the host (one synchronisation per call), which the scalar-b call does not."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                        # noqa: E402
import levelsetpy_amd as L          # noqa: E402

PEAK = 8e12
CASES = {"201^3": (201, 3, torch.float64), "513^3": (513, 3, torch.float64), "4096^2": (4096, 2, torch.float64),
         "129^4": (129, 4, torch.float32)}


def _pad_extrapolate(x, d):
    n = x.shape[d]
    e0, i0 = x.narrow(d, 0, 1), x.narrow(d, 1, 1)
    e1, i1 = x.narrow(d, n - 1, 1), x.narrow(d, n - 2, 1)
    return torch.cat([e0 + (e0 - i0).abs() * e0.sign(), x, e1 + (e1 - i1).abs() * e1.sign()], d)


def torch_term(phi, b, dx):
    """ydot = b kappa |grad phi| as torch array ops (the array path a user without the kernel would write)."""
    nd = phi.dim()
    P = phi
    for d in range(nd):
        P = _pad_extrapolate(P, d)

    def sl(d, lo, hi, other):
        return tuple(slice(lo, hi) if k == d else other[k] for k in range(nd))
    full = [slice(None)] * nd
    real = [slice(1, n + 1) for n in phi.shape]
    firstP = [(0.5 / dx[i]) * (P[sl(i, 2, None, full)] - P[sl(i, 0, -2, full)]) for i in range(nd)]
    first = [firstP[i][sl(i, None, None, real)] for i in range(nd)]
    g2 = first[0] ** 2
    for i in range(1, nd):
        g2 = g2 + first[i] ** 2
    kap = torch.zeros_like(phi)
    for i in range(nd):
        sii = dx[i] ** -2 * (P[sl(i, 2, None, real)] - 2 * phi + P[sl(i, 0, -2, real)])
        kap = kap + sii * (g2 - first[i] ** 2)
        for j in range(i):
            a = tuple(slice(None) if k == i else (slice(2, None) if k == j else real[k]) for k in range(nd))
            c = tuple(slice(None) if k == i else (slice(0, -2) if k == j else real[k]) for k in range(nd))
            sij = (0.5 / dx[j]) * (firstP[i][a] - firstP[i][c])
            kap = kap - 2 * first[i] * first[j] * sij
    gm = g2.sqrt()
    kap = torch.where(gm > 0, kap / gm ** 3, kap)
    return b * kap * gm, 1 / (2 * float(torch.as_tensor(b).max()) * sum(v ** -2 for v in dx))


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
    dx = [float(v) for v in np.asarray(g.dx).ravel()]
    x = torch.linspace(-1, 1, n, device="cuda", dtype=dt)
    r2 = torch.zeros((n,) * nd, device="cuda", dtype=dt)
    for d in range(nd):
        r2 = r2 + (x.reshape([n if k == d else 1 for k in range(nd)]) - 0.05 * (d + 1)) ** 2
    phi = r2.sqrt() - 0.5
    del r2
    y = phi.reshape(-1, 1)
    cells = phi.numel()
    esz = phi.element_size()
    for kind in ("scalar", "array"):
        b = 0.75 if kind == "scalar" else 0.5 + 0.25 * torch.cos(phi)
        sd = L.Bundle(dict(grid=g, b=b, curvatureFunc=L.curvatureSecond))
        us = _time(lambda: L.termCurvature(0.0, y, sd))
        nbytes = cells * esz * (2 if kind == "scalar" else 3)
        try:
            ut = _time(lambda: torch_term(phi, b, dx), reps=3)
            ref = "torch ops %10.1f us  x%5.1f" % (ut, ut / us)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            ref = "torch ops: out of device memory"
        print("%-7s %-7s %s b: termCurvature %9.1f us/call  %5.3f of 8 TB/s (%d B/cell)  %s"
              % (name, str(dt).replace("torch.", ""), kind, us, nbytes / (us * 1e-6) / PEAK, nbytes // cells, ref), flush=True)
        del b, sd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    for c in (sys.argv[1:] or list(CASES)):
        run(c)
