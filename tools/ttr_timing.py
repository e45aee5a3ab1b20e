#!/usr/bin/env python3
"""Timing of the time-to-reach kernels (levelsetpy_amd/ttr.py, libhj_ttr.so) on one MI355X -> profiles/ttr_timing.txt.

    python tools/ttr_timing.py [--n 201] [--T 33] [--reps 20] [--out FILE]

Workload: a time-first stack of T growing sets on the n^3 Dubins-relative grid, resident on the device, fp64 and fp32.
Measured with device events around each call, after a warm-up, median of --reps calls (min and max beside it):

  (i)   hjt_ttr_from_stack: the whole stack folded in one pass, in TD2TTR's default mode (earliest crossing, no interpolation)
        and in the toolbox's (every crossing overwrites, interpolated); beside it the same result from a loop of torch ops on
        the device (the baseline to beat), and the effective bytes (T n sizeof(T) + 8 n) / time next to the read rate that
        tools/ubench/bw2 achieved on 1 GiB arrays in the same run (a child process started before this one touches the GPU).
  (ii)  hjt_ttr_update: one step, likewise; effective bytes 3 n sizeof(T) (y and last_y read, last_y written) + 8 n where
        the earliest-crossing rule reads the old ttr; the stores to ttr at the crossing nodes are not counted.
  (iii) HJIPDE_solve(keepLast, computeTTR) against the same solve without the option, alternating: the cost per tau interval.

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here, only that the kernel and the torch
loop agree where the arithmetic is a comparison alone.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bw2_rates():
    exe = os.path.join(ROOT, "tools", "ubench", "bw2")
    if not os.path.exists(exe):
        return None
    try:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd="/tmp")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    except Exception:  # noqa: BLE001
        return None


def event_times(torch, fn, reps, warm=3):
    """ms of each of `reps` calls, by device events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms):
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def torch_fold(torch, d, tau, level, first, interp):
    inf = float("inf")
    ttr = torch.where(d[0] <= level, tau[0], inf).to(torch.float64)
    for k in range(1, d.shape[0]):
        y, last = d[k].to(torch.float64), d[k - 1].to(torch.float64)
        changed = (y <= level) & (last > level)
        if first:
            changed &= ttr == inf
        if interp:
            a, b = last - level, y - level
            tc = tau[k - 1] - ((tau[k] - tau[k - 1]) * a) / (b - a)
            ttr = torch.where(changed, tc, ttr)
        else:
            ttr = torch.where(changed, tau[k], ttr)
    return ttr


def torch_update(torch, y, last, ttr, t, t_last, level, first, interp):
    inf = float("inf")
    yd, ld = y.to(torch.float64), last.to(torch.float64)
    changed = (yd <= level) & (ld > level)
    if first:
        changed &= ttr == inf
    tc = (t_last - ((t - t_last) * (ld - level)) / ((yd - level) - (ld - level))) if interp else t
    return torch.where(changed, tc, ttr), y.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=201)
    ap.add_argument("--T", type=int, default=33)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--solve-n", type=int, default=201)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ttr_timing.txt"))
    args = ap.parse_args()

    rates = bw2_rates()                    # before this process touches the GPU
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/ttr_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import _tffi, ttr as TT

    n, T = args.n, args.T
    prop = torch.cuda.get_device_properties(0)
    read = rates["hbm_1GiB"].get("read") if rates else None
    lines = ["Time-to-reach kernels on one MI355X: %d^3 nodes, T = %d slices" % (n, T),
             "tools/ttr_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "device events around each call, %d calls after 3 warm-up calls: median (min .. max) in ms" % args.reps,
             "tools/ubench/bw2 in this run, 1 GiB arrays, TB/s: %s" % (json.dumps(rates["hbm_1GiB"]) if rates else "not measured (bw2 not built)"),
             ""]
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2, low_mem=True)
    vs = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
    x, y, th = vs[0][:, None, None], vs[1][None, :, None], vs[2][None, None, :]
    base = torch.sqrt(x * x + y * y) + 0.15 * torch.sin(th) * x
    tau_h = np.linspace(0.0, 1.2, T)
    tau = torch.as_tensor(tau_h, device="cuda")
    radii = np.linspace(0.5, 1.7, T)
    nn = n ** 3
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dname, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        d = torch.stack([(base - r).to(dt) for r in radii])
        size = d.element_size()
        lines.append("%s stack, %.2f GB" % (dname, d.numel() * size / 1e9))
        for label, first, interp in (("earliest crossing, no interpolation (TD2TTR's default)", True, False),
                                     ("every crossing overwrites, interpolated (the toolbox's rule)", False, True)):
            mode = (_tffi.FIRST if first else 0) | (0 if interp else _tffi.NO_INTERP)
            out = torch.empty(nn, dtype=torch.float64, device="cuda")

            def kernel():
                _tffi.check(_tffi.lib().hjt_ttr_from_stack(1 if dt == torch.float32 else 0, d.data_ptr(), T, nn, nn, tau.data_ptr(), 0.0,
                                                           mode, out.data_ptr(), stream))
            km = stats(event_times(torch, kernel, args.reps))
            tm = stats(event_times(torch, lambda: torch_fold(torch, d, tau, 0.0, first, interp), max(3, args.reps // 4), warm=1))
            ref = torch_fold(torch, d, tau, 0.0, first, interp).reshape(-1)
            equal = bool(torch.equal(out, ref))
            if not interp:
                assert equal, "hjt_ttr_from_stack and the torch loop disagree"
            eff = (T * nn * size + 8 * nn) / (km[0] * 1e-3) / 1e12
            lines.append("  (i) %s" % label)
            lines.append("      hjt_ttr_from_stack   %8.3f (%.3f .. %.3f)   effective %.2f TB/s%s" % (
                km + (eff, "   = %.2f of bw2's read rate" % (eff / read) if read else "")))
            lines.append("      loop of torch ops    %8.3f (%.3f .. %.3f)   %.1fx the kernel's time; same bits: %s" % (tm + (tm[0] / km[0], equal)))
            # (ii) one update step, from the state after half of the stack
            h = T // 2
            ttr0 = TT.ttr_from_stack(d, h, nn, nn, tau_h[:h], 0.0, mode)
            last0 = d[h - 1].reshape(-1).clone()
            yk = d[h].reshape(-1)
            ttr, last = ttr0.clone(), last0.clone()

            def upd():
                _tffi.check(_tffi.lib().hjt_ttr_update(1 if dt == torch.float32 else 0, yk.data_ptr(), nn, float(tau_h[h]), float(tau_h[h - 1]),
                                                       0.0, mode, ttr.data_ptr(), last.data_ptr(), stream))
            um = stats(event_times(torch, upd, args.reps))
            tum = stats(event_times(torch, lambda: torch_update(torch, yk, last0, ttr0, float(tau_h[h]), float(tau_h[h - 1]), 0.0, first, interp),
                                    args.reps))
            effu = (3 * nn * size + (8 * nn if first else 0)) / (um[0] * 1e-3) / 1e12
            lines.append("  (ii) hjt_ttr_update      %8.3f (%.3f .. %.3f)   effective %.2f TB/s%s" % (
                um + (effu, "   = %.2f of bw2's read rate" % (effu / read) if read else "")))
            lines.append("       torch ops           %8.3f (%.3f .. %.3f)   %.1fx the kernel's time" % (tum + (tum[0] / um[0],)))
        lines.append("")
        del d
    # (iii) the solve
    m = args.solve_n
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / m)]]).T
    gs = L.createGrid(gmin, gmax, m * np.ones((3, 1), dtype=np.int64), 2)
    d0 = torch.as_tensor(L.shapeCylinder(gs, 2, np.zeros((3, 1)), .5), device="cuda")
    s = L.DubinsVehicleRel(gs, 1, 1)
    sd = L.Bundle(dict(grid=gs, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF,
                       CoStateCalc=L.upwindFirstWENO5))
    taus = np.linspace(0.0, 0.2, 9)

    def solve(on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.HJIPDE_solve(d0, taus, sd, 'minVOverTime', L.Bundle(dict(quiet=True, keepLast=True, computeTTR=on)))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    solve(True), solve(False)
    runs = {True: [], False: []}
    for _ in range(7):
        for on in (False, True):
            runs[on].append(solve(on))
    a, b = stats(runs[False]), stats(runs[True])
    lines.append("(iii) HJIPDE_solve, %d^3 Dubins BRT (minVOverTime, keepLast, device tensor in), %d tau intervals, host clock around the whole" % (m, len(taus) - 1))
    lines.append("      solve ending in a synchronisation, 7 rounds alternating: median (min .. max) in ms")
    lines.append("      without computeTTR   %9.3f (%.3f .. %.3f)" % a)
    lines.append("      with computeTTR      %9.3f (%.3f .. %.3f)" % b)
    lines.append("      difference of the medians per tau interval: %.3f ms (%.2f %% of the solve)" % ((b[0] - a[0]) / (len(taus) - 1),
                                                                                                  100 * (b[0] - a[0]) / a[0]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
