#!/usr/bin/env python3
"""Timing of HJIPDE_solve_batch (levelsetpy_amd/batch.py, libhj_batch.so) on one MI355X -> profiles/batch_timing.txt.

    python tools/batch_timing.py [--n 51] [--span 0.4] [--out FILE]

Workload: the air3D game on n^3 nodes (default 51, the size of the reference's notebooks), as-shipped WENO5, fp64, ONE tau
interval [0, span] that takes every problem at least 50 RK3 steps; B = 1, 8, 64, 256 problems whose evader / pursuer speeds and
turn rates are spread, so their step counts differ.  Device tensors in, keepLast.  Three ways over the same problems, taking turns
in the same process, device events around each call after a warm-up, median of the repetitions (min .. max beside it):
  batch       HJIPDE_solve_batch: one launch of batch_substep_kernel per RK stage for all problems
  launches    hjb_integrate alone on prepared buffers: the batch without the front end (tables, step bounds, NaN guard, gather)
  loop        one HJIPDE_solve per problem with the default HJ_DIRECT_BELOW: what a sweep cost before the batch existed
A problem-step is one RK3 step of one problem; algorithmic bytes are 64 per cell and RK3 step (bench.py's accounting); the working
set is about 5 arrays of B x n^3 x 8 bytes, set against the 256 MiB Infinity Cache.

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=51)
    ap.add_argument("--span", type=float, default=0.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/batch_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import _bffi, _ffi, _marshal, batch

    n = args.n
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
    cells = n ** 3
    target = L.shapeCylinder(g, 2, np.zeros((3, 1)), .5)
    tau = np.array([0.0, args.span])
    dev = torch.device("cuda", torch.cuda.current_device())
    prop = torch.cuda.get_device_properties(0)
    lines = ["HJIPDE_solve_batch on one MI355X: air3D, %d^3 nodes, as-shipped WENO5, fp64, one interval [0, %.3g], keepLast, device tensors" % (n, args.span),
             "tools/batch_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the three ways take turns in one process; device events around each call; median (min .. max) in ms", ""]
    rng = np.random.default_rng(0)
    for B, reps in ((1, 15), (8, 9), (64, 5), (256, 3)):
        systems = []
        for b in range(B):
            s = L.DubinsVehicleRel(g, 1.0, 1.0 if B == 1 else float(rng.uniform(0.6, 1.2)))
            if B > 1:
                s.v_e, s.v_p = float(rng.uniform(0.75, 1.5)), float(rng.uniform(0.75, 1.5))
            systems.append(s)
        sds = [L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, derivFunc=L.upwindFirstWENO5)) for s in systems]
        data0 = torch.as_tensor(np.broadcast_to(target, (B,) + target.shape).copy(), device=dev)
        ea = L.Bundle(dict(quiet=True, keepLast=True))

        def run_batch():
            return L.HJIPDE_solve_batch(data0, tau, sds, 'minVOverTime', ea)

        def run_loop():
            return [L.HJIPDE_solve(data0[b], tau, sds[b], 'minVOverTime', L.Bundle(dict(quiet=True, keepLast=True)))[0] for b in range(B)]

        # hjb_integrate alone, on buffers prepared once
        desc, _ = _marshal.descriptor(g, "float64")
        tab = batch.tables(g, torch, dev)
        st, why = batch.classify(data0, sds, 'minVOverTime', ea)
        assert why is None, why
        par = torch.as_tensor(np.asarray(st.params, dtype=np.float64), device=dev)
        sbs = batch.step_bounds(g, tab, desc, st.ham, par, B, torch, dev)
        bufs = torch.empty((3, B, cells), dtype=torch.float64, device=dev)
        probs = (_bffi.Problem * B)()
        flat = data0.reshape(B, cells)
        for b in range(B):
            probs[b].y_in, probs[b].buf_a, probs[b].buf_b, probs[b].work = (flat[b].data_ptr(), bufs[0, b].data_ptr(), bufs[1, b].data_ptr(),
                                                                             bufs[2, b].data_ptr())

        def run_launches():
            return batch.integrate_batch(g, tab, desc, st.scheme, st.ham, par, sbs, probs, tau[0], tau[1], 3, _ffi.POST_MIN_PREV,
                                         torch=torch, device=dev)

        out_b = run_batch()
        out_l = run_loop()
        run_launches()
        torch.cuda.synchronize()
        same = all(torch.equal(out_b[0][b], out_l[b]) for b in range(B))
        steps = out_b[2].steps[:, 0]
        total = int(steps.sum())
        tb, tl, tk = [], [], []
        for _ in range(reps):
            tb.append(event_ms(torch, run_batch))
            tk.append(event_ms(torch, run_launches))
            tl.append(event_ms(torch, run_loop))
        ws = 5 * B * cells * 8 / 2.0 ** 20
        lines.append("B = %d: %s; steps per problem %d .. %d, %d problem-steps in %d stage launches; results equal the loop's bit for bit: %s" % (
            B, batch.last_path(), steps.min(), steps.max(), total, 3 * int(steps.max()), same))
        lines.append("  working set about %.0f MiB = %.2f of the 256 MiB Infinity Cache" % (ws, ws / 256.0))
        for name, ms in (("batch", tb), ("launches", tk), ("loop", tl)):
            med, lo, hi = stats(ms)
            sec = med * 1e-3
            lines.append("  %-9s %10.3f (%.3f .. %.3f)   %8.2f us per problem-step   %.3e cell-substeps/s   %.4f of 8 TB/s on algorithmic bytes" % (
                name, med, lo, hi, 1e3 * med / total, 3.0 * cells * total / sec, 64.0 * cells * total / sec / 8e12))
        mb, ml = stats(tb)[0], stats(tl)[0]
        lines.append("  loop / batch = %.2f: per problem-step the batch is %s than the loop" % (ml / mb, "FASTER" if mb < ml else "SLOWER"))
        lines.append("")
    text = "\n".join(lines[:-1]) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
