#!/usr/bin/env python3
"""A parameter sweep of the air3D game in ONE batched solve: every combination of evader speed, pursuer speed and turn rate.

    python examples/batch_solve.py [n] [horizon]

The small air3D problem (examples/air3d_brt.py) asks from which relative states a pursuer can force a capture.  The answer
depends on the vehicles: here the evader's speed, the pursuer's speed and the common turn rate are swept over a 4 x 4 x 4
lattice, 64 backward reachable tubes on one n^3 grid (default 41).  HJIPDE_solve_batch advances all of them together -- one
launch per Runge-Kutta stage for the whole sweep; the problems' CFL bounds differ, so each takes its own number of steps and sits
out the launches it does not need.  Printed: the volume of each tube's capture set, steps taken, and the time against the same
sweep as a loop of HJIPDE_solve calls (whose results are the same bits).  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import batch

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
target = lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 0.5)

sweep = [(ve, vp, w) for ve in (0.75, 1.0, 1.25, 1.5) for vp in (0.75, 1.0, 1.25, 1.5) for w in (0.6, 0.8, 1.0, 1.2)]
systems = []
for ve, vp, w in sweep:
    s = lsp.DubinsVehicleRel(g, 1.0, w)          # scalar bounds: the native system; the two speeds are set apart afterwards
    s.v_e, s.v_p = ve, vp
    systems.append(s)
B = len(systems)
schemeData = lsp.Bundle(dict(grid=g, hamFunc=systems[0].hamiltonian, partialFunc=systems[0].dissipation,
                             derivFunc=lsp.upwindFirstWENO5))
tau = np.linspace(0, horizon, 5)
data0s = torch.as_tensor(np.broadcast_to(target, (B,) + target.shape).copy(), device="cuda")
args = lsp.Bundle(dict(quiet=True, keepLast=True, systems=systems))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


lsp.HJIPDE_solve_batch(data0s[:2], tau[:2], schemeData, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True, systems=systems[:2])))
(tubes, _, outs), sec_batch = timed(lambda: lsp.HJIPDE_solve_batch(data0s, tau, schemeData, 'minVOverTime', args))


def loop():
    res = []
    for b, s in enumerate(systems):
        sd = lsp.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, derivFunc=lsp.upwindFirstWENO5))
        res.append(lsp.HJIPDE_solve(data0s[b], tau, sd, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True)))[0])
    return torch.stack(res)


loop()
single, sec_loop = timed(loop)
cell = float(np.prod(np.asarray(g.dx)))
vol = (tubes <= 0).reshape(B, -1).sum(1).double().cpu().numpy() * cell
steps = outs.steps.sum(1)
print("air3D sweep on %d^3, horizon %.2f: %d tubes, %s" % (n, horizon, B, batch.last_path()))
print("steps per problem %d .. %d (%d in all): %d stage launches carry them all in the batch" % (
    steps.min(), steps.max(), steps.sum(), 3 * outs.steps.max(0).sum()))
print("batched %.1f ms, loop of HJIPDE_solve %.1f ms (%.1fx); the same bits: %s" % (
    1e3 * sec_batch, 1e3 * sec_loop, sec_loop / sec_batch, bool(torch.equal(tubes, single))))
print(" v_e   v_p    w    capture volume   steps")
for (ve, vp, w), v, k in zip(sweep, vol, steps):
    print("%4.2f  %4.2f  %4.2f  %12.4f  %6d" % (ve, vp, w, v, k))
