#!/usr/bin/env python3
"""Check a reachable tube after the solve: roll out many closed-loop trajectories through the stored stack in ONE launch.

    python examples/batch_opt_traj.py [n] [pairs]

The small air3D problem (examples/air3d_brt.py) is solved once with every set stored (time first, flipped: index 0 is the
tube of the full horizon, the last index the target).  computeOptTrajs then follows `pairs` pursuit / evasion pairs from
random relative states: at every time stamp each pair finds, by bisection, the latest stored set that still holds it, takes
the costate there, and both players act optimally for it (the evader maximises, the pursuer minimises).  A pair that starts
inside the tube should be captured -- driven into the target -- within the horizon whatever the evader does; a pair that starts
outside should not be.  The fractions of both kinds are printed.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import rollout

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 100000

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
radius, speed, turn = 0.5, 1.0, 1.0
data0 = lsp.shapeCylinder(g, 2, np.zeros((3, 1)), radius)
dubins = lsp.DubinsVehicleRel(g, speed, turn)
schemeData = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation,
                             dissFunc=lsp.artificialDissipationGLF, CoStateCalc=lsp.upwindFirstWENO5))
tau = np.linspace(0, 2.0, 11)
stack, _, _ = lsp.HJIPDE_solve(data0, tau, schemeData, 'minVOverTime', lsp.Bundle(dict(quiet=True, flipOutput=True)))
V = torch.as_tensor(np.asarray(stack), device="cuda")

rng = np.random.default_rng(0)
lo, hi = np.array([0.0, -0.8, -np.pi]), np.array([2.2, 0.8, np.pi])
X = torch.as_tensor(lo + rng.random((pairs, 3)) * (hi - lo), device="cuda")
v0 = lsp.eval_u(g, V[0], X)                                          # the tube of the full horizon at the initial states

args = lsp.Bundle(dict(uMode='max', dMode='min', subSamples=4, status=True))
lsp.computeOptTrajs(g, V, tau, dubins, X[:64], args)                 # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
trajs, lengths, _, outs = lsp.computeOptTrajs(g, V, tau, dubins, X, args)
torch.cuda.synchronize()
sec = time.perf_counter() - t0

captured = outs.status == rollout.REACHED
left = outs.status == rollout.LEFT_GRID
inside, outside = v0 < -0.05, v0 > 0.05                              # a margin of about half a cell around the tube's boundary
steps = int((lengths.to(torch.int64) - 1).sum()) * 4
print("grid %d^3 x %d stored sets, %d pairs: one launch of %s, %.1f ms, %.2e trajectory-steps/s" % (
    n, len(tau), pairs, outs.path, 1e3 * sec, steps / sec))
for name, sel in (("inside the tube ", inside), ("outside the tube", outside)):
    k = int(sel.sum())
    print("started %s  %7d pairs: %6.2f %% captured within the horizon, %5.2f %% left the grid" % (
        name, k, 100.0 * int((captured & sel).sum()) / max(k, 1), 100.0 * int((left & sel).sum()) / max(k, 1)))
