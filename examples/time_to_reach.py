#!/usr/bin/env python3
"""The time-to-reach function of a backward reachable tube, and what a rollout reads from it.

    python examples/time_to_reach.py [n] [pairs]

The small air3D problem (examples/air3d_brt.py) is solved in keepLast mode with computeTTR: HJIPDE_solve records, on the
device and without storing the stack, the time at which the growing tube first swept over every node -- extraOuts.TTR,
+inf outside the tube.  For the pursuer this is the minimum time to capture against the best evader.  Pairs that start
inside the tube are then rolled out in closed loop (both players optimal, controls from eval_costate on the tube's
value function, as in examples/closed_loop_rollout.py), and eval_u reads the TTR at each pair's state along the way: it
falls by about the time that has passed, and capture happens when it reaches zero.  Needs an MI355X (the package has
no CPU fallback).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 2048

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
radius, speed, turn = 0.5, 1.0, 1.0
data0 = torch.as_tensor(lsp.shapeCylinder(g, 2, np.zeros((3, 1)), radius), device="cuda")
dubins = lsp.DubinsVehicleRel(g, speed, turn)
schemeData = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation,
                             dissFunc=lsp.artificialDissipationGLF, CoStateCalc=lsp.upwindFirstWENO5))
horizon = 2.0
V, tau, outs = lsp.HJIPDE_solve(data0, np.linspace(0, horizon, 41), schemeData, 'minVOverTime',
                                lsp.Bundle(dict(quiet=True, keepLast=True, computeTTR=True, ttrInterpolate=True)))
TTR = outs.TTR                                  # a device tensor, as data0 was one
reached = torch.isfinite(TTR)
print("grid %d^3: %d of %d nodes are reached within %.1f; the largest time to reach is %.3f" % (
    n, int(reached.sum()), TTR.numel(), horizon, float(TTR[reached].max())))

# pairs that start inside the tube but outside the target, with a finite TTR at every corner of their cell
rng = np.random.default_rng(0)
lo, hi = np.array([0.0, -0.8, -np.pi]), np.array([2.2, 0.8, np.pi])
X = torch.as_tensor(lo + rng.random((16 * pairs, 3)) * (hi - lo), device="cuda")
ttr0 = lsp.eval_u(g, TTR, X)
keep = torch.isfinite(ttr0) & (ttr0 > 0.3) & (ttr0 < 0.8 * horizon)
X, ttr0 = X[keep][:pairs].contiguous(), ttr0[keep][:pairs]
M = X.shape[0]


def dynamics(x, a, b):
    """Relative coordinates, the evader at the origin: evader turn rate a, pursuer turn rate b."""
    return torch.stack([-speed + speed * torch.cos(x[:, 2]) + a * x[:, 1],
                        speed * torch.sin(x[:, 2]) - a * x[:, 0],
                        b - a], dim=1)


dt, t = 0.02, 0.0
captured_at = torch.full((M,), float("inf"), dtype=torch.float64, device="cuda")
print("%d pairs; time passed, mean TTR at the pairs' states still at large, captured so far" % M)
for step in range(int(round(horizon / dt)) + 1):
    dist = torch.hypot(X[:, 0], X[:, 1])
    captured_at = torch.where((dist <= radius) & torch.isinf(captured_at), t, captured_at)
    free = torch.isinf(captured_at)
    if step % 10 == 0:
        now = lsp.eval_u(g, TTR, X)
        ok = free & torch.isfinite(now)
        print("  t = %.2f   mean TTR %.3f   captured %d" % (t, float(now[ok].mean()) if bool(ok.any()) else 0.0, int((~free).sum())))
    if not bool(free.any()):
        break
    p = torch.nan_to_num(lsp.eval_costate(g, V, X))
    a = turn * torch.sign(p[:, 0] * X[:, 1] - p[:, 1] * X[:, 0] - p[:, 2])      # evader: maximise V
    b = -turn * torch.sign(p[:, 2])                                              # pursuer: minimise V
    k1 = dynamics(X, a, b)
    k2 = dynamics(X + .5 * dt * k1, a, b)
    k3 = dynamics(X + .5 * dt * k2, a, b)
    k4 = dynamics(X + dt * k3, a, b)
    X = torch.where(free[:, None], X + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4), X)
    t += dt
done = torch.isfinite(captured_at)
err = (captured_at - ttr0)[done]
print("captured %d of %d; capture time minus the TTR read at the start: mean %+.3f, worst %.3f (grid spacing %.3f)" % (
    int(done.sum()), M, float(err.mean()) if err.numel() else 0.0, float(err.abs().max()) if err.numel() else 0.0,
    float(np.asarray(g.dx).ravel()[0])))
