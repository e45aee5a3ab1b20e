#!/usr/bin/env python3
"""Closed-loop use of a value function: thousands of pursuit / evasion pairs rolled out in parallel, each pair's
controls taken from the costate at its own state at every control step.

    python examples/closed_loop_rollout.py [n] [pairs] [steps]

The small air3D problem (examples/air3d_brt.py) is solved once; its value function V stays on the GPU.  Each control
step is ONE eval_costate call for all pairs -- grad V at the M relative states, computed from the 2^3 corner stencils
of each state, no full-grid derivative array -- followed by the optimal controls of both players
(dubins_relative.py:83-88: the evader turns with sign(p1 x2 - p2 x1 - p3), the pursuer against sign(p3)) and a
Runge-Kutta step of the relative dynamics, all on the device.  Pairs that start outside the reachable tube should
stay outside it, and never be captured.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40

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
brt, _, _ = lsp.HJIPDE_solve(data0, np.linspace(0, 2.0, 11), schemeData, 'minVOverTime',
                             lsp.Bundle(dict(quiet=True, keepLast=True)))
V = torch.as_tensor(np.asarray(brt), device="cuda")

# relative states well inside the grid; keep the pairs that start outside the tube by a margin
rng = np.random.default_rng(0)
lo, hi = np.array([0.0, -0.8, -np.pi]), np.array([2.2, 0.8, np.pi])
X = torch.as_tensor(lo + rng.random((4 * pairs, 3)) * (hi - lo), device="cuda")
X = X[lsp.eval_u(g, V, X) > 0.1][:pairs].contiguous()
M = X.shape[0]


def dynamics(x, a, b):
    """Relative coordinates, the evader at the origin: evader turn rate a, pursuer turn rate b."""
    return torch.stack([-speed + speed * torch.cos(x[:, 2]) + a * x[:, 1],
                        speed * torch.sin(x[:, 2]) - a * x[:, 0],
                        b - a], dim=1)


dt = 0.02
closest = torch.hypot(X[:, 0], X[:, 1])
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    p = lsp.eval_costate(g, V, X)                                   # (M, 3): one launch for all pairs
    p = torch.nan_to_num(p)                                         # a pair that left the grid keeps going straight
    a = turn * torch.sign(p[:, 0] * X[:, 1] - p[:, 1] * X[:, 0] - p[:, 2])      # evader: maximise V
    b = -turn * torch.sign(p[:, 2])                                              # pursuer: minimise V
    k1 = dynamics(X, a, b)
    k2 = dynamics(X + .5 * dt * k1, a, b)
    k3 = dynamics(X + .5 * dt * k2, a, b)
    k4 = dynamics(X + dt * k3, a, b)
    X = X + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    closest = torch.minimum(closest, torch.hypot(X[:, 0], X[:, 1]))
torch.cuda.synchronize()
sec = time.perf_counter() - t0

v_end = lsp.eval_u(g, V, X)                                         # NaN where a pair has left the grid
left = int(torch.isnan(v_end).sum())
outside = int((v_end > 0).sum())
print("grid %d^3, %d pairs, %d control steps of %.2f: %.1f ms per step (costates, controls, RK4)" % (n, M, steps, dt, 1e3 * sec / steps))
print("still outside the reachable tube  %d of %d on the grid (%d left the grid)" % (outside, M - left, left))
print("captured (distance <= %.1f)        %d" % (radius, int((closest <= radius).sum())))
