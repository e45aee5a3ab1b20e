#!/usr/bin/env python3
"""Targets and obstacles of a 6-D problem built on the device: the pursuit game of two Dubins cars with obstacles.

    python examples/six_d_shapes.py [n] [horizon]

examples/two_cars_6d.py writes its capture set by hand, with reshaped torch vectors.  Here every set comes from the shape
library, on a low_mem grid (no dense coordinate arrays exist at any point):

  * the capture set sqrt((x0 - x3)^2 + (x1 - x4)^2) - r is sphere_between((0, 1), (3, 4), r): a sphere in differences of axes;
  * a static obstacle for the evader, a rectangle in (x0, x1) unbounded along the other four axes;
  * a moving obstacle, a cylinder in (x0, x1) whose centre travels along tau, handed to HJIPDE_solve as a ShapeSeries: the
    solver evaluates member i when interval i begins, one launch each, and the stack (len(tau),) + g.shape never exists.

The static and the moving obstacle are one TREE: the union of a shared rectangle and a batched cylinder is a batched shape, so
one series holds both.  Solved with DubinsPair6D; prints the path the solve took, the members the series evaluated and the
bytes its stack would have taken.

Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import hidim, shapes as S

n = int(sys.argv[1]) if len(sys.argv) > 1 else 13
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 0.4
nth = 12
speed, turn, radius = 1.0, 1.0, 0.8
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
top = 2 * np.pi * (1 - 1.0 / nth)
inf = np.inf

g6 = lsp.createGrid(col([-2, -2, 0, -2, -2, 0]), col([2, 2, top, 2, 2, top]), col([n, n, nth, n, n, nth], np.int64), [2, 5], low_mem=True)
pair = lsp.DubinsPair6D(g6, v_e=speed, v_p=speed, w_e=turn, w_p=turn)
shape = tuple(int(v) for v in np.asarray(g6.N).ravel())
tau = np.linspace(0.0, horizon, 5)

# ---- the capture set, one launch
t0 = time.time()
data0 = lsp.evaluate_shape(g6, lsp.sphere_between((0, 1), (3, 4), radius))
torch.cuda.synchronize()
print("capture set on %s = %.3g nodes: %.1f ms, %s, flags %s" % (shape, float(np.prod(shape)), 1e3 * (time.time() - t0),
                                                               S.last_info()["kernel"], S.last_info()["flags"]))

# ---- obstacles for the evader: a wall that stands, a disc that moves from left to right over tau
wall = S.rectangle_by_corners([0.8, -0.5, -inf, -inf, -inf, -inf], [1.2, 0.5, inf, inf, inf, inf])
centers = np.zeros((len(tau), 6))
centers[:, 0] = np.linspace(-1.5, -0.5, len(tau))
centers[:, 1] = 1.0
disc = S.cylinder([2, 3, 4, 5], centers, 0.4)
obstacles = lsp.series(g6, wall | disc)
print("obstacles: a ShapeSeries of %d members, shape %s; its stack would take %.2f GB, a member takes %.2f GB" % (
    len(obstacles), obstacles.shape, 8 * float(np.prod(obstacles.shape)) / 1e9, 8 * float(np.prod(shape)) / 1e9))

sd6 = lsp.Bundle(dict(grid=g6, hamFunc=pair.hamiltonian, partialFunc=pair.dissipation, derivFunc=lsp.upwindFirstENO2))
t0 = time.time()
V6, _, outs = lsp.HJIPDE_solve(data0, tau, sd6, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True, obstacleFunction=obstacles)))
torch.cuda.synchronize()
print("solved to t = %.2f over %d intervals: %.2f s" % (horizon, len(tau) - 1, time.time() - t0))
print("  last_path: %s" % hidim.last_path())
print("  series.evaluated: %s" % obstacles.evaluated)
print("  value function: min %.3f, max %.3f, %.1f %% of the nodes inside the reachable tube" % (
    float(V6.min()), float(V6.max()), 100 * float((V6 <= 0).double().mean())))
