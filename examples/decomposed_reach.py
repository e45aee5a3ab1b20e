#!/usr/bin/env python3
"""A six-dimensional reach set from three two-dimensional solves.

    python examples/decomposed_reach.py [n] [horizon]

Three double integrators (position, velocity; acceleration bounds 0.6, 1.5 and 2.4) are self-contained subsystems of one
6-D system: its state is (x1, v1, x2, v2, x3, v3) and it has reached the target when ALL three have, so its value function
is the maximum of theirs -- the intersection of the back-projected reach sets, which is exact for sets (module docstring of
levelsetpy_amd/decomp.py).  The three share one n x n grid (default 101), and that is the point: ONE HJIPDE_solve_batch call
advances them together.  The 6-D array would have n^6 nodes (10^12 at the default: 8 TB); it is never built.  Instead
Decomposition keeps the three 2-D arrays on the device and is asked:

  * V and the active subsystem -- the vehicle that is furthest from done -- at 10^5 random 6-D states, in one launch;
  * the costate at a few of them (the active vehicle's gradient on its own two axes, zero elsewhere);
  * a 3-D slice (x1, v1, x2) at fixed (v2, x3, v3), handed to extract_level_set as any 3-D value function would be.

Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import batch, decomp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 101
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5

gmin, gmax = np.array([[-1.0], [-1.5]]), np.array([[1.0], [1.5]])
g = lsp.createGrid(gmin, gmax, n * np.ones((2, 1), dtype=np.int64), None)
bounds = (0.6, 1.5, 2.4)
systems = [lsp.DoubleIntegrator(g, u) for u in bounds]
sd = lsp.Bundle(dict(grid=g, hamFunc=systems[0].hamiltonian, partialFunc=systems[0].dissipation, derivFunc=lsp.upwindFirstENO2))
target = lsp.shapeSphere(g, np.zeros((2, 1)), 0.3)
data0s = torch.as_tensor(np.broadcast_to(target, (3,) + target.shape).copy(), device="cuda")
tubes, _, _ = lsp.HJIPDE_solve_batch(data0s, np.array([0.0, horizon]), sd, 'minVOverTime',
                                     lsp.Bundle(dict(quiet=True, keepLast=True, systems=systems)))
print("three double integrators on %d x %d to t = %.2f in one batched solve: %s" % (n, n, horizon, batch.last_path()))

dims = [[0, 1], [2, 3], [4, 5]]
dec = lsp.Decomposition([g] * 3, [tubes[b] for b in range(3)], dims, mode='intersection')
print("the 6-D grid would hold %.3g nodes; the decomposition holds %d" % (float(n) ** 6, 3 * n * n))

M = 100000
lo, hi = np.tile(gmin.ravel(), 3), np.tile(gmax.ravel(), 3)
xs = torch.as_tensor(lo + np.random.default_rng(0).random((M, 6)) * (hi - lo), device="cuda")
V = dec.eval_u(xs)
active = dec.eval_active(xs)
inside = V <= 0
print("%d random states (%s): %.2f %% can reach all three targets; the slowest vehicle (bound %.1f) decides for %.1f %% of them" % (
    M, decomp.last_path(), 100.0 * inside.double().mean().item(), bounds[0], 100.0 * (active == 0).double().mean().item()))
p = dec.eval_costate(xs[:3], lsp.upwindFirstENO2)
for x, v, a, row in zip(xs[:3].cpu().numpy(), V[:3].cpu().numpy(), active[:3].cpu().numpy(), p.cpu().numpy()):
    print("  x = %s  V = %+.4f  active %d  costate %s" % (np.round(x, 2), v, a, np.round(row, 3)))

six = lsp.createGrid(lo.reshape(-1, 1), hi.reshape(-1, 1), n * np.ones((6, 1), dtype=np.int64), None, low_mem=True)
fixed = [0.2, 0.1, -0.3]                                     # v2, x3, v3
sl = dec.slice(six, [0, 1, 2], fixed)
g3 = lsp.createGrid(lo[:3].reshape(-1, 1), hi[:3].reshape(-1, 1), n * np.ones((3, 1), dtype=np.int64), None, low_mem=True)
mesh = lsp.extract_level_set(g3, sl, 0.0)
print("slice (x1, v1, x2) at (v2, x3, v3) = %s: %s nodes (%s); its zero level set has %d vertices and %d triangles" % (
    fixed, "x".join(map(str, sl.shape)), decomp.last_path(), len(mesh.verts), len(mesh.faces)))
