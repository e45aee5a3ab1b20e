#!/usr/bin/env python3
"""One reach set, many vehicles: the air3D collision tube placed at the pose of K other vehicles and used, as ONE obstacle, in a solve.

    python examples/placed_union.py [n] [K]

A reach set in relative coordinates is computed once: the states from which a pursuer at the origin can force a collision within the
horizon.  In a scene with K other vehicles the set to stay out of is the union of that tube placed at each vehicle's pose,
    obstacle(x) = min_k tube(R(-theta_k) (x - p_k), heading - theta_k),
the shiftData / rotateData of helperOC applied K times and a chain of minima.  transformData does it in one launch of
resample_kernel: each node folds the K interpolated values in registers, and neither the K placed copies nor any coordinate array
exist in memory.  The union is then the obstacle of a reach-avoid solve on the same grid.

Nothing is asserted.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import resample

n = int(sys.argv[1]) if len(sys.argv) > 1 else 101
K = int(sys.argv[2]) if len(sys.argv) > 2 else 12
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731

g = lsp.createGrid(col([-6, -6, -np.pi]), col([6, 6, np.pi * (1 - 2.0 / n)]), col([n, n, n], np.int64), 2)
car = lsp.DubinsVehicleRel(g, 1, 1)
sd = lsp.Bundle(dict(grid=g, hamFunc=car.hamiltonian, partialFunc=car.dissipation, derivFunc=lsp.upwindFirstENO2))
quiet = dict(quiet=True, keepLast=True)

# ---- the tube, once: air3D's collision set of radius 0.6 grown backwards for 1.0
target = torch.as_tensor(np.asarray(lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 0.6)), device="cuda")
tube = lsp.HJIPDE_solve(target, np.array([0.0, 1.0]), sd, 'minVOverTime', lsp.Bundle(quiet))[0]

# ---- K poses on a circle of radius 3.5, each heading along the circle: y = R(-theta) (x - p), heading - theta
angles = np.linspace(0.0, 2 * np.pi, K, endpoint=False)
A, _ = resample.rotateMap(g, angles + np.pi / 2, (0, 1), 2)
p = 3.5 * np.stack([np.cos(angles), np.sin(angles)], axis=1)
b = np.zeros((K, 3))
b[:, :2] = -np.einsum('kij,kj->ki', A[:, :2, :2], p)
b[:, 2] = -(angles + np.pi / 2)

torch.cuda.synchronize()
start = time.time()
obstacle, info = lsp.transformData(g, tube, A=A, b=b, reduce='min', return_info=True)
torch.cuda.synchronize()
print("the tube on %s placed at %d poses and folded in %.4f s (%s); %d of %d nodes lie inside at least one placed grid"
      % (tuple(tube.shape), K, time.time() - start, resample.last_path(), int(info["counts"]), info["nodes"]))
cell = float(np.prod(np.asarray(g.dx).ravel()))
print("volume of one tube %.3f, of the union %.3f" % (cell * float((tube <= 0).sum()), cell * float((obstacle <= 0).sum())))

# ---- a reach-avoid solve with the union as its obstacle: reach the disc at the origin without entering any placed tube
goal = torch.as_tensor(np.asarray(lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 1.0)), device="cuda")
free = lsp.HJIPDE_solve(goal, np.array([0.0, 1.5]), sd, 'minVOverTime', lsp.Bundle(quiet))[0]
avoid = lsp.HJIPDE_solve(goal, np.array([0.0, 1.5]), sd, 'minVOverTime', lsp.Bundle(dict(quiet, obstacleFunction=obstacle)))[0]
print("reach set after 1.5: volume %.3f without obstacles, %.3f with the %d placed tubes" % (cell * float((free <= 0).sum()), cell * float((avoid <= 0).sum()), K))
