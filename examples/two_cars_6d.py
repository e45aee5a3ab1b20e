#!/usr/bin/env python3
"""The pursuit game of two Dubins cars in ABSOLUTE coordinates, six dimensions, set against the 3-D relative solve.

    python examples/two_cars_6d.py [n] [horizon]

The reference's air3D game lives in the evader's frame: three states.  Code that needs both vehicles' absolute states (flocking, several
pairs that share obstacles) cannot use that frame, and the absolute game -- evader (x0, x1, x2), pursuer (x3, x4, x5) -- does not
decompose: the collision set couples the two.  DubinsPair6D solves it directly on a coarse 6-D grid (n nodes per position axis, default
13, about n^4 * 144 cells), one hjh_integrate call per tau interval.

Both games have the same value: with the change of coordinates
    r1 =  cos(x2) (x3 - x0) + sin(x2) (x4 - x1),   r2 = -sin(x2) (x3 - x0) + cos(x2) (x4 - x1),   r3 = x5 - x2
V6(x, t) = V3(r(x), t).  The script solves the 3-D game on a fine grid, evaluates it at the relative state of every 6-D node (eval_u, one
launch), and PRINTS the difference where the relative state lies inside the 3-D grid: what a coarse 6-D grid costs in accuracy.  Nothing
is asserted.

Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import hidim

n = int(sys.argv[1]) if len(sys.argv) > 1 else 13
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 0.4
nth = 12
speed, turn, radius = 1.0, 1.0, 0.8
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
top = 2 * np.pi * (1 - 1.0 / nth)

# ---- the 6-D absolute game
g6 = lsp.createGrid(col([-2, -2, 0, -2, -2, 0]), col([2, 2, top, 2, 2, top]), col([n, n, nth, n, n, nth], np.int64), [2, 5], low_mem=True)
pair = lsp.DubinsPair6D(g6, v_e=speed, v_p=speed, w_e=turn, w_p=turn)
ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g6.vs]
shape = tuple(int(v) for v in np.asarray(g6.N).ravel())
X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
data0 = (((X[0] - X[3]) ** 2 + (X[1] - X[4]) ** 2).sqrt() - radius).expand(shape).contiguous()
sd6 = lsp.Bundle(dict(grid=g6, hamFunc=pair.hamiltonian, partialFunc=pair.dissipation, derivFunc=lsp.upwindFirstENO2))
tau = np.array([0.0, horizon])
t0 = time.time()
V6, _, outs = lsp.HJIPDE_solve(data0, tau, sd6, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True)))
torch.cuda.synchronize()
print("6-D absolute game on %s = %.3g cells to t = %.2f: %.2f s, %s" % (shape, float(np.prod(shape)), horizon, time.time() - t0, outs.path))
print("  explain_plan: %s" % lsp.explain_plan(sd6))

# ---- the 3-D relative game on a fine grid that holds every relative position of the 6-D grid
n3 = 121
g3 = lsp.createGrid(col([-6, -6, 0]), col([6, 6, 2 * np.pi * (1 - 1.0 / 48)]), col([n3, n3, 48], np.int64), 2)
rel = lsp.DubinsVehicleRel(g3, u_bound=speed, w_bound=turn)
d3 = lsp.shapeCylinder(g3, 2, np.zeros((3, 1)), radius)
sd3 = lsp.Bundle(dict(grid=g3, hamFunc=rel.hamiltonian, partialFunc=rel.dissipation, derivFunc=lsp.upwindFirstENO2))
V3, _, _ = lsp.HJIPDE_solve(torch.as_tensor(d3, device="cuda"), tau, sd3, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True)))

# ---- V3 at the relative state of every 6-D node
dx, dy = (X[3] - X[0]).expand(shape), (X[4] - X[1]).expand(shape)
c, s = X[2].cos().expand(shape), X[2].sin().expand(shape)
r = torch.stack([(c * dx + s * dy).reshape(-1), (-s * dx + c * dy).reshape(-1), (X[5] - X[2]).expand(shape).reshape(-1)], dim=1).contiguous()
V3_at = lsp.eval_u(g3, V3, r).reshape(shape)
diff = (V6 - V3_at).abs()
inside = torch.isfinite(diff)
# the extrapolated position boundaries feed the 6-D solve where the collision set touches them (both cars in the same corner of the
# domain: the ghost cells continue a negative slope outwards); the relative grid is far larger and has no such nodes.  So: all nodes, and
# the nodes at least `margin` nodes away from every position boundary
margin = 3
keep = torch.ones(shape, dtype=torch.bool, device="cuda")
for d in (0, 1, 3, 4):
    idx = torch.arange(shape[d], device="cuda").reshape([shape[d] if k == d else 1 for k in range(6)])
    keep &= (idx >= margin) & (idx < shape[d] - margin)
print("3-D relative game on %s, evaluated at %d relative states (%d inside its grid)" % (tuple(int(v) for v in np.asarray(g3.N).ravel()), r.shape[0], int(inside.sum())))
for what, m in (("all nodes", inside), ("%d nodes from the position boundaries" % margin, inside & keep)):
    d = diff[m]
    print("  |V6 - V3 o r|, %s (%d): max %.3g, mean %.3g, median %.3g" % (what, d.numel(), float(d.max()), float(d.mean()), float(d.median())))
print("  (6-D position step %.3g, heading step %.3g rad)" % (float(np.asarray(g6.dx).ravel()[0]), float(np.asarray(g6.dx).ravel()[2])))
same_sign = ((V6 <= 0) == (V3_at <= 0))[inside].double().mean()
print("  the two agree on which side of the reachable tube a node lies for %.2f %% of the nodes" % (100 * float(same_sign)))
print("  last 5-D / 6-D path: %s" % hidim.last_path())
