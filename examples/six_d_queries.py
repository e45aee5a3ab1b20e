#!/usr/bin/env python3
"""What a caller does with a 6-D value function: project it, slice it, mesh the slice, roll out joint states.

    python examples/six_d_queries.py [n] [horizon] [M]

The pursuit game of examples/two_cars_6d.py -- two Dubins cars in absolute coordinates, evader (x0, x1, x2), pursuer
(x3, x4, x5) -- solved on a coarse grid (n nodes per position axis, default 13, 12 per heading) in store-all mode.  Then

  1. the reachable tube projected onto the evader's position plane: proj with 'min' over the other four axes (one launch of
     hi_project_minmax_kernel), and how much of the plane it covers;
  2. the slice at one pursuer state: proj with a point (hi_interp_points_kernel), a 3-D array on the evader's (x, y, heading)
     grid, meshed by extract_level_set -- a 6-D set is meshed by a projection or a slice to at most three axes first;
  3. the costate at a few joint states (eval_costate, hi_costate_points_kernel);
  4. M joint states (default 400) rolled out by computeOptTrajs in one launch of hi_rollout_kernel -- the evader maximises,
     the pursuer minimises --, and the capture statistics.

Nothing is asserted.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import rollout

n = int(sys.argv[1]) if len(sys.argv) > 1 else 13
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 0.6
M = int(sys.argv[3]) if len(sys.argv) > 3 else 400
nth = 12
speed, turn, radius = 1.0, 1.0, 0.8
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
top = 2 * np.pi * (1 - 1.0 / nth)

# ---- the 6-D absolute game, every time stamp kept
g6 = lsp.createGrid(col([-2, -2, 0, -2, -2, 0]), col([2, 2, top, 2, 2, top]), col([n, n, nth, n, n, nth], np.int64), [2, 5], low_mem=True)
pair = lsp.DubinsPair6D(g6, v_e=speed, v_p=speed, w_e=turn, w_p=turn)
ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g6.vs]
shape = tuple(int(v) for v in np.asarray(g6.N).ravel())
X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
data0 = (((X[0] - X[3]) ** 2 + (X[1] - X[4]) ** 2).sqrt() - radius).expand(shape).contiguous()
sd6 = lsp.Bundle(dict(grid=g6, hamFunc=pair.hamiltonian, partialFunc=pair.dissipation, derivFunc=lsp.upwindFirstENO2))
tau = np.linspace(0.0, horizon, 7)
t0 = time.time()
V, _, outs = lsp.HJIPDE_solve(data0, tau, sd6, 'minVOverTime', lsp.Bundle(dict(quiet=True)))
torch.cuda.synchronize()
print("6-D pursuit game on %s = %.3g cells, %d time stamps to t = %.2f: %.2f s, %s" % (shape, float(np.prod(shape)), len(tau), horizon, time.time() - t0, outs.path))
tube = V[-1]                                                 # the reachable tube of the whole horizon

# ---- 1. the tube on the evader's position plane
t0 = time.time()
gxy, on_plane = lsp.proj(g6, tube, [0, 0, 1, 1, 1, 1], 'min')
torch.cuda.synchronize()
print("1. min over heading and pursuer -> %s on the evader's position plane (%.1f ms): %.0f %% of the plane can be caught from some pursuer state; min %.3f"
      % (tuple(on_plane.shape), 1e3 * (time.time() - t0), 100 * float((on_plane <= 0).double().mean()), float(on_plane.min())))
_, worst = lsp.proj(g6, tube, [0, 0, 1, 1, 1, 1], 'max')
print("   max over the same axes: %.0f %% of the plane is caught from every pursuer state" % (100 * float((worst <= 0).double().mean())))

# ---- 2. the slice at one pursuer state, meshed
pursuer = [0.5, -0.25, np.pi / 2]
g3, cut = lsp.proj(g6, tube, [0, 0, 0, 1, 1, 1], pursuer)
mesh = lsp.extract_level_set(g3, cut, 0.0)
size, _ = lsp.level_set_measure(mesh.verts, mesh.faces)
print("2. slice at pursuer (%.2f, %.2f, %.2f): %s on the evader's grid; its zero level set: %d vertices, %d triangles, area %.3f"
      % (pursuer[0], pursuer[1], pursuer[2], tuple(cut.shape), mesh.verts.shape[0], mesh.faces.shape[0], float(size)))
stack3 = lsp.proj(g6, V, [0, 0, 0, 1, 1, 1], pursuer)[1]
inside = [(s <= 0).double().mean().item() for s in stack3]
print("   the same slice of every time stamp: inside fractions %s" % ", ".join("%.3f" % v for v in inside))

# ---- 3. costates at a few joint states
xs = np.array([[0.0, 0.0, 0.0, 1.0, 0.2, np.pi], [-0.5, 0.4, 1.0, 0.6, 0.9, 4.0], [1.0, -1.0, 2.0, 0.2, -0.6, 0.5]])
p = lsp.eval_costate(g6, tube, xs, lsp.upwindFirstENO2)
v = lsp.eval_u(g6, tube, xs)
for k in range(len(xs)):
    print("3. x = %s: V = %+.3f, grad V = %s" % (np.round(xs[k], 2).tolist(), float(v[k]), np.round(p[k].cpu().numpy(), 3).tolist()))

# ---- 4. many joint states in one launch
rng = np.random.default_rng(0)
x0 = np.column_stack([rng.uniform(-1.2, 1.2, M), rng.uniform(-1.2, 1.2, M), rng.uniform(0, 2 * np.pi, M),
                      rng.uniform(-1.2, 1.2, M), rng.uniform(-1.2, 1.2, M), rng.uniform(0, 2 * np.pi, M)])
flipped = torch.flip(V, dims=[0]).contiguous()               # index 0: the full horizon, the last index the target
args = lsp.Bundle(dict(uMode='max', dMode='min', subSamples=4, derivFunc=lsp.upwindFirstENO2, status=True))
t0 = time.time()
trajs, lengths, _, o = lsp.computeOptTrajs(g6, flipped, tau, pair, torch.as_tensor(x0, device="cuda"), args)
torch.cuda.synchronize()
print("4. %d joint states rolled out in %.1f ms by %s" % (M, 1e3 * (time.time() - t0), rollout.last_path()))
status, lengths = o.status.cpu().numpy(), lengths.cpu().numpy()
start = lsp.eval_u(g6, tube, x0).cpu().numpy()
caught = status == lsp.rollout.REACHED
print("   caught (reached the collision set): %d; escaped for the whole horizon: %d; left the grid: %d"
      % (int(caught.sum()), int((status == lsp.rollout.EXHAUSTED).sum()), int((status == lsp.rollout.LEFT_GRID).sum())))
print("   of the %d states that start inside the tube (V <= 0), %d are caught; of the %d outside, %d"
      % (int((start <= 0).sum()), int((caught & (start <= 0)).sum()), int((start > 0).sum()), int((caught & (start > 0)).sum())))
if caught.any():
    print("   time to capture of the caught: mean %.3f, max %.3f" % (float(tau[lengths[caught] - 1].mean()), float(tau[lengths[caught] - 1].max())))
last = trajs.cpu().numpy()[np.arange(M), :, lengths - 1]
dist = np.hypot(last[:, 0] - last[:, 3], last[:, 1] - last[:, 4])
ok = np.isfinite(dist)
print("   distance between the vehicles at the last recorded state: min %.3f, median %.3f (capture radius %.2f)" % (dist[ok].min(), np.median(dist[ok]), radius))
