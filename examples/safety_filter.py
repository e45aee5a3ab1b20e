#!/usr/bin/env python3
"""The least-restrictive safety filter: an evader that would rather fly straight, supervised by the air3D avoid tube.

    python examples/safety_filter.py [n] [states] [margin in grid spacings]

The small air3D problem (examples/air3d_brt.py) is solved once with every time slice stored; the stack stays on the GPU.  The
evader's nominal controller is "fly straight" (turn rate a = 0), the pursuer plays its worst case.  A few thousand relative states
ahead of the evader, each outside the tube by more than the margin plus one grid spacing, are rolled out twice in one launch each
(computeSafeTrajs, filtered_rollout_kernel): unfiltered (margin -inf: the nominal alone) and filtered (the value function's optimal
control takes over whenever V(x) - margin is used up).  Printed: the collisions of both runs and how often the filter stepped in.
safeControls then answers the runtime question for the start states: which control is applied right now?
Needs an MI355X (the package has no CPU fallback).  Nothing is asserted.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
states = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
spacings = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
radius, speed, turn = 0.5, 1.0, 1.0
dubins = lsp.DubinsVehicleRel(g, speed, turn)
schemeData = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation,
                             dissFunc=lsp.artificialDissipationGLF, CoStateCalc=lsp.upwindFirstWENO5))
tau = np.linspace(0, 2.0, 21)
stack, _, _ = lsp.HJIPDE_solve(lsp.shapeCylinder(g, 2, np.zeros((3, 1)), radius), tau, schemeData, 'minVOverTime',
                               lsp.Bundle(dict(quiet=True, flipOutput=True)))          # store-all, ordered for a rollout
V = torch.as_tensor(np.asarray(stack), device="cuda")

dx = float(np.asarray(g.dx).ravel()[0])
margin = spacings * dx
rng = np.random.default_rng(0)
lo, hi = np.array([0.7, -0.6, np.pi - 0.8]), np.array([2.8, 0.6, np.pi + 0.8])         # the pursuer ahead, roughly head-on
X = lo + rng.random((8 * states, 3)) * (hi - lo)
X[:, 2] = (X[:, 2] + np.pi) % (2 * np.pi) - np.pi
X = torch.as_tensor(X, device="cuda")
X = X[lsp.eval_u(g, V[0], X) - margin > dx][:states].contiguous()
M = int(X.shape[0])
straight = torch.zeros((len(tau) - 1, 1), dtype=torch.float64, device="cuda")

args = dict(uMode='max', dMode='min', subSamples=4, keepTrajs=False)
free = lsp.computeSafeTrajs(g, V, tau, dubins, X, straight, lsp.Bundle(dict(args, margin=-np.inf)))
safe = lsp.computeSafeTrajs(g, V, tau, dubins, X, straight, lsp.Bundle(dict(args, margin=margin)))
nsteps = (len(tau) - 1) * 4

print("grid %d^3, %d stored sets over %.1f s, %d start states with V - margin > one spacing (margin %.2f = %.2g spacings)"
      % (n, len(tau), tau[-1], M, margin, spacings))
print("kernel: %s" % safe.path)
for name, outs in (("flying straight", free), ("filtered       ", safe)):
    status = outs.status
    print("%s  collided %5d   stayed clear %5d   left the grid %4d   smallest V along the way %+.3f"
          % (name, int((status == 1).sum()), int((status == 0).sum()), int((status == 2).sum()), float(outs.gapMin[status != 2].min())))
acted = safe.interventions.to(torch.float64)
print("interventions per state: mean %.1f of %d sub-steps, %d states never touched, first one after %.2f s on average"
      % (float(acted.mean()), nsteps, int((safe.interventions == 0).sum()),
         float(safe.firstIntervention[safe.interventions > 0].to(torch.float64).mean()) * (tau[1] - tau[0]) / 4))

now = lsp.safeControls(g, V[0], dubins, X, torch.zeros((M, 1), dtype=torch.float64, device="cuda"),
                       lsp.Bundle(dict(uMode='max', dMode='min', margin=margin)))
print("right now the filter overrides %d of %d states; their applied turn rates: %s"
      % (int(now.active.sum()), M, sorted(set(now.controls[now.active][:, 0].tolist()))))
