#!/usr/bin/env python3
"""A Monte Carlo check of a stochastic value function: E[l(x_T)] under the time-consistent policy against V(x0, 0).

    python examples/monte_carlo_reach.py [n] [t_end] [s] [realisations]

The air3D game of examples/stochastic_reach.py with noise s on the two positions and s / 2 on the heading, solved WITHOUT a
minimum over time (compMethod 'none'), so that V(x, t) = E[l(x_T)] under the optimal closed loop.  computeStochTrajs then rolls
out dx = f(x, u*, d*) dt + G dW from 16 states, G = sqrt(2) sigma, reading slice `it` of the stored stack at column `it` (policy
'clock'), one launch for all realisations.  Printed per state: the mean of valueEnd = l(x_T), its standard error, V[0](x0) and
their distance in standard errors; then reachProbability of the target at the end and along the path.  The two columns differ by
the discretisation of the solve (grid, dissipation) and of the rollout (Euler-Maruyama noise, controls held over a sub-step):
the gap is reported, not asserted.  A realisation that leaves the grid has no value and is left out of its state's mean.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 61
t_end = float(sys.argv[2]) if len(sys.argv) > 2 else 0.4
s = float(sys.argv[3]) if len(sys.argv) > 3 else 0.2
R = int(sys.argv[4]) if len(sys.argv) > 4 else 16384

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
data0 = lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 0.5)
dubins = lsp.DubinsVehicleRel(g, 1, 1)
tau = np.linspace(0, t_end, 11)
sigma = np.diag([s, s, s / 2]) / np.sqrt(2)

sd = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation, CoStateCalc=lsp.upwindFirstWENO5))
t0 = time.perf_counter()
stack, _, souts = lsp.HJIPDE_solve(data0, tau, sd, 'none', lsp.Bundle(dict(quiet=True, flipOutput=True,
                                                                          addGaussianNoiseStandardDeviation=sigma)))
stack = np.asarray(stack)                                      # time first, index 0 the full horizon, the last index the target function l
print("grid %d^3, t_end %.2f, s = %.3g: solved by %s in %.2f s" % (n, t_end, s, souts.path, time.perf_counter() - t0))

rng = np.random.default_rng(0)
# the relative state moves by up to about 3 t_end: states from which few realisations reach the grid's edge within the horizon
x0 = np.array([0.7, -0.3, -np.pi]) + rng.random((16, 3)) * np.array([1.0, 0.6, 2 * np.pi])
args = lsp.Bundle(dict(uMode='max', dMode='min', subSamples=4, realisations=R, seed=2026, policy='clock'))
t0 = time.perf_counter()
outs = lsp.computeStochTrajs(g, stack, tau, dubins, x0, sigma, args)
sec = time.perf_counter() - t0
print("%d states x %d realisations by %s in %.3f s (copies included)" % (len(x0), R, outs.path, sec))

v0 = np.asarray(lsp.eval_u(g, stack[0], x0))
# a realisation that left the grid has no value (NaN): it is counted in the last column and left out of the mean, which biases it
lost = np.isnan(outs.valueEnd).sum(axis=1)
kept = np.maximum(R - lost, 2)
total = np.nansum(outs.valueEnd, axis=1)
mean = np.where(lost < R, total / kept, np.nan)
se = np.sqrt(np.maximum(np.nansum(outs.valueEnd ** 2, axis=1) - kept * mean ** 2, 0.0) / (kept - 1) / kept)
p_end, e_end = lsp.reachProbability(outs, 0.0, 'end')
p_min, e_min = lsp.reachProbability(outs, 0.0, 'min')
print("   x0                        E[l(x_T)]   +-se      V[0](x0)   gap     gap/se   P(end in target)  P(path enters)  left grid")
for m in range(len(x0)):
    print("  (%5.2f, %5.2f, %5.2f)     %8.4f  %7.4f   %8.4f  %7.4f  %6.1f     %.4f +-%.4f   %.4f +-%.4f   %d"
          % (x0[m, 0], x0[m, 1], x0[m, 2], mean[m], se[m], v0[m], mean[m] - v0[m], (mean[m] - v0[m]) / se[m], p_end[m], e_end[m],
             p_min[m], e_min[m], lost[m]))
print("largest |E[l(x_T)] - V[0](x0)| over the states: %.4f (grid spacing %.4f)" % (float(np.nanmax(np.abs(mean - v0))), float(np.ravel(g.dx)[0])))
