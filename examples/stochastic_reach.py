#!/usr/bin/env python3
"""The air3D backward reachable tube (examples/air3d_brt.py) with and without noise on the relative dynamics.

    python examples/stochastic_reach.py [n] [t_end] [s]

With extraArgs.addGaussianNoiseStandardDeviation = sigma, HJIPDE_solve integrates
    phi_t + H(x, grad phi) = trace(sigma^T D^2phi sigma)
(no factor 1/2: for dx = f dt + s dW pass sigma = s / sqrt(2)).  Here the noise is independent per state, s on the two
positions and s / 2 on the heading -- a diagonal sigma, which runs as one fused launch per Runge-Kutta stage.  Needs an MI355X
(the package has no CPU fallback).  Prints which route ran and setVolume of both tubes.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 101
t_end = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
s = float(sys.argv[3]) if len(sys.argv) > 3 else 0.2

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
data0 = lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 0.5)
dubins = lsp.DubinsVehicleRel(g, 1, 1)
tau = np.linspace(0, t_end, 11)
sigma = np.diag([s, s, s / 2]) / np.sqrt(2)


def solve(extra):
    sd = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation, CoStateCalc=lsp.upwindFirstWENO5))
    t0 = time.perf_counter()
    tube, _, outs = lsp.HJIPDE_solve(data0, tau, sd, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True, **extra)))
    return tube, outs, time.perf_counter() - t0


plain, _, sec0 = solve({})
noisy, outs, sec1 = solve({'addGaussianNoiseStandardDeviation': sigma})
print("grid %d^3, t_end %.2f, s = %.3g" % (n, t_end, s))
print("route of the noisy solve: %s (%d time steps)" % (outs.path, int(np.sum(outs.steps))))
print("volume of the target set          %.5f" % lsp.setVolume(g, data0))
print("volume of the tube without noise  %.5f   (%.2f s)" % (lsp.setVolume(g, plain), sec0))
print("volume of the tube with noise     %.5f   (%.2f s)" % (lsp.setVolume(g, noisy), sec1))
print("largest change of the value function %.4f" % float(np.max(np.abs(np.asarray(noisy) - np.asarray(plain)))))
