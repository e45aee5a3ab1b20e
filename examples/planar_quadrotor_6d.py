#!/usr/bin/env python3
"""A small backward reach set of a planar quadrotor, six dimensions, solved FUSED through a Hamiltonian registered at run time.

    python examples/planar_quadrotor_6d.py [n] [horizon]

State (x, vx, z, vz, phi, omega), two rotors with thrusts T1, T2 in [0, Tmax] at arm length l:
    xdot = vx,  vxdot = -(Cv/m) vx - (T1 + T2) sin(phi) / m,   zdot = vz,  vzdot = -(Cv/m) vz - g + (T1 + T2) cos(phi) / m,
    phidot = omega,  omegadot = -(Cphi/I) omega + l (T1 - T2) / I
No built-in kernel serves it.  register_hidim_hamiltonian takes H and alpha once as a device expression (sin phi and cos phi from tables
NumPy makes of grid.vs[4]); hidim_substep_kernel is compiled around it with hipRTC on first use, and HJIPDE_solve then runs a whole tau
interval in one native call, one launch per Runge-Kutta stage, with no derivative arrays.  Without the registration the same callbacks take
the split path: 12 derivative arrays of the grid's size and one torch expression after the other.  The script solves a coarse grid both
ways and prints the paths, the times and the largest difference.  Nothing is asserted.

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
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 0.1
nphi = 16
m, I, l, Cv, Cphi, g, Tmax = 1.3, 0.15, 0.25, 0.4, 0.02, 9.81, 9.0
params = [m, I, l, Cv, Cphi, g, Tmax, -1.0]             # the last one: -1, the thrusts MINIMISE the value (they steer into the target)
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731

Quad = lsp.register_hidim_hamiltonian("planar_quad", 6, '''
    const T sn = aux[0], cs = aux[1];                       // sin(phi), cos(phi) of this cell, from the caller's tables
    const T cvm = par[3] / par[0], cpi = par[4] / par[1];
    const T k = (p[3] * cs - p[1] * sn) / par[0];           // what T1 + T2 multiplies
    const T r = p[5] * par[2] / par[1];                     // what T1 - T2 multiplies
    const T kp = k + r, km = k - r;                         // the coefficients of T1 and T2
    const T op = par[7] < T(0) ? fmin(kp, T(0)) : fmax(kp, T(0));
    const T om = par[7] < T(0) ? fmin(km, T(0)) : fmax(km, T(0));
    H = p[0] * x[1] - p[1] * (cvm * x[1]) + p[2] * x[3] - p[3] * (cvm * x[3] + par[5]) + p[4] * x[5] - p[5] * (cpi * x[5])
        + par[6] * op + par[6] * om;
    const T tmm = T(2) * par[6] / par[0];
    alpha[0] = fabs(x[1]);  alpha[1] = fabs(cvm * x[1]) + tmm * fabs(sn);
    alpha[2] = fabs(x[3]);  alpha[3] = fabs(cvm * x[3] + par[5]) + tmm * fabs(cs);
    alpha[4] = fabs(x[5]);  alpha[5] = fabs(cpi * x[5]) + par[2] * par[6] / par[1];
''', nparams=8, aux_axes=(4, 4))
Quad.check("ENO2", "float64")                               # a mistake in the text would be reported here, as planar_quad:line


def _coef(self, like):
    """vx, vz, omega, sin phi, cos phi, broadcastable against the grid, in the array type of `like`."""
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in self.grid.vs]
    shp = lambda d: [-1 if k == d else 1 for k in range(6)]      # noqa: E731
    c = [vs[1].reshape(shp(1)), vs[3].reshape(shp(3)), vs[5].reshape(shp(5)), np.sin(vs[4]).reshape(shp(4)), np.cos(vs[4]).reshape(shp(4))]
    return [torch.as_tensor(a, dtype=like.dtype, device=like.device) for a in c] if torch.is_tensor(like) else c


def py_ham(self, t, data, p, sd=None):
    m, I, l, Cv, Cphi, g, Tmax, s = self.params
    vx, vz, w, sn, cs = _coef(self, p[0])
    k, r = (p[3] * cs - p[1] * sn) / m, p[5] * l / I
    opt = (lambda v: v.clamp(max=0) if torch.is_tensor(v) else np.minimum(v, 0)) if s < 0 else (lambda v: v.clamp(min=0) if torch.is_tensor(v) else np.maximum(v, 0))
    return (p[0] * vx - p[1] * (Cv / m * vx) + p[2] * vz - p[3] * (Cv / m * vz + g) + p[4] * w - p[5] * (Cphi / I * w)
            + Tmax * opt(k + r) + Tmax * opt(k - r))


def py_diss(self, t, data, derivMin, derivMax, sd, dim):
    m, I, l, Cv, Cphi, g, Tmax, s = self.params
    vx, vz, w, sn, cs = _coef(self, data)
    return [abs(vx), abs(Cv / m * vx) + 2 * Tmax / m * abs(sn), abs(vz), abs(Cv / m * vz + g) + 2 * Tmax / m * abs(cs), abs(w),
            abs(Cphi / I * w) + l * Tmax / I][dim]


top = 2 * np.pi * (1 - 1.0 / nphi)
grid = lsp.createGrid(col([-2, -3, -2, -3, 0, -4]), col([2, 3, 2, 3, top, 4]), col([n, n, n, n, nphi, n], np.int64), [4], low_mem=True)
phi = np.asarray(grid.vs[4], dtype=np.float64).ravel()
quad = Quad(grid, params, tables=[np.sin(phi), np.cos(phi)], hamiltonian=py_ham, dissipation=py_diss)

shape = tuple(int(v) for v in np.asarray(grid.N).ravel())
ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in grid.vs]
X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
# the target: hovering near the origin -- a ball in position and velocity, any attitude
data0 = ((X[0] ** 2 + X[2] ** 2 + 0.25 * (X[1] ** 2 + X[3] ** 2)).sqrt() - 0.7).expand(shape).contiguous()
tau = np.array([0.0, horizon])
args = lsp.Bundle(dict(quiet=True, keepLast=True))

sd = lsp.Bundle(dict(grid=grid, hamFunc=quad.hamiltonian, partialFunc=quad.dissipation, derivFunc=lsp.upwindFirstENO2))
print("explain_plan: %s" % lsp.explain_plan(lsp.Bundle(dict(sd.__dict__, dissFunc=lsp.artificialDissipationGLF))))
t0 = time.time()
V, _, outs = lsp.HJIPDE_solve(data0, tau, sd, 'minVOverTime', args)
torch.cuda.synchronize()
print("registered: %s = %.3g cells to t = %.2f in %.2f s (the first run compiles or loads the kernel), path %s"
      % (shape, float(np.prod(shape)), horizon, time.time() - t0, hidim.last_path()))
t0 = time.time()
V, _, outs = lsp.HJIPDE_solve(data0, tau, sd, 'minVOverTime', args)
torch.cuda.synchronize()
t_fused = time.time() - t0
print("registered, again: %.2f s, path %s" % (t_fused, outs.path))
print("  reach set: %.1f %% of the nodes (target: %.1f %%)" % (100 * float((V <= 0).double().mean()), 100 * float((data0 <= 0).double().mean())))

# the same callbacks handed over unregistered: the split path
plain = lsp.Bundle(dict(grid=grid, hamFunc=lambda *a: quad.hamiltonian(*a), partialFunc=lambda *a: quad.dissipation(*a), derivFunc=lsp.upwindFirstENO2))
t0 = time.time()
Vs, _, outs = lsp.HJIPDE_solve(data0, tau, plain, 'minVOverTime', args)
torch.cuda.synchronize()
t_split = time.time() - t0
print("unregistered: %.2f s (%.1fx), path %s" % (t_split, t_split / t_fused, hidim.last_path()))
print("  max |registered - unregistered| = %.3g (the expression above contracts and orders its sums as C++ does, the callbacks as NumPy does)"
      % float((V - Vs).abs().max()))
