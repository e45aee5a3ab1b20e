#!/usr/bin/env python3
"""The least-restrictive safety filter on the planar quadrotor: filtered rollouts of a plant registered at run time, in ONE launch.

    python examples/quadrotor_safety.py [n] [horizon] [M]

The system and the solve of examples/quadrotor_rollout.py: state (x, vx, z, vz, phi, omega), thrusts T1, T2 in [0, Tmax], the reach tube of
a hover region solved fused.  The filter keeps the vehicle inside that tube (from there the hover region can still be reached): a nominal
pilot holds the hover thrust m g / 2 on both rotors while V(x) is below `level` by more than `margin`, and the value function's optimal
thrusts take over once the margin is used up.  No precompiled filter kernel serves a registered plant; with extraArgs.plantKernel=True
computeSafeTrajs has libhj_plant.so compile user_filtered_rollout_kernel around the registered statements (hipRTC, on first use) and runs
every state in one launch, and computeStochTrajs does the same with user_noisy_rollout_kernel.  The script prints the paths, the
interventions and the statuses, filtered against unfiltered, and the Monte Carlo check of a noisy version.  Nothing is asserted.

Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import hidim, montecarlo, safety
from levelsetpy_amd.dynamics import _rk4

n = int(sys.argv[1]) if len(sys.argv) > 1 else 11
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 0.2
M = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
nphi, nt = 16, 5
m, I, l, Cv, Cphi, g, Tmax = 1.3, 0.15, 0.25, 0.4, 0.02, 9.81, 9.0
params = [m, I, l, Cv, Cphi, g, Tmax, -1.0]             # the last one: -1, the thrusts MINIMISE the value (they steer into the target)
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731

QuadHam = lsp.register_hidim_hamiltonian("planar_quad", 6, '''
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

# The plant: the thrusts that optimise p . f -- T1 multiplies kp, T2 multiplies km -- switched through sgn, so that a NaN costate (a state
# that left the grid) gives NaN thrusts; then f.  One operation per statement where the Python methods below have one.
QuadPlant = lsp.register_plant("planar_quad", 6, controls_src='''
    const double cs = cos(x[4]);
    const double sn = sin(x[4]);
    const double k = (p[3] * cs - p[1] * sn) / par[0];
    const double r = p[5] * par[2] / par[1];
    const double sp = sgn(k + r);
    const double sm = sgn(k - r);
    u[0] = 0.5 * par[6] * (u_max ? 1.0 + sp : 1.0 - sp);
    u[1] = 0.5 * par[6] * (u_max ? 1.0 + sm : 1.0 - sm);
''', dynamics_src='''
    const double cvm = par[3] / par[0], cpi = par[4] / par[1];
    const double tm = (u[0] + u[1]) / par[0];
    dx[0] = x[1];
    dx[1] = -(cvm * x[1]) - tm * sin(x[4]);
    dx[2] = x[3];
    dx[3] = tm * cos(x[4]) - (cvm * x[3] + par[5]);
    dx[4] = x[5];
    dx[5] = par[2] * (u[0] - u[1]) / par[1] - cpi * x[5];
''', ncontrols=2, nparams=8)
QuadPlant.check("ENO2", "float64")                          # a mistake in either text would be reported here, as planar_quad:line


def sgn(s):
    return 1.0 if s >= 0 else (-1.0 if s < 0 else float("nan"))


class Quadrotor(object):
    """The user's own class: the solver's callbacks and computeOptTraj's dynSys protocol, in Python."""
    x = None

    def __init__(self, grid, params):
        self.grid, self.params = grid, list(params)

    def _coef(self, like):
        vs = [np.asarray(v, dtype=np.float64).ravel() for v in self.grid.vs]
        shp = lambda d: [-1 if k == d else 1 for k in range(6)]      # noqa: E731
        c = [vs[1].reshape(shp(1)), vs[3].reshape(shp(3)), vs[5].reshape(shp(5)), np.sin(vs[4]).reshape(shp(4)), np.cos(vs[4]).reshape(shp(4))]
        return [torch.as_tensor(a, dtype=like.dtype, device=like.device) for a in c] if torch.is_tensor(like) else c

    def hamiltonian(self, t, data, p, sd=None):
        m, I, l, Cv, Cphi, g, Tmax, s = self.params
        vx, vz, w, sn, cs = self._coef(p[0])
        k, r = (p[3] * cs - p[1] * sn) / m, p[5] * l / I
        opt = (lambda v: v.clamp(max=0) if torch.is_tensor(v) else np.minimum(v, 0)) if s < 0 else (lambda v: v.clamp(min=0) if torch.is_tensor(v) else np.maximum(v, 0))
        return (p[0] * vx - p[1] * (Cv / m * vx) + p[2] * vz - p[3] * (Cv / m * vz + g) + p[4] * w - p[5] * (Cphi / I * w)
                + Tmax * opt(k + r) + Tmax * opt(k - r))

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        m, I, l, Cv, Cphi, g, Tmax, s = self.params
        vx, vz, w, sn, cs = self._coef(data)
        return [abs(vx), abs(Cv / m * vx) + 2 * Tmax / m * abs(sn), abs(vz), abs(Cv / m * vz + g) + 2 * Tmax / m * abs(cs), abs(w),
                abs(Cphi / I * w) + l * Tmax / I][dim]

    def get_opt_u(self, t, p, uMode, x):
        m, I, l, Cv, Cphi, g, Tmax, s = self.params
        k, r = (p[3] * np.cos(x[4]) - p[1] * np.sin(x[4])) / m, p[5] * l / I
        sp, sm = sgn(k + r), sgn(k - r)
        return (0.5 * Tmax * (1.0 + sp), 0.5 * Tmax * (1.0 + sm)) if uMode == 'max' else (0.5 * Tmax * (1.0 - sp), 0.5 * Tmax * (1.0 - sm))

    def get_opt_v(self, t, p, dMode, x):
        return None

    def dynamics(self, t, x, u, d=None):
        m, I, l, Cv, Cphi, g, Tmax, s = self.params
        tm = (u[0] + u[1]) / m
        return np.array([x[1], -(Cv / m * x[1]) - tm * np.sin(x[4]), x[3], tm * np.cos(x[4]) - (Cv / m * x[3] + g), x[5],
                         l * (u[0] - u[1]) / I - Cphi / I * x[5]])

    def update_state(self, u, dt, x, d=None):
        self.x = _rk4(lambda z: self.dynamics(None, z, u), x, dt)
        return self.x


top = 2 * np.pi * (1 - 1.0 / nphi)
grid = lsp.createGrid(col([-2, -3, -2, -3, 0, -4]), col([2, 3, 2, 3, top, 4]), col([n, n, n, n, nphi, n], np.int64), [4], low_mem=True)
phi = np.asarray(grid.vs[4], dtype=np.float64).ravel()
quad = Quadrotor(grid, params)
QuadHam.attach(quad, params=lambda q: q.params, tables=[np.sin(phi), np.cos(phi)])      # it solves fused ...
QuadPlant.attach(quad, params=lambda q: q.params)                                        # ... and rolls out fused

shape = tuple(int(v) for v in np.asarray(grid.N).ravel())
ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in grid.vs]
X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
# the target: hovering near the origin -- a ball in position and velocity, any attitude
data0 = ((X[0] ** 2 + X[2] ** 2 + 0.25 * (X[1] ** 2 + X[3] ** 2)).sqrt() - 0.7).expand(shape).contiguous()
tau = np.linspace(0.0, horizon, nt)
sd = lsp.Bundle(dict(grid=grid, hamFunc=quad.hamiltonian, partialFunc=quad.dissipation, derivFunc=lsp.upwindFirstENO2))
t0 = time.time()
V, _, outs = lsp.HJIPDE_solve(data0, tau, sd, 'minVOverTime', lsp.Bundle(dict(quiet=True, flipOutput=True)))
torch.cuda.synchronize()
V = torch.as_tensor(V, device="cuda") if not torch.is_tensor(V) else V
print("solved: %s = %.3g cells, %d stored sets to t = %.2f in %.2f s, path %s" % (shape, float(np.prod(shape)), nt, horizon, time.time() - t0, hidim.last_path()))
print("  reach set: %.1f %% of the nodes (target: %.1f %%)" % (100 * float((V[0] <= 0).double().mean()), 100 * float((V[-1] <= 0).double().mean())))
# M states around the target: positions within 1.5, small velocities, any attitude within 0.5 rad of level
rng = np.random.default_rng(0)
x0 = np.zeros((M, 6))
x0[:, [0, 2]] = 3.0 * (rng.random((M, 2)) - 0.5)
x0[:, [1, 3]] = 1.0 * (rng.random((M, 2)) - 0.5)
x0[:, 4] = (1.0 * (rng.random(M) - 0.5)) % (2 * np.pi)
x0[:, 5] = 1.0 * (rng.random(M) - 0.5)
x0_t = torch.as_tensor(x0, device="cuda")
hover = torch.full((nt - 1, 2), 0.5 * m * g, dtype=torch.float64, device="cuda")          # the nominal pilot: both rotors at m g / 2
for kind in ("filtered", "decide", "noisy"):
    QuadPlant.check("ENO2", "float64", kind)                # the three kernels of extraArgs.plantKernel compile (no launch yet)
for label, margin in (("unfiltered (margin -inf: the pilot alone)", -np.inf), ("filtered, margin 0.1", 0.1), ("filtered, again", 0.1)):
    args = lsp.Bundle(dict(uMode='min', subSamples=4, derivFunc=lsp.upwindFirstENO2, level=0.0, margin=margin, keepTrajs=False, plantKernel=True))
    torch.cuda.synchronize()
    t0 = time.time()
    outs = lsp.computeSafeTrajs(grid, V, tau, quad, x0_t, hover, args)
    torch.cuda.synchronize()
    st = outs.status.cpu().numpy()
    print("%s: %d states in %.4f s, path %s" % (label, M, time.time() - t0, safety.last_path()))
    print("  safe %d, violated %d, left the grid %d; %d states saw an intervention, %.1f acting sub-steps a state of %d"
          % (int((st == lsp.safety.SAFE).sum()), int((st == lsp.safety.VIOLATED).sum()), int((st == lsp.safety.LEFT_GRID).sum()),
             int((outs.interventions > 0).sum()), float(outs.interventions.double().mean()), (nt - 1) * 4))
dec = lsp.safeControls(grid, V[0], quad, x0_t[:8], hover[0], lsp.Bundle(dict(uMode='min', derivFunc=lsp.upwindFirstENO2, margin=0.1, plantKernel=True)))
print("the decision at 8 states (%s): active %s" % (safety.last_path(), dec.active.cpu().numpy().astype(int).tolist()))
print("  thrusts", np.round(dec.controls.cpu().numpy(), 3).tolist())
# the same tube under noise: 16 realisations a state with the optimal thrusts throughout
mc = lsp.computeStochTrajs(grid, V, tau, quad, x0_t, 0.02 * np.eye(6), lsp.Bundle(dict(uMode='min', subSamples=4, derivFunc=lsp.upwindFirstENO2,
                                                                                        realisations=16, seed=1, plantKernel=True)))
prob, err = lsp.reachProbability(mc, 0.0, 'end')
print("Monte Carlo, 16 realisations a state, path %s: mean reach probability %.3f" % (montecarlo.last_path(), float(prob.mean())))
