#!/usr/bin/env python3
"""The planar quadrotor of examples/planar_quadrotor_6d.py written ONLY as NumPy-style callbacks, solved with the 5-D / 6-D tracer off and on.

    python examples/traced_quadrotor_6d.py [n] [horizon]

Nothing is registered and no device expression is written: hamFunc and partialFunc below are plain array code (NumPy arrays in, or device
tensors on the split path).  With set_hidim_trace(False), the default, such callbacks take the split path: 12 derivative arrays of the
grid's size and one torch expression after the other.  With set_hidim_trace(True) they are called once with symbolic arrays, written out as
a body for hidim_substep_kernel, compiled with hipRTC and checked once against the split path on the caller's data; np.sin(grid.xs[4]) and
np.cos(grid.xs[4]) become tables NumPy makes of grid.vs[4], so the kernel does no trigonometry per cell.  The script prints explain_plan,
both paths, the times and the largest difference.  Nothing is asserted.

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
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731


def like(a, ref):
    """A host array in the array type of `ref`: a device tensor on the split path, as it is otherwise (NumPy, or the tracer's stand-ins)."""
    return torch.as_tensor(np.ascontiguousarray(a), dtype=ref.dtype, device=ref.device) if torch.is_tensor(ref) else a


class Quadrotor(object):
    """State (x, vx, z, vz, phi, omega), thrusts T1, T2 in [0, Tmax] that minimise the value."""

    def __init__(self, grid, m=1.3, I=0.15, l=0.25, Cv=0.4, Cphi=0.02, g=9.81, Tmax=9.0):
        self.grid, self.m, self.I, self.l, self.Cv, self.Cphi, self.g, self.Tmax = grid, m, I, l, Cv, Cphi, g, Tmax

    def coef(self, ref):
        x = self.grid.xs
        return like(x[1], ref), like(x[3], ref), like(x[5], ref), like(np.sin(x[4]), ref), like(np.cos(x[4]), ref)

    def hamiltonian(self, t, data, p, sd=None):
        vx, vz, w, sn, cs = self.coef(p[0])
        k = (p[3] * cs - p[1] * sn) / self.m                 # what T1 + T2 multiplies
        r = p[5] * self.l / self.I                           # what T1 - T2 multiplies
        kp, km = k + r, k - r
        zero = 0 * kp
        opt = np.where(kp < 0, kp, zero) + np.where(km < 0, km, zero) if not torch.is_tensor(kp) else kp.clamp(max=0) + km.clamp(max=0)
        cvm, cpi = self.Cv / self.m, self.Cphi / self.I
        return (p[0] * vx - p[1] * (cvm * vx) + p[2] * vz - p[3] * (cvm * vz + self.g) + p[4] * w - p[5] * (cpi * w) + self.Tmax * opt)

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        vx, vz, w, sn, cs = self.coef(data)
        cvm, cpi, tmm = self.Cv / self.m, self.Cphi / self.I, 2 * self.Tmax / self.m
        return [abs(vx), abs(cvm * vx) + tmm * abs(sn), abs(vz), abs(cvm * vz + self.g) + tmm * abs(cs), abs(w),
                abs(cpi * w) + self.l * self.Tmax / self.I][dim]


top = 2 * np.pi * (1 - 1.0 / nphi)
grid = lsp.createGrid(col([-2, -3, -2, -3, 0, -4]), col([2, 3, 2, 3, top, 4]), col([n, n, n, n, nphi, n], np.int64), [4], low_mem=True)
quad = Quadrotor(grid)
shape = tuple(int(v) for v in np.asarray(grid.N).ravel())
ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in grid.vs]
X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
data0 = ((X[0] ** 2 + X[2] ** 2 + 0.25 * (X[1] ** 2 + X[3] ** 2)).sqrt() - 0.7).expand(shape).contiguous()
tau = np.array([0.0, horizon])
args = lsp.Bundle(dict(quiet=True, keepLast=True))


def scheme_data():
    return lsp.Bundle(dict(grid=grid, hamFunc=quad.hamiltonian, partialFunc=quad.dissipation, dissFunc=lsp.artificialDissipationGLF,
                           derivFunc=lsp.upwindFirstENO2))


def run(label):
    sd = scheme_data()
    t0 = time.time()
    V, _, outs = lsp.HJIPDE_solve(data0, tau, sd, 'minVOverTime', args)
    torch.cuda.synchronize()
    print("%s: %s = %.3g cells to t = %.2f in %.2f s\n  path %s" % (label, shape, float(np.prod(shape)), horizon, time.time() - t0, outs.path))
    return V, sd


lsp.set_hidim_trace(False)
print("switch off, explain_plan: %s" % lsp.explain_plan(scheme_data()))
Vs, _ = run("switch off")
lsp.set_hidim_trace(True)
V, sd = run("switch on, first solve (traces, compiles or loads the kernel, checks it against the split path once)")
V, sd = run("switch on, again")
e = lsp.explain_plan(sd)
print("switch on, explain_plan: path %(path)s, library %(library)s, ham_id %(ham_id)d, verified %(verified)s in %(verified_dtypes)s" % e)
print("  params %s\n  tables along axes %s, hoisted %s\n  source:\n    %s" % (e["params"], e["aux_axes"], e["hoisted"], e["source"].replace("\n", "\n    ")))
print("last_path(): %s" % hidim.last_path())
print("reach set: %.1f %% of the nodes (target: %.1f %%)" % (100 * float((V <= 0).double().mean()), 100 * float((data0 <= 0).double().mean())))
print("max |switch on - switch off| = %.3g" % float((V - Vs).abs().max()))
