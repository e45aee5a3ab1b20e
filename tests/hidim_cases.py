"""What tests/test_hidim_host.py and tests/test_gpu_hidim.py share: the two 5-D / 6-D systems restated in the oracle's style
(NumPy, the expressions of include/hj_hidim.h in its order), the grids and the data.  The trig factors are the grid's tables
(O.Grid.cos / sin: np.cos(xs[d]) in fp64, rounded once in the oracle's float32 mode, as hidim.py builds them).

Shapes: the smallest that still catch a wrong stride or decode -- distinct extents, more than one workgroup, a total that is no
multiple of 256, a last axis shorter than a wave; and one whose last axis holds a whole wave inside one row.  Each periodic
axis ends one step short of 2 pi.

Data: a distorted sphere in the position axes, plus 0.05 sin(3 x_0) cos(2 x_last), plus 0.02 standard_normal from a fixed seed.
The noise matters: symmetric data puts 60-80 % of the cells on exact ENO selector ties (oracle.eno_selector_margin); with it
the fraction is 0 to 4e-5.
"""
import numpy as np

from oracle import hj_oracle as O

SHAPES = {
    "plane5d": ((7, 6, 8, 5, 9), [2]),
    "pair6d": ((6, 5, 7, 5, 6, 8), [2, 5]),
    "plane5d_long": ((5, 5, 6, 5, 70), [2]),
}
TWO_PI = 2 * np.pi


class Plane5D(object):
    """H = p0 (x3 cos x2) + p1 (x3 sin x2) + p2 x4 + s (a_max |p3|) + s (alpha_max |p4|), left to right."""

    def __init__(self, grid, a_max=1.0, alpha_max=1.0, u_mode='min'):
        self.grid, self.a_max, self.alpha_max = grid, a_max, alpha_max
        self.s = -1.0 if u_mode == 'min' else 1.0

    def hamiltonian(self, t, data, p, sd=None):
        x = self.grid.xs
        return (p[0] * (x[3] * self.grid.cos(2)) + p[1] * (x[3] * self.grid.sin(2)) + p[2] * x[4] + self.s * (self.a_max * np.abs(p[3]))
                + self.s * (self.alpha_max * np.abs(p[4])))

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        x = self.grid.xs
        if dim == 0:
            return np.abs(x[3] * self.grid.cos(2))
        if dim == 1:
            return np.abs(x[3] * self.grid.sin(2))
        if dim == 2:
            return np.abs(x[4])
        return self.a_max if dim == 3 else self.alpha_max


class DubinsPair6D(object):
    """H = -( p0 (v_e cos x2) + p1 (v_e sin x2) + p3 (v_p cos x5) + p4 (v_p sin x5) + w_e |p2| - w_p |p5| ), left to right."""

    def __init__(self, grid, v_e=5, v_p=5, w_e=5, w_p=5):
        self.grid, self.v_e, self.v_p, self.w_e, self.w_p = grid, v_e, v_p, w_e, w_p

    def hamiltonian(self, t, data, p, sd=None):
        x = self.grid.xs
        return -(p[0] * (self.v_e * self.grid.cos(2)) + p[1] * (self.v_e * self.grid.sin(2)) + p[3] * (self.v_p * self.grid.cos(5))
                 + p[4] * (self.v_p * self.grid.sin(5)) + self.w_e * np.abs(p[2]) - self.w_p * np.abs(p[5]))

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        x = self.grid.xs
        if dim == 0:
            return np.abs(self.v_e * self.grid.cos(2))
        if dim == 1:
            return np.abs(self.v_e * self.grid.sin(2))
        if dim == 3:
            return np.abs(self.v_p * self.grid.cos(5))
        if dim == 4:
            return np.abs(self.v_p * self.grid.sin(5))
        return self.w_e if dim == 2 else self.w_p


def limits(name):
    """(gmin, gmax, N, periodic axes) of a case."""
    N, pd = SHAPES[name]
    if len(N) == 5:
        gmin, gmax = [-2.0, -2.2, 0.0, 0.5, -1.0], [2.1, 2.0, TWO_PI, 2.0, 1.2]
    else:
        gmin, gmax = [-2.0, -2.2, 0.0, -2.1, -1.9, 0.0], [2.1, 2.0, TWO_PI, 1.9, 2.2, TWO_PI]
    for d in pd:
        gmax[d] = TWO_PI * (1.0 - 1.0 / N[d])
    return gmin, gmax, list(N), list(pd)


def oracle_grid(name):
    gmin, gmax, N, pd = limits(name)
    return O.Grid(gmin, gmax, N, pd)


def oracle_system(name, og, **kw):
    return (Plane5D if og.dim == 5 else DubinsPair6D)(og, **kw)


def data(og, seed=7):
    x = og.xs
    if og.dim == 5:
        base = np.sqrt(x[0] ** 2 + 1.2 * x[1] ** 2 + 0.01) - 1
    else:
        base = np.sqrt((x[0] - x[3]) ** 2 + (x[1] - x[4]) ** 2 + 0.01) - 1
    rng = np.random.default_rng(seed)
    return base + 0.05 * np.sin(3 * x[0]) * np.cos(2 * x[-1]) + 0.02 * rng.standard_normal(og.shape)


PARAMS = {"plane5d": dict(a_max=0.8, alpha_max=1.3, u_mode='min'), "pair6d": dict(v_e=1.5, v_p=1.1, w_e=0.9, w_p=1.4),
          "plane5d_long": dict(a_max=0.8, alpha_max=1.3, u_mode='max')}
