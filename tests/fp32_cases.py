"""What tests/test_oracle_fp32.py (no device) and tests/test_gpu_fp32_exact.py share: the grids, the two data sets, the derived
rounding bounds and the references, each computed once and never written.

Grids: (9, 8), (13, 11, 9), (8, 7, 8, 7) -- distinct extents, more than one workgroup from 3-D on, totals that are no multiple of
256 -- each with every axis extrapolated and with the last axis periodic (one step short of the period).  The boxes are symmetric
about the origin, where the sphere sits.

Data, always rounded to float32 first (both precisions see the same numbers):
  "noisy"      signed distance to a sphere + 0.05 standard_normal (seed 1): next to no ENO selector ties
  "symmetric"  the sphere alone: a large share of the cells sits on exact or rounding-level ties of |D2| / |D3|

THE BOUND.  u = eps32 / 2 is the unit roundoff, M = max|data|, G = max|ghosted data|, A = G / dx.  On a periodic axis G = M; an
extrapolated ghost is edge + k (edge - inner) sign(..), k <= 3, so G <= M + 3 * 2M = 7M, formed with three roundings of
quantities <= G: a ghost carries an absolute error <= 3uG (interior cells none: both precisions read the same float32 data).
First-order error of what the float32 evaluation forms, fl(a o b) = (a o b)(1 + d), |d| <= u, each constant (1/dx, 0.5/dx,
(1/3)/dx, dx, dx^2, 2dx^2) one more relative u:
  D1 = K0 (v1 - v0)        |D1| <= 2A          error <= (2 * 3 + 2 + 2 + 2) uA                     = 12 uA
  D2 = K1 (D1b - D1a)      |D2| <= 2A/dx       error <= (2 * 12 + 3 * 4) uA / (2dx)                = 18 uA/dx
  D3 = K2 (D2b - D2a)      |D3| <= (4/3)A/dx^2 error <= (2 * 18 + 3 * 4) uA / (3dx^2)              = 16 uA/dx^2
  ENO2  L = D1 + dx D2     |dx D2| <= 2A, |L| <= 4A:  12 + 18 + 2 + 2 (constant, product) + 4 (sum) = 38 uA
  ENO3  L = (D1 + dx D2) + c D3, c <= 2dx^2, |c D3| <= (8/3)A:  38 + 2 * 16 + 2 * 8/3 + (4 + 8/3)    <= 83 uA
  as-shipped WENO5: its smoothness estimates are exact zeros in either precision (v - 2v + v and v - 4v + 3v cancel exactly), so it
        is sum w_k d_k / sum w_k over the three ENO3 candidates (|d_k| <= (20/3)A) with the weights rounded (u), divided by eps^2 (u),
        multiplied (u), summed (2u), the weight sum likewise (2u + 2u) and one division (u): 10u * (20/3)A <= 67 uA more = 150 uA
The same counts hold for R.  In the form C eps32 M / dx (u = eps32 / 2, A <= g M / dx with g = 1 periodic, 7 extrapolated):
  C = g * 19 (ENO2),  g * 41.5 (ENO3),  g * 75 (as-shipped WENO5).
Nothing here is fitted to what a restatement or a kernel gives.
"""
import numpy as np

from oracle import hj_oracle as O

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 64 * EPS32                    # ENO cells whose selector margin is below this are left out of the accuracy comparison ...
MAX_LEFT_OUT = 0.01                    # ... and may be at most this share per axis and scheme
C_SCHEME = {"ENO2": 19.0, "ENO3": 41.5, "WENO5_ASSHIPPED": 75.0}
GHOST_FACTOR = {"periodic": 1.0, "extrapolate": 7.0}

BOX = {2: ([-1.0, -1.5], [1.0, 1.5]), 3: ([-1.5, -1.25, -np.pi], [1.5, 1.25, np.pi]), 4: ([-np.pi, -2.0, -np.pi, -2.0], [np.pi, 2.0, np.pi, 2.0])}
SHAPE = {2: (9, 8), 3: (13, 11, 9), 4: (8, 7, 8, 7)}
RADIUS = {2: 0.45, 3: 0.5, 4: 1.5}
GRIDS = [(nd, per) for nd in (2, 3, 4) for per in (False, True)]
DATA_SETS = ("noisy", "symmetric")
OFN = {"ENO2": O.upwind_first_eno2, "ENO3": O.upwind_first_eno3,
       "WENO5_ASSHIPPED": lambda g, d, i: O.upwind_first_weno5(g, d, i, "asshipped"),
       "WENO5": lambda g, d, i: O.upwind_first_weno5(g, d, i, "weno5")}


def limits(nd, periodic):
    """(gmin, gmax, N, periodic axes): the last axis periodic, or none."""
    lo, hi = (list(v) for v in BOX[nd])
    N = list(SHAPE[nd])
    pd = [nd - 1] if periodic else []
    for d in pd:
        hi[d] = hi[d] - (hi[d] - lo[d]) / N[d]
    return lo, hi, N, pd


def bound(og, scheme, data, dim):
    """C eps32 max|data| / dx_dim of the module docstring."""
    return C_SCHEME[scheme] * GHOST_FACTOR[og.bc[dim]] * EPS32 * float(np.abs(data).max()) / og.dx.item(dim)


class Case(object):
    """One grid in both precisions, its data sets (float32) and the derivative references."""
    cache = {}

    def __init__(self, nd, periodic):
        lo, hi, N, pd = limits(nd, periodic)
        self.nd, self.periodic, self.lo, self.hi, self.N, self.pd = nd, periodic, lo, hi, N, pd
        self.og64 = O.Grid(lo, hi, N, pd)
        self.og32 = O.Grid(lo, hi, N, pd, dtype=np.float32)
        sphere = O.shape_sphere(self.og64, None, RADIUS[nd])
        rng = np.random.default_rng(1)
        self.data = {"noisy": (sphere + 0.05 * rng.standard_normal(self.og64.shape)).astype(np.float32), "symmetric": sphere.astype(np.float32)}
        self.start = {k: (v.astype(np.float64) + 0.03 * np.cos(2 * self.og64.xs[0])).astype(np.float32) for k, v in self.data.items()}     # y0 of the RK stages
        self._refs = {}

    @classmethod
    def get(cls, nd, periodic):
        if (nd, periodic) not in cls.cache:
            cls.cache[(nd, periodic)] = cls(nd, periodic)
        return cls.cache[(nd, periodic)]

    def og(self, prec):
        return self.og32 if prec == 32 else self.og64

    def values(self, what, prec, start=False):
        a = (self.start if start else self.data)[what]
        return a if prec == 32 else a.astype(np.float64)

    def deriv(self, what, scheme, prec):
        """[(derivL, derivR) per axis] of the oracle in fp64 or in its float32 mode, on the same float32 data."""
        key = ("deriv", what, scheme, prec)
        if key not in self._refs:
            self._refs[key] = [OFN[scheme](self.og(prec), self.values(what, prec), d) for d in range(self.nd)]
        return self._refs[key]

    def margin(self, what, scheme):
        """eno_selector_margin per axis, from the fp64 oracle."""
        key = ("margin", what, scheme)
        if key not in self._refs:
            self._refs[key] = [O.eno_selector_margin(self.og64, self.values(what, 64), d, scheme) for d in range(self.nd)]
        return self._refs[key]

    def system(self, prec, par=None):
        g = self.og(prec)
        if self.nd == 2:
            return O.DoubleIntegrator(g, *(par or (1.25,)))
        if self.nd == 3:
            return O.DubinsRel(g, *(par or (1, 1)))
        return O.DoublePendulum4D(g, *(par or (1.0,)))

    def term(self, what, scheme, prec, par=None):
        """(ydot, stepBound) of term_lax_friedrichs with the grid's built-in system."""
        key = ("term", what, scheme, prec, par)
        if key not in self._refs:
            yd, sb = O.term_lax_friedrichs(self.og(prec), self.system(prec, par), scheme, 0.0, self.values(what, prec).reshape(-1, 1))
            self._refs[key] = (yd.reshape(self.og64.shape), sb)
        return self._refs[key]


def within_bound(case, what, scheme, got, side, dim, masked):
    """`got` (derivL if side == 0, derivR if 1, along `dim`) against the fp64 oracle: every cell (masked=False) or every cell whose ENO
    selector margin is at least MARGIN within bound(); returns (largest error / bound, share of cells left out) for the message."""
    ref = case.deriv(what, scheme, 64)[dim][side]
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    keep = case.margin(what, scheme)[dim] >= MARGIN if masked else np.ones(ref.shape, dtype=bool)
    b = bound(case.og64, scheme, case.values(what, 64), dim)
    return float(err[keep].max()) / b, 1.0 - float(keep.mean())
