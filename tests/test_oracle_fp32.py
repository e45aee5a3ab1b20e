"""The float32 mode of the NumPy oracle (oracle/hj_oracle.py, "WORKING PRECISION"), no device: what it returns is float32
throughout, and it agrees with the fp64 oracle on the same float32-rounded data within the rounding bound DERIVED in
tests/fp32_cases.py (C eps32 max|data| / dx: operation counts and coefficient sums of the stencils, nothing fitted):
  as-shipped WENO5  derivL / derivR on every cell;
  ENO2 / ENO3       on every cell whose eno_selector_margin is at least 64 eps32 -- at most 1 % of the cells per axis and scheme may
                    be left out (a condition of the test).
On the symmetric sphere only the WENO5 bound and the types are asserted, and that at least 5 % of the ENO3 cells are below the
margin: the data on which tests/test_gpu_fp32_exact.py's bitwise comparisons mean something."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import hj_oracle as O  # noqa: E402
import fp32_cases as F  # noqa: E402
import hidim_cases as HC  # noqa: E402

IDS = ["%dd-%s" % (nd, "periodic" if per else "extrapolated") for nd, per in F.GRIDS]


def all_float32(x, what):
    """Every array in x (nested lists / tuples / dicts) is float32; scalars are host values (Python floats)."""
    if isinstance(x, (list, tuple)):
        for a in x:
            all_float32(a, what)
    elif isinstance(x, dict):
        for k, a in x.items():
            all_float32(a, "%s[%s]" % (what, k))
    elif isinstance(x, np.ndarray):
        assert x.dtype == np.float32, (what, x.dtype)
    else:
        assert isinstance(x, float) and not isinstance(x, np.floating), (what, type(x))


@pytest.mark.parametrize("what", F.DATA_SETS)
@pytest.mark.parametrize("nd,per", F.GRIDS, ids=IDS)
def test_every_array_of_the_float32_mode_is_float32(nd, per, what):
    c = F.Case.get(nd, per)
    g, data = c.og32, c.values(what, 32)
    all_float32(g.vs, "vs"), all_float32(g.xs, "xs"), all_float32([g.cos(nd - 1), g.sin(0)], "trig tables")
    assert g.dx.dtype == np.float64                       # host values stay fp64
    for d in range(nd):
        for w in (1, 2, 3):
            all_float32(O.add_ghost(g, data, d, w), "add_ghost")
            all_float32(O.add_ghost_extrapolate(data, d, w, True, np.float32), "add_ghost_extrapolate")
            all_float32(O.add_ghost_periodic(data, d, w, np.float32), "add_ghost_periodic")
        all_float32(O.eno3_helper(g, data, d, approx4=True), "eno3_helper")          # dL, dR, D1, D2, D3, D1u
        for scheme in F.OFN:
            all_float32(F.OFN[scheme](g, data, d), scheme)
        all_float32(O.max_d1_squared(g, data, d), "max_d1_squared")
    all_float32(O.add_ghost_all_dims(g, data, 2), "add_ghost_all_dims")
    system, y = c.system(32), data.reshape(-1, 1)
    for scheme in F.OFN:
        derivs = [F.OFN[scheme](g, data, d) for d in range(nd)]
        diss, sb = O.artificial_dissipation_glf(g, system, 0.0, data, [a[0] for a in derivs], [a[1] for a in derivs])
        all_float32([diss, sb], "artificial_dissipation_glf")
        all_float32(O.term_lax_friedrichs(g, system, scheme, 0.0, y), "term_lax_friedrichs " + scheme)
        all_float32(O.compute_gradients(g, data, scheme), "compute_gradients")
        lo, hi = O.costate_range(g, scheme, y)
        assert all(isinstance(v, np.float32) for v in lo + hi)
        for ode in (O.ode_cfl_1, O.ode_cfl_2, O.ode_cfl_3):
            t, y1 = ode(lambda tt, v: O.term_lax_friedrichs(g, system, scheme, tt, v), [0.0, 10.0], y, 0.8, single_step=True, dtype=np.float32)
            all_float32(y1, ode.__name__)
            assert isinstance(t, float) and t > 0.0             # time is a host value: fp64 (np.float64 is a float)


@pytest.mark.parametrize("name", ["plane5d", "pair6d"])
def test_the_5d_and_6d_systems_in_the_float32_mode(name):
    gmin, gmax, N, pd = HC.limits(name)
    g64, g32 = O.Grid(gmin, gmax, N, pd), O.Grid(gmin, gmax, N, pd, dtype=np.float32)
    d32 = HC.data(g64).astype(np.float32)
    for scheme in ("ENO2", "ENO3", "WENO5_ASSHIPPED"):
        yd32, sb32 = O.term_lax_friedrichs(g32, HC.oracle_system(name, g32, **HC.PARAMS[name]), scheme, 0.0, d32.reshape(-1))
        yd64, sb64 = O.term_lax_friedrichs(g64, HC.oracle_system(name, g64, **HC.PARAMS[name]), scheme, 0.0, d32.astype(np.float64).reshape(-1))
        all_float32([yd32, sb32], name)
        # the bound's inputs are maxima of tables rounded once: the two precisions agree to a few eps32
        assert abs(sb32 - sb64) <= 4 * F.EPS32 * sb64, (sb32, sb64)
        if scheme.startswith("WENO"):
            assert float(np.abs(yd32 - yd64).max()) <= 1e-3 * float(np.abs(yd64).max())


@pytest.mark.parametrize("scheme", ["ENO2", "ENO3", "WENO5_ASSHIPPED"])
@pytest.mark.parametrize("nd,per", F.GRIDS, ids=IDS)
def test_float32_mode_is_within_the_derived_bound_of_the_fp64_oracle(nd, per, scheme):
    c = F.Case.get(nd, per)
    got = c.deriv("noisy", scheme, 32)
    for d in range(nd):
        for side in (0, 1):
            ratio, left_out = F.within_bound(c, "noisy", scheme, got[d][side], side, d, masked=scheme.startswith("ENO"))
            print("%s axis %d %s: error / bound %.3g, left out %.4f" % (scheme, d, "LR"[side], ratio, left_out))
            assert left_out <= F.MAX_LEFT_OUT, (scheme, d, left_out)
            assert ratio <= 1.0, (scheme, d, side, ratio)


@pytest.mark.parametrize("nd,per", F.GRIDS, ids=IDS)
def test_symmetric_sphere_weno5_bound_and_the_share_of_eno3_ties(nd, per):
    c = F.Case.get(nd, per)
    got = c.deriv("symmetric", "WENO5_ASSHIPPED", 32)
    below, cells = 0, 0
    for d in range(nd):
        for side in (0, 1):
            assert got[d][side].dtype == np.float32
            ratio, _ = F.within_bound(c, "symmetric", "WENO5_ASSHIPPED", got[d][side], side, d, masked=False)
            assert ratio <= 1.0, (d, side, ratio)
        m = c.margin("symmetric", "ENO3")[d]
        below += int(np.sum(m < F.MARGIN))
        cells += m.size
        all_float32(c.deriv("symmetric", "ENO3", 32)[d], "ENO3")
    print("ENO3 cells below the margin: %.3f" % (below / cells))
    assert below >= 0.05 * cells, (below, cells)
