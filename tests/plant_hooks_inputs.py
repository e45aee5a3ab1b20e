"""The inputs tests/test_plant_hooks_ref.py (the conditions, with the restatement alone) and tests/test_gpu_plant_hooks.py (the device)
share, and their restated results, each computed once -- TEST INFRASTRUCTURE, NOT PRODUCT.

Two horizons on analytic stacks (tests/hiquery_cases.smooth, a different seed per time stamp), no solve: four time stamps, two
sub-steps, 67 states.
  lin    three controls and two disturbances on (5, 6, 4, 7) with axis 3 periodic, uMode 'max' (gap = V - level), to t = 0.3; the states
         of tests/query_ref.state_set (nodes, first / last cells, outside, periods away, a NaN state)
  quad   the planar quadrotor on its 6-D grid, uMode 'min' (gap = level - V), to t = 0.06 (gravity empties the grid soon after); states
         from the inner 70 % of the box, the last two outside an axis and NaN
The seeds, levels and margins were chosen with the restatement (tests/test_plant_hooks_ref.py states the conditions).
The table nominal of state m at column it is A_j cos(0.9 it + 0.37 m + j): it pushes in and out of the level set.
"""
import numpy as np

import hiquery_cases as XC
import plant_cases as PC
import plant_hooks_ref as PH
import query_ref as Q

TAUS = {"lin": np.linspace(0.0, 0.3, 4), "quad": np.linspace(0.0, 0.06, 4)}
NT = 4
SUB = 2
M = 67
_CASES, _REFS = {}, {}

# name -> (restatement's plant, parameters, NU, NDST, uMode, dMode, level, margin, state seed)
SPEC = {
    "lin": ("lin", PC.LIN_PAR, 3, 2, 'max', 'min', 0.9, 0.15, 1),
    "quad": ("quad", PC.QUAD_PAR, 2, 0, 'min', 'min', 2.7, 0.05, 21),
}


def case(name):
    """(grid, oracle grid, stack (4,) + shape fp64, states (67, dim), table (67, 3, NU))."""
    if name not in _CASES:
        g, og = Q.make_grids(Q.SHAPES[4], (3,)) if name == "lin" else PC.quad_grids()
        data = np.stack([XC.smooth(g, k) for k in range(NT)])
        if name == "lin":
            xs = Q.state_set(g, M, SPEC[name][8])
        else:
            lo = np.array([float(np.asarray(v).ravel()[0]) for v in og.vs])
            hi = np.array([float(np.asarray(v).ravel()[-1]) for v in og.vs])
            xs = lo + (0.15 + 0.7 * np.random.default_rng(SPEC[name][8]).random((M, 6))) * (hi - lo)
            xs[-2, 0], xs[-1, 2] = hi[0] + 0.1, np.nan
        nu = SPEC[name][2]
        amp = (0.5, 0.9, 0.3) if name == "lin" else (0.5 * PC.QUAD_PAR[6], 0.5 * PC.QUAD_PAR[6])
        it, m, j = np.arange(NT - 1)[None, :, None], np.arange(M)[:, None, None], np.arange(nu)[None, None, :]
        table = np.asarray(amp)[None, None, :] * np.cos(0.9 * it + 0.37 * m + j)
        if name == "quad":
            table = table + 0.5 * PC.QUAD_PAR[6]             # thrusts in [0, Tmax]
        for a in (data, xs, table):
            a.setflags(write=False)
        _CASES[name] = (g, og, data, xs, table)
    return _CASES[name]


def nominal_value(name):
    """A second value function on the case's grid, one field for every column: another seed of the same family."""
    g = case(name)[0]
    nom = XC.smooth(g, 5)
    nom.setflags(write=False)
    return nom


def ref(name, dtype="float64", kind="table", scheme="ENO2"):
    """kind: 'table', 'value' (the one-field nominal, the case's uMode negated), 'zero' (table, disturbance 'zero'), 'static' (slice 2)."""
    key = (name, dtype, kind, scheme)
    if key not in _REFS:
        g, og, data, xs, table = case(name)
        plant, par, nu, ndst, uMode, dMode, level, margin, _ = SPEC[name]
        t = np.float64 if dtype == "float64" else np.float32
        kw = dict(uMode=uMode, dMode=dMode, subSamples=SUB, scheme=scheme, margin=margin, level=level)
        nominal = table
        if kind == "value":
            nominal = dict(data=nominal_value(name).astype(t), uMode='min' if uMode == 'max' else 'max')
        elif kind == "zero":
            kw.update(dstb='zero')
        elif kind == "static":
            kw.update(policy='static', slice=2)
        _REFS[key] = PH.filter_ref(og, data.astype(t), TAUS[name], plant, par, xs, nominal, **kw)
    return _REFS[key]
