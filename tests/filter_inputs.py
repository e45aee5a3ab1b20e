"""The inputs the filter's tests share (tests/test_filter_ref.py checks the conditions on them with the restatement alone,
tests/test_gpu_filter.py runs them on the device) and their restated results, each computed once -- TEST INFRASTRUCTURE, NOT
PRODUCT.  The value functions are tests/test_gpu_rollout.py's oracle-solved cases, by import.
"""
import numpy as np

import filter_ref as F
import rollout_ref as R

ND = {"float64": np.float64, "float32": np.float32}
_REFS = {}

# ---- the double integrator, whole horizon: test_gpu_rollout.integrator_case (41^2 x 21, 67 states, uMode 'min': a reach tube, so
# the gap is level - V).  The nominal of state m at column it is 0.9 cos(0.9 it + 0.37 m): it pushes in and out of the level set.
DI_LEVEL, DI_MARGIN, DI_SUB, DI_SCHEME = 0.3, 0.05, 4, "ENO3"


def di_case():
    from test_gpu_rollout import integrator_case
    g, og, data, tau, xs = integrator_case()
    it, m = np.arange(len(tau) - 1), np.arange(xs.shape[0])
    table = (0.9 * np.cos(0.9 * it[None, :] + 0.37 * m[:, None]))[:, :, None]
    table.setflags(write=False)
    return g, og, data, tau, xs, table


def di_nominal_value():
    """A second value function on the integrator's grid: the distance to a point off centre, one field for every column.  Its
    control is the sign of its second costate, which vanishes on x2 = -0.2137: with |u| = 1 and dt_small = 0.0125 every velocity the
    value nominal reaches from the lattice is -0.7 + 0.0125 k, at least 0.0012 from that line, so the sign does not hang on the
    last place of an fp32 stencil."""
    g, og, data, tau, xs, _ = di_case()
    X = np.meshgrid(*[np.asarray(v).ravel() for v in og.vs], indexing='ij')
    nom = np.sqrt((X[0] - 0.4) ** 2 + (X[1] + 0.2137) ** 2 + 0.01)
    nom.setflags(write=False)
    return nom


def di_ref(dtype, kind):
    """kind: 'table' (clock), 'value' (clock, the one-field nominal, uMode min), 'static' (slice 7 of the stack, table), 'single'
    (data[7] alone as a stride-0 field, table: the same trajectories as 'static'), 'always' (margin +inf), 'never' (-inf)."""
    key = ("di", dtype, kind)
    if key not in _REFS:
        g, og, data, tau, xs, table = di_case()
        d = data.astype(ND[dtype])
        kw = dict(uMode='min', dMode='min', subSamples=DI_SUB, scheme=DI_SCHEME, margin=DI_MARGIN, level=DI_LEVEL)
        nominal = table
        if kind == 'value':
            nominal = dict(data=di_nominal_value().astype(ND[dtype]), uMode='min')
        elif kind == 'static':
            kw.update(policy='static', slice=7)
        elif kind == 'single':
            d = d[7]
            kw.update(policy='static', slice=0)
        elif kind == 'always':
            kw.update(margin=np.inf)
        elif kind == 'never':
            kw.update(margin=-np.inf)
        _REFS[key] = F.filter_ref(og, d, tau, "integrator", (1.0,), xs, nominal, **kw)
    return _REFS[key]


# ---- Dubins, whole horizon: test_gpu_rollout.dubins_case (the air3D avoid tube on 21^3 x 11, 64 states, uMode 'max', dMode 'min'),
# the evader's nominal "fly straight" (a = 0)
DUB_MARGIN, DUB_SUB, DUB_SCHEME, DUB_PAR = 0.05, 4, "ENO2", (1.0, 1.0, 1.0)


def dubins_ref():
    if "dub" not in _REFS:
        from test_gpu_rollout import dubins_case
        g, og, data, tau, xs = dubins_case()
        _REFS["dub"] = F.filter_ref(og, data, tau, "dubins", DUB_PAR, xs, np.zeros((len(tau) - 1, 1)), 'max', 'min', DUB_SUB, DUB_SCHEME,
                                    margin=DUB_MARGIN)
    return _REFS["dub"]


# ---- the filter does its job: the same tube, the pursuer roughly head-on ahead of the evader.  Of 1200 states drawn in the box the
# first 64 with V[0](x0) - margin above one grid spacing (the largest of the two position axes', 0.2); margin = JOB_K spacings.
# JOB_K was found with the restatement (tests/test_filter_ref.py prints the sweep): on this 21^3 grid a margin of 0.25 or 0.5
# spacings still lets bang-bang trajectories dip through the level set between two sub-steps, 0.75 keeps the smallest gap at 0.009,
# one spacing at 0.06.
JOB_DX, JOB_K = 0.2, 1.0


def job_states(k=JOB_K):
    from test_gpu_rollout import dubins_case
    g, og, data, tau, xs = dubins_case()
    lo, hi = np.array([0.7, -0.5, np.pi - 0.6]), np.array([2.6, 0.5, np.pi + 0.6])
    draw = lo + np.random.default_rng(11).random((1200, 3)) * (hi - lo)
    draw[:, 2] = (draw[:, 2] + np.pi) % (2 * np.pi) - np.pi
    v0 = R._eval(og, data[0], draw)
    return draw[v0 - k * JOB_DX > JOB_DX][:64].copy()


def job_ref(filtered, k=JOB_K):
    key = ("job", filtered, k)
    if key not in _REFS:
        from test_gpu_rollout import dubins_case
        g, og, data, tau, xs = dubins_case()
        _REFS[key] = F.filter_ref(og, data, tau, "dubins", DUB_PAR, job_states(k), np.zeros((len(tau) - 1, 1)), 'max', 'min', DUB_SUB,
                                  DUB_SCHEME, margin=k * JOB_DX if filtered else -np.inf)
    return _REFS[key]
