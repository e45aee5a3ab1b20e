"""The refusals of libhj_filter.so's two entry points as rows (tests/test_filter_host.py asserts every one without a device: every
check comes before the first HIP call, so host arrays stand in for the device's) -- TEST INFRASTRUCTURE, NOT PRODUCT.

A row is (keyword arguments that replace the good call's, the code, a word of the text).  The good call is a 9 x 9 fp64 grid, four
stored sets, three states of the double integrator.
"""
import ctypes as C

import numpy as np

from levelsetpy_amd import _ffi, _fffi, _qffi, _rffi

EINVAL, EUNSUPPORTED = -1, -3
M, T, ND, N, SUB = 3, 4, 2, 81, 2
NSTEPS = (T - 1) * SUB
NAN, INF = float("nan"), float("inf")


def grid(nd=2, n=9):
    return _qffi.grid_descriptor(nd, [n] * nd, [-1.0] * nd, [1.0] * nd, [2.0 / (n - 1)] * nd, [_ffi.BC_EXTRAPOLATE] * nd, [0.0] * nd, "float64")


DI = _rffi.plant_descriptor(_ffi.HAM_DOUBLE_INTEGRATOR, 0, 0, [1.0])
DUBINS = _rffi.plant_descriptor(_ffi.HAM_DUBINS_REL, 1, 0, [1.0, 1.0, 1.0])
BAD_MODE = _rffi.plant_descriptor(_ffi.HAM_DOUBLE_INTEGRATOR, 2, 0, [1.0])
USER = _rffi.plant_descriptor(_ffi.HAM_USER_BASE, 0, 0, [1.0])


def arrays():
    """Sentinel-filled outputs and zero inputs of the good calls."""
    f64 = {k: np.full(s, 5.0) for k, s in dict(final=(M, ND), gmin=(M,), vend=(M,), traj=(M, ND, T), applied=(M, NSTEPS, 2),
                                                 p_applied=(M, 2), p_value=(M,), p_gap=(M,), p_costate=(M, ND)).items()}
    i32 = {k: np.full(s, -77, dtype=np.int32) for k, s in dict(count=(M,), first=(M,), length=(M,), status=(M,)).items()}
    u8 = {k: np.full(s, 9, dtype=np.uint8) for k, s in dict(active=(M, NSTEPS), p_active=(M,)).items()}
    ins = dict(data=np.zeros((T, 9, 9)), x0=np.zeros((M, ND)), u_nom=np.zeros((M, T - 1, 1)), nom=np.zeros((T, 9, 9)))
    return f64, i32, u8, ins


def untouched(f64, i32, u8):
    return all((a == 5.0).all() for a in f64.values()) and all((a == -77).all() for a in i32.values()) and \
        all((a == 9).all() for a in u8.values())


def rollout_call(lib, f64, i32, u8, ins, **kw):
    ad = lambda a: a.ctypes.data                                            # noqa: E731
    a = dict(desc=grid(2), scheme=_ffi.ENO2, data=ad(ins["data"]), T=T, stride=N, x0=ad(ins["x0"]), M=M, sub=SUB, dt=0.01, plant=DI,
             policy=_fffi.SLICE_CLOCK, slice=0, nominal=_fffi.NOMINAL_TABLE, u_nom=ad(ins["u_nom"]), nom=None, nom_T=0, nom_stride=0,
             nom_mode=0, level=0.0, margin=0.1, dstb=0, final=ad(f64["final"]), gmin=ad(f64["gmin"]), vend=ad(f64["vend"]),
             count=ad(i32["count"]), first=ad(i32["first"]), length=ad(i32["length"]), status=ad(i32["status"]), traj=ad(f64["traj"]),
             active=ad(u8["active"]), applied=ad(f64["applied"]))
    for k, v in kw.items():
        assert k in a, k
        a[k] = ad(ins[v]) if isinstance(v, str) else v
    return lib.hjf_rollout(C.byref(a["desc"]) if a["desc"] is not None else None, a["scheme"], a["data"], a["T"], a["stride"], a["x0"],
                           a["M"], a["sub"], a["dt"], C.byref(a["plant"]) if a["plant"] is not None else None, a["policy"], a["slice"],
                           a["nominal"], a["u_nom"], a["nom"], a["nom_T"], a["nom_stride"], a["nom_mode"], a["level"], a["margin"],
                           a["dstb"], a["final"], a["gmin"], a["vend"], a["count"], a["first"], a["length"], a["status"], a["traj"],
                           a["active"], a["applied"], None)


def decide_call(lib, f64, i32, u8, ins, **kw):
    ad = lambda a: a.ctypes.data                                            # noqa: E731
    a = dict(desc=grid(2), scheme=_ffi.ENO2, data=ad(ins["data"]), F=T, stride=N, slice=1, xs=ad(ins["x0"]), M=M, plant=DI,
             u_nom=ad(ins["u_nom"]), level=0.0, margin=0.1, dstb=0, applied=ad(f64["p_applied"]), active=ad(u8["p_active"]),
             value=ad(f64["p_value"]), gap=ad(f64["p_gap"]), costate=ad(f64["p_costate"]))
    for k, v in kw.items():
        assert k in a, k
        a[k] = v
    return lib.hjf_decide(C.byref(a["desc"]) if a["desc"] is not None else None, a["scheme"], a["data"], a["F"], a["stride"], a["slice"],
                          a["xs"], a["M"], C.byref(a["plant"]) if a["plant"] is not None else None, a["u_nom"], a["level"], a["margin"],
                          a["dstb"], a["applied"], a["active"], a["value"], a["gap"], a["costate"], None)


VALUE = dict(nominal=_fffi.NOMINAL_VALUE, u_nom=None, nom="nom", nom_T=T, nom_stride=N, nom_mode=1)

# check_rollout's, in its order, then the filter's own
ROLLOUT_ROWS = [
    (dict(desc=None), EINVAL, b"null grid"),
    (dict(plant=None), EINVAL, b"null plant"),
    (dict(M=-1), EINVAL, b"nstates"),
    (dict(T=1), EINVAL, b"at least two stored sets"),
    (dict(sub=0), EINVAL, b"sub_samples"),
    (dict(dt=NAN), EINVAL, b"dt_small"),
    (dict(stride=N - 1), EINVAL, b"field_stride"),
    (dict(stride=0), EINVAL, b"field_stride 0"),                                     # one field for every stamp: not under the clock
    (dict(scheme=_ffi.WENO5), EUNSUPPORTED, b"scheme"),
    (dict(scheme=9), EUNSUPPORTED, b"scheme"),
    (dict(plant=USER), EUNSUPPORTED, b"no filter kernel"),
    (dict(plant=DUBINS), EINVAL, b"3 states"),
    (dict(desc=grid(3), stride=729), EINVAL, b"2 states"),
    (dict(plant=BAD_MODE), EINVAL, b"u_mode / d_mode"),
    (dict(desc=grid(2, 2)), EINVAL, b"grid too small"),
    (dict(data=None), EINVAL, b"null argument"),
    (dict(x0=None), EINVAL, b"null argument"),
    (dict(final=None), EINVAL, b"null argument"),
    (dict(length=None), EINVAL, b"null argument"),
    (dict(status=None), EINVAL, b"null argument"),
    (dict(policy=2), EINVAL, b"slice_policy"),
    (dict(policy=-1), EINVAL, b"slice_policy"),
    (dict(policy=_fffi.SLICE_STATIC, slice=T), EINVAL, b"slice 4 outside 0..3"),
    (dict(policy=_fffi.SLICE_STATIC, slice=-1), EINVAL, b"slice -1"),
    (dict(policy=_fffi.SLICE_STATIC, stride=0, slice=1), EINVAL, b"slice 1 outside 0..0"),
    (dict(level=INF), EINVAL, b"level"),
    (dict(level=NAN), EINVAL, b"level"),
    (dict(margin=NAN), EINVAL, b"margin must not be NaN"),
    (dict(dstb=2), EINVAL, b"dstb"),
    (dict(nominal=2), EINVAL, b"nominal 2"),
    (dict(VALUE, nom_T=2), EINVAL, b"nom_ntimes 2"),
    (dict(VALUE, nom_T=0), EINVAL, b"nom_ntimes 0"),
    (dict(VALUE, nom_stride=N - 1), EINVAL, b"nom_field_stride"),
    (dict(VALUE, nom_mode=2), EINVAL, b"nom_u_mode"),
    (dict(T=2 ** 30 + 1, sub=4), EINVAL, b"step index"),
    (dict(gmin=None), EINVAL, b"null argument"),
    (dict(vend=None), EINVAL, b"null argument"),
    (dict(count=None), EINVAL, b"null argument"),
    (dict(first=None), EINVAL, b"null argument"),
    (dict(u_nom=None), EINVAL, b"null argument"),
    (dict(VALUE, nom=None), EINVAL, b"null argument"),
    (dict(M=2 ** 30), EINVAL, b"split over states"),
    (dict(M=2 ** 40), EINVAL, b"split over states"),
]

DECIDE_ROWS = [
    (dict(desc=None), EINVAL, b"null grid"),
    (dict(plant=None), EINVAL, b"null plant"),
    (dict(M=-1), EINVAL, b"nstates"),
    (dict(scheme=_ffi.WENO5), EUNSUPPORTED, b"scheme"),
    (dict(plant=USER), EUNSUPPORTED, b"no filter kernel"),
    (dict(plant=DUBINS), EINVAL, b"3 states"),
    (dict(plant=BAD_MODE), EINVAL, b"u_mode / d_mode"),
    (dict(desc=grid(2, 2)), EINVAL, b"grid too small"),
    (dict(data=None), EINVAL, b"null argument"),
    (dict(xs=None), EINVAL, b"null argument"),
    (dict(applied=None), EINVAL, b"null argument"),
    (dict(active=None), EINVAL, b"null argument"),
    (dict(value=None), EINVAL, b"null argument"),
    (dict(F=0), EINVAL, b"nfields 0"),
    (dict(stride=N - 1), EINVAL, b"field_stride"),
    (dict(slice=T), EINVAL, b"slice 4 outside 0..3"),
    (dict(F=1, stride=0, slice=1), EINVAL, b"slice 1 outside 0..0"),
    (dict(level=NAN), EINVAL, b"level"),
    (dict(margin=NAN), EINVAL, b"margin must not be NaN"),
    (dict(dstb=-1), EINVAL, b"dstb"),
    (dict(gap=None), EINVAL, b"null argument"),
    (dict(u_nom=None), EINVAL, b"null argument"),
    (dict(M=2 ** 30), EINVAL, b"split over states"),
]
