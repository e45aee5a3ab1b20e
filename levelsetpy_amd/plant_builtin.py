"""Plane5D and DubinsPair6D as registered plants, and the route of extraArgs.plantKernel.

computeStochTrajs (montecarlo.py), computeSafeTrajs and safeControls (safety.py) have precompiled kernels for the three built-in 2-D .. 4-D
systems only.  Under extraArgs.plantKernel=True a registered plant (plant.register_plant) runs in the kernel libhj_plant.so compiles around
it at run time -- user_noisy_rollout_kernel, user_filtered_rollout_kernel, user_decide_points_kernel -- and so do the package's own two
5-D / 6-D systems: their controls and dynamics stand below as device statements, in the operation order of include/hj_hiquery.h's table,
with the parameters in the order dynamics.native_plant_hi returns them, and are registered once per process, at their first use.
"""
from . import _hffi
from .dynamics import native_plant_hi
from .query import point_scheme
from .rollout import _get
from .utilities import error

__all__ = ["TEXTS", "registration_hi", "plant_hi", "route", "flag"]

# plant id -> (name, dim, controls_src, dynamics_src, ncontrols, ndisturbances, nparams)
TEXTS = {
    _hffi.HAM_PLANE5D: ("Plane5D", 5, """
        u[0] = par[0] * sgn(p[3]);
        u[1] = par[1] * sgn(p[4]);
        if (!u_max) { u[0] = -u[0]; u[1] = -u[1]; }
    """, """
        const double c = cos(x[2]);
        const double s = sin(x[2]);
        dx[0] = x[3] * c;
        dx[1] = x[3] * s;
        dx[2] = x[4];
        dx[3] = u[0];
        dx[4] = u[1];
    """, 2, 0, 2),
    _hffi.HAM_DUBINS_PAIR6D: ("DubinsPair6D", 6, """
        u[0] = par[2] * sgn(p[2]);
        if (!u_max) u[0] = -u[0];
        dst[0] = par[3] * sgn(p[5]);
        if (!d_max) dst[0] = -dst[0];
    """, """
        const double ve = par[0], vp = par[1];
        const double c2 = cos(x[2]);
        const double s2 = sin(x[2]);
        const double c5 = cos(x[5]);
        const double s5 = sin(x[5]);
        dx[0] = ve * c2;
        dx[1] = ve * s2;
        dx[2] = u[0];
        dx[3] = vp * c5;
        dx[4] = vp * s5;
        dx[5] = dst[0];
    """, 1, 1, 4),
}

_registered = {}


def registration_hi(plant_id):
    """The PlantRegistration of HAM_PLANE5D / HAM_DUBINS_PAIR6D: made at the first call, the same object afterwards."""
    if plant_id not in _registered:
        from .plant import register_plant
        name, dim, ctl, dyn, nu, nd, npar = TEXTS[plant_id]
        _registered[plant_id] = register_plant(name, dim, ctl, dyn, nu, nd, npar)
    return _registered[plant_id]


def plant_hi(dynSys):
    """(registration, parameters) for a Plane5D / DubinsPair6D that native_plant_hi's identity rule lets through, else None."""
    nat = native_plant_hi(dynSys)
    if nat is None:
        return None
    reg = registration_hi(nat[0])
    return reg, [float(v) for v in nat[1][:reg.nparams]]


def route(dynSys, derivFunc, g):
    """The two rules extraArgs.plantKernel adds after the built-in one: (registration, parameters), None when a run-time kernel computes
    what dynSys's methods would on grid g with derivFunc; None, why when dynSys is such a plant and the call is not one for the kernel;
    None, None when dynSys is neither a registered plant nor one of the two systems above."""
    from .plant import plant_of
    user = plant_of(dynSys) or plant_hi(dynSys)
    if user is None:
        return None, None
    if user[0].dim != g.dim:
        return None, "%s has no native plant on a %d-D grid" % (type(dynSys).__name__, g.dim)
    if point_scheme(derivFunc) is None:
        return None, "derivFunc %s has no point kernel" % getattr(derivFunc, "__name__", derivFunc)
    return user, None


def flag(extraArgs):
    """extraArgs.plantKernel, a bool (default False); anything else is refused by name."""
    v = _get(extraArgs, 'plantKernel', False)
    if not isinstance(v, bool):
        error('extraArgs.plantKernel must be True or False (got %r)' % (v,))
    return v
