"""The refusal rows of libhj_plant.so's six entry points for noisy and filtered rollouts of registered plants (include/hj_plant.h) --
TEST INFRASTRUCTURE, NOT PRODUCT.  Every check comes before the first HIP call, so host arrays stand in for the device's and
tests/test_plant_hooks_host.py runs the rows without a GPU: (keyword overrides of a good call, the code, a word of the text).
"""
import ctypes as C

import numpy as np

from levelsetpy_amd import _fffi, _marshal, _nffi, _pffi

import plant_cases as PC
import query_ref as Q

NAN, INF = float("nan"), float("inf")
M, T, SUB, R = 5, 3, 2, 2
SENT_F, SENT_I, SENT_B = -12345.5, -77, 201


class Case(object):
    """A registered plant on a grid of its dimension (lin at 4-D: `hi` false; the quadrotor at 6-D: true) with sentinel-filled outputs."""

    def __init__(self, hi):
        self.hi = hi
        self.reg = PC.register_quad() if hi else PC.register_lin()
        self.par = list(PC.QUAD_PAR if hi else PC.LIN_PAR)
        self.g = PC.quad_grids()[0] if hi else Q.make_grids(Q.SHAPES[4], (3,))[0]
        self.other = Q.make_grids(Q.SHAPES[3], ())[0] if not hi else None
        describe = _marshal.descriptor_hi if hi else _marshal.descriptor
        self.desc, N = describe(self.g, "float64")
        self.tiny, _ = describe(self.g, "float64")
        self.tiny.N[0] = 2
        self.n, self.nd = int(np.prod(N)), self.g.dim
        self.nu = self.reg.ncontrols
        self.W = max(2, self.reg.ncontrols + self.reg.ndisturbances)
        nsteps = (T - 1) * SUB
        self.ins = dict(data=np.zeros((T, self.n)), x0=np.zeros((M, self.nd)), u_nom=np.zeros((M, T - 1, self.nu)), nom=np.zeros((T, self.n)),
                        normals=np.zeros((M, R, nsteps, self.nd)), G=np.eye(self.nd))
        self.f64 = dict(final=(M * R, self.nd), gap_min=(M,), value_end=(M * R,), value_min=(M * R,), traj=(M * R, self.nd, T),
                        applied=(M, nsteps, self.W), value=(M,), gap=(M,), costate=(M, self.nd))
        self.i32 = dict(interventions=(M,), first=(M,), length=(M * R,), status=(M * R,), t_earliest=(M * R, T))
        self.f64 = dict((k, np.full(s, SENT_F)) for k, s in self.f64.items())
        self.i32 = dict((k, np.full(s, SENT_I, dtype=np.int32)) for k, s in self.i32.items())
        self.u8 = dict(active=np.full((M, nsteps), SENT_B, dtype=np.uint8))
        self.good = _pffi.plant_descriptor(self.reg.plant_id, 1, 0, self.par)

    def untouched(self):
        return all((a == SENT_F).all() for a in self.f64.values()) and all((a == SENT_I).all() for a in self.i32.values()) and \
            (self.u8["active"] == SENT_B).all()

    def entry(self, name):
        return getattr(_pffi.lib(), "hjp_" + name + ("_hi" if self.hi else ""))

    def _common(self, kw):
        o = dict(desc=self.desc, scheme=0, data=self.ins["data"], T=T, stride=self.n, x0=self.ins["x0"], M=M, sub=SUB, dt=0.05, plant=self.good)
        o.update(kw)
        return o

    @staticmethod
    def _p(a):
        return a.ctypes.data if a is not None else None

    def noisy(self, **kw):
        o = self._common(dict(R=R, first=0, seed=0, normals=self.ins["normals"], G=self.ins["G"], sq=0.2, policy=_nffi.POLICY_CLOCK, final=self.f64["final"],
                              length=self.i32["length"], status=self.i32["status"], value_end=self.f64["value_end"], value_min=self.f64["value_min"],
                              traj=self.f64["traj"], te=self.i32["t_earliest"]))
        o.update(kw)
        p = self._p
        return self.entry("noisy_rollout")(C.byref(o["desc"]) if o["desc"] is not None else None, o["scheme"], p(o["data"]), o["T"], o["stride"],
                                           p(o["x0"]), o["M"], o["R"], o["first"], o["seed"], p(o["normals"]), p(o["G"]), o["sq"], o["policy"],
                                           o["sub"], o["dt"], C.byref(o["plant"]) if o["plant"] is not None else None, p(o["final"]),
                                           p(o["length"]), p(o["status"]), p(o["value_end"]), p(o["value_min"]), p(o["traj"]), p(o["te"]), None)

    def filtered(self, **kw):
        o = self._common(dict(slice_policy=_fffi.SLICE_CLOCK, slice=0, nominal=_fffi.NOMINAL_TABLE, u_nom=self.ins["u_nom"], nom=None, nom_T=0,
                              nom_stride=0, nom_mode=0, level=0.0, margin=0.1, dstb=_fffi.DSTB_WORST, final=self.f64["final"],
                              gap_min=self.f64["gap_min"], value_end=self.f64["value_end"], interventions=self.i32["interventions"],
                              first=self.i32["first"], length=self.i32["length"], status=self.i32["status"], traj=self.f64["traj"],
                              active=self.u8["active"], applied=self.f64["applied"]))
        o.update(kw)
        p = self._p
        return self.entry("filtered_rollout")(C.byref(o["desc"]) if o["desc"] is not None else None, o["scheme"], p(o["data"]), o["T"], o["stride"],
                                              p(o["x0"]), o["M"], o["sub"], o["dt"], C.byref(o["plant"]) if o["plant"] is not None else None,
                                              o["slice_policy"], o["slice"], o["nominal"], p(o["u_nom"]), p(o["nom"]), o["nom_T"], o["nom_stride"],
                                              o["nom_mode"], o["level"], o["margin"], o["dstb"], p(o["final"]), p(o["gap_min"]), p(o["value_end"]),
                                              p(o["interventions"]), p(o["first"]), p(o["length"]), p(o["status"]), p(o["traj"]), p(o["active"]),
                                              p(o["applied"]), None)

    def decide(self, **kw):
        o = self._common(dict(slice=0, u_nom=self.ins["u_nom"], level=0.0, margin=0.1, dstb=_fffi.DSTB_WORST, applied=self.f64["applied"],
                              active=self.u8["active"], value=self.f64["value"], gap=self.f64["gap"], costate=self.f64["costate"]))
        o.update(kw)
        p = self._p
        return self.entry("decide")(C.byref(o["desc"]) if o["desc"] is not None else None, o["scheme"], p(o["data"]), o["T"], o["stride"], o["slice"],
                                    p(o["x0"]), o["M"], C.byref(o["plant"]) if o["plant"] is not None else None, p(o["u_nom"]), o["level"],
                                    o["margin"], o["dstb"], p(o["applied"]), p(o["active"]), p(o["value"]), p(o["gap"]), p(o["costate"]), None)

    # ---- rows.  check_rollout's come first, in its order, for every entry point
    def rollout_rows(self):
        bad_id = _pffi.plant_descriptor(_pffi.PLANT_BASE + 99999, 0, 0, self.par)
        builtin_id = _pffi.plant_descriptor(1, 0, 0, self.par)
        wrong_count = _pffi.plant_descriptor(self.reg.plant_id, 0, 0, self.par[:-1])
        bad_mode = _pffi.plant_descriptor(self.reg.plant_id, 2, 0, self.par)
        rows = [(dict(desc=None), -1, "null grid"), (dict(plant=None), -1, "null plant"), (dict(M=-1), -1, "nstates"),
                (dict(sub=0), -1, "sub_samples"), (dict(dt=NAN), -1, "dt_small"), (dict(scheme=2), -3, "scheme"), (dict(scheme=9), -3, "scheme"),
                (dict(plant=bad_id), -1, "unknown plant id"), (dict(plant=builtin_id), -1, "unknown plant id"),
                (dict(plant=wrong_count), -1, "parameters"), (dict(plant=bad_mode), -1, "u_mode"), (dict(desc=self.tiny), -1, "grid too small"),
                (dict(data=None), -1, "null argument"), (dict(x0=None), -1, "null argument")]
        return rows

    def noisy_rows(self):
        Gbad = np.eye(self.nd)
        Gbad[self.nd - 1, self.nd - 1] = INF                 # the last element: a check that reads G at another width misses it
        return self.rollout_rows() + [
            (dict(T=1), -1, "ntimes"), (dict(stride=self.n - 1), -1, "field_stride"), (dict(final=None), -1, "null argument"),
            (dict(R=0), -1, "nreal"), (dict(policy=2), -1, "HJN_POLICY"), (dict(sq=NAN), -1, "sq must be finite"), (dict(G=None), -1, "G"),
            (dict(G=Gbad), -1, "G[%d][%d]" % (self.nd - 1, self.nd - 1)), (dict(T=2 ** 31 - 1, sub=3), -1, "32 bits"),
            (dict(value_end=None), -1, "null argument"), (dict(value_min=None), -1, "null argument"),
            (dict(M=2 ** 31, R=2 ** 31), -1, "split over states"), (dict(M=(2 ** 32 >> self.nd) // R + 1), -1, "split over states")]

    def filtered_rows(self):
        return self.rollout_rows() + [
            (dict(T=1), -1, "ntimes"), (dict(stride=self.n - 1), -1, "field_stride"), (dict(stride=0), -1, "field_stride"),
            (dict(final=None), -1, "null argument"), (dict(slice_policy=2), -1, "slice_policy"),
            (dict(slice_policy=_fffi.SLICE_STATIC, slice=T), -1, "slice"), (dict(slice_policy=_fffi.SLICE_STATIC, slice=-1), -1, "slice"),
            (dict(slice_policy=_fffi.SLICE_STATIC, stride=0, slice=1), -1, "slice"), (dict(level=INF), -1, "level must be finite"),
            (dict(margin=NAN), -1, "must not be NaN"), (dict(dstb=2), -1, "HJF_DSTB_WORST"), (dict(nominal=2), -1, "nominal"),
            (dict(nominal=_fffi.NOMINAL_VALUE, nom=self.ins["nom"], nom_T=2, nom_stride=self.n), -1, "nom_ntimes"),
            (dict(nominal=_fffi.NOMINAL_VALUE, nom=self.ins["nom"], nom_T=T, nom_stride=self.n - 1), -1, "nom_field_stride"),
            (dict(nominal=_fffi.NOMINAL_VALUE, nom=self.ins["nom"], nom_T=1, nom_mode=2), -1, "nom_u_mode"),
            (dict(T=2 ** 31 - 1, sub=2), -1, "int32"), (dict(gap_min=None), -1, "null argument"), (dict(u_nom=None), -1, "null argument"),
            (dict(nominal=_fffi.NOMINAL_VALUE, nom=None, nom_T=1), -1, "null argument"), (dict(M=(2 ** 32 >> self.nd) + 1), -1, "split over states")]

    def decide_rows(self):
        # (a point has no sub-steps and no step: those two rows are the rollouts')
        return [r for r in self.rollout_rows() if "sub" not in r[0] and "dt" not in r[0]] + [
            (dict(applied=None), -1, "null argument"), (dict(active=None), -1, "null argument"), (dict(value=None), -1, "null argument"),
            (dict(T=0), -1, "nfields"), (dict(stride=self.n - 1), -1, "field_stride"), (dict(slice=T), -1, "slice"), (dict(slice=-1), -1, "slice"),
            (dict(level=NAN), -1, "level must be finite"), (dict(margin=NAN), -1, "must not be NaN"), (dict(dstb=-1), -1, "HJF_DSTB_WORST"),
            (dict(gap=None), -1, "null argument"), (dict(u_nom=None), -1, "null argument"), (dict(M=(2 ** 32 >> self.nd) + 1), -1, "split over states")]
