#!/usr/bin/env python3
"""Register use of the kernels hipRTC builds around TRACED 5-D / 6-D callbacks (levelsetpy_amd/trace_ham.py, set_hidim_trace), offline.

tools/hidim_user_resources.py's report() -- hipcc on hjh_ham_source's translation unit with -Rpass-analysis=kernel-resource-usage -- for the
registrations the tracer makes of tests/hidim_trace_cases.py's pairs, beside the hand-registered figures that tool prints.  Needs no GPU.
`make -C levelsetpy_amd/csrc resource-usage-hidim-trace` prints the table; scratch or spills are reported as found, nothing is asserted.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def traced_registrations(hoist=None):
    """[(label, HidimRegistration)] of the traced Plane5D, DubinsPair6D and quadrotor (stored tables, trig inside the callbacks)."""
    import levelsetpy_amd as L
    from levelsetpy_amd import trace_ham as T
    import hidim_cases as HC
    import hidim_trace_cases as TC
    import hidim_user_cases as UC
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731

    def grid(lim):
        gmin, gmax, N, pd = lim
        return L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd)
    g5, g6, gq = grid(HC.limits("plane5d")), grid(HC.limits("pair6d")), grid(UC.quad_limits())
    pairs = [("Plane5D, stored tables", g5, TC.PlanePair(g5, **HC.PARAMS["plane5d"])),
             ("DubinsPair6D, trig in the callbacks", g6, TC.DubinsPair(g6, **HC.PARAMS["pair6d"])),
             ("quadrotor, stored tables", gq, TC.QuadTables(gq, UC.QUAD_PAR)),
             ("quadrotor, trig in the callbacks", gq, TC.QuadInline(gq, UC.QUAD_PAR))]
    if hoist is not None:
        os.environ["HJ_TRACE_HOIST"] = hoist
    try:
        return [(label, T._registration(T.trace_callbacks(g, s.hamiltonian, s.dissipation))) for label, g, s in pairs]
    finally:
        os.environ.pop("HJ_TRACE_HOIST", None)


def main():
    import hidim_user_resources as UR
    regs = traced_registrations() + [(label + ", HJ_TRACE_HOIST=off", r) for label, r in traced_registrations("off")[3:]]
    for label, reg in regs:
        print("%s: %s (%d-D, %d parameters, tables along %s)" % (label, reg.name, reg.dim, reg.nparams, list(reg.aux_axes)))
        for r in UR.report(reg):
            print("  %-70s VGPRs %3d  SGPRs %3d  scratch %3d B/lane  occupancy %d waves/SIMD" % (
                r["kernel"].replace("hjh::", ""), r["vgprs"], r["sgprs"], r["scratch"], r["occupancy"]))


if __name__ == "__main__":
    main()
