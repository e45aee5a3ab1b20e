#!/usr/bin/env python3
"""What extraArgs.plantKernel costs and saves, measured on the device: writes profiles/plant_hooks_timing.txt.

  1. Dubins registered as text (tests/plant_cases.py) under the flag against filtered_rollout_kernel / noisy_rollout_kernel of the same
     plant, on a 41^3 x 11 analytic stack (tests/hiquery_cases.smooth: the timing does not hang on the values), M = 4096 and 262144,
     four sub-steps, ENO2, fp64: the launches alone (safety.filtered_rollout_states / montecarlo.noisy_rollout_states on device tensors),
     device events, the median of REPS turns with the two candidates taking turns in one process, after one untimed turn each (the
     run-time compile or the disk cache's load is in that one).
  2. The planar quadrotor and Plane5D under the flag against the host loop they take without it, at M = 8 (the loop needs seconds):
     computeSafeTrajs and computeStochTrajs as a caller sees them, wall clock around a synchronised call, the median of 3.  Both
     computeStochTrajs runs are given their normals: the host loop's generator (hjn_normals_host) stops at four normals a step.
No ratio is promised: the file says what was found.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS = 9


def main():
    import torch
    import levelsetpy_amd as L
    from levelsetpy_amd import _fffi, _nffi, _pffi, _rffi, montecarlo, safety
    import hiquery_cases as XC
    import plant_cases as PC
    import query_ref as Q
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def turns(cands):
        for fn in cands.values():
            fn()
        torch.cuda.synchronize()
        ms = dict((k, []) for k in cands)
        for _ in range(REPS):
            for k, fn in cands.items():
                ms[k].append(timed(fn))
        return dict((k, float(np.median(v))) for k, v in ms.items())

    say("device: %s" % torch.cuda.get_device_name(0))
    # ---- 1. the same plant, precompiled and compiled at run time
    g, _ = Q.make_grids((41, 41, 41), (2,))
    T, sub = 11, 4
    data = torch.as_tensor(np.stack([XC.smooth(g, k) for k in range(T)]), device="cuda")
    tau = np.linspace(0.0, 1.0, T)
    dt = (tau[1] - tau[0]) / sub
    reg = PC.register_builtin("dubins")
    par = [1.0, 1.0, 1.0]
    bd, ud = _rffi.plant_descriptor(0, 1, 0, par), _pffi.plant_descriptor(reg.plant_id, 1, 0, par)
    lo = np.array([float(np.asarray(v).ravel()[0]) for v in g.vs])
    hi = np.array([float(np.asarray(v).ravel()[-1]) for v in g.vs])
    G = 0.05 * np.eye(3)
    say("1. Dubins as text under the flag against the precompiled kernels: 41^3 x 11, %d sub-steps, ENO2, fp64, median of %d [ms]" % (sub, REPS))
    for M in (4096, 262144):
        xs = torch.as_tensor(lo + (0.2 + 0.6 * np.random.default_rng(1).random((M, 3))) * (hi - lo), device="cuda")
        table = torch.zeros((M, T - 1, 1), dtype=torch.float64, device="cuda")
        level = 1.0
        f = lambda pl: (lambda: safety.filtered_rollout_states(g, data, T, xs, 0, sub, dt, pl, _fffi.SLICE_CLOCK, 0, table, None, 0, level, 0.1,    # noqa: E731
                                                               _fffi.DSTB_WORST, False, False))
        n = lambda pl: (lambda: montecarlo.noisy_rollout_states(g, data, xs, 0, sub, dt, pl, G, float(np.sqrt(dt)), 1, 0, 7, None,                # noqa: E731
                                                                _nffi.POLICY_CLOCK, False))
        r = turns({"filtered_rollout_kernel": f(bd), "user_filtered_rollout_kernel": f(ud)})
        say("   M = %6d  filtered: precompiled %8.3f   run-time %8.3f   (x%.2f)" % (M, r["filtered_rollout_kernel"], r["user_filtered_rollout_kernel"],
                                                                                  r["user_filtered_rollout_kernel"] / r["filtered_rollout_kernel"]))
        r = turns({"noisy_rollout_kernel": n(bd), "user_noisy_rollout_kernel": n(ud)})
        say("   M = %6d  noisy:    precompiled %8.3f   run-time %8.3f   (x%.2f)" % (M, r["noisy_rollout_kernel"], r["user_noisy_rollout_kernel"],
                                                                                  r["user_noisy_rollout_kernel"] / r["noisy_rollout_kernel"]))
    # ---- 2. the systems that had the host loop only
    say("2. under the flag against the host loop of today, M = 8, T = 3, 2 sub-steps, ENO2, fp64, wall clock, median of 3 [ms]")
    gq, _ = PC.quad_grids()
    quad = PC.register_quad().attach(PC.Quadrotor(gq), params=lambda o: o.params)
    g5, _ = XC.grids("plane5d")
    for name, gg, system, nu, uMode in (("planar quadrotor", gq, quad, 2, 'min'), ("Plane5D", g5, XC.system("plane5d", g5), 2, 'max')):
        stack = torch.as_tensor(np.stack([XC.smooth(gg, k) for k in range(3)]), device="cuda")
        tt = np.linspace(0.0, 0.04, 3)
        l5 = np.array([float(np.asarray(v).ravel()[0]) for v in gg.vs])
        h5 = np.array([float(np.asarray(v).ravel()[-1]) for v in gg.vs])
        xs = torch.as_tensor(l5 + (0.3 + 0.4 * np.random.default_rng(2).random((8, gg.dim))) * (h5 - l5), device="cuda")
        table = torch.full((8, 2, nu), 0.1, dtype=torch.float64, device="cuda")
        S = 0.02 * np.eye(gg.dim)
        xi = torch.as_tensor(np.random.default_rng(3).standard_normal((8, 1, 4, gg.dim)), device="cuda")
        for what, call in (("computeSafeTrajs", lambda a: L.computeSafeTrajs(gg, stack, tt, system, xs, table, a)),
                           ("computeStochTrajs", lambda a: L.computeStochTrajs(gg, stack, tt, system, xs, S, a))):
            res = {}
            for flag in (True, False):
                args = L.Bundle(dict(uMode=uMode, subSamples=2, derivFunc=L.upwindFirstENO2, level=2.0, margin=0.1, policy='clock', plantKernel=flag,
                                     quiet=True))
                if what == "computeStochTrajs":
                    args.normals = xi
                call(args)
                ms = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = call(args)
                    torch.cuda.synchronize()
                    ms.append(1e3 * (time.perf_counter() - t0))
                res[flag] = (float(np.median(ms)), out.path)
            say("   %-17s %-18s kernel %9.3f   host loop %10.3f   (%s | %s)" % (name, what, res[True][0], res[False][0], res[True][1], res[False][1]))
    with open(os.path.join(ROOT, "profiles", "plant_hooks_timing.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
