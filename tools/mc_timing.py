#!/usr/bin/env python3
"""Timing of noisy_rollout_kernel (libhj_mc.so) beside the untouched rollout_kernel (libhj_rollout.so) on one MI355X
-> profiles/mc_timing.txt.

    python tools/mc_timing.py [--n 41] [--reps 20] [--out FILE]

Workload: tools/rollout_timing.py's -- the air3D reachable tube on n^3 nodes, 11 stored sets (tau = linspace(0, 2, 11),
minVOverTime, flipped), resident on the device in fp64; states drawn in [0, 2.2] x [-0.8, 0.8] x [-pi, pi]; uMode 'max', dMode
'min', 4 sub-samples, as-shipped WENO5 costates.  M R = 4096 and 262144 trajectories: M = M R / 16 states with R = 16 realisations
each for the noisy kernel (G = diag(0.2, 0.2, 0.1), policy 'earliest', the paths not kept unless the row says so), the same states
repeated 16 times for rollout_kernel.  The calls take turns in ONE process: in every repetition each variant runs once, in the
order of the rows; device events around each call (the output tensors' allocation included), median of --reps repetitions after 3
warm-up rounds (min and max beside it).  The variants do not do the same work: the noise changes when a trajectory reaches the
target, so the control steps each took are counted and the time per control step is given beside the call's.

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=41)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/mc_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _nffi, _rffi, montecarlo, rollout

    n, sub, R = args.n, 4, 16
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
    sys_ = L.DubinsVehicleRel(g, 1.0, 1.0)
    sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, dissFunc=L.artificialDissipationGLF,
                       CoStateCalc=L.upwindFirstWENO5))
    tau = np.linspace(0, 2.0, 11)
    stack, _, _ = L.HJIPDE_solve(L.shapeCylinder(g, 2, np.zeros((3, 1)), .5), tau, sd, 'minVOverTime',
                                 L.Bundle(dict(quiet=True, flipOutput=True)))
    V = torch.as_tensor(np.asarray(stack), device="cuda")
    T = len(tau)
    dt = (tau[1] - tau[0]) / sub
    sq = float(np.sqrt(np.float64(dt)))
    nsteps = (T - 1) * sub
    G = np.diag([0.2, 0.2, 0.1])
    nat = sys_.native()
    plant = _rffi.plant_descriptor(nat[0], _rffi.MODE_MAX, _rffi.MODE_MIN, nat[1])
    sid = _ffi.WENO5_ASSHIPPED
    rng = np.random.default_rng(0)
    lo, hi = np.array([0.0, -0.8, -np.pi]), np.array([2.2, 0.8, np.pi])
    prop = torch.cuda.get_device_properties(0)
    lines = ["noisy_rollout_kernel beside rollout_kernel on one MI355X: air3D tube, %d^3 nodes x %d stored sets (fp64), %d sub-samples, "
             "dt_small %.3g, G = diag(0.2, 0.2, 0.1), R = %d" % (n, T, sub, dt, R),
             "tools/mc_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the variants take turns in one process; device events around each call, %d repetitions after 3 warm-up rounds: "
             "median (min .. max) in ms" % args.reps, ""]
    for MR in (4096, 262144):
        M = MR // R
        X = torch.as_tensor(lo + rng.random((M, 3)) * (hi - lo), device="cuda")
        XR = X.repeat_interleave(R, dim=0).contiguous()
        Z = torch.empty((M, R, nsteps, 3), dtype=torch.float64, device="cuda")
        _nffi.check(_nffi.lib().hjn_normals(1, 0, MR, 0, nsteps, 3, None, Z.data_ptr(), None))
        torch.cuda.synchronize()

        def noisy(normals, keep, policy=_nffi.POLICY_EARLIEST):
            return montecarlo.noisy_rollout_states(g, V, X, sid, sub, dt, plant, G, sq, R, 0, 1, normals, policy, keep)
        variants = [
            ("rollout_kernel (no noise, paths kept)", lambda: rollout.rollout_states(g, V, XR, sid, sub, dt, plant), lambda o: o[1]),
            ("noisy, generated normals", lambda: noisy(None, False), lambda o: o[1]),
            ("noisy, supplied normals", lambda: noisy(Z, False), lambda o: o[1]),
            ("noisy, generated, paths kept", lambda: noisy(None, True), lambda o: o[1]),
            ("noisy, generated, policy clock", lambda: noisy(None, False, _nffi.POLICY_CLOCK), lambda o: o[1]),
        ]
        steps, names = [], []
        for name, fn, length in variants:
            out = fn()
            names.append(_rffi.last_kernel() if name.startswith("rollout") else _nffi.last_kernel())
            steps.append(int((length(out).to(torch.int64) - 1).sum()) * sub)
        ms = [[] for _ in variants]
        for rep in range(3 + args.reps):
            for k, (name, fn, _) in enumerate(variants):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 3:
                    ms[k].append(a.elapsed_time(b))
        base = float(np.median(ms[0]))
        lines.append("M R = %d (%d states x %d):" % (MR, M, R))
        for k, (name, _, _) in enumerate(variants):
            med = float(np.median(ms[k]))
            lines.append("  %-38s %9.3f (%.3f .. %.3f)   %9d control steps, %.3e steps/s, %.2fx rollout_kernel's time, %.2fx per control step   %s"
                         % (name, med, min(ms[k]), max(ms[k]), steps[k], steps[k] / (med * 1e-3), med / base,
                            (med / steps[k]) / (base / steps[0]), names[k]))
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
