#!/usr/bin/env python3
"""Timing of computeOptTrajs (levelsetpy_amd/rollout.py, libhj_rollout.so) on one MI355X -> profiles/rollout_timing.txt.

    python tools/rollout_timing.py [--n 41] [--reps 20] [--out FILE]

Workload: the air3D reachable tube on n^3 nodes, 11 stored sets (tau = linspace(0, 2, 11), minVOverTime, flipped), resident on
the device in fp64; M = 1, 4096 and 262144 pursuit / evasion pairs drawn in [0, 2.2] x [-0.8, 0.8] x [-pi, pi]; uMode 'max',
dMode 'min', 4 sub-samples, as-shipped WENO5 costates.  Device events around each call after a warm-up, median of --reps calls
(min and max beside it).  A control step is one {costate, controls, RK4 step}.

Two baselines that exist without the rollout kernel:
  M = 1     computeOptTraj with DubinsVehicleRel's own dynSys methods (host clock around the call: it synchronises at every
            sub-sample).  The same algorithm: bisection over the stored sets, stop at the target.
  M = 4096  the per-step loop of examples/closed_loop_rollout.py: one eval_costate launch and a chain of torch operators per
            control step, through a STATIC V (the first stored set) -- NO bisection over the stored sets and no stopping at the
            target, so every pair takes every step.  It does less work per step than the kernel and is compared per control step.

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def event_times(torch, fn, reps, warm=3):
    """ms of each of `reps` calls, by device events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms):
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=41)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/rollout_timing.py needs an MI355X: there is nothing to measure without one"
    from torch.utils._python_dispatch import TorchDispatchMode
    import levelsetpy_amd as L
    from levelsetpy_amd import rollout

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, a=(), kw=None):
            Count.n += 1
            return func(*a, **(kw or {}))

    n, sub = args.n, 4
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
    speed = turn = 1.0
    sys_ = L.DubinsVehicleRel(g, speed, turn)
    sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, dissFunc=L.artificialDissipationGLF,
                       CoStateCalc=L.upwindFirstWENO5))
    tau = np.linspace(0, 2.0, 11)
    stack, _, _ = L.HJIPDE_solve(L.shapeCylinder(g, 2, np.zeros((3, 1)), .5), tau, sd, 'minVOverTime',
                                 L.Bundle(dict(quiet=True, flipOutput=True)))
    V = torch.as_tensor(np.asarray(stack), device="cuda")
    T = len(tau)
    dt = (tau[1] - tau[0]) / sub
    rng = np.random.default_rng(0)
    lo, hi = np.array([0.0, -0.8, -np.pi]), np.array([2.2, 0.8, np.pi])
    prop = torch.cuda.get_device_properties(0)
    lines = ["computeOptTrajs on one MI355X: air3D tube, %d^3 nodes x %d stored sets (fp64), %d sub-samples, dt_small %.3g" % (n, T, sub, dt),
             "tools/rollout_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "device events around each call, %d calls after 3 warm-up calls: median (min .. max) in ms" % args.reps, ""]
    args_k = L.Bundle(dict(uMode='max', dMode='min', subSamples=sub))
    for M in (1, 4096, 262144):
        X = torch.as_tensor(lo + rng.random((M, 3)) * (hi - lo), device="cuda")
        trajs, lengths, _ = L.computeOptTrajs(g, V, tau, sys_, X, args_k)
        steps = int((lengths.to(torch.int64) - 1).sum()) * sub
        km = stats(event_times(torch, lambda: L.computeOptTrajs(g, V, tau, sys_, X, args_k), args.reps))
        lines.append("M = %d: %s, 1 launch, %d control steps in all (mean length %.2f of %d)" % (
            M, rollout.last_path(), steps, float(lengths.double().mean()), T))
        lines.append("  computeOptTrajs            %10.3f (%.3f .. %.3f)   %.3e trajectory-steps/s" % (km + (steps / (km[0] * 1e-3),)))
        if M == 1:
            x0 = X[0].cpu().numpy()

            def single():
                s = L.DubinsVehicleRel(g, speed, turn)
                s.x = x0.copy()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                traj, _ = L.computeOptTraj(g, V, tau, s, args_k)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0), traj
            single()
            runs = [single() for _ in range(max(3, args.reps // 4))]
            hm = stats([r[0] for r in runs])
            nsteps = (runs[0][1].shape[1] - 1) * sub
            launches = (runs[0][1].shape[1] - 1) * (1 + sub) + (1 if runs[0][1].shape[1] < T else 0)
            same = runs[0][1].shape[1] == int(lengths[0]) and float(np.nanmax(np.abs(runs[0][1] - trajs[0].cpu().numpy()[:, :runs[0][1].shape[1]]))) <= 1e-12
            lines.append("  computeOptTraj (host clock) %9.3f (%.3f .. %.3f)   %d launches and as many device-to-host copies for %d control steps; "
                         "%.1fx the kernel's time; the same trajectory to 1e-12: %s" % (hm + (launches, nsteps, hm[0] / km[0], same)))
        if M == 4096:
            V0 = V[0].contiguous()

            def dyn(x, a, b):
                return torch.stack([-speed + speed * torch.cos(x[:, 2]) + a * x[:, 1], speed * torch.sin(x[:, 2]) - a * x[:, 0], b - a], dim=1)

            def step(x):
                p = torch.nan_to_num(L.eval_costate(g, V0, x))
                a = turn * torch.sign(p[:, 0] * x[:, 1] - p[:, 1] * x[:, 0] - p[:, 2])
                b = -turn * torch.sign(p[:, 2])
                k1 = dyn(x, a, b)
                k2 = dyn(x + .5 * dt * k1, a, b)
                k3 = dyn(x + .5 * dt * k2, a, b)
                k4 = dyn(x + dt * k3, a, b)
                return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
            nloop = (T - 1) * sub

            def loop():
                x = X
                for _ in range(nloop):
                    x = step(x)
                return x
            with Count():
                Count.n = 0
                step(X)
                ops = Count.n
            lm = stats(event_times(torch, loop, max(3, args.reps // 4), warm=1))
            per_k, per_l = km[0] / (steps / M), lm[0] / nloop
            lines.append("  per-step torch loop        %10.3f (%.3f .. %.3f)   %d control steps for every pair through a STATIC V: no bisection, no stop "
                         "at the target; %d torch operator calls per control step (the costate launch among them), %d in all"
                         % (lm + (nloop, ops, ops * nloop)))
            lines.append("  per control step of all %d pairs: kernel %.4f ms (mean over the steps its trajectories took), loop %.4f ms: the loop takes "
                         "%.1fx the kernel's time per step" % (M, per_k, per_l, per_l / per_k))
            lines.append("  expectation (one launch beats the per-step launches at M = 4096): %s" % ("confirmed" if per_l > per_k else "REFUTED"))
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
