#!/usr/bin/env python3
"""Timing of filtered_rollout_kernel and decide_points_kernel (libhj_filter.so) beside the routes they replace, on one MI355X
-> profiles/filter_timing.txt.

    python tools/filter_timing.py [--n 41] [--reps 20] [--out FILE]

Workload: tools/rollout_timing.py's -- the air3D avoid tube on n^3 nodes, 11 stored sets (tau = linspace(0, 2, 11), minVOverTime,
flipped), resident on the device in fp64; states drawn in [0, 2.2] x [-0.8, 0.8] x [-pi, pi]; uMode 'max', dMode 'min', 4
sub-samples, as-shipped WENO5 costates; margin 0.1, level 0, the evader's nominal "fly straight" (a = 0) as a table, or as the value
nominal the tube itself (the same arithmetic as any second stack).  M = 4096 and 262144 states.  The candidates take turns in ONE
process: in every repetition each runs once, in the order of the rows; device events around each call (the output tensors' allocation
included), median of --reps repetitions after 3 warm-up rounds (min and max beside it).  They do not do the same work:
rollout_kernel stops a trajectory inside the last stored set and bisects over the stack, the filtered kernel runs every trajectory to
the end and reads V as well as grad V at every sub-step; the sub-steps each took are counted.  The per-step torch loop is
examples/closed_loop_rollout.py's with the value query and a torch.where switch added: eval_u, eval_costate, the controls, the switch
and an RK4 step in torch operators, once per sub-step.  safeControls at M = 10^6 stands beside eval_u + eval_costate + the controls'
formula (DubinsVehicleRel.get_opt_u's, written on tensors: the method itself takes one state) + the switch.

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/filter_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _fffi, _rffi, rollout, safety

    n, sub = args.n, 4
    margin, level = 0.1, 0.0
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
    nsteps = (T - 1) * sub
    nat = sys_.native()
    plant = _rffi.plant_descriptor(nat[0], _rffi.MODE_MAX, _rffi.MODE_MIN, nat[1])
    sid = _ffi.WENO5_ASSHIPPED
    speed = turn = 1.0
    rng = np.random.default_rng(0)
    lo, hi = np.array([0.0, -0.8, -np.pi]), np.array([2.2, 0.8, np.pi])
    prop = torch.cuda.get_device_properties(0)
    lines = ["filtered_rollout_kernel and decide_points_kernel beside the routes they replace on one MI355X: air3D tube, %d^3 nodes x %d "
             "stored sets (fp64), %d sub-samples, dt_small %.3g, margin %.2g" % (n, T, sub, dt, margin),
             "tools/filter_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the candidates take turns in one process; device events around each call, %d repetitions after 3 warm-up rounds: "
             "median (min .. max) in ms" % args.reps, ""]

    def dynamics(x, a, b):
        return torch.stack([-speed + speed * torch.cos(x[:, 2]) + a * x[:, 1], speed * torch.sin(x[:, 2]) - a * x[:, 0], b - a], dim=1)

    def controls(p, x):
        """DubinsVehicleRel.get_opt_u / get_opt_v (uMode 'max', dMode 'min') on tensors."""
        a = turn * torch.sign(p[:, 0] * x[:, 1] - p[:, 1] * x[:, 0] - p[:, 2])
        b = -turn * torch.sign(p[:, 2])
        return a, b

    def decide_torch(field, x, a_nom):
        v = L.eval_u(g, field, x)
        a, b = controls(L.eval_costate(g, field, x), x)
        act = ~((v - level) > margin)
        return torch.where(act, a, a_nom), b, act

    def torch_loop(X):
        a_nom = torch.zeros(X.shape[0], dtype=torch.float64, device="cuda")
        for it in range(T - 1):
            for _ in range(sub):
                a, b, _act = decide_torch(V[it], X, a_nom)
                k1 = dynamics(X, a, b)
                k2 = dynamics(X + .5 * dt * k1, a, b)
                k3 = dynamics(X + .5 * dt * k2, a, b)
                k4 = dynamics(X + dt * k3, a, b)
                X = X + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        return X

    def timed(variants, reps):
        ms = [[] for _ in variants]
        for rep in range(3 + reps):
            for k, (_, fn) in enumerate(variants):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 3:
                    ms[k].append(a.elapsed_time(b))
        return ms

    for M in (4096, 262144):
        X = torch.as_tensor(lo + rng.random((M, 3)) * (hi - lo), device="cuda")
        U = torch.zeros((M, T - 1, 1), dtype=torch.float64, device="cuda")

        def filt(nominal_value, keep_controls, keep=True):
            return safety.filtered_rollout_states(g, V, T, X, sid, sub, dt, plant, _fffi.SLICE_CLOCK, 0, None if nominal_value else U,
                                                  V if nominal_value else None, _rffi.MODE_MAX, level, margin, _fffi.DSTB_WORST, keep,
                                                  keep_controls)
        variants = [
            ("rollout_kernel (optimal controls, bisection, stops in the target)", lambda: rollout.rollout_states(g, V, X, sid, sub, dt, plant)),
            ("filtered, table nominal", lambda: filt(False, False)),
            ("filtered, table nominal, keepControls", lambda: filt(False, True)),
            ("filtered, value nominal", lambda: filt(True, False)),
            ("filtered, value nominal, keepControls", lambda: filt(True, True)),
            ("filtered, table nominal, no paths kept", lambda: filt(False, False, False)),
            ("per-step torch loop with a torch.where switch", lambda: torch_loop(X)),
        ]
        out = variants[0][1]()
        names = [_rffi.last_kernel()]
        steps = [int((out[1].to(torch.int64) - 1).sum()) * sub]
        for name, fn in variants[1:-1]:
            o = fn()
            names.append(_fffi.last_kernel())
            steps.append(M * nsteps)
        names.append("")
        steps.append(M * nsteps)
        acting = int(filt(False, False)[3].to(torch.int64).sum())
        ms = timed(variants, args.reps if M <= 4096 else max(5, args.reps // 4))
        base = float(np.median(ms[0]))
        lines.append("M = %d states (%d of their %d filtered sub-steps act):" % (M, acting, M * nsteps))
        for k, (name, _) in enumerate(variants):
            med = float(np.median(ms[k]))
            lines.append("  %-68s %10.3f (%.3f .. %.3f)   %10d sub-steps, %.3e sub-steps/s, %.2fx rollout_kernel's time   %s"
                         % (name, med, min(ms[k]), max(ms[k]), steps[k], steps[k] / (med * 1e-3), med / base,
                            names[k] if k < len(variants) - 1 else "torch operators; eval_u and eval_costate launch once per sub-step"))
        lines.append("")

    M = 10 ** 6
    X = torch.as_tensor(lo + rng.random((M, 3)) * (hi - lo), device="cuda")
    a_nom = torch.zeros(M, dtype=torch.float64, device="cuda")
    U1 = torch.zeros((M, 1), dtype=torch.float64, device="cuda")
    variants = [
        ("safeControls (decide_points_kernel)", lambda: safety.decide_states(g, V, 0, X, sid, plant, U1, level, margin, _fffi.DSTB_WORST)),
        ("eval_u + eval_costate + controls + torch.where", lambda: decide_torch(V[0], X, a_nom)),
    ]
    variants[0][1]()
    name = _fffi.last_kernel()
    ms = timed(variants, args.reps)
    lines.append("the decision at M = %d states, slice 0 of the stack:" % M)
    for k, (what, _) in enumerate(variants):
        med = float(np.median(ms[k]))
        lines.append("  %-68s %10.3f (%.3f .. %.3f)   %.3e states/s   %s" % (what, med, min(ms[k]), max(ms[k]), M / (med * 1e-3),
                                                                            name if k == 0 else "two point launches and torch operators"))
    lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
