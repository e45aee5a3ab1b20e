#!/usr/bin/env python3
"""Timing of computeOptTrajs with a plant registered at run time (levelsetpy_amd/plant.py, libhj_plant.so) on one MI355X
-> profiles/plant_timing.txt.

    python tools/plant_timing.py [--n 41] [--nq 11] [--reps 20] [--out FILE]

Part 1: DubinsVehicleRel registered again as text (tests/plant_cases.py) on the stack of tools/rollout_timing.py -- the air3D tube on
n^3 nodes, 11 stored sets, fp64, uMode 'max', dMode 'min', 4 sub-samples, as-shipped WENO5 costates -- against the built-in
rollout_kernel, which is what a registered plant is measured against, and against the host loop (computeOptTraj once per state).
Part 2: the planar quadrotor on the grid of examples/quadrotor_rollout.py (nq^4 x 16 x nq nodes, 5 stored sets, ENO2), which has no
built-in kernel, against the host loop.
M = 1, 4096 and 262144 states.  Device events around each call after a warm-up; the candidates take turns inside one process, call
by call; median of --reps calls (min and max beside it).  The host loop is timed by the host clock on a few states and reported per
state.  Also recorded: the wall time of the first call with an empty code-object cache (it compiles) and of the first call of a fresh
child process with the cache filled (it loads).

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here, and no ratio is promised.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SUB = 4


def turns(torch, fns, reps, warm=3):
    """ms of each of `reps` calls of every candidate, by device events; the candidates alternate call by call."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return [(float(np.median(ms)), float(min(ms)), float(max(ms))) for ms in out]


def dubins_setup(L, torch, n):
    import plant_cases as PC
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
    builtin = L.DubinsVehicleRel(g, 1.0, 1.0)
    sd = L.Bundle(dict(grid=g, hamFunc=builtin.hamiltonian, partialFunc=builtin.dissipation, dissFunc=L.artificialDissipationGLF,
                       CoStateCalc=L.upwindFirstWENO5))
    tau = np.linspace(0, 2.0, 11)
    stack, _, _ = L.HJIPDE_solve(L.shapeCylinder(g, 2, np.zeros((3, 1)), .5), tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True, flipOutput=True)))
    V = torch.as_tensor(np.asarray(stack), device="cuda")
    reg = PC.register_builtin("dubins")
    mine = PC.wrapped(reg, builtin, [1.0, 1.0, 1.0])
    lo, hi = np.array([0.0, -0.8, -np.pi]), np.array([2.2, 0.8, np.pi])
    return g, V, tau, builtin, mine, (lo, hi), L.Bundle(dict(uMode='max', dMode='min', subSamples=SUB))


def quad_setup(L, torch, nq):
    import plant_cases as PC
    nphi = 16
    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    top = 2 * np.pi * (1 - 1.0 / nphi)
    g = L.createGrid(col([-2, -3, -2, -3, 0, -4]), col([2, 3, 2, 3, top, 4]), col([nq, nq, nq, nq, nphi, nq], np.int64), [4], low_mem=True)
    q = PC.quadrotor(g)
    shape = tuple(int(v) for v in np.asarray(g.N).ravel())
    ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
    X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
    data0 = ((X[0] ** 2 + X[2] ** 2 + 0.25 * (X[1] ** 2 + X[3] ** 2)).sqrt() - 0.7).expand(shape).contiguous()
    tau = np.linspace(0.0, 0.2, 5)
    sd = L.Bundle(dict(grid=g, hamFunc=q.hamiltonian, partialFunc=q.dissipation, derivFunc=L.upwindFirstENO2))
    V, _, _ = L.HJIPDE_solve(data0, tau, sd, 'minVOverTime', L.Bundle(dict(quiet=True, flipOutput=True)))
    V = V if torch.is_tensor(V) else torch.as_tensor(np.asarray(V), device="cuda")
    lo, hi = np.array([-1.5, -0.5, -1.5, -0.5, -0.5, -0.5]), np.array([1.5, 0.5, 1.5, 0.5, 0.5, 0.5])
    return g, V, tau, None, q, (lo, hi), L.Bundle(dict(uMode='min', subSamples=SUB, derivFunc=L.upwindFirstENO2))


def first_call(which, n, nq):
    """Wall time of this process's first rollout of 4096 states with the registered plant, and what the cache did."""
    import torch
    import levelsetpy_amd as L
    g, V, tau, builtin, mine, (lo, hi), args = (dubins_setup(L, torch, n) if which == "dubins" else quad_setup(L, torch, nq))
    X = torch.as_tensor(lo + np.random.default_rng(0).random((4096, g.dim)) * (hi - lo), device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    L.computeOptTrajs(g, V, tau, mine, X, args)
    torch.cuda.synchronize()
    return dict(ms=1e3 * (time.perf_counter() - t0), stats=L.plant_kernel_cache_stats())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=41)
    ap.add_argument("--nq", type=int, default=11)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_timing.txt"))
    ap.add_argument("--first-call", choices=["dubins", "quad"], help="(internal) print the first call's time as JSON and exit")
    args = ap.parse_args()
    if args.first_call:
        print(json.dumps(first_call(args.first_call, args.n, args.nq)))
        return 0
    import torch
    assert torch.cuda.is_available(), "tools/plant_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import rollout
    prop = torch.cuda.get_device_properties(0)
    lines = ["computeOptTrajs with a registered plant on one MI355X (tools/plant_timing.py)",
             "device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "device events around each call, %d calls of every candidate after 3 warm-up calls, the candidates taking turns: median (min .. max) in ms" % args.reps, ""]

    # first call with an empty cache (compiles), then a fresh process with the cache filled (loads): two fresh children each
    with tempfile.TemporaryDirectory() as cache:
        for which in ("dubins", "quad"):
            env = dict(os.environ, HJ_RTC_CACHE=os.path.join(cache, which))
            got = []
            for _ in range(2):
                pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-call", which, "--n", str(args.n), "--nq", str(args.nq)],
                                    env=env, capture_output=True, text=True, timeout=600)
                assert pr.returncode == 0, pr.stderr[-2000:]
                got.append(json.loads(pr.stdout.strip().splitlines()[-1]))
            lines.append("first call of a process, %s plant, M = 4096 (host clock, kernel build included): %.1f ms with an empty cache (compiled, loaded) = %s; "
                         "%.1f ms in a second process (compiled, loaded) = %s" % (which, got[0]["ms"], tuple(got[0]["stats"]), got[1]["ms"], tuple(got[1]["stats"])))
    lines.append("")

    for part, setup in (("1: DubinsVehicleRel registered again, air3D tube on %d^3 nodes x 11 stored sets (fp64), as-shipped WENO5" % args.n,
                         lambda: dubins_setup(L, torch, args.n)),
                        ("2: planar quadrotor, %d^4 x 16 x %d nodes x 5 stored sets (fp64), ENO2" % (args.nq, args.nq), lambda: quad_setup(L, torch, args.nq))):
        g, V, tau, builtin, mine, (lo, hi), a = setup()
        lines.append("part " + part)
        rng = np.random.default_rng(0)
        for M in (1, 4096, 262144):
            X = torch.as_tensor(lo + rng.random((M, g.dim)) * (hi - lo), device="cuda")
            trajs, lengths, _ = L.computeOptTrajs(g, V, tau, mine, X, a)
            name = rollout.last_path()
            steps = int((lengths.to(torch.int64) - 1).sum()) * SUB
            fns = [lambda: L.computeOptTrajs(g, V, tau, mine, X, a)]
            if builtin is not None:
                ref = L.computeOptTrajs(g, V, tau, builtin, X, a)
                bname = rollout.last_path()
                equal = bool(torch.equal(torch.nan_to_num(ref[0]), torch.nan_to_num(trajs)) and torch.equal(ref[1], lengths))
                fns.append(lambda: L.computeOptTrajs(g, V, tau, builtin, X, a))
            t = turns(torch, fns, args.reps)
            lines.append("  M = %d: %d control steps in all (mean length %.2f of %d)" % (M, steps, float(lengths.double().mean()), len(tau)))
            lines.append("    %-58s %10.3f (%.3f .. %.3f)" % ((name,) + t[0]))
            if builtin is not None:
                lines.append("    %-58s %10.3f (%.3f .. %.3f)   registered / built-in = %.3f; the same trajectories bit for bit: %s"
                             % ((bname,) + t[1] + (t[0][0] / t[1][0], equal)))
            if M == 1 or M == 4096:
                k = 1 if M == 1 else 8
                xs = X[:k].cpu().numpy()
                rollout._host_loop(g, V, tau, mine, xs, a, False)
                runs = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rollout._host_loop(g, V, tau, mine, xs, a, False)
                    torch.cuda.synchronize()
                    runs.append(1e3 * (time.perf_counter() - t0) / k)
                lines.append("    host loop (host clock, %d state%s, per state)               %10.3f (%.3f .. %.3f)   %d states in the kernel take %.3gx one state's time in the loop"
                             % (k, "" if k == 1 else "s", float(np.median(runs)), min(runs), max(runs), M, t[0][0] / float(np.median(runs))))
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
