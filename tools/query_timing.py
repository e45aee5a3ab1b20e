#!/usr/bin/env python3
"""Timing of the value-function queries (levelsetpy_amd/query.py) on one MI355X -> profiles/query_timing.txt.

    python tools/query_timing.py [--n 201] [--T 21] [--parent-root DIR] [--commits TEXT] [--out FILE]

Workload: a fp64 value function on the n^3 Dubins-relative grid (heading periodic) with T stored sets, resident on
the device.  Measured, each as a host clock around work that ends in a device synchronisation, after a warm-up:

  (i)   one trajectory step of computeOptTraj (find_earliest_BRS_ind, then subSamples = 4 costate evaluations and plant
        updates).  With --parent-root DIR (a checkout of the parent commit's package; it binds this build's libhj_mi355x.so) the
        parent and this tree are timed in fresh child processes in the same session, ALTERNATING, several rounds.
  (ii)  eval_u and eval_costate at M = 1, 4096 and 10^6 states.
  (iii) proj 'min' over theta (one array and the T-stack) beside torch.amin, and a theta-slice of the T-stack.

This is a measurement tool, not the benchmark (bench.py), and no figure is asserted here except that (i) must not be
slower than the parent: the tool exits non-zero if it is.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Pursuer(object):
    """The dynSys protocol of computeOptTraj on the Dubins-relative grid: x' = (-1 + cos x3 + u x2, sin x3 - u x1, -u)."""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)

    def get_opt_u(self, t, deriv, uMode, x):
        det = deriv[0] * x[1] - deriv[1] * x[0] - deriv[2]
        s = 1.0 if det >= 0 else -1.0
        return -s if uMode == 'min' else s

    def update_state(self, u, dt, x, d=None):
        f = lambda z: np.array([-1.0 + np.cos(z[2]) + u * z[1], np.sin(z[2]) - u * z[0], -u])    # noqa: E731
        k1 = f(x); k2 = f(x + .5 * dt * k1); k3 = f(x + .5 * dt * k2); k4 = f(x + dt * k3)
        self.x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        return self.x


def workload(L, torch, n, T):
    """Grid and a T-stack of shrinking sets (index 0 the largest, as HJIPDE_solve's flipped output): a cylinder whose
    radius falls from 1.7 to 0.5, bent so that the costates are not constant."""
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2, low_mem=True)
    vs = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
    x, y, th = vs[0][:, None, None], vs[1][None, :, None], vs[2][None, None, :]
    base = torch.sqrt(x * x + y * y) + 0.15 * torch.sin(th) * x
    radii = np.linspace(1.7, 0.5, T)
    return g, torch.stack([base - r for r in radii])


def sync_time(torch, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def traj_step_ms(L, torch, g, data, reps):
    """ms per trajectory step: whole computeOptTraj calls over the number of steps they took."""
    tau = np.linspace(0, 1.2, data.shape[0])
    extra = L.Bundle(dict(uMode='min', subSamples=4))
    out = []
    for r in range(reps + 1):
        plant = Pursuer([1.4, 0.3, 2.9])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        traj, _ = L.computeOptTraj(g, data, tau, plant, extra)
        torch.cuda.synchronize()
        if r:                                                   # the first call is the warm-up
            out.append(1e3 * (time.perf_counter() - t0) / max(1, traj.shape[1] - 1))
    return out, traj


def child(args):
    sys.path.insert(0, args.root)
    import torch
    import levelsetpy_amd as L
    assert os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))) == os.path.abspath(args.root)
    g, data = workload(L, torch, args.n, args.T)
    ms, traj = traj_step_ms(L, torch, g, data, args.reps)
    print(json.dumps(dict(label=args.label, ms=ms, steps=int(traj.shape[1] - 1), end=[float(v) for v in traj[:, -1]])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=201)
    ap.add_argument("--T", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--commits", default="not given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_timing.txt"))
    ap.add_argument("--root", default=None, help="child mode: time the trajectory step of the package under this root")
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    if args.root:
        return child(args)

    lines = ["Value-function queries on one MI355X: %d^3 fp64 Dubins-relative value function, T = %d stored sets" % (args.n, args.T),
             "tools/query_timing.py; commits: %s" % args.commits,
             "host clock around work that ends in a device synchronisation, after warm-up", ""]
    # (i) alternating child processes
    runs = {"parent": [], "this": []}
    ends = {}
    roots = [("parent", args.parent_root), ("this", ROOT)] if args.parent_root else [("this", ROOT)]
    for r in range(args.rounds):
        for label, root in roots:
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--label", label, "--n", str(args.n),
                   "--T", str(args.T), "--reps", str(args.reps)]
            # the parent's package binds the library of THIS build (HJ_LIB): the same kernels under both
            env = dict(os.environ, HJ_LIB=os.path.join(ROOT, "levelsetpy_amd", "csrc", "libhj_mi355x.so"))
            res = json.loads(subprocess.check_output(cmd, timeout=600, env=env).decode().strip().splitlines()[-1])
            runs[label].append(res["ms"])
            ends[label] = (res["steps"], res["end"])
            print("round %d %-6s %s ms per trajectory step (%d steps)" % (r, label, ["%.2f" % v for v in res["ms"]], res["steps"]), flush=True)
    lines.append("(i) computeOptTraj, ms per trajectory step (subSamples = 4), %d rounds alternating, %d calls each:" % (args.rounds, args.reps))
    med = {}
    for label, _ in roots:
        flat = [v for rr in runs[label] for v in rr]
        med[label] = float(np.median(flat))
        lines.append("    %-7s median %9.3f   min %9.3f   max %9.3f   per round %s" % (
            label, med[label], min(flat), max(flat), ["%.3f" % float(np.median(rr)) for rr in runs[label]]))
    if args.parent_root:
        same = ends["parent"] == ends["this"]
        lines.append("    same number of steps and the same final state, bit for bit: %s" % same)
        lines.append("    speed-up of the trajectory step: %.1fx" % (med["parent"] / med["this"]))
    lines.append("")

    sys.path.insert(0, ROOT)
    import torch
    import levelsetpy_amd as L
    g, data = workload(L, torch, args.n, args.T)
    rng = np.random.default_rng(0)
    lo = np.array([float(np.asarray(v).ravel()[0]) for v in g.vs])
    hi = np.array([float(np.asarray(v).ravel()[-1]) for v in g.vs])
    lines.append("(ii) at M states, one stored set (us per call; the 10^6 rows also as states per second):")
    for M in (1, 4096, 10 ** 6):
        X = torch.as_tensor(lo + rng.random((M, 3)) * (hi - lo), device="cuda")
        reps = 200 if M < 10 ** 6 else 20
        tu = sync_time(torch, lambda: L.eval_u(g, data[3], X), reps)
        tc = sync_time(torch, lambda: L.eval_costate(g, data[3], X), reps)
        tcs = sync_time(torch, lambda: L.eval_costate(g, data, X[:max(1, M // args.T)]), reps)
        lines.append("    M = %-8d eval_u %10.1f   eval_costate %10.1f   eval_costate on the T-stack at M/T states %10.1f%s" % (
            M, 1e6 * tu, 1e6 * tc, 1e6 * tcs,
            "   (%.2e / %.2e states per second)" % (M / tu, M / tc) if M >= 10 ** 6 else ""))
    lines.append("")
    lines.append("(iii) projections (us per call; bytes read / time in GB/s):")
    one, nb = data[3], data[3].numel() * 8
    for name, fn, b in (("proj min over theta, one array", lambda: L.proj(g, one, [0, 0, 1], 'min'), nb),
                        ("torch.amin(dim=-1), one array", lambda: torch.amin(one, dim=-1), nb),
                        ("proj min over theta, T-stack", lambda: L.proj(g, data, [0, 0, 1], 'min'), nb * args.T),
                        ("torch.amin(dim=-1), T-stack", lambda: torch.amin(data, dim=-1), nb * args.T),
                        ("proj min over x (last axis kept), one array", lambda: L.proj(g, one, [1, 0, 0], 'min'), nb),
                        ("torch.amin(dim=0), one array", lambda: torch.amin(one, dim=0), nb),
                        ("proj theta-slice of the T-stack", lambda: L.proj(g, data, [0, 0, 1], [0.3]), None)):
        t = sync_time(torch, fn, 20)
        lines.append("    %-46s %10.1f%s" % (name, 1e6 * t, "   %7.1f GB/s" % (b / t / 1e9) if b else ""))
    assert torch.equal(L.proj(g, data, [0, 0, 1], 'min')[1], torch.amin(data, dim=-1))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if args.parent_root and med["this"] > med["parent"]:
        print("the trajectory step is SLOWER than the parent's: a defect to find")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
