#!/usr/bin/env python3
"""Timing of the 5-D / 6-D queries (levelsetpy_amd/query.py and rollout.py on libhj_hiquery.so) on one MI355X
-> profiles/hiquery_timing.txt.

    python tools/hiquery_timing.py [--shapes 41x5,25x6] [--reps 7] [--states 100000] [--out FILE]

Three sections; in each the candidates take turns in one process, device events around each after a warm-up, median of the
repetitions (min .. max beside it):
  projection   proj(..., 'min') over four axes and over one axis (the first ones: the last axis is kept; and the last ones: it
               is removed), fp64 and fp32, against torch.amin over the same axes and against clone() of the input -- one read
               and one write of the array, more than a projection has to move: the streaming floor
  point query  eval_u and eval_costate (as-shipped WENO5 and ENO2) at --states random states, fp64, against the route they
               replace: computeGradients over the whole grid, then eval_u on each of its derivC arrays
  rollout      computeOptTrajs for M = 1, 4096 and 262144 joint states through a five-slice stack on the 6-D grid of
               examples/six_d_queries.py (13^4 x 12^2), against the host loop (computeOptTraj per state) on four states, scaled

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def turns(torch, cands, reps):
    """name -> times (ms): a warm-up of every candidate, then `reps` rounds in which they take turns."""
    for _, run in cands:
        run()
    torch.cuda.synchronize()
    times = dict((name, []) for name, _ in cands)
    for _ in range(reps):
        for name, run in cands:
            times[name].append(event_ms(torch, run))
    return times


def make_grid(L, n, nd, nth=None):
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    pd = [2] if nd == 5 else [2, 5]
    N = [n] * nd
    lo, hi = [-2.0] * nd, [2.0] * nd
    for d in pd:
        N[d] = nth or n
        lo[d], hi[d] = 0.0, 2 * np.pi * (1 - 1.0 / N[d])
    return L.createGrid(col(lo, np.float64), col(hi, np.float64), col(N, np.int64), pd, low_mem=True), N


def field(torch, g, N, td, pair=False):
    """A smooth field plus seeded noise, made on the device; pair: the distance of the two vehicles' positions."""
    nd = len(N)
    vs = [torch.as_tensor(np.asarray(v).ravel(), dtype=torch.float64, device="cuda") for v in g.vs]
    shp = lambda d: [N[k] if k == d else 1 for k in range(nd)]      # noqa: E731
    x = [vs[d].reshape(shp(d)) for d in range(nd)]
    if pair:
        base = ((x[0] - x[3]) ** 2 + (x[1] - x[4]) ** 2 + 0.01).sqrt() - 0.8
    else:
        base = (x[0] * x[0] + x[1] * x[1] + 0.01).sqrt() - 1 + 0.05 * (3 * x[0]).sin() * (2 * x[nd - 1]).cos()
    gen = torch.Generator(device="cuda").manual_seed(7)
    return (base.expand(N) + 0.02 * torch.randn(N, generator=gen, device="cuda", dtype=torch.float64)).to(td).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="41x5,25x6", help="comma-separated NxD: N nodes on each of D axes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--states", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hiquery_timing.txt"))
    args = ap.parse_args()
    import torch
    import levelsetpy_amd as L
    from levelsetpy_amd import _xffi, rollout
    if not torch.cuda.is_available():
        print("hiquery_timing needs an MI355X: no device, nothing is measured", file=sys.stderr)
        return 2
    props = torch.cuda.get_device_properties(0)
    lines = ["5-D / 6-D queries on one MI355X: libhj_hiquery.so through proj, eval_u, eval_costate and computeOptTrajs",
             "tools/hiquery_timing.py; device %s (%s), HIP %s, torch %s" % (props.name, getattr(props, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the candidates take turns in one process; device events around each; median (min .. max) in ms; %d repetitions after a warm-up" % args.reps, ""]

    # ---- projection
    lines.append("PROJECTION: proj(g, data, mask, 'min') against torch.amin over the same axes and clone() of the input")
    for spec in args.shapes.split(","):
        n, nd = (int(v) for v in spec.split("x"))
        g, N = make_grid(L, n, nd)
        cells = n ** nd
        for dtype, td, esz in (("float64", torch.float64, 8), ("float32", torch.float32, 4)):
            y = field(torch, g, N, td)
            keep = []
            for what, axes in (("four axes, last axis kept", tuple(range(4))), ("four axes, last axis removed", tuple(range(nd - 4, nd))),
                               ("one axis (the first), last axis kept", (0,)), ("one axis (the last) removed", (nd - 1,))):
                mask = [1 if d in axes else 0 for d in range(nd)]
                cands = [("proj", lambda: keep.__setitem__(slice(None), [L.proj(g, y, mask, 'min', process=False)[1]])),
                         ("torch.amin", lambda: keep.__setitem__(slice(None), [torch.amin(y, dim=axes)])),
                         ("clone", lambda: keep.__setitem__(slice(None), [y.clone()]))]
                t = turns(torch, cands, args.reps)
                assert torch.equal(L.proj(g, y, mask, 'min', process=False)[1], torch.amin(y, dim=axes))
                kernel = _xffi.last_kernel()
                lines.append("%d^%d = %.3e cells, %s (%.2f GB), min over %s: %s" % (n, nd, cells, dtype, cells * esz / 1e9, what, kernel))
                for name, _ in cands:
                    med, lo_, hi_ = stats(t[name])
                    lines.append("  %-11s %10.3f (%.3f .. %.3f)   %.3f of 8 TB/s on the input's bytes" % (name, med, lo_, hi_, cells * esz / (med * 1e-3) / 8e12))
                mp, ma, mc = (stats(t[k])[0] for k in ("proj", "torch.amin", "clone"))
                lines.append("  proj / torch.amin = %.2f;  proj / clone = %.2f" % (mp / ma, mp / mc))
            keep[:] = []
            del y
            torch.cuda.empty_cache()
        lines.append("")

    # ---- point queries
    M = args.states
    lines.append("POINT QUERIES at %d random states, fp64: the kernels against computeGradients over the whole grid + eval_u per derivC array" % M)
    for spec in args.shapes.split(","):
        n, nd = (int(v) for v in spec.split("x"))
        g, N = make_grid(L, n, nd)
        y = field(torch, g, N, torch.float64)
        lo = torch.as_tensor([float(np.asarray(v).ravel()[0]) for v in g.vs], device="cuda")
        hi = torch.as_tensor([float(np.asarray(v).ravel()[-1]) for v in g.vs], device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(3)
        xs = (lo + torch.rand((M, nd), generator=gen, device="cuda", dtype=torch.float64) * (hi - lo)).contiguous()
        keep = []
        t = turns(torch, [("eval_u", lambda: keep.__setitem__(slice(None), [L.eval_u(g, y, xs)]))], args.reps)
        med, lo_, hi_ = stats(t["eval_u"])
        mu = med
        lines.append("%d^%d, eval_u: %s" % (n, nd, _xffi.last_kernel()))
        lines.append("  %-26s %10.3f (%.3f .. %.3f)   %.3e states/s" % ("eval_u", med, lo_, hi_, M / (med * 1e-3)))
        for scheme, fn in (("as-shipped WENO5", L.upwindFirstWENO5), ("ENO2", L.upwindFirstENO2)):
            def route():
                dC, _, _ = L.computeGradients(g, y, derivFunc=fn)
                keep[:] = [torch.stack([L.eval_u(g, dC[d], xs) for d in range(nd)], dim=-1)]
            cands = [("eval_costate", lambda: keep.__setitem__(slice(None), [L.eval_costate(g, y, xs, fn)])), ("computeGradients + eval_u", route)]
            t = turns(torch, cands, max(3, args.reps // 2))
            L.eval_costate(g, y, xs, fn)
            lines.append("%d^%d, eval_costate, %s: %s" % (n, nd, scheme, _xffi.last_kernel()))
            for name, _ in cands:
                med, lo_, hi_ = stats(t[name])
                lines.append("  %-26s %10.3f (%.3f .. %.3f)   %.3e states/s" % (name, med, lo_, hi_, M / (med * 1e-3)))
            lines.append("  computeGradients + eval_u / eval_costate = %.1f;  eval_costate / eval_u = %.1f" % (
                stats(t["computeGradients + eval_u"])[0] / stats(t["eval_costate"])[0], stats(t["eval_costate"])[0] / mu))
            keep[:] = []
            torch.cuda.empty_cache()
        del y, xs
        torch.cuda.empty_cache()
    lines.append("")

    # ---- rollout
    g, N = make_grid(L, 13, 6, nth=12)
    T = 5
    tau = np.linspace(0.0, 0.4, T)
    base = field(torch, g, N, torch.float64, pair=True)
    data = torch.stack([base + 0.12 * k for k in range(T)]).contiguous()          # the sets shrink along the time axis
    pair = L.DubinsPair6D(g, 1.0, 1.0, 1.0, 1.0)
    args_r = L.Bundle(dict(uMode='max', dMode='min', subSamples=4, derivFunc=L.upwindFirstENO2))
    lo = torch.as_tensor([float(np.asarray(v).ravel()[0]) for v in g.vs], device="cuda")
    hi = torch.as_tensor([float(np.asarray(v).ravel()[-1]) for v in g.vs], device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    lines.append("ROLLOUT: computeOptTrajs, DubinsPair6D on %s, %d stored sets, 4 sub-samples, ENO2, fp64" % ("x".join(str(v) for v in N), T))
    x4 = (lo + 0.25 * (hi - lo) + 0.5 * torch.rand((4, 6), generator=gen, device="cuda", dtype=torch.float64) * (hi - lo)).contiguous()
    system = L.DubinsPair6D(g, 1.0, 1.0, 1.0, 1.0)
    system.get_opt_u = lambda t, deriv, uMode, x: L.DubinsPair6D.get_opt_u(pair, t, deriv, uMode, x)      # an instance attribute: the host loop
    L.computeOptTrajs(g, data, tau, system, x4, args_r)
    assert rollout.last_path().startswith("host loop")
    t0 = time.perf_counter()
    _, lens, _ = L.computeOptTrajs(g, data, tau, system, x4, args_r)
    torch.cuda.synchronize()
    per_state = (time.perf_counter() - t0) * 1e3 / 4
    lines.append("  host loop (computeOptTraj per state): %.2f ms per state (wall clock, 4 states, lengths %s)" % (per_state, lens.tolist()))
    for M in (1, 4096, 262144):
        xs = (lo + 0.25 * (hi - lo) + 0.5 * torch.rand((M, 6), generator=gen, device="cuda", dtype=torch.float64) * (hi - lo)).contiguous()
        keep = []
        t = turns(torch, [("kernel", lambda: keep.__setitem__(slice(None), [L.computeOptTrajs(g, data, tau, pair, xs, args_r)]))], args.reps)
        med, lo_, hi_ = stats(t["kernel"])
        lengths = keep[0][1]
        lines.append("  M = %6d: %s %10.3f (%.3f .. %.3f)   %.3e trajectories/s; mean length %.2f; host loop scaled to M: %.3e ms, %.0f times the launch" % (
            M, rollout.last_path(), med, lo_, hi_, M / (med * 1e-3), float(lengths.double().mean()), per_state * M, per_state * M / med))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
