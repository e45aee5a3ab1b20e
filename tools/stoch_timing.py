#!/usr/bin/env python3
"""Timing of stochastic reachability (levelsetpy_amd/stochastic.py, libhj_stoch.so) on one MI355X -> profiles/stoch_timing.txt.

    python tools/stoch_timing.py [--sizes 51,101,201] [--steps 4] [--reps 7] [--out FILE]

Workload: one tau interval of the air3D problem (examples/air3d_brt.py: DubinsVehicleRel with unit bounds, the cylinder target,
minVOverTime) on n^3 nodes, fp64, as-shipped WENO5, with a dense sigma and with a diagonal sigma, each scaled so that the trace
term's step bound equals the Lax-Friedrichs term's.  The interval is `--steps` time steps of the noisy problem long.  Per
configuration four candidates take turns in one process, device events around each after a warm-up, median of the repetitions
(min .. max beside it):
  fused          hjw_integrate: 3 launches of stoch_substep_kernel per step, nothing else
  generic        the termSum route on device tensors, as HJIPDE_solve drives it: per stage the Lax-Friedrichs kernel, the Hessian
                 kernel, a tensor add and the stage kernel, a host round trip for the step bound; the min with the previous step
  deterministic  the fused solve of the SAME interval without noise (hj_rk_integrate): the floor of the fused route.  Its step
                 bound is the Lax-Friedrichs term's alone, so it takes fewer, longer steps; it is reported per step of its own
  clone          torch's clone() of the state: one read and one write of it, the streaming floor of a substep
Times are per problem-step (an RK3 step: three substeps).  Loads per cell and substep, as the kernels issue them in 3-D: 18
stencil neighbours + the cell for the Lax-Friedrichs term; the general instantiation adds 2 nd (nd - 1) = 12 diagonal neighbours,
the diagonal one none.

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here.
"""
import argparse
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="51,101,201")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoch_timing.txt"))
    args = ap.parse_args()
    import torch
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _marshal, _wffi, stochastic as ST
    from levelsetpy_amd.batch import plan_interval
    from levelsetpy_amd.integration import integrate_span_device
    if not torch.cuda.is_available():
        print("stoch_timing needs an MI355X: no device, nothing is measured", file=sys.stderr)
        return 2
    props = torch.cuda.get_device_properties(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = ["stochastic reachability on one MI355X: one tau interval of the air3D problem, fp64, as-shipped WENO5, minVOverTime",
             "tools/stoch_timing.py; device %s (%s), HIP %s, torch %s" % (props.name, getattr(props, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the candidates take turns in one process; device events around each; median (min .. max) in ms per problem-step (RK3: three "
             "substeps); %d repetitions after a warm-up; the interval is %d noisy steps long" % (args.reps, args.steps), ""]
    opts = L.odeCFLset(L.Bundle({'factorCFL': 0.8, 'singleStep': 'on'}))
    for n in [int(v) for v in args.sizes.split(",")]:
        gmin = np.array([[-.75, -1.25, -np.pi]]).T
        gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
        g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
        data0 = L.shapeCylinder(g, 2, np.zeros((3, 1)), 0.5)
        sys_ = L.DubinsVehicleRel(g, 1, 1)
        ham, par = sys_.native()
        sd = L.Bundle(dict(grid=g, hamFunc=sys_.hamiltonian, partialFunc=sys_.dissipation, dissFunc=L.artificialDissipationGLF,
                           derivFunc=L.upwindFirstWENO5))
        y0 = torch.as_tensor(np.ascontiguousarray(data0), dtype=torch.float64, device=dev).reshape(-1)
        cells = y0.numel()
        rng = np.random.default_rng(5)
        shapes = {"dense": np.eye(3) + 0.4 * rng.uniform(-1, 1, (3, 3)), "diagonal": np.diag([1.0, 1.3, 1.6])}
        for key, M in shapes.items():
            _, sb_lf, sb_th = ST.step_bound(g, ham, par, M)
            sigma = np.sqrt(sb_th / sb_lf) * M                       # sb_TH(c M) = sb_TH(M) / c^2
            call = ST._Call(g, ham, _ffi.WENO5_ASSHIPPED, par, sigma, torch, dev)
            sb, sb_lf, sb_th = call.step_bound()
            tf = (args.steps - 0.5) * 0.8 * sb
            a, b, w = torch.empty_like(y0), torch.empty_like(y0), torch.empty_like(y0)
            count = {}

            def fused():
                _, count["fused"], _ = call.integrate(sb, y0, a, b, w, 0.0, tf, 3, 0, _ffi.POST_MIN_PREV)

            f, data = ST.noise_scheme('numbers', sigma, g, L.termLaxFriedrichs, sd)

            def generic():
                t, y, k = 0.0, y0.reshape(-1, 1), 0
                while t < tf - ST.SMALL:
                    last = y
                    t, y, _ = L.odeCFL3(f, [t, tf], y, opts, data)
                    y = torch.minimum(_marshal.unlazy(y), last)
                    k += 1
                count["generic"] = k

            def deterministic():
                integrate_span_device(L.termLaxFriedrichs, sd, y0.reshape(-1, 1), 0.0, tf, opts, ST.SMALL, _ffi.POST_MIN_PREV)
                count["deterministic"] = len(plan_interval(sb_lf, 0.0, tf)[0])

            def clone():
                y0.clone()
                count["clone"] = 1

            cands = [("fused", fused), ("generic", generic), ("deterministic", deterministic), ("clone", clone)]
            for _, fn in cands:
                fn()
            torch.cuda.synchronize()
            ms = dict((k, []) for k, _ in cands)
            for _ in range(args.reps):
                for k, fn in cands:
                    ms[k].append(event_ms(torch, fn) / count[k])
            kernel = _wffi.kernel_name(ham, _ffi.WENO5_ASSHIPPED, key == "diagonal")
            lines.append("%d^3 = %.3e cells, %s sigma: %s; %d loads per cell and substep; sb_LF %.4g, sb_TH %.4g, sb %.4g"
                         % (n, cells, key, kernel, 19 + (0 if key == "diagonal" else 12), sb_lf, sb_th, sb))
            med = {}
            for k, _ in cands:
                m, lo, hi = stats(ms[k])
                med[k] = m
                extra = "" if k == "clone" else "   %d step%s in the interval   %.3e cell-steps/s" % (count[k], "" if count[k] == 1 else "s", cells / (m * 1e-3))
                lines.append("  %-14s %9.3f (%.3f .. %.3f)%s" % (k, m, lo, hi, extra))
            lines.append("  generic / fused = %.2f;  fused / deterministic = %.2f;  fused / (3 clones) = %.2f"
                         % (med["generic"] / med["fused"], med["fused"] / med["deterministic"], med["fused"] / (3 * med["clone"])))
            lines.append("")
            print("\n".join(lines[-7:]), flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines).rstrip() + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
