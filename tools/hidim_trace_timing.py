#!/usr/bin/env python3
"""What Python callbacks traced into hidim_substep_kernel cost on 5-D / 6-D grids (levelsetpy_amd/trace_ham.py, set_hidim_trace)
-> profiles/hidim_trace_timing.txt.

    python tools/hidim_trace_timing.py [--shapes 41x5,25x6] [--reps 7] [--out FILE]

Workload: tools/hidim_user_timing.py's -- 41^5 and 25^6 nodes, fp64, a smooth field plus seeded noise made on the device -- with the as-shipped
WENO5 and with ENO2.  The systems are tests/hidim_trace_cases.py's, written as callbacks only: Plane5D (5-D), DubinsPair6D and the planar
quadrotor with np.sin / np.cos inside the callbacks (6-D).  One substep (HJ_STAGE_EULER), the candidates taking turns in one process, device
events around each after a warm-up, median of the repetitions (min .. max beside it):
  native            the built-in kernel (Plane5D, DubinsPair6D) or the expression registered by hand (the quadrotor, tests/hidim_user_cases.py)
  traced            the kernel generated from the callbacks (tables hoisted)
  traced, no hoist  the quadrotor traced under HJ_TRACE_HOIST=off: device sin / cos per cell
  split term        termLaxFriedrichs of the same callbacks with the switch off (the path they take without this tracer)
and, per system, what the FIRST call costs: trace + run-time compile (the disk cache is off for this tool unless HJ_RTC_CACHE is set) +
the verification against the split path, wall clock, with the peak of device memory allocated during it beside the size of one array.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HJ_RTC_CACHE", "0")

from hidim_timing import event_ms, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="41x5,25x6", help="comma-separated NxD: N nodes on each of D axes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hidim_trace_timing.txt"))
    args = ap.parse_args()
    import torch
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _hffi, hidim, term
    import hidim_trace_cases as TC
    import hidim_user_cases as UC
    if not torch.cuda.is_available():
        print("hidim_trace_timing needs an MI355X: no device, nothing is measured", file=sys.stderr)
        return 2
    props = torch.cuda.get_device_properties(0)
    lines = ["One fp64 substep on one MI355X: hamFunc / partialFunc traced into hidim_substep_kernel (set_hidim_trace) beside the native kernel and the split path",
             "tools/hidim_trace_timing.py; device %s (%s), HIP %s, torch %s" % (props.name, getattr(props, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the candidates take turns in one process; device events around each; median (min .. max) in ms; %d repetitions after a warm-up" % args.reps, ""]
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    for spec in args.shapes.split(","):
        n, nd = (int(v) for v in spec.split("x"))
        cells = n ** nd
        systems = ["plane"] if nd == 5 else ["pair", "quad"]
        for which in systems:
            pd = {"plane": [2], "pair": [2, 5], "quad": [4]}[which]
            lo, hi = [-2.0] * nd, [2.0] * nd
            for d in pd:
                lo[d], hi[d] = 0.0, 2 * np.pi * (1 - 1.0 / n)
            g = L.createGrid(col(lo, np.float64), col(hi, np.float64), col([n] * nd, np.int64), pd, low_mem=True)
            vs_host = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
            if which == "plane":
                nat_sys = L.Plane5D(g, 0.8, 1.3, 'min')
                nat_ham, nat_par = nat_sys.native()
                nat_obj = None
                cb = TC.PlanePair(g, 0.8, 1.3, 'min')
            elif which == "pair":
                nat_sys = L.DubinsPair6D(g, 1.5, 1.1, 0.9, 1.4)
                nat_ham, nat_par = nat_sys.native()
                nat_obj = None
                cb = TC.DubinsPair(g, 1.5, 1.1, 0.9, 1.4)
            else:
                reg = L.register_hidim_hamiltonian("planar_quad", 6, UC.QUAD_SRC, nparams=8, aux_axes=UC.QUAD_AXES)
                nat_obj = reg(g, UC.QUAD_PAR, tables=UC.quad_tables(vs_host))
                nat_ham, nat_par = reg.ham_id, list(UC.QUAD_PAR)
                cb = TC.QuadInline(g, UC.QUAD_PAR)
            hg = hidim.hi_grid(g, "float64")
            vs = [torch.as_tensor(v, dtype=torch.float64, device="cuda") for v in vs_host]
            shp = lambda d: [n if k == d else 1 for k in range(nd)]      # noqa: E731
            x0, x1, xl = vs[0].reshape(shp(0)), vs[1].reshape(shp(1)), vs[nd - 1].reshape(shp(nd - 1))
            base = (x0 * x0 + x1 * x1 + 0.01).sqrt() - 1 + 0.05 * (3 * x0).sin() * (2 * xl).cos()
            gen = torch.Generator(device="cuda").manual_seed(7)
            y = (base.expand([n] * nd) + 0.02 * torch.randn([n] * nd, generator=gen, device="cuda", dtype=torch.float64)).contiguous()
            del base
            out = torch.empty_like(y)
            lines.append("%s, %d^%d = %.3e cells, float64; one array %.2f GB" % ({"plane": "Plane5D", "pair": "DubinsPair6D", "quad": "planar quadrotor"}[which],
                                                                               n, nd, cells, cells * 8 / 1e9))
            for scheme, sid, deriv in (("as-shipped WENO5", _ffi.WENO5_ASSHIPPED, L.upwindFirstWENO5), ("ENO2", _ffi.ENO2, L.upwindFirstENO2)):
                def bundle(s):
                    return L.Bundle(dict(grid=g, dissFunc=L.artificialDissipationGLF, derivFunc=deriv, hamFunc=s.hamiltonian, partialFunc=s.dissipation))

                def first_call(s, hoist=None):
                    """(plan, seconds, peak bytes, kernels compiled) of the first use of the callbacks of s with the switch on."""
                    if hoist is not None:
                        os.environ["HJ_TRACE_HOIST"] = hoist
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before, made = torch.cuda.memory_allocated(), L.hidim_kernel_cache_stats()[0]
                    L.set_hidim_trace(True)
                    try:
                        t0 = time.perf_counter()
                        yd = L.termLaxFriedrichs(0.0, y.reshape(-1, 1), bundle(s))[0]
                        torch.cuda.synchronize()
                        sec = time.perf_counter() - t0
                        path = hidim.last_path()
                        plan = term.native_plan(bundle(s), y.reshape(-1, 1))
                    finally:
                        L.set_hidim_trace(False)
                        os.environ.pop("HJ_TRACE_HOIST", None)
                    del yd
                    if plan is None or "HamUser:traced_" not in path:
                        raise RuntimeError("%s was not traced: %s" % (type(s).__name__, L.explain_plan(bundle(s))))
                    return plan, sec, torch.cuda.max_memory_allocated() - before, L.hidim_kernel_cache_stats()[0] - made
                plan, sec, peak, made = first_call(cb)
                if sid == _ffi.WENO5_ASSHIPPED:
                    firsts = ["first call of the traced term (trace + %d kernels compiled + verification against the split path): %.2f s; peak device "
                              "memory during it %.2f GB beyond the state = %.1f arrays" % (made, sec, peak / 1e9, peak / (cells * 8.0))]
                else:
                    firsts = ["first call of the traced term with another scheme (trace + %d kernel compiled; verified already): %.2f s; peak device "
                              "memory during it %.2f GB beyond the state = %.1f arrays" % (made, sec, peak / 1e9, peak / (cells * 8.0))]
                cands = [("native", nat_ham, nat_par, hg.tables_of(nat_obj)[0] if nat_obj is not None else None),
                         ("traced", plan[2], list(plan[3]), hg.tables_of(plan.system)[0])]
                keepalive = [plan]
                if which == "quad":
                    cb2 = TC.QuadInline(g, UC.QUAD_PAR)
                    plan2, sec2, _, made2 = first_call(cb2, hoist="off")
                    keepalive.append(plan2)
                    cands.append(("traced, no hoist", plan2[2], list(plan2[3]), hg.tables_of(plan2.system)[0]))
                sb = hg.step_bound(nat_ham, nat_par, nat_obj)
                dt = 0.8 * sb
                names = {}

                def substep_of(label, hm, pr, tab):
                    def run():
                        hidim._substep(hg, sid, hm, pr, _ffi.STAGE_EULER, 0, y, None, out, dt, tab=tab)
                        names.setdefault(label, _hffi.last_kernel())
                    return run
                keep = []
                sd_split = bundle(cb)

                def run_split():
                    keep[:] = [L.termLaxFriedrichs(0.0, y.reshape(-1, 1), sd_split)[0]]
                runs = [(label, substep_of(label, hm, pr, tab)) for label, hm, pr, tab in cands] + [("split term", run_split)]
                results = {}
                for label, run in runs[:-1]:
                    run()
                    results[label] = out.clone()
                run_split()
                assert hidim.last_path() != names["traced"]
                torch.cuda.synchronize()
                scale = float(results["native"].abs().max())
                agree = ", ".join("%s %.2e" % (k, float((results[k] - results["native"]).abs().max()) / scale) for k in results if k != "native")
                del results
                times = dict((label, []) for label, _ in runs)
                for _ in range(args.reps):
                    for label, run in runs:
                        times[label].append(event_ms(torch, run))
                keep[:] = []
                lines.append("  %s" % scheme)
                ref = stats(times["native"])[0]
                for label, _ in runs:
                    med, lo_, hi_ = stats(times[label])
                    lines.append("    %-17s %9.3f (%.3f .. %.3f)   %.3e cell-substeps/s   %5.2fx the native kernel   %s" % (
                        label, med, lo_, hi_, cells / (med * 1e-3), med / ref, names.get(label, "hjh_upwind, callbacks and dissipation as torch expressions")))
                lines.append("    max |candidate - native| / max |native| of the substep's output: %s" % agree)
                for f in firsts:
                    lines.append("    " + f)
                del keepalive
            lines.append("")
            del y, out
            torch.cuda.empty_cache()
    text = "\n".join(lines[:-1]) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
