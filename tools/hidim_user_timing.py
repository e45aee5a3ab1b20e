#!/usr/bin/env python3
"""What a registered 5-D / 6-D Hamiltonian costs beside the built-in kernel (levelsetpy_amd/hidim_ham.py) -> profiles/hidim_user_timing.txt.

    python tools/hidim_user_timing.py [--shapes 41x5,25x6] [--reps 7] [--out FILE]

Workload: tools/hidim_timing.py's -- Plane5D on 41^5 nodes and DubinsPair6D on 25^6 nodes, fp64, the as-shipped WENO5, a smooth field plus
seeded noise made on the device.  One substep (HJ_STAGE_EULER), four candidates taking turns in one process, device events around each after
a warm-up, median of the repetitions (min .. max beside it):
  built-in          hidim_substep_kernel<double, HamPlane5D | HamDubinsPair6D, 3>, compiled with the library
  registered        the same system as an expression over tables (tests/hidim_user_cases.py), compiled at run time around HamUser
  registered, trig  the same expression with device sin / cos of the coordinate in place of the tables
  split term        termLaxFriedrichs with the system's methods handed over as plain callbacks
The ratios are against the built-in kernel of the same run.

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hidim_timing import event_ms, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="41x5,25x6", help="comma-separated NxD: N nodes on each of D axes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hidim_user_timing.txt"))
    args = ap.parse_args()
    import torch
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _hffi, hidim
    import hidim_user_cases as UC
    if not torch.cuda.is_available():
        print("hidim_user_timing needs an MI355X: no device, nothing is measured", file=sys.stderr)
        return 2
    props = torch.cuda.get_device_properties(0)
    lines = ["One fp64 substep of the as-shipped WENO5 on one MI355X: a Hamiltonian registered at run time beside the built-in kernel (libhj_hidim.so)",
             "tools/hidim_user_timing.py; device %s (%s), HIP %s, torch %s" % (props.name, getattr(props, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the candidates take turns in one process; device events around each; median (min .. max) in ms; %d repetitions after a warm-up" % args.reps, ""]
    sid = _ffi.WENO5_ASSHIPPED
    for spec in args.shapes.split(","):
        n, nd = (int(v) for v in spec.split("x"))
        col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
        pd = [2] if nd == 5 else [2, 5]
        lo, hi = [-2.0] * nd, [2.0] * nd
        for d in pd:
            lo[d], hi[d] = 0.0, 2 * np.pi * (1 - 1.0 / n)
        g = L.createGrid(col(lo, np.float64), col(hi, np.float64), col([n] * nd, np.int64), pd, low_mem=True)
        system = L.Plane5D(g, 0.8, 1.3, 'min') if nd == 5 else L.DubinsPair6D(g, 1.5, 1.1, 0.9, 1.4)
        ham, par = system.native()
        src, axes, npar = (UC.PLANE_SRC, UC.PLANE_AXES, 3) if nd == 5 else (UC.PAIR_SRC, UC.PAIR_AXES, 4)
        trig = src.replace("aux[0]", "cos(x[2])").replace("aux[1]", "sin(x[2])").replace("aux[2]", "cos(x[5])").replace("aux[3]", "sin(x[5])")
        name = "plane5d" if nd == 5 else "pair6d"
        reg_t = L.register_hidim_hamiltonian(name + "_tables", nd, src, nparams=npar, aux_axes=axes)
        reg_s = L.register_hidim_hamiltonian(name + "_trig", nd, trig, nparams=npar)
        vs_host = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
        sys_t = reg_t(g, par[:npar], tables=UC.builtin_tables(vs_host))
        sys_s = reg_s(g, par[:npar])
        cells = n ** nd
        hg = hidim.hi_grid(g, "float64")
        vs = [torch.as_tensor(v, dtype=torch.float64, device="cuda") for v in vs_host]
        shp = lambda d: [n if k == d else 1 for k in range(nd)]      # noqa: E731
        x0, x1, xl = vs[0].reshape(shp(0)), vs[1].reshape(shp(1)), vs[nd - 1].reshape(shp(nd - 1))
        base = (x0 * x0 + x1 * x1 + 0.01).sqrt() - 1 + 0.05 * (3 * x0).sin() * (2 * xl).cos()
        gen = torch.Generator(device="cuda").manual_seed(7)
        y = (base.expand([n] * nd) + 0.02 * torch.randn([n] * nd, generator=gen, device="cuda", dtype=torch.float64)).contiguous()
        del base
        out = torch.empty_like(y)
        sb = hg.step_bound(ham, par)
        dt = 0.8 * sb
        sd = L.Bundle(dict(grid=g, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstWENO5,
                           hamFunc=lambda t, d_, p, s_=None: system.hamiltonian(t, d_, p, s_),
                           partialFunc=lambda t, d_, lo_, hi_, s_, i: system.dissipation(t, d_, lo_, hi_, s_, i)))
        names = {}

        def substep_of(label, hm, pr, tab):
            def run():
                hidim._substep(hg, sid, hm, pr, _ffi.STAGE_EULER, 0, y, None, out, dt, tab=tab)
                names.setdefault(label, _hffi.last_kernel())
            return run
        keep = []

        def run_split():
            keep[:] = [L.termLaxFriedrichs(0.0, y.reshape(-1, 1), sd)[0]]
        cands = [("built-in", substep_of("built-in", ham, par, None)),
                 ("registered", substep_of("registered", reg_t.ham_id, par[:npar], hg.tables_of(sys_t)[0])),
                 ("registered, trig", substep_of("registered, trig", reg_s.ham_id, par[:npar], hg.tables_of(sys_s)[0])),
                 ("split term", run_split)]
        results = {}
        for label, run in cands[:3]:            # warm-up (the run-time kernels are compiled or loaded here), and the three kernels agree
            run()
            results[label] = out.clone()
        run_split()
        torch.cuda.synchronize()
        scale = float(results["built-in"].abs().max())
        agree = ", ".join("%s %.2e" % (k, float((results[k] - results["built-in"]).abs().max()) / scale) for k in ("registered", "registered, trig"))
        del results
        times = dict((label, []) for label, _ in cands)
        for _ in range(args.reps):
            for label, run in cands:
                times[label].append(event_ms(torch, run))
        keep[:] = []
        lines.append("%d^%d = %.3e cells, float64, as-shipped WENO5; one array %.2f GB" % (n, nd, cells, cells * 8 / 1e9))
        ref = stats(times["built-in"])[0]
        for label, _ in cands:
            med, lo_, hi_ = stats(times[label])
            lines.append("  %-17s %9.3f (%.3f .. %.3f)   %.3e cell-substeps/s   %5.2fx the built-in kernel   %s" % (
                label, med, lo_, hi_, cells / (med * 1e-3), med / ref, names.get(label, "hjh_upwind, callbacks and dissipation as torch expressions")))
        lines.append("  max |registered - built-in| / max |built-in| of the substep's output: %s" % agree)
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
