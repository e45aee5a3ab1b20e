#!/usr/bin/env python3
"""Timing of the 5-D / 6-D substep (levelsetpy_amd/hidim.py, libhj_hidim.so) on one MI355X -> profiles/hidim_timing.txt.

    python tools/hidim_timing.py [--shapes 41x5,25x6] [--reps 7] [--out FILE]

Workload: Plane5D on 41^5 nodes and DubinsPair6D on 25^6 nodes (periodic heading axes), fp64 and fp32, as-shipped WENO5 and ENO2,
a smooth field plus seeded noise made on the device.  Per configuration four candidates take turns in one process, device events
around each after a warm-up, median of the repetitions (min .. max beside it):
  substep     ONE launch of hidim_substep_kernel (HJ_STAGE_EULER): read the state through the stencils, write the new state
  rk3 step    hjh_integrate over one step: three launches
  clone       torch's clone() of the same array: one read and one write of it, the streaming floor of a substep
  split term  termLaxFriedrichs with the same system handed over as plain callbacks: hjh_upwind, the callbacks and the dissipation as
              torch expressions -- what a foreign Hamiltonian costs per substep
Algorithmic bytes as profiles/batch_timing.txt counts them: 64 per cell and RK3 step in fp64 (32 in fp32), 16 (8) per cell for a single
substep and for the clone.

This is a measurement tool, not the benchmark (bench.py): no figure is asserted here.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--shapes", default="41x5,25x6", help="comma-separated NxD: N nodes on each of D axes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hidim_timing.txt"))
    args = ap.parse_args()
    import torch
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _hffi, hidim
    if not torch.cuda.is_available():
        print("hidim_timing needs an MI355X: no device, nothing is measured", file=sys.stderr)
        return 2
    props = torch.cuda.get_device_properties(0)
    lines = ["5-D / 6-D substeps on one MI355X: hidim_substep_kernel (libhj_hidim.so), one thread per cell, stencils gathered from global memory",
             "tools/hidim_timing.py; device %s (%s), HIP %s, torch %s" % (props.name, getattr(props, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "the candidates take turns in one process; device events around each; median (min .. max) in ms; %d repetitions after a warm-up" % args.reps,
             "fraction of 8 TB/s on algorithmic bytes: 16 (fp32: 8) bytes per cell for a substep and the clone, 64 (32) per cell for an RK3 step", ""]
    for spec in args.shapes.split(","):
        n, nd = (int(v) for v in spec.split("x"))
        col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
        pd = [2] if nd == 5 else [2, 5]
        lo = [-2.0] * nd
        hi = [2.0] * nd
        for d in pd:
            lo[d], hi[d] = 0.0, 2 * np.pi * (1 - 1.0 / n)
        g = L.createGrid(col(lo, np.float64), col(hi, np.float64), col([n] * nd, np.int64), pd, low_mem=True)
        system = L.Plane5D(g, 0.8, 1.3, 'min') if nd == 5 else L.DubinsPair6D(g, 1.5, 1.1, 0.9, 1.4)
        ham, par = system.native()
        cells = n ** nd
        for dtype in ("float64", "float32"):
            td = torch.float64 if dtype == "float64" else torch.float32
            esz = 8 if dtype == "float64" else 4
            hg = hidim.hi_grid(g, dtype)
            vs = [torch.as_tensor(np.asarray(v).ravel(), dtype=torch.float64, device="cuda") for v in g.vs]
            shp = lambda d: [n if k == d else 1 for k in range(nd)]      # noqa: E731
            x0, x1, xl = vs[0].reshape(shp(0)), vs[1].reshape(shp(1)), vs[nd - 1].reshape(shp(nd - 1))
            base = (x0 * x0 + x1 * x1 + 0.01).sqrt() - 1 + 0.05 * (3 * x0).sin() * (2 * xl).cos()
            gen = torch.Generator(device="cuda").manual_seed(7)
            y = (base.expand([n] * nd) + 0.02 * torch.randn([n] * nd, generator=gen, device="cuda", dtype=torch.float64)).to(td).contiguous()
            del base
            out, a, b, w = (torch.empty_like(y) for _ in range(4))
            sb = hg.step_bound(ham, par)
            dt = 0.8 * sb
            for scheme, fn, sid in (("as-shipped WENO5", L.upwindFirstWENO5, _ffi.WENO5_ASSHIPPED), ("ENO2", L.upwindFirstENO2, _ffi.ENO2)):
                sd = L.Bundle(dict(grid=g, dissFunc=L.artificialDissipationGLF, derivFunc=fn,
                                   hamFunc=lambda t, d_, p, s_=None: system.hamiltonian(t, d_, p, s_),
                                   partialFunc=lambda t, d_, lo_, hi_, s_, i: system.dissipation(t, d_, lo_, hi_, s_, i)))
                tout, ns, where = C.c_double(), C.c_int64(), C.c_int32()

                def run_substep():
                    hidim._substep(hg, sid, ham, par, _ffi.STAGE_EULER, 0, y, None, out, dt)

                def run_step():
                    _hffi.check(hg.lib.hjh_integrate(C.byref(hg.desc), C.byref(hg.tab), sid, ham, 3, 0, 0, _hffi.params(par), sb, hg.ptr(y), hg.ptr(a),
                                                     hg.ptr(b), hg.ptr(w), 0, None, 0, None, 0.0, dt, 0.8, 1e300, -1.0, C.byref(tout), C.byref(ns),
                                                     C.byref(where), hg.stream()))

                keep = []

                def run_clone():
                    keep[:] = [y.clone()]

                def run_split():
                    keep[:] = [L.termLaxFriedrichs(0.0, y.reshape(-1, 1), sd)[0]]

                cands = [("substep", run_substep, 1, 2 * esz), ("rk3 step", run_step, 3, 8 * esz), ("clone", run_clone, 0, 2 * esz),
                         ("split term", run_split, 1, 2 * esz)]
                for _, run, _, _ in cands:          # warm-up: code objects, the allocator's blocks
                    run()
                torch.cuda.synchronize()
                kernel = _hffi.kernel_name(dtype, ham, sid)
                assert ns.value == 1
                times = dict((name, []) for name, _, _, _ in cands)
                for _ in range(args.reps):
                    for name, run, _, _ in cands:
                        times[name].append(event_ms(torch, run))
                keep[:] = []
                lines.append("%d^%d = %.3e cells, %s, %s: %s; one array %.2f GB (axis 0's stride %.1f MB)" % (
                    n, nd, cells, dtype, scheme, kernel, cells * esz / 1e9, cells // n * esz / 1e6))
                for name, _, substeps, nbytes in cands:
                    med, lo_, hi_ = stats(times[name])
                    sec = med * 1e-3
                    rate = ("%.3e cell-substeps/s" % (substeps * cells / sec)) if substeps else "%-26s" % ""
                    lines.append("  %-10s %10.3f (%.3f .. %.3f)   %s   %.4f of 8 TB/s on algorithmic bytes" % (name, med, lo_, hi_, rate, nbytes * cells / sec / 8e12))
                ms, mc, mp, mr = (stats(times[k])[0] for k in ("substep", "clone", "split term", "rk3 step"))
                lines.append("  substep / clone = %.2f;  split term / substep = %.2f;  rk3 step / substep = %.2f" % (ms / mc, mp / ms, mr / ms))
                lines.append("")
            del y, out, a, b, w
            torch.cuda.empty_cache()
    text = "\n".join(lines[:-1]) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
