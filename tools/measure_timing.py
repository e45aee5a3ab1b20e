#!/usr/bin/env python3
"""Timing of the set-measure kernels (levelsetpy_amd/measure.py, libhj_measure.so) on one MI355X -> profiles/measure_timing.txt.

    python tools/measure_timing.py [--reps 5] [--out FILE] [--only NAME[,NAME...]]

Cases, named <data>-<size>: the sizes 201^3 and 513^3 in fp64, 129^4 in fp32, 41^5 and 25^6 in fp64, each with
  ball    a ball of radius 0.6: the cut cells are a surface's worth
  noisy   uniform noise in [-1, 1]: every cell is cut, the worst case (D! simplices of arithmetic per cell)
and compare-<size> for 201^3 and 41^5: setCompare of two overlapping balls.

Candidates of a case, taking turns in ONE process:
  kernels  hjv_measure on preallocated records and workspace: the launches alone (memset, measure_kernel, measure_fold_kernel)
  call     levelsetpy_amd.setVolume / setCompare on a device tensor: the launches, the allocations, the copy of the records and
           the synchronisation
  count    (data <= level).sum(): the node count the examples used as a stand-in
  clone    torch's clone() of the data: the streaming floor of an array of that size
  torch    compare only: the route setCompare replaces -- torch.minimum, torch.maximum and four (x <= level).sum() -- with the peak
           memory it allocates beside the inputs
Every candidate is timed by device events around the call: median (min .. max) of --reps calls after one warm-up call.  A case the
device cannot hold is reported as skipped.

This is a measurement tool, not the benchmark (bench.py): no threshold is set.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIZES = [(201, 3, "float64"), (513, 3, "float64"), (129, 4, "float32"), (41, 5, "float64"), (25, 6, "float64")]
COMPARE = [(201, 3, "float64"), (41, 5, "float64")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_timing.txt"))
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else None
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/measure_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import measure, _vffi, _ffi

    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    TD = {"float64": torch.float64, "float32": torch.float32}

    def grid(n, D):
        return L.createGrid(col([-1.0] * D), col([1.0] * D), col([n] * D, np.int64), None, low_mem=True)

    def ball(g, dtype, centre=0.0, r=0.6):
        vs = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
        shape = [len(v) for v in vs]
        s = torch.zeros(shape, dtype=torch.float64, device="cuda")
        for d, v in enumerate(vs):
            s += ((v - centre) ** 2).reshape([shape[d] if k == d else 1 for k in range(len(vs))])
        return (s.sqrt_() - r).to(dtype)

    def noisy(g, dtype):
        gen = torch.Generator(device="cuda").manual_seed(7)
        shape = [int(v) for v in np.asarray(g.N).ravel()]
        return (torch.rand(shape, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1).to(dtype)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    def raw(g, a, b=None):
        """hjv_measure on buffers made once."""
        N = tuple(int(v) for v in np.asarray(g.N).ravel())
        name = lambda t: "float32" if t.dtype == torch.float32 else "float64"      # noqa: E731
        desc = _vffi.extents_descriptor(N, (), name(a))
        sets = 4 if b is not None else 1
        rec = torch.empty((sets, _vffi.RECORD_WORDS), dtype=torch.int64, device="cuda")
        work = torch.empty(int(_vffi.lib().hjv_workspace_size(C.byref(desc), 1, int(b is not None))) // 8, dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pb = C.c_void_p(b.data_ptr()) if b is not None else None
        fb = _ffi.F32 if b is not None and b.dtype == torch.float32 else _ffi.F64

        def run():
            _vffi.check(_vffi.lib().hjv_measure(C.byref(desc), C.c_void_p(a.data_ptr()), 1, a.numel(), pb, fb, 1, a.numel(), 0.0,
                                                C.c_void_p(rec.data_ptr()), C.c_void_p(work.data_ptr()), stream))
            return rec
        return run

    lines = ["set-measure kernels on %s, %d calls per candidate after one warm-up call, device events, ms: median (min .. max)"
             % (torch.cuda.get_device_name(0), args.reps), ""]

    def report(name, what, cands, note):
        for fn in cands.values():
            fn()
        torch.cuda.synchronize()
        times = dict((k, []) for k in cands)
        for _ in range(args.reps):
            for k, fn in cands.items():
                times[k].append(timed(fn)[0])
        med = dict((k, float(np.median(v))) for k, v in times.items())
        lines.append("%s: %s  [%s]" % (name, what, measure.last_path()))
        for k in cands:
            lines.append("  %-8s %10.3f (%.3f .. %.3f)" % (k, med[k], min(times[k]), max(times[k])))
        lines.append("  " + note(med))

    def guarded(name, body):
        if only and name not in only:
            return
        at = len(lines)
        try:
            body()
        except (RuntimeError, MemoryError) as e:                 # the device cannot hold the case
            lines.append("%s: skipped: %s" % (name, str(e).splitlines()[0][:160]))
        lines.append("")
        torch.cuda.empty_cache()
        print("\n".join(lines[at:]), flush=True)

    for n, D, dt in SIZES:
        for kind, make in (("ball", ball), ("noisy", noisy)):
            name = "%s-%d^%d" % (kind, n, D)

            def body():
                g = grid(n, D)
                data = make(g, TD[dt])
                vol, info = L.setVolume(g, data, return_info=True)
                what = "%d^%d %s, %s: %d of %d cells cut, volume %.6g (%d nodes inside)" % (n, D, dt, kind, info["cut"], info["cells"], vol,
                                                                                             info["inside"])
                run = raw(g, data)
                report(name, what, {"kernels": run, "call": lambda: L.setVolume(g, data), "count": lambda: (data <= 0).sum(),
                                    "clone": lambda: data.clone()},
                       lambda m: "kernels / clone %.2f, kernels / count %.2f, call - kernels %.3f ms; %.1f GB/s of data through the kernels"
                       % (m["kernels"] / m["clone"], m["kernels"] / m["count"], m["call"] - m["kernels"],
                          data.numel() * data.element_size() / m["kernels"] / 1e6))
            guarded(name, body)

    for n, D, dt in COMPARE:
        name = "compare-%d^%d" % (n, D)

        def body():
            g = grid(n, D)
            a, b = ball(g, TD[dt]), ball(g, TD[dt], 0.15, 0.55)
            out = L.setCompare(g, a, b)

            def route():
                u, i = torch.minimum(a, b), torch.maximum(a, b)
                return (a <= 0).sum(), (b <= 0).sum(), (u <= 0).sum(), (i <= 0).sum()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            route()
            torch.cuda.synchronize()
            extra_old = torch.cuda.max_memory_allocated() - base
            torch.cuda.reset_peak_memory_stats()
            L.setCompare(g, a, b)
            torch.cuda.synchronize()
            extra_new = torch.cuda.max_memory_allocated() - base
            what = "%d^%d %s, two balls: union %.6g intersection %.6g symdiff %.6g iou %.4f" % (n, D, dt, out.union, out.intersection,
                                                                                              out.symdiff, out.iou)
            report(name, what, {"kernels": raw(g, a, b), "call": lambda: L.setCompare(g, a, b), "torch": route, "clone": lambda: a.clone()},
                   lambda m: "torch / kernels %.2f, torch / call %.2f; peak extra memory: torch route %.1f MB, setCompare %.3f MB"
                   % (m["torch"] / m["kernels"], m["torch"] / m["call"], extra_old / 1e6, extra_new / 1e6))
        guarded(name, body)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
