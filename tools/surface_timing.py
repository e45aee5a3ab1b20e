#!/usr/bin/env python3
"""Timing of the level-set extraction (levelsetpy_amd/surface.py, libhj_surface.so) on one MI355X -> profiles/surface_timing.txt.

    python tools/surface_timing.py [--out FILE] [--commits TEXT] [--stats-csv FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/surface_timing.py --trace-only      # per-kernel times, a run of its own

Workloads, fp64, resident on the device: (A) the last slice of the 201^3 Dubins-relative reachable tube (HJIPDE_solve, t = 0.5);
(B) a sphere of radius 0.6 on 513^3 nodes over [-1, 1]^3.  For each, several rounds ALTERNATING, after a warm-up:

  count, emit   device events around hjs_count and around hjs_emit (the host reads 16 bytes in between)
  whole call    extract_level_set, host clock around a call that ends in a device synchronisation
  copy          the same array device -> host into pinned memory, and into pageable memory: the floor of any host mesher
  RK step       one odeCFL3 step of the solver at that size, for scale (the solver is the parent commit's, unchanged here)

Bytes are computed from shapes: the array read once, 16 bytes per scan tile, 6 bytes written per node of the tiles the level
crosses and 2 read back, the mesh written.  A measurement tool, not the benchmark (bench.py); nothing is asserted.
"""
import argparse
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
TILE = 1024


def dubins(L, n):
    gmin = np.array([[-.75, -1.25, -np.pi]]).T
    gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
    g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2, low_mem=True)
    s = L.DubinsVehicleRel(g, 1, 1)
    sd = L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF,
                       CoStateCalc=L.upwindFirstWENO5))
    return g, sd, L.shapeCylinder(g, 2, np.zeros((3, 1)), .5)


def tube_slice(L, torch, n):
    g, sd, d0 = dubins(L, n)
    out, _, _ = L.HJIPDE_solve(torch.as_tensor(d0, device="cuda"), np.linspace(0, 0.5, 3), sd, 'minVOverTime',
                               L.Bundle(dict(quiet=True, keepLast=True)))
    return g, out.contiguous()


def sphere(L, torch, n):
    g = L.createGrid(-np.ones((3, 1)), np.ones((3, 1)), n * np.ones((3, 1), dtype=np.int64), None, low_mem=True)
    x = torch.linspace(-1, 1, n, dtype=torch.float64, device="cuda")
    r2 = (x[:, None, None] - 0.03) ** 2 + (x[None, :, None] + 0.02) ** 2 + (x[None, None, :] - 0.01) ** 2
    return g, (torch.sqrt(r2) - 0.6).contiguous()


def rk_step_ms(L, torch, n, steps=5):
    g, sd, d0 = dubins(L, n)
    op = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='on')))
    y = torch.as_tensor(d0, device="cuda").reshape(-1, 1)
    t = 0.
    for _ in range(2):
        t, y, _ = L.odeCFL3(L.termLaxFriedrichs, [t, 10.], y, op, sd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t, y, _ = L.odeCFL3(L.termLaxFriedrichs, [t, 10.], y, op, sd)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


class Extraction(object):
    """hjs_count / hjs_emit on one array with buffers allocated once."""

    def __init__(self, torch, g, t):
        from levelsetpy_amd import _sffi, surface
        self.torch, self.sffi, self.t = torch, _sffi, t
        self.lib = _sffi.lib()
        self.desc, self.N = surface.descriptor(g, "float64")
        self.nodes = int(np.prod(self.N))
        need = C.c_size_t(0)
        _sffi.check(self.lib.hjs_workspace_size(C.byref(self.desc), 1, C.byref(need)))
        self.need = need.value
        self.work = torch.empty((self.need + 7) // 8, dtype=torch.int64, device="cuda")
        self.counts = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.count()
        self.nv, self.nf = [int(v) for v in self.counts.cpu().numpy().ravel()]
        self.hc = (C.c_int64 * 2)(self.nv, self.nf)
        self.verts = torch.empty((self.nv, 3), dtype=torch.float64, device="cuda")
        self.faces = torch.empty((self.nf, 3), dtype=torch.int32, device="cuda")
        ntiles = (self.nodes + TILE - 1) // TILE
        ex = self.work[:2 * (ntiles + 1)].cpu().numpy()
        self.ntiles = ntiles
        self.active = int(np.count_nonzero((np.diff(ex[:ntiles + 1]) != 0) | (np.diff(ex[ntiles + 1:]) != 0)))

    def p(self, t):
        return C.c_void_p(t.data_ptr())

    def count(self):
        self.sffi.check(self.lib.hjs_count(C.byref(self.desc), self.p(self.t), 1, self.nodes, 0.0, self.p(self.work), self.need,
                                           self.p(self.counts), self.stream))

    def emit(self):
        self.sffi.check(self.lib.hjs_emit(C.byref(self.desc), self.p(self.t), 1, self.nodes, 0.0, self.p(self.work), self.need, self.hc,
                                          self.p(self.verts), self.p(self.faces), self.stream))

    def bytes_count(self):
        return self.nodes * 8 + self.ntiles * 16 * 3 + self.active * TILE * 6

    def bytes_emit(self):
        return self.active * TILE * 2 + self.nv * 24 + self.nf * 12


def event_ms(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def host_ms(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_timing.txt"))
    ap.add_argument("--commits", default="not given")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="201,513")
    ap.add_argument("--trace-only", action="store_true", help="run each extraction 5 times and exit (under rocprofv3)")
    ap.add_argument("--stats-csv", default=None, help="kernel_stats.csv of the rocprofv3 run, quoted in the report")
    args = ap.parse_args()
    import torch
    import levelsetpy_amd as L
    n_tube, n_sphere = [int(v) for v in args.sizes.split(",")]
    lines = ["Level-set extraction on one MI355X (fp64): (A) last slice of the %d^3 Dubins tube, (B) sphere r = 0.6 on %d^3" % (n_tube, n_sphere),
             "tools/surface_timing.py; commits: %s" % args.commits,
             "%d rounds alternating after a warm-up; ms; median [min .. max]" % args.rounds, ""]
    for label, make, n in (("A", tube_slice, n_tube), ("B", sphere, n_sphere)):
        g, t = make(L, torch, n)
        E = Extraction(torch, g, t)
        if args.trace_only:
            for _ in range(5):
                E.count()
                E.emit()
            torch.cuda.synchronize()
            del E, t
            continue
        pinned = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        for fn in (E.count, E.emit, lambda: L.extract_level_set(g, t), lambda: pinned.copy_(t)):
            fn()
        torch.cuda.synchronize()
        rows = {k: [] for k in ("count", "emit", "whole call", "copy pinned", "copy pageable")}
        for _ in range(args.rounds):
            rows["count"].append(event_ms(torch, E.count, 20))
            rows["copy pinned"].append(host_ms(torch, lambda: pinned.copy_(t), 3))
            rows["emit"].append(event_ms(torch, E.emit, 20))
            rows["copy pageable"].append(host_ms(torch, lambda: t.cpu(), 1))
            rows["whole call"].append(host_ms(torch, lambda: L.extract_level_set(g, t), 5))
        med = {k: float(np.median(v)) for k, v in rows.items()}
        nbytes = E.nodes * 8
        lines.append("(%s) %d^3 = %d nodes, %.1f MB; nv = %d, nf = %d; %d of %d scan tiles crossed; workspace %.1f MB" % (
            label, n, E.nodes, nbytes / 1e6, E.nv, E.nf, E.active, E.ntiles, E.need / 1e6))
        for k in ("count", "emit", "whole call", "copy pinned", "copy pageable"):
            b = {"count": E.bytes_count(), "emit": E.bytes_emit(), "copy pinned": nbytes, "copy pageable": nbytes}.get(k)
            lines.append("    %-14s %9.3f [%9.3f .. %9.3f]%s" % (k, med[k], min(rows[k]), max(rows[k]),
                                                                "   %8.1f MB -> %7.1f GB/s" % (b / 1e6, b / med[k] / 1e6) if b else ""))
        both = med["count"] + med["emit"]
        lines.append("    count + emit   %9.3f ms on the device = %.1f MB of mesh; the copy alone takes %.1fx (pinned) / %.1fx (pageable) as long" % (
            both, (E.nv * 24 + E.nf * 12) / 1e6, med["copy pinned"] / both, med["copy pageable"] / both))
        if both > med["copy pinned"]:
            lines.append("    EXTRACTION COSTS MORE THAN THE COPY at this size")
        del E, t, pinned
        torch.cuda.empty_cache()
        lines.append("    one odeCFL3 step (three substeps) of the Dubins solve at %d^3, for scale: %9.3f ms" % (n, rk_step_ms(L, torch, n)))
        lines.append("")
        torch.cuda.empty_cache()
    if args.trace_only:
        return 0
    if args.stats_csv and os.path.exists(args.stats_csv):
        lines.append("per kernel, from a rocprofv3 --kernel-trace --stats run of its own (5 extractions of each workload + the first count; ns):")
        with open(args.stats_csv) as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if any(k in name for k in ("classify_kernel", "scan_blocks_kernel", "emit_kernel")):
                    lines.append("    %-60s calls %4s   total %12s   average %12s   min %10s   max %10s" % (
                        name[:60], r.get("Calls"), r.get("TotalDurationNs"), r.get("AverageNs"), r.get("MinNs"), r.get("MaxNs")))
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
