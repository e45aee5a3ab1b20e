#!/usr/bin/env python3
"""Timing of the shape kernel (levelsetpy_amd/shapes.py, libhj_shapes.so) on one MI355X -> profiles/shapes_timing.txt.

    python tools/shapes_timing.py [--reps 15] [--host-reps 2] [--sizes 201,513,129] [--out FILE]

Sizes: n^3 Dubins-relative grids in fp64 (201, 513) and an n^4 grid in fp32 (129); a size the device or the host cannot hold is
reported as skipped.  Per size:

  (a) one sphere                (b) the scene of 8 leaves at depth 8 (tests/shapes_ref.nested_scene)
and once (c) K = 64 spheres of different radii on 51^3, one launch.

Each is measured three ways, the device sides taking turns in ONE process (kernel, fill, kernel, fill, ...):
  kernel    hjg_evaluate alone, device events around the call, median (min .. max) of --reps calls after 3 warm-up calls
  fill      torch's fill_ of the same output tensor, likewise: the store-bandwidth yardstick; the ratio kernel / fill beside it
  call      evaluate_shape as a user calls it -- compile, parameter upload, launch, flag read-back -- host clock, ending synchronised
  host      the route before this library: NumPy over dense coordinates on the host, then .to('cuda'); host clock, median
            of --host-reps runs (1 for the scene at the two large sizes).  For the sphere it is the package's shapeSphere on a dense
            grid (whose construction is timed apart); for the scene, the NumPy restatement of the same program.

The kernel's resource usage (make -C levelsetpy_amd/csrc resource-usage-shapes) heads the file when hipcc is present.
This is a measurement tool, not the benchmark (bench.py): nothing is asserted but that the kernel and the host route agree.
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def resource_usage():
    try:
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "resource-usage-shapes"], capture_output=True,
                           text=True, timeout=300)
    except Exception:  # noqa: BLE001
        return ["resource usage: not read (no compiler here)"]
    out, name = [], None
    for ln in (r.stdout + r.stderr).splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", ln)
        if m:
            if m.group(1) == "Function Name":
                name = "scene_kernel<double>" if "IdEE" in m.group(2) else "scene_kernel<float>"
                out.append("  %s:" % name)
            else:
                out[-1] += " %s %s;" % (m.group(1), m.group(2))
    return ["kernel resource usage (-Rpass-analysis=kernel-resource-usage, gfx950):"] + out if out else ["resource usage: not read"]


def host_bytes_available():
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable:"):
                return 1024 * int(ln.split()[1])
    except OSError:
        pass
    return None


def stats(ms):
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--sizes", default="201,513,129")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shapes_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    assert torch.cuda.is_available(), "tools/shapes_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _gffi, _marshal, shapes as S
    import shapes_ref as R

    prop = torch.cuda.get_device_properties(0)
    lines = ["Shapes on the device (libhj_shapes.so, scene_kernel) on one MI355X",
             "tools/shapes_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "kernel and fill: device events, %d calls each after 3 warm-up calls, taking turns: median (min .. max) in ms" % args.reps,
             "call and host: host clock around the whole route, ending synchronised, in ms"] + resource_usage() + [""]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def grid(n, dim, dense):
        if dim == 3:
            lo, hi, pd = [-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / n)], 2
        else:
            lo, hi, pd = [-1.0] * dim, [1.0] * dim, None
        return L.createGrid(np.array([lo]).T, np.array([hi]).T, n * np.ones((dim, 1), dtype=np.int64), pd, low_mem=not dense)

    def device_sides(g, node, dtype):
        """-> (kernel stats, fill stats, call ms, output tensor)."""
        comp = S.compile_program(node, g.dim)
        desc, N = _marshal.descriptor(g, dtype)
        coords = S._coord_tables(g, torch, torch.device("cuda", 0))
        prog = _gffi.program(comp.ops, [], [c.data_ptr() for c in coords])
        params = torch.from_numpy(comp.params).cuda()
        K, P = comp.members, comp.params.shape[1]
        out = torch.empty((K,) + N, dtype=torch.float64 if dtype == "float64" else torch.float32, device="cuda")
        flags = torch.zeros(K, dtype=torch.int32, device="cuda")
        did = _ffi.F64 if dtype == "float64" else _ffi.F32

        def kernel():
            _gffi.check(_gffi.lib().hjg_evaluate(desc, prog, params.data_ptr(), K, P, out.data_ptr(), did, flags.data_ptr(), stream))

        def fill():
            out.fill_(1.0)
        for _ in range(3):
            kernel(), fill()
        torch.cuda.synchronize()
        km, fm = [], []
        for _ in range(args.reps):
            for fn, acc in ((kernel, km), (fill, fm)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                acc.append(a.elapsed_time(b))
        kernel()
        torch.cuda.synchronize()
        calls = []
        for _ in range(4):
            t0 = time.perf_counter()
            res = S.evaluate_shape(g, node, dtype)
            torch.cuda.synchronize()
            calls.append(1e3 * (time.perf_counter() - t0))
            assert torch.equal(res.reshape(out.shape), out)
            del res
        return stats(km), stats(fm), float(np.median(calls[1:])), out

    def report(label, g, node, dtype, host_fn, host_reps, host_arrays=12):
        size = 8 if dtype == "float64" else 4
        km, fm, call, out = device_sides(g, node, dtype)
        nbytes = out.numel() * size
        say("  %s" % label)
        say("    kernel  %9.3f (%.3f .. %.3f)   %.2f TB/s stored" % (km + (nbytes / (km[0] * 1e-3) / 1e12,)))
        say("    fill    %9.3f (%.3f .. %.3f)   %.2f TB/s stored;  kernel / fill = %.2f" % (fm + (nbytes / (fm[0] * 1e-3) / 1e12, km[0] / fm[0])))
        say("    call    %9.3f" % call)
        host = []
        avail = host_bytes_available()
        if avail is not None and avail < host_arrays * out.numel() * 8:
            say("    host    skipped: about %d dense fp64 arrays of %.2f GB are live at once, the host has %.0f GB available" % (
                host_arrays, out.numel() * 8 / 1e9, avail / 1e9))
            return
        try:
            for _ in range(host_reps):
                t0 = time.perf_counter()
                arr = host_fn()
                dev = torch.from_numpy(np.ascontiguousarray(arr.astype(np.float32) if dtype == "float32" else arr)).to("cuda")
                torch.cuda.synchronize()
                host.append(1e3 * (time.perf_counter() - t0))
                same = bool(torch.equal(dev.reshape(out.shape), out))
                del arr, dev
                assert same, "the kernel and the host route disagree"
            h = float(np.median(host))
            say("    host    %9.1f   = %.0fx the call, %.0fx the kernel; same bits: True" % (h, h / call, h / km[0]))
        except MemoryError:
            say("    host    skipped: the host cannot hold the dense arrays")
        del out
        torch.cuda.empty_cache()

    for n in [int(v) for v in args.sizes.split(",") if v]:
        dim, dtype = (4, "float32") if n == 129 else (3, "float64")
        nodes = n ** dim
        say("%d^%d, %s: %.2f GB per array" % (n, dim, "fp64" if dtype == "float64" else "fp32", nodes * (8 if dtype == "float64" else 4) / 1e9))
        free = torch.cuda.mem_get_info()[0]
        if nodes * 8 * 2 > free:
            say("  skipped: the device has %.1f GB free" % (free / 1e9))
            continue
        g = grid(n, dim, dense=False)
        try:
            t0 = time.perf_counter()
            gd = grid(n, dim, dense=True)
            say("  createGrid with dense xs (the host route's coordinates): %.1f ms, %d x %.2f GB" % (1e3 * (time.perf_counter() - t0), dim, nodes * 8 / 1e9))
        except MemoryError:
            gd = None
            say("  createGrid with dense xs: the host cannot hold them")
        c = np.linspace(0.1, 0.3, dim)
        big = nodes > 50e6
        if gd is not None:
            report("(a) one sphere", g, S.sphere(c, 0.6), dtype, lambda: L.shapeSphere(gd, c.reshape(-1, 1), 0.6), args.host_reps)
        del gd
        node = R.nested_scene(S, dim)[0]
        comp = S.compile_program(node, dim)
        report("(b) scene of 8 leaves at depth 8 (%d instructions)" % len(comp.ops), g, node, dtype, lambda: R.run_program(g, comp)[0],
               1 if big else args.host_reps, host_arrays=dim + 8 + 6)
        say("")
    g = grid(51, 3, dense=True)
    radii = np.linspace(0.3, 0.9, 64)
    say("(c) K = 64 spheres on 51^3, fp64, one launch")
    report("64 members", g, S.sphere([0.1, 0.2, 0.3], radii), "float64",
           lambda: np.stack([L.shapeSphere(g, np.array([[0.1, 0.2, 0.3]]).T, r) for r in radii]), args.host_reps)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
