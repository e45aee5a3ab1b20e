#!/usr/bin/env python3
"""Timing of the 1-D .. 6-D shape kernel (levelsetpy_amd/shapes.py, libhj_hishapes.so) on one MI355X -> profiles/hishapes_timing.txt.

    python tools/hishapes_timing.py [--reps 15] [--out FILE]

Cases:
  (a) one sphere and (b) the scene of 8 leaves at depth 8 (tests/shapes_ref.nested_scene) on 41^5 and on 25^6, fp64 and fp32;
  (c) the capture set of two vehicles, sphere_between((0, 1), (3, 4), r), on 25^6 in fp64, beside the torch broadcast expression
      a user writes today (examples/two_cars_6d.py): reshaped coordinate vectors, subtract, square, add, sqrt, subtract, expand,
      contiguous;
  (d) the SAME program through hjk_evaluate (hi_scene_kernel) and hjg_evaluate (scene_kernel) on 129^4 in fp32 and 513^3 in
      fp64: new kernel against old, with the same bits (asserted).

Every candidate is timed by device events around the call, median (min .. max) of --reps calls after 3 warm-up calls, the
candidates of a case taking turns in ONE process (kernel, fill, kernel, fill, ...).  fill is torch's fill_ of the same output
tensor: the store-bandwidth yardstick.  A case the device cannot hold is reported as skipped.

The kernel's resource usage (make -C levelsetpy_amd/csrc resource-usage-hishapes) heads the file when hipcc is present.
This is a measurement tool, not the benchmark (bench.py): nothing is asserted but that the candidates of a case agree.
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def resource_usage():
    try:
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "resource-usage-hishapes"], capture_output=True,
                           text=True, timeout=300)
    except Exception:  # noqa: BLE001
        return ["resource usage: not read (no compiler here)"]
    out = []
    for ln in (r.stdout + r.stderr).splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", ln)
        if m:
            if m.group(1) == "Function Name":
                out.append("  %s:" % ("hi_scene_kernel<double>" if "IdEE" in m.group(2) else "hi_scene_kernel<float>"))
            else:
                out[-1] += " %s %s;" % (m.group(1), m.group(2))
    return ["kernel resource usage (-Rpass-analysis=kernel-resource-usage, gfx950):"] + out if out else ["resource usage: not read"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hishapes_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    assert torch.cuda.is_available(), "tools/hishapes_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import _ffi, _gffi, _kffi, _marshal, shapes as S
    import shapes_ref as R

    prop = torch.cuda.get_device_properties(0)
    lines = ["Shapes on 1-D .. 6-D grids on the device (libhj_hishapes.so, hi_scene_kernel) on one MI355X",
             "tools/hishapes_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "device events, %d calls each after 3 warm-up calls, the candidates of a case taking turns: median (min .. max) in ms" % args.reps]
    lines += resource_usage() + [""]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    TD = {"float64": torch.float64, "float32": torch.float32}

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def grid(shape):
        dim = len(shape)
        return L.createGrid(-np.ones((dim, 1)), np.ones((dim, 1)), np.array(shape, dtype=np.int64).reshape(-1, 1), None, low_mem=True)

    def turns(candidates):
        """{name: callable} -> {name: (median, min, max)}."""
        for _ in range(3):
            for fn in candidates.values():
                fn()
        torch.cuda.synchronize()
        ms = dict((k, []) for k in candidates)
        for _ in range(args.reps):
            for name, fn in candidates.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        return dict((k, (float(np.median(v)), float(min(v)), float(max(v)))) for k, v in ms.items())

    def launcher(g, node, dtype, hi, out):
        comp = S.compile_program_hi(node, g.dim) if hi else S.compile_program(node, g.dim)
        N = [int(v) for v in np.asarray(g.N).ravel()]
        coords = S._coord_tables(g, torch, torch.device("cuda", 0))
        params = torch.from_numpy(comp.params).cuda()
        flags = torch.zeros(comp.members, dtype=torch.int32, device="cuda")
        did = _ffi.F64 if dtype == "float64" else _ffi.F32
        ffi = _kffi if hi else _gffi
        desc = _kffi.grid_descriptor(N, dtype) if hi else _marshal.descriptor(g, dtype)[0]
        prog = ffi.program(comp.ops, [], [c.data_ptr() for c in coords])
        fn = ffi.lib().hjk_evaluate if hi else ffi.lib().hjg_evaluate
        keep = (comp, coords, params, flags, desc, prog)

        def run():
            ffi.check(fn(desc, prog, params.data_ptr(), comp.members, comp.params.shape[1], out.data_ptr(), did, flags.data_ptr(), stream))
            return keep
        return run, len(comp.ops)

    def line(name, st, nbytes):
        say("    %-12s %9.3f (%.3f .. %.3f)   %.2f TB/s stored" % (name, st[0], st[1], st[2], nbytes / (st[0] * 1e-3) / 1e12))

    def fits(nodes, dtype, arrays=1):
        need = arrays * nodes * (8 if dtype == "float64" else 4)
        free = torch.cuda.mem_get_info()[0]
        if need > 0.9 * free:
            say("    skipped: %.1f GB needed, the device has %.1f GB free" % (need / 1e9, free / 1e9))
            return False
        return True

    # ---- (a), (b): one sphere and the scene on 41^5 and 25^6
    for shape in ((41,) * 5, (25,) * 6):
        g, dim, nodes = grid(shape), len(shape), int(np.prod(shape))
        for dtype in ("float64", "float32"):
            size = 8 if dtype == "float64" else 4
            say("%d^%d, %s: %.2f GB per array" % (shape[0], dim, "fp64" if dtype == "float64" else "fp32", nodes * size / 1e9))
            if not fits(nodes, dtype):
                continue
            out = torch.empty(shape, dtype=TD[dtype], device="cuda")
            for label, node in (("(a) one sphere", S.sphere(np.linspace(0.1, 0.3, dim), 0.6)),
                                ("(b) scene of 8 leaves at depth 8", R.nested_scene(S, dim)[0])):
                run, n_ops = launcher(g, node, dtype, True, out)
                st = turns({"kernel": run, "fill": lambda: out.fill_(1.0)})
                say("  %s (%d instructions)" % (label, n_ops))
                line("kernel", st["kernel"], nodes * size)
                line("fill", st["fill"], nodes * size)
                say("    kernel / fill = %.2f" % (st["kernel"][0] / st["fill"][0]))
            del out
            torch.cuda.empty_cache()
        say("")

    # ---- (c): the capture set on 25^6 against the torch broadcast expression
    shape = (25,) * 6
    g, nodes = grid(shape), 25 ** 6
    say("(c) capture set sqrt((x0 - x3)^2 + (x1 - x4)^2) - r on 25^6, fp64: %.2f GB" % (nodes * 8 / 1e9))
    if fits(nodes, "float64", arrays=3):
        out = torch.empty(shape, dtype=torch.float64, device="cuda")
        run, _ = launcher(g, S.sphere_between((0, 1), (3, 4), 0.8), "float64", True, out)
        ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
        X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
        held = {}

        def broadcast():
            held["t"] = (((X[0] - X[3]) ** 2 + (X[1] - X[4]) ** 2).sqrt() - 0.8).expand(shape).contiguous()
        st = turns({"kernel": run, "fill": lambda: out.fill_(1.0), "torch": broadcast})
        line("kernel", st["kernel"], nodes * 8)
        line("fill", st["fill"], nodes * 8)
        line("torch", st["torch"], nodes * 8)
        say("    kernel / fill = %.2f;  torch / kernel = %.2f" % (st["kernel"][0] / st["fill"][0], st["torch"][0] / st["kernel"][0]))
        run()
        torch.cuda.synchronize()
        worst = float((out - held["t"]).abs().max())
        say("    max |kernel - torch| = %.3g (torch squares with pow and sums in its own order: not the contract's bits)" % worst)
        assert worst < 1e-14
        del out, held, X
        torch.cuda.empty_cache()
    say("")

    # ---- (d): the same program through both kernels on grids of at most four dimensions
    say("(d) the same program through hi_scene_kernel (hjk_evaluate) and scene_kernel (hjg_evaluate)")
    for shape, dtype in (((129,) * 4, "float32"), ((513,) * 3, "float64")):
        dim, nodes = len(shape), int(np.prod(shape))
        size = 8 if dtype == "float64" else 4
        say("  %d^%d, %s: %.2f GB per array" % (shape[0], dim, "fp64" if dtype == "float64" else "fp32", nodes * size / 1e9))
        if not fits(nodes, dtype, arrays=2):
            continue
        g = grid(shape)
        new, old = torch.empty(shape, dtype=TD[dtype], device="cuda"), torch.empty(shape, dtype=TD[dtype], device="cuda")
        for label, node in (("one sphere", S.sphere(np.linspace(0.1, 0.3, dim), 0.6)), ("scene of 8 leaves", R.nested_scene(S, dim)[0])):
            run_new, _ = launcher(g, node, dtype, True, new)
            run_old, _ = launcher(g, node, dtype, False, old)
            st = turns({"new": run_new, "old": run_old, "fill": lambda: new.fill_(1.0)})
            run_new()
            torch.cuda.synchronize()
            same = bool(torch.equal(new.view(torch.int64 if size == 8 else torch.int32), old.view(torch.int64 if size == 8 else torch.int32)))
            say("    %s" % label)
            line("  new", st["new"], nodes * size)
            line("  old", st["old"], nodes * size)
            line("  fill", st["fill"], nodes * size)
            say("      new / fill = %.2f;  old / fill = %.2f;  old / new = %.2f;  same bits: %s" % (
                st["new"][0] / st["fill"][0], st["old"][0] / st["fill"][0], st["old"][0] / st["new"][0], same))
            assert same, "the two kernels disagree"
        del new, old
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
