#!/usr/bin/env python3
"""Timing of the decomposition kernels (levelsetpy_amd/decomp.py, libhj_decomp.so) on one MI355X -> profiles/decomp_timing.txt.

    python tools/decomp_timing.py [--reps 15] [--out FILE]

Back-projection (the nodes kernel), the candidates taking turns in ONE process (kernel, fill, broadcast, kernel, ...):
  (a) two 2-D subsystems on axes (0, 2) and (1, 3) onto 129^4 in fp32 (1.1 GB)
  (b) two 2-D subsystems on axes (0, 2) and (1, 2) -- a shared last axis -- onto 201^3 in fp64 (65 MB)
each against
  fill       torch's fill_ of the same output tensor: the store floor; the ratio kernel / fill beside it
  broadcast  what a user would otherwise write, torch.maximum(a[:, None, :, None], b[None, :, None, :]) (and its 3-D form)
Queries at states:
  (c) .eval_u of three 2-D subsystems (a 6-D space) at M = 10^5 states against three eval_u calls and two torch.maximum.
Every figure: device events around the call, median (min .. max) of --reps calls after 3 warm-up calls, in ms.

The kernels' resource usage (make -C levelsetpy_amd/csrc resource-usage-decomp) heads the file when hipcc is present.
This is a measurement tool, not the benchmark (bench.py): nothing is asserted but that the candidates agree.
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
NAMES = {"24backproject_nodes": "backproject_nodes_kernel", "25backproject_coords": "backproject_coords_kernel", "20decomp_points": "decomp_points_kernel"}


def resource_usage():
    try:
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "resource-usage-decomp"], capture_output=True,
                           text=True, timeout=300)
    except Exception:  # noqa: BLE001
        return ["resource usage: not read (no compiler here)"]
    out = []
    for ln in (r.stdout + r.stderr).splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", ln)
        if m:
            if m.group(1) == "Function Name":
                stem = next((v for k, v in NAMES.items() if k in m.group(2)), m.group(2))
                out.append("  %s<%s>:" % (stem, "double" if "IdEE" in m.group(2) else "float"))
            else:
                out[-1] += " %s %s;" % (m.group(1), m.group(2))
    return ["kernel resource usage (-Rpass-analysis=kernel-resource-usage, gfx950):"] + out if out else ["resource usage: not read"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decomp_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/decomp_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import _dffi, _ffi, decomp

    prop = torch.cuda.get_device_properties(0)
    lines = ["Decomposed value functions on the device (libhj_decomp.so) on one MI355X",
             "tools/decomp_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "device events, %d calls each after 3 warm-up calls, the candidates taking turns: median (min .. max) in ms" % args.reps]
    lines += resource_usage() + [""]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def turns(candidates):
        """name -> callable; every candidate once per round, 3 warm-up rounds -> name -> (median, min, max)."""
        ms = dict((k, []) for k in candidates)
        for rep in range(args.reps + 3):
            for name, fn in candidates.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 3:
                    ms[name].append(a.elapsed_time(b))
        return dict((k, (float(np.median(v)), float(min(v)), float(max(v)))) for k, v in ms.items())

    def fmt(s):
        return "%9.3f (%8.3f .. %8.3f)" % s

    def grid(shape):
        nd = len(shape)
        return L.createGrid(-np.ones((nd, 1)), np.ones((nd, 1)), np.array(shape, dtype=np.int64).reshape(-1, 1), None, low_mem=True)

    def back_projection(tag, shape, dims, dtype, broadcast):
        td = torch.float32 if dtype == "float32" else torch.float64
        g = grid(shape)
        gs = [grid([shape[a] for a in axes]) for axes in dims]
        gen = torch.Generator(device="cuda").manual_seed(1)
        datas = [torch.rand([shape[a] for a in axes], generator=gen, device="cuda", dtype=td) for axes in dims]
        dec = decomp.Decomposition(gs, datas, dims, 'intersection')
        out = torch.empty(shape, dtype=td, device="cuda")
        did = _ffi.F64 if dtype == "float64" else _ffi.F32
        ext, lib = _dffi.extents(shape), _dffi.lib()

        def kernel():
            _dffi.check(lib.hjd_backproject_nodes(C.byref(dec.desc), ext, 1, out.data_ptr(), did, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

        keep = {}

        def bcast():
            keep["b"] = broadcast(*datas)

        t = turns({"kernel": kernel, "fill": lambda: out.fill_(1.0), "broadcast": bcast})
        kernel()
        agree = bool(torch.equal(out, keep["b"]))
        gb = out.numel() * out.element_size() / 1e9
        say("(%s) %s onto %s %s, %.3f GB written; the candidates agree: %s" % (tag, dims, "x".join(map(str, shape)), dtype, gb, agree))
        say("    kernel     %s   %7.0f GB/s   %s" % (fmt(t["kernel"]), gb / t["kernel"][0] * 1e3, _dffi.last_kernel()))
        say("    fill       %s   %7.0f GB/s   kernel / fill = %.2f" % (fmt(t["fill"]), gb / t["fill"][0] * 1e3, t["kernel"][0] / t["fill"][0]))
        say("    broadcast  %s                 broadcast / kernel = %.2f" % (fmt(t["broadcast"]), t["broadcast"][0] / t["kernel"][0]))
        assert agree

    back_projection("a", (129,) * 4, [[0, 2], [1, 3]], "float32", lambda a, b: torch.maximum(a[:, None, :, None], b[None, :, None, :]))
    back_projection("b", (201,) * 3, [[0, 2], [1, 2]], "float64", lambda a, b: torch.maximum(a[:, None, :], b[None, :, :]))

    # (c) states
    M, n = 100000, (101, 101)
    g2 = grid(n)
    gen = torch.Generator(device="cuda").manual_seed(2)
    datas = [torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) for _ in range(3)]
    dims = [[0, 1], [2, 3], [4, 5]]
    dec = decomp.Decomposition([g2] * 3, datas, dims)
    xs = torch.rand((M, 6), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1
    cols = [xs[:, a].contiguous() for a in dims]
    keep = {}

    def fused():
        keep["f"] = dec.eval_u(xs)

    def separate():
        v = [L.eval_u(g2, d, c) for d, c in zip(datas, cols)]
        keep["s"] = torch.maximum(torch.maximum(v[0], v[1]), v[2])

    t = turns({"eval_u": fused, "separate": separate})
    agree = bool(torch.equal(keep["f"], keep["s"]))
    say("(c) .eval_u of three 2-D subsystems (101 x 101, fp64) at M = %d states in 6-D; the candidates agree: %s" % (M, agree))
    say("    Decomposition.eval_u          %s   %s" % (fmt(t["eval_u"]), _dffi.last_kernel()))
    say("    3 x eval_u + 2 x maximum      %s   separate / fused = %.2f" % (fmt(t["separate"]), t["separate"][0] / t["eval_u"][0]))
    assert agree
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
