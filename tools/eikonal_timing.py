#!/usr/bin/env python3
"""Timing of signedDistance (levelsetpy_amd/eikonal.py, libhj_eikonal.so) on one MI355X -> profiles/eikonal_timing.txt.

    python tools/eikonal_timing.py [--reps 5] [--out FILE] [--small]

  (a) 201^3 and 513^3 fp64: one sphere, the union of 8 spheres, and the sphere with band = 10 dx -- ms, passes, and the
      share of tile launches that did work;
  (b) 129^4 fp32: one sphere;
  (c) what the package offered for the same job before: termReinit under odeCFL2 with ENO2 derivatives, run for the
      pseudo-time in which distance reaches the band (10 dx), and for the full grid (201^3 measured; 513^3 full grid
      scaled from its band run by the pseudo-times, and marked so); these runs take turns with the others;
  (d) fill_ of the same tensor: the floor of ONE pass that visits every node.
Every figure: device events around the call, median (min .. max) of --reps calls after 1 warm-up call, the candidates of
a group taking turns in one process.  The first lines hold the largest difference from the NumPy restatement on small
grids (0 is expected) and the kernels' resource usage when hipcc is present.
This is a measurement tool, not the benchmark (bench.py): nothing is asserted.  --small runs 65^3 / 33^4 only.
"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def resource_usage():
    try:
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "resource-usage-eikonal"], capture_output=True,
                           text=True, timeout=300)
    except Exception:  # noqa: BLE001
        return ["resource usage: not read (no compiler here)"]
    out = []
    for ln in (r.stdout + r.stderr).splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", ln)
        if m:
            if m.group(1) == "Function Name":
                name = m.group(2)
                stem = "eikonal_tile_kernel<%s>" % name.split("ILi")[1][0] if "tile" in name else \
                    ("eikonal_init_kernel" if "init" in name else "eikonal_finish_kernel") + ("<double>" if "IdEE" in name else "<float>")
                out.append("  %s:" % stem)
            else:
                out[-1] += " %s %s;" % (m.group(1), m.group(2))
    return ["kernel resource usage (-Rpass-analysis=kernel-resource-usage, gfx950):"] + out if out else ["resource usage: not read"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eikonal_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    assert torch.cuda.is_available(), "tools/eikonal_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    import eikonal_ref as R

    prop = torch.cuda.get_device_properties(0)
    lines = ["signedDistance on the device (libhj_eikonal.so) on one MI355X",
             "tools/eikonal_timing.py; device %s (%s), HIP %s, torch %s" % (prop.name, getattr(prop, "gcnArchName", "?"), torch.version.hip, torch.__version__),
             "device events, %d calls each after 1 warm-up call, the candidates taking turns: median (min .. max) in ms" % args.reps]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def grid(shape):
        nd = len(shape)
        return L.createGrid(-np.ones((nd, 1)), np.ones((nd, 1)), np.array(shape, dtype=np.int64).reshape(-1, 1), None, low_mem=True)

    def axes(shape):
        return [torch.linspace(-1, 1, n, device="cuda", dtype=torch.float64).reshape([-1 if e == d else 1 for e in range(len(shape))])
                for d, n in enumerate(shape)]

    def spheres(shape, centres, radius, td=torch.float64):
        X = axes(shape)
        out = None
        for c in centres:
            r = torch.sqrt(sum((x - ci) ** 2 for x, ci in zip(X, c))) - radius
            out = r if out is None else torch.minimum(out, r)
        return (out * (1.0 + 0.5 * X[0])).to(td).contiguous()

    def turns(candidates):
        ms = dict((k, []) for k in candidates)
        for rep in range(args.reps + 1):
            for name, fn in candidates.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 1:
                    ms[name].append(a.elapsed_time(b))
        return dict((k, (float(np.median(v)), float(min(v)), float(max(v)))) for k, v in ms.items())

    def fmt(s):
        return "%10.3f (%9.3f .. %9.3f)" % s

    # ---- agreement with the restatement on small grids
    worst = 0.0
    for shape in ((37,), (40, 70), (33, 27, 29), (7, 6, 5, 6)):
        g = grid(shape)
        data = spheres(shape, [[0.1] * len(shape)], 0.5).cpu().numpy()
        want = R.signed_distance(data, np.asarray(g.dx).ravel())
        worst = max(worst, float(np.abs(L.signedDistance(g, data) - want).max()))
    say("largest |device - restatement| on (37,), (40, 70), (33, 27, 29), (7, 6, 5, 6): %.3g" % worst)
    lines.extend(resource_usage() + [""])

    rng = np.random.default_rng(1)

    def reinit(g, phi, pseudo_time):
        """termReinit under odeCFL2 with ENO2 for `pseudo_time`, as the package offered before: a candidate for turns()."""
        sd = L.Bundle(dict(grid=g, derivFunc=L.upwindFirstENO2, initial=phi, subcell_fix_order=1))
        opts = L.odeCFLset(L.Bundle(dict(factorCFL=0.5)))
        y = phi.reshape(-1, 1)
        return lambda: L.odeCFL2(L.termReinit, [0.0, pseudo_time], y, opts, sd)

    def solve_group(tag, shape, td, reinit_full=False):
        g = grid(shape)
        nd = len(shape)
        dx = float(np.asarray(g.dx).ravel()[0])
        one = spheres(shape, [[0.1] * nd], 0.5, td)
        cases = {"one sphere": (one, np.inf)}
        if nd == 3:
            eight = spheres(shape, rng.uniform(-0.6, 0.6, (8, nd)).tolist(), 0.2, td)
            cases["union of 8 spheres"] = (eight, np.inf)
            cases["one sphere, band 10 dx"] = (one, 10 * dx)
        info = {}

        def run(name):
            d, band = cases[name]

            def fn():
                info[name] = L.signedDistance(g, d, band=band, return_info=True)[1]
            return fn

        cand = dict((name, run(name)) for name in cases)
        scratch = torch.empty_like(one)
        cand["fill_"] = lambda: scratch.fill_(1.0)
        far = float(np.sqrt(3) * 1.1 + 0.5)                           # the farthest corner from the sphere's surface
        if nd == 3:
            cand["reinit band"] = reinit(g, one, 10 * dx)
            if reinit_full:
                cand["reinit full"] = reinit(g, one, far)
        t = turns(cand)
        gb = one.numel() * one.element_size() / 1e9
        say("(%s) %s %s, %.3f GB per array" % (tag, "x".join(map(str, shape)), str(td).split(".")[1], gb))
        for name in cases:
            i = info[name]
            say("    %-24s %s   passes %4d   tile launches that did work %5.1f %%   = %.1f x fill_" % (
                name, fmt(t[name]), i.passes, 100 * i.active_tile_launch_fraction, t[name][0] / t["fill_"][0]))
        say("    %-24s %s   %7.0f GB/s" % ("fill_ (one pass's floor)", fmt(t["fill_"]), gb / t["fill_"][0] * 1e3))
        if nd == 3:
            say("    termReinit, odeCFL2, ENO2, pseudo-time 10 dx (the band)   %s   = %.1f x signedDistance with the band" % (
                fmt(t["reinit band"]), t["reinit band"][0] / t["one sphere, band 10 dx"][0]))
            if reinit_full:
                say("    termReinit, pseudo-time %.2f (the full grid)              %s   = %.1f x signedDistance" % (
                    far, fmt(t["reinit full"]), t["reinit full"][0] / t["one sphere"][0]))
            else:
                full_ms = t["reinit band"][0] * far / (10 * dx)
                say("    termReinit, pseudo-time %.2f (the full grid), SCALED from the band's median by the pseudo-times, NOT RUN: %10.0f ms   = %.0f x signedDistance" % (
                    far, full_ms, full_ms / t["one sphere"][0]))
        del g, one, scratch
        torch.cuda.empty_cache()

    sizes = [("a1", (65,) * 3)] if args.small else [("a1", (201,) * 3), ("a2", (513,) * 3)]
    for tag, shape in sizes:
        solve_group(tag, shape, torch.float64, reinit_full=shape[0] <= 201)
    solve_group("b", (33,) * 4 if args.small else (129,) * 4, torch.float32)

    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
