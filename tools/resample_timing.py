#!/usr/bin/env python3
"""Timing of the resampling kernels (levelsetpy_amd/resample.py, libhj_resample.so) on one MI355X -> profiles/resample_timing.txt.

    python tools/resample_timing.py [--reps 9] [--out FILE] [--only NAME]

Cases:
  migrate6   migrateGrid 15^6 -> 25^6, fp64          migrate5   migrateGrid 21^5 -> 41^5, fp64
  migrate3   migrateGrid 101^3 -> 201^3, fp64        migrate3f  the same in fp32
  rotate1    rotateData on 201^3, one angle          rotate64   rotateData on 201^3, 64 angles folded with min

Candidates of a case, taking turns in ONE process (new, old, clone, new, old, clone, ...):
  new    the one call of levelsetpy_amd.resample (tensor in, tensor out)
  old    the route it replaces: the destination's dense node coordinates built on the device (meshgrid, stack; for a rotation the
         matrix product and the shift), eval_u at them, and for the fold a chain of torch.minimum over the 64 results
  clone  torch's clone() of the result: the streaming floor of an array of that size
Every candidate is timed by device events around the call: median (min .. max) of --reps calls after 2 warm-up calls.  A case the
device cannot hold is reported as skipped.  new and old are compared where neither is NaN (asserted equal for the migrations: the
same interpolant at the same coordinates; the rotations' old route forms its coordinates by a matrix product, in another order).

This is a measurement tool, not the benchmark (bench.py): no threshold is set.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_timing.txt"))
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "tools/resample_timing.py needs an MI355X: there is nothing to measure without one"
    import levelsetpy_amd as L
    from levelsetpy_amd import resample

    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731

    def grid(n, D, scale=1.0):
        top = 2 * np.pi * (1 - 1.0 / n)
        lo = [-scale] * D
        hi = [scale] * D
        pd = [2] if D >= 3 else None
        if D >= 3:
            lo[2], hi[2] = 0.0, top
        return L.createGrid(col(lo), col(hi), col([n] * D, np.int64), pd, low_mem=True)

    def field(g, dtype):
        vs = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
        shape = [len(v) for v in vs]
        out = torch.zeros(shape, dtype=torch.float64, device="cuda")
        for d, v in enumerate(vs):
            out += torch.sin(1.3 * v + d).reshape([shape[d] if k == d else 1 for k in range(len(vs))])
        return out.to(dtype)

    def dense(g):
        vs = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
        return torch.stack([m.reshape(-1) for m in torch.meshgrid(*vs, indexing='ij')], dim=1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    lines = ["resampling kernels on %s, %d calls per candidate after 2 warm-up calls, device events, ms: median (min .. max)"
             % (torch.cuda.get_device_name(0), args.reps), ""]

    def case(name, what, new, old, check):
        if args.only and args.only != name:
            return
        try:
            for _ in range(2):
                r_new, r_old = new(), old()
            if check == "equal":
                same = torch.equal(torch.nan_to_num(r_new, nan=7.0), torch.nan_to_num(r_old.reshape(r_new.shape), nan=7.0))
                note = "new == old bit for bit: %s" % same
                assert same
            else:
                both = ~(torch.isnan(r_new) | torch.isnan(r_old.reshape(r_new.shape)))
                note = "max |new - old| where both are inside: %.3g" % float((r_new - r_old.reshape(r_new.shape))[both].abs().max())
            new()
            path = resample.last_path()
            del r_old
            times = {"new": [], "old": [], "clone": []}
            for _ in range(args.reps):
                times["new"].append(timed(new)[0])
                times["old"].append(timed(old)[0])
                times["clone"].append(timed(lambda: r_new.clone())[0])
            med = dict((k, float(np.median(v))) for k, v in times.items())
            lines.append("%s: %s  [%s]" % (name, what, path))
            for k in ("new", "old", "clone"):
                lines.append("  %-6s %10.3f (%.3f .. %.3f)" % (k, med[k], min(times[k]), max(times[k])))
            lines.append("  old / new %.2f, new / clone %.2f; %s" % (med["old"] / med["new"], med["new"] / med["clone"], note))
        except (RuntimeError, MemoryError) as e:                 # the device cannot hold the case
            lines.append("%s: %s  skipped: %s" % (name, what, str(e).splitlines()[0][:160]))
        lines.append("")
        torch.cuda.empty_cache()
        print("\n".join(lines[-7:]), flush=True)

    def migrate(name, nC, nF, D, dtype=torch.float64):
        gC, gF = grid(nC, D), grid(nF, D, 1.1)
        data = field(gC, dtype)
        shape = tuple([nF] * D)
        case(name, "migrateGrid %d^%d -> %d^%d, %s, fill 'nan'" % (nC, D, nF, D, str(dtype).split(".")[1]),
             lambda: L.migrateGrid(gC, data, gF, fill='nan'), lambda: L.eval_u(gC, data, dense(gF)).reshape(shape), "equal")

    migrate("migrate3", 101, 201, 3)
    migrate("migrate3f", 101, 201, 3, torch.float32)
    migrate("migrate5", 21, 41, 5)
    migrate("migrate6", 15, 25, 6)

    g = grid(201, 3, 2.0)
    data = field(g, torch.float64)
    shape = (201,) * 3

    def old_rotate(thetas):
        out = None
        for th in thetas:
            A, b = resample.rotateMap(g, float(th), (0, 1), 2)
            xs = dense(g) @ torch.as_tensor(A.T, device="cuda") + torch.as_tensor(b, device="cuda")
            v = L.eval_u(g, data, xs).reshape(shape)
            v = torch.where(torch.isnan(v), torch.full_like(v, float('inf')), v)
            out = v if out is None else torch.minimum(out, v)
        return torch.where(torch.isinf(out), torch.full_like(out, float('nan')), out)

    one, many = np.array(0.4), np.linspace(-3.0, 3.0, 64)
    case("rotate1", "rotateData 201^3, one angle, fp64, fill 'nan'", lambda: L.rotateData(g, data, one, (0, 1), 2, fill='nan'),
         lambda: old_rotate([one]), "close")
    case("rotate64", "rotateData 201^3, 64 angles folded with min, fp64, fill 'nan'",
         lambda: L.rotateData(g, data, many, (0, 1), 2, fill='nan', reduce='min'), lambda: old_rotate(many), "close")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
