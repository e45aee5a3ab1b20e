#!/usr/bin/env python3
"""Randomised runs of the OTHER terms and of the local Lax-Friedrichs variants against the CPU oracle (test infrastructure; not collected).
    python tests/fuzz_terms.py [seconds] [seed]
Every case: a random 2-D / 3-D fp64 grid (random extents, random periodic axes), a random derivative scheme, one of
  termNormal (scalar or array speed), termReinit (sub-cell fix order 0 / 1), termConvection (scalar / array / exactly-zero components),
  termLaxFriedrichs with artificialDissipationLLF / LLLF on the Dubins / double-integrator systems,
through the TILED kernel (HJ_TERM_TILED_FROM=0) or the direct one (-1) -- ydot and stepBound against oracle.term_* at the suite's
tolerances (1e-11 of the scale; termReinit 1e-10: its quotient chain is rounded differently by the compiler) -- and one odeCFL3 step."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HJ_DIRECT_BELOW", "0")
import torch  # noqa: E402
import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd.context import device_grid  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402

DERIV = {"ENO2": L.upwindFirstENO2, "ENO3": L.upwindFirstENO3, "WENO5_ASSHIPPED": L.upwindFirstWENO5, "WENO5": L.upwindFirstWENO5Intended}


def mk(gmin, gmax, N, pd):
    g = L.createGrid(np.asarray(gmin, dtype=np.float64).reshape(-1, 1), np.asarray(gmax, dtype=np.float64).reshape(-1, 1),
                     np.asarray(N, dtype=np.int64).reshape(-1, 1), pd if pd else None)
    return g, O.Grid(gmin, gmax, [int(n) for n in N], list(pd) if pd else [])


def reinit_bound_without_noise_cells(og, phi, y, scheme, order):
    """oracle.term_reinit's step bound with the cells left out whose upwinded gradient is rounding noise (|g| <= 1e-13: there the
    quotient S g_d / max(|g|, eps) is 0 or |S| depending on the last bit of g).  Same selection rules as the oracle's."""
    dxs = og.dx.ravel()
    S = np.sign(phi) if order else phi / np.sqrt(phi ** 2 + np.max(dxs) ** 2)
    deriv = []
    for i in range(og.dim):
        Ld, Rd = O.SCHEMES[scheme](og, y, i, None)
        sL, sR = S * Ld, S * Rd
        pick = np.zeros(phi.shape, dtype=np.int8)
        pick[(sR <= 0) & (sL <= 0)] = 1
        pick[(sR >= 0) & (sL >= 0)] = 2
        conv = (sR < 0) & (sL > 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            sgn = S * (np.abs(Rd) - np.abs(Ld)) / (Rd - Ld)
        pick[conv & (sgn < 0)] = 1
        pick[conv & (sgn >= 0)] = 2
        both = ((sR <= 0) & (sL <= 0)) & ((sR >= 0) & (sL >= 0))
        gg = np.where(pick == 1, Rd, np.where(pick == 2, Ld, 0.0))
        deriv.append(np.where(both, Ld + Rd, gg))
    mag = np.sqrt(sum(d * d for d in deriv))
    keep = mag > 1e-13
    sbi = sum((np.max(np.abs(S * deriv[i] / np.maximum(mag, O.EPS))[keep]) if keep.any() else 0.0) / dxs[i] for i in range(og.dim))
    return 1.0 / sbi if sbi > 0 else np.inf


def tt(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def case(rng, k):
    os.environ["HJ_TERM_TILED_FROM"] = str(rng.choice(["0", "-1"]))
    if rng.random() < 0.5:
        os.environ["HJ_MIN_CHUNK"] = str(int(rng.integers(1, 6)))
    else:
        os.environ.pop("HJ_MIN_CHUNK", None)
    kind = str(rng.choice(["normal", "reinit", "convection", "llf", "lllf"]))
    scheme = str(rng.choice(list(DERIV)))
    if kind in ("llf", "lllf"):
        three = rng.random() < 0.6
        if three:
            N = [int(rng.integers(7, 40)) for _ in range(3)]
            pd = [d for d in range(3) if rng.random() < (0.8 if d == 2 else 0.2)]
            gmin, gmax = [-.75, -1.25, -np.pi], [3.25, 1.25, np.pi]
            mkp, mko = (lambda g: L.DubinsVehicleRel(g, 1, 1)), (lambda og: O.DubinsRel(og, 1, 1))
        else:
            N = [int(rng.integers(9, 120)) for _ in range(2)]
            pd = [d for d in range(2) if rng.random() < 0.2]
            gmin, gmax = [-1., -1.], [1., 1.]
            mkp, mko = (lambda g: L.DoubleIntegrator(g, 1)), (lambda og: O.DoubleIntegrator(og, 1))
    else:
        nd = int(rng.integers(2, 4))
        N = [int(rng.integers(7, {2: 110, 3: 36}[nd])) for _ in range(nd)]
        pd = [d for d in range(nd) if rng.random() < 0.3]
        gmin, gmax = [-1.0] * nd, [1.0] * nd
    nd = len(N)
    gmax = [gmax[d] - (gmax[d] - gmin[d]) / N[d] if d in pd else gmax[d] for d in range(nd)]
    g, og = mk(gmin, gmax, N, pd)
    phi = O.shape_sphere(og, None, .45 * min(b - a for a, b in zip(gmin, gmax)) / 2) * (1.0 + 0.4 * np.sin(3 * og.xs[0]) * np.cos(2 * og.xs[1])) \
        + 0.02 * rng.standard_normal(N)
    y = tt(phi.reshape(-1, 1))
    tol = 1e-11
    if kind == "normal":
        speed = (0.5 + 0.3 * np.cos(og.xs[0]) * np.ones(N)) if rng.random() < 0.6 else float(rng.uniform(-1.5, 1.5))
        sd = L.Bundle(dict(grid=g, derivFunc=DERIV[scheme], speed=tt(speed) if isinstance(speed, np.ndarray) else speed))
        fn = L.termNormal
        ofn = lambda t_, y_: O.term_normal(og, speed, scheme, t_, y_)  # noqa: E731
    elif kind == "reinit":
        order = int(rng.integers(0, 2))
        sd = L.Bundle(dict(grid=g, derivFunc=DERIV[scheme], initial=tt(phi), subcell_fix_order=order))
        fn = L.termReinit
        ofn = lambda t_, y_: O.term_reinit(og, phi, scheme, t_, y_, order)  # noqa: E731
        tol = 1e-10
    elif kind == "convection":
        vels = []
        for d in range(nd):
            r = rng.random()
            if r < 0.4:
                vels.append(float(rng.uniform(-1, 1)))
            else:
                v = np.sin(2 * og.xs[(d + 1) % nd]) * np.ones(N) + float(rng.uniform(-.5, .5))
                if r > 0.8:
                    v[np.abs(v) < 0.1] = 0.0
                vels.append(v)
        sd = L.Bundle(dict(grid=g, derivFunc=DERIV[scheme], velocity=[tt(v) if isinstance(v, np.ndarray) else v for v in vels]))
        fn = L.termConvection
        ofn = lambda t_, y_: O.term_convection(og, vels, scheme, t_, y_)  # noqa: E731
    else:
        sysp, syso = mkp(g), mko(og)
        sd = L.Bundle(dict(grid=g, hamFunc=sysp.hamiltonian, partialFunc=sysp.dissipation, CoStateCalc=DERIV[scheme],
                           dissFunc=L.artificialDissipationLLF if kind == "llf" else L.artificialDissipationLLLF))
        fn = L.termLaxFriedrichs
        ofn = lambda t_, y_: O.term_lax_friedrichs(og, syso, scheme, t_, y_, diss=kind)  # noqa: E731
    yd, sb, _ = fn(0., y, sd)
    dg = device_grid(g, "float64")
    used = dg.lib.hj_last_kernel(dg.ctx).decode()
    yo, sbo = ofn(0., phi.reshape(-1, 1))
    scale = max(1.0, float(np.abs(yo).max()))
    err = float(np.abs(yd.cpu().numpy() - yo).max()) / scale
    # termReinit's bound is max |S g_d / max(|g|, eps)| per dimension: at a cell where every one-sided derivative is rounding noise (|g| below
    # eps: the clamp decides) the quotient is 0 or |S| depending on the last bit of g -- such a cell can own the maximum (seed 5015: the
    # bounds differ by 1.2e-5 with ydot equal to 3e-16, seed 57706: by 1.3e-3; tests/diag/r05_reinit_diag.py)
    # -- so the product's bound has to lie between the oracle's with and without such cells
    if kind == "reinit":
        sb_hi = reinit_bound_without_noise_cells(og, phi, phi, scheme, order)
        ok = err <= tol and sbo * (1 - 1e-12) <= sb <= sb_hi * (1 + 1e-12)
    else:
        ok = err <= tol and (abs(sb - sbo) <= 1e-12 * abs(sbo) or (np.isinf(sb) and np.isinf(sbo)))
    # one RK3 step through the integrator (the generic loop for the other terms, the fused one for LLF / LLLF)
    err3 = 0.0
    if ok and np.isfinite(sbo) and abs(sb - sbo) <= 1e-12 * abs(sbo):
        t3, y3, _ = L.odeCFL3(fn, [0., 10.], y, L.odeCFLset(L.Bundle(dict(factorCFL=.5, singleStep='on'))), sd)
        to, y3o = O.ode_cfl_3(ofn, [0., 10.], phi.reshape(-1, 1), 0.5, single_step=True)
        d3 = np.abs(y3.cpu().numpy() - y3o)
        err3 = float(d3.max()) / max(1.0, float(np.abs(y3o).max()))
        if scheme.startswith("ENO") or kind == "reinit":      # selections / the sub-cell sign tests can flip on last-bit differences: masked
            ok = ok and float((d3 > 10 * tol * scale).mean()) <= 5e-3 and abs(t3 - to) <= 1e-12 * to
        else:
            ok = ok and err3 <= 10 * tol and abs(t3 - to) <= 1e-12 * to
    print("%4d %-10s N=%-12s pd=%-9s %-16s tiled_from=%-2s kernel %-22s err %.1e step %.1e sb %.15g/%.15g %s%s" % (
        k, kind, "x".join(map(str, N)), pd, scheme, os.environ["HJ_TERM_TILED_FROM"], used, err, err3, sb, sbo, "ok" if ok else "MISMATCH", (" order %d" % order) if kind == "reinit" else ""), flush=True)
    return ok, kind + ":" + used


if __name__ == "__main__":
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 4242
    t_end = time.time() + budget
    k, used_all = 0, {}
    while time.time() < t_end:
        ok, used = case(np.random.default_rng(seed0 + k), k)
        used_all[used] = used_all.get(used, 0) + 1
        if not ok:
            print("FAILED: replay with  python tests/fuzz_terms.py 1 %d" % (seed0 + k))
            sys.exit(1)
        k += 1
    print("term fuzz: %d cases ok in %.0f s; %s" % (k, budget, used_all))
