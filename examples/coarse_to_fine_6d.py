#!/usr/bin/env python3
"""Coarse to fine in six dimensions: solve the two-car pursuit game on a coarse grid, move the result onto a finer grid on the
device, and continue there.

    python examples/coarse_to_fine_6d.py [n_coarse] [n_fine] [horizon]

A 6-D solve is affordable on a coarse grid and expensive on a fine one.  The usual remedy (helperOC's migrateGrid) is to spend most
of the horizon on the coarse grid and only the end on the fine one.  migrateGrid resamples the coarse value function at every node of
the fine grid in one launch of resample_kernel, from the fine grid's coordinate vectors alone: both grids are `low_mem` here and no
dense coordinate array is ever built (eval_u, the route before, wants the fine grid's nodes as an M x 6 fp64 array).

The script prints the time of each part and, against a solve that ran the whole horizon on the fine grid, what the shortcut costs in
accuracy.  Nothing is asserted.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import resample

nC = int(sys.argv[1]) if len(sys.argv) > 1 else 9
nF = int(sys.argv[2]) if len(sys.argv) > 2 else 13
horizon = float(sys.argv[3]) if len(sys.argv) > 3 else 0.4
nth = 12
speed, turn, radius = 1.0, 1.0, 0.8
col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
top = 2 * np.pi * (1 - 1.0 / nth)


def game(n):
    g = lsp.createGrid(col([-2, -2, 0, -2, -2, 0]), col([2, 2, top, 2, 2, top]), col([n, n, nth, n, n, nth], np.int64), [2, 5], low_mem=True)
    pair = lsp.DubinsPair6D(g, v_e=speed, v_p=speed, w_e=turn, w_p=turn)
    sd = lsp.Bundle(dict(grid=g, hamFunc=pair.hamiltonian, partialFunc=pair.dissipation, derivFunc=lsp.upwindFirstENO2))
    return g, sd


def capture_set(g):
    ax = [torch.as_tensor(np.asarray(v).ravel(), device="cuda") for v in g.vs]
    shape = tuple(len(a) for a in ax)
    X = [a.reshape([shape[d] if k == d else 1 for k in range(6)]) for d, a in enumerate(ax)]
    return (((X[0] - X[3]) ** 2 + (X[1] - X[4]) ** 2).sqrt() - radius).expand(shape).contiguous()


def solve(sd, data, t0, t1):
    torch.cuda.synchronize()
    start = time.time()
    V = lsp.HJIPDE_solve(data, np.array([t0, t1]), sd, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True)))[0]
    torch.cuda.synchronize()
    return V, time.time() - start


gC, sdC = game(nC)
gF, sdF = game(nF)
split = 0.75 * horizon

VC, tC = solve(sdC, capture_set(gC), 0.0, split)
torch.cuda.synchronize()
start = time.time()
VF0, info = lsp.transformData(gC, VC, gF, return_info=True)              # migrateGrid(gC, VC, gF), with the counts
torch.cuda.synchronize()
tM = time.time() - start
VF, tF = solve(sdF, VF0, split, horizon)
print("coarse %s to t = %.2f: %.2f s; migrated onto %s in %.4f s (%s; %d of %d nodes inside the coarse grid); fine to t = %.2f: %.2f s"
      % (tuple(VC.shape), split, tC, tuple(VF0.shape), tM, resample.last_path(), int(info["counts"]), info["nodes"], horizon, tF))

Vref, tR = solve(sdF, capture_set(gF), 0.0, horizon)
diff = (VF - Vref).abs()
print("the whole horizon on the fine grid: %.2f s; |coarse-to-fine - fine| max %.3g, mean %.3g (position step %.3g -> %.3g)"
      % (tR, float(diff.max()), float(diff.mean()), float(np.asarray(gC.dx).ravel()[0]), float(np.asarray(gF.dx).ravel()[0])))
print("the two agree on the side of the tube for %.2f %% of the nodes" % (100 * float(((VF <= 0) == (Vref <= 0)).double().mean())))
