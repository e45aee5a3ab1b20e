#!/usr/bin/env python3
"""Curvature-regularised front propagation, as a ToolboxLS script writes it: termSum of motion in the normal direction
(termNormal) and motion by mean curvature (termCurvature), integrated with odeCFL3 on device tensors.

    python examples/curvature_flow.py [n] [t_end]

A star-shaped front grows outward at speed a while curvature b smooths its points.  Needs an MI355X.  Prints the time,
the area inside the front and the maximum curvature on it at a few instants; the level set never leaves the GPU.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                    # noqa: E402
import levelsetpy_amd as lsp    # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 201
t_end = float(sys.argv[2]) if len(sys.argv) > 2 else 0.2

g = lsp.createGrid(-np.ones((2, 1)), np.ones((2, 1)), n * np.ones((2, 1), dtype=np.int64))
x, y = g.xs
theta = np.arctan2(y, x)
data0 = np.sqrt(x ** 2 + y ** 2) - (0.4 + 0.12 * np.cos(5 * theta))      # a five-pointed star

normal = lsp.Bundle(dict(grid=g, speed=0.5, derivFunc=lsp.upwindFirstWENO5))
curvature = lsp.Bundle(dict(grid=g, b=0.02, curvatureFunc=lsp.curvatureSecond))
schemeData = lsp.Bundle(dict(grid=g, innerFunc=[lsp.termNormal, lsp.termCurvature], innerData=[normal, curvature]))
options = lsp.odeCFLset(lsp.Bundle(dict(factorCFL=0.5)))

phi = torch.as_tensor(data0.reshape(-1, 1), device="cuda")
cell = float(np.prod(np.asarray(g.dx).ravel()))
t = 0.0
t0 = time.perf_counter()
for t_next in np.linspace(0, t_end, 5)[1:]:
    t, phi, schemeData = lsp.odeCFL3(lsp.termSum, [t, float(t_next)], phi, options, schemeData)
    kappa, _ = lsp.curvatureSecond(g, phi.reshape(g.shape))
    front = phi.reshape(g.shape).abs() < float(np.max(np.asarray(g.dx)))
    print("t = %.3f  area %.4f  max |kappa| on the front %.2f  (%s, %.2f s)"
          % (t, float((phi < 0).sum()) * cell, float(kappa[front].abs().max()), phi.device, time.perf_counter() - t0))
