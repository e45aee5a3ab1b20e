#!/usr/bin/env python3
"""The boundary of a backward reachable tube as a triangle mesh, extracted on the device.

    python examples/reachable_tube_mesh.py [n] [t_end] [out.obj]

The air3D problem of examples/air3d_brt.py is solved with every tau slice kept; the stack never leaves the GPU.
ONE extract_level_set call turns all slices into indexed meshes of their zero level sets (marching simplices on the
Kuhn subdivision, libhj_surface.so): only two counts per slice and the O(n^2) meshes cross to the host, never the
O(n^3) value functions.  Prints vertices, triangles, area and enclosed volume per slice, next to the node count the
other examples stop at; with a third argument the last slice is written as a Wavefront .obj.  The heading axis is
periodic: augmentPeriodicData adds the node that closes the last cell, so the mesh spans the whole period.  It stays
open on the two heading faces, where the tube runs through; the volume is therefore the flux of F = (x, y, 0) / 2
(div F = 1, no flux through a heading face), exact for a triangle mesh.  Needs an MI355X (the package has no CPU
fallback).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 61
t_end = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
obj = sys.argv[3] if len(sys.argv) > 3 else None

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
data0 = torch.as_tensor(lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 0.5), device="cuda")     # a tensor in: tensors out
dubins = lsp.DubinsVehicleRel(g, 1, 1)
schemeData = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation,
                             dissFunc=lsp.artificialDissipationGLF, CoStateCalc=lsp.upwindFirstWENO5))
tau = np.linspace(0, t_end, 6)
tube, tau_out, _ = lsp.HJIPDE_solve(data0, tau, schemeData, 'minVOverTime', lsp.Bundle(dict(quiet=True)))

gFull, tubeFull = lsp.augmentPeriodicData(g, tube)     # still on the device: one more heading plane per slice
torch.cuda.synchronize()
t0 = time.perf_counter()
meshes = lsp.extract_level_set(gFull, tubeFull, 0.0)   # the whole stack: one count pass, one emit launch per slice
torch.cuda.synchronize()                               # the emit launches are asynchronous
sec = time.perf_counter() - t0
assert len(meshes) == len(tau_out)


def flux_volume(verts, faces):
    p = verts[faces.long()]
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    normal = 0.5 * torch.linalg.cross(b - a, c - a)     # area vector, toward increasing V: out of the tube
    centre = (a + b + c) / 3.0
    return float(0.5 * (centre[:, 0] * normal[:, 0] + centre[:, 1] * normal[:, 1]).sum())


cell = float(np.prod(np.asarray(g.dx)))
inside = (tube <= 0).flatten(1).sum(1).cpu().numpy()
print("grid %d^3, %d tau slices meshed in %.1f ms" % (n, len(meshes), 1e3 * sec))
print("   tau    verts    faces     area   volume   (nodes <= 0) * cell")
for t, m, count in zip(tau_out, meshes, inside):
    area, _ = lsp.level_set_measure(m.verts, m.faces)
    print("%6.3f %8d %8d %8.4f %8.4f %10.4f" % (t, m.verts.shape[0], m.faces.shape[0], area, flux_volume(m.verts, m.faces),
                                                cell * count))

if obj:
    last = meshes[-1]
    verts, faces = last.verts.cpu().numpy(), last.faces.cpu().numpy()
    with open(obj, "w") as f:
        f.write("# zero level set of the air3D reachable tube at tau = %g: x, y, relative heading\n" % tau_out[-1])
        for x, y, z in verts:
            f.write("v %.17g %.17g %.17g\n" % (x, y, z))
        for a, b, c in faces + 1:
            f.write("f %d %d %d\n" % (a, b, c))
    print("wrote %s: %d vertices, %d triangles" % (obj, len(verts), len(faces)))
