"""Level sets of a value function as indexed meshes, extracted on the device: extract_level_set, level_set_measure,
implicit_mesh (reference Visualization/mesh_implicit.py:12) -- the last step of a reachability workflow: the
boundary of the reachable set as line segments (2-D grids) or triangles (3-D grids).

All of it runs in libhj_surface.so (include/hj_surface.h): `classify_kernel`, `scan_blocks_kernel`, `emit_kernel`.
Only the two counts per array and the O(N^(D-1)) mesh cross to the host, never the O(N^D) value function.
NumPy in -> NumPy out; a device tensor or HostView in -> tensors on the same device.  Stored value functions with
a time axis are time FIRST, as everywhere in this package.

Parity.  UNPINNED, checked against the NumPy restatement tests/surface_ref.py: the reference's implicit_mesh calls
skimage's Lewiner marching cubes, which cannot be run here; this module is marching simplices on the Kuhn
subdivision ("Level-set extraction"), which is watertight by construction, has no ambiguous cases and
serves 2-D and 3-D alike.  The surfaces agree to second order in dx; the triangles do not.
"""
import ctypes as C

import numpy as np

from . import _sffi
from .context import is_tensor, require_gpu
from .lazy import HostView
from ._marshal import device_data, dtype_name, fields, ptr, stream, unlazy, wants_tensor
from .utilities import Bundle, error

__all__ = ["extract_level_set", "level_set_measure", "implicit_mesh"]


def descriptor(g, dtype_name):
    """hjq_grid of the nodes g.vs (not g.N: augmentPeriodicData lengthens vs and leaves N); boundary kinds are not read."""
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
    dx = [float(v) for v in np.asarray(g.dx).ravel()]
    N = tuple(len(v) for v in vs)
    D = len(N)
    return _sffi.grid_descriptor(D, N, [float(v[0]) for v in vs], [float(v[-1]) for v in vs], dx, [0] * D, [0] * D, dtype_name), N


def extract_fields(desc, N, t, level):
    """The meshes of one array or a time-first stack `t` (contiguous device tensor) on the grid `desc` describes:
    a list of (verts (nv, D) fp64, faces (nf, D) int32) device tensors, one pair per array."""
    torch = require_gpu()
    lib = _sffi.lib()
    D = len(N)
    F, stride = fields(t, N)
    level = float(level)
    need = C.c_size_t(0)
    _sffi.check(lib.hjs_workspace_size(C.byref(desc), F, C.byref(need)))
    work = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=t.device)
    counts = torch.empty((F, 2), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        raw = stream(torch, t.device)
        _sffi.check(lib.hjs_count(C.byref(desc), ptr(t), F, stride, level, ptr(work), need.value, ptr(counts), raw))
        host = counts.cpu().numpy()                      # the one synchronisation: 16 bytes per array
        if int(host.max()) >= 2 ** 31:
            error('level set of %d vertices / %d faces: int32 indices hold fewer than 2^31' % (host[:, 0].max(), host[:, 1].max()))
        nv, nf = host[:, 0], host[:, 1]
        verts = torch.empty((int(nv.sum()), D), dtype=torch.float64, device=t.device)
        faces = torch.empty((int(nf.sum()), D), dtype=torch.int32, device=t.device)
        hc = (C.c_int64 * (2 * F))(*[int(v) for v in host.ravel()])
        _sffi.check(lib.hjs_emit(C.byref(desc), ptr(t), F, stride, level, ptr(work), need.value, hc,
                                 ptr(verts) if verts.numel() else None, ptr(faces) if faces.numel() else None, raw))
    v0 = np.concatenate([[0], np.cumsum(nv)])
    f0 = np.concatenate([[0], np.cumsum(nf)])
    return [(verts[int(v0[f]):int(v0[f + 1])], faces[int(f0[f]):int(f0[f + 1])]) for f in range(F)]


def _bundle(pair, proto):
    verts, faces = pair
    if wants_tensor(proto):
        p = unlazy(proto)
        if is_tensor(p) and not p.is_cuda:
            verts, faces = verts.to(p.device), faces.to(p.device)
    else:
        verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    return Bundle(dict(verts=verts, faces=faces))


def extract_level_set(g, data, level=0.0):
    """The set {x : data(x) = level} on grid g as an indexed mesh: Bundle(verts, faces).

      verts  (nv, g.dim) fp64 coordinates, one per grid or diagonal edge that the level crosses
      faces  (nf, g.dim) int32 indices into verts: line segments with the inside (data <= level) to their left on a
             2-D grid, triangles whose right-hand normal points toward increasing data on a 3-D grid

    A stack with a leading time axis gives a list of bundles, one per array, from one pass over the stack.  NumPy /
    HostView / device tensor in -> NumPy / tensor / tensor out.  Periodic axes are not closed: apply
    augmentPeriodicData first for the cell between the last and the first node.  NaN / inf nodes cut a hole.
    """
    if g.dim not in (2, 3):
        error('extract_level_set works on 2-D and 3-D grids (this one has %d dimensions): take a slice or a '
              'projection with proj(g, data, dimsToRemove, xs) first' % g.dim)
    t = device_data(data)
    desc, N = descriptor(g, dtype_name(t))
    if tuple(t.shape) == tuple(N) + (1,):
        t = t.reshape(N)
    out = [_bundle(pair, data) for pair in extract_fields(desc, N, t, level)]
    return out if t.dim() == len(N) + 1 else out[0]


def level_set_measure(verts, faces):
    """(size, enclosed) of a mesh from extract_level_set: length and enclosed area of 2-D segments (shoelace formula),
    area and enclosed volume of 3-D triangles (divergence theorem).  `enclosed` is positive for a closed mesh around
    an inside region and meaningless for an open one."""
    if isinstance(verts, HostView):
        verts = unlazy(verts)
    if isinstance(faces, HostView):
        faces = unlazy(faces)
    if is_tensor(verts):
        import torch
        p = verts[faces.long()]                              # (nf, D, D)
        if p.shape[-1] == 2:
            a, b = p[:, 0], p[:, 1]
            size = torch.linalg.norm(b - a, dim=1).sum()
            enclosed = 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).sum()
        else:
            a, b, c = p[:, 0], p[:, 1], p[:, 2]
            size = 0.5 * torch.linalg.norm(torch.linalg.cross(b - a, c - a), dim=1).sum()
            enclosed = (a * torch.linalg.cross(b, c)).sum() / 6.0
        return float(size), float(enclosed)
    p = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    if p.shape[-1] == 2:
        a, b = p[:, 0], p[:, 1]
        return float(np.linalg.norm(b - a, axis=1).sum()), float(0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).sum())
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    return (float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()),
            float((a * np.cross(b, c)).sum() / 6.0))


def implicit_mesh(surface, level=None, spacing=(1., 1., 1.), gd='ascent', edge_color='k', face_color='r'):
    """mesh_implicit.py:12: the level set of a 3-D array as a matplotlib Poly3DCollection: Bundle(mesh, verts, faces) --
    the reference's Bundle(mesh, verts) plus the index array, so that mesh = Poly3DCollection(verts[faces]) can be rebuilt.

    The array's first node is the origin and `spacing` the node distance per axis, so verts are in units of spacing.
    level=None: the mean of the array's min and max (as skimage's marching_cubes).  gd='ascent': the triangles' right-hand
    normal points toward increasing values; 'descent' reverses every triangle.  The mesh is this package's marching
    simplices, extracted on the device, not Lewiner marching cubes (module docstring).  matplotlib is imported here
    only: without it everything else in this module works."""
    if gd not in ('ascent', 'descent'):
        error("gd must be 'ascent' or 'descent'")
    t = device_data(surface)
    if t.dim() != 3:
        error('implicit_mesh takes a 3-D array')
    if len(spacing) != 3:
        error('spacing must have 3 entries')
    from mpl_toolkits.mplot3d.art3d import Poly3DCollection
    if level is None:
        level = 0.5 * (float(t.min()) + float(t.max()))
    N = tuple(int(n) for n in t.shape)
    dx = [float(s) for s in spacing]
    desc = _sffi.grid_descriptor(3, N, [0.0] * 3, [(n - 1) * h for n, h in zip(N, dx)], dx, [0] * 3, [0] * 3, dtype_name(t))
    verts, faces = extract_fields(desc, N, t, level)[0]
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    if gd == 'descent':
        faces = faces[:, ::-1]
    mesh = Poly3DCollection(verts[faces])
    mesh.set_edgecolor(edge_color)
    mesh.set_facecolor(face_color)
    return Bundle(dict(mesh=mesh, verts=verts, faces=np.ascontiguousarray(faces)))
