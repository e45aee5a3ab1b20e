"""NumPy restatement of the level-set extraction of include/hj_surface.h (levelsetpy_amd/surface.py): marching
simplices on the Kuhn subdivision, vectorised over the grid.  UNPINNED -- the reference's implicit_mesh is skimage's
Lewiner marching cubes, which cannot be run here; tests/test_surface_ref.py proves this restatement on closed-form
surfaces (manifoldness, Euler characteristic, enclosed volume, orientation against geometry, contourpy in 2-D), and
tests/test_gpu_surface.py holds the kernels to it bit for bit.

Definition.  Node x_d(i) = xmin[d] + i*dx[d] (product and sum rounded separately).  Inside: phi <= level.  Corner b of
a cell: bit d selects the upper node of axis d.  Simplex s of a cell: the s-th permutation p of (0..D-1) in
lexicographic order, vertices v0 = 0, v_k = v_{k-1} | 1 << p[k-1].  Edge a < b (bit sets) of a cell: key =
node(a) * (2^D - 1) + ((b & ~a) - 1); active iff both ends finite and exactly one inside; its vertex sits at
t = (level - phi_a) / (phi_b - phi_a).  verts in ascending key; faces by cell, then simplex.
"""
import itertools

import numpy as np


def permutations(D):
    """[(p, chain of corner numbers v0..vD, parity of p)] in lexicographic order of p."""
    out = []
    for p in itertools.permutations(range(D)):
        chain = [0]
        for a in p:
            chain.append(chain[-1] | (1 << a))
        inv = sum(1 for i in range(D) for j in range(i + 1, D) if p[i] > p[j])
        out.append((p, chain, inv & 1))
    return out


def parity(seq):
    return sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j]) & 1


def simplex_faces(D, inside, par):
    """The oriented faces of one simplex: `inside` is the tuple of D + 1 booleans of its vertices v0..vD, `par` the parity
    of its permutation.  Each face is a list of D edges (i, o): simplex vertex numbers, i inside, o outside."""
    ins = [k for k in range(D + 1) if inside[k]]
    outs = [k for k in range(D + 1) if not inside[k]]
    if not ins or not outs:
        return []
    flip = par ^ parity(ins + outs)
    if D == 3:
        if len(ins) == 1:
            faces = [[(ins[0], o) for o in outs]]
        elif len(ins) == 3:
            faces = [[(i, outs[0]) for i in ins]]
        else:
            q = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
            faces = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
        if flip:
            faces = [[f[0], f[2], f[1]] for f in faces]
        return faces
    if len(ins) == 1:
        face = [(ins[0], outs[0]), (ins[0], outs[1])]
    else:
        face = [(ins[0], outs[0]), (ins[1], outs[0])]
    if flip ^ (len(ins) == 2):
        face = face[::-1]
    return [face]


def _shift(N, c, upper):
    """Slices of the nodes that have a neighbour at corner offset c (upper: that neighbour)."""
    return tuple((slice(1, n) if upper else slice(0, n - 1)) if (c >> d) & 1 else slice(None) for d, n in enumerate(N))


def _corner(N, c):
    """Slices of corner c of every cell."""
    return tuple(slice(1, n) if (c >> d) & 1 else slice(0, n - 1) for d, n in enumerate(N))


def level_set_ref(N, xmin, dx, phi, level=0.0, with_simplex=False):
    """(verts (nv, D) fp64, faces (nf, D) int32) of the array phi (shape N, fp64 or fp32) on the grid (N, xmin, dx).
    with_simplex: also (cell linear index in the cell grid, simplex number) of every face."""
    N = tuple(int(n) for n in N)
    D = len(N)
    assert D in (2, 3) and all(n >= 2 for n in N)
    level = float(level)
    p = np.asarray(phi).astype(np.float64).reshape(N)
    with np.errstate(invalid="ignore"):
        inside = p <= level
    fin = np.isfinite(p)
    NE = (1 << D) - 1
    stride = [int(np.prod(N[d + 1:])) for d in range(D)]

    # ---- edges: active[node, class]
    active = np.zeros(N + (NE,), dtype=bool)
    for c in range(1, NE + 1):
        lo, hi = _shift(N, c, False), _shift(N, c, True)
        active[lo + (c - 1,)] = fin[lo] & fin[hi] & (inside[lo] != inside[hi])
    flat = active.reshape(-1)
    vid = (np.cumsum(flat, dtype=np.int64) - flat).reshape(N + (NE,))       # exclusive: ascending key
    keys = np.flatnonzero(flat)
    node, c = keys // NE, keys % NE + 1
    idx = np.unravel_index(node, N)
    other = node + sum(((c >> d) & 1) * stride[d] for d in range(D))
    pf = p.reshape(-1)
    pa, pb = pf[node], pf[other]
    t = (level - pa) / (pb - pa)
    verts = np.empty((len(keys), D), dtype=np.float64)
    for d in range(D):
        step = idx[d].astype(np.float64) * float(dx[d])
        x = float(xmin[d]) + step
        move = t * float(dx[d])
        verts[:, d] = np.where((c >> d) & 1, x + move, x)

    # ---- faces: per cell and simplex up to two faces
    M = tuple(n - 1 for n in N)
    perms = permutations(D)
    cin = [inside[_corner(N, b)] for b in range(1 << D)]
    cfin = [fin[_corner(N, b)] for b in range(1 << D)]
    slots = np.full(M + (len(perms), 2, D), -1, dtype=np.int64)
    for s, (perm, chain, par) in enumerate(perms):
        ok = np.ones(M, dtype=bool)
        code = np.zeros(M, dtype=np.int64)
        for k, b in enumerate(chain):
            ok &= cfin[b]
            code |= cin[b].astype(np.int64) << k
        for pat in range(1, (1 << (D + 1)) - 1):
            sel = ok & (code == pat)
            if not sel.any():
                continue
            faces = simplex_faces(D, tuple(bool((pat >> k) & 1) for k in range(D + 1)), par)
            for j, face in enumerate(faces):
                for m, (i, o) in enumerate(face):
                    a, b = chain[min(i, o)], chain[max(i, o)]
                    ids = vid[_corner(N, a) + ((b & ~a) - 1,)]
                    slots[..., s, j, m][sel] = ids[sel]
    used = slots[..., 0] >= 0
    faces = slots[used]
    assert len(verts) < 2 ** 31 and len(faces) < 2 ** 31
    faces = faces.astype(np.int32)
    if with_simplex:
        where = np.argwhere(used)
        cell = np.ravel_multi_index(tuple(where[:, d] for d in range(D)), M)
        return verts, faces, cell, where[:, D]
    return verts, faces


# ------------------------------------------------------------------------------------------ what the tests measure
def canonical(faces):
    """Every face rotated so that its smallest index comes first (orientation kept)."""
    faces = np.asarray(faces)
    if faces.shape[0] == 0:
        return faces
    k = np.argmin(faces, axis=1)
    D = faces.shape[1]
    cols = (k[:, None] + np.arange(D)[None, :]) % D
    return np.take_along_axis(faces, cols, axis=1)


def directed_edges(faces):
    """3-D: the 3 directed edges of every triangle, (3 nf, 2)."""
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_census(faces):
    """(undirected edges (ne, 2), faces per undirected edge, occurrences of the most frequent directed edge)."""
    e = directed_edges(faces)
    _, dcount = np.unique(e, axis=0, return_counts=True)
    und, ucount = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    return und, ucount, int(dcount.max()) if len(dcount) else 0


def euler_characteristic(nv, faces):
    und, _, _ = edge_census(faces)
    return int(nv) - len(und) + len(faces)


def measure(verts, faces):
    """(length, signed area) in 2-D, (area, signed volume) in 3-D."""
    p = np.asarray(verts)[np.asarray(faces, dtype=np.int64)]
    if p.shape[-1] == 2:
        a, b = p[:, 0], p[:, 1]
        return float(np.linalg.norm(b - a, axis=1).sum()), float(0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).sum())
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()), float((a * np.cross(b, c)).sum() / 6.0)


def mesh_grid(N, xmin, dx):
    return np.meshgrid(*[float(xmin[d]) + np.arange(N[d]) * float(dx[d]) for d in range(len(N))], indexing="ij")


def linspace_grid(lo, hi, N):
    """(xmin, dx) of nodes linspace(lo[d], hi[d], N[d])."""
    return [float(v) for v in lo], [(float(h) - float(l)) / (n - 1) for l, h, n in zip(lo, hi, N)]


# ------------------------------------------------------------------------------------------ the closed-form cases
def _case(N, lo, hi, fn, level=0.0):
    xmin, dx = linspace_grid(lo, hi, N)
    # nodes as np.linspace gives them, so that lattice points such as 0.5 are exact
    X = np.meshgrid(*[np.linspace(l, h, n) for l, h, n in zip(lo, hi, N)], indexing="ij")
    phi = fn(*X)
    phi.setflags(write=False)
    return dict(N=tuple(N), xmin=xmin, dx=dx, phi=phi, level=level)


def sphere(n, r=0.6, centre=(0.03, -0.02, 0.01)):
    cx, cy, cz = centre
    return _case((n,) * 3, (-1,) * 3, (1,) * 3, lambda x, y, z: np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r)


def torus(n=17, R=0.6, r=0.25):
    return _case((n,) * 3, (-1,) * 3, (1,) * 3, lambda x, y, z: np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r)


def sphere_on_nodes(n=17):
    """r = 0.5 about the origin: the 6 nodes (+-0.5, 0, 0), ... lie exactly on the level."""
    return sphere(n, 0.5, (0.0, 0.0, 0.0))


def anisotropic():
    return _case((9, 11, 13), (-1,) * 3, (1,) * 3, lambda x, y, z: np.sqrt(x * x + y * y + z * z) - 0.5, level=0.1)


def cut_sphere(n=17):
    """A sphere whose centre is 0.1 inside the face x = xmin: the surface is open there."""
    return sphere(n, 0.5, (-0.9, 0.02, -0.03))


def ellipse():
    return _case((23, 31), (-1, -1.5), (1, 1), lambda x, y: np.sqrt((x - .05) ** 2 + (.8 * (y + .2)) ** 2) - .6)


def extract(case, **kw):
    return level_set_ref(case["N"], case["xmin"], case["dx"], case["phi"], case["level"], **kw)
