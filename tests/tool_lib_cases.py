"""The argument checks of nine stateless libraries (libhj_query / surface / ttr / rollout / batch / hiquery / plant / shapes / hishapes .so) as data:
calls that are refused, or accepted as "nothing to do", before the first HIP call -- so they run on a machine without a GPU.

Every case is (library, id, function, arguments, return code, word of <prefix>_last_error()).  An argument is an int, a float,
None (a null pointer: every data pointer is null, so no case can reach a launch), FAKE (a non-null address where a check wants
one: it is only compared with null, never read) or a Grid / Plant / UserPlant / Tables / Program spec below, passed by address.
tests/test_tool_libs_host.py asserts the cases through ctypes; tools/tool_lib_refusals.py dumps code and whole message of every
call (to compare two builds of the libraries) and writes the same calls as a stand-alone C++ program (for the host sanitizers)."""
import ctypes as C
import math

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
ENO2, WENO5 = 0, 2
DUBINS, INTEGRATOR, USER = 0, 1, 100
PLANE5D, PAIR6D = 50, 51
NAN = float("nan")
FAKE = "fake"                     # address 0x1000

LIBS = {"query": "hjq", "surface": "hjs", "ttr": "hjt", "rollout": "hjr", "batch": "hjb", "hiquery": "hjx", "plant": "hjp", "shapes": "hjg",
        "hishapes": "hjk"}


class Grid:
    """hjq_grid (width 4) or hjh_grid (width 6) by value: n nodes per axis from 0 with spacing 0.1, extrapolated; `put` overwrites
    (field, axis 0) entries, or with a list the leading ones."""
    def __init__(self, ndim, n=8, dtype=0, width=4, **put):
        self.ndim, self.dtype, self.width = ndim, dtype, width
        self.N, self.xmin, self.xlast = [n] * width, [0.0] * width, [0.1 * (n - 1)] * width
        self.dx, self.bc, self.toward_zero = [0.1] * width, [0] * width, [0] * width
        for k, v in put.items():
            v = v if isinstance(v, list) else [v]
            getattr(self, k)[:len(v)] = v


class Plant:
    """hjr_plant: both modes min, every parameter 1."""
    def __init__(self, id):
        self.id = id


class UserPlant(Plant):
    """hjp_plant: both modes min, no parameter."""


class Tables:
    """hjb_tables with every coordinate and aux table at FAKE."""


class Program:
    """hjg_program (width 4) or hjk_program (width 6): (code, arg, off) triples, (address, dtype id, per_member) triples with FAKE
    or None for the address, and one coordinate-table address (FAKE or None) per entry of `coord`; n_ops / n_arrays overwrite the
    counts the lists give."""
    def __init__(self, ops, arrays=(), coord=(), width=4, n_ops=None, n_arrays=None):
        self.ops, self.arrays, self.coord, self.width = list(ops), list(arrays), list(coord), width
        self.n_ops = len(self.ops) if n_ops is None else n_ops
        self.n_arrays = len(self.arrays) if n_arrays is None else n_arrays


def grid_variants(ndim, too_few, width=4, bad_ndim=(0, 5)):
    """(id, Grid or None, word of the refusal the table of descriptor cases expects from query / rollout / surface / hiquery / plant).
    toolarge: 2^30 nodes on each of three axes, whose product does not fit 64 bits (only ndim >= 3 has three axes)."""
    def G(nd, **kw):
        return Grid(nd, width=width, **kw)
    return [("null", None, "null")] + [("ndim%d" % nd, G(nd), "ndim") for nd in bad_ndim] + [
            ("dtype7", G(ndim, dtype=7), "dtype"), ("N0", G(ndim, N=0), "N[0]")] + [("N%d" % n, G(ndim, N=n), "N[0]") for n in too_few] + [
            ("bc9", G(ndim, bc=9), "boundary"), ("dx0", G(ndim, dx=0.0), "dx"), ("dxnan", G(ndim, dx=NAN), "dx"),
            ("toolarge", G(max(ndim, 3), N=[1 << 30] * 3), "too large")]


def cases():
    out = []

    def add(lib, cid, fn, args, rc, word=""):
        out.append((lib, cid, LIBS[lib] + "_" + fn, args, rc, word))

    # ---- query: (a) V at states, (b) costates, (c) projection
    def query(g, scheme=ENO2, costate=None):
        return [("interp_points", [g, None, 1, 0, None, 1, None, 0, None]),
                ("costate_points", [g, scheme, None, 1, 0, None, 1, costate, None, None, None, 0, None]),
                ("project_minmax", [g, None, 1, 0, 1, 0, None, None])]
    for cid, g, word in grid_variants(2, ()):
        for fn, args in query(g):
            add("query", "%s-%s" % (fn, cid), fn, args, EINVAL, word)
    for fn, args in query(Grid(2)):
        add("query", "%s-nulldata" % fn, fn, args, EINVAL, "null")
    for sch in (WENO5, 9):
        add("query", "costate_points-scheme%d" % sch, *query(Grid(2), sch, FAKE)[1], EUNSUPPORTED, "scheme")   # its output is tested first

    # ---- surface: the boundary kinds are not read, so bc 9 reaches the null-argument check
    def surface(g):
        return [("workspace_size", [g, 1, None]), ("count", [g, None, 1, 0, 0.0, None, 0, None, None]),
                ("emit", [g, None, 1, 0, 0.0, None, 0, None, None, None, None])]
    for cid, g, word in grid_variants(2, (1,)):
        for fn, args in surface(g):
            if cid == "toolarge":         # the library's own cap, tested axis by axis: more than 2^32 - 256 nodes have no kernel
                add("surface", "%s-%s" % (fn, cid), fn, args, EUNSUPPORTED, "more than 2^32")
            else:
                add("surface", "%s-%s" % (fn, cid), fn, args, EINVAL, "null" if cid == "bc9" else word)
    for nd in (1, 4):
        for fn, args in surface(Grid(nd)):
            add("surface", "%s-ndim%d" % (fn, nd), fn, args, EUNSUPPORTED, "2-D and 3-D")
    for fn, args in surface(Grid(3)):
        add("surface", "%s-nulldata" % fn, fn, args, EINVAL, "null")
    # no vertex and no face anywhere: nothing is launched and nothing is read (the addresses are only compared with null)
    add("surface", "emit-nothing", "emit", [Grid(2), FAKE, 1, 0, 0.0, FAKE, 1 << 40, [0, 0], None, None, None], OK)

    # ---- ttr: no descriptor; dtype, mode, n
    def ttr(dtype=0, n=1, mode=0):
        return [("ttr_init", [dtype, None, n, 0.0, 0.0, None, None, None]),
                ("ttr_update", [dtype, None, n, 1.0, 0.0, 0.0, mode, None, None, None]),
                ("ttr_from_stack", [dtype, None, 2, max(n, 0), n, None, 0.0, mode, None, None])]
    for cid, kw, rc, word in (("dtype7", dict(dtype=7), EUNSUPPORTED, "dtype"), ("mode4", dict(mode=4), EINVAL, "mode"),
                              ("n-1", dict(n=-1), EINVAL, "negative"), ("n0", dict(n=0), OK, ""), ("nulldata", {}, EINVAL, "null")):
        for fn, args in ttr(**kw):
            if cid != "mode4" or fn != "ttr_init":              # hjt_ttr_init takes no mode
                add("ttr", "%s-%s" % (fn, cid), fn, args, rc, word)

    # ---- rollout: the double integrator on a 2-D grid
    def rollout(g, scheme=ENO2, plant=Plant(INTEGRATOR), nstates=1):
        return ["rollout", [g, scheme, None, 2, 64, None, nstates, 4, 0.01, plant, None, None, None, None, None]]
    for cid, g, word in grid_variants(2, ()):
        add("rollout", "rollout-%s" % cid, *rollout(g), EINVAL, word)
    for sch in (WENO5, 9):
        add("rollout", "rollout-scheme%d" % sch, *rollout(Grid(2), sch), EUNSUPPORTED, "scheme")
    add("rollout", "rollout-nullplant", *rollout(Grid(2), plant=None), EINVAL, "null plant")
    add("rollout", "rollout-plant3d", *rollout(Grid(2), plant=Plant(DUBINS)), EINVAL, "3 states")
    add("rollout", "rollout-userplant", *rollout(Grid(2), plant=Plant(USER)), EUNSUPPORTED, "plant 100")
    add("rollout", "rollout-N2", *rollout(Grid(2, N=2)), EINVAL, "too small")
    add("rollout", "rollout-nulldata", *rollout(Grid(2)), EINVAL, "null argument")
    add("rollout", "rollout-nostates", *rollout(Grid(2), nstates=0), OK)

    # ---- batch: the relative Dubins system on a 3-D grid; its own check reports a grid of another dimension
    def batch(g, tab=Tables(), scheme=ENO2, ham=DUBINS):
        return [("step_bounds", [g, tab, ham, None, 1, None, None, None, None]),
                ("substep", [g, tab, scheme, ham, 1, 0, None, None, 1, None]),
                ("integrate", [g, tab, scheme, ham, 3, 0, 0, None, None, None, 1, 0.0, 1.0, 0.8, 1e300, 1e-4, None, 0, None, None,
                               None, None])]
    for cid, g, word in grid_variants(3, (2,)):
        for fn, args in batch(g):
            add("batch", "%s-%s" % (fn, cid), fn, args, EINVAL, "dimensions" if cid in ("ndim0", "ndim5") else word)
    for fn, args in batch(Grid(3), tab=None):
        add("batch", "%s-nulltables" % fn, fn, args, EINVAL, "null")
    for fn, args in batch(Grid(3), ham=INTEGRATOR):
        add("batch", "%s-ham2d" % fn, fn, args, EINVAL, "2-D grids")
    for fn, args in batch(Grid(3), ham=USER):
        add("batch", "%s-userham" % fn, fn, args, EUNSUPPORTED, "Hamiltonian 100")
    for sch in (WENO5, 9):
        for fn, args in batch(Grid(3), scheme=sch)[1:]:
            add("batch", "%s-scheme%d" % (fn, sch), fn, args, EUNSUPPORTED, "scheme")
    for fn, args in batch(Grid(3)):
        add("batch", "%s-nulldata" % fn, fn, args, EINVAL, "null argument")
    add("batch", "nan_flags-dtype7", "nan_flags", [7, None, 1, 1, None, None], EINVAL, "dtype")

    # ---- hiquery: the entry points of query and rollout on a 5-D grid of six-axis descriptors; the plane on it
    def G5(**kw):
        return Grid(5, width=6, **kw)

    def hiquery(g, scheme=ENO2, costate=None):
        return [(fn, args) for fn, args in query(g, scheme, costate)]

    def hirollout(g, scheme=ENO2, plant=Plant(PLANE5D), nstates=1):
        return ["rollout", [g, scheme, None, 2, 8 ** 5, None, nstates, 4, 0.01, plant, None, None, None, None, None]]
    for cid, g, word in grid_variants(5, (), 6, (4, 7)):
        for fn, args in hiquery(g) + [tuple(hirollout(g))]:
            add("hiquery", "%s-%s" % (fn, cid), fn, args, EINVAL, word)
    for fn, args in hiquery(G5()):
        add("hiquery", "%s-nulldata" % fn, fn, args, EINVAL, "null")
    for sch in (WENO5, 9):
        add("hiquery", "costate_points-scheme%d" % sch, *hiquery(G5(), sch, FAKE)[1], EUNSUPPORTED, "scheme")
        add("hiquery", "rollout-scheme%d" % sch, *hirollout(G5(), sch), EUNSUPPORTED, "scheme")
    add("hiquery", "rollout-nullplant", *hirollout(G5(), plant=None), EINVAL, "null plant")
    add("hiquery", "rollout-plant6d", *hirollout(G5(), plant=Plant(PAIR6D)), EINVAL, "6 states")
    add("hiquery", "rollout-solverplant", *hirollout(G5(), plant=Plant(DUBINS)), EUNSUPPORTED, "plant 0")
    add("hiquery", "rollout-N2", *hirollout(G5(N=2)), EINVAL, "too small")
    add("hiquery", "rollout-nulldata", *hirollout(G5()), EINVAL, "null argument")
    add("hiquery", "rollout-nostates", *hirollout(G5(), nstates=0), OK)

    # ---- plant: both entry points up to the look at the registry -- id 5 is below HJP_PLANT_BASE, so nothing answers to it
    # whatever else the process has registered
    def plant(hi, g, scheme=ENO2, p=UserPlant(5), nstates=1, ntimes=2, sub=4, dt=0.01, stride=None):
        stride = (8 ** 5 if hi else 64) if stride is None else stride
        return ["rollout_hi" if hi else "rollout", [g, scheme, None, ntimes, stride, None, nstates, sub, dt, p, None, None, None, None, None]]
    for hi, nd, width, bad in ((False, 2, 4, (1, 5)), (True, 5, 6, (4, 7))):
        def G(**kw):
            return Grid(nd, width=width, **kw)
        fn = plant(hi, None)[0]
        for cid, g, word in grid_variants(nd, (), width, bad):
            add("plant", "%s-%s" % (fn, cid), *plant(hi, g), EINVAL, word)
        for cid, kw, rc, word in (("nullplant", dict(p=None), EINVAL, "null plant"), ("negative", dict(nstates=-1), EINVAL, "negative"),
                                  ("oneset", dict(ntimes=1), EINVAL, "two stored sets"), ("sub0", dict(sub=0), EINVAL, "sub_samples"),
                                  ("dtnan", dict(dt=NAN), EINVAL, "dt_small"), ("stride", dict(stride=10), EINVAL, "field_stride"),
                                  ("scheme2", dict(scheme=WENO5), EUNSUPPORTED, "scheme"), ("scheme9", dict(scheme=9), EUNSUPPORTED, "scheme"),
                                  ("unknownplant", {}, EINVAL, "unknown plant id 5")):
            add("plant", "%s-%s" % (fn, cid), *plant(hi, G(), **kw), rc, word)

    # ---- shapes (2-D grid of four-axis descriptors, rows of 8 values) and hishapes (5-D, six axes, rows of 64): a bad program
    # is a refusal with a message, never a launch.  SPHERE .. COMPLEMENT are 1 .. 9, SPHERE_OF (hishapes only) 10
    SPH, ARR, U, I, D, NOT, OF = (1, 0, 0), (5, 0, 0), (6, 0, 0), (7, 0, 0), (8, 0, 0), (9, 0, 0), (10, 2, 0)
    one = [(FAKE, 0, 0)]

    def scenes(lib, width, nd, n, P0):
        def G(ndim=nd, **kw):
            return Grid(ndim, n=n, width=width, **kw)

        def scene(cid, word, ops=(SPH,), g=G(), K=1, P=P0, out=None, out_dtype=0, flags=None, params=None, program=True, ncoord=None, **prog):
            prog.setdefault("coord", [FAKE] * ((nd if width == 4 else 6) if ncoord is None else ncoord))
            add(lib, "evaluate-" + cid, "evaluate", [g, Program(ops, width=width, **prog) if program else None, params, K, P, out, out_dtype,
                                                     flags, None], EUNSUPPORTED if out_dtype == 7 else EINVAL, word)
        return scene, G
    (lo, G4), (hi, G6) = scenes("shapes", 4, 2, 8, 8), scenes("hishapes", 6, 5, 4, 64)
    for scene, G, leaf in ((lo, G4, SPH), (hi, G6, OF)):       # the rows of the stack run the new leaf where the library has it
        scene("null-grid", "null grid", g=None)
        scene("dtype7", "dtype", g=G(dtype=7))
        scene("N-negative", "N[0]", g=G(N=-1))
        scene("out-dtype7", "out_dtype", out_dtype=7)
        # the program as a whole
        scene("null-program", "null program", program=False)
        scene("K0", "at least one member", K=0)
        scene("K-negative", "at least one member", K=-3)
        scene("P-negative", "negative", [ARR], arrays=one, P=-1)
        scene("no-instructions", "1 .. 64 instructions", [])
        scene("65-instructions", "1 .. 64 instructions", [SPH] + [NOT] * 63, n_ops=65)
        scene("9-arrays", "at most 8 array leaves", [ARR], arrays=one, n_arrays=9)
        scene("opcode0", "unknown opcode 0", [(0, 0, 0)])
        scene("opcode-negative", "unknown opcode -1", [(-1, 0, 0)])
        # the stack
        scene("underflow-union", "stack underflow", [leaf, U])
        scene("underflow-first", "stack underflow", [D, SPH])
        scene("underflow-complement", "stack underflow", [NOT])
        scene("overflow", "stack overflow", [SPH] * 8 + [leaf] + [U] * 8)
        scene("two-left", "leaves 2 values", [SPH, leaf])
        scene("three-left", "leaves 2 values", [leaf, SPH, SPH, I])
        scene("sphere-off-negative", "outside a row", [(1, 0, -1)], P=8)
        scene("sphere-P0", "outside a row", P=0)
        scene("mask-negative", "mask", [(2, -1, 0)])
        # array leaves
        scene("array-null", "array leaf 0 is null", [ARR], arrays=[(None, 0, 0)])
        scene("array-second-null", "array leaf 1 is null", [ARR, (5, 1, 0), U], arrays=[(FAKE, 0, 0), (None, 1, 1)])
        scene("array-dtype", "dtype 5", [ARR], arrays=[(FAKE, 5, 0)])
        scene("array-slot", "slot 1", [(5, 1, 0)], arrays=one)
        scene("array-none-declared", "slot 0 of 0", [ARR])
        # outputs: after the program
        scene("null-out", "null argument", params=FAKE, flags=FAKE)
        scene("null-flags", "null argument", params=FAKE, out=FAKE)
        scene("null-params", "null argument", out=FAKE, flags=FAKE)
    # the rows with a library's own numbers: the descriptor's limits, the first opcode past the last, parameter offsets (a sphere needs
    # ndim + 1 values, a rectangle and a halfspace 2 ndim, a sphere_of J ndim + J + 1), cylinder masks, the null coordinate table
    lo("ndim0", "ndim", g=G4(0), ncoord=0)
    lo("ndim5", "ndim", g=G4(5))
    lo("opcode10", "unknown opcode 10", [SPH, (10, 0, 0)])
    lo("sphere-off", "outside a row", [(1, 0, 6)], P=8)
    lo("cylinder-off", "outside a row", [(2, 1, 0)], P=2)
    lo("rect-off", "outside a row", [(3, 0, 5)], P=8)
    lo("halfspace-off", "outside a row", [(4, 0, 0)], g=G4(3), P=5, ncoord=3)
    lo("mask-axis2-of-2", "mask", [(2, 4, 0)])
    lo("mask-axis3-of-3", "mask", [(2, 8, 0)], g=G4(3), ncoord=3)
    lo("array-slot-negative", "slot -1", [(5, -1, 0)], arrays=one)
    lo("null-coord", "coordinate table of axis 1", coord=[FAKE, None])
    hi("ndim0", "ndim 0", g=G6(0))
    hi("ndim7", "ndim 7", g=G6(7))
    hi("N-2^31", "N[0]", g=G6(2, N=2 ** 31))
    hi("opcode11", "unknown opcode 11", [SPH, (11, 0, 0)])
    hi("sphere-off", "outside a row", [(1, 0, 3)], P=8)
    hi("rect-off", "outside a row", [(3, 0, 1)], g=G6(6), P=12)
    hi("halfspace-off", "outside a row", [(4, 0, 0)], P=9)
    hi("of-off", "outside a row", [(10, 2, 0)], P=12)
    hi("of-off-6x6", "+ 43 values", [(10, 6, 1)], g=G6(6), P=43)
    hi("of-off-negative", "outside a row", [(10, 1, -1)])
    for J in (0, 7, -1):
        hi("J%s" % ("-negative" if J < 0 else J), "J = %d" % J, [(10, J, 0)])
    for nd, mask in ((5, 32), (6, 64), (2, 4)):
        hi("mask-axis%d-of-%d" % (nd, nd), "mask", [(2, mask, 0)], g=G6(nd))
    hi("null-coord", "coordinate table of axis 4", coord=[FAKE] * 4 + [None, FAKE])

    # ---- hishapes: hjk_plan refuses what the grid check refuses (an axis of 2^31 nodes or more is outside the descriptor's
    # contract, as in libhj_shapes.so: (2^31 + 5, 2) is refused, by name) and hjk_decode with it; a node outside the grid
    def GN(*N):
        return Grid(len(N), width=6, N=list(N))
    for cid, g, word in (("N0-2^31+5", GN(2 ** 31 + 5, 2), "N[0] = 2147483653"), ("N1-2^31", GN(2, 2 ** 31), "N[1]"),
                         ("2^63", GN(*(2 ** 31 - 1,) * 3), "2^63")):
        add("hishapes", "plan-" + cid, "plan", [g, 1, FAKE], EINVAL, word)
        add("hishapes", "decode-" + cid, "decode", [g, 0, FAKE], EINVAL, word)
    add("hishapes", "plan-K0", "plan", [GN(4, 4), 0, FAKE], EINVAL, "at least one member")
    add("hishapes", "plan-null", "plan", [GN(4, 4), 1, None], EINVAL, "null argument")
    for node in (-1, 60):
        add("hishapes", "decode-node%d" % node, "decode", [GN(3, 4, 5), node, FAKE], EINVAL, "node")
    add("hishapes", "decode-null", "decode", [GN(3, 4, 5), 0, None], EINVAL, "null argument")
    return out


CASES = cases()


# ------------------------------------------------------------------------------------------ through ctypes
def modules():
    from levelsetpy_amd import _bffi, _gffi, _kffi, _pffi, _qffi, _rffi, _sffi, _tffi, _xffi
    return {"query": _qffi, "surface": _sffi, "ttr": _tffi, "rollout": _rffi, "batch": _bffi, "hiquery": _xffi, "plant": _pffi, "shapes": _gffi,
            "hishapes": _kffi}


def _ctypes_arg(a, keep):
    from levelsetpy_amd import _bffi, _gffi, _hffi, _kffi, _pffi, _qffi, _rffi
    addr = {FAKE: 0x1000, None: None}
    if isinstance(a, list):
        keep.append((C.c_int64 * len(a))(*a))
        return keep[-1]
    if isinstance(a, Grid):
        g = (_qffi if a.width == 4 else _hffi).Grid()
        g.ndim, g.dtype = a.ndim, a.dtype
        for k in ("N", "xmin", "xlast", "dx", "bc", "toward_zero"):
            for d in range(a.width):
                getattr(g, k)[d] = getattr(a, k)[d]
        keep.append(g)
    elif isinstance(a, UserPlant):
        keep.append(_pffi.plant_descriptor(a.id, 0, 0, []))
    elif isinstance(a, Plant):
        keep.append(_rffi.plant_descriptor(a.id, 0, 0, [1.0] * 4))
    elif isinstance(a, Program):
        p = (_gffi if a.width == 4 else _kffi).program(a.ops, [(addr[d], t, m) for d, t, m in a.arrays], [addr[c] for c in a.coord])
        p.n_ops, p.n_arrays = a.n_ops, a.n_arrays
        keep.append(p)
    elif isinstance(a, Tables):
        t = _bffi.Tables()
        for d in range(4):
            t.coord[d] = t.aux[d] = 0x1000
        keep.append(t)
    else:
        return a
    return C.byref(keep[-1])


def run(case, mods=None):
    """-> (return code, <prefix>_last_error() text, <prefix>_last_kernel() text) of one case."""
    lib_name, _, fn, args, _, _ = case
    f = getattr((mods or modules())[lib_name].lib(), fn)
    keep = []
    rc = f(*[C.cast(0x1000, t) if a is FAKE else _ctypes_arg(a, keep) for a, t in zip(args, f.argtypes)])   # FAKE: as the parameter's type
    pre, lib = LIBS[lib_name], (mods or modules())[lib_name].lib()
    return rc, getattr(lib, pre + "_last_error")().decode(), getattr(lib, pre + "_last_kernel")().decode()


def line(case, rc, err, kernel):
    return "%s %s rc=%d error=[%s] kernel=[%s]" % (case[0], case[1], rc, err, kernel)


# ------------------------------------------------------------------------------------------ as a C++ program
def _cxx_num(v):
    if isinstance(v, float):
        return "NAN" if math.isnan(v) else repr(v)
    return "%dll" % v if abs(v) > 2 ** 31 else str(v)


def cxx_program(lib_name):
    """The cases of one library as a program that prints line() of each: link it with that library's .hip file."""
    pre = LIBS[lib_name]
    body = []
    for k, case in enumerate(c for c in CASES if c[0] == lib_name):
        decl, call = [], []
        for j, a in enumerate(case[3]):
            v = "a%d_%d" % (k, j)
            if a is None:
                call.append("nullptr")
            elif a is FAKE:
                call.append("P")
            elif isinstance(a, list):
                decl.append("int64_t %s[] = {%s};" % (v, ", ".join(map(str, a))))
                call.append(v)
            elif isinstance(a, Grid):
                rows = ", ".join("{%s}" % ", ".join(_cxx_num(x) for x in getattr(a, f)) for f in ("N", "xmin", "xlast", "dx", "bc", "toward_zero"))
                decl.append("%s %s = {%d, %d, %s};" % ("hjq_grid" if a.width == 4 else "hjh_grid", v, a.ndim, a.dtype, rows))
                call.append("&" + v)
            elif isinstance(a, UserPlant):
                decl.append("hjp_plant %s = {%d, 0, 0, 0, {0.0}};" % (v, a.id))
                call.append("&" + v)
            elif isinstance(a, Plant):
                decl.append("hjr_plant %s = {%d, 0, 0, 0, {1.0, 1.0, 1.0, 1.0}};" % (v, a.id))
                call.append("&" + v)
            elif isinstance(a, Program):
                ptr = {FAKE: "P", None: "nullptr"}
                decl.append("%s %s = {%d, %d, {%s}, {%s}, {%s}};" % (
                    "hjg_program" if a.width == 4 else "hjk_program", v, a.n_ops, a.n_arrays, ", ".join("{%d, %d, %d}" % o for o in a.ops[:64]),
                    ", ".join("{%s, %d, %d}" % (ptr[d], t, m) for d, t, m in a.arrays), ", ".join(ptr[c] for c in a.coord)))
                call.append("&" + v)
            elif isinstance(a, Tables):
                decl.append("hjb_tables %s = {{P, P, P, P}, {P, P, P, P}};" % v)
                call.append("&" + v)
            else:
                call.append(_cxx_num(a))
        body.append("    { %s\n      const int rc = %s(%s);\n      printf(\"%s %s rc=%%d error=[%%s] kernel=[%%s]\\n\", rc, %s_last_error(), %s_last_kernel()); }"
                    % (" ".join(decl), case[2], ", ".join(call), case[0], case[1], pre, pre))
    return ("#include <cmath>\n#include <cstdio>\n#include \"hj_%s.h\"\n\n"
            "static const struct { template <typename T> operator T*() const { return (T*)0x1000; } } P{};    // FAKE, as any pointer type\n\n"
            "int main() {\n%s\n    return 0;\n}\n" % (lib_name, "\n".join(body)))
