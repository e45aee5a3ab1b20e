"""Guarded buffers: does an operation stay inside the arrays it is given?

Every other test of this suite compares what a kernel wrote INSIDE its output array with an oracle.  This module
checks the other half of the contract of include/hj_mi355x.h (arrays "owned by the caller", "y_in is never written",
"planes [plane_begin, plane_end) are updated"): an operation is handed views of ONE large allocation the test owns,
each view surrounded by guard bands, and afterwards

  (a) every guard of every argument is bitwise unchanged                                  -> BoundsError.kind "guard"
  (b) every input is bitwise equal to its state before the call                           -> "input"
  (c) the region of every output the contract says is updated holds no sentinel: every
      cell was written                                                                    -> "unwritten"
  (d) the regions the contract says are NOT updated (planes of `out` outside
      [plane_begin, plane_end), pad planes of a slab output) still hold what they held    -> "outside"
  (e) scratch arguments have intact guards; their contents are unspecified                -> "guard"

and, by `same_bits`, the results (arrays and host scalars) are bit for bit those of a reference run on fresh,
unguarded arrays                                                                          -> "differs".

Guard width, derived rather than tuned.  The farthest a stencil of the library reaches is HJ_STENCIL = 3 planes of
axis 0 (3 * depth for the deep-halo slab stepper).  Each guard is therefore max(4, 3 * depth + 1) axis-0 planes plus
256 elements (one more plane than the reach, and a workgroup's worth of elements for 1-D arrays and flat elementwise
kernels).  A stray access within that distance of an array lands in memory this pool owns: it is seen, and it cannot
fault the device.  STRAYS BEYOND THE GUARD ARE OUT OF THIS MODULE'S SIGHT: an access farther away than that lands in
another argument's region (seen, by that argument's own checks), in the unused rest of the pool (unseen), or outside
the pool (unseen here).

Fills.  The guards of inputs hold, in turn, quiet NaN, +1e30 and -1e30: NaN alone is not enough, because
fmax(NaN, x) = x hides a stray value in a max reduction, while the two finite fills win every max / min they
reach.  Outputs, scratch arrays and their guards hold a sentinel: a quiet NaN with a fixed payload, compared through
the integer view of the pool and never as a float (a kernel that legitimately produces NaN produces another payload).

Alignment.  The body of a carved array starts 512 bytes aligned plus `offset_elems` elements, so that a case can be
run at the alignment a fresh allocation has (0) and at element alignment (1, 2, 3): what a caller's view
`pool[k:k + n]` presents.

The same harness runs on CPU tensors (tests/test_guarded_pool.py proves with NumPy stand-ins that each check can
fail) and on the GPU (tests/test_gpu_memory_bounds.py, through the C ABI).
"""
import ctypes as C

import torch

STENCIL = 3
FILLS = {"nan": float("nan"), "+1e30": 1e30, "-1e30": -1e30}
OFFSETS = (0, 1, 2, 3)
SENTINEL_BITS = {torch.float64: 0x7FF80000DEADBEEF, torch.float32: 0x7FC0BEEF}
INT_VIEW = {torch.float64: torch.int64, torch.float32: torch.int32}
ALIGN_BYTES = 512


def guard_planes(depth=1):
    return max(4, STENCIL * depth + 1)


class BoundsError(AssertionError):
    """A failed check; `kind` names it: guard | input | unwritten | outside | differs."""

    def __init__(self, kind, message):
        AssertionError.__init__(self, "[%s] %s" % (kind, message))
        self.kind = kind


def _prod(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _planes(spec, n0):
    """None -> all body planes; (a, b) -> that range; a list of ranges stays; () -> none."""
    if spec is None:
        return [(0, n0)]
    if len(spec) == 2 and not isinstance(spec[0], (tuple, list)):
        return [(int(spec[0]), int(spec[1]))] if spec[1] > spec[0] else []
    return [(int(a), int(b)) for a, b in spec if b > a]


class Arg(object):
    """One array argument: `view` is the array the operation is told about (pointer `ptr`), `full` the same with its pad
    planes (slab buffers), `written` the plane ranges (body coordinates, pads negative / beyond n0) it must fill."""

    def __init__(self, name, role, view, full, lead, written, start=None):
        self.name, self.role, self.view, self.full, self.lead = name, role, view, full, lead
        self.written = written
        self.start = start              # flat index of the body in the pool (None: unguarded)
        self.ranges = []                # (kind, flat begin, flat end) of the frozen regions; ("unwritten", ...) of the must-write ones

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def result(self):
        """The planes the operation must have written, as one flat tensor (what same_bits compares)."""
        plane = _prod(self.view.shape[1:])
        flat = self.full.reshape(-1)
        parts = [flat[(a + self.lead) * plane:(b + self.lead) * plane] for a, b in self.written]
        return torch.cat(parts) if parts else flat[:0]


class _Alloc(object):
    """What a case sees: inp / out / inout / scratch hand out arguments, arm() is called right before the operation."""

    def inp(self, name, data, lead=None, trail=None):
        """An input: `data` (tensor of the array's shape) and, for slab buffers, its pad planes."""
        return self._make(name, "input", tuple(data.shape), data, lead, trail, ())

    def out(self, name, shape, lead=0, trail=0, written=None, free=()):
        """An output; `written`: plane range(s) of the body the call must fill (default all of it); `free`: plane ranges the
        call may write or not (the pads of a slab output that halo copies or redundant stage planes land in); the rest stays."""
        return self._make(name, "output", tuple(shape), None, lead, trail, _planes(written, shape[0]), _planes(free, shape[0]))

    def inout(self, name, data, lead=None, trail=None, written=None, free=()):
        """Read AND written in place; `free`: plane ranges the call may write or not (the pads of a slab state buffer that
        the halo copies fill)."""
        return self._make(name, "inout", tuple(data.shape), data, lead, trail, _planes(written, data.shape[0]),
                          _planes(free, data.shape[0]))

    def scratch(self, name, shape, lead=0, trail=0):
        """Caller scratch: contents unspecified, guards intact.  May be None-d by the case simply by not passing it."""
        n0 = shape[0]
        return self._make(name, "scratch", tuple(shape), None, lead, trail, [], [(-lead, n0 + trail)])


def _pads(x, shape, like):
    """Pad planes given as a tensor, a plane count or None -> (count, tensor or None)."""
    if x is None:
        return 0, None
    if isinstance(x, int):
        return x, None
    assert tuple(x.shape[1:]) == tuple(shape[1:])
    return int(x.shape[0]), x


class PlainAlloc(_Alloc):
    """The reference run: fresh, unguarded arrays; outputs from torch.zeros."""

    def __init__(self, dtype, device):
        self.dtype, self.device = dtype, torch.device(device)
        self.args = []

    def _make(self, name, role, shape, data, lead, trail, written, free=()):
        nl, tl = _pads(lead, shape, data)
        nt, tt = _pads(trail, shape, data)
        full = torch.zeros((nl + shape[0] + nt,) + tuple(shape[1:]), dtype=self.dtype, device=self.device)
        view = full[nl:nl + shape[0]]
        if data is not None:
            view.copy_(data)
        if tl is not None:
            full[:nl].copy_(tl)
        if tt is not None:
            full[nl + shape[0]:].copy_(tt)
        a = Arg(name, role, view, full, nl, written)
        self.args.append(a)
        return a

    def arm(self):
        pass

    def check(self):
        pass

    def results(self):
        return dict((a.name, a.result().clone()) for a in self.args if a.written)


class GuardedPool(_Alloc):
    """One allocation of `capacity` elements, made once and reused by every case of a test module."""

    def __init__(self, dtype, device, capacity):
        self.dtype, self.device = dtype, torch.device(device)
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        slack = ALIGN_BYTES // self.itemsize
        self._store = torch.empty(int(capacity) + slack, dtype=dtype, device=self.device)
        first = (-self._store.data_ptr() % ALIGN_BYTES) // self.itemsize       # element at which the pool is ALIGN_BYTES aligned
        self.flat = self._store[first:first + int(capacity)]
        assert self.flat.data_ptr() % ALIGN_BYTES == 0
        self.bits = self.flat.view(INT_VIEW[dtype])
        self.sentinel = SENTINEL_BITS[dtype]
        self.begin()

    # ---------------------------------------------------------------- one guarded run
    def begin(self, fill=float("nan"), offset_elems=0, depth=1):
        """Start a run: forget the previous arguments; inputs get guards of `fill`, bodies start 512 bytes + offset_elems."""
        self.fill, self.offset_elems, self.depth = float(fill), int(offset_elems), int(depth)
        self.cursor = 0
        self.args = []
        self.frozen = []        # (arg, kind, begin, end, clone of the bits)
        self.armed = False
        return self

    def guard_elems(self, shape):
        return guard_planes(self.depth) * _prod(shape[1:]) + 256

    def carve(self, shape, lead_planes=0, trail_planes=0, offset_elems=None):
        """A contiguous view of `shape` whose first element is 512-byte aligned plus offset_elems elements, preceded by
        lead_planes and followed by trail_planes pad planes, with a guard band outside those.  Also returns the flat ranges
        (guard_lo, lead, body, trail, guard_hi) as (begin, end) pairs."""
        k = self.offset_elems if offset_elems is None else int(offset_elems)
        plane, n = _prod(shape[1:]), _prod(shape)
        g = self.guard_elems(shape)
        per = ALIGN_BYTES // self.itemsize
        body = self.cursor + g + lead_planes * plane
        body = -(-body // per) * per + k
        lead0 = body - lead_planes * plane
        trail1 = body + n + trail_planes * plane
        end = trail1 + g
        if end > self.flat.numel():
            raise MemoryError("GuardedPool of %d elements is too small for this case (needs %d)" % (self.flat.numel(), end))
        lay = dict(guard_lo=(self.cursor, lead0), lead=(lead0, body), body=(body, body + n), trail=(body + n, trail1),
                   guard_hi=(trail1, end))
        self.cursor = end
        return self.flat[body:body + n].view(shape), lay

    def _make(self, name, role, shape, data, lead, trail, written, free=()):
        assert not self.armed, "carve every argument before arm()"
        nl, tl = _pads(lead, shape, data)
        nt, tt = _pads(trail, shape, data)
        view, lay = self.carve(shape, nl, nt)
        plane = _prod(shape[1:])
        lo, hi = lay["guard_lo"][0], lay["guard_hi"][1]
        if role in ("input", "inout"):
            self.flat[lo:hi].fill_(self.fill)
        else:
            self.bits[lo:hi].fill_(self.sentinel)
        full = self.flat[lay["lead"][0]:lay["trail"][1]].view((nl + shape[0] + nt,) + tuple(shape[1:]))
        if data is not None:
            view.copy_(data)
        if tl is not None:
            full[:nl].copy_(tl)
        if tt is not None:
            full[nl + shape[0]:].copy_(tt)
        a = Arg(name, role, view, full, nl, written, lay["body"][0])
        b0 = lay["body"][0]
        a.ranges.append(("guard", lay["guard_lo"][0], lay["guard_lo"][1]))
        a.ranges.append(("guard", lay["guard_hi"][0], lay["guard_hi"][1]))
        # planes of [lead | body | trail] that are neither must-write nor free stay as they are
        loose = sorted(list(written) + list(free))
        at = -nl
        for pa, pb in loose + [(shape[0] + nt, shape[0] + nt)]:
            if pa > at:
                a.ranges.append(("input" if role == "input" else "outside", b0 + at * plane, b0 + pa * plane))
            at = max(at, pb)
        for pa, pb in written:
            a.ranges.append(("unwritten", b0 + pa * plane, b0 + pb * plane))
        self.args.append(a)
        return a

    def arm(self):
        """Right before the operation: remember the bits of everything that must not change."""
        for a in self.args:
            for kind, b, e in a.ranges:
                if kind != "unwritten" and e > b:
                    self.frozen.append((a, kind, b, e, self.bits[b:e].clone()))
        self.armed = True

    def _where(self, a, flat_index):
        plane = _prod(a.view.shape[1:])
        rel = flat_index - a.start
        return "element %d relative to the array's first (axis-0 plane %d, offset %d in the plane; array of %d elements)" % (
            rel, rel // plane, rel % plane, a.view.numel())

    def check(self, case_result=None):
        """(a)-(e) of the module docstring for the run that arm() started.  `case_result` is what the operation returned
        (unused here, passed through so that `pool.check(op(...))` reads naturally)."""
        if not self.armed:
            raise AssertionError("the case never called arm(): nothing was checked")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for a, kind, b, e, was in self.frozen:
            now = self.bits[b:e]
            if not torch.equal(now, was):
                i = int(torch.nonzero(now != was)[0])
                n = int((now != was).sum())
                raise BoundsError(kind, "%s `%s`: %d element(s) of its %s changed, first at %s: %#x -> %#x" % (
                    a.role, a.name, n, {"guard": "guard band", "input": "contents", "outside": "not-updated region"}[kind],
                    self._where(a, b + i), int(was[i]) & (2 ** (8 * self.itemsize) - 1), int(now[i]) & (2 ** (8 * self.itemsize) - 1)))
        for a in self.args:
            for kind, b, e in a.ranges:
                if kind == "unwritten" and a.role == "output":
                    miss = self.bits[b:e] == self.sentinel
                    if bool(miss.any()):
                        i = int(torch.nonzero(miss)[0])
                        raise BoundsError("unwritten", "output `%s`: %d element(s) of the updated region were never written, "
                                          "first at %s" % (a.name, int(miss.sum()), self._where(a, b + i)))
        return case_result

    def results(self):
        return dict((a.name, a.result().clone()) for a in self.args if a.written)


# -------------------------------------------------------------------- bitwise comparison with the reference run
def _bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype]) if t.dtype in INT_VIEW else t


def same_bits(got, ref, what=""):
    """Every array and every host scalar of `got` equals `ref` bit for bit (dicts name -> tensor | float | int | str |
    tuple of those).  NaN equals NaN of the same bits."""
    import struct
    if set(got) != set(ref):
        raise BoundsError("differs", "%s: results %s vs reference %s" % (what, sorted(got), sorted(ref)))
    for k in sorted(ref):
        g, r = got[k], ref[k]
        if torch.is_tensor(r):
            gb, rb = _bits(g), _bits(r)
            if gb.shape != rb.shape or not torch.equal(gb, rb):
                bad = torch.nonzero(gb.reshape(-1) != rb.reshape(-1))
                i = int(bad[0])
                raise BoundsError("differs", "%s: array `%s` differs from the reference run in %d element(s), first at flat %d: "
                                  "%r vs %r" % (what, k, bad.numel(), i, g.reshape(-1)[i].item(), r.reshape(-1)[i].item()))
            continue
        gs = g if isinstance(g, (tuple, list)) else (g,)
        rs = r if isinstance(r, (tuple, list)) else (r,)
        enc = lambda v: struct.pack("<d", v) if isinstance(v, float) else v      # noqa: E731
        if len(gs) != len(rs) or any(enc(a) != enc(b) for a, b in zip(gs, rs)):
            raise BoundsError("differs", "%s: host result `%s` = %r, the reference run gave %r" % (what, k, g, r))


def run_case(op, pool, offsets=OFFSETS, fills=None, depth=1, what="", ref_op=None):
    """The protocol of one table row.  `op(alloc)` carves its arguments from `alloc`, calls alloc.arm(), runs the operation and
    returns a dict of host results.  One reference run on fresh unguarded zeros, then one guarded run per element offset
    and input fill; each must pass check() and equal the reference bit for bit.  Returns the reference's results.
    `ref_op`: the operation of the reference run when it is not `op` itself (the self-test's wrong stand-ins must never run on
    memory without guards)."""
    fills = FILLS if fills is None else fills
    plain = PlainAlloc(pool.dtype, pool.device)
    ref = dict((ref_op or op)(plain))
    if pool.device.type == "cuda":
        torch.cuda.synchronize(pool.device)
    ref_arrays = plain.results()
    for k in offsets:
        for fname, fill in fills.items():
            tag = "%s offset %d fill %s" % (what, k, fname)
            pool.begin(fill, k, depth)
            try:
                got = dict(op(pool))
                pool.check(got)
                same_bits(got, ref, tag)
                same_bits(pool.results(), ref_arrays, tag)
            except BoundsError as e:
                raise BoundsError(e.kind, "%s: %s" % (tag, str(e)))
    return ref, ref_arrays
