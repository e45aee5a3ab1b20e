"""The guarded-buffer harness (tests/guarded_pool.py) checked against itself, on CPU tensors: NumPy stand-ins for an
"operation" that receives raw pointers, as the C ABI does.  One stand-in is correct; each of the others is wrong in one
way, and the matching check must report it.  This proves that the checks tests/test_gpu_memory_bounds.py relies on
can fail.  Nothing here touches a GPU, and every access of every stand-in lies inside the pool."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from guarded_pool import (ALIGN_BYTES, FILLS, SENTINEL_BITS, BoundsError, GuardedPool, PlainAlloc, guard_planes,  # noqa: E402
                          run_case, same_bits)

SHAPE = (7, 5, 6)
NP_T = {torch.float64: np.float64, torch.float32: np.float32}
CT_T = {torch.float64: C.c_double, torch.float32: C.c_float}
REACH = 40      # how far around its pointers a stand-in may look: well inside a guard (4 planes * 30 + 256 elements)


def window(ptr, n, tdtype):
    """NumPy array over [ptr - REACH, ptr + n + REACH) elements, and the index of the pointer's element in it."""
    item = np.dtype(NP_T[tdtype]).itemsize
    buf = (CT_T[tdtype] * (n + 2 * REACH)).from_address(ptr - REACH * item)
    return np.ctypeslib.as_array(buf), REACH


def standin(bug=None):
    """out[p0:p1] = 2 * x[p0:p1] + 1 plane by plane, and max(x) as a host scalar -- through raw pointers."""
    def op_ptr(x_ptr, out_ptr, shape, p0, p1, tdtype):
        n, plane = int(np.prod(shape)), int(np.prod(shape[1:]))
        xw, xo = window(x_ptr, n, tdtype)
        ow, oo = window(out_ptr, n, tdtype)
        x = xw[xo:xo + n].reshape(shape)
        out = ow[oo:oo + n].reshape(shape)
        if bug == "skips_last_row":
            out[p0:p1, :-1] = 2 * x[p0:p1, :-1] + 1
        else:
            out[p0:p1] = 2 * x[p0:p1] + 1
        m = float(np.max(x))
        if bug == "past_end":
            ow[oo + n] = 1.0
        elif bug == "before_start":
            ow[oo - 1] = 1.0
        elif bug == "plane_outside":
            ow[oo + p1 * plane:oo + (p1 + 1) * plane] = 3.0
        elif bug == "modifies_input":
            x[2, 1, 3] += 1.0
        elif bug == "reads_guard":
            m = float(np.fmax(m, xw[xo + n]))        # one element past the input joins the max reduction
        elif bug == "writes_input_guard":
            xw[xo - 2] = 0.0
        return m
    return op_ptr


def case(fn, tdtype, p0=0, p1=SHAPE[0], lead=0, trail=0):
    data = torch.from_numpy(np.random.default_rng(4).standard_normal(SHAPE).astype(NP_T[tdtype]))

    def op(A):
        x = A.inp("x", data)
        out = A.out("out", SHAPE, lead=lead, trail=trail, written=(p0, p1))
        A.arm()
        m = fn(x.view.data_ptr(), out.view.data_ptr(), SHAPE, p0, p1, tdtype)
        return {"max": m}
    return op


@pytest.fixture(scope="module", params=[torch.float64, torch.float32], ids=["fp64", "fp32"])
def pool(request):
    return GuardedPool(request.param, "cpu", 1 << 14)


def test_correct_standin_passes_every_offset_and_fill(pool):
    ref, arrays = run_case(case(standin(), pool.dtype), pool)
    assert np.isfinite(ref["max"]) and arrays["out"].numel() == int(np.prod(SHAPE))
    run_case(case(standin(), pool.dtype, 2, 5), pool)                  # a proper sub-range of planes
    run_case(case(standin(), pool.dtype, 0, SHAPE[0], 3, 3), pool)     # slab pads around the output stay sentinel


@pytest.mark.parametrize("bug,kind", [("past_end", "guard"), ("before_start", "guard"), ("skips_last_row", "unwritten"),
                                      ("plane_outside", "outside"), ("modifies_input", "input"), ("reads_guard", "differs"),
                                      ("writes_input_guard", "guard")])
def test_each_wrong_standin_trips_its_check(pool, bug, kind):
    with pytest.raises(BoundsError) as e:
        run_case(case(standin(bug), pool.dtype, 1, 5), pool, ref_op=case(standin(), pool.dtype, 1, 5))
    assert e.value.kind == kind, str(e.value)


def test_stray_write_into_a_slab_pad_of_the_output_is_seen(pool):
    """Whole-grid range, so plane p1 is the first trail PAD of the output, not a guard."""
    with pytest.raises(BoundsError) as e:
        run_case(case(standin("plane_outside"), pool.dtype, 0, SHAPE[0], 3, 3), pool, ref_op=case(standin(), pool.dtype, 0, SHAPE[0], 3, 3))
    assert e.value.kind == "outside"


def test_nan_fill_alone_hides_a_stray_read_in_a_max_and_the_finite_fills_do_not(pool):
    op, good = case(standin("reads_guard"), pool.dtype), case(standin(), pool.dtype)
    run_case(op, pool, fills={"nan": FILLS["nan"]}, ref_op=good)             # fmax(NaN, x) = x: the defect passes
    with pytest.raises(BoundsError) as e:
        run_case(op, pool, fills={"+1e30": 1e30}, ref_op=good)
    assert e.value.kind == "differs"
    # a MIN reduction that strays is the mirror image: -1e30 shows it
    def op_min(stray):
        def op(A):
            x = A.inp("x", torch.zeros(SHAPE, dtype=pool.dtype))
            A.arm()
            w, o = window(x.view.data_ptr(), x.view.numel(), pool.dtype)
            m = w[o:o + x.view.numel()].min()
            return {"min": float(np.fmin(m, w[o - 1]) if stray else m)}
        return op
    run_case(op_min(True), pool, fills={"+1e30": 1e30}, ref_op=op_min(False))
    with pytest.raises(BoundsError):
        run_case(op_min(True), pool, fills={"-1e30": -1e30}, ref_op=op_min(False))


def test_a_skipped_cell_is_seen_even_when_the_stale_value_would_be_right(pool):
    """Defect 2 of the issue: with torch.empty outputs a skipped cell usually still holds the previous call's (correct)
    value.  Here the pool is first filled by a correct run; the sentinel fill of the next run still exposes the skip."""
    run_case(case(standin(), pool.dtype), pool, offsets=(0,), fills={"nan": FILLS["nan"]})
    with pytest.raises(BoundsError) as e:
        run_case(case(standin("skips_last_row"), pool.dtype), pool, offsets=(0,), fills={"nan": FILLS["nan"]},
                 ref_op=case(standin(), pool.dtype))
    assert e.value.kind == "unwritten"


def test_layout_alignment_and_guard_width(pool):
    item = pool.itemsize
    for depth in (1, 2, 3):
        for k in (0, 1, 2, 3):
            pool.begin(1e30, k, depth)
            v, lay = pool.carve(SHAPE, 3 * depth, 3 * depth)
            assert v.is_contiguous() and tuple(v.shape) == SHAPE
            assert v.data_ptr() % ALIGN_BYTES == k * item
            want = guard_planes(depth) * 30 + 256
            assert guard_planes(depth) == max(4, 3 * depth + 1)
            assert lay["guard_lo"][1] - lay["guard_lo"][0] >= want and lay["guard_hi"][1] - lay["guard_hi"][0] == want
            assert lay["lead"][1] - lay["lead"][0] == 3 * depth * 30 == lay["trail"][1] - lay["trail"][0]
            assert lay["guard_lo"][0] >= 0 and lay["guard_hi"][1] <= pool.flat.numel()
            v2, lay2 = pool.carve((41,))
            assert lay2["guard_lo"][0] == lay["guard_hi"][1] and v2.data_ptr() % ALIGN_BYTES == k * item
    with pytest.raises(MemoryError):
        pool.begin().carve((1 << 14,))


def test_sentinel_is_compared_as_bits_and_a_computed_nan_is_not_the_sentinel(pool):
    pool.begin()
    o = pool.out("o", (4, 3))
    assert bool((o.view != o.view).all())                               # the sentinel is a NaN ...
    assert int(pool.bits[o.start]) == SENTINEL_BITS[pool.dtype]         # ... with a fixed payload
    pool.arm()
    o.view.fill_(float("nan"))                                          # an operation that legitimately writes NaN everywhere
    pool.check()
    pool.begin()
    o = pool.out("o", (4, 3))
    pool.arm()
    o.view[:3].fill_(0.0)
    with pytest.raises(BoundsError) as e:
        pool.check()
    assert e.value.kind == "unwritten" and "plane 3" in str(e.value)


def test_check_without_arm_and_scratch_and_inout(pool):
    pool.begin()
    pool.out("o", (4, 3))
    with pytest.raises(AssertionError):
        pool.check()
    # scratch: contents free, guards not
    pool.begin()
    s = pool.scratch("work", (4, 3), 1, 1)
    pool.arm()
    s.full.fill_(7.0)
    pool.check()
    pool.begin()
    s = pool.scratch("work", (4, 3))
    pool.arm()
    pool.flat[s.start + 12] = 7.0
    with pytest.raises(BoundsError) as e:
        pool.check()
    assert e.value.kind == "guard"
    # inout with pads the call may fill (a slab state buffer) and pads it may not
    d = torch.ones((4, 3), dtype=pool.dtype)
    pad = torch.zeros((2, 3), dtype=pool.dtype)
    pool.begin()
    b = pool.inout("state", d, pad, pad, written=(), free=[(-2, 0), (4, 6)])
    pool.arm()
    b.full[:2] = 5.0
    pool.check()
    pool.begin()
    b = pool.inout("state", d, pad, pad, written=(), free=[(-2, 0)])
    pool.arm()
    b.full[-1] = 5.0
    with pytest.raises(BoundsError) as e:
        pool.check()
    assert e.value.kind == "outside"


def test_same_bits_distinguishes_what_float_comparison_would_not():
    a = torch.tensor([0.0, float("nan")], dtype=torch.float64)
    same_bits({"x": a, "s": float("nan"), "k": "kernel", "t": (1.0, 2)}, {"x": a.clone(), "s": float("nan"), "k": "kernel", "t": (1.0, 2)})
    with pytest.raises(BoundsError):
        same_bits({"x": torch.tensor([-0.0, float("nan")], dtype=torch.float64)}, {"x": a})
    with pytest.raises(BoundsError):
        same_bits({"s": -0.0}, {"s": 0.0})
    with pytest.raises(BoundsError):
        same_bits({"k": "a"}, {"k": "b"})
    p = PlainAlloc(torch.float32, "cpu")
    o = p.out("o", (3, 2), lead=1, trail=1, written=(1, 3))
    assert o.full.shape == (5, 2) and o.result().numel() == 4 and float(o.full.abs().sum()) == 0.0


def test_output_with_free_pads_must_still_be_written(pool):
    """A slab output whose pads the call may fill: the pads are unconstrained, a skipped cell of the body is still seen."""
    pool.begin()
    o = pool.out("y_out", (4, 3), 2, 2, free=[(-2, 0), (4, 6)])
    pool.arm()
    o.full.fill_(1.0)
    pool.check()
    pool.begin()
    o = pool.out("y_out", (4, 3), 2, 2, free=[(-2, 0), (4, 6)])
    pool.arm()
    o.full[:5].fill_(1.0)           # lead pads and three body planes: the last body plane is skipped
    with pytest.raises(BoundsError) as e:
        pool.check()
    assert e.value.kind == "unwritten"
    pool.begin()
    o = pool.out("y_out", (4, 3), 2, 2, free=[(-2, 0)])
    pool.arm()
    o.full.fill_(1.0)               # the trail pads are not free here
    with pytest.raises(BoundsError) as e:
        pool.check()
    assert e.value.kind == "outside"
