"""CPU-only: the node walk of libhj_hishapes.so, libhj_resample.so and libhj_measure.so (levelsetpy_amd/csrc/hj_index_dev.h), once
for the three of them through their <prefix>_plan and <prefix>_decode.

  * the plan: the launches cover every node exactly once, on grids below and past 2^32 nodes, where one launch (fewer than 2^32
    threads: 2^24 - 1 workgroups) does not hold the grid;
  * the decode: the DEVICE decode function run on the host against np.unravel_index, on the nodes either side of 2^31, 2^32
    and 2^33, on the ends of rows, waves and workgroups and on random nodes -- the precedent of tests/test_large_plans.py: no
    device sees these grids;
  * the plan's two limits lowered through the environment (a test facility): on the small grids of tests/node_walk_cases.py the
    plan takes the head axes, several workgroups per head index and several launches, still covers every node once, and the
    decode is np.unravel_index at EVERY node; unset or set to the constants the plan is unchanged, anything else is refused;
  * the walk is written once: the header holds it and none of the three sources restates it.
What a library adds to the plan (members, output arrays, fields and slots), its named grids and its refusals stay in
tests/test_hishapes_host.py, tests/test_resample_host.py and tests/test_measure_host.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from levelsetpy_amd import _kffi as K, _mffi as M, _vffi as V
import node_walk_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0

LAUNCH_MOST = (2 ** 32 - 1) // 256            # workgroups of 256 threads in one launch: fewer than 2^32 threads
BIG = [(25,) * 6, (41,) * 6, (3, 2 ** 31 - 1), (65535, 65535, 2), (41, 41, 41, 41, 41, 80), (46341, 46341, 2 ** 31 - 1)]
COMMON = [(7, 6, 8, 5, 9), (65535,), (37,), (5, 5, 6, 5, 70)]
PLANE = [(12, 7), (9, 12, 10), (3, 3)]
SHAPES = BIG + COMMON + [(1, 1, 1, 1, 1, 1), (1, 2, 3, 25, 41, 70), (2, 2, 2, 2, 2), (3, 1, 4, 1, 5, 1)]
MEASURE = BIG + COMMON + PLANE + [(2, 2, 2, 2, 2, 2), (2, 2, 3, 25, 41, 70)]     # no axis of one node: its grid check refuses them

# library -> (binding, descriptor of the extents N, the bound <prefix>_decode, random nodes per grid, its grids,
#             what the plan of one member / array / field says of the library's own fields)
LIBS = {
    "hishapes": (K, K.grid_descriptor, lambda: K.lib().hjk_decode, 10000, SHAPES, lambda p, blocks: p.member_launches == 1),
    "resample": (M, M.extents_descriptor, lambda: M.lib().hjm_decode, 4000, SHAPES + PLANE, lambda p, blocks: p.arrays == 1 and p.array_launches == 1),
    "measure": (V, V.extents_descriptor, lambda: V.lib().hjv_decode, 4000, MEASURE,
                lambda p, blocks: p.nfields == 1 and p.field_launches == 1 and p.slots == min(32, 1 << max(0, (blocks - 1).bit_length()))
                and p.slots & (p.slots - 1) == 0),
}
PAIRS = [(name, N) for name in LIBS for N in LIBS[name][4]]
pairs = pytest.mark.parametrize("name,N", PAIRS, ids=["%s-%s" % (name, "x".join(map(str, N))) for name, N in PAIRS])


def nodes_of(N):
    total = 1
    for n in N:
        total *= int(n)
    return total


def crossings(total):
    out = [0, total - 1]
    for b in (2 ** 31, 2 ** 32, 2 ** 33):
        out += [n for n in (b - 2, b - 1, b, b + 1) if 0 <= n < total]
    return out


@pairs
def test_the_plan_covers_every_node_exactly_once(name, N):
    p = LIBS[name][0].plan(N)
    total = nodes_of(N)
    assert p.total == total and p.head * p.tail == total and 1 <= p.tail < 2 ** 31
    # the tail is the LONGEST suffix below 2^31: one more axis would pass it
    assert p.tail == nodes_of(N[p.first_tail:]) and (p.first_tail == 0 or p.tail * N[p.first_tail - 1] >= 2 ** 31)
    # a workgroup owns 256 consecutive tail nodes of one head index: the chunks of a head index cover its tail, the last one partly
    assert (p.chunks - 1) * 256 < p.tail <= p.chunks * 256
    # the launches split the head indices, none of 2^32 threads or more: the runtime takes gridDim.x * blockDim.x modulo 2^32
    assert p.launches >= 1 and (p.launches - 1) * p.heads_per_launch < p.head <= p.launches * p.heads_per_launch
    last_heads = p.head - (p.launches - 1) * p.heads_per_launch
    assert p.blocks_last == last_heads * p.chunks and 1 <= p.blocks_last <= LAUNCH_MOST
    assert (p.launches > 1) == (p.head * p.chunks > LAUNCH_MOST) and (total < 2 ** 32 or p.launches > 1)
    if p.launches > 1:
        assert p.blocks_full == p.heads_per_launch * p.chunks <= LAUNCH_MOST
        assert (p.heads_per_launch + 1) * p.chunks > LAUNCH_MOST           # a full launch is as large as the runtime lets it be
    assert (p.launches - 1) * p.blocks_full + p.blocks_last == p.head * p.chunks
    assert LIBS[name][5](p, p.head * p.chunks)


@pairs
def test_decode_is_unravel_index(name, N):
    _, descriptor, bound, sample, _, _ = LIBS[name]
    total = nodes_of(N)
    rng = np.random.default_rng(total % (2 ** 32))
    nodes = crossings(total) + [int(v) for v in rng.integers(0, total, sample, dtype=np.int64)]
    # the ends of rows, of workgroups and of waves
    nodes += [n for n in (63, 64, 255, 256, N[-1] - 1, N[-1], nodes_of(N[-2:]) - 1, nodes_of(N[-2:])) if 0 <= n < total]
    decode, g, idx = bound(), descriptor(N), (C.c_int32 * 6)()
    want = np.empty((len(nodes), len(N)), dtype=np.int64)
    rest = list(nodes)
    for d in range(len(N) - 1, -1, -1):                   # np.unravel_index in Python integers: 2^62 nodes pass int64 products
        want[:, d] = [int(r) % int(N[d]) for r in rest]
        rest = [int(r) // int(N[d]) for r in rest]
    if total < 2 ** 62:
        assert np.array_equal(want, np.stack(np.unravel_index(np.array(nodes, dtype=np.int64), N), axis=1))
    for n, w in zip(nodes, want):
        assert decode(C.byref(g), n, C.byref(idx)) == OK
        assert tuple(idx[:len(N)]) == tuple(w) and all(v == 0 for v in idx[len(N):]), (N, n)


# ------------------------------------------------------------------------------------------ the plan's limits, lowered
# HJ_INDEX_TAIL_BELOW and HJ_INDEX_LAUNCH_BLOCKS (include/hj_hishapes.h) bring the head axes, the workgroup quotient and the walk
# over several launches to grids small enough that EVERY node is decoded here, before tests/test_gpu_node_walk.py lets a kernel
# rely on the same plans.
LOWERED = [(name, N, form) for name in LIBS for N in W.GRIDS if not (name == "measure" and N == W.ONE_NODE_AXES) for form in W.forms_of(N)]
lowered = pytest.mark.parametrize("name,N,form", LOWERED, ids=["%s-%s-%s" % (name, "x".join(map(str, N)), form) for name, N, form in LOWERED])


@lowered
def test_lowered_limits_the_plan_covers_every_node_exactly_once(name, N, form, monkeypatch):
    W.set_limits(monkeypatch)
    default = LIBS[name][0].plan(N)
    assert default.first_tail == 0 and default.head == 1 and default.launches == 1     # what every device run took so far
    W.set_limits(monkeypatch, N, form)
    p = W.check_form(LIBS[name][0].plan(N), N, form)
    tail_below, launch_blocks = W.limits(N, form)
    # the tail is the longest suffix below the limit that holds the last axis: one more axis would pass it
    assert p.tail < max(tail_below, N[-1] + 1) <= p.tail * N[p.first_tail - 1]
    if launch_blocks is not None:                                 # a full launch is as large as the limit lets it be
        assert p.blocks_full <= launch_blocks < (p.heads_per_launch + 1) * p.chunks
    # the nodes of launch l, workgroup b, thread t as head_launches and the kernels lay them out: each node once, none outside
    seen = np.zeros(p.total, dtype=np.int64)
    for l in range(p.launches):
        blocks = p.blocks_full if l + 1 < p.launches else p.blocks_last
        hl, chunk = np.divmod(np.arange(blocks, dtype=np.int64), p.chunks)
        t = chunk[:, None] * 256 + np.arange(256, dtype=np.int64)[None, :]
        node = l * p.heads_per_launch * p.tail + hl[:, None] * p.tail + t
        np.add.at(seen, node[t < p.tail], 1)
    assert seen.min() == 1 and seen.max() == 1
    assert LIBS[name][5](p, p.head * p.chunks)


@lowered
def test_lowered_limits_decode_is_unravel_index_at_every_node(name, N, form, monkeypatch):
    _, descriptor, bound, _, _, _ = LIBS[name]
    W.set_limits(monkeypatch, N, form)
    total = nodes_of(N)
    want = np.stack(np.unravel_index(np.arange(total), N), axis=1)
    assert (want >= 0).all() and (want < np.array(N)).all()
    decode, g, idx = bound(), descriptor(N), (C.c_int32 * 6)()
    got = np.empty((total, 6), dtype=np.int64)
    for n in range(total):
        assert decode(C.byref(g), n, C.byref(idx)) == OK
        got[n] = idx[:]
    assert np.array_equal(got[:, :len(N)], want) and not got[:, len(N):].any()       # inside every axis, before a kernel relies on it


@pytest.mark.parametrize("name", list(LIBS))
def test_unset_limits_are_the_constants_and_wrong_ones_are_refused_by_name(name, monkeypatch):
    binding = LIBS[name][0]
    N = (6, 5, 7, 5, 6, 8)
    W.set_limits(monkeypatch)
    fields = [f for f, _ in binding.LaunchPlan._fields_]
    default = [getattr(binding.plan(N), f) for f in fields]
    monkeypatch.setenv(W.ENV_TAIL, str(2 ** 31))                  # the constants themselves: the same plan
    monkeypatch.setenv(W.ENV_BLOCKS, str(LAUNCH_MOST))
    assert [getattr(binding.plan(N), f) for f in fields] == default and binding.decode(N, 50399) == (5, 4, 6, 4, 5, 7)
    for env, most in ((W.ENV_TAIL, 2 ** 31), (W.ENV_BLOCKS, LAUNCH_MOST)):
        for bad in ("0", "-3", str(most + 1), "12x", "", "1e3", str(2 ** 70)):
            W.set_limits(monkeypatch)
            monkeypatch.setenv(env, bad)
            for call in (lambda: binding.plan(N), lambda: binding.decode(N, 7)):
                with pytest.raises(Exception, match=env):
                    call()
    # a launch limit below the workgroups of one head index still holds that head index whole
    W.set_limits(monkeypatch)
    monkeypatch.setenv(W.ENV_BLOCKS, "3")
    p = binding.plan(N)
    assert p.chunks == 197 and p.head == 1 and p.heads_per_launch == 1 and p.launches == 1 and p.blocks_last == 197


@pytest.mark.parametrize("name", list(LIBS))
def test_decode_past_the_crossings_exists_in_the_cases(name):
    grids = LIBS[name][4]
    assert (41,) * 6 in grids and (41, 41, 41, 41, 41, 80) in grids and (3, 2 ** 31 - 1) in grids
    assert nodes_of((41,) * 6) > 2 ** 32 and nodes_of((41, 41, 41, 41, 41, 80)) > 2 ** 33 and nodes_of((3, 2 ** 31 - 1)) > 2 ** 32
    assert LIBS[name][0].decode((41,) * 6, 2 ** 32) == tuple(int(v) for v in np.unravel_index(2 ** 32, (41,) * 6))


def test_one_source_for_the_node_walk():
    """The reciprocal, the multiply-high quotient, the carry through the head axes and the plan's arithmetic stand once, in
    hj_index_dev.h: the three libraries' kernels, plans and decodes are frames around them."""
    src = lambda n: open(os.path.join(ROOT, "levelsetpy_amd", "csrc", n)).read()      # noqa: E731
    dev, users = src("hj_index_dev.h"), [src("hj_hishapes.hip"), src("hj_resample.hip"), src("hj_measure.hip")]
    for marker in ("(unsigned long long)v * (unsigned)(r >> 32)", "0xffffffffffffffffull / n", "heads_per_launch = std::min", "X.h0[d] + up",
                   "0x80000000ll", "head % (long long)X.n[d]"):
        assert dev.count(marker) == 1 and not any(marker in u for u in users), marker
    for name in ("quotient", "recip64", "set_head", "split_block", "node_index", "make_plan", "head_launches", "decode"):
        assert len(re.findall(r"^(?:static|__host__ __device__ __forceinline__) [^;=(]*\b%s\(" % name, dev, re.M)) == 1, name
        assert not any(re.search(r"^(?:static|__host__ __device__ __forceinline__) [^;=(]*\b%s\(" % name, u, re.M) for u in users), name
    assert all('#include "hj_index_dev.h"' in u and "switch (" not in u for u in users)
