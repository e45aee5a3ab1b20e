"""CPU: what the library plans for arrays past 2 GiB, 4 GiB and 2^31 cells (dist.plan_substep = hj_plan_substep: the launch code run without
a device).  tests/test_gpu_large_arrays.py runs these very launches on a GPU and asserts the same kernels and chunkings there.

The invariant every tiled launch must keep: one buffer descriptor spans a chunk of the march plus 3 planes either side, and the kernels form
byte offsets within it as 32-bit unsigned numbers (hj_fused.h), so  (chunk_planes + 6) * plane_bytes < 2^32.  The transposed launch (march
along axis 1) steps by rows, and its descriptors also reach over all axis-0 planes:  (N0 - 1) * plane_bytes + (chunk + 6) * row_bytes < 2^32."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from levelsetpy_amd import _ffi, dist  # noqa: E402

GiB = float(1 << 30)
XP_NAME = "fused_pair_kernel (march along axis 1)"
SCHEMES = ["ENO2", "ENO3", "WENO5", "WENO5_ASSHIPPED"]
STAGES = [_ffi.STAGE_YDOT, _ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF, _ffi.STAGE_RK3_FULL]
DUBINS, DINT, PEND = _ffi.HAM_DUBINS_REL, _ffi.HAM_DOUBLE_INTEGRATOR, _ffi.HAM_DOUBLE_PENDULUM
LIGHT = ("ENO2", "WENO5_ASSHIPPED")         # the schemes of the pair kernel's light configuration; ENO3 and the intended WENO5 plan alike

# (shape, dtype, system, bc, environment) -> {scheme class: (kernel, chunks, planes per chunk, tile or None)}; "light" / "heavy" as above
TABLE = [
    ((1030, 512, 512), "f64", DUBINS, [0, 0, 1], {},
     {"light": ("fused_pair_kernel", 2, 515, [32, 64]), "heavy": ("fused_pair_kernel", 1, 1030, [16, 32])}),
    ((1030, 512, 512), "f64", DUBINS, [0, 0, 1], {"HJ_TARGET_BLOCKS": "1"},
     {"light": ("fused_pair_kernel", 1, 1030, [32, 64]), "heavy": ("fused_pair_kernel", 1, 1030, [16, 32])}),
    ((2056, 512, 512), "f64", DUBINS, [0, 0, 1], {},
     {"light": ("fused_pair_kernel", 2, 1028, [32, 64]), "heavy": ("fused_pair_kernel", 2, 1028, [16, 32])}),
    ((2056, 512, 512), "f64", DUBINS, [0, 0, 1], {"HJ_TARGET_BLOCKS": "1"},
     {"light": ("fused_pair_kernel", 2, 2041, [32, 64]), "heavy": ("fused_pair_kernel", 2, 2041, [16, 32])}),
    ((8200, 512, 512), "f32", DUBINS, [0, 0, 1], {},
     {"light": ("fused_pair_kernel", 4, 2050, [32, 64]), "heavy": ("fused_pair_kernel", 3, 2734, [16, 32])}),
    ((8200, 512, 512), "f32", DUBINS, [0, 0, 1], {"HJ_TARGET_BLOCKS": "1"},
     {"light": ("fused_pair_kernel", 3, 4089, [32, 64]), "heavy": ("fused_pair_kernel", 3, 4089, [16, 32])}),
    ((40, 7400, 7400), "f32", DUBINS, [0, 0, 1], {},
     {"light": ("fused_pair_kernel", 4, 10, [17, 120]), "heavy": ("direct_substep_kernel", 1, 0, [])}),
    ((40, 7400, 7400), "f32", DUBINS, [0, 0, 1], {"HJ_TARGET_BLOCKS": "1"},
     {"light": ("fused_pair_kernel", 4, 13, [17, 120]), "heavy": ("direct_substep_kernel", 1, 0, [])}),
    ((1001, 129, 129, 129), "f32", PEND, [1, 1, 1, 1], {},
     {"light": ("fused_pair_kernel", 4, 251, [5, 6, 34]), "heavy": ("fused_substep_kernel", 3, 334, [5, 6, 33])}),
    ((1001, 129, 129, 129), "f32", PEND, [1, 1, 1, 1], {"HJ_TARGET_BLOCKS": "1"},
     {"light": ("fused_pair_kernel", 3, 494, [5, 6, 34]), "heavy": ("fused_substep_kernel", 3, 494, [5, 6, 33])}),
    ((520, 129, 129, 129), "f32", PEND, [1, 1, 1, 1], {},
     {"light": ("fused_flat4_kernel", 5, 104, [3, 5, 129]), "heavy": ("fused_substep_kernel", 2, 260, [5, 6, 33])}),
    ((32768, 16400), "f64", DINT, [0, 0], {},
     {"light": ("fused_pair_kernel", 85, 386, [2048]), "heavy": ("fused_pair_kernel", 31, 1058, [512])}),
    ((32768, 16400), "f64", DINT, [0, 0], {"HJ_TARGET_BLOCKS": "1"},
     {"light": ("fused_pair_kernel", 2, 32730, [2048]), "heavy": ("fused_pair_kernel", 2, 32730, [512])}),
    ((24, 3400, 3400), "f64", DUBINS, [0, 0, 1], {},
     {"light": (XP_NAME, 6, 567, [24, 84]), "heavy": (XP_NAME, 22, 155, [8, 64])}),
    ((24, 3400, 3400), "f64", DUBINS, [0, 0, 1], {"HJ_XP": "2"},
     {"light": (XP_NAME, 6, 567, [24, 84]), "heavy": (XP_NAME, 22, 155, [8, 64])}),
    ((24, 3400, 3400), "f64", DUBINS, [0, 0, 1], {"HJ_XP": "0"},
     {"light": ("fused_pair_kernel", None, None, None), "heavy": ("fused_pair_kernel", None, None, None)}),
    ((24, 4800, 4800), "f64", DUBINS, [0, 0, 1], {"HJ_XP": "2"},       # the cap refuses the transposed span
     {"light": ("fused_pair_kernel", 2, 12, [26, 78]), "heavy": ("fused_pair_kernel", 2, 12, [6, 78])}),
    ((24, 9500, 9500), "f32", DUBINS, [0, 0, 1], {"HJ_XP": "2"},       # 2^31 cells refuse it
     {"light": ("fused_pair_kernel", 5, 5, [13, 156]), "heavy": ("direct_substep_kernel", 1, 0, [])}),
]
KNOBS = ("HJ_TARGET_BLOCKS", "HJ_XP", "HJ_XP_TRIALS", "HJ_FORCE_DIRECT", "HJ_MIN_CHUNK", "HJ_AUTOTUNE")


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def span_bytes(N, dtype, plan):
    """Bytes one buffer descriptor of the planned launch spans; None for a launch without descriptors (the direct kernel)."""
    esz = 8 if dtype == "f64" else 4
    if not plan["kernel"].startswith("fused_"):
        return None
    plane = int(np.prod(N[1:], dtype=np.int64)) * esz
    if plan["kernel"] == XP_NAME:
        return (N[0] - 1) * plane + (plan["chunk_planes"] + 6) * N[2] * esz
    return (plan["chunk_planes"] + 6) * plane


def check_invariants(N, dtype, plan):
    span = span_bytes(N, dtype, plan)
    if span is None:
        return
    assert span < (1 << 32), (N, dtype, plan, span)
    marched = N[1] if plan["kernel"] == XP_NAME else N[0]
    assert plan["chunks"] * plan["chunk_planes"] >= marched, (N, dtype, plan)
    assert (plan["chunks"] - 1) * plan["chunk_planes"] < marched, (N, dtype, plan)           # no empty chunk


@pytest.mark.parametrize("row", range(len(TABLE)), ids=["%s-%s-%s" % ("x".join(map(str, r[0])), r[1], "+".join(
    "%s=%s" % kv for kv in sorted(r[4].items())) or "default") for r in TABLE])
def test_plans_of_the_large_shapes(row, monkeypatch):
    N, dtype, ham, bc, env, want = TABLE[row]
    set_env(monkeypatch, env)
    for scheme in SCHEMES:
        kern, chunks, chunk, tile = want["light" if scheme in LIGHT else "heavy"]
        for stage in STAGES:
            p = dist.plan_substep(N, bc, dtype, _ffi.SCHEME_IDS[scheme], ham, stage, 0, N[0])
            assert p["kernel"] == kern, (scheme, stage, p)
            if chunks is not None:
                assert (p["chunks"], p["chunk_planes"], p["tile"]) == (chunks, chunk, tile), (scheme, stage, p)
            check_invariants(N, dtype, p)


def test_the_spans_the_table_was_chosen_for(monkeypatch):
    """Each shape sits where it does for a reason: pin the reason."""
    set_env(monkeypatch, {"HJ_TARGET_BLOCKS": "1"})
    p = dist.plan_substep((1030, 512, 512), [0, 0, 1], "f64", _ffi.ENO2, DUBINS, _ffi.STAGE_EULER, 0, 1030)
    assert (1 << 31) < span_bytes((1030, 512, 512), "f64", p) < (1 << 32)                     # one descriptor past 2^31 bytes
    p = dist.plan_substep((32768, 16400), [0, 0], "f64", _ffi.ENO2, DINT, _ffi.STAGE_EULER, 0, 32768)
    assert span_bytes((32768, 16400), "f64", p) == 4294963200 == (1 << 32) - 4096              # 4095 B under the limit
    for N, dt in (((2056, 512, 512), "f64"), ((8200, 512, 512), "f32"), ((1001, 129, 129, 129), "f32")):
        p = dist.plan_substep(N, [0, 0, 1] if len(N) == 3 else [1] * 4, dt, _ffi.ENO2, DUBINS if len(N) == 3 else PEND, _ffi.STAGE_EULER, 0, N[0])
        esz = 8 if dt == "f64" else 4
        plane = int(np.prod(N[1:])) * esz
        assert p["chunks"] > 1 and span_bytes(N, dt, p) + plane >= (1 << 32), (N, p)           # the cap binds: one more plane would not fit
    assert 8200 * 512 * 512 >= (1 << 31) > 8191 * 512 * 512 and 1001 * 129 ** 3 >= (1 << 31) and 24 * 9500 * 9500 >= (1 << 31)
    assert 520 * 129 ** 3 < (1 << 31) and 520 * 129 ** 3 * 4 > (1 << 32)


def _random_shape(rng):
    while True:
        nd = int(rng.integers(2, 5))
        dtype = "f32" if rng.random() < 0.5 else "f64"
        esz = 4 if dtype == "f32" else 8
        nbytes = GiB * 2.0 ** rng.uniform(0, 6)
        if nd == 2:
            rest = [int(rng.integers(64, 60000))]
        elif nd == 3:
            rest = [int(2 ** rng.uniform(4, 13)) for _ in range(2)]
        else:
            rest = [int(2 ** rng.uniform(3, 8.6)) for _ in range(3)]
        plane = int(np.prod(rest, dtype=np.int64))
        n0 = int(round(nbytes / esz / plane))
        if n0 < 8 or plane >= (1 << 31) or not GiB <= n0 * plane * esz <= 64 * GiB:
            continue
        bc = [int(rng.random() < 0.4) for _ in range(nd)]
        return [n0] + rest, dtype, {2: DINT, 3: DUBINS, 4: PEND}[nd], bc


@pytest.mark.parametrize("tb1", [False, True], ids=["default", "TB1"])
def test_random_large_shapes_keep_the_span_below_4GiB(tb1, monkeypatch):
    set_env(monkeypatch, {"HJ_TARGET_BLOCKS": "1"} if tb1 else {})
    rng = np.random.default_rng(20241)
    kernels = {}
    for k in range(200):
        N, dtype, ham, bc = _random_shape(rng)
        scheme = SCHEMES[k % 4]
        stage = STAGES[(k // 4) % 4]
        p = dist.plan_substep(N, bc, dtype, _ffi.SCHEME_IDS[scheme], ham, stage, 0, N[0])    # raises on any planner error
        check_invariants(N, dtype, p)
        kernels[p["kernel"]] = kernels.get(p["kernel"], 0) + 1
    assert kernels.get("fused_pair_kernel", 0) > 50, kernels
