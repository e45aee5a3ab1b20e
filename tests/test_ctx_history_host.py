"""The op table and the sequence generator of tests/ctx_history_cases.py, without a device.

  * every entry point of include/hj_mi355x.h that takes an hj_ctx* is issued by an op of the table or is EXCLUDED with a reason: a setter
    added later fails here until the model knows about it;
  * sequence() is deterministic per seed, every step finds its required settings in force and its input arrays written, and the default
    seeds cover every op at least twice and every refused call;
  * every knob set selects the kernel family it claims on its grids (the dry planner)."""
import ctypes as C

import pytest

import ctx_history_cases as H
import instantiation_recipes as IR
from levelsetpy_amd import _ffi


def test_every_ctx_entry_point_is_an_op_or_excluded():
    names = H.header_ctx_entry_points()
    assert len(names) >= 58 and "hj_ctx_set_stream" in names and "hj_rk_substep" in names and "hj_ctx_create" in names
    in_ops = set(c for o in H.OPS for c in o.calls)
    assert in_ops <= set(names), sorted(in_ops - set(names))
    missing = [n for n in names if n not in in_ops and n not in H.EXCLUDED]
    assert not missing, "entry points the history model does not know: %s" % missing
    both = [n for n in H.EXCLUDED if n in in_ops]
    assert not both, both
    assert set(H.EXCLUDED) <= set(names), sorted(set(H.EXCLUDED) - set(names))
    assert all(len(r.split()) >= 3 and "\n" not in r for r in H.EXCLUDED.values())


def test_every_setter_is_a_sticky_setting_of_the_model():
    setters = [n for n in H.header_ctx_entry_points() if n.startswith("hj_ctx_set_")]
    assert len(setters) == 10, setters
    # one setting per setter (the launch-record switch is the eleventh: hj_launch_record)
    assert len(H.INITIAL_SETTINGS) == len(setters) + 1 == len(H.REPLAY_ORDER)
    assert set(H.INITIAL_SETTINGS) == set(H.REPLAY_ORDER)
    assert set(H.SETTERS) | set(H.GROUP_SETTINGS) == set(H.INITIAL_SETTINGS)
    # new coordinates reset the tables: replay writes them in that order
    assert H.REPLAY_ORDER.index("coords") < H.REPLAY_ORDER.index("aux")


def test_op_names_are_unique_and_the_header_refers_to_the_contract():
    names = [o.name for o in H.OPS]
    assert len(set(names)) == len(names)
    assert "tests/ctx_history_cases.py" in open(H.HEADER).read()
    assert H.__doc__.count("sticky") + H.__doc__.count("STICKY") >= 2 and "refused call" in H.__doc__


@pytest.mark.parametrize("case", sorted(H.CASES))
def test_sequences_are_deterministic_and_well_formed(case):
    for seed in H.DEFAULT_SEEDS:
        a, b = H.sequence(seed, case), H.sequence(seed, case)
        assert len(a) == H.DEFAULT_N
        assert [(s.op.name, s.p, s.needs) for s in a] == [(s.op.name, s.p, s.needs) for s in b]
        model = H.Model(H.CASES[case])
        for i, s in enumerate(a):
            assert s.op.applies(H.CASES[case]), (seed, i, s.op.name)
            assert model.satisfied(s.needs), (seed, i, s.op.name, s.needs, model.settings)
            assert set(s.op.reads) <= model.written, (seed, i, s.op.name, s.op.reads, sorted(model.written))
            # the settings the group ops restore themselves are never left changed
            assert all(model.settings[k] == H.INITIAL_SETTINGS[k] for k in H.GROUP_SETTINGS)
            if s.op.name == "read_step_bound":
                assert s.p["slot"] in model.slots, (seed, i)
            slot = s.op.slot(s.p)
            assert slot is None or 0 <= slot < H.USER_SLOTS, (seed, i, s.op.name, slot)
            model.apply(s)
            H.note_slots(model, s, i)
    assert [s.op.name for s in H.sequence(0, case)] != [s.op.name for s in H.sequence(1, case)]


@pytest.mark.parametrize("case", sorted(H.CASES))
def test_the_default_seeds_cover_every_op_twice_and_every_refusal(case):
    count = {}
    for seed in H.DEFAULT_SEEDS:
        for s in H.sequence(seed, case):
            count[s.op.name] = count.get(s.op.name, 0) + 1
    for o in H.applicable(H.CASES[case]):
        assert count.get(o.name, 0) >= 2, (o.name, count)
    assert sum(1 for o in H.OPS if o.refused) == 3
    for o in H.OPS:
        if o.refused:
            assert count.get(o.name, 0) >= 1, o.name
    assert set(count) <= set(o.name for o in H.applicable(H.CASES[case]))


def test_setters_in_front_of_a_step_see_each_other():
    """New coordinates reset the tables: a step that needs base coordinates AND NumPy's tables, drawn while the coordinates are perturbed
    and the tables NumPy's, gets set_coords and then set_aux in front of it.  Many seeds and long sequences, every need in force."""
    hit = 0
    for seed in range(40):
        steps = H.sequence(seed, "dubins64", 150)
        model = H.Model(H.CASES["dubins64"])
        for i, s in enumerate(steps):
            assert model.satisfied(s.needs), (seed, i, s.op.name, s.needs, model.settings)
            if (s.op.name == "set_aux" and i and steps[i - 1].op.name == "set_coords" and i + 1 < len(steps) and steps[i + 1].needs.get("aux") == "numpy"
                    and steps[i + 1].needs.get("coords") == "base"):
                hit += 1
            model.apply(s)
    assert hit >= 1, hit


def test_the_table_covers_what_a_session_mixes():
    names = set(o.name for o in H.OPS)
    for want in ("lf_term", "substep_first", "substep_later", "read_step_bound", "rk_step_post", "rk_stage12", "rk_integrate", "static_step_bound_aba",
                 "max_d1sq", "weno_eps_source", "minmax_with", "any_nan", "upwind", "ghost", "lf_split", "rk_combine", "term_normal", "term_reinit",
                 "term_convection", "term_curvature", "hessian_second", "term_trace_hessian", "set_diss", "set_coords", "set_aux", "slab", "stream",
                 "launch_record", "range_step", "refused_alias", "refused_scheme", "refused_stage12"):
        assert want in names, want
    for ham, psets in H.PSETS.items():
        assert len(psets) >= 2 and psets[0] != psets[1] and len(psets[0]) == {0: 4, 1: 1, 2: 1}[ham]
    assert len(H.RING_PSETS) == 8 and len(set(map(tuple, H.RING_PSETS))) == 8
    assert set(H.SCHEMES) == {0, 1, 2, 3} and set(H.STAGES) == {0, 1, 2, 3, 4}
    assert {c.N for c in H.CASES.values()} == {(14, 12, 16), (24, 19), (9, 8, 10, 12), (8, 8, 8)}
    assert {(c.N, c.dtype) for c in H.CASES.values()} >= {((14, 12, 16), "float64"), ((14, 12, 16), "float32"), ((9, 8, 10, 12), "float32")}


@pytest.mark.parametrize("knobs", sorted(H.KNOBS))
def test_every_knob_set_selects_its_family_on_its_grids(knobs):
    """The dry planner under the knob set: a whole-grid substep (a plane range of a slab for the size rule's tiled fallback) launches the
    family the GPU test asserts in the launch record -- fused12 excepted, which is no substep launch (hj_rk_plan answers on the GPU)."""
    k = H.KNOBS[knobs]
    assert k.cases and set(k.cases) <= set(H.CASES)
    for name in k.cases:
        case = H.CASES[name]
        nd = len(case.N)
        bc = [_ffi.BC_PERIODIC if d in case.periodic else _ffi.BC_EXTRAPOLATE for d in range(nd)]
        seen = set()
        for scheme in H.SCHEMES:
            for stage in (_ffi.STAGE_YDOT, _ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF):
                out, buf = (C.c_int64 * 12)(), C.create_string_buffer(1 << 14)
                with IR.environment(k.env):
                    _ffi.check(_ffi.lib().hj_plan_substep_symbols(nd, (C.c_int64 * nd)(*case.N), (C.c_int * nd)(*bc), _ffi.F64 if case.dtype == "float64" else _ffi.F32,
                                                                  scheme, case.ham, stage, 0, case.N[0], 0, 0, 256, out, buf, len(buf)))
                seen |= set(s for s in buf.value.decode().split("\n") if s)
        if knobs != "fuse12":
            assert any(f in s for f in k.family for s in seen), (knobs, name, sorted(seen))
