"""The recipe table of tests/instantiation_recipes.py, checked without a GPU: every kernel instantiation the library ships has
exactly one recipe (or a justified exclusion), and every substep recipe, run through the dry planner, selects exactly the
instantiation it claims -- on a plan with several ragged tiles and chunks, the smallest shape at which tile seams, shifted last
tiles and chunk warm-up can go wrong."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instantiation_recipes as IR  # noqa: E402

MAX_EXCLUDED = 15
ALLOWED_REASON = "no entry point and no knob can select it"


def _recipes():
    return IR.recipes() if os.path.exists(IR._ffi.LIB_PATH) else []


PLANNED = [r for r in _recipes() if r.planned]


def test_every_instantiation_has_exactly_one_recipe_or_is_excluded():
    insts = IR.instantiations()
    assert len(insts) >= 700 and len(set(i.symbol for i in insts)) == len(insts)
    symbols = set(i.symbol for i in insts)
    assert len(IR.EXCLUDED) <= MAX_EXCLUDED
    for sym, reason in IR.EXCLUDED.items():
        assert sym in symbols, "excluded instantiation is not in the library (drop it from the list): %s" % sym
        assert reason == ALLOWED_REASON, (sym, reason)
    missing = []
    for i in insts:
        if i.symbol in IR.EXCLUDED:
            continue
        try:
            r = IR.recipe_for(i)
        except IR.NoRecipe as e:
            missing.append(str(e))
            continue
        assert r.symbol == i.symbol and r.call in ("substep", "term", "curv", "coop", "stage12", "helper")
    assert not missing, "no recipe:\n" + "\n".join(missing)
    count = collections.Counter(r.symbol for r in IR.recipes())
    assert set(count) == symbols - set(IR.EXCLUDED) and max(count.values()) == 1


def test_kernel_symbol_is_the_stub_without_its_prefix():
    for i in IR.instantiations()[::37]:
        assert IR.STUB in i.stub and IR.STUB not in i.symbol and i.family in i.symbol
        assert len(i.stub) - len(i.symbol) == len(IR.STUB) + (len(str(len(i.family) + len(IR.STUB))) - len(str(len(i.family))))


def test_every_substep_family_is_planned():
    fams = collections.Counter(r.family for r in PLANNED)
    for fam in ("fused_substep_kernel", "fused_pair_kernel", "fused_pair4_kernel", "fused_flat4_kernel", "direct_substep_kernel"):
        assert fams[fam] > 0, fam
    assert any("HamDubinsRelX" in r.inst.demangled for r in PLANNED)
    # every instantiation of those families is planned, but for the term operators (reached through hj_term_*, not hj_rk_substep)
    for r in IR.recipes():
        if r.family in fams and not r.planned:
            assert "TermOp" in r.inst.demangled, r.describe()


def test_recipes_set_every_knob_they_depend_on():
    for r in IR.recipes():
        assert set(r.env) == set(IR.BASE_ENV), r.describe()
        assert r.env["HJ_DIRECT_BELOW"] is not None


def test_grids_are_small_and_mix_boundary_kinds():
    for r in IR.recipes():
        cells = 1
        for n in r.N:
            cells *= n
        assert cells <= 60000, r.describe()
        nd = len(r.N)
        all_periodic = r.family in ("fused_pair4_kernel", "fused_flat4_kernel") and r.inst.targs[-2] == "false"
        if all_periodic:
            assert len(r.periodic) == nd, r.describe()
        elif nd >= 2:
            assert 0 < len(r.periodic) < nd, r.describe()


@pytest.mark.parametrize("r", PLANNED, ids=[r.id for r in PLANNED])
def test_substep_recipe_plans_exactly_its_instantiation(r):
    p = IR.plan(r)
    assert p.symbols == (r.symbol,), "planned %r\n%s" % (p.symbols, r.describe())
    if not r.tiled:
        assert p.ntiles == 0
        return
    nd = len(r.N)
    # extents of the plan are in the kernel's axis order: the marched axis first, then the tiled axes in grid order
    marched = r.extra.get("marched_axis", 0)
    axes = [d for d in range(nd) if d != marched]
    assert p.nchunks >= 2 and p.chunk >= 2 and r.N[marched] % p.chunk != 0, (p, r.describe())
    ntiles = 1
    for k, d in enumerate(axes):
        e = p.E[k]
        if d in r.tiled_axes:
            assert 0 < e < r.N[d] and r.N[d] % e != 0, "axis %d: tile %d of %d cells\n%s" % (d, e, r.N[d], r.describe())
        else:
            assert e == r.N[d], (d, e, r.describe())
        ntiles *= -(-r.N[d] // e)
    assert p.ntiles == ntiles and p.nblocks >= p.ntiles * p.nchunks, (p, r.describe())
