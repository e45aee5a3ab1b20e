#!/usr/bin/env python3
"""Which kernel instantiations of libhj_mi355x.so does a run launch, and which does the suite compare with a reference?

    python tools/kernel_coverage.py RECORD [levelsetpy_amd/csrc/libhj_mi355x.so] [-v]

RECORD is either
  * a launch record: mangled kernel symbols, one per line -- what hj_launch_record_read returns, and what
    tests/test_gpu_instantiations.py appends to the file named by HJ_INSTANTIATION_REPORT for every row that passed
    (HJ_INSTANTIATION_REPORT=compared.txt python -m pytest tests/test_gpu_instantiations.py); or
  * a "calls<TAB>kernel name" table from a rocprofv3 --kernel-trace --stats run (demangled names).
Per kernel family it prints: instantiations built, with a recipe, excluded, and in RECORD; an instantiation without a recipe is named.
The list of instantiations and their recipes is the test suite's (tests/instantiation_recipes.py: the tool reports on that table, so it
needs the test tree beside it).  -v lists the instantiations that are not in RECORD."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import instantiation_recipes as IR  # noqa: E402


def norm(s):
    """demangled kernel or stub name -> 'family<args>' without namespace, blanks and parameter list"""
    s = re.sub(r'^void ', '', s.strip()).replace('hj::__device_stub__', '').replace('hj::', '')
    i = s.find('<')
    if i < 0:
        return s.split('(')[0]
    depth = 0
    for k in range(i, len(s)):
        depth += s[k] == '<'
        if s[k] == '>':
            depth -= 1
            if depth == 0:
                return s[:k + 1].replace(' ', '')
    return s.replace(' ', '')


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    if not args:
        sys.exit(__doc__)
    lib = args[1] if len(args) > 1 else os.path.join(ROOT, "levelsetpy_amd", "csrc", "libhj_mi355x.so")
    insts = IR.instantiations(lib)
    by_symbol = {i.symbol: i for i in insts}
    by_name = {norm(i.demangled): i for i in insts}
    seen, other = set(), 0
    for ln in open(args[0]):
        ln = ln.rstrip('\n')
        if not ln:
            continue
        if '\t' in ln:
            inst = by_name.get(norm(ln.split('\t', 1)[1]))
        else:
            inst = by_symbol.get(ln.strip())
        if inst is None:
            other += 1
        else:
            seen.add(inst.symbol)
    with_recipe, no_recipe = set(), []
    for i in insts:
        if i.symbol in IR.EXCLUDED:
            continue
        try:
            IR.recipe_for(i)
            with_recipe.add(i.symbol)
        except IR.NoRecipe as e:
            no_recipe.append(str(e))
    fams = collections.OrderedDict()
    for i in insts:
        f = fams.setdefault(i.family, [0, 0, 0, 0])
        f[0] += 1
        f[1] += i.symbol in with_recipe
        f[2] += i.symbol in IR.EXCLUDED
        f[3] += i.symbol in seen
    print("%-26s %6s %12s %9s %10s" % ("family", "built", "with recipe", "excluded", "in record"))
    for name, f in sorted(fams.items(), key=lambda kv: (-kv[1][0], kv[0])):
        print("%-26s %6d %12d %9d %10d" % ((name,) + tuple(f)))
    tot = [sum(f[k] for f in fams.values()) for k in range(4)]
    print("%-26s %6d %12d %9d %10d" % (("total",) + tuple(tot)))
    for msg in no_recipe:
        print("NO RECIPE:", msg)
    if other:
        print("(%d record lines name no instantiation of this library: run-time kernels, other libraries)" % other)
    if "-v" in sys.argv:
        for i in insts:
            if i.symbol not in seen:
                print("not in record:", i.demangled)


if __name__ == "__main__":
    main()
