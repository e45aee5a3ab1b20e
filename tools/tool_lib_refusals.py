#!/usr/bin/env python3
"""The argument checks of nine stateless libraries (tests/tool_lib_cases.py), for comparing two builds of them.  No GPU.

    tools/tool_lib_refusals.py dump [--libdir DIR]   one line per call: return code, whole error text, last-kernel record.
                                                     DIR holds the libhj_*.so to load (default: levelsetpy_amd/csrc); the dumps
                                                     of two builds are compared with cmp
    tools/tool_lib_refusals.py cxx LIB               the same calls of one library (query, surface, ttr, rollout, batch, hiquery,
                                                     plant, shapes, hishapes) as a C++ program with a main(); compiled with hj_LIB.hip and
                                                     -Xarch_host -fsanitize=address,undefined it prints the lines of `dump`
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["dump", "cxx"])
    ap.add_argument("lib", nargs="?")
    ap.add_argument("--libdir")
    a = ap.parse_args()
    if a.libdir:            # before the bindings are imported: they read the variables once
        for name in ("query", "surface", "ttr", "rollout", "batch", "hiquery", "plant", "shapes", "hishapes"):
            os.environ["HJ_%s_LIB" % name.upper()] = os.path.join(os.path.abspath(a.libdir), "libhj_%s.so" % name)
    import tool_lib_cases as T
    if a.what == "cxx":
        sys.stdout.write(T.cxx_program(a.lib))
        return
    mods = T.modules()
    for case in T.CASES:
        if a.lib in (None, case[0]):
            print(T.line(case, *T.run(case, mods)))


if __name__ == "__main__":
    main()
