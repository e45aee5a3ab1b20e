#!/usr/bin/env python3
"""Register use of the kernels hipRTC builds around registered 5-D / 6-D expressions (levelsetpy_amd/hidim_ham.py), offline.

The translation unit hjh_ham_source returns is compiled by hipcc for gfx950 with the options the run-time compile uses and
-Rpass-analysis=kernel-resource-usage; every substep instantiation (2 types x 3 schemes) and the two bound kernels are
instantiated explicitly.  Needs no GPU.  `make -C levelsetpy_amd/csrc resource-usage-hidim-user` prints the table for the three
systems of tests/hidim_user_cases.py; report() is what tests/test_hidim_user_host.py asserts on.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCHEMES = (0, 1, 3)             # HJ_ENO2, HJ_ENO3, HJ_WENO5_ASSHIPPED
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def report(reg):
    """[{kernel, vgprs, sgprs, scratch (bytes per lane), occupancy (waves per SIMD), lds}] of a HidimRegistration's kernels."""
    src = reg.source()
    for t in ("double", "float"):
        for k in SCHEMES:
            src += "template __global__ void hjh::hidim_substep_kernel<%s, hjh::HamUser<%s>, %d>(const hjh::SubstepArgs<%s, %d>);\n" % (t, t, k, t, reg.dim)
        src += ("template __global__ void hjh::hidim_bound_kernel<%s, hjh::HamUser<%s>>(const hj::GridArgs<%s, %d>, const hjh::HiTables<%s>, "
                "unsigned long long*);\n" % (t, t, t, reg.dim, t))
    csrc = os.path.join(ROOT, "levelsetpy_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hj_user_ham.hip")
        with open(path, "w") as f:
            f.write(src)
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(tmp, "out.o"), path]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if out.returncode != 0:
        raise RuntimeError("hipcc failed on the generated source of '%s':\n%s" % (reg.name, out.stdout[-3000:]))
    rows, cur = [], None
    for line in out.stdout.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = subprocess.check_output(["c++filt", m.group(1)], universal_newlines=True).strip()
            cur = dict(kernel=re.sub(r"^void |\(.*$", "", name))
            rows.append(cur)
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    if len(rows) != 2 * (len(SCHEMES) + 1):
        raise RuntimeError("expected %d kernels in the remarks of '%s', found %d" % (2 * (len(SCHEMES) + 1), reg.name, len(rows)))
    return rows


def test_registrations():
    """The three systems of tests/hidim_user_cases.py."""
    import levelsetpy_amd as L
    import hidim_user_cases as UC
    return [L.register_hidim_hamiltonian("plane5d_tables", 5, UC.PLANE_SRC, nparams=3, aux_axes=UC.PLANE_AXES),
            L.register_hidim_hamiltonian("pair6d_tables", 6, UC.PAIR_SRC, nparams=4, aux_axes=UC.PAIR_AXES),
            L.register_hidim_hamiltonian("planar_quad", 6, UC.QUAD_SRC, nparams=8, aux_axes=UC.QUAD_AXES)]


def main():
    for reg in test_registrations():
        print("%s (%d-D)" % (reg.name, reg.dim))
        for r in report(reg):
            print("  %-70s VGPRs %3d  SGPRs %3d  scratch %3d B/lane  occupancy %d waves/SIMD" % (
                r["kernel"].replace("hjh::", ""), r["vgprs"], r["sgprs"], r["scratch"], r["occupancy"]))


if __name__ == "__main__":
    main()
