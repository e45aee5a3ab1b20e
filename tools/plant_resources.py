#!/usr/bin/env python3
"""Register use of the kernels hipRTC builds around registered plants (levelsetpy_amd/plant.py), offline.

The translation unit hjp_plant_source returns is compiled by hipcc for gfx950 with the options the run-time compile uses and
-Rpass-analysis=kernel-resource-usage; the six instantiations (2 types x 3 schemes) of user_rollout_kernel and of the three
kernels of extraArgs.plantKernel (user_noisy_rollout_kernel, user_filtered_rollout_kernel, user_decide_points_kernel) are
instantiated explicitly.  Needs no GPU.  `make -C levelsetpy_amd/csrc resource-usage-plant` prints the table for the plants of
tests/plant_cases.py, each re-registered built-in plant next to nothing else: the built-in kernels' own figures come from
`make resource-usage-hiquery` and hipcc on hj_rollout.hip.
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
# kind -> (kernel, its argument block)
KINDS = {"rollout": ("user_rollout_kernel", "RolloutArgs"), "noisy": ("user_noisy_rollout_kernel", "NoisyArgs"),
         "filtered": ("user_filtered_rollout_kernel", "FilterArgs"), "decide": ("user_decide_points_kernel", "FilterArgs")}
ALL_KINDS = ("rollout", "noisy", "filtered", "decide")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def report(reg, kinds=("rollout",), keep=None):
    """[{kernel, vgprs, sgprs, scratch (bytes per lane), occupancy (waves per SIMD), lds}] of a PlantRegistration's kernels of `kinds`.
    keep: a path the device object is copied to (for tools/codeobj_diff.py)."""
    src = reg.source()
    md = 6 if reg.dim > 4 else 4
    kinds = [k for k in kinds if reg.ncontrols > 0 or k in ("rollout", "noisy")]        # nothing to filter without a control
    for kind in kinds:
        for t in ("double", "float"):
            for k in SCHEMES:
                src += "template __global__ void hjp::%s<%s, %d>(hjp::%s<%s, %d>);\n" % (KINDS[kind][0], t, k, KINDS[kind][1], t, md)
    csrc = os.path.join(ROOT, "levelsetpy_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hj_user_plant.hip")
        with open(path, "w") as f:
            f.write(src)
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-DHJ_RTC=1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(tmp, "out.o"), path]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        if keep and out.returncode == 0:
            import shutil
            shutil.copyfile(os.path.join(tmp, "out.o"), keep)
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
    if len(rows) != 2 * len(SCHEMES) * len(kinds):
        raise RuntimeError("expected %d kernels in the remarks of '%s', found %d" % (2 * len(SCHEMES) * len(kinds), reg.name, len(rows)))
    return rows


def test_registrations():
    """The plants of tests/plant_cases.py."""
    import plant_cases as PC
    return [PC.register_builtin(n) for n in sorted(PC.BUILTIN, key=lambda n: PC.BUILTIN[n][0])] + [PC.register_lin(), PC.register_quad()]


def main():
    for reg in test_registrations():
        print("%s (%d-D)" % (reg.name, reg.dim))
        for r in report(reg, ALL_KINDS):
            print("  %-46s VGPRs %3d  SGPRs %3d  scratch %4d B/lane  occupancy %d waves/SIMD" % (
                r["kernel"].replace("hjp::", ""), r["vgprs"], r["sgprs"], r["scratch"], r["occupancy"]))


if __name__ == "__main__":
    main()
