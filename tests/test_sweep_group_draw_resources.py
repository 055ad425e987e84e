"""CPU tier: the resources of the group sweep's draw kernels (tgp_sweep_group.hip k_sweep_group_draw<D, XS>) as the build gives them, from
the code-object metadata of the built library.  All 16 instantiations (d = 5 .. 8, XS = 0 .. 3) are shipped, none uses scratch memory or spills a vector
register, and a workgroup's LDS is the posterior kernels' (16 000 / 19 584 / 14 720 / 17 024 B at d = 5 .. 8), within DESIGN 4.10's budget: 160 KiB by
eight one-wave workgroups = 20 480 bytes.  The register counts are recorded in profiles/sweep_group_draw_resources.txt (a record, not a threshold: the
plan's waves per CU follow them, tgp_sweep_plan.hpp group_draw_waves_per_cu).  The 32 + 16 kernels the unit had before keep the lines of
profiles/sweep_group_resources.txt and profiles/sweep_group_adjoint_resources.txt: smooth_step shares its factorisation and gain solve with the draw
step, and the refactoring moved no count."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")
LDS_LIMIT = 160 * 1024 // 8
LDS_STATED = {5: 16000, 6: 19584, 7: 14720, 8: 17024}

needs_lib = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                               reason="needs the built library and the LLVM binutils")


def lds_expected(d):
    """A (64 doubles) + eight exchange tiles of 82 doubles + eight groups' blocks of B packed filtering states"""
    ns, B = d + d * (d + 1) // 2, (8 if d <= 6 else 4)
    return 8 * (64 + 8 * 82 + 8 * B * ns)


@pytest.fixture(scope="module")
def unit_kernels():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_sweep_group::k_sweep_group" in k["name"]]


def recorded(name):
    """the table of a resources file: {(kernel, d, XS): (VGPRs, scratch, LDS, VGPR spills, SGPR spills)}"""
    rows = {}
    for ln in open(os.path.join(ROOT, "profiles", name)):
        m = re.match(r"(\w+)\s+(\d)\s+(\d)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", ln)
        if m:
            rows[(m.group(1), int(m.group(2)), int(m.group(3)))] = tuple(int(v) for v in m.groups()[3:])
    return rows


def line_of(k):
    return (k["vgpr"], k["scratch"], k["lds"], k["vspill"], k["sspill"])


@needs_lib
def test_every_draw_instantiation_is_shipped_without_scratch_and_with_the_posterior_kernels_lds(unit_kernels):
    seen = {}
    for k in unit_kernels:
        m = re.search(r"k_sweep_group_draw<(\d), (\d)>", k["name"])
        if m:
            seen[(int(m.group(1)), int(m.group(2)))] = k
    assert sorted(seen) == sorted((d, x) for d in (5, 6, 7, 8) for x in range(4)), sorted(seen)
    for key, k in sorted(seen.items()):
        print(key, {f: k.get(f) for f in ("vgpr", "scratch", "lds", "vspill", "sspill")})
    assert not [(key, k["scratch"]) for key, k in seen.items() if k["scratch"] != 0], "scratch memory"
    assert not [key for key, k in seen.items() if k["vspill"]], "vector registers spilled"
    for (d, _), k in seen.items():
        assert k["lds"] == lds_expected(d) == LDS_STATED[d] <= LDS_LIMIT, (d, k["lds"])
    # the plan's waves per CU follow the register counts: 8 where a wave takes at most 256 registers (two waves per SIMD), else 4
    for d in (5, 6, 7, 8):
        worst = max(k["vgpr"] for (dd, _), k in seen.items() if dd == d)
        assert (worst <= 256) == (d <= 5), (d, worst)
    # the record is the build's
    rec = recorded("sweep_group_draw_resources.txt")
    assert {("draw",) + key: line_of(k) for key, k in seen.items()} == rec


@needs_lib
def test_the_units_other_kernels_keep_their_recorded_lines(unit_kernels):
    got = {}
    for k in unit_kernels:
        m = re.search(r"k_sweep_group<(\d), (\d), (true|false)>", k["name"])
        if m:
            got[("posterior" if m.group(3) == "true" else "logpdf", int(m.group(1)), int(m.group(2)))] = line_of(k)
        m = re.search(r"k_sweep_group_adjoint<(\d), (\d)>", k["name"])
        if m:
            got[("adjoint", int(m.group(1)), int(m.group(2)))] = line_of(k)
    want = {**recorded("sweep_group_resources.txt"), **recorded("sweep_group_adjoint_resources.txt")}
    assert len(want) == 48 and sorted(got) == sorted(want)
    moved = {key: (got[key], want[key]) for key in want if got[key] != want[key]}
    assert not moved, moved
