"""CPU tier: the resources of the group-sweep kernels for SDE-described models (tgp_sweep_group_sde.hip k_sweep_group_sde<D, XS, POST>) as
the build gives them, from the code-object metadata of the built library.  All 32 instantiations (d = 5 .. 8, XS = 0 .. 3, logpdf / posterior) are
shipped, none uses scratch memory or spills a vector register, a workgroup's LDS is what DESIGN 4.13 states -- N1 and N2 (1024 B), eight exchange
tiles of 82 doubles and, in a posterior call, the groups' blocks of packed filtering states: 16 512 / 20 096 / 15 232 / 17 536 B at d = 5 .. 8 --
within DESIGN 4.10's budget of 20 480 B, the lines are those of profiles/sweep_group_sde_resources.txt, and the plan's waves per CU
(tgp_sweep_plan.hpp group_sde_waves_per_cu) follow the register counts."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")
LDS_LIMIT = 160 * 1024 // 8
LDS_STATED = {5: 16512, 6: 20096, 7: 15232, 8: 17536}

needs_lib = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                               reason="needs the built library and the LLVM binutils")


def lds_expected(d, post):
    ns, B = d + d * (d + 1) // 2, (8 if d <= 6 else 4)
    return 1024 + 8 * (8 * 82 + (8 * B * ns if post else 0))


@pytest.fixture(scope="module")
def seen():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for blob in mod.code_objects(LIB):
        for k in mod.kernels(blob):
            m = re.search(r"tgp_sweep_group::k_sweep_group_sde<(\d), (\d), (true|false)>", k["name"])
            if m:
                out[(int(m.group(1)), int(m.group(2)), m.group(3) == "true")] = k
    return out


@needs_lib
def test_every_instantiation_is_shipped_without_scratch_and_with_the_stated_lds(seen):
    assert sorted(seen) == sorted((d, x, p) for d in (5, 6, 7, 8) for x in range(4) for p in (False, True)), sorted(seen)
    for key, k in sorted(seen.items()):
        print(key, {f: k.get(f) for f in ("vgpr", "scratch", "lds", "vspill", "sspill")})
    assert not [(key, k["scratch"]) for key, k in seen.items() if k["scratch"] != 0], "scratch memory"
    assert not [key for key, k in seen.items() if k["vspill"]], "vector registers spilled"
    for (d, _, post), k in seen.items():
        assert k["lds"] == lds_expected(d, post) <= LDS_LIMIT, (d, post, k["lds"])
        if post:
            assert k["lds"] == LDS_STATED[d]


@needs_lib
def test_the_lines_are_the_recorded_ones(seen):
    rec = {}
    for ln in open(os.path.join(ROOT, "profiles", "sweep_group_sde_resources.txt")):
        m = re.match(r"(logpdf|posterior)\s+(\d)\s+(\d)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", ln)
        if m:
            rec[(int(m.group(2)), int(m.group(3)), m.group(1) == "posterior")] = tuple(int(v) for v in m.groups()[3:])
    assert len(rec) == 32
    assert {key: (k["vgpr"], k["scratch"], k["lds"], k["vspill"], k["sspill"]) for key, k in seen.items()} == rec


@needs_lib
def test_the_plans_waves_per_cu_follow_the_register_counts(seen, tmp_path):
    """8 where every instantiation of (d, call) takes at most 256 registers (two waves per SIMD), else 4"""
    src = tmp_path / "wpc.cpp"
    src.write_text('#include <cstdio>\n#include "%s"\nint main() { for (int d = 5; d <= 8; ++d) for (int p = 0; p < 2; ++p) '
                   'std::printf("%%d %%d %%d\\n", d, p, tgp_sweep::group_sde_waves_per_cu(d, p != 0)); }\n'
                   % os.path.join(ROOT, "temporalgps.jl_amd", "csrc", "tgp_sweep_plan.hpp"))
    exe = str(tmp_path / "wpc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, str(src)])
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        d, p, w = (int(v) for v in ln.split())
        worst = max(k["vgpr"] for (dd, _, post), k in seen.items() if dd == d and post == bool(p))
        assert w == (8 if worst <= 256 else 4), (d, p, w, worst)
