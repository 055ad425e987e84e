"""CPU tier: the resources of the group sweep's adjoint kernels (tgp_sweep_group.hip k_sweep_group_adjoint<D, XS>) as the build gives them,
from the code-object metadata of the built library.  All 16 instantiations (d = 5 .. 8, XS = 0 .. 3) are shipped, none uses scratch memory or spills a
vector register, and a workgroup's LDS stays within DESIGN 4.10's budget: 160 KiB by eight one-wave workgroups = 20 480 bytes.  The register counts are
recorded in profiles/sweep_group_adjoint_resources.txt (a record, not a threshold: the plan's waves per CU follow them, tgp_sweep_plan.hpp
group_adjoint_waves_per_cu)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")
LDS_LIMIT = 160 * 1024 // 8


def lds_expected(d):
    """A (64 doubles) + eight exchange tiles of 82 doubles + eight groups' blocks of B packed states (the states in FRONT of a block's steps)"""
    ns, B = d + d * (d + 1) // 2, (8 if d <= 6 else 4)
    return 8 * (64 + 8 * 82 + 8 * B * ns)


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_every_adjoint_instantiation_is_shipped_without_scratch_and_within_the_lds_budget():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_sweep_group::k_sweep_group_adjoint<" in k["name"]]
    seen = {}
    for k in ks:
        m = re.search(r"k_sweep_group_adjoint<(\d), (\d)>", k["name"])
        assert m, k["name"]
        seen[(int(m.group(1)), int(m.group(2)))] = k
    assert sorted(seen) == sorted((d, x) for d in (5, 6, 7, 8) for x in range(4)), sorted(seen)
    for key, k in sorted(seen.items()):
        print(key, {f: k.get(f) for f in ("vgpr", "scratch", "lds", "vspill", "sspill")})
    assert not [(key, k["scratch"]) for key, k in seen.items() if k["scratch"] != 0], "scratch memory"
    assert not [key for key, k in seen.items() if k["vspill"]], "vector registers spilled"
    for (d, _), k in seen.items():
        assert k["lds"] == lds_expected(d) <= LDS_LIMIT, (d, k["lds"])
    # the plan's waves per CU follow the register counts: 8 where a wave takes at most 256 registers (two waves per SIMD), else 4
    for d in (5, 6, 7, 8):
        worst = max(k["vgpr"] for (dd, _), k in seen.items() if dd == d)
        assert (worst <= 256) == (d <= 6), (d, worst)
