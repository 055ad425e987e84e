"""CPU tier: the register budget of the sweep engine's adjoint kernel for SDE-described models (tgp_sweep.hip k_sweep_adjoint_sde<D, XS>) as
the build gives it.  All 16 instantiations (d = 1 .. 4, XS = 0 .. 3) are shipped and none sits at 512 registers with spills (the regime
tests/test_kernel_resources.py guards).  With the blocks of the other passes (8 steps at d = 3, 4 at d = 4) the build put d = 3 and d = 4 at 512 with 50 -
139 spilled registers; with blocks of 4 steps at d = 3 and 2 at d = 4, and a lane's gl / gN2 sums in LDS at d = 4, the widest -- d = 4, XS = 3 -- has 496.
Scratch is 36 bytes per lane at d = 1 (no vector register spilled: the compiler's own stack use) and zero elsewhere; static LDS stays under 40 KiB, four
workgroups per CU as for the other passes."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")
LDS_LIMIT = 40 * 1024      # a CU's 160 KiB by four workgroups


def scratch_allowed(d, xs):
    """bytes per lane, from the build (roc-7.2, -O3)"""
    return 36 if d == 1 else 0


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_every_sde_adjoint_instantiation_is_shipped_within_its_budget():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_sweep::k_sweep_adjoint_sde<" in k["name"]]
    seen = {}
    for k in ks:
        m = re.search(r"k_sweep_adjoint_sde<(\d), (\d)>", k["name"])
        assert m, k["name"]
        seen[(int(m.group(1)), int(m.group(2)))] = k
    assert sorted(seen) == [(d, x) for d in (1, 2, 3, 4) for x in range(4)], sorted(seen)
    print({key: {f: k.get(f) for f in ("vgpr", "scratch", "lds", "vspill", "sspill")} for key, k in sorted(seen.items())})
    risky = [k["name"] for k in ks if k["vgpr"] >= 512 and (k["vspill"] or k["sspill"])]
    assert not risky, f"k_sweep_adjoint_sde instantiations at 512 registers with spills: {risky}"
    assert not [k["name"] for k in ks if k["vspill"]], "vector registers spilled"
    over = [(k["name"], k["vgpr"], k["scratch"]) for key, k in seen.items() if k["scratch"] > scratch_allowed(*key)]
    assert not over, over
    assert max(k["lds"] for k in ks) <= LDS_LIMIT, [(k["name"], k["lds"]) for k in ks]
