"""CPU tier: the register budget of the sweep engine's adjoint kernel (tgp_sweep.hip k_sweep_adjoint<D, XS>) as the build gives it.
All 16 instantiations (d = 1 .. 4, XS = 0 .. 3; LTI form) are shipped: none sits at 512 registers with spills (the regime tests/test_kernel_resources.py
guards), the widest -- d = 4, XS = 3 -- at 450 with the 36 sums of a lane's block gradients in registers.  Scratch is zero except 68 bytes per lane at
d = 3, XS = 3 (the bytes k_sweep<3, lti, ...> and k_sweep_draw<3, lti, ...> have from the code the three share)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")


def scratch_allowed(d, xs):
    """bytes per lane, from the build (roc-7.2, -O3)"""
    return 68 if (d, xs) == (3, 3) else 0


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_every_adjoint_instantiation_is_shipped_within_its_budget():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_sweep::k_sweep_adjoint<" in k["name"]]
    seen = {}
    for k in ks:
        m = re.search(r"k_sweep_adjoint<(\d), (\d)>", k["name"])
        assert m, k["name"]
        seen[(int(m.group(1)), int(m.group(2)))] = k
    assert sorted(seen) == [(d, x) for d in (1, 2, 3, 4) for x in range(4)], sorted(seen)
    risky = [k["name"] for k in ks if k["vgpr"] >= 512 and (k["vspill"] or k["sspill"])]
    assert not risky, f"k_sweep_adjoint instantiations at 512 registers with spills: {risky}"
    over = [(k["name"], k["vgpr"], k["scratch"]) for key, k in seen.items() if k["scratch"] > scratch_allowed(*key)]
    assert not over, over
