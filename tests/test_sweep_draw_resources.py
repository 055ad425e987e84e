"""CPU tier: the register budget of the sweep engine's draw kernel (tgp_sweep.hip k_sweep_draw<D, SDE, XS>) as the build gives it.
All 32 instantiations (d = 1 .. 4, LTI / SDE, XS = 0 .. 3) are shipped: none sits at 512 registers with spills (the regime tests/test_kernel_resources.py
guards), the widest -- d = 3, SDE, XS = 3 -- at 498.  Scratch is zero except where k_sweep<..., posterior> has the same bytes from the code the two share:
36 bytes per lane at d = 1 SDE, 68 at d = 3 LTI and at d = 4 LTI with XS = 3."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")


def scratch_allowed(d, sde, xs):
    """bytes per lane, from the build (roc-7.2, -O3)"""
    if d == 1 and sde:
        return 36
    if (d == 3 and not sde) or (d == 4 and not sde and xs == 3):
        return 68
    return 0


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_every_draw_instantiation_is_shipped_within_its_budget():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_sweep::k_sweep_draw<" in k["name"]]
    seen = {}
    for k in ks:
        m = re.search(r"k_sweep_draw<(\d), (true|false), (\d)>", k["name"])
        assert m, k["name"]
        seen[(int(m.group(1)), m.group(2) == "true", int(m.group(3)))] = k
    assert sorted(seen) == [(d, s, x) for d in (1, 2, 3, 4) for s in (False, True) for x in range(4)], sorted(seen)
    risky = [k["name"] for k in ks if k["vgpr"] >= 512 and (k["vspill"] or k["sspill"])]
    assert not risky, f"k_sweep_draw instantiations at 512 registers with spills: {risky}"
    over = [(k["name"], k["vgpr"], k["scratch"]) for key, k in seen.items() if k["scratch"] > scratch_allowed(*key)]
    assert not over, over
