"""CPU tier: k_sweep_tile_draw<XS> in the built library's code-object metadata: four instantiations, no scratch, no vector spill, at most 256
registers (two waves per SIMD), the adjoint's LDS figure within 160 KiB / 8.  The counts are recorded in profiles/sweep_tile_draw_resources.txt."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")
LDS, LDS_LIMIT = (1 + 8) * 16 * 17 * 8, 160 * 1024 // 8


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_every_draw_instantiation_is_shipped_without_scratch_and_within_its_budgets():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    found = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_sweep_tile::k_sweep_tile_draw<" in k["name"]]
    seen = {int(re.search(r"k_sweep_tile_draw<(\d)>", k["name"]).group(1)): k for k in found}
    assert sorted(seen) == [0, 1, 2, 3], sorted(seen)
    for xs, k in seen.items():
        print(k["name"], {f: k.get(f) for f in ("vgpr", "agpr", "sgpr", "scratch", "lds", "vspill", "sspill")})
        assert k["scratch"] == 0 and not k["vspill"] and k["vgpr"] <= 256 and k["lds"] == LDS <= LDS_LIMIT, (xs, k)
