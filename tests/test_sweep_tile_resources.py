"""CPU tier: the resources of k_sweep_tile<XS, POST> (tgp_sweep_tile.hip) from the code-object metadata of the built library.  All 8 instantiations
are shipped (d is a run-time argument), none uses scratch or spills a vector register, at most 256 registers, and a workgroup's LDS is the one padded 16 x 17
transpose tile DESIGN 4.16 states, within 160 KiB / 8 = 20 480 bytes.  The counts are recorded in profiles/sweep_tile_resources.txt."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")
LDS, LDS_LIMIT = 16 * 17 * 8, 160 * 1024 // 8


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_every_tile_sweep_instantiation_is_shipped_without_scratch_and_within_its_budgets():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}
    for k in (k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_sweep_tile::k_sweep_tile<" in k["name"]):
        m = re.search(r"k_sweep_tile<(\d), (true|false)>", k["name"])
        assert m, k["name"]
        seen[(int(m.group(1)), m.group(2) == "true")] = k
        print(m.groups(), {f: k.get(f) for f in ("vgpr", "agpr", "sgpr", "scratch", "lds", "vspill", "sspill")})
    assert sorted(seen) == sorted((x, p) for x in range(4) for p in (False, True)), sorted(seen)
    for key, k in seen.items():
        assert k["scratch"] == 0 and not k["vspill"] and k["vgpr"] <= 256, (key, k)
        assert k["lds"] == LDS <= LDS_LIMIT, (key, k["lds"])
