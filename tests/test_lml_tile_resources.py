"""CPU tier: every k_lml_stream instantiation that a DEFAULT geometry can launch (csrc/tgp_lml.hip choose_geometry: steps per lane and waves per
SIMD by state dimension; a halo longer than a 1024-step tile moves a sixteen-step dimension to thirty-two steps and two waves) uses no scratch and
fits the register budget of its waves per SIMD -- 512 / waves registers per lane.  Built on scripts/list_kernel_resources.py, like
tests/test_kernel_resources.py.

(Why it exists: the thirty-two-step builds of d = 4 and d = 5 carried a private segment of 68 and 36 bytes that no instruction used -- the stack slot of
a 512-bit tuple of scalar loads that the allocator spilled and then rematerialised at every use -- until csrc/tgp_lml.hip ended the coefficients'
live ranges in front of the scan / behind it for those two dimensions and read an odd pointer's pair as one 16-byte copy.)"""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")

# state dimension -> (steps per lane, waves per SIMD): the defaults of choose_geometry
DEFAULT = {1: (16, 4), 2: (32, 2), 3: (32, 2), 4: (32, 2), 5: (32, 2), 6: (32, 2), 7: (32, 2), 8: (32, 2)}


def launchable():
    out = {}
    for d, (n, wps) in DEFAULT.items():
        out[(d, n)] = wps
        out.setdefault((d, 32), 2)      # (the halo rule)
    return out


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_default_geometries_launch_kernels_without_scratch_inside_their_register_budget():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob) if "tgp_lml::k_lml_stream<" in k["name"]]
    want = launchable()
    seen, bad = set(), []
    for k in ks:
        m = re.search(r"k_lml_stream<(\d+), (\d+), (true|false)", k["name"])
        key = (int(m.group(1)), int(m.group(2)))
        if key not in want:
            continue
        seen.add((key, m.group(3)))
        print(f"{k['name']}: vgpr {k['vgpr']} agpr {k['agpr']} scratch {k['scratch']} vgpr_spill {k['vspill']} sgpr_spill {k['sspill']}")
        if k["scratch"] != 0 or k["vspill"] != 0 or k["vgpr"] > 512 // want[key]:
            bad.append((k["name"], k["vgpr"], k["scratch"], k["vspill"]))
    # both pointer alignments of every launchable (d, steps per lane) are in the library
    assert seen == {(key, a) for key in want for a in ("true", "false")}, sorted(seen)
    assert not bad, bad
