"""CPU tier: the dense engine's draw kernels (csrc/tgp_dense_draw.hpp: dk_chunk_draw, dk_fused_draw, DP = 32, 48, 64) hold the MFMA fragments of A, the Q
tiles and a step of prefetched stores in registers while two factorisations sweep LDS: a spill there is a scratch round trip per row of a sweep.  All six
instantiations are in the library, use no scratch, spill no VGPR, and their LDS is the configuration's (FusedDrawCfg<DP>::LDS_BYTES, restated here and
pinned by a static_assert in the header; the manner of tests/test_dense_chunk_resources.py)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def lds_doubles(DP):
    """FusedDrawCfg<DP>::TOTAL: [Pp | T1 | z] | P | delta, m_f, eps | partial sums | H rows | scalars | records"""
    LD, NG = DP + 4, 256 // DP
    return DP * 2 * LD + DP * LD + 3 * DP + NG * DP + 16 * DP + 64 + 16 * (DP + 2)


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(READELF) or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_draw_kernels_use_no_scratch_and_the_configured_lds():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob)]
    watched = {m.group(1) + m.group(2): k for k in ks for m in [re.search(r"tgp_dense::dk_(chunk|fused)_draw<(\d+)>", k["name"])] if m}
    assert sorted(watched) == ["chunk32", "chunk48", "chunk64", "fused32", "fused48", "fused64"], [k["name"] for k in ks if "_draw" in k["name"]]
    bad = [(k["name"], k["scratch"], k["vspill"]) for k in watched.values() if k["scratch"] or k["vspill"]]
    assert not bad, bad
    # the dynamic LDS a launch asks for is the configuration's: the host passes FusedDrawCfg<DP>::LDS_BYTES, which fits one workgroup per CU (160 KiB)
    src = open(os.path.join(ROOT, "temporalgps.jl_amd", "csrc", "tgp_dense.hip")).read()
    for DP in (32, 48, 64):
        assert lds_doubles(DP) * 8 <= 160 * 1024
        for kern in ("dk_chunk_draw", "dk_fused_draw"):
            assert re.search(rf"hipLaunchKernelGGL\({kern}<{DP}>, [^;]*FusedDrawCfg<{DP}>::LDS_BYTES", src), (kern, DP)
    assert lds_doubles(64) * 8 == 125184 and lds_doubles(48) * 8 == 76032 and lds_doubles(32) * 8 == 39424
