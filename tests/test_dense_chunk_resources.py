"""CPU tier: the dense engine's chunk kernels (csrc/tgp_dense_chunked.hpp: dk_chunk_filter, dk_chunk_smooth, DP = 32, 48, 64) keep the covariance tiles and
the MFMA fragments of A in registers through the step, as the sequential kernels they share their bodies with: a spill there is a scratch round trip per
product.  All six instantiations are in the library and use no scratch and spill no VGPR (the style of tests/test_wide_draw_resources.py)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_chunk_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob)]
    watched = {m.group(1) + m.group(2): k for k in ks for m in [re.search(r"tgp_dense::dk_chunk_(filter|smooth)<(\d+)>", k["name"])] if m}
    assert sorted(watched) == ["filter32", "filter48", "filter64", "smooth32", "smooth48", "smooth64"], [k["name"] for k in ks if "dk_chunk" in k["name"]]
    bad = [(k["name"], k["scratch"], k["vspill"]) for k in watched.values() if k["scratch"] or k["vspill"]]
    assert not bad, bad
