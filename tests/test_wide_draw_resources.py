"""CPU tier: the posterior draw kernel of the wide-state engine (csrc/tgp_wide.hip k_wide_post_rand<32>, <64>) holds the lane's rows of G and U' -- 2 DP
doubles -- in registers through an unrolled step: a spill there is a scratch round trip per multiply-add.  Both instantiations are in the library and use no
scratch (the style of tests/test_kernel_resources.py)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_posterior_draw_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for blob in mod.code_objects(LIB) for k in mod.kernels(blob)]
    watched = {m.group(1): k for k in ks for m in [re.search(r"tgp_wide::.*k_wide_post_rand<(\d+)>", k["name"])] if m}
    assert sorted(watched) == ["32", "64"], [k["name"] for k in ks if "k_wide_post" in k["name"]]
    bad = [(k["name"], k["scratch"], k["vspill"], k["sspill"]) for k in watched.values() if k["scratch"] or k["vspill"]]
    assert not bad, bad
