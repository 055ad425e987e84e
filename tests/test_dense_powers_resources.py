"""CPU tier: the register and scratch budget of the dense-power one-launch kernels (csrc/tgp_powers.hip: k_rand_one, k_filter_one, k_adjoint_one,
k_smooth_one<D, 8, MINW, RAND>) as the build gives it.  Exactly 42 instantiations are shipped.  The kernels read their coefficients in place from
the kernel-argument segment; a shared block that indexed an argument table with a run-time index, or was not inlined, would send a copy of the
arguments to scratch -- so no instantiation may use more scratch than it did when every kernel carried its own copy of the scan blocks (the
build of commit 592ea6f, roc-7.2, -O3: the values below), and none may leave its register class (<= 128 where it was, else <= 256)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "temporalgps.jl_amd", "libtgp_hip.so")

# kernel<template arguments> -> (vgpr, scratch bytes per lane) of the build before the blocks were shared
BEFORE = {}
for d, v in zip(range(1, 9), (46, 68, 95, 125, 154, 186, 214, 244)):
    BEFORE[f"k_rand_one<{d}, 8>"] = (v, 0)
for d, v, s in zip(range(1, 9), (54, 92, 112, 132, 224, 228, 220, 232), (0, 0, 0, 0, 0, 132, 132, 388)):
    BEFORE[f"k_filter_one<{d}, 8>"] = (v, s)
for d, v, s in zip(range(1, 7), (61, 85, 117, 156, 199, 248), (0, 0, 0, 0, 80, 0)):
    BEFORE[f"k_adjoint_one<{d}, 8>"] = (v, s)
for d, v, s in zip(range(1, 7), (72, 80, 80, 90, 112, 128), (0, 0, 0, 0, 0, 64)):
    BEFORE[f"k_smooth_one<{d}, 8, 4, false>"] = (v, s)
for d, v in zip(range(1, 9), (86, 82, 90, 90, 112, 138, 168, 204)):
    BEFORE[f"k_smooth_one<{d}, 8, 2, false>"] = (v, 0)
for d, v in zip(range(1, 7), (94, 91, 107, 126, 144, 162)):
    BEFORE[f"k_smooth_one<{d}, 8, 2, true>"] = (v, 0)


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the built library and the LLVM binutils")
def test_every_dense_power_instantiation_is_shipped_within_its_budget():
    assert len(BEFORE) == 42
    spec = importlib.util.spec_from_file_location("list_kernel_resources", os.path.join(ROOT, "scripts", "list_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}
    for blob in mod.code_objects(LIB):
        for k in mod.kernels(blob):
            m = re.search(r"\btgp_\w+::(k_(?:rand|filter|adjoint|smooth)_one<[^>]*>)$", k["name"])
            if m:
                assert m.group(1) not in seen, f"{m.group(1)} is shipped twice"
                assert "tgp_powers::" in k["name"], k["name"]
                seen[m.group(1)] = k
    assert sorted(seen) == sorted(BEFORE), sorted(set(seen) ^ set(BEFORE))
    more_scratch = [(n, k["scratch"], BEFORE[n][1]) for n, k in seen.items() if k["scratch"] > BEFORE[n][1]]
    assert not more_scratch, f"(kernel, scratch bytes, allowed): {more_scratch}"
    out_of_class = [(n, k["vgpr"], BEFORE[n][0]) for n, k in seen.items() if k["vgpr"] > (128 if BEFORE[n][0] <= 128 else 256)]
    assert not out_of_class, f"(kernel, vgpr, before): {out_of_class}"
