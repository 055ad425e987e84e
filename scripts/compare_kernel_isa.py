#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two sets of gfx950 device assembly (hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S):
registers, scratch (private_segment_fixed_size), instructions in the kernel's body and whether the count per mnemonic is the same.
Kernels are matched by their demangled name without namespaces, so a kernel that moved to another unit or namespace is still paired.
usage: compare_kernel_isa.py --before a.s [b.s ...] --after c.s [d.s ...] [--filter REGEX] [--diff]      prints a markdown table
(--diff: the mnemonics whose counts differ, per kernel)"""
import collections
import re
import subprocess
import sys


def parse(path):
    """{mangled name: dict(vgpr, scratch, hist)} of one .s file"""
    out, cur, body = {}, None, None
    meta = {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and cur is None:
            cur, body = m.group(1), collections.Counter()
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[cur] = dict(hist=body)
                cur = None
                continue
            s = line.split(";")[0].strip()
            if not s or s.startswith(".") or s.endswith(":"):
                continue
            body[s.split()[0]] += 1
            continue
        m = re.match(r"\s*\.name:\s+(_Z\w+)", line)
        if m:
            meta["name"] = m.group(1)
        for key in ("vgpr_count", "private_segment_fixed_size"):
            m = re.match(rf"\s*-?\s*\.{key}:\s+(\d+)", line)
            if m:
                meta[key] = int(m.group(1))
        if re.match(r"\s*\.wavefront_size:", line) and "name" in meta:      # (the last key of a kernel's metadata block)
            if meta["name"] in out:
                out[meta["name"]].update(vgpr=meta.get("vgpr_count"), scratch=meta.get("private_segment_fixed_size"))
            meta = {}
    return {k: v for k, v in out.items() if "vgpr" in v}


def demangle(names):
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, dem):
        d = d.replace("(anonymous namespace)::", "").split("(")[0]
        d = re.sub(r"^void ", "", d)
        short[n] = re.sub(r"\b\w+::", "", d)
    return short


def load(paths):
    ks = {}
    for p in paths:
        ks.update(parse(p))
    short = demangle(list(ks))
    return {short[n]: v for n, v in ks.items()}


if __name__ == "__main__":
    a = sys.argv[1:]
    flt = re.compile(a[a.index("--filter") + 1]) if "--filter" in a else None
    show = "--diff" in a
    stop = [i for i, x in enumerate(a) if x.startswith("--")]
    grab = lambda flag: a[a.index(flag) + 1:min(i for i in stop + [len(a)] if i > a.index(flag))]
    before, after = load(grab("--before")), load(grab("--after"))
    print("| kernel | vgpr before | vgpr after | scratch before/after | instructions before | instructions after | same histogram |")
    print("|---|---|---|---|---|---|---|")
    differ = 0
    for name in sorted(set(before) | set(after)):
        if flt and not flt.search(name):
            continue
        b, n = before.get(name), after.get(name)
        if b is None or n is None:
            print(f"| `{name}` | {'-' if b is None else b['vgpr']} | {'-' if n is None else n['vgpr']} | only {'after' if b is None else 'before'} | | | |")
            continue
        same = b["hist"] == n["hist"]
        differ += not same
        print(f"| `{name}` | {b['vgpr']} | {n['vgpr']} | {b['scratch']} / {n['scratch']} | {sum(b['hist'].values())} | {sum(n['hist'].values())} | {'yes' if same else 'NO'} |")
        if show and not same:
            d = {k: n["hist"][k] - b["hist"][k] for k in set(b["hist"]) | set(n["hist"]) if n["hist"][k] != b["hist"][k]}
            print("|  | " + ", ".join(f"{k} {v:+d}" for k, v in sorted(d.items())) + " | | | | | |")
    print(f"\nkernels that differ: {differ}")
