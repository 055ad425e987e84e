#!/usr/bin/env python3
"""Writes what the build of THIS tree computes on the dense-power one-launch kernels (csrc/tgp_powers.hip) to an .npz, for a bytewise
comparison of two builds: every class of tests/_dense_powers_edges.py at three lengths -- nhs + C + 1, nhs + 2 C + halo + 1 and the first
length = 3 (mod 8) beyond nhs + 8 C (C, halo: the filter's) -- and per length logpdf, posterior marginals (shared and per-step new noise),
_filter, the evaluated posterior, the prior draw, the posterior draw (d <= 6) and tgp_logpdf_adjoint's gradient, on the seeded inputs of
tests/test_gpu_dense_powers_edges.py.  The kernels that served each call are stored beside its arrays.
usage: dump_dense_powers.py out.npz            (one build)
       dump_dense_powers.py --compare a.npz b.npz      -> a table classes x operations: `same` or the number of arrays that differ"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("logpdf", "marginals", "filter", "posterior", "rand_prior", "rand_post", "adjoint")


def dump(path):
    sys.path.insert(0, ROOT)
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lgssm as L
    from tests import _dense_powers_edges as E
    from tests import _util as U
    from tests import test_gpu_dense_powers_edges as G
    lib = tgp._lib
    out = {}

    def keep(key, fn, dm):
        try:
            res, names = U.kernels_of(tgp, dm, fn)
        except Exception as e:      # (an operation a class does not have: both builds must say the same)
            res, names = {"error": np.frombuffer(type(e).__name__.encode(), dtype=np.uint8)}, set()
        for k, v in res.items():
            out[f"{key}/{k}"] = np.ascontiguousarray(G._np(v))
        out[f"{key}/kernels"] = np.frombuffer(",".join(sorted(names)).encode(), dtype=np.uint8)

    for name in E.CLASSES:
        case = G.case_of(name)
        g = case.geo
        nhs, C, halo = g["nhs"], g["C_filter"], g["halo_f"]
        t3 = nhs + 8 * C + 1
        for T in (nhs + C + 1, nhs + 2 * C + halo + 1, t3 + (3 - t3) % 8):
            key = f"{name}/{T}"
            dms, ys = U.device_model(tgp, case.smodel(T)), case.sy(T)
            keep(key + "/logpdf", lambda: dict(lp=np.array(L.logpdf(dms, ys))), dms)
            for tag, Rn in (("shared", case.Rn0), ("per_step", case.Rn[:T])):
                keep(f"{key}/marginals_{tag}", lambda: dict(zip(("lp", "mean", "var"), L.logpdf_and_posterior_marginals(dms, ys, Rn))), dms)
            dm, y = U.device_model(tgp, case.lti(T)), np.ascontiguousarray(case.y_lti[:T])

            def filt():
                hd = dm.handle()
                gm, gP, lml = np.empty((T, case.d)), np.empty((T, case.d, case.d)), ctypes.c_double()
                hd.check(hd.lib.tgp_filter(hd.h, lib.ptr(y), None, 0, lib.ptr(gm), lib.ptr(gP), ctypes.byref(lml)))
                return dict(m=gm, P=gP, lp=np.array(lml.value))

            def post():
                p = L.posterior(dm, y).materialise()
                return dict(G=p.transitions.As, g=p.transitions.as_, L=p.transitions.Qs, x0m=p.x0.m, x0P=p.x0.P)

            def adjoint():
                lp, gr = L.logpdf_adjoint(dm, y)
                return dict(lp=np.array(lp), **{k: np.asarray(v, dtype=np.float64) for k, v in gr.items()})

            keep(key + "/filter", filt, dm)
            keep(key + "/posterior", post, dm)
            keep(key + "/rand_prior", lambda: dict(y=L.rand((case.eps[0][:T], case.eps[1][:T], case.eps[2]), dm)), dm)
            if case.d <= 6:
                deps = (case.deps[0][:T], case.deps[1][:T], case.deps[2])
                for tag, Rn in (("shared", case.Rn0), ("per_step", case.Rn[:T])):
                    keep(f"{key}/rand_post_{tag}", lambda: dict(y=L.rand(deps, L.replace_observation_noise_cov(L.posterior(dm, y), Rn))), dm)
            keep(key + "/adjoint", adjoint, dm)
        print(f"{name}: done", flush=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    bad, served = {}, {}
    for k in a.files:
        name, _, op = k.split("/")[:3]
        op = next(o for o in OPS if op.startswith(o))
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        bad[(name, op)] = bad.get((name, op), 0) + (not same)
        if k.endswith("/error"):
            served.setdefault((name, op), set()).add("raised " + a[k].tobytes().decode())
        if k.endswith("/kernels"):
            served.setdefault((name, op), set()).update(x for x in a[k].tobytes().decode().split(",") if x.startswith(("k_smooth_one", "k_filter_one", "k_rand_one", "k_adjoint_one")))      # (the kernels of this family among those that served)
    names = sorted({n for n, _ in bad})
    print("| class | " + " | ".join(OPS) + " |")
    print("|---|" + "---|" * len(OPS))
    for n in names:
        cells = []
        for o in OPS:
            if (n, o) not in bad:
                cells.append("-")
            else:
                by = "/".join(sorted(served.get((n, o), ()))) or "other kernels"
                cells.append(("same" if bad[(n, o)] == 0 else f"{bad[(n, o)]} DIFFER") + f" ({by})")
        print(f"| {n} | " + " | ".join(cells) + " |")
    total = sum(bad.values())
    print(f"\n{len(a.files)} arrays compared bytewise; {total} differ")
    return 1 if total else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
