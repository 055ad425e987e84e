#!/usr/bin/env python3
"""Times the calls the dense-power one-launch kernels serve (csrc/tgp_powers.hip), device-resident inputs, T = 1e7, for an A/B of two builds:
  Matern-5/2, d = 3:                      prior draw (k_rand_one), _filter and the evaluated posterior (k_filter_one), tgp_logpdf_adjoint (k_adjoint_one)
  Matern-5/2 + Matern-5/2, one scale, d = 6: logpdf, posterior marginals and the posterior draw (k_smooth_one<logpdf | posterior | rand>)
(the calls of scripts/r04_time_rand.py, r04_time_filter.py, r04_time_posterior.py, r04_adjoint_phases.py).  One process = one line of JSON per
figure: the median per call on the host clock between two device synchronisations, and the handle's hipEvent figure of the kernel.
usage: time_dense_powers.py LABEL            (imports the package of the tree this file lies in; appends to stdout)
       time_dense_powers.py --table FILE...  (the processes' outputs -> the table: parent's range, result's median, verdict)"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 10_000_000


def run(label):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import _lib
    from temporalgps_jl_amd import lgssm as L

    def timed(what, model, fn, kernel, n, warm=3):
        hd = model.handle()
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        hd.set_option(_lib.OPT_PROFILE, 1)
        hd.profile_reset()
        for _ in range(5):
            fn()
        hd.set_option(_lib.OPT_PROFILE, 0)
        prof = {k: v["total_ms"] / v["calls"] for k, v in hd.profile().items()}
        print(json.dumps(dict(label=label, what=what, ms=statistics.median(ts) * 1e3)), flush=True)
        assert kernel in prof, (what, sorted(prof))      # (served by the kernel this script is about)
        print(json.dumps(dict(label=label, what=f"{what} event: {kernel}", ms=prof[kernel])), flush=True)

    gen = torch.Generator(device="cuda:0").manual_seed(5)
    randn = lambda *s: torch.randn(s, dtype=torch.float64, device="cuda:0", generator=gen)      # noqa: E731
    m3 = bench.build_model(tgp, "matern52_d3", T, "lti", 0)
    eps = (randn(T, 3), randn(T), np.random.default_rng(0).standard_normal(3))
    y = tgp.rand(eps, m3)      # (a series of the model itself)
    timed("d3_rand_prior", m3, lambda: tgp.rand(eps, m3), "k_rand_one", 20)
    del eps
    timed("d3_filter", m3, lambda: tgp._filter(m3, y), "k_filter_one", 12)
    timed("d3_posterior", m3, lambda: tgp.posterior(m3, y).materialise(), "k_filter_one", 12)
    hd = m3.handle()
    g = [np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3)), np.zeros(3), np.zeros(1), np.zeros(1), np.zeros(3), np.zeros((3, 3))]
    lml = ctypes.c_double()
    args = (hd.h, _lib.ptr(y), _lib.IN_DEVICE, ctypes.byref(lml), *[_lib.ptr(x) for x in g])
    timed("d3_adjoint", m3, lambda: hd.check(hd.lib.tgp_logpdf_adjoint(*args)), "k_adjoint_one", 30)
    del m3, hd
    m6 = bench.build_model(tgp, "sum52_52_d6", T, "lti", 0)
    eps = (randn(T, 6), randn(T), np.random.default_rng(1).standard_normal(6))
    y = tgp.rand(eps, m6)
    Rn = torch.tensor([0.05], dtype=torch.float64, device="cuda:0")
    timed("d6_logpdf", m6, lambda: L.logpdf(m6, y), "k_smooth_one<logpdf>", 30)
    timed("d6_marginals", m6, lambda: L.logpdf_and_posterior_marginals(m6, y, Rn), "k_smooth_one<posterior>", 20)
    timed("d6_rand_post", m6, lambda: L.rand(eps, L.replace_observation_noise_cov(L.posterior(m6, y), Rn)), "k_smooth_one<rand>", 12)


def table(paths):
    rows = {}
    for p in paths:
        for line in open(p):
            if line.startswith("{"):
                r = json.loads(line)
                rows.setdefault(r["what"], {}).setdefault(r["label"].split("#")[0], []).append(r["ms"])
    for what, by in rows.items():
        pa, re_ = by["parent"], by["result"]
        lo, hi, med = min(pa), max(pa), statistics.median(re_)
        verdict = "below (faster)" if med < lo else "inside" if med <= hi else "ABOVE (slower)"
        print(f"{what:44s} parent " + " ".join(f"{v:8.4f}" for v in pa) + f"  [{lo:.4f}, {hi:.4f}] spread {100 * (hi - lo) / statistics.median(pa):4.1f} %   result "
              + " ".join(f"{v:8.4f}" for v in re_) + f"  median {med:.4f} ({100 * (med / statistics.median(pa) - 1):+5.1f} %): {verdict}")


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        table(sys.argv[2:])
    else:
        run(sys.argv[1])
