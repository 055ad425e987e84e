"""Wall time of logpdf + gradient of a d <= 4 GP on irregularly spaced (plain-array) inputs with missing observations by ONE adjoint pass on the sweep
engine (logpdf_and_gradient(method="sweep") -> tgp_logpdf_adjoint_sde -> k_sweep_adjoint<sde>) beside (a) the tangent scans for the same call on
the same series in the same process (method="tangent" -> tgp_logpdf_grad_sde: one dual-number pass of the general engine per hyper-parameter -- the route
these inputs have by default) and (b) k_sweep<sde,posterior> on the same series, the yardstick for the kernel.
Device-resident series, gaps ~ U(0.05, 0.15), 10 % of the steps missing, medians of --reps calls after a warm-up call with min and max; the two routes
alternate call by call.
gp: the GP-level call, which binds the model anew (time stamps to the device) in every call on either route; bound: the same device work on a model bound
once (lgssm.logpdf_adjoint_sde / lgssm.logpdf_and_grad_sde), with the per-kernel times of one more call from tgp_profile_get.
Writes profiles/sweep_adjoint_sde_time.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M32, M52 = ("matern32",), ("matern52",)
KERNELS = {      # d: (kernel, noise variance); hyper-parameters: a variance and an inverse length scale per term, the noise variance
    2: (("scaled", 0.8, ("stretched", 1.3, M32)), 0.1),
    3: (("scaled", 0.8, ("stretched", 1.3, M52)), 0.1),
    4: (("sum", ("scaled", 0.8, ("stretched", 1.3, M32)), ("scaled", 0.5, ("stretched", 0.7, M32))), 0.1),
}


def timed(fn, reps):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def timed_pair(fa, fb, reps):
    """the two routes on the same series, alternating call by call: a drift of the machine falls on both"""
    import torch
    fa()
    fb()
    ts = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return tuple(dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4)) for t in ts)


def profiled(tgp, hd, fn):
    import torch
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    fn()
    torch.cuda.synchronize()
    out = {k: round(v["total_ms"], 4) for k, v in hd.profile().items()}
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="2:3000,3:3000,4:3000,2:1000000,3:1000000,4:1000000,2:10000000,3:10000000,4:10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_adjoint_sde_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lgssm as L
    from temporalgps_jl_amd import lti_sde as P
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        k, s2 = KERNELS[d]
        rng = np.random.default_rng(d)
        t = np.cumsum(rng.uniform(0.05, 0.15, T))
        fx = P.to_sde(P.GP(P.to_kernel(k)))(t, s2)
        y = rng.standard_normal(T) * np.sqrt(1.0 + s2)
        missing = rng.random(T) < 0.1
        obs = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out = dict(d=d, T=T, missing=0.1, reps=args.reps)
        res = {}
        gs, gt = timed_pair(lambda: res.__setitem__("sweep", P.logpdf_and_gradient(fx, obs, method="sweep")),
                            lambda: res.__setitem__("tangent", P.logpdf_and_gradient(fx, obs, method="tangent")), args.reps)
        out["sweep"], out["tangent"] = dict(gp=gs), dict(gp=gt)
        (lp_s, g_s), (lp_t, g_t) = res["sweep"], res["tangent"]
        scale = max(abs(v) for v in g_t.values())
        out["parameters"] = len(g_t)
        out["gradient_deviation"] = float(max(abs(g_s[n] - g_t[n]) for n in g_t) / scale)
        out["logpdf_deviation"] = float(abs(lp_s - lp_t) / abs(lp_t))
        # the same device work on a model bound once
        dm = P.build_lgssm(fx.f.f.kernel, fx.x, fx.sigma2, fx.f.f.mean, fx.f.storage.device, device_components=True)
        assert dm.dim == d
        plist = P.parameters(fx.f.f.kernel)
        names = [n for n, _, _ in plist] + ["noise"]
        tangents = P._sde_param_tangents(fx, names, plist)
        calls = dict(sweep=lambda: L.logpdf_adjoint_sde(dm, obs), tangent=lambda: L.logpdf_and_grad_sde(dm, obs, tangents, 1e-6))
        out["sweep"]["bound"], out["tangent"]["bound"] = timed_pair(calls["sweep"], calls["tangent"], args.reps)
        for tag in ("sweep", "tangent"):
            if tag == "sweep":
                calls[tag]()
                out["info"] = dm.handle().sweep_info()
                assert out["info"]["served"] == 1, out["info"]
            out[tag]["kernels_ms"] = profiled(tgp, dm.handle(), calls[tag])
            assert ("k_sweep_adjoint<sde>" in out[tag]["kernels_ms"]) == (tag == "sweep"), out[tag]["kernels_ms"]
        post = lambda: tgp.logpdf_and_posterior_marginals(dm, obs, Rn)      # noqa: E731
        out["posterior_marginals"] = timed(post, args.reps)
        out["posterior_marginals"]["kernels_ms"] = profiled(tgp, dm.handle(), post)
        assert "k_sweep<sde,posterior>" in out["posterior_marginals"]["kernels_ms"], out["posterior_marginals"]
        out["tangent_over_sweep_gp"] = round(out["tangent"]["gp"]["median_ms"] / out["sweep"]["gp"]["median_ms"], 2)
        out["tangent_over_sweep_bound"] = round(out["tangent"]["bound"]["median_ms"] / out["sweep"]["bound"]["median_ms"], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del obs, fx, dm
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_adjoint_sde.py: wall ms (median, min, max of `reps` calls) of logpdf + gradient, device-resident series, plain-array\n"
                    "# inputs with gaps ~ U(0.05, 0.15), 10 % of the steps missing.  sweep: ONE adjoint pass on k_sweep_adjoint<sde>; tangent: the tangent scans of\n"
                    "# the general engine (one pass per hyper-parameter) on the same series in the same process.  gp: lti_sde.logpdf_and_gradient (binds the model\n"
                    "# in every call, either route); bound: the lgssm-level call on a model bound once; posterior_marginals: k_sweep<sde,posterior>, same series.\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
