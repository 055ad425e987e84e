"""Wall time of a draw from the posterior on the wide-state engine (tgp_posterior_rand: forward kernel + k_wide_post_rand) beside the evaluated
route (tgp_posterior, the Reverse model bound, tgp_rand -- what serves the call with TGP_OPT_WIDE = 0) in one process: device-resident series and draws,
medians of --reps calls after a warm-up.  The evaluated route writes T (2 d^2 + d) doubles, so it runs at a shorter series (--eval-cases) and is scaled
per step; the ratio printed is of the per-step times.  The plan's figures come from the engine's TGP_STEADY_DEBUG line of one more call (stderr).
Per-kernel times: run under rocprofv3 --kernel-trace --stats (a separate run, --reps 3 --no-eval)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {
    9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))),
    12: ("product", ("matern32",), ("approx_periodic", 3, 1.0)),
    28: ("product", ("approx_periodic", 7, 1.0), ("matern32",)),
    42: ("product", ("approx_periodic", 7, 1.0), ("matern52",)),
}


def med_ms(fn, reps):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def device_model(tgp, model, wide):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], model["h"], model["R"]), T=model["T"])
    dm.handle_options[tgp._lib.OPT_WIDE] = wide
    return dm


def inputs(model, d, T):
    import numpy as np
    import torch
    rng = np.random.default_rng(d)
    y = rng.standard_normal(T) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + 0.1)
    gen = torch.Generator(device="cuda").manual_seed(d)
    eps = (torch.randn((T, d), dtype=torch.float64, device="cuda", generator=gen), torch.randn((T,), dtype=torch.float64, device="cuda", generator=gen),
           rng.standard_normal(d))
    return torch.from_numpy(y).cuda(), eps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="28:1000000,42:1000000,9:10000000,12:10000000")
    ap.add_argument("--eval-cases", default="28:20000,42:10000,9:200000,12:200000")
    ap.add_argument("--eval-reps", type=int, default=3)
    ap.add_argument("--no-eval", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import temporalgps_jl_amd as tgp
    from oracle import components as oc
    T_eval = dict((int(a), int(b)) for a, b in (c.split(":") for c in args.eval_cases.split(",")))
    Rn = np.array([1e-6])
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)
        y, eps = inputs(model, d, T)
        dm = device_model(tgp, model, 1)
        post = tgp.replace_observation_noise_cov(tgp.posterior(dm, y), Rn)
        hd = dm.handle()
        hd.set_option(tgp._lib.OPT_PROFILE, 1)
        hd.profile_reset()
        tgp.rand(eps, post)
        names = sorted(hd.profile())
        hd.set_option(tgp._lib.OPT_PROFILE, 0)
        out = dict(d=d, T=T, kernels=names)
        out["draw_ms"] = med_ms(lambda: tgp.rand(eps, post), args.reps)
        out["marginals_ms"] = med_ms(lambda: tgp.posterior_marginals(dm, y, Rn), args.reps)
        out["draw_ns_per_step"] = out["draw_ms"] * 1e6 / T
        os.environ["TGP_STEADY_DEBUG"] = "1"
        tgp.rand(eps, post)
        del os.environ["TGP_STEADY_DEBUG"]
        sys.stderr.flush()
        del y, eps, post, dm
        if not args.no_eval:
            Te = T_eval[d]
            model_e = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, Te), 0.1)
            ye, epse = inputs(model_e, d, Te)
            dm0 = device_model(tgp, model_e, 0)

            def evaluated():
                p0 = tgp.replace_observation_noise_cov(tgp.posterior(dm0, ye), Rn)
                p0.materialise()
                return tgp.rand(epse, p0)
            out["evaluated_T"] = Te
            out["evaluated_ms"] = med_ms(evaluated, args.eval_reps)
            out["evaluated_ns_per_step"] = out["evaluated_ms"] * 1e6 / Te
            out["ratio_per_step"] = out["evaluated_ns_per_step"] / out["draw_ns_per_step"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
