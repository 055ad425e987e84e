"""Wall time of a draw from the posterior of a d <= 4 model with missing steps on the sweep engine's draw kernel (tgp_posterior_rand_missing -> k_sweep_draw,
DESIGN 4.7) beside (a) the evaluated route for the same call in the same process -- TGP_OPT_SWEEP = 0: tgp_posterior on the general engine writes the
T x (2 d^2 + d) reverse-time model, tgp_rand draws from it -- and (b) k_sweep<lti,posterior> on the same series, whose backward pass does comparable work.
Device-resident series and draws, 10 % of the steps missing (NaN), medians of --reps calls after a warm-up call with min and max; per-kernel times of one
more call from tgp_profile_get; device memory a route holds after its calls (the handle keeps its buffers and torch its blocks: the route's peak) from
hipMemGetInfo.  Writes profiles/sweep_draw_time.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {
    2: (("matern32",), 0.1, 0.1),
    3: (("matern52",), 0.1, 0.1),
    4: (("sum", ("matern32",), ("stretched", 0.7, ("matern32",))), 0.15, 0.1),
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
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def used_mib():
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2**20


def profiled(tgp, dm, fn):
    import torch
    hd = dm.handle()
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
    ap.add_argument("--cases", default="2:1000000,3:1000000,4:1000000,2:10000000,3:10000000,4:10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_draw_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from oracle import components as oc
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        k, dt, s2 = KERNELS[d]
        model = dict(oc.build_lgssm(k, ("regular", 0.0, dt, 64), s2), T=T)
        rng = np.random.default_rng(d)
        y = rng.standard_normal(T) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + s2)
        missing = rng.random(T) < 0.1
        # the draw's mirror takes a device series with its missing steps as NaN (the mask is made on the device); the evaluated route and the
        # posterior marginals take the series with its mask beside it
        obs = torch.from_numpy(np.where(missing, np.nan, y)).cuda()
        obs_mask = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        g = torch.Generator(device="cuda").manual_seed(d)
        eps = (torch.randn((T, d), dtype=torch.float64, device="cuda", generator=g), torch.randn(T, dtype=torch.float64, device="cuda", generator=g),
               rng.standard_normal(d))
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out = dict(d=d, T=T, missing=0.1, reps=args.reps)
        for tag, sweep in (("draw_kernel", 1), ("evaluated", 0)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = used_mib()
            tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
            dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], model["h"], model["R"]), T=T)
            dm.handle_options[tgp._lib.OPT_SWEEP] = sweep
            series = obs if sweep else obs_mask
            call = lambda: tgp.rand(eps, tgp.replace_observation_noise_cov(tgp.posterior(dm, series), Rn))      # noqa: E731
            out[tag] = timed(call, args.reps)
            out[tag]["held_MiB"] = round(used_mib() - before, 1)
            info = dm.handle().sweep_info()
            assert info["served"] == sweep, info
            out[tag]["kernels_ms"] = profiled(tgp, dm, call)      # (the prior's handle: the evaluated route's tgp_rand runs on the Reverse model's own)
            assert ("k_sweep_draw<lti>" in out[tag]["kernels_ms"]) == bool(sweep), out[tag]["kernels_ms"]
            if sweep:
                out["info"] = info
                post = lambda: tgp.logpdf_and_posterior_marginals(dm, obs_mask, Rn)      # noqa: E731
                out["posterior_marginals"] = timed(post, args.reps)
                out["posterior_marginals"]["kernels_ms"] = profiled(tgp, dm, post)
                assert "k_sweep<lti,posterior>" in out["posterior_marginals"]["kernels_ms"], out["posterior_marginals"]
            del dm, tr
        out["evaluated_over_draw_kernel"] = round(out["evaluated"]["median_ms"] / out["draw_kernel"]["median_ms"], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del obs, obs_mask, eps
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_draw.py: wall ms (median, min, max of `reps` calls), device-resident series and draws, 10 % of the steps missing.\n"
                    "# draw_kernel: tgp_posterior_rand_missing on k_sweep_draw; evaluated: the same call with TGP_OPT_SWEEP = 0 (tgp_posterior + tgp_rand);\n"
                    "# posterior_marginals: k_sweep<lti,posterior> on the same series.  held_MiB: device memory the route holds after its calls.\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
