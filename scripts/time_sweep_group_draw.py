"""Wall time of a draw from the posterior of a 5 <= d <= 8 model with missing steps on the group sweep's draw kernel (tgp_posterior_rand_group ->
k_sweep_group_draw) beside (a) the evaluated route for the same call in the same process -- rand's default chain at these d: tgp_posterior on
the general engine writes the T x (2 d^2 + d) reverse-time model, tgp_rand draws from it -- and (b) k_sweep_group<lti,posterior> on the same series, whose
backward pass does comparable work.  Device-resident series and draws, regular grid, 10 % of the steps missing (NaN), medians of --reps calls after --warm
calls with min and max; per-kernel times of one more call of its own from tgp_profile_get; device memory a route holds after its calls (the handle keeps
its buffers and torch its blocks: the route's peak) from hipMemGetInfo.  Writes profiles/sweep_group_draw_time.txt."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M52, M32 = ("matern52",), ("matern32",)
KERNELS = {      # tests/_sweep_group.py's models
    5: (("sum", M52, M32), 0.1, 0.1),
    6: (("sum", M52, ("stretched", 0.7, M52)), 0.1, 0.1),
    7: (("sum", M52, M32, ("stretched", 0.7, M32)), 0.1, 0.1),
    8: (("sum", M52, ("stretched", 0.7, M52), M32), 0.1, 0.1),
}
DRAW, POST = "k_sweep_group_draw<lti>", "k_sweep_group<lti,posterior>"


def timed(fn, reps, warm):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


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
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--cases", default="5:1000000,6:1000000,7:1000000,8:1000000,5:10000000,6:10000000,7:10000000,8:10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_group_draw_time.txt"))
    ap.add_argument("--append", action="store_true", help="keep the lines the file already has (a run split over several processes)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from oracle import components as oc
    lines = []
    if args.append and os.path.exists(args.out):
        lines = [ln.rstrip("\n") for ln in open(args.out) if ln.startswith("{")]
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        k, dt, s2 = KERNELS[d]
        model = dict(oc.build_lgssm(k, ("regular", 0.0, dt, 64), s2), T=T)
        assert len(model["x0m"]) == d
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
        out = dict(d=d, T=T, missing=0.1, reps=args.reps, warm=args.warm)
        for tag, method, sweep in (("draw_kernel", "sweep", 2), ("evaluated", None, 0)):
            gc.collect()      # (the handle and the tensors of the route before: their device memory must not count against this one)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = used_mib()
            tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
            dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], model["h"], model["R"]), T=T)
            dm.handle_options[tgp._lib.OPT_SWEEP] = sweep      # (2: the posterior marginals below run on the group sweep as well)
            series = obs if method else obs_mask
            call = lambda: tgp.rand(eps, tgp.replace_observation_noise_cov(tgp.posterior(dm, series), Rn), method=method)      # noqa: E731
            out[tag] = timed(call, args.reps, args.warm)
            out[tag]["held_MiB"] = round(used_mib() - before, 1)
            info = dm.handle().sweep_info()
            assert info["served"] == (1 if method else 0), info
            out[tag]["kernels_ms"] = profiled(tgp, dm, call)      # (the prior's handle: the evaluated route's tgp_rand runs on the Reverse model's own)
            assert (DRAW in out[tag]["kernels_ms"]) == bool(method), out[tag]["kernels_ms"]
            if method:
                out["info"] = info
                post = lambda: tgp.logpdf_and_posterior_marginals(dm, obs_mask, Rn)      # noqa: E731
                out["posterior_marginals"] = timed(post, args.reps, args.warm)
                out["posterior_marginals"]["kernels_ms"] = profiled(tgp, dm, post)
                assert POST in out["posterior_marginals"]["kernels_ms"], out["posterior_marginals"]
                out["draw_over_posterior_kernel"] = round(out[tag]["kernels_ms"][DRAW] / out["posterior_marginals"]["kernels_ms"][POST], 3)
            del dm, tr, call
        out["evaluated_over_draw_kernel"] = round(out["evaluated"]["median_ms"] / out["draw_kernel"]["median_ms"], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del obs, obs_mask, eps
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_group_draw.py: wall ms (median, min, max of `reps` calls after `warm`), device-resident series and draws, regular grid,\n"
                    "# 10 % of the steps missing.  draw_kernel: tgp_posterior_rand_group on k_sweep_group_draw; evaluated: rand's default chain at these d\n"
                    "# (tgp_posterior + tgp_rand); posterior_marginals: k_sweep_group<lti,posterior> on the same series (TGP_OPT_SWEEP = 2).  kernels_ms: one more\n"
                    "# call of its own under tgp_profile_get.  held_MiB: device memory the route holds after its calls.\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
