"""Wall time of a draw from the posterior of an SDE-described 5 <= d <= 8 model on irregular inputs with missing steps on the group sweep's draw kernel
(tgp_posterior_rand_group_sde -> k_sweep_group_draw<sde>) beside the evaluated route for the same call on the SAME bound model in the same
process -- what rand runs today: tgp_posterior on the general engine writes the T x (2 d^2 + d) reverse-time model, tgp_rand draws from it.  Device-resident
series and draws, gaps U(0.05, 0.15), 10 % of the steps missing (NaN), the model bound once; medians of --reps calls after --warm calls with min and max
(DESIGN 6.1).  Per-kernel times of one more call of its own from tgp_profile_get, beside k_sweep_group<sde,posterior> on the same model and
k_sweep_group_draw<lti> on a regular grid at the same d and T.  Device memory a route holds after its calls from hipMemGetInfo (usable at T = 1e7 only,
DESIGN 4.12).  Writes profiles/sweep_group_draw_sde_time.txt."""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_sweep_group_draw import KERNELS, profiled, timed, used_mib      # noqa: E402

DRAW, POST, DRAW_LTI = "k_sweep_group_draw<sde>", "k_sweep_group<sde,posterior>", "k_sweep_group_draw<lti>"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--cases", default="5:1000000,6:1000000,7:1000000,8:1000000,5:10000000,6:10000000,7:10000000,8:10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_group_draw_sde_time.txt"))
    ap.add_argument("--append", action="store_true", help="keep the lines the file already has (a run split over several processes)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lti_sde as P
    from oracle import components as oc
    lines = []
    if args.append and os.path.exists(args.out):
        lines = [ln.rstrip("\n") for ln in open(args.out) if ln.startswith("{")]
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        k, dt, s2 = KERNELS[d]
        lti = dict(oc.build_lgssm(k, ("regular", 0.0, dt, 64), s2), T=T)
        rng = np.random.default_rng(d)
        times = np.cumsum(rng.uniform(0.05, 0.15, T))
        y = rng.standard_normal(T) * np.sqrt(float(lti["H"][0] @ lti["x0P"] @ lti["H"][0]) + s2)
        missing = rng.random(T) < 0.1
        obs = torch.from_numpy(np.where(missing, np.nan, y)).cuda()
        obs_mask = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        g = torch.Generator(device="cuda").manual_seed(d)
        eps = (torch.randn((T, d), dtype=torch.float64, device="cuda", generator=g), torch.randn(T, dtype=torch.float64, device="cuda", generator=g),
               rng.standard_normal(d))
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out = dict(d=d, T=T, missing=0.1, reps=args.reps, warm=args.warm)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = used_mib()
        dm = P.build_lgssm(P.to_kernel(k), times, s2, device_components=True)      # bound once: both routes and the posterior kernel run on this handle
        dm.handle().set_option(tgp._lib.OPT_SWEEP, 2)                              # (2: the posterior marginals below run on the group sweep as well)
        for tag, method in (("draw_kernel", "sweep"), ("evaluated", None)):
            series = obs if method else obs_mask
            call = lambda: tgp.rand(eps, tgp.replace_observation_noise_cov(tgp.posterior(dm, series), Rn), method=method)      # noqa: E731
            out[tag] = timed(call, args.reps, args.warm)
            out[tag]["held_MiB"] = round(used_mib() - before, 1)      # (cumulative on the one handle: the evaluated route's figure includes the draw's)
            info = dm.handle().sweep_info()
            assert info["served"] == (1 if method else 0), info
            out[tag]["kernels_ms"] = profiled(tgp, dm, call)
            assert (DRAW in out[tag]["kernels_ms"]) == bool(method), out[tag]["kernels_ms"]
            if method:
                out["info"] = info
                post = lambda: tgp.logpdf_and_posterior_marginals(dm, obs_mask, Rn)      # noqa: E731
                out["posterior_marginals"] = timed(post, args.reps, args.warm)
                out["posterior_marginals"]["kernels_ms"] = profiled(tgp, dm, post)
                assert POST in out["posterior_marginals"]["kernels_ms"], out["posterior_marginals"]
                out["draw_over_posterior_kernel"] = round(out[tag]["kernels_ms"][DRAW] / out["posterior_marginals"]["kernels_ms"][POST], 3)
        out["evaluated_over_draw_kernel"] = round(out["evaluated"]["median_ms"] / out["draw_kernel"]["median_ms"], 2)
        del dm, call, post
        gc.collect()
        torch.cuda.empty_cache()
        # the LTI draw kernel at the same d and T (a regular grid with the median gap)
        tr = tgp.GaussMarkovModel(tgp.Forward, lti["A"], lti["a"], lti["Q"], tgp.Gaussian(lti["x0m"], lti["x0P"]))
        dl = tgp.LGSSM(tr, tgp.ScalarOutputLGC(lti["H"], lti["h"], lti["R"]), T=T)
        call = lambda: tgp.rand(eps, tgp.replace_observation_noise_cov(tgp.posterior(dl, obs), Rn), method="sweep")      # noqa: E731
        call()
        out["lti_draw_kernel_ms"] = profiled(tgp, dl, call)[DRAW_LTI]
        del dl, tr, call
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del obs, obs_mask, eps
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_group_draw_sde.py: wall ms (median, min, max of `reps` calls after `warm`), device-resident series and draws, gaps\n"
                    "# U(0.05, 0.15), 10 % of the steps missing, the model bound once.  draw_kernel: tgp_posterior_rand_group_sde on k_sweep_group_draw<sde>;\n"
                    "# evaluated: rand's default chain on the same bound model (tgp_posterior + tgp_rand); posterior_marginals: k_sweep_group<sde,posterior>\n"
                    "# on the same model (TGP_OPT_SWEEP = 2); lti_draw_kernel_ms: k_sweep_group_draw<lti> on a regular grid at the same d and T.  kernels_ms:\n"
                    "# one more call of its own under tgp_profile_get.  held_MiB: device memory held after the route's calls (cumulative on the one handle;\n"
                    "# usable at T = 1e7 only).\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
