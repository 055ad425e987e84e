"""Wall time of tgp_logpdf and of the combined call (tgp_logpdf_and_posterior_marginals) for SDE-described d = 5 .. 8 models on irregular inputs on the
group sweep (tgp_sweep_group_sde.hip; TGP_OPT_SWEEP = 2) beside the same call under TGP_OPT_SWEEP = 1 in the same process -- the general
chunked-scan engine, the route such a call takes by default.  Gaps ~ U(0.05, 0.15), device-resident series with 10 % of the steps missing, medians of
--reps calls after --warmup calls with min and max, the two routes' handles alive side by side.  Writes profiles/sweep_group_sde_time.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M52, M32 = ("matern52",), ("matern32",)
KERNELS = {
    5: (("sum", M52, M32), 0.1),
    6: (("sum", M52, ("stretched", 0.7, M52)), 0.1),
    7: (("sum", M52, M32, ("stretched", 0.7, M32)), 0.1),
    8: (("sum", M52, ("stretched", 0.7, M52), M32), 0.1),
}


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="5:1000000,6:1000000,7:1000000,8:1000000,5:10000000,6:10000000,7:10000000,8:10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_group_sde_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lti_sde as P
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        k, s2 = KERNELS[d]
        rng = np.random.default_rng(d)
        t = np.cumsum(rng.uniform(0.05, 0.15, T))
        y = rng.standard_normal(T) * np.sqrt(len(k) - 1 + s2)      # (unit-variance summands)
        missing = rng.random(T) < 0.1
        obs = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out = dict(d=d, T=T, gaps="U(0.05, 0.15)", missing=0.1, reps=args.reps, warmup=args.warmup)
        routes = {}
        for tag, sweep in (("group_sweep", 2), ("general", 1)):
            dm = P.build_lgssm(P.to_kernel(k), t, s2, device_components=True)
            dm.handle().set_option(tgp._lib.OPT_SWEEP, sweep)
            routes[tag] = dm
        vals = {}
        for what, fn in (("logpdf", lambda m: tgp.logpdf(m, obs)), ("combined", lambda m: tgp.logpdf_and_posterior_marginals(m, obs, Rn))):
            out[what] = {}
            for tag, sweep in (("group_sweep", 2), ("general", 1)):
                dm = routes[tag]
                out[what][tag] = timed(lambda: fn(dm), args.reps, args.warmup)
                info = dm.handle().sweep_info()
                assert info["served"] == int(sweep == 2), (tag, info)
                if sweep == 2:
                    out[what]["info"] = {key: info[key] for key in ("C", "W", "Wb", "waves", "attempts")}
                r = fn(dm)
                vals[(what, tag)] = float(r if what == "logpdf" else r[0])
            a, b = vals[(what, "group_sweep")], vals[(what, "general")]
            assert abs(a - b) <= 1e-9 * abs(b), (what, a, b)      # (the two routes on the same series: a sanity check, not the parity test)
            out[what]["general_over_group_sweep"] = round(out[what]["general"]["median_ms"] / out[what]["group_sweep"]["median_ms"], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del routes, obs
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_group_sde.py: wall ms (median, min, max of `reps` calls after `warmup` calls), device-resident series, gaps ~ U(0.05, 0.15), 10 % of the steps missing.\n"
                    "# group_sweep: k_sweep_group_sde (TGP_OPT_SWEEP = 2); general: the same call with TGP_OPT_SWEEP = 1 in the same process (the chunked-scan engine).\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
