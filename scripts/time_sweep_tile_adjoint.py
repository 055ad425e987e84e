"""Wall time of logpdf_and_gradient(fx, y, method="sweep") at d = 9, 12, 16 on the tile sweep's adjoint kernel (tgp_logpdf_adjoint_group ->
k_sweep_tile_adjoint; TGP_OPT_SWEEP = 2 on the bound model) beside method="fd" -- central differences of the device logpdf, what these calls run
today -- on the same device-resident series with 10 % of the steps missing, in the same process.  Medians of --reps calls after --warmup calls with min and
max; beside them the kernel time of the adjoint call (walk + sum of the records, from the handle's profile) and of k_sweep_tile<posterior> on the same
series, and the device memory the adjoint call holds (free memory before / after its first call).  No threshold: the file states what was measured, and
every case of the full list that was not run says "not measured".  Writes profiles/sweep_tile_adjoint_time.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M52, M32, M12 = ("matern52",), ("matern32",), ("matern12",)
AP3 = ("approx_periodic", 3, 1.0)
KERNELS = {9: ("product", M52, ("stretched", 0.7, M52)), 12: ("product", M32, AP3), 16: ("sum", ("product", AP3, M32), M52, M12)}
DT, S2 = 0.2, 0.1
FULL = "9:1000000,12:1000000,16:1000000,9:10000000,12:10000000,16:10000000"


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
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def kernel_ms(hd, L, fn):
    hd.set_option(L.OPT_PROFILE, 1)
    hd.profile_reset()
    fn()
    out = {k: round(v["total_ms"], 3) for k, v in hd.profile().items()}
    hd.set_option(L.OPT_PROFILE, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fd-reps", type=int, default=None, help="calls of the fd route (default: --reps)")
    ap.add_argument("--cases", default=FULL)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_tile_adjoint_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lti_sde as P
    L, lines = tgp._lib, []
    for case in FULL.split(","):
        d, T = (int(v) for v in case.split(":"))
        if case not in args.cases.split(","):
            lines.append(json.dumps(dict(d=d, T=T, result="not measured")))
            continue
        rng = np.random.default_rng(d)
        missing = rng.random(T) < 0.1
        obs = (torch.from_numpy(np.where(missing, 0.0, rng.standard_normal(T))).cuda(), torch.from_numpy(missing).cuda())
        fx = P.to_sde(P.GP(P.to_kernel(KERNELS[d])))(P.RegularSpacing(0.0, DT, T), S2)
        dm = fx.build_lgssm()
        assert dm.dim == d
        hd = dm.handle()
        out = dict(d=d, T=T, missing=0.1, reps=args.reps, warmup=args.warmup, parameters=len(P.parameters(fx.f.f.kernel)) + 1)
        out["fd"] = timed(lambda: P.logpdf_and_gradient(fx, obs, method="fd"), args.fd_reps or args.reps, min(args.warmup, 2))      # (TGP_OPT_SWEEP = 1: today's route)
        lp_f, g_f = P.logpdf_and_gradient(fx, obs, method="fd")
        dm = fx.build_lgssm()      # (the differences rebind the model: the option goes to the handle the next calls run on)
        hd = dm.handle()
        hd.set_option(L.OPT_SWEEP, 2)
        free0 = torch.cuda.mem_get_info()[0]
        lp_s, g_s = P.logpdf_and_gradient(fx, obs, method="sweep")
        out["device_MiB_held"] = round((free0 - torch.cuda.mem_get_info()[0]) / 2**20, 1)
        info = hd.sweep_info()
        assert info["served"] == 1, info
        out["info"] = {k: info[k] for k in ("C", "W", "Wb", "waves", "attempts")}
        scale = max(abs(v) for v in g_f.values())
        assert abs(lp_s - lp_f) <= 1e-9 * abs(lp_f) and all(abs(g_s[n] - g_f[n]) <= 1e-5 * scale for n in g_f), (lp_s, lp_f, g_s, g_f)      # (a sanity check)
        out["sweep"] = timed(lambda: P.logpdf_and_gradient(fx, obs, method="sweep"), args.reps, args.warmup)
        out["fd_over_sweep"] = round(out["fd"]["median_ms"] / out["sweep"]["median_ms"], 2)
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out["kernel_ms"] = dict(kernel_ms(hd, L, lambda: P.logpdf_and_gradient(fx, obs, method="sweep")),
                                **kernel_ms(hd, L, lambda: tgp.logpdf_and_posterior_marginals(dm, obs, Rn)))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del fx, dm, hd, obs
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("# scripts/time_sweep_tile_adjoint.py: wall ms (median, min, max of `reps` calls after `warmup` calls), device-resident series, 10 % missing.\n"
                "# sweep: logpdf_and_gradient(method=\"sweep\") under TGP_OPT_SWEEP = 2 (k_sweep_tile_adjoint); fd: method=\"fd\" on the same series in the same process.\n"
                "# kernel_ms: one profiled call each (the adjoint's walk and record sum under one name; k_sweep_tile<posterior> on the same series).\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
