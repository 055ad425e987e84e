"""Wall time of tgp_logpdf and of the combined call (tgp_logpdf_and_posterior_marginals) for d = 9, 12, 16 models with missing steps on the tile sweep
(tgp_sweep_tile.hip) beside the same call with TGP_OPT_SWEEP = 0 in the same process -- the general chunked-scan engine, the route such a
call takes by default.  Device-resident series with 10 % of the steps missing, medians of --reps calls after --warmup calls with min and max, the two
routes' handles alive side by side.  No threshold: the file states what was measured.  Writes profiles/sweep_tile_time.txt."""
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
KERNELS = {
    9: ("product", M52, ("stretched", 0.7, M52)),
    12: ("product", M32, AP3),
    16: ("sum", ("product", AP3, M32), M52, M12),
}
DT, S2 = 0.2, 0.1


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
    ap.add_argument("--cases", default="9:1000000,12:1000000,16:1000000,9:10000000,12:10000000,16:10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_tile_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from oracle import components as oc
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        model = dict(oc.build_lgssm(KERNELS[d], ("regular", 0.0, DT, 64), S2), T=T)
        assert len(model["x0m"]) == d
        rng = np.random.default_rng(d)
        y = rng.standard_normal(T) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + S2)
        missing = rng.random(T) < 0.1
        obs = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out = dict(d=d, T=T, missing=0.1, reps=args.reps, warmup=args.warmup)
        routes = {}
        for tag, sweep in (("tile_sweep", 2), ("general", 0)):
            tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
            dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], model["h"], model["R"]), T=T)
            dm.handle_options[tgp._lib.OPT_SWEEP] = sweep
            routes[tag] = dm
        vals = {}
        for what, fn in (("logpdf", lambda m: tgp.logpdf(m, obs)), ("combined", lambda m: tgp.logpdf_and_posterior_marginals(m, obs, Rn))):
            out[what] = {}
            for tag, sweep in (("tile_sweep", 2), ("general", 0)):
                dm = routes[tag]
                out[what][tag] = timed(lambda: fn(dm), args.reps, args.warmup)
                info = dm.handle().sweep_info()
                assert info["served"] == int(sweep > 0), (tag, info)
                if sweep:
                    out[what]["info"] = {key: info[key] for key in ("C", "W", "Wb", "waves", "attempts")}
                r = fn(dm)
                vals[(what, tag)] = float(r if what == "logpdf" else r[0])
            a, b = vals[(what, "tile_sweep")], vals[(what, "general")]
            assert abs(a - b) <= 1e-9 * abs(b), (what, a, b)      # (the two routes on the same series: a sanity check, not the parity test)
            out[what]["general_over_tile_sweep"] = round(out[what]["general"]["median_ms"] / out[what]["tile_sweep"]["median_ms"], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del routes, obs
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_tile.py: wall ms (median, min, max of `reps` calls after `warmup` calls), device-resident series, 10 % of the steps missing.\n"
                    "# tile_sweep: k_sweep_tile (TGP_OPT_SWEEP = 2); general: the same call with TGP_OPT_SWEEP = 0 in the same process (the chunked-scan engine).\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
