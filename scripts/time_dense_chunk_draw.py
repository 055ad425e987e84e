"""Wall time of a draw from the posterior of a mid-sized model with missing data on the dense engine's draw pass (tgp_posterior_rand_missing: dk_chunk_filter +
dk_chunk_draw, csrc/tgp_dense_draw.hpp) beside the route of before for the same call -- TGP_OPT_DENSE_CHUNKED = 0 in the same process: the
materialised posterior (tgp_posterior) bound as a Reverse model and drawn by the dense engine's sequential rand.  Device-resident series and draws, medians of
--reps calls after a warm-up call.  The comparison leg runs at a series it can hold (--seq-T, --seq-reps) and is compared per step.  Per-kernel times of one
more call come from tgp_profile_get.  Writes profiles/dense_chunk_draw_time.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {
    28: ("product", ("approx_periodic", 7, 1.0), ("matern32",)),      # ApproxPeriodicKernel() * Matern32Kernel()
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


def device_model(tgp, model, chunked):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], model["h"], model["R"]), T=model["T"])
    dm.handle_options[tgp._lib.OPT_DENSE_CHUNKED] = chunked
    dm.handle_options[tgp._lib.OPT_WIDE] = 0          # (the joined series of a prediction has per-step blocks: the wide engine never sees it)
    return dm


def inputs(model, d, T):
    import numpy as np
    import torch
    rng = np.random.default_rng(d)
    y = rng.standard_normal(T) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + 0.1)
    missing = rng.random(T) < 0.1            # 10 % of the steps missing
    g = torch.Generator(device="cuda").manual_seed(d)
    et = torch.randn((T, d), dtype=torch.float64, device="cuda", generator=g)
    ee = torch.randn(T, dtype=torch.float64, device="cuda", generator=g)
    return torch.from_numpy(y).cuda(), torch.from_numpy(missing).cuda(), (et, ee, rng.standard_normal(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="28:1000000,42:1000000")
    ap.add_argument("--seq-T", type=int, default=20000)
    ap.add_argument("--seq-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_chunk_draw_time.txt"))
    args = ap.parse_args()
    import torch
    import temporalgps_jl_amd as tgp
    from oracle import components as oc
    Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        out = dict(d=d, T=T, seq_T=args.seq_T, missing=0.1)
        for chunked, Tn, reps in ((1, T, args.reps), (0, args.seq_T, args.seq_reps)):
            model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, Tn), 0.1)
            y, missing, eps = inputs(model, d, Tn)
            dm = device_model(tgp, model, chunked)
            if chunked:       # a device series carries its missing steps as NaN (the mask is made on the device)
                obs = torch.where(missing, torch.full_like(y, float("nan")), y)
            else:             # the evaluated route takes a device series with its mask beside it
                obs = (y, missing)
            call = lambda: tgp.rand(eps, tgp.replace_observation_noise_cov(tgp.posterior(dm, obs), Rn))      # noqa: E731
            tag = "draw_pass" if chunked else "evaluated"
            out[f"{tag}_ms"] = med_ms(call, reps)
            info = dm.handle().dense_chunk_info()
            assert info["served"] == chunked, info
            if chunked:
                out["info"] = info
                hd = dm.handle()
                hd.set_option(tgp._lib.OPT_PROFILE, 1)
                hd.profile_reset()
                call()
                torch.cuda.synchronize()
                out["kernels"] = hd.profile()
                hd.set_option(tgp._lib.OPT_PROFILE, 0)
            del dm, y, missing, eps, obs
        per_c, per_s = out["draw_pass_ms"] / T, out["evaluated_ms"] / args.seq_T
        out["us_per_step_draw_pass"], out["us_per_step_evaluated"], out["ratio_per_step"] = 1e3 * per_c, 1e3 * per_s, per_s / per_c
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_dense_chunk_draw.py: medians (ms), device-resident series and draws, 10 % of the steps missing; the evaluated leg\n"
                    "# (TGP_OPT_DENSE_CHUNKED = 0: tgp_posterior, then tgp_rand on the Reverse model) runs at seq_T steps and is compared per step\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
