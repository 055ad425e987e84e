"""Wall time of logpdf and posterior marginals of a mid-sized model with missing data on the dense engine's passes across the chip (TGP_OPT_DENSE_CHUNKED = 1,
csrc/tgp_dense_chunked.hpp) beside the sequential passes (option 20 = 0: the path of before, unchanged) in one process: device-resident inputs,
medians of --reps calls after a warm-up call.  The sequential leg runs at a shorter series (--seq-T, --seq-reps) and is scaled per step; the ratio printed is
of the per-step times.  Per-kernel times of one more chunked call come from tgp_profile_get.  Writes profiles/dense_chunked_time.txt."""
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
    return dm


def series(model, d, T):
    import numpy as np
    import torch
    rng = np.random.default_rng(d)
    y = rng.standard_normal(T) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + 0.1)
    missing = rng.random(T) < 0.1            # 10 % of the steps missing
    y[missing] = 0.0
    return torch.from_numpy(y).cuda(), torch.from_numpy(missing).cuda()      # (device series: the mask beside it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="28:1000000,42:1000000")
    ap.add_argument("--seq-T", type=int, default=20000)
    ap.add_argument("--seq-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_chunked_time.txt"))
    args = ap.parse_args()
    import torch
    import temporalgps_jl_amd as tgp
    from oracle import components as oc
    Rn = torch.full((1,), 0.05, dtype=torch.float64, device="cuda")
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        out = dict(d=d, T=T, seq_T=args.seq_T, missing=0.1)
        for chunked, Tn, reps in ((1, T, args.reps), (0, args.seq_T, args.seq_reps)):
            model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, Tn), 0.1)
            y = series(model, d, Tn)
            dm = device_model(tgp, model, chunked)
            tag = "chunked" if chunked else "sequential"
            out[f"logpdf_{tag}_ms"] = med_ms(lambda: tgp.logpdf(dm, y), reps)
            info_l = dm.handle().dense_chunk_info()
            out[f"posterior_{tag}_ms"] = med_ms(lambda: tgp.posterior_marginals(dm, y, Rn), reps)
            info_p = dm.handle().dense_chunk_info()
            assert info_l["served"] == chunked and info_p["served"] == chunked, (info_l, info_p)
            if chunked:
                out["info_logpdf"], out["info_posterior"] = info_l, info_p
                hd = dm.handle()
                hd.set_option(tgp._lib.OPT_PROFILE, 1)
                hd.profile_reset()
                tgp.logpdf(dm, y)
                tgp.posterior_marginals(dm, y, Rn)
                torch.cuda.synchronize()
                out["kernels_logpdf_plus_posterior"] = hd.profile()
                hd.set_option(tgp._lib.OPT_PROFILE, 0)
            del dm, y
        for call in ("logpdf", "posterior"):
            per_c, per_s = out[f"{call}_chunked_ms"] / T, out[f"{call}_sequential_ms"] / args.seq_T
            out[f"{call}_us_per_step_chunked"], out[f"{call}_us_per_step_sequential"] = 1e3 * per_c, 1e3 * per_s
            out[f"{call}_ratio_per_step"] = per_s / per_c
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_dense_chunked.py: medians (ms), device-resident inputs, 10 % of the steps missing; the sequential leg (TGP_OPT_DENSE_CHUNKED = 0)\n"
                    "# runs at seq_T steps and is compared per step\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
