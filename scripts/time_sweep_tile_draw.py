"""Wall time of a draw from the posterior of a 9 <= d <= 16 model with missing steps on the tile sweep's draw kernel (tgp_posterior_rand_group ->
k_sweep_tile_draw; TGP_OPT_SWEEP = 2 on the bound model) beside the evaluated route for the same call in the same process -- rand's default
chain at these d: tgp_posterior on the general engine writes the T x (2 d^2 + d) reverse-time model, tgp_rand draws from it.  Device-resident series and
draws, regular grid, 10 % of the steps missing, medians of --reps calls after --warm calls with min and max; per-kernel times of one more call of its own
from the handle's profile, beside k_sweep_tile<posterior> and k_sweep_tile_adjoint on the same series; device memory the draw call holds after its first call.  No
threshold: the file states what was measured, and every case of the full list that was not run says "not measured".  Writes
profiles/sweep_tile_draw_time.txt."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M52, M32, M12 = ("matern52",), ("matern32",), ("matern12",)
AP3 = ("approx_periodic", 3, 1.0)
KERNELS = {9: ("product", M52, ("stretched", 0.7, M52)), 12: ("product", M32, AP3), 16: ("sum", ("product", AP3, M32), M52, M12)}      # scripts/time_sweep_tile_adjoint.py's
DT, S2 = 0.2, 0.1
FULL = "9:1000000,12:1000000,16:1000000,9:10000000,12:10000000,16:10000000"
DRAW, POST, ADJ = "k_sweep_tile_draw<lti>", "k_sweep_tile<posterior>", "k_sweep_tile_adjoint<lti>"


def timed(fn, reps, warm):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        gc.collect()      # (outside the timed span: the evaluated route's Reverse models of the calls before, T (2 d^2 + d) doubles each)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


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
    out = {k: round(v["total_ms"], 3) for k, v in hd.profile().items()}
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--cases", default=FULL)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_tile_draw_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from oracle import components as oc
    lines = []
    for case in FULL.split(","):
        d, T = (int(v) for v in case.split(":"))
        if case not in args.cases.split(","):
            lines.append(json.dumps(dict(d=d, T=T, result="not measured")))
            continue
        model = dict(oc.build_lgssm(KERNELS[d], ("regular", 0.0, DT, 64), S2), T=T)
        assert len(model["x0m"]) == d
        rng = np.random.default_rng(d)
        y = rng.standard_normal(T) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + S2)
        missing = rng.random(T) < 0.1
        obs = torch.from_numpy(np.where(missing, np.nan, y)).cuda()      # the draw's mirror makes the mask from the NaNs on the device
        obs_mask = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        g = torch.Generator(device="cuda").manual_seed(d)
        eps = (torch.randn((T, d), dtype=torch.float64, device="cuda", generator=g), torch.randn(T, dtype=torch.float64, device="cuda", generator=g),
               rng.standard_normal(d))
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out = dict(d=d, T=T, missing=0.1, reps=args.reps, warm=args.warm)
        for tag, method, sweep in (("draw_kernel", "sweep", 2), ("evaluated", None, 1)):      # (1: the default option)
            gc.collect()      # (the handle and the tensors of the route before: their device memory must not count against this one)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = used_mib()
            tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
            dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], model["h"], model["R"]), T=T)
            dm.handle_options[tgp._lib.OPT_SWEEP] = sweep
            series = obs if method else obs_mask
            call = lambda: tgp.rand(eps, tgp.replace_observation_noise_cov(tgp.posterior(dm, series), Rn), method=method)      # noqa: E731
            try:
                call()      # (the first call: what the route allocates, before the timed calls' garbage of Reverse models blurs the balance)
                torch.cuda.synchronize()
                held = round(used_mib() - before, 1)
                out[tag] = timed(call, args.reps, args.warm)
            except Exception as e:      # (the evaluated route's model does not fit: the row says so and nothing more is run)
                out[tag], args.cases = "not measured: " + (str(e).splitlines() or [type(e).__name__])[0][:160], ""
                break
            if method:      # (the evaluated route's balance is not a measurement: its Reverse models are bound on handles of their own and freed by the
                out[tag]["held_MiB"] = held      # collector whenever it runs; its model alone is T (2 d^2 + d) doubles)
                out["evaluated_model_MiB"] = round(T * (2 * d * d + d) * 8 / 2**20, 1)
            out[tag]["kernels_ms"] = profiled(tgp, dm, call)      # (the prior's handle: the evaluated route's tgp_rand runs on the Reverse model's own)
            assert (DRAW in out[tag]["kernels_ms"]) == bool(method), out[tag]["kernels_ms"]
            if method:
                info = dm.handle().sweep_info()
                assert info["served"] == 1, info
                out["info"] = {k: info[k] for k in ("C", "W", "Wb", "waves", "attempts")}
                beside = dict(profiled(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, obs_mask, Rn)),
                              **profiled(tgp, dm, lambda: tgp.lgssm.logpdf_adjoint_group(dm, obs_mask)))
                out["beside_ms"] = {k: beside[k] for k in (POST, ADJ)}
                out["draw_over_posterior_kernel"] = round(out[tag]["kernels_ms"][DRAW] / beside[POST], 2)
            del dm, tr, call
            gc.collect()
        if isinstance(out.get("evaluated"), dict):
            out["evaluated_over_draw_kernel"] = round(out["evaluated"]["median_ms"] / out["draw_kernel"]["median_ms"], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del obs, obs_mask, eps
    with open(args.out, "w") as f:
        f.write("# scripts/time_sweep_tile_draw.py: wall ms (median, min, max of `reps` calls after `warm`), device-resident series and draws, regular grid,\n"
                "# 10 % of the steps missing.  draw_kernel: tgp_posterior_rand_group on k_sweep_tile_draw (TGP_OPT_SWEEP = 2); evaluated: rand's default chain at\n"
                "# these d (tgp_posterior + tgp_rand) on the same series in the same process.  kernels_ms: one more call of its own under the handle's profile;\n"
                "# beside_ms: k_sweep_tile<posterior> and k_sweep_tile_adjoint on the same series and handle.  held_MiB: device memory the draw call holds after its first call;\n"
                "# evaluated_model_MiB: T (2 d^2 + d) doubles, the reverse-time model the evaluated route writes (arithmetic, not a measurement).\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
