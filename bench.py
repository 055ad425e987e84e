#!/usr/bin/env python3
"""Benchmark of the LGSSM hot path on MI355X: Kalman steps/s for one `logpdf` pass plus one
posterior-marginals pass (forward filter + RTS smoother + emission predict) over the same series.

    python bench.py --gpus N --steps K --warmup W

A "step" of the bench = logpdf(fx, y) + marginals(posterior(fx, y)(x)) over one synthetic RegularSpacing
series that is already resident in HBM (y is drawn from the model itself on the device, as
bench/single_output_gps.jl:143-145 does on the CPU). value = whole-job Kalman steps / seconds-per-step.
N > 1: ONE series is time-sharded, one contiguous segment per rank, with one all_gather of the tiny
per-segment scan elements per scan direction plus one scalar all_reduce (RCCL via torch.distributed).
`--gpus N` launched directly (no torch.distributed environment) drives the N GPUs from ONE process through the in-library multi-GPU
handle (tgp_create_multi: RCCL inside the library); under the driver's torchrun launch -- or with --torchrun -- it is one rank per GPU. N > 1 defaults to BASELINE config 4: STRONG scaling of ONE T = 1e8, d = 4 series
(`--scaling weak` keeps --T points per GPU instead; `--workload/--T` override the series).
`--workload cfg5` runs BASELINE config 5 (Separable space-time, 256 spatial points, dense d = 768 / p = 256 recursion on the
fp64 MFMA kernels; sequential in time: N > 1 means N independent replicas).
Prints ONE JSON line (rank 0). A plain run does only what that line's headline needs: set-up, W warm-up steps, the K timed steps.
`--full` adds everything else the bench measures: per-kernel hipEvent profiles and rooflines, the other engines, layouts and
configurations, the CPU baselines, the single-GPU reference of N > 1. `--dump-outputs DIR` writes what the last timed step
returned (logpdf; posterior mean and variance, a fixed seeded sample of them at the default T) as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured-achievable)

WORKLOADS = {
    # name: (kernel spec, d, dt, sigma2_obs)
    "matern52_d3": (("matern52",), 3, 0.1, 0.1),     # BASELINE "Matern32 d=3": d=3 is what Matern-5/2 produces
    "matern32_d2": (("matern32",), 2, 0.1, 0.1),     # the named kernel at the d the reference really produces
    "sum52_12_d4": (("sum", ("matern52",), ("matern12",)), 4, 0.1, 0.1),   # BASELINE config 4's "Matern52, d=4"
    "sum52_32_d5": (("sum", ("matern52",), ("matern32",)), 5, 0.1, 0.1),
    "sum52_52_d6": (("sum", ("matern52",), ("matern52",)), 6, 0.1, 0.1),   # BASELINE config 3's "d=6"
    "sum52_32_32_d7": (("sum", ("matern52",), ("matern32",), ("matern32",)), 7, 0.1, 0.1),
    "sum52_52_32_d8": (("sum", ("matern52",), ("matern52",), ("matern32",)), 8, 0.1, 0.1),
    # the same state dimensions with DISTINCT length scales (two identical summands make the difference of the components unobservable:
    # the closed loop keeps a defective eigenvalue and the one-launch path declines; these are the models a user fits)
    "sum52_52s_d6": (("sum", ("matern52",), ("stretched", 2.0, ("matern52",))), 6, 0.1, 0.1),
    "sum52_32s_32_d7": (("sum", ("matern52",), ("stretched", 2.0, ("matern32",)), ("matern32",)), 7, 0.1, 0.1),
    "sum52_52s_32_d8": (("sum", ("matern52",), ("stretched", 2.0, ("matern52",)), ("stretched", 0.5, ("matern32",))), 8, 0.1, 0.1),
}


def build_model(tgp, name, T, layout, device):
    """Host-side component construction (reference: lti_sde.jl:148-160 -> Fill blocks for RegularSpacing)."""
    from temporalgps_jl_amd import lti_sde
    k, d, dt, s2 = WORKLOADS[name]
    return lti_sde.build_lgssm(lti_sde.to_kernel(k), lti_sde.RegularSpacing(0.0, dt, T), s2, device=device,
                               force_per_step=(layout == "per_step"))


def cpu_baseline(name, T_sample):
    """Oracle C restatement (the SArrayStorage-equivalent sequential path) on ONE host core."""
    from oracle import components as oc
    from oracle import seq_kalman as sk
    k, d, dt, s2 = WORKLOADS[name]
    model = oc.build_lgssm(k, ("regular", 0.0, dt, T_sample), s2)
    rng = np.random.default_rng(0)
    y = sk.rand(model, rng.standard_normal((T_sample, d)), rng.standard_normal(T_sample), rng.standard_normal(d))
    sk.logpdf(model, y)          # warm
    # repeated passes over the sample until ~10 s of CPU work have been timed (bounded: the default run stays in minutes)
    t_lp = t_pm = 0.0
    reps = 0
    while t_lp + t_pm < 10.0 and reps < 200:
        t0 = time.perf_counter()
        sk.logpdf(model, y)
        t1 = time.perf_counter()
        sk.posterior_marginals(model, y, np.array([1e-18]))
        t2 = time.perf_counter()
        t_lp += t1 - t0
        t_pm += t2 - t1
        reps += 1
    return dict(value=reps * T_sample / (t_lp + t_pm), unit="Kalman steps/s", cores=1, kind="port",
                sample=f"oracle/seq_kalman.c (compile-time d={d}), same model, T={T_sample} x {reps} passes = {t_lp + t_pm:.1f}s of CPU work: "
                       f"logpdf {t_lp / reps:.3f}s/pass ({reps * T_sample / t_lp:.3e} steps/s) + posterior marginals {t_pm / reps:.3f}s/pass")


_START_AFFINITY = None


def cpu_baseline_all_cores(name, T_sample):
    """the time-parallel chunked scan on EVERY host core (oracle/omp_scan.py: the product's chunk functions
    and monoids compiled for the host with OpenMP), so that the GPU speed-up is not quoted against one core only."""
    from oracle import components as oc
    from oracle import omp_scan
    from oracle import seq_kalman as sk
    k, d, dt, s2 = WORKLOADS[name]
    if d > 8:
        return None
    model = oc.build_lgssm(k, ("regular", 0.0, dt, T_sample), s2)
    rng = np.random.default_rng(0)
    y = sk.rand(model, rng.standard_normal((T_sample, d)), rng.standard_normal(T_sample), rng.standard_normal(d))
    Rn = np.array([1e-18])
    omp_scan.logpdf(model, y)            # builds on first use, warms the threads
    t_lp = t_pm = 0.0
    reps = 0
    while t_lp + t_pm < 10.0 and reps < 400:
        t0 = time.perf_counter()
        omp_scan.logpdf(model, y)
        t1 = time.perf_counter()
        omp_scan.posterior_marginals(model, y, Rn)
        t2 = time.perf_counter()
        t_lp += t1 - t0
        t_pm += t2 - t1
        reps += 1
    return dict(value=reps * T_sample / (t_lp + t_pm), unit="Kalman steps/s", cores=os.cpu_count(), kind="port",
                sample=f"oracle/omp_scan.py (chunked associative scan, OpenMP, {os.cpu_count()} threads), same model, T={T_sample} x {reps} passes = "
                       f"{t_lp + t_pm:.1f}s: logpdf {t_lp / reps:.4f}s/pass ({reps * T_sample / t_lp:.3e} steps/s) + posterior marginals {t_pm / reps:.4f}s/pass")


def general_layout_leg(tgp, torch, name, T, d, device, steps):
    """The same series with the model in the GENERAL (per-step) layout -- every step carries its own A, a, Q, H, h, R
    (what irregular spacing / prediction at new inputs produce, lti_sde.jl:135-146): the HBM-bound regime the
    scan kernel's roofline target is stated for. Returns the roofline of its dominant kernel."""
    model = build_model(tgp, name, T, "per_step", device)
    hd = model.handle()
    gen = torch.Generator(device=f"cuda:{device}")
    gen.manual_seed(99)
    y = torch.randn((T,), dtype=torch.float64, device=f"cuda:{device}", generator=gen)
    Rnew = torch.full((1,), 1e-18, dtype=torch.float64, device=f"cuda:{device}")
    # one combined call per step, as in the headline: the model is read by three passes (pass 1, pass 2, pass 3), not five
    for _ in range(2):
        tgp.logpdf_and_posterior_marginals(model, y, Rnew)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tgp.logpdf_and_posterior_marginals(model, y, Rnew)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    for _ in range(steps):
        tgp.logpdf_and_posterior_marginals(model, y, Rnew)
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    prof = {k: v for k, v in hd.profile().items() if k.startswith(("k_reduce_filter", "k_apply_filter", "k_smooth"))}
    # The PATH is three passes over the step records (reduce, apply, smooth); each re-reads the model.  Whole-path figure: the path's algorithmic
    # bytes (the step record once + y + the outputs) over the SUM of its kernels; per kernel: the bytes THAT kernel must move at least
    # (the step record + y, plus the scan elements / outputs it writes) over its own duration, and its measured traffic (rocprofv3 PMC, profiles/)
    rec = 8 * (2 * d * d + 2 * d + 3)
    per_unit = rec + 24
    sum_ms = sum(v["total_ms"] / v["calls"] for v in prof.values())
    ach = per_unit * T / (sum_ms * 1e-3) / 1e9
    per_kernel = {}
    for k, v in prof.items():
        ms = v["total_ms"] / v["calls"]
        own = rec + (24 if k.startswith("k_smooth") else 8)      # the record + y (+ mean, var out: the smoother); scratch between the passes is not algorithmic
        tr = pmc_traffic(k, d, "per_step") if T == 10_000_000 else None
        per_kernel[k] = dict(avg_kernel_ms=ms, algorithmic_bytes_per_step=own, achieved=own * T / (ms * 1e-3) / 1e9, frac=own * T / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             traffic=tr, traffic_over_algorithmic=(tr / (own * T) if tr else None),
                             moved_GBs=(tr / (ms * 1e-3) / 1e9 if tr else None))
    return dict(bound="hbm", path="k_reduce_filter + k_apply_filter + k_smooth (one combined call)", achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s",
                frac=ach / HBM_PEAK_GBS, sum_kernel_ms=sum_ms, algorithmic_bytes=per_unit * T, algorithmic_bytes_per_step=per_unit,
                per_kernel=per_kernel, steps_per_s=T / dt, ms_per_step=dt * 1e3,
                traffic=(sum(v["traffic"] for v in per_kernel.values()) if all(v["traffic"] for v in per_kernel.values()) else None),
                note="whole path: algorithmic bytes of the PATH over the SUM of its kernels' durations (round-5 verdict: dividing them by one kernel's "
                     "time overstated the fraction); `per_kernel`: each pass against the bytes it must move itself, with its PMC traffic",
                kernels={k: dict(avg_ms=v["total_ms"] / max(1, v["calls"]), calls=v["calls"]) for k, v in hd.profile().items()})


def predict_path_legs(tgp, torch, name, T, d, device, steps):
    """The reference's predict path on the same kernel (round-4 verdict, item 1): models whose GAINS vary in time -- 10 % of the steps missing
    (missings.jl:25-41), a noise variance per step (lti_sde.jl:71-80 with a vector of variances), irregular spacing (lti_sde.jl:135-146) --
    one logpdf + posterior-marginals call per step, device-resident.  Served by the sweep engine (TGP_OPT_SWEEP) in ONE launch;
    `general_engine` = the same call with it switched off (the chunked-scan engine of round 2).  The kernel is bound by its fp64 instruction
    stream (every lane carries the covariance recursion of its chunk): its roofline is quoted against the fp64 vector peak on the sequential
    recursion's flops AND against HBM on its algorithmic bytes (y + the per-step stream in, mean + var out)."""
    from temporalgps_jl_amd import lti_sde as P
    k, _, dt, s2 = WORKLOADS[name]
    rng = np.random.default_rng(3)
    gen = torch.Generator(device=f"cuda:{device}")
    gen.manual_seed(98)
    y = torch.randn((T,), dtype=torch.float64, device=f"cuda:{device}", generator=gen)
    Rnew = torch.full((1,), 1e-18, dtype=torch.float64, device=f"cuda:{device}")
    kal = 4.0 * d ** 3 + 7.0 * d ** 2 + 8.0 * d
    rts = (12.0 + 1.0 / 3.0) * d ** 3
    out = {}

    def one(label, model, yin, bytes_per_step, what, xs_suffix=""):
        hd = model.handle()
        res = {}
        for sweep in (1, 0):
            hd.set_option(tgp._lib.OPT_SWEEP, sweep)
            for _ in range(2):
                lp, _, _ = tgp.logpdf_and_posterior_marginals(model, yin, Rnew)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tgp.logpdf_and_posterior_marginals(model, yin, Rnew)
            torch.cuda.synchronize()
            dts = (time.perf_counter() - t0) / steps
            t0 = time.perf_counter()
            for _ in range(steps):
                tgp.logpdf(model, yin)
            torch.cuda.synchronize()
            dtl = (time.perf_counter() - t0) / steps
            per_call = []
            hd.set_option(tgp._lib.OPT_PROFILE, 1)
            for _ in range(steps):
                hd.profile_reset()
                tgp.logpdf_and_posterior_marginals(model, yin, Rnew)
                per_call.append({kk: v["total_ms"] / max(1, v["calls"]) for kk, v in hd.profile().items()})
            hd.set_option(tgp._lib.OPT_PROFILE, 0)
            kern = {kk: float(np.mean([pc[kk] for pc in per_call if kk in pc])) for kk in per_call[-1]}
            r = dict(ms_per_step=dts * 1e3, steps_per_s=T / dts, logpdf_ms=dtl * 1e3, lml=float(lp), kernels_ms=kern)
            if sweep:
                info = hd.sweep_info()
                r["engine"] = {kk: info[kk] for kk in ("served", "C", "W", "Wb", "waves", "attempts")}
                dom = max(kern.items(), key=lambda kv: kv[1])
                samples = sorted(pc[dom[0]] for pc in per_call if dom[0] in pc)
                ach_b = bytes_per_step * T / (dom[1] * 1e-3) / 1e9
                ach_f = (kal + rts) * T / (dom[1] * 1e-3) / 1e12
                r["roofline"] = dict(bound="fp64_valu", kernel=dom[0], achieved=ach_f, peak=78.6, unit="TFLOP/s", frac=ach_f / 78.6,
                                     algorithmic_flops_per_step=kal + rts, avg_kernel_ms=dom[1],
                                     kernel_ms_min_median_max=[samples[0], samples[len(samples) // 2], samples[-1]],
                                     hbm=dict(achieved=ach_b, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach_b / HBM_PEAK_GBS,
                                              algorithmic_bytes_per_step=bytes_per_step, algorithmic_bytes=bytes_per_step * T,
                                              traffic=(pmc_traffic(dom[0] + xs_suffix, d, "sweep") if T == 10_000_000 else None),
                                              traffic_unit="bytes per launch (rocprofv3 PMC: 2*FETCH_SIZE + WRITE_SIZE, profiles/; a replayed builder number)"),
                                     note="one kernel per call; bound by its fp64 VALU instruction stream (one wave per SIMD, no MFMA: d x d = 3 x 3 blocks), "
                                          "not by HBM: the warm-ups re-process " + what)
                res.update(r)
            else:
                res["general_engine"] = dict(ms_per_step=r["ms_per_step"], steps_per_s=r["steps_per_s"], logpdf_ms=r["logpdf_ms"], kernels_ms=kern,
                                             lml_rel_diff=abs(res["lml"] - r["lml"]) / abs(r["lml"]))
        hd.set_option(tgp._lib.OPT_SWEEP, 1)
        out[label] = res

    miss = torch.rand((T,), device=f"cuda:{device}", generator=gen) < 0.1
    model = P.build_lgssm(P.to_kernel(k), P.RegularSpacing(0.0, dt, T), s2, device=device)
    one("missing_10pct", model, (y, miss), 25, "W / C of the forward and Wb / C of the backward steps")
    out["missing_10pct"]["workload"] = f"{name}, RegularSpacing(0,{dt},T={T}), 10 % of the steps missing (mask resident on the device)"
    del model
    S = s2 * (0.5 + rng.random(T))
    model = P.build_lgssm(P.to_kernel(k), P.RegularSpacing(0.0, dt, T), S, device=device)
    one("per_step_noise", model, y, 32, "W / C of the forward and Wb / C of the backward steps", "[xs=1]")
    out["per_step_noise"]["workload"] = f"{name}, RegularSpacing(0,{dt},T={T}), noise variance per step ~ {s2} U(0.5, 1.5)"
    del model, S
    t = np.cumsum(rng.uniform(0.5 * dt, 1.5 * dt, T))
    model = P.build_lgssm(P.to_kernel(k), t, s2, device=device, device_components=True)
    one("irregular_spacing", model, y, 32, "W / C of the forward and Wb / C of the backward steps; every step evaluates exp(F dt_k) in closed form")
    out["irregular_spacing"]["workload"] = f"{name}, T = {T}, dt ~ U({0.5 * dt:g}, {1.5 * dt:g}) (transitions from the 8-byte gap, closed form per Matern block)"
    return out


def gradient_leg(tgp, torch, name, T, d, device, steps, y):
    """logpdf + its gradient w.r.t. the kernel hyper-parameters and the noise variance -- the quantity the north_star target is stated
    on (reference: Mooncake.gradient(logpdf, fx, y), bench/single_output_gps.jl:155-156). Default method: ONE adjoint (reverse-time)
    pass on the stationary-gain engine (tgp_logpdf_adjoint) + exact block tangents on the host, cost independent of the number of
    parameters; the forward-mode tangent scans (one pass per parameter) are timed beside it. Same series as the headline leg; a
    second case with 8 parameters (Matern-5/2 + 3/2 + 1/2, each scaled and stretched, constant mean, noise; d = 6)."""
    from temporalgps_jl_amd import lti_sde as P
    k, _, dt, s2 = WORKLOADS[name]

    def timed(fx, method, n):
        for _ in range(2):
            P.logpdf_and_gradient(fx, y, method=method)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            lp, g = P.logpdf_and_gradient(fx, y, method=method)
        return (time.perf_counter() - t0) / n, lp, g

    def logpdf_ms(fx):
        P.logpdf(fx, y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            P.logpdf(fx, y)
        return (time.perf_counter() - t0) / steps * 1e3
    fx = P.to_sde(P.GP(P.ScaledKernel(1.0, P.StretchedKernel(1.0, P.to_kernel(k)))), P.HIPStorage(device=device))(P.RegularSpacing(0.0, dt, T), s2)
    dt_s, lp, g = timed(fx, None, steps)
    dt_t, _, g_t = timed(fx, "tangent", max(2, steps // 3))
    lp_ms = logpdf_ms(fx)
    k8 = (P.ScaledKernel(1.0, P.StretchedKernel(1.0, P.Matern52Kernel())) + P.ScaledKernel(0.5, P.StretchedKernel(1.5, P.Matern32Kernel()))
          + P.ScaledKernel(0.3, P.StretchedKernel(0.7, P.Matern12Kernel())))
    fx8 = P.to_sde(P.GP(P.ConstMean(0.3), k8), P.HIPStorage(device=device))(P.RegularSpacing(0.0, dt, T), s2)
    dt8, lp8, g8 = timed(fx8, None, steps)
    lp8_ms = logpdf_ms(fx8)
    return dict(metric=f"Kalman steps/sec (logpdf + gradient w.r.t. {len(g)} hyper-parameters)", value=T / dt_s, ms_per_eval=dt_s * 1e3,
                n_params=len(g), method="one adjoint pass on the device (tgp_logpdf_adjoint) + exact block tangents (Van Loan) on the host",
                logpdf=lp, gradient={kk: float(v) for kk, v in g.items()}, logpdf_ms=lp_ms, cost_in_logpdf_evaluations=dt_s * 1e3 / lp_ms,
                tangent_scans=dict(ms_per_eval=dt_t * 1e3, value=T / dt_t, note="forward-mode tangent scans, one pass per parameter (round 2's method)",
                                   max_rel_difference=max(abs(g[kk] - g_t[kk]) for kk in g) / max(abs(v) for v in g_t.values())),
                eight_parameters=dict(workload="sum of scaled, stretched Matern-5/2 + 3/2 + 1/2 with a constant mean (d = 6), same series length",
                                      n_params=len(g8), value=T / dt8, ms_per_eval=dt8 * 1e3, logpdf_ms=lp8_ms,
                                      cost_in_logpdf_evaluations=dt8 * 1e3 / lp8_ms, logpdf=lp8))


def lti_interface_leg(tgp, torch, model, y, T, d, local, steps):
    """The rest of the LTI interface on the same model and series, device-resident: rand with the draws supplied
    (lgssm.jl:65-91), a draw from the posterior (rand of the reverse-time model, not evaluated), _filter (:171-187), the evaluated posterior
    (:193-221) -- wall clock per call and the kernels each one launched."""
    hd = model.handle()

    def timed(fn, n):
        for _ in range(2):
            r = fn()
        del r
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            r = fn()
        del r
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        hd.set_option(tgp._lib.OPT_PROFILE, 1)
        hd.profile_reset()
        r = fn()
        del r
        torch.cuda.synchronize()
        hd.set_option(tgp._lib.OPT_PROFILE, 0)
        return dt, {k: v["total_ms"] / v["calls"] for k, v in hd.profile().items()}

    out = {}
    gen = torch.Generator(device=f"cuda:{local}")
    gen.manual_seed(99)
    eps_t = torch.randn((T, d), dtype=torch.float64, device=f"cuda:{local}", generator=gen)
    eps_e = torch.randn((T,), dtype=torch.float64, device=f"cuda:{local}", generator=gen)
    x0 = np.random.default_rng(5).standard_normal(d)
    t, k = timed(lambda: tgp.rand((eps_t, eps_e, x0), model), steps)
    out["rand"] = dict(ms=t * 1e3, steps_per_s=T / t, bytes_per_step=8 * (d + 2), kernels_ms=k)
    if d <= 6:      # a draw from the posterior without evaluating it (posterior_lti_sde.jl:48-58; tgp_posterior_rand)
        t, k = timed(lambda: tgp.rand((eps_t, eps_e, x0), tgp.posterior(model, y)), steps)
        out["posterior_rand"] = dict(ms=t * 1e3, steps_per_s=T / t, bytes_per_step=8 * (d + 3), kernels_ms=k)
    del eps_t, eps_e
    # logpdf of the posterior at the training inputs (posterior_lti_sde.jl:62-78's last line) without a posterior: tgp_pair_statistic + two
    # logpdf calls of the prior, the second on a model bound inside the call
    y_new = y + 0.3 * torch.randn((T,), dtype=torch.float64, device=f"cuda:{local}", generator=gen)
    R_new = np.array([0.05])
    t, k = timed(lambda: tgp.logpdf(tgp.replace_observation_noise_cov(tgp.posterior(model, y), R_new), y_new), steps)
    out["posterior_logpdf"] = dict(ms=t * 1e3, steps_per_s=T / t, bytes_per_step=40, kernels_ms=k,
                                   note="two logpdf launches on the prior's handle (the joint model through tgp_logpdf_noise) + the pair pass (k_pair_statistic, not in kernels_ms)")
    del y_new
    t, k = timed(lambda: tgp._filter(model, y), steps)
    out["filter"] = dict(ms=t * 1e3, steps_per_s=T / t, bytes_per_step=8 * (1 + d + d * d), kernels_ms=k)
    t, k = timed(lambda: tgp.posterior(model, y).materialise(), steps)
    out["posterior_evaluated"] = dict(ms=t * 1e3, steps_per_s=T / t, bytes_per_step=8 * (1 + d + 2 * d * d), kernels_ms=k)
    return out


def split_leg(tgp, torch, model, y, Rnew, T, steps):
    """the two passes of a step reported separately (resident data, wall clock per call), and the same two calls
    END TO END from host memory -- y uploaded over PCIe, (mean, var) returned to the host -- which is never `value`."""
    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n
    t_lp = timed(lambda: tgp.logpdf(model, y), steps)
    t_pm = timed(lambda: tgp.posterior_marginals(model, y, Rnew), steps)
    y_host = y.cpu().numpy()
    rn_host = Rnew.cpu().numpy()
    t_lp_h = timed(lambda: tgp.logpdf(model, y_host), 3)
    t_pm_fresh = timed(lambda: tgp.posterior_marginals(model, y_host, rn_host), 3)
    outs = (np.empty(T), np.empty(T))
    t_pm_h = timed(lambda: tgp.posterior_marginals(model, y_host, rn_host, out=outs), 3)
    return dict(logpdf_ms=t_lp * 1e3, posterior_marginals_ms=t_pm * 1e3, logpdf_steps_per_s=T / t_lp, posterior_marginals_steps_per_s=T / t_pm,
                host_memory=dict(logpdf_ms=t_lp_h * 1e3, posterior_marginals_ms=t_pm_h * 1e3, steps_per_s=T / (t_lp_h + t_pm_h),
                                 posterior_marginals_into_fresh_arrays_ms=t_pm_fresh * 1e3,
                                 note="inputs in pageable host memory, outputs to host arrays the caller reuses: 8 B/step in, 16 B/step out over PCIe "
                                      "(profiles/r03_host_memory.md); freshly allocated output arrays add their first-touch page faults on the caller's side"))


def cpu_gradient_baseline(name, T_sample):
    """CPU stand-in for logpdf + gradient: central finite differences of the sequential C restatement over the same 3
    hyper-parameters = 6 logpdf evaluations on one core (the reference uses reverse-mode AD of the same loop, whose
    published cost is ~5x one logpdf: README.md:79-86)."""
    from oracle import components as oc
    from oracle import seq_kalman as sk
    k, d, dt, s2 = WORKLOADS[name]
    build = lambda a, b, c: oc.build_lgssm(("scaled", a, ("stretched", b, k)), ("regular", 0.0, dt, T_sample), c)
    y = np.random.default_rng(0).standard_normal(T_sample)
    t0 = time.perf_counter()
    for i in range(3):
        for sgn in (1, -1):
            th = [1.0, 1.0, s2]
            th[i] *= 1 + sgn * 1e-5
            sk.logpdf(build(*th), y)
    t1 = time.perf_counter()
    return dict(value=T_sample / (t1 - t0), unit="Kalman steps/s", cores=1, kind="port",
                sample=f"6 sequential logpdf evaluations (central differences, 3 parameters), T={T_sample}: {t1 - t0:.3f}s")


def pmc_traffic(kname, d, layout):
    """HBM bytes per launch of `kname` from the committed PMC summary (profiles/r01_pmc_traffic.json: separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same command, FETCH doubled per
    MI355X_MICROARCH.md). None when the summary has no entry (other d / workload)."""
    for pj in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json"):         # keyed by the profile label, "d=<d>" -> label -> bytes
        p3 = os.path.join(ROOT, "profiles", pj)
        if kname.startswith(("k_steady", "k_sweep", "k_post_stream", "k_lml_stream", "k_reduce_filter", "k_apply_filter", "k_smooth<")) and os.path.exists(p3):
            ent = json.load(open(p3)).get("sweep" if kname.startswith("k_sweep") else layout, {}).get(f"d={d}", {}).get(kname)
            if ent is not None:
                return ent["hbm_bytes"]
    if kname.startswith(("k_steady", "k_sweep", "k_post_stream", "k_lml_stream")):
        return None
    path = os.path.join(ROOT, "profiles", "r02s_pmc_traffic.json")      # (r01_pmc_traffic.json: the kernels before the stationary-covariance steps)
    if not os.path.exists(path):
        return None
    table = json.load(open(path)).get(layout, {})
    lti = "true" if layout == "lti" else "false"
    base = kname.split("<")[0]
    mode = {"logpdf": 0, "filter": 1, "posterior": 2, "materialise": 3, "scratch": 4}
    if base == "k_reduce_filter":
        key = f"{base}<{d}, {lti}>"
    elif base == "k_smooth":
        key = f"{base}<{d}, {lti}, false>"      # the bench passes ONE shared R_new (RSTREAM = false)
    elif base == "k_apply_filter":
        key = f"{base}<{d}, {lti}, {mode.get(kname.split(',')[1].rstrip('>'), -1)}>"
    else:
        return None
    # kernels that exist in two builds carry one more template argument (plain / with the stationary-covariance steps): the bench
    # workload runs the latter
    ent = table.get(key[:-1] + ", true>") or table.get(key)
    return None if ent is None else ent["hbm_bytes"]


def valu_utilisation(prof, d, layout):
    """fp64 vector-ALU issue-rate utilisation of the chunk kernels: SQ_INSTS_VALU per launch (rocprofv3 PMC pass committed
    as profiles/r01_sq_counters_<layout>.json, T = 1e7) over the launch duration measured HERE, against the issue peak
    256 CUs x 4 SIMDs x one wave64 fp64 instruction per 4 cycles at 2.4 GHz (= the 78.6 TFLOP/s datasheet figure counted
    in instructions). The LTI kernels are bound by this, not by HBM."""
    p3 = os.path.join(ROOT, "profiles", f"r06_sq_counters_{layout}.json")        # keyed by the profile label
    for older in (f"r04_sq_counters_{layout}.json", f"r03_sq_counters_{layout}.json"):
        if not (os.path.exists(p3) and any(k in json.load(open(p3)).get(f"d={d}", {}) for k in prof)):
            p3 = os.path.join(ROOT, "profiles", older)
    if os.path.exists(p3) and any(k.startswith(("k_steady", "k_post_stream", "k_lml_stream")) for k in prof):
        table = json.load(open(p3)).get(f"d={d}", {})
        peak = 256 * 4 * 2.4e9 / 4.0
        out = {}
        for pk, ent in table.items():
            if pk in prof and "SQ_INSTS_VALU" in ent:
                dur = prof[pk]["total_ms"] / max(1, prof[pk]["calls"]) * 1e-3
                n = ent["SQ_INSTS_VALU"]
                out[pk] = dict(valu_wave_instructions=n, achieved=n / dur, peak=peak, unit="wave64 fp64 VALU instructions/s", frac=n / dur / peak,
                               waves=ent.get("SQ_WAVES"), wait_any_frac=ent.get("SQ_WAIT_ANY", 0.0) / max(1.0, ent.get("SQ_WAVE_CYCLES", 1.0)),
                               executed_tflops_if_every_instruction_were_an_fma=n * 64 * 2 / dur / 1e12,
                               note="EXECUTED instructions (SQ_INSTS_VALU of the committed PMC pass, profiles/) over this run's kernel time -- not the "
                                    "sequential recursion's flop count")
        return out or None
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"r02s_sq_counters_{layout}.json")
    if not os.path.exists(path):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"r01_sq_counters_{layout}.json")
    if not os.path.exists(path):
        return None
    table = json.load(open(path))
    peak = 256 * 4 * 2.4e9 / 4.0
    lti = "true" if layout == "lti" else "false"
    names = {f"k_reduce_filter<{'lti' if layout == 'lti' else 'per-step'}>": f"k_reduce_filter<{d}, {lti}>",
             f"k_apply_filter<{'lti' if layout == 'lti' else 'per-step'},logpdf>": f"k_apply_filter<{d}, {lti}, 0>",
             f"k_apply_filter<{'lti' if layout == 'lti' else 'per-step'},posterior>": f"k_apply_filter<{d}, {lti}, 2>",
             f"k_smooth<{'lti' if layout == 'lti' else 'per-step'}>": f"k_smooth<{d}, {lti}, false>"}
    out = {}
    for pk, ck in names.items():
        if ck[:-1] + ", true>" in table and layout == "lti":       # the build with the stationary-covariance steps (what the bench workload runs)
            ck = ck[:-1] + ", true>"
        if pk in prof and ck in table and "SQ_INSTS_VALU" in table[ck]:
            dur = prof[pk]["total_ms"] / max(1, prof[pk]["calls"]) * 1e-3
            n = table[ck]["SQ_INSTS_VALU"]
            out[pk] = dict(valu_wave_instructions=n, achieved=n / dur, peak=peak, unit="wave64 fp64 VALU instructions/s", frac=n / dur / peak,
                           wait_any_frac=table[ck].get("SQ_WAIT_ANY", 0.0) / max(1.0, table[ck].get("SQ_WAVE_CYCLES", 1.0)))
    return out or None


MFMA_F64_PEAK_TFS = 78.6     # MI355X datasheet fp64 matrix peak; v_mfma_f64_16x16x4_f64 measured at 64 cycles / SIMD = 77.7 TF/s (scripts/ubench_mfma_f64.hip)

# --dump-outputs: a per-step output longer than this is written as this many elements at fixed, seeded positions (2 x 8 MB for mean, var)
DUMP_SAMPLE = 1 << 20


def dump_sample(T, parts):
    """The --dump-outputs sample of a length-T output held as segments [(offset, device tensor or host array), ...]: the elements at
    DUMP_SAMPLE positions drawn once from a fixed seed (all T of them when T <= DUMP_SAMPLE), in order, as float64 on the host.
    Segments that hold none of the positions contribute an empty array (a rank of a sharded series)."""
    idx = np.arange(T) if T <= DUMP_SAMPLE else np.sort(np.random.default_rng(20240607).choice(T, DUMP_SAMPLE, replace=False))
    vals = []
    for lo, a in parts:
        sel = idx[(idx >= lo) & (idx < lo + a.shape[0])] - lo
        if hasattr(a, "index_select"):
            import torch
            vals.append(a.index_select(0, torch.from_numpy(sel).to(a.device)).cpu().numpy())
        else:
            vals.append(np.asarray(a)[sel])
    return np.concatenate(vals).astype(np.float64)


def write_outputs(dirname, arrays):
    """--dump-outputs: each array as DIR/<name>.npy in float64."""
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, f"{name}.npy"), np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64))


def respawn_under_torchrun(n):
    """`python bench.py --gpus N` as the driver calls it: become `python -m torch.distributed.run ... bench.py <same args>`."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execv(sys.executable, cmd)


def cfg5_cpu_baseline(Nr, sample_T):
    """The oracle's literal restatement of the dense recursion (predict + posterior_and_lml(SmallOutputLGC), NumPy on the
    host's BLAS threads) over a bounded number of steps of the same model."""
    from oracle import components as oc
    from oracle import lgssm_ref as ref
    r = np.linspace(-3.0, 3.0, Nr)
    model = oc.build_lgssm_separable(("se",), ("matern52",), r, ("regular", 0.0, 0.01, sample_T), 0.1)
    Y = np.random.default_rng(0).standard_normal((sample_T, Nr))
    ref.logpdf(dict(model, T=2), Y[:2])
    t0 = time.perf_counter()
    ref.logpdf(model, Y)
    dt = time.perf_counter() - t0
    return dict(value=sample_T / dt, unit="Kalman steps/s", cores=os.cpu_count(), kind="port",
                sample=f"oracle/lgssm_ref.py (NumPy / BLAS, up to {os.cpu_count()} threads), same model, {sample_T} steps: {dt:.1f}s")


def run_cfg5(args, torch, tgp, world, rank, local, emit=True):
    """BASELINE config 5: Separable(SE, Matern-5/2) on 256 spatial points x T regularly spaced times, sigma^2 = 0.1: the
    reference's dense d = 768, p = 256 model (to_gauss_markov.jl:1-20), logpdf. One bench step = one logpdf pass."""
    from temporalgps_jl_amd import lti_sde, space_time
    Nr, T = 256, args.T
    r = np.linspace(-3.0, 3.0, Nr)
    k = space_time.Separable(space_time.SEKernel(), lti_sde.Matern52Kernel())
    grid = space_time.RectilinearGrid(r, lti_sde.RegularSpacing(0.0, 0.01, T))
    model = space_time.build_lgssm(k, grid, 0.1, device=local)
    model.handle_options[tgp._lib.OPT_DENSE_STRUCTURE] = 0 if args.dense_products else 1
    hd = model.handle()
    gen = torch.Generator(device=f"cuda:{local}")
    gen.manual_seed(5 + rank)
    Y = torch.randn((T, Nr), dtype=torch.float64, device=f"cuda:{local}", generator=gen) * 0.7
    for _ in range(args.warmup):
        tgp.logpdf(model, Y)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lp = tgp.logpdf(model, Y)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt_s = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, dict(logpdf=float(lp)))
    if args.full:
        hd.set_option(tgp._lib.OPT_PROFILE, 1)
        hd.profile_reset()
        tgp.logpdf(model, Y)
        hd.set_option(tgp._lib.OPT_PROFILE, 0)
        prof = hd.profile()
    if world > 1:
        tmax = torch.tensor([dt_s], dtype=torch.float64, device=f"cuda:{local}")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt_s = float(tmax.item())
    if rank != 0:
        return
    d, p = 3 * Nr, Nr
    sec_per_step = dt_s / args.steps / T
    out = dict(
        metric="Kalman steps/sec (logpdf), separable space-time 256 spatial x T, dense d=768 p=256", value=world * T / (dt_s / args.steps),
        unit="Kalman steps/s", n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=dt_s / args.steps * 1e3,
        higher_is_better=True, scaling="weak", vs_baseline=None, dtype="f64", data="synthetic",
        config=dict(workload=f"cfg5: Separable(SE, Matern52), 256 spatial points x RegularSpacing(0,0.01,T={T}), sigma2_obs=0.1, "
                             f"ArrayStorage-equivalent dense model d=768 p=256; one logpdf pass per step; "
                             + ("dense A / H products (the reference's arithmetic)" if args.dense_products else "A = I (x) A_t, H = I (x) H_t applied in sparse form"),
                    T=T, d=d, p=p, parallelism=f"replicas x{world} (sequential in time: the dense path does not time-shard)",
                    us_per_kalman_step=sec_per_step * 1e6, logpdf=lp))
    if not args.full:
        if emit:
            print(json.dumps(out))
        return out
    # algorithmic flops of the reference's dense step: predict 2 x 2 d^3, update 2 p d^2 + 2 p^2 d + p^3 / 3 + p^2 d + 2 p d^2
    flops = {"dk_gemm<A P>": 2.0 * d ** 3, "dk_gemm<(A P) A' + Q>": 2.0 * d ** 3, "dk_gemm<H Pp>": 2.0 * p * d * d,
             "dk_gemm<V H' + R>": 2.0 * p * p * d, "dk_chol": p ** 3 / 3.0, "dk_trsm": 1.0 * p * p * d, "dk_gemm<Pp - B'B>": 2.0 * p * d * d}
    step_flops = 2 * 2.0 * d ** 3 + 2.0 * p * d * d + 2.0 * p * p * d + p ** 3 / 3.0 + p * p * d + 2.0 * p * d * d
    kernels = {kn: dict(avg_us=v["total_ms"] / max(1, v["calls"]) * 1e3, calls=v["calls"],
                        tflops=(flops[kn] / (v["total_ms"] / max(1, v["calls"]) * 1e-3) / 1e12) if kn in flops else None)
               for kn, v in prof.items()}
    dom = max(prof.items(), key=lambda kv: kv[1]["total_ms"] / max(1, kv[1]["calls"]))[0]
    gemms = {kn: v for kn, v in kernels.items() if kn.startswith("dk_gemm")}
    domg = max(gemms.items(), key=lambda kv: kv[1]["avg_us"])[0] if gemms else None
    ach = step_flops / sec_per_step / 1e12
    # what the kernels EXECUTE with A = I (x) A_t, H = I (x) H_t applied in sparse form (three non-zeros per row): the two dense products that
    # remain (B = U'\\V: p^2 d, Pp - B'B: 2 p d^2), the Cholesky factorisation and the sparse products -- 0.367 GF at d = 768, p = 256, against
    # 0.364 GF counted on the device (SQ_INSTS_VALU_MFMA_MOPS_F64 x 512: profiles/r05_sq_counters_cfg5.txt); the dense-products run executes step_flops
    exec_flops = step_flops if args.dense_products else (2 * 2.0 * 3 * d * d + 2.0 * 3 * p * d + 2.0 * 3 * p * p + p ** 3 / 3.0 + 1.0 * p * p * d + 2.0 * p * d * d)
    ach_exec = exec_flops / sec_per_step / 1e12
    out.update(
        roofline=dict(bound="mfma", kernel="whole time step (kernel chain)", achieved=ach, peak=MFMA_F64_PEAK_TFS, unit="TFLOP/s", frac=ach / MFMA_F64_PEAK_TFS,
                      traffic=None, algorithmic_flops_per_step=step_flops,
                      executed_flops_per_step=exec_flops, executed_achieved=ach_exec, executed_frac=ach_exec / MFMA_F64_PEAK_TFS,
                      note="`frac` divides the REFERENCE's dense step (2.57 GF) by the step time: flops the structured kernels do not execute. "
                           "`executed_frac`: the flops they do execute (0.37 GF per step, MFMA counter-checked) -- the utilisation figure",
                      dominant_kernel=dom, dominant_kernel_avg_us=kernels[dom]["avg_us"], dominant_kernel_tflops=kernels[dom]["tflops"],
                      dominant_gemm=domg, dominant_gemm_tflops=(gemms[domg]["tflops"] if domg else None),
                      dominant_gemm_frac=(gemms[domg]["tflops"] / MFMA_F64_PEAK_TFS if domg else None)),
        kernels=kernels)
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cfg5_cpu_baseline(Nr, 120)
    if not emit:
        return out
    print(json.dumps(out))


def other_config_legs(args, torch, tgp, local):
    """Short samples of BASELINE configs 3 and 5 inside the default line (round-5 verdict: the driver's record should see them): cfg3 = posterior
    marginals (+ logpdf) of the d = 5 / d = 6 sum kernels at T = 10^6 (the full-size runs: profiles/r06_bench_sum52_*.json), cfg5 = the dense
    d = 768, p = 256 space-time model over T = 2000 steps (full size: profiles/r06_bench_cfg5.json)."""
    import copy
    legs = {}
    for name in ("sum52_32_d5", "sum52_52s_d6"):
        try:
            T3 = 1_000_000
            model = build_model(tgp, name, T3, "lti", local)
            hd = model.handle()
            y3 = torch.randn((T3,), dtype=torch.float64, device=f"cuda:{local}")
            R3 = torch.full((1,), 1e-18, dtype=torch.float64, device=f"cuda:{local}")
            for _ in range(3):
                tgp.logpdf(model, y3)
                tgp.posterior_marginals(model, y3, R3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 10
            for _ in range(n):
                tgp.logpdf(model, y3)
                tgp.posterior_marginals(model, y3, R3)
            torch.cuda.synchronize()
            dt3 = (time.perf_counter() - t0) / n
            hd.set_option(tgp._lib.OPT_PROFILE, 1)
            hd.profile_reset()
            tgp.logpdf(model, y3)
            tgp.posterior_marginals(model, y3, R3)
            hd.set_option(tgp._lib.OPT_PROFILE, 0)
            legs[f"cfg3_{name}"] = dict(workload=f"cfg3: {name}, RegularSpacing(0,0.1,T={T3}), the reference's two calls", T=T3, ms_per_step=dt3 * 1e3,
                                        steps_per_s=T3 / dt3, kernels_ms={k: v["total_ms"] / max(1, v["calls"]) for k, v in hd.profile().items()})
            del model, y3
        except Exception as ex:      # (an extra leg: never at the cost of the line)
            legs[f"cfg3_{name}"] = dict(error=repr(ex))
    try:
        # wide states (16 < d <= 63; lti_sde.jl:377-400: ApproxPeriodicKernel() * Matern32Kernel(), d = 28): the stationary closed loop across the chip
        # (tgp_wide.hip) against the dense engine's sequential passes on one compute unit (TGP_OPT_WIDE = 0; one call of each, a 1e5-step sample)
        from temporalgps_jl_amd import lti_sde as _P
        Tw, dw = 1_000_000, 28
        spec = ("product", ("approx_periodic", 7, 1.0), ("matern32",))
        mw = _P.build_lgssm(_P.to_kernel(spec), _P.RegularSpacing(0.0, 0.1, Tw), 0.1)
        yw = torch.randn((Tw,), dtype=torch.float64, device=f"cuda:{local}")
        Rw = torch.full((1,), 1e-18, dtype=torch.float64, device=f"cuda:{local}")
        outw = (torch.empty_like(yw), torch.empty_like(yw))
        for _ in range(2):
            tgp.logpdf(mw, yw)
            tgp.posterior_marginals(mw, yw, Rw, out=outw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 10
        for _ in range(n):
            tgp.logpdf(mw, yw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n):
            tgp.posterior_marginals(mw, yw, Rw, out=outw)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        hw = mw.handle()
        hw.set_option(tgp._lib.OPT_PROFILE, 1)
        hw.profile_reset()
        tgp.logpdf(mw, yw)
        kms = {k: v["total_ms"] / max(1, v["calls"]) for k, v in hw.profile().items()}
        hw.set_option(tgp._lib.OPT_PROFILE, 0)
        Ts = 100_000
        m0 = _P.build_lgssm(_P.to_kernel(spec), _P.RegularSpacing(0.0, 0.1, Ts), 0.1)
        m0.handle_options[tgp._lib.OPT_WIDE] = 0
        tgp.logpdf(m0, yw[:Ts])
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        tgp.logpdf(m0, yw[:Ts])
        torch.cuda.synchronize()
        dense_us_per_step = (time.perf_counter() - t3) / Ts * 1e6
        lp_ms, pm_ms = (t1 - t0) / n * 1e3, (t2 - t1) / n * 1e3
        flops = 2.0 * dw * dw * Tw      # (the mean recursion's multiply-adds: the covariance half is the host plan's, data-free)
        legs["wide_d28"] = dict(workload=f"ApproxPeriodicKernel() * Matern32Kernel() (d = {dw}), RegularSpacing(0,0.1,T={Tw}), sigma2_obs=0.1", T=Tw, d=dw,
                                logpdf_ms=lp_ms, posterior_marginals_ms=pm_ms, ms_per_step=lp_ms + pm_ms, steps_per_s=Tw / ((lp_ms + pm_ms) * 1e-3),
                                kernels_ms=kms, dense_engine_logpdf_us_per_step=dense_us_per_step,
                                speedup_logpdf_vs_one_cu_pass=dense_us_per_step * Tw * 1e-3 / lp_ms,
                                roofline=dict(bound="valu", kernel="k_wide_lml4", achieved=flops / (kms.get("k_wide_lml4", lp_ms) * 1e-3) / 1e12, peak=78.6, unit="TFLOP/s",
                                              frac=flops / (kms.get("k_wide_lml4", lp_ms) * 1e-3) / 1e12 / 78.6,
                                              note="algorithmic flops 2 d^2 per step over the logpdf kernel's hipEvent duration, against the fp64 vector peak; the kernel "
                                                   "executes (1 + halo / chunk) x 32^2 / 28^2 of them (chunks of 245 steps behind 272 warm-up steps): four chunks per wave, "
                                                   "the state's components broadcast inside v_fmac_f64_dpp (8-9 cycles each, measured), DESIGN 4.4"))
        del mw, m0, yw, outw
    except Exception as ex:
        legs["wide_d28"] = dict(error=repr(ex))
    try:
        # ... and the same engine one component per lane (d <= 15): Matern52Kernel() * Matern52Kernel() (d = 9) at the headline's length
        from temporalgps_jl_amd import lti_sde as _P
        T9 = 10_000_000
        m9 = _P.build_lgssm(_P.to_kernel(("product", ("matern52",), ("matern52",))), _P.RegularSpacing(0.0, 0.1, T9), 0.1)
        y9 = torch.randn((T9,), dtype=torch.float64, device=f"cuda:{local}")
        R9 = torch.full((1,), 1e-18, dtype=torch.float64, device=f"cuda:{local}")
        out9 = (torch.empty_like(y9), torch.empty_like(y9))
        for _ in range(2):
            tgp.logpdf(m9, y9)
            tgp.posterior_marginals(m9, y9, R9, out=out9)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 10
        for _ in range(n):
            tgp.logpdf(m9, y9)
            tgp.posterior_marginals(m9, y9, R9, out=out9)
        torch.cuda.synchronize()
        dt9 = (time.perf_counter() - t0) / n
        h9 = m9.handle()
        h9.set_option(tgp._lib.OPT_PROFILE, 1)
        h9.profile_reset()
        tgp.logpdf(m9, y9)
        tgp.posterior_marginals(m9, y9, R9, out=out9)
        k9 = {k: v["total_ms"] / max(1, v["calls"]) for k, v in h9.profile().items()}
        h9.set_option(tgp._lib.OPT_PROFILE, 0)
        legs["wide_d9"] = dict(workload=f"Matern52Kernel() * Matern52Kernel() (d = 9), RegularSpacing(0,0.1,T={T9}), the reference's two calls", T=T9, d=9, ms_per_step=dt9 * 1e3,
                               steps_per_s=T9 / dt9, kernels_ms=k9,
                               note="rounds 2-5: the general chunked scan's group layout, 10.8 + 53.1 ms (scripts/r06_mid_d_time.py with TGP_WIDE=0)")
        del m9, y9, out9
    except Exception as ex:
        legs["wide_d9"] = dict(error=repr(ex))
    try:
        a5 = copy.copy(args)
        a5.T, a5.steps, a5.warmup, a5.no_cpu_baseline, a5.dense_products, a5.dump_outputs = 2000, 1, 1, True, False, None
        o5 = run_cfg5(a5, torch, tgp, 1, 0, local, emit=False)
        legs["cfg5"] = dict(workload=o5["config"]["workload"], T=2000, ms_per_step=o5["ms_per_step"], steps_per_s=o5["value"],
                            us_per_kalman_step=o5["config"]["us_per_kalman_step"], roofline=o5["roofline"],
                            kernels_us={k: v["avg_us"] for k, v in o5["kernels"].items()})
    except Exception as ex:
        legs["cfg5"] = dict(error=repr(ex))
    return legs


def run_multi_inprocess(args):
    """`python bench.py --gpus N` launched directly (no torch.distributed environment): ONE process drives the N GPUs through the
    in-library multi-GPU handle (tgp_create_multi: one device handle, HIP stream, worker thread and RCCL communicator per GPU; the
    per-segment scan elements are exchanged with ncclAllGather inside the library). Strong scaling of BASELINE config 4 by default
    (one T = 1e8, d = 4 series; --scaling weak keeps --T per GPU). `--devices 0,0` puts several ranks on one GPU (a test hook:
    the event-ordered copy transport instead of RCCL)."""
    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lti_sde
    devices = [int(x) for x in args.devices.split(",")] if args.devices else list(range(args.gpus))
    W = len(devices)
    name = args.workload
    k, d, dt, s2 = WORKLOADS[name]
    T = args.T * W if args.scaling == "weak" else args.T
    model = lti_sde.build_lgssm(lti_sde.to_kernel(k), lti_sde.RegularSpacing(0.0, dt, T), s2, device=devices[0], force_per_step=(args.layout == "per_step"))
    ms = tgp.MultiLGSSM(model, devices=devices)
    parts = []
    for r, (lo, hi) in enumerate(ms.bounds):
        gen = torch.Generator(device=f"cuda:{devices[r]}")
        gen.manual_seed(123456 + r)
        parts.append(torch.randn((hi - lo,), dtype=torch.float64, device=f"cuda:{devices[r]}", generator=gen) * 0.8)
    Rnew = np.array([1e-18])

    def step():
        return ms.logpdf_and_posterior_marginals(parts, Rnew)
    for _ in range(args.warmup):
        step()
    for dv in set(devices):
        torch.cuda.synchronize(dv)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lp, mean, var = step()
    for dv in set(devices):
        torch.cuda.synchronize(dv)
    dt_s = time.perf_counter() - t0
    if args.dump_outputs:
        write_outputs(args.dump_outputs, dict(logpdf=lp, mean=dump_sample(T, [(lo, m) for (lo, _), m in zip(ms.bounds, mean)]),
                                              var=dump_sample(T, [(lo, v) for (lo, _), v in zip(ms.bounds, var)])))
    out = dict(metric="Kalman steps/sec (logpdf + posterior marginals), T=10^7 Matern32 d=3", value=T / (dt_s / args.steps), unit="Kalman steps/s",
               n_gpus=W, steps=args.steps, warmup=args.warmup, ms_per_step=dt_s / args.steps * 1e3, higher_is_better=True, scaling=args.scaling,
               vs_baseline=None, dtype="f64", data="synthetic",
               config=dict(workload=f"{'cfg4' if name == 'sum52_12_d4' else 'cfg2'}: {name}, RegularSpacing(0,0.1,T={T}), sigma2_obs=0.1, layout={args.layout}; per step: "
                                    "logpdf AND posterior marginals of the series (one combined call: tgp_multi_logpdf_and_posterior_marginals)",
                           T=T, T_per_gpu=T // W, d=d, layout=args.layout, devices=devices,
                           parallelism=f"time-shard x{W} in ONE process (tgp_create_multi), {args.scaling}", ranks=W, backend=ms.transport, logpdf=lp))
    if not args.full:
        print(json.dumps(out))
        return
    ms.mh.set_option(tgp._lib.OPT_PROFILE, 1)
    step()
    ms.mh.set_option(tgp._lib.OPT_PROFILE, 0)
    out["kernels_rank0"] = {kk: dict(avg_ms=v["total_ms"] / max(1, v["calls"]), calls=v["calls"]) for kk, v in ms.mh.rank_profile(0).items()}
    if not args.no_single_gpu_reference and args.scaling == "strong":
        try:
            full = lti_sde.build_lgssm(lti_sde.to_kernel(k), lti_sde.RegularSpacing(0.0, dt, T), s2, device=devices[0])
            yf = torch.randn((T,), dtype=torch.float64, device=f"cuda:{devices[0]}")
            rn = torch.full((1,), 1e-18, dtype=torch.float64, device=f"cuda:{devices[0]}")
            for _ in range(2):
                tgp.logpdf_and_posterior_marginals(full, yf, rn)
            torch.cuda.synchronize(devices[0])
            t1 = time.perf_counter()
            n1 = max(2, args.steps // 4)
            for _ in range(n1):
                tgp.logpdf_and_posterior_marginals(full, yf, rn)
            torch.cuda.synchronize(devices[0])
            one = T / ((time.perf_counter() - t1) / n1)
            out["single_gpu_reference"] = dict(value=one, unit="Kalman steps/s", speedup=out["value"] / one,
                                               note="the whole series on ONE GPU with the single-GPU entry point (LTI model: the stationary-gain engine, as the shards)")
        except Exception as ex:      # noqa: BLE001
            out["single_gpu_reference"] = dict(error=repr(ex))
    print(json.dumps(out))


def run_engine_factory(args, world, rank):
    """Test hook (tests/test_bench_spawn.py): the N > 1 launch + sharding + collective path on a CPU box -- gloo backend, the
    per-segment device work supplied by `module:function` (a host emulation). Never a measurement."""
    import importlib
    import torch.distributed as dist
    from temporalgps_jl_amd import parallel
    mod, fn = args.engine_factory.split(":")
    if world == 1:   # a one-rank group: the engine interface always goes through the collectives
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    T = args.T
    seg = parallel.segment_bounds(T, world, rank)
    eng, y, Rnew = getattr(importlib.import_module(mod), fn)(args.workload, T, seg)
    shard = parallel.ShardedLGSSM(None, world, rank, engine=eng)
    for _ in range(args.warmup):
        shard.logpdf(y)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lp = shard.logpdf(y)
        shard.posterior_marginals(y, Rnew)
    if world > 1:
        dist.barrier()
    dt_s = time.perf_counter() - t0
    if rank == 0:
        print(json.dumps(dict(metric="(CPU test harness, not a measurement)", value=T / (dt_s / args.steps), unit="Kalman steps/s", n_gpus=world,
                              steps=args.steps, warmup=args.warmup, ms_per_step=dt_s / args.steps * 1e3, higher_is_better=True,
                              scaling=args.scaling, vs_baseline=None, dtype="f64", data="synthetic (host emulation engine)",
                              config=dict(workload=args.workload, T=T, ranks=world, exchange=shard.transport, backend="gloo"), logpdf=lp)))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # (defaults: 200 timed steps behind 50 untimed ones -- 22 ms of headline work; the first tens of milliseconds after an idle spell run at lower clocks:
    #  20 steps behind 3 read 0.109 - 0.111 ms per step where 400 behind 400 read 0.106 on the same box)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--T", type=int, default=None, help="series length (default: 1e7 on one GPU, 1e8 for the N > 1 strong-scaling series, 1e5 for cfg5)")
    ap.add_argument("--workload", default=None, choices=list(WORKLOADS) + ["cfg5"])
    ap.add_argument("--layout", default="lti", choices=["lti", "per_step"])
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-general-leg", action="store_true", help="skip the per-step-layout roofline leg")
    ap.add_argument("--no-single-gpu-reference", action="store_true", help="N > 1 strong scaling: skip timing the whole series on rank 0 alone")
    ap.add_argument("--model-reuse", action="store_true", help="time the headline WITH TGP_OPT_SHARED_PARTS (a per-model table reused across "
                    "the timed steps); by default that is only the extra `with_model_reuse` leg")
    ap.add_argument("--hip-graph", action="store_true", help="replay the launch chain of the repeated step from a recorded hipGraph (TGP_OPT_GRAPH)")
    ap.add_argument("--combined-call", action="store_true", help="a step = ONE tgp_logpdf_and_posterior_marginals call (the log marginal likelihood as "
                    "a by-product of the filter the posterior needs) instead of the reference's two calls; by default that is the extra `with_fused_call` leg")
    ap.add_argument("--separate-calls", action="store_true", help=argparse.SUPPRESS)      # (the default since round 5; kept so that older command lines still parse)
    ap.add_argument("--dense-products", action="store_true", help="cfg5: the reference's dense A / H products (TGP_OPT_DENSE_STRUCTURE = 0)")
    ap.add_argument("--cpu-sample", type=int, default=2_000_000)
    ap.add_argument("--torchrun", action="store_true", help="N > 1 launched directly: re-launch under torch.distributed.run (one PROCESS per GPU, collectives "
                    "through torch.distributed) instead of driving the N GPUs from this process through the in-library multi-GPU handle")
    ap.add_argument("--devices", default=None, help="in-process multi-GPU path: comma-separated device ordinals, one per rank (repeat one to share a GPU)")
    ap.add_argument("--engine-factory", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-bind", action="store_true", help="leave the process on whatever CPUs it was started on (A/B: tgp_bind_host_thread)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: per-kernel hipEvent profiles and rooflines, the other engines, "
                    "layouts and configurations, the CPU baselines and the single-GPU reference of N > 1 (off: set-up, warm-up, the timed steps, the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step returned as "
                    f"DIR/<name>.npy (float64; an output longer than {DUMP_SAMPLE} elements as a fixed, seeded sample of that many)")
    args = ap.parse_args()
    # the headline is T / (t_logpdf + t_post), the two calls the reference's API has (lti_sde.jl:60-68, posterior_lti_sde.jl:27-36)
    args.separate_calls = not args.combined_call

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    inproc = (args.gpus > 1 or args.devices) and "WORLD_SIZE" not in os.environ and not args.torchrun and not args.engine_factory and args.workload != "cfg5"
    if inproc:
        # launched directly: ONE process, the library owns the N GPUs (tgp_create_multi). The driver's torchrun launch (WORLD_SIZE set) and
        # --torchrun take the one-process-per-GPU path below.
        args.workload = args.workload or "sum52_12_d4"
        args.scaling = args.scaling or "strong"
        args.T = args.T or (10_000_000 if args.scaling == "weak" else 100_000_000)
        return run_multi_inprocess(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args.gpus)          # does not return
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # defaults: one GPU = the headline (cfg2); several GPUs = BASELINE config 4, strong scaling of one T = 1e8, d = 4 series
    if args.workload is None:
        args.workload = "matern52_d3" if world == 1 else "sum52_12_d4"
    if args.scaling is None:
        args.scaling = "weak" if (world == 1 or args.workload == "cfg5") else "strong"
    if args.T is None:
        args.T = 100_000 if args.workload == "cfg5" else (10_000_000 if (world == 1 or args.scaling == "weak") else 100_000_000)
    if args.engine_factory:
        return run_engine_factory(args, world, rank)

    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import parallel

    torch.cuda.set_device(local)
    # one process per GPU, on the CPUs next to it (tgp_bind_host_thread: a host thread on the far socket of a two-socket box pays ~13 us per headline step
    # for the call's hand-overs through pinned memory); the CPU baselines below run with the affinity the process was started with
    global _START_AFFINITY
    _START_AFFINITY = os.sched_getaffinity(0)
    host_bound = (not args.no_bind) and tgp._lib.bind_host_thread(local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    if args.workload == "cfg5":
        run_cfg5(args, torch, tgp, world, rank, local)
        if world > 1:
            dist.destroy_process_group()
        return
    T, name = (args.T * world if args.scaling == "weak" else args.T), args.workload
    d = WORKLOADS[name][1]

    # this rank's time segment (strong scaling: the T-point series is split across ranks)
    seg = parallel.segment_bounds(T, world, rank)
    Tseg = seg[1] - seg[0]
    model = build_model(tgp, name, Tseg, args.layout, local)
    hd = model.handle()
    if args.chunk:
        hd.set_option(tgp._lib.OPT_CHUNK, args.chunk)
    if args.hip_graph:
        hd.set_option(tgp._lib.OPT_GRAPH, 1)
    # The headline is timed with NOTHING carried over from one step to the next: TGP_OPT_SHARED_PARTS (pass 1 reusing a table of
    # the model's observation-independent quantities across calls on the same bound model) is switched off for it and measured
    # as an extra leg below (`with_model_reuse`), so that no step of the timed region runs on work cached by an earlier one.
    hd.set_option(tgp._lib.OPT_SHARED_PARTS, 1 if args.model_reuse else 0)
    # synthetic observations: a draw from the model, generated on the device by the product's own `rand`
    gen = torch.Generator(device=f"cuda:{local}")
    gen.manual_seed(123456 + rank)
    eps_t = torch.randn((Tseg, d), dtype=torch.float64, device=f"cuda:{local}", generator=gen)
    eps_e = torch.randn((Tseg,), dtype=torch.float64, device=f"cuda:{local}", generator=gen)
    y = tgp.rand((eps_t, eps_e, np.random.default_rng(rank).standard_normal(d)), model)
    del eps_t, eps_e
    Rnew = torch.full((1,), 1e-18, dtype=torch.float64, device=f"cuda:{local}")
    shard = parallel.ShardedLGSSM(model, world, rank)

    def step():
        # logpdf(fx, y) and marginals(posterior(fx, y)(x)) of the same series: one forward filter + RTS smoother delivers
        # both (tgp_logpdf_and_posterior_marginals); --separate-calls issues the reference's two independent calls instead
        if args.separate_calls:
            lp = shard.logpdf(y)
            if world == 1:      # (the result buffers of the previous step are reused, as in the combined call below: no allocation inside the timed region)
                mean, var = shard.posterior_marginals(y, Rnew, out=step.out)
                step.out = (mean, var)
            else:
                mean, var = shard.posterior_marginals(y, Rnew)
            return lp, mean, var
        if world == 1:
            # the result buffers of the previous step are reused (a repeated call with identical device pointers is what
            # TGP_OPT_GRAPH can replay; off by default, --hip-graph switches it on)
            res = shard.logpdf_and_posterior_marginals(y, Rnew, out=step.out)
            step.out = res[1:]
            return res
        return shard.logpdf_and_posterior_marginals(y, Rnew)

    step.out = None
    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt_s = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt_s], dtype=torch.float64, device=f"cuda:{local}")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt_s = float(tmax.item())
    if args.dump_outputs:
        # (logpdf of the whole series; mean, var: this rank's segment -> rank 0)
        lp, mean, var = last
        mv = (dump_sample(T, [(seg[0], mean)]), dump_sample(T, [(seg[0], var)]))
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, mv)
            mv = tuple(np.concatenate([p[i] for p in parts]) for i in (0, 1))
        if rank == 0:
            write_outputs(args.dump_outputs, dict(logpdf=float(lp), mean=mv[0], var=mv[1]))

    def steady_steps():
        # how many of the series' steps passes 2 / 3 of the last call ran in the mean-only form (TGP_OPT_STEADY; decided at run time, bit for bit)
        import ctypes as _ct
        st_fast, st_total = _ct.c_int64(0), _ct.c_int64(0)
        hd.check(hd.lib.tgp_steady_steps(hd.h, _ct.byref(st_fast), _ct.byref(st_total)))
        return int(st_fast.value), int(st_total.value)

    mean_only, total = steady_steps()
    out = dict(
        metric="Kalman steps/sec (logpdf + posterior marginals), T=10^7 Matern32 d=3",
        value=T / (dt_s / args.steps), unit="Kalman steps/s", n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=dt_s / args.steps * 1e3,
        higher_is_better=True, scaling=args.scaling, vs_baseline=None, dtype="f64", data="synthetic",
        config=dict(workload=f"{'cfg4' if (world > 1 and name == 'sum52_12_d4') else 'cfg2'}: {name}, RegularSpacing(0,0.1,T={T}), sigma2_obs=0.1, "
                             f"layout={args.layout}; per step: logpdf AND posterior marginals of the series "
                             + ("(the reference's two calls: logpdf(fx, y), then marginals(posterior(fx, y)(x)) -- value = T / (t_logpdf + t_post), SURVEY.md 8d)"
                                if args.separate_calls else "(one combined call: tgp_logpdf_and_posterior_marginals)"),
                    T=T, T_per_gpu=Tseg, d=d, calls=("separate" if args.separate_calls else "combined"),
                    layout=args.layout, host_thread_bound_to_gpu_socket=bool(host_bound),
                    parallelism=f"time-shard x{world} ({args.scaling}: {'T per GPU fixed' if args.scaling == 'weak' else 'total T fixed'})",
                    ranks=world, backend=("rccl" if world > 1 else "none"), exchange=shard.transport,
                    hip_graph_replays=int(hd.lib.tgp_graph_replays(hd.h)),
                    stationary_covariance_steps=dict(
                        mean_only=mean_only, total=total,
                        note="steps served with the stationary gains: every step behind the head of n0 steps over which the filter covariance "
                             "is iterated until it no longer changes (on the host, inside every timed call: tgp_steady_plan.hpp; nothing is carried "
                             "over between calls). `with_five_launch_engine`: round 3's form of the same engine; `with_general_engine` / "
                             "`with_full_steps`: the same steps on the general engine (--full)")))
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return
    # per-kernel durations: the SAME K steps once more with every launch bracketed by hipEvents on the
    # handle's stream (kept out of the timed region above: two event records per launch slow the host
    # enqueue enough to open gaps between the ~20-300 us kernels).
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    prof_all = hd.profile()
    # ... and once more step by step: the spread of each kernel's duration over the K steps (a kernel that waits for the host -- flags in pinned
    # memory, tables pulled over PCIe -- shows it here: round-4 verdict, item 2b)
    per_step_ms = {}
    for _ in range(args.steps):
        hd.profile_reset()
        step()
        torch.cuda.synchronize()
        for kk, vv in hd.profile().items():
            per_step_ms.setdefault(kk, []).append(vv["total_ms"] / max(1, vv["calls"]))
    hd.profile_reset()
    # what the hipEvent bracket itself reads: an EMPTY kernel inside the same bracket on the same stream (tgp_profile_empty_launch). rocprofv3's kernel
    # trace times the kernel alone, so its durations (profiles/*_kernel_stats.md) stand this much below the hipEvent ones above
    for _ in range(30):
        hd.check(hd.lib.tgp_profile_empty_launch(hd.h))
    _pe = hd.profile().get("k_empty")
    event_bracket_ms = (_pe["total_ms"] / max(1, _pe["calls"])) if _pe else None
    hd.profile_reset()
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    fused = None
    if world == 1 and args.separate_calls:
        def fused_step():
            res = shard.logpdf_and_posterior_marginals(y, Rnew, out=fused_step.out)
            fused_step.out = res[1:]
        fused_step.out = None
        for _ in range(max(2, args.warmup)):
            fused_step()
        torch.cuda.synchronize()
        tf0 = time.perf_counter()
        for _ in range(args.steps):
            fused_step()
        torch.cuda.synchronize()
        dt_f = (time.perf_counter() - tf0) / args.steps
        fused = dict(value=T / dt_f, ms_per_step=dt_f * 1e3,
                     note="ONE tgp_logpdf_and_posterior_marginals call per step: the log marginal likelihood is a by-product of the filter the posterior "
                          "needs anyway (a convenience the reference's API does not have; rounds 1-4 quoted this as `value`)")
    mean_only, total = steady_steps()
    out["config"]["stationary_covariance_steps"].update(mean_only=mean_only, total=total)
    prof = prof_all
    steady_engine = any(k.startswith("k_steady") for k in prof)

    def timed_leg(option_value):
        """the same K steps with TGP_OPT_STEADY = option_value (1: the general chunked-scan engine with its per-chunk stationary steps,
        0: the general engine with every step in full)"""
        hd.set_option(tgp._lib.OPT_STEADY, option_value)
        for _ in range(max(2, args.warmup)):
            step()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt_n = time.perf_counter() - t1
        if world > 1:
            tn = torch.tensor([dt_n], dtype=torch.float64, device=f"cuda:{local}")
            dist.all_reduce(tn, op=dist.ReduceOp.MAX)
            dt_n = float(tn.item())
        return dict(value=T / (dt_n / args.steps), ms_per_step=dt_n / args.steps * 1e3)

    general, no_steady, five = None, None, None
    if mean_only > 0 and args.layout == "lti":
        if any(k.startswith("k_steady_one") for k in prof):
            five = dict(timed_leg(2), note="TGP_OPT_STEADY = 2: round 3's form of the stationary-gain engine (set-up kernel, two passes over y, carry "
                                           "and reduction kernels: five launches)")
        if steady_engine:
            general = dict(timed_leg(1), note="TGP_OPT_STEADY = 1: the general chunked-scan engine (round 2's path: full Kalman / RTS steps per chunk, "
                                              "mean-only once a chunk's covariance repeats bit for bit); agrees with the headline path to rounding")
        no_steady = dict(timed_leg(0), note="TGP_OPT_STEADY = 0: the general engine with every step in full (what a model with per-step blocks, per-step "
                                            "noise or missing data gets)")
        hd.set_option(tgp._lib.OPT_STEADY, 3)
    reuse = None

    if rank == 0:
        value = out["value"]
        # roofline of the dominant kernel (by accumulated hipEvent time in the timed region)
        dom = max(prof.items(), key=lambda kv: kv[1]["total_ms"]) if prof else None
        lti = args.layout == "lti"
        bytes_per_step_in = 8 if lti else 8 * (2 * d * d + 2 * d + 3)
        roof = None
        if dom is not None:
            kname, st = dom
            avg_ms = st["total_ms"] / max(1, st["calls"])
            # algorithmic bytes per time step of the PATH the kernel belongs to:
            #   logpdf: inputs only; posterior marginals: inputs + R_new + (mean, var) out
            per_unit = bytes_per_step_in + (24 if ("posterior" in kname or "smooth" in kname) and not lti else 0)
            if lti and ("posterior" in kname or "smooth" in kname or kname.startswith("k_post_stream")):
                per_unit = 24
            ach = per_unit * Tseg / (avg_ms * 1e-3) / 1e9
            traffic = pmc_traffic(kname, d, args.layout) if (T == 10_000_000 and world == 1) else None
            smp = sorted(per_step_ms.get(kname, [avg_ms]))
            roof = dict(bound="hbm", kernel=kname, achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS,
                        kernel_ms_min_median_max=[smp[0], smp[len(smp) // 2], smp[-1]],
                        frac_min_median_max=[per_unit * Tseg / (v * 1e-3) / 1e9 / HBM_PEAK_GBS for v in (smp[-1], smp[len(smp) // 2], smp[0])],
                        traffic=traffic, traffic_unit="bytes per launch (rocprofv3 PMC: 2*FETCH_SIZE + WRITE_SIZE, profiles/)",
                        algorithmic_bytes=per_unit * Tseg, avg_kernel_ms=avg_ms, algorithmic_bytes_per_step=per_unit,
                        note=(("stationary-gain engine, STREAMING posterior kernel (DESIGN 3.20): ONE kernel per call, 2048 persistent waves, each a run of "
                               "1024-step tiles; reads y once (8 B/step) plus one halo per run, writes mean, var (16 B/step); nothing else of size T moves "
                               "(`traffic` = PMC bytes of this kernel)" if kname.startswith("k_post_stream") else
                               "stationary-gain engine, one-launch form (DESIGN 3.13): ONE kernel per call reads y once (8 B/step, plus the workgroups' "
                               "halos out of L2) and writes mean, var (16 B/step); nothing else of size T moves, no other kernel runs "
                               "(`traffic` = PMC bytes of this kernel)" if kname.startswith("k_steady_one") else
                               "no modal form (a defective closed loop): ONE kernel per call on DENSE powers of the closed loop and of the settled "
                               "reverse-time transition (DESIGN 3.15); reads y once, writes mean, var once -- bound by its fp64 instruction stream "
                               "(~230 FMAs per step at d = 6), not by HBM" if kname.startswith("k_smooth_one") else
                               "stationary-gain engine (DESIGN 3.11): the output pass reads y (8 B/step) and writes mean, var (16 B/step), nothing else "
                               "of size T moves; pass 1 reads y once more (`traffic` = PMC bytes of this kernel alone)" if kname.startswith("k_steady") else
                               "LTI (Fill) layout, general engine: streams only y in / (mean,var) out (plus the smoother scratch: `traffic`): the launch "
                               "is not HBM bound -- one wave per SIMD, it lasts as long as the dependent fp64 chain of its slowest wave (DESIGN 3.10)")
                              if lti else "per-step layout: HBM bound"))
        def net_of_bracket(r, nbytes):
            # (beside `frac`, never instead of it: `frac` stays the plain hipEvent figure)
            if r is None or event_bracket_ms is None:
                return
            net = r["avg_kernel_ms"] - event_bracket_ms
            r["event_bracket_ms"] = event_bracket_ms
            r["frac_net_of_event_bracket"] = (nbytes / (net * 1e-3) / 1e9 / HBM_PEAK_GBS) if net > 0 else None
            r["event_bracket_note"] = ("an EMPTY kernel inside the same hipEvent bracket reads event_bracket_ms; rocprofv3 --kernel-trace times the kernel alone "
                                       "(profiles/r06_lti_kernel_stats.md), so its average sits about that far below avg_kernel_ms and corresponds to "
                                       "frac_net_of_event_bracket")
        if roof is not None:
            net_of_bracket(roof, roof["algorithmic_bytes"])
        roof_lp = None
        lp_names = [k for k in prof if k.startswith("k_lml_stream") or (k.startswith("k_steady_one") and "logpdf" in k)]
        if lti and lp_names and roof is not None and lp_names[0] != roof["kernel"]:
            kn = lp_names[0]
            smp = sorted(per_step_ms.get(kn, [prof[kn]["total_ms"] / max(1, prof[kn]["calls"])]))
            avg = prof[kn]["total_ms"] / max(1, prof[kn]["calls"])
            ach_lp = 8 * Tseg / (avg * 1e-3) / 1e9
            roof_lp = dict(bound="hbm", kernel=kn, achieved=ach_lp, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach_lp / HBM_PEAK_GBS,
                           kernel_ms_min_median_max=[smp[0], smp[len(smp) // 2], smp[-1]], avg_kernel_ms=avg, algorithmic_bytes=8 * Tseg,
                           algorithmic_bytes_per_step=8, traffic=pmc_traffic(kn, d, args.layout) if (T == 10_000_000 and world == 1) else None,
                           note="the logpdf call's ONE kernel: reads y once (8 B/step), writes nothing of size T; 80 MB per launch -- a launch this short "
                                "is bound by its fp64 instruction stream and its ramps as much as by HBM (DESIGN 3.19)")
        net_of_bracket(roof_lp, 8 * Tseg)
        out["config"]["hip_graph_replays"] = int(hd.lib.tgp_graph_replays(hd.h))
        out["config"]["pass1"] = ("shared matrix parts (TGP_OPT_SHARED_PARTS): the observation-independent half of the chunk recursion is tabulated "
                                  "once per bound model -- on a side stream, launched by the second call, 1.4 ms at d = 3 -- and reused by later "
                                  "calls on the same model; the warm-up steps bind and warm the model, the timed steps reuse the table"
                                  if any("shared parts" in k for k in prof) else "general")
        out["roofline"] = roof
        out["kernels"] = {k: dict(avg_ms=v["total_ms"] / max(1, v["calls"]), calls=v["calls"]) for k, v in prof.items()}
        if roof_lp is not None:
            out["roofline_logpdf_kernel"] = roof_lp
        if fused is not None:
            out["with_fused_call"] = fused
        if five is not None:
            out["with_five_launch_engine"] = five
        if general is not None:
            out["with_general_engine"] = general
        if no_steady is not None:
            out["with_full_steps"] = no_steady
        if world > 1 and args.scaling == "strong" and not args.no_single_gpu_reference:
            # the SAME series on rank 0 alone (the other ranks idle): what the strong-scaling speed-up is measured against
            try:
                full = build_model(tgp, name, T, args.layout, local)
                yf = torch.randn((T,), dtype=torch.float64, device=f"cuda:{local}")
                for _ in range(2):
                    tgp.logpdf(full, yf)
                    tgp.posterior_marginals(full, yf, Rnew)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                n1 = max(2, args.steps // 4)
                for _ in range(n1):
                    tgp.logpdf(full, yf)
                    tgp.posterior_marginals(full, yf, Rnew)
                torch.cuda.synchronize()
                one = T / ((time.perf_counter() - t1) / n1)
                out["single_gpu_reference"] = dict(value=one, unit="Kalman steps/s", speedup=value / one,
                                                   note="the whole T-point series on rank 0 alone, same process, same kernels")
                del full, yf
            except Exception as ex:      # noqa: BLE001 -- e.g. the whole series does not fit one GPU
                out["single_gpu_reference"] = dict(error=repr(ex))
        if args.layout == "lti":
            # The LTI layout streams 8-24 B per step against ~10^2-10^3 flop: its binding roofline is the fp64 vector ALU, not HBM.
            # (round 6: the `roofline_fp64_valu` entry of rounds 3-5 charged the SEQUENTIAL recursion's flops to kernels that execute an O(d) modal
            #  recursion -- not evidence, the round-5 verdict said; `valu` below counts the instructions the kernels EXECUTE)
            pass
        if T == 10_000_000 and world == 1 and d == 3 and not args.chunk:
            out["valu"] = valu_utilisation(prof, d, args.layout)
        if world == 1 and not args.no_general_leg:
            out["split"] = split_leg(tgp, torch, model, y, Rnew, T, max(3, args.steps // 2))
        if args.layout == "lti" and world == 1 and not args.no_general_leg:
            try:
                out["lti_interface"] = lti_interface_leg(tgp, torch, model, y, T, d, local, max(3, args.steps // 2))
            except Exception as ex:      # (an extra leg: never at the cost of the line)
                out["lti_interface"] = dict(error=repr(ex))
            out["logpdf_and_grad"] = gradient_leg(tgp, torch, name, T, d, local, max(3, args.steps // 2), y)
            if not args.no_cpu_baseline:
                out["logpdf_and_grad"]["cpu_baseline"] = cpu_gradient_baseline(name, args.cpu_sample)
            out["roofline_general_layout"] = general_layout_leg(tgp, torch, name, T, d, local, max(3, args.steps // 2))
            try:
                out["predict_path"] = predict_path_legs(tgp, torch, name, T, d, local, max(3, args.steps // 2))
                for kk in ("missing_10pct", "per_step_noise", "irregular_spacing"):      # (top level: what the round-4 verdict asked to see in the driver's line)
                    out[kk] = {q: out["predict_path"][kk][q] for q in ("ms_per_step", "steps_per_s", "roofline", "engine", "workload") if q in out["predict_path"][kk]}
                    out[kk]["general_engine_ms_per_step"] = out["predict_path"][kk]["general_engine"]["ms_per_step"]
            except Exception as ex:      # (an extra leg: never at the cost of the line)
                out["predict_path"] = dict(error=repr(ex))
            if name == "matern52_d3" and T == 10_000_000:
                out["other_configs"] = other_config_legs(args, torch, tgp, local)
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(name, args.cpu_sample)
            if world == 1 and args.layout == "lti":
                try:
                    bound_to = os.sched_getaffinity(0)
                    os.sched_setaffinity(0, _START_AFFINITY)      # (every core the process was given, not only the GPU's socket)
                    try:
                        out["cpu_baseline_all_cores"] = cpu_baseline_all_cores(name, args.cpu_sample * 4)
                    finally:
                        os.sched_setaffinity(0, bound_to)
                except Exception as ex:      # noqa: BLE001 -- no g++ / OpenMP on the host: the one-core baseline stands alone
                    out["cpu_baseline_all_cores"] = dict(error=repr(ex))
        if "split" in out:
            # informational only (vs_baseline stays null: the reference publishes no number for the combined metric): what its
            # README plots show for the two quantities it did time, read off the axes (unstated CPU, 1 thread)
            pub = dict(source="BASELINE.md section 1 (reference README plots, approximate)", logpdf_steps_per_s=[2e7, 5e7],
                       logpdf_and_gradient_steps_per_s=[4e6, 1e7])
            pub["logpdf_speedup"] = [out["split"]["logpdf_steps_per_s"] / v for v in pub["logpdf_steps_per_s"][::-1]]
            if "logpdf_and_grad" in out:
                pub["logpdf_and_gradient_speedup"] = [out["logpdf_and_grad"]["value"] / v for v in pub["logpdf_and_gradient_steps_per_s"][::-1]]
            out["published_reference"] = pub
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
