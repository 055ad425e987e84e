"""Wall time of logpdf + gradient of a GP with state dimension 5 .. 8 on a regular grid with missing observations by ONE adjoint pass on the group sweep
(logpdf_and_gradient(method="sweep") -> tgp_logpdf_adjoint_group -> k_sweep_group_adjoint) beside (a) the tangent scans for the same call on
the same series in the same process (method="tangent": one dual-number pass of the general engine per hyper-parameter -- the route these calls have
without the kernel) and (b) k_sweep_group<lti,posterior> on the same series (TGP_OPT_SWEEP = 2), the yardstick for the kernel: the same forward half, the
RTS step in place of the adjoint step.  tests/_sweep_group.py's kernels, every Matern term with a variance and an inverse length scale of its own (at their
neutral values 1: the same model) beside the noise variance: 5 parameters at d = 5, 6 and 7 at d = 7, 8.  The protocol of scripts/time_sweep_adjoint.py:
device-resident series, 10 % of the steps missing, medians of --reps calls after --warm calls with min and max; per-kernel times of one more call from
tgp_profile_get.  Writes profiles/sweep_group_adjoint_time.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADJOINT, POSTERIOR = "k_sweep_group_adjoint<lti>", "k_sweep_group<lti,posterior>"


def with_parameters(spec):
    """("sum", term, ...) with every term as ("scaled", 1, ("stretched", s, Matern)): the same kernel, a variance and an inverse length scale per term"""
    terms = []
    for t in spec[1:]:
        s, base = (t[1], t[2]) if t[0] == "stretched" else (1.0, t)
        terms.append(("scaled", 1.0, ("stretched", s, base)))
    return ("sum",) + tuple(terms)


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


def profiled(tgp, hd, fn):
    import torch
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_group_adjoint_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lti_sde as P
    from tests._sweep_group import KERNELS
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        k, dt, s2 = KERNELS[d]
        fx = P.to_sde(P.GP(P.to_kernel(with_parameters(k))))(P.RegularSpacing(0.0, dt, T), s2)
        dm = fx.build_lgssm()
        assert dm.dim == d
        rng = np.random.default_rng(d)
        y = rng.standard_normal(T) * np.sqrt(1.0 + s2)
        missing = rng.random(T) < 0.1
        obs = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        out = dict(d=d, T=T, missing=0.1, reps=args.reps, warm=args.warm)
        res = {}
        for tag in ("sweep", "tangent"):
            call = lambda: res.__setitem__(tag, P.logpdf_and_gradient(fx, obs, method=tag))      # noqa: E731
            out[tag] = timed(call, args.reps, args.warm)
            if tag == "sweep":
                out["info"] = dm.handle().sweep_info()
                assert out["info"]["served"] == 1, out["info"]
            out[tag]["kernels_ms"] = profiled(tgp, dm.handle(), call)
            assert (ADJOINT in out[tag]["kernels_ms"]) == (tag == "sweep"), out[tag]["kernels_ms"]
        (lp_s, g_s), (lp_t, g_t) = res["sweep"], res["tangent"]
        scale = max(abs(v) for v in g_t.values())
        out["parameters"] = len(g_t)
        out["gradient_deviation"] = float(max(abs(g_s[n] - g_t[n]) for n in g_t) / scale)
        out["logpdf_deviation"] = float(abs(lp_s - lp_t) / abs(lp_t))
        dm.handle().set_option(tgp._lib.OPT_SWEEP, 2)      # (the posterior kernel is not on the default route at these d)
        post = lambda: tgp.logpdf_and_posterior_marginals(dm, obs, Rn)      # noqa: E731
        out["posterior_marginals"] = timed(post, args.reps, args.warm)
        out["posterior_marginals"]["kernels_ms"] = profiled(tgp, dm.handle(), post)
        assert POSTERIOR in out["posterior_marginals"]["kernels_ms"], out["posterior_marginals"]
        out["tangent_over_sweep"] = round(out["tangent"]["median_ms"] / out["sweep"]["median_ms"], 2)
        out["adjoint_kernel_over_posterior_kernel"] = round(out["sweep"]["kernels_ms"][ADJOINT] / out["posterior_marginals"]["kernels_ms"][POSTERIOR], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del obs, fx, dm
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_group_adjoint.py: wall ms (median, min, max of `reps` calls after `warm`) of logpdf_and_gradient, device-resident series,\n"
                    "# regular grid, 10 % of the steps missing.  sweep: ONE adjoint pass on k_sweep_group_adjoint; tangent: the tangent scans of the general engine\n"
                    "# (one pass per hyper-parameter) on the same series in the same process; posterior_marginals: k_sweep_group<lti,posterior> on the same series.\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
