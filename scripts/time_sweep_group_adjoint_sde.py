"""Wall time of logpdf + block gradients of an SDE-described model with state dimension 5 .. 8 on irregular time stamps by ONE adjoint pass on the group
sweep (lgssm.logpdf_adjoint_group_sde -> tgp_logpdf_adjoint_group_sde -> k_sweep_group_adjoint<sde>), on a model bound ONCE (the binding's
upload of the time stamps is not in the figure).  Beside it, in the same process: (a) central differences of tgp_logpdf on the same bound model -- 2 x the
number of hyper-parameters calls on the route they take by default, the only device gradient these models had; (b) the kernel times, from the profile, of
k_sweep_group<sde,posterior> on the same model (TGP_OPT_SWEEP = 2) and of k_sweep_group_adjoint<lti> at the same d and T on a regular grid: yardsticks for
the kernel itself.  tests/_sweep_group.py's kernels with a variance and an inverse length scale per Matern term beside the noise variance: 5 parameters at
d = 5, 6 and 7 at d = 7, 8.  Device-resident series, gaps U(0.05, 0.15), 10 % of the steps missing, medians of --reps calls after --warm calls with min
and max.  Writes profiles/sweep_group_adjoint_sde_time.txt."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_sweep_group_adjoint import profiled, timed, with_parameters      # noqa: E402

ADJOINT, POSTERIOR, ADJOINT_LTI = "k_sweep_group_adjoint<sde>", "k_sweep_group<sde,posterior>", "k_sweep_group_adjoint<lti>"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--cases", default="5:1000000,6:1000000,7:1000000,8:1000000,5:10000000,6:10000000,7:10000000,8:10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_group_adjoint_sde_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lgssm as L
    from temporalgps_jl_amd import lti_sde as P
    from tests._sweep_group import KERNELS
    lines = []
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        k, dt, s2 = KERNELS[d]
        kern = P.to_kernel(with_parameters(k))
        nparams = len(P.parameters(kern)) + 1
        rng = np.random.default_rng(d)
        t = np.cumsum(rng.uniform(0.5 * dt, 1.5 * dt, T))
        y = rng.standard_normal(T) * np.sqrt(1.0 + s2)
        missing = rng.random(T) < 0.1
        obs = (torch.from_numpy(np.where(missing, 0.0, y)).cuda(), torch.from_numpy(missing).cuda())
        dm = P.build_lgssm(kern, t, s2, device_components=True)
        assert dm.dim == d and isinstance(dm.transitions, L.SDETransitions)
        hd = dm.handle()
        out = dict(d=d, T=T, missing=0.1, parameters=nparams, reps=args.reps, warm=args.warm)
        adj = lambda: L.logpdf_adjoint_group_sde(dm, obs)      # noqa: E731
        out["adjoint"] = timed(adj, args.reps, args.warm)
        out["info"] = hd.sweep_info()
        assert out["info"]["served"] == 1, out["info"]
        out["adjoint"]["kernels_ms"] = profiled(tgp, hd, adj)
        assert set(out["adjoint"]["kernels_ms"]) == {ADJOINT}, out["adjoint"]["kernels_ms"]
        fd = lambda: [tgp.logpdf(dm, obs) for _ in range(2 * nparams)]      # noqa: E731
        out["central_differences"] = timed(fd, args.reps, args.warm)
        out["central_differences"]["kernels_ms"] = profiled(tgp, hd, lambda: tgp.logpdf(dm, obs))
        hd.set_option(tgp._lib.OPT_SWEEP, 2)      # (the posterior kernel is not on the default route at these d)
        Rn = torch.full((1,), 1e-6, dtype=torch.float64, device="cuda")
        post = lambda: tgp.logpdf_and_posterior_marginals(dm, obs, Rn)      # noqa: E731
        post()
        out["posterior_kernel_ms"] = profiled(tgp, hd, post)[POSTERIOR]
        reg = P.to_sde(P.GP(kern))(P.RegularSpacing(0.0, dt, T), s2).build_lgssm()
        lti = lambda: L.logpdf_adjoint_group(reg, obs)      # noqa: E731
        lti()
        out["lti_adjoint_kernel_ms"] = profiled(tgp, reg.handle(), lti)[ADJOINT_LTI]
        out["differences_over_adjoint"] = round(out["central_differences"]["median_ms"] / out["adjoint"]["median_ms"], 2)
        out["adjoint_kernel_over_posterior_kernel"] = round(out["adjoint"]["kernels_ms"][ADJOINT] / out["posterior_kernel_ms"], 2)
        out["adjoint_kernel_over_lti_adjoint_kernel"] = round(out["adjoint"]["kernels_ms"][ADJOINT] / out["lti_adjoint_kernel_ms"], 2)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del obs, dm, reg
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# scripts/time_sweep_group_adjoint_sde.py: wall ms (median, min, max of `reps` calls after `warm`), device-resident series, gaps U(0.05, 0.15),\n"
                    "# 10 % of the steps missing, the model bound once.  adjoint: ONE pass of k_sweep_group_adjoint<sde>; central_differences: 2 x parameters calls\n"
                    "# of tgp_logpdf on the same bound model (default route); posterior_kernel_ms / lti_adjoint_kernel_ms: k_sweep_group<sde,posterior> on the same\n"
                    "# model and k_sweep_group_adjoint<lti> at the same d and T on a regular grid, from the profile.\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
