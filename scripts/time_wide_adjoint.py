"""Wall time of logpdf_and_gradient(method="adjoint") on the wide-state engine against method="fd" and against logpdf alone (one process, device-resident
y, medians of --reps calls after a warm-up), for d = 9 at T = 1e7 and d = 28, 42 at T = 1e6; the plan and host-finish figures come from the engine's
TGP_STEADY_DEBUG line of one more adjoint call (stderr).  Per-kernel times: run under rocprofv3 --kernel-trace --stats (a separate run)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model(P, d, T):
    if d == 9:
        k = 0.8 * (P.Matern52Kernel() * P.Matern52Kernel().stretch(0.7))
    elif d == 28:
        k = 1.4 * (P.ApproxPeriodicKernel(7, 1.1).stretch(0.8) * P.Matern32Kernel().stretch(0.3))
    else:
        k = 1.4 * (P.ApproxPeriodicKernel(7, 1.1).stretch(0.8) * P.Matern52Kernel().stretch(0.3))
    fx = P.to_sde(P.GP(0.25, k))(P.RegularSpacing(0.0, 0.05, T), 0.1)
    assert fx.build_lgssm().dim == d
    return fx


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="9:10000000,28:1000000,42:1000000")
    args = ap.parse_args()
    import numpy as np
    import torch
    from temporalgps_jl_amd import lti_sde as P
    for case in args.cases.split(","):
        d, T = (int(v) for v in case.split(":"))
        fx = model(P, d, T)
        rng = np.random.default_rng(d)
        y = torch.as_tensor(np.sin(np.arange(T) * 0.3) + rng.standard_normal(T) * 0.3, device="cuda")
        out = dict(d=d, T=T, params=len(P.parameters(fx.f.f.kernel)) + 2)
        out["adjoint_ms"] = med_ms(lambda: P.logpdf_and_gradient(fx, y, method="adjoint"), args.reps)
        out["fd_ms"] = med_ms(lambda: P.logpdf_and_gradient(fx, y, method="fd"), max(1, args.reps // 2))
        out["logpdf_ms"] = med_ms(lambda: P.logpdf(fx, y), args.reps)
        out["adjoint_over_fd"] = out["adjoint_ms"] / out["fd_ms"]
        print(json.dumps(out), flush=True)
        os.environ["TGP_STEADY_DEBUG"] = "1"
        P.logpdf_and_gradient(fx, y, method="adjoint")
        del os.environ["TGP_STEADY_DEBUG"]
        sys.stderr.flush()


if __name__ == "__main__":
    main()
