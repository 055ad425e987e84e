"""The dense engine's passes across the chip (csrc/tgp_dense_chunked.hpp), restated in NumPy on top of oracle/lgssm_ref.py: what the kernels
compute, chunk by chunk, with nothing of their layout.

Forward: chunk c owns the steps [s_c, s_c+1), s_c = c C.  It starts at max(0, s_c - W) from the model's x0 and records nothing before s_c; at s_c it keeps
the state its warm-up reached, at s_c+1 the state its own run reached.  Hand-over c compares chunk c's warm-up state with chunk c - 1's end state: largest
|difference| over the largest |entry| of the end state (P and m together).  Chunk 0 is exact, so by induction every chunk whose hand-over passes started from
(nearly) the sequential state.

Backward (modified Bryson-Frazier, ref.bryson_frazier_marginals is the sequential form): chunk c starts at min(T, s_c+1 + Wb) from (lambda, Lambda) = 0, moves
the adjoints only until it reaches s_c+1 - 1, keeps the pair it has there, writes its own steps' marginals, and keeps the pair it carries out of step s_c.
Hand-over c compares chunk c's warm-up pair with the pair chunk c + 1 carried out.

run(): a pass whose check fails (forwards 1e-12, backwards 1e-11) is repeated with the warm-up doubled while C >= 2 W; beyond that, or with a forced
geometry, the call is declined (the device then runs its sequential passes).

Scalar observations (the models to_sde builds); the device applies vector observations as p scalar updates of the same form.

usage: dense_chunk_proto.py        prints, per test model, the hand-over distances at the geometry tests/test_gpu_dense_chunked.py forces"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import components as oc  # noqa: E402
from oracle import lgssm_ref as ref  # noqa: E402

TOL_F, TOL_B = 1e-12, 1e-11
LOG2PI = np.log(2.0 * np.pi)

# product kernels (lti_sde.jl:377-400) of the state dimensions the three instantiations DP = 32, 48, 64 serve
KERNELS = {
    18: ("product", ("approx_periodic", 3, 1.0), ("matern52",)),
    28: ("product", ("approx_periodic", 7, 1.0), ("matern32",)),
    42: ("product", ("approx_periodic", 7, 1.0), ("matern52",)),
    54: ("product", ("approx_periodic", 9, 1.0), ("matern52",)),
}
# d: (T, input spacing, noise variance, steps per chunk, W, Wb) -- chosen here so that the restatement passes both checks with no repair
# (test_dense_chunk_proto.py asserts it); the GPU tests force the same values.  A larger spacing makes a product kernel forget faster.
GEOMETRY = {
    18: (4100, 0.2, 0.1, 530, 128, 128),
    28: (4100, 0.2, 0.1, 530, 128, 128),
    42: (4100, 0.2, 0.1, 530, 128, 128),
    54: (4100, 0.2, 0.1, 530, 128, 128),
}


def test_model(d):
    T, dt, s2, C, W, Wb = GEOMETRY[d]
    return oc.build_lgssm(KERNELS[d], ("regular", 0.0, dt, T), s2), (C, W, Wb)


def test_series(model, seed, frac_missing=0.1, per_step_noise=False):
    """a draw of the model, a mask with frac_missing of the steps missing, optionally a noise variance per step"""
    T, d = model["T"], len(model["x0m"])
    rng = np.random.default_rng(seed)
    y = np.asarray(ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))).reshape(T)
    missing = rng.random(T) < frac_missing
    if per_step_noise:
        model = dict(model, R=(float(np.ravel(model["R"])[0]) * (0.5 + rng.random(T))).reshape((T,) + np.shape(model["R"])[1:]))
    return model, y, missing


def _step(model, t, m, P, y, miss):
    """predict + the scalar update of step t (lgc.jl:46-52, 247-257; a missing step as y := 0, R := 1e15, missings.jl:25-53)"""
    A, a, Q = ref.transition(model, t)
    H, h, R = ref.emission(model, t)
    H = np.ravel(H)
    m = A @ m + np.ravel(a)
    P = A @ P @ A.T + Q
    v = P @ H
    s = H @ v + (ref.LARGE_VAR if miss else float(np.ravel(R)[0]))
    nu = (0.0 if miss else y) - H @ m - float(np.ravel(h)[0])
    lml = -0.5 * (LOG2PI + np.log(s) + nu * nu / s) + (0.5 * (LOG2PI + np.log(ref.LARGE_VAR)) if miss else 0.0)
    return m + v * nu / s, P - np.outer(v, v) / s, (v, s, nu), lml


def _dist(x, r):
    return float(np.max(np.abs(x - r)) / max(np.max(np.abs(r)), 1e-300))


def forward(model, ys, missing, C, W):
    T = model["T"]
    n = -(-T // C)
    lml, rec, mf, Pf = np.zeros(n), [None] * T, [None] * T, [None] * T
    warm, fin = [None] * n, [None] * n
    for c in range(n):
        s0, s1 = c * C, min(T, (c + 1) * C)
        m, P = model["x0m"].copy(), model["x0P"].copy()
        for t in range(max(0, s0 - W), s1):
            if t == s0 and t > max(0, s0 - W):
                warm[c] = np.concatenate([P.ravel(), m])
            m, P, upd, term = _step(model, t, m, P, ys[t], bool(missing[t]))
            if t >= s0:              # (a warm-up step records nothing)
                lml[c] += term
                rec[t], mf[t], Pf[t] = upd, m, P
        fin[c] = np.concatenate([P.ravel(), m])
    dist = max([_dist(warm[c], fin[c - 1]) for c in range(1, n) if warm[c] is not None] or [0.0])
    return dict(lml=float(np.sum(lml)), rec=rec, mf=mf, Pf=Pf, dist=dist, chunks=n)


def backward(model, fwd, R_new, C, Wb):
    T, d = model["T"], len(model["x0m"])
    n = -(-T // C)
    Rn = np.broadcast_to(np.ravel(np.asarray(R_new, dtype=np.float64)), (T,)) if np.size(R_new) > 1 else np.full(T, float(np.ravel(R_new)[0]))
    mean, var = np.zeros(T), np.zeros(T)
    warm, out = [None] * n, [None] * n
    for c in range(n):
        s0, s1 = c * C, min(T, (c + 1) * C)
        top = min(T, s1 + Wb)
        lam, Lam = np.zeros(d), np.zeros((d, d))
        for t in range(top - 1, s0 - 1, -1):
            A = ref.transition(model, t)[0]
            H, h, _ = ref.emission(model, t)
            H = np.ravel(H)
            if t == s1 - 1 and top > s1:
                warm[c] = np.concatenate([Lam.ravel(), lam])
            if t < s1:
                w = fwd["Pf"][t] @ H
                mean[t] = H @ fwd["mf"][t] + float(np.ravel(h)[0]) - w @ lam
                var[t] = H @ w - w @ Lam @ w + Rn[t]
            v, s, nu = fwd["rec"][t]
            Cm = np.eye(d) - np.outer(v / s, H)
            Lam = Cm.T @ Lam @ Cm + np.outer(H, H) / s
            lam = Cm.T @ lam - H * nu / s
            if t == 0:
                break
            Lam = A.T @ Lam @ A
            lam = A.T @ lam
        out[c] = np.concatenate([Lam.ravel(), lam])
    dist = max([_dist(warm[c], out[c + 1]) for c in range(n - 1) if warm[c] is not None] or [0.0])
    return dict(mean=mean, var=var, dist=dist)


def run(model, ys, missing, R_new=None, C=0, W=0, Wb=0, guess=32):
    """the call as the host runs it: forced geometry (any of C, W, Wb non-zero) is never repaired; automatic geometry doubles a warm-up whose check
    fails while C >= 2 W.  status bits as tgp_dense_chunk_info: 1 forward, 2 backward warm-up too short."""
    T = model["T"]
    forced = bool(C or W or Wb)
    W, Wb = W or guess, Wb or guess
    if not C:
        nmax = T // (4 * max(W, Wb if R_new is not None else 0))
        if nmax < 8:
            return dict(served=0, attempts=0, status=0)
        C = -(-T // nmax)
    attempts = 0
    while True:
        attempts += 1
        f = forward(model, ys, missing, C, W)
        if f["dist"] <= TOL_F:
            break
        if forced or C < 4 * W:
            return dict(served=0, attempts=attempts, status=1, dist_f=f["dist"], C=C, W=W, Wb=Wb)
        W *= 2
    out = dict(served=1, lml=f["lml"], dist_f=f["dist"], chunks=f["chunks"], C=C, W=W)
    if R_new is not None:
        while True:
            attempts += 1
            b = backward(model, f, R_new, C, Wb)
            if b["dist"] <= TOL_B:
                break
            if forced or C < 4 * Wb:
                return dict(served=0, attempts=attempts, status=2, dist_f=f["dist"], dist_b=b["dist"], C=C, W=W, Wb=Wb)
            Wb *= 2
        out.update(mean=b["mean"], var=b["var"], dist_b=b["dist"])
    out.update(attempts=attempts, status=0, Wb=Wb)
    return out


if __name__ == "__main__":
    for d in sorted(GEOMETRY):
        model, (C, W, Wb) = test_model(d)
        for per_step in (False, True):
            mdl, y, missing = test_series(model, d, per_step_noise=per_step)
            r = run(mdl, y, missing, np.array([0.05]), C, W, Wb)
            print(f"d = {d} per-step noise {int(per_step)}: T = {mdl['T']} C = {C} W = {W} Wb = {Wb}: served {r['served']} attempts {r['attempts']} "
                  f"dist_f {r.get('dist_f', float('nan')):.2e} dist_b {r.get('dist_b', float('nan')):.2e}", flush=True)
