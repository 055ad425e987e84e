"""Shared by the tile-sweep tests (tgp_sweep_tile.hip): the models at d = 9, 12, 13, 16, their cases with the oracle's answers, and the kernel's
algorithm restated in NumPy -- the padded state, A (A P)' + Q, the 20-double record, the Bryson-Frazier walk on (r, N), a chunk with its warm-ups and both checks."""
import functools

import numpy as np

from tests import _sweep_group as SG
from tests import _util as U
from tests.test_gpu_sweep import _reference

DP, DT = 16, 0.2
KERNELS = {d: U.WIDE_ADJOINT_KERNELS[d] for d in (9, 12, 16)}
KERNELS[13] = ("sum", U.WIDE_ADJOINT_KERNELS[9], SG.M32, ("stretched", 0.7, SG.M32))
KERNELS[8], KERNELS[17] = SG.KERNELS[8][0], U.WIDE_ADJOINT_KERNELS[17]      # the decline cases on either side


def mask(T, seed, frac=0.1):
    missing = np.random.default_rng(seed).random(T) < frac
    missing[[0, 5, 6, 7, 8, T - 3, T - 2, T - 1]] = True
    return missing


@functools.lru_cache(maxsize=None)
def case(d, T, xs=0, masked=True, rn_per_step=False):
    """xs bit 0: a noise variance per step, bit 1: an emission offset per step.  Returns model, y, missing, Rn and the oracle's (lp, pm, pv)."""
    rng = np.random.default_rng(1000 * d + T + xs)
    s2 = rng.uniform(0.05, 0.5, T) if xs & 1 else 0.1
    model, y, _ = U.gp_case(KERNELS[d], ("regular", 0.0, DT, T), s2, seed=d + xs, mean=("custom", lambda t: np.sin(t)) if xs & 2 else None)
    assert len(model["x0m"]) == d
    missing = mask(T, 100 + d + xs) if masked else None
    Rn = rng.random(T) * 0.05 if rn_per_step else np.array([1e-18])
    return model, y, missing, Rn, _reference(model, y, missing, Rn, fast=True)


def run_tile_sweep(model, y, missing, Rnew, C, W, Wb):
    """returns lml, mean, var, (dist_f, dist_b) as k_sweep_tile computes them"""
    d, T = len(model["x0m"]), len(y)
    pad = lambda M: np.pad(M, ((0, DP - d), (0, DP - d)))      # noqa: E731
    vec = lambda v: np.pad(v, (0, DP - d))      # noqa: E731
    A, Q, a, H = pad(model["A"][0]), pad(0.5 * (model["Q"][0] + model["Q"][0].T)), vec(model["a"][0]), vec(model["H"][0])
    Rt, ht, Rn = (np.broadcast_to(np.atleast_1d(v), (T,)) for v in (model["R"], model["h"], Rnew))
    Pinf = model["x0P"]      # (a GP's series starts from its stationary prior, mean zero: where a warm-up starts as well)
    assert np.allclose(model["A"][0] @ Pinf @ model["A"][0].T + model["Q"][0], Pinf, rtol=0, atol=1e-12) and not model["x0m"].any()
    gen = x0 = (np.zeros(DP), pad(np.triu(Pinf) + np.triu(Pinf, 1).T))
    sd = vec(np.sqrt(np.diag(Pinf)))
    isd = np.where(sd > 0, 1.0 / np.where(sd > 0, sd, 1.0), 0.0)
    miss = np.zeros(T, dtype=bool) if missing is None else missing
    mean, var, lml, dist = np.full(T, np.nan), np.full(T, np.nan), 0.0, [0.0, 0.0]

    def fstep(x, t, rec=None):
        m, P = x
        Pm, mp = A @ (A @ P).T + Q, A @ m + a
        wR, wC = Pm @ H, Pm.T @ H
        hph, hm, obs = float(H @ wC), float(H @ mp), not miss[t]
        S = hph + Rt[t] if obs else 1.0
        iS, v = (1.0 / S, y[t] - (hm + ht[t])) if obs else (0.0, 0.0)
        if rec is not None:
            rec[t] = (wC, hph, hm, v, S if obs else 0.0)
        return (mp + wC * (v * iS), Pm - np.outer(wR, wC * iS)), (np.log(2 * np.pi * S) + v * v * iS if obs else 0.0)

    def bstep(x, t, rec):
        r, N = x
        w, hph, hm, v, s = rec[t]
        Np, rp = A.T @ (A.T @ N).T, A.T @ r
        uR, uC = Np @ w, Np.T @ w
        q, rho, iS = float(w @ uC), float(w @ rp), (1.0 / s if s > 0 else 0.0)
        c = 1.0 - hph * iS
        out = (rho * c + hph * v * iS + (hm + ht[t]), hph * c - q * c * c)
        return (rp + H * ((v - rho) * iS), Np - iS * (np.outer(H, uC) + np.outer(uR, H)) + np.outer(H, H) * (q * iS * iS + iS)), out

    def forward(x, ta, tb, rec=None):
        acc = 0.0
        for t in range(ta, tb):
            x, l = fstep(x, t, rec)
            acc += l
        return x, acc

    for t0 in range(0, T, C):
        t1, rec = min(t0 + C, T), {}
        x, _ = forward(x0 if t0 - W <= 0 else gen, max(t0 - W, 0), t0)
        xend, acc = forward(x, t0, t1, rec)
        lml += -0.5 * acc
        te = min(t1 + Wb, T)
        forward(xend, t1, te, rec)
        if t1 < T:
            e1, _ = forward(x0 if t1 - W <= 0 else gen, max(t1 - W, 0), t1)
            dist[0] = max(dist[0], (np.abs(xend[0] - e1[0])[:d] / (sd[:d] + np.abs(xend[0][:d]) + np.abs(e1[0][:d]))).max(),
                          (np.abs(xend[1] - e1[1]) * np.outer(isd, isd)).max())
        b = (np.zeros(DP), np.zeros((DP, DP)))
        for t in range(te - 1, t1 - 1, -1):
            b, _ = bstep(b, t, rec)
        for t in range(t1 - 1, t0 - 1, -1):
            b, (mu, vr) = bstep(b, t, rec)
            assert np.isnan(mean[t])
            mean[t], var[t] = mu, vr + Rn[t]
        if t0 > 0:
            b1 = (np.zeros(DP), np.zeros((DP, DP)))
            for t in range(min(t0 + Wb, t1) - 1, t0 - 1, -1):
                b1, _ = bstep(b1, t, rec)
            dist[1] = max(dist[1], (np.abs(b[0] - b1[0]) * sd).max(), (np.abs(b[1] - b1[1]) * np.outer(sd, sd)).max())
        assert not xend[0][d:].any() and not xend[1][d:].any() and not xend[1][:, d:].any() and not b[0][d:].any() and not b[1][d:].any()      # the padding stays zero
    return lml, mean, var, dist
