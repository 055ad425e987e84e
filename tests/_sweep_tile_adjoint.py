"""Shared by the tile sweep's adjoint tests (k_sweep_tile_adjoint): the parity cases with the long-double reference, and the kernel's chunked walk
restated in NumPy -- padded tiles, a checkpoint every B steps, the three backward walks, both hand-over checks."""
import functools

import numpy as np

from tests import _sweep_adjoint as SA
from tests import _sweep_tile as ST

DP, B = 16, 8
# (d, T, xs, C, W, Wa): C = 0 on the GPU tier means the plan's own geometry, which the host tier restates with the values of tests/test_sweep_tile_host.py
CASES = [(9, 2053, 0, 64, 128, 64), (12, 2048, 1, 104, 112, 104), (13, 2053, 3, 120, 136, 120), (16, 2048, 2, 144, 152, 144)]


@functools.lru_cache(maxsize=None)
def case(d, T, xs, masked=True):
    """model, y, missing and `restated`'s (lml, g)"""
    model, y, missing, _, _ = ST.case(d, T, xs, masked)
    return (model, y, missing) + SA.restated(model, y, missing)


def run_tile_adjoint(model, y, missing, C, W, Wa):
    """returns lml, g (as `restated` gives it), (dist_f, dist_b) as k_sweep_tile_adjoint computes them"""
    d, T = len(model["x0m"]), len(y)
    pad = lambda M: np.pad(M, ((0, DP - d), (0, DP - d)))      # noqa: E731
    vec = lambda v: np.pad(v, (0, DP - d))      # noqa: E731
    A, Q, a, H = pad(model["A"][0]), pad(0.5 * (model["Q"][0] + model["Q"][0].T)), vec(model["a"][0]), vec(model["H"][0])
    Rt, ht = (np.broadcast_to(np.atleast_1d(v), (T,)) for v in (model["R"], model["h"]))
    Pinf = model["x0P"]
    gen = x0 = (np.zeros(DP), pad(np.triu(Pinf) + np.triu(Pinf, 1).T))
    sd = vec(np.sqrt(np.diag(Pinf)))
    isd = np.where(sd > 0, 1.0 / np.where(sd > 0, sd, 1.0), 0.0)
    miss = np.zeros(T, dtype=bool) if missing is None else missing
    g = dict(A=np.zeros((DP, DP)), a=np.zeros(DP), Q=np.zeros((DP, DP)), H=np.zeros(DP), h_steps=np.full(T, np.nan), R_steps=np.full(T, np.nan))
    lml, dist = 0.0, [0.0, 0.0]

    def fstep(x, t):
        (m, P), obs = x, not miss[t]
        Pm, mp = A @ (A @ P).T + Q, A @ m + a
        V = Pm @ H
        S = float(H @ V) + Rt[t] if obs else 1.0
        iS, v = (1.0 / S, y[t] - (float(H @ mp) + ht[t])) if obs else (0.0, 0.0)
        return (mp + V * (v * iS), Pm - np.outer(V, V * iS)), (np.log(2 * np.pi * S) + v * v * iS if obs else 0.0)

    def astep(x, ad, t, add):
        (m, P), (lam, Lam), obs = x, ad, not miss[t]
        AP = A @ P
        Pm, mp = A @ AP.T + Q, A @ m + a
        V = Pm @ H
        S = float(H @ V) + Rt[t] if obs else 1.0
        iS, v = (1.0 / S, y[t] - (float(H @ mp) + ht[t])) if obs else (0.0, 0.0)
        LV, lV = Lam @ V, float(lam @ V)
        vb = (lV - v) * iS
        Sb = (float(V @ LV) - lV * v) * iS * iS - 0.5 * (iS - (v * iS) ** 2)
        Vb = Sb * H + lam * (v * iS) - 2.0 * iS * LV
        mb, Pb = lam - vb * H, Lam + 0.5 * (np.outer(Vb, H) + np.outer(H, Vb))
        if add:
            g["h_steps"][t], g["R_steps"][t] = -vb, Sb
            g["H"] += Pm @ Vb + Sb * V - vb * mp
            g["a"] += mb
            g["Q"] += Pb
            g["A"] += np.outer(mb, m) + 2.0 * Pb @ AP
        return A.T @ mb, A.T @ (A.T @ Pb).T

    def forward(x, ta, tb, ck=None, t0=0):
        acc = 0.0
        for t in range(ta, tb):
            if ck is not None and (t - t0) % B == 0:
                ck[t] = x
            x, l = fstep(x, t)
            acc += l
        return x, acc

    def walk(ad, ta, tb, ck, add):      # backwards over tb - 1 .. ta: every block's states forwards from its checkpoint, then the adjoint over them
        for tb0 in range(ta + (tb - ta - 1) // B * B, ta - 1, -B) if tb > ta else ():
            xs, x = [], ck[tb0]
            for t in range(tb0, min(tb0 + B, tb)):
                xs.append(x)
                x, _ = fstep(x, t)
            for t in range(min(tb0 + B, tb) - 1, tb0 - 1, -1):
                ad = astep(xs[t - tb0], ad, t, add)
        return ad

    zero = (np.zeros(DP), np.zeros((DP, DP)))
    for t0 in range(0, T, C):
        t1, ck = min(t0 + C, T), {}
        te = min(t1 + Wa, T)
        x, _ = forward(x0 if t0 - W <= 0 else gen, max(t0 - W, 0), t0)
        xend, acc = forward(x, t0, t1, ck, t0)
        lml += -0.5 * acc
        forward(xend, t1, te, ck, t0)
        if t1 < T:
            e1, _ = forward(x0 if t1 - W <= 0 else gen, max(t1 - W, 0), t1)
            dist[0] = max(dist[0], (np.abs(xend[0] - e1[0])[:d] / (sd[:d] + np.abs(xend[0][:d]) + np.abs(e1[0][:d]))).max(),
                          (np.abs(xend[1] - e1[1]) * np.outer(isd, isd)).max())
        ad = walk(walk(zero, t1, te, ck, False), t0, t1, ck, True)
        if t0 > 0:
            ad1 = walk(zero, t0, min(t0 + Wa, t1), ck, False)
            dist[1] = max(dist[1], (np.abs(ad[0] - ad1[0]) * sd).max(), (np.abs(ad[1] - ad1[1]) * np.outer(sd, sd)).max())
        else:
            g["x0m"], g["x0P"] = ad
        assert not ad[0][d:].any() and not ad[1][d:].any() and not ad[1][:, d:].any()      # the padding stays zero
    assert not g["A"][d:].any() and not g["A"][:, d:].any() and not g["Q"][d:].any() and not g["H"][d:].any() and not g["a"][d:].any()
    out = {k: (v[:d, :d] if v.ndim == 2 else v[:d]) for k, v in g.items() if k not in ("h_steps", "R_steps")}
    out["Q"], out["x0P"] = 0.5 * (out["Q"] + out["Q"].T), 0.5 * (out["x0P"] + out["x0P"].T)
    out.update(h=float(g["h_steps"].sum()), R=float(g["R_steps"].sum()), h_steps=g["h_steps"], R_steps=g["R_steps"])
    return lml, out, dist
