"""The wide-state engine's ADJOINT pass (csrc/tgp_wide.hip: tgp_wide::adjoint) restated in NumPy: the forward chunks keep m_t and r_t, the backward
chunks run lam_t = h r_t / S + Psi lam_(t+1) from zero `halo_b` steps ahead of their end, and the sums behind the head are ONE Gram matrix
G = sum_t (lam_(t+1), r_t, 1) (m_(t-1), r_t, 1)', turned into the record of csrc/tgp_adjoint_host.hpp (mu_t = A m_(t-1) + a).  The plan is
scripts/wide_proto.py's.  Held against the sequential sums by tests/test_wide_adjoint_proto.py."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("wide_proto", os.path.join(os.path.dirname(os.path.abspath(__file__)), "wide_proto.py"))
wide_proto = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wide_proto)
plan = wide_proto.plan


def sums(pl, y, chunks=7):
    """-> dict SA, Sa, Sk, Srm, Sr, SSQ (over the steps t >= n0), psi = lam_(n0), mu = mu_(n0)"""
    T, d, n0 = len(y), pl["d"], pl["n0"]
    A, a, h, hh = pl["A"], pl["a"], pl["h"], pl["hh"]
    m = pl["x0m"].copy()
    for t in range(n0):                                  # the head, on the host
        mp = A @ m + a
        m = mp + pl["Ks"][t] * (y[t] - hh - h @ mp)
    mT, rT, lamT = np.zeros((T, d)), np.zeros(T), np.zeros((T + 1, d))
    mT[n0 - 1] = m
    Tb = T - n0
    ln = -(-Tb // chunks)
    bounds = [(n0 + k * ln, min(T, n0 + (k + 1) * ln)) for k in range(-(-Tb // ln))]
    for s0, s1 in bounds:                                # forward: from zero `halo` steps early, or from the head's end state
        from_head = s0 - pl["halo"] <= n0
        z = m.copy() if from_head else np.zeros(d)
        for t in range(n0 if from_head else s0 - pl["halo"], s1):
            u = y[t] - hh
            r = u - pl["g"] @ z - pl["g0"]
            z = pl["Phi"] @ z + pl["K"] * u + pl["c"]
            if t >= s0:
                mT[t], rT[t] = z, r
    for s0, s1 in bounds:                                # backward: from zero `halo_b` steps ahead (exact at T)
        lam = np.zeros(d)
        for t in range(min(T, s1 + pl["halo_b"]) - 1, s0 - 1, -1):
            lam = h * rT[t] / pl["S"] + pl["Psi"] @ lam
            if t < s1:
                lamT[t] = lam
    U = np.concatenate([lamT[n0 + 1:T + 1], rT[n0:, None], np.ones((Tb, 1))], axis=1)
    W = np.concatenate([mT[n0 - 1:T - 1], rT[n0:, None], np.ones((Tb, 1))], axis=1)
    G = U.T @ W
    Glm, Sa, Sk, Grm, Sr, SSQ = G[:d, :d], G[:d, d + 1], G[:d, d], G[d, :d], G[d, d + 1], G[d, d]
    return dict(SA=Glm @ A.T + np.outer(Sa, a), Sa=Sa, Sk=Sk, Srm=A @ Grm + Sr * a, Sr=Sr, SSQ=SSQ, psi=lamT[n0], mu=A @ m + a)
