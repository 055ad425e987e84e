"""The ALGORITHM of the wide-state engine's posterior draw (csrc/tgp_wide.hip: plan_draw, k_wide_post_rand) restated in NumPy beside
scripts/wide_proto.py, so that the CPU tier can hold it against the oracle without a GPU (tests/test_wide_draw_proto.py).

rand of the Reverse model posterior(model, y) builds (lgssm.jl:193-238, then lgssm.jl:65-91) is, for t = T-1 ... 0,

    y*_t = h . x_t + hh_t + sqrt(Rnew_t) e_t,        x_(t-1) = G_t x_t + g_t + chol(L_t + 1e-9 I).U' eps_t,     g_t = m_(t-1) - G_t (A m_(t-1) + a)

from x_(T-1) = m_(T-1) + chol(P_(T-1) + 1e-12 I).U' eps_0.  In the deviation from the filtered mean, dl_t = x_t - m_t, and with the filter's
own update m_t = (A m_(t-1) + a) + K_t r_t, the same recursion reads

    dl_(t-1) = G_t (dl_t + K_t r_t) + U_t' eps_t,       y*_t = y_t - (R / S_t) r_t + h . dl_t + sqrt(Rnew_t) e_t

(h . m_t + hh_t = y_t - (1 - h . K_t) r_t and 1 - h . K_t = R / S_t): no filtered mean enters, only the innovations r_t the forward kernel keeps.
Behind the head G_t = G, U_t = U_L and K_t = K are constants, G forgets a state within halo_draw steps, and a chunk that starts halo_draw steps late
from dl = 0 on the same streams is exact to rounding on its own steps.  The head's n0 steps run on the host with the per-step G_t, U_t.  Not the
product path: the HIP kernel is checked by tests/test_gpu_wide_draw.py."""
import numpy as np


def invert(Pprev, A, Q):
    """(G, L) of lgssm.jl:231-238 from the filtered covariance of the step before"""
    d = len(A)
    Pp = A @ Pprev @ A.T + Q + 1e-10 * np.eye(d)
    U = np.linalg.cholesky(0.5 * (Pp + Pp.T)).T
    Gt = np.linalg.solve(U, np.linalg.solve(U.T, A @ Pprev))
    UG = U @ Gt
    return Gt.T, Pprev - UG.T @ UG


def halo_of(M):
    k, Mk = 1, M.copy()
    while np.abs(Mk).sum(axis=1).max() > 2.0 ** -60:
        Mk, k = Mk @ Mk, 2 * k
        if k > 2 ** 20:
            return None
    return k


def plan_draw(model, pl, Pfs):
    """pl: wide_proto.plan's dictionary; Pfs: the head's filtered covariances [n0][d][d] (the last one settled)"""
    A, Q = model["A"][0], model["Q"][0]
    d, n0 = pl["d"], pl["n0"]
    eye = np.eye(d)
    Gs, Us = [], []
    for t in range(n0 + 1):      # (entry n0: the settled step)
        G, L = invert(model["x0P"] if t == 0 else Pfs[t - 1], A, Q)
        Lj = L + 1e-9 * eye
        Us.append(np.linalg.cholesky(0.5 * (Lj + Lj.T)).T)
        Gs.append(G)
    Pe = Pfs[n0 - 1] + 1e-12 * eye
    return dict(Gs=Gs, Us=Us, G=Gs[n0], U=Us[n0], halo=halo_of(Gs[n0]), Uend=np.linalg.cholesky(0.5 * (Pe + Pe.T)).T)


def head_covariances(model, n0):
    A, Q, h, R = model["A"][0], model["Q"][0], model["H"][0], float(np.atleast_1d(model["R"])[0])
    P, out = 0.5 * (model["x0P"] + model["x0P"].T), []
    for _ in range(n0):
        Pp = A @ P @ A.T + Q
        v = Pp @ h
        P = Pp - np.outer(v, v) / float(h @ v + R)
        P = 0.5 * (P + P.T)
        out.append(P)
    return out


def run(pl, dp, y, Rnew, eps_t, eps_e, eps_0, chunks=5):
    """the draw as the engine computes it: forward (innovations kept), `chunks` chunks backward behind the head, the head on the host"""
    T, d, n0 = len(y), pl["d"], pl["n0"]
    A, a, h, hh, R, K, S = pl["A"], pl["a"], pl["h"], pl["hh"], pl["R"], pl["K"], pl["S"]
    Rn = np.broadcast_to(np.asarray(Rnew, dtype=np.float64).reshape(-1), (T,))
    r, m = np.zeros(T), pl["x0m"].copy()
    for t in range(T):      # (the forward kernel's chunking is wide_proto.run's: here the plain recursion)
        mp = A @ m + a
        r[t] = y[t] - hh - h @ mp
        m = mp + (pl["Ks"][t] if t < n0 else K) * r[t]
    GK, G, U, halo = dp["G"] @ K, dp["G"], dp["U"], dp["halo"]
    out = np.zeros(T)
    Tb = T - n0
    ln = -(-Tb // chunks)
    dl_head = None
    for c in range(chunks):
        s0, s1 = n0 + c * ln, min(T, n0 + (c + 1) * ln)
        if s0 >= s1:
            continue
        w = min(T, s1 + halo)
        dl = dp["Uend"].T @ eps_0 if w == T else np.zeros(d)
        for t in range(w - 1, s0 - 1, -1):
            if t < s1:
                out[t] = y[t] - (R / S) * r[t] + h @ dl + np.sqrt(Rn[t]) * eps_e[t]      # (the observer lane: h . dl_t)
            dl = G @ dl + GK * r[t] + U.T @ eps_t[t]
        if c == 0:
            dl_head = dl
    dl = dl_head
    for t in range(n0 - 1, -1, -1):      # the head on the host
        out[t] = y[t] - (R / pl["Ss"][t]) * r[t] + h @ dl + np.sqrt(Rn[t]) * eps_e[t]
        dl = dp["Gs"][t] @ (dl + pl["Ks"][t] * r[t]) + dp["Us"][t].T @ eps_t[t]
    return out
