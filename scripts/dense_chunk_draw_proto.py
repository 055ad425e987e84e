"""The dense engine's posterior draw across the chip (csrc/tgp_dense_draw.hpp), restated in NumPy beside scripts/dense_chunk_proto.py: what
dk_chunk_draw / dk_fused_draw compute, with nothing of their layout.  Its oracle is ref.posterior_missing + ref.replace_observation_noise_cov + ref.rand
on the same draws (lgssm.jl:193-238, :65-91).

The reference draws from the Reverse model that `posterior` builds:
    x_{T-1} = m_{T-1} + chol(P_{T-1} + 1e-12 I).U' eps_0,     y*_t = H_t x_t + h_t + sqrt(Rnew_t) e_t   (vector emissions: sqrt(Rnew_t + 1e-9)),
    x_{t-1} = G_t x_t + g_t + U_t' eps_t[t],   (G_t, L_t) = invert_dynamics (1e-10 on the predicted covariance),   U_t = chol(L_t + 1e-9 I).U.
Index conventions (pinned by tests/test_dense_chunk_draw_proto.py): row t of eps_t drives the transition OUT of step t (into t - 1), row t of eps_e the
emission of step t; the transition out of step 0 (row 0 of eps_t) moves the state to a step nobody emits, so it is not computed.

Here the walk carries the deviation from the filtered mean, delta_t = x_t - m_t (the wide engine's form):
    delta_{T-1} = chol(P_f[T-1] + 1e-12 I).U' eps_0
    delta_{t-1} = G_t (delta_t + (m_t - m^p_t)) + U_t' eps_t[t],      y*_t = H_t (m_t + delta_t) + h_t + sqrt(Rnew_t) e_t
with m_t - m^p_t = sum_j v_j nu_j / s_j from the forward pass's records (zero at a missing step), and per step from P = P_f[t-1] and the step's A, Q:
    T1 = A P,  Pp = T1 A' + Q,  Lc = chol(Pp + 1e-10 I),  W = Lc^-1 T1,  L = P - W'W,  U = chol(L + 1e-9 I).U,  G z = W'(Lc^-1 z)      (G is never formed).

Chunks: G_t has the closed loop's spectrum (with P_f = Pp (I - K h)', G is similar to (A (I - K h))'), so the walk forgets its start as the filter does.
Chunk c owns [c C, (c + 1) C); it walks down from min(T, (c + 1) C + Wd) with delta = 0 at its first step, on the SAME rows of eps_t, and writes nothing
before it reaches its own steps; a chunk whose walk starts at T - 1 starts from delta_{T-1}.  Every chunk keeps delta at the crossing into its own steps and
the delta it carries out of its first step; hand-over c compares chunk c's crossing value with what chunk c + 1 carried out: largest |difference| over
the largest |entry| of the latter (tolerance 1e-11, the engine's backward tolerance; the draw is linear in delta, so the emission inherits it times |h|_1).

usage: dense_chunk_draw_proto.py        prints the distances to the oracle of the cases tests/test_dense_chunk_draw_proto.py asserts"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import lgssm_ref as ref  # noqa: E402

TOL_D = 1e-11


def blocks_of(model, ys, missing):
    """per step (A, a, Q, H (p, d), h (p,), R (p,), y (p,)) with a missing entry as y := 0, R := 1e15 (missings.jl:25-53); diagonal noise"""
    out = []
    for t in range(model["T"]):
        A, a, Q = ref.transition(model, t)
        H, h, R = ref.emission(model, t)
        H, h = np.atleast_2d(H), np.atleast_1d(h)
        Rd = np.array(np.atleast_1d(R) if np.ndim(R) < 2 else np.diagonal(R), dtype=np.float64)
        yt = np.array(np.atleast_1d(ys[t]), dtype=np.float64)
        if missing is not None:
            mt = np.broadcast_to(np.atleast_1d(missing[t]), Rd.shape)
            Rd[mt], yt[mt] = ref.LARGE_VAR, 0.0
        out.append((A, np.ravel(a), Q, H, h, Rd, yt))
    return out


def forward(model, ys, missing=None):
    """the sequential filter as the device runs it (p scalar updates per step): filtering means / covariances and the records (v, s, nu)"""
    blocks = blocks_of(model, ys, missing)
    m, P = model["x0m"].copy(), model["x0P"].copy()
    mf, Pf, rec = [], [], []
    for (A, a, Q, H, h, Rd, yt) in blocks:
        m, P, upd = A @ m + a, A @ P @ A.T + Q, []
        for j in range(len(h)):
            v = P @ H[j]
            s = H[j] @ v + Rd[j]
            nu = yt[j] - H[j] @ m - h[j]
            m, P = m + v * nu / s, P - np.outer(v, v) / s
            upd.append((v, s, nu))
        mf.append(m), Pf.append(P), rec.append(upd)
    return dict(blocks=blocks, mf=mf, Pf=Pf, rec=rec)


def start_state(fwd, eps_0):
    P = fwd["Pf"][-1]
    return ref.chol_upper(P + 1e-12 * np.eye(len(eps_0))).T @ eps_0


def move(fwd, t, delta, eps, records=True):
    """delta_{t-1} from delta_t (t >= 1)"""
    A, a = fwd["blocks"][t][0], fwd["blocks"][t][1]
    P = fwd["Pf"][t - 1]
    d = len(delta)
    if records:
        dm = np.zeros(d)
        for (v, s, nu) in fwd["rec"][t]:
            dm = dm + v * (nu / s)
    else:
        dm = fwd["mf"][t] - (A @ fwd["mf"][t - 1] + a)
    T1 = A @ P
    Pp = T1 @ A.T + fwd["blocks"][t][2]
    Uc = ref.chol_upper(Pp + 1e-10 * np.eye(d))          # Lc = Uc'
    W = np.linalg.solve(Uc.T, T1)
    L = P - W.T @ W
    U = ref.chol_upper(L + 1e-9 * np.eye(d))
    return W.T @ np.linalg.solve(Uc.T, delta + dm) + U.T @ eps


def emit(model, fwd, t, delta, Rn_t, e_t):
    H, h = fwd["blocks"][t][3], fwd["blocks"][t][4]
    jit = 0.0 if model["kind"] == "scalar" else 1e-9       # (lgc.jl:84-87 against lgc.jl:241-243)
    return H @ (fwd["mf"][t] + delta) + h + np.sqrt(Rn_t + jit) * np.atleast_1d(e_t)


def _rnew(model, R_new):
    T, p = model["T"], len(np.atleast_1d(ref.emission(model, 0)[1]))
    Rn = np.asarray(R_new, dtype=np.float64)
    if Rn.ndim == 3:
        Rn = np.diagonal(Rn, axis1=-2, axis2=-1)
    return np.broadcast_to(Rn.reshape(-1, p), (T, p))


def _dist(x, r):
    return float(np.max(np.abs(x - r)) / max(np.max(np.abs(r)), 1e-300))


def draw(model, fwd, R_new, eps_t, eps_e, eps_0, C=0, Wd=0, records=True):
    """C == 0: the sequential walk (dk_fused_draw); else the chunks (dk_chunk_draw) and their hand-over distance"""
    T = model["T"]
    Rn = _rnew(model, R_new)
    p = Rn.shape[1]
    ee = np.asarray(eps_e, dtype=np.float64).reshape(T, p)
    y = np.zeros((T, p))
    d0 = start_state(fwd, eps_0)
    C = C or T
    n = -(-T // C)
    warm, out = [None] * n, [None] * n
    for c in range(n):
        s0, s1 = c * C, min(T, (c + 1) * C)
        top = min(T, s1 + Wd)
        delta = d0.copy() if top == T else np.zeros_like(d0)
        for t in range(top - 1, s0 - 1, -1):
            if t == s1 - 1 and top > s1:
                warm[c] = delta.copy()
            if t < s1:
                y[t] = emit(model, fwd, t, delta, Rn[t], ee[t])
            if t == 0:
                break
            delta = move(fwd, t, delta, eps_t[t], records)
        out[c] = delta
    dist = max([_dist(warm[c], out[c + 1]) for c in range(n - 1) if warm[c] is not None] or [0.0])
    return dict(y=y[:, 0] if model["kind"] == "scalar" else y, dist=dist, chunks=n)


def oracle(model, ys, missing, R_new, eps_t, eps_e, eps_0):
    post = ref.posterior_missing(model, ys, missing) if missing is not None else ref.posterior(model, ys)
    return np.asarray(ref.rand(ref.replace_observation_noise_cov(post, R_new), eps_t, eps_e, eps_0))


def first_guess(model):
    """the host's first guess of a warm-up (csrc/tgp_dense.hip chunk_estimate; shared blocks): the closed loop of the fully observed stationary filter,
    squared until its infinity norm is below 1e-13, plus an eighth; at least 32"""
    A, _, Q = ref.transition(model, 0)
    H, _, R = ref.emission(model, 0)
    H = np.atleast_2d(H)
    Rd = np.atleast_1d(R) if np.ndim(R) < 2 else np.diagonal(R)
    P = Q.copy()
    for _ in range(600):
        M, Phi = A @ P @ A.T + Q, A.copy()
        for j in range(H.shape[0]):
            v = M @ H[j]
            s = H[j] @ v + Rd[j]
            M = M - np.outer(v, v) / s
            Phi = Phi - np.outer(v, H[j] @ Phi) / s
        settled = np.max(np.abs(M - P)) <= 1e-9 * np.max(np.abs(M))
        P = M
        if settled:
            break
    k = 1
    while not np.max(np.sum(np.abs(Phi), axis=1)) <= 1e-13 and k < (1 << 22):
        Phi, k = Phi @ Phi, 2 * k
    return max(32, k + k // 8)


def run(model, ys, missing, R_new, eps, C=0, Wd=0, guess=32):
    """the draw pass as the host runs it behind a served forward pass: a forced geometry (Wd non-zero) is never repaired, an automatic one doubles Wd while
    C >= 2 Wd; status bit 2: the warm-up was too short (the sequential walk then serves the call)"""
    fwd = forward(model, ys, missing)
    forced = bool(Wd)
    Wd = Wd or guess
    attempts = 0
    while True:
        attempts += 1
        r = draw(model, fwd, R_new, *eps, C=C, Wd=Wd)
        if r["dist"] <= TOL_D:
            return dict(served=1, attempts=attempts, status=0, Wd=Wd, **r)
        if forced or C < 4 * Wd:
            return dict(served=0, attempts=attempts, status=2, Wd=Wd, dist=r["dist"], y=draw(model, fwd, R_new, *eps)["y"])
        Wd *= 2


def rel(x, r):
    return float(np.max(np.abs(np.asarray(x) - np.asarray(r))) / np.max(np.abs(r)))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from tests._util import random_model  # noqa: E402
    for d, p in ((17, 1), (33, 1), (33, 3)):
        rng = np.random.default_rng(100 + d + p)
        T = 600
        model, Rd = random_model(rng, T, d, p, rho=0.6)
        y = rng.standard_normal((T, p))
        mk = rng.random((T, p)) < 0.1
        eps = (rng.standard_normal((T, d)), rng.standard_normal((T, p)), rng.standard_normal(d))
        Rn = np.stack([np.diag(r) for r in rng.uniform(0.05, 0.3, size=(T, p))])
        want = oracle(model, y, mk, Rn, *eps)
        fwd = forward(model, y, mk)
        a = draw(model, fwd, Rn, *eps)
        b = draw(model, fwd, Rn, *eps, records=False)
        c = draw(model, fwd, Rn, *eps, C=96, Wd=64)
        print(f"d = {d} p = {p}: records {rel(a['y'], want):.2e} mean-difference {rel(b['y'], want):.2e} chunked (C 96, Wd 64) vs sequential "
              f"{rel(c['y'], a['y']):.2e} hand-over {c['dist']:.2e}", flush=True)
