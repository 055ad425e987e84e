"""Helpers of the tests of the sweep engine's adjoint gradient for SDE-described models (test infrastructure): a NumPy long-double restatement
of the walk -- the transitions from the gaps by the closed form, the covariance half through Pinf, d logpdf / d A_t contracted on the spot into sums over the
closed form's coefficients, the host's chain rule from those to d logpdf / d F -- and the host simulation of k_sweep_adjoint_sde
(tests/hostsim/sweepadjsdesim.cpp)."""
import ctypes
import os
import subprocess

import numpy as np

from oracle import components as oc
from oracle import lgssm_ref as ref
from tests import _util as U

LD = np.longdouble
BLOCKS = ("F", "Pinf", "A1", "a", "H", "h", "R", "x0m", "x0P")
LP_BAR, GRAD_BAR = 1e-10, 1e-8      # tests/_sweep_adjoint.py's bars: logpdf relative; a gradient entry relative to its block's largest


def components_of(F):
    """the connected components of F's sparsity pattern, each a sorted list of rows (tgp_api.hip sde_closed_form)"""
    d = F.shape[0]
    left, out = set(range(d)), []
    while left:
        S, grow = [min(left)], True
        while grow:
            grow = False
            for j in sorted(left - set(S)):
                if any(F[j, s] != 0 or F[s, j] != 0 for s in S):
                    S.append(j)
                    grow = True
        out.append(sorted(S))
        left -= set(S)
    return out


def coefficients(F):
    """(lam (d,), N1 (d, d), N2 (d, d)) of sde_closed_form's map, in F's dtype: per component S of n rows lam = -tr F_SS / n, N = F_SS + lam I,
    N1 = [n >= 2] N, N2 = [n >= 3] N N / 2.  Nilpotency is NOT checked: the map is what is differentiated."""
    d = F.shape[0]
    lam, N1, N2 = np.zeros(d, dtype=F.dtype), np.zeros((d, d), dtype=F.dtype), np.zeros((d, d), dtype=F.dtype)
    for S in components_of(F):
        n, ix = len(S), np.ix_(S, S)
        l = -np.trace(F[ix]) / n
        N = F[ix] + l * np.eye(n, dtype=F.dtype)
        lam[S] = l
        if n >= 2:
            N1[ix] = N
        if n >= 3:
            N2[ix] = N @ N / 2
    return lam, N1, N2


def closed_form(coef, tau):
    """(A, e): A = diag(e) (I + tau N1 + tau^2 N2), e_i = exp(-lam_i tau)"""
    lam, N1, N2 = coef
    e = np.exp(-lam * tau)
    return e[:, None] * (np.eye(len(lam), dtype=lam.dtype) + tau * N1 + tau * tau * N2), e


def chain_rule(F, gl, gN1, gN2):
    """d logpdf / d F from the sums over the coefficients: the transpose of `coefficients` (zero outside the components)"""
    d = F.shape[0]
    gF = np.zeros((d, d), dtype=gl.dtype)
    _, N1, _ = coefficients(np.asarray(F, dtype=gl.dtype))
    for S in components_of(F):
        n, ix = len(S), np.ix_(S, S)
        N = N1[ix]
        gN = np.zeros((n, n), dtype=gl.dtype)
        if n >= 2:
            gN = gN + gN1[ix]
        if n >= 3:
            gN = gN + (gN2[ix] @ N.T + N.T @ gN2[ix]) / 2
        gF[ix] = gN - (gl[S].sum() + np.trace(gN)) / n * np.eye(n, dtype=gl.dtype)
    return gF


def restated(F, Pinf, A1, a, H, h, R, x0m, x0P, times, y, missing=None):
    """logpdf and its gradient by reverse mode through the sequential filter of the SDE-described model, in long double.  A1: the explicit first transition,
    or None (step 0 takes the closed form with tau = 1: its share goes to F, gA1 = 0).  h, R: scalars or (T,).  Returns (lml, g): g holds the BLOCKS as
    lgssm.logpdf_adjoint_sde gives them (Pinf, x0P symmetrised; h, R the sums over the observed steps), h_steps / R_steps (T,), the coefficient sums lam, N1,
    N2, and sumG = sum_t d logpdf / d A_t, sumPb = sum_t d logpdf / d P_p,t."""
    times = np.asarray(times, dtype=np.float64)
    T, d = times.shape[0], F.shape[0]
    Fl, a, H = np.asarray(F, dtype=LD), np.asarray(a, dtype=LD).reshape(d), np.asarray(H, dtype=LD).reshape(d)
    Pi = np.asarray(Pinf, dtype=LD)
    Pi = LD(0.5) * (Pi + Pi.T)
    coef = coefficients(Fl)
    tau = np.concatenate([[1.0], np.diff(times)]).astype(LD)
    hs = np.broadcast_to(np.atleast_1d(np.asarray(h, dtype=LD)), (T,))
    Rs = np.broadcast_to(np.atleast_1d(np.asarray(R, dtype=LD)), (T,))
    miss = np.zeros(T, dtype=bool) if missing is None else np.asarray(missing, dtype=bool)
    yv = np.where(miss, 0.0, np.asarray(y, dtype=np.float64)).astype(LD)
    As, es = np.empty((T, d, d), dtype=LD), np.empty((T, d), dtype=LD)
    for t in range(T):
        As[t], es[t] = closed_form(coef, tau[t])
    if A1 is not None:
        As[0] = np.asarray(A1, dtype=LD)
    m, P = np.asarray(x0m, dtype=LD), np.asarray(x0P, dtype=LD)
    P = LD(0.5) * (P + P.T)
    ms, Ps = np.empty((T, d), dtype=LD), np.empty((T, d, d), dtype=LD)      # the filtering state in FRONT of every step
    lml = LD(0.0)
    log2pi = np.log(LD(2.0) * np.arccos(LD(-1.0)))
    for t in range(T):
        ms[t], Ps[t] = m, P
        A = As[t]
        m, P = A @ m + a, A @ (P - Pi) @ A.T + Pi
        if not miss[t]:
            V = P @ H
            S = H @ V + Rs[t]
            v = yv[t] - H @ m - hs[t]
            lml -= LD(0.5) * (log2pi + np.log(S) + v * v / S)
            m, P = m + V * (v / S), P - np.outer(V, V) / S
    z = lambda *s: np.zeros(s, dtype=LD)      # noqa: E731
    g = dict(lam=z(d), N1=z(d, d), N2=z(d, d), Pinf=z(d, d), A1=z(d, d), a=z(d), H=z(d), sumG=z(d, d), sumPb=z(d, d))
    gh, gR = z(T), z(T)
    lam, Lam = z(d), z(d, d)
    for t in range(T - 1, -1, -1):
        m, P, A = ms[t], Ps[t], As[t]
        mp, AD = A @ m + a, A @ (P - Pi)
        Pp = AD @ A.T + Pi
        if miss[t]:
            mb, Pb = lam, Lam
        else:
            V = Pp @ H
            S = H @ V + Rs[t]
            v = yv[t] - H @ mp - hs[t]
            lV, LV = lam @ V, Lam @ V
            vb = lV / S - v / S
            Sb = -lV * v / S**2 + (V @ LV) / S**2 - LD(0.5) * (1 / S - v * v / S**2)
            Vb = lam * (v / S) - 2 * LV / S + Sb * H
            gR[t], gh[t] = Sb, -vb
            g["H"] += Pp @ Vb + Sb * V - vb * mp
            mb = lam - vb * H
            Pb = Lam + LD(0.5) * (np.outer(Vb, H) + np.outer(H, Vb))
        G = np.outer(mb, m) + 2 * Pb @ AD
        g["sumG"] += G
        g["sumPb"] += Pb
        g["a"] += mb
        lam, Lam2 = A.T @ mb, A.T @ Pb @ A
        g["Pinf"] += Pb - Lam2
        Lam = Lam2
        if t == 0 and A1 is not None:
            g["A1"] = G
        else:      # (step 0 of a model without A1: the closed form at tau = 1)
            g["lam"] -= tau[t] * (G * A).sum(axis=1)
            g["N1"] += tau[t] * es[t][:, None] * G
            g["N2"] += tau[t] ** 2 * es[t][:, None] * G
    g["x0m"], g["x0P"] = lam, Lam
    g["F"] = chain_rule(np.asarray(F, dtype=np.float64), g["lam"], g["N1"], g["N2"])
    out = {k: np.asarray(v, dtype=np.float64) for k, v in g.items()}
    out["h"], out["R"] = float(gh.sum()), float(gR.sum())
    out["h_steps"], out["R_steps"] = gh.astype(np.float64), gR.astype(np.float64)
    return float(lml), out


def oracle_model(F, Pinf, A1, a, H, h, R, x0m, x0P, times):
    """the oracle's model dict with per-step blocks rebuilt from (F, Pinf, A1) by the closed form: A_t, Q_t = Pinf - A_t Pinf A_t'"""
    times = np.asarray(times, dtype=np.float64)
    T, d = times.shape[0], F.shape[0]
    coef = coefficients(np.asarray(F, dtype=np.float64))
    tau = np.concatenate([[1.0], np.diff(times)])
    A = np.stack([closed_form(coef, t)[0] for t in tau])
    if A1 is not None:
        A[0] = A1
    Ps = 0.5 * (np.asarray(Pinf, dtype=np.float64) + np.asarray(Pinf, dtype=np.float64).T)
    Q = np.stack([Ps - Ai @ Ps @ Ai.T for Ai in A])
    return dict(ordering="F", kind="scalar", T=T, A=A, a=np.asarray(a, dtype=np.float64).reshape(1, d), Q=Q, H=np.asarray(H, dtype=np.float64).reshape(1, d),
                h=np.atleast_1d(np.asarray(h, dtype=np.float64)), R=np.atleast_1d(np.asarray(R, dtype=np.float64)), x0m=np.asarray(x0m, dtype=np.float64),
                x0P=np.asarray(x0P, dtype=np.float64))


def gp_blocks(k, times):
    """(F, Pinf, A1, a, H, x0m) of a kernel expression at plain-array inputs: the drift and emission of its SDE, the stationary covariance, and the first
    transition by the reference's rule (dt_1 := 1 in each sub-kernel's own stretched time, lti_sde.jl:139)"""
    F, H = U.kernel_sde(k)
    A, _, _, _, _, (m0, P0) = oc.lgssm_components(k, np.asarray(times, dtype=np.float64)[:1])
    d = F.shape[0]
    return np.asarray(F, float), ref.symmetric(np.asarray(P0, float)), np.asarray(A[0], float), np.zeros(d), np.asarray(H, float), np.asarray(m0, float)


def irregular_times(rng, T, ties=(), long_gap=None, typical=0.1):
    """gaps U(0.5, 1.5) x typical; ties: steps whose gap is exactly 0; long_gap: a step whose gap is 50 typical gaps"""
    gaps = typical * (0.5 + rng.random(T))
    for t in ties:
        gaps[t] = 0.0
    if long_gap is not None:
        gaps[long_gap] = 50.0 * typical
    gaps[0] = 0.0
    return np.cumsum(gaps)


def draw(F, Pinf, A1, a, H, h, R, x0m, x0P, times, seed):
    """a series from the model (a tie has Q = 0: the transition noise goes through a symmetric square root, not a Cholesky factor)"""
    model = oracle_model(F, Pinf, A1, a, H, h, R, x0m, x0P, times)
    rng = np.random.default_rng(seed)
    T, d = model["T"], F.shape[0]

    def root(M):
        w, V = np.linalg.eigh(0.5 * (M + M.T))
        return V * np.sqrt(np.clip(w, 0.0, None))

    x = np.asarray(x0m, dtype=np.float64) + root(np.asarray(x0P, dtype=np.float64)) @ rng.standard_normal(d)
    hs, Rs = np.broadcast_to(model["h"], (T,)), np.broadcast_to(model["R"], (T,))
    y = np.empty(T)
    for t in range(T):
        x = model["A"][t] @ x + model["a"][0] + root(model["Q"][t]) @ rng.standard_normal(d)
        y[t] = model["H"][0] @ x + hs[t] + np.sqrt(Rs[t]) * rng.standard_normal()
    return y


def block_deviations(g, g_ref, blocks=BLOCKS):
    """{block: worst entry / the largest entry of the reference's own block}"""
    out = {}
    for k in blocks:
        sc = float(np.abs(np.asarray(g_ref[k])).max())
        out[k] = float(np.abs(np.asarray(g[k]) - np.asarray(g_ref[k])).max()) / (sc if sc > 0.0 else 1.0)
    return out


_SIM = None


def sim():
    global _SIM
    if _SIM is None:
        src = os.path.join(U.HERE, "hostsim", "sweepadjsdesim.cpp")
        so = os.path.join(U.HERE, "hostsim", "libsweepadjsdesim.so")
        deps = [src] + [os.path.join(U.ROOT, "temporalgps.jl_amd", "csrc", f) for f in ("tgp_math.hpp", "tgp_sweep_body.hpp", "tgp_sweep_plan.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        _SIM = ctypes.CDLL(so)
        _SIM.sweepadjsdesim_run.restype = ctypes.c_int
    return _SIM


def sim_run(F, Pinf, A1, a, H, h, R, x0m, x0P, times, y, missing=None, C=0, W=0, Wa=0, num_cu=1, w_hint=0, wa_hint=0):
    """the host simulation of k_sweep_adjoint_sde on an explicit first transition A1.  Returns dict(rc, lml, status, dist_f, dist_a, C, W, Wa, nwaves, g) with
    g as `restated` gives it (the BLOCKS, the steps, lam / N1 / N2)."""
    T, d = len(times), F.shape[0]
    cm = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)      # noqa: E731
    R = np.atleast_1d(np.asarray(R, dtype=np.float64))
    h = np.atleast_1d(np.asarray(h, dtype=np.float64))
    Rstep = np.ascontiguousarray(R) if R.shape[0] > 1 else None
    hstep = np.ascontiguousarray(h) if h.shape[0] > 1 else None
    Rrep = U.sweep_representative(R, noise=True)
    coef = U.sde_coef(F)
    tau = np.concatenate([[-1.0], np.diff(np.asarray(times, dtype=np.float64))])
    tau_typ = U.sweep_representative(tau[1:], noise=False)
    Ps = ref.symmetric(np.asarray(Pinf, dtype=np.float64))
    Q1 = Ps - A1 @ Ps @ A1.T
    yv = np.ascontiguousarray(np.where(np.isnan(y), 0.0, y), dtype=np.float64)
    mk = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    ghs, gRs, out = np.full(T, np.nan), np.full(T, np.nan), np.zeros(8)
    dd = d * d
    gv = np.zeros(5 * dd + 4 * d + 2)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    p = U._p
    rc = sim().sweepadjsdesim_run(
        d, U._i64(T), p(cm(A1)), p(np.ascontiguousarray(a, dtype=np.float64)), p(cm(Q1)), p(np.ascontiguousarray(H, dtype=np.float64)),
        ctypes.c_double(float(h[0])), ctypes.c_double(Rrep), p(np.ascontiguousarray(x0m, dtype=np.float64)), p(cm(x0P)), p(cm(Ps)), p(coef),
        ctypes.c_double(tau_typ), p(yv), None if mk is None else mk.ctypes.data_as(u8), p(Rstep), p(hstep), p(np.ascontiguousarray(tau)), C, W, Wa, w_hint,
        wa_hint, num_cu, p(ghs), p(gRs), p(gv), p(out))
    sq = lambda v: v.reshape(d, d).T.copy()      # noqa: E731  (column-major block -> [i][k])
    o = np.cumsum([0, d, dd, dd, dd, d, d, 1, 1, dd, d, dd])
    parts = [gv[o[i]:o[i + 1]] for i in range(11)]
    g = dict(lam=parts[0].copy(), N1=sq(parts[1]), N2=sq(parts[2]), Pinf=sq(parts[3]), a=parts[4].copy(), H=parts[5].copy(), h=float(parts[6][0]),
             R=float(parts[7][0]), A1=sq(parts[8]), x0m=parts[9].copy(), x0P=sq(parts[10]), h_steps=ghs, R_steps=gRs)
    g["F"] = chain_rule(np.asarray(F, dtype=np.float64), g["lam"], g["N1"], g["N2"])
    return dict(rc=rc, lml=out[0], status=int(out[1]), dist_f=out[2], dist_a=out[3], C=int(out[4]), W=int(out[5]), Wa=int(out[6]), nwaves=int(out[7]), g=g)


# ---- the cases the host and the GPU tier share -----------------------------------------------------------------------------------------------------
M12, M32, M52 = ("matern12",), ("matern32",), ("matern52",)
MODELS = {1: M12, 2: M32, 3: M52, 4: ("sum", M32, ("stretched", 0.7, M32))}
WORK_GAP = {1: 0.1, 2: 0.1, 3: 0.1, 4: 0.15}      # typical gaps: the working spacing of tests/_sweep_edges.py (automatic warm-ups of 32 ... 168 steps)
FAST_GAP = {1: 5.0, 2: 4.0, 3: 4.0, 4: 6.0}       # ... and its fast-forgetting spacing: a start state is gone within 8 steps
_CASES = {}


def case(d, T, xs=0, fast=False, x0=False, gap_at=None, seed=0, kernel=None):
    """One series on irregular times -- gaps U(0.5, 1.5) x typical, two ties, one gap of 50 typical gaps (not at the fast spacing: the filter would start
    anew behind it, which the ties and the mask already exercise) -- with 10 % missing, a run of missing steps [5:9], missing ends, 40 missing steps around
    gap_at; xs bit 0: a noise variance per step, bit 1: an emission offset per step; x0: a prior of the series that is not the stationary one.
    Returns dict(blocks, times, y, missing, lp, g) with (lp, g) = restated(...), computed once per case."""
    key = (d, T, xs, fast, x0, gap_at, seed, kernel)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(977 * d + 31 * xs + T + seed)
    typical = (FAST_GAP if fast else WORK_GAP)[d]
    times = irregular_times(rng, T, ties=(T // 3, T // 3 + 1, 2 * T // 3), long_gap=None if fast else T // 2, typical=typical)
    F, Pinf, A1, a, H, x0m = gp_blocks(kernel or MODELS[d], times)
    R = 0.1 * (0.5 + rng.random(T)) if xs & 1 else 0.1
    h = np.sin(0.3 * times) if xs & 2 else 0.2
    x0P = Pinf
    if x0:
        B = rng.standard_normal((d, d))
        x0m, x0P = x0m + np.array([1.0, -2.0, 0.5, 0.25])[:d], 0.3 * Pinf + 0.05 * B @ B.T
    blocks = dict(F=F, Pinf=Pinf, A1=A1, a=a, H=H, h=h, R=R, x0m=x0m, x0P=x0P)
    y = draw(times=times, seed=seed + d, **blocks)
    missing = rng.random(T) < 0.1
    missing[5:9] = True
    missing[0] = missing[T - 1] = True
    if gap_at is not None:
        missing[gap_at - 20:gap_at + 20] = True
    lp, g = restated(times=times, y=y, missing=missing, **blocks)
    _CASES[key] = dict(blocks=blocks, times=times, y=y, missing=missing, lp=lp, g=g)
    return _CASES[key]
