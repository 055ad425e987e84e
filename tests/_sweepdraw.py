"""Helpers of the sweep engine's posterior-draw tests (test infrastructure): the host simulation of k_sweep_draw (tests/hostsim/sweepdrawsim.cpp)
and a NumPy restatement of the walk it performs."""
import ctypes
import os
import subprocess

import numpy as np

from oracle import lgssm_ref as ref
from tests import _util as U

_SIM = None


def sweepdrawsim():
    global _SIM
    if _SIM is None:
        src = os.path.join(U.HERE, "hostsim", "sweepdrawsim.cpp")
        so = os.path.join(U.HERE, "hostsim", "libsweepdrawsim.so")
        deps = [src] + [os.path.join(U.ROOT, "temporalgps.jl_amd", "csrc", f) for f in ("tgp_math.hpp", "tgp_sweep_body.hpp", "tgp_sweep_plan.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        _SIM = ctypes.CDLL(so)
        _SIM.sweepdrawsim_run.restype = ctypes.c_int
    return _SIM


def sweepdrawsim_run(model, y, eps, missing=None, Rnew=None, sde=None, C=0, W=0, Wd=0, num_cu=1, w_hint=0, wd_hint=0):
    """model: oracle dict with SHARED A, a, Q, H (or, with sde = (F, times): transitions by the closed form from the gaps); R / h may be per step.
    eps = (eps_t (T, d), eps_e (T,), eps_0 (d,)).  Returns dict(rc, status, dist_f, dist_d, C, W, Wd, nwaves, y)."""
    T, d = model["T"], len(model["x0m"])
    cm = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)      # noqa: E731
    R = np.atleast_1d(np.asarray(model["R"], dtype=np.float64))
    h = np.atleast_1d(np.asarray(model["h"], dtype=np.float64))
    Rstep = np.ascontiguousarray(R) if R.shape[0] > 1 else None
    hstep = np.ascontiguousarray(h) if h.shape[0] > 1 else None
    Rrep = U.sweep_representative(R, noise=True)
    coef, tau, tau_typ = None, None, 0.0
    if sde is not None:
        F, times_ = sde
        coef = U.sde_coef(F)
        tau = np.concatenate([[-1.0], np.diff(np.asarray(times_, dtype=np.float64))])
        tau_typ = U.sweep_representative(tau[1:], noise=False)
    A, Q = cm(model["A"][0]), cm(model["Q"][0])
    a = np.ascontiguousarray(model["a"][0], dtype=np.float64)
    H = np.ascontiguousarray(model["H"][0], dtype=np.float64)
    x0m = np.ascontiguousarray(model["x0m"], dtype=np.float64)
    x0P = cm(model["x0P"])
    yv = np.ascontiguousarray(np.where(np.isnan(y), 0.0, y), dtype=np.float64)
    mk = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    rn = np.ascontiguousarray(np.atleast_1d(Rnew if Rnew is not None else 0.0), dtype=np.float64)
    et, ee, e0 = (np.ascontiguousarray(e, dtype=np.float64) for e in eps)
    assert et.shape == (T, d) and ee.shape == (T,) and e0.shape == (d,)
    y_out, out = np.full(T, np.nan), np.zeros(8)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    p = U._p
    rc = sweepdrawsim().sweepdrawsim_run(
        d, int(sde is not None), U._i64(T), p(A), p(a), p(Q), p(H), ctypes.c_double(float(h[0])), ctypes.c_double(Rrep), p(x0m), p(x0P),
        p(coef), ctypes.c_double(tau_typ), p(yv), None if mk is None else mk.ctypes.data_as(u8), p(Rstep), p(hstep), p(tau), p(rn),
        int(rn.shape[0] > 1), p(et), p(ee), p(e0), C, W, Wd, w_hint, wd_hint, num_cu, p(y_out), p(out))
    return dict(rc=rc, status=int(out[1]), dist_f=out[2], dist_d=out[3], C=int(out[4]), W=int(out[5]), Wd=int(out[6]), nwaves=int(out[7]), y=y_out)


def sweepdrawsim_served(model, y, eps, **kw):
    """sweepdrawsim_run inside the repair loop of the C ABI's call (tgp_api_engines.inc sweep_draw_call): up to four attempts, a warm-up that a check found
    short doubled for the next one.  Returns the last attempt's dict with `attempts` and `tries` added."""
    w, wd = 0, 0
    tries = []
    for attempt in range(4):
        r = sweepdrawsim_run(model, y, eps, w_hint=w, wd_hint=wd, **kw)
        r["attempts"] = attempt + 1
        tries.append((r["C"], r["W"], r["Wd"], r["status"], float(r["dist_f"]), float(r["dist_d"])))
        r["tries"] = tries      # one (C, W, Wd, status, dist_f, dist_d) per attempt
        if r["rc"] != 0 or r["status"] & 12 or not r["status"] & 3:
            return r
        if r["status"] & 1:
            w = 2 * r["W"]
        if r["status"] & 2:
            wd = 2 * r["Wd"]
    return r


def draw_restated(model, y, missing, Rnew, eps):
    """The walk in NumPy, missing steps skipped: x_(T-1) = mf + chol(Pf + 1e-12 I).U' eps_0;  x_(t-1) = mf[t-1] + G (x_t - mp[t]) + chol(L + 1e-9 I).U' eps_t[t];
    y*_t = H x_t + h_t + sqrt(Rnew_t) eps_e[t].  (Parity with ref.rand on ref.posterior_missing: 2e-14 ... 5e-12, tests/test_sweep_draw_host.py.)"""
    T, d = model["T"], len(model["x0m"])
    et, ee, e0 = eps
    Rn = np.broadcast_to(np.asarray(Rnew, dtype=np.float64), (T,))
    miss = np.zeros(T, dtype=bool) if missing is None else np.asarray(missing, dtype=bool)
    cu = lambda M: np.linalg.cholesky(M).T      # noqa: E731
    m, P = model["x0m"].copy(), model["x0P"].copy()
    mf, Pf, mps, Pps, As = [], [], [], [], []
    for t in range(T):
        A, a, Q = ref.transition(model, t)
        H, h, R = ref.emission(model, t)
        mp, Pp = A @ m + a, A @ P @ A.T + Q
        if miss[t]:
            m, P = mp, Pp
        else:
            V = Pp @ H
            S = H @ V + R
            m, P = mp + V * (y[t] - H @ mp - h) / S, Pp - np.outer(V, V) / S
        mf.append(m), Pf.append(P), mps.append(mp), Pps.append(Pp), As.append(A)
    x = mf[T - 1] + cu(Pf[T - 1] + 1e-12 * np.eye(d)).T @ e0
    out = np.zeros(T)
    I = np.eye(d)
    for t in range(T - 1, -1, -1):
        H, h, _ = ref.emission(model, t)
        out[t] = H @ x + h + np.sqrt(Rn[t]) * ee[t]
        if t == 0:
            break
        Uc = cu(Pps[t] + 1e-10 * I)
        Gt = np.linalg.solve(Uc, np.linalg.solve(Uc.T, As[t] @ Pf[t - 1]))
        UG = Uc @ Gt
        L = Pf[t - 1] - UG.T @ UG
        x = mf[t - 1] + Gt.T @ (x - mps[t]) + cu(L + 1e-9 * I).T @ et[t]
    return out
