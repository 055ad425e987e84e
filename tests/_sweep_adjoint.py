"""Helpers of the sweep engine's adjoint-gradient tests (test infrastructure): a NumPy long-double restatement of the adjoint of the Kalman recursion
 over the oracle's model dict, and the host simulation of k_sweep_adjoint (tests/hostsim/sweepadjsim.cpp)."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _util as U

LD = np.longdouble
BLOCKS = U.GRADIENT_BLOCKS
LP_BAR, GRAD_BAR = 1e-10, 1e-8      # tests/test_gpu_adjoint_edges.py's bars: logpdf relative; a gradient entry relative to its block's largest


def restated(model, y, missing=None):
    """logpdf and its gradient by reverse mode through the sequential filter, in long double.  model: oracle dict with SHARED A, a, Q, H; h and R of length 1
    or T; missing: (T,) bool or None.  Returns (lml, g) with g as lgssm.logpdf_adjoint gives it (Q and x0P symmetrised; h and R: the sums over the observed
    steps) plus h_steps and R_steps (T,), zero at missing steps."""
    T, d = int(model["T"]), len(model["x0m"])
    A, a, Q, H = (np.asarray(model[k][0], dtype=LD) for k in ("A", "a", "Q", "H"))
    hs = np.broadcast_to(np.atleast_1d(np.asarray(model["h"], dtype=LD)), (T,))
    Rs = np.broadcast_to(np.atleast_1d(np.asarray(model["R"], dtype=LD)), (T,))
    miss = np.zeros(T, dtype=bool) if missing is None else np.asarray(missing, dtype=bool)
    yv = np.where(miss, 0.0, np.asarray(y, dtype=np.float64)).astype(LD)
    m, P = np.asarray(model["x0m"], dtype=LD), np.asarray(model["x0P"], dtype=LD)
    P = LD(0.5) * (P + P.T)
    ms, Ps = np.empty((T, d), dtype=LD), np.empty((T, d, d), dtype=LD)      # the filtering state in FRONT of every step
    lml = LD(0.0)
    log2pi = np.log(LD(2.0) * np.arccos(LD(-1.0)))
    for t in range(T):
        ms[t], Ps[t] = m, P
        m, P = A @ m + a, A @ P @ A.T + Q
        if not miss[t]:
            V = P @ H
            S = H @ V + Rs[t]
            v = yv[t] - H @ m - hs[t]
            lml -= LD(0.5) * (log2pi + np.log(S) + v * v / S)
            m, P = m + V * (v / S), P - np.outer(V, V) / S
    g = dict(A=np.zeros((d, d), dtype=LD), a=np.zeros(d, dtype=LD), Q=np.zeros((d, d), dtype=LD), H=np.zeros(d, dtype=LD))
    gh, gR = np.zeros(T, dtype=LD), np.zeros(T, dtype=LD)
    lam, Lam = np.zeros(d, dtype=LD), np.zeros((d, d), dtype=LD)
    for t in range(T - 1, -1, -1):
        m, P = ms[t], Ps[t]
        mp, AP = A @ m + a, A @ P
        Pp = AP @ A.T + Q
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
        g["A"] += np.outer(mb, m) + 2 * Pb @ AP
        g["a"] += mb
        g["Q"] += Pb
        lam, Lam = A.T @ mb, A.T @ Pb @ A
    g["x0m"], g["x0P"] = lam, Lam
    out = {k: np.asarray(v, dtype=np.float64) for k, v in g.items()}
    out["h"], out["R"] = float(gh.sum()), float(gR.sum())
    out["h_steps"], out["R_steps"] = gh.astype(np.float64), gR.astype(np.float64)
    return float(lml), out


def block_deviations(g, g_ref, blocks=BLOCKS):
    """{block: worst entry / the largest entry of the reference's own block}"""
    out = {}
    for k in blocks:
        sc = float(np.abs(np.asarray(g_ref[k])).max())
        out[k] = float(np.abs(np.asarray(g[k]) - np.asarray(g_ref[k])).max()) / (sc if sc > 0.0 else 1.0)
    return out


_SIM = None


def sweepadjsim():
    global _SIM
    if _SIM is None:
        src = os.path.join(U.HERE, "hostsim", "sweepadjsim.cpp")
        so = os.path.join(U.HERE, "hostsim", "libsweepadjsim.so")
        deps = [src] + [os.path.join(U.ROOT, "temporalgps.jl_amd", "csrc", f) for f in ("tgp_math.hpp", "tgp_sweep_body.hpp", "tgp_sweep_plan.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        _SIM = ctypes.CDLL(so)
        _SIM.sweepadjsim_run.restype = ctypes.c_int
    return _SIM


def sweepadjsim_run(model, y, missing=None, C=0, W=0, Wa=0, num_cu=1, w_hint=0, wa_hint=0):
    """model: oracle dict with SHARED A, a, Q, H; R / h may be per step.  Returns dict(rc, lml, status, dist_f, dist_a, C, W, Wa, nwaves, g) with g as
    `restated` gives it."""
    T, d = model["T"], len(model["x0m"])
    cm = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)      # noqa: E731
    R = np.atleast_1d(np.asarray(model["R"], dtype=np.float64))
    h = np.atleast_1d(np.asarray(model["h"], dtype=np.float64))
    Rstep = np.ascontiguousarray(R) if R.shape[0] > 1 else None
    hstep = np.ascontiguousarray(h) if h.shape[0] > 1 else None
    Rrep = U.sweep_representative(R, noise=True)
    A, Q = cm(model["A"][0]), cm(model["Q"][0])
    a = np.ascontiguousarray(model["a"][0], dtype=np.float64)
    H = np.ascontiguousarray(model["H"][0], dtype=np.float64)
    x0m = np.ascontiguousarray(model["x0m"], dtype=np.float64)
    x0P = cm(model["x0P"])
    yv = np.ascontiguousarray(np.where(np.isnan(y), 0.0, y), dtype=np.float64)
    mk = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    ghs, gRs, out = np.full(T, np.nan), np.full(T, np.nan), np.zeros(8)
    gv = np.zeros(3 * d * d + 4 * d + 2)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    p = U._p
    rc = sweepadjsim().sweepadjsim_run(
        d, U._i64(T), p(A), p(a), p(Q), p(H), ctypes.c_double(float(h[0])), ctypes.c_double(Rrep), p(x0m), p(x0P), p(yv),
        None if mk is None else mk.ctypes.data_as(u8), p(Rstep), p(hstep), C, W, Wa, w_hint, wa_hint, num_cu, p(ghs), p(gRs), p(gv), p(out))
    dd = d * d
    sq = lambda v: v.reshape(d, d).T.copy()      # noqa: E731  (column-major block -> [i][k])
    o = np.cumsum([0, dd, d, dd, d, 1, 1, d, dd])
    parts = [gv[o[i]:o[i + 1]] for i in range(8)]
    g = dict(A=sq(parts[0]), a=parts[1].copy(), Q=sq(parts[2]), H=parts[3].copy(), h=float(parts[4][0]), R=float(parts[5][0]), x0m=parts[6].copy(),
             x0P=sq(parts[7]), h_steps=ghs, R_steps=gRs)
    return dict(rc=rc, lml=out[0], status=int(out[1]), dist_f=out[2], dist_a=out[3], C=int(out[4]), W=int(out[5]), Wa=int(out[6]), nwaves=int(out[7]), g=g)


def sweepadjsim_served(model, y, **kw):
    """sweepadjsim_run inside the repair loop of the C ABI's call (tgp_api_engines.inc sweep_adjoint_call): up to four attempts, a warm-up that a check found
    short doubled for the next one.  Returns the last attempt's dict with `attempts` and `tries` added."""
    w, wa = 0, 0
    tries = []
    for attempt in range(4):
        r = sweepadjsim_run(model, y, w_hint=w, wa_hint=wa, **kw)
        r["attempts"] = attempt + 1
        tries.append((r["C"], r["W"], r["Wa"], r["status"], float(r["dist_f"]), float(r["dist_a"])))
        r["tries"] = tries      # one (C, W, Wa, status, dist_f, dist_a) per attempt
        if r["rc"] != 0 or r["status"] & 12 or not r["status"] & 3:
            return r
        if r["status"] & 1:
            w = 2 * r["W"]
        if r["status"] & 2:
            wa = 2 * r["Wa"]
    return r
