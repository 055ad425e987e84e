"""Shared by the CPU tests of the group sweep on SDE-described models (tgp_sweep_group_sde.hip): the closed form of exp(F tau) as
tgp_api.hip sde_closed_form finds it, restated in NumPy, and the stand-alone plan harness."""
import os
import subprocess

import numpy as np

from oracle import components as oc

HERE = os.path.dirname(os.path.abspath(__file__))


def sde_blocks(k):
    """(F, H, Pinf, blocks) of a sum of Matern terms: F block-diagonal, blocks = the index ranges of the summands"""
    terms = k[1:] if k[0] == "sum" else (k,)
    Fs, Hs, Ps = zip(*[(oc.to_sde(t)[0], oc.to_sde(t)[2], oc.stationary_distribution(t)[1]) for t in terms])
    d = sum(F.shape[0] for F in Fs)
    F, P, blocks, o = np.zeros((d, d)), np.zeros((d, d)), [], 0
    for Fb, Pb in zip(Fs, Ps):
        n = Fb.shape[0]
        F[o:o + n, o:o + n], P[o:o + n, o:o + n] = Fb, Pb
        blocks.append((o, o + n))
        o += n
    return F, np.concatenate(Hs), P, blocks


def closed_form(F, blocks):
    """lam per row, N1 = F + lam I per block, N2 = N1^2 / 2: exp(F tau) = diag(e^(-lam tau)) (I + tau N1 + tau^2 N2)"""
    d = F.shape[0]
    lam, N1, N2 = np.zeros(d), np.zeros((d, d)), np.zeros((d, d))
    for lo, hi in blocks:
        n = hi - lo
        l = -np.trace(F[lo:hi, lo:hi]) / n
        Nb = F[lo:hi, lo:hi] + l * np.eye(n)
        lam[lo:hi] = l
        if n >= 2:
            N1[lo:hi, lo:hi] = Nb
        if n >= 3:
            N2[lo:hi, lo:hi] = 0.5 * Nb @ Nb
    return lam, N1, N2


def step_A(lam, N1, N2, tau):
    """the kernel's A_t (tgp_sweep_body.hpp sde_A)"""
    return np.exp(-lam * tau)[:, None] * (np.eye(len(lam)) + tau * N1 + tau * tau * N2)


def plan_program(tmpdir):
    exe = os.path.join(str(tmpdir), "sweep_group_sde_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "hostsim", "sweep_group_sde_plan.cpp")])
    return exe


def write_model(path, k, model, tau_typ, d=None, R=None):
    """an SDE-described oracle model (irregular inputs: per-step A, Q) as the plan program reads it; d: truncate / pad the state (decline cases)"""
    F, H, P, blocks = sde_blocks(k)
    lam, N1, N2 = closed_form(F, blocks)
    n = len(lam)
    d = n if d is None else d

    def sq(M, diag=0.0):
        out = np.eye(d) * diag
        q = min(n, d)
        out[:q, :q] = M[:q, :q]
        return out

    def vec(v, fill=0.0):
        out = np.full(d, fill)
        out[:min(n, d)] = np.asarray(v)[:min(n, d)]
        return out

    A1, Q1 = sq(model["A"][0], 0.5), sq(model["Q"][0])
    Pd = sq(P, 1.0)
    if d != n:
        Q1 = Pd - A1 @ Pd @ A1.T
    vals = np.concatenate([vec(lam, 1.0), sq(N1).ravel(order="F"), sq(N2).ravel(order="F"), vec(model["a"][0]), vec(H), [0.0],
                           [float(np.atleast_1d(model["R"])[0]) if R is None else R], vec(model["x0m"]), Pd.ravel(order="F"), A1.ravel(order="F"),
                           Q1.ravel(order="F"), [tau_typ]])
    with open(path, "w") as f:
        f.write(f"{d}\n" + "\n".join(repr(float(v)) for v in vals) + "\n")


def run_plan(exe, path, T, num_cu=256, post=1, fC=0, fW=0, fWb=0, w_hint=0, wb_hint=0):
    out = subprocess.run([exe, path] + [str(v) for v in (T, num_cu, post, fC, fW, fWb, w_hint, wb_hint)], check=True, capture_output=True, text=True).stdout.splitlines()
    if out[0].startswith("declined"):
        return dict(ok=False, why=out[0].split(": ", 1)[1])
    d, B, owned, C, W, Wb, nchunks, nwaves = (int(v) for v in out[0].split()[1:])
    spans = [tuple(int(v) for v in ln.split()[1:]) for ln in out[1:] if ln.startswith("span")]
    extra = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out[1:] if not ln.startswith("span")}
    return dict(ok=True, d=d, B=B, owned=owned, C=C, W=W, Wb=Wb, nchunks=nchunks, nwaves=nwaves, spans=spans, **extra)


def typical_gap(t):
    """the binding's typical gap (tgp_model_set_sde): the median of the first 4096 gaps, as nth_element leaves it"""
    g = np.sort(np.diff(np.asarray(t, dtype=np.float64))[:4096])
    return float(g[len(g) // 2]) if len(g) else 1.0


REPAIR_D, REPAIR_T, REPAIR_SEED = 5, 5003, 39


def repair_gaps(dt, C, W, stretched=True):
    """The repair case (tests/test_sweep_group_sde_host.py shows its distances, tests/test_gpu_sweep_group_sde.py runs it): gaps U(0.5, 1.5) dt and,
    behind the edge of chunk 10 of the plan's geometry (C, W of the unstretched series), W / 2 gaps of 0.003 dt -- steps through which the filter forgets
    hardly anything, so that the first guess W leaves W / 2 ordinary steps in front of the edge and the doubled one 3 W / 2"""
    gaps = np.random.default_rng(9).uniform(0.5 * dt, 1.5 * dt, REPAIR_T)
    if stretched:
        e = 10 * C
        gaps[e - W // 2:e] = 0.003 * dt
    return gaps
