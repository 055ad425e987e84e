"""Shared by the group-sweep tests (tgp_sweep_group.hip): the models at d = 5 .. 8 and the stand-alone plan harness."""
import os
import subprocess

import numpy as np

from oracle import components as oc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

M52, M32 = ("matern52",), ("matern32",)
# (kernel, dt, noise variance): sums of Matern terms, the reference's everyday kernels just above the lane sweep's d <= 4
KERNELS = {
    5: (("sum", M52, M32), 0.1, 0.1),
    6: (("sum", M52, ("stretched", 0.7, M52)), 0.1, 0.1),
    7: (("sum", M52, M32, ("stretched", 0.7, M32)), 0.1, 0.1),
    8: (("sum", M52, ("stretched", 0.7, M52), M32), 0.1, 0.1),
}


def lti_model(d, T):
    k, dt, s2 = KERNELS[d]
    return oc.build_lgssm(k, ("regular", 0.0, dt, T), s2)


def plan_program(tmpdir):
    """tests/hostsim/sweep_group_plan.cpp, compiled for the host into tmpdir"""
    exe = os.path.join(str(tmpdir), "sweep_group_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "hostsim", "sweep_group_plan.cpp")])
    return exe


def write_model(path, model, d=None):
    """the shared blocks of an LTI oracle model as the plan program reads them (d: truncate / pad the state to another dimension -- decline cases)"""
    A, a, Q, H = model["A"][0], model["a"][0], model["Q"][0], model["H"][0]
    n = len(a)
    d = n if d is None else d

    def sq(M):
        out = np.eye(d) * (0.5 if M is A else 1.0)
        k = min(n, d)
        out[:k, :k] = M[:k, :k]
        return out

    def vec(v, fill=0.0):
        out = np.full(d, fill)
        out[:min(n, d)] = v[:min(n, d)]
        return out

    vals = np.concatenate([sq(A).ravel(order="F"), vec(a), sq(Q).ravel(order="F"), vec(H), [float(np.atleast_1d(model["h"])[0])], [float(np.atleast_1d(model["R"])[0])],
                           vec(model["x0m"]), sq(model["x0P"]).ravel(order="F")])
    with open(path, "w") as f:
        f.write(f"{d}\n" + "\n".join(repr(float(v)) for v in vals) + "\n")


def run_plan(exe, path, T, num_cu=256, post=1, fC=0, fW=0, fWb=0, w_hint=0, wb_hint=0):
    out = subprocess.run([exe, path] + [str(v) for v in (T, num_cu, post, fC, fW, fWb, w_hint, wb_hint)], check=True, capture_output=True, text=True).stdout.splitlines()
    if out[0].startswith("declined"):
        return dict(ok=False, why=out[0].split(": ", 1)[1])
    d, B, owned, C, W, Wb, nchunks, nwaves = (int(v) for v in out[0].split()[1:])
    spans = [tuple(int(v) for v in ln.split()[1:]) for ln in out[1:]]
    return dict(ok=True, d=d, B=B, owned=owned, C=C, W=W, Wb=Wb, nchunks=nchunks, nwaves=nwaves, spans=spans)


def device_model(tgp, model, sweep=2):
    """the LTI device model with TGP_OPT_SWEEP = 2: every (d, call) pair on the group sweep, not only the pairs the default routing takes
    (tgp_api_engines.inc sweep_group_default_route); sweep=None: the default routing"""
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    if sweep is not None:
        dm.handle().set_option(tgp._lib.OPT_SWEEP, sweep)
    return dm
