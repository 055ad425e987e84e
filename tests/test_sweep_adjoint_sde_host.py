"""CPU tier: the sweep engine's adjoint gradient for SDE-described models (tgp_sweep.hip k_sweep_adjoint_sde) run on the host -- the product's
own plan and per-lane code (tests/hostsim/sweepadjsdesim.cpp) -- against the long-double restatement of the walk (tests/_sweep_adjoint_sde.py, itself held
against oracle/seq_adjoint and central differences in tests/test_sweep_adjoint_sde_ref.py).  Bars: logpdf 1e-10 relative, a gradient entry 1e-8 of its
block's largest (tests/_sweep_adjoint.py's LP_BAR / GRAD_BAR), the hand-over distances 1e-12 forwards and 1e-11 backwards (the plan's kTol / kTolBack)."""
import numpy as np
import pytest

from tests import _sweep_adjoint_sde as SS

ALL = SS.BLOCKS + ("lam", "N1", "N2", "h_steps", "R_steps")


def _run(c, **kw):
    return SS.sim_run(times=c["times"], y=c["y"], missing=c["missing"], **c["blocks"], **kw)


def _served(c):
    """the repair loop of the C ABI's call: up to four attempts, a warm-up that a check found short doubled for the next one"""
    w = wa = 0
    for _ in range(4):
        r = _run(c, w_hint=w, wa_hint=wa)
        if r["rc"] != 0 or r["status"] & 12 or not r["status"] & 3:
            return r
        w, wa = (2 * r["W"] if r["status"] & 1 else w), (2 * r["Wa"] if r["status"] & 2 else wa)
    return r


def _check(r, c):
    lp, g = c["lp"], c["g"]
    assert r["rc"] == 0 and r["status"] == 0, {k: v for k, v in r.items() if k != "g"}
    assert r["dist_f"] <= 1e-12 and r["dist_a"] <= 1e-11, (r["dist_f"], r["dist_a"])
    assert abs(r["lml"] - lp) <= SS.LP_BAR * abs(lp), (r["lml"], lp)
    dev = SS.block_deviations(r["g"], g, ALL)
    print({k: f"{v:.1e}" for k, v in dev.items()}, "dist", r["dist_f"], r["dist_a"], "C W Wa", r["C"], r["W"], r["Wa"])
    assert max(dev.values()) <= SS.GRAD_BAR, dev
    m = c["missing"]
    assert np.all(r["g"]["h_steps"][m] == 0.0) and np.all(r["g"]["R_steps"][m] == 0.0)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("xs", [0, 3])
def test_irregular_times_with_the_plans_own_geometry(d, xs):
    """T = 1203: a last block of three steps; ties, a gap of 50 typical gaps, a prior that is not the stationary one"""
    c = SS.case(d, 1203, xs=xs, x0=True)
    _check(_served(c), c)


def test_a_component_of_three_beside_one():
    c = SS.case(4, 900, xs=1, kernel=("sum", SS.M52, SS.M12))
    _check(_served(c), c)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [1000, 1001])
def test_chunks_of_eight_steps_across_wave_seams(d, T):
    """125 and 126 chunks: two wave seams (62 chunks per wave), a last chunk of one step; at the fast-forgetting spacing eight steps are a warm-up"""
    c = SS.case(d, T, xs=2, fast=True, x0=True)
    r = _run(c, C=8, W=8, Wa=8)
    assert r["nwaves"] == 3
    _check(r, c)


def test_short_adjoint_warm_up_is_detected_and_the_plans_own_geometry_passes():
    c = SS.case(3, 3000, kernel=("stretched", 1.0 / 2.3, SS.M52))      # slow mixing: a length scale of 23 typical gaps
    r = _run(c, C=64, Wa=16)
    assert r["status"] & 2 and r["dist_a"] > 1e-11, (r["status"], r["dist_a"])
    r = _served(c)
    _check(r, c)
    assert r["Wa"] <= r["C"]
