"""CPU tier: the sweep engine's adjoint gradient (tgp_sweep.hip k_sweep_adjoint) run on the host -- the product's own plan and per-lane code
(tests/hostsim/sweepadjsim.cpp) -- against the long-double restatement of the adjoint recursion (tests/_sweep_adjoint.py, itself held against
oracle/seq_adjoint and central differences in tests/test_sweep_adjoint_ref.py).  Bars: logpdf 1e-10 relative, a gradient entry 1e-8 of its block's largest
(tests/test_gpu_adjoint_edges.py's), the hand-over distances 1e-12 forwards and 1e-11 backwards (the plan's kTol / kTolBack)."""
import numpy as np
import pytest

from tests import _sweep_adjoint as SA
from tests import _util as U
from tests.test_sweep_host import CASES

ALL = SA.BLOCKS + ("h_steps", "R_steps")


def _check(r, lp, g):
    assert r["rc"] == 0 and r["status"] == 0, {k: v for k, v in r.items() if k != "g"}
    assert r["dist_f"] <= 1e-12 and r["dist_a"] <= 1e-11, (r["dist_f"], r["dist_a"])
    assert abs(r["lml"] - lp) <= SA.LP_BAR * abs(lp), (r["lml"], lp)
    dev = SA.block_deviations(r["g"], g, ALL)
    print({k: f"{v:.1e}" for k, v in dev.items()}, "dist", r["dist_f"], r["dist_a"], "C W Wa", r["C"], r["W"], r["Wa"])
    assert max(dev.values()) <= SA.GRAD_BAR, dev


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("T", [700, 1203])
def test_missing_data_on_a_regular_grid(i, T):
    k, dt, s2 = CASES[i]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=i)
    rng = np.random.default_rng(100 + i)
    missing = rng.random(T) < 0.1
    missing[5:9] = True
    lp, g = SA.restated(model, y, missing)
    r = SA.sweepadjsim_served(model, np.where(missing, np.nan, y), missing=missing, num_cu=1)
    _check(r, lp, g)
    assert np.all(r["g"]["h_steps"][missing] == 0.0) and np.all(r["g"]["R_steps"][missing] == 0.0)


@pytest.mark.parametrize("i", [1, 2, 3])
def test_per_step_noise_and_offset(i):
    k, dt, s2 = CASES[i]
    T = 900
    rng = np.random.default_rng(7 + i)
    S = s2 * (0.5 + rng.random(T))
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), S, seed=i, mean=("custom", lambda t: np.sin(t)))
    missing = rng.random(T) < 0.1
    lp, g = SA.restated(model, y, missing)
    _check(SA.sweepadjsim_served(model, y, missing=missing), lp, g)
    lp, g = SA.restated(model, y)      # no mask
    _check(SA.sweepadjsim_served(model, y), lp, g)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [1000, 1001])
def test_chunks_of_eight_steps_across_wave_seams(d, T):
    """125 and 126 chunks: two wave seams, a last chunk of one step; the fast-forgetting spacing of tests/_sweep_edges.py, where eight steps are a warm-up"""
    from tests import _sweep_edges as E
    model, y, _ = U.gp_case(E.MODELS[d], ("regular", 0.0, E.FAST_DT[d], T), E.S2, seed=d)
    missing = np.random.default_rng(d).random(T) < 0.1
    missing[0] = missing[T - 1] = True
    lp, g = SA.restated(model, y, missing)
    r = SA.sweepadjsim_run(model, y, missing=missing, C=8, W=8, Wa=8)
    assert r["nwaves"] == 3
    _check(r, lp, g)


def test_short_adjoint_warm_up_is_detected_and_the_plans_own_geometry_passes():
    k, dt, s2 = CASES[5]                    # the bench parametrisation: slow mixing (dt = 0.05, l = 2.3)
    T = 3000
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=3)
    missing = np.random.default_rng(1).random(T) < 0.1
    lp, g = SA.restated(model, y, missing)
    r = SA.sweepadjsim_run(model, y, missing=missing, C=64, Wa=16)
    assert r["status"] & 2 and r["dist_a"] > 1e-11, (r["status"], r["dist_a"])
    r = SA.sweepadjsim_served(model, y, missing=missing)       # the plan's own estimate, repaired as the C ABI's call repairs it
    print(r["tries"])
    _check(r, lp, g)
    assert r["Wa"] <= r["C"]
