"""GPU tier (-m gpu): the group sweep (tgp_sweep_group.hip) at its edges -- forced geometries (TGP_OPT_SWEEP_CHUNK / _WARMUP /
_WARMUP_BACK: reported, never repaired), a partly filled last wave, a short last chunk, runs of missing steps over chunk and checkpoint-block
edges, the repair loop, the requests that send a call to the general engine, what stays unsupported at d >= 5, and the error path.  Values against
the oracle's C restatement with the project's tolerances (logpdf 1e-10 relative, marginals 1e-8 of their scale)."""
import ctypes

import numpy as np
import pytest

from oracle import seq_kalman as sk
from tests import _sweep_group as SG
from tests import _util as U
from tests.test_gpu_sweep import _reference

pytestmark = pytest.mark.gpu

NAMES = {"k_sweep_group<lti,logpdf>", "k_sweep_group<lti,posterior>"}
T_EDGE = 4100      # 65 chunks of 64 steps: the last one 4 steps long, the last wave (6 / 7 chunks per wave) partly filled
DT_EDGE = 0.5      # (a grid on which the filter forgets within a chunk of 64 steps)


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


@pytest.fixture(scope="module")
def edge_case():
    """one series per d with runs of missing steps: a whole chunk and both its edges, a checkpoint-block edge, the series' ends; its reference, computed once"""
    out = {}
    for d in (5, 8):
        k, _, s2 = SG.KERNELS[d]
        model, y, _ = U.gp_case(k, ("regular", 0.0, DT_EDGE, T_EDGE), s2, seed=20 + d)
        missing = np.random.default_rng(30 + d).random(T_EDGE) < 0.1
        missing[630:710] = True         # chunk [640, 704) whole, straddling both its edges
        missing[1030:1036] = True       # the block edge at 1032 (B = 8 and B = 4)
        missing[1276:1284] = True       # a chunk edge (1280) inside a run
        missing[0] = True
        missing[T_EDGE - 3:] = True
        lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
        out[d] = dict(model=model, y=y, missing=missing, yin=np.where(missing, np.nan, y), lp=lp, pm=pm, pv=pv)
    return out


def _values_ok(c, lp, mean=None, var=None):
    assert abs(lp - c["lp"]) <= 1e-10 * abs(c["lp"]), (lp, c["lp"])
    if mean is not None:
        assert np.abs(mean - c["pm"]).max() <= 1e-8 * max(1.0, np.abs(c["pm"]).max())
        assert np.abs(var - c["pv"]).max() <= 1e-8 * max(1.0, c["pv"].max())


def _both_calls(tgp, dm, c):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    lp = tgp.logpdf(dm, c["yin"])
    i1 = hd.sweep_info()
    lp2, mean, var = tgp.logpdf_and_posterior_marginals(dm, c["yin"], np.array([1e-18]))
    i2 = hd.sweep_info()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    print(i1, i2, names)
    _values_ok(c, lp)
    _values_ok(c, lp2, mean, var)
    return i1, i2, names


@pytest.mark.parametrize("d", [5, 8])
def test_short_chunks_a_partly_filled_wave_and_a_backward_warm_up_as_long_as_the_chunk(tgp, edge_case, d):
    c = edge_case[d]
    dm = SG.device_model(tgp, c["model"])
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_SWEEP_CHUNK, 64)
    hd.set_option(tgp._lib.OPT_SWEEP_WARMUP_BACK, 64)
    i1, i2, names = _both_calls(tgp, dm, c)
    for info, owned in ((i1, 7), (i2, 6)):
        assert info["served"] == 1 and info["attempts"] == 1 and info["status"] == 0, info
        assert info["C"] == 64 and info["Wb"] == 64 and info["waves"] == -(-65 // owned), info
    assert names == NAMES, names


@pytest.mark.parametrize("d", [5, 8])
def test_a_forced_warm_up_that_is_too_short_is_reported_not_repaired(tgp, edge_case, d):
    c = edge_case[d]
    dm = SG.device_model(tgp, c["model"])
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_SWEEP_CHUNK, 64)
    hd.set_option(tgp._lib.OPT_SWEEP_WARMUP, 8)
    i1, i2, names = _both_calls(tgp, dm, c)      # (the values are the general engine's)
    for info in (i1, i2):
        assert info["served"] == 0 and info["status"] & 1 and info["attempts"] == 1 and info["W"] == 8, info
    assert NAMES <= names and any(n.startswith("k_group") or n.startswith("k_reduce") or n.startswith("k_apply") for n in names), names


def _repaired_or_handed_over(tgp, model, y, missing, launched):
    """the outcome the repair loop allows for a series whose warm-ups the plan underestimates: served after >= 2 attempts, or the engine switched off for
    the bound model and the next call launching nothing of it; the values are right either way"""
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    c = dict(yin=np.where(missing, np.nan, y), lp=lp, pm=pm, pv=pv)
    dm = SG.device_model(tgp, model)
    hd = dm.handle()
    lp2, mean, var = tgp.logpdf_and_posterior_marginals(dm, c["yin"], np.array([1e-18]))
    info = hd.sweep_info()
    print(info)
    _values_ok(c, lp2, mean, var)
    if info["served"] == 1:
        assert info["attempts"] >= 2 and info["state"] == 1, info
    else:
        assert info["state"] == -1 and info["attempts"] >= launched, info
        hd.set_option(tgp._lib.OPT_PROFILE, 1)
        hd.profile_reset()
        _values_ok(c, tgp.logpdf(dm, c["yin"]))
        assert hd.sweep_info()["attempts"] == 0 and not any(n.startswith("k_sweep") for n in hd.profile())
        hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return info


def test_a_slowly_forgetting_series_is_handed_over_by_the_plan(tgp):
    """Matern-3/2 terms, one of them stretched by 0.1, with the first and last 800 of 4096 steps missing.  This case covers the PLAN's decline only: the
    backward warm-up the plan estimates no longer leaves six chunks of 4096 steps, so the engine is switched off without a launch (attempts == 0) and the
    general engine serves the call.  With stretches (0.7, 0.5) and (0.25, 0.5) the estimate -- W = 352 / 640, Wb = 328 / 592 -- holds at the first attempt
    (measured distances 2e-14 / 1.4e-13): stretches of missing steps at the ends do not make a hand-over fail, because a warm-up inside them starts from
    the exact state.  The repair loop itself is the next test's."""
    T = 4096
    k = ("sum", SG.M32, ("stretched", 0.1, SG.M32), ("stretched", 0.5, SG.M32))
    model, y, _ = U.gp_case(k, ("regular", 0.0, 0.1, T), 0.1, seed=5)
    assert len(model["x0m"]) == 6
    missing = np.zeros(T, dtype=bool)
    missing[:800] = True
    missing[T - 800:] = True
    _repaired_or_handed_over(tgp, model, y, missing, launched=0)


def test_sparse_observations_fail_the_first_hand_over_check_unforced(tgp):
    """one step in sixteen observed: the filter forgets far more slowly, in steps, than the plan's estimate for a series observed at every step, so the first
    attempt's hand-over check fails without any forced geometry and sweep_run doubles the warm-ups: served after >= 2 attempts, or -- warm-ups beyond four
    chunks / still short after four attempts -- declined after at least one launch, the engine off for the bound model"""
    T = 8192
    k, dt, s2 = SG.KERNELS[5]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=7)
    missing = np.ones(T, dtype=bool)
    missing[::16] = False
    info = _repaired_or_handed_over(tgp, model, y, missing, launched=1)
    assert info["attempts"] >= 2 or info["status"] & 3, info


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_default_routing_takes_the_measured_winners_only(tgp, d):
    """TGP_OPT_SWEEP = 1 (the default): logpdf at d = 6, 7, 8 runs on the group sweep, logpdf at d = 5 and the combined call at every d stay on the general
    engine (profiles/sweep_group_time.txt: they lose at T = 1e6 or 1e7); TGP_OPT_SWEEP = 2 is what every other test here sets"""
    T = 2048
    k, dt, s2 = SG.KERNELS[d]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=60 + d)
    missing = np.random.default_rng(d).random(T) < 0.1
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    c = dict(yin=np.where(missing, np.nan, y), lp=lp, pm=pm, pv=pv)
    i1, i2, names = _both_calls(tgp, SG.device_model(tgp, model, sweep=None), c)
    assert i1["served"] == int(d >= 6) and i2["served"] == 0 and i2["attempts"] == 0, (i1, i2)
    assert ("k_sweep_group<lti,logpdf>" in names) == (d >= 6) and "k_sweep_group<lti,posterior>" not in names, names


@pytest.mark.parametrize("option,value", [("OPT_SWEEP", 0), ("OPT_CHUNK", 16)])
def test_requests_for_the_general_engine(tgp, edge_case, option, value):
    c = edge_case[5]
    dm = SG.device_model(tgp, c["model"])
    dm.handle().set_option(getattr(tgp._lib, option), value)
    i1, i2, names = _both_calls(tgp, dm, c)
    assert i1["served"] == 0 and i2["served"] == 0 and i1["attempts"] == 0 and i2["attempts"] == 0, (i1, i2)
    assert not any(n.startswith("k_sweep") for n in names), names


def test_the_adjoint_and_the_draw_stay_unsupported_at_d5(tgp, edge_case):
    c = edge_case[5]
    dm = SG.device_model(tgp, c["model"])
    hd = dm.handle()
    with pytest.raises(tgp._lib.Unsupported):
        tgp.lgssm.logpdf_adjoint_missing(dm, c["yin"])
    assert hd.sweep_info()["attempts"] == 0
    T, d = T_EDGE, 5
    rng = np.random.default_rng(1)
    yy = np.ascontiguousarray(np.where(c["missing"], 0.0, c["y"]))
    mm = np.ascontiguousarray(c["missing"].astype(np.uint8))
    Rn, et, ee, e0 = np.array([1e-18]), rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d)
    out = np.full(T, -7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = hd.lib.tgp_posterior_rand_missing(hd.h, p(yy), p(mm), p(Rn), p(et), p(ee), p(e0), tgp._lib.SHARED_R, p(out))
    assert rc == tgp._lib.EUNSUPPORTED and np.all(out == -7.0) and hd.sweep_info()["attempts"] == 0


def test_a_negative_noise_variance_inside_a_chunk_takes_the_general_engines_error_path(tgp):
    d, T = 5, 4100
    k, _, _ = SG.KERNELS[d]
    S = np.full(T, 0.1)
    S[1000] = -10.0      # inside chunk 15 of 64 steps: the innovation variance of that step is negative
    model, y, _ = U.gp_case(k, ("regular", 0.0, DT_EDGE, T), np.abs(S), seed=6)
    model = dict(model, R=S)

    def outcome(dm):
        try:
            return ("values", tgp.logpdf(dm, y))
        except Exception as e:      # noqa: BLE001 (the exception IS the outcome that is compared)
            return ("raised", type(e), str(e))

    dm, off = SG.device_model(tgp, model), SG.device_model(tgp, model, sweep=0)
    dm.handle().set_option(tgp._lib.OPT_SWEEP_CHUNK, 64)
    got = outcome(dm)
    info = dm.handle().sweep_info()
    print(info, got)
    assert info["served"] == 0 and info["status"] & 4 and info["attempts"] == 1 and info["state"] == -1, info
    want = outcome(off)
    assert off.handle().sweep_info()["attempts"] == 0
    assert got[0] == want[0]
    if got[0] == "raised":
        assert got[1:] == want[1:], (got, want)
    else:
        np.testing.assert_allclose(got[1], want[1], rtol=1e-12, equal_nan=True)


def test_the_served_flag_is_cleared_by_a_later_call_of_a_stationary_engine(tgp, edge_case):
    c = edge_case[5]
    dm = SG.device_model(tgp, c["model"])
    hd = dm.handle()
    _values_ok(c, tgp.logpdf(dm, c["yin"]))
    assert hd.sweep_info()["served"] == 1
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    got = tgp.logpdf(dm, c["y"])      # fully observed, one noise variance: the stationary-gain engines' (the sweep engines are never asked)
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    assert not any(n.startswith("k_sweep") for n in names), names
    assert hd.sweep_info()["served"] == 0 and hd.sweep_info()["attempts"] == 0
    want = sk.logpdf(c["model"], c["y"])
    assert abs(got - want) <= 1e-10 * abs(want)
