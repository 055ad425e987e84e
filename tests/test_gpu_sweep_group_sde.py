"""GPU tier (-m gpu): the group sweep on SDE-described models (tgp_sweep_group_sde.hip) -- irregular inputs at d = 5 .. 8 bound by
tgp_model_set_sde, the transition of every step built in the kernel from its gap -- through the C ABI against the oracle, as
tests/test_gpu_sweep.py::test_irregular_spacing checks the lane sweep.  Tolerances as everywhere: logpdf 1e-10 relative, posterior mean
1e-8 of max(1, |mean|), variance 1e-8 of max(1, var).  Every model is bound with build_lgssm(..., device_components=True) and runs under
TGP_OPT_SWEEP = 2 on its handle; every parity case asserts that the engine served the call (tgp_sweep_info) and that the profile names its two
kernels and no other: no case passes by falling back."""
import numpy as np
import pytest

from tests import _sweep_group as SG
from tests import _sweep_group_sde as SS
from tests import _util as U
from tests.test_gpu_sweep import _reference

pytestmark = pytest.mark.gpu

NAMES = {"k_sweep_group<sde,logpdf>", "k_sweep_group<sde,posterior>"}
DT_EDGE = 0.5      # (median gap at which the filter forgets within a forced chunk of 64 steps: a forced geometry is reported, never repaired)
M52, M32 = SG.M52, SG.M32


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _bind(tgp, k, t, s2, mean=None, sweep=2):
    from temporalgps_jl_amd import lti_sde as P
    dm = P.build_lgssm(P.to_kernel(k), t, s2, mean=mean, device_components=True)
    if sweep is not None:
        dm.handle().set_option(tgp._lib.OPT_SWEEP, sweep)
    return dm


def _errors(got, lp, mean, pm, var, pv):
    return (abs(got - lp) / abs(lp), np.abs(mean - pm).max() / max(1.0, np.abs(pm).max()), np.abs(var - pv).max() / max(1.0, pv.max()))


def _check(tgp, dm, yin, Rn, lp, pm, pv, served=True):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    got = tgp.logpdf(dm, yin)
    info = hd.sweep_info()
    print("logpdf", info, abs(got - lp) / abs(lp))
    assert info["served"] == int(served), info
    assert abs(got - lp) <= 1e-10 * abs(lp), (got, lp, info)
    got2, mean, var = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = hd.sweep_info()
    print("posterior", info, _errors(got2, lp, mean, pm, var, pv))
    assert info["served"] == int(served), info
    assert abs(got2 - lp) <= 1e-10 * abs(lp), (got2, lp, info)
    assert np.abs(mean - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max()), info
    assert np.abs(var - pv).max() <= 1e-8 * max(1.0, pv.max()), info
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    if served:
        mean2, var2 = tgp.posterior_marginals(dm, yin, Rn)
        assert hd.sweep_info()["served"] == 1 and np.array_equal(mean2, mean) and np.array_equal(var2, var)
        assert names == NAMES, names
    else:
        assert not any(n.startswith("k_sweep_group") for n in names), names
    return info


def _times(T, dt, seed, lo=0.5, hi=1.5):
    return np.cumsum(np.random.default_rng(seed).uniform(lo * dt, hi * dt, T))


def _mask(T, seed, frac=0.15):
    missing = np.random.default_rng(seed).random(T) < frac
    missing[:3] = True
    missing[5:9] = True
    missing[T - 3:] = True
    return missing


@pytest.mark.parametrize("T", [2048, 5003])
@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_plan_geometry_every_dimension_and_stream_set(tgp, d, T):
    """gaps U(0.5, 1.5) dt, 15 % missing with a missing head and tail; the four stream sets XS = 0 .. 3 go round with (d, T); Rnew per step where
    both streams are"""
    from temporalgps_jl_amd import lti_sde as P
    k, dt, s2 = SG.KERNELS[d]
    xs = (d + (T > 3000)) % 4
    rng = np.random.default_rng(10 * d + xs)
    t = _times(T, dt, 40 + d)
    S = rng.uniform(0.05, 0.5, T) if xs & 1 else s2
    mean_o = ("custom", lambda tt: np.cos(0.3 * tt)) if xs & 2 else None
    mean_d = P.CustomMean(lambda v: np.cos(0.3 * v)) if xs & 2 else None
    model, y, _ = U.gp_case(k, t, S, seed=d, mean=mean_o)
    assert len(model["x0m"]) == d
    missing = _mask(T, 100 + d)
    Rn = rng.random(T) * 0.05 if xs == 3 else np.array([1e-18])
    lp, pm, pv = _reference(model, y, missing, Rn if xs == 3 else 1e-18, fast=True)
    info = _check(tgp, _bind(tgp, k, t, S, mean=mean_d), np.where(missing, np.nan, y), Rn, lp, pm, pv)
    assert info["attempts"] == 1 and info["Wb"] <= info["C"] and info["C"] % 8 == 0, info


@pytest.mark.parametrize("d", [6, 8])
def test_forced_chunks_cross_wave_seams_and_a_last_chunk_of_four_steps(tgp, d):
    """C = 64 at T = 4100: 65 chunks, 10 or 11 waves, the last chunk 4 steps; group_block = 8 (d = 6) and 4 (d = 8)"""
    k, _, s2 = SG.KERNELS[d]
    T = 4100
    t = _times(T, DT_EDGE, 7 + d)
    model, y, _ = U.gp_case(k, t, s2, seed=20 + d)
    missing = _mask(T, 30 + d)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    dm = _bind(tgp, k, t, s2)
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_SWEEP_CHUNK, 64)
    hd.set_option(tgp._lib.OPT_SWEEP_WARMUP_BACK, 64)
    info = _check(tgp, dm, np.where(missing, np.nan, y), np.array([1e-18]), lp, pm, pv)
    assert info["C"] == 64 and info["waves"] == 11 and info["status"] == 0, info      # (the posterior call: 65 chunks, 6 per wave)


def test_first_transition_given_and_defaulted(tgp):
    """given: a stretched term, so that A1 (dt_1 = 1 in every term's own stretched time) is exp(F tau) of no tau; defaulted: the binding's dt_1 := 1,
    which for unstretched terms is the reference's own first step"""
    from temporalgps_jl_amd import lgssm as L
    from temporalgps_jl_amd import lti_sde as P
    T = 2500
    k, dt, s2 = SG.KERNELS[7]
    t = _times(T, dt, 3)
    model, y, _ = U.gp_case(k, t, s2, seed=31)
    lp, pm, pv = _reference(model, y, None, 1e-18, fast=True)
    _check(tgp, _bind(tgp, k, t, s2), y, np.array([1e-18]), lp, pm, pv)
    k, dt, s2 = SG.KERNELS[5]
    model, y, _ = U.gp_case(k, t, s2, seed=32)
    lp, pm, pv = _reference(model, y, None, 1e-18, fast=True)
    F, H, m0, P0 = P.to_kernel(k).sde_blocks()
    trans = L.SDETransitions(L.Forward, F, t, L.Gaussian(np.asarray(m0, float), np.asarray(P0, float)))
    dm = L.LGSSM(trans, L.ScalarOutputLGC(np.asarray(H, float)[None], np.zeros(1), np.array([s2])), T=T)
    dm.handle().set_option(tgp._lib.OPT_SWEEP, 2)
    _check(tgp, dm, y, np.array([1e-18]), lp, pm, pv)


def test_runs_of_equal_time_stamps_also_across_a_chunk_edge(tgp):
    k, _, s2 = SG.KERNELS[6]
    T, dt = 4100, DT_EDGE
    gaps = np.random.default_rng(5).uniform(0.5 * dt, 1.5 * dt, T)
    gaps[100:104] = 0.0
    gaps[62:67] = 0.0          # across the edge of chunk 0 (C = 64)
    gaps[1022:1027] = 0.0      # ... and of a wave's last owned chunk
    gaps[T - 2:] = 0.0
    t = np.cumsum(gaps)
    model, y, _ = U.gp_case(k, t, s2, seed=33)
    missing = _mask(T, 34)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    dm = _bind(tgp, k, t, s2)
    dm.handle().set_option(tgp._lib.OPT_SWEEP_CHUNK, 64)
    dm.handle().set_option(tgp._lib.OPT_SWEEP_WARMUP_BACK, 64)
    _check(tgp, dm, np.where(missing, np.nan, y), np.array([1e-18]), lp, pm, pv)


@pytest.mark.parametrize("d", [5, 8])
def test_log_uniform_gaps_over_six_decades(tgp, d):
    k, dt, s2 = SG.KERNELS[d]
    T = 3001
    t = np.cumsum(10.0 ** np.random.default_rng(50 + d).uniform(-4.0, 2.0, T))
    model, y, _ = U.gp_case(k, t, s2, seed=35 + d)
    missing = _mask(T, 36 + d)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    _check(tgp, _bind(tgp, k, t, s2), np.where(missing, np.nan, y), np.array([1e-18]), lp, pm, pv)


def test_identical_summands_share_their_decay_rate(tgp):
    """Matern52 + Matern52: equal lam in two blocks (one exponential serves both)"""
    k, dt, s2 = ("sum", M52, M52), 0.1, 0.1
    T = 2500
    t = _times(T, dt, 8)
    model, y, _ = U.gp_case(k, t, s2, seed=37)
    missing = _mask(T, 38)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    _check(tgp, _bind(tgp, k, t, s2), np.where(missing, np.nan, y), np.array([1e-18]), lp, pm, pv)


def test_a_short_warm_up_is_repaired_once_and_remembered_and_a_forced_one_is_reported(tgp):
    """the median gap sets the warm-up; a stretch of gaps a hundred times smaller behind a chunk edge forgets a hundred times slower per step: the
    hand-over check fails at the first guess and one doubling repairs it.  The construction is tests/_sweep_group_sde.py repair_gaps;
    tests/test_sweep_group_sde_host.py::test_the_repair_case restates the walk for exactly these gaps and this seed and asserts the forward distance
    above 1e-12 at the first guess W and below it at 2 W"""
    k, dt, s2 = SG.KERNELS[SS.REPAIR_D]
    gaps = SS.repair_gaps(dt, 0, 0, stretched=False)
    dm0 = _bind(tgp, k, np.cumsum(gaps), s2)
    model0, y0, _ = U.gp_case(k, np.cumsum(gaps), s2, seed=SS.REPAIR_SEED)
    tgp.logpdf(dm0, y0)
    g0 = dm0.handle().sweep_info()
    assert g0["served"] == 1 and g0["attempts"] == 1, g0
    C, W = g0["C"], g0["W"]
    t = np.cumsum(SS.repair_gaps(dt, C, W))
    model, y, _ = U.gp_case(k, t, s2, seed=SS.REPAIR_SEED)
    lp, pm, pv = _reference(model, y, None, 1e-18, fast=True)
    dm = _bind(tgp, k, t, s2)
    hd = dm.handle()
    got = tgp.logpdf(dm, y)
    info = hd.sweep_info()
    print(info)
    assert info["served"] == 1 and info["attempts"] == 2 and info["W"] == 2 * W, (info, g0)
    assert abs(got - lp) <= 1e-10 * abs(lp)
    got = tgp.logpdf(dm, y)
    info2 = hd.sweep_info()
    assert info2["served"] == 1 and info2["attempts"] == 1 and info2["W"] == info["W"], info2
    hd.set_option(tgp._lib.OPT_SWEEP_WARMUP, W)
    got = tgp.logpdf(dm, y)
    info3 = hd.sweep_info()
    assert info3["served"] == 0 and info3["status"] & 1 and info3["attempts"] == 1, info3
    assert abs(got - lp) <= 1e-10 * abs(lp)


def test_host_and_device_inputs_and_two_calls_in_a_row_give_the_same_bits(tgp):
    import torch
    k, dt, s2 = SG.KERNELS[7]
    T = 3001
    t = _times(T, dt, 12)
    model, y, _ = U.gp_case(k, t, s2, seed=41)
    missing = _mask(T, 42)
    dm = _bind(tgp, k, t, s2)
    hd = dm.handle()
    rn = np.array([1e-18])
    a = tgp.logpdf_and_posterior_marginals(dm, np.where(missing, np.nan, y), rn)
    assert hd.sweep_info()["served"] == 1
    b = tgp.logpdf_and_posterior_marginals(dm, np.where(missing, np.nan, y), rn)
    assert hd.sweep_info()["served"] == 1
    yd = torch.as_tensor(np.where(missing, 0.0, y), device="cuda:0")
    md = torch.as_tensor(missing, device="cuda:0")
    c = tgp.logpdf_and_posterior_marginals(dm, (yd, md), torch.full((1,), 1e-18, dtype=torch.float64, device="cuda:0"))
    assert hd.sweep_info()["served"] == 1
    assert a[0] == b[0] == c[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[1], c[1].cpu().numpy()) and np.array_equal(a[2], c[2].cpu().numpy())


@pytest.mark.parametrize("case", ["closed_form_off", "sweep_1", "sweep_0", "chunk"])
def test_declines_with_the_general_engines_answer(tgp, case):
    k, dt, s2 = SG.KERNELS[6]
    T = 2500
    t = _times(T, dt, 13)
    model, y, _ = U.gp_case(k, t, s2, seed=43)
    missing = _mask(T, 44)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    dm = _bind(tgp, k, t, s2, sweep={"sweep_1": 1, "sweep_0": 0}.get(case, 2))
    if case == "closed_form_off":
        dm.handle().set_option(tgp._lib.OPT_SDE_CLOSED_FORM, 0)
    if case == "chunk":
        dm.handle().set_option(tgp._lib.OPT_CHUNK, 64)
    _check(tgp, dm, np.where(missing, np.nan, y), np.array([1e-18]), lp, pm, pv, served=False)


def test_declines_a_model_the_filter_cannot_forget_within_4096_steps(tgp):
    """gaps some hundred times below the length scale and a noisy observation: the plan's estimate finds no warm-up (state -1, nothing launched, no
    second look)"""
    k, _, s2 = SG.KERNELS[5]
    T = 2500
    t = _times(T, 2e-3, 14)
    model, y, _ = U.gp_case(k, t, 10.0, seed=45)
    lp, pm, pv = _reference(model, y, None, 1e-18, fast=True)
    dm = _bind(tgp, k, t, 10.0)
    info = _check(tgp, dm, y, np.array([1e-18]), lp, pm, pv, served=False)
    assert info["attempts"] == 0 and info["state"] == -1, info


def test_gp_level_prediction_matches_the_default_route(tgp):
    from temporalgps_jl_amd import lti_sde as P
    k, dt, s2 = SG.KERNELS[5]
    T = 3000
    x = _times(T, dt, 15)
    _, y, _ = U.gp_case(k, x, s2, seed=46)
    f = P.to_sde(P.GP(P.to_kernel(k)))
    fx = f(x, s2)
    lp = P.logpdf(fx, y)
    m0, v0 = P.mean_and_var(P.posterior(fx, y)(x))
    dm = fx.build_lgssm()
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_SWEEP, 2)
    got = tgp.logpdf(dm, y)
    assert hd.sweep_info()["served"] == 1, hd.sweep_info()
    assert abs(got - lp) <= 1e-10 * abs(lp), (got, lp)
    _, m1, v1 = tgp.logpdf_and_posterior_marginals(dm, y, np.array([1e-18]))
    assert hd.sweep_info()["served"] == 1
    assert np.abs(m1 - m0).max() <= 1e-8 * max(1.0, np.abs(m0).max())
    assert np.abs(v1 - v0).max() <= 1e-8 * max(1.0, v0.max())
