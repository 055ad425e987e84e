"""GPU tier (-m gpu): the group sweep (tgp_sweep_group.hip) -- the sweep engine's algorithm at d = 5 .. 8 with a chunk spread over 8
lanes -- through the C ABI against the oracle, as tests/test_gpu_sweep.py checks the lane sweep.  Tolerances as everywhere: logpdf
1e-10 relative, posterior mean 1e-8 of max(1, |mean|), variance 1e-8 of max(1, var).  Every case asserts that the engine served the call
(tgp_sweep_info) and that the profile names its two kernels and no other."""
import numpy as np
import pytest

from tests import _sweep_group as SG
from tests import _util as U
from tests.test_gpu_sweep import _reference

pytestmark = pytest.mark.gpu

NAMES = {"k_sweep_group<lti,logpdf>", "k_sweep_group<lti,posterior>"}


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _check(tgp, dm, yin, Rn, lp, pm, pv):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    got = tgp.logpdf(dm, yin)
    info = hd.sweep_info()
    assert info["served"] == 1, info
    assert abs(got - lp) <= 1e-10 * abs(lp), (got, lp, info)
    got2, mean, var = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = hd.sweep_info()
    assert info["served"] == 1, info
    assert abs(got2 - lp) <= 1e-10 * abs(lp), (got2, lp, info)
    assert np.abs(mean - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max()), info
    assert np.abs(var - pv).max() <= 1e-8 * max(1.0, pv.max()), info
    mean2, var2 = tgp.posterior_marginals(dm, yin, Rn)
    assert hd.sweep_info()["served"] == 1 and np.array_equal(mean2, mean) and np.array_equal(var2, var)
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    assert names == NAMES, names
    return info


def _mask(T, seed, frac=0.1):
    missing = np.random.default_rng(seed).random(T) < frac
    missing[5:9] = True
    missing[T - 3:] = True
    missing[0] = True
    return missing


@pytest.mark.parametrize("T", [2048, 5003])
@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_missing_data_on_a_regular_grid(tgp, d, T):
    k, dt, s2 = SG.KERNELS[d]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=d)
    assert len(model["x0m"]) == d
    missing = _mask(T, 100 + d)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    info = _check(tgp, SG.device_model(tgp, model), np.where(missing, np.nan, y), np.array([1e-18]), lp, pm, pv)
    assert info["attempts"] == 1 and info["Wb"] <= info["C"] and info["C"] % 8 == 0, info


def test_noise_variance_per_step_d6(tgp):
    k, dt, _ = SG.KERNELS[6]
    T = 4500
    rng = np.random.default_rng(7)
    S = rng.uniform(0.05, 0.5, T)
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), S, seed=1)
    lp, pm, pv = _reference(model, y, None, 1e-18, fast=True)
    _check(tgp, SG.device_model(tgp, model), y, np.array([1e-18]), lp, pm, pv)


def test_emission_offset_per_step_d5(tgp):
    k, dt, s2 = SG.KERNELS[5]
    T = 4500
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=2, mean=("custom", lambda t: np.sin(t)))
    Rn = np.random.default_rng(8).random(T) * 0.05      # the replaced noise per step
    lp, pm, pv = _reference(model, y, None, Rn, fast=True)
    dm = SG.device_model(tgp, model)
    # (a fully observed series with one noise variance and a mean function is the stationary one-launch path's, in front of the sweep engines
    #  -- TGP_OPT_STEADY = 3; with that path off the offset stream alone reaches the group sweep)
    dm.handle().set_option(tgp._lib.OPT_STEADY, 2)
    _check(tgp, dm, y, Rn, lp, pm, pv)
    # ... and with the default routing a single missing step is enough
    missing = np.zeros(T, dtype=bool)
    missing[1234] = True
    lp, pm, pv = _reference(model, y, missing, Rn, fast=True)
    _check(tgp, SG.device_model(tgp, model), np.where(missing, np.nan, y), Rn, lp, pm, pv)


@pytest.mark.parametrize("d", [6, 7])
def test_noise_offset_and_mask_together(tgp, d):
    k, dt, _ = SG.KERNELS[d]
    T = 3001
    rng = np.random.default_rng(9 + d)
    S = rng.uniform(0.05, 0.5, T)
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), S, seed=3, mean=("custom", lambda t: np.sin(t)))
    missing = _mask(T, 11 + d, 0.2)
    yin = np.where(missing, np.nan, y)
    Rn = rng.random(T) * 0.05
    lp, pm, pv = _reference(model, y, missing, Rn, fast=True)
    _check(tgp, SG.device_model(tgp, model), yin, Rn, lp, pm, pv)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)      # ... and the shared replaced noise
    _check(tgp, SG.device_model(tgp, model), yin, np.array([1e-18]), lp, pm, pv)


def test_device_resident_inputs_and_outputs_d6(tgp):
    import torch
    k, dt, s2 = SG.KERNELS[6]
    T = 5003
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=4)
    missing = _mask(T, 17)
    lp, pm, pv = _reference(model, y, missing, 1e-18, fast=True)
    dm = SG.device_model(tgp, model)
    yd = torch.as_tensor(np.where(missing, 0.0, y), device="cuda:0")
    md = torch.as_tensor(missing, device="cuda:0")
    rn = torch.full((1,), 1e-18, dtype=torch.float64, device="cuda:0")
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    got1 = tgp.logpdf(dm, (yd, md))
    assert hd.sweep_info()["served"] == 1 and abs(got1 - lp) <= 1e-10 * abs(lp)
    got, mean, var = tgp.logpdf_and_posterior_marginals(dm, (yd, md), rn)
    info = hd.sweep_info()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    assert info["served"] == 1 and info["attempts"] == 1, info
    assert names == NAMES, names
    assert mean.is_cuda and var.is_cuda
    assert abs(got - lp) <= 1e-10 * abs(lp)
    assert float((mean.cpu() - torch.as_tensor(pm)).abs().max()) <= 1e-8 * max(1.0, np.abs(pm).max())
    assert float((var.cpu() - torch.as_tensor(pv)).abs().max()) <= 1e-8 * max(1.0, pv.max())
