"""GPU tier (-m gpu): the tile sweep (tgp_sweep_tile.hip) through the C ABI under TGP_OPT_SWEEP = 2 against the oracle, as
tests/test_gpu_sweep_group.py checks the group sweep: logpdf 1e-10 relative, mean and variance 1e-8 of max(1, .).  Every served case asserts tgp_sweep_info's
"served" and that the profile names the engine's two kernels and no other; tests/test_sweep_tile_host.py holds the algorithm and the hand-overs on the CPU."""
import numpy as np
import pytest

from tests import _sweep_group as SG
from tests import _sweep_tile as ST
from tests import _util as U

pytestmark = pytest.mark.gpu

NAMES = {"k_sweep_tile<logpdf>", "k_sweep_tile<posterior>"}


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _calls(tgp, dm, yin, Rn, ref):      # logpdf, the combined call and the marginals alone with the profile on; values at the project's bars
    lp, pm, pv = ref
    (got, i1, (got2, mean, var), i2, (mean2, var2)), names = U.kernels_of(tgp, dm, lambda: (
        tgp.logpdf(dm, yin), dm.handle().sweep_info(), tgp.logpdf_and_posterior_marginals(dm, yin, Rn), dm.handle().sweep_info(), tgp.posterior_marginals(dm, yin, Rn)))
    print(i1, i2, sorted(names))
    assert abs(got - lp) <= 1e-10 * abs(lp) and abs(got2 - lp) <= 1e-10 * abs(lp), (got, got2, lp)
    assert np.abs(mean - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max()), i2
    assert np.abs(var - pv).max() <= 1e-8 * max(1.0, pv.max()), i2
    assert np.array_equal(mean2, mean) and np.array_equal(var2, var)      # two calls on one handle: the same bits
    return i1, i2, names


def _served(tgp, c, **options):
    model, y, missing, Rn, ref = c
    dm = SG.device_model(tgp, model)
    for name, v in options.items():
        dm.handle().set_option(getattr(tgp._lib, name), v)
    i1, i2, names = _calls(tgp, dm, y if missing is None else np.where(missing, np.nan, y), Rn, ref)
    assert i1["served"] == 1 and i2["served"] == 1 and i2["status"] == 0 and names == NAMES, (i1, i2, names)
    return i1, i2


@pytest.mark.parametrize("d,T", [(9, 2053), (12, 2048), (13, 2053), (16, 2048)])
def test_missing_data_on_a_regular_grid(tgp, d, T):
    """the most padding, a full accumulator row group, one row into the last group, no padding; T = 2053: the last chunk is shorter than the others"""
    _served(tgp, ST.case(d, T))


def test_forced_chunks_of_64_steps_d9(tgp):
    """33 chunks: every seam and both hand-overs 32 times, at the first attempt (host tier: 3.2e-16 / 2.2e-15 against 1e-12 / 1e-11)"""
    for info in _served(tgp, ST.case(9, 2053), OPT_SWEEP_CHUNK=64, OPT_SWEEP_WARMUP=128, OPT_SWEEP_WARMUP_BACK=64):
        assert info["attempts"] == 1 and info["C"] == 64 and info["W"] == 128 and info["Wb"] == 64 and info["waves"] == 33, info


@pytest.mark.parametrize("xs,masked", [(0, True), (1, False), (2, True), (3, True)])
def test_the_four_input_stream_variants_d13(tgp, xs, masked):
    """mask only; a noise variance per step (fully observed); an emission offset per step; both -- each with a replaced noise per step"""
    _served(tgp, ST.case(13, 2053, xs, masked, True))


def test_device_resident_inputs_and_outputs_d12(tgp):
    import torch
    model, y, missing, Rn, (lp, pm, pv) = ST.case(12, 2048)
    dm = SG.device_model(tgp, model)
    yin = (torch.as_tensor(np.where(missing, 0.0, y), device="cuda:0"), torch.as_tensor(missing, device="cuda:0"))
    (got, mean, var), names = U.kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, yin, torch.as_tensor(Rn, device="cuda:0")))
    assert dm.handle().sweep_info()["served"] == 1 and names == {"k_sweep_tile<posterior>"} and mean.is_cuda and var.is_cuda, names
    assert abs(got - lp) <= 1e-10 * abs(lp)
    assert np.abs(mean.cpu().numpy() - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max()) and np.abs(var.cpu().numpy() - pv).max() <= 1e-8 * max(1.0, pv.max())


def test_a_forced_warm_up_that_is_too_short_is_reported_not_repaired(tgp):
    model, y, missing, Rn, ref = ST.case(9, 2053)
    dm = SG.device_model(tgp, model)
    for name, v in (("OPT_SWEEP_CHUNK", 64), ("OPT_SWEEP_WARMUP", 16)):
        dm.handle().set_option(getattr(tgp._lib, name), v)
    i1, i2, names = _calls(tgp, dm, np.where(missing, np.nan, y), Rn, ref)      # (the values are the general engine's)
    for info in (i1, i2):
        assert info["served"] == 0 and info["status"] & 1 and info["attempts"] == 1 and info["W"] == 16, info
    assert NAMES < names, names


def test_sparse_observations_are_repaired_and_remembered(tgp):
    """one step in eight observed (d = 9, T = 4096): slower forgetting than the plan's estimate -- 1e-9 / 9e-9 at the first geometry, 1e-16 with both warm-ups doubled"""
    model, y, _, Rn, _ = ST.case(9, 4096, 0, False)
    missing = np.ones(4096, dtype=bool)
    missing[::8] = False
    i1, i2 = _served(tgp, (model, y, missing, Rn, ST._reference(model, y, missing, Rn, fast=True)))
    assert i1["attempts"] >= 2 and i2["attempts"] >= 1 and i2["state"] == 1, (i1, i2)


@pytest.mark.parametrize("what", ["d8", "d17", "T2047", "reverse", "A_per_step", "default_option"])
def test_declines_leave_the_former_kernels(tgp, what):
    d, T = {"d8": 8, "d17": 17}.get(what, 9), 2047 if what == "T2047" else 2048
    model, y, missing, Rn, ref = ST.case(d, T)
    yin = np.where(missing, np.nan, y)
    if what == "A_per_step":
        model = dict(model, A=np.repeat(model["A"], T, axis=0))
    if what == "reverse":
        rng = np.random.default_rng(3)
        tr = U.random_lgssm(rng, False, 9, T, ordering="R")
        dm = tgp.LGSSM(tgp.GaussMarkovModel(tgp.Reverse, tr["A"], tr["a"], tr["Q"], tgp.Gaussian(tr["x0m"], tr["x0P"])), tgp.ScalarOutputLGC(tr["H"], tr["h"], tr["R"]), T=T)
        dm.handle().set_option(tgp._lib.OPT_SWEEP, 2)
        _, names = U.kernels_of(tgp, dm, lambda: tgp.logpdf(dm, yin))
    else:
        dm = SG.device_model(tgp, model, sweep=None if what == "default_option" else 2)
        i1, i2, names = _calls(tgp, dm, yin, Rn, ref)
        assert i2["served"] == (1 if what == "d8" else 0), i2
    info = dm.handle().sweep_info()
    assert not (names & NAMES) and (what == "d8" or info["attempts"] == 0), (names, info)
    if what == "d8":
        assert names == {"k_sweep_group<lti,logpdf>", "k_sweep_group<lti,posterior>"}, names
    if what == "d17":
        assert any(n.startswith("dk_") for n in names), names


def test_gp_level_logpdf_with_nans(tgp):
    """a GP on a RegularSpacing with NaNs in y (Matern52 * stretched Matern52, d = 9): the bound model under TGP_OPT_SWEEP = 2"""
    from temporalgps_jl_amd import lti_sde as P
    model, y, missing, _, (lp, _, _) = ST.case(9, 2053)
    fx = P.to_sde(P.GP(P.to_kernel(ST.KERNELS[9])))(P.RegularSpacing(0.0, ST.DT, 2053), 0.1)
    dm = fx.build_lgssm()
    dm.handle().set_option(tgp._lib.OPT_SWEEP, 2)
    got, names = U.kernels_of(tgp, dm, lambda: P.logpdf(fx, np.where(missing, np.nan, y)))
    assert dm.handle().sweep_info()["served"] == 1 and names == {"k_sweep_tile<logpdf>"}, names
    assert abs(got - lp) <= 1e-10 * abs(lp)
