"""GPU tier: the streaming kernels on their input-normalised modal form (csrc/tgp_stream_form.hpp) -- csrc/tgp_lml.hip and
csrc/tgp_post.hip run x' = M x + e u~ with the input entering every block with coefficient 1 and no constant; the head's end state, the backward state
handed back to the head and the host's closure of the records are mapped at the kernels' boundary.  Against the oracle's sequential filter / smoother
(oracle/seq_kalman.c) through the C ABI, TGP_OPT_STREAM_MIN_T = 0 on the handle so that the streaming kernels serve these short series; logpdf, mean and
var to rtol = atol = 1e-10.

Lengths: head + two tiles + 37 steps (a run seam, a last tile that straddles the series' end) and head + exactly three tiles (whole tiles
only: k_lml_stream's full-tile branch from the first tile to the last) -- tiles of 1024 steps for the posterior kernel, 1024 (d = 1) and 2048 (d >= 2) for the logpdf kernel,
as its choose_geometry picks them.  Structures at d = 3: a closed loop of three real modes (a slot of two real modes and an unpaired one) and one with
a conjugate pair, asserted on the plan.  A model whose last mode the observation barely excites cannot be normalised by its input: it is served by
k_steady_one, in the plan's coordinates."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from oracle import components as oc
from oracle import seq_kalman as sk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-10, atol=1e-10)
RN = np.array([0.3])

KERNELS = {
    1: ("matern12",),
    2: ("matern32",),
    3: ("matern52",),
    4: ("sum", ("matern52",), ("matern12",)),
    5: ("sum", ("matern52",), ("matern32",)),
    6: ("sum", ("matern52",), ("stretched", 0.4, ("matern52",))),
    7: ("sum", ("matern52",), ("stretched", 0.5, ("matern32",)), ("scaled", 0.3, ("matern32",))),
    8: ("sum", ("matern52",), ("stretched", 2.0, ("matern52",)), ("stretched", 0.5, ("matern32",))),
}
# d = 3, (spacing, noise variance): the stationary closed loop of a Matern-5/2 model has three real modes at the first, a conjugate pair at the second
ALL_REAL, ONE_PAIR = (1.0, 1e-3), (0.1, 0.1)
# the last mode enters the observation with 1e-18 of the variance of the others: its input coefficient is ~1e-11 of theirs
WEAK = ("sum", ("matern32",), ("scaled", 1e-18, ("matern12",)))


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


@functools.lru_cache(maxsize=None)
def proto():
    spec = importlib.util.spec_from_file_location("modal_proto", os.path.join(ROOT, "scripts", "modal_proto.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def head_of(kern, dt, s2):
    pl = proto().plan(oc.build_lgssm(kern, ("regular", 0.0, dt, 20000), s2), 20000)      # (the head does not depend on the length)
    assert pl["why"] == 0, pl
    return pl


@functools.lru_cache(maxsize=None)
def case(kern, dt, s2, T, offsets=False):
    """model, series and the oracle's answers: computed once, shared, never written to"""
    model = oc.build_lgssm(kern, ("regular", 0.0, dt, T), s2)
    d = len(model["x0m"])
    if offsets:
        rng = np.random.default_rng(5)
        model["a"] = np.broadcast_to(0.1 * rng.standard_normal(d), np.asarray(model["a"]).shape).copy()
        model["h"] = np.broadcast_to(np.array(0.7), np.asarray(model["h"]).shape).copy()
    rng = np.random.default_rng(T + d)
    y = sk.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    if offsets:
        y = y + 2.5      # (a mean the model does not know about: the innovations carry it)
    lp = sk.logpdf(model, y)
    mean, var = sk.posterior_marginals(model, y, RN)
    for a in (y, mean, var):
        a.setflags(write=False)
    return model, y, lp, mean, var


def device_model(tgp, model):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    dm.handle_options[tgp._lib.OPT_STREAM_MIN_T] = 0
    return dm


def kernels_of(tgp, dm, fn):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    out = fn()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out, names


def lengths(nhs, tile):
    return (nhs + 2 * tile + 37, nhs + 3 * tile)


def check_logpdf(tgp, kern, dt, s2, T, offsets=False):
    model, y, lp_ref, _, _ = case(kern, dt, s2, T, offsets)
    dm = device_model(tgp, model)
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, y))
    print(f"logpdf T {T}: {names} rel {abs(lp - lp_ref) / abs(lp_ref):.2e}")
    assert len(names) == 1 and next(iter(names)).startswith("k_lml_stream"), names
    np.testing.assert_allclose(lp, lp_ref, **TOL)
    return dm, lp


def check_posterior(tgp, kern, dt, s2, T, offsets=False):
    model, y, lp_ref, m_ref, v_ref = case(kern, dt, s2, T, offsets)
    dm = device_model(tgp, model)
    (lp, mean, var), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, y, RN))
    print(f"posterior T {T}: {names} logpdf rel {abs(lp - lp_ref) / abs(lp_ref):.2e} mean {np.max(np.abs(mean - m_ref)):.2e} var {np.max(np.abs(var - v_ref)):.2e}")
    assert names == {"k_post_stream"}, names
    np.testing.assert_allclose(lp, lp_ref, **TOL)
    np.testing.assert_allclose(mean, m_ref, **TOL)
    np.testing.assert_allclose(var, v_ref, **TOL)
    return dm, (lp, mean, var)


@pytest.mark.parametrize("d", sorted(KERNELS))
def test_logpdf_at_every_state_dimension(tgp, d):
    nhs = head_of(KERNELS[d], 0.1, 0.1)["nhs"]
    for T in lengths(nhs, 1024 if d == 1 else 2048):
        check_logpdf(tgp, KERNELS[d], 0.1, 0.1, T)


@pytest.mark.parametrize("d", (1, 2, 3))
def test_posterior_at_every_state_dimension_it_serves(tgp, d):
    nhs = head_of(KERNELS[d], 0.1, 0.1)["nhs"]
    for T in lengths(nhs, 1024):
        check_posterior(tgp, KERNELS[d], 0.1, 0.1, T)


@pytest.mark.parametrize("dt,s2,npair", [ALL_REAL + (0,), ONE_PAIR + (1,)])
def test_all_real_and_one_pair_closed_loops_at_d3(tgp, dt, s2, npair):
    pl = head_of(KERNELS[3], dt, s2)
    assert pl["npair"] == npair, pl["npair"]
    for T in lengths(pl["nhs"], 2048):
        check_logpdf(tgp, KERNELS[3], dt, s2, T)
    for T in lengths(pl["nhs"], 1024):
        check_posterior(tgp, KERNELS[3], dt, s2, T)


def test_transition_and_emission_offsets_and_a_series_off_zero(tgp):
    """the state shift and the folded emission offset: a != 0, h != 0, observations around 2.5"""
    for dt, s2 in (ALL_REAL, ONE_PAIR):
        nhs = head_of(KERNELS[3], dt, s2)["nhs"]
        check_logpdf(tgp, KERNELS[3], dt, s2, lengths(nhs, 2048)[0], offsets=True)
        for T in lengths(nhs, 1024):
            check_posterior(tgp, KERNELS[3], dt, s2, T, offsets=True)


def test_a_repeated_call_is_bit_identical(tgp):
    dt, s2 = ONE_PAIR
    nhs = head_of(KERNELS[3], dt, s2)["nhs"]
    T = lengths(nhs, 2048)[0]
    model, y, _, _, _ = case(KERNELS[3], dt, s2, T)
    dm, lp = check_logpdf(tgp, KERNELS[3], dt, s2, T)
    assert tgp.logpdf(dm, y) == lp
    T = lengths(nhs, 1024)[0]
    model, y, _, _, _ = case(KERNELS[3], dt, s2, T)
    dm, (lp, mean, var) = check_posterior(tgp, KERNELS[3], dt, s2, T)
    lp2, mean2, var2 = tgp.logpdf_and_posterior_marginals(dm, y, RN)
    assert lp2 == lp and np.array_equal(mean2, mean) and np.array_equal(var2, var)


def test_a_mode_the_observation_barely_excites_is_served_by_k_steady_one(tgp):
    pl = head_of(WEAK, 0.1, 0.1)
    fb = np.abs(pl["fb"])
    assert fb.min() < 1e-8 * fb.max(), fb      # (what the guard of the normal form looks at)
    T = lengths(pl["nhs"], 1024)[0]
    model, y, lp_ref, m_ref, v_ref = case(WEAK, 0.1, 0.1, T)
    dm = device_model(tgp, model)
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, y))
    assert len(names) == 1 and next(iter(names)).startswith("k_steady_one"), names
    np.testing.assert_allclose(lp, lp_ref, **TOL)
    (lp, mean, var), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, y, RN))
    assert len(names) == 1 and next(iter(names)).startswith("k_steady_one"), names
    np.testing.assert_allclose(lp, lp_ref, **TOL)
    np.testing.assert_allclose(mean, m_ref, **TOL)
    np.testing.assert_allclose(var, v_ref, **TOL)
