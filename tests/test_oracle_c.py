"""The C restatement (oracle/seq_kalman.c) must agree with the NumPy restatement (oracle/lgssm_ref.py)."""
import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref
from oracle import seq_kalman as sk

from ._util import BOUNDARY_KERNELS

CASES = [
    (("matern12",), ("regular", 0.0, 0.1, 200), 0.1),
    (("matern32",), ("regular", 0.0, 0.1, 200), 0.1),
    (("matern52",), ("regular", 0.0, 0.1, 200), 0.1),
    (("sum", ("matern52",), ("matern32",)), ("regular", 0.0, 0.1, 150), 0.1),
    (("sum", ("matern52",), ("matern52",)), ("regular", 0.0, 0.1, 100), 0.2),
    (("scaled", 1.5, ("stretched", 0.7, ("matern52",))), None, None),   # irregular + hetero
    (("sum", ("matern52",), ("matern12",)), None, None),
]


def _case(i):
    rng = np.random.default_rng(100 + i)
    k, t, s2 = CASES[i]
    if t is None:
        t = np.cumsum(rng.random(120) * 0.1 + 0.05)
        s2 = rng.random(120) * 0.2 + 0.05
    model = oc.build_lgssm(k, t, s2)
    T, d = model["T"], len(model["x0m"])
    eps = rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d)
    y = ref.rand(model, *eps)
    return model, y, eps


@pytest.mark.parametrize("i", range(len(CASES)))
def test_c_matches_numpy(i):
    model, y, eps = _case(i)
    np.testing.assert_allclose(sk.rand(model, *eps), y, rtol=1e-12, atol=1e-12)
    lp = ref.logpdf(model, y)
    lml, ms, Ps = sk.filter_(model, y, want_states=True)
    assert abs(lml - lp) <= 1e-12 * abs(lp)
    rm, rP = ref.filter_(model, y)
    np.testing.assert_allclose(ms, rm, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(Ps, rP, rtol=1e-11, atol=1e-13)
    post_c, post = sk.posterior(model, y), ref.posterior(model, y)
    for key in ("A", "a", "Q", "x0m", "x0P"):
        np.testing.assert_allclose(post_c[key], post[key], rtol=1e-9, atol=1e-11)
    Rn = np.full(model["T"], 1e-18)
    mean, var = sk.posterior_marginals(model, y, Rn)
    rmean, rvar = ref.marginals(ref.replace_observation_noise_cov(post, Rn))
    np.testing.assert_allclose(mean, rmean, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(var, rvar, rtol=1e-9, atol=1e-12)
    pm, pv = sk.prior_marginals(model)
    qm, qv = ref.marginals(model)
    np.testing.assert_allclose(pm, qm, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(pv, qv, rtol=1e-12)


WIDE = {9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))), 17: BOUNDARY_KERNELS[17], 33: BOUNDARY_KERNELS[33], 63: BOUNDARY_KERNELS[63]}


@pytest.mark.parametrize("d", sorted(WIDE))
def test_c_with_a_run_time_state_dimension_matches_numpy(d):
    """The run-time path of oracle/seq_kalman.c (8 < d <= 64) against the NumPy restatement: the same recursion in the same precision, so logpdf at
    1e-12 relative and the filtered states at 1e-10 (scaled by the largest entry, at least one) -- two decades inside what the GPU tier asks of the
    engine.  Measured here at T = 1500 (spacing 0.1, noise 0.1): logpdf 0 ... 3e-16, filtered means and covariances <= 1e-15 at every d, d = 63 included
    (logpdf 0.0, means 9.8e-16, covariances 3.0e-16): the restatement's own rounding at d = 63 leaves these bounds three decades of room, they stand as
    set.  d = 63 at this length also crosses a block boundary of posterior_marginals (1048 steps of reverse dynamics at a time)."""
    T = 1500
    model = oc.build_lgssm(WIDE[d], ("regular", 0.0, 0.1, T), 0.1)
    assert len(model["x0m"]) == d
    rng = np.random.default_rng(d)
    eps = rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d)
    y = ref.rand(model, *eps)
    np.testing.assert_allclose(sk.rand(model, *eps), y, rtol=0, atol=1e-12 * np.abs(y).max())
    lp = ref.logpdf(model, y)
    assert abs(sk.logpdf(model, y) - lp) <= 1e-12 * abs(lp)
    lml, ms, Ps = sk.filter_(model, y, want_states=True)
    assert abs(lml - lp) <= 1e-12 * abs(lp), (lml, lp)
    rm, rP = ref.filter_(model, y)
    assert np.max(np.abs(ms - rm)) <= 1e-10 * max(1.0, np.abs(rm).max()), np.max(np.abs(ms - rm))
    assert np.max(np.abs(Ps - rP)) <= 1e-10 * max(1.0, np.abs(rP).max()), np.max(np.abs(Ps - rP))
    # the RTS chain: both sides solve against the same predicted covariances (condition up to 3e9), rounding alone apart
    post_c, post = sk.posterior(model, y), ref.posterior(model, y)
    for key in ("A", "a", "Q", "x0m", "x0P"):
        np.testing.assert_allclose(post_c[key], post[key], rtol=1e-9, atol=1e-9 * max(1.0, np.abs(post[key]).max()))
    for Rn in (np.array([0.05]), rng.random(T) * 0.3 + 0.01):
        mean, var = sk.posterior_marginals(model, y, Rn)
        rmean, rvar = ref.marginals(ref.replace_observation_noise_cov(post, Rn if Rn.size > 1 else np.full(T, Rn[0])))
        rmean, rvar = np.asarray(rmean).reshape(T), np.asarray(rvar).reshape(T)
        assert np.max(np.abs(mean - rmean)) <= 1e-10 * max(1.0, np.abs(rmean).max()), np.max(np.abs(mean - rmean))
        assert np.max(np.abs(var - rvar)) <= 1e-10 * max(1.0, rvar.max()), np.max(np.abs(var - rvar))
    pm, pv = sk.prior_marginals(model)
    qm, qv = ref.marginals(model)
    np.testing.assert_allclose(pm, np.asarray(qm).reshape(T), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(pv, np.asarray(qv).reshape(T), rtol=1e-12)


def test_openmp_host_build_of_the_chunk_functions_compiles():
    """bench.py's all-core CPU leg (oracle/omp_scan.py) compiles tests/hostsim/hostsim.cpp with -fopenmp; a pragma in front of
    a non-loop statement only shows up in that build (the GPU box rebuilds it: file times differ there)."""
    import shutil
    import pytest
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from oracle import omp_scan
    so = omp_scan.build(force=True)
    import os
    assert os.path.exists(so)
