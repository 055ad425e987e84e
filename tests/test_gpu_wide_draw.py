"""GPU tier: a draw from the posterior on the wide-state engine (8 < d <= 63; csrc/tgp_wide.hip k_wide_post_rand) --
rand(rng, replace_observation_noise_cov(posterior(model, y), Rnew)) (posterior_lti_sde.jl:48-58; lgssm.jl:65-91 on the Reverse model of :193-238) of a
Forward LTI model with scalar observations WITHOUT evaluating that model: the forward kernel keeping its innovations, the reverse-time draw behind the head
on the settled transition, the head on the host.  The algorithm itself (no kernel): tests/test_wide_draw_proto.py; the host plan: tests/test_wide_draw_plan.py.

Tolerances.
  * Same draws against the literal restatement (ref.posterior + ref.rand), relative to the path's largest value: 1e-6 at d = 28, 42 -- the project's bar
    against the literal RTS chain at these d (tests/test_gpu_wide.py::test_wide_posterior_marginals): the restatement solves in double precision against a
    predicted covariance of condition 3e8 ... 3e9 -- and 1e-9 at d = 9, 12, the bar of tgp_rand: the NumPy prototype of the algorithm stands 6.2e-13
    (d = 9) and 6.8e-15 (d = 12) from the restatement on the case below (CPU, T = 3000), so the restatement supports it with more than a decade to spare.
  * All draws zero against the dense GP's posterior mean on the model's own covariance function: ten times the distance at which the ORACLE's zero-draw
    restatement stands from that dense GP on the same case (CPU, absolute): 1.61e-9 (d = 9), 7.89e-9 (d = 12), 3.97e-8 (d = 28), 5.95e-8 (d = 42).
  * Device arrays against host arrays: 1e-12 (the same kernels on the same numbers; the head's arithmetic is the host's in both)."""
import ctypes

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref

pytestmark = pytest.mark.gpu

KERNELS = {
    9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))),
    12: ("product", ("matern32",), ("approx_periodic", 3, 1.0)),
    28: ("product", ("approx_periodic", 7, 1.0), ("matern32",)),
    42: ("product", ("approx_periodic", 7, 1.0), ("matern52",)),
}
REL_RESTATEMENT = {9: 1e-9, 12: 1e-9, 28: 1e-6, 42: 1e-6}
ORACLE_ZERO_DRAW_FROM_DENSE_GP = {9: 1.61e-9, 12: 7.89e-9, 28: 3.97e-8, 42: 5.95e-8}      # (absolute; measured on the CPU on case() below)
EUNSUPPORTED = 4
T_CASE = 3000


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def device_model(tgp, model, wide=1):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    dm.handle_options[tgp._lib.OPT_WIDE] = wide
    return dm


def kernels_of(tgp, dm, fn):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    out = fn()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out, names


_cases = {}


def case(d):
    """spacing 0.1, noise 0.1, T = 3000: a series drawn from the model, then the draws of the posterior sample -- one generator, seed d"""
    if d not in _cases:
        T = T_CASE
        model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)
        assert len(model["x0m"]) == d
        rng = np.random.default_rng(d)
        y = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
        eps = (rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
        _cases[d] = (model, y, eps)
    return _cases[d]


def draw_c(tgp, dm, y, Rn, eps):
    """tgp_posterior_rand through ctypes on host arrays: (return code, path)"""
    hd = dm.handle()
    L = tgp._lib
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))      # noqa: E731
    yy, Rr, et, ee, e0 = c(y), c(Rn), c(eps[0]), c(eps[1]), c(eps[2])
    out = np.zeros(len(yy))
    flags = L.SHARED_R if Rr.shape[0] == 1 else 0
    rc = hd.lib.tgp_posterior_rand(hd.h, L.ptr(yy), L.ptr(Rr), L.ptr(et), L.ptr(ee), L.ptr(e0), flags, L.ptr(out))
    return rc, out


def dense_gp_mean(model, y):
    """The posterior mean from the model's OWN covariance function, k(s - t) = h' A^|s - t| P_inf h, by a dense Cholesky: no state-space recursion involved"""
    from scipy.linalg import cho_factor, cho_solve, toeplitz
    T = model["T"]
    A, H, P, R = model["A"][0], model["H"][0], model["x0P"], float(model["R"][0])
    c, v = np.empty(T), P @ H
    for k in range(T):
        c[k] = H @ v
        v = A @ v
    K = toeplitz(c)
    return K @ cho_solve(cho_factor(K + R * np.eye(T), lower=True), y)


@pytest.mark.parametrize("d", sorted(KERNELS))
def test_the_draw_is_served_by_the_wide_engine_and_equals_the_restatement(tgp, d):
    """items 1-3: TGP_OK and k_wide_post_rand in the profile (TGP_EUNSUPPORTED with TGP_OPT_WIDE = 0, as before the engine had the draw); the same draws
    against ref.posterior + ref.rand; all draws zero against the dense GP's posterior mean"""
    model, y, eps = case(d)
    T = T_CASE
    Rn = np.array([1e-6])
    dm = device_model(tgp, model)
    (rc, got), names = kernels_of(tgp, dm, lambda: draw_c(tgp, dm, y, Rn, eps))
    assert rc == 0, (rc, dm.handle().last_error() if hasattr(dm.handle(), "last_error") else None)
    assert len(names) == 1 and "k_wide_post_rand" in next(iter(names)), names
    dm0 = device_model(tgp, model, wide=0)
    rc0, _ = draw_c(tgp, dm0, y, Rn, eps)
    assert rc0 == EUNSUPPORTED, rc0
    post = ref.replace_observation_noise_cov(ref.posterior(model, y), Rn)
    want = ref.rand(post, *eps)
    err = np.max(np.abs(got - want)) / np.abs(want).max()
    print(f"d {d}: draw vs restatement {err:.3e} (bound {REL_RESTATEMENT[d]:.0e})")
    assert err <= REL_RESTATEMENT[d], (d, err)
    # a second call keeps the plans: the same numbers
    rc2, again = draw_c(tgp, dm, y, Rn, eps)
    assert rc2 == 0
    np.testing.assert_array_equal(got, again)
    # all draws zero: h . (smoothed mean) + hh
    zero = (np.zeros((T, d)), np.zeros(T), np.zeros(d))
    rcz, path0 = draw_c(tgp, dm, y, Rn, zero)
    assert rcz == 0
    m_gp = dense_gp_mean(model, y)
    ez = np.max(np.abs(path0 - m_gp))
    print(f"d {d}: zero draw vs dense GP {ez:.3e} (oracle's own: {ORACLE_ZERO_DRAW_FROM_DENSE_GP[d]:.2e})")
    assert ez <= 10.0 * ORACLE_ZERO_DRAW_FROM_DENSE_GP[d], (d, ez)


@pytest.mark.parametrize("d", (9, 12))
def test_the_draw_equals_the_evaluated_route(tgp, d):
    """item 4: tgp_posterior, the Reverse model bound, tgp_rand (what serves the call with TGP_OPT_WIDE = 0) on the same draws"""
    model, y, eps = case(d)
    for Rn in (np.array([0.05]), None):
        dm = device_model(tgp, model)
        post = tgp.posterior(dm, y)
        if Rn is not None:
            post = tgp.replace_observation_noise_cov(post, Rn)
        got, names = kernels_of(tgp, dm, lambda: tgp.rand(eps, post))
        assert len(names) == 1 and "k_wide_post_rand" in next(iter(names)), names
        dm2 = device_model(tgp, model, wide=0)
        post2 = tgp.posterior(dm2, y)
        if Rn is not None:
            post2 = tgp.replace_observation_noise_cov(post2, Rn)
        post2.materialise()
        want = tgp.rand(eps, post2)
        err = np.max(np.abs(got - want)) / np.abs(want).max()
        print(f"d {d}: draw vs evaluated route {err:.3e}")
        assert err <= REL_RESTATEMENT[d], (d, err)


def test_per_step_noise_and_a_mean_function_at_the_inputs(tgp):
    """item 5's two cases: Rnew per step; an emission offset per step (it enters y*_t and the forward kernel only)"""
    d = 28
    model, y, eps = case(d)
    T = T_CASE
    rng = np.random.default_rng(77)
    Rn = rng.random(T) * 0.3 + 0.01
    dm = device_model(tgp, model)
    (rc, got), names = kernels_of(tgp, dm, lambda: draw_c(tgp, dm, y, Rn, eps))
    assert rc == 0 and "k_wide_post_rand" in next(iter(names)), (rc, names)
    want = ref.rand(ref.replace_observation_noise_cov(ref.posterior(model, y), Rn), *eps)
    assert np.max(np.abs(got - want)) <= REL_RESTATEMENT[d] * np.abs(want).max(), np.max(np.abs(got - want))
    ht = 0.8 * np.sin(0.013 * np.arange(T)) + 0.0004 * np.arange(T) - 0.5
    model_h = dict(model, h=ht)
    dmh = device_model(tgp, model_h)
    Rs = np.array([0.02])
    (rc, got), names = kernels_of(tgp, dmh, lambda: draw_c(tgp, dmh, y + ht, Rs, eps))
    assert rc == 0 and "k_wide_post_rand" in next(iter(names)), (rc, names)
    want = ref.rand(ref.replace_observation_noise_cov(ref.posterior(model_h, y + ht), Rs), *eps)
    assert np.max(np.abs(got - want)) <= REL_RESTATEMENT[d] * np.abs(want).max(), np.max(np.abs(got - want))


def test_device_resident_series_and_draws(tgp):
    """item 5: T = 1e6 at d = 28 on device arrays runs and names the kernel; at T = 60000 the device-array call equals the host-array call to 1e-12"""
    import torch
    d = 28
    for T in (60_000, 1_000_000):
        model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)
        rng = np.random.default_rng(5)
        # (white noise of the prior's marginal variance is as good a series for parity as a draw of the model, without the restatement's Python loop)
        y = rng.standard_normal(T) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + 0.1)
        gen = torch.Generator(device="cuda").manual_seed(T)
        et = torch.randn((T, d), dtype=torch.float64, device="cuda", generator=gen)
        ee = torch.randn((T,), dtype=torch.float64, device="cuda", generator=gen)
        e0 = rng.standard_normal(d)
        yd = torch.from_numpy(y).cuda()
        dm = device_model(tgp, model)
        post = tgp.replace_observation_noise_cov(tgp.posterior(dm, yd), np.array([0.05]))
        got, names = kernels_of(tgp, dm, lambda: tgp.rand((et, ee, e0), post))
        assert len(names) == 1 and "k_wide_post_rand" in next(iter(names)), names
        assert got.is_cuda and got.shape == (T,) and bool(torch.isfinite(got).all())
        if T == 60_000:
            dm2 = device_model(tgp, model)
            post2 = tgp.replace_observation_noise_cov(tgp.posterior(dm2, y), np.array([0.05]))
            got2, names2 = kernels_of(tgp, dm2, lambda: tgp.rand((et.cpu().numpy(), ee.cpu().numpy(), e0), post2))
            assert "k_wide_post_rand" in next(iter(names2)), names2
            assert np.max(np.abs(got.cpu().numpy() - got2)) <= 1e-12 * max(1.0, np.abs(got2).max())


def test_gp_level_draw_on_a_product_kernel(tgp, monkeypatch):
    """item 6: the reference's own call chain (posterior_lti_sde.jl:48-58) -- rand(rng, posterior(fx, y)(x, 1e-6)) on ApproxPeriodicKernel() * Matern32Kernel()
    binds ONE model, and its profile shows the draw kernel"""
    from temporalgps_jl_amd import lti_sde as P
    rng = np.random.default_rng(2)
    T = 1800
    x = P.RegularSpacing(0.0, 0.1, T)
    f = P.to_sde(P.GP(P.ApproxPeriodicKernel() * P.Matern32Kernel()), P.HIPStorage())
    fx = f(x, 0.1)
    y = np.asarray(P.rand(rng, fx))
    built, real = [], P.build_lgssm

    def profiled(*a, **k):      # (every model the API binds from here on records its kernels)
        mdl = real(*a, **k)
        mdl.handle_options[tgp._lib.OPT_PROFILE] = 1
        built.append(mdl)
        return mdl
    monkeypatch.setattr(P, "build_lgssm", profiled)
    path = np.asarray(P.rand(np.random.default_rng(3), P.posterior(fx, y)(fx.x, 1e-6)))
    assert path.shape == (T,) and np.isfinite(path).all()
    bound = [b for b in built if b._handle is not None]
    assert len(bound) == 1 and bound[0].dim == 28 and bound[0].T == T, [(b.dim, b.T) for b in built]
    names = set(bound[0].handle().profile())
    assert len(names) == 1 and "k_wide_post_rand" in next(iter(names)), names
    # a sample of the posterior lies near the data: within a few posterior standard deviations of the posterior mean
    m, sd = P.marginals(P.posterior(fx, y)(fx.x, 1e-6))
    assert np.max(np.abs(path - np.asarray(m)) / np.asarray(sd)) < 7.0


def wide_head(model, T):
    """n0 of the wide-state engine's plan for this model and length (the pure host function tgp_wide_plan)"""
    from temporalgps_jl_amd import _lib
    lib = _lib.load()
    d = len(model["x0m"])
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))      # noqa: E731
    blocks = [c(model["A"][0].T), c(model["a"][0]), c(model["Q"][0].T), c(model["H"][0]), c(np.atleast_1d(model["h"])[:1]),
              c(np.atleast_1d(model["R"])[:1]), c(model["x0m"]), c(model["x0P"].T)]
    info, K, S, vp = np.zeros(8, dtype=np.int64), np.zeros(d), np.zeros(1), np.zeros(2)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert lib.tgp_wide_plan(d, *[p(b) for b in blocks], T, 0, p(info), p(K), p(S), p(vp)) == 0 and info[0] == 0, info
    return int(info[1])


@pytest.mark.parametrize("d", [9, 12])
def test_no_stale_reduction_or_diagnostic_behind_a_wide_draw(tgp, d):
    """item 7: a general-engine call on y1, then a wide posterior draw on y2, then a TGP_REUSE_REDUCE call (which the wide engine declines) must not run
    on the reduction of y1; tgp_steady_steps reports the draw (T - n0 of T)"""
    T = 3000
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)
    rng = np.random.default_rng(d)
    mk = lambda: ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))      # noqa: E731
    y1, y2 = mk(), mk()
    eps = (rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    dm = device_model(tgp, model, wide=0)
    hd = dm.handle()
    lib = hd.lib
    p = lambda x: x.ctypes.data      # noqa: E731
    lml = ctypes.c_double()
    mean, var, Rn = np.zeros(T), np.zeros(T), np.array([1e-18])
    hd.check(lib.tgp_logpdf_and_posterior_marginals(hd.h, p(y1), None, p(Rn), tgp._lib.SHARED_R, ctypes.byref(lml), p(mean), p(var)))   # general engine, y1
    hd.set_option(tgp._lib.OPT_WIDE, 1)
    (rc, path), names = kernels_of(tgp, dm, lambda: draw_c(tgp, dm, y2, np.array([1e-6]), eps))
    assert rc == 0 and any("k_wide_post_rand" in n for n in names), (rc, names)
    want = ref.rand(ref.replace_observation_noise_cov(ref.posterior(model, y2), np.array([1e-6])), *eps)
    assert np.max(np.abs(path - want)) <= REL_RESTATEMENT[d] * np.abs(want).max()
    fast, total = ctypes.c_int64(), ctypes.c_int64()
    hd.check(lib.tgp_steady_steps(hd.h, ctypes.byref(fast), ctypes.byref(total)))
    hd.check(lib.tgp_logpdf_and_posterior_marginals(hd.h, p(y2), None, p(Rn), tgp._lib.SHARED_R | tgp._lib.REUSE_REDUCE, ctypes.byref(lml),
                                                    p(mean), p(var)))
    lp_ref = ref.logpdf(model, y2)
    assert abs(lml.value - lp_ref) <= 1e-10 * abs(lp_ref), (lml.value, lp_ref, ref.logpdf(model, y1))
    m_ref, _ = tgp.posterior_marginals(device_model(tgp, model, wide=0), y2, Rn)       # a fresh handle
    assert np.max(np.abs(mean - m_ref)) <= 1e-8 * max(1.0, np.abs(m_ref).max()), np.max(np.abs(mean - m_ref))
    n0 = wide_head(model, T)
    assert 0 < n0 < T and (fast.value, total.value) == (T - n0, T), (fast.value, total.value, n0)
