"""GPU tier: the adjoint gradient of logpdf on the wide-state engine (8 < d <= 63; csrc/tgp_wide.hip: tgp_wide::adjoint) -- block gradients against
central differences of the oracle's sequential logpdf along random directions (every backward family: one, two and three components per lane, the LDS
form), hyper-parameter gradients of products of kernels (lti_sde.jl:377-400) against the tangent scans and against differences of the oracle, a long
series against the device logpdf and the "fd" route, the models it refuses, and no stale reduction behind it."""
import ctypes

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref
from tests._util import BOUNDARY_KERNELS, wide_form_label

pytestmark = pytest.mark.gpu

BLOCKS = ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")
KERNELS = {
    12: ("product", ("matern32",), ("approx_periodic", 3, 1.0)),
    28: ("product", ("approx_periodic", 7, 1.3), ("matern32",)),
    42: ("product", ("approx_periodic", 7, 1.3), ("matern52",)),
    60: ("product", ("approx_periodic", 10, 1.3), ("matern52",)),
    # the two upper form boundaries and the observer in the wave's last lane (tests/test_gpu_wide_edges.py)
    **{d: BOUNDARY_KERNELS[d] for d in (31, 32, 47, 48, 63)},
}


def adjoint_label(d):
    """the profile label of the adjoint call: the form the plan chose names the backward family too (k_wide_bwd4<NB, true> behind k_wide_lml4<true, NB>,
    k_wide_bwd<DP, true> behind k_wide_lml<DP>)"""
    return "k_wide_adjoint: " + wide_form_label(d) + " + k_wide_bwd + k_wide_gram"


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


def profiled(tgp, dm, fn):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    out = fn()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out, names


def oracle_model(blocks, T):
    return dict(ordering="F", kind="scalar", T=T, A=blocks["A"][None], a=blocks["a"][None], Q=blocks["Q"][None], H=blocks["H"][None],
                h=np.array([float(blocks["h"])]), R=np.array([float(blocks["R"])]), x0m=np.asarray(blocks["x0m"], float), x0P=np.asarray(blocks["x0P"], float))


@pytest.mark.parametrize("d", sorted(KERNELS))
def test_block_gradients_against_directional_differences_of_the_oracle(tgp, d):
    T = 2000
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.2, T), 0.1)
    model["h"] = np.array([0.3])
    rng = np.random.default_rng(d)
    y = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    dm = device_model(tgp, model)
    (lp, g), names = profiled(tgp, dm, lambda: tgp.lgssm.logpdf_adjoint(dm, y))
    assert names and all(n.startswith("k_wide_adjoint") for n in names), names
    assert names == {adjoint_label(d)}, (d, names)
    lp_ref = ref.logpdf(model, y)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)
    eps = 1e-6
    for _ in range(3):
        D = {}
        for k in BLOCKS:
            v = np.asarray(model[k][0] if k in ("A", "a", "Q", "H", "h", "R") else model[k], dtype=float)
            z = rng.standard_normal(v.shape) * (np.abs(v) + 1e-3 * max(1e-3, np.abs(v).max()))      # (see test_wide_adjoint_host.py)
            D[k] = 0.5 * (z + z.T) if k in ("Q", "x0P") else z

        def shifted(sgn):
            m = dict(model)
            for k in ("A", "a", "Q", "H"):
                m[k] = model[k] + sgn * eps * D[k][None]
            for k in ("h", "R", "x0m", "x0P"):
                m[k] = model[k] + sgn * eps * D[k]
            return ref.logpdf(m, y)

        fd = (shifted(1.0) - shifted(-1.0)) / (2 * eps)
        terms = [float(np.sum(np.asarray(g[k]) * D[k])) for k in BLOCKS]
        ad, gross = sum(terms), sum(abs(t) for t in terms)
        assert abs(ad - fd) <= 2e-6 * max(1.0, abs(fd), gross), (d, ad, fd, gross)


def test_hyper_parameters_of_products_of_kernels(tgp):
    from temporalgps_jl_amd import lti_sde as P
    # d = 9 against the tangent scans (an independent engine)
    T = 3000
    rng = np.random.default_rng(9)
    y = rng.standard_normal(T)
    fx = P.to_sde(P.GP(0.3, 0.8 * (P.Matern52Kernel() * P.Matern52Kernel().stretch(0.7))))(P.RegularSpacing(0.0, 0.1, T), 0.2)
    assert fx.build_lgssm().dim == 9
    lp_a, g_a = P.logpdf_and_gradient(fx, y, method="adjoint")
    lp_t, g_t = P.logpdf_and_gradient(fx, y, method="tangent")
    assert list(g_a) == list(g_t)
    assert abs(lp_a - lp_t) <= 1e-11 * abs(lp_t)
    scale = max(abs(v) for v in g_t.values())
    for n in g_t:
        assert abs(g_a[n] - g_t[n]) <= 1e-8 * scale, (n, g_a[n], g_t[n])
    # d = 28: sigma^2 (ApproxPeriodicKernel().stretch(s1) * Matern32Kernel().stretch(s2)) with a constant mean, against differences of the oracle
    T = 5000
    k = 1.4 * (P.ApproxPeriodicKernel(7, 1.1).stretch(0.8) * P.Matern32Kernel().stretch(0.3))
    fx = P.to_sde(P.GP(0.25, k))(P.RegularSpacing(0.0, 0.05, T), 0.1)
    assert fx.build_lgssm().dim == 28
    y = np.sin(np.arange(T) * 0.3) + rng.standard_normal(T) * 0.3
    lp, g = P.logpdf_and_gradient(fx, y, method="adjoint")
    plist = P.parameters(fx.f.f.kernel)
    assert list(g) == [n for n, _, _ in plist] + ["noise", "mean.c"] and len(g) == 6

    def lp_oracle():
        return ref.logpdf(oracle_model(P._shared_blocks(fx), T), y)

    assert abs(lp - lp_oracle()) <= 1e-10 * abs(lp)
    entries = list(plist) + [("noise", None, None), ("mean.c", fx.f.f.mean, "c")]
    for name, owner, attr in entries:
        v0 = float(fx.sigma2[0]) if owner is None else getattr(owner, attr)
        hs = 1e-6 * abs(v0)
        vals = []
        for sgn in (1.0, -1.0):
            if owner is None:
                fx.sigma2 = np.array([v0 + sgn * hs])
            else:
                setattr(owner, attr, v0 + sgn * hs)
            vals.append(lp_oracle())
        if owner is None:
            fx.sigma2 = np.array([v0])
        else:
            setattr(owner, attr, v0)
        fd = (vals[0] - vals[1]) / (2 * hs)
        assert abs(g[name] - fd) <= 2e-6 * max(1.0, abs(fd)), (name, g[name], fd)


def test_long_series_on_the_device(tgp):
    import torch
    from temporalgps_jl_amd import lti_sde as P
    T = 1_000_000
    k = 1.4 * (P.ApproxPeriodicKernel(7, 1.1).stretch(0.8) * P.Matern32Kernel().stretch(0.3))
    fx = P.to_sde(P.GP(0.25, k))(P.RegularSpacing(0.0, 0.05, T), 0.1)
    rng = np.random.default_rng(28)
    y = torch.as_tensor(np.sin(np.arange(T) * 0.3) + rng.standard_normal(T) * 0.3, device="cuda")
    lp_a, g_a = P.logpdf_and_gradient(fx, y, method="adjoint")
    lp = P.logpdf(fx, y)
    assert abs(lp_a - lp) <= 1e-12 * abs(lp), (lp_a, lp)
    lp_b, g_b = P.logpdf_and_gradient(fx, y, method="adjoint")
    assert lp_b == lp_a and g_b == g_a                         # bit-identical
    _, g_f = P.logpdf_and_gradient(fx, y, method="fd")
    scale = max(abs(v) for v in g_f.values())
    for n in g_f:
        assert abs(g_a[n] - g_f[n]) <= 1e-6 * scale, (n, g_a[n], g_f[n])


def test_what_the_wide_adjoint_refuses(tgp):
    from temporalgps_jl_amd import lti_sde as P
    Unsup = (tgp._lib.Unsupported, NotImplementedError)
    T = 3000
    k = P.ApproxPeriodicKernel(7, 1.1) * P.Matern32Kernel()
    fx = P.to_sde(P.GP(k))(P.RegularSpacing(0.0, 0.05, T), 0.1)
    y = np.random.default_rng(1).standard_normal(T)
    assert np.isfinite(P.logpdf_and_gradient(fx, y, method="adjoint")[0])
    ym = y.copy()
    ym[7] = np.nan
    with pytest.raises(Unsup):                                                     # missing data
        P.logpdf_and_gradient(fx, ym, method="adjoint")
    with pytest.raises(Unsup):                                                     # noise per step
        P.logpdf_and_gradient(P.to_sde(P.GP(k))(P.RegularSpacing(0.0, 0.05, T), np.full(T, 0.1)), y, method="adjoint")
    with pytest.raises(Unsup):                                                     # a mean function at the inputs
        P.logpdf_and_gradient(P.to_sde(P.GP(P.CustomMean(np.sin), k))(P.RegularSpacing(0.0, 0.05, T), 0.1), y, method="adjoint")
    with pytest.raises(Unsup):                                                     # never settles
        P.logpdf_and_gradient(P.to_sde(P.GP(P.ApproxPeriodicKernel()))(P.RegularSpacing(0.0, 0.05, T), 0.1), y, method="adjoint")
    model = oc.build_lgssm(KERNELS[28], ("regular", 0.0, 0.2, T), 0.1)
    y28 = ref.rand(model, *(np.random.default_rng(2).standard_normal(s) for s in ((T, 28), T, 28)))
    with pytest.raises(tgp._lib.Unsupported):                                      # TGP_OPT_WIDE = 0
        tgp.lgssm.logpdf_adjoint(device_model(tgp, model, wide=0), y28)
    info = np.zeros(8, dtype=np.int64)
    z = lambda n: np.zeros(n)
    b = {k: np.ascontiguousarray(model[k][0].T if k in ("A", "Q") else model[k][0]) for k in ("A", "a", "Q", "H")}
    x0P = np.ascontiguousarray(model["x0P"].T)
    p = lambda x: x.ctypes.data
    tgp._lib.load().tgp_wide_plan(28, p(b["A"]), p(b["a"]), p(b["Q"]), p(b["H"]), p(np.atleast_1d(model["h"])), p(np.atleast_1d(model["R"])), p(model["x0m"]), p(x0P),
                                  T, 0, p(info), p(z(28)), p(z(1)), p(z(2)))
    n0 = int(info[1])
    assert info[0] == 0 and n0 > 0
    Ts = n0 + 63                                                                   # shorter than head + 64
    short = oc.build_lgssm(KERNELS[28], ("regular", 0.0, 0.2, Ts), 0.1)
    with pytest.raises(tgp._lib.Unsupported):
        tgp.lgssm.logpdf_adjoint(device_model(tgp, short), y28[:Ts])
    long_enough = oc.build_lgssm(KERNELS[28], ("regular", 0.0, 0.2, n0 + 64), 0.1)
    lp, _ = tgp.lgssm.logpdf_adjoint(device_model(tgp, long_enough), y28[:n0 + 64])
    assert abs(lp - ref.logpdf(long_enough, y28[:n0 + 64])) <= 1e-10 * abs(lp)


def test_no_stale_reduction_behind_the_adjoint_call(tgp):
    T, d = 3000, 28
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.2, T), 0.1)
    rng = np.random.default_rng(5)
    y1 = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    y2 = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    dm = device_model(tgp, model, wide=0)
    hd = dm.handle()
    lib = hd.lib
    p = lambda x: x.ctypes.data
    lml = ctypes.c_double()
    hd.check(lib.tgp_logpdf(hd.h, p(y1), None, 0, ctypes.byref(lml)))             # the general path on y1
    hd.set_option(tgp._lib.OPT_WIDE, 1)
    g = [np.zeros(d * d), np.zeros(d), np.zeros(d * d), np.zeros(d), np.zeros(1), np.zeros(1), np.zeros(d), np.zeros(d * d)]
    hd.check(lib.tgp_logpdf_adjoint(hd.h, p(y2), 0, ctypes.byref(lml), *[p(x) for x in g]))      # the wide adjoint pass on y2
    lp2 = lml.value
    hd.set_option(tgp._lib.OPT_WIDE, 0)
    mean, var, Rn = np.zeros(T), np.zeros(T), np.array([1e-18])
    hd.check(lib.tgp_logpdf_and_posterior_marginals(hd.h, p(y2), None, p(Rn), tgp._lib.SHARED_R | tgp._lib.REUSE_REDUCE, ctypes.byref(lml), p(mean), p(var)))
    lp_ref = ref.logpdf(model, y2)
    assert abs(lp2 - lp_ref) <= 1e-10 * abs(lp_ref)
    assert abs(lml.value - lp_ref) <= 1e-10 * abs(lp_ref), (lml.value, lp_ref, ref.logpdf(model, y1))
    m_ref, _ = tgp.posterior_marginals(device_model(tgp, model, wide=0), y2, Rn)       # a fresh handle
    assert np.max(np.abs(mean - m_ref)) <= 1e-8 * max(1.0, np.abs(m_ref).max())
