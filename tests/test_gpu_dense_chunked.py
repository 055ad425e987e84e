"""GPU tier: the dense engine's persistent passes across the chip (csrc/tgp_dense_chunked.hpp, TGP_OPT_DENSE_CHUNKED; 16 < d <= 64, p <= 16, Forward models
whose gains vary in time) -- a workgroup per chunk of steps behind a checked warm-up -- against the literal restatement (oracle/lgssm_ref.py) and against
the sequential passes of the same handle (option 20 = 0).  Every case asserts the diagnostic (tgp_dense_chunk_info): served, more than one chunk, one
attempt each way, both hand-over distances below their tolerance -- so that a silent fallback cannot pass the parity asserts.

The forced geometries of the product-kernel models are those of scripts/dense_chunk_proto.py (tests/test_dense_chunk_proto.py: the restatement passes both
checks there with no repair).  The random dense models (tests/test_gpu_dense.py's random_model, copied) contract by |A_t| ~ U(0.4, 0.9) per step even without
an observation: 96 steps leave e^(96 E log rho) ~ 1e-19 of a start state, far below the checks' 1e-12."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import lgssm_ref as ref

from tests._util import DENSE_TOL_B as TOL_B
from tests._util import DENSE_TOL_F as TOL_F
from tests._util import against_sequential, forced, random_model, scalar_dev, sequential, served_once, vector_dev, with_missing

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


@pytest.fixture(scope="module")
def proto():
    spec = importlib.util.spec_from_file_location("dense_chunk_proto", os.path.join(ROOT, "scripts", "dense_chunk_proto.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ product kernels, DP = 32, 48, 64
@pytest.mark.parametrize("d", (18, 28, 42, 54))
def test_product_kernel_parity_with_missing_data_and_a_noise_variance_per_step(tgp, proto, d):
    """10 % of the steps missing AND a noise variance per step; T = 4100 in chunks of 530 (a short last chunk), W = Wb = 128"""
    model, geometry = proto.test_model(d)
    mdl, y, missing = proto.test_series(model, d, per_step_noise=True)
    T = mdl["T"]
    assert T % geometry[0] != 0 and len(mdl["x0m"]) == d
    yin = np.where(missing, np.nan, y)
    Rn = np.array([0.05])
    dm = scalar_dev(tgp, mdl, geometry)
    lp_ref = ref.logpdf_missing(mdl, y, missing)
    lp = tgp.logpdf(dm, yin)
    info = served_once(dm, False)
    print(d, "logpdf", abs(lp - lp_ref) / abs(lp_ref), info)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)
    fm_ref, fP_ref = ref.filter_missing(mdl, y, missing)
    fm, fP = tgp._filter(dm, yin)
    served_once(dm, False)
    np.testing.assert_allclose(fm, fm_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(fm_ref).max()))
    np.testing.assert_allclose(fP, fP_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(fP_ref).max()))
    pm, pv = ref.marginals(ref.replace_observation_noise_cov(ref.posterior_missing(mdl, y, missing), np.full(T, Rn[0])))
    pm, pv = np.asarray(pm).reshape(T), np.asarray(pv).reshape(T)
    out = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = served_once(dm, True)
    print(d, "posterior", np.abs(out[1] - pm).max() / max(1.0, np.abs(pm).max()), np.abs(out[2] - pv).max() / max(1.0, pv.max()), info)
    assert abs(out[0] - lp_ref) <= 1e-10 * abs(lp_ref)
    np.testing.assert_allclose(out[1], pm, rtol=0, atol=1e-6 * max(1.0, np.abs(pm).max()))
    np.testing.assert_allclose(out[2], pv, rtol=0, atol=1e-6 * max(1.0, pv.max()))
    seq = sequential(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, yin, Rn))
    against_sequential(out, seq)
    fm0, fP0 = sequential(tgp, dm, lambda: tgp._filter(dm, yin))
    np.testing.assert_allclose(fm, fm0, rtol=0, atol=1e-9 * max(1.0, np.abs(fm0).max()))
    np.testing.assert_allclose(fP, fP0, rtol=0, atol=1e-9 * max(1.0, np.abs(fP0).max()))


# ------------------------------------------------------------------------------------------------ edges (d = 18: the smallest model that has them)
@pytest.fixture(scope="module")
def edge(proto):
    from oracle import components as oc
    T = 2400                  # exactly 8 chunks of 300
    model = oc.build_lgssm(proto.KERNELS[18], ("regular", 0.0, 0.2, T), 0.1)
    mdl, y, _ = proto.test_series(model, 77, frac_missing=0.0)
    return mdl, y


def _edge_case(tgp, edge, missing, geometry, T=None):
    mdl, y = edge
    T = T or mdl["T"]
    mdl, y, missing = dict(mdl, T=T), y[:T], missing[:T]
    yin = np.where(missing, np.nan, y)
    Rn = np.array([0.05])
    dm = scalar_dev(tgp, mdl, geometry)
    out = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = served_once(dm, True)
    lp_ref = ref.logpdf_missing(mdl, y, missing)
    assert abs(out[0] - lp_ref) <= 1e-10 * abs(lp_ref), (out[0], lp_ref)
    m_bf, v_bf = ref.bryson_frazier_marginals(mdl, y, Rn, missing=missing)      # (the exact posterior: the sequential form of the same recursion, 1e-8)
    np.testing.assert_allclose(out[1], m_bf, rtol=0, atol=1e-8 * max(1.0, np.abs(m_bf).max()))
    np.testing.assert_allclose(out[2], v_bf, rtol=0, atol=1e-8 * max(1.0, v_bf.max()))
    against_sequential(out, sequential(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, yin, Rn)))
    return dm, yin, Rn, out, info


def test_missing_steps_on_both_sides_of_every_chunk_boundary_and_at_both_ends_of_the_series(tgp, edge):
    T, C = edge[0]["T"], 300
    missing = np.zeros(T, dtype=bool)
    for s in range(C, T, C):
        missing[s - 3:s + 3] = True
    missing[0] = missing[T - 1] = True
    *_, info = _edge_case(tgp, edge, missing, (C, 128, 128))
    assert info["chunks"] == 8 and info["C"] == C         # T is exactly 8 chunks


def test_warm_up_longer_than_a_chunk_starts_at_step_zero(tgp, edge):
    T = 830
    missing = np.random.default_rng(3).random(T) < 0.1
    *_, info = _edge_case(tgp, edge, missing, (100, 128, 128), T=T)       # chunk 1 = [100, 200) starts at max(0, 100 - 128) = 0
    assert info["chunks"] == 9 and info["W"] > info["C"]


def test_two_identical_calls_are_bit_identical(tgp, edge):
    T = 1250
    missing = np.random.default_rng(4).random(T) < 0.1
    dm, yin, Rn, out, _ = _edge_case(tgp, edge, missing, (300, 128, 128), T=T)
    again = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    served_once(dm, True)
    assert out[0] == again[0]
    assert np.asarray(out[1]).tobytes() == np.asarray(again[1]).tobytes() and np.asarray(out[2]).tobytes() == np.asarray(again[2]).tobytes()
    f1, f2 = tgp._filter(dm, yin), tgp._filter(dm, yin)
    served_once(dm, False)
    assert np.asarray(f1[0]).tobytes() == np.asarray(f2[0]).tobytes() and np.asarray(f1[1]).tobytes() == np.asarray(f2[1]).tobytes()
    assert tgp.logpdf(dm, yin) == tgp.logpdf(dm, yin) == out[0]


# ------------------------------------------------------------------------------------------------ random dense models: vector observations, per-step blocks
@pytest.mark.parametrize("d,p", [(20, 2), (40, 16)])
def test_vector_observations_with_every_block_per_step(tgp, d, p):
    """per-step A, Q (sA != 0), H, h, R and an element-wise mask; p scalar updates per step, forwards and backwards"""
    rng = np.random.default_rng(6000 + d)
    T = 1650          # 9 chunks of 200, the last one of 50
    model, Rd = random_model(rng, T, d, p, per_step=True)
    y = rng.standard_normal((T, p))
    mk = rng.random((T, p)) < 0.15
    yin = np.where(mk, np.nan, y)
    m2, y2, comp = with_missing(model, y, mk)
    dm = vector_dev(tgp, model, Rd, forced(tgp, 200, 96, 96))
    lp_ref = ref.logpdf(m2, y2) + comp
    lp = tgp.logpdf(dm, yin)
    served_once(dm, False)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)
    fm_ref, fP_ref = ref.filter_(m2, y2)
    fm, fP = tgp._filter(dm, yin)
    served_once(dm, False)
    np.testing.assert_allclose(fm, fm_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(fm_ref).max()))
    np.testing.assert_allclose(fP, fP_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(fP_ref).max()))
    Rn = rng.uniform(0.01, 0.2, size=(T, p))
    out = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    served_once(dm, True)
    pm, pC = ref.marginals(ref.replace_observation_noise_cov(ref.posterior(m2, y2), np.stack([np.diag(r) for r in Rn])))
    np.testing.assert_allclose(out[1], pm, rtol=0, atol=1e-6 * max(1.0, np.abs(pm).max()))
    pv = np.diagonal(pC, axis1=-2, axis2=-1)
    np.testing.assert_allclose(out[2], pv, rtol=0, atol=1e-6 * max(1.0, pv.max()))
    against_sequential(out, sequential(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, yin, Rn)))


# ------------------------------------------------------------------------------------------------ repair and declines
def _strongly_observed(rng, T, d=20, p=16):
    """A = 0.995 x orthogonal, stationary prior: without observations a state is remembered for hundreds of steps, with 16 accurate ones per step for a few
    dozen -- the first guess (the fully observed closed loop) is short, and a missing stretch defeats it"""
    rho = 0.995
    A = (np.linalg.qr(rng.standard_normal((d, d)))[0] * rho)[None]
    model = dict(ordering="F", kind="small", T=T, A=A, a=np.zeros((1, d)), Q=((1 - rho ** 2) * np.eye(d))[None], H=rng.standard_normal((1, p, d)) / np.sqrt(d),
                 h=np.zeros((1, p)), R=np.stack([0.01 * np.eye(p)] * T), x0m=np.zeros(d), x0P=np.eye(d))
    return model, np.full((T, p), 0.01)


def test_a_missing_stretch_is_repaired_by_a_longer_warm_up_and_declined_under_a_forced_one(tgp):
    rng = np.random.default_rng(11)
    T, p = 5000, 16          # (the first guess of this model is 144 steps: 8 chunks of 4 x 144)
    model, Rd = _strongly_observed(rng, T)
    y = ref.rand(model, rng.standard_normal((T, 20)), rng.standard_normal((T, p)), rng.standard_normal(20))
    L = tgp._lib
    pilot = vector_dev(tgp, model, Rd, {})
    lp0 = tgp.logpdf(pilot, y)
    first = pilot.handle().dense_chunk_info()
    assert first["served"] == 1 and first["attempts"] == 1 and first["chunks"] >= 8 and first["C"] >= 4 * first["W"], first
    lp_ref0 = ref.logpdf(model, y)
    assert abs(lp0 - lp_ref0) <= 1e-10 * abs(lp_ref0)
    # one stretch of 3 W0 steps: 1.1 W0 in front of a chunk boundary (the first warm-up lies inside it), 1.9 W0 behind
    W0, C = first["W"], first["C"]
    s = 4 * C
    mk = np.zeros((T, p), dtype=bool)
    mk[s - (11 * W0) // 10:s + (19 * W0) // 10] = True
    yin = np.where(mk, np.nan, y)
    m2, y2, comp = with_missing(model, y, mk)
    lp_ref = ref.logpdf(m2, y2) + comp
    fm_ref, fP_ref = ref.filter_(m2, y2)

    def check(dm):
        lp = tgp.logpdf(dm, yin)
        info = dm.handle().dense_chunk_info()
        assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref, info)
        fm, fP = tgp._filter(dm, yin)
        np.testing.assert_allclose(fm, fm_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(fm_ref).max()))
        np.testing.assert_allclose(fP, fP_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(fP_ref).max()))
        return info, dm.handle().dense_chunk_info()

    info, later = check(vector_dev(tgp, model, Rd, {}))
    assert info["served"] == 1 and info["attempts"] >= 2 and info["W"] > W0 and info["dist_f"] <= TOL_F, info
    assert later["served"] == 1 and later["attempts"] == 1 and later["W"] == info["W"], later      # (the bound model remembers the W it needed)
    info, later = check(vector_dev(tgp, model, Rd, {L.OPT_DENSE_WARMUP: W0}))
    assert info["served"] == 0 and info["status"] & 1 and info["attempts"] == 1 and info["state"] == -1 and info["dist_f"] > TOL_F, info
    assert later["served"] == 0 and later["attempts"] == 0 and later["state"] == -1, later         # (no new attempt on the bound model)


def test_declines_leave_the_sequential_passes_results(tgp):
    rng = np.random.default_rng(12)
    L = tgp._lib
    T, d, p = 1650, 24, 3
    y = rng.standard_normal((T, p))
    # a Reverse-ordered model
    model, Rd = random_model(rng, T, d, p, ordering="R")
    dm = vector_dev(tgp, model, Rd, forced(tgp, 200, 96, 96))
    lp = tgp.logpdf(dm, y)
    info = dm.handle().dense_chunk_info()
    assert info["served"] == 0 and info["attempts"] == 0, info
    lp_ref = ref.logpdf(model, y)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    # option 20 = 0 against the default on a model the chunks serve: what the sequential passes give, and no attempt
    model, Rd = random_model(rng, T, d, p)
    on, off = vector_dev(tgp, model, Rd, forced(tgp, 200, 96, 96)), vector_dev(tgp, model, Rd, {**forced(tgp, 200, 96, 96), L.OPT_DENSE_CHUNKED: 0})
    a, b = tgp.logpdf(on, y), tgp.logpdf(off, y)
    assert on.handle().dense_chunk_info()["served"] == 1
    info = off.handle().dense_chunk_info()
    assert info["served"] == 0 and info["attempts"] == 0, info
    lp_ref = ref.logpdf(model, y)
    assert abs(a - lp_ref) <= 1e-10 * abs(lp_ref) and abs(b - lp_ref) <= 1e-10 * abs(lp_ref)
    # a series shorter than 8 chunks of 4 warm-ups (automatic geometry; the warm-up is at least 32 steps): never tried
    short, Rs = random_model(rng, 200, d, p)
    dm = vector_dev(tgp, short, Rs, {})
    ys = rng.standard_normal((200, p))
    lp = tgp.logpdf(dm, ys)
    info = dm.handle().dense_chunk_info()
    assert info["served"] == 0 and info["attempts"] == 0 and info["state"] == 0, info
    lp_ref = ref.logpdf(short, ys)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)


# ------------------------------------------------------------------------------------------------ the public route
def test_gp_prediction_at_new_inputs_runs_across_the_chip(tgp, monkeypatch):
    """marginals(posterior(fx, y)(x_new)) (posterior_lti_sde.jl:20-37, 97-131) on ApproxPeriodicKernel() * Matern32Kernel() (d = 28): training and
    prediction inputs merged, the prediction points missing -- the wide engine declines the mask, the dense engine's chunks serve the model with default
    options.  Values against the dense GP on the kernel itself, at tests/test_gpu_wide.py's tolerance for this model."""
    from oracle import dense_gp as dg
    from temporalgps_jl_amd import lti_sde as P
    rng = np.random.default_rng(2)
    ntr, npr = 2400, 600
    x = P.RegularSpacing(0.0, 0.5, ntr)
    xs = x.collect()
    x_new = np.sort(rng.uniform(xs[0], xs[-1], npr))
    f = P.to_sde(P.GP(P.ApproxPeriodicKernel() * P.Matern32Kernel()), P.HIPStorage())
    fx = f(x, 0.1)
    y = np.asarray(P.rand(rng, fx))
    built, real = [], P.build_lgssm

    def recorded(*a, **k):
        mdl = real(*a, **k)
        built.append(mdl)
        return mdl
    monkeypatch.setattr(P, "build_lgssm", recorded)
    m, sd = P.marginals(P.posterior(fx, y)(x_new, 1e-9))
    merged = [b for b in built if b.T == ntr + npr]
    assert merged and merged[-1].dim == 28
    info = merged[-1].handle().dense_chunk_info()
    assert info["served"] == 1 and info["chunks"] >= 8 and info["dist_f"] <= TOL_F and info["dist_b"] <= TOL_B, info
    md, vd = dg.posterior_marginals(("product", ("approx_periodic", 7, 1.0), ("matern32",)), xs, 0.1, y, x_new, 1e-9)
    assert np.max(np.abs(np.asarray(m) - md)) <= 1e-4 and np.max(np.abs(np.asarray(sd) ** 2 - vd)) <= 1e-4
