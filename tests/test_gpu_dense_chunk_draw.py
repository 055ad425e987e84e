"""GPU tier: a draw from the posterior on the dense engine (tgp_posterior_rand_missing: dk_chunk_filter, then dk_chunk_draw / dk_fused_draw, DESIGN 4.6;
csrc/tgp_dense_draw.hpp) against the reference restated in NumPy on the SAME draws (ref.posterior_missing + ref.replace_observation_noise_cov + ref.rand
through scripts/dense_chunk_draw_proto.py: oracle()), through ctypes on the C entry unless a test says otherwise.

The bar is the project's bar for draws at these sizes: 1e-6 of the path's largest value (tests/test_gpu_wide_draw.py: REL_RESTATEMENT); the NumPy
prototype of the kernels' algorithm stands at <= 1e-7 on every case used here (tests/test_dense_chunk_draw_proto.py).  Every case asserts
tgp_dense_chunk_info, so that a silent fallback cannot pass.  T <= 3000; small series are chunked through the forced geometry of options 21 / 22 / 23.

Measured on an MI355X (largest |difference| over the largest |entry| of the restatement's path): the six template edges 4.9e-16 ... 2.7e-15, hand-over
distances 5.2e-15 ... 8.3e-15; one block per step 4.2e-16 ... 1.3e-15; p = 3 / p = 16: 7.1e-16 / 1.5e-15; zero draws against the marginals call's mean
2.0e-11 ... 4.2e-11, the prototype's own distance to within 1e-15 of it; a forced Wd = 4: distance 0.23, the sequential pass serves; the repair case: Wd 36
fails, 72 passes at 3.0e-16; T = 1e6 at d = 28: 512 chunks of 1954, Wd = 288, distance 1.4e-15."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import lgssm_ref as ref

from tests._util import DENSE_TOL_B as TOL_B
from tests._util import forced, kernels_of, random_model, scalar_dev, vector_dev

pytestmark = pytest.mark.gpu
REL = 1e-6
T1, GEOM = 700, (96, 96, 64)          # 8 chunks of 96, the last one of 28; the draw pass's warm-up in the backward slot
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _proto():
    spec = importlib.util.spec_from_file_location("dense_chunk_draw_proto", os.path.join(ROOT, "scripts", "dense_chunk_draw_proto.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


proto = _proto()


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def as_scalar(model, Rd):
    return dict(model, kind="scalar", H=model["H"][:, 0, :], h=model["h"][:, 0], R=np.ascontiguousarray(Rd[:, 0]))


def make_case(seed, T, d, p, rho=0.6, per_step=False, frac=0.1, shared_rn=False):
    """(model in the oracle's shapes, Rd (vector models), y, mask, Rnew as the C entry takes it, draws)"""
    rng = np.random.default_rng(seed)
    model, Rd = random_model(rng, T, d, p, per_step=per_step, rho=rho)
    if p == 1:
        model, Rd = as_scalar(model, Rd), None
    shape = (T,) if p == 1 else (T, p)
    y, mk = rng.standard_normal(shape), rng.random(shape) < frac
    Rn = rng.uniform(0.01, 0.2, size=(1,) + shape[1:] if shared_rn else shape)
    eps = (rng.standard_normal((T, d)), rng.standard_normal(shape), rng.standard_normal(d))
    return model, Rd, y, mk, Rn, eps


def device(tgp, model, Rd, geometry, fused=2):
    if Rd is None:
        return scalar_dev(tgp, model, geometry, fused)
    L = tgp._lib
    opts = forced(tgp, *geometry, fused=fused) if geometry else {L.OPT_DENSE_FUSED: fused}
    return vector_dev(tgp, model, Rd, {L.OPT_WIDE: 0, **opts})


def restatement(model, y, mk, Rn, eps):
    Rr = Rn if model["kind"] == "scalar" else np.stack([np.diag(r) for r in Rn])
    return proto.oracle(model, y, mk, Rr, *eps)


def draw_call(tgp, dm, y, mk, Rn, eps, fill=np.nan):
    """tgp_posterior_rand_missing through ctypes on host arrays: (return code, path)"""
    hd, L = dm.handle(), tgp._lib
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64)      # noqa: E731
    yy, Rr, et, ee, e0 = c(np.where(mk, 0.0, y) if mk is not None else y), c(Rn), c(eps[0]), c(eps[1]), c(eps[2])
    mm = None if mk is None else np.ascontiguousarray(mk, dtype=np.uint8)
    out = np.full(yy.shape, fill)
    flags = L.SHARED_R if Rr.shape[0] == 1 else 0
    rc = hd.lib.tgp_posterior_rand_missing(hd.h, L.ptr(yy), L.ptr(mm), L.ptr(Rr), L.ptr(et), L.ptr(ee), L.ptr(e0), flags, L.ptr(out))
    return rc, out


def rel(x, r):
    return float(np.max(np.abs(x - r)) / np.max(np.abs(r)))


def served(dm, geometry=None, attempts=2):
    info = dm.handle().dense_chunk_info()
    assert info["served"] == 1 and info["chunks"] > 1 and info["status"] == 0 and info["state"] == 1, info
    assert attempts is None or info["attempts"] == attempts, info
    assert info["dist_b"] <= TOL_B, info
    if geometry:
        assert (info["C"], info["W"], info["Wb"]) == tuple(geometry), info
    return info


# ------------------------------------------------------------------------------------------------ 1. served and equal, at the edges of the three templates
@pytest.mark.parametrize("d", (17, 32, 33, 48, 49, 64))
def test_served_and_equal_to_the_restatement(tgp, d):
    """The entry point does not exist before the draw pass: this test fails there."""
    model, Rd, y, mk, Rn, eps = make_case(1000 + d, T1, d, 1)
    dm = device(tgp, model, Rd, GEOM)
    (rc, out), names = kernels_of(tgp, dm, lambda: draw_call(tgp, dm, y, mk, Rn, eps))
    assert rc == 0
    assert "dk_chunk_draw" in names and "dk_chunk_filter" in names and "dk_fused_draw" not in names, names
    info = served(dm, GEOM)
    assert info["chunks"] == 8, info
    want = restatement(model, y, mk, Rn, eps)
    print("d", d, "rel", rel(out, want), info)
    assert rel(out, want) <= REL
    rc2, again = draw_call(tgp, dm, y, mk, Rn, eps)
    assert rc2 == 0 and np.array_equal(out, again)


# ------------------------------------------------------------------------------------------------ 2. zero draws: the posterior mean
@pytest.mark.parametrize("d", (17, 32, 33, 48, 49, 64))
def test_zero_draws_give_the_posterior_mean(tgp, d):
    """All draws zero, Rnew = 1e-18: the path is the smoothed mean of the reference's reverse-time model, the marginals call's mean is the exact
    posterior's (Bryson-Frazier).  The two differ by the effect of the reference's jitters; the tolerance is ten times what the NumPy prototype's zero
    draw shows against ref.bryson_frazier_marginals on the same case (measured here on the CPU; d = 17: 3.3e-11, d = 64: 2.0e-11 of the mean's size), at
    most 1e-6."""
    model, Rd, y, mk, _, eps = make_case(1000 + d, T1, d, 1)
    zero = tuple(np.zeros_like(e) for e in eps)
    Rn = np.array([1e-18])
    mine = proto.draw(model, proto.forward(model, y, mk), Rn, *zero)["y"]
    bf = ref.bryson_frazier_marginals(model, y, Rn, missing=mk)[0]
    shown = rel(mine, bf)
    tol = min(10.0 * shown, 1e-6)
    dm = device(tgp, model, Rd, GEOM)
    rc, out = draw_call(tgp, dm, y, mk, Rn, zero)
    assert rc == 0
    served(dm, GEOM)
    _, mean, _ = tgp.logpdf_and_posterior_marginals(dm, np.where(mk, np.nan, y), Rn)
    print("d", d, "prototype against Bryson-Frazier", shown, "device", rel(out, mean))
    assert rel(out, mean) <= tol


# ------------------------------------------------------------------------------------------------ 3. geometry edges (d = 17)
# name: (T, (C, W, Wd), chunks; 0: the chunks do not take the geometry and dk_fused_draw serves the call)
# "C = 1": a forced C = 1 is a geometry like any other (T chunks of one step behind their warm-ups; the check passes and the call is served, as the forward
# and backward passes serve it in tests/test_gpu_dense_chunked_edges.py).  The geometry the chunks decline is ONE chunk (C = T): nothing is tried and
# the sequential kernels serve the call.
GEOMETRIES = {
    "last chunk of one step": (7 * 96 + 1, GEOM, 8),
    "two chunks": (T1, (400, 96, 64), 2),
    "warm-up of the whole series": (T1, (96, 96, T1), 8),
    "chunks of one step": (T1, (1, 96, 64), T1),
    "one chunk": (T1, (T1, 96, 64), 0),
    "T not a multiple of C": (T1 + 37, (100, 96, 64), 8),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_geometry_edges(tgp, name):
    T, geometry, chunks = GEOMETRIES[name]
    model, Rd, y, mk, Rn, eps = make_case(2000 + T + geometry[0], T, 17, 1)
    dm = device(tgp, model, Rd, geometry)
    (rc, out), names = kernels_of(tgp, dm, lambda: draw_call(tgp, dm, y, mk, Rn, eps))
    assert rc == 0
    info = dm.handle().dense_chunk_info()
    print(name, info)
    if chunks:
        assert "dk_chunk_draw" in names and "dk_fused_draw" not in names, names
        assert served(dm, geometry)["chunks"] == chunks, info
    else:
        assert "dk_fused_draw" in names and "dk_chunk_draw" not in names, names
        assert info["served"] == 0 and info["attempts"] == 0 and info["status"] == 0, info
    assert rel(out, restatement(model, y, mk, Rn, eps)) <= REL


def test_the_last_chunk_starts_from_the_draw_of_the_final_state(tgp):
    """eps_0 moves the last steps, and only them: behind 128 steps (0.6^128) the two paths agree to 1e-11 of the path's size"""
    model, Rd, y, mk, Rn, eps = make_case(2100, T1, 17, 1)
    dm = device(tgp, model, Rd, GEOM)
    rc0, with0 = draw_call(tgp, dm, y, mk, Rn, eps)
    rc1, without = draw_call(tgp, dm, y, mk, Rn, (eps[0], eps[1], np.zeros_like(eps[2])))
    assert rc0 == 0 and rc1 == 0
    served(dm, GEOM)
    size = np.abs(with0).max()
    assert np.abs(with0[-1] - without[-1]) > 1e-3 * size
    assert np.abs(with0[:-128] - without[:-128]).max() <= 1e-11 * size
    want = restatement(model, y, mk, Rn, eps)
    assert rel(with0, want) <= REL


# ------------------------------------------------------------------------------------------------ 4. decline and repair
def test_a_forced_warm_up_that_is_too_short_hands_over_to_the_sequential_draw(tgp):
    model, Rd, y, mk, Rn, eps = make_case(3000, T1, 17, 1)
    geometry = (96, 96, 4)          # 0.6^4: the check's 1e-11 is out of reach
    dm = device(tgp, model, Rd, geometry)
    (rc, out), names = kernels_of(tgp, dm, lambda: draw_call(tgp, dm, y, mk, Rn, eps))
    assert rc == 0
    info = dm.handle().dense_chunk_info()
    print(info)
    assert info["served"] == 0 and info["status"] & 2 and not info["status"] & 1 and info["attempts"] == 2 and info["Wb"] == 4, info
    assert info["dist_b"] > TOL_B, info
    assert {"dk_chunk_filter", "dk_chunk_draw", "dk_fused_draw"} <= names, names
    want = restatement(model, y, mk, Rn, eps)
    assert rel(out, want) <= REL
    # the decline is the draw pass's own: the filter of the same handle stays across the chip, and the next draw does not try the chunks again
    assert info["state"] == 1, info
    lp = tgp.logpdf(dm, np.where(mk, np.nan, y))
    after = dm.handle().dense_chunk_info()
    lp_ref = ref.logpdf_missing(model, y, mk)
    assert after["served"] == 1 and after["state"] == 1 and abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), after
    (rc, again), names = kernels_of(tgp, dm, lambda: draw_call(tgp, dm, y, mk, Rn, eps))
    later = dm.handle().dense_chunk_info()
    assert rc == 0 and "dk_chunk_draw" not in names and {"dk_chunk_filter", "dk_fused_draw"} <= names, names
    assert later["served"] == 0 and later["status"] == 2 and later["attempts"] == 1 and np.array_equal(out, again), later


def repair_inputs():
    """0.97 x orthogonal, 16 accurate observations per step: the first guess (the fully observed closed loop) is short; a stretch of missing steps
    behind a chunk boundary, where the draw pass's warm-up lies, forgets at 0.97 per step and defeats it"""
    rng = np.random.default_rng(31)
    T, d, p, rho = 3000, 17, 16, 0.97
    A = (np.linalg.qr(rng.standard_normal((d, d)))[0] * rho)[None]
    model = dict(ordering="F", kind="small", T=T, A=A, a=np.zeros((1, d)), Q=((1 - rho ** 2) * np.eye(d))[None], H=rng.standard_normal((1, p, d)) / np.sqrt(d),
                 h=np.zeros((1, p)), R=np.stack([0.01 * np.eye(p)] * T), x0m=np.zeros(d), x0P=np.eye(d))
    Rd = np.full((T, p), 0.01)
    y = rng.standard_normal((T, p))
    Rn = rng.uniform(0.01, 0.2, size=(T, p))
    eps = (rng.standard_normal((T, d)), rng.standard_normal((T, p)), rng.standard_normal(d))
    return model, Rd, y, Rn, eps


def test_a_draw_check_that_fails_is_repaired_by_a_longer_warm_up(tgp):
    """automatic geometry: the first call finds the first guess W0 and its chunks; a stretch of 5 W0 / 4 missing steps behind a boundary then fails the
    draw pass's check at W0 and passes after doubling (the NumPy prototype's run() shows the same on this case, tests/test_dense_chunk_draw_proto.py)"""
    model, Rd, y, Rn, eps = repair_inputs()
    T, p = y.shape
    L = tgp._lib
    pilot = vector_dev(tgp, model, Rd, {L.OPT_WIDE: 0})
    rc, out0 = draw_call(tgp, pilot, y, np.zeros((T, p), dtype=bool), Rn, eps)
    assert rc == 0
    first = served(pilot)
    W0, C = first["Wb"], first["C"]
    assert first["W"] == W0 and C >= 4 * W0, first
    mk = np.zeros((T, p), dtype=bool)
    s = (first["chunks"] // 2) * C
    mk[s:s + (5 * W0) // 4] = True
    dm = vector_dev(tgp, model, Rd, {L.OPT_WIDE: 0})
    rc, out = draw_call(tgp, dm, y, mk, Rn, eps)
    assert rc == 0
    info = dm.handle().dense_chunk_info()
    print(first, info)
    assert info["served"] == 1 and info["status"] == 0 and info["attempts"] > 2 and info["W"] == W0 and info["Wb"] > W0, info
    assert info["dist_b"] <= TOL_B, info
    assert rel(out, restatement(model, y, mk, Rn, eps)) <= REL
    rc, again = draw_call(tgp, dm, y, mk, Rn, eps)
    later = dm.handle().dense_chunk_info()
    assert rc == 0 and later["attempts"] == 2 and later["Wb"] == info["Wb"] and np.array_equal(out, again), later      # (the bound model remembers Wd)


def test_with_the_chunked_passes_off_the_entry_point_declines_and_writes_nothing(tgp):
    model, Rd, y, mk, Rn, eps = make_case(1017, T1, 17, 1)
    dm = device(tgp, model, Rd, GEOM)
    dm.handle().set_option(tgp._lib.OPT_DENSE_CHUNKED, 0)
    rc, out = draw_call(tgp, dm, y, mk, Rn, eps, fill=-7.0)
    assert rc == tgp._lib.EUNSUPPORTED and np.all(out == -7.0)
    dm.handle().set_option(tgp._lib.OPT_DENSE_CHUNKED, 1)
    rc, out = draw_call(tgp, dm, y, mk, Rn, eps, fill=-7.0)
    assert rc == 0 and rel(out, restatement(model, y, mk, Rn, eps)) <= REL


# ------------------------------------------------------------------------------------------------ 5. blocks one at a time (d = 33)
T5 = 500
BLOCKS = ("A", "Q", "H", "R", "a")


def block_case(which):
    """d = 33, p = 2: every block shared but one; "H": H and h per step; "R": R and Rnew per step (else one Rnew); "a": a != 0 per step against a = 0"""
    d, p = 33, 2
    rng = np.random.default_rng(5000 + BLOCKS.index(which))
    model, Rd = random_model(rng, T5, d, p, rho=0.6)
    per_step, _ = random_model(rng, T5, d, p, per_step=True, rho=0.6)
    model["a"] = np.zeros_like(model["a"])
    if which == "a":
        model["a"] = 5.0 * per_step["a"]
    elif which == "H":
        model["H"], model["h"] = per_step["H"], 5.0 * per_step["h"]
    elif which in ("A", "Q"):
        model[which] = per_step[which]
    if which != "R":
        Rd = np.repeat(Rd[:1], T5, axis=0)
        model["R"] = np.stack([np.diag(r) for r in Rd])
    y, mk = rng.standard_normal((T5, p)), rng.random((T5, p)) < 0.1
    Rn = rng.uniform(0.01, 0.2, size=(T5 if which == "R" else 1, p))
    eps = (rng.standard_normal((T5, d)), rng.standard_normal((T5, p)), rng.standard_normal(d))
    return model, Rd, y, mk, Rn, eps


@pytest.mark.parametrize("which", BLOCKS)
def test_one_block_per_step_and_every_other_shared(tgp, which):
    model, Rd, y, mk, Rn, eps = block_case(which)
    dm = device(tgp, model, Rd, GEOM)
    rc, out = draw_call(tgp, dm, y, mk, Rn, eps)
    assert rc == 0
    served(dm, GEOM)
    Rr = np.repeat(Rn, T5, axis=0) if Rn.shape[0] == 1 else Rn
    want = restatement(model, y, mk, Rr, eps)
    print(which, rel(out, want))
    assert rel(out, want) <= REL
    # the mutation of this group: the reference fed the transition draws of the neighbouring step must FAIL the bar
    shifted = restatement(model, y, mk, Rr, (np.roll(eps[0], 1, axis=0), eps[1], eps[2]))
    assert rel(out, shifted) > REL


@pytest.mark.parametrize("d,p", ((33, 3), (17, 16)))
def test_vector_observations_with_an_element_wise_mask(tgp, d, p):
    model, Rd, y, mk, Rn, eps = make_case(5100 + p, T5, d, p, per_step=True)
    assert mk.any(axis=1).sum() > mk.all(axis=1).sum()
    dm = device(tgp, model, Rd, GEOM)
    rc, out = draw_call(tgp, dm, y, mk, Rn, eps)
    assert rc == 0
    served(dm, GEOM)
    want = restatement(model, y, mk, Rn, eps)
    print(d, p, rel(out, want))
    assert rel(out, want) <= REL
    shifted = restatement(model, y, mk, Rn, (eps[0], np.roll(eps[1], 1, axis=0), eps[2]))
    assert rel(out, shifted) > REL


# ------------------------------------------------------------------------------------------------ 6. inputs
def test_device_arrays_host_nan_series_and_a_clean_handle_afterwards(tgp):
    import torch
    model, Rd, y, mk, Rn, eps = make_case(6000, T1, 17, 1)
    dm = device(tgp, model, Rd, GEOM)
    rc, host = draw_call(tgp, dm, y, mk, Rn, eps)
    assert rc == 0
    # NaN in a host series through lgssm.rand: the explicit mask through the C entry, bit for bit
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, np.where(mk, np.nan, y)), Rn)
    via_rand, names = kernels_of(tgp, dm, lambda: tgp.rand(eps, post))
    assert "dk_chunk_draw" in names, names
    served(dm, GEOM)
    assert np.array_equal(np.asarray(via_rand), host)
    # device arrays against host arrays
    cu = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")      # noqa: E731
    post_d = tgp.replace_observation_noise_cov(tgp.posterior(dm, cu(np.where(mk, np.nan, y))), cu(Rn))
    on_device = tgp.rand((cu(eps[0]), cu(eps[1]), eps[2]), post_d)
    assert on_device.is_cuda
    served(dm, GEOM)
    assert rel(on_device.cpu().numpy(), host) <= 1e-12
    # nothing stale is left for the calls that follow on the same handle
    yin = np.where(mk, np.nan, y)
    lp = tgp.logpdf(dm, yin)
    lp_ref = ref.logpdf_missing(model, y, mk)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    _, mean, var = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    bm, bv = ref.bryson_frazier_marginals(model, y, Rn, missing=mk)
    assert np.abs(mean - bm).max() <= 1e-8 * max(1.0, np.abs(bm).max()) and np.abs(var - bv).max() <= 1e-8 * max(1.0, np.abs(bv).max())


def test_a_handle_bound_again_plans_the_right_residency(tgp, monkeypatch):
    """d = 17 -> 49 -> 17 on ONE handle (DP = 32 -> 64 -> 32; tgp_model_set on a handle that already holds a model, as LGSSM.handle() calls it): each
    draw is served at the forced geometry and equal to the restatement"""
    hd = None
    for d in (17, 49, 17):
        model, Rd, y, mk, Rn, eps = make_case(1000 + d, T1, d, 1)
        dm = device(tgp, model, Rd, GEOM)
        if hd is not None:
            with monkeypatch.context() as mp:
                mp.setattr(tgp._lib, "Handle", lambda device=0: hd)
                assert dm.handle() is hd
        hd = dm.handle()
        rc, out = draw_call(tgp, dm, y, mk, Rn, eps)
        assert rc == 0
        assert served(dm, GEOM)["chunks"] == 8
        assert rel(out, restatement(model, y, mk, Rn, eps)) <= REL


# ------------------------------------------------------------------------------------------------ 7. GP level
def test_rand_of_a_posterior_at_new_inputs_of_a_product_kernel(tgp, monkeypatch):
    """rand(rng, posterior(fx, y)(x_new, 1e-6)), ApproxPeriodicKernel() * Matern32Kernel() (d = 28): merge_datasets' joined series -- missing steps, per-step
    transitions and noise, two dt = 0 ties -- on the draw pass; equal to the evaluated route (option 20 = 0) on the same generator seed, and within six
    posterior standard deviations of the posterior mean at every point"""
    from temporalgps_jl_amd import lti_sde as P
    L = tgp._lib
    rng = np.random.default_rng(70)
    x = P.RegularSpacing(0.0, 0.1, 1500)
    xs = x.collect()
    f = P.to_sde(P.GP(P.ApproxPeriodicKernel() * P.Matern32Kernel()), P.HIPStorage())
    fx = f(x, 0.1)
    y = P.rand(np.random.default_rng(71), fx)
    x_new = np.sort(np.concatenate([rng.uniform(0.0, 150.0, size=298), xs[[200, 1200]]]))
    # 1800 joined steps with per-step blocks are too few for the automatic geometry (first guess 64: fewer than 8 chunks of 4 x 64): four chunks of
    # 450 behind warm-ups of 450 joined steps -- 37 time units; the regular series' own first guess is 288 steps of 0.1
    built, real, options = [], P.build_lgssm, {L.OPT_PROFILE: 1, L.OPT_DENSE_CHUNK_STEPS: 450, L.OPT_DENSE_WARMUP: 450, L.OPT_DENSE_WARMUP_BACK: 450}

    def build(*a, **k):
        m = real(*a, **k)
        m.handle_options.update(options)
        built.append(m)
        return m
    monkeypatch.setattr(P, "build_lgssm", build)
    path = P.rand(np.random.default_rng(72), P.posterior(fx, y)(x_new, 1e-6))
    assert len(built) == 1 and built[0].T == 1800 and built[0].dim == 28
    names = set(built[0].handle().profile())
    info = built[0].handle().dense_chunk_info()
    print(info, sorted(names))
    assert "dk_chunk_draw" in names and info["served"] == 1 and info["chunks"] == 4 and info["dist_b"] <= TOL_B, (names, info)
    del built[:]
    options[L.OPT_DENSE_CHUNKED] = 0          # the route of every call before the draw pass: the materialised posterior + the Reverse model's rand
    evaluated = P.rand(np.random.default_rng(72), P.posterior(fx, y)(x_new, 1e-6))
    assert not any(n.startswith("dk_chunk") or n == "dk_fused_draw" for n in built[0].handle().profile()), built[0].handle().profile()
    print("GP level: against the evaluated route", rel(path, evaluated))
    assert path.shape == (300,) and rel(path, evaluated) <= REL
    mean, sd = P.marginals(P.posterior(fx, y)(x_new, 1e-6))
    assert np.all(np.abs(path - mean) <= 6.0 * sd)


# ------------------------------------------------------------------------------------------------ 8. one full-size run
def test_one_full_size_run(tgp):
    """d = 28, T = 1e6, device-resident: served across the chip, finite, the hand-over distance reported"""
    import torch
    from oracle import components as oc
    T, d = 1_000_000, 28
    need = T * (d * d + d + (d + 2) + d + 4) * 8
    free, _ = torch.cuda.mem_get_info(0)
    if need > 0.5 * free:
        pytest.skip("the device has not the memory for the filtering states of 1e6 steps at d = 28")
    model = oc.build_lgssm(("product", ("approx_periodic", 7, 1.0), ("matern32",)), ("regular", 0.0, 0.1, T), 0.1)
    assert len(model["x0m"]) == d
    dm = scalar_dev(tgp, model, None, fused=1)
    g = torch.Generator(device="cuda:0").manual_seed(8)
    yd = torch.randn(T, dtype=torch.float64, device="cuda:0", generator=g)
    yd[torch.rand(T, device="cuda:0", generator=g) < 0.1] = float("nan")
    et = torch.randn((T, d), dtype=torch.float64, device="cuda:0", generator=g)
    ee = torch.randn(T, dtype=torch.float64, device="cuda:0", generator=g)
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, yd), np.array([1e-6]))
    out = tgp.rand((et, ee, np.random.default_rng(8).standard_normal(d)), post)
    info = dm.handle().dense_chunk_info()
    print(info)
    assert info["served"] == 1 and info["chunks"] >= 8 and info["status"] == 0 and info["dist_b"] <= TOL_B, info
    assert out.is_cuda and bool(torch.isfinite(out).all())
