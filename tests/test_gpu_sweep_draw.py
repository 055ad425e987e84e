"""GPU tier (-m gpu): a draw from the posterior on the sweep engine (tgp_posterior_rand_missing -> k_sweep_draw) -- Forward models with scalar
observations and d <= 4 whose gains vary in time -- through ctypes on the C entry (host arrays unless a test says otherwise) against the walk restated
in NumPy on the SAME draws (tests/_sweepdraw.py draw_restated; its own parity with ref.posterior_missing + ref.rand: tests/test_sweep_draw_host.py).

The bar is the project's for draws at small d: 1e-9 * max(1, max |y_ref|).  Every served case asserts the return code, tgp_sweep_info's "served" and the
profiled kernel name, so that a silent fall-back cannot pass; every declined one that y_out kept its sentinel.

Largest error / scale seen on an MI355X, per group: regular grid 1.4e-13; irregular spacing with ties 1.1e-11; every stream at once 1.3e-11; zero draws
against k_sweep's posterior mean 0 (the same arithmetic with zero noise) and <= 1e-8 against the reference's; forced geometries 1.4e-13; the repaired call
4.7e-13; the shifted-eps_t mutation misses by more than three decades.  Largest hand-over distance of a served draw: 4.7e-12 (Matern-1/2 at Wd = 32 behind
ties; the check is 1e-11), otherwise <= 6.5e-13."""
import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref
from tests import _sweepdraw as SD
from tests import _util as U

pytestmark = pytest.mark.gpu

BAR = 1e-9
M12, M32, M52 = ("matern12",), ("matern32",), ("matern52",)
SUM4 = ("sum", M32, ("stretched", 0.7, M32))
GRID = [(M12, 0.1, 0.1), (M32, 0.1, 0.1), (M52, 0.1, 0.1), (SUM4, 0.15, 0.1)]      # d = 1, 2, 3, 4
SENTINEL = -7.0


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _lti(tgp, model):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    return tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])


def _eps(rng, T, d):
    return rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d)


def draw_call(tgp, dm, y, mk, Rn, eps):
    """tgp_posterior_rand_missing through ctypes on host arrays, the kernels it ran: (return code, path, sweep info, kernel names)"""
    hd, L = dm.handle(), tgp._lib
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64)      # noqa: E731
    yy, Rr, et, ee, e0 = c(np.where(mk, 0.0, y) if mk is not None else y), c(np.atleast_1d(Rn)), c(eps[0]), c(eps[1]), c(eps[2])
    mm = None if mk is None else np.ascontiguousarray(mk, dtype=np.uint8)
    out = np.full(yy.shape, SENTINEL)
    flags = L.SHARED_R if Rr.shape[0] == 1 else 0
    hd.set_option(L.OPT_PROFILE, 1)
    hd.profile_reset()
    rc = hd.lib.tgp_posterior_rand_missing(hd.h, L.ptr(yy), L.ptr(mm), L.ptr(Rr), L.ptr(et), L.ptr(ee), L.ptr(e0), flags, L.ptr(out))
    names = set(hd.profile())
    hd.set_option(L.OPT_PROFILE, 0)
    return rc, out, hd.sweep_info(), names


def err(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def served(tgp, dm, y, mk, Rn, eps, want, kernel, bar=BAR, attempts=1):
    rc, out, info, names = draw_call(tgp, dm, y, mk, Rn, eps)
    e = err(out, want) if rc == 0 else float("nan")
    print("rc %d info %s kernels %s error / scale %.3g" % (rc, info, sorted(names), e))
    assert rc == 0 and info["served"] == 1 and info["status"] == 0, (rc, info, dm.handle().lib.tgp_last_error(dm.handle().h))
    assert names == {f"k_sweep_draw<{kernel}>"}, names
    assert info["dist_f"] <= 1e-12 and info["dist_b"] <= 1e-11 and info["Wb"] <= info["C"], info
    assert (info["attempts"] == attempts) if isinstance(attempts, int) else attempts(info["attempts"]), info
    assert e <= bar, e
    return out, info


def declined(tgp, dm, y, mk, Rn, eps):
    rc, out, info, names = draw_call(tgp, dm, y, mk, Rn, eps)
    print("rc %d info %s kernels %s" % (rc, info, sorted(names)))
    assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0 and np.all(out == SENTINEL), (rc, info)
    return info, names


# ------------------------------------------------------------------------------------------------------------ 1. regular grid with missing steps
_grid = {}


def grid_case(i, T):
    if (i, T) not in _grid:
        k, dt, s2 = GRID[i]
        model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=i)
        rng = np.random.default_rng(100 + i)
        mk = rng.random(T) < 0.1
        mk[0] = mk[T - 1] = True
        Rn = np.where(mk, 0.05, 0.0)
        eps = _eps(rng, T, len(model["x0m"]))
        _grid[(i, T)] = (model, y, mk, Rn, eps, SD.draw_restated(model, y, mk, Rn, eps))
    return _grid[(i, T)]


@pytest.mark.parametrize("i", range(len(GRID)))
@pytest.mark.parametrize("T", [2048, 5003])
def test_missing_data_on_a_regular_grid(tgp, i, T):
    """d = 1 .. 4; T = 2048 is the engine's minimum, T = 5003 has a last block of three steps and (C = 64 at d <= 2) more than 62 chunks: a hand-over
    crosses waves"""
    model, y, mk, Rn, eps, want = grid_case(i, T)
    _, info = served(tgp, _lti(tgp, model), y, mk, Rn, eps, want, "lti", attempts=lambda a: a <= 2)
    assert T != 5003 or i > 1 or info["waves"] >= 2, info


# ------------------------------------------------------------------------------------------------------------ 2. irregular spacing, ties
def irregular_case(i, T, with_missing, seed=40):
    k, dt, s2 = GRID[i]
    rng = np.random.default_rng(seed + i)
    t = np.cumsum(rng.uniform(0.5 * dt, 1.5 * dt, T))
    t[400:420] = t[400]
    t[T - 700:T - 695] = t[T - 700]
    model, y, _ = U.gp_case(k, t, s2, seed=i)
    mk = None
    if with_missing:
        mk = rng.random(T) < 0.15
        mk[:4] = True
        mk[T - 3:] = True
    Rn = np.full(T, 0.02) if mk is None else np.where(mk, 0.05, 0.0)
    return k, t, s2, model, y, mk, Rn, _eps(rng, T, len(model["x0m"]))


@pytest.mark.parametrize("i", range(len(GRID)))
@pytest.mark.parametrize("with_missing", [False, True])
def test_irregular_spacing_with_ties(tgp, i, with_missing):
    """closed-form transitions from the gaps (build_lgssm's device-side components), two runs of dt = 0 ties; the plan's first guess of the draw's warm-up
    may be found short behind a tie (Matern-1/2: tests/test_sweep_draw_host.py) and is then repaired"""
    from temporalgps_jl_amd import lti_sde as P
    k, t, s2, model, y, mk, Rn, eps = irregular_case(i, 6000, with_missing)
    want = SD.draw_restated(model, y, mk, Rn, eps)
    dm = P.build_lgssm(P.to_kernel(k), t, s2, device_components=True)
    served(tgp, dm, y, mk, Rn, eps, want, "sde", attempts=lambda a: a <= 3)


# ------------------------------------------------------------------------------------------------------------ 3. every stream at once
@pytest.mark.parametrize("i", [2, 3])
def test_every_stream_at_once(tgp, i):
    """gaps, noise variance and emission offset per step, a mask, new noise per step: k_sweep_draw<d, sde, 3>, the widest variant (d = 3, 4; shipped:
    tests/test_sweep_draw_resources.py)"""
    from temporalgps_jl_amd import lti_sde as P
    k, dt, s2 = GRID[i]
    T = 4500
    rng = np.random.default_rng(60 + i)
    t = np.cumsum(rng.uniform(0.5 * dt, 1.5 * dt, T))
    S = s2 * (0.5 + rng.random(T))
    model, y, _ = U.gp_case(k, t, S, seed=i, mean=("custom", lambda tt: np.cos(0.3 * tt)))
    mk = rng.random(T) < 0.1
    Rn = rng.random(T) * 0.05
    eps = _eps(rng, T, len(model["x0m"]))
    want = SD.draw_restated(model, y, mk, Rn, eps)
    dm = P.build_lgssm(P.to_kernel(k), t, S, mean=P.CustomMean(lambda v: np.cos(0.3 * v)), device_components=True)
    served(tgp, dm, y, mk, Rn, eps, want, "sde", attempts=lambda a: a <= 2)
    # the same through the mirror (rand of an unevaluated posterior reaches the kernel through _posterior_rand_sweep)
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, np.where(mk, np.nan, y)), Rn)
    got, names = U.kernels_of(tgp, dm, lambda: tgp.rand(eps, post))
    assert names == {"k_sweep_draw<sde>"}, names
    assert err(np.asarray(got), want) <= BAR


# ------------------------------------------------------------------------------------------------------------ 4. zero draws, 5. a mutation
@pytest.mark.parametrize("i", [0, 2, 3])
def test_zero_draws_give_the_posterior_mean(tgp, i):
    """with every draw zero the path is the smoother's mean: against logpdf_and_posterior_marginals' mean (k_sweep<lti,posterior>: an oracle the draw code
    shares nothing with) at 1e-8, and against the reference's"""
    model, y, mk, _, _, _ = grid_case(i, 5003)
    T, d = model["T"], len(model["x0m"])
    dm = _lti(tgp, model)
    _, mean, _ = tgp.logpdf_and_posterior_marginals(dm, np.where(mk, np.nan, y), np.array([0.3]))
    z = (np.zeros((T, d)), np.zeros(T), np.zeros(d))
    out, _ = served(tgp, dm, y, mk, 0.3, z, np.asarray(mean), "lti", bar=1e-8)
    pm, _ = ref.marginals(ref.replace_observation_noise_cov(ref.posterior_missing(model, np.where(mk, 0.0, y), mk), np.full(T, 0.3)))
    assert err(out, pm) <= 1e-8


def test_a_shifted_eps_t_misses_the_bar(tgp):
    """the mutation: eps_t moved by one row (the off-by-one the index roles invite) must not pass"""
    model, y, mk, Rn, eps, want = grid_case(2, 2048)
    rc, out, info, _ = draw_call(tgp, _lti(tgp, model), y, mk, Rn, (np.roll(eps[0], 1, axis=0), eps[1], eps[2]))
    assert rc == 0 and info["served"] == 1
    assert err(out, want) > 1e3 * BAR, err(out, want)


# ------------------------------------------------------------------------------------------------------------ 6. forced geometries
# Matern-5/2 at dt = 0.1, sigma^2 = 0.1: the walk's forgetting at a hand-over is 5.7e-3 at Wd = 16 and 0 at Wd = 256 (measured on the NumPy restatement;
# the check is 1e-11); the d = 4 sum: 0.30 and 0.
def _force(tgp, dm, C, W, Wd):
    L = tgp._lib
    dm.handle_options.update({L.OPT_SWEEP_CHUNK: C, L.OPT_SWEEP_WARMUP: W, L.OPT_SWEEP_WARMUP_BACK: Wd})
    return dm


@pytest.mark.parametrize("i", [2, 3])
def test_forced_geometry_that_passes_and_one_that_is_too_short(tgp, i):
    model, y, mk, Rn, eps, want = grid_case(i, 2048)
    _, info = served(tgp, _force(tgp, _lti(tgp, model), 256, 256, 256), y, mk, Rn, eps, want, "lti")
    assert (info["C"], info["W"], info["Wb"]) == (256, 256, 256), info
    info, names = declined(tgp, _force(tgp, _lti(tgp, model), 256, 256, 16), y, mk, Rn, eps)
    assert info["status"] == 2 and info["attempts"] == 1 and info["Wb"] == 16 and info["dist_b"] > 1e-10 and names == {"k_sweep_draw<lti>"}, info


def test_a_last_chunk_of_one_step_and_exactly_two_chunks(tgp):
    k, dt, s2 = GRID[2]
    T = 2049
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=12)
    rng = np.random.default_rng(13)
    mk = rng.random(T) < 0.1
    Rn = np.where(mk, 0.05, 0.0)
    eps = _eps(rng, T, 3)
    want = SD.draw_restated(model, y, mk, Rn, eps)
    _, info = served(tgp, _force(tgp, _lti(tgp, model), 256, 256, 256), y, mk, Rn, eps, want, "lti")      # 8 chunks of 256 and one of ONE step
    assert info["C"] == 256
    _, info = served(tgp, _force(tgp, _lti(tgp, model), 1032, 256, 256), y, mk, Rn, eps, want, "lti")     # C = 8 * 129: exactly two chunks
    assert info["C"] == 1032 and info["waves"] == 1


def test_a_first_guess_that_is_too_short_is_repaired(tgp):
    """automatic geometry: Matern-1/2's first guess (Wd = 32, estimated for a series observed at every step) is short behind ties and missing steps --
    5.9e-10 against the check's 1e-11 in the host simulation of this very series -- and the call repeats with a longer one"""
    from temporalgps_jl_amd import lti_sde as P
    k, t, s2, model, y, mk, Rn, eps = irregular_case(0, 2500, True)
    F, _ = U.kernel_sde(k)
    first = SD.sweepdrawsim_run(model, y, eps, missing=mk, Rnew=Rn, sde=(F, t), num_cu=256)
    print("host simulation of the first guess: status %d, draw distance %.3g" % (first["status"], first["dist_d"]))
    assert first["status"] & 2 and first["dist_d"] > 1e-10      # (the premise, a decade from the check)
    want = SD.draw_restated(model, y, mk, Rn, eps)
    dm = P.build_lgssm(P.to_kernel(k), t, s2, device_components=True)
    _, info = served(tgp, dm, y, mk, Rn, eps, want, "sde", attempts=lambda a: a >= 2)
    # the bound model remembers the warm-up it needed: the next call is served at once
    served(tgp, dm, y, mk, Rn, eps, want, "sde", attempts=1)


# ------------------------------------------------------------------------------------------------------------ 7. the switch
def test_switched_off_the_call_declines_and_writes_nothing(tgp):
    model, y, mk, Rn, eps, want = grid_case(2, 2048)
    dm = _lti(tgp, model)
    dm.handle().set_option(tgp._lib.OPT_SWEEP, 0)
    info, names = declined(tgp, dm, y, mk, Rn, eps)
    assert not names and info["attempts"] == 0, (names, info)
    dm.handle().set_option(tgp._lib.OPT_SWEEP, 1)
    served(tgp, dm, y, mk, Rn, eps, want, "lti")


# ------------------------------------------------------------------------------------------------------------ 8. device arrays, rebinding
def _bind(tgp, hd, model):
    L, pk = tgp._lib, U.pack(model)
    flags = 0
    for bit, s in zip((L.SHARED_A, L.SHARED_a, L.SHARED_Q, L.SHARED_H, L.SHARED_h, L.SHARED_R), (pk["sA"], pk["sa"], pk["sQ"], pk["sH"], pk["sh"], pk["sR"])):
        flags |= bit if s == 0 else 0
    hd.check(hd.lib.tgp_model_set(hd.h, pk["T"], pk["d"], 1, 0, flags, *[L.ptr(pk[n]) for n in ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")]))


def test_device_arrays_rebinding_and_an_unchanged_logpdf(tgp):
    import torch
    L = tgp._lib
    model, y, mk, Rn, eps, want = grid_case(2, 5003)
    dm = _lti(tgp, model)
    hd = dm.handle()
    yin = np.where(mk, np.nan, y)
    lp0 = tgp.logpdf(dm, yin)

    def device_draw(model, y, mk, Rn, eps):
        dev = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda:0")      # noqa: E731
        yd, md, rd, et, ee = dev(np.where(mk, 0.0, y)), dev(mk, torch.uint8), dev(Rn), dev(eps[0]), dev(eps[1])
        out = torch.full((model["T"],), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        rc = hd.lib.tgp_posterior_rand_missing(hd.h, L.ptr(yd), L.ptr(md), L.ptr(rd), L.ptr(et), L.ptr(ee), L.ptr(np.ascontiguousarray(eps[2])),
                                               L.IN_DEVICE | L.OUT_DEVICE, L.ptr(out))
        return rc, out.cpu().numpy()

    rc, out = device_draw(model, y, mk, Rn, eps)
    info = hd.sweep_info()
    assert rc == 0 and info["served"] == 1, (rc, info)
    assert err(out, want) <= BAR
    assert tgp.logpdf(dm, yin) == lp0      # (to the last bit: the draw leaves nothing behind that a later call would reuse)
    # the same handle bound to a model of another d
    model4, y4, mk4, Rn4, eps4, want4 = grid_case(3, 2048)
    _bind(tgp, hd, model4)
    rc, out = device_draw(model4, y4, mk4, Rn4, eps4)
    info = hd.sweep_info()
    assert rc == 0 and info["served"] == 1, (rc, info)
    assert err(out, want4) <= BAR
    _bind(tgp, hd, model)
    rc, out = device_draw(model, y, mk, Rn, eps)
    assert rc == 0 and err(out, want) <= BAR
    assert tgp.logpdf(dm, yin) == lp0


# ------------------------------------------------------------------------------------------------------------ 9. GP level
def test_rand_of_a_posterior_gp_at_new_inputs(tgp):
    """rand(rng, posterior(fx, y)(x_new)) with x_new interleaved with and beyond the training inputs (n_train + n_new = 2600): through lti_sde's
    _rand_merged and lgssm.rand on k_sweep_draw<sde>; against the oracle's posterior_rand on the same draws at its 1e-7, and against the evaluated route
    (TGP_OPT_SWEEP = 0: tgp_posterior + tgp_rand) at 1e-8"""
    from temporalgps_jl_amd import lti_sde as P
    rng = np.random.default_rng(5)
    spec = ("scaled", 0.8, ("stretched", 1.7, M52))
    ntr, npr, s2 = 1800, 800, 0.1
    xtr = np.sort(rng.uniform(0.0, 180.0, ntr))
    xpr = np.sort(np.concatenate([rng.uniform(0.0, 180.0, npr - 50), rng.uniform(180.0, 184.0, 50)]))
    _, ytr, _ = U.gp_case(spec, xtr, s2, seed=9)
    f = P.to_sde(P.GP(P.to_kernel(spec)))
    fpost = P.posterior(f(xtr, s2), ytr)
    seen = []
    from temporalgps_jl_amd import lgssm as Lg
    inner = Lg._posterior_rand_sweep

    def spy(*a):
        r = inner(*a)
        seen.append(r is not None)
        return r

    Lg._posterior_rand_sweep = spy
    try:
        ys = P.rand(np.random.default_rng(11), fpost(xpr, 0.2))
    finally:
        Lg._posterior_rand_sweep = inner
    assert seen == [True], seen
    g = np.random.default_rng(11)
    T, d = ntr + npr, 3
    eps_t, eps_e = g.standard_normal((T, d)), g.standard_normal(T)
    eps_0 = g.standard_normal(d)
    np.testing.assert_allclose(ys, oc.posterior_rand(spec, xtr, s2, ytr, xpr, 0.2, eps_t, eps_e, eps_0), rtol=1e-7, atol=1e-7)
    # the same call with TGP_OPT_SWEEP = 0 on the model it builds: the library declines, the evaluated route draws
    fx = fpost(xpr, 0.2)
    build = type(fx)._posterior_model
    declined_ = []

    def switched_off(self, *a):
        m = build(self, *a)
        m.handle().set_option(tgp._lib.OPT_SWEEP, 0)
        return m

    def spy0(*a):
        r = inner(*a)
        declined_.append(r is None)
        return r

    type(fx)._posterior_model = switched_off
    Lg._posterior_rand_sweep = spy0
    try:
        ys0 = P.rand(np.random.default_rng(11), fx)
    finally:
        type(fx)._posterior_model = build
        Lg._posterior_rand_sweep = inner
    assert declined_ == [True], declined_
    assert np.abs(ys - ys0).max() <= 1e-8 * max(1.0, np.abs(ys0).max())
