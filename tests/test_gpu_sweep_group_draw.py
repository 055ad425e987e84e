"""GPU tier (-m gpu): a draw from the posterior on the group sweep (tgp_posterior_rand_group -> k_sweep_group_draw) -- Forward LTI models with
scalar observations and 5 <= d <= 8, with missing steps, a noise variance or an emission offset per step -- through ctypes on the C entry (host arrays unless
a test says otherwise) and through the mirrors, against the walk restated in NumPy on the SAME draws (tests/_sweepdraw.py draw_restated; its parity with
ref.rand on ref.posterior_missing at these models: tests/test_sweep_group_draw_host.py, 2e-13 .. 2.4e-12).

The bar is the project's for draws at small d: largest error <= 1e-9 * max(1, max |y*|).  Nothing slowly mixing is among the cases (the reference
cannot arbitrate there).  Every served case asserts the return code, tgp_sweep_info's "served" and the profiled kernel name, so that a silent fall-back
cannot pass; every declined one that y_out kept its sentinel."""
import functools

import numpy as np
import pytest

from oracle import lgssm_ref as ref
from tests import _sweep_group as SG
from tests import _sweep_group_draw as GD
from tests import _sweepdraw as SD
from tests import _util as U

pytestmark = pytest.mark.gpu

BAR = 1e-9
SENTINEL = -7.0
KERNEL = "k_sweep_group_draw<lti>"
C_EDGE, T_EDGE = 64, 4100      # 65 chunks of 64 steps: the last one 4 steps long, the last wave (6 chunks per wave) partly filled
DT_EDGE = 0.5                  # (a grid on which the filter and the walk forget within a chunk of 64 steps)


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _lti(tgp, model, ordering=None, C=0, W=0, Wd=0, **options):
    tr = tgp.GaussMarkovModel(ordering or tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    L = tgp._lib
    dm.handle_options.update({L.OPT_SWEEP_CHUNK: C, L.OPT_SWEEP_WARMUP: W, L.OPT_SWEEP_WARMUP_BACK: Wd})
    dm.handle_options.update({getattr(L, k): v for k, v in options.items()})
    return dm


def draw_call(tgp, dm, y, mk, Rn, eps, device=False, entry="tgp_posterior_rand_group"):
    """the C entry through ctypes, y_out pre-filled with a sentinel: (return code, y_out, sweep info, kernel names).  device: every stream but eps_0 is a
    torch tensor on the device, y_out too."""
    hd, L = dm.handle(), tgp._lib
    c = lambda x: np.ascontiguousarray(x, dtype=np.float64)      # noqa: E731
    yy, Rr, et, ee, e0 = c(np.where(mk, 0.0, y) if mk is not None else y), c(np.atleast_1d(Rn)), c(eps[0]), c(eps[1]), c(eps[2])
    mm = None if mk is None else np.ascontiguousarray(mk, dtype=np.uint8)
    flags = L.SHARED_R if Rr.shape[0] == 1 else 0
    if device:
        import torch
        yy, Rr, et, ee = (torch.as_tensor(v, device="cuda:0") for v in (yy, Rr, et, ee))
        mm = None if mm is None else torch.as_tensor(mm, device="cuda:0")
        out = torch.full((yy.shape[0],), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        flags |= L.IN_DEVICE | L.OUT_DEVICE
    else:
        out = np.full(yy.shape, SENTINEL)
    hd.set_option(L.OPT_PROFILE, 1)
    hd.profile_reset()
    rc = getattr(hd.lib, entry)(hd.h, L.ptr(yy), L.ptr(mm), L.ptr(Rr), L.ptr(et), L.ptr(ee), L.ptr(e0), flags, L.ptr(out))
    names = set(hd.profile())
    hd.set_option(L.OPT_PROFILE, 0)
    return rc, (out.cpu().numpy() if device else out), hd.sweep_info(), names


def served(tgp, dm, y, mk, Rn, eps, want, bar=BAR, attempts=1, device=False):
    rc, out, info, names = draw_call(tgp, dm, y, mk, Rn, eps, device)
    e = GD.err(out, want) if rc == 0 else float("nan")
    print("rc %d info %s kernels %s error / scale %.3g" % (rc, info, sorted(names), e))
    assert rc == 0 and info["served"] == 1 and info["status"] == 0, (rc, info, dm.handle().lib.tgp_last_error(dm.handle().h))
    assert names == {KERNEL}, names
    assert info["dist_f"] <= 1e-12 and info["dist_b"] <= 1e-11 and info["Wb"] <= info["C"], info
    assert (info["attempts"] == attempts) if isinstance(attempts, int) else attempts(info["attempts"]), info
    assert e <= bar, e
    return out, info


def declined(tgp, dm, y, mk, Rn, eps, device=False):
    rc, out, info, names = draw_call(tgp, dm, y, mk, Rn, eps, device)
    print("rc %d info %s kernels %s" % (rc, info, sorted(names)))
    assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0 and np.all(out == SENTINEL), (rc, info)
    return info, names


# ------------------------------------------------------------------------------------------------------------ 1. every d and every XS
@functools.lru_cache(maxsize=None)
def grid_case(d, xs, T):
    model, y, mk, Rn, eps = GD.case(d, T, seed=1000 + 10 * d + xs, xs=xs)
    return model, y, mk, Rn, eps, SD.draw_restated(model, y, mk, Rn, eps)


@pytest.mark.parametrize("d", [5, 6, 7, 8])
@pytest.mark.parametrize("xs", [0, 1, 2, 3])
@pytest.mark.parametrize("T", [2048, 5003])
def test_mask_noise_and_offset_per_step(tgp, d, xs, T):
    """k_sweep_group_draw<d, xs> in the plan's own geometry: 10 % missing with the first and the last step among them, new noise per step; T = 2048 is the
    engine's minimum, T = 5003 no multiple of 8 (a last row of three steps)"""
    model, y, mk, Rn, eps, want = grid_case(d, xs, T)
    assert len(model["x0m"]) == d and np.atleast_1d(model["R"]).shape[0] == (T if xs & 1 else 1) and np.atleast_1d(model["h"]).shape[0] == (T if xs & 2 else 1)
    served(tgp, _lti(tgp, model), y, mk, Rn, eps, want, attempts=lambda a: a <= 2)


# ------------------------------------------------------------------------------------------------------------ 2. wave seams, a short last chunk
def edge_mask(T, seed):
    mk = np.random.default_rng(seed).random(T) < 0.1
    mk[630:710] = True         # chunk [640, 704) whole, straddling both its edges
    mk[1030:1036] = True       # the checkpoint-block edge at 1032 (B = 8 and B = 4)
    mk[1276:1284] = True       # a chunk edge (1280) inside a run
    mk[0] = True
    mk[T - 3:] = True
    return mk


@functools.lru_cache(maxsize=None)
def edge_case(d, xs=0):
    model, y, _, Rn, eps = GD.case(d, T_EDGE, seed=2000 + 10 * d + xs, xs=xs, dt=DT_EDGE)
    mk = edge_mask(T_EDGE, 30 + d)
    return model, y, mk, Rn, eps, SD.draw_restated(model, y, mk, Rn, eps)


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_chunks_of_64_steps_over_several_waves(tgp, d):
    """TGP_OPT_SWEEP_CHUNK = 64 at T = 4100: 11 waves, every sixth hand-over crosses a wave seam (group 7 of a wave repeats the warm-up of the next wave's
    group 1), the last chunk is 4 steps long, the last wave partly filled; a missing run over a whole chunk and both its edges"""
    model, y, mk, Rn, eps, want = edge_case(d)
    _, info = served(tgp, _lti(tgp, model, C=C_EDGE), y, mk, Rn, eps, want)
    assert info["C"] == C_EDGE and info["waves"] == 11, info


# ------------------------------------------------------------------------------------------------------------ 3. zero draws, 4. a mutation
@pytest.mark.parametrize("d", [5, 8])
def test_zero_draws_give_the_posterior_mean(tgp, d):
    """with every draw zero the path is the smoother's mean: against the oracle's posterior mean at 1e-8"""
    model, y, mk, _, _, _ = grid_case(d, 0, 5003)
    T = model["T"]
    z = (np.zeros((T, d)), np.zeros(T), np.zeros(d))
    pm, _ = ref.marginals(ref.replace_observation_noise_cov(ref.posterior_missing(model, np.where(mk, 0.0, y), mk), np.full(T, 0.3)))
    served(tgp, _lti(tgp, model), y, mk, 0.3, z, pm, bar=1e-8, attempts=lambda a: a <= 2)


def test_a_shifted_eps_t_misses_the_bar(tgp):
    """the mutation: eps_t moved by one row (the off-by-one the index roles invite) must not pass"""
    model, y, mk, Rn, eps, want = grid_case(5, 0, 2048)
    rc, out, info, _ = draw_call(tgp, _lti(tgp, model), y, mk, Rn, (np.roll(eps[0], 1, axis=0), eps[1], eps[2]))
    assert rc == 0 and info["served"] == 1
    assert GD.err(out, want) > 1e3 * BAR, GD.err(out, want)


# ------------------------------------------------------------------------------------------------------------ 5. forced geometry, 6. repair
def test_a_forced_draw_warm_up_that_is_too_short_is_reported_not_repaired(tgp):
    """TGP_OPT_SWEEP_WARMUP_BACK = 8 forces the draw's warm-up: status bit 2, one launch, y_out untouched on the host and on the device"""
    model, y, mk, Rn, eps, _ = edge_case(5)
    for device in (False, True):
        info, names = declined(tgp, _lti(tgp, model, C=C_EDGE, Wd=8), y, mk, Rn, eps, device=device)
        assert info["attempts"] == 1 and names == {KERNEL}, (info, names)
        assert info["status"] & 2 and info["Wb"] == 8 and info["dist_b"] > 1e-10, info
    # ... and through the mirror: Unsupported
    dm = _lti(tgp, model, C=C_EDGE, Wd=8)
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, np.where(mk, np.nan, y)), Rn)
    with pytest.raises(tgp._lib.Unsupported):
        tgp.lgssm.posterior_rand_group(post, *eps)
    with pytest.raises(tgp._lib.Unsupported):
        tgp.rand(eps, post, method="sweep")


def test_a_long_gap_behind_a_chunk_edge_is_repaired_and_remembered(tgp):
    """default options, d = 5, T = 4096.  A run of missing steps as long as the first guess of Wd right behind a chunk edge does NOT make that guess short
    at these models: the plan's estimate is close to the prior's own forgetting rate, which is what the walk has inside a gap (NumPy restatement in the
    plan's geometry: draw distance 6.7e-13 with the gap, 4.0e-14 without) -- that call is served at once.  What is short is the guess behind a long stretch
    observed only at every 16th step (chunks 2 .. 5; restated: 1.06e-10 against the check's 1e-11, the forward distance 2.4e-12 against 1e-12): the call
    repeats with doubled warm-ups in a longer chunk, and the bound model remembers them."""
    d, T = 5, 4096
    model, y, mk0, Rn, eps = GD.case(d, T, seed=77)
    rc, _, first, _ = draw_call(tgp, _lti(tgp, model), y, mk0, Rn, eps)
    assert rc == 0 and first["attempts"] == 1, first      # the geometry of the first guess: the same model and length on a fresh handle
    C, W, Wd = first["C"], first["W"], first["Wb"]
    B = 8
    mk = mk0.copy()
    mk[3 * C:3 * C + Wd] = True
    served(tgp, _lti(tgp, model), y, mk, Rn, eps, SD.draw_restated(model, y, mk, Rn, eps), attempts=lambda a: a <= 2)
    mk = mk0.copy()
    mk[2 * C:6 * C] = True
    mk[2 * C:6 * C:16] = False
    _, dist_f, dist_d = GD.chunked_draw(model, y, mk, Rn, eps, C, W, Wd, B)
    print("restated in the first guess's geometry (C %d W %d Wd %d): distances %.3g / %.3g" % (C, W, Wd, dist_f, dist_d))
    assert dist_d > 5e-11      # (the premise: five times the check)
    want = SD.draw_restated(model, y, mk, Rn, eps)
    dm = _lti(tgp, model)
    _, info = served(tgp, dm, y, mk, Rn, eps, want, attempts=lambda a: a >= 2)
    assert info["Wb"] > Wd and info["state"] == 1, info
    _, again = served(tgp, dm, y, mk, Rn, eps, want, attempts=1)
    assert (again["C"], again["W"], again["Wb"]) == (info["C"], info["W"], info["Wb"]), (info, again)


# ------------------------------------------------------------------------------------------------------------ 7. / 8. declines
def test_declines_without_a_launch(tgp):
    from temporalgps_jl_amd import lti_sde as P
    rng = np.random.default_rng(2)
    k5, _, s2 = SG.KERNELS[5]

    def nothing_ran(dm, y):
        T, d = dm.T, dm.dim
        info, names = declined(tgp, dm, y, None, 0.1, GD.eps_of(rng, T, d))
        assert not names and info["attempts"] == 0, (names, info)

    model, y, _ = U.gp_case(("sum", SG.M52, ("matern12",)), ("regular", 0.0, 0.1, 2100), s2, seed=1)      # d = 4
    assert len(model["x0m"]) == 4
    nothing_ran(_lti(tgp, model), y)
    model, y, _ = U.gp_case(("sum", SG.M52, ("stretched", 0.7, SG.M52), ("stretched", 0.5, SG.M52)), ("regular", 0.0, 0.1, 2100), s2, seed=1)      # d = 9
    assert len(model["x0m"]) == 9
    nothing_ran(_lti(tgp, model), y)
    model, y, _ = U.gp_case(k5, ("regular", 0.0, 0.1, 2047), s2, seed=1)                              # T = 2047
    nothing_ran(_lti(tgp, model), y)
    t = np.cumsum(rng.uniform(0.05, 0.15, 2100))                                                      # an SDE-described model
    sde = P.build_lgssm(P.to_kernel(k5), t, s2, device_components=True)
    assert sde.dim == 5 and isinstance(sde.transitions, tgp.lgssm.SDETransitions)
    nothing_ran(sde, rng.standard_normal(2100))
    model, y, mk, Rn, eps, want = grid_case(5, 0, 2048)
    nothing_ran(_lti(tgp, model, OPT_SWEEP=0), y)                                                     # TGP_OPT_SWEEP = 0
    nothing_ran(_lti(tgp, model, OPT_CHUNK=16), y)                                                    # an explicit request for the general engine
    for sweep in (1, 2):                                                                              # ... and the same model without them is served,
        served(tgp, _lti(tgp, model, OPT_SWEEP=sweep), y, mk, Rn, eps, want, attempts=lambda a: a <= 2)      # under the default routing as well


@pytest.mark.parametrize("bad,bits", [("negR", 4), ("inf", 8)])
def test_declines_after_a_launch(tgp, bad, bits):
    """a negative noise variance inside a chunk: a pivot that is not positive (bit 4); an infinite observation (bit 8): status reports of the engine, the
    call is declined and y_out is untouched, on the host and on the device"""
    model, y, mk, Rn, eps, _ = edge_case(5, 1)
    mk = mk.copy()
    mk[2148] = False
    if bad == "negR":
        model = dict(model, R=np.where(np.arange(T_EDGE) == 2148, -50.0, model["R"]))
    else:
        y = y.copy()
        y[2148] = np.inf
    for device in (False, True):
        info, names = declined(tgp, _lti(tgp, model, C=C_EDGE), y, mk, Rn, eps, device=device)
        assert info["status"] & bits and info["attempts"] == 1 and names == {KERNEL}, info


# ------------------------------------------------------------------------------------------------------------ 9. bit identity, 10. kernel names
def test_two_calls_and_host_and_device_inputs_are_bit_identical(tgp):
    model, y, mk, Rn, eps, want = edge_case(6, 3)
    dm = _lti(tgp, model, C=C_EDGE)
    o1, _ = served(tgp, dm, y, mk, Rn, eps, want)
    o2, _ = served(tgp, dm, y, mk, Rn, eps, want)
    o3, _ = served(tgp, dm, y, mk, Rn, eps, want, device=True)
    assert np.array_equal(o1, o2) and np.array_equal(o1, o3)


def test_the_mirrors_run_the_draw_kernel_and_no_other(tgp):
    """lgssm.posterior_rand_group and rand(method="sweep") on host and on device arrays: k_sweep_group_draw alone in the profile"""
    import torch
    model, y, mk, Rn, eps, want = grid_case(7, 3, 2048)
    dm = _lti(tgp, model)
    yin = np.where(mk, np.nan, y)
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, yin), Rn)
    got, names = U.kernels_of(tgp, dm, lambda: tgp.lgssm.posterior_rand_group(post, *eps))
    assert names == {KERNEL} and GD.err(np.asarray(got), want) <= BAR, names
    got, names = U.kernels_of(tgp, dm, lambda: tgp.rand(eps, post, method="sweep"))
    assert names == {KERNEL} and GD.err(np.asarray(got), want) <= BAR, names
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0")      # noqa: E731
    postd = tgp.replace_observation_noise_cov(tgp.posterior(dm, dev(yin)), dev(Rn))
    got, names = U.kernels_of(tgp, dm, lambda: tgp.rand((dev(eps[0]), dev(eps[1]), eps[2]), postd, method="sweep"))
    assert names == {KERNEL} and torch.is_tensor(got) and GD.err(got.cpu().numpy(), want) <= BAR, names
    # the lane sweep's entry point keeps declining these dimensions with no attempt made
    rc, out, info, names = draw_call(tgp, dm, y, mk, Rn, eps, entry="tgp_posterior_rand_missing")
    assert rc == tgp._lib.EUNSUPPORTED and not names and info["attempts"] == 0 and np.all(out == SENTINEL), (rc, info, names)


# ------------------------------------------------------------------------------------------------------------ 11. GP level
@pytest.mark.parametrize("d", [5, 8])
def test_gp_level_rand_at_the_training_inputs_with_nans(tgp, d):
    """lti_sde.rand(rng, posterior(fx, y)(fx.x), method="sweep") on a regular grid with NaNs in y: the T-step posterior with its noise replaced on
    k_sweep_group_draw, against the walk restated on the draws the mirror takes from the same rng (eps_t, eps_e, eps_0 in lgssm.rand's order)"""
    from temporalgps_jl_amd import lti_sde as P
    from temporalgps_jl_amd import lgssm as Lg
    T, s2, s2_new = 3000, 0.1, 0.2
    spec = SG.KERNELS[d][0]
    x = P.RegularSpacing(0.0, 0.1, T)
    model, y, _ = U.gp_case(spec, ("regular", 0.0, 0.1, T), s2, seed=90 + d)
    rng = np.random.default_rng(91 + d)
    mk = rng.random(T) < 0.1
    yin = np.where(mk, np.nan, y)
    f = P.to_sde(P.GP(P.to_kernel(spec)))
    fx = P.posterior(f(x, s2), yin)(x, s2_new)
    seen = []
    inner = Lg.posterior_rand_group

    def spy(post, *a):
        hd = post._prior.handle()
        hd.set_option(tgp._lib.OPT_PROFILE, 1)
        hd.profile_reset()
        r = inner(post, *a)
        seen.append((set(hd.profile()), hd.sweep_info()["served"]))
        hd.set_option(tgp._lib.OPT_PROFILE, 0)
        return r

    Lg.posterior_rand_group = spy
    try:
        ys = P.rand(np.random.default_rng(11), fx, method="sweep")
    finally:
        Lg.posterior_rand_group = inner
    assert seen == [({KERNEL}, 1)], seen
    g = np.random.default_rng(11)
    eps = (g.standard_normal((T, d)), g.standard_normal(T), g.standard_normal(d))
    want = SD.draw_restated(model, y, mk, s2_new, eps)
    e = GD.err(np.asarray(ys), want)
    print("error / scale %.3g" % e)
    assert e <= BAR, e
    # other inputs under method="sweep"
    with pytest.raises(NotImplementedError):
        P.rand(np.random.default_rng(11), P.posterior(f(x, s2), y)(x, s2_new), method="sweep")                            # no NaN in y
    with pytest.raises(NotImplementedError):
        P.rand(np.random.default_rng(11), P.posterior(f(x, s2), yin)(P.RegularSpacing(0.05, 0.1, T), s2_new), method="sweep")      # other inputs
    with pytest.raises(NotImplementedError):
        P.rand(np.random.default_rng(11), f(x, s2), method="sweep")                                                       # a prior


# ------------------------------------------------------------------------------------------------------------ 12. the default policy
def test_the_default_rand_runs_what_it_ran_before(tgp):
    """lgssm.rand(eps, post) with method=None at d = 5: today's chain, untouched -- the one-launch smoother does not take a series with NaNs, the lane sweep
    and the dense engine do not take d = 5, so the posterior is evaluated on the general engine and tgp_rand draws from the Reverse model: no sweep-group
    kernel among the kernels of the call, and the values are the restated walk's (the evaluated route's own parity, 1e-8)"""
    model, y, mk, Rn, eps, want = grid_case(5, 0, 2048)
    dm = _lti(tgp, model)
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, np.where(mk, np.nan, y)), Rn)
    got, names = U.kernels_of(tgp, dm, lambda: tgp.rand(eps, post))
    print(sorted(names))
    # (the kernels of tgp_posterior on the prior's handle, as before this entry point existed; tgp_rand runs on the Reverse model's own handle)
    assert names == {"k_reduce_filter<lti>", "k_group_scan_apply<filter,top>", "k_apply_filter<lti,materialise>", "k_finalize"}, names
    assert dm.handle().sweep_info()["served"] == 0
    assert GD.err(np.asarray(got), want) <= 1e-8
