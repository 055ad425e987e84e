"""GPU tier (-m gpu): a draw from the posterior of an SDE-described model on the group sweep (tgp_posterior_rand_group_sde -> k_sweep_group_draw<sde>,
DESIGN 4.15) -- irregular inputs at d = 5 .. 8 with tied stamps, a long gap, missing steps, noise / offset per step -- through the C entry and the mirrors,
against the walk restated in NumPy on the oracle's per-step model with the SAME draws (tests/_sweepdraw.py draw_restated), at the project's bar for draws:
largest error <= 1e-9 * max(1, max |y*|).  A served case asserts return code, "served", both hand-over distances and the profiled kernel name."""
import functools

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref
from tests import _sweep_group as SG
from tests import _sweep_group_draw as GD
from tests import _sweepdraw as SD
from tests import _util as U
from tests.test_gpu_sweep_group_draw import BAR, SENTINEL, _lti, draw_call, edge_mask, tgp      # noqa: F401  (BAR = 1e-9; tgp: the module's fixture)

pytestmark = pytest.mark.gpu

ENTRY, KERNEL = "tgp_posterior_rand_group_sde", "k_sweep_group_draw<sde>"
C_EDGE, T_EDGE, DT_EDGE = 64, 4100, 0.5      # 65 chunks of 64 steps, 6 per wave: 11 waves, the last chunk 4 steps; a gap the walk forgets 64 of


def bind(tgp, k, t, S, mean=None, **options):
    from temporalgps_jl_amd import lti_sde as P
    dm = P.build_lgssm(P.to_kernel(k), t, S, mean=mean, device_components=True)
    assert isinstance(dm.transitions, tgp.lgssm.SDETransitions) == (dm.dim <= 8)      # (d = 9: build_lgssm evaluates the transitions on the host)
    for name, v in options.items():
        dm.handle().set_option(getattr(tgp._lib, name), v)
    return dm


def served(tgp, dm, y, mk, Rn, eps, want, bar=BAR, attempts=lambda a: a <= 2, device=False):
    rc, out, info, names = draw_call(tgp, dm, y, mk, Rn, eps, device, entry=ENTRY)
    e = GD.err(out, want) if rc == 0 else float("nan")
    print("rc %d info %s kernels %s error / scale %.3g" % (rc, info, sorted(names), e))
    assert rc == 0 and info["served"] == 1 and info["status"] == 0, (rc, info, dm.handle().lib.tgp_last_error(dm.handle().h))
    assert names == {KERNEL}, names
    assert info["dist_f"] <= 1e-12 and info["dist_b"] <= 1e-11 and info["Wb"] <= info["C"], info
    assert attempts(info["attempts"]), info
    assert e <= bar, e
    return out, info


def declined(tgp, dm, y, mk, Rn, eps, device=False):
    rc, out, info, names = draw_call(tgp, dm, y, mk, Rn, eps, device, entry=ENTRY)
    assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0 and np.all(out == SENTINEL), (rc, info)
    return info, names


@functools.lru_cache(maxsize=None)
def case(d, xs, T, dt=None, edge=False):
    """gaps U(0.5, 1.5) dt, two tie runs, 12 % missing with missing ends, new noise per step, one gap of 50 typical gaps.  edge (C = 64): tie runs across a chunk
    edge (64), a wave seam (384) and a checkpoint-block edge (1032), the LTI file's mask.  Returns (bind arguments, model, y, missing, Rnew, eps, restated walk)."""
    from temporalgps_jl_amd import lti_sde as P
    k, dt0, s2 = SG.KERNELS[d]
    dt = dt0 if dt is None else dt
    rng = np.random.default_rng(3000 + 100 * d + 10 * xs + T % 7)
    gaps = rng.uniform(0.5 * dt, 1.5 * dt, T)
    if edge:
        gaps[62:67] = gaps[382:387] = gaps[1030:1035] = 0.0
        mk = edge_mask(T, 30 + d)
    else:
        gaps[100:104] = gaps[T - 2:] = 0.0
        gaps[T // 2] = 50.0 * dt
        mk = rng.random(T) < 0.12
        mk[:3] = mk[T - 3:] = True
    t = np.cumsum(gaps)
    S = s2 * (0.5 + rng.random(T)) if xs & 1 else s2
    fn = lambda v: np.sin(0.3 * np.asarray(v))      # noqa: E731
    model, y, _ = U.gp_case(k, t, S, seed=d + xs, mean=("custom", fn) if xs & 2 else None)
    Rn = np.where(mk, 0.05, 0.02 * rng.random(T))
    eps = GD.eps_of(rng, T, d)
    return (k, t, S, P.CustomMean(fn) if xs & 2 else None), model, y, mk, Rn, eps, SD.draw_restated(model, y, mk, Rn, eps)


@pytest.mark.parametrize("d,xs,T", [(d, xs, 2048) for d in (5, 6, 7, 8) for xs in range(4)] + [(d, 3, 5003) for d in (5, 6, 7, 8)])
def test_gaps_ties_mask_noise_and_offset_per_step(tgp, d, xs, T):
    """k_sweep_group_draw_sde<d, xs> in the plan's own geometry; T = 2048 is the engine's minimum, T = 5003 has a last row of three steps"""
    b, _, y, mk, Rn, eps, want = case(d, xs, T)
    served(tgp, bind(tgp, *b), y, mk, Rn, eps, want)


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_chunks_of_64_steps_over_several_waves(tgp, d):
    """TGP_OPT_SWEEP_CHUNK = 64 at T = 4100: the gap a step takes at a row's, block's, chunk's and wave's last step is the first gap behind it"""
    b, _, y, mk, Rn, eps, want = case(d, 0, T_EDGE, DT_EDGE, True)
    _, info = served(tgp, bind(tgp, *b, OPT_SWEEP_CHUNK=C_EDGE), y, mk, Rn, eps, want, attempts=lambda a: a == 1)
    assert info["C"] == C_EDGE and info["waves"] == 11, info


@pytest.mark.parametrize("d", [5, 8])
def test_zero_draws_give_the_posterior_mean(tgp, d):
    """with every draw zero the path is the smoother's mean: against the oracle's posterior mean (independent of the restated walk) at 1e-8"""
    T = 5003
    b, model, y, mk, _, _, _ = case(d, 3, T)
    pm, _ = ref.marginals(ref.replace_observation_noise_cov(ref.posterior_missing(model, np.where(mk, 0.0, y), mk), np.full(T, 0.3)))
    served(tgp, bind(tgp, *b), y, mk, 0.3, (np.zeros((T, d)), np.zeros(T), np.zeros(d)), pm, bar=1e-8)


def test_a_forced_draw_warm_up_that_is_too_short_is_reported_not_repaired(tgp):
    """TGP_OPT_SWEEP_WARMUP_BACK = 8 forces the draw's warm-up: status bit 2, one launch, y_out untouched on the host and on the device"""
    b, _, y, mk, Rn, eps, _ = case(5, 0, T_EDGE, DT_EDGE, True)
    for device in (False, True):
        info, names = declined(tgp, bind(tgp, *b, OPT_SWEEP_CHUNK=C_EDGE, OPT_SWEEP_WARMUP_BACK=8), y, mk, Rn, eps, device=device)
        assert info["attempts"] == 1 and names == {KERNEL}, (info, names)
        assert info["status"] & 2 and info["Wb"] == 8 and info["dist_b"] > 1e-10, info
    post = tgp.replace_observation_noise_cov(tgp.posterior(bind(tgp, *b, OPT_SWEEP_CHUNK=C_EDGE, OPT_SWEEP_WARMUP_BACK=8), np.where(mk, np.nan, y)), Rn)
    for mirror in (lambda: tgp.lgssm.posterior_rand_group_sde(post, *eps), lambda: tgp.rand(eps, post, method="sweep")):
        with pytest.raises(tgp._lib.Unsupported):
            mirror()


def test_declines_without_a_launch(tgp):
    rng = np.random.default_rng(2)
    k5, dt, s2 = SG.KERNELS[5]

    def nothing_ran(dm, T):
        info, names = declined(tgp, dm, rng.standard_normal(T), None, 0.1, GD.eps_of(rng, T, dm.dim))
        assert not names and info["attempts"] == 0, (names, info)

    times = lambda T: np.cumsum(rng.uniform(0.5 * dt, 1.5 * dt, T))      # noqa: E731
    model, _, _ = U.gp_case(k5, ("regular", 0.0, dt, 2100), s2, seed=1)                                        # a model in LTI form
    nothing_ran(_lti(tgp, model), 2100)
    for k, d in ((("sum", SG.M52, ("matern12",)), 4), (("sum", SG.M52, SG.M52, SG.M52), 9)):                    # d = 4, d = 9
        assert (dm := bind(tgp, k, times(2100), s2)).dim == d
        nothing_ran(dm, 2100)
    nothing_ran(bind(tgp, k5, times(2047), s2), 2047)                                                          # T = 2047
    b, _, y, mk, Rn, eps, want = case(5, 0, 2048)
    nothing_ran(bind(tgp, *b, OPT_SWEEP=0), 2048)                                                              # TGP_OPT_SWEEP = 0
    nothing_ran(bind(tgp, *b, OPT_CHUNK=16), 2048)                                                             # a request for the general engine
    for sweep in (1, 2):                                                                                       # ... and the same model without them
        served(tgp, bind(tgp, *b, OPT_SWEEP=sweep), y, mk, Rn, eps, want)


def test_a_replaced_prior_is_served(tgp):
    """tgp_model_set_x0 with x0P != Pinf: the warm-ups start from Pinf of the closed-form record, step 0 from the replaced prior"""
    b, model, _, mk, Rn, eps, _ = case(6, 1, 2048)
    d, B = 6, np.random.default_rng(4).standard_normal((6, 6))
    x0m, x0P = model["x0m"] + np.linspace(1.0, -2.0, d), 0.3 * model["x0P"] + 0.05 * B @ B.T
    m2 = dict(model, x0m=x0m, x0P=x0P)
    y = ref.rand(m2, *GD.eps_of(np.random.default_rng(5), 2048, d))
    hd = (dm := bind(tgp, *b)).handle()
    hd.check(hd.lib.tgp_model_set_x0(hd.h, tgp._lib.ptr(np.ascontiguousarray(x0m)), tgp._lib.ptr(np.ascontiguousarray(x0P.T))))
    served(tgp, dm, y, mk, Rn, eps, SD.draw_restated(m2, y, mk, Rn, eps))


def test_two_calls_and_host_and_device_inputs_are_bit_identical(tgp):
    b, _, y, mk, Rn, eps, want = case(6, 3, 2048)
    dm = bind(tgp, *b)
    o1, _ = served(tgp, dm, y, mk, Rn, eps, want)
    o2, _ = served(tgp, dm, y, mk, Rn, eps, want, attempts=lambda a: a == 1)
    o3, _ = served(tgp, dm, y, mk, Rn, eps, want, attempts=lambda a: a == 1, device=True)
    assert np.array_equal(o1, o2) and np.array_equal(o1, o3)


def test_the_mirrors_run_the_draw_kernel_and_no_other(tgp):
    import torch
    b, _, y, mk, Rn, eps, want = case(7, 3, 2048)
    dm = bind(tgp, *b)
    yin = np.where(mk, np.nan, y)
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, yin), Rn)
    for mirror in (lambda: tgp.lgssm.posterior_rand_group_sde(post, *eps), lambda: tgp.rand(eps, post, method="sweep")):
        got, names = U.kernels_of(tgp, dm, mirror)
        assert names == {KERNEL} and GD.err(np.asarray(got), want) <= BAR, names
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0")      # noqa: E731
    postd = tgp.replace_observation_noise_cov(tgp.posterior(dm, dev(yin)), dev(Rn))
    got, names = U.kernels_of(tgp, dm, lambda: tgp.rand((dev(eps[0]), dev(eps[1]), eps[2]), postd, method="sweep"))
    assert names == {KERNEL} and torch.is_tensor(got) and GD.err(got.cpu().numpy(), want) <= BAR, names


@pytest.mark.parametrize("d", [5, 8])
def test_gp_level_rand_at_new_inputs(tgp, d):
    """x_new interleaved with and beyond a sorted random x_train: the merged series on k_sweep_group_draw<sde>, against the oracle's posterior_rand at its 1e-7"""
    from temporalgps_jl_amd import lgssm as Lg
    from temporalgps_jl_amd import lti_sde as P
    rng = np.random.default_rng(5 + d)
    spec, _, s2 = SG.KERNELS[d]
    ntr, npr = 1800, 800
    xtr = np.sort(rng.uniform(0.0, 180.0, ntr))
    xpr = np.sort(np.concatenate([rng.uniform(0.0, 180.0, npr - 50), rng.uniform(180.0, 184.0, 50)]))
    _, ytr, _ = U.gp_case(spec, xtr, s2, seed=9 + d)
    f = P.to_sde(P.GP(P.to_kernel(spec)))
    seen = []
    inner = Lg.posterior_rand_group_sde

    def spy(post, *a):
        out, names = U.kernels_of(tgp, post._prior, lambda: inner(post, *a))
        seen.append((names, post._prior.handle().sweep_info()["served"]))
        return out

    Lg.posterior_rand_group_sde = spy
    try:
        ys = P.rand(np.random.default_rng(11), P.posterior(f(xtr, s2), ytr)(xpr, 0.2), method="sweep")
    finally:
        Lg.posterior_rand_group_sde = inner
    assert seen == [({KERNEL}, 1)], seen
    g = np.random.default_rng(11)
    eps_t, eps_e = g.standard_normal((ntr + npr, d)), g.standard_normal(ntr + npr)
    np.testing.assert_allclose(ys, oc.posterior_rand(spec, xtr, s2, ytr, xpr, 0.2, eps_t, eps_e, g.standard_normal(d)), rtol=1e-7, atol=1e-7)
    # training inputs on a RegularSpacing keep their own branch: other prediction inputs are not served there
    with pytest.raises(NotImplementedError):
        P.rand(np.random.default_rng(11), P.posterior(f(P.RegularSpacing(0.0, 0.1, 2100), s2), np.where(np.arange(2100) % 9 == 0, np.nan, 0.0))(xpr, 0.2), method="sweep")


def test_the_default_rand_runs_what_it_ran_before(tgp):
    """lgssm.rand(eps, post) without a method at d = 5: the evaluated route -- no k_sweep_group_draw kernel in the call; values at that route's parity, 1e-8"""
    b, _, y, mk, Rn, eps, want = case(5, 0, 2048)
    dm = bind(tgp, *b)
    post = tgp.replace_observation_noise_cov(tgp.posterior(dm, np.where(mk, np.nan, y)), Rn)
    got, names = U.kernels_of(tgp, dm, lambda: tgp.rand(eps, post))
    assert names and not any(n.startswith("k_sweep_group_draw") for n in names), names
    assert dm.handle().sweep_info()["served"] == 0
    assert GD.err(np.asarray(got), want) <= 1e-8
