"""CPU tier: the dense-powers one-launch smoother (logpdf + posterior marginals of LTI models WITHOUT a modal form -- a sum of two
kernels with one length scale has a defective closed loop) run on the host -- the product's own plan and head functions
(tgp_steady_plan.hpp build_smooth / smooth_head_*) and a lane-by-lane restatement of k_smooth_one's orchestration
(tests/hostsim/smoothsim.cpp) -- against the oracle's literal restatement of the reference's sequential recursions (lgssm.jl:99-238).
Tolerances (fp64): logpdf rel 1e-10; posterior marginals abs 1e-8 * scale."""
import numpy as np
import pytest

from oracle import lgssm_ref as ref
from tests import _util as U

CASES = [
    (("sum", ("matern52",), ("matern52",)), 0.1, 0.1),          # SURVEY 8d's cfg3 at d = 6: no modal form
    (("sum", ("matern32",), ("matern32",)), 0.1, 0.2),
    (("sum", ("matern52",), ("matern52",), ("matern32",)), 0.1, 0.1),      # d = 8
    (("matern52",), 0.1, 0.1),                                  # (models WITH a modal form run through it just as well)
    (("sum", ("matern52",), ("matern32",)), 0.05, 0.3),
    (("matern12",), 0.2, 0.5),
    (("sum", ("matern12",), ("matern12",)), 0.1, 0.1),
]


def _reference(model, y, Rn):
    lp = ref.logpdf(model, y)
    post = ref.posterior(model, y)
    pm, pv = ref.marginals(ref.replace_observation_noise_cov(post, np.broadcast_to(Rn, (model["T"],)).copy()))
    return lp, pm, pv


def _check(r, lp, pm, pv):
    assert r["rc"] == 0 and r["why"] == 0, r
    assert abs(r["lml"] - lp) <= 1e-10 * abs(lp), (r["lml"], lp)
    sc = max(1.0, np.abs(pm).max())
    assert np.abs(r["mean"] - pm).max() <= 1e-8 * sc, np.abs(r["mean"] - pm).max()
    assert np.abs(r["var"] - pv).max() <= 1e-8 * max(1.0, pv.max()), np.abs(r["var"] - pv).max()


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("T", [4200, 9000])
def test_dense_powers_smoother_equals_oracle(i, T):
    k, dt, s2 = CASES[i]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=i)
    Rn = 0.05
    lp, pm, pv = _reference(model, y, Rn)
    r = U.smoothsim_run(model, y, Rn)
    _check(r, lp, pm, pv)
    assert r["nwg"] >= 2      # (several spans: the halos and the chain over the tiles are exercised)


def test_per_step_new_noise_and_a_series_ending_inside_a_tile():
    k, dt, s2 = CASES[0]
    T = 5003
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=11)
    Rn = np.random.default_rng(3).random(T) * 0.1
    lp, pm, pv = _reference(model, y, Rn)
    _check(U.smoothsim_run(model, y, Rn), lp, pm, pv)


def test_a_series_too_short_is_declined():
    k, dt, s2 = CASES[0]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, 90), s2, seed=2)
    r = U.smoothsim_run(model, y, 0.1)
    assert r["why"] != 0


@pytest.mark.parametrize("i", [0, 1, 3, 4, 5, 6])
def test_a_draw_from_the_posterior_equals_the_oracles(i):
    """rand(rng, replace_observation_noise_cov(posterior(model, y), Rn)) with the draws supplied (posterior_lti_sde.jl:48-58 -> lgssm.jl:65-91 on
    the reverse-time model of :193-221): the kernel's recursion with a noise input (k_smooth_one<RAND>, d <= 6) against the oracle's literal loop
    over the EVALUATED posterior"""
    k, dt, s2 = CASES[i]
    T = 5003
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=20 + i)
    d = len(model["x0m"])
    if d > 6:
        pytest.skip("the draw's kernel holds d <= 6")
    rng = np.random.default_rng(i)
    eps = (rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    for Rn in (0.05, rng.random(T) * 0.1):
        post = ref.replace_observation_noise_cov(ref.posterior(model, y), np.broadcast_to(Rn, (T,)).copy())
        want = ref.rand(post, *eps)
        r = U.smoothsim_run(model, y, Rn, eps=eps)
        assert r["rc"] == 0 and r["why"] == 0, r
        assert np.abs(r["mean"] - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), np.abs(r["mean"] - want).max()


def test_a_halo_longer_than_a_span():
    """two Matern-1/2 of one (long) length scale at a short spacing: the recursions forget within 1520 steps -- under the 1536 the tile chain covers,
    but longer than the 1056 steps a span then holds: the second workgroup's run-in would reach back into the head and in front of the series (found
    as a GPU memory fault by scripts/stress_modal.py, seed 101, case 367).  It starts behind the head instead, from the head's exact end state."""
    spec = ("sum", ("scaled", 0.718, ("stretched", 0.6924527157043311, ("matern12",))), ("scaled", 0.605, ("stretched", 0.6924527157043311, ("matern12",))))
    T = 20000
    model, y, _ = U.gp_case(spec, ("regular", 0.0, 0.04, T), 2.56e-2, seed=1)
    Rn = np.random.default_rng(3).random(T) * 0.1
    lp, pm, pv = _reference(model, y, Rn)
    r = U.smoothsim_run(model, y, Rn)
    assert r["halo"] > 1365 and r["nwg"] > 3, r
    _check(r, lp, pm, pv)


# ---------------------------------------------------------------------------- the edge suite's geometry without a GPU (tests/_dense_powers_edges.py)
def _edge_case(name):
    from oracle import seq_kalman as sk
    from tests import _dense_powers_edges as E
    spec, dt, noise, route = E.CLASSES[name]
    blocks = E.blocks_of(spec, dt, noise)
    d, N = len(blocks["x0m"]), E.T_CAP
    rng = np.random.default_rng(17)
    y = sk.rand(dict(blocks, T=N), rng.standard_normal((N, d)), rng.standard_normal(N), rng.standard_normal(d))
    hh = E.offsets(N) if route == "offset" else None
    if hh is not None:
        y = y - float(blocks["h"][0]) + hh
    return blocks, d, y, hh, 0.01 + 0.1 * rng.random(N), (rng.standard_normal((N, d)), rng.standard_normal(N), rng.standard_normal(d))


def _edge_names():
    from tests import _dense_powers_edges as E
    return [n for n in E.CLASSES if E.EXPECTED[n]["why"] == 0]


def _restatements_head_and_tail(blocks, sp):
    """The restatement compiles the plan header itself, without the fused multiply-adds of the library's build.  Halos (16-step multiples with a 2^-60 margin)
    agree with tgp_smooth_plan; the two lengths that end where a recursion stops changing by 2 ulp may differ by a step or two -- the head (the 16-step
    multiple behind n0) then by 16 steps where n0 sits next to a multiple (stretched_d6: n0 = 351), the tail n1 by a step.  The lengths of these tests are
    placed by the restatement's own head and tail, through the same edge_lengths()."""
    from tests import _dense_powers_edges as E
    r = U.smoothsim_run(dict(blocks, T=E.T_CAP), np.zeros(E.T_CAP), 0.1)
    assert r["why"] == 0 and r["halo"] == sp["halo"] and r["nhs"] - sp["nhs"] in (-16, 0, 16) and abs(r["n1"] - sp["n1"]) <= 2, (r["nhs"], r["halo"], r["n1"], sp)
    return r["nhs"], r["n1"]


@pytest.mark.parametrize("name", _edge_names())
def test_posterior_marginals_at_the_edge_suites_lengths(name):
    """the host restatement of k_smooth_one<posterior> at the lengths tests/test_gpu_dense_powers_edges.py computes for the class from tgp_smooth_plan -- the
    `from_head` classes among them, and the lengths that put the variance tail over two workgroups (no served class has a tail longer than a span:
    _dense_powers_edges.EXPECTED); "offset" classes with their emission offset per step.  Against
    the oracle's C restatement (oracle/seq_kalman.py: tests/test_oracle_c.py holds it to the literal loops used above)."""
    from oracle import seq_kalman as sk
    from tests import _dense_powers_edges as E
    blocks, d, y, hh, Rn, _ = _edge_case(name)
    sp = E.smooth_plan(blocks, E.T_CAP)
    assert sp["why"] == 0
    nhs, C, halo, n1 = sp["nhs"], sp["span"], sp["halo"], sp["n1"]
    nhs, n1 = _restatements_head_and_tail(blocks, sp)
    tmin = nhs + n1 + 16
    worst = [0.0, 0.0, 0.0]
    for T in sorted(set(E.edge_lengths(nhs, C, halo, n1) + [tmin, tmin - 1])):
        model = dict(blocks, T=T) if hh is None else dict(blocks, T=T, h=hh[:T].copy())
        r = U.smoothsim_run(model, y[:T], Rn[:T], hh_t=None if hh is None else hh[:T])
        if T < tmin:
            assert r["why"] == E.WHY_TOO_SHORT, (T, r["why"])
            continue
        assert (r["why"], r["nhs"], r["halo"], r["n1"], r["nwg"]) == (0, nhs, halo, n1, -(-(T - nhs) // C)), (T, r)
        lp, (pm, pv) = sk.logpdf(model, y[:T]), sk.posterior_marginals(model, y[:T], Rn[:T])
        dev = (abs(r["lml"] - lp) / abs(lp), np.abs(r["mean"] - pm).max() / max(1.0, np.abs(pm).max()), np.abs(r["var"] - pv).max())
        worst = [max(a, b) for a, b in zip(worst, dev)]
        assert dev[0] <= 1e-10 and dev[1] <= 1e-8 and dev[2] <= 1e-8, (T, dev)
    print(f"{name}: worst lp {worst[0]:.1e} mean {worst[1]:.1e} var {worst[2]:.1e}")


@pytest.mark.parametrize("name", [n for n in _edge_names() if int(n.rsplit("_d", 1)[1]) <= 6])
def test_posterior_draws_at_the_edge_suites_lengths(name):
    """... and of k_smooth_one<rand> (the LTI form of every class with d <= 6), against the vectorised restatement of the literal draw on the oracle's evaluated posterior"""
    from oracle import seq_kalman as sk
    from tests import _dense_powers_edges as E
    blocks, d, y, hh, Rn, eps = _edge_case(name)
    if hh is not None:
        y = y - hh + float(blocks["h"][0])      # (the draw's kernel serves the LTI form)
    sp = E.smooth_plan(blocks, E.T_CAP)
    C, halo = sp["span"], sp["halo"]
    nhs, n1 = _restatements_head_and_tail(blocks, sp)
    worst = 0.0
    for T in (T for T in E.edge_lengths(nhs, C, halo, n1) + [nhs + n1 + 16] if T >= nhs + n1 + 16):
        model = dict(blocks, T=T)
        e = (eps[0][:T], eps[1][:T], eps[2])
        r = U.smoothsim_run(model, y[:T], Rn[:T], eps=e)
        assert r["rc"] == 0 and r["why"] == 0, (T, r)
        want = U.posterior_draw(sk.posterior(model, y[:T]), Rn[:T], *e)
        dev = np.abs(r["mean"] - want).max() / max(1.0, np.abs(want).max())
        worst = max(worst, dev)
        assert dev <= 1e-8, (T, dev)
    print(f"{name}: worst draw {worst:.1e}")


@pytest.mark.parametrize("i,T", [(0, 700), (4, 333)])
def test_the_vectorised_posterior_draw_is_the_literal_loop(i, T):
    """tests/_util.py posterior_draw (batched factorisations, a plain loop backwards) against ref.rand on the evaluated posterior with replaced noise, on the
    literal and on the C oracle's posterior; 1e-12 of the draw's scale (the same sums in another order)"""
    from oracle import seq_kalman as sk
    k, dt, s2 = CASES[i]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=60 + i)
    d = len(model["x0m"])
    rng = np.random.default_rng(i)
    eps = (rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    post = ref.posterior(model, y)
    for Rn in (np.array([0.05]), rng.random(T) * 0.1, None):
        lit = post if Rn is None else ref.replace_observation_noise_cov(post, np.broadcast_to(Rn, (T,)).copy())
        want = ref.rand(lit, *eps)
        sc = max(1.0, np.abs(want).max())
        assert np.abs(U.posterior_draw(post, Rn, *eps) - want).max() <= 1e-12 * sc
        assert np.abs(U.posterior_draw(sk.posterior(model, y), Rn, *eps) - want).max() <= 1e-9 * sc      # (the C oracle's posterior: tests/test_oracle_c.py's bar)


def test_the_oracles_filter_and_evaluated_posterior_of_a_prefix_are_a_prefix():
    """what tests/test_gpu_dense_powers_edges.py shares among the lengths of a class: both run forwards -- the first T steps do not see what follows"""
    from oracle import seq_kalman as sk
    from tests import _dense_powers_edges as E
    blocks, d, y, _, _, _ = _edge_case("identical_d6")
    N, T = 3000, 1777
    _, fm, fP = sk.filter_(dict(blocks, T=N), y[:N], want_states=True)
    _, fm1, fP1 = sk.filter_(dict(blocks, T=T), y[:T], want_states=True)
    assert np.array_equal(fm[:T], fm1) and np.array_equal(fP[:T], fP1)
    p, p1 = sk.posterior(dict(blocks, T=N), y[:N]), sk.posterior(dict(blocks, T=T), y[:T])
    assert all(np.array_equal(p[k][:T], p1[k]) for k in ("A", "a", "Q"))
    assert np.array_equal(p1["x0m"], fm[T - 1]) and np.allclose(p1["x0P"], fP[T - 1], rtol=0, atol=1e-15)


@pytest.mark.parametrize("i", [0, 3, 4, 6])
def test_an_emission_offset_per_step(i):
    """a GP with a mean function on a regular grid (lti_sde.jl:118-131): every block shared but the emission offset h_t = m(x_t).  The gains never see
    the offset: the stationary structure holds, the kernel subtracts the offset per step (SmoothCall::hh_t)"""
    k, dt, s2 = CASES[i]
    T = 6000
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=40 + i, mean=("custom", lambda t: np.sin(0.7 * t) + 0.1 * t))
    hh = np.asarray(model["h"], dtype=np.float64)
    assert hh.shape[0] == T
    Rn = np.random.default_rng(i).random(T) * 0.1
    lp, pm, pv = _reference(model, y, Rn)
    r = U.smoothsim_run(model, y, Rn, hh_t=hh)
    _check(r, lp, pm, pv)
