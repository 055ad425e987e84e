"""CPU tier: the structure of the group sweep's draw kernel (tgp_sweep_group.hip k_sweep_group_draw) restated in NumPy
(tests/_sweep_group_draw.py chunked_draw: forward chunks with checkpoints, the backward warm-up over Wd steps with the real draws, the hand-over, the
check distance, the step with Z = U G' from the factor and L = Pf - Z'Z) against the oracle's two restatements of the walk on the SAME draws:
ref.rand(ref.replace_observation_noise_cov(ref.posterior_missing(...))) and tests/_sweepdraw.py draw_restated.

tests/_sweep_group.py's models at d = 5 .. 8, T = 2048, 10 % missing with the first and the last step among them, in the geometry tgp_sweep_plan.hpp's
plan_group chooses for a posterior call of a 256-CU device (the draw's plan: the same slots, the backward warm-up's estimate as the first guess of Wd).
The bar is the draws' 1e-9 of max(1, max |y*|); the two references differ by 1.7e-13 .. 2.1e-12 on these cases."""
import numpy as np
import pytest

from oracle import lgssm_ref as ref
from tests import _sweep_group as SG
from tests import _sweep_group_draw as GD
from tests import _sweepdraw as SD

BAR = 1e-9
T = 2048


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return SG.plan_program(tmp_path_factory.mktemp("sweep_group_draw_plan"))


@pytest.fixture(scope="module")
def cases(plan_exe, tmp_path_factory):
    out = {}
    tmp = tmp_path_factory.mktemp("sweep_group_draw_models")
    for d in (5, 6, 7, 8):
        model, y, mk, Rn, eps = GD.case(d, T, seed=80 + d)
        assert mk[0] and mk[T - 1] and 0.07 < mk.mean() < 0.13
        path = str(tmp / f"model{d}.txt")
        SG.write_model(path, model)
        plan = SG.run_plan(plan_exe, path, T, num_cu=256, post=1)
        assert plan["ok"], plan
        want = ref.rand(ref.replace_observation_noise_cov(ref.posterior_missing(model, np.where(mk, 0.0, y), mk), Rn.copy()), *eps)
        out[d] = dict(model=model, y=y, mk=mk, Rn=Rn, eps=eps, plan=plan, want=want, restated=SD.draw_restated(model, y, mk, Rn, eps))
    return out


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_the_chunked_walk_equals_both_restatements_in_the_plans_geometry(cases, d):
    c = cases[d]
    p = c["plan"]
    print(d, {k: p[k] for k in ("C", "W", "Wb", "B", "nchunks", "nwaves")}, "references apart by %.3g" % GD.err(c["restated"], c["want"]))
    assert GD.err(c["restated"], c["want"]) <= BAR / 100      # (the reference side stays far under the bar)
    got, dist_f, dist_d = GD.chunked_draw(c["model"], c["y"], c["mk"], c["Rn"], c["eps"], p["C"], p["W"], p["Wb"], p["B"])
    e1, e2 = GD.err(got, c["want"]), GD.err(got, c["restated"])
    print(d, "error / scale %.3g (ref.rand), %.3g (draw_restated); hand-over distances %.3g / %.3g" % (e1, e2, dist_f, dist_d))
    assert np.isfinite(got).all()
    assert e1 <= BAR and e2 <= BAR, (e1, e2)
    assert dist_f <= GD.TOL_F and dist_d <= GD.TOL_D, (dist_f, dist_d)      # the plan's own warm-ups pass both checks


@pytest.mark.parametrize("d", [5, 8])
def test_a_draw_warm_up_that_is_too_short_shows_in_the_check_distance(cases, d):
    c = cases[d]
    p = c["plan"]
    got, dist_f, dist_d = GD.chunked_draw(c["model"], c["y"], c["mk"], c["Rn"], c["eps"], p["C"], p["W"], 8, p["B"])
    print(d, "Wd = 8: draw distance %.3g, error / scale %.3g" % (dist_d, GD.err(got, c["want"])))
    assert dist_f <= GD.TOL_F and dist_d > 10 * GD.TOL_D, (dist_f, dist_d)      # what the kernel reports as status bit 2


def test_zero_draws_walk_the_smoothers_mean(cases):
    """with every draw zero the walk is the reverse-time model's mean recursion: the posterior mean of the oracle, at the marginals' 1e-8"""
    c = cases[6]
    p = c["plan"]
    d = 6
    z = (np.zeros((T, d)), np.zeros(T), np.zeros(d))
    got, _, dist_d = GD.chunked_draw(c["model"], c["y"], c["mk"], 0.3, z, p["C"], p["W"], p["Wb"], p["B"])
    pm, _ = ref.marginals(ref.replace_observation_noise_cov(ref.posterior_missing(c["model"], np.where(c["mk"], 0.0, c["y"]), c["mk"]), np.full(T, 0.3)))
    assert GD.err(got, pm) <= 1e-8 and dist_d <= GD.TOL_D
