"""CPU tier: the geometry of a group-sweep call on an SDE-described model (tgp_sweep_plan.hpp plan_group's SDE branch) through a
stand-alone host program (tests/hostsim/sweep_group_sde_plan.cpp): no GPU.  It accepts d = 5 .. 8 with the LTI plan's properties (C a multiple of 8
and of the checkpoint block, every step owned by exactly one group), sizes the grid by this family's waves per CU, hands the kernel the prior
predicted through the first transition, and declines d = 4 and 9, T = 2047, fewer chunks than a wave owns and a warm-up beyond four chunks."""
import numpy as np
import pytest

from oracle import components as oc
from tests import _sweep_group as SG
from tests import _sweep_group_sde as SS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return SS.plan_program(tmp_path_factory.mktemp("sweep_group_sde_plan"))


def _model(d):
    k, dt, s2 = SG.KERNELS[d]
    t = np.cumsum(np.random.default_rng(d).uniform(0.5 * dt, 1.5 * dt, 64))
    return k, dt, oc.build_lgssm(k, t, s2)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d0 = tmp_path_factory.mktemp("sweep_group_sde_models")
    out = {}
    for d in (5, 6, 7, 8):
        k, dt, m = _model(d)
        out[d] = str(d0 / f"m{d}.txt")
        SS.write_model(out[d], k, m, dt)
    k, dt, m = _model(5)
    out[4] = str(d0 / "m4.txt")
    SS.write_model(out[4], k, m, dt, d=4)
    k, dt, m = _model(8)
    out[9] = str(d0 / "m9.txt")
    SS.write_model(out[9], k, m, dt, d=9)
    return out


@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("T", [2048, 5003, 40_000])
@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_accepts_and_every_step_has_one_owner(exe, models, d, T, post):
    p = SS.run_plan(exe, models[d], T, post=post)
    assert p["ok"], p
    assert p["d"] == d and p["B"] == (8 if d <= 6 else 4) and p["owned"] == (6 if post else 7)
    assert p["C"] % 8 == 0 and p["C"] % p["B"] == 0 and p["C"] >= 64
    assert p["W"] % 8 == 0 and p["Wb"] % 8 == 0 and 8 <= p["Wb"] <= p["C"] and p["W"] <= 4 * p["C"]
    assert p["nchunks"] == -(-T // p["C"]) and p["nwaves"] == -(-p["nchunks"] // p["owned"])
    owner = np.zeros(T, dtype=int)
    for wave, g, t0, t1, runs, owned in p["spans"]:
        assert 0 <= t0 <= t1 <= T and t0 % 8 == 0 and t1 - t0 <= p["C"]
        if owned:
            assert runs and 1 <= g <= p["owned"] and (t1 - t0 == p["C"] or t1 == T)
            owner[t0:t1] += 1
    assert owner.min() == 1 and owner.max() == 1


def test_the_grid_is_sized_by_this_familys_waves_per_cu(exe, models):
    """a series long enough for the chunk length to follow the slots: 256 CUs x (8 logpdf | 4 posterior) waves x owned chunks"""
    T = 4_000_000
    for post, per_cu, owned in ((0, 8, 7), (1, 4, 6)):
        p = SS.run_plan(exe, models[6], T, post=post)
        slots = 256 * per_cu * owned
        assert p["ok"] and p["C"] == -(-(-(-T // slots)) // 8) * 8, (p["C"], slots)


@pytest.mark.parametrize("d", [5, 7])
def test_the_kernel_is_given_the_prior_predicted_through_the_first_transition(exe, models, d):
    k, dt, m = _model(d)
    p = SS.run_plan(exe, models[d], 4096)
    A1, Q1, P0 = m["A"][0], m["Q"][0], m["x0P"]
    want = A1 @ P0 @ A1.T + Q1
    assert np.abs(p["x0P"].reshape(d, d, order="F") - want).max() <= 1e-14 * np.abs(P0).max()
    assert np.abs(p["x0m"] - (A1 @ m["x0m"] + m["a"][0])).max() <= 1e-15
    F, _, _, blocks = SS.sde_blocks(k)
    assert np.array_equal(p["N1"].reshape(d, d), SS.closed_form(F, blocks)[1])


@pytest.mark.parametrize("d", [4, 9])
def test_declines_other_dimensions(exe, models, d):
    p = SS.run_plan(exe, models[d], 4096)
    assert not p["ok"] and p["why"] == "state dimension"


def test_declines_short_series(exe, models):
    assert SS.run_plan(exe, models[6], 2048)["ok"]
    p = SS.run_plan(exe, models[6], 2047)
    assert not p["ok"] and "2048" in p["why"]


def test_declines_a_doubled_warm_up_beyond_four_chunks(exe, models):
    p = SS.run_plan(exe, models[5], 4096)
    assert p["ok"]
    w = p["W"]
    while w <= 4 * p["C"]:      # the repair loop's doubling
        assert SS.run_plan(exe, models[5], 4096, w_hint=w)["ok"]
        w *= 2
    q = SS.run_plan(exe, models[5], 4096, w_hint=w)
    assert not q["ok"] and q["why"] == "forward warm-up longer than four chunks"


def test_declines_fewer_chunks_than_a_wave_owns(exe, models):
    p = SS.run_plan(exe, models[8], 2048, fC=512)
    assert not p["ok"] and p["why"] == "fewer chunks than one wave owns"
