"""CPU tier: the geometry of a group-sweep call (tgp_sweep_plan.hpp plan_group / group_span) through a stand-alone host program
(tests/hostsim/sweep_group_plan.cpp): no GPU.  It accepts d = 5 .. 8 at T = 2048, 2049 and 40 000 with C a multiple of 8 and of the checkpoint
block, every step owned by exactly one group (the last chunk may be short), and declines d = 4, d = 9, T = 2047, a warm-up hint beyond four
chunks and a forced chunk so long that a wave has fewer chunks than it owns."""
import pytest

from tests import _sweep_group as SG


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return SG.plan_program(tmp_path_factory.mktemp("sweep_group_plan"))


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d0 = tmp_path_factory.mktemp("sweep_group_models")
    out = {}
    for d in (5, 6, 7, 8):
        out[d] = str(d0 / f"m{d}.txt")
        SG.write_model(out[d], SG.lti_model(d, 64))
    out[4] = str(d0 / "m4.txt")
    SG.write_model(out[4], SG.lti_model(5, 64), d=4)
    out[9] = str(d0 / "m9.txt")
    SG.write_model(out[9], SG.lti_model(8, 64), d=9)
    return out


@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("T", [2048, 2049, 40_000])
@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_accepts_and_every_step_has_one_owner(exe, models, d, T, post):
    p = SG.run_plan(exe, models[d], T, post=post)
    assert p["ok"], p
    assert p["d"] == d and p["B"] == (8 if d <= 6 else 4) and p["owned"] == (6 if post else 7)
    assert p["C"] % 8 == 0 and p["C"] % p["B"] == 0 and p["C"] >= 64
    assert p["W"] % 8 == 0 and p["Wb"] % 8 == 0 and 8 <= p["Wb"] <= p["C"] and p["W"] <= 4 * p["C"]
    assert p["nchunks"] == -(-T // p["C"]) and p["nwaves"] == -(-p["nchunks"] // p["owned"])
    assert len(p["spans"]) == 8 * p["nwaves"]
    owner = [0] * T
    for wave, g, t0, t1, runs, owned in p["spans"]:
        assert 0 <= t0 <= t1 <= T and t0 % 8 == 0 and t1 - t0 <= p["C"]
        assert not (owned and not runs) and not (g == 0 and runs) and not (g > p["owned"] and owned)
        if owned:
            assert t1 > t0 and (t1 - t0 == p["C"] or t1 == T)      # only the last chunk may be short
            for t in range(t0, t1):
                owner[t] += 1
    assert min(owner) == 1 and max(owner) == 1
    # a group that owns output has a neighbour in its wave on either side that hands it its start states
    by = {(w, g): (t0, t1, runs) for w, g, t0, t1, runs, _ in p["spans"]}
    for wave, g, t0, t1, runs, owned in p["spans"]:
        if owned and t0 > 0:
            assert by[(wave, g - 1)][1] == t0      # the forward warm-up of the chunk in front
        if owned and post and t1 < T:
            nt0, _, nruns = by[(wave, g + 1)]
            assert nt0 == t1 and nruns                 # the backward warm-up of the chunk behind (it runs its own forward pass)


def test_forced_geometry_is_taken(exe, models):
    p = SG.run_plan(exe, models[5], 4100, fC=64, fW=40, fWb=64)
    assert p["ok"] and (p["C"], p["W"], p["Wb"]) == (64, 40, 64) and p["nchunks"] == 65 and p["nwaves"] == 11
    assert [s for s in p["spans"] if s[5]][-1][2:4] == (4096, 4100)      # the last chunk is short, the last wave partly filled


@pytest.mark.parametrize("d", [4, 9])
def test_declines_other_dimensions(exe, models, d):
    p = SG.run_plan(exe, models[d], 4096)
    assert not p["ok"] and p["why"] == "state dimension"


def test_declines_short_series(exe, models):
    assert SG.run_plan(exe, models[6], 2048)["ok"]
    p = SG.run_plan(exe, models[6], 2047)
    assert not p["ok"] and "2048" in p["why"]


def test_declines_a_doubled_warm_up_beyond_four_chunks(exe, models):
    p = SG.run_plan(exe, models[5], 4096)
    assert p["ok"]
    w = p["W"]
    while w <= 4 * p["C"]:      # the repair loop's doubling
        assert SG.run_plan(exe, models[5], 4096, w_hint=w)["ok"]
        w *= 2
    q = SG.run_plan(exe, models[5], 4096, w_hint=w)
    assert not q["ok"] and q["why"] == "forward warm-up longer than four chunks"


def test_declines_fewer_chunks_than_a_wave_owns(exe, models):
    p = SG.run_plan(exe, models[8], 2048, fC=512)
    assert not p["ok"] and p["why"] == "fewer chunks than one wave owns"
