"""CPU tier: the two pure host functions the dense-powers one-launch kernels' edge suite places its lengths by -- tgp_smooth_plan (the plan of
k_smooth_one<logpdf | posterior | rand>, tgp_powers::plan_smooth) and tgp_rand_plan (the plan of k_rand_one, tgp_powers::plan_rand) -- against tgp_filter_plan,
against the geometry the kernels' launch code derives from a plan (csrc/tgp_powers.hip launch_smooth / launch_rand: span = 4096 - one or two halos,
workgroups = ceil(steps behind the head / span)), and on the declines they document (include/tgp_hip.h)."""
import numpy as np
import pytest

from tests import _dense_powers_edges as E


def _model(name):
    spec, dt, noise, _ = E.CLASSES[name]
    return E.blocks_of(spec, dt, noise)


@pytest.mark.parametrize("name", list(E.CLASSES))
def test_the_table_of_the_edge_suite_is_what_the_plans_report(name):
    geo = E.geometry(name)
    print(name, geo)
    assert geo == E.EXPECTED[name], (name, geo)


@pytest.mark.parametrize("name", list(E.CLASSES))
def test_smooth_plan_agrees_with_the_filter_plan_and_the_launch_geometry(name):
    m = _model(name)
    fp = E.filter_plan(m, E.T_CAP)
    assert fp["why"] == 0, fp
    for post in (False, True):
        sp = E.smooth_plan(m, E.T_CAP, post)
        assert (sp["n0"], sp["nhs"], sp["halo_f"]) == (fp["n0"], fp["nhs"], fp["halo"]), (post, sp, fp)
        if sp["why"] != 0:
            assert post and sp["why"] == E.WHY_SLOW_MIXING and sp["nwg"] == 0, sp      # (only the backward half can decline what the filter plan took)
            continue
        if post:
            assert sp["halo"] >= fp["halo"] and sp["halo"] % 16 == 0 and 0 < sp["n1"] <= 2048, sp
        else:
            assert sp["halo"] == fp["halo"] and sp["n1"] == 0, sp
        assert sp["span"] == E.SPAN - (2 if post else 1) * sp["halo"] and sp["span"] >= 1024, sp
        C, nhs = sp["span"], sp["nhs"]
        for T in (nhs + sp["n1"] + 16, nhs + C - 1, nhs + C, nhs + C + 1, nhs + 8 * C, nhs + 8 * C + 1, E.T_CAP):
            q = E.smooth_plan(m, T, post)
            assert q["nwg"] == -(-(T - nhs) // C), (T, q)
            assert {k: v for k, v in q.items() if k != "nwg"} == {k: v for k, v in sp.items() if k != "nwg"}, (T, q, sp)      # (T only counts the workgroups)


@pytest.mark.parametrize("name", list(E.CLASSES))
def test_rand_plan_reports_the_launch_geometry_of_the_prior_draw(name):
    m = _model(name)
    rp = E.rand_plan(m, E.T_CAP)
    if E.EXPECTED[name]["why_r"] != 0:      # (the open loop at a spacing <= 0.01 does not forget within 1536 steps)
        assert rp == dict(why=E.WHY_SLOW_MIXING, halo=rp["halo"], span=0, nwg=0), rp
        return
    assert rp["why"] == 0 and 16 <= rp["halo"] <= 1536 and rp["halo"] % 16 == 0, rp
    assert rp["span"] == E.SPAN - rp["halo"], rp
    C = rp["span"]
    for T in (1, 2, C - 1, C, C + 1, 8 * C, 8 * C + 1, E.T_CAP):
        q = E.rand_plan(m, T)
        assert q["nwg"] == -(-T // C) and (q["why"], q["halo"], q["span"]) == (0, rp["halo"], C), (T, q)


@pytest.mark.parametrize("name", ["tiny_d1", "from_head_d3", "identical_d6", "declined_d8"])
def test_a_series_one_step_too_short_is_declined_as_too_short(name):
    m = _model(name)
    sp = E.smooth_plan(m, E.T_CAP)
    nhs, n1 = sp["nhs"], sp["n1"]
    assert E.smooth_plan(m, nhs + n1 + 16)["why"] == 0                                  # head + tail + 16 steps: the shortest series with the backward half
    short = E.smooth_plan(m, nhs + n1 + 15)
    assert short["why"] == E.WHY_TOO_SHORT and short["nwg"] == 0, short
    assert (short["nhs"], short["halo_f"], short["n1"]) == (nhs, sp["halo_f"], n1), short      # (what was known when the plan stopped is still reported)
    t_lp = E.shortest_served(lambda T: E.smooth_plan(m, T, post=False), 1, nhs + 64)
    assert t_lp == E.shortest_served(lambda T: E.filter_plan(m, T), 1, nhs + 64)        # the forward half alone: the filter plan's own condition
    assert E.smooth_plan(m, t_lp - 1, post=False)["why"] == E.WHY_TOO_SHORT


def test_slow_mixing_is_declined_with_the_documented_code():
    # the closed loop's powers are not below 2^-60 after 1536 steps (the class tests/test_gpu_adjoint_edges.py declines on): the filter plan's verdict, passed on
    m = E.blocks_of(E.M52, 0.01, 2.0)
    assert E.filter_plan(m, 10 ** 6)["why"] == E.WHY_SLOW_MIXING
    for post in (False, True):
        sp = E.smooth_plan(m, 10 ** 6, post)
        assert sp["why"] == E.WHY_SLOW_MIXING and sp["span"] == 0 and sp["nwg"] == 0, sp
    # the filter's halo is the longest served (1536) and the settled reverse-time transition forgets more slowly still: the backward half alone declines
    spec, dt, noise, _ = E.DECLINED_BY_THE_BACKWARD_HALF
    m = E.blocks_of(spec, dt, noise)
    assert E.filter_plan(m, E.T_CAP)["why"] == 0 and E.smooth_plan(m, E.T_CAP, post=False)["why"] == 0
    assert E.smooth_plan(m, E.T_CAP)["why"] == E.WHY_SLOW_MIXING
    # the open loop at a very short spacing (tests/test_gpu_modal.py's fall-back case of tgp_rand)
    rp = E.rand_plan(E.blocks_of(E.M52, 0.0005, 0.05), 30_000)
    assert rp["why"] == E.WHY_SLOW_MIXING and rp["span"] == 0 and rp["nwg"] == 0, rp


def test_arguments_the_functions_refuse():
    from temporalgps_jl_amd import _lib
    lib = _lib.load()
    m = _model("tiny_d1")
    b = [x.ctypes.data for x in E._plan_args(m)]
    i8, i4 = np.zeros(8, dtype=np.int32), np.zeros(4, dtype=np.int32)
    assert lib.tgp_smooth_plan(9, *b, 1000, 1, i8.ctypes.data) == 1 and lib.tgp_rand_plan(0, *b, 1000, i4.ctypes.data) == 1      # TGP_EINVAL: d outside 1 .. 8
    assert lib.tgp_smooth_plan(1, *b, 0, 1, i8.ctypes.data) == 1 and lib.tgp_rand_plan(1, *b, 0, i4.ctypes.data) == 1            # ... T <= 0
    assert lib.tgp_smooth_plan(1, *b, 1000, 1, None) == 1 and lib.tgp_rand_plan(1, *b[:7], None, 1000, i4.ctypes.data) == 1      # ... a null pointer
