"""GPU tier (-m gpu): the sweep engine (csrc/tgp_sweep.hip, tgp_sweep_body.hpp, tgp_sweep_plan.hpp, sweep_call / sweep_draw_call) where
tests/test_gpu_sweep.py and tests/test_gpu_sweep_draw.py do not go: every kernel instantiation, chunk / wave / series edges through forced geometries, long
gaps against the warm-ups with the repair loop and its declines, ties, values that must not be served, and the engine's own buffers and remembered state.
Through the C ABI.  The cases are the entries of tests/_sweep_edges.py; tests/test_sweep_edges_host.py runs the same table through the host simulation.

Bars: logpdf 1e-10 relative, marginals 1e-8 of their scale against oracle/lgssm_ref.py (oracle/seq_kalman above 6000 steps); a draw 1e-9 against the walk
restated in NumPy on the same draws (tests/_sweepdraw.py), helpers of tests/test_gpu_sweep_draw.py.  Every case asserts tgp_sweep_info -- served, C, W, Wb,
waves, attempts, status, state -- and the profiled kernel name: a silent fallback to the general engine cannot pass a parity assert.  The HOST decides what a
check finds: _util.sweepsim_served / _sweepdraw.sweepdrawsim_served run the product's plan and per-lane code inside the call's repair loop, the table holds
the outcome, and only cases whose host distances lie a factor 10 on their side of kTol = 1e-12 / kTolBack = 1e-11 in every attempt are kept.

Models: d = 1 Matern-1/2, d = 2 Matern-3/2, d = 3 Matern-5/2, d = 4 Matern-3/2 + stretched(0.7) Matern-3/2; noise 0.1.  Working spacing dt = 0.1, 0.1, 0.1,
0.15 (automatic W / Wb = 32 / 32, 80 / 72, 112 / 104, 168 / 160); fast-forgetting spacing dt = 5, 4, 4, 6 (a start state is gone within 8 steps).

Host distances (dist_f, dist_b | draw: dist_f, dist_d), `python -m tests.test_sweep_edges_host` prints every entry:
    A  32 k_sweep cases, T = 2053, automatic geometry: <= 2.1e-14, <= 7.0e-14;  24 draws: <= 1.3e-14, <= 2.8e-13 (A-draw-d4-sde-xs1 with its name's
       seed had 1.03e-12, a factor 9.7 from the check: seed 1 is used)
    B  x0 not the stationary prior, (64, 256, 64): logpdf 0, -;  posterior declined backwards alone (Wb = 64): 0, 7.1e-09
    B  fast models at (8, 8, 8), every T: <= 7.3e-17, <= 5.7e-16;  one chunk / two chunks / W = Wb = C >= T: <= 5e-19 (0 where the warm-up reaches
       step 0), <= 1.5e-16;  C = 256 with W = 512 / 1280: 0 (1.1e-16 SDE), <= 1.9e-15;  draws: <= 3.9e-17, <= 1.1e-15
    C  T = 4096, boundary s = 2048 at C = 256, (short geometry | automatic geometry, per attempt):
       d = 3 [s, s + 350):        (256, 112, 104): 2.4e-15, 1.5e-09 -- only the backward check fails
                                  auto (104, 112, 104): 4.8e-11, 9.4e-09;  (208, 224, 208): 1.4e-16, 2.6e-15
       d = 3 [s - 400, s):        (256, 112, 104): 1.4e-11, 1.8e-14 -- only the forward check fails
                                  auto (104, 112, 104): 2.1e-09, 2.9e-09;  (208, 224, 208): 1.4e-16, 2.6e-15
       d = 3 [s - 100, s + 100):  (256, 112, 104): 7.6e-10, 1.6e-08;  auto: 4.9e-11, 1.5e-09;  then 8e-24, 3.2e-15
       d = 3 first / last 120:    (256, 112, 104): 1.5e-09, 3.9e-10;  auto: the same;  then 8.3e-24, 2.1e-15
       d = 4 [s, s + 400):        (256, 144, 144): 4.2e-15, 1.4e-10 -- backward only;  auto (160, 168, 160) passes: 1.2e-14, 2.9e-15
       d = 4 [s - 150, s):        (256, 144, 144): 1.6e-11, 3.0e-15 -- forward only;   auto passes: 1.2e-15, 3.9e-14
       d = 1 first / last 170:    (256, 32, 32): 3.7e-08, 2.9e-08;  auto: FOUR attempts -- (64, 32, 32) 1.3e-02, 1.1e-02; (64, 64, 64) 2.2e-05, 1.8e-05;
                                  (128, 128, 128) 3.7e-08, 2.9e-08; (256, 256, 256) 0, 3.3e-16  [logpdf call: C stays 64, W = 32 ... 256]
       d = 2 first / last 120:    (256, 80, 72): 1.4e-08, 3.5e-09;  auto: 1.4e-08, 1.4e-08; then (144, 160, 144) 4.9e-17, 1.3e-13
       d = 4 [s - 200, s + 200):  (256, 96, 96): 5.5e-10, 3.2e-10;  auto passes: 9.7e-16, 9.4e-13  (at (256, 144, 144) the gap is forgotten: 5.9e-15, 3.3e-15)
       d = 4 first / last 120:    (256, 112, 112): 7.7e-09, 6.1e-09;  auto passes: 5.8e-16, 4.9e-14  (first / last 170: 5.1e-13 at auto, borderline)
       d = 3 whole chunks [1024, 2048): (256, 112, 104) passes: 1.6e-15, 1.8e-14;  auto: 4.6e-10, 2.9e-09; then 1.4e-16, 2.6e-15
                                  ([1024, 3072) leaves the automatic geometry 1.9e-11 backwards, borderline: the shorter run is used)
       d = 4 whole chunks [1024, 3072): (256, 96, 96): 5.5e-10, 2.3e-10;  auto passes: 1.7e-15, 1e-14
       (256, 512, 256) serves every shape at once: <= 5.6e-16, <= 3.2e-15
       decline by the plan, d = 2 first / last 800, logpdf call: (72, 80, 72) 3.4e-06; (72, 160, 72) 2.3e-11; W = 320 > 4 x 72: declined, state -1.
       The posterior call of the same series is served at the third attempt: (72, 80, 72) 3.4e-06, 2.6e-06; (144, 160, 144) 2.3e-11, 3.2e-15;
       (144, 320, 144) 8.9e-16, 3.2e-15.
       draws, d = 3, default options: behind (104, 112, 104) -> (208, 224, 208); before the same: two attempts, Wd repaired with W
    D  ties, T = 2400: d = 1 seed 2 (64, 40, 32) 3.0e-11 fails forwards, (64, 80, 32) 5e-17, 3.6e-14;  d = 2 seed 1: 1.8e-14, 6.9e-13;  d = 4 seed 1:
       4.5e-15, 1.1e-13;  d = 3, both tied steps observed, seed 24: 9.4e-14, 5.4e-13;  d = 3 with missing tied steps at (256, 512, 256), seed 1:
       6.0e-16, 2.6e-15 (at the automatic geometry seeds 1 .. 39 all leave a distance within a factor 10 of a tolerance: the ties shorten the time that
       W steps cover)
    E  (256, 512, 256): negative noise variance: status 12 (the chunk's product of innovation variances turns negative, its logarithm is NaN: bit 8
       beside bit 4), the draw 4;  an infinite observation: 8
    F  (64, 8, 8) / (2048, 8, 8) <= 1e-16;  2050 waves at (8, 8, 8), T = 1 016 307: 6.8e-17, 1.8e-16, 0.2 s on the host

Which test launches which instantiation (profile names carry form and pass; D and XS follow from the case):
    k_sweep<D, form, XS, logpdf | posterior>, all 64: test_every_instantiation[A-k-d{D}-{form}-xs{XS}] (one logpdf and one posterior call each)
    k_sweep_draw<D, form, XS = 1, 2, 3>, 24 of 32: test_every_draw_instantiation[A-draw-d{D}-{form}-xs{XS}]
    k_sweep_draw<D, form, XS = 0>: tests/test_gpu_sweep_draw.py test_missing_data_on_a_regular_grid (lti), test_irregular_spacing_with_ties (sde), D = 1 .. 4
    (k_sweep_draw<D = 3 and 4, sde, 3> also: tests/test_gpu_sweep_draw.py test_every_stream_at_once)

Routing facts these tests turned up (DESIGN 3 / 4.7 have them too):
  * A series-caused decline switches the engine off for the BOUND MODEL, not for the call: after the plan's "forward warm-up longer than four chunks" (or four
    short attempts) sweep_state is -1, the next call on the handle -- whatever series -- goes to the general engine without a launch (attempts = 0), and only
    tgp_model_set or one of the options 14-17 brings the engine back.
  * A logpdf call repairs W alone and keeps C = max(64, Wb): at d = 2 the third attempt's W = 320 exceeds four chunks of 72 and the plan declines a series
    whose posterior call (C grows with Wb) is served.
  * A negative noise variance at one step gives status 12, not 4, and state -1; an infinite observation gives 8 and leaves the state alone.
  * A draw repairs Wd apart from Wb: the posterior call that follows a repaired draw on the same handle starts from the draw's W and its own first guess
    of Wb, and repairs that.
  * tgp_sweep_info behind a plan decline in a LATER attempt keeps the last launch's C, W, Wb and status.

Defects these tests found, fixed with them:
  * tgp_sweep_info kept the previous call's C, W, Wb, attempts and status beside served = 0 when the engine was not asked for a call (a model switched
    off by a decline showed attempts = 2 on a call that made none): check_ready clears the record now (csrc/tgp_api.hip).
  * the mirror ignored handle_options for SDE-described models (lgssm.py _handle_sde): a forced geometry on build_lgssm(..., device_components=True)
    was silently the automatic one.  Every forced SDE case of group B failed on that.
  * test infrastructure: the host simulation took the median of ALL noise variances / gaps where tgp_model_set takes the upper median of the first 4096
    (_util.sweep_representative restates the product's rule now).
  None in the kernels, the plan or the repair loop.

Mutations (one scratch build each, never committed, run on the device against this whole file):
  B  `lane <= kOwned` -> `<` in both kernels: 27 fail -- every case of more than 61 chunks (all B-seam / B-min / B-rem / B-warm-2 / -5 / B-125 cases, the four
     B draws, the 2048-step routing case, C-ends170-d1-auto at its attempts with C = 64, F-ckpt, F-part).
  B  `(t1 + 7) & ~7` -> `t1` in both kernels: 73 fail -- every case whose T is no multiple of 8 (all of group A, the 62 k + 1 seams, B-rem, one / two
     chunks, W >= T, the C = 256 cases, the rebind sequence, F-ckpt, F-part); T = 2480 / 2048 / 4096 / 2400 pass, as they must.
  B  dropping `if (t0 == 0) x = x0`: EQUIVALENT, all pass -- lane 0 of wave 0 has no chunk, its warm-up processes nothing from x0 (tw = -W <= 0), so what
     lane 1 receives through the shift IS x0; lanes without a chunk own nothing.
  B  `tw <= 0` -> `tw < 0`: EQUIVALENT to the checks' tolerance, all pass -- tw = 0 means the warm-up covers W whole steps from step 0, and W steps are what
     forgets a start state (and every GP model's x0 is the stationary prior the other branch starts from).  B-x0-not-stationary-d3 was added for the
     branch itself (a prior that is not the stationary one, chunks of 64 steps): with `x = gen` for every warm-up B-x0-not-stationary-d3 fails,
     and nothing else.
  C  the repair loop takes a pass with bit 2 set (`status & 3` -> `status & 1` in sweep_call): C-behind350-d3-short and C-behind400-d4-short fail (served
     where the table says declined), and both test_a_draw_repairs_its_own_warm_up cases (the posterior call behind the draw fails backwards alone under
     default options and is taken at attempt 1).  The C-*-auto cases pass: their first attempt fails forwards as well.
  A  load_inputs gives every step of a block the noise variance of the block's first step (`R[tc[0]]`): 36 fail -- all 32 XS = 1 and XS = 3 cases of
     group A (k_sweep and the draw, every d, both forms), the negative-variance cases in the middle of a chunk (the variance is no longer where the table
     put it), the rebind sequence (two of its models have a noise per step) and the GP-level prediction; every XS = 0 and XS = 2 case passes.
  D  load_inputs turns a gap of exactly 0 into 1e-6: all five test_ties cases and test_prediction_at_training_inputs fail, nothing else.
  E  sweep_call leaves sweep_state alone behind bit 4: E-negR-mid-d3 and E-negR-edge-d3 fail (state 0 where the table says -1), nothing else.
  F  tgp_model_set keeps sweep_W / sweep_Wb / sweep_Wd of the previous model: test_one_handle_bound_to_one_model_after_the_other fails (the geometry
     is not a fresh handle's), nothing else.
  A  c.R and c.hh swapped in fill_args: NOT RUN -- the kernel is chosen from the unswapped pointers, so at XS = 1 / 2 it would read through a null pointer.
  F  need_part never regrown: NOT RUN -- 2050 waves would write their records behind the end of a pinned host buffer.
  (A memory fault on a shared device is not a test outcome.  The XS = 1 / 2 cases of group A compare per-step noise and offset against the oracle with
  the other stream absent, and F-part asserts waves = 2050 with values at the bars over every wave's share of the sum.)

Not covered, and why:
  * a series that exhausts four attempts: none within T <= 8192 keeps the margin.  At d = 1 the fourth attempt's W = 256 leaves at most exp(-25.6) =
    7.6e-12 of a start state, less than a factor 10 above kTol (seen: 1.3e-12 ... 6e-12); at d >= 2 a logpdf call's doubled W exceeds four chunks first
    (the plan's decline, above) and a posterior call's chunk grows with Wb.
  * the automatic geometry on ties at d = 3 with missing tied steps, d = 4 with 170 steps missing at both ends, and d = 3 with [1024, 3072) missing:
    each leaves a host distance within a factor 10 of a tolerance; the neighbouring sizes above are used."""
import numpy as np
import pytest

from oracle import components as oc
from tests import _sweep_edges as E
from tests import _util as U
from tests.test_gpu_sweep_draw import BAR, SENTINEL, draw_call, err

pytestmark = pytest.mark.gpu


def names(group, what="k"):
    return [c.name for c in E.TABLE if c.group == group and c.what == what]


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def device_model(tgp, c, sweep=1):
    """the case's model on a handle of its own, the forced geometry in its options"""
    from temporalgps_jl_amd import lti_sde as P
    i, L = E.inputs(c), tgp._lib
    model = i["model"]
    if c.sde:
        dm = P.build_lgssm(P.to_kernel(E.MODELS[c.d]), i["t"], i["S"], mean=None if i["mean"] is None else P.CustomMean(i["mean"]), device_components=True)
    else:
        tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
        dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    if c.force:
        dm.handle_options.update({L.OPT_SWEEP_CHUNK: c.force[0], L.OPT_SWEEP_WARMUP: c.force[1], L.OPT_SWEEP_WARMUP_BACK: c.force[2]})
    if not sweep:
        dm.handle_options[L.OPT_SWEEP] = 0
    return dm


def bind_on(tgp, hd, dm):
    """binds dm's model on the EXISTING handle hd (tgp_model_set / the SDE entry, as dm.handle() calls them)"""
    L = tgp._lib
    make = L.Handle
    L.Handle = lambda *a, **k: hd
    try:
        assert dm.handle() is hd
    finally:
        L.Handle = make
    return dm


def yin(c):
    """NaN == missing; from 65536 steps on the mask itself (the mirror sends so long a host series unscanned to the stationary-gain engine first and
    finds its NaNs from the NaN that comes back: one more kernel in the profile)"""
    i = E.inputs(c)
    if i["mk"] is None:
        return i["y"]
    return (np.where(i["mk"], 0.0, i["y"]), i["mk"]) if c.T >= 1 << 16 else np.where(i["mk"], np.nan, i["y"])


def call(tgp, dm, c, post):
    """one logpdf / posterior call with the profile on: (values, tgp_sweep_info, kernel names)"""
    fn = (lambda: tgp.logpdf_and_posterior_marginals(dm, yin(c), E.inputs(c)["Rn"])) if post else (lambda: (tgp.logpdf(dm, yin(c)),))
    out, kn = U.kernels_of(tgp, dm, fn)
    return out, dm.handle().sweep_info(), kn


def at_the_bars(c, out):
    lp, pm, pv = E.reference(c)
    assert abs(out[0] - lp) <= 1e-10 * abs(lp), (out[0], lp)
    if len(out) > 1:
        assert np.abs(out[1] - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max())
        assert np.abs(out[2] - pv).max() <= 1e-8 * max(1.0, pv.max())


def kname(c, post):
    return "k_sweep<%s,%s>" % ("sde" if c.sde else "lti", "posterior" if post else "logpdf")


def as_the_host(c, post, info, kn, h=None, values=None):
    """tgp_sweep_info and the profile against the host's account of the call (h: E.host(c, post) unless given)"""
    h = E.host(c, post) if h is None else h
    print(c.name, "posterior" if post else "logpdf", "device", info, "host", h["tries"], h["why"])
    got = {k: info[k] for k in ("served", "C", "W", "Wb", "waves", "attempts", "status", "state")}
    assert got == {k: h[k] for k in got}, (got, h["tries"], h["why"])
    if h["served"]:
        assert kn == {kname(c, post)}, kn
        assert info["dist_f"] <= E.TOL_F and info["dist_b"] <= E.TOL_B, info
    else:
        assert (kname(c, post) in kn) == (h["attempts"] > 0), kn
    if values is not None:
        at_the_bars(c, values)


def check_k(tgp, c):
    """the case's logpdf call and its posterior call, each on a fresh handle, against the table, the host and the oracle"""
    for post, want in ((False, c.lp), (True, c.post)):
        if want is None:
            continue
        dm = device_model(tgp, c)
        out, info, kn = call(tgp, dm, c, post)
        assert (info["served"], info["status"], info["attempts"]) == want, info
        as_the_host(c, post, info, kn, values=out)
        if c.force is None and info["served"] and info["attempts"] > 1:
            # the bound model remembers the warm-ups it needed: the same call again is served at once, with them
            out2, info2, _ = call(tgp, dm, c, post)
            assert (info2["served"], info2["attempts"]) == (1, 1) and (info2["W"], info2["Wb"]) == (info["W"], info["Wb"]), info2
            at_the_bars(c, out2)


def check_draw(tgp, c):
    i, h = E.inputs(c), E.host(c)
    dm = device_model(tgp, c)
    rc, out, info, kn = draw_call(tgp, dm, i["y"], i["mk"], i["Rn"], i["eps"])
    print(c.name, "device", rc, info, "host", h.get("tries"), h["status"])
    assert rc == 0 and (info["served"], info["status"], info["attempts"]) == c.draw, (rc, info)
    assert (info["C"], info["W"], info["Wb"], info["waves"]) == (h["C"], h["W"], h["Wd"], h["nwaves"]), (info, h["C"], h["W"], h["Wd"])
    assert kn == {"k_sweep_draw<%s>" % ("sde" if c.sde else "lti")}, kn
    assert info["dist_f"] <= E.TOL_F and info["dist_b"] <= E.TOL_B, info
    assert err(out, E.draw_reference(c)) <= BAR
    return dm, info


# ------------------------------------------------------------------------------------------------------------ A: every instantiation
@pytest.mark.parametrize("name", names("A"))
def test_every_instantiation(tgp, name):
    check_k(tgp, E.BY_NAME[name])


@pytest.mark.parametrize("name", names("A", "draw"))
def test_every_draw_instantiation(tgp, name):
    check_draw(tgp, E.BY_NAME[name])


# ------------------------------------------------------------------------------------------------------------ B: geometry
@pytest.mark.parametrize("name", names("B"))
def test_forced_geometry(tgp, name):
    c = E.BY_NAME[name]
    check_k(tgp, c)
    nchunks = -(-c.T // c.force[0])
    assert E.host(c)["waves"] == -(-nchunks // 62)


@pytest.mark.parametrize("name", names("B", "draw"))
def test_forced_geometry_of_a_draw(tgp, name):
    check_draw(tgp, E.BY_NAME[name])


@pytest.mark.parametrize("T, served", [(8 * 62, 0), (2047, 0), (2048, 1)])
def test_the_shortest_series_the_engine_takes(tgp, T, served):
    """kMinT = 2048: 62 chunks of 8 and 2047 steps stay on the general engine (no launch), 2048 steps are served at (8, 8, 8)"""
    c = E.case("B-min-d3-T2048", "B", 3, T, fast=True, force=(8, 8, 8))
    out, info, kn = call(tgp, device_model(tgp, c), c, True)
    if served:
        as_the_host(c, True, info, kn, values=out)
        assert (info["C"], info["W"], info["Wb"], info["waves"], info["attempts"]) == (8, 8, 8, 5, 1), info
    else:      # the engine is not asked: no launch, an empty record, the state untouched
        assert not any(n.startswith("k_sweep") for n in kn), kn
        assert {k: info[k] for k in ("served", "C", "W", "Wb", "waves", "attempts", "status", "state")} == dict.fromkeys(
            ("served", "C", "W", "Wb", "waves", "attempts", "status", "state"), 0), info
        at_the_bars(c, out)


# ------------------------------------------------------------------------------------------------------------ C: long gaps, repair, declines
@pytest.mark.parametrize("name", [n for n in names("C") if n != "C-decline-plan-d2"])
def test_long_gaps_at_a_chunk_boundary(tgp, name):
    """short geometry: declined with the status bits the host predicts, the general engine's values at the bars; long geometry: served at once; default
    options: served after as many attempts as the host predicts, with its W / Wb, and at once the second time"""
    check_k(tgp, E.BY_NAME[name])


@pytest.mark.parametrize("lift", ["bound again", "option 14", "option 15"])
def test_a_decline_by_the_plan_switches_the_engine_off_until_the_model_is_bound_again(tgp, lift):
    c = E.BY_NAME["C-decline-plan-d2"]
    dm = device_model(tgp, c)
    out, info, kn = call(tgp, dm, c, False)
    assert (info["served"], info["status"], info["attempts"], info["state"]) == (0, 1, 2, -1), info
    as_the_host(c, False, info, kn, values=out)
    # the engine stays off for the bound model: the posterior call of the same series -- which a fresh handle serves -- is not tried
    out, info, kn = call(tgp, dm, c, True)
    assert (info["served"], info["C"], info["attempts"], info["status"], info["state"]) == (0, 0, 0, 0, -1), info
    assert not any(n.startswith("k_sweep") for n in kn), kn
    at_the_bars(c, out)
    # the model bound again, or one of the engine's options set: it is back, with nothing remembered
    hd, L = dm.handle(), tgp._lib
    if lift == "bound again":
        dm = bind_on(tgp, hd, device_model(tgp, c))
    elif lift == "option 14":
        hd.set_option(L.OPT_SWEEP, 1)
    else:
        hd.set_option(L.OPT_SWEEP_CHUNK, 0)
    out, info, kn = call(tgp, dm, c, True)
    assert (info["served"], info["status"], info["attempts"]) == c.post, info
    as_the_host(c, True, info, kn, values=out)


@pytest.mark.parametrize("name", names("C", "draw"))
def test_a_draw_repairs_its_own_warm_up(tgp, name):
    """default options: the draw is served at the second attempt and at once the second time.  Wd is remembered apart from Wb: the posterior call that
    follows on the handle starts from the draw's W and its own first guess of Wb"""
    c = E.BY_NAME[name]
    i = E.inputs(c)
    dm, info = check_draw(tgp, c)
    rc, out, info2, _ = draw_call(tgp, dm, i["y"], i["mk"], i["Rn"], i["eps"])
    assert rc == 0 and (info2["served"], info2["attempts"]) == (1, 1) and (info2["W"], info2["Wb"]) == (info["W"], info["Wb"]), info2
    assert err(out, E.draw_reference(c)) <= BAR
    ck = c._replace(what="k", lp=None, post=None, draw=None)
    h = U.sweepsim_served(i["model"], np.where(i["mk"], 0.0, i["y"]), w0=info["W"], wb0=0, missing=i["mk"], Rnew=i["Rn"], num_cu=E.NUM_CU)
    assert h["served"] == 1 and h["attempts"] == 2 and h["tries"][0][2] < info["Wb"] and E.margins_hold(h["tries"]), h["tries"]
    out, kinfo, kn = call(tgp, dm, ck, True)
    as_the_host(ck, True, kinfo, kn, h=h, values=out)


# ------------------------------------------------------------------------------------------------------------ D: ties
@pytest.mark.parametrize("name", names("D"))
def test_ties(tgp, name):
    check_k(tgp, E.BY_NAME[name])


def test_prediction_at_training_inputs(tgp):
    """GP level: mean_and_var(posterior(f(x_tr, 0.1), y)(x_pr)) with x_pr = every third training input (the merged series has a tie at each) and points
    before the first and behind the last one, against the oracle's posterior_marginals"""
    from temporalgps_jl_amd import lti_sde as P
    rng = np.random.default_rng(31)
    k, ntr = E.M52, 1800
    xtr = np.cumsum(rng.uniform(0.05, 0.15, ntr))
    xpr = np.concatenate([xtr[0] - np.array([0.7, 0.3, 0.1]), xtr[::3], xtr[-1] + np.array([0.05, 0.4, 1.1])])
    _, ytr, _ = U.gp_case(k, xtr, 0.1, seed=32)
    pm, pv = oc.posterior_marginals(k, xtr, 0.1, ytr, x_pr=xpr, sigma2_pr=1e-18)
    f = P.to_sde(P.GP(P.to_kernel(k)))
    L, made = tgp._lib, []
    make = L.Handle

    class Recorded(make):      # (the mirror builds the merged model itself: keep the handles it makes, profiled, to ask them who served what)
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_option(L.OPT_PROFILE, 1)
            made.append(self)

    L.Handle = Recorded
    try:
        mean, var = P.mean_and_var(P.posterior(f(xtr, 0.1), ytr)(xpr))
    finally:
        L.Handle = make
    # the merged series (training and prediction inputs sorted: a tie at every third training input) has ntr + len(xpr) = 2406 steps; the training series
    # alone, 1800, is below the engine's minimum of 2048: a handle whose record shows a launch is the merged model's
    assert ntr < 2048 <= ntr + len(xpr)
    records = [(h.sweep_info(), set(h.profile())) for h in made]
    print(records)
    merged = [(i, kn) for i, kn in records if i["attempts"] > 0]
    assert len(merged) == 1, records
    info, kn = merged[0]
    assert (info["served"], info["status"], info["state"]) == (1, 0, 1) and 1 <= info["attempts"] <= 2, info
    assert info["C"] >= info["Wb"] >= 104 and info["W"] >= 112 and info["dist_f"] <= E.TOL_F and info["dist_b"] <= E.TOL_B, info
    assert "k_sweep<sde,posterior>" in kn and not any(n.startswith("k_smooth") or n.startswith("k_apply") for n in kn), kn
    assert np.abs(mean - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max())
    assert np.abs(var - pv).max() <= 1e-8 * max(1.0, pv.max())


# ------------------------------------------------------------------------------------------------------------ E: values that must not be served
def outcome(fn):
    try:
        return ("values",) + tuple(np.asarray(v) for v in fn())
    except Exception as e:      # noqa: BLE001 (the exception IS the outcome that is compared)
        return ("raised", type(e), str(e))


@pytest.mark.parametrize("name", names("E"))
def test_values_that_must_not_be_served(tgp, name):
    """a non-positive innovation variance / a non-finite value: declined with the host's status bits, and the call's outcome is the one TGP_OPT_SWEEP = 0
    gives on a second handle -- the same exception type and message, or the same values"""
    c = E.BY_NAME[name]
    for post, want in ((False, c.lp), (True, c.post)):
        dm, off = device_model(tgp, c), device_model(tgp, c, sweep=0)
        fn = lambda m: (lambda: tgp.logpdf_and_posterior_marginals(m, yin(c), E.inputs(c)["Rn"])) if post else (lambda: (tgp.logpdf(m, yin(c)),))      # noqa: E731
        got, kn = U.kernels_of(tgp, dm, lambda: outcome(fn(dm)))
        info = dm.handle().sweep_info()
        print(name, post, info, got[:3] if got[0] == "raised" else got[1])
        assert (info["served"], info["status"], info["attempts"]) == want and kname(c, post) in kn, (info, kn)
        assert info["state"] == E.host(c, post)["state"] == (-1 if want[1] & 4 else 0), info
        ref_ = outcome(fn(off))
        assert off.handle().sweep_info()["attempts"] == 0
        assert got[0] == ref_[0]
        if got[0] == "raised":
            assert got[1:] == ref_[1:], (got, ref_)
        else:
            for a, b in zip(got[1:], ref_[1:]):
                np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", names("E", "draw"))
def test_a_declined_draw_writes_nothing(tgp, name):
    c = E.BY_NAME[name]
    i = E.inputs(c)
    dm = device_model(tgp, c)
    rc, out, info, kn = draw_call(tgp, dm, i["y"], i["mk"], i["Rn"], i["eps"])
    print(name, rc, info)
    assert rc == tgp._lib.EUNSUPPORTED and np.all(out == SENTINEL), rc
    assert (info["served"], info["status"], info["attempts"]) == c.draw and kn == {"k_sweep_draw<lti>"}, (info, kn)
    assert E.host(c)["status"] == info["status"]


# ------------------------------------------------------------------------------------------------------------ F: the engine's own state
def test_one_handle_bound_to_one_model_after_the_other(tgp):
    """d = 1 -> 4 -> 2, then LTI -> SDE -> LTI at d = 3, a posterior call each time: geometry and values as a fresh handle's"""
    seq = ["A-k-d1-lti-xs0", "A-k-d4-lti-xs3", "A-k-d2-lti-xs1", "A-k-d3-lti-xs0", "A-k-d3-sde-xs2", "A-k-d3-lti-xs0"]
    c0 = E.BY_NAME[seq[0]]
    first = device_model(tgp, c0)
    hd, keep = first.handle(), [first]
    for n, name in enumerate(seq):
        c = E.BY_NAME[name]
        dm = first if n == 0 else bind_on(tgp, hd, device_model(tgp, c))
        keep.append(dm)
        out, info, kn = call(tgp, dm, c, True)
        as_the_host(c, True, info, kn, values=out)
        fresh, finfo, _ = call(tgp, device_model(tgp, c), c, True)
        assert {k: info[k] for k in ("C", "W", "Wb", "waves", "attempts")} == {k: finfo[k] for k in ("C", "W", "Wb", "waves", "attempts")}
        assert out[0] == fresh[0] and np.array_equal(out[1], fresh[1]) and np.array_equal(out[2], fresh[2])      # (the same geometry: the same bits)


def test_the_checkpoint_buffer_grows_with_the_chunk(tgp):
    """a posterior call at C = 64, then at C = 2048 on the same handle: the checkpoints of a wave are C / B states per lane"""
    small, big = E.BY_NAME["F-ckpt-C64-d3"], E.BY_NAME["F-ckpt-C2048-d3"]
    dm = device_model(tgp, small)
    out, info, kn = call(tgp, dm, small, True)
    as_the_host(small, True, info, kn, values=out)
    dm.handle().set_option(tgp._lib.OPT_SWEEP_CHUNK, 2048)
    out, info, kn = call(tgp, dm, big, True)
    as_the_host(big, True, info, kn, values=out)
    assert info["C"] == 2048 and info["waves"] == 1


def test_the_record_buffer_grows_beyond_2048_waves(tgp):
    """the pinned records are allocated for 2048 waves on first use: a small call, then T = 8 * 62 * 2049 + 3 at (8, 8, 8) -- 2050 waves -- on the same
    handle, logpdf and posterior, against the C restatement"""
    small, big = E.BY_NAME["B-seam-d1-T2480"], E.BY_NAME["F-part-2050-waves-d1"]
    dm = device_model(tgp, small)
    out, info, kn = call(tgp, dm, small, True)
    as_the_host(small, True, info, kn, values=out)
    dm2 = bind_on(tgp, dm.handle(), device_model(tgp, big))
    for post in (False, True):
        out, info, kn = call(tgp, dm2, big, post)
        assert info["waves"] == 2050
        as_the_host(big, post, info, kn, values=out)
