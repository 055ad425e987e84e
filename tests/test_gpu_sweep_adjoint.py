"""GPU tier (-m gpu): the adjoint gradient on the sweep engine (tgp_logpdf_adjoint_missing -> k_sweep_adjoint) -- Forward LTI models with scalar
observations and d <= 4, with missing steps, a noise variance or an emission offset per step -- through ctypes on the C entry against (a) the oracle's
exact sequential adjoint on gap-free models and (b) the long-double restatement of the adjoint recursion (tests/_sweep_adjoint.py; its own parity with the
oracle and with central differences: tests/test_sweep_adjoint_ref.py).

Bars (tests/test_gpu_adjoint_edges.py's): logpdf 1e-10 relative; every gradient entry 1e-8 of its block's largest; the per-step gradients 1e-8 of their
largest.  Every served case asserts the return code, tgp_sweep_info's "served" and the profiled kernel name, so that a silent fall-back cannot pass; every
declined one that each output kept its sentinel."""
import functools

import numpy as np
import pytest

from oracle import seq_adjoint
from tests import _sweep_adjoint as SA
from tests import _sweep_edges as E
from tests import _util as U
from tests.test_sweep_host import CASES

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
KERNEL = "k_sweep_adjoint<lti>"
BLOCK_SHAPES = lambda d: dict(A=(d, d), a=(d,), Q=(d, d), H=(d,), h=(1,), R=(1,), x0m=(d,), x0P=(d, d))      # noqa: E731


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _lti(tgp, model, ordering=None):
    tr = tgp.GaussMarkovModel(ordering or tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    return tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])


def _force(tgp, dm, C=0, W=0, Wa=0):
    L = tgp._lib
    dm.handle_options.update({L.OPT_SWEEP_CHUNK: C, L.OPT_SWEEP_WARMUP: W, L.OPT_SWEEP_WARMUP_BACK: Wa})
    return dm


def adj_call(tgp, dm, y, mk, device=False):
    """tgp_logpdf_adjoint_missing through ctypes, every output pre-filled with a sentinel: (return code, lml, g, sweep info, kernel names).  device: y, the mask
    and the per-step outputs are torch tensors on the device."""
    hd, L = dm.handle(), tgp._lib
    d, T = dm.dim, dm.T
    yy = np.ascontiguousarray(np.where(mk, 0.0, y) if mk is not None else y, dtype=np.float64)
    mm = None if mk is None else np.ascontiguousarray(mk, dtype=np.uint8)
    g = {k: np.full(s, SENTINEL) for k, s in BLOCK_SHAPES(d).items()}
    lml = np.full(1, SENTINEL)
    flags = 0
    if device:
        import torch
        yy = torch.as_tensor(yy, device="cuda:0")
        mm = None if mm is None else torch.as_tensor(mm, device="cuda:0")
        hs, Rs = (torch.full((T,), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(2))
        torch.cuda.synchronize()
        flags = L.IN_DEVICE | L.OUT_DEVICE
    else:
        hs, Rs = np.full(T, SENTINEL), np.full(T, SENTINEL)
    hd.set_option(L.OPT_PROFILE, 1)
    hd.profile_reset()
    rc = hd.lib.tgp_logpdf_adjoint_missing(hd.h, L.ptr(yy), L.ptr(mm), flags, lml.ctypes.data_as(L._dp), *[L.ptr(g[k]) for k in SA.BLOCKS], L.ptr(hs), L.ptr(Rs))
    names = set(hd.profile())
    hd.set_option(L.OPT_PROFILE, 0)
    if device:
        hs, Rs = hs.cpu().numpy(), Rs.cpu().numpy()
    raw = dict(g, lml=lml, h_steps=hs, R_steps=Rs)
    out = {k: (g[k].T.copy() if k in ("A", "Q", "x0P") else g[k].copy()) for k in SA.BLOCKS}      # column-major blocks -> [i][k]
    out["h"], out["R"] = float(out["h"][0]), float(out["R"][0])
    out["h_steps"], out["R_steps"] = hs, Rs
    return rc, float(lml[0]), out, hd.sweep_info(), names, raw


def served(tgp, dm, y, mk, lp, want, attempts=1, steps=True, device=False):
    rc, lml, g, info, names, _ = adj_call(tgp, dm, y, mk, device)
    assert rc == 0 and info["served"] == 1 and info["status"] == 0, (rc, info, dm.handle().lib.tgp_last_error(dm.handle().h))
    assert names == {KERNEL}, names
    assert info["dist_f"] <= 1e-12 and info["dist_b"] <= 1e-11 and info["Wb"] <= info["C"], info
    assert (info["attempts"] == attempts) if isinstance(attempts, int) else attempts(info["attempts"]), info
    dev = SA.block_deviations(g, want, SA.BLOCKS + (("h_steps", "R_steps") if steps else ()))
    print("info %s lml rel %.2e deviations %s" % (info, abs(lml - lp) / abs(lp), {k: f"{v:.1e}" for k, v in dev.items()}))
    assert abs(lml - lp) <= SA.LP_BAR * abs(lp), (lml, lp)
    assert max(dev.values()) <= SA.GRAD_BAR, dev
    return g, info


def declined(tgp, dm, y, mk, device=False):
    rc, _, _, info, names, raw = adj_call(tgp, dm, y, mk, device)
    print("rc %d info %s kernels %s" % (rc, info, sorted(names)))
    assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0, (rc, info)
    touched = [k for k, v in raw.items() if not np.all(v == SENTINEL)]
    assert not touched, touched
    return info, names


# ------------------------------------------------------------------------------------------------------------ 1. gap-free, against the oracle's adjoint
@functools.lru_cache(maxsize=None)
def gap_free_case(d, T):
    model, y, _ = U.gp_case(E.MODELS[d], ("regular", 0.0, E.WORK_DT[d], T), E.S2, seed=d)
    return (model, y) + seq_adjoint.logpdf_adjoint(model, y)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [2048, 5003])
def test_gap_free_series_against_the_sequential_adjoint(tgp, d, T):
    """XS = 0, no mask; T = 2048 is the engine's minimum, T = 5003 has a last block of three steps and (C = 64 at d <= 2) more than 62 chunks: both hand-overs
    cross waves"""
    model, y, lp, g0 = gap_free_case(d, T)
    _, info = served(tgp, _lti(tgp, model), y, None, lp, g0, attempts=lambda a: a <= 3, steps=False)
    assert T != 5003 or d > 2 or info["waves"] >= 2, info


# ------------------------------------------------------------------------------------------------------------ 2. every stream alone and all at once
T_STREAMS, C_STREAMS = 5003, 256


@functools.lru_cache(maxsize=None)
def stream_case(d, xs):
    T = T_STREAMS
    rng = np.random.default_rng(1000 + 10 * d + xs)
    S = E.S2 * (0.5 + rng.random(T)) if xs & 1 else E.S2
    mean = ("custom", lambda v: np.sin(0.3 * np.asarray(v))) if xs & 2 else None
    model, y, _ = U.gp_case(E.MODELS[d], ("regular", 0.0, E.WORK_DT[d], T), S, seed=d, mean=mean)
    mk = rng.random(T) < 0.1
    mk[5:9] = True
    mk[2 * C_STREAMS - 20:2 * C_STREAMS + 20] = True      # 40 steps across the boundary of the second and third chunk
    mk[0] = mk[T - 1] = True
    return (model, y, mk) + SA.restated(model, y, mk)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("xs", [0, 1, 2, 3])
def test_mask_noise_and_offset_per_step(tgp, d, xs):
    """all 16 instantiations: 10 % missing, a run [5:9], 40 steps across a chunk boundary, the first and the last step missing (chunks of 256 steps, the
    warm-ups 256: the 40-step gap lengthens what a hand-over behind it needs)"""
    model, y, mk, lp, want = stream_case(d, xs)
    g, _ = served(tgp, _force(tgp, _lti(tgp, model), C_STREAMS, 256, 256), y, mk, lp, want)
    assert np.all(g["h_steps"][mk] == 0.0) and np.all(g["R_steps"][mk] == 0.0)
    # the sums of the per-step gradients are the block outputs (another order of 5003 additions: T eps = 6e-13 of the sum of magnitudes)
    for k in ("h", "R"):
        assert abs(g[k + "_steps"].sum() - g[k]) <= 1e-12 * np.abs(g[k + "_steps"]).sum(), k


def test_a_shifted_mask_misses_the_bar(tgp):
    """the mutation: the same series with the mask moved by one step differs from the reference beyond the bar -- the mask is read"""
    model, y, mk, lp, want = stream_case(3, 0)
    rc, lml, g, info, _, _ = adj_call(tgp, _force(tgp, _lti(tgp, model), C_STREAMS, 256, 256), y, np.roll(mk, 1))
    assert rc == 0 and info["served"] == 1
    dev = SA.block_deviations(g, want)
    assert max(dev.values()) > 1e3 * SA.GRAD_BAR and abs(lml - lp) > 1e3 * SA.LP_BAR * abs(lp), (dev, lml, lp)


# ------------------------------------------------------------------------------------------------------------ 3. chunks of eight steps, wave seams
@functools.lru_cache(maxsize=None)
def seam_case(d, T):
    model, y, _ = U.gp_case(E.MODELS[d], ("regular", 0.0, E.FAST_DT[d], T), E.S2, seed=20 + d)
    mk = np.random.default_rng(30 + d).random(T) < 0.1
    return (model, y, mk) + SA.restated(model, y, mk)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [2480, 2481])
def test_chunks_of_eight_steps_across_wave_seams(tgp, d, T):
    """310 and 311 chunks: a wave seam at every 62nd chunk and a last chunk of one step (the fast-forgetting spacing: eight steps are a warm-up)"""
    model, y, mk, lp, want = seam_case(d, T)
    _, info = served(tgp, _force(tgp, _lti(tgp, model), 8, 8, 8), y, mk, lp, want)
    assert (info["C"], info["W"], info["Wb"], info["waves"]) == (8, 8, 8, 5 if T == 2480 else 6), info


# ------------------------------------------------------------------------------------------------------------ 4. repair, forced geometry
@pytest.mark.parametrize("name,gap", [("m32+m12", 350), ("m52", 200)])
def test_long_gaps_behind_a_chunk_boundary_are_repaired_and_remembered(tgp, name, gap):
    """default options, `gap` missing steps right behind a chunk boundary.  Matern-3/2 + Matern-1/2: the plan's first guess (W = 280, Wa = C = 256) holds --
    the prior of this model decays faster over a gap than its closed loop forgets.  Matern-5/2: the first guess (W = 112, Wa = 104) is short -- 2.7e-8
    against the check's 1e-11 in the host simulation of this very series -- and the call repeats with longer warm-ups.  Either way the call is served with a
    clean status, the bound model remembers the warm-ups (the next call takes one launch), and the posterior call's own Wb is not touched by it."""
    k, dt, s2 = CASES[3] if name == "m32+m12" else (E.M52, 0.1, E.S2)
    T = 4096
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=903)
    C = SA.sweepadjsim_run(model, y, num_cu=E.NUM_CU)["C"]      # (the plan's chunk length does not depend on the mask)
    s = (2048 // C) * C
    mk = np.zeros(T, dtype=bool)
    mk[s:s + gap] = True
    host = SA.sweepadjsim_served(model, y, missing=mk, num_cu=E.NUM_CU)
    print("host simulation: (C, W, Wa, status, dist_f, dist_a) per attempt", host["tries"])
    assert host["status"] == 0 and host["attempts"] == (1 if name == "m32+m12" else 2)
    assert all(E.margin_ok(f, E.TOL_F, bool(st & 1)) and E.margin_ok(a, E.TOL_B, bool(st & 2)) for _, _, _, st, f, a in host["tries"]), host["tries"]
    lp, want = SA.restated(model, y, mk)
    dm = _lti(tgp, model)
    _, info = served(tgp, dm, y, mk, lp, want, attempts=host["attempts"])
    assert (info["C"], info["W"], info["Wb"]) == host["tries"][-1][:3], (info, host["tries"])
    _, again = served(tgp, dm, y, mk, lp, want, attempts=1)
    assert (again["C"], again["W"], again["Wb"]) == (info["C"], info["W"], info["Wb"]), (info, again)
    tgp.logpdf_and_posterior_marginals(dm, np.where(mk, np.nan, y), np.array([0.1]))
    post = dm.handle().sweep_info()
    assert post["served"] == 1 and post["status"] == 0, post
    served(tgp, dm, y, mk, lp, want, attempts=1)
    tgp.logpdf_and_posterior_marginals(dm, np.where(mk, np.nan, y), np.array([0.1]))
    post2 = dm.handle().sweep_info()
    assert post2["served"] == 1 and post2["attempts"] == 1 and post2["Wb"] == post["Wb"], (post, post2)


def test_a_forced_adjoint_warm_up_that_is_too_short_is_reported_not_repaired(tgp):
    """TGP_OPT_SWEEP_WARMUP_BACK = 8 on the bench parametrisation: bit 2, one launch, every output untouched -- the device gh_steps / gR_steps included"""
    k, dt, s2 = CASES[5]
    T = 3000
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=3)
    mk = np.random.default_rng(1).random(T) < 0.1
    for device in (False, True):
        info, names = declined(tgp, _force(tgp, _lti(tgp, model), Wa=8), y, mk, device=device)
        assert info["status"] & 2 and info["attempts"] == 1 and info["Wb"] == 8 and info["dist_b"] > 1e-10 and names == {KERNEL}, info


# ------------------------------------------------------------------------------------------------------------ 5. declines
def test_declines_without_a_launch(tgp):
    from temporalgps_jl_amd import lti_sde as P
    L = tgp._lib
    rng = np.random.default_rng(2)

    def nothing_ran(dm, y):
        info, names = declined(tgp, dm, y, None)
        assert not names and info["attempts"] == 0, (names, info)

    model, y, _ = U.gp_case(E.MODELS[3], ("regular", 0.0, 0.1, 2047), E.S2, seed=1)                 # T = 2047
    nothing_ran(_lti(tgp, model), y)
    model5, y5, _ = U.gp_case(("sum", E.M52, E.M32), ("regular", 0.0, 0.1, 2100), E.S2, seed=1)      # d = 5
    assert len(model5["x0m"]) == 5
    nothing_ran(_lti(tgp, model5), y5)
    t = np.cumsum(rng.uniform(0.05, 0.15, 2100))                                                      # an SDE-bound model
    nothing_ran(P.build_lgssm(P.to_kernel(E.M52), t, E.S2, device_components=True), rng.standard_normal(2100))
    modelr = U.random_lgssm(rng, False, 3, 2100, ordering="R")                                        # Reverse ordering
    nothing_ran(_lti(tgp, modelr, tgp.Reverse), rng.standard_normal(2100))
    model, y, _ = U.gp_case(E.MODELS[3], ("regular", 0.0, 0.1, 2100), E.S2, seed=1)                  # TGP_OPT_SWEEP = 0
    dm = _lti(tgp, model)
    dm.handle().set_option(L.OPT_SWEEP, 0)
    nothing_ran(dm, y)
    dm.handle().set_option(L.OPT_SWEEP, 1)
    lp, g0 = seq_adjoint.logpdf_adjoint(model, y)
    served(tgp, dm, y, None, lp, g0, attempts=lambda a: a <= 3, steps=False)


@pytest.mark.parametrize("bad,bits", [("negR", 4), ("inf", 8)])
def test_declines_after_a_launch(tgp, bad, bits):
    """a negative noise variance inside a chunk: an innovation variance that is not positive (bit 4); an infinite observation (bit 8): status reports of the
    engine, the call is declined and writes nothing"""
    T = 4096
    rng = np.random.default_rng(9)
    S = E.S2 * (0.5 + rng.random(T))
    model, y, _ = U.gp_case(E.MODELS[3], ("regular", 0.0, 0.1, T), S, seed=4)
    mk = rng.random(T) < 0.1
    mk[2148] = False
    if bad == "negR":
        model = dict(model, R=np.where(np.arange(T) == 2148, -50.0, model["R"]))
    else:
        y = y.copy()
        y[2148] = np.inf
    info, names = declined(tgp, _force(tgp, _lti(tgp, model), 256, 512, 256), y, mk)
    assert info["status"] & bits and info["attempts"] == 1 and names == {KERNEL}, info


# ------------------------------------------------------------------------------------------------------------ 6. bit identity
def test_two_calls_and_host_and_device_inputs_are_bit_identical(tgp):
    model, y, mk, lp, want = stream_case(3, 3)
    dm = _force(tgp, _lti(tgp, model), C_STREAMS, 256, 256)
    _, l1, _, _, _, r1 = adj_call(tgp, dm, y, mk)
    _, l2, _, _, _, r2 = adj_call(tgp, dm, y, mk)
    _, l3, _, i3, _, r3 = adj_call(tgp, dm, y, mk, device=True)
    assert i3["served"] == 1
    for k in r1:
        assert np.array_equal(r1[k], r2[k]) and np.array_equal(r1[k], r3[k]), k


# ------------------------------------------------------------------------------------------------------------ 7. GP level
def _fx(P, d, T, sigma2, mean=None):
    kern = P.ScaledKernel(0.8, P.StretchedKernel(1.3, {2: P.Matern32Kernel, 3: P.Matern52Kernel}[d]()))
    return P.to_sde(P.GP(kern) if mean is None else P.GP(mean, kern))(P.RegularSpacing(0.0, 0.1, T), sigma2)


@pytest.mark.parametrize("d", [2, 3])
def test_gp_level_missing_data_against_the_tangent_scans(tgp, d):
    from temporalgps_jl_amd import lti_sde as P
    T = 3000
    rng = np.random.default_rng(40 + d)
    fx = _fx(P, d, T, 0.1)
    y = rng.standard_normal(T) * 0.8
    y[rng.random(T) < 0.1] = np.nan
    lp_s, g_s = P.logpdf_and_gradient(fx, y, method="sweep")
    assert fx.build_lgssm().handle().sweep_info()["served"] == 1
    lp_t, g_t = P.logpdf_and_gradient(fx, y, method="tangent")
    assert abs(lp_s - lp_t) <= 1e-10 * abs(lp_t) and set(g_s) == set(g_t) and "noise" in g_s
    scale = max(abs(v) for v in g_t.values())
    for n in g_t:
        assert abs(g_s[n] - g_t[n]) <= 1e-8 * scale, (n, g_s[n], g_t[n])
    with pytest.raises((NotImplementedError, tgp._lib.Unsupported)):      # "adjoint" keeps its meaning
        P.logpdf_and_gradient(fx, y, method="adjoint")


def test_gp_level_noise_per_step_against_differences_and_a_const_mean(tgp):
    from temporalgps_jl_amd import lti_sde as P
    T = 3000
    rng = np.random.default_rng(50)
    S = 0.1 * (0.5 + rng.random(T))
    fx = _fx(P, 3, T, S, mean=P.ConstMean(0.4))
    y = rng.standard_normal(T) * 0.8 + 0.4
    lp_s, g_s = P.logpdf_and_gradient(fx, y, method="sweep")
    assert fx.build_lgssm().handle().sweep_info()["served"] == 1
    lp_f, g_f = P.logpdf_and_gradient(fx, y, method="fd")      # (good to ~1e-7 by its own docstring)
    assert "noise" not in g_s and "mean.c" in g_s and set(g_s) == set(g_f)
    assert abs(lp_s - lp_f) <= 1e-10 * abs(lp_f)
    scale = max(abs(v) for v in g_f.values())
    for n in g_f:
        assert abs(g_s[n] - g_f[n]) <= 1e-6 * scale, (n, g_s[n], g_f[n])
    with pytest.raises((NotImplementedError, tgp._lib.Unsupported)):
        P.logpdf_and_gradient(fx, y, method="adjoint")


def test_the_default_policy_takes_the_sweep_engine_for_these_models(tgp):
    """profiles/sweep_adjoint_time.txt routed it: the default call on a series with missing observations, and on one with a noise variance per observation
    (which had no device gradient before), is the sweep engine's; a series the engine declines (T < 2048) keeps the earlier route"""
    from temporalgps_jl_amd import lti_sde as P
    T = 3000
    rng = np.random.default_rng(60)
    y = rng.standard_normal(T) * 0.8
    ym = y.copy()
    ym[rng.random(T) < 0.1] = np.nan
    for fx, yy in ((_fx(P, 3, T, 0.1), ym), (_fx(P, 2, T, 0.1 * (0.5 + rng.random(T))), y)):
        want = P.logpdf_and_gradient(fx, yy, method="sweep")
        got, names = U.kernels_of(tgp, fx.build_lgssm(), lambda: P.logpdf_and_gradient(fx, yy))
        assert fx.build_lgssm().handle().sweep_info()["served"] == 1 and names == {KERNEL}, names
        assert got == want
    fx = _fx(P, 3, 2000, 0.1)
    got, names = U.kernels_of(tgp, fx.build_lgssm(), lambda: P.logpdf_and_gradient(fx, ym[:2000]))
    assert KERNEL not in names and names and set(got[1]) == {"kernel.sigma2", "kernel.kernel.s", "noise"}, (names, got)
