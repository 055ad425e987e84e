"""GPU tier (-m gpu): the adjoint gradient of SDE-described models on the sweep engine (tgp_logpdf_adjoint_sde -> k_sweep_adjoint<sde>) --
Forward models on irregular time stamps with scalar observations and d <= 4, with missing steps, a noise variance or an emission offset per step -- through
ctypes on the C entry against the long-double restatement of the walk (tests/_sweep_adjoint_sde.py; its own parity with the oracle's sequential adjoint and
with central differences: tests/test_sweep_adjoint_sde_ref.py), and at GP level against the tangent scans and central differences of the oracle's logpdf.

Bars (tests/_sweep_adjoint.py's): logpdf 1e-10 relative; every gradient entry 1e-8 of its block's largest; the per-step gradients 1e-8 of their largest.
Every served case asserts the return code, tgp_sweep_info's "served" and the profiled kernel name, so that a silent fall-back cannot pass; every declined
one that each output kept its sentinel.  (p > 1 cannot be bound through tgp_model_set_sde: that decline has no case.)"""
import numpy as np
import pytest

from oracle import components as oc
from tests import _sweep_adjoint_sde as SS
from tests import _util as U

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
KERNEL = "k_sweep_adjoint<sde>"
SHAPES = lambda d: dict(F=(d, d), Pinf=(d, d), A1=(d, d), a=(d,), H=(d,), h=(1,), R=(1,), x0m=(d,), x0P=(d, d))      # noqa: E731
NUM_CU = 256


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _sde(tgp, c, times=None, first=True, ordering=None, force=None, replace_x0=True):
    """the case bound through tgp_model_set_sde (x0P = Pinf there); a prior of the series that is not the stationary one goes in through tgp_model_set_x0"""
    b = c["blocks"]
    d = b["F"].shape[0]
    Ps = b["Pinf"]
    stationary = b["x0P"] is Ps
    A1 = b["A1"] if first else None
    tr = tgp.lgssm.SDETransitions(ordering or tgp.Forward, b["F"], c["times"] if times is None else times,
                                  tgp.Gaussian(b["x0m"] if stationary else np.zeros(d), Ps), A1, None if A1 is None else Ps - A1 @ Ps @ A1.T)
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(b["H"][None], np.atleast_1d(b["h"]), np.atleast_1d(b["R"])), T=len(c["times"]))
    if force is not None:
        L = tgp._lib
        dm.handle_options.update({L.OPT_SWEEP_CHUNK: force[0], L.OPT_SWEEP_WARMUP: force[1], L.OPT_SWEEP_WARMUP_BACK: force[2]})
    if not stationary and replace_x0:
        hd = dm.handle()
        x0m, x0P = np.ascontiguousarray(b["x0m"], dtype=np.float64), np.ascontiguousarray(np.asarray(b["x0P"], dtype=np.float64).T)
        hd.check(hd.lib.tgp_model_set_x0(hd.h, tgp._lib.ptr(x0m), tgp._lib.ptr(x0P)))
    return dm


def adj_call(tgp, dm, y, mk, device=False):
    """tgp_logpdf_adjoint_sde through ctypes, every output pre-filled with a sentinel: (return code, lml, g, sweep info, kernel names, raw outputs)"""
    hd, L = dm.handle(), tgp._lib
    d, T = dm.dim, dm.T
    yy = np.ascontiguousarray(np.where(mk, 0.0, y) if mk is not None else y, dtype=np.float64)
    mm = None if mk is None else np.ascontiguousarray(mk, dtype=np.uint8)
    g = {k: np.full(s, SENTINEL) for k, s in SHAPES(d).items()}
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
    rc = hd.lib.tgp_logpdf_adjoint_sde(hd.h, L.ptr(yy), L.ptr(mm), flags, lml.ctypes.data_as(L._dp), *[L.ptr(g[k]) for k in SS.BLOCKS], L.ptr(hs), L.ptr(Rs))
    names = set(hd.profile())
    hd.set_option(L.OPT_PROFILE, 0)
    if device:
        hs, Rs = hs.cpu().numpy(), Rs.cpu().numpy()
    raw = dict(g, lml=lml, h_steps=hs, R_steps=Rs)
    out = {k: (g[k].T.copy() if k in ("F", "Pinf", "A1", "x0P") else g[k].copy()) for k in SS.BLOCKS}      # column-major blocks -> [i][k]
    out["h"], out["R"] = float(out["h"][0]), float(out["R"][0])
    out["h_steps"], out["R_steps"] = hs, Rs
    return rc, float(lml[0]), out, hd.sweep_info(), names, raw


def served(tgp, dm, c, attempts=1, device=False, mk=None):
    mk = c["missing"] if mk is None else mk
    lp, want = c["lp"], c["g"]
    rc, lml, g, info, names, _ = adj_call(tgp, dm, c["y"], mk, device)
    assert rc == 0 and info["served"] == 1 and info["status"] == 0, (rc, info, dm.handle().lib.tgp_last_error(dm.handle().h))
    assert names == {KERNEL}, names
    assert info["dist_f"] <= 1e-12 and info["dist_b"] <= 1e-11 and info["Wb"] <= info["C"], info
    assert (info["attempts"] == attempts) if isinstance(attempts, int) else attempts(info["attempts"]), info
    dev = SS.block_deviations(g, want, SS.BLOCKS + ("h_steps", "R_steps"))
    print("info %s lml rel %.2e deviations %s" % (info, abs(lml - lp) / abs(lp), {k: f"{v:.1e}" for k, v in dev.items()}))
    assert abs(lml - lp) <= SS.LP_BAR * abs(lp), (lml, lp)
    assert max(dev.values()) <= SS.GRAD_BAR, dev
    assert np.all(g["h_steps"][mk] == 0.0) and np.all(g["R_steps"][mk] == 0.0)
    for k in ("h", "R"):      # (the sums of the per-step gradients are the block outputs: another order of T additions)
        assert abs(g[k + "_steps"].sum() - g[k]) <= 1e-12 * np.abs(g[k + "_steps"]).sum(), k
    return g, info


def declined(tgp, dm, y, mk, device=False):
    rc, _, _, info, names, raw = adj_call(tgp, dm, y, mk, device)
    print("rc %d info %s kernels %s" % (rc, info, sorted(names)))
    assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0, (rc, info)
    touched = [k for k, v in raw.items() if not np.all(v == SENTINEL)]
    assert not touched, touched
    return info, names


# ------------------------------------------------------------------------------------------------------------ 1. every instantiation
C_STREAMS = 256


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("xs", [0, 1, 2, 3])
def test_every_instantiation_at_the_shortest_series(tgp, d, xs):
    """T = 2048, the engine's minimum, the plan's own geometry: 10 % missing, a run [5:9], missing ends, three ties, one gap of 50 typical gaps; x0P = Pinf"""
    served(tgp, _sde(tgp, SS.case(d, 2048, xs=xs)), SS.case(d, 2048, xs=xs), attempts=lambda a: a <= 3)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("xs", [0, 1, 2, 3])
def test_every_instantiation_with_a_replaced_prior(tgp, d, xs):
    """T = 5003 (a last block of three steps), chunks of 256 steps and warm-ups of 256: the same mask with 40 missing steps across the boundary of the second
    and third chunk; x0 replaced through tgp_model_set_x0, so that step 0 runs through P - Pinf != 0: gA1's covariance term and gx0P are exercised"""
    c = SS.case(d, 5003, xs=xs, x0=True, gap_at=2 * C_STREAMS)
    g, _ = served(tgp, _sde(tgp, c, force=(C_STREAMS, 256, 256)), c)
    assert np.abs(g["x0P"]).max() > 0.0 and np.abs(g["A1"]).max() > 0.0


def test_a_component_of_three_beside_one(tgp):
    c = SS.case(4, 2500, xs=1, kernel=("sum", SS.M52, SS.M12))
    served(tgp, _sde(tgp, c), c, attempts=lambda a: a <= 3)


def test_shifted_time_stamps_miss_the_bar(tgp):
    """the mutation: the same series with the gaps moved by one step differs from the reference beyond the bar -- the time stamps are read"""
    c = SS.case(3, 5003, xs=0, x0=True, gap_at=2 * C_STREAMS)
    shifted = np.concatenate([c["times"][:1], c["times"][:-1]])
    rc, lml, g, info, _, _ = adj_call(tgp, _sde(tgp, c, times=shifted, force=(C_STREAMS, 256, 256)), c["y"], c["missing"])
    assert rc == 0 and info["served"] == 1
    dev = SS.block_deviations(g, c["g"])
    assert max(dev.values()) > 1e3 * SS.GRAD_BAR and abs(lml - c["lp"]) > 1e3 * SS.LP_BAR * abs(c["lp"]), (dev, lml, c["lp"])


def test_a_model_bound_without_a_first_transition(tgp):
    """no A1: step 0 takes exp(F 1) by the closed form; the host contracts that step's G_0 into gF and gA1 is zero.  (The prior is replaced: from the
    stationary one with a zero mean G_0 = mb m' + 2 Pb A (P - Pinf) vanishes and the step would leave nothing to see.)"""
    c0 = SS.case(3, 2048, xs=0, x0=True)
    b = dict(c0["blocks"], A1=None)
    lp, want = SS.restated(times=c0["times"], y=c0["y"], missing=c0["missing"], **b)
    c = dict(c0, blocks=b, lp=lp, g=want)
    g, _ = served(tgp, _sde(tgp, c, first=False), c, attempts=lambda a: a <= 3)
    assert np.all(g["A1"] == 0.0)
    assert np.abs(want["F"] - c0["g"]["F"]).max() > 1e3 * SS.GRAD_BAR * np.abs(want["F"]).max()      # (step 0's share of gF is visible at the bar)


# ------------------------------------------------------------------------------------------------------------ 2. chunks of eight steps, wave seams
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [2480, 2481])
def test_chunks_of_eight_steps_across_wave_seams(tgp, d, T):
    """310 and 311 chunks: a wave seam at every 62nd chunk and a last chunk of one step (the fast-forgetting spacing: eight steps are a warm-up)"""
    c = SS.case(d, T, xs=2, fast=True, x0=True)
    _, info = served(tgp, _sde(tgp, c, force=(8, 8, 8)), c)
    assert (info["C"], info["W"], info["Wb"], info["waves"]) == (8, 8, 8, 5 if T == 2480 else 6), info


# ------------------------------------------------------------------------------------------------------------ 3. repair, forced geometry
def _repair_case():
    c = dict(SS.case(3, 4096, xs=0, seed=7))
    kw = dict(times=c["times"], y=c["y"], num_cu=NUM_CU, **c["blocks"])
    C = SS.sim_run(missing=c["missing"], **kw)["C"]      # (the plan's chunk length does not depend on the mask)
    s = (2048 // C) * C
    mk = c["missing"].copy()
    mk[s:s + 200] = True      # 200 missing steps right behind a chunk boundary
    w, wa, tries = 0, 0, []
    for _ in range(4):
        r = SS.sim_run(missing=mk, w_hint=w, wa_hint=wa, **kw)
        tries.append((r["C"], r["W"], r["Wa"], r["status"], float(r["dist_f"]), float(r["dist_a"])))
        if not r["status"] & 3:
            break
        w, wa = (2 * r["W"] if r["status"] & 1 else w), (2 * r["Wa"] if r["status"] & 2 else wa)
    c["missing"] = mk
    c["lp"], c["g"] = SS.restated(times=c["times"], y=c["y"], missing=mk, **c["blocks"])
    return c, tries


def test_a_long_gap_behind_a_chunk_boundary_is_repaired_and_remembered(tgp):
    """default options.  The plan's first guess for the adjoint's warm-up (Wa = C = 104) is short behind 200 missing steps -- 1.7e-8 against the check's
    1e-11 in the host simulation of this very series -- and the call repeats with Wa doubled.  The call is served with a clean status, the bound model
    remembers the warm-ups (the next call takes one launch), and the posterior call's own Wb is not touched by it."""
    c, tries = _repair_case()
    print("host simulation: (C, W, Wa, status, dist_f, dist_a) per attempt", tries)
    assert len(tries) == 2 and tries[0][3] == 2 and tries[1][3] == 0, tries
    assert tries[0][5] >= 10.0 * 1e-11 and tries[1][5] <= 1e-11 / 10.0 and all(t[4] <= 1e-12 / 5.0 for t in tries), tries      # (margins on both sides)
    dm = _sde(tgp, c)
    _, info = served(tgp, dm, c, attempts=2)
    assert (info["C"], info["W"], info["Wb"]) == tries[-1][:3], (info, tries)
    _, again = served(tgp, dm, c, attempts=1)
    assert (again["C"], again["W"], again["Wb"]) == (info["C"], info["W"], info["Wb"]), (info, again)
    yn = np.where(c["missing"], np.nan, c["y"])
    tgp.logpdf_and_posterior_marginals(dm, yn, np.array([0.1]))
    post = dm.handle().sweep_info()
    assert post["served"] == 1 and post["status"] == 0, post
    served(tgp, dm, c, attempts=1)
    tgp.logpdf_and_posterior_marginals(dm, yn, np.array([0.1]))
    post2 = dm.handle().sweep_info()
    assert post2["served"] == 1 and post2["attempts"] == 1 and post2["Wb"] == post["Wb"], (post, post2)


def test_a_forced_adjoint_warm_up_that_is_too_short_is_reported_not_repaired(tgp):
    """TGP_OPT_SWEEP_WARMUP_BACK = 8 on a slowly mixing model: bit 2, one launch, every output untouched -- the device gh_steps / gR_steps included"""
    c = SS.case(3, 3000, kernel=("stretched", 1.0 / 2.3, SS.M52))
    for device in (False, True):
        info, names = declined(tgp, _sde(tgp, c, force=(0, 0, 8)), c["y"], c["missing"], device=device)
        assert info["status"] & 2 and info["attempts"] == 1 and info["Wb"] == 8 and info["dist_b"] > 1e-10 and names == {KERNEL}, info


# ------------------------------------------------------------------------------------------------------------ 4. declines
def test_declines_without_a_launch(tgp):
    L = tgp._lib
    rng = np.random.default_rng(2)

    def nothing_ran(dm, y):
        info, names = declined(tgp, dm, y, None)
        assert not names and info["attempts"] == 0, (names, info)
        return dm

    c = SS.case(3, 2047)                                                                                   # T = 2047
    nothing_ran(_sde(tgp, c), c["y"])
    t5 = np.cumsum(rng.uniform(0.05, 0.15, 2100))
    F, Pinf, A1, a, H, x0m = SS.gp_blocks(("sum", SS.M52, SS.M32), t5)                                      # d = 5
    c5 = dict(blocks=dict(F=F, Pinf=Pinf, A1=A1, a=a, H=H, h=0.0, R=0.1, x0m=x0m, x0P=Pinf), times=t5)
    assert F.shape[0] == 5
    nothing_ran(_sde(tgp, c5), rng.standard_normal(2100))
    model, y, _ = U.gp_case(SS.M52, ("regular", 0.0, 0.1, 2100), 0.1, seed=1)                              # a model in LTI form
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = nothing_ran(tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=2100), y)
    assert b"tgp_logpdf_adjoint_missing" in dm.handle().lib.tgp_last_error(dm.handle().h)
    c = SS.case(3, 2100)
    nothing_ran(_sde(tgp, c, ordering=tgp.Reverse), c["y"])                                                # Reverse ordering
    for opt in (L.OPT_SWEEP, L.OPT_SDE_CLOSED_FORM):                                                        # TGP_OPT_SWEEP = 0; no closed form
        dm = _sde(tgp, c)
        dm.handle().set_option(opt, 0)
        nothing_ran(dm, c["y"])
        dm.handle().set_option(opt, 1)
        served(tgp, dm, c, attempts=lambda a: a <= 3)


@pytest.mark.parametrize("bad,bits", [("negR", 4), ("inf", 8)])
def test_declines_after_a_launch(tgp, bad, bits):
    """a negative noise variance inside a chunk: an innovation variance that is not positive (bit 4); an infinite observation (bit 8): status reports of the
    engine, the call is declined and writes nothing.  Bit 4 turns the engine off for the bound model: the next call is declined without a launch."""
    c = SS.case(3, 4096, xs=1)
    b, y, mk = dict(c["blocks"]), c["y"].copy(), c["missing"].copy()
    mk[2148] = False
    if bad == "negR":
        b["R"] = np.where(np.arange(4096) == 2148, -50.0, b["R"])
    else:
        y[2148] = np.inf
    dm = _sde(tgp, dict(c, blocks=b), force=(256, 512, 256))
    info, names = declined(tgp, dm, y, mk)
    assert info["status"] & bits and info["attempts"] == 1 and names == {KERNEL}, info
    if bad == "negR":
        info, names = declined(tgp, dm, y, mk)
        assert info["state"] == -1 and info["attempts"] == 0 and not names, (info, names)


# ------------------------------------------------------------------------------------------------------------ 5. bit identity
def test_two_calls_and_host_and_device_inputs_are_bit_identical(tgp):
    c = SS.case(3, 5003, xs=3, x0=True, gap_at=2 * C_STREAMS)
    dm = _sde(tgp, c, force=(C_STREAMS, 256, 256))
    _, l1, _, _, _, r1 = adj_call(tgp, dm, c["y"], c["missing"])
    _, l2, _, _, _, r2 = adj_call(tgp, dm, c["y"], c["missing"])
    _, l3, _, i3, _, r3 = adj_call(tgp, dm, c["y"], c["missing"], device=True)
    assert i3["served"] == 1
    for k in r1:
        assert np.array_equal(r1[k], r2[k]) and np.array_equal(r1[k], r3[k]), k


# ------------------------------------------------------------------------------------------------------------ 6. Python and GP level
def test_lgssm_logpdf_adjoint_sde_with_steps(tgp):
    c = SS.case(2, 2048, xs=3)
    dm = _sde(tgp, c)
    lp, g = tgp.lgssm.logpdf_adjoint_sde(dm, (np.where(c["missing"], 0.0, c["y"]), c["missing"]), per_step=True)
    assert dm.handle().sweep_info()["served"] == 1
    assert abs(lp - c["lp"]) <= SS.LP_BAR * abs(c["lp"])
    dev = SS.block_deviations(g, c["g"], SS.BLOCKS + ("h_steps", "R_steps"))
    assert max(dev.values()) <= SS.GRAD_BAR, dev


GP_CASES = {
    "matern12": (("scaled", 0.8, ("stretched", 1.7, SS.M12)), [0.8, 1.7]),
    "matern32": (("scaled", 0.8, ("stretched", 1.7, SS.M32)), [0.8, 1.7]),
    "matern52": (("scaled", 1.3, ("stretched", 0.9, SS.M52)), [1.3, 0.9]),
    "sum52_12": (("sum", ("scaled", 0.7, ("stretched", 1.4, SS.M52)), ("scaled", 0.5, ("stretched", 2.0, SS.M12))), [0.7, 1.4, 0.5, 2.0]),
    "sum32_32": (("sum", ("scaled", 0.7, ("stretched", 1.4, SS.M32)), ("scaled", 0.5, ("stretched", 0.6, SS.M32))), [0.7, 1.4, 0.5, 0.6]),
}


def _with(k, th):
    """the kernel expression with its (sigma2, s) pairs replaced, in order"""
    it = iter(th)
    def walk(e):      # noqa: E306
        if e[0] == "sum":
            return ("sum",) + tuple(walk(x) for x in e[1:])
        if e[0] == "scaled":
            s2 = next(it)
            return ("scaled", s2, ("stretched", next(it), e[2][2]))
        return e
    return walk(k)


@pytest.mark.parametrize("name", list(GP_CASES))
@pytest.mark.parametrize("variant", ["plain", "const_mean", "noise_per_observation"])
def test_gp_level_against_the_tangent_scans_and_oracle_differences(tgp, name, variant):
    """lti_sde.logpdf_and_gradient(method="sweep") on plain-array inputs with 10 % NaNs, against method="tangent" on the same call and against central
    differences of the oracle's gp_logpdf, at tests/test_gpu_gradient.py::test_gradient_irregular_spacing_vs_oracle_fd's bar: 2e-5 max(1, |fd|); logpdf
    1e-10 relative"""
    from temporalgps_jl_amd import lti_sde as P
    T = 3000
    rng = np.random.default_rng(11)
    t = np.cumsum(rng.uniform(0.05, 0.15, T))
    y = rng.standard_normal(T)
    miss = rng.random(T) < 0.1
    ym = np.where(miss, np.nan, y)
    k0, th0 = GP_CASES[name]
    th0 = list(th0)
    noise = 0.2 + 0.3 * rng.random(T) if variant == "noise_per_observation" else 0.3
    mean = ("const", 0.4) if variant == "const_mean" else None
    names = [n for n, _, _ in P.parameters(P.to_kernel(k0))]
    assert len(names) == len(th0)
    tail = []
    if variant != "noise_per_observation":
        tail.append(("noise", noise))
    if mean is not None:
        tail.append(("mean.c", 0.4))

    def oracle_lp(th, extra):
        s2 = extra.get("noise", noise)
        mn = ("const", extra["mean.c"]) if "mean.c" in extra else mean
        return oc.gp_logpdf(_with(k0, th), t, s2, y, mean=mn, missing=miss)

    gp = P.GP(P.to_kernel(k0)) if mean is None else P.GP(0.4, P.to_kernel(k0))
    fx = P.to_sde(gp)(t, noise)
    lp, g = P.logpdf_and_gradient(fx, ym, method="sweep")
    lp_t, g_t = P.logpdf_and_gradient(fx, ym, method="tangent")
    lp_ref = oracle_lp(th0, {})
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref) and abs(lp - lp_t) <= 1e-10 * abs(lp_t), (lp, lp_t, lp_ref)
    assert set(g) == set(g_t) == set(names) | {n for n, _ in tail}, (sorted(g), sorted(g_t))
    worst = {}
    for n in g:
        assert abs(g[n] - g_t[n]) <= 2e-5 * max(1.0, abs(g_t[n])), (n, g[n], g_t[n])
    for i, n in enumerate(names):
        hstep = 1e-5 * max(1.0, abs(th0[i]))
        tp, tm = list(th0), list(th0)
        tp[i] += hstep
        tm[i] -= hstep
        fd = (oracle_lp(tp, {}) - oracle_lp(tm, {})) / (2 * hstep)
        worst[n] = (abs(g[n] - fd) / max(1.0, abs(fd)), abs(g_t[n] - fd) / max(1.0, abs(fd)))
        assert abs(g[n] - fd) <= 2e-5 * max(1.0, abs(fd)), (n, g[n], fd)
    for n, v in tail:
        hstep = 1e-5 * max(1.0, abs(v))
        fd = (oracle_lp(th0, {n: v + hstep}) - oracle_lp(th0, {n: v - hstep})) / (2 * hstep)
        worst[n] = (abs(g[n] - fd) / max(1.0, abs(fd)), abs(g_t[n] - fd) / max(1.0, abs(fd)))
        assert abs(g[n] - fd) <= 2e-5 * max(1.0, abs(fd)), (n, g[n], fd)
    print("deviation from the oracle's differences (sweep, tangent):", {n: "%.1e %.1e" % v for n, v in worst.items()})


def test_gp_level_runs_the_sde_adjoint_kernel_takes_a_mask_beside_a_device_series_and_is_the_default(tgp, monkeypatch):
    """the kernel behind method="sweep" on plain-array inputs, by name (the route binds a model of its own: the entry it calls is wrapped to profile that
    model's handle); NaNs in a host y and a mask beside a device y give the same bits"""
    import torch
    from temporalgps_jl_amd import lti_sde as P
    T = 3000
    rng = np.random.default_rng(12)
    t = np.cumsum(rng.uniform(0.05, 0.15, T))
    y = rng.standard_normal(T)
    miss = rng.random(T) < 0.1
    fx = P.to_sde(P.GP(P.to_kernel(GP_CASES["matern52"][0])))(t, 0.3)
    seen = []
    entry = P.L.logpdf_adjoint_sde

    def profiled(model, yy, per_step=False):
        hd = model.handle()
        hd.set_option(tgp._lib.OPT_PROFILE, 1)
        hd.profile_reset()
        out = entry(model, yy, per_step)
        seen.append((set(hd.profile()), hd.sweep_info()["served"]))
        return out

    monkeypatch.setattr(P.L, "logpdf_adjoint_sde", profiled)
    want = P.logpdf_and_gradient(fx, np.where(miss, np.nan, y), method="sweep")
    yd = torch.as_tensor(np.where(miss, 0.0, y), device="cuda:0")
    md = torch.as_tensor(miss.astype(np.uint8), device="cuda:0")
    got = P.logpdf_and_gradient(fx, (yd, md), method="sweep")
    assert seen == [({KERNEL}, 1), ({KERNEL}, 1)], seen
    assert got == want
    # the default policy (profiles/sweep_adjoint_sde_time.txt routed it): plain-array inputs at d <= 4 and T >= 2048 take this pass; a rel_step asks for the
    # tangent scans, and a series the engine would decline (T < 2048) keeps them
    assert P.logpdf_and_gradient(fx, np.where(miss, np.nan, y)) == want and len(seen) == 3 and seen[2] == ({KERNEL}, 1), seen
    lp_t, g_t = P.logpdf_and_gradient(fx, np.where(miss, np.nan, y), rel_step=1e-6)
    assert len(seen) == 3 and abs(lp_t - want[0]) <= 1e-10 * abs(want[0]) and set(g_t) == set(want[1])
    fx_short = P.to_sde(P.GP(P.to_kernel(GP_CASES["matern52"][0])))(t[:2000], 0.3)
    assert set(P.logpdf_and_gradient(fx_short, y[:2000])[1]) == set(want[1]) and len(seen) == 3
