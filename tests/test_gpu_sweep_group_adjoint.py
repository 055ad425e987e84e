"""GPU tier (-m gpu): the adjoint gradient on the group sweep (tgp_logpdf_adjoint_group -> k_sweep_group_adjoint) -- Forward LTI models with
scalar observations and 5 <= d <= 8, with missing steps, a noise variance or an emission offset per step -- through ctypes on the C entry against (a) the
oracle's exact sequential adjoint on gap-free models and (b) the long-double restatement of the adjoint recursion (tests/_sweep_adjoint.py::restated, which
agrees with the oracle to <= 7e-13 of every block at these d).

Bars (tests/_sweep_adjoint.py): logpdf 1e-10 relative; every gradient entry 1e-8 of its block's largest; the per-step gradients 1e-8 of their largest.
Everything runs at T <= 8192, most of it with chunks of 64 steps on a grid where the filter forgets within a chunk: several waves, seams and a partly
filled last wave.  Every served case asserts the return code, tgp_sweep_info's "served" and the profiled kernel name, so that a silent fall-back cannot
pass; every declined one that each output kept its sentinel."""
import functools

import numpy as np
import pytest

from oracle import seq_adjoint
from tests import _sweep_adjoint as SA
from tests import _sweep_group as SG
from tests import _util as U

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
KERNEL = "k_sweep_group_adjoint<lti>"
BLOCK_SHAPES = lambda d: dict(A=(d, d), a=(d,), Q=(d, d), H=(d,), h=(1,), R=(1,), x0m=(d,), x0P=(d, d))      # noqa: E731
C_EDGE, T_EDGE = 64, 4100      # 65 chunks of 64 steps: the last one 4 steps long, the last wave (6 chunks per wave) partly filled
DT_EDGE = 0.5                  # (a grid on which the filter and the adjoint forget within a chunk of 64 steps)


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def _lti(tgp, model, ordering=None, C=0, W=0, Wa=0, **options):
    tr = tgp.GaussMarkovModel(ordering or tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    L = tgp._lib
    dm.handle_options.update({L.OPT_SWEEP_CHUNK: C, L.OPT_SWEEP_WARMUP: W, L.OPT_SWEEP_WARMUP_BACK: Wa})
    dm.handle_options.update({getattr(L, k): v for k, v in options.items()})
    return dm


def adj_call(tgp, dm, y, mk, device=False):
    """tgp_logpdf_adjoint_group through ctypes, every output pre-filled with a sentinel: (return code, lml, g, sweep info, kernel names, raw outputs).
    device: y, the mask and the per-step outputs are torch tensors on the device."""
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
    rc = hd.lib.tgp_logpdf_adjoint_group(hd.h, L.ptr(yy), L.ptr(mm), flags, lml.ctypes.data_as(L._dp), *[L.ptr(g[k]) for k in SA.BLOCKS], L.ptr(hs), L.ptr(Rs))
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
    k, _, s2 = SG.KERNELS[d]
    model, y, _ = U.gp_case(k, ("regular", 0.0, DT_EDGE, T), s2, seed=d)
    return (model, y) + seq_adjoint.logpdf_adjoint(model, y)


@pytest.mark.parametrize("d", [5, 6, 7, 8])
@pytest.mark.parametrize("T", [2048, T_EDGE])
def test_gap_free_series_against_the_sequential_adjoint(tgp, d, T):
    """XS = 0, no mask; T = 2048 is the engine's minimum (32 chunks: 6 waves, the last with 2 chunks), T = 4100 is no multiple of 8 or 64 and its last wave
    is partly filled.  Every block, gx0m / gx0P included (SA.BLOCKS)."""
    model, y, lp, g0 = gap_free_case(d, T)
    assert len(model["x0m"]) == d
    _, info = served(tgp, _lti(tgp, model, C=C_EDGE), y, None, lp, g0, steps=False)
    assert info["C"] == C_EDGE and info["waves"] == -(-(-(-T // C_EDGE)) // 6), info


# ------------------------------------------------------------------------------------------------------------ 2. all 16 instantiations
def edge_mask(T, seed):
    mk = np.random.default_rng(seed).random(T) < 0.1
    mk[630:710] = True         # chunk [640, 704) whole, straddling both its edges
    mk[1030:1036] = True       # the checkpoint-block edge at 1032 (B = 8 and B = 4)
    mk[1276:1284] = True       # a chunk edge (1280) inside a run
    mk[0] = True
    mk[T - 3:] = True
    return mk


@functools.lru_cache(maxsize=None)
def stream_case(d, xs):
    T = T_EDGE
    k, _, s2 = SG.KERNELS[d]
    rng = np.random.default_rng(1000 + 10 * d + xs)
    S = s2 * (0.5 + rng.random(T)) if xs & 1 else s2
    mean = ("custom", lambda v: np.sin(0.3 * np.asarray(v))) if xs & 2 else None
    model, y, _ = U.gp_case(k, ("regular", 0.0, DT_EDGE, T), S, seed=d, mean=mean)
    mk = edge_mask(T, 30 + d)
    return (model, y, mk) + SA.restated(model, y, mk)


@pytest.mark.parametrize("d", [5, 6, 7, 8])
@pytest.mark.parametrize("xs", [0, 1, 2, 3])
def test_mask_noise_and_offset_per_step(tgp, d, xs):
    """k_sweep_group_adjoint<d, xs>: 10 % missing, a run over a whole chunk and both its edges, runs across a checkpoint-block edge and a chunk edge, step 0
    and the last three steps missing; chunks of 64 steps, the adjoint's warm-up as long as the chunk"""
    model, y, mk, lp, want = stream_case(d, xs)
    g, info = served(tgp, _lti(tgp, model, C=C_EDGE), y, mk, lp, want)
    assert info["C"] == C_EDGE and info["waves"] == 11, info
    assert np.all(g["h_steps"][mk] == 0.0) and np.all(g["R_steps"][mk] == 0.0)
    # the sums of the per-step gradients are the block outputs (another order of 4100 additions: T eps = 5e-13 of the sum of magnitudes)
    for k in ("h", "R"):
        assert abs(g[k + "_steps"].sum() - g[k]) <= 1e-12 * np.abs(g[k + "_steps"]).sum(), k


def test_a_shifted_mask_misses_the_bar(tgp):
    """the mutation: the same series with the mask moved by one step differs from the reference beyond the bar -- the mask is read"""
    model, y, mk, lp, want = stream_case(5, 0)
    rc, lml, g, info, _, _ = adj_call(tgp, _lti(tgp, model, C=C_EDGE), y, np.roll(mk, 1))
    assert rc == 0 and info["served"] == 1
    dev = SA.block_deviations(g, want)
    assert max(dev.values()) > 1e3 * SA.GRAD_BAR and abs(lml - lp) > 1e3 * SA.LP_BAR * abs(lp), (dev, lml, lp)


# ------------------------------------------------------------------------------------------------------------ 3. forced geometry, repair
@pytest.mark.parametrize("which", ["Wa", "W"])
def test_a_forced_warm_up_that_is_too_short_is_reported_not_repaired(tgp, which):
    """TGP_OPT_SWEEP_WARMUP_BACK = 8 forces the adjoint's warm-up: bit 2, one launch, every output untouched -- the device gh_steps / gR_steps included;
    TGP_OPT_SWEEP_WARMUP = 8: the same with bit 1"""
    model, y, mk, _, _ = stream_case(5, 0)
    for device in (False, True):
        info, names = declined(tgp, _lti(tgp, model, C=C_EDGE, **{which: 8}), y, mk, device=device)
        assert info["attempts"] == 1 and names == {KERNEL}, (info, names)
        if which == "Wa":
            assert info["status"] & 2 and info["Wb"] == 8 and info["dist_b"] > 1e-10, info
        else:
            assert info["status"] & 1 and info["W"] == 8 and info["dist_f"] > 1e-10, info


def test_sparse_observations_are_repaired_and_remembered_or_handed_over(tgp):
    """one step in sixteen observed (d = 5, T = 8192, default geometry): the filter forgets far more slowly, in steps, than the plan's estimate for a series
    observed at every step.  The repair loop allows two outcomes: served after >= 2 attempts with the warm-ups remembered (the next call takes one launch),
    or -- warm-ups beyond four chunks / still short after four attempts -- declined after >= 1 launch with the engine off for the bound model (the next call
    launches nothing).  The values are checked where served."""
    T = 8192
    k, dt, s2 = SG.KERNELS[5]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=7)
    mk = np.ones(T, dtype=bool)
    mk[::16] = False
    dm = _lti(tgp, model)
    rc, lml, g, info, names, raw = adj_call(tgp, dm, y, mk)
    print(rc, info)
    if rc == 0:
        lp, want = SA.restated(model, y, mk)
        assert info["served"] == 1 and info["attempts"] >= 2 and info["state"] == 1 and info["status"] == 0 and names == {KERNEL}, info
        dev = SA.block_deviations(g, want, SA.BLOCKS + ("h_steps", "R_steps"))
        assert abs(lml - lp) <= SA.LP_BAR * abs(lp) and max(dev.values()) <= SA.GRAD_BAR, (lml, lp, dev)
        _, again = served(tgp, dm, y, mk, lp, want, attempts=1)
        assert (again["C"], again["W"], again["Wb"]) == (info["C"], info["W"], info["Wb"]), (info, again)
    else:
        assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0 and info["state"] == -1 and info["attempts"] >= 1, (rc, info)
        assert not [k for k, v in raw.items() if not np.all(v == SENTINEL)]
        info2, names2 = declined(tgp, dm, y, mk)
        assert info2["attempts"] == 0 and not names2, (info2, names2)


# ------------------------------------------------------------------------------------------------------------ 4. declines
def test_declines_without_a_launch(tgp):
    from temporalgps_jl_amd import lti_sde as P
    L = tgp._lib
    rng = np.random.default_rng(2)
    k5, _, s2 = SG.KERNELS[5]

    def nothing_ran(dm, y):
        info, names = declined(tgp, dm, y, None)
        assert not names and info["attempts"] == 0, (names, info)

    model, y, _ = U.gp_case(("sum", SG.M52, ("matern12",)), ("regular", 0.0, 0.1, 2100), s2, seed=1)      # d = 4
    assert len(model["x0m"]) == 4
    nothing_ran(_lti(tgp, model), y)
    model, y, _ = U.gp_case(("sum", SG.M52, ("stretched", 0.7, SG.M52), ("stretched", 0.5, SG.M52)), ("regular", 0.0, 0.1, 2100), s2, seed=1)      # d = 9
    assert len(model["x0m"]) == 9
    nothing_ran(_lti(tgp, model), y)
    model, y, _ = U.gp_case(k5, ("regular", 0.0, 0.1, 2047), s2, seed=1)                              # T = 2047
    nothing_ran(_lti(tgp, model), y)
    t = np.cumsum(rng.uniform(0.05, 0.15, 2100))                                                      # an SDE-bound model
    sde = P.build_lgssm(P.to_kernel(k5), t, s2, device_components=True)
    assert sde.dim == 5 and isinstance(sde.transitions, tgp.lgssm.SDETransitions)
    nothing_ran(sde, rng.standard_normal(2100))
    modelr = U.random_lgssm(rng, False, 5, 2100, ordering="R")                                        # Reverse ordering
    nothing_ran(_lti(tgp, modelr, tgp.Reverse), rng.standard_normal(2100))
    model, y, _ = U.gp_case(k5, ("regular", 0.0, DT_EDGE, 2100), s2, seed=1)
    nothing_ran(_lti(tgp, model, OPT_SWEEP=0), y)                                                     # TGP_OPT_SWEEP = 0
    nothing_ran(_lti(tgp, model, OPT_CHUNK=16), y)                                                    # an explicit request for the general engine
    lp, g0 = seq_adjoint.logpdf_adjoint(model, y)
    served(tgp, _lti(tgp, model, C=C_EDGE), y, None, lp, g0, steps=False)                             # ... and the same model without them is served


@pytest.mark.parametrize("bad,bits", [("negR", 4), ("inf", 8)])
def test_declines_after_a_launch(tgp, bad, bits):
    """a negative noise variance inside a chunk: an innovation variance that is not positive (bit 4); an infinite observation (bit 8): status reports of the
    engine, the call is declined and writes nothing"""
    model, y, mk, _, _ = stream_case(5, 1)
    mk = mk.copy()
    mk[2148] = False
    if bad == "negR":
        model = dict(model, R=np.where(np.arange(T_EDGE) == 2148, -50.0, model["R"]))
    else:
        y = y.copy()
        y[2148] = np.inf
    info, names = declined(tgp, _lti(tgp, model, C=C_EDGE), y, mk)
    assert info["status"] & bits and info["attempts"] == 1 and names == {KERNEL}, info


# ------------------------------------------------------------------------------------------------------------ 5. bit identity
def test_two_calls_and_host_and_device_inputs_are_bit_identical(tgp):
    model, y, mk, lp, want = stream_case(6, 3)
    dm = _lti(tgp, model, C=C_EDGE)
    _, l1, _, _, _, r1 = adj_call(tgp, dm, y, mk)
    _, l2, _, _, _, r2 = adj_call(tgp, dm, y, mk)
    _, l3, _, i3, _, r3 = adj_call(tgp, dm, y, mk, device=True)
    assert i3["served"] == 1
    for k in r1:
        assert np.array_equal(r1[k], r2[k]) and np.array_equal(r1[k], r3[k]), k


# ------------------------------------------------------------------------------------------------------------ 6. GP level
def _fx(P, d, T, sigma2):
    """d = 5: Matern52 + Matern32, each term with a variance and a length scale of its own (4 parameters and the noise); d = 8: tests/_sweep_group.py's kernel"""
    kern = P.to_kernel(SG.KERNELS[d][0]) if d == 8 else P.KernelSum(P.ScaledKernel(0.8, P.StretchedKernel(1.3, P.Matern52Kernel())),
                                                                    P.ScaledKernel(0.6, P.StretchedKernel(0.9, P.Matern32Kernel())))
    return P.to_sde(P.GP(kern))(P.RegularSpacing(0.0, 0.1, T), sigma2)


@pytest.mark.parametrize("d", [5, 8])
def test_gp_level_missing_data_against_the_tangent_scans_and_differences(tgp, d):
    """logpdf_and_gradient(method="sweep") at d = 5 (Matern52 + Matern32) and d = 8 with NaNs in y: the default geometry, the kernel by its profile name"""
    from temporalgps_jl_amd import lti_sde as P
    T = 3000
    rng = np.random.default_rng(40 + d)
    fx = _fx(P, d, T, 0.1)
    assert fx.build_lgssm().dim == d
    y = rng.standard_normal(T) * 0.8
    y[rng.random(T) < 0.1] = np.nan
    (lp_s, g_s), names = U.kernels_of(tgp, fx.build_lgssm(), lambda: P.logpdf_and_gradient(fx, y, method="sweep"))
    assert fx.build_lgssm().handle().sweep_info()["served"] == 1 and names == {KERNEL}, names
    lp_t, g_t = P.logpdf_and_gradient(fx, y, method="tangent")
    assert abs(lp_s - lp_t) <= 1e-10 * abs(lp_t) and set(g_s) == set(g_t) and "noise" in g_s
    scale = max(abs(v) for v in g_t.values())
    for n in g_t:
        assert abs(g_s[n] - g_t[n]) <= 1e-8 * scale, (n, g_s[n], g_t[n])
    lp_f, g_f = P.logpdf_and_gradient(fx, y, method="fd")      # (good to ~1e-7 by its own docstring)
    scale = max(abs(v) for v in g_f.values())
    for n in g_f:
        assert abs(g_s[n] - g_f[n]) <= 1e-6 * scale, (n, g_s[n], g_f[n])


def test_gp_level_noise_per_observation_against_differences(tgp):
    """one variance per observation had no device gradient at these d: no "noise" entry, the kernel's parameters against central differences"""
    from temporalgps_jl_amd import lti_sde as P
    T = 3000
    rng = np.random.default_rng(50)
    fx = _fx(P, 5, T, 0.1 * (0.5 + rng.random(T)))
    y = rng.standard_normal(T) * 0.8
    lp_s, g_s = P.logpdf_and_gradient(fx, y, method="sweep")
    assert fx.build_lgssm().handle().sweep_info()["served"] == 1
    lp_f, g_f = P.logpdf_and_gradient(fx, y, method="fd")
    assert "noise" not in g_s and set(g_s) == set(g_f)
    assert abs(lp_s - lp_f) <= 1e-10 * abs(lp_f)
    scale = max(abs(v) for v in g_f.values())
    for n in g_f:
        assert abs(g_s[n] - g_f[n]) <= 1e-6 * scale, (n, g_s[n], g_f[n])
