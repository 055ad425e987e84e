"""GPU tier (-m gpu): the adjoint gradient of SDE-described models at d = 5 .. 8 on the group sweep (tgp_logpdf_adjoint_group_sde ->
k_sweep_group_adjoint<sde>) through ctypes on the C entry against the long-double restatement of the walk (tests/_sweep_adjoint_sde.py restated,
itself held against the oracle by tests/test_sweep_adjoint_sde_ref.py), and at GP level against central differences of the oracle's logpdf.

Bars (tests/_sweep_adjoint_sde.py): logpdf 1e-10 relative; every gradient block and the per-step gradients 1e-8 of the reference block's largest entry.
Every served case asserts the return code, tgp_sweep_info's "served" and "attempts" and that the profile holds this kernel alone; every declined one that
each output kept its sentinel."""
import numpy as np
import pytest

from oracle import components as oc
from tests import _sweep_adjoint_sde as SS
from tests import _sweep_group as SG
from tests import _sweep_group_sde as GS
from tests import _util as U
from tests.test_gpu_sweep_adjoint_sde import SENTINEL, SHAPES, _sde, _with

pytestmark = pytest.mark.gpu

KERNEL = "k_sweep_group_adjoint<sde>"
STEPS = SS.BLOCKS + ("h_steps", "R_steps")
_CASES = {}


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def case(d, T, xs=0, x0=False, typical=None, first=True, kernel=None, gaps=None):
    """gaps U(0.5, 1.5) typical with two ties and one gap of 50 typical gaps (or `gaps`); 10 % missing with a missing head, a run [5:9] and a missing tail;
    xs bit 0: a noise variance per step, bit 1: an emission offset per step; x0: a prior that is not the stationary one; the reference computed once"""
    key = (d, T, xs, x0, typical, first, kernel, None if gaps is None else gaps.tobytes())
    if key not in _CASES:
        k, dt, s2 = SG.KERNELS.get(d, (kernel, 0.1, 0.1))
        rng = np.random.default_rng(131 * d + 17 * xs + T)
        times = (SS.irregular_times(rng, T, ties=(T // 3, 2 * T // 3), long_gap=T // 2, typical=typical or dt) if gaps is None
                 else np.cumsum(np.concatenate([[0.0], gaps[1:]])))
        F, Pinf, A1, a, H, x0m = SS.gp_blocks(kernel or k, times)
        n = F.shape[0]
        x0P = Pinf
        if x0:
            B = rng.standard_normal((n, n))
            x0m, x0P = x0m + np.linspace(1.0, -2.0, n), 0.3 * Pinf + 0.05 * B @ B.T
        b = dict(F=F, Pinf=Pinf, A1=A1 if first else None, a=a, H=H, h=np.sin(0.3 * times) if xs & 2 else 0.2,
                 R=s2 * (0.5 + rng.random(T)) if xs & 1 else s2, x0m=x0m, x0P=x0P)
        y = SS.draw(times=times, seed=d, **dict(b, A1=A1))
        missing = rng.random(T) < 0.1
        missing[5:9] = True
        missing[0] = missing[T - 1] = True
        lp, g = SS.restated(times=times, y=y, missing=missing, **b)
        _CASES[key] = dict(blocks=b, times=times, y=y, missing=missing, lp=lp, g=g)
    return _CASES[key]


def adj_call(tgp, dm, y, mk, device=False):
    """the C entry with every output pre-filled with a sentinel: (return code, lml, g, sweep info, kernel names, raw outputs)"""
    hd, L = dm.handle(), tgp._lib
    d, T = dm.dim, dm.T
    yy = np.ascontiguousarray(np.where(mk, 0.0, y) if mk is not None else y, dtype=np.float64)
    mm = None if mk is None else np.ascontiguousarray(mk, dtype=np.uint8)
    g = {k: np.full(s, SENTINEL) for k, s in SHAPES(d).items()}
    lml = np.full(1, SENTINEL)
    hs, Rs, flags = np.full(T, SENTINEL), np.full(T, SENTINEL), 0
    if device:
        import torch
        yy, mm, hs, Rs = (None if v is None else torch.as_tensor(v, device="cuda:0") for v in (yy, mm, hs, Rs))
        torch.cuda.synchronize()
        flags = L.IN_DEVICE | L.OUT_DEVICE
    hd.set_option(L.OPT_PROFILE, 1)
    hd.profile_reset()
    rc = hd.lib.tgp_logpdf_adjoint_group_sde(hd.h, L.ptr(yy), L.ptr(mm), flags, lml.ctypes.data_as(L._dp), *[L.ptr(g[k]) for k in SS.BLOCKS], L.ptr(hs), L.ptr(Rs))
    names = set(hd.profile())
    hd.set_option(L.OPT_PROFILE, 0)
    if device:
        hs, Rs = hs.cpu().numpy(), Rs.cpu().numpy()
    raw = dict(g, lml=lml, h_steps=hs, R_steps=Rs)
    out = {k: (g[k].T.copy() if g[k].ndim == 2 else g[k].copy()) for k in SS.BLOCKS}      # column-major blocks -> [i][k]
    out.update(h=float(out["h"][0]), R=float(out["R"][0]), h_steps=hs, R_steps=Rs)
    return rc, float(lml[0]), out, hd.sweep_info(), names, raw


def served(tgp, dm, c, attempts=lambda a: a <= 3, device=False):
    rc, lml, g, info, names, _ = adj_call(tgp, dm, c["y"], c["missing"], device)
    assert rc == 0 and info["served"] == 1 and info["status"] == 0, (rc, info, dm.handle().lib.tgp_last_error(dm.handle().h))
    assert names == {KERNEL} and attempts(info["attempts"]), (names, info)
    assert info["dist_f"] <= 1e-12 and info["dist_b"] <= 1e-11 and info["Wb"] <= info["C"], info
    dev = SS.block_deviations(g, c["g"], STEPS)
    print("info %s lml rel %.2e deviations %s" % (info, abs(lml - c["lp"]) / abs(c["lp"]), {k: f"{v:.1e}" for k, v in dev.items()}))
    assert abs(lml - c["lp"]) <= SS.LP_BAR * abs(c["lp"]), (lml, c["lp"])
    assert max(dev.values()) <= SS.GRAD_BAR, dev
    assert np.all(g["h_steps"][c["missing"]] == 0.0) and np.all(g["R_steps"][c["missing"]] == 0.0)
    return g, info


def declined(tgp, dm, y, mk, device=False):
    rc, _, _, info, names, raw = adj_call(tgp, dm, y, mk, device)
    print("rc %d info %s kernels %s" % (rc, info, sorted(names)))
    assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0, (rc, info)
    touched = [k for k, v in raw.items() if not np.all(v == SENTINEL)]
    assert not touched, touched
    return info, names


@pytest.mark.parametrize("d", [5, 6, 7, 8])
@pytest.mark.parametrize("xs", [0, 1, 2, 3])
def test_every_instantiation_at_the_shortest_series(tgp, d, xs):
    c = case(d, 2048, xs=xs)
    served(tgp, _sde(tgp, c), c)


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_several_waves_with_a_replaced_prior(tgp, d):
    """T = 5003; the prior replaced through tgp_model_set_x0: step 0 runs through x0P - Pinf != 0 and gx0P stands apart from gPinf"""
    c = case(d, 5003, xs=d % 4, x0=True)
    g, info = served(tgp, _sde(tgp, c), c)
    assert info["waves"] > 1 and np.abs(g["x0P"] - g["Pinf"]).max() > 0.0 and np.abs(g["A1"]).max() > 0.0, info


@pytest.mark.parametrize("d", [6, 8])
def test_forced_chunks_of_64_steps_and_a_last_chunk_of_four(tgp, d):
    c = case(d, 4100, xs=1, x0=True, typical=0.5)
    _, info = served(tgp, _sde(tgp, c, force=(64, 0, 64)), c, attempts=lambda a: a == 1)
    assert (info["C"], info["Wb"], info["waves"]) == (64, 64, 11), info


def test_a_model_bound_without_a_first_transition(tgp):
    c = case(5, 2048, x0=True, first=False)
    g, _ = served(tgp, _sde(tgp, c, first=False), c)
    assert np.all(g["A1"] == 0.0)
    assert np.abs(c["g"]["F"] - case(5, 2048, x0=True)["g"]["F"]).max() > 1e3 * SS.GRAD_BAR * np.abs(c["g"]["F"]).max()      # (step 0's share of gF is visible)


def test_a_forced_adjoint_warm_up_that_is_too_short_is_reported_not_repaired(tgp):
    c = case(5, 3000)
    for device in (False, True):
        info, names = declined(tgp, _sde(tgp, c, force=(0, 0, 8)), c["y"], c["missing"], device=device)
        assert info["status"] & 2 and info["attempts"] == 1 and info["Wb"] == 8 and info["dist_b"] > 1e-10 and names == {KERNEL}, info


def test_a_short_warm_up_is_repaired_and_remembered(tgp):
    """tests/_sweep_group_sde.py repair_gaps: a stretch of gaps a few hundred times smaller at a chunk edge of the first guess's geometry"""
    d, T = GS.REPAIR_D, GS.REPAIR_T
    dt = SG.KERNELS[d][1]
    c0 = case(d, T, gaps=GS.repair_gaps(dt, 0, 0, stretched=False))
    _, i0 = served(tgp, _sde(tgp, c0), c0, attempts=lambda a: a == 1)
    c = case(d, T, gaps=GS.repair_gaps(dt, i0["C"], i0["W"]))
    dm = _sde(tgp, c)
    _, info = served(tgp, dm, c, attempts=lambda a: a > 1)
    assert info["Wb"] >= 2 * i0["Wb"], (i0, info)
    _, again = served(tgp, dm, c, attempts=lambda a: a == 1)
    assert (again["C"], again["W"], again["Wb"]) == (info["C"], info["W"], info["Wb"]), (info, again)


def test_declines_without_a_launch(tgp):
    L = tgp._lib

    def nothing_ran(dm, y):
        info, names = declined(tgp, dm, y, None)
        assert not names and info["attempts"] == 0, (names, info)

    c4 = case(4, 2100, kernel=SS.MODELS[4])                                                                # an SDE model at d = 4
    nothing_ran(_sde(tgp, c4), c4["y"])
    model, y, _ = U.gp_case(SG.KERNELS[5][0], ("regular", 0.0, 0.1, 2100), 0.1, seed=1)                    # a model in LTI form at d = 5
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    nothing_ran(tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=2100), y)
    c = case(5, 2047)                                                                                      # T = 2047
    nothing_ran(_sde(tgp, c), c["y"])
    c = case(5, 2048)
    for opt in (L.OPT_SWEEP, L.OPT_SDE_CLOSED_FORM):                                                        # TGP_OPT_SWEEP = 0; no closed form
        dm = _sde(tgp, c)
        dm.handle().set_option(opt, 0)
        nothing_ran(dm, c["y"])


def test_two_calls_and_host_and_device_inputs_are_bit_identical(tgp):
    c = case(7, 5003, xs=3, x0=True)
    dm = _sde(tgp, c)
    runs = [adj_call(tgp, dm, c["y"], c["missing"], device=dev) for dev in (False, False, True)]
    assert all(r[3]["served"] == 1 for r in runs)
    for k in runs[0][5]:
        assert np.array_equal(runs[0][5][k], runs[1][5][k]) and np.array_equal(runs[0][5][k], runs[2][5][k]), k


@pytest.mark.parametrize("variant", ["plain", "const_mean", "noise_per_observation"])
def test_gp_level_against_oracle_differences(tgp, variant, monkeypatch):
    """lti_sde.logpdf_and_gradient(method="sweep"), Matern52 + Matern32 on plain-array inputs with NaNs in y, against central differences (step 1e-4) of the
    oracle's gp_logpdf at DESIGN 4.9's bar, 2e-5 max(1, |fd|); the kernel by its profile name (the route binds a model of its own)"""
    from temporalgps_jl_amd import lti_sde as P
    T, h = 3000, 1e-4
    rng = np.random.default_rng(11)
    t = np.cumsum(rng.uniform(0.05, 0.15, T))
    y = rng.standard_normal(T)
    miss = rng.random(T) < 0.1
    k0 = ("sum", ("scaled", 0.7, ("stretched", 1.4, SG.M52)), ("scaled", 0.5, ("stretched", 2.0, SG.M32)))
    th0 = [0.7, 1.4, 0.5, 2.0]
    noise = 0.2 + 0.3 * rng.random(T) if variant == "noise_per_observation" else 0.3
    c0 = 0.4 if variant == "const_mean" else None
    names = [n for n, _, _ in P.parameters(P.to_kernel(k0))]
    at = dict(zip(names, th0), **({} if variant == "noise_per_observation" else {"noise": 0.3}), **({"mean.c": c0} if c0 is not None else {}))

    def oracle_lp(v):
        return oc.gp_logpdf(_with(k0, [v[n] for n in names]), t, v.get("noise", noise), y, mean=("const", v["mean.c"]) if "mean.c" in v else None, missing=miss)

    seen, entry = [], P.L.logpdf_adjoint_group_sde

    def profiled(model, yy, per_step=False):
        (out, kernels), info = U.kernels_of(tgp, model, lambda: entry(model, yy, per_step)), model.handle().sweep_info()
        seen.append((kernels, info["served"], info["attempts"] <= 3))
        return out

    monkeypatch.setattr(P.L, "logpdf_adjoint_group_sde", profiled)
    gp = P.GP(P.to_kernel(k0)) if c0 is None else P.GP(c0, P.to_kernel(k0))
    lp, g = P.logpdf_and_gradient(P.to_sde(gp)(t, noise), np.where(miss, np.nan, y), method="sweep")
    assert seen == [({KERNEL}, 1, True)], seen
    lp_ref = oracle_lp(at)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref) and set(g) == set(at), (lp, lp_ref, sorted(g))
    for n in at:
        fd = (oracle_lp(dict(at, **{n: at[n] + h})) - oracle_lp(dict(at, **{n: at[n] - h}))) / (2 * h)
        print(n, g[n], fd, abs(g[n] - fd) / max(1.0, abs(fd)))
        assert abs(g[n] - fd) <= 2e-5 * max(1.0, abs(fd)), (n, g[n], fd)
