"""GPU tier (-m gpu): the adjoint gradient on the tile sweep (tgp_logpdf_adjoint_group at 9 <= d <= 16 -> k_sweep_tile_adjoint) through ctypes on
the C entry, under TGP_OPT_SWEEP = 2, against the long-double recursion (tests/_sweep_adjoint.py restated): logpdf 1e-10 relative, every gradient entry and
per-step gradient 1e-8 of its block's largest.  Every served case asserts the return code, tgp_sweep_info's "served" and "status" and that the profile holds
the one name under which the walk and the sum of its records are launched, so that a silent fall-back cannot pass; every declined one that each output kept
its sentinel.  tests/test_sweep_tile_adjoint_host.py holds the same walk and the hand-overs of the same cases on the CPU."""
import numpy as np
import pytest

from oracle import seq_adjoint
from tests import _sweep_adjoint as SA
from tests import _sweep_tile as ST
from tests import _sweep_tile_adjoint as TA
from tests import _util as U
from tests.test_gpu_sweep_group_adjoint import SENTINEL, _lti, adj_call

pytestmark = pytest.mark.gpu

KERNEL = "k_sweep_tile_adjoint<lti>"


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def served(tgp, dm, y, mk, lp, want, attempts=1, steps=True, device=False):
    rc, lml, g, info, names, raw = adj_call(tgp, dm, y, mk, device)
    assert rc == 0 and info["served"] == 1 and info["status"] == 0, (rc, info, dm.handle().lib.tgp_last_error(dm.handle().h))
    assert names == {KERNEL}, names
    assert info["dist_f"] <= 1e-12 and info["dist_b"] <= 1e-11 and info["attempts"] == attempts, info
    dev = SA.block_deviations(g, want, SA.BLOCKS + (("h_steps", "R_steps") if steps else ()))
    print("info %s lml rel %.2e deviations %s" % (info, abs(lml - lp) / abs(lp), {k: f"{v:.1e}" for k, v in dev.items()}))
    assert abs(lml - lp) <= SA.LP_BAR * abs(lp), (lml, lp)
    assert max(dev.values()) <= SA.GRAD_BAR, dev
    return g, info, raw


def declined(tgp, dm, y, mk):
    rc, _, _, info, names, raw = adj_call(tgp, dm, y, mk)
    print("rc %d info %s kernels %s" % (rc, info, sorted(names)))
    assert rc == tgp._lib.EUNSUPPORTED and info["served"] == 0, (rc, info)
    assert not [k for k, v in raw.items() if not np.all(v == SENTINEL)]
    return info, names


@pytest.mark.parametrize("d,T,xs,C,W,Wa", TA.CASES)
def test_parity_with_the_long_double_recursion(tgp, d, T, xs, C, W, Wa):
    """the four instantiations: d = 9 in forced chunks of 64 steps (33 chunks, a short last one, the most padding), the others in the plan's own geometry"""
    model, y, mk, lp, want = TA.case(d, T, xs)
    dm = _lti(tgp, model, OPT_SWEEP=2, **(dict(C=C, W=W, Wa=Wa) if d == 9 else {}))
    g, info, _ = served(tgp, dm, y, mk, lp, want)
    assert d != 9 or (info["C"], info["W"], info["Wb"], info["waves"]) == (64, 128, 64, 33), info
    assert np.all(g["h_steps"][mk] == 0.0) and np.all(g["R_steps"][mk] == 0.0)


def test_a_gap_free_series_under_an_all_false_mask_against_the_sequential_adjoint(tgp):
    model, y, _, _, _ = ST.case(9, 2053, 0, False)
    lp, g0 = seq_adjoint.logpdf_adjoint(model, y)
    served(tgp, _lti(tgp, model, OPT_SWEEP=2), y, np.zeros(2053, dtype=bool), lp, g0, steps=False)


def test_two_calls_and_host_and_device_inputs_are_bit_identical(tgp):
    model, y, mk, lp, want = TA.case(13, 2053, 3)
    dm = _lti(tgp, model, OPT_SWEEP=2)
    runs = [served(tgp, dm, y, mk, lp, want, device=device)[2] for device in (False, False, True)]
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k], runs[2][k]), k


def test_a_forced_adjoint_warm_up_that_is_too_short_is_reported_not_repaired(tgp):
    model, y, mk, _, _ = TA.case(9, 2053, 0)
    info, names = declined(tgp, _lti(tgp, model, C=64, Wa=8, OPT_SWEEP=2), y, mk)
    assert info["status"] & 2 and info["attempts"] == 1 and info["Wb"] == 8 and info["dist_b"] > 1e-11 and names == {KERNEL}, (info, names)


def test_sparse_observations_are_repaired_and_remembered(tgp):
    """one step in eight observed (d = 9, T = 4096): slower forgetting than the plan's estimate for a series observed at every step"""
    model, y, _, _, _ = ST.case(9, 4096, 0, False)
    mk = np.ones(4096, dtype=bool)
    mk[::8] = False
    lp, want = SA.restated(model, y, mk)
    dm = _lti(tgp, model, OPT_SWEEP=2)
    rc, _, _, first, names, _ = adj_call(tgp, dm, y, mk)
    assert rc == 0 and first["served"] == 1 and first["attempts"] >= 2 and first["state"] == 1 and names == {KERNEL}, (rc, first, names)
    _, again, _ = served(tgp, dm, y, mk, lp, want, attempts=1)
    assert (again["C"], again["W"], again["Wb"]) == (first["C"], first["W"], first["Wb"]), (first, again)


@pytest.mark.parametrize("what", ["default_option", "d17", "T2047", "reverse", "sde", "no_mask_one_noise"])
def test_declines_without_a_launch(tgp, what):
    from temporalgps_jl_amd import lti_sde as P
    rng = np.random.default_rng(4)
    T = 2047 if what == "T2047" else 2048
    model, y, mk, _, _ = ST.case(17 if what == "d17" else 9, T)
    if what == "reverse":
        dm, y = _lti(tgp, U.random_lgssm(rng, False, 9, T, ordering="R"), tgp.Reverse, OPT_SWEEP=2), rng.standard_normal(T)
    elif what == "sde":      # (tgp_model_set_sde binds d <= 8 only: the widest SDE-bound model there is, under the tile sweep's option)
        dm = P.build_lgssm(P.to_kernel(ST.KERNELS[8]), np.cumsum(rng.uniform(0.1, 0.3, T)), 0.1, device_components=True)
        dm.handle_options[tgp._lib.OPT_SWEEP] = 2
        assert dm.dim == 8 and isinstance(dm.transitions, tgp.lgssm.SDETransitions)
    else:
        dm = _lti(tgp, model, OPT_SWEEP=1 if what == "default_option" else 2)
    info, names = declined(tgp, dm, y, None if what == "no_mask_one_noise" else mk)
    assert not names and info["attempts"] == 0, (names, info)


def test_gp_level_product_kernel_with_nans(tgp):
    """logpdf_and_gradient(method="sweep") for Matern52 * stretched Matern52 (d = 9) with NaNs in y, TGP_OPT_SWEEP = 2 on the bound model, against the
    recursion's block gradients contracted with the exact block tangents"""
    from temporalgps_jl_amd import lti_sde as P
    model, y, mk, lp, want = TA.case(9, 2053, 0)
    fx = P.to_sde(P.GP(P.to_kernel(ST.KERNELS[9])))(P.RegularSpacing(0.0, ST.DT, 2053), 0.1)
    dm = fx.build_lgssm()
    dm.handle().set_option(tgp._lib.OPT_SWEEP, 2)
    (lp_s, g_s), names = U.kernels_of(tgp, dm, lambda: P.logpdf_and_gradient(fx, np.where(mk, np.nan, y), method="sweep"))
    assert dm.handle().sweep_info()["served"] == 1 and names == {KERNEL}, names
    plist = P.parameters(fx.f.f.kernel)
    pnames = [n for n, _, _ in plist] + ["noise"]
    ref = {n: sum(P._contract(want[k], v) for k, v in t.items()) for n, t in zip(pnames, P._shared_block_tangents(fx, pnames, plist))}
    assert abs(lp_s - lp) <= SA.LP_BAR * abs(lp) and set(g_s) == set(ref)
    scale = max(abs(v) for v in ref.values())
    for n in ref:
        assert abs(g_s[n] - ref[n]) <= SA.GRAD_BAR * scale, (n, g_s[n], ref[n])
