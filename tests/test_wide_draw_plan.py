"""CPU tier: the draw half of the wide-state engine's host plan (csrc/tgp_wide.hip plan_draw through the pure host function tgp_wide_plan_draw of
libtgp_hip.so; 8 < d <= 63) -- the reverse-time transition of lgssm.jl:231-238 at the settled filter covariance -- against the oracle's own
invert_dynamics at the fixed point of the oracle's filter recursion.  The HIP kernel: tests/test_gpu_wide_draw.py.

Bounds: the oracle solves against Pp + 1e-10 I in double precision, so ITS G carries a relative error of the order eps * cond(Pp + 1e-10 I) (2e4 at
d = 9 ... 2.7e9 at d = 42); the plan solves in extended precision.  G is held at 100 eps cond max|G|, L = Pf - G (Pp + 1e-10 I) G' at the same
factor times max|Pf|."""
import ctypes

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref

KERNELS = {
    9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))),
    12: ("product", ("matern32",), ("approx_periodic", 3, 1.0)),
    28: ("product", ("approx_periodic", 7, 1.0), ("matern32",)),
    42: ("product", ("approx_periodic", 7, 1.0), ("matern52",)),
}


def plan_draw(model, T):
    from temporalgps_jl_amd import _lib
    lib = _lib.load()
    d = len(model["x0m"])
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))      # noqa: E731
    A, a, Q = c(model["A"][0].T), c(model["a"][0]), c(model["Q"][0].T)      # column-major blocks
    H, hh, R = c(model["H"][0]), c(np.atleast_1d(model["h"])[:1]), c(np.atleast_1d(model["R"])[:1])
    x0m, x0P = c(model["x0m"]), c(model["x0P"].T)
    info = np.full(6, -7, dtype=np.int64)
    G, L, U = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d))
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert lib.tgp_wide_plan_draw(d, p(A), p(a), p(Q), p(H), p(hh), p(R), p(x0m), p(x0P), T, p(info), p(G), p(L), p(U)) == 0
    return info, G, L, U


@pytest.mark.parametrize("d", sorted(KERNELS))
def test_settled_reverse_time_transition_is_the_oracles_invert_dynamics_at_its_fixed_point(d):
    T = 200_000
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)
    assert len(model["x0m"]) == d
    info, G, L, U = plan_draw(model, T)
    assert info[0] == 0 and 0 < info[1] < 8192 and info[2] == 0 and info[3] > 0 and info[4] >= 1 and info[4] * info[5] >= T - info[1], info
    A, a, Q = model["A"][0], model["a"][0], model["Q"][0]
    H, R = model["H"][0], float(model["R"][0])
    m, P = model["x0m"].copy(), model["x0P"].copy()
    for _ in range(4 * int(info[1])):      # the oracle's filter covariance, iterated well beyond the plan's head
        mp, Pp = ref.predict(m, P, A, a, Q)
        m, P, _ = ref.posterior_and_lml_scalar(mp, Pp, H, 0.0, R, 0.0)
    mp, Pp = ref.predict(m, P, A, a, Q)
    G_ref, _, L_ref = ref.invert_dynamics(m, P, mp, Pp, A)
    factor = 100.0 * 2.220446049250313e-16 * np.linalg.cond(Pp + 1e-10 * np.eye(d))
    eG, eL = np.max(np.abs(G - G_ref)), np.max(np.abs(L - L_ref))
    print(f"d {d}: n0 {info[1]} halo_draw {info[3]} |G - G_ref| {eG:.3e} (bound {factor * np.abs(G_ref).max():.3e}) |L - L_ref| {eL:.3e} (bound {factor * np.abs(P).max():.3e})")
    assert eG <= factor * np.abs(G_ref).max(), (eG, factor)
    assert eL <= factor * np.abs(P).max(), (eL, factor)
    # the noise factor is that of L + 1e-9 I, upper triangular
    assert np.max(np.abs(np.tril(U, -1))) == 0.0
    assert np.max(np.abs(U.T @ U - (L + 1e-9 * np.eye(d)))) <= 1e-13 * max(1.0, np.abs(L).max())
    # G forgets: |G^halo_draw| <= 2^-60 as tested by the plan
    assert np.abs(np.linalg.matrix_power(G, int(info[3]))).sum(axis=1).max() <= 2.0 ** -59


def test_draw_plan_declines_what_the_engine_does_not_serve():
    # ApproxPeriodicKernel() alone: no settled covariance -- the wide plan itself declines, the draw plan is never reached
    model = oc.build_lgssm(("approx_periodic", 7, 1.0), ("regular", 0.0, 0.1, 100_000), 0.1)
    info, _, _, _ = plan_draw(model, 100_000)
    assert info[0] != 0 and info[2] == -1, info
    # fewer than 64 steps behind the head
    model = oc.build_lgssm(KERNELS[28], ("regular", 0.0, 0.1, 120), 0.1)
    info, _, _, _ = plan_draw(model, 120)
    assert info[0] == 4 and info[2] == -1, info
