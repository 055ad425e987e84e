"""CPU tier: the host half of the wide models' adjoint gradient (tgp_adjoint_finish_wide, csrc/tgp_wide_adjoint_host.hpp) on a record that NumPy
builds the way the wide-state engine does -- the head is the n0 + 1 steps up to the settled gain, the sums run over the steps behind it -- against
central differences of the ORACLE's sequential logpdf along random directions in every model block, for products of kernels with 9 <= d <= 60; and, entry
by entry, against the oracle's exact sequential adjoint in long double for every class of the GPU tier's edge tests (9 <= d <= 63)."""
import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref
from oracle import seq_adjoint as sa
from tests import _util as U

KERNELS = {
    9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))),
    12: ("product", ("matern32",), ("approx_periodic", 3, 1.0)),
    28: ("product", ("approx_periodic", 7, 1.3), ("matern32",)),
    42: ("product", ("approx_periodic", 7, 1.3), ("matern52",)),
    60: ("product", ("approx_periodic", 10, 1.3), ("matern52",)),
}
BLOCKS = ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")


def blocks_of(model):
    return dict(A=model["A"][0], a=model["a"][0], Q=model["Q"][0], H=model["H"][0], h=float(model["h"][0]), R=float(model["R"][0]),
                x0m=model["x0m"], x0P=model["x0P"])


def wide_record(model, y, tol=1e-13, max_steps=8192):
    """the record tgp_wide::adjoint hands to the host half (NumPy, sequential): returns (record, head steps, the engine's logpdf)"""
    b = blocks_of(model)
    A, a, Q, h, hh, R, x0m, P = b["A"], b["a"], b["Q"], b["H"], b["h"], b["R"], b["x0m"], b["x0P"].copy()
    d, T = len(x0m), len(y)
    K, S = [], []
    n0 = None
    settled = False
    for t in range(max_steps):
        Pp = A @ P @ A.T + Q
        v = Pp @ h
        s = h @ v + R
        K.append(v / s)
        S.append(s)
        if settled:
            n0 = t
            break
        Pn = Pp - np.outer(v, v) / s
        settled = not np.any(np.abs(Pn - P) > tol * np.abs(Pn).max())
        P = Pn
    assert n0 is not None, "covariance did not settle"
    nh = n0 + 1
    assert nh + 64 <= T
    ix = lambda t: min(t, n0)
    mu = A @ x0m + a
    mus, rs = np.zeros((T, d)), np.zeros(T)
    for t in range(T):
        mus[t] = mu
        rs[t] = y[t] - hh - h @ mu
        mu = A @ mu + a + A @ K[ix(t)] * rs[t]
    kA = A @ K[n0]
    psi = np.zeros(d)
    SA, Sa, Sk, Srm = np.zeros((d, d)), np.zeros(d), np.zeros(d), np.zeros(d)
    Sr = SSQ = 0.0
    for t in range(T - 1, nh - 1, -1):
        SA += np.outer(psi, mus[t])
        Sa += psi
        Sk += psi * rs[t]
        Srm += rs[t] * mus[t]
        Sr += rs[t]
        SSQ += rs[t] ** 2
        rho = -rs[t] / S[n0] + kA @ psi
        psi = A.T @ psi - h * rho
    x0P = model["x0P"]
    packed = np.concatenate([x0m, np.array([x0P[r, c] for c in range(d) for r in range(c + 1)])])
    rec = np.concatenate([SA.reshape(-1), Sa, Sk, Srm, [Sr, SSQ], psi, mus[nh], [n0, 0.0, T, 1.0],
                          A.T.reshape(-1), a, Q.T.reshape(-1), h, [hh, R], packed])
    lp = -0.5 * sum(np.log(2 * np.pi) + np.log(S[ix(t)]) + rs[t] ** 2 / S[ix(t)] for t in range(T))
    return np.ascontiguousarray(rec), nh, lp


def finish_wide(lib, d, rec, y_head, head_steps):
    out = dict(A=np.zeros((d, d)), a=np.zeros(d), Q=np.zeros((d, d)), H=np.zeros(d), h=np.zeros(1), R=np.zeros(1), x0m=np.zeros(d), x0P=np.zeros((d, d)))
    p = lambda x: x.ctypes.data
    rc = lib.tgp_adjoint_finish_wide(d, p(rec), len(rec), p(y_head), len(y_head), head_steps, *[p(out[k]) for k in BLOCKS])
    assert rc == 0, rc
    for k in ("A", "Q", "x0P"):
        out[k] = out[k].T.copy()       # column-major -> [i][k]
    out["h"], out["R"] = float(out["h"][0]), float(out["R"][0])
    return out


def perturbed(model, D, eps):
    m = {k: (np.array(v, dtype=float, copy=True) if isinstance(v, np.ndarray) else v) for k, v in model.items()}
    for k in ("A", "a", "Q", "H"):
        m[k][0] += eps * D[k]
    m["h"][0] += eps * D["h"]
    m["R"][0] += eps * D["R"]
    m["x0m"] += eps * D["x0m"]
    m["x0P"] += eps * D["x0P"]
    return m


def random_direction(rng, model):
    b = blocks_of(model)
    D = {}
    for k in BLOCKS:
        v = np.asarray(b[k], dtype=float)
        # (entry by entry relative to the block: Q of a smooth product kernel spans many orders of magnitude, and a step sized by its largest
        #  entry leaves the central difference's second-order term above the tolerance)
        z = rng.standard_normal(v.shape) * (np.abs(v) + 1e-3 * max(1e-3, np.abs(v).max()))
        if k in ("Q", "x0P"):
            z = 0.5 * (z + z.T)
        D[k] = float(z) if v.ndim == 0 else z
    return D


@pytest.mark.parametrize("d", sorted(KERNELS))
def test_wide_host_half_against_directional_differences_of_the_oracle(d):
    import temporalgps_jl_amd as tgp
    lib = tgp._lib.load()
    rng = np.random.default_rng(70 + d)
    T = 900
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.2, T), 0.1)
    assert model["A"].shape[1] == d
    y = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    rec, nh, lp_engine = wide_record(model, y)
    lp = ref.logpdf(model, y)
    assert abs(lp_engine - lp) <= 1e-10 * abs(lp), (lp_engine, lp)
    g = finish_wide(lib, d, rec, np.ascontiguousarray(y[:nh]), nh)
    eps = 1e-6
    for _ in range(3):
        D = random_direction(rng, model)
        fd = (ref.logpdf(perturbed(model, D, eps), y) - ref.logpdf(perturbed(model, D, -eps), y)) / (2 * eps)
        terms = [np.sum(np.asarray(g[k]) * np.asarray(D[k])) for k in BLOCKS]
        ad, gross = float(sum(terms)), float(sum(abs(t) for t in terms))
        assert abs(ad - fd) <= 2e-6 * max(1.0, abs(fd), gross), (ad, fd, gross)


# --------------------------------------------------------------------------- the algorithm against the exact gradient, entry by entry
def restated_gradient(lib, model, y):
    """wide_record (NumPy) + tgp_adjoint_finish_wide: the gradient the wide-state engine's algorithm gives with no kernel involved -> (logpdf, gradient)"""
    rec, nh, lp = wide_record(model, y)
    return lp, finish_wide(lib, len(model["x0m"]), rec, np.ascontiguousarray(y[:nh]), nh)


@pytest.mark.parametrize("d,dt,T", [(d, dt, U.wide_adjoint_length(d)) for d, dt in U.WIDE_ADJOINT_CLASSES] + U.WIDE_ADJOINT_HOST_EXTRA)
def test_the_algorithm_against_the_exact_sequential_adjoint_entry_by_entry(d, dt, T):
    """What the stationary head and the truncated covariance recursion cost, apart from any kernel: every entry of every block against the oracle's exact
    sequential adjoint in long double (oracle/seq_adjoint.py), for every class of tests/test_gpu_wide_adjoint_edges.py.  Asserted: the plan accepts the class;
    the worst entry stands within 1e-9 of the largest entry of the whole gradient (the GPU tier's 1e-8 keeps a decade); every block stands within ten times the
    figure measured for it (tests/_util.py WIDE_ADJOINT_MEASURED: the worst entry of a block over the block's own largest entry, the largest over the class's
    lengths).  Lengths: wide_adjoint_length(d) for every class, and the GPU tier's lengths at which a class stands farthest (WIDE_ADJOINT_HOST_EXTRA) -- d = 9 at
    spacing 0.1 and T = 524 335 is the nearest to the limit: 8.7e-10 (H: 3.9e-9 of its own block).  Not a class: d = 14 at spacing 0.1 (3.9e-9, x0P 1.5e-7 of its
    own block) and d = 9 at spacing 0.1 and T = 528 425 (1.09e-9): the algorithm's own cost there is outside the 1e-9 that keeps a decade under the GPU tier's 1e-8."""
    import temporalgps_jl_amd as tgp
    lib = tgp._lib.load()
    model = U.wide_adjoint_model(d, dt, T)
    pl = U.wide_plan(model, T)
    assert pl["why"] == 0 and pl["n0"] + 64 <= T, pl
    y = U.wide_adjoint_draw(model, 17)
    lp, g = restated_gradient(lib, model, y)
    lp_ref, g_ref = sa.logpdf_adjoint(model, y)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)
    glob, own = U.gradient_deviations(g, g_ref)
    print(f"d {d} dt {dt} T {T} plan {pl}: global {max(glob.values()):.1e} | own " + " ".join(f"{k} {v:.1e}" for k, v in own.items()))
    assert max(glob.values()) <= 1e-9, (d, dt, glob)
    measured = U.WIDE_ADJOINT_MEASURED[(d, dt)]
    for k in BLOCKS:      # (a figure at rounding level is floored at T 2^-53: sums of T fp64 terms in another order differ by that much)
        assert own[k] <= 10.0 * max(measured[k], T * 2.0 ** -53), (d, dt, k, own[k], measured[k])


def test_wide_host_half_refuses_records_that_do_not_fit():
    import temporalgps_jl_amd as tgp
    lib = tgp._lib.load()
    d = 12
    n = 3 * d * d + 8 * d + 8 + d * (d + 1) // 2
    rec, yh, z = np.zeros(n), np.zeros(64), np.zeros(d * d)
    p = lambda x: x.ctypes.data
    assert lib.tgp_adjoint_finish_wide(d, p(rec), n, p(yh), 64, 32, *[p(z)] * 8) == tgp._lib.EINVAL       # "applies" word is 0
    assert lib.tgp_adjoint_finish_wide(d, p(rec), n - 1, p(yh), 64, 32, *[p(z)] * 8) == tgp._lib.EINVAL   # wrong length
    assert lib.tgp_adjoint_finish_wide(64, p(rec), n, p(yh), 64, 32, *[p(z)] * 8) == tgp._lib.EINVAL      # d > 63
