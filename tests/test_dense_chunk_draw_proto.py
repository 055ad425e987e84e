"""CPU tier: the NumPy restatement of the dense engine's posterior draw (scripts/dense_chunk_draw_proto.py; the kernels are csrc/tgp_dense_draw.hpp) against
the reference restated (ref.posterior_missing + ref.replace_observation_noise_cov + ref.rand) on the same draws, its chunked form against its sequential
form, and -- the one check of the DISTRIBUTION rather than of the same-draws map -- the covariance of the linear map draws -> path against the joint Gaussian.

The GPU tier's bar is 1e-6 of the path's largest value (tests/test_gpu_dense_chunk_draw.py); the prototype has to stand at <= 1e-7 on every case used there.
Measured (largest |difference| over the largest |entry| of the reference path):
    d = 17 / 33, p = 1, T = 600, 10 % missing: 4.3e-16 / 5.7e-16;   p = 3: 5.9e-16;   per-step A, Q with two dt = 0 steps: 1.1e-12 (a tie's predicted
        covariance is the filtering one plus the 1e-10 jitter: its solve amplifies rounding); m_t - m^p_t from the records or from the stored means: the same
    the warm-up form (C = 96, Wd = 64) against the sequential form: <= 7.7e-16, hand-over distance <= 8.0e-15; Wd = 4 fails the check
    M M' + diag(Rnew) against the joint Gaussian's posterior covariance (d = 17, T = 24): 2.2e-9 of its largest entry (the reference's jitters: 1e-9 on
        every reverse-time covariance), the mean 1.7e-11
    zero draws against ref.bryson_frazier_marginals (what the GPU tier's zero-draw tolerance is ten times of): 3.3e-11 (d = 17), 2.0e-11 (d = 64)
    the GPU tier's cases: <= 1.7e-15; its repair case 1.3e-14"""
import importlib.util
import os

import numpy as np
import pytest

from oracle import lgssm_ref as ref
from tests._util import random_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-7


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


proto = _load(os.path.join(ROOT, "scripts", "dense_chunk_draw_proto.py"), "dense_chunk_draw_proto")
gpu = _load(os.path.join(ROOT, "tests", "test_gpu_dense_chunk_draw.py"), "gpu_dense_chunk_draw_cases")


def _case(d, p, T=600, ties=False):
    rng = np.random.default_rng(100 + d + p + ties)
    model, _ = random_model(rng, T, d, p, per_step=ties, rho=0.6)
    if ties:          # the joined-inputs tie of merge_datasets: dt = 0, the state does not move
        for t in (200, 431):
            model["A"][t], model["a"][t], model["Q"][t] = np.eye(d), 0.0, 0.0
    y, mk = rng.standard_normal((T, p)), rng.random((T, p)) < 0.1
    eps = (rng.standard_normal((T, d)), rng.standard_normal((T, p)), rng.standard_normal(d))
    Rn = np.stack([np.diag(r) for r in rng.uniform(0.05, 0.3, size=(T, p))])
    return model, y, mk, Rn, eps


@pytest.mark.parametrize("d,p,ties", ((17, 1, False), (33, 1, False), (33, 3, False), (17, 1, True)))
def test_the_restatement_equals_the_reference_on_the_same_draws(d, p, ties):
    model, y, mk, Rn, eps = _case(d, p, ties=ties)
    want = proto.oracle(model, y, mk, Rn, *eps)
    fwd = proto.forward(model, y, mk)
    seq = proto.draw(model, fwd, Rn, *eps)
    print(d, p, ties, proto.rel(seq["y"], want), proto.rel(proto.draw(model, fwd, Rn, *eps, records=False)["y"], want))
    assert proto.rel(seq["y"], want) <= BAR
    # index conventions: row t of eps_t drives the transition out of step t, row t of eps_e the emission of step t; row 0 of eps_t is never used
    assert proto.rel(proto.draw(model, fwd, Rn, np.roll(eps[0], 1, axis=0), eps[1], eps[2])["y"], want) > 1e-3
    assert proto.rel(proto.draw(model, fwd, Rn, eps[0], np.roll(eps[1], 1, axis=0), eps[2])["y"], want) > 1e-3
    moved = eps[0].copy()
    moved[0] += 1.0
    assert np.array_equal(proto.draw(model, fwd, Rn, moved, eps[1], eps[2])["y"], seq["y"])
    # the warm-up form
    ch = proto.draw(model, fwd, Rn, *eps, C=96, Wd=64)
    print("chunked", proto.rel(ch["y"], seq["y"]), ch["dist"])
    assert ch["chunks"] == 7 and ch["dist"] <= proto.TOL_D and proto.rel(ch["y"], seq["y"]) <= BAR
    short = proto.draw(model, fwd, Rn, *eps, C=96, Wd=4)
    assert short["dist"] > proto.TOL_D


def test_the_map_from_draws_to_path_has_the_posterior_covariance():
    """d = 17, T = 24, p = 1: y* = mu + M eps is linear in the draws; mu and M M' + diag(Rnew) against the joint Gaussian of (states, observations)
    formed directly from the model's blocks.  The difference is the reference's own: 1e-9 / 1e-10 / 1e-12 on its covariances."""
    T, d = 24, 17
    rng = np.random.default_rng(5)
    model, Rd = random_model(rng, T, d, 1, rho=0.6)
    model = dict(model, kind="scalar", H=model["H"][:, 0, :], h=model["h"][:, 0], R=np.ascontiguousarray(Rd[:, 0]))
    y, mk = rng.standard_normal(T), np.zeros(T, dtype=bool)
    mk[[5, 6, 17]] = True
    Rn = rng.uniform(0.05, 0.3, size=T)
    fwd = proto.forward(model, y, mk)
    n = T * d + T + d
    zero = np.zeros(n)
    split = lambda e: (e[:T * d].reshape(T, d), e[T * d:T * d + T], e[T * d + T:])      # noqa: E731
    mu = proto.draw(model, fwd, Rn, *split(zero))["y"]
    M = np.zeros((T, n))
    for k in range(n):
        e = zero.copy()
        e[k] = 1.0
        M[:, k] = proto.draw(model, fwd, Rn, *split(e))["y"] - mu
    cov = M @ M.T
    # the joint Gaussian: x_t = A x_{t-1} + a + q_t, f_t = H x_t + h; condition f on the observed y = f + r
    A, a, Q, H, h = model["A"][0], model["a"][0], model["Q"][0], model["H"][0], float(model["h"][0])
    m, P = model["x0m"], model["x0P"]
    means, covs = [], [[None] * T for _ in range(T)]
    for t in range(T):
        m, P = A @ m + a, A @ P @ A.T + Q
        means.append(m)
        covs[t][t] = P
        for s in range(t):
            covs[t][s] = A @ covs[t - 1][s]
            covs[s][t] = covs[t][s].T
    fm = np.array([H @ mm + h for mm in means])
    K = np.array([[H @ covs[t][s] @ H for s in range(T)] for t in range(T)])
    ob = ~mk
    S = K[np.ix_(ob, ob)] + np.diag(model["R"][ob])
    G = np.linalg.solve(S, K[ob]).T
    pm = fm + G @ (y[ob] - fm[ob])
    pc = K - G @ K[ob] + np.diag(Rn)
    print("mean", np.abs(mu - pm).max() / np.abs(pm).max(), "cov", np.abs(cov - pc).max() / np.abs(pc).max())
    assert np.abs(mu - pm).max() <= 1e-7 * np.abs(pm).max()
    assert np.abs(cov - pc).max() <= 1e-7 * np.abs(pc).max()


def _gpu_cases():
    for d in (17, 32, 33, 48, 49, 64):
        yield f"edge-{d}", lambda d=d: gpu.make_case(1000 + d, gpu.T1, d, 1)
    for which in gpu.BLOCKS:
        yield f"block-{which}", lambda which=which: gpu.block_case(which)
    for d, p in ((33, 3), (17, 16)):
        yield f"vector-{d}-{p}", lambda d=d, p=p: gpu.make_case(5100 + p, gpu.T5, d, p, per_step=True)
    for name, (T, geometry, _) in sorted(gpu.GEOMETRIES.items()):
        yield f"geometry-{name}", lambda T=T, geometry=geometry: gpu.make_case(2000 + T + geometry[0], T, 17, 1)
    for seed in (2100, 3000, 6000):
        yield f"seed-{seed}", lambda seed=seed: gpu.make_case(seed, gpu.T1, 17, 1)


@pytest.mark.parametrize("name,make", list(_gpu_cases()), ids=[n for n, _ in _gpu_cases()])
def test_the_restatement_stands_below_the_bar_on_the_gpu_tiers_cases(name, make):
    model, Rd, y, mk, Rn, eps = make()
    T = model["T"]
    Rr = np.repeat(Rn, T, axis=0) if Rn.shape[0] == 1 and T > 1 else Rn
    want = gpu.restatement(model, y, mk, Rr, eps)
    got = proto.draw(model, proto.forward(model, y, mk), Rr, *eps)["y"]
    print(name, proto.rel(got, want))
    assert proto.rel(got, want) <= BAR


def test_zero_draws_against_the_exact_posterior_mean():
    """what the GPU tier's zero-draw tolerance is made of: the prototype's zero draw against ref.bryson_frazier_marginals, d = 17 ... 64 (measured:
    3.3e-11 and 2.0e-11 of the mean's size -- the reference's 1e-10 jitter on the predicted covariance)"""
    for d in (17, 64):
        model, Rd, y, mk, _, eps = gpu.make_case(1000 + d, gpu.T1, d, 1)
        zero = tuple(np.zeros_like(e) for e in eps)
        Rn = np.array([1e-18])
        mine = proto.draw(model, proto.forward(model, y, mk), Rn, *zero)["y"]
        bf = ref.bryson_frazier_marginals(model, y, Rn, missing=mk)[0]
        print(d, proto.rel(mine, bf))
        assert proto.rel(mine, bf) <= 1e-7


def test_a_missing_stretch_behind_a_boundary_is_repaired_by_doubling():
    """the GPU tier's repair case as run() sees it: first guess 36, 20 chunks of 150; the stretch defeats Wd = 36 and 72 passes"""
    model, Rd, y, Rn, eps = gpu.repair_inputs()
    T = model["T"]
    W0 = proto.first_guess(model)
    C = -(-T // (T // (4 * W0)))
    n = -(-T // C)
    assert (W0, C, n) == (36, 150, 20)
    mk = np.zeros(y.shape, dtype=bool)
    s = (n // 2) * C
    mk[s:s + (5 * W0) // 4] = True
    Rr = np.stack([np.diag(r) for r in Rn])
    r = proto.run(model, y, mk, Rr, eps, C=C, guess=W0)
    print({k: v for k, v in r.items() if k != "y"})
    assert r["served"] == 1 and r["attempts"] == 2 and r["Wd"] == 2 * W0 and r["dist"] <= proto.TOL_D
    assert proto.rel(r["y"], proto.oracle(model, y, mk, Rr, *eps)) <= BAR
    forced = proto.run(model, y, mk, Rr, eps, C=C, Wd=W0)
    assert forced["served"] == 0 and forced["status"] == 2 and proto.rel(forced["y"], r["y"]) <= BAR
