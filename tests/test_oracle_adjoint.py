"""CPU tier: the exact sequential adjoint of the oracle (oracle/seq_adjoint.c through oracle/seq_adjoint.py) -- the reverse-mode derivative of
the full sequential recursion of seq_kalman.filter_ with respect to the shared blocks, in long double -- the reference the device's block
gradients are held against at lengths the mpmath oracle cannot reach (tests/test_gpu_adjoint_edges.py).

Measured here (x86-64, 64-bit mantissa), against the 50-digit central differences of oracle/lgssm_mp.py (step 1e-20, every elementary direction
of every block, symmetric pairs for Q and x0P), relative to the largest gradient entry:

    model                          T     long double    double build
    random_lgssm d = 1           100     1.4e-18        1.1e-15
    random_lgssm d = 2           100     4.1e-18        9.2e-16
    random_lgssm d = 3            80     0.0            5.1e-16
    random_lgssm d = 5            70     0.0            4.1e-16
    random_lgssm d = 8            60     4.1e-18        1.1e-15
    Matern-3/2 dt 0.01 noise 10  100     0.0            3.7e-14       (a, h non-zero)

Both sides of that comparison are rounded once to fp64, so it cannot resolve less than 2^-53 = 1.1e-16 of an entry: the measurement is taken as
max(4.1e-18, 2^-53) = 1.1e-16, the asserted bar is that x 100 = 1.1e-14, three decades under the 1e-11 it must not exceed (which in turn is three
decades under the 1e-8 the GPU tests assert with this oracle).

At the GPU tests' lengths (T = 12 000): the long-double and double builds differ by 4.6e-14 (Matern-5/2 dt 0.01, d = 3), 7.9e-15 (random d = 3),
3.2e-13 (Matern-5/2 + stretched Matern-5/2 dt 0.02, d = 6), 7.8e-15 (random d = 6) of the largest entry, against a bar of 1e-9: the double build
would do as a 1e-8 reference at these lengths; the long-double one removes its rounding altogether. (profiles/adjoint_edges_parity.txt keeps the figures.)"""
import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_mp as M
from oracle import seq_adjoint as sa
from oracle import seq_kalman as sk
from tests import _util as U

BLOCKS = ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")
MEASURED_VS_MPMATH = max(4.1e-18, 2.0 ** -53)      # the table above; floored at what an fp64-rounded comparison resolves
BAR_VS_MPMATH = 100 * MEASURED_VS_MPMATH


def _draw(model, seed):
    T, d = model["T"], len(model["x0m"])
    rng = np.random.default_rng(seed)
    return sk.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))


def _slow_matern32(T):
    model = oc.build_lgssm(("matern32",), ("regular", 0.0, 0.01, T), 10.0)
    model["a"] = np.array([[0.3, -0.2]])
    model["h"] = np.array([0.7])
    return model


def _max_dev(g, want):
    scale = max(np.abs(np.asarray(want[k])).max() for k in BLOCKS)
    return max(np.abs(np.asarray(g[k]) - np.asarray(want[k])).max() for k in BLOCKS) / scale


def test_the_reference_arithmetic_has_a_64_bit_mantissa():
    """a platform whose long double is the 53-bit double would make the 'reference' build a copy of the double one: fail loudly"""
    assert sa.mant_dig() >= 64, sa.mant_dig()


def test_the_bar_against_mpmath_is_three_decades_under_the_gpu_tier_bar():
    assert BAR_VS_MPMATH <= 1e-11


@pytest.mark.parametrize("case,T", [("random1", 100), ("random2", 100), ("random3", 80), ("random5", 70), ("random8", 60), ("matern32_slow", 100)])
def test_adjoint_against_50_digit_central_differences_of_every_block_entry(case, T):
    if case.startswith("random"):
        d = int(case[6:])
        model = U.random_lgssm(np.random.default_rng(200 + d), False, d, T)
    else:
        model = _slow_matern32(T)
    y = _draw(model, 5)
    lp_mp, g_mp = M.block_gradient_mp(model, y)
    lp_run = M.run(model, y)["logpdf"]                 # (the gradient's loop is run()'s)
    assert abs(lp_mp - lp_run) <= 1e-15 * abs(lp_run)
    lp, g = sa.logpdf_adjoint(model, y)
    lp_d, g_d = sa.logpdf_adjoint(model, y, use_double=True)
    dev, dev_d = _max_dev(g, g_mp), _max_dev(g_d, g_mp)
    print(f"{case} T={T}: long double {dev:.2e}, double build {dev_d:.2e} of the largest entry (bar {BAR_VS_MPMATH:.1e})")
    assert abs(lp - lp_mp) <= 1e-15 * abs(lp_mp)
    for k in ("Q", "x0P"):
        assert np.array_equal(g[k], g[k].T)            # symmetrised
    assert dev <= BAR_VS_MPMATH, (case, dev)
    assert dev_d <= 1e-11, (case, dev_d)               # (the double build is the same derivation: it too sits far below the GPU tier's bar here)


def _picks(d, rng, n=24):
    """a seeded sample of at least n entries per block (the whole block where it has fewer); upper-triangle pairs for Q and x0P"""
    some = lambda pairs: [pairs[i] for i in sorted(rng.choice(len(pairs), size=min(n, len(pairs)), replace=False))]      # noqa: E731
    full = [(i, k) for i in range(d) for k in range(d)]
    upper = [(i, k) for i in range(d) for k in range(i, d)]
    vec = [(i,) for i in range(d)]
    return dict(A=some(full), a=some(vec), Q=some(upper), H=some(vec), h=[()], R=[()], x0m=some(vec), x0P=some(upper))


@pytest.mark.parametrize("d,T,every_entry", [(9, 25, True), (17, 20, False)])
def test_wide_adjoint_against_50_digit_central_differences(d, T, every_entry):
    """the wide-state engine's models (tests/_util.py WIDE_ADJOINT_KERNELS, spacing 0.2, a and h non-zero) through the same derivation at d > 8: every entry at d = 9;
    at d = 17 (1296 evaluations of 0.14 s for all 648 entries) a seeded sample of 24 entries per block, every entry of a, H, x0m, h and R.  Measured here:
        d = 9  T = 25   long double 1.2e-19   double build 5.1e-16   (every entry)
        d = 17 T = 20   long double 1.8e-19   double build 3.7e-16   (the sample)
    -- below the module's MEASURED_VS_MPMATH, so within BAR_VS_MPMATH as the d <= 8 cases are."""
    model = U.wide_adjoint_model(d, 0.2, T)
    y = _draw(model, 5)
    lp, g = sa.logpdf_adjoint(model, y)
    lp_d, g_d = sa.logpdf_adjoint(model, y, use_double=True)
    if every_entry:
        lp_mp, g_mp = M.block_gradient_mp(model, y)
        assert abs(lp - lp_mp) <= 1e-15 * abs(lp_mp)
        dev, dev_d = _max_dev(g, g_mp), _max_dev(g_d, g_mp)
    else:
        picks = _picks(d, np.random.default_rng(1700 + d))
        assert all(len(picks[k]) >= min(24, np.size(g[k])) for k in ("A", "a", "Q", "H", "x0m", "x0P"))
        want = M.block_gradient_entries_mp(model, y, picks)
        scale = max(np.abs(np.asarray(g[k])).max() for k in BLOCKS)      # (of the long-double gradient: the sample need not hold the largest entry)
        at = lambda gg, k, idx: float(np.asarray(gg[k])[idx]) if idx else float(gg[k])      # noqa: E731
        dev = max(abs(at(g, k, idx) - w) for k in BLOCKS for idx, w in zip(picks[k], want[k])) / scale
        dev_d = max(abs(at(g_d, k, idx) - w) for k in BLOCKS for idx, w in zip(picks[k], want[k])) / scale
    print(f"wide d={d} T={T}: long double {dev:.2e}, double build {dev_d:.2e} of the largest entry (bar {BAR_VS_MPMATH:.1e})")
    for k in ("Q", "x0P"):
        assert np.array_equal(g[k], g[k].T)
    assert dev <= BAR_VS_MPMATH, (d, dev)
    assert dev_d <= 1e-11, (d, dev_d)


@pytest.mark.parametrize("d", [14, 30, 46, 63])
def test_wide_adjoint_long_double_against_double_build(d):
    """T = 2500 at spacing 0.1 (the slower of the two spacings: the longer memory), the Gram kernel's tile-edge dimensions.  Measured here: 3.8e-15 (d = 14),
    3.7e-15 (30), 6.3e-15 (46), 3.9e-15 (63) of the largest entry, against a bar of 1e-9."""
    model = U.wide_adjoint_model(d, 0.1, 2500)
    y = _draw(model, 6)
    lp, g = sa.logpdf_adjoint(model, y)
    lp_ref = sk.logpdf(model, y)
    assert abs(lp - lp_ref) <= 1e-12 * abs(lp_ref)
    lp_d, g_d = sa.logpdf_adjoint(model, y, use_double=True)
    dev = _max_dev(g_d, g)
    print(f"wide d={d} T=2500: long double against double build {dev:.2e} of the largest entry (bar 1e-9)")
    assert dev <= 1e-9, (d, dev)


def test_the_oracle_refuses_a_state_wider_than_its_cap():
    model = U.random_lgssm(np.random.default_rng(1), False, 65, 10)
    with pytest.raises(AssertionError):
        sa.logpdf_adjoint(model, np.zeros(10))


def long_cases():
    """the models of the long checks: a slow and a fast one at d = 3 and d = 6, at the GPU tests' lengths"""
    T = 12_000
    out = {}
    for name, spec, dt, noise in (("matern52_slow_d3", ("matern52",), 0.01, 1.0),
                                  ("sum52_52s_slow_d6", ("sum", ("matern52",), ("stretched", 0.4, ("matern52",))), 0.02, 0.1)):
        model = oc.build_lgssm(spec, ("regular", 0.0, dt, T), noise)
        d = len(model["x0m"])
        model["a"] = 0.01 * np.linspace(-1.0, 1.0, d)[None]
        model["h"] = np.array([0.4])
        out[name] = model
    for d in (3, 6):
        out[f"random_fast_d{d}"] = U.random_lgssm(np.random.default_rng(300 + d), False, d, T)
    return out


@pytest.mark.parametrize("case", ["matern52_slow_d3", "random_fast_d3", "sum52_52s_slow_d6", "random_fast_d6"])
def test_adjoint_at_the_gpu_tests_lengths(case):
    model = long_cases()[case]
    d = len(model["x0m"])
    y = _draw(model, 6)
    lp, g = sa.logpdf_adjoint(model, y)
    lp_ref = sk.logpdf(model, y)
    assert abs(lp - lp_ref) <= 1e-12 * abs(lp_ref)
    lp_d, g_d = sa.logpdf_adjoint(model, y, use_double=True)
    dev = _max_dev(g_d, g)
    print(f"{case}: long double against double build {dev:.2e} of the largest entry (bar 1e-9)")
    assert dev <= 1e-9, (case, dev)
    # the directional derivative against central differences of the sequential logpdf (tests/test_gpu_gradient.py: 2e-6 of the gross sum);
    # every entry's direction in units of that entry, so that a step stays small beside what it moves (the entries of a slow model's Q span
    # ten decades)
    rng = np.random.default_rng(400 + d)
    sym = lambda X: 0.5 * (X + X.T)
    unit = {k: np.abs(np.asarray(model[k][0] if k in ("A", "a", "Q", "H", "h", "R") else model[k])) for k in BLOCKS}
    for trial in range(3):
        dirs = dict(A=rng.standard_normal((d, d)), a=rng.standard_normal(d), Q=sym(rng.standard_normal((d, d))), H=rng.standard_normal(d),
                    h=rng.standard_normal(), R=rng.standard_normal(), x0m=rng.standard_normal(d), x0P=sym(rng.standard_normal((d, d))))
        dirs = {k: v * unit[k] for k, v in dirs.items()}
        dirs["Q"], dirs["x0P"] = sym(dirs["Q"]), sym(dirs["x0P"])
        want = sum(float(np.sum(np.asarray(g[k]) * np.asarray(v))) for k, v in dirs.items())
        gross = sum(float(np.sum(np.abs(np.asarray(g[k]) * np.asarray(v)))) for k, v in dirs.items())
        eps = 1e-6

        def shifted(sgn):
            m = dict(model)
            for k in ("A", "a", "Q", "H"):
                m[k] = model[k] + sgn * eps * dirs[k][None]
            for k in ("h", "R", "x0m", "x0P"):
                m[k] = model[k] + sgn * eps * dirs[k]
            return sk.logpdf(m, y)
        fd = (shifted(1.0) - shifted(-1.0)) / (2 * eps)
        assert abs(want - fd) <= 2e-6 * max(1.0, abs(fd), gross), (trial, want, fd, gross)
