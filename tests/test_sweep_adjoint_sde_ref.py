"""CPU tier: the formulas of the sweep engine's adjoint gradient for SDE-described models, restated in NumPy long double
(tests/_sweep_adjoint_sde.py), against
(a) the oracle's exact sequential adjoint (oracle/seq_adjoint) on equally spaced, gap-free series, where the SDE form is the LTI model of the same blocks:
    sum_t Pb_t = gQ, sum_t G_t = gA - 2 gQ A Pinf (the LTI model's Q = Pinf - A Pinf A' is a block of its own there, here it follows A),
    gPinf = gQ - A' gQ A, and a, H, h, R, x0 as they are -- every entry at 1e-12 of its block's largest;
(b) central differences of ref.logpdf_missing on irregular times (two ties, one gap of 50 typical gaps) with a mask, a noise variance and an emission offset
    per step and a prior that is not the stationary one, the oracle running on per-step blocks rebuilt from the perturbed block, at 1e-6 of the block's
    largest entry (tests/test_sweep_adjoint_ref.py's bar).  The step is 1e-4 of the entry: the oracle takes a missing step as one observed at noise 1e15
    and compensates the volume, ~35 added and removed per missing step, so its logpdf carries ~60 x 35 x 1e-16 ~ 1e-12 of rounding here, 1e-8 of a
    gradient entry behind the division -- and the blocks only step 0 reads (x0m, x0P, A1) have the smallest entries; the truncation term, a sixth of
    step^2 times the third derivative, stays below that;
(c) the host's chain rule alone: random sums over (lam, N1, N2) contracted with the directional derivative of the map F -> coefficients.  The map is a
    polynomial of degree two in F, so a central difference of it is exact to rounding: the bar is 1e-10 of the sum of the contraction's absolute terms."""
import numpy as np
import pytest

from oracle import lgssm_ref as ref
from oracle import seq_adjoint
from tests import _sweep_adjoint as SA
from tests import _sweep_adjoint_sde as SS
from tests import _util as U

M12, M32, M52 = ("matern12",), ("matern32",), ("matern52",)
EQUAL = [(M12, 0.1, 0.1), (M32, 0.1, 0.1), (M52, 0.1, 0.1), (("sum", M32, M12), 0.1, 0.2), (("sum", M32, ("stretched", 0.7, M32)), 0.15, 0.1)]


@pytest.mark.parametrize("i", range(len(EQUAL)))
def test_equal_gaps_against_the_sequential_adjoint(i):
    k, dt, s2 = EQUAL[i]
    T = 600
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, T), s2, seed=i)
    d = len(model["x0m"])
    assert d == (1, 2, 3, 3, 4)[i]
    lp0, g0 = seq_adjoint.logpdf_adjoint(model, y)
    F, H = U.kernel_sde(k)
    A = model["A"][0]
    lp, g = SS.restated(F, model["x0P"], A, np.zeros(d), H, 0.0, s2, model["x0m"], model["x0P"], dt * np.arange(T), y)
    assert abs(lp - lp0) <= 1e-12 * abs(lp0), (lp, lp0)
    gQ = np.asarray(g0["Q"])
    Ps = ref.symmetric(model["x0P"])
    got = dict(A=g["sumG"] + 2.0 * gQ @ A @ Ps, Q=g["sumPb"], a=g["a"], H=g["H"], h=g["h"], R=g["R"], x0m=g["x0m"], x0P=g["x0P"])
    dev = SA.block_deviations(got, g0)
    want = gQ - A.T @ gQ @ A
    dev["Pinf"] = float(np.abs(g["Pinf"] - want).max() / np.abs(gQ).max())      # (the two sums it is the difference of set the scale)
    print(k, {b: f"{v:.1e}" for b, v in dev.items()})
    assert max(dev.values()) <= 1e-12, dev


def irregular_case(k, seed, T=300):
    rng = np.random.default_rng(seed)
    times = SS.irregular_times(rng, T, ties=(57, 201), long_gap=150)
    F, Pinf, A1, a, H, x0m = SS.gp_blocks(k, times)
    d = F.shape[0]
    a = 0.05 * rng.standard_normal(d)
    R = 0.1 * (0.5 + rng.random(T))
    h = np.sin(times)
    x0m = x0m + rng.standard_normal(d)
    B = rng.standard_normal((d, d))
    x0P = 0.3 * Pinf + 0.1 * B @ B.T      # a prior of the series that is not the stationary one
    y = SS.draw(F, Pinf, A1, a, H, h, R, x0m, x0P, times, seed)
    missing = rng.random(T) < 0.2
    missing[120:145] = True
    missing[[40, 200, 57, 150]] = False
    missing[77] = True
    return dict(F=F, Pinf=Pinf, A1=A1, a=a, H=H, h=h, R=R, x0m=x0m, x0P=x0P), times, y, missing


@pytest.mark.parametrize("k", [M52, ("sum", M32, ("stretched", 0.7, M32)), ("sum", M52, M12)], ids=["3", "2+2", "3+1"])
def test_irregular_times_against_central_differences(k):
    blocks, times, y, missing = irregular_case(k, seed=5)
    d = blocks["F"].shape[0]
    lp, g = SS.restated(times=times, y=y, missing=missing, **blocks)
    lp0 = ref.logpdf_missing(SS.oracle_model(times=times, **blocks), y, missing)
    assert abs(lp - lp0) <= 1e-10 * abs(lp0), (lp, lp0)

    def fd(key, idx, sym=False):
        out = []
        x = np.asarray(blocks[key], dtype=np.float64)
        step = 1e-4 * max(abs(float(x[idx])), 0.1)
        for s in (+1.0, -1.0):
            b2 = dict(blocks)
            v = x.copy()
            v[idx] += s * step
            if sym and idx[0] != idx[1]:
                v[idx[1], idx[0]] += s * step
            b2[key] = v
            out.append(ref.logpdf_missing(SS.oracle_model(times=times, **b2), y, missing))
        return (out[0] - out[1]) / (2.0 * step)

    worst = {}
    inside = [(i, j) for S in SS.components_of(blocks["F"]) for i in S for j in S]
    outside = [(i, j) for i in range(d) for j in range(d) if (i, j) not in inside]
    assert all(g["F"][ij] == 0.0 for ij in outside)
    sc = np.abs(g["F"]).max()
    for ij in inside:
        worst["F"] = max(worst.get("F", 0.0), abs(fd("F", ij) - g["F"][ij]) / sc)
    sc = np.abs(g["A1"]).max()
    for i in range(d):
        for j in range(d):
            worst["A1"] = max(worst.get("A1", 0.0), abs(fd("A1", (i, j)) - g["A1"][i, j]) / sc)
    for key in ("Pinf", "x0P"):
        sc = np.abs(g[key]).max()
        for i in range(d):
            for j in range(i, d):
                want = g[key][i, j] * (2.0 if i != j else 1.0)      # (a symmetrised gradient pairs with a symmetric tangent)
                worst[key] = max(worst.get(key, 0.0), abs(fd(key, (i, j), True) - want) / sc)
    for key in ("a", "H", "x0m"):
        sc = np.abs(g[key]).max()
        for i in range(d):
            worst[key] = max(worst.get(key, 0.0), abs(fd(key, (i,)) - g[key][i]) / sc)
    for key, steps in (("R", "R_steps"), ("h", "h_steps")):
        sc = np.abs(g[steps]).max()
        for t in (40, 200, 57, 150):      # (57: behind a tie; 150: behind the long gap)
            assert not missing[t]
            worst[steps] = max(worst.get(steps, 0.0), abs(fd(key, (t,)) - g[steps][t]) / sc)
            assert g[steps][t] != 0.0
        for t in (77, 130):
            assert missing[t] and g[steps][t] == 0.0
    print({k_: f"{v:.1e}" for k_, v in worst.items()})
    assert max(worst.values()) <= 1e-6, worst
    assert g["h"] == pytest.approx(g["h_steps"].sum(), rel=1e-14) and g["R"] == pytest.approx(g["R_steps"].sum(), rel=1e-14)


def test_a_model_without_an_explicit_first_transition_puts_step_zero_into_F():
    """A1 = None: step 0 takes the closed form at tau = 1, gA1 = 0 and gF carries the step -- against central differences through the same map"""
    blocks, times, y, missing = irregular_case(M52, seed=6)
    blocks["A1"] = None
    lp, g = SS.restated(times=times, y=y, missing=missing, **blocks)
    assert np.all(g["A1"] == 0.0)
    sc, worst = np.abs(g["F"]).max(), 0.0
    for i in range(3):
        for j in range(3):
            vals = []
            step = 1e-4 * max(abs(blocks["F"][i, j]), 0.1)
            for s in (+1.0, -1.0):
                b2 = dict(blocks)
                b2["F"] = blocks["F"].copy()
                b2["F"][i, j] += s * step
                vals.append(ref.logpdf_missing(SS.oracle_model(times=times, **b2), y, missing))
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * step) - g["F"][i, j]) / sc)
    print(f"{worst:.1e}")
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("shape", [(1,), (2,), (3,), (2, 2), (3, 1), (1, 1, 2)], ids=lambda s: "+".join(map(str, s)))
def test_the_chain_rule_alone(shape):
    rng = np.random.default_rng(sum(shape) * 10 + len(shape))
    d = sum(shape)
    F, o = np.zeros((d, d)), 0
    for n in shape:
        F[o:o + n, o:o + n] = rng.standard_normal((n, n)) + 0.5      # (dense blocks: the components are the blocks)
        o += n
    assert [len(S) for S in SS.components_of(F)] == list(shape)
    dF = np.where(F != 0.0, rng.standard_normal((d, d)), 0.0)
    gl, gN1, gN2 = rng.standard_normal(d), rng.standard_normal((d, d)), rng.standard_normal((d, d))
    gF = SS.chain_rule(F, gl, gN1, gN2)
    assert np.all(gF[F == 0.0] == 0.0)
    step = 1e-3
    cp, cm = SS.coefficients(F + step * dF), SS.coefficients(F - step * dF)
    terms = [g * (p - m) / (2 * step) for g, p, m in zip((gl, gN1, gN2), cp, cm)]
    want = sum(float(t.sum()) for t in terms)
    got = float((gF * dF).sum())
    scale = sum(float(np.abs(t).sum()) for t in terms)
    print(shape, got, want)
    assert abs(got - want) <= 1e-10 * scale, (got, want)
