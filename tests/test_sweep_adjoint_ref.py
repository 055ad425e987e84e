"""CPU tier: the formulas of the sweep engine's adjoint gradient, restated in NumPy long double (tests/_sweep_adjoint.py), against
(a) the oracle's exact sequential adjoint (oracle/seq_adjoint) on gap-free models, every entry at 1e-12 of its block's largest (measured: <= 1.7e-15), and
(b) central differences of ref.logpdf_missing with a mask, a noise variance and an emission offset per step, at 1e-6 of the block's largest entry
(central differences with a step of 1e-5 carry ~1e-16 |logpdf| / 1e-5 ~ 1e-8 of rounding and less of truncation; measured: 2e-9 ... 9e-8)."""
import numpy as np
import pytest

from oracle import lgssm_ref as ref
from oracle import seq_adjoint
from tests import _sweep_adjoint as SA
from tests import _util as U

GAP_FREE = [
    (("matern12",), 0.1, 0.1),
    (("matern32",), 0.1, 0.1),
    (("matern52",), 0.1, 0.1),
    (("sum", ("matern32",), ("matern12",)), 0.1, 0.2),
    (("sum", ("matern32",), ("stretched", 0.7, ("matern32",))), 0.15, 0.1),
]


@pytest.mark.parametrize("i", range(len(GAP_FREE)))
def test_restatement_against_the_sequential_adjoint(i):
    k, dt, s2 = GAP_FREE[i]
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt, 600), s2, seed=i)
    assert len(model["x0m"]) == (1, 2, 3, 3, 4)[i]
    lp0, g0 = seq_adjoint.logpdf_adjoint(model, y)
    lp, g = SA.restated(model, y)
    assert abs(lp - lp0) <= 1e-12 * abs(lp0), (lp, lp0)
    dev = SA.block_deviations(g, g0)
    print(k, {b: f"{v:.1e}" for b, v in dev.items()})
    assert max(dev.values()) <= 1e-12, dev
    assert abs(g["h_steps"].sum() - g0["h"]) <= 1e-12 * abs(g0["h"]) and abs(g["R_steps"].sum() - g0["R"]) <= 1e-12 * abs(g0["R"])


def test_restatement_against_central_differences_with_mask_noise_and_offset_per_step():
    T = 300
    rng = np.random.default_rng(11)
    S = 0.1 * (0.5 + rng.random(T))
    model, y, _ = U.gp_case(("matern52",), ("regular", 0.0, 0.1, T), S, seed=2, mean=("custom", lambda t: np.sin(t)))
    assert model["R"].shape == (T,) and np.atleast_1d(model["h"]).shape == (T,)
    missing = rng.random(T) < 0.2
    missing[120:155] = True
    missing[[40, 200]] = False
    missing[77] = True
    lp, g = SA.restated(model, y, missing)
    lp0 = ref.logpdf_missing(model, y, missing)
    assert abs(lp - lp0) <= 1e-10 * abs(lp0), (lp, lp0)

    def fd(key, idx, sym=False):
        out = []
        x = np.asarray(model[key], dtype=np.float64)
        step = 1e-5 * max(abs(float(x[idx])), 0.1)
        for s in (+1.0, -1.0):
            m2 = dict(model)
            v = x.copy()
            v[idx] += s * step
            if sym and idx[-1] != idx[-2]:
                v[idx[:-2] + (idx[-1], idx[-2])] += s * step
            m2[key] = v
            out.append(ref.logpdf_missing(m2, y, missing))
        return (out[0] - out[1]) / (2.0 * step)

    d = 3
    worst = {}
    for key, lead in (("A", (0,)), ("Q", (0,)), ("x0P", ())):
        sym = key != "A"
        sc = np.abs(g[key]).max()
        for i in range(d):
            for j in range(i if sym else 0, d):
                want = g[key][i, j] * (2.0 if sym and i != j else 1.0)      # (a symmetrised gradient pairs with a symmetric tangent)
                worst[key] = max(worst.get(key, 0.0), abs(fd(key, lead + (i, j), sym) - want) / sc)
    for key, lead in (("a", (0,)), ("H", (0,)), ("x0m", ())):
        sc = np.abs(g[key]).max()
        for i in range(d):
            worst[key] = max(worst.get(key, 0.0), abs(fd(key, lead + (i,)) - g[key][i]) / sc)
    for key, steps in (("R", "R_steps"), ("h", "h_steps")):
        sc = np.abs(g[steps]).max()
        for t in (40, 200):
            assert not missing[t]
            worst[steps] = max(worst.get(steps, 0.0), abs(fd(key, (t,)) - g[steps][t]) / sc)
            assert g[steps][t] != 0.0
        for t in (77, 130):
            assert missing[t] and g[steps][t] == 0.0
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-6, worst
    assert g["h"] == pytest.approx(g["h_steps"].sum(), rel=1e-14) and g["R"] == pytest.approx(g["R_steps"].sum(), rel=1e-14)
