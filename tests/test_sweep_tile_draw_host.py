"""CPU tier: the step of k_sweep_tile_draw restated in NumPy on the padded 16 x 16 tile -- a unit diagonal on the padding of every factorised
matrix, the right-looking factor a pivot at a time, [Z | q] by forward substitution of [A P | x - m-] in the same sweep, G (x - m-) = Z' q and
L = P - Z' Z -- over a whole series at the four parity cases against draw_restated on the same draws (bar 1e-12; it prints 3e-15 .. 3e-14)."""
import functools

import numpy as np
import pytest

from tests import _sweep_group_draw as GD
from tests import _sweep_tile as ST
from tests import _sweep_tile_adjoint as TA
from tests import _sweepdraw as SD

DP = ST.DP


@functools.lru_cache(maxsize=None)
def draw_case(d, T, xs):
    """ST.case's model and mask with a new noise variance per step and draws: model, y, missing, Rn, eps, draw_restated's y*"""
    model, y, mk, _, _ = ST.case(d, T, xs)
    Rn = np.where(mk, 0.05, 0.02 * np.random.default_rng(7000 + d).random(T))
    eps = GD.eps_of(np.random.default_rng(7000 + d), T, d)
    return model, y, mk, Rn, eps, SD.draw_restated(model, y, mk, Rn, eps)


def factor(M, d, jit, B=None, c=None, e=None):
    """M + jit I_d + I_pad = U'U right-looking; returns (Z, Z'q) for the right-hand side [B | c], else U'e"""
    M = M + np.diag(np.where(np.arange(DP) < d, jit, 1.0))
    B, c, out = (None if B is None else B.copy()), (None if c is None else c.copy()), np.zeros(DP)
    for k in range(DP):
        assert M[k, k] > 0.0
        s = 1.0 / np.sqrt(M[k, k])
        u = np.where(np.arange(DP) < k, 0.0, M[k] * s)
        if B is not None:
            z, q = B[k] * s, c[k] * s
            c, out = c - u * q, out + z * q
            B = B - np.outer(u, z)
            B[k] = z
        else:
            out = out + u * e[k]
        M = M - np.outer(u, u)
    return (B, out) if B is not None else out


@pytest.mark.parametrize("d,T,xs", [c[:3] for c in TA.CASES])
def test_the_padded_step_walks_the_restated_draw(d, T, xs):
    model, y, mk, Rn, (et, ee, e0), want = draw_case(d, T, xs)
    pad = lambda M: np.pad(M, ((0, DP - d), (0, DP - d)))      # noqa: E731
    vec = lambda v: np.pad(v, (0, DP - d))      # noqa: E731
    A, Q, a, H = pad(model["A"][0]), pad(0.5 * (model["Q"][0] + model["Q"][0].T)), vec(model["a"][0]), vec(model["H"][0])
    ht = np.broadcast_to(np.atleast_1d(model["h"]), (T,))
    gl, st, front = GD.Columns(model), (model["x0m"], model["x0P"]), []
    for t in range(T):      # the filter: the state in front of every step, padded
        front.append((vec(st[0]), pad(st[1])))
        st = gl.fstep(*st, t, y, mk)
    m, P = vec(st[0]), pad(st[1])
    x, out = m + factor(P, d, 1e-12, e=vec(e0)), np.zeros(T)
    for t in range(T - 1, -1, -1):
        out[t] = H @ x + ht[t] + np.sqrt(Rn[t]) * ee[t]
        if t > 0:
            m, P = front[t]
            AP = A @ P
            Z, g = factor(A @ AP.T + Q, d, 1e-10, B=AP, c=x - (A @ m + a))
            x = m + g + factor(P - Z.T @ Z, d, 1e-9, e=vec(et[t]))
            assert not x[d:].any() and not Z[d:].any() and not Z[:, d:].any()      # the padding stays zero
    err = GD.err(out, want)
    print("d %d T %d xs %d: error / scale %.3g" % (d, T, xs, err))
    assert err <= 1e-12
