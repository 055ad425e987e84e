"""Shared by the group sweep's posterior-draw tests (tgp_sweep_group.hip k_sweep_group_draw): a NumPy restatement of the chunked walk as the
kernel lays it out -- lane j of a group holds column j of every matrix and element j of the sample -- and the cases both tiers draw on."""
import numpy as np

from oracle import lgssm_ref as ref
from tests import _sweep_group as SG
from tests import _util as U

JIT, JIT_DRAW, JIT_START = 1e-10, 1e-9, 1e-12
TOL_F, TOL_D = 1e-12, 1e-11      # tgp_sweep_plan.hpp kTol / kTolBack


def eps_of(rng, T, d):
    return rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d)


def err(got, want):
    """largest error / max(1, max |y*|): the bar's scale"""
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def case(d, T, seed, xs=0, dt=None, frac=0.1):
    """An LTI model of tests/_sweep_group.py at dimension d with `frac` of the steps missing, the first and the last among them.  xs bit 0: a noise
    variance per step, bit 1: an emission offset per step.  Returns (model, y, missing, Rnew (T,), eps)."""
    k, dt0, s2 = SG.KERNELS[d]
    rng = np.random.default_rng(seed)
    S = s2 * (0.5 + rng.random(T)) if xs & 1 else s2
    mean = ("custom", lambda v: np.sin(0.3 * np.asarray(v))) if xs & 2 else None
    model, y, _ = U.gp_case(k, ("regular", 0.0, dt0 if dt is None else dt, T), S, seed=seed, mean=mean)
    mk = rng.random(T) < frac
    mk[0] = mk[T - 1] = True
    Rn = np.where(mk, 0.05, 0.02 * rng.random(T))
    return model, y, mk, Rn, eps_of(rng, T, d)


def chol_upper(M):
    return np.linalg.cholesky(M).T


def stationary(model):
    """(gm, gP, sd): the stationary prior a warm-up starts from and the scale of a state's elements (tgp_sweep_plan.hpp stationary_prior)"""
    A, a, Q = model["A"][0], model["a"][0], model["Q"][0]
    d = len(a)
    Qs = 0.5 * (Q + Q.T)
    P = np.linalg.solve(np.eye(d * d) - np.kron(A, A), Qs.reshape(-1)).reshape(d, d)
    P = 0.5 * (P + P.T)
    return np.linalg.solve(np.eye(d) - A, a), P, np.sqrt(np.diag(P))


class Columns:
    """One group: lane j owns column j.  The steps below are written column by column where the kernel's data flow shows in the arithmetic (which factor
    is solved against, what Z and L are formed from); NumPy's own order of additions stands in for the lanes' fma chains."""

    def __init__(self, model):
        self.model = model
        self.A, self.a, self.Q = model["A"][0], model["a"][0], 0.5 * (model["Q"][0] + model["Q"][0].T)
        self.d = len(self.a)

    def fstep(self, m, P, t, y, missing):
        """the filter's step t: predict, then the update unless the step is missing (steps behind the series' end are)"""
        mp, Pp = self.A @ m + self.a, self.A @ P @ self.A.T + self.Q
        if t >= self.model["T"] or missing[t]:
            return mp, Pp
        H, h, R = ref.emission(self.model, t)
        V = Pp @ H
        S = H @ V + R
        return mp + V * ((y[t] - H @ mp - h) / S), Pp - np.outer(V, V) / S

    def draw_start(self, mf, Pf, e0):
        return mf + chol_upper(Pf + JIT_START * np.eye(self.d)).T @ e0

    def draw_step(self, mf, Pf, x, e):
        """x_(t+1) -> x_t from the filtering state of step t and eps_t[t + 1] (Lane::draw_step)"""
        I = np.eye(self.d)
        mp, Pp = self.A @ mf + self.a, self.A @ Pf @ self.A.T + self.Q
        AP = self.A @ Pf
        Uc = chol_upper(Pp + JIT * I)                              # the 8-lane factorisation; U is published
        Gt = np.linalg.solve(Uc, np.linalg.solve(Uc.T, AP))        # column j of G': U' z = AP[:, j], U w = z
        Z = Uc @ Gt                                                # column j of U G' from the published U
        L = Pf - Z.T @ Z                                           # one publication of Z; the reference's form
        UL = chol_upper(L + JIT_DRAW * I)                          # the second 8-lane factorisation
        nz = np.array([UL[:j + 1, j] @ e[:j + 1] for j in range(self.d)])      # lane-local: column j against the gathered draws
        return mf + nz + Gt.T @ (x - mp)


def distance_state(sd, a, b):
    (ma, Pa), (mb, Pb) = a, b
    return max(np.max(np.abs(ma - mb) / (sd + np.abs(ma) + np.abs(mb))), np.max(np.abs(Pa - Pb) / np.outer(sd, sd)))


def distance_sample(sd, a, b):
    """the mean part of the state distance: what the draw's hand-over check compares"""
    return float(np.max(np.abs(a - b) / (sd + np.abs(a) + np.abs(b))))


def chunked_draw(model, y, missing, Rnew, eps, C, W, Wd, B):
    """k_sweep_group_draw's structure: chunks of C steps (a multiple of 8), a chunk per group.
    Forwards: a chunk starts from the previous chunk's warm-up over its last W steps from the stationary prior (from x0 where the window reaches step 0),
    keeps a checkpoint every B steps, and compares its end state with its own warm-up's (dist_f).
    Backwards: a chunk first walks its own first Wd steps from x = m_f behind them with the real draws (from the true x_(T-1) where the window reaches the
    series' end); the result goes to the chunk before it, which walks its steps from it -- the filtering states of a block recomputed from its
    checkpoint -- writes y* and compares its x at its first step with its own warm-up's (dist_d).
    (Which group of which wave computes a warm-up does not show in the values: group 7 of a wave repeats group 1's work of the next wave.)
    Returns (y*, dist_f, dist_d)."""
    T, d = model["T"], len(model["x0m"])
    et, ee, e0 = eps
    Rn = np.broadcast_to(np.asarray(Rnew, dtype=np.float64), (T,))
    miss = np.zeros(T, dtype=bool) if missing is None else np.asarray(missing, dtype=bool)
    gl = Columns(model)
    gm, gP, sd = stationary(model)
    x0 = (np.asarray(model["x0m"], dtype=np.float64), ref.symmetric(np.asarray(model["x0P"], dtype=np.float64)))
    assert C % 8 == 0 and C % B == 0 and W % 8 == 0 and Wd % 8 == 0 and Wd <= C
    nchunks = -(-T // C)
    span = lambda c: (c * C, min(c * C + C, T))      # noqa: E731
    # ---- forwards
    ends, ckpts, dist_f = {}, {}, 0.0
    for c in range(nchunks):
        t0, t1 = span(c)
        t1r = -(-t1 // 8) * 8
        tw = t1r - W
        st = x0 if tw <= 0 else (gm, gP)
        for t in range(max(tw, 0), t1r):
            st = gl.fstep(*st, t, y, miss)
        ends[c] = st
        st = x0 if c == 0 else ends[c - 1]
        ck = []
        for t in range(t0, t1r):
            if (t - t0) % B == 0:
                ck.append(st)
            st = gl.fstep(*st, t, y, miss)
        ckpts[c] = ck
        dist_f = max(dist_f, distance_state(sd, st, ends[c]))

    def block_states(c, tsb):
        """the filtering states of the block that starts at step tsb, forwards from its checkpoint"""
        st, out = ckpts[c][(tsb - span(c)[0]) // B], []
        for k in range(B):
            st = gl.fstep(*st, tsb + k, y, miss)
            out.append(st)
        return out

    def walk(c, hi, x, start, emit):
        t0 = span(c)[0]
        tsb = (hi - 1 - t0) // B * B + t0
        while tsb >= t0:
            F = block_states(c, tsb)
            for k in range(B - 1, -1, -1):
                t = tsb + k
                if t >= hi:
                    continue
                mf, Pf = F[k]
                if start and t == hi - 1:
                    x = gl.draw_start(mf, Pf, e0) if start == 2 else mf.copy()
                else:
                    x = gl.draw_step(mf, Pf, x, et[t + 1])
                if emit is not None:
                    H, h, _ = ref.emission(model, t)
                    emit[t] = H @ x + h + np.sqrt(Rn[t]) * ee[t]
            tsb -= B
        return x

    # ---- backwards: the warm-ups, then the chunks
    b1 = {}
    for c in range(nchunks):
        t0, t1 = span(c)
        te = min(t0 + Wd, t1)
        b1[c] = walk(c, te, None, 2 if te == T else 1, None)
    out, dist_d = np.full(T, np.nan), 0.0
    for c in range(nchunks):
        t0, t1 = span(c)
        x = walk(c, t1, None if t1 == T else b1[c + 1], 2 if t1 == T else 0, out)
        dist_d = max(dist_d, distance_sample(sd, x, b1[c]))
    return out, dist_f, dist_d
