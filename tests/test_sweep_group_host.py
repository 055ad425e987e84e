"""CPU tier: the group sweep's algorithm (tgp_sweep_group.hip) restated in NumPy, against oracle.lgssm_ref at d = 5 and d = 8, T = 2100,
C = 64 -- so that a wrong formula is not debugged on the GPU.  The restatement keeps the kernel's structure: a state by COLUMNS in 8 lanes (lanes j >= d
hold zeros and must contribute zeros), A P A' through one transpose of a tile whose rows >= d are never written, the Cholesky of Pp + 1e-10 I row by
row, G' by two triangular solves per column, the RTS step in gain form; waves of 8 groups of which 6 own output, the forward warm-up over a chunk's last
W steps and its hand-over to the next group, the backward warm-up over a chunk's first Wb steps and its hand-over to the previous one, both checks, and
backward blocks recomputed from packed checkpoints every B steps (B = 8 at d = 5: it does not divide the last chunk of 52 steps; B = 4 at d = 8).
Tolerances: the project's (logpdf 1e-10 relative, marginals 1e-8 of their scale)."""
import numpy as np
import pytest

from oracle import lgssm_ref as ref
from tests import _sweep_group as SG
from tests import _util as U

G, JIT = 8, 1e-10
T, C, W, WB = 2100, 64, 128, 64
DT = 0.5      # (a grid on which the filter forgets within two chunks of 64 steps)


class Group:
    """the column layout: Pc[i, j] = P[i][j] held by lane j (i < d); lanes j >= d are padding"""

    def __init__(self, model):
        d = self.d = len(model["x0m"])
        self.act = np.arange(G) < d
        pad = lambda M: np.pad(M, ((0, G - d), (0, G - d)))      # noqa: E731
        vec = lambda v: np.pad(v, (0, G - d))      # noqa: E731
        self.A, self.Q = pad(model["A"][0]), pad(0.5 * (model["Q"][0] + model["Q"][0].T))
        self.a, self.H = vec(model["a"][0]), vec(model["H"][0])
        self.tile = np.full((G, G), np.nan)      # rows >= d stay NaN: reading one would poison the result

    def state(self, m, P):
        d = self.d
        return np.pad(m, (0, G - d)), np.pad(P, ((0, G - d), (0, G - d)))

    def predict(self, m, Pc):
        Wm = self.A @ Pc                                  # lane-local: column j of A P
        self.tile[:self.d, :] = Wm[:self.d, :]            # lane j writes column j, rows < d
        rows = np.where(self.act[None, :], self.tile.T, 0.0)      # lane j reads row j of the tile; padding lanes take zeros, never the unwritten rows
        return self.A @ m + self.a, self.A @ rows + self.Q, Wm

    def update(self, m, Pc, y, R, h, obs):
        v = Pc.T @ self.H                                 # (P H)_j = H . P[:, j]
        S = float(self.H @ v) + R if obs else 1.0
        iS = 1.0 / S if obs else 0.0
        e = (y - (float(self.H @ m) + h)) if obs else 0.0
        return m + v * (e * iS), Pc - np.outer(v, v * iS), S, e * e * iS

    def smooth(self, mf, Pf, ms, Ps):
        d = self.d
        mp, Pp, AP = self.predict(mf, Pf)
        U = np.zeros((G, G))                              # U[i, j]: row i of lane j's column
        rinv = np.zeros(G)
        for i in range(d):
            acc = Pp[i, :] + np.where(np.arange(G) == i, JIT, 0.0)
            dg = acc[i] - U[:i, i] @ U[:i, i]
            assert dg > 0.0
            acc = acc - U[:i, i] @ U[:i, :]
            rinv[i] = 1.0 / np.sqrt(dg)
            U[i, :] = np.where((np.arange(G) > i) & self.act, acc * rinv[i], 0.0)
            U[i, i] = np.sqrt(dg)
        X = np.zeros((G, G))                              # X[:, j] = column j of G'
        for i in range(d):
            X[i, :] = (AP[i, :] - U[:i, i] @ X[:i, :]) * rinv[i]
        for i in range(d - 1, -1, -1):
            X[i, :] = (X[i, :] - U[i, i + 1:d] @ X[i + 1:d, :]) * rinv[i]
        X[:, ~self.act] = 0.0
        ms2 = mf + X.T @ (ms - mp)
        Dm = np.where(self.act[None, :], Ps - Pp - JIT * np.eye(G), 0.0)
        N = X.T @ Dm                                      # G Dm, column j lane-local
        Ps2 = np.where(self.act[None, :], Pf + N @ X, 0.0)
        return ms2, Ps2

    def pack(self, m, Pc):
        d = self.d
        return np.concatenate([m[:d], Pc[:d, :d][np.triu_indices(d)]])

    def unpack(self, q):
        d = self.d
        P = np.zeros((d, d))
        P[np.triu_indices(d)] = q[d:]
        return self.state(q[:d], P + np.triu(P, 1).T)

    def distance(self, sd, a, b):
        d = self.d
        dm = np.abs(a[0] - b[0])[:d] / (sd + np.abs(a[0][:d]) + np.abs(b[0][:d]))
        dP = np.abs(a[1] - b[1])[:d, :d] / np.outer(sd, sd)
        return max(dm.max(), dP.max())


def run_group_sweep(model, y, missing, Rnew, B, W=W, Wb=WB):
    d = len(model["x0m"])
    gl = Group(model)
    R, h = float(np.atleast_1d(model["R"])[0]), float(np.atleast_1d(model["h"])[0])
    Pinf = model["x0P"]      # (a GP's series starts from its stationary prior, mean zero: where a warm-up starts as well)
    assert np.allclose(model["A"][0] @ Pinf @ model["A"][0].T + model["Q"][0], Pinf, rtol=0, atol=1e-12) and not model["x0m"].any()
    gen, x0 = gl.state(np.zeros(d), Pinf), gl.state(model["x0m"], np.triu(model["x0P"]) + np.triu(model["x0P"], 1).T)
    sd = np.sqrt(np.diag(Pinf))
    owned_n = 6
    nchunks = -(-T // C)
    nwaves = -(-nchunks // owned_n)
    mean, var, lml, dist = np.full(T, np.nan), np.full(T, np.nan), 0.0, [0.0, 0.0]
    written = np.zeros(T, dtype=int)

    def fstep(x, t):
        m, Pc, _ = gl.predict(*x)
        obs = t < T and not missing[t]
        m, Pc, S, q = gl.update(m, Pc, y[min(t, T - 1)], R, h, obs)
        return (m, Pc), (np.log(2 * np.pi * S) + q if obs else 0.0)

    for wave in range(nwaves):
        span = []
        for g in range(G):
            c = wave * owned_n + g - 1
            active = 0 <= c < nchunks
            t0 = c * C if active else 0
            t1 = min(t0 + C, T) if active else 0
            span.append((t0, t1, active and g >= 1, active and 1 <= g <= owned_n))
        e1, ck, xend, b1 = [None] * G, [dict() for _ in range(G)], [None] * G, [gen] * G
        for g, (t0, t1, runs, owned) in enumerate(span):      # forward warm-up: the last W steps of the group's own chunk
            t1r = (t1 + 7) // 8 * 8
            tw = t1r - W
            x = x0 if tw <= 0 else gen
            for t in range(max(tw, 0), t1r):
                x, _ = fstep(x, t)
            e1[g] = x
        for g, (t0, t1, runs, owned) in enumerate(span):      # the chunk from the previous group's end state
            if not runs:
                continue
            t1r = (t1 + 7) // 8 * 8
            x = x0 if t0 == 0 else e1[g - 1]
            acc = 0.0
            for t in range(t0, t1r):
                if (t - t0) % B == 0:
                    ck[g][(t - t0) // B] = gl.pack(*x)
                x, l = fstep(x, t)
                acc += l
            xend[g] = x
            if owned:
                lml += -0.5 * acc
                dist[0] = max(dist[0], gl.distance(sd, x, e1[g]))

        def backward(g, hi, fresh, xs, emit):
            t0 = span[g][0]
            for b in range((hi - t0 + B - 1) // B - 1, -1, -1):
                tsb = t0 + b * B
                x = gl.unpack(ck[g][b])
                F = []
                for k in range(B):
                    x, _ = fstep(x, tsb + k)
                    F.append(gl.unpack(gl.pack(*x)))      # through the packed LDS record, as the kernel
                for k in range(B - 1, -1, -1):
                    t = tsb + k
                    if t >= hi:
                        continue
                    xs = F[k] if (fresh and t == hi - 1) else gl.smooth(*F[k], *xs)
                    if emit:
                        mean[t] = gl.H @ xs[0] + h
                        var[t] = gl.H @ (xs[1].T @ gl.H) + Rnew[t]
                        written[t] += 1
            return xs

        for g, (t0, t1, runs, owned) in enumerate(span):      # backward warm-up over the chunk's first Wb steps
            if runs:
                b1[g] = backward(g, min(t0 + Wb, t1), True, gen, False)
        for g, (t0, t1, runs, owned) in enumerate(span):
            if owned:
                xs = backward(g, t1, t1 == T, b1[g + 1] if g + 1 < G else gen, True)
                dist[1] = max(dist[1], gl.distance(sd, xs, b1[g]))
        # padding lanes never leave zero
        for g in range(G):
            for st in (e1[g], xend[g], b1[g]):
                if st is not None and st is not gen:
                    assert not st[0][d:].any() and not st[1][:, d:].any() and not st[1][d:, :].any()
    assert written.min() == 1 and written.max() == 1
    return lml, mean, var, dist


@pytest.fixture(scope="module")
def cases():
    out = {}
    for d in (5, 8):
        k, _, s2 = SG.KERNELS[d]
        model, y, _ = U.gp_case(k, ("regular", 0.0, DT, T), s2, seed=40 + d)
        rng = np.random.default_rng(50 + d)
        missing = rng.random(T) < 0.1
        missing[0] = True
        missing[60:70] = True           # across the first chunk edge
        missing[T - 3:] = True
        Rn = rng.random(T) * 0.05
        lp = ref.logpdf_missing(model, y, missing)
        pm, pv = ref.marginals(ref.replace_observation_noise_cov(ref.posterior_missing(model, y, missing), Rn))
        out[d] = dict(model=model, y=y, missing=missing, Rn=Rn, lp=lp, pm=pm, pv=pv)
    return out


@pytest.mark.parametrize("d", [5, 8])
def test_group_algorithm_equals_the_oracle(cases, d):
    c = cases[d]
    B = 8 if d <= 6 else 4
    assert (T - (T // C) * C) == 52 and (d != 5 or 52 % B != 0)      # the last chunk is short; at d = 5 the block does not divide it
    lml, mean, var, dist = run_group_sweep(c["model"], c["y"], c["missing"], c["Rn"], B)
    print(d, lml, c["lp"], dist)
    assert abs(lml - c["lp"]) <= 1e-10 * abs(c["lp"])
    assert np.abs(mean - c["pm"]).max() <= 1e-8 * max(1.0, np.abs(c["pm"]).max())
    assert np.abs(var - c["pv"]).max() <= 1e-8 * max(1.0, c["pv"].max())
    assert dist[0] <= 1e-12 and dist[1] <= 1e-11, dist      # both hand-over checks hold at these warm-ups ...


def test_the_hand_over_checks_see_warm_ups_that_are_too_short(cases):
    c = cases[5]
    lml, mean, var, dist = run_group_sweep(c["model"], c["y"], c["missing"], c["Rn"], 8, W=8, Wb=8)
    print(dist, abs(lml - c["lp"]) / abs(c["lp"]))
    assert dist[0] > 1e-12 and dist[1] > 1e-11      # ... and fail where the kernel would report bits 1 and 2
