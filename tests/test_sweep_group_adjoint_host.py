"""CPU tier: the group sweep's adjoint kernel (k_sweep_group_adjoint) restated in NumPy, against tests/_sweep_adjoint.py::restated (long double)
at d = 5 and d = 8, T = 2100, C = 64, with a missing mask and a noise variance per step -- so that a wrong formula is not debugged on the GPU.  The
restatement keeps the kernel's structure: states AND adjoints by COLUMNS in 8 lanes (lanes j >= d hold zeros and must contribute zeros), a tile whose rows
>= d hold NaN and are never read, the publication of Pb through that tile, (L V)_j lane-local by the symmetry of L, waves of 8 groups of which 6 own
output, the forward warm-up and its hand-over, the adjoint warm-up over a chunk's first Wa steps from zero and its hand-over to the previous group, both
checks, blocks recomputed from packed checkpoints every B steps with a step reading the state in FRONT of it, the sums by columns and the packed record.
Tolerances: the project's (tests/_sweep_adjoint.py LP_BAR, GRAD_BAR)."""
import numpy as np
import pytest

from tests import _sweep_adjoint as SA
from tests import _sweep_group as SG
from tests import _util as U
from tests.test_sweep_group_host import Group

G = 8
T, C, W, WA = 2100, 64, 128, 64
DT = 0.5      # (a grid on which the filter forgets within two chunks of 64 steps, the adjoint within one)


class AdjointGroup(Group):
    def adjoint_step(self, xf, y, R, h, obs, ad, acc):
        """tgp_sweep_group.hip Lane::adjoint_step: xf the state in front of the step, ad = (l, Lc) behind it; returns the adjoint in front, gh_t, gR_t"""
        d, H = self.d, self.H
        l, Lc = ad
        mp, Pp, AP = self.predict(*xf)
        V = Pp.T @ H                                      # V_j = sum_i Pp[i][j] H_i: lane-local
        S = float(H @ V) + R if obs else 1.0
        iS = 1.0 / S if obs else 0.0
        v = (y - (float(H @ mp) + h)) if obs else 0.0
        LV = Lc.T @ V                                     # (L V)_j = sum_i L[i][j] V_i: lane-local because L is symmetric
        lV, VLV = float(l @ V), float(V @ LV)
        vbar = (lV - v) * iS
        Sbar = (VLV - lV * v) * iS * iS - 0.5 * (iS - (v * iS) ** 2)
        Vb = Sbar * H + l * (v * iS) - 2.0 * iS * LV
        mb = l - vbar * H
        Pb = Lc + 0.5 * (np.outer(Vb, H) + np.outer(H, Vb))      # column j in lane j
        if acc is not None:
            acc["H"] += Pp.T @ Vb + Sbar * V - vbar * mp
            acc["a"] += mb
            acc["Q"] += Pb
            acc["h"] -= vbar
            acc["R"] += Sbar
        self.tile[:d, :] = Pb[:d, :]                      # lane j writes column j, rows < d; every lane reads rows and columns < d only
        Pbt = self.tile[:d, :d]
        assert np.isfinite(Pbt).all()
        u = np.zeros((G, G))
        w = np.zeros((G, G))
        u[:d, :] = Pbt @ AP[:d, :]                        # u[:, j] = Pb (A P)[:, j]
        w[:d, :] = Pbt @ self.A[:d, :]                    # w[:, j] = Pb A[:, j]
        if acc is not None:
            acc["A"] += np.outer(mb, xf[0]) + 2.0 * u     # gA[:, j] += mb m_j + 2 u
        return (self.A.T @ mb, self.A.T @ w), -vbar, Sbar

    def adjoint_distance(self, sd, a, b):
        d = self.d
        return max((np.abs(a[0] - b[0])[:d] * sd).max(), (np.abs(a[1] - b[1])[:d, :d] * np.outer(sd, sd)).max())


def run_group_adjoint(model, y, missing, B, W=W, Wa=WA):
    d = len(model["x0m"])
    gl = AdjointGroup(model)
    Rs = np.broadcast_to(np.atleast_1d(model["R"]), (T,))
    h = float(np.atleast_1d(model["h"])[0])
    Pinf = model["x0P"]
    assert np.allclose(model["A"][0] @ Pinf @ model["A"][0].T + model["Q"][0], Pinf, rtol=0, atol=1e-12) and not model["x0m"].any()
    gen, x0 = gl.state(np.zeros(d), Pinf), gl.state(model["x0m"], np.triu(model["x0P"]) + np.triu(model["x0P"], 1).T)
    zero = (np.zeros(G), np.zeros((G, G)))
    sd = np.sqrt(np.diag(Pinf))
    owned_n = 6
    nchunks = -(-T // C)
    nwaves = -(-nchunks // owned_n)
    ds = d * (d + 1) // 2
    NG = d * d + d + ds + d + 2 + d + ds
    total = np.zeros(NG)
    gh, gR = np.full(T, np.nan), np.full(T, np.nan)
    written = np.zeros(T, dtype=int)
    lml, dist = 0.0, [0.0, 0.0]

    def inputs(t):
        tc = min(t, T - 1)
        return y[tc], Rs[tc], t < T and not missing[t]

    def fstep(x, t):
        m, Pc, _ = gl.predict(*x)
        yt, Rt, obs = inputs(t)
        m, Pc, S, q = gl.update(m, Pc, yt, Rt, h, obs)
        return (m, Pc), (np.log(2 * np.pi * S) + q if obs else 0.0)

    for wave in range(nwaves):
        span = []
        for g in range(G):
            c = wave * owned_n + g - 1
            active = 0 <= c < nchunks
            t0 = c * C if active else 0
            t1 = min(t0 + C, T) if active else 0
            span.append((t0, t1, active and g >= 1, active and 1 <= g <= owned_n))
        e1, ck, b1 = [None] * G, [dict() for _ in range(G)], [zero] * G
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
                x, lq = fstep(x, t)
                acc += lq
            if owned:
                lml += -0.5 * acc
                dist[0] = max(dist[0], gl.distance(sd, x, e1[g]))

        def walk(g, hi, ad, acc):
            t0 = span[g][0]
            for b in range((hi - t0 + B - 1) // B - 1, -1, -1):
                tsb = t0 + b * B
                x = gl.unpack(ck[g][b])
                F = [x]                                       # slot k: the state in FRONT of step k (the block's last state is not computed)
                for k in range(B - 1):
                    x, _ = fstep(x, tsb + k)
                    F.append(gl.unpack(gl.pack(*x)))          # through the packed LDS record, as the kernel
                for k in range(B - 1, -1, -1):
                    t = tsb + k
                    if t >= hi:
                        continue
                    yt, Rt, obs = inputs(t)
                    ad, gh_t, gR_t = gl.adjoint_step(F[k], yt, Rt, h, obs, ad, acc)
                    if acc is not None:
                        gh[t], gR[t] = gh_t, gR_t
                        written[t] += 1
            return ad

        for g, (t0, t1, runs, owned) in enumerate(span):      # the adjoint's warm-up over the chunk's first Wa steps, from zero
            if runs:
                b1[g] = walk(g, min(t0 + Wa, t1), zero, None)
        part = np.zeros(NG)
        for g, (t0, t1, runs, owned) in enumerate(span):
            if not owned:
                continue
            acc = dict(A=np.zeros((G, G)), a=np.zeros(G), Q=np.zeros((G, G)), H=np.zeros(G), h=0.0, R=0.0)
            ad = walk(g, t1, zero if t1 == T else b1[g + 1], acc)
            dist[1] = max(dist[1], gl.adjoint_distance(sd, ad, b1[g]))
            for st in (ad, b1[g], (acc["a"], acc["A"]), (acc["H"], acc["Q"])):      # padding lanes never leave zero
                assert not st[0][d:].any() and not st[1][:, d:].any() and not st[1][d:, :].any()
            first = t0 == 0
            # the wave's record: columns of lanes < d; the symmetric blocks as the upper triangle of the lanes' columns (packed column by column)
            part += np.concatenate([acc["A"][:d, :d].T.ravel(), acc["a"][:d], _pack_upper(acc["Q"], d), acc["H"][:d],
                                    [acc["h"], acc["R"]], ad[0][:d] if first else np.zeros(d), _pack_upper(ad[1], d) if first else np.zeros(ds)])
        total += part
    assert written.min() == 1 and written.max() == 1
    o = np.cumsum([0, d * d, d, ds, d, 1, 1, d, ds])
    p = [total[o[i]:o[i + 1]] for i in range(8)]
    g = dict(A=p[0].reshape(d, d).T.copy(), a=p[1], Q=_unpack_upper(p[2], d), H=p[3], h=float(p[4][0]), R=float(p[5][0]), x0m=p[6], x0P=_unpack_upper(p[7], d),
             h_steps=gh, R_steps=gR)
    return lml, g, dist


def _pack_upper(M, d):
    """[j (j + 1) / 2 + i] = M[i][j], i <= j: lane j writes the upper part of its column"""
    return np.concatenate([M[:j + 1, j] for j in range(d)])


def _unpack_upper(q, d):
    M = np.zeros((d, d))
    for j in range(d):
        for i in range(j + 1):
            M[i, j] = M[j, i] = q[j * (j + 1) // 2 + i]
    return M


@pytest.fixture(scope="module")
def cases():
    out = {}
    for d in (5, 8):
        k, _, s2 = SG.KERNELS[d]
        model, y, _ = U.gp_case(k, ("regular", 0.0, DT, T), s2, seed=60 + d)
        rng = np.random.default_rng(70 + d)
        missing = rng.random(T) < 0.1
        missing[0] = True
        missing[60:70] = True           # across the first chunk edge
        missing[T - 3:] = True
        model = dict(model)
        model["R"] = s2 * (0.5 + rng.random(T))      # a noise variance per step
        lp, g = SA.restated(model, y, missing)
        out[d] = dict(model=model, y=y, missing=missing, lp=lp, g=g)
    return out


@pytest.mark.parametrize("d", [5, 8])
def test_group_adjoint_equals_the_restated_gradient(cases, d):
    c = cases[d]
    B = 8 if d <= 6 else 4
    assert (T - (T // C) * C) == 52 and (d != 5 or 52 % B != 0)      # the last chunk is short; at d = 5 the block does not divide it
    lml, g, dist = run_group_adjoint(c["model"], c["y"], c["missing"], B)
    dev = SA.block_deviations(g, c["g"])
    print(d, lml, c["lp"], dist, dev)
    assert abs(lml - c["lp"]) <= SA.LP_BAR * abs(c["lp"])
    assert max(dev.values()) <= SA.GRAD_BAR, dev
    for k in ("h_steps", "R_steps"):
        assert np.abs(g[k] - c["g"][k]).max() <= SA.GRAD_BAR * np.abs(c["g"][k]).max()
        assert (g[k][c["missing"]] == 0.0).all()
    assert dist[0] <= 1e-12 and dist[1] <= 1e-11, dist      # both hand-over checks hold at these warm-ups ...


def test_the_hand_over_checks_see_warm_ups_that_are_too_short(cases):
    c = cases[5]
    lml, g, dist = run_group_adjoint(c["model"], c["y"], c["missing"], 8, W=8, Wa=8)
    print(dist, SA.block_deviations(g, c["g"]))
    assert dist[0] > 1e-12 and dist[1] > 1e-11      # ... and fail where the kernel would report bits 1 and 2
