"""CPU tier: the arithmetic and the walk of k_sweep_group_sde (tgp_sweep_group_sde.hip), restated in NumPy and held to bounds, no GPU:
the closed-form A_t against the oracle's per-step blocks (expm), the Pinf identity P_p = Pinf + A (P_f - Pinf) A' against A P_f A' + Q_t, the band
the kernel multiplies, the host-predicted step 0, and the whole chunked walk in the geometry plan_group returns (tests/hostsim/sweep_group_sde_plan.cpp)
-- warm-ups from (x0m, Pinf), hand-overs with their distances, checkpoint blocks, the backward pass with the gap of step t + 1 taken at row, block and
chunk ends as the kernel takes it -- against ref.logpdf_missing and ref.posterior_missing within the project's bars (logpdf 1e-10 relative, marginals
1e-8 of their scale).  The repair case of tests/test_gpu_sweep_group_sde.py is chosen here: the forward distance is above 1e-12 at the first guess
and below it after one doubling."""
import numpy as np
import pytest

from oracle import lgssm_ref as ref
from tests import _sweep_group as SG
from tests import _sweep_group_sde as SS
from tests import _util as U


def _case(d, T, seed, lo=0.5, hi=1.5):
    k, dt, s2 = SG.KERNELS[d]
    t = np.cumsum(np.random.default_rng(seed).uniform(lo * dt, hi * dt, T))
    model, y, _ = U.gp_case(k, t, s2, seed=seed)
    F, H, P, blocks = SS.sde_blocks(k)
    return k, t, model, y, F, H, P, blocks


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_closed_form_transition_and_the_pinf_identity(d):
    """A_t to 1e-13 of its scale (a Pade expm of norm ~1 and a handful of products: some tens of ulps on either side) and the identity to 1e-13 of
    the state's scale"""
    k, t, model, y, F, H, P, blocks = _case(d, 400, 10 + d)
    lam, N1, N2 = SS.closed_form(F, blocks)
    i, j = np.indices(F.shape)
    assert not N1[np.abs(i - j) > 2].any() and not N2[np.abs(i - j) > 2].any()      # the band the kernel multiplies
    rng = np.random.default_rng(d)
    worst_a = worst_p = 0.0
    for s in range(1, 400):
        tau = t[s] - t[s - 1]
        A = SS.step_A(lam, N1, N2, tau)
        worst_a = max(worst_a, np.abs(A - model["A"][s]).max() / max(1.0, np.abs(model["A"][s]).max()))
        L = rng.standard_normal((d, d)) * np.sqrt(np.diag(P))[:, None] * 0.3
        Pf = L @ L.T
        worst_p = max(worst_p, np.abs(P + A @ (Pf - P) @ A.T - (A @ Pf @ A.T + model["Q"][s])).max() / np.abs(P).max())
    print(d, worst_a, worst_p)
    assert worst_a <= 1e-13 and worst_p <= 1e-13


def test_equal_stamps_give_the_identity():
    k, t, model, y, F, H, P, blocks = _case(8, 8, 3)
    assert np.array_equal(SS.step_A(*SS.closed_form(F, blocks), 0.0), np.eye(8))


@pytest.mark.parametrize("d", [5, 8])
def test_the_filter_walked_with_the_kernels_step_matches_the_reference(d):
    """step 0 from the host-predicted prior (A1 of a stretched term is exp(F tau) of no tau), every later step with the closed form and the identity"""
    T = 600
    k, t, model, y, F, H, P, blocks = _case(d, T, 20 + d)
    missing = np.random.default_rng(d).random(T) < 0.15
    missing[:3] = True
    lam, N1, N2 = SS.closed_form(F, blocks)
    R = float(np.atleast_1d(model["R"])[0])
    A1, Q1 = model["A"][0], model["Q"][0]
    m, Pc = A1 @ model["x0m"] + model["a"][0], A1 @ model["x0P"] @ A1.T + Q1
    q = logs = n = 0.0
    for s in range(T):
        if s > 0:
            A = SS.step_A(lam, N1, N2, t[s] - t[s - 1])
            m, Pc = A @ m, P + A @ (Pc - P) @ A.T
        if not missing[s]:
            V = Pc @ H
            S = H @ V + R
            v = y[s] - H @ m
            m, Pc = m + V * (v / S), Pc - np.outer(V, V) / S
            q, logs, n = q + v * v / S, logs + np.log(S), n + 1
    lp = -0.5 * (n * np.log(2 * np.pi) + logs + q)
    want = ref.logpdf_missing(model, y, missing)
    print(d, lp, want, abs(lp - want) / abs(want))
    assert abs(lp - want) <= 1e-10 * abs(want)


# ---- the chunked walk of k_sweep_group_sde in the plan's geometry, restated ----------------------------------------------------------------------
class Walk:
    """One chunk per group as the kernel walks it (tgp_sweep_group_sde.hip): forwards a warm-up over the chunk's last W steps from (x0m, Pinf) -- its
    end state starts the NEXT chunk -- then the chunk itself with a packed checkpoint every B steps and the hand-over distance; backwards a warm-up
    over the chunk's first Wb steps from the filtering state behind them -- its result is what the PREVIOUS chunk continues from -- then the chunk,
    block by block from the checkpoints, the smoothing step t + 1 -> t with the gap in front of step t + 1 taken as the kernel takes it (the row's next
    lane, or `tau_next`: the first gap of the row behind).  Steps behind the series' end are missing ones with the last gap (the rows are padded)."""

    def __init__(self, model, y, missing, t, H, P, lam, N1, N2, C, W, Wb, B):
        self.T = T = len(y)
        self.y, self.missing, self.H, self.Pinf, self.cf = y, missing, H, P, (lam, N1, N2)
        self.tau = np.concatenate([[-1.0], np.diff(t)])
        self.R = float(np.atleast_1d(model["R"])[0])
        self.C, self.W, self.Wb, self.B = C, W, Wb, B
        A1, Q1 = model["A"][0], model["Q"][0]
        self.x0 = (A1 @ model["x0m"] + model["a"][0], A1 @ model["x0P"] @ A1.T + Q1)      # the host's step 0
        self.gen = (np.asarray(model["x0m"], float).copy(), P.copy())
        self.sd = np.sqrt(np.diag(P))
        self.nchunks = -(-T // C)

    def A(self, tau):
        return SS.step_A(*self.cf, tau)

    def fstep(self, x, s, acc=None):
        m, Pc = x
        if s != 0:      # (t == 0: the state is the host's, kept)
            A = self.A(self.tau[min(s, self.T - 1)])
            m, Pc = A @ m, self.Pinf + A @ (Pc - self.Pinf) @ A.T
        if s < self.T and not self.missing[s]:
            V = Pc @ self.H
            S = self.H @ V + self.R
            v = self.y[s] - self.H @ m
            m, Pc = m + V * (v / S), Pc - np.outer(V, V) / S
            if acc is not None:
                acc += np.array([v * v / S, np.log(S), 1.0])
        return m, Pc

    def distance(self, a, b):
        dm = np.abs(a[0] - b[0]) / (self.sd + np.abs(a[0]) + np.abs(b[0]))
        return max(dm.max(), (np.abs(a[1] - b[1]) / np.outer(self.sd, self.sd)).max())

    def span(self, c):
        t0 = c * self.C
        t1 = min(t0 + self.C, self.T)
        return t0, t1, (t1 + 7) // 8 * 8

    def forward(self):
        """-> (logpdf, worst hand-over distance); keeps the checkpoints of every chunk"""
        acc, worst, self.ck, handed = np.zeros(3), 0.0, {}, None
        for c in range(self.nchunks):
            t0, t1, t1r = self.span(c)
            tw = t1r - self.W
            e1 = self.x0 if tw <= 0 else self.gen
            for s in range(max(tw, 0), t1r):
                e1 = self.fstep(e1, s)
            x = self.x0 if c == 0 else handed
            for s in range(t0, t1r):
                if (s - t0) % self.B == 0:
                    self.ck[s] = x
                x = self.fstep(x, s, acc)
            worst = max(worst, self.distance(x, e1))
            handed = e1
        return -0.5 * (acc[2] * np.log(2 * np.pi) + acc[1] + acc[0]), worst

    def smooth(self, xf, xs, tau):
        A = self.A(tau)
        mf, Pf = xf
        AP, AG = A @ Pf, A @ self.Pinf      # (the two products formed separately, as predict_r)
        mp, Pp = A @ mf, self.Pinf + (AP - AG) @ A.T
        Gt = np.linalg.solve(Pp + 1e-10 * np.eye(len(mf)), AP)      # G'
        return mf + Gt.T @ (xs[0] - mp), Pf + Gt.T @ (xs[1] - Pp - 1e-10 * np.eye(len(mf))) @ Gt

    def backward_run(self, t0, nrows, hi, fresh, xs, out=None):
        """tgp_sweep_group_sde.hip backward_run_s: rows nrows - 1 .. 0 of the chunk at t0, the steps below hi"""
        tau_of = lambda s: self.tau[min(max(s, 0), self.T - 1)]
        tau_next = tau_of(t0 + 8 * nrows)
        for r in range(nrows - 1, -1, -1):
            tb = t0 + 8 * r
            row_tau = [tau_of(tb + q) for q in range(8)]
            for sb in range(8 // self.B - 1, -1, -1):
                tsb = tb + sb * self.B
                if tsb >= hi:
                    continue
                x, F = self.ck[tsb], []
                for k in range(self.B):      # the block's filtering states, forwards from its checkpoint
                    x = self.fstep(x, tsb + k)
                    F.append(x)
                for k in range(self.B - 1, -1, -1):
                    s, q = tsb + k, sb * self.B + k
                    if s >= hi:
                        continue
                    xs = F[k] if (fresh and s == hi - 1) else self.smooth(F[k], xs, tau_next if q == 7 else row_tau[q + 1])
                    if out is not None:
                        out[0][s], out[1][s] = self.H @ xs[0], self.H @ xs[1] @ self.H
            tau_next = row_tau[0]
        return xs

    def backward(self):
        """-> (mean, var without the replaced noise, worst hand-over distance); behind forward()"""
        T, worst, b1 = self.T, 0.0, {}
        out = (np.zeros(T), np.zeros(T))
        for c in range(self.nchunks):
            t0, t1, _ = self.span(c)
            b1[c] = self.backward_run(t0, self.Wb // 8, min(t0 + self.Wb, t1), True, self.gen)
        for c in range(self.nchunks):
            t0, t1, _ = self.span(c)
            xs = self.backward_run(t0, self.C // 8, t1, t1 == T, b1.get(c + 1, self.gen), out)
            worst = max(worst, self.distance(xs, b1[c]))
        return out[0], out[1], worst


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return SS.plan_program(tmp_path_factory.mktemp("sweep_group_sde_host"))


def _walk(exe, tmp_path, d, t, model, y, missing, post, w_hint=0):
    k = SG.KERNELS[d][0]
    F, H, P, blocks = SS.sde_blocks(k)
    path = str(tmp_path / f"m{d}_{post}_{w_hint}.txt")
    SS.write_model(path, k, model, SS.typical_gap(t))
    p = SS.run_plan(exe, path, len(y), post=post, w_hint=w_hint)
    assert p["ok"], p
    return p, Walk(model, y, missing, t, H, P, *SS.closed_form(F, blocks), p["C"], p["W"], p["Wb"], p["B"])


@pytest.mark.parametrize("d", [5, 8])
def test_the_whole_walk_in_the_plans_geometry_matches_the_reference(exe, tmp_path, d):
    """T = 2100: 8 or 9 chunks of the plan's C, the last one short and padded to a row; group_block = 8 (d = 5) and 4 (d = 8); a stretched term at
    d = 8 (A1 is exp(F tau) of no tau).  logpdf to 1e-10 relative, marginals to 1e-8 of their scale, both hand-overs within the kernel's checks."""
    T = 2100
    k, dt, s2 = SG.KERNELS[d]
    t = np.cumsum(np.random.default_rng(70 + d).uniform(0.5 * dt, 1.5 * dt, T))
    t[1000:1004] = t[1000]      # equal stamps
    t = np.sort(t)
    model, y, _ = U.gp_case(k, t, s2, seed=71 + d)
    missing = np.random.default_rng(72 + d).random(T) < 0.15
    missing[:3] = True
    missing[T - 3:] = True
    p, w = _walk(exe, tmp_path, d, t, model, y, missing, post=1)
    assert p["nchunks"] >= 6 and T % p["C"] != 0
    lp, df = w.forward()
    mean, var, db = w.backward()
    want = ref.logpdf_missing(model, y, missing)
    pm, pv = ref.marginals(ref.replace_observation_noise_cov(ref.posterior_missing(model, y, missing), np.full(T, 1e-18)))
    print(d, p["C"], p["W"], p["Wb"], abs(lp - want) / abs(want), np.abs(mean - pm).max(), np.abs(var + 1e-18 - pv).max(), df, db)
    assert df <= 1e-12 and db <= 1e-11
    assert abs(lp - want) <= 1e-10 * abs(want)
    assert np.abs(mean - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max())
    assert np.abs(var + 1e-18 - pv).max() <= 1e-8 * max(1.0, pv.max())


def test_the_repair_case(exe, tmp_path):
    """tests/test_gpu_sweep_group_sde.py's repair case, gaps and seed: the forward hand-over distance is above the check's 1e-12 at the plan's first
    guess W and below it at 2 W (one doubling of sweep_run's repair loop), and the unstretched series passes at W"""
    d = SS.REPAIR_D
    k, dt, s2 = SG.KERNELS[d]
    t0 = np.cumsum(SS.repair_gaps(dt, 0, 0, stretched=False))
    model0, y0, _ = U.gp_case(k, t0, s2, seed=SS.REPAIR_SEED)
    none = np.zeros(SS.REPAIR_T, dtype=bool)
    p0, w0 = _walk(exe, tmp_path, d, t0, model0, y0, none, post=0)
    assert w0.forward()[1] <= 1e-12
    t = np.cumsum(SS.repair_gaps(dt, p0["C"], p0["W"]))
    model, y, _ = U.gp_case(k, t, s2, seed=SS.REPAIR_SEED)
    p1, w1 = _walk(exe, tmp_path, d, t, model, y, none, post=0)
    assert (p1["C"], p1["W"]) == (p0["C"], p0["W"])      # (the stretch does not move the median gap's plan)
    lp1, d1 = w1.forward()
    p2, w2 = _walk(exe, tmp_path, d, t, model, y, none, post=0, w_hint=2 * p1["W"])
    assert p2["W"] == 2 * p1["W"]
    lp2, d2 = w2.forward()
    print(p1["C"], p1["W"], d1, d2)
    assert d1 > 1e-12 and d2 <= 1e-12
    want = ref.logpdf(model, y)
    assert abs(lp2 - want) <= 1e-10 * abs(want)
