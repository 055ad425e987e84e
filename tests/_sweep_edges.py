"""The case table of the sweep engine's edge tests (test infrastructure): tests/test_sweep_edges_host.py runs every entry through the host simulations
(tests/hostsim/sweepsim.cpp, sweepdrawsim.cpp: the product's own plan and per-lane code), tests/test_gpu_sweep_edges.py through the C ABI on the device.
One entry holds the model, the spacing, the length, the per-step streams, the mask, a forced geometry and what tgp_sweep_info must show behind the call."""
import functools
from collections import namedtuple

import numpy as np

from oracle import components as oc
from oracle import lgssm_ref as ref
from oracle import seq_kalman as sk
from tests import _sweepdraw as SD
from tests import _util as U

M12, M32, M52 = ("matern12",), ("matern32",), ("matern52",)
SUM4 = ("sum", M32, ("stretched", 0.7, M32))
MODELS = {1: M12, 2: M32, 3: M52, 4: SUM4}
WORK_DT = {1: 0.1, 2: 0.1, 3: 0.1, 4: 0.15}       # the working spacing: automatic warm-ups of 32 ... 168 steps
FAST_DT = {1: 5.0, 2: 4.0, 3: 4.0, 4: 6.0}        # the fast-forgetting spacing: a start state is gone within 8 steps
S2 = 0.1
NUM_CU = 256                                      # the plan's machine (MI355X)
TOL_F, TOL_B = 1e-12, 1e-11                       # csrc/tgp_sweep_plan.hpp kTol / kTolBack
MARGIN = 10.0                                     # a host distance lies at least this factor on its side of the tolerance

# what: "k" (tgp_logpdf + tgp_logpdf_and_posterior_marginals -> k_sweep), "draw" (tgp_posterior_rand_missing -> k_sweep_draw)
# mask: a tuple of ("random", fraction) / ("range", first, behind) / ("ends", n);  bad: ("negR" | "inf", step)
# ties: 0 none, 1 a fifth of the gaps exactly 0 (see _times), 2 the same with both steps of every tie observed
# x0: 1 a prior of the series that is NOT the stationary one (mean (1, -2, 0.5, ...), 0.3 x its covariance): what a warm-up that reaches step 0 starts from
# force: (C, W, Wb) through options 15-17 (the draw: Wb is its Wd);  lp / post / draw: (served, status, attempts) of the logpdf call, the posterior call
# and the draw, each on a handle of its own (None: the call is not made)
Case = namedtuple("Case", "name group what d sde fast T xs mask force ties bad seed lp post draw x0")
OK = (1, 0, 1)
# group A draws whose name's own seed leaves a host distance within a factor 10 of a check (A-draw-d4-sde-xs1: draw distance 1.03e-12; seed 1: 2.8e-13)
DRAW_SEEDS = {(4, True, 1): 1}


def case(name, group, d, T, what="k", sde=False, fast=False, xs=0, mask=(("random", 0.1),), force=None, ties=0, bad=None, seed=None, lp=OK, post=OK, draw=OK, x0=0):
    seed = (sum(map(ord, name)) * 7919 + d) % 100003 if seed is None else seed
    if what == "draw":
        lp = post = None
    else:
        draw = None
    return Case(name, group, what, d, bool(sde), bool(fast), int(T), xs, tuple(mask), force, ties, bad, seed, lp, post, draw, x0)


def _table():
    t = []
    form = lambda s: "sde" if s else "lti"      # noqa: E731
    # ---- A: every instantiation.  T = 2053 (T mod 8 = 5, T mod 4 = 1), 10 % missing, automatic geometry at the working spacing
    for d in (1, 2, 3, 4):
        for s in (False, True):
            for xs in (0, 1, 2, 3):
                t.append(case(f"A-k-d{d}-{form(s)}-xs{xs}", "A", d, 2053, sde=s, xs=xs))
            for xs in (1, 2, 3):      # (XS = 0 and d = 3, 4 / sde / XS = 3 are tests/test_gpu_sweep_draw.py's; every instantiation is code of its own)
                t.append(case(f"A-draw-d{d}-{form(s)}-xs{xs}", "A", d, 2053, what="draw", sde=s, xs=xs, seed=DRAW_SEEDS.get((d, s, xs))))
    # ---- B: geometry, forced
    f8 = (8, 8, 8)
    for d in (1, 2, 3, 4):      # 62 k chunks and 62 k + 1 with a last chunk of one step: k = 5 is the smallest with 8 * 62 k >= 2048
        t.append(case(f"B-seam-d{d}-T2480", "B", d, 2480, fast=True, force=f8))
        t.append(case(f"B-seam-d{d}-T2481", "B", d, 2481, fast=True, force=f8))
    t.append(case("B-seam-d3-sde-T2480", "B", 3, 2480, sde=True, fast=True, force=f8))
    t.append(case("B-seam-d3-sde-T2481", "B", 3, 2481, sde=True, fast=True, force=f8))
    t.append(case("B-min-d3-T2048", "B", 3, 2048, fast=True, force=f8))
    for T in (2049, 2055):      # T mod 8 = 1, 7
        t.append(case(f"B-rem-d3-T{T}", "B", 3, T, fast=True, force=f8))
    for T in (2049, 2051):      # T mod 4 = 1, 3 at B = 4
        t.append(case(f"B-rem-d4-T{T}", "B", 4, T, fast=True, force=f8))
    t.append(case("B-one-chunk-d2", "B", 2, 2050, fast=True, force=(2056, 8, 8)))
    t.append(case("B-two-chunks-d2", "B", 2, 2060, fast=True, force=(1032, 8, 8)))
    t.append(case("B-warm-whole-series-d2", "B", 2, 2050, fast=True, force=(2056, 2056, 2056)))
    t.append(case("B-warm-whole-series-d4-sde", "B", 4, 2050, sde=True, fast=True, force=(2056, 2056, 2056)))
    t.append(case("B-warm-2-chunks-d3", "B", 3, 256 * 63 + 1, force=(256, 512, 256)))
    t.append(case("B-warm-5-chunks-d4", "B", 4, 256 * 63 + 1, force=(256, 1280, 256)))
    t.append(case("B-warm-5-chunks-d1-sde", "B", 1, 256 * 63 + 1, sde=True, force=(256, 1280, 256)))
    t.append(case("B-125-chunks-d3", "B", 3, 256 * 124 + 9, force=(256, 512, 256)))
    # (every other model here starts from its stationary prior, the state a warm-up inside the series starts from as well: here the warm-ups of the first
    # four chunks reach step 0 and must start from x0, chunk 3's exactly at step 0)
    # (chunks of 64 steps: a start state is still visible at a chunk's end, 1e-7 of it -- the logpdf call is what this case is about; its Wb = 64 is
    # short for the posterior call, which is declined by the backward check alone)
    t.append(case("B-x0-not-stationary-d3", "B", 3, 2053, force=(64, 256, 64), x0=1, post=(0, 2, 1)))
    t.append(case("B-draw-seam-d3-T2480", "B", 3, 2480, what="draw", fast=True, force=f8))
    t.append(case("B-draw-seam-d3-T2481", "B", 3, 2481, what="draw", fast=True, force=f8))
    t.append(case("B-draw-seam-d4-T2481", "B", 4, 2481, what="draw", fast=True, force=f8))
    t.append(case("B-draw-warm-5-chunks-d3", "B", 3, 256 * 63 + 1, what="draw", force=(256, 1280, 256)))
    # ---- C: long gaps at a chunk boundary (s = 2048 at C = 256), T = 4096, no other step missing.  Sizes and seeds: those whose host distances keep the
    # margin (module docstring of tests/test_gpu_sweep_edges.py); (served, status, attempts) as the host found them
    s, long_ = 2048, (256, 512, 256)
    two, dec = (1, 0, 2), lambda bits: (0, bits, 1)      # noqa: E731
    gaps = [  # d, seed, name, mask, short geometry, short lp / post, auto lp / post
        (3, 903, "behind350", (("range", s, s + 350),), (256, 112, 104), OK, dec(2), two, two),
        (3, 903, "before400", (("range", s - 400, s),), (256, 112, 104), dec(1), dec(1), two, two),
        (3, 903, "across200", (("range", s - 100, s + 100),), (256, 112, 104), dec(1), dec(3), two, two),
        (3, 903, "ends120", (("ends", 120),), (256, 112, 104), dec(1), dec(3), two, two),
        (3, 903, "chunks1024-2048", (("range", 1024, 2048),), (256, 112, 104), OK, OK, two, two),
        (4, 904, "behind400", (("range", s, s + 400),), (256, 144, 144), OK, dec(2), OK, OK),
        (4, 904, "before150", (("range", s - 150, s),), (256, 144, 144), dec(1), dec(1), OK, OK),
        (4, 904, "across400", (("range", s - 200, s + 200),), (256, 96, 96), dec(1), dec(3), OK, OK),
        (4, 904, "ends120", (("ends", 120),), (256, 112, 112), dec(1), dec(3), OK, OK),
        (4, 904, "chunks1024-3072", (("range", 1024, 3072),), (256, 96, 96), dec(1), dec(3), OK, OK),
        (1, 901, "ends170", (("ends", 170),), (256, 32, 32), dec(1), dec(3), (1, 0, 4), (1, 0, 4)),
        (2, 902, "ends120", (("ends", 120),), (256, 80, 72), dec(1), dec(3), two, two),
    ]
    for d, seed, nm, mask, short, slp, spost, alp, apost in gaps:
        if short is not None:
            t.append(case(f"C-{nm}-d{d}-short", "C", d, 4096, mask=mask, force=short, seed=seed, lp=slp, post=spost))
        t.append(case(f"C-{nm}-d{d}-long", "C", d, 4096, mask=mask, force=long_, seed=seed))
        if alp is not None:
            t.append(case(f"C-{nm}-d{d}-auto", "C", d, 4096, mask=mask, seed=seed, lp=alp, post=apost))
    # the plan's "forward warm-up longer than four chunks": a logpdf call doubles W alone (80 -> 160 -> 320 > 4 x 72); the posterior call grows C with Wb
    t.append(case("C-decline-plan-d2", "C", 2, 4096, mask=(("ends", 800),), seed=902, lp=(0, 1, 2), post=(1, 0, 3)))
    t.append(case("C-draw-behind350-d3", "C", 3, 4096, what="draw", mask=(("range", s, s + 350),), seed=903, draw=(1, 0, 2)))
    t.append(case("C-draw-before400-d3", "C", 3, 4096, what="draw", mask=(("range", s - 400, s),), seed=903, draw=(1, 0, 2)))
    # ---- D: ties (gaps of exactly 0), SDE form, T = 2400, 15 % missing on top
    for d, seed, exp in ((1, 2, two), (2, 1, OK), (4, 1, OK)):
        t.append(case(f"D-ties-d{d}", "D", d, 2400, sde=True, ties=1, mask=(("random", 0.15),), seed=seed, lp=exp, post=exp))
    # (d = 3 at the automatic geometry: seeds 1 .. 39 all leave a distance within a factor 10 of a tolerance -- the ties shorten the time W steps cover;
    # the forced geometry keeps the margin and runs the same tie arithmetic, missing tied steps included)
    t.append(case("D-ties-d3-forced", "D", 3, 2400, sde=True, ties=1, mask=(("random", 0.15),), force=long_, seed=1))
    t.append(case("D-ties-observed-d3", "D", 3, 2400, sde=True, ties=2, mask=(("random", 0.15),), seed=24))
    # ---- E: values that must not be served (forced geometry: the step sits in the middle of a chunk / is a chunk's first / last step)
    for nm, bad, xs, bits in (("negR-mid", ("negR", 2148), 1, 12), ("negR-edge", ("negR", 2048), 1, 12), ("inf-mid", ("inf", 2148), 0, 8),
                              ("inf-edge", ("inf", 2048), 0, 8), ("inf-last-of-chunk", ("inf", 2047), 0, 8)):
        # (10 % missing: a fully observed LTI series with one noise variance is the stationary-gain engines', the sweep engine is never asked)
        t.append(case(f"E-{nm}-d3", "E", 3, 4096, xs=xs, force=long_, bad=bad, lp=dec(bits), post=dec(bits)))
        t.append(case(f"E-draw-{nm}-d3", "E", 3, 4096, what="draw", xs=xs, force=long_, bad=bad, draw=dec(bits & ~8 if bits & 4 else bits)))
    # ---- F: the engine's own state
    t.append(case("F-ckpt-C64-d3", "F", 3, 4100, fast=True, force=(64, 8, 8), seed=77))
    t.append(case("F-ckpt-C2048-d3", "F", 3, 4100, fast=True, force=(2048, 8, 8), seed=77))
    t.append(case("F-part-2050-waves-d1", "F", 1, 8 * 62 * 2049 + 3, fast=True, force=f8))
    return t


@functools.lru_cache(maxsize=None)
def _times(c):
    """regular: the oracle's ("regular", 0, dt, T);  sde: time stamps with gaps U(0.5, 1.5) dt (fast spacing: U(0.9, 1.1) dt).  ties: a fifth of the gaps
    exactly 0, among them step 1, the last step, sixteen in a row from step 800 (two whole blocks of eight, four of four) and the first steps of the second
    and fourth chunk (C forced, or the automatic geometry's, which two more ties do not move: the host test asserts it)."""
    dt = (FAST_DT if c.fast else WORK_DT)[c.d]
    if not c.sde:
        return ("regular", 0.0, dt, c.T), None
    rng = np.random.default_rng(c.seed + 1)
    gaps = rng.uniform(0.9 * dt, 1.1 * dt, c.T) if c.fast else rng.uniform(0.5 * dt, 1.5 * dt, c.T)
    tie = None
    if c.ties:
        tie = rng.random(c.T) < 0.2
        tie[0] = False
        tie[1] = tie[c.T - 1] = True
        tie[800:816] = True
        g0 = np.where(tie, 0.0, gaps)      # (the plan reads the median gap: the ties move it, two more do not)
        t0 = np.cumsum(g0)
        C = c.force[0] if c.force else U.sweepsim_run(oc.build_lgssm(MODELS[c.d], t0, S2), np.zeros(c.T), post=False,
                                                      sde=(U.kernel_sde(MODELS[c.d])[0], t0), num_cu=NUM_CU)["C"]
        tie[C] = tie[3 * C] = True
        gaps[tie] = 0.0
    return np.cumsum(gaps), tie


def _mask(c, rng, tie):
    mk = np.zeros(c.T, dtype=bool)
    for m in c.mask:
        if m[0] == "random":
            mk |= rng.random(c.T) < m[1]
        elif m[0] == "range":
            mk[m[1]:m[2]] = True
        elif m[0] == "ends":
            mk[:m[1]] = True
            mk[c.T - m[1]:] = True
    if c.ties == 2:      # duplicate training inputs: both steps of every tie observed
        mk[tie] = False
        mk[np.nonzero(tie)[0] - 1] = False
    return mk if c.mask else None


def _key(c):
    """the fields the inputs depend on: cases that differ in their forced geometry or expectations share inputs and references"""
    return c._replace(name="", group="", force=c.force if c.ties else None, lp=None, post=None, draw=None)      # (the ties sit on the chunk boundaries)


def inputs(c):
    return _inputs(_key(c))


def reference(c):
    return _reference(_key(c))


def draw_reference(c):
    return _draw_reference(_key(c))


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """dict(model (oracle convention), y, mk (or None), Rn, t (time stamps or None), S (noise variance(s) the model was built with), mean (a function of the
    inputs or None), eps (the draw's), F (the drift, SDE form))"""
    rng = np.random.default_rng(c.seed)
    k = MODELS[c.d]
    t, tie = _times(c)
    S = S2 * (0.5 + rng.random(c.T)) if c.xs & 1 else S2
    mean = (lambda v: np.sin(0.3 * np.asarray(v))) if c.xs & 2 else None
    long_ = c.T > 20000      # (the oracle's NumPy draw of y is a Python loop: above this the model is built short and y drawn by the C restatement)
    model, y, _ = U.gp_case(k, ("regular", 0.0, t[2], 64) if long_ else t, S, seed=c.seed, mean=None if mean is None else ("custom", mean))
    if long_:
        assert not c.sde and c.xs == 0
        model = dict(model, T=c.T)
        y = sk.rand(model, rng.standard_normal((c.T, c.d)), rng.standard_normal(c.T), rng.standard_normal(c.d))
    if c.x0:
        assert not c.sde      # (the SDE form starts from the stationary prior by construction)
        model = dict(model, x0m=np.array([1.0, -2.0, 0.5, 1.5])[:c.d], x0P=0.3 * model["x0P"])
    mk = _mask(c, rng, tie)
    Rn = rng.random(c.T) * 0.05 if (c.xs & 1 or c.what == "draw") else np.array([1e-18])
    eps = (rng.standard_normal((c.T, c.d)), rng.standard_normal(c.T), rng.standard_normal(c.d)) if c.what == "draw" else None
    if c.bad is not None:
        kind, step = c.bad
        if kind == "negR":      # an innovation variance H' P H + R <= 0 at one step
            assert c.xs & 1
            S = S.copy()
            S[step] = -50.0
            model = dict(model, R=S)
        else:
            y = y.copy()
            y[step] = np.inf
        if mk is not None:
            mk[step] = False      # (the step is observed)
    F = U.kernel_sde(k)[0] if c.sde else None
    return dict(model=model, y=y, mk=mk, Rn=Rn, t=t if c.sde else None, S=S, mean=mean, eps=eps, F=F, tie=tie)


def _sim_kw(c, i):
    kw = dict(missing=i["mk"], Rnew=i["Rn"], num_cu=NUM_CU)
    if c.sde:
        kw["sde"] = (i["F"], i["t"])
    return kw


@functools.lru_cache(maxsize=None)
def host(c, post=True):
    """the call on the host: sweepsim_served (k) / sweepdrawsim_served (draw) on the case's inputs and forced geometry"""
    i = inputs(c)
    y0 = np.where(i["mk"], 0.0, i["y"]) if i["mk"] is not None else i["y"]
    C, W, Wb = c.force or (0, 0, 0)
    if c.what == "k":
        return U.sweepsim_served(i["model"], y0, C=C, W=W, Wb=Wb, post=post, **_sim_kw(c, i))
    kw = _sim_kw(c, i)
    if c.force:
        r = SD.sweepdrawsim_run(i["model"], y0, i["eps"], C=C, W=W, Wd=Wb, **kw)
        r["attempts"] = 1
    else:
        r = SD.sweepdrawsim_served(i["model"], y0, i["eps"], **kw)
    r["served"] = int(r["rc"] == 0 and r["status"] == 0)
    return r


@functools.lru_cache(maxsize=None)
def _reference(c):
    """(logpdf, mean, var) of the oracle: oracle/lgssm_ref.py, the C restatement above 6000 steps (missing steps as the reference has them: y := 0,
    R := 1e15, compensated volume), as tests/test_gpu_sweep.py"""
    i = inputs(c)
    model, y, mk, T = i["model"], i["y"], i["mk"], c.T
    Rn = np.broadcast_to(i["Rn"], (T,)).copy()
    if T > 6000:
        m2, y0, comp = model, y, 0.0
        if mk is not None:
            R = np.broadcast_to(np.atleast_1d(model["R"]), (T,)).copy()
            R[mk] = 1e15
            m2, y0, comp = dict(model, R=R), np.where(mk, 0.0, y), ref.volume_compensation(int(mk.sum()))
        return (sk.logpdf(m2, y0) + comp,) + tuple(sk.posterior_marginals(m2, y0, Rn))
    if mk is not None:
        lp, post = ref.logpdf_missing(model, y, mk), ref.posterior_missing(model, y, mk)
    else:
        lp, post = ref.logpdf(model, y), ref.posterior(model, y)
    return (lp,) + tuple(ref.marginals(ref.replace_observation_noise_cov(post, Rn)))


@functools.lru_cache(maxsize=None)
def _draw_reference(c):
    i = inputs(c)
    return SD.draw_restated(i["model"], i["y"], i["mk"], i["Rn"], i["eps"])


def margins_hold(tries, post=True):
    """every attempt's distances keep MARGIN from their tolerances (tries: sweepsim_served's / sweepdrawsim_served's)"""
    return all(margin_ok(f, TOL_F, bool(st & 1)) and (not post or margin_ok(b, TOL_B, bool(st & 2))) for _, _, _, st, f, b in tries)


def margin_ok(dist, tol, failed):
    """a host distance at least MARGIN on the intended side of its tolerance: rounding differences between host and device cannot flip the outcome"""
    return dist >= MARGIN * tol if failed else dist <= tol / MARGIN


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)
