"""Shared by the streaming kernels' envelope tests (tests/test_stream_envelope_host.py, tests/test_gpu_stream_envelope.py): the case
table, the product's own host plan through scripts/modal_proto.plan, the input-normalised form of csrc/tgp_stream_form.hpp restated in NumPy, and the
host code's serving conditions restated as plain arithmetic.

Every case is a literal -- kernel spec for oracle.components.build_lgssm, spacing, noise variance, optional offsets -- with the plan values it is meant to
have.  The spacings were found once by bisection on the plan (the halo grows monotonically as the spacing shrinks) and are written down as numbers: the
tests assert the placement and never search.  Threshold pairs sit about half a percent of the spacing apart, four steps of warm-up either side of the
threshold: far enough that the last bits of a matrix exponential cannot move a case across it."""
import functools
import importlib.util
import os

import numpy as np

from oracle import components as oc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

M12, M32, M52 = ("matern12",), ("matern32",), ("matern52",)

# ---- the constants of the host code the placement is about (asserted against the sources by the host tier)
K_TILE_POST = 1024        # tgp_post.hpp kTile = 64 * kN
K_HALO_MAX = 1536         # tgp_steady_plan.hpp kHaloMax
K_N0_MAX = 623            # tgp_steady_plan.hpp kN0Max
K_TAIL_MAX = 2048         # tgp_steady_plan.hpp kTailMax
K_COND_MAX = 1e5          # tgp_steady_plan.hpp kCondMax
K_REL_MIN = 1e-8          # tgp_stream_form.hpp kRelMin
K_CLOSURE_AMP_MAX = 64.0  # tgp_stream_form.hpp kClosureAmpMax
OK, NOT_SETTLED, ILL_CONDITIONED, SLOW_MIXING = 0, 1, 4, 5      # tgp_steady_plan.hpp Why

LP_BAR, MV_BAR = 1e-10, 1e-8      # the project's bars: logpdf relative, mean / var times max(1, scale)


@functools.lru_cache(maxsize=None)
def proto():
    spec = importlib.util.spec_from_file_location("modal_proto", os.path.join(ROOT, "scripts", "modal_proto.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def model_of(case, T):
    """the oracle's model of a case at length T; offsets: a literal transition offset `a` (d values) and emission offset `h`"""
    model = oc.build_lgssm(case["kern"], ("regular", 0.0, case["dt"], T), case["s2"])
    if case.get("off"):
        a, h = case["off"]
        model["a"] = np.asarray(a, dtype=np.float64).reshape(np.asarray(model["a"]).shape).copy()
        model["h"] = np.full(np.asarray(model["h"]).shape, float(h))
    return model


@functools.lru_cache(maxsize=None)
def _plan(name):
    return proto().plan(model_of(BY_NAME[name], 20000), 20000)      # (head, halo and modal form do not depend on the length)


def plan_of(case):
    return _plan(case["name"])


# ---- csrc/tgp_stream_form.hpp in NumPy
def _partner(i, npair):
    return i ^ 1 if i < 2 * npair else i


def block_magnitudes(c, npair):
    """detail::scaling: a real mode by |c|, both members of a pair by the modulus of the complex number (c_0, c_1) stand for"""
    c = np.asarray(c, dtype=np.float64)
    return np.array([np.hypot(c[i & ~1], c[(i & ~1) + 1]) if i < 2 * npair else abs(c[i]) for i in range(len(c))])


def form_ratio(pl):
    """the smallest block magnitude over the largest, the smaller of the forward (fb) and the backward (gc) figure: the form declines below kRelMin"""
    f, g = block_magnitudes(pl["fb"], pl["npair"]), block_magnitudes(pl["gc"], pl["npair"])
    return min(f.min() / f.max(), g.min() / g.max())


def form_accepts(pl):
    f, g = block_magnitudes(pl["fb"], pl["npair"]), block_magnitudes(pl["gc"], pl["npair"])
    return bool(np.all(f >= K_REL_MIN * f.max()) and np.all(f > 0) and np.all(g >= K_REL_MIN * g.max()) and np.all(g > 0))


def normal_form(pl):
    """build(): the forward half -- w~ = fw B, the shift s from (I - M - e w~') s = B^-1 fa, h~ = hh + w~ . s.  Returns (w~, s, h~, M, e)"""
    d, np_ = pl["d"], pl["npair"]
    fb, fw, fa = pl["fb"], pl["fw"], pl["fa"]
    p = np.array([fb[i & ~1] if i < 2 * np_ else fb[i] for i in range(d)])
    q = np.array([-fb[(i & ~1) + 1] if i < 2 * np_ else 0.0 for i in range(d)])
    wt, b = np.zeros(d), np.zeros(d)
    for i in range(d):
        k = _partner(i, np_)
        if k == i:
            wt[i], b[i] = fw[i] * p[i], fa[i] / p[i]
        else:
            n2 = p[i] * p[i] + q[i] * q[i]
            wt[i] = fw[i] * p[i] + fw[k] * q[i] if i & 1 else fw[i] * p[i] - fw[k] * q[i]
            b[i] = (p[i] * fa[i] + q[i] * fa[k] if i & 1 else p[i] * fa[i] - q[i] * fa[k]) / n2
    M = np.zeros((d, d))
    for i in range(d):
        M[i, i] = pl["fd"][i]
        if _partner(i, np_) != i:
            M[i, _partner(i, np_)] = pl["fo"][i]
    e = np.array([0.0 if (_partner(i, np_) != i and i & 1) else 1.0 for i in range(d)])
    s = np.linalg.solve(np.eye(d) - M - np.outer(e, wt), b) if np.any(fa != 0.0) else np.zeros(d)
    return wt, s, pl["hh"] + wt @ s, M, e


def closure_amp(pl):
    """build(): amp = sum_i |w~_i| / |1 - lambda_i| -- what the logpdf kernel's quadratic closure of its first tile amplifies rounding by"""
    wt = normal_form(pl)[0]
    return float(np.sum(np.abs(wt) / np.hypot(1.0 - np.asarray(pl["fd"]), np.asarray(pl["fo"]))))


def state_spread(pl, y):
    """the largest standard deviation, over the components, of the normal form's forward state along the series y (behind the head)"""
    wt, s, ht, M, e = normal_form(pl)
    x, xs = np.zeros(pl["d"]), []
    for t in range(len(y)):
        x = M @ x + e * (y[t] - ht)
        xs.append(x)
    return float(np.max(np.std(np.array(xs)[pl["nhs"]:], axis=0)))


# ---- who serves a call: tgp_modal.hip plan() / use_post_stream(), tgp_post.hip applies(), tgp_lml.hip choose_geometry(), with TGP_OPT_STREAM_MIN_T = 0
LML16, LML32, POST, STEADY, OTHER = "k_lml_stream<16>", "k_lml_stream<32>", "k_post_stream", "k_steady_one", "other"


def lml_tile(pl):
    """choose_geometry: g.n = d <= 1 ? 16 : 32; if (64 * g.n < md.halo) g.n = 32 -- the tile is 64 g.n steps"""
    n = 16 if pl["d"] <= 1 else 32
    if 64 * n < pl["halo"]:
        n = 32
    return 64 * n


def server(pl, T, posterior):
    """the kernel family that must serve a call of T steps (every series-sized buffer on a 16-byte boundary, as NumPy and torch allocate them)"""
    if pl["why"] != OK or pl["nhs"] + 2 > T:      # build_core: kTooShort
        return OTHER
    # without the tables behind the launch (`deferred`: T >= nhs + kTailMax + 1) plan() builds them first, and they decline a series shorter than
    # head + variance transient: build_tables_tail, nhs + n1 + 1 > T
    deferred = T >= pl["nhs"] + K_TAIL_MAX + 1
    steady = STEADY if deferred or pl["nhs"] + pl["n1"] + 1 <= T else OTHER
    if not form_accepts(pl):
        return steady
    if not posterior:      # plan(): logpdf_only && sf.ok && sf.amp <= kClosureAmpMax -- no tables, any length the core accepts
        return (LML16 if lml_tile(pl) == 1024 else LML32) if closure_amp(pl) <= K_CLOSURE_AMP_MAX else steady
    # use_post_stream(): the head on the host (hosthead = deferred) and tgp_post::applies (d <= 3, halo <= kTile, T - nhs >= 1)
    if deferred and pl["d"] <= 3 and pl["halo"] <= K_TILE_POST:
        return POST
    return steady


def lengths(pl, tile):
    """the lengths of a case from its own head, halo and tile; all below 10 000"""
    nhs, halo = pl["nhs"], pl["halo"]
    out = [nhs + 2, nhs + halo - 1, nhs + halo + 1, nhs + tile + 1, nhs + 2 * tile + 37, nhs + 3 * tile]
    out = sorted(set(T for T in out if T >= nhs + 2))
    assert out[-1] < 10000
    return out


# ---- the table
K6 = ("sum", M52, ("stretched", 0.4, M52))                                 # d = 6, as tests/test_gpu_stream_form.py KERNELS[6]
W4 = ("sum", M32, ("stretched", 0.4, M32))                                 # d = 4: two Matern-3/2 terms, two conjugate pairs under heavy noise
S6 = ("sum", ("stretched", 0.4, M52), ("scaled", 0.01, M52))               # d = 6: a slow term and a faint fast one -- the slowest mode carries the smoother's weight
OFF_REAL, OFF_PAIR = ((600.0, -200.0, 400.0), 1000.0), ((120.0, -40.0, 80.0), 1000.0)      # transition offset a, emission offset h
SERVED, NO_COND = (K_REL_MIN, 1.0 + 1e-12), (0.99, 1e4)


def _case(group, name, kern, dt, s2, why=OK, halo=None, n0=None, npair=None, cond=NO_COND, ratio=SERVED, off=None, amp=(0.0, K_CLOSURE_AMP_MAX)):
    return dict(group=group, name=name, kern=kern, dt=dt, s2=s2, off=off, why=why, halo=halo, n0=n0, npair=npair, cond=cond, ratio=ratio, amp=amp)


def _halo(d, kern, s2, dts, n0s, npairs, ratio_min):
    """five spacings of one kernel at one noise variance: the smallest halo, 1024 (the last k_post_stream takes; need = 1019..1021 steps), 1040 (the
    first it hands to k_steady_one, at d = 1 the first on the 2048-step logpdf tile; need = 1028..1030), the cap's last 16 (need = 1529..1531) and the
    first model beyond the cap (need = 1542..1544 > kHaloMax)"""
    tags, halos = ("min", "1024", "1040", "cap", "beyond"), (16, 1024, 1040, 1536, None)
    return [_case("halo", f"halo_d{d}_{t}", kern, dt, s2, why=SLOW_MIXING if h is None else OK, halo=h, n0=(n - 8, n + 8), npair=p,
                  ratio=(ratio_min if t == "min" else SERVED) if h else None)
            for t, h, dt, n, p in zip(tags, halos, dts, n0s, npairs)]


CASES = (
    # -- halo.  The smallest halo is reached at a spacing of several length scales, where the fast modes are barely excited: those cases double as
    #    natural weak-input ones (ratios 3e-3 .. 4e-3 at d = 2, 3, 6) and are placed on the ratio as well.  Noise variance 0.1 at d = 1, 2; at d = 3
    #    and d = 6 noise variance 1, and at d = 6 the sum S6: with 0.1, and with the sum K6 at any noise, the slowest mode decides the halo but carries
    #    so little of the smoother's weight that an observation moves the mean 256 steps away by 3e-7 (d = 3, cap) and 4e-10 .. 5e-9 (K6) only --
    #    long on paper, not in effect (tests/test_stream_envelope_host.py test_the_long_halo_cases_really_are_long).
    _halo(1, M12, 0.1, (1.0, 9.46e-5, 9.31e-5, 4.2e-5, 4.14e-5), (7, 386, 389, 571, 575), (0, 0, 0, 0, 0), SERVED)
    + _halo(2, M32, 0.1, (4.0, 0.004062, 0.004021, 0.00237, 0.002347), (5, 386, 385, 568, 571), (0, 1, 1, 1, 1), (1e-3, 1e-2))
    + _halo(3, M52, 1.0, (4.0, 0.01521, 0.01506, 0.009514, 0.009421), (4, 386, 389, 575, 577), (0, 1, 1, 1, 1), (1e-3, 1e-2))
    + _halo(6, S6, 1.0, (4.0, 0.03545, 0.03507, 0.02164, 0.02142), (7, 384, 384, 569, 574), (2, 2, 2, 2, 2), (1e-3, 1e-2))
    + [
        # -- head.  n0 >= 560 needs a slowly settling covariance under the halo cap: n0 / halo is about 0.37 for these kernels, so only the last
        #    halos reach it.  At d = 6 the sum K6 stops at n0 = 509..532 under the cap at every noise variance tried (1e-3 .. 10; below, the covariance
        #    no longer settles within kN0Max steps and the plan declines with kNotSettled before the halo is looked at); S6 reaches 563.  The smallest n0 is 2 (a spacing of 16 length scales); at d = 6 the smallest with the form still
        #    serving is 4 (beyond a spacing of 8 the fastest block's input coefficient falls below kRelMin).
        _case("head", "head_d3_long", M52, 0.0027, 1e-3, halo=1504, n0=(560, K_N0_MAX), npair=1),
        _case("head", "head_d6_long", S6, 0.0219, 1.0, halo=1520, n0=(560, K_N0_MAX), npair=2),
        _case("head", "head_d3_short", M52, 16.0, 10.0, halo=16, n0=(2, 2), npair=0, ratio=(1e-4, 1e-3)),
        _case("head", "head_d6_short", K6, 8.0, 10.0, halo=16, n0=(3, 5), npair=1, ratio=(1e-7, 1e-5)),
        # -- conditioning: max(cond_f, cond_g) in [1e4, 1e5].  d = 3: a Matern-5/2 closed loop 1e-6 in the spacing past the point where its conjugate
        #    pair turns into two real modes (0.32827786...; within 2e-7 of that point the plan's residual rule declines at cond 5e4, further out it
        #    serves).  d = 4 .. 8: two nearly identical terms.  The pair around kCondMax: 8.4e4 and 1.1e5.
        #    That d = 3 case is the table's finding: k_lml_stream missed the logpdf bar on it (2.7e-10 at nhs + 2, 1.5e-9 absolute), where its
        #    two nearly coincident real modes make the normal form's w~ 1e3 with alternating signs and the kernel's quadratic closure of the first
        #    tile loses amp^2 = 3.5e6 (tgp_stream_form.hpp kClosureAmpMax).  It stays in the table on the declined side of that guard for logpdf
        #    (k_post_stream, which has no such closure, serves its posterior call at 2e-14), with a pair around the guard 1e-3 and 3e-4 from the
        #    point: amp = 59 and 106.
        _case("cond", "cond_d3", M52, 0.3282788608, 1e-3, halo=32, n0=(9, 25), npair=0, cond=(1e4, 1e5), amp=(1e3, 3e3)),
        _case("cond", "amp_in", M52, 0.3292778608, 1e-3, halo=32, n0=(8, 24), npair=0, amp=(40.0, K_CLOSURE_AMP_MAX)),
        _case("cond", "amp_beyond", M52, 0.3285778608, 1e-3, halo=32, n0=(8, 24), npair=0, amp=(K_CLOSURE_AMP_MAX, 150.0)),
        _case("cond", "cond_d4", ("sum", M32, ("stretched", 0.9997, M32)), 0.1, 0.1, halo=272, n0=(42, 58), npair=2, cond=(1e4, 1e5), ratio=(1e-5, 1e-4)),
        _case("cond", "cond_d5", ("sum", M32, ("stretched", 0.9997, M32), M12), 0.1, 0.1, halo=416, n0=(126, 142), npair=1, cond=(1e4, 1e5), ratio=(1e-5, 1e-4)),
        _case("cond", "cond_d6", ("sum", M52, ("stretched", 0.97, M52)), 0.1, 0.1, halo=208, n0=(56, 72), npair=2, cond=(1e4, 1e5)),
        _case("cond", "cond_d7", ("sum", M52, ("stretched", 0.97, M52), M12), 0.1, 0.1, halo=416, n0=(126, 142), npair=2, cond=(1e4, 1e5)),
        _case("cond", "cond_d8", ("sum", M52, ("stretched", 0.97, M52), M32), 0.1, 0.1, halo=256, n0=(75, 91), npair=3, cond=(1e4, 1e5)),
        _case("cond", "cond_d6_in", ("sum", M52, ("stretched", 0.983, M52)), 0.1, 0.1, halo=208, n0=(54, 70), npair=2, cond=(5e4, 1e5)),
        _case("cond", "cond_d6_beyond", ("sum", M52, ("stretched", 0.985, M52)), 0.1, 0.1, why=ILL_CONDITIONED, cond=(1e5, 2e5), ratio=None),
        # -- weak mode.  A faint Matern-1/2 summand is a real mode.  A faint Matern summand is never a member of a conjugate pair: its closed loop is
        #    its open loop, whose eigenvalues are real (a faint Matern-3/2 term gives two real modes with input coefficients of opposite sign and
        #    ordinary size, ratio 0.17, until the plan declines it as ill conditioned).  The weak PAIR is therefore the fast term of W4 at a spacing
        #    of 8 and 12 length scales under noise variance 10, where both terms are pairs and the fast one is excited 5e-4 and 8e-6 as much.
        #    The pair around kRelMin: ratios 1.2e-8 (served) and 8.4e-9 (k_steady_one serves both calls).
        _case("weak", "weak_real_lo", ("sum", M32, ("scaled", 1e-6, M12)), 0.1, 0.1, halo=448, n0=(70, 86), npair=1, ratio=(1e-7, 1e-5)),
        _case("weak", "weak_real_hi", ("sum", M32, ("scaled", 1e-2, M12)), 0.1, 0.1, halo=448, n0=(116, 132), npair=1, ratio=(1e-4, 1e-2)),
        _case("weak", "weak_pair_lo", W4, 12.0, 10.0, halo=16, n0=(3, 5), npair=2, ratio=(1e-7, 1e-5)),
        _case("weak", "weak_pair_hi", W4, 8.0, 10.0, halo=16, n0=(4, 6), npair=2, ratio=(1e-4, 1e-2)),
        _case("weak", "relmin_in", ("sum", M32, ("scaled", 2.5e-12, M12)), 0.1, 0.1, halo=448, n0=(30, 46), npair=1, ratio=(K_REL_MIN, 1.5e-8)),
        _case("weak", "relmin_below", ("sum", M32, ("scaled", 1.2e-12, M12)), 0.1, 0.1, halo=448, n0=(30, 46), npair=1, ratio=(5e-9, K_REL_MIN)),
        # -- noise variance over signal variance (1 for a Matern kernel) at d = 3
        _case("noise", "noise_1e-6", M52, 0.1, 1e-6, halo=48, n0=(13, 29), npair=0, amp=(30.0, 50.0)),
        _case("noise", "noise_1e-4", M52, 0.1, 1e-4, halo=64, n0=(13, 29), npair=1),
        _case("noise", "noise_10", M52, 0.1, 10.0, halo=240, n0=(79, 95), npair=1),
        _case("noise", "noise_1e3", M52, 0.1, 1e3, halo=224, n0=(78, 94), npair=1),
        # -- offsets on the all-real and the one-pair closed loop of tests/test_gpu_stream_form.py: the stationary mean of the series is 2e3 and 2.5e3
        #    standard deviations from zero, the form's shift 8e3 and 2e3 spreads of its state.  (The one-pair case was first tried at five times
        #    these offsets, 8.5e3 standard deviations: the host harness then measures 1.8e-12 between the two recursions, over its 1e-12 -- the loss
        #    is the plan-coordinate side's, whose input y - hh is 7.5e3 against innovations of order one; it grows in proportion to the offset.)
        _case("offsets", "offsets_all_real", M52, 1.0, 1e-3, halo=48, n0=(8, 24), npair=0, ratio=(1e-3, 1e-2), off=OFF_REAL),
        _case("offsets", "offsets_one_pair", M52, 0.1, 0.1, halo=160, n0=(50, 66), npair=1, off=OFF_PAIR),
    ])
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SERVED_CASES = [c for c in CASES if c["why"] == OK]
# threshold pairs: (the last model inside, the first beyond)
PAIRS = [(f"halo_d{d}_1024", f"halo_d{d}_1040") for d in (1, 2, 3, 6)] + [(f"halo_d{d}_cap", f"halo_d{d}_beyond") for d in (1, 2, 3, 6)] + [
    ("cond_d6_in", "cond_d6_beyond"), ("relmin_in", "relmin_below"), ("amp_in", "amp_beyond")]


def case_lengths(case, posterior):
    """lengths of a served case for the logpdf call (its own tile) or the posterior call (tile 1024)"""
    pl = plan_of(case)
    return lengths(pl, K_TILE_POST if posterior else lml_tile(pl))


def declined_lengths(case):
    """a case the plan declines has no head, halo or tile of its own: the lengths of its partner inside the threshold"""
    inside = next(a for a, b in PAIRS if b == case["name"])
    pl = plan_of(BY_NAME[inside])
    return lengths(pl, lml_tile(pl))


# ---- series and the oracle's answers: computed once, shared, never written to
RN = np.array([0.3])


def rnew_per_step(T):
    return 0.05 + np.random.default_rng(T).random(T)


@functools.lru_cache(maxsize=None)
def series(name, T):
    model = model_of(BY_NAME[name], T)
    d = len(model["x0m"])
    rng = np.random.default_rng(T + d)
    from oracle import seq_kalman as sk
    y = sk.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    y.setflags(write=False)
    return model, y


@functools.lru_cache(maxsize=None)
def reference(name, T, posterior=True):
    """(logpdf, mean, var under the shared RN, var under rnew_per_step(T)) of the oracle's sequential filter / smoother in double"""
    from oracle import seq_kalman as sk
    model, y = series(name, T)
    lp = sk.logpdf(model, y)
    if not posterior:
        return lp, None, None, None
    mean, var = sk.posterior_marginals(model, y, RN)
    _, var_t = sk.posterior_marginals(model, y, rnew_per_step(T))
    for a in (mean, var, var_t):
        a.setflags(write=False)
    return lp, mean, var, var_t


def all_lengths(case):
    """every length a case is run at, either call"""
    if case["why"] != OK:
        return declined_lengths(case)
    return sorted(set(case_lengths(case, False)) | (set(case_lengths(case, True)) if plan_of(case)["d"] <= 3 else set()))
