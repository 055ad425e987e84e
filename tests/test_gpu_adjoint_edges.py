"""GPU tier: logpdf + block gradients by ONE adjoint pass (tgp_logpdf_adjoint) at d <= 8, placed on the edges of the two device paths that serve it,
against the oracle's exact sequential adjoint in long double (oracle/seq_adjoint.py; tests/test_oracle_adjoint.py holds it to 1.1e-14 of the
50-digit gradient). Bars: logpdf 1e-10 relative to seq_kalman.logpdf, every entry of every block gradient 1e-8 of the largest entry of the
reference gradient (the project's gradient bar, tests/test_gpu_gradient.py).

Geometry of k_adjoint_one (csrc/tgp_powers.hip, d <= 6; launch_adjoint and the kernel's first lines), on the plan of tgp_plan::build_filter:
  * a span is 8 waves x 64 lanes x 8 steps = 4096 steps; a lane loads its 8 steps with 16-byte loads when t0 + 8 <= T and y is 16-byte aligned,
    one by one otherwise;
  * a workgroup owns C = 4096 - 2 halo steps behind the head (nhs steps, run on the host): [nhs + g C, nhs + (g + 1) C), and starts `halo` steps early from
    a zero state -- or AT the head, from the head's end state, when that start would lie in front of it (`from_head`: the first workgroup always, the
    second one too when C < halo, i.e. halo >= 1376);
  * nwg = ceil((T - nhs) / C) workgroups, mapped to blocks in 8 groups of per = ceil(nwg / 8): block b serves g = (b & 7) per + (b >> 3), blocks with
    g >= nwg are empty;
  * waves (512-step tiles) chain over at most three tiles behind / in front of them: Phi^512 (PT[0]) and Phi^1024 (PT[1]) -- halo <= 1536;
  * the sums count a step when c_lo <= t < min(c_lo + C, T) (`own`).
Geometry of the five-launch pass (csrc/tgp_steady.hip: k_steady_setup / reduce / carry / apply<adjoint> / final<adjoint>; d = 7, 8 and what the filter
plan declines): 512-step tiles, a head of th = n0 // 512 + 1 <= 4 tiles, kBlkThreads / 64 = 8 tiles (4096 steps) per workgroup.

Classes (model = oracle.components.build_lgssm(kernel, dt, noise) with a and h set non-zero; nhs and halo as tgp_filter_plan reports them -- asserted):

    class            kernel                                   dt     noise   d   n0    nhs   halo    C      serves
    tiny_d1          Matern-1/2                               0.1    0.1     1   15    16    32      4032   k_adjoint_one
    one_tile_d2      Matern-3/2                               0.01   0.1     2   196   208   512     3072   k_adjoint_one
    one_tile_d3      Matern-5/2                               0.03   0.5     3   200   208   512     3072   k_adjoint_one
    two_three_d5     Matern-5/2 + Matern-3/2                  0.02   0.1     5   375   384   1232    1632   k_adjoint_one
    from_head_d2     Matern-3/2                               0.01   10      2   550   560   1408    1280   k_adjoint_one
    from_head_d3     Matern-5/2                               0.01   1.0     3   551   560   1440    1216   k_adjoint_one
    three_tiles_d3   Matern-5/2                               0.01   1.5     3   558   560   1536    1024   k_adjoint_one   (the longest halo served)
    sum_d4           Matern-5/2 + Matern-1/2                  0.05   0.1     4   250   256   736     2624   k_adjoint_one
    stretched_d6     Matern-5/2 + stretched(0.4) Matern-5/2   0.05   0.1     6   351   352   992     2112   k_adjoint_one
    identical_d6     Matern-5/2 + Matern-5/2                  0.05   0.1     6   95    96    448     3200   k_adjoint_one

profiles/adjoint_edges_parity.txt keeps the largest deviation seen per class and block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import components as oc
from oracle import seq_adjoint as sa
from oracle import seq_kalman as sk
from tests import _util as U

pytestmark = pytest.mark.gpu

SPAN = 8 * 64 * 8            # k_adjoint_one: waves x lanes x steps per lane
TILE = 512                   # both paths: steps per wave
BLK = 8 * TILE               # the five-launch pass: kBlkThreads / 64 tiles per workgroup
BLOCKS = ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")
LP_BAR, GRAD_BAR = 1e-10, 1e-8
FIVE = {"k_steady_setup", "k_steady_reduce<adjoint>", "k_steady_carry<adjoint>", "k_steady_apply<adjoint>", "k_steady_final<adjoint>"}

M12, M32, M52 = ("matern12",), ("matern32",), ("matern52",)
#                 kernel, dt, noise, (n0, nhs, halo) as the plan reports them (nhs and halo are asserted: they place every length below)
CLASSES = {
    "tiny_d1": (M12, 0.1, 0.1, (15, 16, 32)),
    "one_tile_d2": (M32, 0.01, 0.1, (196, 208, 512)),
    "one_tile_d3": (M52, 0.03, 0.5, (200, 208, 512)),
    "two_three_d5": (("sum", M52, M32), 0.02, 0.1, (375, 384, 1232)),
    "from_head_d2": (M32, 0.01, 10.0, (550, 560, 1408)),
    "from_head_d3": (M52, 0.01, 1.0, (551, 560, 1440)),
    "three_tiles_d3": (M52, 0.01, 1.5, (558, 560, 1536)),
    "sum_d4": (("sum", M52, M12), 0.05, 0.1, (250, 256, 736)),
    "stretched_d6": (("sum", M52, ("stretched", 0.4, M52)), 0.05, 0.1, (351, 352, 992)),
    "identical_d6": (("sum", M52, M52), 0.05, 0.1, (95, 96, 448)),
}
_CACHE = {}


def blocks_of(spec, dt, noise):
    """the shared blocks of the class's model, with non-zero a and h (the kernels' a and hh terms are otherwise multiplied by zero)"""
    model = oc.build_lgssm(spec, ("regular", 0.0, dt, 4), noise)
    d = len(model["x0m"])
    model["a"] = 0.01 * np.linspace(-1.0, 1.0, d)[None] if d > 1 else np.array([[0.01]])
    model["h"] = np.array([0.4])
    return model


def filter_plan(model, T):
    """why, n0, nhs, halo of tgp_plan::build_filter for this model and length (the pure host function tgp_filter_plan)"""
    from temporalgps_jl_amd import _lib
    lib = _lib.load()
    d = len(model["x0m"])
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))      # noqa: E731
    blocks = [c(model["A"][0].T), c(model["a"][0]), c(model["Q"][0].T), c(model["H"][0]), c(np.atleast_1d(model["h"])[:1]),
              c(np.atleast_1d(model["R"])[:1]), c(model["x0m"]), c(model["x0P"].T)]
    info = np.zeros(4, dtype=np.int32)
    assert lib.tgp_filter_plan(d, *[b.ctypes.data for b in blocks], int(T), info.ctypes.data) == 0
    return dict(why=int(info[0]), n0=int(info[1]), nhs=int(info[2]), halo=int(info[3]))


def settle_n0(model, tol=4.5e-16):
    """the step from which the gains are stationary, by the criterion of tests/test_adjoint_host.py (device_like_record): what the five-launch pass's
    k_steady_setup finds; its head is n0 // 512 + 1 tiles"""
    A, Q, h, R = model["A"][0], model["Q"][0], model["H"][0], float(model["R"][0])
    P = model["x0P"].copy()
    settled = False
    for t in range(4 * TILE):
        Pp = A @ P @ A.T + Q
        v = Pp @ h
        s = h @ v + R
        if settled:
            return t
        Pn = Pp - np.outer(v, v) / s
        scale = 0.5 * (np.diag(Pp)[:, None] + np.diag(Pp)[None, :])
        settled = not np.any(np.abs(Pn - P) > tol * scale)
        P = Pn
    raise AssertionError("covariance did not settle")


def edge_lengths(nhs, halo):
    """the lengths of a class on k_adjoint_one's geometry (the declined nhs + 1 apart)"""
    C = SPAN - 2 * halo
    Ts = [nhs + 2, nhs + 7, nhs + 8, nhs + 9, nhs + 511, nhs + 512, nhs + 513, nhs + C - 1, nhs + C, nhs + C + 1, nhs + 2 * C - 1, nhs + 2 * C + 1,
          nhs + 2 * C + halo - 1, nhs + 2 * C + halo + 1, nhs + 8 * C + 1, nhs + 9 * C + 1]
    t3 = nhs + 3 * C + 40
    Ts.append(t3 + (3 - t3) % 8)          # one T = 3 (mod 8)
    return sorted(set(Ts))


class Case:
    """model blocks, one long draw and the oracle's gradients of a class, computed once per module"""

    def __init__(self, spec, dt, noise, Tmax):
        self.blocks = blocks_of(spec, dt, noise)
        self.d = len(self.blocks["x0m"])
        self.Tmax = int(Tmax)
        m = self.model(self.Tmax)
        rng = np.random.default_rng(17)
        self.y = sk.rand(m, rng.standard_normal((self.Tmax, self.d)), rng.standard_normal(self.Tmax), rng.standard_normal(self.d))
        self._ref = {}

    def model(self, T):
        m = dict(self.blocks)
        m["T"] = int(T)
        return m

    def ref(self, T, y=None):
        key = (int(T), None if y is None else y.tobytes()[:64])
        if key not in self._ref:
            yy = self.y[:T] if y is None else y
            m = self.model(T)
            self._ref[key] = (sk.logpdf(m, yy), sa.logpdf_adjoint(m, yy)[1])
        return self._ref[key]


def case_of(name):
    if name not in _CACHE:
        spec, dt, noise, _ = CLASSES[name]
        plan = filter_plan(blocks_of(spec, dt, noise), 10 ** 6)
        Tmax = 300_001 if name == "one_tile_d3" else (max(edge_lengths(plan["nhs"], plan["halo"])) if plan["why"] == 0 else 4 * BLK + 4 * TILE + 2)
        _CACHE[name] = (Case(spec, dt, noise, Tmax), plan)
    return _CACHE[name]


def deviations(lp, g, lp_ref, g_ref):
    """-> (relative deviation of the logpdf, {block: largest deviation relative to the largest entry of the reference gradient})"""
    scale = max(np.abs(np.asarray(g_ref[k])).max() for k in BLOCKS)
    return abs(lp - lp_ref) / abs(lp_ref), {k: float(np.abs(np.asarray(g[k]) - np.asarray(g_ref[k])).max() / scale) for k in BLOCKS}


def run_device(tgp, case, T, y=None, steady=None):
    """one fresh handle: (lp, gradient, profile names)"""
    from temporalgps_jl_amd import lgssm as L
    dm = U.device_model(tgp, case.model(T))
    if steady is not None:
        dm.handle_options[tgp._lib.OPT_STEADY] = steady
    (lp, g), names = U.kernels_of(tgp, dm, lambda: L.logpdf_adjoint(dm, case.y[:T] if y is None else y))
    return lp, g, names


def check(tgp, case, T, failures, worst, tag, want_names, steady=None, y=None, y_ref=None):
    lp, g, names = run_device(tgp, case, T, y=y, steady=steady)
    lp_ref, g_ref = case.ref(T, y_ref)
    dlp, dev = deviations(lp, g, lp_ref, g_ref)
    print(f"{tag} T={T}: lp {dlp:.1e} | " + " ".join(f"{k} {v:.1e}" for k, v in dev.items()) + f" | {sorted(names)}")
    for k, v in dev.items():
        worst[k] = max(worst.get(k, 0.0), v)
    worst["lp"] = max(worst.get("lp", 0.0), dlp)
    if not dlp <= LP_BAR:
        failures.append((tag, T, "lp", dlp))
    failures.extend((tag, T, k, v) for k, v in dev.items() if not v <= GRAD_BAR)
    if want_names == "one":
        if "k_adjoint_one" not in names or any(n.startswith("k_steady") for n in names):
            failures.append((tag, T, "engine", sorted(names)))
    elif not FIVE <= names or "k_adjoint_one" in names:
        failures.append((tag, T, "engine", sorted(names)))
    return g


# ------------------------------------------------------------------------------------------------ k_adjoint_one: span, halo and series edges
@pytest.mark.parametrize("name", list(CLASSES))
def test_one_launch_adjoint_at_span_halo_and_series_edges(name):
    import temporalgps_jl_amd as tgp
    case, plan = case_of(name)
    want = CLASSES[name][3]
    print(f"{name}: plan {plan}")
    assert plan["why"] == 0 and (plan["nhs"], plan["halo"]) == want[1:], (name, plan, want)      # the class, as the header's table records it
    nhs, halo = plan["nhs"], plan["halo"]
    C = SPAN - 2 * halo
    if name.startswith("from_head") or name == "three_tiles_d3":
        assert halo >= 1376 and C < halo          # T = nhs + C + 1 and longer: two or more workgroups, the second one too starts at the head
    failures, worst = [], {}
    # one step short of the shortest accepted series: another path or Unsupported, never a wrong value
    try:
        lp, g, names = run_device(tgp, case, nhs + 1)
        dlp, dev = deviations(lp, g, *case.ref(nhs + 1))
        print(f"{name} T={nhs + 1} (declined by the plan): lp {dlp:.1e} worst {max(dev.values()):.1e} | {sorted(names)}")
        assert "k_adjoint_one" not in names and dlp <= LP_BAR and max(dev.values()) <= GRAD_BAR, (nhs + 1, names, dlp, dev)
    except tgp._lib.Unsupported:
        print(f"{name} T={nhs + 1} (declined by the plan): Unsupported")
    assert filter_plan(case.blocks, nhs + 1)["why"] == 3 and -(-(nhs + C + 1 - nhs) // C) == 2      # (too short; and nhs + C + 1 below has two workgroups)
    Ts = edge_lengths(nhs, halo) + ([300_001] if name == "one_tile_d3" else [])
    for T in Ts:
        assert filter_plan(case.blocks, T) == plan            # (the plan does not depend on the length beyond "long enough")
        check(tgp, case, T, failures, worst, name, "one")
    print(f"{name}: worst " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ pointer alignment
@pytest.mark.parametrize("name", ["one_tile_d2", "from_head_d3", "stretched_d6"])
def test_series_on_the_device_eight_bytes_past_a_16_byte_boundary(name):
    """the lanes' 16-byte loads need a 16-byte aligned series: with y 8 bytes past such a boundary they must not be taken, the result is the same"""
    import torch
    import temporalgps_jl_amd as tgp
    case, plan = case_of(name)
    assert plan["why"] == 0
    T = plan["nhs"] + 2 * (SPAN - 2 * plan["halo"]) + 1
    buf = torch.zeros(T + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:T + 1] = torch.from_numpy(case.y[:T]).cuda()
    y_odd = buf[1:T + 1]
    assert y_odd.data_ptr() % 16 == 8 and y_odd.is_contiguous()
    failures, worst = [], {}
    g_odd = check(tgp, case, T, failures, worst, name + " (y + 8 bytes)", "one", y=y_odd)
    g_al = check(tgp, case, T, failures, worst, name + " (aligned)", "one", y=torch.from_numpy(case.y[:T]).cuda())
    assert not failures, failures
    scale = max(np.abs(np.asarray(g_al[k])).max() for k in BLOCKS)
    for k in BLOCKS:                                      # the same numbers through either load: the same sums in the same order
        assert np.abs(np.asarray(g_odd[k]) - np.asarray(g_al[k])).max() <= 1e-14 * scale, k


# ------------------------------------------------------------------------------------------------ call sequences on one handle
def test_three_series_on_one_handle_each_get_their_own_gradient():
    """the host / device hand-over of the head carries a sequence number: a second and third call on the handle must not read the first call's head"""
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lgssm as L
    case, plan = case_of("from_head_d3")
    T = plan["nhs"] + (SPAN - 2 * plan["halo"]) + 1
    dm = U.device_model(tgp, case.model(T))
    rng = np.random.default_rng(23)
    failures = []
    for i in range(3):
        y = case.y[:T] if i == 0 else case.y[i * 100:i * 100 + T] * (1.0 + 0.5 * i) + 0.3 * rng.standard_normal(T)
        lp, g = L.logpdf_adjoint(dm, y)
        dlp, dev = deviations(lp, g, *case.ref(T, None if i == 0 else y))
        print(f"series {i}: lp {dlp:.1e} worst {max(dev.values()):.1e}")
        if not (dlp <= LP_BAR and max(dev.values()) <= GRAD_BAR):
            failures.append((i, dlp, dev))
    assert not failures, failures


def test_adjoint_between_logpdf_and_posterior_calls_on_one_handle():
    """logpdf, posterior_marginals, logpdf_adjoint, logpdf_adjoint, posterior_marginals on ONE handle: the pinned head buffer and the hand-over flags are shared
    with the one-launch smoother"""
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lgssm as L
    case, plan = case_of("one_tile_d3")
    T = plan["nhs"] + 2 * (SPAN - 2 * plan["halo"]) + 1
    dm = U.device_model(tgp, case.model(T))
    y = case.y[:T]
    lp_ref, g_ref = case.ref(T)
    Rn = np.array([1e-18])
    mean_ref, var_ref = sk.posterior_marginals(case.model(T), y, Rn)
    assert abs(L.logpdf(dm, y) - lp_ref) <= LP_BAR * abs(lp_ref)
    mean, var = L.posterior_marginals(dm, y, Rn)
    assert np.abs(mean - mean_ref).max() <= 1e-8 and np.abs(var - var_ref).max() <= 1e-8
    for rep in range(2):
        dlp, dev = deviations(*L.logpdf_adjoint(dm, y), lp_ref, g_ref)
        assert dlp <= LP_BAR and max(dev.values()) <= GRAD_BAR, (rep, dlp, dev)
    mean, var = L.posterior_marginals(dm, y, Rn)
    assert np.abs(mean - mean_ref).max() <= 1e-8 and np.abs(var - var_ref).max() <= 1e-8


# ------------------------------------------------------------------------------------------------ the synchronous path
def sync_cases():
    """(class, T) of the child process: the shortest series, a lane's scalar tail, two workgroups with the second from the head, empty blocks"""
    out = []
    for name in ("tiny_d1", "from_head_d2", "from_head_d3", "stretched_d6"):
        plan = case_of(name)[1]
        C = SPAN - 2 * plan["halo"]
        out += [(name, plan["nhs"] + 2), (name, plan["nhs"] + 9), (name, plan["nhs"] + C + 1), (name, plan["nhs"] + 9 * C + 1)]
    return out


def _child_main():
    import temporalgps_jl_amd as tgp
    res = []
    for name, T in sync_cases():
        case = case_of(name)[0]
        lp, g, names = run_device(tgp, case, T)
        dlp, dev = deviations(lp, g, *case.ref(T))
        res.append(dict(name=name, T=T, lp=dlp, dev=dev, names=sorted(names)))
    print("RESULT " + json.dumps(res))


def test_head_state_by_value_when_launches_are_synchronous():
    """TGP_MODAL_OVERLAP=0 (read once per process: a fresh child): copy, synchronise, head on the host, launch -- the head's end state goes to the kernel
    by value instead of through the hand-over"""
    env = dict(os.environ, TGP_MODAL_OVERLAP="0")
    out = subprocess.run([sys.executable, "-c", "from tests import test_gpu_adjoint_edges as t; t._child_main()"], cwd=U.ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[7:])
    assert len(res) == len(sync_cases())
    for r in res:
        print(f"{r['name']} T={r['T']}: lp {r['lp']:.1e} worst {max(r['dev'].values()):.1e}")
        assert r["lp"] <= LP_BAR and max(r["dev"].values()) <= GRAD_BAR and "k_adjoint_one" in r["names"], r


# ------------------------------------------------------------------------------------------------ the five-launch pass
FIVE_CLASSES = {
    "one_tile_d2": None, "one_tile_d3": None, "two_three_d5": None,           # the classes above, with TGP_OPT_STEADY = 2
    "fast_d7": (("sum", M52, M32, M32), 0.2, 0.25),
    "slow_d7": (("sum", M52, ("stretched", 0.5, M32), M32), 0.02, 0.1),
    "fast_d8": (("sum", M52, M52, M32), 0.2, 0.25),
    "slow_d8": (("sum", M52, ("stretched", 0.5, M52), M32), 0.02, 0.1),
    "head3_d3": (M52, 0.004, 1.0),                                            # heads of three and four tiles
    "head3_d8": (("sum", M52, ("stretched", 0.5, M52), M32), 0.01, 0.1),
    "head4_d8": (("sum", M52, ("stretched", 0.5, M52), M32), 0.007, 0.1),
}


def five_case(name):
    key = "five:" + name
    if key not in _CACHE:
        spec, dt, noise = FIVE_CLASSES[name] or CLASSES[name][:3]
        n0 = settle_n0(blocks_of(spec, dt, noise))
        th = n0 // TILE + 1
        _CACHE[key] = (Case(spec, dt, noise, th * TILE + 3 * BLK + 1), n0, th)
    return _CACHE[key]


@pytest.mark.parametrize("name", list(FIVE_CLASSES))
def test_five_launch_adjoint_at_tile_head_and_workgroup_edges(name):
    import temporalgps_jl_amd as tgp
    case, n0, th = five_case(name)
    print(f"{name}: d {case.d} n0 {n0} head {th} tiles")
    assert th == {"slow_d7": 2, "slow_d8": 2, "head3_d3": 3, "head3_d8": 3, "head4_d8": 4}.get(name, 1), (name, n0, th)
    assert 1 <= th <= 4 and min(n0 % TILE, TILE - n0 % TILE) >= 32, (n0, th)      # (a head whose tile count a rounding of the criterion cannot move)
    nh = th * TILE
    failures, worst = [], {}
    steady = 2 if case.d <= 6 else None
    for T in (nh + 2, nh + 511, nh + 512, nh + 513, nh + BLK - 1, nh + BLK, nh + BLK + 1, nh + 3 * BLK + 1):
        check(tgp, case, T, failures, worst, name, "five", steady=steady)
    print(f"{name}: worst " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ declines
def test_a_model_the_filter_plan_declines_for_slow_mixing_is_served_by_the_five_launch_pass_or_refused():
    import temporalgps_jl_amd as tgp
    spec, dt, noise = M52, 0.01, 2.0
    plan = filter_plan(blocks_of(spec, dt, noise), 10 ** 6)
    print(f"slow mixing: plan {plan}")
    assert plan["why"] == 5, plan                   # kSlowMixing: the closed loop's powers are not below 2^-60 after 1536 steps
    n0 = settle_n0(blocks_of(spec, dt, noise))
    th = n0 // TILE + 1
    case = Case(spec, dt, noise, th * TILE + BLK + 1)
    failures, worst = [], {}
    for T in (th * TILE + 2, th * TILE + BLK + 1):
        try:
            check(tgp, case, T, failures, worst, "slow_mixing", "five")
        except tgp._lib.Unsupported:
            print(f"slow_mixing T={T}: Unsupported")
    assert not failures, failures


@pytest.mark.parametrize("name", ["tiny_d1", "from_head_d3", "slow_d8"])
def test_a_series_shorter_than_the_head_raises_unsupported(name):
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lgssm as L
    if name in CLASSES:
        case, plan = case_of(name)
        T = plan["n0"] - 2
    else:
        case, n0, th = five_case(name)
        T = n0 - 2
    dm = U.device_model(tgp, case.model(T))
    with pytest.raises(tgp._lib.Unsupported):
        L.logpdf_adjoint(dm, case.y[:T])
