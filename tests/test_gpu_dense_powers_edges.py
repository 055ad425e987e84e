"""GPU tier: the five operations of the d <= 8 LTI interface that run on ONE kernel skeleton on dense matrix powers (csrc/tgp_powers.hip) -- placed on the
edges of that skeleton, against the oracle's sequential restatement of the reference (oracle/seq_kalman.py) entry by entry.

    kernel label               serves                                                                    span C
    k_smooth_one<logpdf>       logpdf of models the modal plan declines; of models with a mean function   4096 - halo
    k_smooth_one<posterior>    posterior marginals (+ logpdf) of the same                                 4096 - 2 halo
    k_smooth_one<rand>         rand(posterior(fx, y)) of every Forward LTI model, d <= 6                  4096 - 2 halo
    k_filter_one               _filter; posterior evaluated (G, g, L)                                     4096 - halo
    k_rand_one                 rand of the prior                                                          4096 - halo, no head

Geometry (launch_smooth / launch_filter / launch_rand and the kernels' first lines): a span is 8 waves x 64 lanes x 8 steps = 4096 steps; a lane loads its 8
steps with 16-byte loads when t0 + 8 <= T and the series is 16-byte aligned, one by one otherwise; workgroup g owns [nhs + g C, nhs + (g + 1) C) behind the head
(nhs steps, run on the host beside the kernel), starts `halo` steps early from a zero state -- or AT the head from the head's end state when that start would
lie in front of it (`from_head`: the first workgroup always, the second one too when C < halo) -- and, with the backward half, runs `halo` steps past its
range, cut by T; nwg = ceil((T - nhs) / C) workgroups are mapped to blocks as g = (b & 7) per + (b >> 3), per = ceil(nwg / 8), blocks with g >= nwg are empty;
the last n1 steps take their variance from the tail table tvb (pinned memory, read in place); the evaluated posterior's g changes hands at step nhs.

Classes (tests/_dense_powers_edges.py CLASSES: model = oracle.components.build_lgssm(kernel, dt, noise) with a and h set non-zero).  Every figure is what
tgp_smooth_plan (with and without the posterior half) and tgp_rand_plan report -- asserted at run time against _dense_powers_edges.EXPECTED, here and in
tests/test_dense_powers_plan.py.  halo_f: the filter's halo (k_smooth_one<logpdf>, k_filter_one: C = 4096 - halo_f); halo: the smoother's (the longer of
halo_f and the settled reverse-time transition's; k_smooth_one<posterior | rand>: C = 4096 - 2 halo); halo_r: the prior draw's (open loop; k_rand_one: C = 4096 - halo_r).

    class             kernel                                  dt     noise d  route     nhs halo_f  C_lp  halo   n1 C_post halo_r C_rand
    tiny_d1           Matern-1/2                              0.1    0.1   1  offset     16     32  4064    32   15   4032    416   3680
    one_tile_d3       Matern-5/2                              0.03   0.5   3  offset    208    512  3584   528  171   3040    752   3344
    sum_d4            Matern-5/2 + Matern-1/2                 0.05   0.1   4  offset    256    736  3360   736  149   2624    832   3264
    stretched_d6      Matern-5/2 + stretched(0.4) Matern-5/2  0.05   0.1   6  offset    352    992  3104   992  178   2112   1136   2960
    two_three_d5      Matern-5/2 + Matern-3/2                 0.02   0.1   5  offset    384   1232  2864  1264  157   1568   1328   2768
    from_head_d3      Matern-5/2                              0.01   1.0   3  offset    560   1440  2656  1456  401   1184  declined
    three_tiles_d3    Matern-5/2                              0.01   1.5   3  offset    560   1536  2560  declined (436)  declined
    three_tiles_d2    Matern-3/2                              0.006  2.0   2  offset    608   1520  2576  1536  432   1024  declined
    identical_d6      Matern-5/2 + Matern-5/2                 0.05   0.1   6  declined   96    448  3648   448   84   3200    464   3632
    identical_slow_d6 Matern-5/2 + Matern-5/2                 0.015  0.1   6  declined  256   1488  2608  1488  192   1120   1504   2592
    declined_d7       Matern-3/2 + Matern-3/2 + Matern-5/2    0.1    0.1   7  declined   80    272  3824   272   37   3552    272   3824
    declined_d8       Matern-5/2 + Matern-5/2 + Matern-3/2    0.1    0.1   8  declined   96    240  3856   256   33   3584    272   3824

    (C_lp is also k_filter_one's C.  k_smooth_one<logpdf>, k_smooth_one<posterior> and k_filter_one serve every class, k_smooth_one<rand> the classes with d <= 6,
    k_rand_one every class -- but for the "declined" entries: three_tiles_d3's settled reverse-time transition does not forget within 1536 steps, so its
    posterior marginals and posterior draws are DECLINE cases (why 5; three_tiles_d2 is the served neighbour with the longest halo, C = 1024), and the open
    loop of the three classes at spacings <= 0.01 does not either, so their prior draws are decline cases too.  from_head_d3, three_tiles_d2 and
    identical_slow_d6 are served with C_post < halo: their second workgroup too starts at the head.  No served class has n1 > C_post -- see
    _dense_powers_edges.EXPECTED for the search -- the lengths nhs + k C + n1 // 2 put the tail over two workgroups instead.)

Routes to k_smooth_one<logpdf | posterior>: "offset" -- the model has a modal form (k_steady_one / the streaming kernels serve its LTI form), the suite gives
it the emission offset per step h_t = 0.4 + sin(0.7 t) of a mean function (lti_but_offset); "declined" -- the modal plan declines the LTI model itself.
k_filter_one, k_rand_one and k_smooth_one<rand> (d <= 6) serve the LTI form of every class.

Lengths per (class, operation), from that operation's nhs, C, halo and n1 (_dense_powers_edges.edge_lengths): the shortest served length and one below it,
nhs + {7, 8, 9, 511, 512, 513}, nhs + C + {-1, 0, 1}, nhs + 2C +- 1, nhs + 2C + halo +- 1, nhs + {7C + 1, 8C, 8C + 1, 9C + 1}, T - n1 at a span edge + {-1, 0, 1}
and at a tile edge +- 1 of the first and of the second workgroup, one T = 3 (mod 8); k_rand_one the same with nhs = 0.  Lengths below the shortest served one
are decline cases: the right answer, and not by the one-launch kernel.

Bars (the project's): logpdf 1e-10 relative; posterior mean 1e-8 max(1, max |m|), variance 1e-8; filter and evaluated posterior 1e-8 max(1, max |ref|) per
array; prior draw 1e-9 max(1, max |y|); posterior draw 1e-8 max(1, max |y|).

profiles/dense_powers_edges_parity.txt keeps the largest deviation seen per class and operation."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import seq_kalman as sk
from tests import _dense_powers_edges as E
from tests import _util as U

pytestmark = pytest.mark.gpu

OPS = ("logpdf", "marginals", "filter", "posterior", "rand_prior", "rand_post")
KERNEL = {"logpdf": "k_smooth_one<logpdf>", "marginals": "k_smooth_one<posterior>", "filter": "k_filter_one", "posterior": "k_filter_one",
          "rand_prior": "k_rand_one", "rand_post": "k_smooth_one<rand>"}
ONE_LAUNCH = ("k_smooth_one", "k_filter_one", "k_rand_one")
_CACHE = {}


def ops_of(name):
    d = int(name.rsplit("_d", 1)[1])
    return [op for op in OPS if op != "rand_post" or d <= 6]      # (the posterior draw's kernel holds d <= 6)


class Case:
    """a class's model blocks, one long series, its draws and the oracle's results that every prefix shares -- computed once per module"""

    def __init__(self, name):
        spec, dt, noise, self.route = E.CLASSES[name]
        self.name = name
        self.blocks = E.blocks_of(spec, dt, noise)
        self.d = len(self.blocks["x0m"])
        self.geo = E.geometry(name)
        N = E.T_CAP
        rng = np.random.default_rng(17)
        self.eps = (rng.standard_normal((N, self.d)), rng.standard_normal(N), rng.standard_normal(self.d))      # the prior draw's, and the series'
        # rand runs forwards: the draw of a T-step model is the first T steps of the N-step model's -- the series of every length, and the prior draw's reference
        self.y_lti = sk.rand(self.lti(N), *self.eps)
        self.hh = E.offsets(N)
        self.y_off = self.y_lti - float(self.blocks["h"][0]) + self.hh      # (the same draw under the offset model)
        rng = np.random.default_rng(18)
        self.deps = (rng.standard_normal((N, self.d)), rng.standard_normal(N), rng.standard_normal(self.d))      # the posterior draw's
        self.Rn = 0.01 + 0.1 * rng.random(N)
        self.Rn0 = np.array([0.05])
        self._filter = self._post = None

    def lti(self, T):
        return dict(self.blocks, T=int(T))

    def smodel(self, T):
        """the model whose logpdf / posterior marginals k_smooth_one serves"""
        return dict(self.blocks, T=int(T), h=self.hh[:T].copy()) if self.route == "offset" else self.lti(T)

    def sy(self, T):
        return (self.y_off if self.route == "offset" else self.y_lti)[:T]

    # the filter runs forwards, and so does what posterior() evaluates (G_t, L_t from the covariances up to t, g_t from the filtered mean at t): the
    # results of a T-step series are the first T of the N-step series' -- one oracle run per class (tests/test_smooth_host.py holds the oracle to that)
    def filter_states(self):
        if self._filter is None:
            self._filter = sk.filter_(self.lti(E.T_CAP), self.y_lti, want_states=True)[1:]
        return self._filter

    def posterior(self, T):
        """the oracle's evaluated posterior of the T-step LTI model (ordering "R": G, g, L in A, a, Q; x0 the last filtering state)"""
        if self._post is None:
            self._post = sk.posterior(self.lti(E.T_CAP), self.y_lti)
        fm, fP = self.filter_states()
        p = self._post
        return dict(self.lti(T), ordering="R", A=p["A"][:T], a=p["a"][:T], Q=p["Q"][:T], x0m=fm[T - 1], x0P=fP[T - 1])


def case_of(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


def steady_steps(dm):
    hd = dm.handle()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    hd.check(hd.lib.tgp_steady_steps(hd.h, ctypes.byref(a), ctypes.byref(b)))
    return a.value


def op_geometry(case, op):
    """(why, nhs, C, the halo behind a span that T may cut, n1, the run-in in front of a span) of an operation on a class"""
    g = case.geo
    if op == "logpdf":
        return g["why_lp"], g["nhs"], g["C_lp"], g["halo_f"], 0, g["halo_f"]
    if op in ("marginals", "rand_post"):
        return g["why"], g["nhs"], g["C_post"], g["halo"], g["n1"], g["halo"]
    if op in ("filter", "posterior"):
        return g["why_f"], g["nhs"], g["C_filter"], g["halo_f"], 0, g["halo_f"]
    return g["why_r"], 0, g["C_rand"], g["halo_r"], 0, g["halo_r"]


def plan_of(case, op):
    m = case.blocks
    if op == "logpdf":
        return lambda T: E.smooth_plan(m, T, post=False)
    if op in ("marginals", "rand_post"):
        return lambda T: E.smooth_plan(m, T)
    if op in ("filter", "posterior"):
        return lambda T: E.filter_plan(m, T)
    return lambda T: E.rand_plan(m, T) if T >= 2 else dict(why=E.WHY_TOO_SHORT)      # (tgp_rand takes the one-launch path from two steps on)


def lengths_of(case, op):
    """-> (the shortest served length, every length of the (class, operation))"""
    why, nhs, C, halo, n1, hl = op_geometry(case, op)
    assert why == 0
    tmin = E.shortest_served(plan_of(case, op), 1, nhs + n1 + 64)
    if n1:
        assert tmin == nhs + n1 + 16, (tmin, nhs, n1)      # head + tail + 16
    return tmin, sorted(set(E.edge_lengths(nhs, C, halo, n1, hl) + [tmin, max(tmin - 1, 1)]))


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _rel(got, ref):
    return float(np.abs(_np(got) - ref).max() / max(1.0, float(np.abs(ref).max())))


def run_op(tgp, case, op, T, dev=False, dm=None, series=None):
    """One call (two or three where the operation has variants of its new noise) on a fresh handle (or on dm), against the oracle.
    -> ({figure: (deviation, bar)}, kernel names seen, tgp_steady_steps behind the last call or None).  dev: every per-step array is device-resident.
    series: another series in place of the class's own (the first T steps are taken) -- the references are then computed for it."""
    import torch
    from temporalgps_jl_amd import lgssm as L
    lib = tgp._lib
    own = series is None
    to = (lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()) if dev else (lambda x: x)
    out, names = {}, set()
    if op in ("logpdf", "marginals"):
        model, y = case.smodel(T), (case.sy(T) if own else series[:T])
        dm = dm or U.device_model(tgp, model)
        lp_ref = sk.logpdf(model, y)
        if op == "logpdf":
            lp, names = U.kernels_of(tgp, dm, lambda: L.logpdf(dm, to(y)))
            out["lp"] = (abs(lp - lp_ref) / abs(lp_ref), 1e-10)
        else:
            m_ref, v_ref = sk.posterior_marginals(model, y, case.Rn[:T])
            for tag, Rn, vr in (("shared", case.Rn0, v_ref - case.Rn[:T] + case.Rn0[0]), ("per_step", case.Rn[:T], v_ref)):      # (var = h' Ps h + R_new)
                (lp, mean, var), nm = U.kernels_of(tgp, dm, lambda: L.logpdf_and_posterior_marginals(dm, to(y), to(Rn)))
                names |= nm
                out["lp_" + tag] = (abs(lp - lp_ref) / abs(lp_ref), 1e-10)
                out["mean_" + tag] = (_rel(mean, m_ref), 1e-8)
                out["var_" + tag] = (float(np.abs(_np(var) - vr).max()), 1e-8)
        return out, names, steady_steps(dm)
    model = case.lti(T)
    y = case.y_lti[:T] if own else series[:T]
    dm = dm or U.device_model(tgp, model)
    if op == "filter":
        fm, fP = case.filter_states() if own else sk.filter_(model, y, want_states=True)[1:]
        hd = dm.handle()
        yy = to(np.ascontiguousarray(y))
        gm = torch.empty((T, case.d), dtype=torch.float64, device="cuda") if dev else np.empty((T, case.d))
        gP = torch.empty((T, case.d, case.d), dtype=torch.float64, device="cuda") if dev else np.empty((T, case.d, case.d))
        lml = ctypes.c_double()
        flags = (lib.IN_DEVICE | lib.OUT_DEVICE) if dev else 0
        if dev:
            torch.cuda.synchronize()
        _, names = U.kernels_of(tgp, dm, lambda: hd.check(hd.lib.tgp_filter(hd.h, lib.ptr(yy), None, flags, lib.ptr(gm), lib.ptr(gP), ctypes.byref(lml))))
        if dev:
            torch.cuda.synchronize()
        lp_ref = sk.logpdf(model, y)
        out["m"] = (_rel(gm, fm[:T]), 1e-8)
        out["P"] = (_rel(gP, fP[:T]), 1e-8)      # (symmetric blocks: column-major reads as row-major)
        out["lp"] = (abs(lml.value - lp_ref) / abs(lp_ref), 1e-10)
    elif op == "posterior":
        ref = case.posterior(T) if own else sk.posterior(model, y)
        dpost, names = U.kernels_of(tgp, dm, lambda: L.posterior(dm, to(y)).materialise())
        got = dict(G=_np(dpost.transitions.As), g=_np(dpost.transitions.as_), L=_np(dpost.transitions.Qs))
        want = dict(G=ref["A"], g=ref["a"], L=ref["Q"])
        nhs = case.geo["nhs"]
        for k in ("G", "g", "L"):
            sc = max(1.0, float(np.abs(want[k]).max()))
            out[k] = (float(np.abs(got[k] - want[k]).max()) / sc, 1e-8)
            for t in (nhs - 1, nhs, nhs + 1):      # where the head's steps (the host's) and the kernel's meet
                if t < T:
                    out[f"{k}[nhs{t - nhs:+d}]"] = (float(np.abs(got[k][t] - want[k][t]).max()) / sc, 1e-8)
        out["x0m"] = (_rel(dpost.x0.m, ref["x0m"]), 1e-8)
        out["x0P"] = (_rel(dpost.x0.P, ref["x0P"]), 1e-8)
    elif op == "rand_prior":
        assert own
        eps = (to(case.eps[0][:T]), to(case.eps[1][:T]), case.eps[2])
        got, names = U.kernels_of(tgp, dm, lambda: L.rand(eps, dm))
        out["y"] = (_rel(got, case.y_lti[:T]), 1e-9)
        return out, names, None
    else:
        ref = case.posterior(T) if own else sk.posterior(model, y)
        base = U.posterior_draw(ref, np.zeros(1), case.deps[0][:T], case.deps[1][:T], case.deps[2])      # (the noise-free draw: the state path is shared)
        eps = (to(case.deps[0][:T]), to(case.deps[1][:T]), case.deps[2])
        for tag, Rn in (("shared", case.Rn0), ("per_step", case.Rn[:T]), ("prior_noise", None)):
            post = L.posterior(dm, to(y))
            if Rn is not None:
                post = L.replace_observation_noise_cov(post, Rn)
            got, nm = U.kernels_of(tgp, dm, lambda: L.rand(eps, post))
            names |= nm
            want = base + np.sqrt(np.broadcast_to(model["R"] if Rn is None else Rn, (T,))) * case.deps[1][:T]
            out["y_" + tag] = (_rel(got, want), 1e-8)
    return out, names, steady_steps(dm)


def note(out, failures, worst, tag):
    for k, (v, bar) in out.items():
        key = k.split("[")[0]
        worst[key] = max(worst.get(key, 0.0), v)
        if not v <= bar:
            failures.append((tag, k, v, bar))


def fmt(out):
    return " ".join(f"{k} {v:.1e}" for k, (v, _) in out.items())


def check_served(tgp, case, op, T, failures, worst, dev=False, tag=None):
    out, names, steps = run_op(tgp, case, op, T, dev=dev)
    tag = tag or f"{case.name} {op}"
    print(f"{tag} T={T}: {fmt(out)} | {sorted(names)}")
    note(out, failures, worst, (tag, T))
    if names != {KERNEL[op]}:
        failures.append((tag, T, "kernel", sorted(names)))
    if steps is not None and not steps > T - case.geo["nhs"] - 1:
        failures.append((tag, T, "tgp_steady_steps", steps))


def check_declined(tgp, case, op, T, failures, worst):
    """a length the operation's plan declines: the right answer, by other kernels"""
    out, names, _ = run_op(tgp, case, op, T)
    print(f"{case.name} {op} T={T} (declined by the plan): {fmt(out)} | {sorted(names)}")
    note(out, failures, worst, (case.name, op, T, "declined"))
    if KERNEL[op] in names or not names:
        failures.append((case.name, op, T, "served by the kernel its plan declines", sorted(names)))


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", list(E.CLASSES))
def test_the_table_is_what_the_plans_report(name):
    case = case_of(name)
    print(name, case.geo)
    assert case.geo == E.EXPECTED[name], (name, case.geo)
    g = case.geo
    assert g["C_lp"] == g["C_filter"] == E.SPAN - g["halo_f"] and (g["why_r"] != 0 or g["C_rand"] == E.SPAN - g["halo_r"])
    if g["why"] == 0:
        assert g["C_post"] == E.SPAN - 2 * g["halo"]
        assert (g["C_post"] < g["halo"]) == (name in E.FROM_HEAD)      # from nhs + C + 1 on the second workgroup too starts at the head
        assert g["n1"] < g["C_post"]                                    # (no served class has it otherwise: the lengths nhs + k C + n1 // 2 split the tail)


# ------------------------------------------------------------------------------------------------ span, halo, head and tail edges
@pytest.mark.parametrize("name,op", [(name, op) for name in E.CLASSES for op in ops_of(name)])
def test_one_launch_kernels_at_span_halo_head_and_tail_edges(name, op):
    import temporalgps_jl_amd as tgp
    case = case_of(name)
    why = op_geometry(case, op)[0]
    failures, worst = [], {}
    if why != 0:
        # the class's plan declines the operation (E.EXPECTED records why): the right answer by other kernels, named
        g = case.geo
        for T in (g["nhs"] + 2 * E.TILE + 1, g["nhs"] + E.SPAN + 1, g["nhs"] + 3 * E.SPAN + 3):
            out, names, _ = run_op(tgp, case, op, T)
            print(f"{name} {op} T={T} (the plan declines the class: why {why}): {fmt(out)} | {sorted(names)}")
            note(out, failures, worst, (name, op, T))
            if not names or KERNEL[op] in names or not names <= E.DECLINED_SERVED_BY[(name, op)]:
                failures.append((name, op, T, "kernels", sorted(names)))
        assert not failures, failures
        return
    tmin, Ts = lengths_of(case, op)
    print(f"{name} {op}: shortest served {tmin}, {len(Ts)} lengths, geometry {op_geometry(case, op)}")
    plan = plan_of(case, op)
    assert plan(max(tmin - 1, 1))["why"] == E.WHY_TOO_SHORT
    for T in Ts:
        if T < tmin:
            check_declined(tgp, case, op, T, failures, worst)
        else:
            check_served(tgp, case, op, T, failures, worst)
    print(f"{name} {op}: worst " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ device-resident arrays
def three_edges(case, op):
    why, nhs, C, halo, n1, hl = op_geometry(case, op)
    t3 = nhs + C + 2 * E.TILE
    return [nhs + C + 1, nhs + 2 * C + halo - 1, t3 + (3 - t3) % 8]


@pytest.mark.parametrize("name", E.BEYOND_LENGTHS)
def test_device_resident_arrays_give_what_host_arrays_give(name):
    """host arrays: the head's inputs are read from the caller; device arrays (and a per-step offset always): workgroup 0 hands them over through pinned
    memory (`hand`).  Both against the oracle, at three edge lengths of every operation"""
    import temporalgps_jl_amd as tgp
    case = case_of(name)
    failures, worst = [], {}
    for op in ops_of(name):
        if op_geometry(case, op)[0] != 0:
            continue
        for T in three_edges(case, op):
            for dev in (False, True):
                check_served(tgp, case, op, T, failures, worst, dev=dev, tag=f"{name} {op} ({'device' if dev else 'host'} arrays)")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ pointers 8 bytes off a 16-byte boundary, sentinels
SENTINEL = 7.25e77


def _off8(x=None, n=None):
    """a device buffer of n doubles 8 bytes past a 16-byte boundary with a sentinel in front and two behind: (whole buffer, the n doubles)"""
    import torch
    n = int(np.size(x)) if x is not None else int(n)
    buf = torch.full((n + 3,), SENTINEL, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:n + 1]
    if x is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(-1)))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return buf, view


def _intact(buf, n):
    return float(buf[0]) == SENTINEL and bool((buf[n + 1:] == SENTINEL).all())


@pytest.mark.parametrize("name", E.BEYOND_LENGTHS)
def test_every_array_eight_bytes_off_a_16_byte_boundary_and_nothing_written_outside_the_outputs(name):
    """the lanes' 16-byte loads and stores need 16-byte aligned arrays: with every input and output 8 bytes past such a boundary they must not be taken, the
    results are the same, and the doubles in front of and behind every output keep their sentinel"""
    import torch
    import temporalgps_jl_amd as tgp
    lib = tgp._lib
    case = case_of(name)
    d = case.d
    FL = lib.IN_DEVICE | lib.OUT_DEVICE
    failures, worst = [], {}

    def done(op, T, out, names, bufs):
        print(f"{name} {op} (+ 8 bytes) T={T}: {fmt(out)} | {sorted(names)}")
        note(out, failures, worst, (name, op, T))
        if names != {KERNEL[op]}:
            failures.append((name, op, T, "kernel", sorted(names)))
        for label, buf, n in bufs:
            if not _intact(buf, n):
                failures.append((name, op, T, "written outside " + label))

    for op in ops_of(name):
        if op_geometry(case, op)[0] != 0:
            continue
        for T in three_edges(case, op):
            out = {}
            lml = ctypes.c_double()
            if op in ("logpdf", "marginals"):
                model, y = case.smodel(T), case.sy(T)
                dm = U.device_model(tgp, model)
                hd = dm.handle()
                lp_ref = sk.logpdf(model, y)
                _, yd = _off8(y)
                if op == "logpdf":
                    torch.cuda.synchronize()
                    _, names = U.kernels_of(tgp, dm, lambda: hd.check(hd.lib.tgp_logpdf(hd.h, lib.ptr(yd), None, lib.IN_DEVICE, ctypes.byref(lml))))
                    bufs = []
                else:
                    m_ref, v_ref = sk.posterior_marginals(model, y, case.Rn[:T])
                    _, rd = _off8(case.Rn[:T])
                    (bm, gm), (bv, gv) = _off8(n=T), _off8(n=T)
                    torch.cuda.synchronize()
                    _, names = U.kernels_of(tgp, dm, lambda: hd.check(hd.lib.tgp_logpdf_and_posterior_marginals(
                        hd.h, lib.ptr(yd), None, lib.ptr(rd), FL, ctypes.byref(lml), lib.ptr(gm), lib.ptr(gv))))
                    torch.cuda.synchronize()
                    out["mean"] = (_rel(gm, m_ref), 1e-8)
                    out["var"] = (float(np.abs(_np(gv) - v_ref).max()), 1e-8)
                    bufs = [("mean", bm, T), ("var", bv, T)]
                out["lp"] = (abs(lml.value - lp_ref) / abs(lp_ref), 1e-10)
                done(op, T, out, names, bufs)
                continue
            model, y = case.lti(T), case.y_lti[:T]
            dm = U.device_model(tgp, model)
            hd = dm.handle()
            _, yd = _off8(y)
            if op == "filter":
                fm, fP = case.filter_states()
                (bm, gm), (bP, gP) = _off8(n=T * d), _off8(n=T * d * d)
                torch.cuda.synchronize()
                _, names = U.kernels_of(tgp, dm, lambda: hd.check(hd.lib.tgp_filter(hd.h, lib.ptr(yd), None, FL, lib.ptr(gm), lib.ptr(gP), ctypes.byref(lml))))
                torch.cuda.synchronize()
                lp_ref = sk.logpdf(model, y)
                out = dict(m=(_rel(gm.reshape(T, d), fm[:T]), 1e-8), P=(_rel(gP.reshape(T, d, d), fP[:T]), 1e-8), lp=(abs(lml.value - lp_ref) / abs(lp_ref), 1e-10))
                done(op, T, out, names, [("m", bm, T * d), ("P", bP, T * d * d)])
            elif op == "posterior":
                ref = case.posterior(T)
                (bG, gG), (bg, gg), (bL, gL) = _off8(n=T * d * d), _off8(n=T * d), _off8(n=T * d * d)
                xfm, xfP = np.empty(d), np.empty((d, d))
                torch.cuda.synchronize()
                _, names = U.kernels_of(tgp, dm, lambda: hd.check(hd.lib.tgp_posterior(hd.h, lib.ptr(yd), None, FL, lib.ptr(gG), lib.ptr(gg), lib.ptr(gL),
                                                                                      lib.ptr(xfm), lib.ptr(xfP))))
                torch.cuda.synchronize()
                out = dict(G=(_rel(gG.reshape(T, d, d).transpose(-1, -2), ref["A"]), 1e-8), g=(_rel(gg.reshape(T, d), ref["a"]), 1e-8),
                           L=(_rel(gL.reshape(T, d, d), ref["Q"]), 1e-8), x0m=(_rel(xfm, ref["x0m"]), 1e-8), x0P=(_rel(xfP.T, ref["x0P"]), 1e-8))
                done(op, T, out, names, [("G", bG, T * d * d), ("g", bg, T * d), ("L", bL, T * d * d)])
            elif op == "rand_prior":
                _, et = _off8(case.eps[0][:T])
                _, ee = _off8(case.eps[1][:T])
                by, gy = _off8(n=T)
                e0 = np.ascontiguousarray(case.eps[2])
                torch.cuda.synchronize()
                _, names = U.kernels_of(tgp, dm, lambda: hd.check(hd.lib.tgp_rand(hd.h, lib.ptr(et), lib.ptr(ee), lib.ptr(e0), FL, lib.ptr(gy))))
                torch.cuda.synchronize()
                done(op, T, dict(y=(_rel(gy, case.y_lti[:T]), 1e-9)), names, [("y", by, T)])
            else:
                ref = case.posterior(T)
                want = U.posterior_draw(ref, case.Rn[:T], case.deps[0][:T], case.deps[1][:T], case.deps[2])
                _, rd = _off8(case.Rn[:T])
                _, et = _off8(case.deps[0][:T])
                _, ee = _off8(case.deps[1][:T])
                by, gy = _off8(n=T)
                e0 = np.ascontiguousarray(case.deps[2])
                torch.cuda.synchronize()
                _, names = U.kernels_of(tgp, dm, lambda: hd.check(hd.lib.tgp_posterior_rand(hd.h, lib.ptr(yd), lib.ptr(rd), lib.ptr(et), lib.ptr(ee), lib.ptr(e0),
                                                                                           FL, lib.ptr(gy))))
                torch.cuda.synchronize()
                done(op, T, dict(y=(_rel(gy, want), 1e-8)), names, [("y", by, T)])
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ call sequences on one handle
@pytest.mark.parametrize("name", E.ON_ONE_HANDLE)
def test_three_series_on_one_handle_rotating_logpdf_posterior_and_draw(name):
    """the host / device hand-over of the head carries a sequence number (the flags hold 2 seq): the second and third series on a handle, and the second and
    third operation on a series, must not read what an earlier call left in the pinned buffers"""
    import temporalgps_jl_amd as tgp
    case = case_of(name)
    assert case.route == "declined" and case.d <= 6      # (logpdf, marginals and the draw of ONE bound model all run on k_smooth_one)
    why, nhs, C, halo, n1, hl = op_geometry(case, "marginals")
    T = nhs + C + 1
    dm = U.device_model(tgp, case.lti(T))
    rng = np.random.default_rng(23)
    ops = ("logpdf", "marginals", "rand_post")
    failures, worst = [], {}
    for i in range(3):
        series = case.y_lti[:T] if i == 0 else case.y_lti[i * 100:i * 100 + T] * (1.0 + 0.5 * i) + 0.3 * rng.standard_normal(T)
        for k in range(3):
            op = ops[(i + k) % 3]
            out, names, steps = run_op(tgp, case, op, T, dm=dm, series=series)
            print(f"{name} series {i} {op}: {fmt(out)} | {sorted(names)}")
            note(out, failures, worst, (name, i, op))
            if names != {KERNEL[op]} or not steps > T - nhs - 1:
                failures.append((name, i, op, sorted(names), steps))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ the synchronous route
def sync_cases():
    """(class, operation, T) of the child process: the shortest series, a second workgroup (from the head where the class has it), empty blocks"""
    out = []
    for name in E.BEYOND_LENGTHS:
        case = case_of(name)
        for op in ops_of(name):
            why, nhs, C, halo, n1, hl = op_geometry(case, op)
            if why != 0:
                continue
            out += [(name, op, lengths_of(case, op)[0]), (name, op, nhs + C + 1), (name, op, nhs + 8 * C + 1)]
    return out


def _child_main():
    import temporalgps_jl_amd as tgp
    res = []
    for name, op, T in sync_cases():
        out, names, steps = run_op(tgp, case_of(name), op, T)
        res.append(dict(name=name, op=op, T=T, out={k: list(v) for k, v in out.items()}, names=sorted(names), steps=steps))
    print("RESULT " + json.dumps(res))


def test_same_results_when_launches_are_synchronous():
    """TGP_MODAL_OVERLAP=0 (read once per process: a fresh child): copy, synchronise, head on the host, launch -- the head's end state goes to the kernel by
    value and the head's outputs are copied behind it, instead of the hand-over through pinned flags"""
    env = dict(os.environ, TGP_MODAL_OVERLAP="0")
    run = subprocess.run([sys.executable, "-c", "from tests import test_gpu_dense_powers_edges as t; t._child_main()"], cwd=U.ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(sync_cases())
    failures = []
    for r in res:
        print(f"{r['name']} {r['op']} T={r['T']}: " + " ".join(f"{k} {v:.1e}" for k, (v, _) in r["out"].items()))
        failures += [(r["name"], r["op"], r["T"], k, v) for k, (v, bar) in r["out"].items() if not v <= bar]
        if r["names"] != [KERNEL[r["op"]]]:
            failures.append((r["name"], r["op"], r["T"], r["names"]))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ a NaN in the series
@pytest.mark.parametrize("name", E.ON_ONE_HANDLE)
def test_a_nan_in_the_head_at_the_head_boundary_and_in_the_last_tile(name):
    """(NaN == missing in the mirrors' convention: they rely on a NaN observation surfacing as a NaN log marginal likelihood from the posterior call, and on
    TGP_EUNSUPPORTED from tgp_posterior_rand, whose caller then takes the evaluated route)"""
    import torch
    import temporalgps_jl_amd as tgp
    lib = tgp._lib
    case = case_of(name)
    why, nhs, C, halo, n1, hl = op_geometry(case, "marginals")
    T = nhs + 2 * C + 1
    FL = lib.IN_DEVICE | lib.OUT_DEVICE | lib.SHARED_R
    for t_nan in (3, nhs, T - 5):
        y = case.y_lti[:T].copy()
        y[t_nan] = np.nan
        hd = U.device_model(tgp, case.lti(T)).handle()
        yd, rd = torch.from_numpy(y).cuda(), torch.from_numpy(case.Rn0).cuda()
        mean, var = torch.zeros(T, dtype=torch.float64, device="cuda"), torch.zeros(T, dtype=torch.float64, device="cuda")
        lml = ctypes.c_double()
        torch.cuda.synchronize()
        rc = hd.lib.tgp_logpdf_and_posterior_marginals(hd.h, lib.ptr(yd), None, lib.ptr(rd), FL, ctypes.byref(lml), lib.ptr(mean), lib.ptr(var))
        torch.cuda.synchronize()
        print(f"{name} NaN at {t_nan}: posterior rc {rc} lml {lml.value}")
        assert rc == 0 and np.isnan(lml.value), (t_nan, rc, lml.value)
        et, ee = torch.from_numpy(case.deps[0][:T].copy()).cuda(), torch.from_numpy(case.deps[1][:T].copy()).cuda()
        out = torch.zeros(T, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = hd.lib.tgp_posterior_rand(hd.h, lib.ptr(yd), lib.ptr(rd), lib.ptr(et), lib.ptr(ee), lib.ptr(np.ascontiguousarray(case.deps[2])), FL, lib.ptr(out))
        torch.cuda.synchronize()
        assert rc == lib.EUNSUPPORTED, (t_nan, rc)
