"""The classes and edge lengths of the dense-powers one-launch kernels' parity tiers (tests/test_gpu_dense_powers_edges.py on the GPU,
tests/test_smooth_host.py and tests/test_dense_powers_plan.py on the CPU): one table, one way of placing a length, whatever runs the case.

Every length comes from what the product's own plans report -- tgp_filter_plan, tgp_smooth_plan, tgp_rand_plan, pure host functions --, none from a constant."""
import numpy as np

from oracle import components as oc

SPAN = 8 * 64 * 8            # waves x lanes x steps per lane of every kernel of the family
TILE = 512                   # steps per wave
T_CAP = 40_000               # no length of the tiers lies above it

M12, M32, M52 = ("matern12",), ("matern32",), ("matern52",)
# name: (kernel, dt, noise, route).  route "offset": the model has a modal form, so logpdf / posterior marginals reach k_smooth_one only with an emission offset
# per step (a mean function); "declined": the modal plan declines the model (summands with one length scale), its LTI form is served by k_smooth_one.
CLASSES = {
    "tiny_d1": (M12, 0.1, 0.1, "offset"),
    "one_tile_d3": (M52, 0.03, 0.5, "offset"),
    "sum_d4": (("sum", M52, M12), 0.05, 0.1, "offset"),
    "stretched_d6": (("sum", M52, ("stretched", 0.4, M52)), 0.05, 0.1, "offset"),
    "two_three_d5": (("sum", M52, M32), 0.02, 0.1, "offset"),
    "from_head_d3": (M52, 0.01, 1.0, "offset"),
    "three_tiles_d3": (M52, 0.01, 1.5, "offset"),            # filter halo 1536; the backward half forgets more slowly still: the posterior plan DECLINES
    "three_tiles_d2": (M32, 0.006, 2.0, "offset"),           # its served neighbour: smoother halo 1536, C = 1024 -- the last span served
    "identical_d6": (("sum", M52, M52), 0.05, 0.1, "declined"),
    "identical_slow_d6": (("sum", M52, M52), 0.015, 0.1, "declined"),      # C < halo (`from_head`) on the route without an offset
    "declined_d7": (("sum", M32, M32, M52), 0.1, 0.1, "declined"),
    "declined_d8": (("sum", M52, M52, M32), 0.1, 0.1, "declined"),
}
# geometry(name) as the docstring table of tests/test_gpu_dense_powers_edges.py records it (why_*: 0 served, 5 declined as slow mixing: the posterior half of
# three_tiles_d3, the open loop of the three classes at spacings <= 0.01).  Searched for with tgp_smooth_plan over 13 kernels x 14 spacings x 15 noise levels
# (1760 served plans): a served class has 32 <= halo <= 1536, so C >= 1024, while its variance tail is through after n1 <= 530 steps (a tail decays with
# G^2j, the halo is set by G^j) -- the largest n1 / C found is 0.52.  No served class has n1 > C; the tail is made to span two workgroups by the lengths
# nhs + k C + n1 // 2 instead.
EXPECTED = {
    "tiny_d1": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=16, halo_f=32, halo=32, n1=15, C_lp=4064, C_post=4032, C_filter=4064, halo_r=416, C_rand=3680),
    "one_tile_d3": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=208, halo_f=512, halo=528, n1=171, C_lp=3584, C_post=3040, C_filter=3584, halo_r=752, C_rand=3344),
    "sum_d4": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=256, halo_f=736, halo=736, n1=149, C_lp=3360, C_post=2624, C_filter=3360, halo_r=832, C_rand=3264),
    "stretched_d6": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=352, halo_f=992, halo=992, n1=178, C_lp=3104, C_post=2112, C_filter=3104, halo_r=1136, C_rand=2960),
    "two_three_d5": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=384, halo_f=1232, halo=1264, n1=157, C_lp=2864, C_post=1568, C_filter=2864, halo_r=1328, C_rand=2768),
    "from_head_d3": dict(why=0, why_lp=0, why_f=0, why_r=5, nhs=560, halo_f=1440, halo=1456, n1=401, C_lp=2656, C_post=1184, C_filter=2656, halo_r=0, C_rand=0),
    "three_tiles_d3": dict(why=5, why_lp=0, why_f=0, why_r=5, nhs=560, halo_f=1536, halo=0, n1=436, C_lp=2560, C_post=0, C_filter=2560, halo_r=0, C_rand=0),
    "three_tiles_d2": dict(why=0, why_lp=0, why_f=0, why_r=5, nhs=608, halo_f=1520, halo=1536, n1=432, C_lp=2576, C_post=1024, C_filter=2576, halo_r=0, C_rand=0),
    "identical_d6": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=96, halo_f=448, halo=448, n1=84, C_lp=3648, C_post=3200, C_filter=3648, halo_r=464, C_rand=3632),
    "identical_slow_d6": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=256, halo_f=1488, halo=1488, n1=192, C_lp=2608, C_post=1120, C_filter=2608, halo_r=1504, C_rand=2592),
    "declined_d7": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=80, halo_f=272, halo=272, n1=37, C_lp=3824, C_post=3552, C_filter=3824, halo_r=272, C_rand=3824),
    "declined_d8": dict(why=0, why_lp=0, why_f=0, why_r=0, nhs=96, halo_f=240, halo=256, n1=33, C_lp=3856, C_post=3584, C_filter=3856, halo_r=272, C_rand=3824),
}
FROM_HEAD = ("from_head_d3", "three_tiles_d2", "identical_slow_d6")      # served with C < smoother halo: the second workgroup too starts at the head
DECLINED_BY_THE_BACKWARD_HALF = CLASSES["three_tiles_d3"]
# What serves an operation the class's plan declines (k_smooth_one<posterior | rand>: three_tiles_d3's backward half; k_rand_one: an open loop that does not
# forget within 1536 steps) -- as observed on an MI355X, asserted since: the sweep engine for a per-step offset at d <= 4, the filter's one-launch kernel and
# the general engine's scans for the evaluated route of a draw, the general engine's affine scan for the prior draw.
_AFFINE_SCAN = {"k_apply_affine<rand>", "k_reduce_affine<rand>", "k_scan_apply<affine,top>", "k_scan_apply<affine>", "k_scan_reduce<affine>"}
DECLINED_SERVED_BY = {
    ("from_head_d3", "rand_prior"): _AFFINE_SCAN,
    ("three_tiles_d3", "rand_prior"): _AFFINE_SCAN,
    ("three_tiles_d2", "rand_prior"): _AFFINE_SCAN,
    # a per-step offset at d = 3: the general engine's scans below 2048 steps, the sweep engine from there on
    ("three_tiles_d3", "marginals"): {"k_apply_filter<per-step,posterior>", "k_finalize", "k_reduce_filter<per-step>", "k_scan_apply<affine,top>",
                                      "k_scan_apply<filter,top>", "k_smooth<per-step>", "k_tile_model", "k_sweep<lti,posterior>"},
    # the LTI form's draw: the evaluated route (tgp_posterior on this handle: k_filter_one; the draw itself runs on the evaluated model's own handle) below
    # 2048 steps, the sweep engine's draw kernel from there on
    ("three_tiles_d3", "rand_post"): {"k_filter_one", "k_sweep_draw<lti>"},
}
BEYOND_LENGTHS = ("from_head_d3", "identical_d6")      # the classes of the tests beyond lengths: one per route, one of them `from_head`
ON_ONE_HANDLE = ("identical_slow_d6",)                 # logpdf, marginals and the draw of ONE bound model all on k_smooth_one; `from_head`
SMOOTH_INFO = ("why", "n0", "nhs", "halo_f", "halo", "n1", "span", "nwg")
RAND_INFO = ("why", "halo", "span", "nwg")
WHY_TOO_SHORT, WHY_SLOW_MIXING = 3, 5      # tgp_plan::Why (csrc/tgp_steady_plan.hpp)


def blocks_of(spec, dt, noise):
    """the shared blocks of a class's model, with non-zero a and h (the kernels' a and hh terms are otherwise multiplied by zero)"""
    model = oc.build_lgssm(spec, ("regular", 0.0, dt, 4), noise)
    d = len(model["x0m"])
    model["a"] = 0.01 * np.linspace(-1.0, 1.0, d)[None] if d > 1 else np.array([[0.01]])
    model["h"] = np.array([0.4])
    return model


def offsets(T):
    """the emission offset per step of the "offset" route: a mean function at the inputs"""
    return 0.4 + np.sin(0.7 * np.arange(T))


def _plan_args(model):
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))      # noqa: E731
    return [c(model["A"][0].T), c(model["a"][0]), c(model["Q"][0].T), c(model["H"][0]), c(np.atleast_1d(model["h"])[:1]),
            c(np.atleast_1d(model["R"])[:1]), c(model["x0m"]), c(model["x0P"].T)]


def filter_plan(model, T):
    """why, n0, nhs, halo of tgp_plan::build_filter (tgp_filter_plan)"""
    from temporalgps_jl_amd import _lib
    blocks, info = _plan_args(model), np.zeros(4, dtype=np.int32)
    assert _lib.load().tgp_filter_plan(len(model["x0m"]), *[b.ctypes.data for b in blocks], int(T), info.ctypes.data) == 0
    return dict(zip(("why", "n0", "nhs", "halo"), (int(v) for v in info)))


def smooth_plan(model, T, post=True):
    """SMOOTH_INFO of the plan k_smooth_one is launched on (tgp_smooth_plan): post = False the logpdf's, True the posterior marginals' and the posterior draw's"""
    from temporalgps_jl_amd import _lib
    blocks, info = _plan_args(model), np.zeros(8, dtype=np.int32)
    assert _lib.load().tgp_smooth_plan(len(model["x0m"]), *[b.ctypes.data for b in blocks], int(T), int(post), info.ctypes.data) == 0
    return dict(zip(SMOOTH_INFO, (int(v) for v in info)))


def rand_plan(model, T):
    """RAND_INFO of the plan k_rand_one is launched on (tgp_rand_plan)"""
    from temporalgps_jl_amd import _lib
    blocks, info = _plan_args(model), np.zeros(4, dtype=np.int32)
    assert _lib.load().tgp_rand_plan(len(model["x0m"]), *[b.ctypes.data for b in blocks], int(T), info.ctypes.data) == 0
    return dict(zip(RAND_INFO, (int(v) for v in info)))


def geometry(name):
    """what the docstring table of tests/test_gpu_dense_powers_edges.py holds for a class: (nhs, filter halo, smoother halo, n1, C of the logpdf, C of the posterior
    half, C of the filter, prior-draw halo, C of the prior draw), from the three plan functions at a long series"""
    spec, dt, noise, _ = CLASSES[name]
    m = blocks_of(spec, dt, noise)
    sp, sl, fp, rp = smooth_plan(m, T_CAP), smooth_plan(m, T_CAP, post=False), filter_plan(m, T_CAP), rand_plan(m, T_CAP)
    return dict(why=sp["why"], why_lp=sl["why"], why_f=fp["why"], why_r=rp["why"], nhs=sp["nhs"], halo_f=sp["halo_f"], halo=sp["halo"], n1=sp["n1"], C_lp=sl["span"],
                C_post=sp["span"], C_filter=SPAN - fp["halo"] if fp["why"] == 0 else 0, halo_r=rp["halo"], C_rand=rp["span"])


def shortest_served(plan, lo, hi):
    """the smallest T in [lo, hi] the plan function accepts (why == 0); the plans' only condition on T is "long enough\""""
    for T in range(max(1, lo), hi + 1):
        if plan(T)["why"] == 0:
            return T
    raise AssertionError("no served length")


def edge_lengths(nhs, C, halo, n1=0, halo_left=None):
    """The lengths of one (class, operation), behind its head of nhs steps (0: the prior draw), with spans of C steps, `halo` steps behind a span that the
    series' end may cut (the forward-only kernels have none: their run-in is given instead, as good a place as any) and a variance tail of n1 steps.
    halo_left: the run-in in front of a span (where the second workgroup's tiles begin).  Lengths the operation's plan finds too short are the callers'
    decline cases."""
    hl = halo if halo_left is None else halo_left
    Ts = [nhs + k for k in (7, 8, 9, 511, 512, 513)]                                         # partial lane, 16-byte load against the one-by-one path, tile edge
    Ts += [nhs + C - 1, nhs + C, nhs + C + 1, nhs + 2 * C - 1, nhs + 2 * C + 1]              # one / two / three workgroups
    Ts += [nhs + 2 * C + halo - 1, nhs + 2 * C + halo + 1]                                   # the halo behind the second span, cut by T
    Ts += [nhs + 7 * C + 1, nhs + 8 * C, nhs + 8 * C + 1, nhs + 9 * C + 1]                   # per: 1 -> 2, with empty blocks
    if n1 > 0:
        # T - n1 (where the variance tail begins) at a span edge +- 1 ...
        Ts += [nhs + k * C + n1 + e for k in (1, 2) for e in (-1, 0, 1)]
        Ts += [nhs + k * C + n1 // 2 for k in (1, 2)]                                        # the tail over two workgroups (no served class has n1 > C)
        # ... and at a tile edge +- 1: of the first workgroup (tiles from nhs), and of the second (tiles from nhs + C - hl, or from nhs: C < hl)
        s1 = nhs if C < hl else nhs + C - hl
        k1 = -(-(nhs + C - s1) // TILE)          # the first tile edge of the second workgroup inside its own range
        Ts += [nhs + 2 * TILE + n1 + e for e in (-1, 1)] + [s1 + k1 * TILE + n1 + e for e in (-1, 1)]
    t3 = nhs + 3 * C + 40
    Ts.append(t3 + (3 - t3) % 8)                                                             # one T = 3 (mod 8)
    assert max(Ts) <= T_CAP, max(Ts)
    return sorted(set(T for T in Ts if T >= 2))
