"""Shared helpers for the test tiers (test infrastructure)."""
import ctypes
import os
import subprocess

import numpy as np

from oracle import components as oc
from oracle import lgssm_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = ctypes.POINTER(ctypes.c_double)
_i64 = ctypes.c_int64


def pack(model):
    """dict model (oracle convention; kind 'scalar', or 'small' with DIAGONAL R) -> flat blocks + strides (0 == Fill)."""
    d = len(model["x0m"])
    if model["kind"] == "small":
        p_ = model["H"].shape[-2]
        R = np.atleast_3d(model["R"])
        assert np.allclose(R, R * np.eye(p_)), "pack(): dense R must be whitened first"
        model = dict(model, R=np.diagonal(R, axis1=-2, axis2=-1))
    A = np.ascontiguousarray(np.swapaxes(model["A"], -1, -2)).reshape(-1)
    Q = np.ascontiguousarray(np.swapaxes(model["Q"], -1, -2)).reshape(-1)
    a = np.ascontiguousarray(model["a"]).reshape(-1)
    H = np.ascontiguousarray(model["H"]).reshape(-1)
    h = np.ascontiguousarray(np.atleast_1d(model["h"]), dtype=np.float64).reshape(-1)
    R = np.ascontiguousarray(np.atleast_1d(model["R"]), dtype=np.float64).reshape(-1)
    st = lambda arr, n: n if arr.shape[0] > 1 else 0
    p = model["H"].shape[-2] if model["kind"] == "small" else 1
    return dict(d=d, p=p, small=int(model["kind"] == "small"), T=model["T"], ordering=0 if model["ordering"] == "F" else 1,
                A=A, sA=st(model["A"], d * d), a=a, sa=st(model["a"], d), Q=Q, sQ=st(model["Q"], d * d),
                H=H, sH=st(model["H"], p * d), h=h, sh=st(np.atleast_1d(model["h"]), p),
                R=R, sR=st(np.atleast_1d(model["R"]), p),
                x0m=np.ascontiguousarray(model["x0m"], dtype=np.float64),
                x0P=np.ascontiguousarray(model["x0P"].T, dtype=np.float64).reshape(-1))


# Models whose state dimension sits on the wide-state engine's kernel-family boundaries (csrc/tgp_wide.hip: components per lane and table width
# change at d = 15/16, 31/32, 47/48; the observer is output d >> 4 of lane d & 15, the wave's last lane at d = 63), and d = 54 in the middle of the LDS
# form.  At spacing 0.1 and noise 0.1 every one settles (n0 = 96 ... 120, n1 = 163 ... 184) and its closed loop forgets within 512 steps.
_m52, _m32, _m12 = ("matern52",), ("matern32",), ("matern12",)


def _ap(n):
    return ("approx_periodic", n, 1.0)


BOUNDARY_KERNELS = {
    17: ("sum", ("product", _ap(4), _m32), _m12),
    31: ("sum", ("product", _ap(7), _m32), ("stretched", 0.6, _m52)),
    32: ("sum", ("product", _ap(7), _m32), ("stretched", 0.6, _m52), _m12),
    33: ("sum", ("product", _ap(5), _m52), ("stretched", 0.6, _m52)),
    47: ("sum", ("product", _ap(11), _m32), ("stretched", 0.6, _m52)),
    48: ("sum", ("product", _ap(11), _m32), ("stretched", 0.6, _m52), _m12),
    49: ("sum", ("product", _ap(11), _m32), ("stretched", 0.6, _m52), ("stretched", 1.7, _m32)),
    54: ("product", _ap(9), _m52),
    63: ("sum", ("product", _ap(10), _m52), ("stretched", 0.6, _m52)),
}


# Models of the wide-state adjoint's parity tiers (tests/test_wide_adjoint_host.py, tests/test_gpu_wide_adjoint_edges.py): the state dimensions at which the
# Gram kernel's two extra columns (r_t at d, the constant at d + 1; csrc/tgp_wide.hip k_wide_gram<NT>, NT = ceil((d + 2) / 16)) are the last two of the last tile
# (d = 14, 30, 46, 62) or split over two tiles (15, 31, 47, 63: the first d of NT = 2 ... 5 too), the d around each change of form (15/16/17, 31/32/33, 47/48/49),
# the smallest d (9), and the d of the chunk-geometry cases (12, 28, 42, 54).
WIDE_ADJOINT_KERNELS = {
    9: ("product", _m52, ("stretched", 0.7, _m52)),
    12: ("product", _m32, _ap(3)),
    14: ("product", _ap(7), _m12),
    15: ("sum", ("product", _ap(3), _m32), ("stretched", 0.6, _m52)),
    16: ("sum", ("product", _ap(3), _m32), _m52, _m12),
    28: ("product", ("approx_periodic", 7, 1.3), _m32),
    30: ("product", _ap(5), _m52),
    42: ("product", ("approx_periodic", 7, 1.3), _m52),
    46: ("sum", ("product", _ap(7), _m52), ("product", _ap(2), _m12)),
    62: ("sum", ("product", _ap(10), _m52), ("stretched", 0.6, _m32)),
    **{d: BOUNDARY_KERNELS[d] for d in (17, 31, 32, 33, 47, 48, 49, 54, 63)},
}


def wide_adjoint_model(d, dt, T):
    """the class (d, dt) of the wide-state adjoint's parity tiers: noise 0.1, non-zero a and h (the kernels' a and hh terms are otherwise multiplied by zero)"""
    model = oc.build_lgssm(WIDE_ADJOINT_KERNELS[d], ("regular", 0.0, dt, int(T)), 0.1)
    assert len(model["x0m"]) == d
    model["a"] = 0.01 * np.linspace(-1.0, 1.0, d)[None]
    model["h"] = np.array([0.4])
    return model


def wide_adjoint_length(d):
    """the length of a class's default case (the long-double oracle takes up to 6 s per case at d = 63, T = 2500)"""
    return 1500 if d >= 46 else 2500


def wide_adjoint_draw(model, seed):
    from oracle import seq_kalman as sk
    T, d = model["T"], len(model["x0m"])
    rng = np.random.default_rng(seed)
    return sk.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))


# every class at spacing 0.2; d = 9 at 0.1 too (the class of the second Gram regime: halo 152, chunks of 129 steps are shorter than their warm-up)
WIDE_ADJOINT_CLASSES = [(d, 0.2) for d in sorted(WIDE_ADJOINT_KERNELS)] + [(9, 0.1)]
# the lengths of the host tier beyond wide_adjoint_length(d): those of the GPU tier's cases at which a class's restatement stands farthest from the exact gradient
# (the two long series of d = 9, a short series at d = 12 and 63, T = 3000 at d = 42 and 54)
WIDE_ADJOINT_HOST_EXTRA = [(9, 0.1, 46 + 2048 * 256 + 1), (9, 0.2, 27 + 4096 * 70 - 5), (12, 0.2, 44 + 80), (63, 0.2, 48 + 64), (42, 0.2, 3000), (54, 0.2, 3000)]
GRADIENT_BLOCKS = ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")
# Measured on the CPU (x86-64): the NumPy restatement of the wide-state engine's algorithm + tgp_adjoint_finish_wide
# (tests/test_wide_adjoint_host.py::test_the_algorithm_against_the_exact_sequential_adjoint_entry_by_entry) against the long-double sequential adjoint, the worst entry
# of each block over the largest entry of that block of the reference -- the LARGEST figure over every (length, series) at which the host tier and
# tests/test_gpu_wide_adjoint_edges.py run the class (draws of seed 17 by wide_adjoint_draw; d = 28 also seeds 18 and 19 scaled by 1.5 and 0.6).  The host tier asserts ten times these; the GPU tier's
# per-block bars are ten times these, floored at 1e-10 (wide_adjoint_block_bar).  "global": the worst entry over the largest entry of the whole gradient.
WIDE_ADJOINT_MEASURED = {
    (9, 0.1): dict(A=5.9e-10, a=2.0e-12, Q=8.5e-10, H=3.9e-09, h=2.1e-12, R=1.4e-10, x0m=6.5e-16, x0P=4.3e-10),      # global 8.7e-10
    (9, 0.2): dict(A=9.4e-11, a=3.2e-13, Q=8.1e-11, H=1.2e-10, h=1.7e-13, R=3.5e-11, x0m=4.7e-16, x0P=2.3e-10),      # global 1.2e-10
    (12, 0.2): dict(A=7.2e-12, a=1.5e-14, Q=9.3e-12, H=5.9e-12, h=8.8e-14, R=1.0e-11, x0m=9.3e-16, x0P=7.8e-11),      # global 6.2e-12
    (14, 0.2): dict(A=2.4e-12, a=1.2e-14, Q=8.2e-11, H=2.1e-12, h=7.8e-15, R=9.5e-12, x0m=4.3e-16, x0P=7.6e-09),      # global 8.2e-11
    (15, 0.2): dict(A=4.4e-13, a=7.9e-15, Q=6.6e-14, H=4.3e-13, h=5.7e-14, R=6.4e-13, x0m=1.6e-15, x0P=1.6e-13),      # global 1.3e-13
    (16, 0.2): dict(A=1.5e-12, a=8.5e-14, Q=1.6e-12, H=1.7e-13, h=6.5e-14, R=5.8e-14, x0m=9.6e-17, x0P=7.6e-12),      # global 1.5e-12
    (17, 0.2): dict(A=1.6e-13, a=8.8e-15, Q=3.7e-14, H=7.1e-14, h=3.3e-15, R=3.7e-13, x0m=5.5e-16, x0P=1.6e-12),      # global 3.7e-14
    (28, 0.2): dict(A=4.6e-12, a=3.8e-14, Q=3.1e-12, H=2.8e-12, h=7.0e-14, R=1.3e-12, x0m=1.6e-15, x0P=1.7e-09),      # global 3.1e-12
    (30, 0.2): dict(A=1.8e-12, a=1.6e-13, Q=3.4e-13, H=3.1e-12, h=1.1e-13, R=5.5e-13, x0m=2.8e-16, x0P=2.0e-12),      # global 3.4e-13
    (31, 0.2): dict(A=1.5e-13, a=5.3e-15, Q=1.5e-14, H=2.4e-13, h=1.5e-14, R=7.8e-15, x0m=3.2e-16, x0P=3.6e-13),      # global 1.5e-14
    (32, 0.2): dict(A=1.1e-12, a=4.1e-15, Q=2.9e-14, H=1.2e-14, h=2.4e-15, R=3.6e-14, x0m=8.0e-16, x0P=1.7e-12),      # global 1.5e-13
    (33, 0.2): dict(A=7.8e-12, a=7.7e-14, Q=1.8e-12, H=8.7e-12, h=5.1e-14, R=3.0e-12, x0m=4.0e-16, x0P=9.4e-12),      # global 4.0e-12
    (42, 0.2): dict(A=8.2e-12, a=1.9e-13, Q=3.2e-12, H=3.1e-11, h=2.1e-13, R=9.5e-12, x0m=7.8e-16, x0P=1.6e-11),      # global 4.4e-12
    (46, 0.2): dict(A=4.4e-12, a=2.9e-14, Q=6.5e-12, H=5.9e-13, h=3.5e-14, R=6.6e-12, x0m=6.7e-16, x0P=7.5e-11),      # global 6.5e-12
    (47, 0.2): dict(A=2.2e-13, a=1.9e-15, Q=1.2e-13, H=1.2e-13, h=1.1e-15, R=2.4e-13, x0m=1.8e-15, x0P=1.0e-13),      # global 1.2e-13
    (48, 0.2): dict(A=2.0e-12, a=1.4e-15, Q=1.4e-13, H=5.3e-14, h=4.2e-15, R=5.9e-14, x0m=6.4e-16, x0P=1.8e-12),      # global 6.9e-13
    (49, 0.2): dict(A=1.2e-12, a=1.3e-15, Q=1.0e-13, H=5.3e-14, h=1.7e-14, R=1.1e-13, x0m=1.6e-15, x0P=2.4e-13),      # global 4.5e-13
    (54, 0.2): dict(A=5.1e-12, a=6.5e-14, Q=4.5e-13, H=1.1e-11, h=7.5e-14, R=4.8e-12, x0m=1.4e-15, x0P=4.0e-13),      # global 7.5e-13
    (62, 0.2): dict(A=2.8e-12, a=5.4e-14, Q=3.5e-13, H=2.4e-12, h=6.2e-14, R=2.5e-12, x0m=4.0e-16, x0P=6.6e-13),      # global 9.7e-13
    (63, 0.2): dict(A=1.5e-11, a=4.2e-13, Q=1.8e-12, H=1.2e-11, h=4.2e-13, R=6.2e-12, x0m=1.5e-15, x0P=2.9e-12),      # global 4.3e-12
}


def wide_adjoint_block_bar(d, dt, block):
    """the GPU tier's bar of a block, relative to the block's own largest entry: ten times the CPU restatement's figure (the device's head length and halo differ a
    little from NumPy's), floored at 1e-10"""
    return max(10.0 * WIDE_ADJOINT_MEASURED[(d, dt)][block], 1e-10)


def gradient_deviations(g, g_ref):
    """-> ({block: worst entry / the largest entry of the whole reference gradient}, {block: worst entry / the largest entry of the reference's own block})"""
    scale = max(np.abs(np.asarray(g_ref[k])).max() for k in GRADIENT_BLOCKS)
    err = {k: float(np.abs(np.asarray(g[k]) - np.asarray(g_ref[k])).max()) for k in GRADIENT_BLOCKS}
    return {k: err[k] / scale for k in GRADIENT_BLOCKS}, {k: err[k] / float(np.abs(np.asarray(g_ref[k])).max()) for k in GRADIENT_BLOCKS}


# --------------------------------------------------------------------------- the wide-state engine's GPU tier (tests/test_gpu_wide*.py)
WIDE_INFO = ("why", "n0", "halo", "why_post", "n1", "halo_back", "chunks", "chunk_len")


def wide_form_label(d, dpp=None):
    """the profile label of the form the wide-state engine's plan chooses at state dimension d (csrc/tgp_wide.hip form_name; TGP_WIDE_DPP=0 in the
    environment: the LDS kernels for every d)"""
    dpp = os.environ.get("TGP_WIDE_DPP") != "0" if dpp is None else dpp
    if dpp and d <= 47:
        return "k_wide_lml4<16>" if d <= 15 else "k_wide_lml4" if d <= 31 else "k_wide_lml4<48>"
    return "k_wide_lml<32>" if d <= 31 else "k_wide_lml<64>"


def device_model(tgp, model, wide=1):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    dm.handle_options[tgp._lib.OPT_WIDE] = wide
    return dm


def kernels_of(tgp, dm, fn):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    out = fn()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out, names


def wide_plan(model, T, post=0):
    """info of the wide-state engine's plan for this model and length (the pure host function tgp_wide_plan), as a dictionary; post = 1: the posterior's plan too
    (why_post, n1, halo_back)"""
    from temporalgps_jl_amd import _lib
    lib = _lib.load()
    d = len(model["x0m"])
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))      # noqa: E731
    blocks = [c(model["A"][0].T), c(model["a"][0]), c(model["Q"][0].T), c(model["H"][0]), c(np.atleast_1d(model["h"])[:1]),
              c(np.atleast_1d(model["R"])[:1]), c(model["x0m"]), c(model["x0P"].T)]
    info, K, S, vp = np.zeros(8, dtype=np.int64), np.zeros(d), np.zeros(1), np.zeros(2)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert lib.tgp_wide_plan(d, *[p(b) for b in blocks], T, post, p(info), p(K), p(S), p(vp)) == 0, info
    return dict(zip(WIDE_INFO, (int(v) for v in info)))


def dense_gp_posterior(model, y, Rn):
    """The posterior marginals from the model's OWN covariance function, k(s - t) = h' A^|s - t| P_inf h (x0 stationary, no offsets), by a dense Cholesky: no
    state-space recursion involved (tests/test_gpu_wide.py)"""
    from scipy.linalg import cho_factor, cho_solve, toeplitz
    T = model["T"]
    A, H, P, R = model["A"][0], model["H"][0], model["x0P"], float(model["R"][0])
    c, v = np.empty(T), P @ H
    for k in range(T):
        c[k] = H @ v
        v = A @ v
    K = toeplitz(c)
    cf = cho_factor(K + R * np.eye(T), lower=True)
    return K @ cho_solve(cf, y), np.diag(K) - np.einsum("ij,ji->i", K, cho_solve(cf, K)) + Rn


def is_lti(pk):
    return pk["sA"] == 0 and pk["sa"] == 0 and pk["sQ"] == 0 and pk["sH"] == 0 and pk["sh"] == 0


def gp_case(k, t, s2, seed, mean=None):
    """Model from a kernel spec + a draw y from it (as the reference bench does, single_output_gps.jl:143-145)."""
    rng = np.random.default_rng(seed)
    model = oc.build_lgssm(k, t, s2, mean)
    T, d = model["T"], len(model["x0m"])
    eps = (rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    return model, ref.rand(model, *eps), eps


def random_lgssm(rng, tv, d, T, ordering="F", tame_reverse=False):
    """test/models/model_test_utils.jl:163-263 (scalar-output variants), stable transitions."""
    def psd(n, lo, hi):
        U = np.linalg.qr(rng.standard_normal((n, n)))[0]
        return (U * (rng.random(n) * (hi - lo) + lo)) @ U.T
    x0m, x0P = rng.standard_normal(d), psd(d, 0.9, 1.1)
    n = T if tv else 1
    A = np.stack([-psd(d, 0.1, 0.9) + 0.2 * rng.standard_normal((d, d)) for _ in range(n)])
    A = np.stack([Ai / max(1.0, 1.1 * np.abs(np.linalg.eigvals(Ai)).max()) for Ai in A])
    a = rng.standard_normal((n, d))
    Q = np.stack([psd(d, 0.2, 1.5) for _ in range(n)])
    H, h, R = rng.standard_normal((n, d)), rng.standard_normal(n), rng.random(n) + 0.1
    if ordering == "R" and tame_reverse:
        # (asked for by the one test that runs the POSTERIOR of a Reverse model forward; the other Reverse tests keep the plain draw)
        # step_posterior(::Reverse) (lgssm.jl:223-228) calls invert_dynamics with predicted and filtered state swapped: its G is
        # (A Pf A' + Q) A' Pf^-1, contractive only for weak transitions and weakly informative observations. Models are drawn there, so
        # that the posterior of a Reverse model can be run forward over hundreds of steps without overflow (in the oracle as well).
        A = 0.3 * A
        R = R + 2.0
    return dict(ordering=ordering, kind="scalar", T=T, A=A, a=a, Q=Q, H=H, h=h, R=R, x0m=x0m, x0P=x0P)


# --------------------------------------------------------------------------- hostsim (CPU emulation of the chunk algorithm)
_HOSTSIM = None


def hostsim():
    global _HOSTSIM
    if _HOSTSIM is None:
        src = os.path.join(HERE, "hostsim", "hostsim.cpp")
        so = os.path.join(HERE, "hostsim", "libhostsim.so")
        deps = [src] + [os.path.join(ROOT, "temporalgps.jl_amd", "csrc", f) for f in ("tgp_math.hpp", "tgp_chunk.hpp", "tgp_math_body.inc", "tgp_chunk_body.inc")]
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        _HOSTSIM = ctypes.CDLL(so)
    return _HOSTSIM


def _p(x):
    return None if x is None else x.ctypes.data_as(_dp)


def hostsim_run(model, what, y=None, missing=None, L0=4, BS=3, Rnew=None, eps=None, want_ggl=False, want_elem=False,
                want_rev=False, xs=None):
    pk = pack(model)
    d, T, p_ = pk["d"], pk["T"], pk["p"]
    L0 = ((L0 + p_ - 1) // p_) * p_          # whole time steps per chunk
    osh = (T,) if p_ == 1 else (T, p_)
    out = {}
    lml = ctypes.c_double(0.0)
    m_out = P_out = G = g = L = xfm = xfP = mean = var = None
    if what == 1:
        m_out, P_out = np.zeros((T, d)), np.zeros((T, d, d))
    if what == 2:
        xfm, xfP = np.zeros(d), np.zeros((d, d))
        if want_ggl:
            G, g, L = np.zeros((T, d, d)), np.zeros((T, d)), np.zeros((T, d, d))
        if Rnew is not None:
            mean, var = np.zeros(osh), np.zeros(osh)
    if what in (3, 4):
        mean, var = np.zeros(osh), np.zeros(osh)
    Rn = None if Rnew is None else np.ascontiguousarray(np.atleast_1d(Rnew), dtype=np.float64)
    miss = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    yv = np.zeros(osh) if y is None else np.ascontiguousarray(y, dtype=np.float64)
    et = ee = None
    x0m = pk["x0m"]
    x0P = pk["x0P"]
    if what == 4:
        et = np.ascontiguousarray(eps[0], dtype=np.float64)
        ee = np.ascontiguousarray(eps[1], dtype=np.float64)
        x0m = ref.rand_x0(eps[2], model["x0m"], model["x0P"])
        x0P = np.zeros(d * d)
    d_ = pk["d"]
    elem = np.zeros(d_ * d_ + 2 * d_ + d_ * (d_ + 1)) if want_elem else None
    rev = np.zeros(d_ * d_ + d_ + d_ * (d_ + 1) // 2) if want_rev else None
    xs_m = None if xs is None else np.ascontiguousarray(xs[0], dtype=np.float64)
    xs_P = None if xs is None else np.ascontiguousarray(np.asarray(xs[1]).T, dtype=np.float64)
    rc = hostsim().hostsim_run(
        d, p_, pk["small"], int(is_lti(pk)), what, L0, BS, _i64(T), pk["ordering"], _p(pk["A"]), _i64(pk["sA"]), _p(pk["a"]), _i64(pk["sa"]),
        _p(pk["Q"]), _i64(pk["sQ"]), _p(pk["H"]), _i64(pk["sH"]), _p(pk["h"]), _i64(pk["sh"]), _p(pk["R"]), _i64(pk["sR"]),
        _p(yv), None if miss is None else miss.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        _p(x0m), _p(x0P), ctypes.byref(lml), _p(m_out), _p(P_out), _p(G), _p(g), _p(L), _p(xfm), _p(xfP),
        _p(Rn), _i64(0 if Rn is None or Rn.size == p_ else 1), _p(mean), _p(var), _p(et), _p(ee),
        _p(elem), _p(rev), _p(xs_m), _p(xs_P))
    out.update(rc=rc, lml=lml.value, m=m_out, P=None if P_out is None else np.swapaxes(P_out, -1, -2),
               G=None if G is None else np.swapaxes(G, -1, -2), g=g, L=None if L is None else np.swapaxes(L, -1, -2),
               xfm=xfm, xfP=None if xfP is None else xfP.T, mean=mean, var=var, elem=elem, rev=rev)
    return out


def random_lgssm_small(rng, tv, d, p, T, ordering="F", dense_R=False):
    """SmallOutputLGC emissions (vector observations), test/models/model_test_utils.jl:187-230."""
    m = random_lgssm(rng, tv, d, T, ordering)
    n = T if tv else 1

    def psd(k, lo, hi):
        U_ = np.linalg.qr(rng.standard_normal((k, k)))[0]
        return (U_ * (rng.random(k) * (hi - lo) + lo)) @ U_.T
    m["kind"] = "small"
    m["H"] = rng.standard_normal((n, p, d))
    m["h"] = rng.standard_normal((n, p))
    if dense_R:
        m["R"] = np.stack([psd(p, 0.9, 1.1) for _ in range(n)])
    else:
        m["R"] = np.stack([np.diag(rng.random(p) + 0.1) for _ in range(n)])
    return m


def hostsim_grad(model, dmodel, y, L0=5, BS=3, missing=None):
    """d logpdf / d theta for an LTI scalar model: `dmodel` holds the tangents of A, a, Q, H, h, R, x0m, x0P (same shapes)."""
    pk, dk = pack(model), pack(dict(model, **dmodel))
    assert is_lti(pk) and pk["sR"] == 0
    lml, dl = ctypes.c_double(), ctypes.c_double()
    miss = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    rc = hostsim().hostsim_grad(pk["d"], L0, BS, _i64(pk["T"]), _p(pk["A"]), _p(pk["a"]), _p(pk["Q"]), _p(pk["H"]), _p(pk["h"]), _p(pk["R"]),
                                _p(yv), None if miss is None else miss.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                _p(pk["x0m"]), _p(pk["x0P"]), _p(dk["A"]), _p(dk["a"]), _p(dk["Q"]), _p(dk["H"]), _p(dk["h"]), _p(dk["R"]),
                                _p(dk["x0m"]), _p(dk["x0P"]), ctypes.byref(lml), ctypes.byref(dl))
    assert rc == 0, rc
    return lml.value, dl.value


def model_tangent(build, theta, k, rel=1e-6):
    """central finite difference of the (tiny, shared) model blocks w.r.t. theta[k]: d(A, a, Q, H, h, R, x0m, x0P)/d theta_k."""
    th = np.array(theta, dtype=np.float64)
    hstep = rel * max(1.0, abs(th[k]))
    tp, tm = th.copy(), th.copy()
    tp[k] += hstep
    tm[k] -= hstep
    mp, mm = build(tp), build(tm)
    return {key: (np.asarray(mp[key], dtype=np.float64) - np.asarray(mm[key], dtype=np.float64)) / (2 * hstep)
            for key in ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")}


# --------------------------------------------------------------------------- sweepsim (CPU emulation of the sweep engine, tgp_sweep.hpp)
_SWEEPSIM = None


def sweepsim():
    global _SWEEPSIM
    if _SWEEPSIM is None:
        src = os.path.join(HERE, "hostsim", "sweepsim.cpp")
        so = os.path.join(HERE, "hostsim", "libsweepsim.so")
        deps = [src] + [os.path.join(ROOT, "temporalgps.jl_amd", "csrc", f) for f in ("tgp_math.hpp", "tgp_sweep_body.hpp", "tgp_sweep_plan.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        _SWEEPSIM = ctypes.CDLL(so)
        _SWEEPSIM.sweepsim_run.restype = ctypes.c_int
    return _SWEEPSIM


_SMOOTHSIM = None


def smoothsim():
    global _SMOOTHSIM
    if _SMOOTHSIM is None:
        src = os.path.join(HERE, "hostsim", "smoothsim.cpp")
        so = os.path.join(HERE, "hostsim", "libsmoothsim.so")
        deps = [src, os.path.join(ROOT, "temporalgps.jl_amd", "csrc", "tgp_steady_plan.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        _SMOOTHSIM = ctypes.CDLL(so)
        _SMOOTHSIM.smoothsim_run.restype = ctypes.c_int
    return _SMOOTHSIM


def smoothsim_run(model, y, Rnew, eps=None, hh_t=None):
    """model: oracle dict with SHARED blocks and one noise variance (an LTI model).  The dense-powers one-launch smoother on the host
    (tests/hostsim/smoothsim.cpp).  Returns dict(rc, lml, why, n0, nhs, n1, halo, nwg, mean, var).
    eps = (eps_t (T, d), eps_e (T,), eps_0 (d,)): a DRAW from the posterior instead (returned as `mean`)."""
    T, d = model["T"], len(model["x0m"])
    cm = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)
    A, Q = cm(model["A"][0]), cm(model["Q"][0])
    a = np.ascontiguousarray(model["a"][0], dtype=np.float64)
    H = np.ascontiguousarray(model["H"][0], dtype=np.float64)
    x0m = np.ascontiguousarray(model["x0m"], dtype=np.float64)
    x0P = cm(model["x0P"])
    yv = np.ascontiguousarray(y, dtype=np.float64)
    rn = np.ascontiguousarray(np.atleast_1d(Rnew), dtype=np.float64)
    mean, var, out = np.zeros(T), np.zeros(T), np.zeros(8)
    keep = [np.ascontiguousarray(e, dtype=np.float64) for e in eps] if eps is not None else []
    ee = [_p(k) for k in keep] if keep else [None, None, None]
    hk = None if hh_t is None else np.ascontiguousarray(hh_t, dtype=np.float64)      # an emission offset per step (the model dict's h may then be per step too)
    rc = smoothsim().smoothsim_run(d, _p(A), _p(a), _p(Q), _p(H), ctypes.c_double(float(np.atleast_1d(model["h"])[0])),
                                   ctypes.c_double(float(np.atleast_1d(model["R"])[0])), _p(x0m), _p(x0P), _i64(T), _p(yv), _p(rn),
                                   int(rn.shape[0] > 1), _p(mean), _p(var), _p(out), *ee, _p(hk))
    return dict(rc=rc, lml=out[0], why=int(out[1]), n0=int(out[2]), nhs=int(out[3]), n1=int(out[4]), halo=int(out[5]), nwg=int(out[6]),
                mean=mean, var=var)


def posterior_draw(post, R_new, eps_t, eps_e, eps_0):
    """ref.rand(ref.replace_observation_noise_cov(post, R_new), eps_t, eps_e, eps_0) of an EVALUATED posterior (ordering "R": oracle.seq_kalman.posterior's
    or oracle.lgssm_ref.posterior's G, g, L in A, a, Q; scalar observations), restated with the factorisations batched: the Cholesky factors of
    Symmetric(L_t + 1e-9 I) (lgc.jl:84-87) and of Symmetric(P_final + 1e-12 I) (gaussian.jl:35-43) at once, then the plain loop backwards over the steps
    (lgssm.jl:65-91).  R_new None: the model's own noise.  tests/test_smooth_host.py holds it to the literal loop."""
    assert post["ordering"] == "R" and post["kind"] == "scalar"
    T, d = post["T"], len(post["x0m"])
    G, g, L = (np.broadcast_to(np.asarray(post[k], dtype=np.float64), (T,) + np.asarray(post[k]).shape[1:]) for k in ("A", "a", "Q"))
    sym = lambda M: np.triu(M) + np.swapaxes(np.triu(M, 1), -1, -2)      # noqa: E731  (LinearAlgebra.Symmetric: the upper triangle is the matrix)
    low = np.linalg.cholesky(sym(L) + 1e-9 * np.eye(d))                    # (T, d, d): U_t'
    push = g + np.einsum("tij,tj->ti", low, np.asarray(eps_t, dtype=np.float64))
    x = post["x0m"] + np.linalg.cholesky(sym(np.asarray(post["x0P"])) + 1e-12 * np.eye(d)) @ np.asarray(eps_0, dtype=np.float64)
    H = np.broadcast_to(np.asarray(post["H"], dtype=np.float64), (T, d))
    hx = np.empty(T)
    for t in range(T - 1, -1, -1):
        hx[t] = H[t] @ x
        x = G[t] @ x + push[t]
    R = np.broadcast_to(np.atleast_1d(np.asarray(post["R"] if R_new is None else R_new, dtype=np.float64)), (T,))
    return hx + np.broadcast_to(np.atleast_1d(np.asarray(post["h"], dtype=np.float64)), (T,)) + np.sqrt(R) * np.asarray(eps_e, dtype=np.float64)


def kernel_sde(k):
    """(F, H) of a kernel expression built from Matern terms with scaled / stretched / sum (what the closed-form transitions cover)."""
    from scipy.linalg import block_diag
    if k[0] == "sum":
        parts = [kernel_sde(kk) for kk in k[1:]]
        return block_diag(*[p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    if k[0] == "scaled":
        F, H = kernel_sde(k[2])
        return F, np.sqrt(k[1]) * H
    if k[0] == "stretched":
        F, H = kernel_sde(k[2])
        return F * k[1], H
    F, _, H = oc.to_sde(k)
    return F, H


def sde_coef(F):
    """[lambda per row | N | N^2 / 2] of a block-diagonal drift with one eigenvalue per block (ModelView::sde; tgp_api.hip sde_closed_form)."""
    d = F.shape[0]
    lam, N, N2 = np.zeros(d), np.zeros((d, d)), np.zeros((d, d))
    seen, i = set(), 0
    while i < d:
        S = [i]
        grow = True
        while grow:
            grow = False
            for j in range(d):
                if j not in S and any(F[j, s] != 0 or F[s, j] != 0 for s in S):
                    S.append(j)
                    grow = True
        S = sorted(S)
        n = len(S)
        l = -np.trace(F[np.ix_(S, S)]) / n
        Nb = F[np.ix_(S, S)] + l * np.eye(n)
        assert np.allclose(np.linalg.matrix_power(Nb, n), 0.0, atol=1e-12 * max(1.0, np.abs(F).max()) ** n)
        lam[S] = l
        if n >= 2:
            N[np.ix_(S, S)] = Nb
        if n >= 3:
            N2[np.ix_(S, S)] = 0.5 * Nb @ Nb
        seen.update(S)
        i = max(S) + 1
    return np.concatenate([lam, N.T.reshape(-1), N2.T.reshape(-1)])     # column-major blocks


def sweep_representative(v, noise):
    """The value tgp_model_set hands the sweep engine's plan for its warm-up estimate (csrc/tgp_api.hip sweep_Rrep / sweep_tau): the upper median of the
    first 4096 entries -- noise variances: of those in (0, 1e14), the shared value as it is; gaps: of all of them -- and 1 where there is none."""
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    if noise and v.shape[0] == 1:
        return float(v[0])
    v = v[:4096]
    if noise:
        v = v[(v > 0.0) & (v < 1e14)]
    return float(np.sort(v)[v.shape[0] // 2]) if v.shape[0] else 1.0


def sweepsim_run(model, y, missing=None, Rnew=None, post=True, sde=None, C=0, W=0, Wb=0, num_cu=1, w_hint=0, wb_hint=0):
    """model: oracle dict with SHARED A, a, Q, H (or, with sde = (F, times): transitions by the closed form from the gaps); R / h may be
    per step.  Returns dict(rc, lml, status, dist_f, dist_b, C, W, Wb, nwaves, mean, var)."""
    T, d = model["T"], len(model["x0m"])
    cm = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(-1)
    R = np.atleast_1d(np.asarray(model["R"], dtype=np.float64))
    h = np.atleast_1d(np.asarray(model["h"], dtype=np.float64))
    Rstep = np.ascontiguousarray(R) if R.shape[0] > 1 else None
    hstep = np.ascontiguousarray(h) if h.shape[0] > 1 else None
    Rrep = sweep_representative(R, noise=True)
    coef, tau, tau_typ = None, None, 0.0
    if sde is not None:
        F, times_ = sde
        coef = sde_coef(F)
        tau = np.concatenate([[-1.0], np.diff(np.asarray(times_, dtype=np.float64))])
        tau_typ = sweep_representative(tau[1:], noise=False)
    A, Q = cm(model["A"][0]), cm(model["Q"][0])
    a = np.ascontiguousarray(model["a"][0], dtype=np.float64)
    H = np.ascontiguousarray(model["H"][0], dtype=np.float64)
    x0m = np.ascontiguousarray(model["x0m"], dtype=np.float64)
    x0P = cm(model["x0P"])
    yv = np.ascontiguousarray(y, dtype=np.float64)
    mk = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    rn = np.ascontiguousarray(np.atleast_1d(Rnew if Rnew is not None else 0.0), dtype=np.float64)
    mean, var, out = np.zeros(T), np.zeros(T), np.zeros(8)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    rc = sweepsim().sweepsim_run(
        d, int(sde is not None), _i64(T), _p(A), _p(a), _p(Q), _p(H), ctypes.c_double(float(h[0])), ctypes.c_double(Rrep), _p(x0m), _p(x0P),
        _p(coef), ctypes.c_double(tau_typ), _p(yv), None if mk is None else mk.ctypes.data_as(u8), _p(Rstep), _p(hstep), _p(tau), _p(rn),
        int(rn.shape[0] > 1), int(post), C, W, Wb, w_hint, wb_hint, num_cu, _p(mean), _p(var), _p(out))
    return dict(rc=rc, lml=out[0], status=int(out[1]), dist_f=out[2], dist_b=out[3], C=int(out[4]), W=int(out[5]), Wb=int(out[6]),
                nwaves=int(out[7]), mean=mean, var=var)


def sweepsim_served(model, y, C=0, W=0, Wb=0, w0=0, wb0=0, **kw):
    """sweepsim_run inside the repair loop of the C ABI's call (csrc/tgp_api_engines.inc sweep_call): up to four attempts, a warm-up that a check found
    short doubled for the next one; a forced geometry is reported, not repaired; the plan may decline a doubled warm-up ("forward warm-up longer than four
    chunks").  Returns what tgp_sweep_info shows behind the call -- served, C, W, Wb, waves, attempts (launches), status, state (1 served, -1 the engine is
    off for the bound model, 0 untouched) -- with the last launch's lml / mean / var, `why` ("", "forced", "values", "plan", "attempts") and `tries`: one
    (C, W, Wb, status, dist_f, dist_b) per launch.  w0 / wb0: the warm-ups the bound model remembers from an earlier served call (0: none)."""
    forced = bool(C or W or Wb)
    out = dict(served=0, C=0, W=0, Wb=0, waves=0, attempts=0, status=0, state=0, why="", tries=[], lml=None, mean=None, var=None)
    w, wb = w0, wb0
    for attempt in range(4):
        r = sweepsim_run(model, y, C=C, W=W, Wb=Wb, w_hint=w, wb_hint=wb, **kw)
        if r["rc"] != 0:
            out.update(state=-1, why="plan")
            return out
        out.update(C=r["C"], W=r["W"], Wb=r["Wb"], waves=r["nwaves"], attempts=attempt + 1, status=r["status"], lml=r["lml"], mean=r["mean"], var=r["var"])
        out["tries"].append((r["C"], r["W"], r["Wb"], r["status"], float(r["dist_f"]), float(r["dist_b"])))
        if r["status"] & 12:
            out.update(state=-1 if r["status"] & 4 else 0, why="values")
            return out
        if r["status"] & 3:
            if forced:
                out.update(why="forced")
                return out
            if r["status"] & 1:
                w = 2 * r["W"]
            if r["status"] & 2:
                wb = 2 * r["Wb"]
            continue
        out.update(served=1, state=1)
        return out
    out.update(state=-1, why="attempts")
    return out


# --------------------------------------------------------------------------- the dense engine's passes across the chip (tests/test_gpu_dense_chunked*.py)
DENSE_TOL_F, DENSE_TOL_B = 1e-12, 1e-11          # the hand-over checks' tolerances (csrc/tgp_dense.hip kChunkTolF / kChunkTolB)


def scalar_dev(tgp, model, geometry=None, fused=2):
    L = tgp._lib
    dm = tgp.LGSSM(tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"])),
                   tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    dm.handle_options[L.OPT_WIDE] = 0                # (the dense engine is what is under test)
    dm.handle_options[L.OPT_DENSE_FUSED] = fused     # 2: the sequential passes of option 20 = 0 are the persistent Bryson-Frazier pass too
    if geometry:
        dm.handle_options.update({L.OPT_DENSE_CHUNK_STEPS: geometry[0], L.OPT_DENSE_WARMUP: geometry[1], L.OPT_DENSE_WARMUP_BACK: geometry[2]})
    return dm


def served_once(dm, backward):
    info = dm.handle().dense_chunk_info()
    assert info["served"] == 1 and info["chunks"] > 1 and info["attempts"] == (2 if backward else 1) and info["status"] == 0 and info["state"] == 1, info
    assert info["dist_f"] <= DENSE_TOL_F and (not backward or info["dist_b"] <= DENSE_TOL_B), info
    return info


def sequential(tgp, dm, fn):
    """the same handle with option 20 = 0: the parent's path"""
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_DENSE_CHUNKED, 0)
    out = fn()
    assert hd.dense_chunk_info()["served"] == 0
    hd.set_option(tgp._lib.OPT_DENSE_CHUNKED, 1)
    return out


def against_sequential(chunked, seq):
    (lp, mean, var), (lp0, mean0, var0) = chunked, seq
    assert abs(lp - lp0) <= 1e-10 * abs(lp0), (lp, lp0)
    np.testing.assert_allclose(mean, mean0, rtol=0, atol=1e-8 * max(1.0, np.abs(mean0).max()))
    np.testing.assert_allclose(var, var0, rtol=1e-8, atol=0)


def _spd(rng, n, scale=1.0):
    X = rng.standard_normal((n, n)) / np.sqrt(n)
    return scale * (X @ X.T + 0.5 * np.eye(n))


def random_model(rng, T, d, p, ordering="F", per_step=False, rho=None):      # (tests/test_gpu_dense.py)
    """rho = None: the contraction |A_t| ~ U(0.4, 0.9) is drawn per block; a number: |A_t| = rho x orthogonal, nothing drawn for it"""
    nA = T if per_step else 1
    A = np.stack([np.linalg.qr(rng.standard_normal((d, d)))[0] * (rng.uniform(0.4, 0.9) if rho is None else rho) for _ in range(nA)])
    a = rng.standard_normal((nA, d)) * 0.1
    Q = np.stack([_spd(rng, d, 0.3) for _ in range(nA)])
    H = rng.standard_normal((nA, p, d)) / np.sqrt(d)
    h = rng.standard_normal((nA, p)) * 0.1
    Rd = rng.uniform(0.05, 0.3, size=(T, p))
    R = np.stack([np.diag(r) for r in Rd])
    model = dict(ordering=ordering, kind="small", T=T, A=A, a=a, Q=Q, H=H, h=h, R=R, x0m=rng.standard_normal(d), x0P=_spd(rng, d))
    return model, Rd


def vector_dev(tgp, model, Rd, opts):
    order = tgp.Forward if model["ordering"] == "F" else tgp.Reverse
    dm = tgp.LGSSM(tgp.GaussMarkovModel(order, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"])),
                   tgp.SmallOutputLGC(model["H"], model["h"], Rd), T=model["T"])
    dm.handle_options.update(opts)
    return dm


def with_missing(model, y, mk):
    m2 = dict(model)
    R2, y2 = model["R"].copy(), y.copy()
    for t, i in zip(*np.nonzero(mk)):
        R2[t][i, i] = 1e15
        y2[t, i] = 0.0
    m2["R"] = R2
    return m2, y2, mk.sum() * 0.5 * np.log(2 * np.pi * 1e15)


def forced(tgp, C, W, Wb, fused=2):
    L = tgp._lib
    return {L.OPT_DENSE_FUSED: fused, L.OPT_DENSE_CHUNK_STEPS: C, L.OPT_DENSE_WARMUP: W, L.OPT_DENSE_WARMUP_BACK: Wb}


def dense_chunk_distances(model, y, mk, C, W, Wb):
    """The hand-over distances (dist_f, dist_b) of the dense engine's chunked passes at the geometry (C, W, Wb), in NumPy: scripts/dense_chunk_proto.py's
    forward() / backward() with the p observations of a step applied as p scalar updates (diagonal noise; a missing entry as y := 0, R := 1e15), so that
    vector-observation models have what run() gives the scalar ones.  mk: (T, p) mask (or None).  Only the adjoint pair is walked backwards: the
    marginals are ref.bryson_frazier_marginals' business."""
    T, d = model["T"], len(model["x0m"])
    n = -(-T // C)
    dist = lambda x, r: float(np.max(np.abs(x - r)) / max(np.max(np.abs(r)), 1e-300))      # noqa: E731
    blocks = []
    for t in range(T):
        A, a, Q = ref.transition(model, t)
        H, h, R = ref.emission(model, t)
        H, h = np.atleast_2d(H), np.atleast_1d(h)
        Rd = np.array(np.atleast_1d(R) if np.ndim(R) < 2 else np.diagonal(R), dtype=np.float64)
        yt = np.array(np.atleast_1d(y[t]), dtype=np.float64)
        if mk is not None:
            mt = np.broadcast_to(np.atleast_1d(mk[t]), Rd.shape)
            Rd[mt], yt[mt] = 1e15, 0.0
        blocks.append((A, np.ravel(a), Q, H, h, Rd, yt))

    def step(t, m, P):
        A, a, Q, H, h, Rd, yt = blocks[t]
        m, P, upd = A @ m + a, A @ P @ A.T + Q, []
        for j in range(len(h)):
            v = P @ H[j]
            s = H[j] @ v + Rd[j]
            nu = yt[j] - H[j] @ m - h[j]
            m, P = m + v * nu / s, P - np.outer(v, v) / s
            upd.append((v, s, nu))
        return m, P, upd
    rec, warm, fin = [None] * T, [None] * n, [None] * n
    for c in range(n):
        s0, s1 = c * C, min(T, (c + 1) * C)
        m, P = model["x0m"].copy(), model["x0P"].copy()
        for t in range(max(0, s0 - W), s1):
            if t == s0 and t > max(0, s0 - W):
                warm[c] = np.concatenate([P.ravel(), m])
            m, P, upd = step(t, m, P)
            if t >= s0:
                rec[t] = upd
        fin[c] = np.concatenate([P.ravel(), m])
    dist_f = max([dist(warm[c], fin[c - 1]) for c in range(1, n) if warm[c] is not None] or [0.0])
    warm, out = [None] * n, [None] * n
    for c in range(n):
        s0, s1 = c * C, min(T, (c + 1) * C)
        top = min(T, s1 + Wb)
        lam, Lam = np.zeros(d), np.zeros((d, d))
        for t in range(top - 1, s0 - 1, -1):
            A, H = blocks[t][0], blocks[t][3]
            if t == s1 - 1 and top > s1:
                warm[c] = np.concatenate([Lam.ravel(), lam])
            for j in range(len(rec[t]) - 1, -1, -1):
                v, s, nu = rec[t][j]
                Cm = np.eye(d) - np.outer(v / s, H[j])
                Lam = Cm.T @ Lam @ Cm + np.outer(H[j], H[j]) / s
                lam = Cm.T @ lam - H[j] * nu / s
            if t == 0:
                break
            Lam, lam = A.T @ Lam @ A, A.T @ lam
        out[c] = np.concatenate([Lam.ravel(), lam])
    dist_b = max([dist(warm[c], out[c + 1]) for c in range(n - 1) if warm[c] is not None] or [0.0])
    return dist_f, dist_b
