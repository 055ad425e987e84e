"""GPU tier: the streaming logpdf kernel's records as LINES (csrc/tgp_lml_record.hpp, tgp_lml.hip): a workgroup leaves its 1 + 2 d values in
one, two or three 64-byte lines of a pinned area of the kernel's own, each line ONE aligned write checked by the host as a whole.  The calls under test
are made UNPROFILED -- a profiled call keeps the synchronising end -- and the kernel's name is asserted in a separate, profiled call.  Oracle:
oracle/seq_kalman.py, logpdf to 1e-10 relative, posterior mean and variance to 1e-8 absolute as everywhere.  The streaming kernels serve every length
(OPT_STREAM_MIN_T = 0, as tests/test_gpu_lml_tiles.py sets it)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import components as oc
from oracle import seq_kalman as sk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# d = 1, 3: one line (three of seven places used; full); d = 4, 6: two lines (two and six places in the second); d = 7, 8: three (one and three places)
KERNELS = {
    1: ("matern12",),
    3: ("matern52",),
    4: ("sum", ("matern52",), ("matern12",)),
    6: ("sum", ("matern52",), ("stretched", 0.4, ("matern52",))),
    7: ("sum", ("matern52",), ("stretched", 0.5, ("matern32",)), ("scaled", 0.3, ("matern32",))),
    8: ("sum", ("matern52",), ("stretched", 2.0, ("matern52",)), ("stretched", 0.5, ("matern32",))),
}
STEPS_PER_LANE = {1: 16, 3: 32, 4: 32, 6: 32, 7: 32, 8: 32}      # the default geometry (tgp_lml::choose_geometry)
RN = 0.3


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


@functools.lru_cache(maxsize=None)
def model_of(d, T):
    return oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)


@functools.lru_cache(maxsize=None)
def head_steps(d):
    """the head of the model's plan (tgp_steady_plan, a pure host function: info_i[3]); it does not depend on the length once the series is long enough"""
    import temporalgps_jl_amd as t
    T = 1_000_000
    model = model_of(d, T)
    A = np.asarray(model["A"]).reshape(-1, d, d)[0]
    Q = np.asarray(model["Q"]).reshape(-1, d, d)[0]
    keep = [np.ascontiguousarray(A.T).reshape(-1), np.asarray(model["a"]).reshape(-1)[:d].copy(), np.ascontiguousarray(Q.T).reshape(-1),
            np.asarray(model["H"]).reshape(-1)[:d].copy(), np.asarray(model["h"]).reshape(-1)[:1].copy(), np.asarray(model["R"]).reshape(-1)[:1].copy(),
            np.asarray(model["x0m"], dtype=np.float64).copy(), np.ascontiguousarray(np.asarray(model["x0P"]).reshape(d, d).T).reshape(-1)]
    ii, dd = np.zeros(8, dtype=np.int32), np.zeros(4)
    t._lib.load().tgp_steady_plan(d, *[k.ctypes.data for k in keep], ctypes.c_int64(T), ii.ctypes.data, dd.ctypes.data, None, None)
    assert ii[0] == 0 and ii[3] > 0, (d, ii)
    return int(ii[3])


def tile_of(d):
    return 64 * STEPS_PER_LANE[d]


def lengths(d):
    """one workgroup with a partial last tile short of / just beyond its second tile, three workgroups, ten workgroups"""
    nhs, tile = head_steps(d), tile_of(d)
    return (nhs + tile - 1, nhs + tile + 1, nhs + 17 * tile + 5, nhs + 80 * tile)


@functools.lru_cache(maxsize=None)
def case(d, T, seed):
    """(y, the oracle's logpdf): computed once, shared between the tests, never written to"""
    model = model_of(d, T)
    rng = np.random.default_rng(seed)
    y = sk.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    y.setflags(write=False)
    return y, sk.logpdf(model, y)


@functools.lru_cache(maxsize=None)
def marginals(d, T, seed):
    m, v = sk.posterior_marginals(model_of(d, T), case(d, T, seed)[0], np.array([RN]))
    m.setflags(write=False)
    v.setflags(write=False)
    return m, v


def device_model(tgp, model):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    dm.handle_options[tgp._lib.OPT_STREAM_MIN_T] = 0
    return dm


def dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()      # (a writable copy: the shared cases are read-only)


def kernels_of(tgp, dm, fn):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    out = fn()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out, names


def bits(x):
    return float(x).hex()


def stream_of(dm):
    """the hipStream_t the model's handle enqueues on (tgp_get_stream)"""
    hd = dm.handle()
    st = ctypes.c_void_p()
    hd.check(hd.lib.tgp_get_stream(hd.h, ctypes.byref(st)))
    assert st.value, "the handle reports no stream"
    return st.value


STREAM_POOL = 8      # kStreamPool of csrc/tgp_api.hip: the handles of a device share that many streams, dealt out in turn


@pytest.mark.parametrize("d,which", [(d, i) for d in sorted(KERNELS) for i in range(4)])
def test_parity_on_the_records_end(tgp, d, which):
    T = lengths(d)[which]
    y, ref = case(d, T, 13 * d + which)
    lp = tgp.logpdf(device_model(tgp, model_of(d, T)), dev(y))
    print(f"d {d} T {T}: relative difference {abs(lp - ref) / abs(ref):.3e}")
    assert abs(lp - ref) <= 1e-10 * abs(ref), (d, T, lp, ref)


@pytest.mark.parametrize("d", (3, 6, 7))
def test_repeated_calls_give_the_first_calls_bits(tgp, d):
    """one handle: five calls with the same series, then another series, then the first again -- lines of an earlier call with the very same values
    must not pass for a later one, and what the later one returns is bit for bit the first"""
    T = lengths(d)[2]
    (y1, ref1), (y2, ref2) = case(d, T, 13 * d + 2), case(d, T, 99)
    dm = device_model(tgp, model_of(d, T))
    y1d, y2d = dev(y1), dev(y2)
    first = tgp.logpdf(dm, y1d)
    assert abs(first - ref1) <= 1e-10 * abs(ref1), (d, first, ref1)
    for k in range(4):
        assert bits(tgp.logpdf(dm, y1d)) == bits(first), (d, k)
    other = tgp.logpdf(dm, y2d)
    assert abs(other - ref2) <= 1e-10 * abs(ref2) and bits(other) != bits(first), (d, other, ref2)
    assert bits(tgp.logpdf(dm, y1d)) == bits(first), d
    # in place: the same device buffer changed and changed back
    buf = y1d.clone()
    assert bits(tgp.logpdf(dm, buf)) == bits(first), d
    buf.copy_(y2d)
    assert bits(tgp.logpdf(dm, buf)) == bits(other), d
    buf.copy_(y1d)
    assert bits(tgp.logpdf(dm, buf)) == bits(first), d


@pytest.mark.parametrize("d", (3,))
def test_interleaved_with_the_posterior_kernels_pairs(tgp, d):
    """logpdf, posterior marginals, logpdf on one handle -- the lines have an area of their own, the posterior kernel's pairs stay in theirs --, then on
    two handles that share a pooled stream: the streams are dealt out in turn, so handles are made until one reports the first one's stream
    (tgp_get_stream), the pool's size and one more at the most"""
    T = lengths(d)[2]
    y, ref = case(d, T, 13 * d + 2)
    m_ref, v_ref = marginals(d, T, 13 * d + 2)
    yd, Rd = dev(y), dev(np.array([RN]))

    def close(mean, var):
        return np.max(np.abs(mean.cpu().numpy() - m_ref)) <= 1e-8 and np.max(np.abs(var.cpu().numpy() - v_ref)) <= 1e-8

    dm = device_model(tgp, model_of(d, T))
    first = tgp.logpdf(dm, yd)
    assert abs(first - ref) <= 1e-10 * abs(ref), (first, ref)
    for k in range(3):
        mean, var = tgp.posterior_marginals(dm, yd, Rd)
        assert close(mean.clone(), var.clone()), k
        assert bits(tgp.logpdf(dm, yd)) == bits(first), k
    others, dm2 = [], None      # (the handles in between stay alive: each holds its place in the pool's turn)
    for _ in range(STREAM_POOL + 1):
        cand = device_model(tgp, model_of(d, T))
        if stream_of(cand) == stream_of(dm):
            dm2 = cand
            break
        others.append(cand)
    assert dm2 is not None, (stream_of(dm), [stream_of(o) for o in others])
    assert dm2.handle() is not dm.handle() and stream_of(dm2) == stream_of(dm)
    for k in range(3):
        assert bits(tgp.logpdf(dm2, yd)) == bits(first), k
        mean, var = tgp.posterior_marginals(dm, yd, Rd)
        assert close(mean.clone(), var.clone()), k
        assert bits(tgp.logpdf(dm, yd)) == bits(first), k
        lp, mean, var = tgp.logpdf_and_posterior_marginals(dm2, yd, Rd)
        assert abs(lp - ref) <= 1e-10 * abs(ref) and close(mean.clone(), var.clone()), k
    assert bits(tgp.logpdf(dm2, yd)) == bits(first)
    assert stream_of(dm2) == stream_of(dm)      # (still one stream behind the calls)


def test_switch_gives_the_synchronising_end_and_the_same_bits(tgp):
    """TGP_LML_RECORDS=0 (read once: a fresh child process) ends the call on the stream and reads the same lines: the same bits as the records end here"""
    cases = [(d, lengths(d)[2]) for d in (3, 6, 8)]
    code = """
import sys
import numpy as np, torch
import temporalgps_jl_amd as tgp
from oracle import components as oc
from oracle import seq_kalman as sk
sys.path.insert(0, "tests")
import test_gpu_lml_records as t
for d, T in %r:
    y, ref = t.case(d, T, 13 * d + 2)
    dm = t.device_model(tgp, t.model_of(d, T))
    yd = t.dev(y)
    for _ in range(2):
        lp = tgp.logpdf(dm, yd)
    print("bits", d, float(lp).hex())
print("checked")
""" % (cases,)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, TGP_LML_RECORDS="0"), cwd=ROOT)
    assert r.returncode == 0 and "checked" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    child = {int(ln.split()[1]): ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith("bits ")}
    for d, T in cases:
        y, ref = case(d, T, 13 * d + 2)
        lp = tgp.logpdf(device_model(tgp, model_of(d, T)), dev(y))
        assert abs(lp - ref) <= 1e-10 * abs(ref), (d, lp, ref)
        assert child[d] == bits(lp), (d, child[d], bits(lp))


@pytest.mark.parametrize("d", sorted(KERNELS))
def test_kernel_name(tgp, d):
    T = lengths(d)[2]
    y, ref = case(d, T, 13 * d + 2)
    dm = device_model(tgp, model_of(d, T))
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, dev(y)))
    assert abs(lp - ref) <= 1e-10 * abs(ref), (d, lp, ref)
    assert names == {f"k_lml_stream<{STEPS_PER_LANE[d]}>"}, (d, names)
